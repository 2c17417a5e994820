"""monodepth2 network (the `--configure kitti` model), restated.

The reference imports it from an un-vendored submodule (nianticlabs/monodepth2 `networks/`; call sites
reference monodepth/monodepth2_model.py:11-12,32-50,75-77) and its weights come from a URL (unreachable).  Restated from the
published `ResnetEncoder(18)` + `DepthDecoder(num_ch_enc, scales=range(4))`:

  encoder   torchvision ResNet-18 as a whole (`fc` included, unused): f0 = relu(bn1(conv1 7x7/2)) (64 ch, 1/2), then layer1(maxpool 3x3/2(f0))
            .. layer4 (64 / 128 / 256 / 512 ch at 1/4 .. 1/32); BasicBlocks (two 3x3 convolutions with BatchNorm, 1x1/2 down-sample + BN).
  decoder   for i = 4 .. 0: x = ConvBlock(i, 0)(x); x = cat(nearest_x2(x), f[i-1] if i > 0); x = ConvBlock(i, 1)(x); disp_i = sigmoid(
            dispconv_i(x)) -- ConvBlock = reflection pad 1 + Conv2d 3x3 (bias) + ELU, dispconv = reflection pad 1 + Conv2d 3x3 -> 1 ch.
            num_ch_dec = (16, 32, 64, 128, 256).  Only disp_0 reaches the loss (monodepth2_model.py:79): dispconv 1-3 are kept (a real
            checkpoint loads strictly) but not evaluated; they, and `encoder.fc`, get zero gradients.

State-dict keys follow upstream: `encoder.conv1.weight`, `encoder.layer2.0.downsample.0.weight`, `encoder.fc.weight` (ResnetEncoder) and
`decoder.0.conv.conv.weight` .. `decoder.9...` (the upconvs for i = 4 .. 0, (0, 1) each), `decoder.10.conv.weight` .. `decoder.13...`
(dispconv 0 .. 3) -- upstream's `nn.ModuleList(list(self.convs.values()))`.  "Parity unpinned" for real weights (no source, no weights
here); the tests pin the layout and compare with an fp64 twin built from the ATen modules.

Everything on the hand-written kernels: every convolution is an ops.conv_layer.HipConv2d (all filters packed by one PackPool launch per
forward; the three 3x3/2 stage entries and their 1x1/2 shortcuts on the native stride-2 kernels of csrc/conv_strided.hip, the
3-channel 7x7/2 stem on the forward / weight-gradient kernels of csrc/conv_stem.hip), BatchNorm (+ residual) (+ ReLU) and the
max-pool on ops.blocks, and the decoder's reflection padding, nearest x2, skip concat, ELU and sigmoid on ops.resample: each decoder
convolution is pad_cat (one gather writing the padded input) -> the "same" 3x3 convolution of the padded tensor -> crop_act (its interior
plus the activation), which is exactly reflection pad + valid Conv2d + activation.  The input's bicubic resize to the feed size (with the
encoder's (x - 0.45) / 0.225 fused in) and the disparity's bicubic resize back run on the same file's kernels.  Eval-mode BatchNorm
(running statistics) falls back to the framework inside ops.blocks.bn_act, as for MiDaS.  Builds on the CPU (layout tests); runs on the
HIP device only.
"""
from __future__ import annotations

import torch.nn as nn

from ..ops import blocks as B
from ..ops.conv_layer import HipConv2d, PackPool
from ..ops.resample import HipReflectConv3x3, bicubic_resize, crop_act, pad_cat

NUM_CH_ENC = (64, 64, 128, 256, 512)
NUM_CH_DEC = (16, 32, 64, 128, 256)
FEED = (320, 1024)           # (height, width) of the mono+stereo 1024x320 weights
NORM = (0.45, 0.225)         # ResnetEncoder.forward: (x - 0.45) / 0.225


class BasicBlock(nn.Module):
    def __init__(self, inplanes, planes, stride=1):
        super().__init__()
        self.conv1 = HipConv2d(inplanes, planes, 3, stride, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = HipConv2d(planes, planes, 3, 1, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.downsample = None
        if stride != 1 or inplanes != planes:
            self.downsample = nn.Sequential(HipConv2d(inplanes, planes, 1, stride, 0, bias=False), nn.BatchNorm2d(planes))

    def forward(self, x):
        idt = x if self.downsample is None else B.bn_act(self.downsample[0](x), self.downsample[1], False)
        out = B.bn_act(self.conv1(x), self.bn1, True)
        return B.bn_act(self.conv2(out), self.bn2, True, res=idt)


class ResNet18(nn.Module):
    """torchvision.models.resnet18's parameters and buffers under its names (conv1, bn1, layer1..4, fc)."""

    def __init__(self):
        super().__init__()
        self.conv1 = HipConv2d(3, 64, 7, 2, 3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        cin = 64
        for i, (planes, stride) in enumerate(((64, 1), (128, 2), (256, 2), (512, 2)), start=1):
            setattr(self, f"layer{i}", nn.Sequential(BasicBlock(cin, planes, stride), BasicBlock(planes, planes)))
            cin = planes
        self.fc = nn.Linear(512, 1000)
        for m in self.modules():      # torchvision's initialisation
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)


class ResnetEncoder(nn.Module):
    """forward(x) -> [f0 .. f4]; x is the NORMALISED feed-size image (the normalisation is fused into the resize, Monodepth2Net)."""
    num_ch_enc = NUM_CH_ENC

    def __init__(self):
        super().__init__()
        self.encoder = ResNet18()

    def forward(self, x):
        e = self.encoder
        f0 = B.bn_act(e.conv1(x), e.bn1, True)
        f1 = e.layer1(B.maxpool3s2(f0))
        f2 = e.layer2(f1)
        f3 = e.layer3(f2)
        return [f0, f1, f2, f3, e.layer4(f3)]


class ConvBlock(nn.Module):
    """Reflection pad 1 + Conv2d 3x3 + ELU; forward takes the PADDED input (ops.resample.pad_cat) and returns the activated interior."""

    def __init__(self, cin, cout):
        super().__init__()
        self.conv = HipReflectConv3x3(cin, cout)

    def forward(self, xp):
        return crop_act(self.conv(xp), "elu")


class DepthDecoder(nn.Module):
    """forward(features) -> disp_0 (N, 1, feed_h, feed_w); `decoder.0` .. `decoder.13` as upstream."""

    def __init__(self, num_ch_enc=NUM_CH_ENC):
        super().__init__()
        convs = []
        for i in range(4, -1, -1):
            convs.append(ConvBlock(num_ch_enc[-1] if i == 4 else NUM_CH_DEC[i + 1], NUM_CH_DEC[i]))
            convs.append(ConvBlock(NUM_CH_DEC[i] + (num_ch_enc[i - 1] if i > 0 else 0), NUM_CH_DEC[i]))
        convs += [HipReflectConv3x3(NUM_CH_DEC[s], 1) for s in range(4)]
        self.decoder = nn.ModuleList(convs)

    def forward(self, features):
        x = features[-1]
        for j, i in enumerate(range(4, -1, -1)):
            x = self.decoder[2 * j](pad_cat(x))
            x = self.decoder[2 * j + 1](pad_cat(x, 2, features[i - 1] if i > 0 else None))
        return crop_act(self.decoder[10](pad_cat(x)), "sigmoid")


def check_feed(feed):
    h, w = int(feed[0]), int(feed[1])
    if h % 32 or w % 32 or h < 64 or w < 64:
        raise ValueError(f"monodepth2: feed size {h} x {w} must be a multiple of 32 in both axes (the encoder halves it five times; "
                         "the decoder's reflection padding needs the 1/32 features to be at least 2 x 2, so 64 at least)")
    return h, w


class Monodepth2Net(nn.Module):
    """images (N, 3, H, W) in [0, 1] -> disparity (N, 1, H, W): bicubic resize to the feed size (+ normalisation), encoder, decoder's
    disp_0, bicubic resize back (reference: monodepth2_model.py:61-91 without the reciprocal)."""

    def __init__(self, feed=FEED):
        super().__init__()
        self.feed = check_feed(feed)
        self.encoder = ResnetEncoder()
        self.depth_decoder = DepthDecoder(self.encoder.num_ch_enc)
        self._pack_pool = PackPool()          # every filter packed by ONE launch per forward (ops/conv_layer.py::PackPool)
        for m in self.modules():
            if isinstance(m, HipConv2d):
                self._pack_pool.register(m)

    def forward(self, images):
        self._pack_pool.run()
        H, W = images.shape[-2:]
        x = bicubic_resize(images, self.feed, norm=NORM)
        disp = self.depth_decoder(self.encoder(x))
        return bicubic_resize(disp, (H, W))
