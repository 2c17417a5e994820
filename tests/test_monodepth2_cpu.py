"""CPU: the monodepth2 network's layout against upstream's (ResnetEncoder(18) + DepthDecoder, written out here by hand) and the host-side
bicubic tables of ops.resample against ATen's bicubic (forward and autograd) in fp64."""
import math

import numpy as np
import pytest


def _resnet18_layout():
    """torchvision resnet18 under ResnetEncoder's `encoder.` prefix: name -> shape, in registration order."""
    d = {}

    def conv(name, co, ci, k):
        d[f"{name}.weight"] = (co, ci, k, k)

    def bn(name, c):
        d[f"{name}.weight"] = (c,)
        d[f"{name}.bias"] = (c,)

    conv("encoder.conv1", 64, 3, 7)
    bn("encoder.bn1", 64)
    cin = 64
    for i, (planes, stride) in enumerate(((64, 1), (128, 2), (256, 2), (512, 2)), start=1):
        for b in range(2):
            pre = f"encoder.layer{i}.{b}"
            ci = cin if b == 0 else planes
            conv(f"{pre}.conv1", planes, ci, 3)
            bn(f"{pre}.bn1", planes)
            conv(f"{pre}.conv2", planes, planes, 3)
            bn(f"{pre}.bn2", planes)
            if b == 0 and (stride != 1 or cin != planes):
                conv(f"{pre}.downsample.0", planes, cin, 1)
                bn(f"{pre}.downsample.1", planes)
        cin = planes
    d["encoder.fc.weight"] = (1000, 512)
    d["encoder.fc.bias"] = (1000,)
    return d


# (input channels, output channels) of decoder.0 .. decoder.13: upconv(4,0), upconv(4,1), ..., upconv(0,1), dispconv 0..3
_DECODER = [(512, 256), (512, 256), (256, 128), (256, 128), (128, 64), (128, 64), (64, 32), (96, 32), (32, 16), (16, 16),
            (16, 1), (32, 1), (64, 1), (128, 1)]


def _decoder_layout():
    d = {}
    for j, (ci, co) in enumerate(_DECODER):
        pre = f"decoder.{j}.conv.conv" if j < 10 else f"decoder.{j}.conv"
        d[f"{pre}.weight"] = (co, ci, 3, 3)
        d[f"{pre}.bias"] = (co,)
    return d


def test_network_layout_is_upstreams():
    from consistent_depth_amd.monodepth.monodepth2_net import Monodepth2Net
    net = Monodepth2Net()       # builds on the CPU
    enc, dec = _resnet18_layout(), _decoder_layout()
    got_enc = {k: tuple(p.shape) for k, p in net.encoder.named_parameters()}
    got_dec = {k: tuple(p.shape) for k, p in net.depth_decoder.named_parameters()}
    assert list(got_enc.items()) == list(enc.items())
    assert list(got_dec.items()) == list(dec.items())
    # BatchNorm buffers as torchvision has them
    bns = {k.rsplit(".", 1)[0] for k in enc if k.endswith(".bias") and "conv" not in k and "fc" not in k and "downsample.0" not in k}
    buffers = {f"{b}.{s}" for b in bns for s in ("running_mean", "running_var", "num_batches_tracked")}
    assert set(net.encoder.state_dict()) == set(enc) | buffers
    assert set(net.depth_decoder.state_dict()) == set(dec)
    n_enc = sum(math.prod(s) for s in enc.values())
    n_dec = sum(math.prod(s) for s in dec.values())
    assert sum(p.numel() for p in net.encoder.parameters()) == n_enc
    assert sum(p.numel() for p in net.depth_decoder.parameters()) == n_dec
    # parameters() order: the encoder's, then the decoder's (reference monodepth2_model.py:58-59)
    assert [id(p) for p in net.parameters()] == [id(p) for p in list(net.encoder.parameters()) + list(net.depth_decoder.parameters())]
    print("monodepth2 parameters:", n_enc, "+", n_dec, "=", n_enc + n_dec)


def test_feed_sizes_that_are_not_multiples_of_32_are_refused():
    from consistent_depth_amd.monodepth.monodepth2_net import Monodepth2Net
    for feed in ((320, 1000), (100, 320), (32, 1024)):
        with pytest.raises(ValueError, match="multiple of 32"):
            Monodepth2Net(feed)


PAIRS = [(224, 1024), (384, 320), (1024, 224), (320, 384), (48, 1024), (64, 320), (7, 7), (1, 5), (5, 1)]


@pytest.mark.parametrize("axis", [2, 3])
@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{p[0]}to{p[1]}")
def test_bicubic_tables_reproduce_aten_fp64(pair, axis):
    import torch
    import torch.nn.functional as F
    from consistent_depth_amd.ops.resample import bicubic_inverse, bicubic_taps
    n_in, n_out = pair
    other = 6
    shape = [2, 3, other, other]
    shape[axis] = n_in
    size = [other, other]
    size[axis - 2] = n_out
    g = torch.Generator().manual_seed(n_in * 7 + n_out + axis)
    x = torch.rand(shape, dtype=torch.float64, generator=g).requires_grad_(True)
    y = F.interpolate(x, size=size, mode="bicubic", align_corners=False)
    dy = torch.randn(y.shape, dtype=torch.float64, generator=g)
    y.backward(dy)

    idx, w = bicubic_taps(n_in, n_out, np.float64)
    assert idx.shape == (n_out, 4) and idx.min() >= 0 and idx.max() <= n_in - 1
    xa = np.moveaxis(x.detach().numpy(), axis, -1)                       # (..., n_in)
    mine = (xa[..., idx] * w).sum(-1)                                    # (..., n_out)
    assert np.abs(mine - np.moveaxis(y.detach().numpy(), axis, -1)).max() <= 1e-12

    off, oo, ww = bicubic_inverse(n_in, n_out, np.float64)
    assert off[0] == 0 and off[-1] == len(oo) == len(ww) and oo.max() <= n_out - 1
    dya = np.moveaxis(dy.numpy(), axis, -1)
    dx = np.stack([(dya[..., oo[off[i]:off[i + 1]]] * ww[off[i]:off[i + 1]]).sum(-1) for i in range(n_in)], -1)
    assert np.abs(dx - np.moveaxis(x.grad.numpy(), axis, -1)).max() <= 1e-12
