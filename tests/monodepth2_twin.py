"""The ATen twin of the monodepth2 network (nn.Conv2d, BatchNorm2d, ReflectionPad2d, ELU, F.interpolate), shared by
tests/test_monodepth2_gpu.py (the whole network) and tests/test_monodepth2_layers_gpu.py (single blocks).  Its module paths and state-dict
keys follow monodepth2_net.Monodepth2Net, so a state dict or a sub-module path carries over; `.double()` makes it the fp64 reference."""


def twin(feed):
    """Upstream's ResnetEncoder(18) + DepthDecoder from the ATen modules (nn.Conv2d, BatchNorm2d, ReflectionPad2d, ELU, F.interpolate) and
    monodepth2_model.estimate_depth's steps up to the disparity at frame size."""
    import torch
    import torch.nn as nn
    import torch.nn.functional as F

    class Block(nn.Module):
        def __init__(self, cin, p, s):
            super().__init__()
            self.conv1, self.bn1 = nn.Conv2d(cin, p, 3, s, 1, bias=False), nn.BatchNorm2d(p)
            self.conv2, self.bn2 = nn.Conv2d(p, p, 3, 1, 1, bias=False), nn.BatchNorm2d(p)
            self.downsample = nn.Sequential(nn.Conv2d(cin, p, 1, s, bias=False), nn.BatchNorm2d(p)) if (s != 1 or cin != p) else None

        def forward(self, x):
            idt = x if self.downsample is None else self.downsample(x)
            return F.relu(self.bn2(self.conv2(F.relu(self.bn1(self.conv1(x))))) + idt)

    class ResNet(nn.Module):
        def __init__(self):
            super().__init__()
            self.conv1, self.bn1 = nn.Conv2d(3, 64, 7, 2, 3, bias=False), nn.BatchNorm2d(64)
            cin = 64
            for i, (p, s) in enumerate(((64, 1), (128, 2), (256, 2), (512, 2)), start=1):
                setattr(self, f"layer{i}", nn.Sequential(Block(cin, p, s), Block(p, p, 1)))
                cin = p
            self.fc = nn.Linear(512, 1000)

    class Encoder(nn.Module):
        def __init__(self):
            super().__init__()
            self.encoder = ResNet()

        def forward(self, x):
            e = self.encoder
            f = [F.relu(e.bn1(e.conv1((x - 0.45) / 0.225)))]
            f.append(e.layer1(F.max_pool2d(f[-1], 3, 2, 1)))
            for layer in (e.layer2, e.layer3, e.layer4):
                f.append(layer(f[-1]))
            return f

    class Conv3x3(nn.Module):
        def __init__(self, cin, cout):
            super().__init__()
            self.pad, self.conv = nn.ReflectionPad2d(1), nn.Conv2d(cin, cout, 3)

        def forward(self, x):
            return self.conv(self.pad(x))

    class ConvBlock(nn.Module):
        def __init__(self, cin, cout):
            super().__init__()
            self.conv, self.nonlin = Conv3x3(cin, cout), nn.ELU(inplace=True)

        def forward(self, x):
            return self.nonlin(self.conv(x))

    class Decoder(nn.Module):
        def __init__(self):
            super().__init__()
            enc, dec = (64, 64, 128, 256, 512), (16, 32, 64, 128, 256)
            convs = []
            for i in range(4, -1, -1):
                convs += [ConvBlock(enc[-1] if i == 4 else dec[i + 1], dec[i]), ConvBlock(dec[i] + (enc[i - 1] if i > 0 else 0), dec[i])]
            convs += [Conv3x3(dec[s], 1) for s in range(4)]
            self.decoder = nn.ModuleList(convs)

        def forward(self, f):
            x = f[-1]
            for j, i in enumerate(range(4, -1, -1)):
                x = [F.interpolate(self.decoder[2 * j](x), scale_factor=2, mode="nearest")]
                if i > 0:
                    x.append(f[i - 1])
                x = self.decoder[2 * j + 1](torch.cat(x, 1))
            return torch.sigmoid(self.decoder[10](x))

    class Twin(nn.Module):
        def __init__(self):
            super().__init__()
            self.encoder, self.depth_decoder = Encoder(), Decoder()

        def forward(self, images):
            H, W = images.shape[-2:]
            x = F.interpolate(images, size=feed, mode="bicubic", align_corners=False)
            disp = self.depth_decoder(self.encoder(x))
            return F.interpolate(disp, size=(H, W), mode="bicubic", align_corners=False)

    return Twin()
