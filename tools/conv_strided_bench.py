"""Stride-2 convolution: the native kernels (csrc/conv_strided.hip) against the stride-1-plus-sub-sampling path of the same layer
(CD_AMD_CONV_STRIDED=0), pass by pass, in one process on the same tensors.

    python tools/conv_strided_bench.py [--iters 20] [--warmup 3]

Shapes: the three stage entries of ResNet-18 at the KITTI feed, the three strided grouped 3x3 of ResNeXt-101 32x8d at 384x384 and
the 1x1 / 2 down-sample shortcuts, N = 8; then the two 7x7 / 2 RGB stems (csrc/conv_stem.hip: monodepth2 at N = 8, 320 x 1024 and midas2
at N = 16, 384 x 384; forward and weight gradient only, native against CD_AMD_CONV_STEM=0).  Per pass (forward, input gradient, weight gradient): median of `iters` launches timed
with HIP events, the speed-up, and the fraction of the split-bf16 roof (2500 / 6 TFLOP/s, bench.py's roofline_conv) on the
STRIDED multiply-add count.  The passes are isolated through autograd: forward = the layer call, input gradient = grad w.r.t. x
only, weight gradient = grad w.r.t. the weight only."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [  # (name, Cin, Cout, k, groups, H, W)
    ("resnet18 layer2.0 3x3", 64, 128, 3, 1, 80, 256), ("resnet18 layer3.0 3x3", 128, 256, 3, 1, 40, 128),
    ("resnet18 layer4.0 3x3", 256, 512, 3, 1, 20, 64),
    ("resnext101 layer2.0 3x3 g32", 512, 512, 3, 32, 96, 96), ("resnext101 layer3.0 3x3 g32", 1024, 1024, 3, 32, 48, 48),
    ("resnext101 layer4.0 3x3 g32", 2048, 2048, 3, 32, 24, 24),
    ("resnet18 layer2.0 1x1", 64, 128, 1, 1, 80, 256), ("resnet18 layer3.0 1x1", 128, 256, 1, 1, 40, 128),
    ("resnet18 layer4.0 1x1", 256, 512, 1, 1, 20, 64),
    ("resnext101 layer2.0 1x1", 256, 512, 1, 1, 96, 96), ("resnext101 layer3.0 1x1", 512, 1024, 1, 1, 48, 48),
    ("resnext101 layer4.0 1x1", 1024, 2048, 1, 1, 24, 24),
]
STEMS = [  # (name, Cin, Cout, k, groups, H, W, N): no input gradient (an image needs none)
    ("monodepth2 stem 7x7", 3, 64, 7, 1, 320, 1024, 8), ("midas2 stem 7x7", 3, 64, 7, 1, 384, 384, 16),
]
ROOF = 2500e12 / 6
N = 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import torch
    from consistent_depth_amd.ops.conv_layer import HipConv2d

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        ts = []
        for _ in range(args.iters):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b) * 1e3)
        return statistics.median(ts)

    print(f"{'shape':32s} {'pass':6s} {'native us':>10s} {'emulated us':>12s} {'speed-up':>9s} {'roof %':>7s}")
    rows = [(s, N, "CD_AMD_CONV_STRIDED", ("fwd", "dgrad", "wgrad")) for s in SHAPES] + [(s[:7], s[7], "CD_AMD_CONV_STEM", ("fwd", "wgrad")) for s in STEMS]
    for (name, Cin, Cout, k, G, H, W), n_img, switch, passes in rows:
        torch.manual_seed(0)
        layer = HipConv2d(Cin, Cout, k, 2, (k - 1) // 2, groups=G, bias=False).cuda()
        x = torch.randn(n_img, Cin, H, W, device="cuda")
        xg = x.clone().requires_grad_(True)
        dy = torch.randn(n_img, Cout, (H + 1) // 2, (W + 1) // 2, device="cuda")
        macs = n_img * dy.shape[2] * dy.shape[3] * Cout * (Cin // G) * k * k
        res = {}
        for mode in ("1", "0"):
            os.environ[switch] = mode
            if "dgrad" in passes:
                layer.weight.requires_grad_(False)
                y_dx = layer(xg)
            layer.weight.requires_grad_(True)
            y_dw = layer(x)
            with torch.no_grad():
                res[mode, "fwd"] = timed(lambda: layer(x))
            if "dgrad" in passes:
                res[mode, "dgrad"] = timed(lambda: torch.autograd.grad(y_dx, xg, dy, retain_graph=True))
            res[mode, "wgrad"] = timed(lambda: torch.autograd.grad(y_dw, layer.weight, dy, retain_graph=True))
        os.environ[switch] = "1"
        for p in passes:
            nat, emu = res["1", p], res["0", p]
            print(f"{name:32s} {p:6s} {nat:10.1f} {emu:12.1f} {emu / nat:8.2f}x {100 * 2 * macs / ROOF / (nat * 1e-6):7.1f}")


if __name__ == "__main__":
    main()
