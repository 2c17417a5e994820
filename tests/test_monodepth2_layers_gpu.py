"""monodepth2's step piece by piece against fp64, at the shapes the real step runs (BS4, two frames per pair: N = 8, feed 320 x 1024).

tests/test_monodepth2_gpu.py holds the whole network to fp64 through GLOBAL norms (all 14.8 M parameter gradients together), which cannot
see a local error: one bias gradient, one BatchNorm's d gamma, a stride-2 shortcut sampled at the wrong phase.  Here every distinct
convolution, BatchNorm block, pooling and decoder assembly runs at its real launch shape -- the 7x7 stem at full resolution, decoder
widths 34 .. 1026 (all = 2 mod 32), the one-input-channel input gradient of dispconv 0, multi-block BatchNorm statistics, max-pool
windows full of ties -- and single blocks check every parameter gradient on its own.

House rule: distance <= max(4 x (ATen fp32's distance to fp64), floor); pieces that only copy or select values are bit-identical.  The
references run on the device: ATen has no MIOpen path for fp64 (im2col + dgemm, asserted below), and the fp32 yardstick is ATen's native
path (MIOpen off), so no MIOpen kernel is compiled for these shapes."""
import numpy as np
import pytest

from tests.gpu_util import report

pytestmark = [pytest.mark.gpu]

N = 8
FEED = (320, 1024)
ENC, DEC = (64, 64, 128, 256, 512), (16, 32, 64, 128, 256)

# every convolution of Monodepth2Net at the feed, as (Cin, Cout, k, stride, bias, input H, input W); the decoder's on padded extents
_ENCODER = {
    "stem": (3, 64, 7, 2, False, 320, 1024),
    "layer1": (64, 64, 3, 1, False, 80, 256),
    "layer2.0.conv1": (64, 128, 3, 2, False, 80, 256),
    "layer2.0.downsample": (64, 128, 1, 2, False, 80, 256),
    "layer2": (128, 128, 3, 1, False, 40, 128),
    "layer3.0.conv1": (128, 256, 3, 2, False, 40, 128),
    "layer3.0.downsample": (128, 256, 1, 2, False, 40, 128),
    "layer3": (256, 256, 3, 1, False, 20, 64),
    "layer4.0.conv1": (256, 512, 3, 2, False, 20, 64),
    "layer4.0.downsample": (256, 512, 1, 2, False, 20, 64),
    "layer4": (512, 512, 3, 1, False, 10, 32),
}
# the decoder's convolutions as the step runs them: x (N, C1, h, w) -> nearest x2 if up == 2 -> cat skip (N, C2, up h, up w) ->
# reflection pad 1 (pad_cat) -> 3x3 convolution with bias -> interior + act (crop_act).  name -> (C1, up, C2, Cout, act, h, w)
_DECODER = {}
for _i in range(4, -1, -1):
    _h, _w = FEED[0] >> (_i + 1), FEED[1] >> (_i + 1)
    _DECODER[f"upconv({_i},0)"] = (ENC[4] if _i == 4 else DEC[_i + 1], 1, 0, DEC[_i], "elu", _h, _w)
    _DECODER[f"upconv({_i},1)"] = (DEC[_i], 2, ENC[_i - 1] if _i else 0, DEC[_i], "elu", _h, _w)
_DECODER["dispconv0"] = (DEC[0], 1, 0, 1, "sigmoid", FEED[0], FEED[1])
_TABLE = dict(_ENCODER)
for _n, (_c1, _up, _c2, _co, _act, _h, _w) in _DECODER.items():
    _TABLE[_n] = (_c1 + _c2, _co, 3, 1, True, _up * _h + 2, _up * _w + 2)

# floors of the house rule: element-wise pieces and convolutions (max-norm), blocks (relative L2 per tensor)
_FLOOR = 2e-6
_BLOCK_FLOOR = 1e-5
# One measured exception.  The bias gradient of upconv(0,0) in the (0, *) stage sums a gradient whose sum cancels to 2.4e-4 of its L1 norm
# (the loss's cos weights), so a systematic per-element error becomes a visible one: the split-bf16 convolutions (the default arithmetic)
# give that gradient within 1.6e-7 (relative L2) of fp64, yet its sum 9.0e-5 off; the library's fp32-instruction kernels
# (CD_AMD_CONV_ARITH=0) 8.9e-7, ATen fp32 8.6e-7.  The sum itself (cd_channel_sum) is within 4.6e-7 of the fp64 sum of the same gradient.
_BLOCK_BOUND = {("decoder (0, *) + dispconv 0 @160x512", "0.conv.conv.bias"): 2e-4}


def _seed(name):
    return sum(ord(c) * (i + 1) for i, c in enumerate(name)) % 100003


def _rnd(g, *shape):
    import torch
    return torch.randn(shape, dtype=torch.float64, device="cuda", generator=g)


def _rel(a, b):
    """max |a - b| / max |b| in fp64 on the device."""
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)


def _rel2(a, b):
    """||a - b|| / ||b|| in fp64 on the device."""
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).norm()) / max(float(b.norm()), 1e-300)


def _check(test, case, got, ref, floor, floors=None):
    report(test, case=case, **{k: f"{v:.2e}" for k, v in got.items()}, **{"ref_" + k: f"{v:.2e}" for k, v in ref.items()})
    floors = floors or {}
    bad = {k: (v, ref[k]) for k, v in got.items() if not v <= max(4 * ref[k], floors.get(k, floor))}
    assert not bad, bad


def _aten32():
    """ATen's native fp32 path: MIOpen off."""
    import torch
    return torch.backends.cudnn.flags(enabled=False)


# ------------------------------------------------------------------------------------------------------------------ 1. the layer table
def test_layer_table_is_the_networks():
    """The distinct (Cin, Cout, k, stride, bias, input H x W) of every HipConv2d in one forward of Monodepth2Net at the feed, N = 8, equal
    the table the tests below are parametrised from (a new shape in the network fails here first, by name); and the references of every
    entry take ATen's native convolution: no MIOpen path in fp64, none in fp32 with MIOpen off."""
    import torch
    from consistent_depth_amd.monodepth.monodepth2_net import Monodepth2Net
    from consistent_depth_amd.ops.conv_layer import HipConv2d
    torch.manual_seed(0)
    net = Monodepth2Net(FEED).cuda().train()
    seen = set()

    def hook(m, inp, out):
        x = inp[0]
        assert x.shape[0] == N
        seen.add((m.in_channels, m.out_channels, m.kernel_size[0], m.stride[0], m.bias is not None) + tuple(x.shape[2:]))
    hooks = [m.register_forward_hook(hook) for m in net.modules() if isinstance(m, HipConv2d)]
    with torch.no_grad():
        net(torch.rand(N, 3, *FEED, device="cuda"))
    for h in hooks:
        h.remove()
    table = set(_TABLE.values())
    assert len(table) == len(_TABLE) == 22
    assert seen == table, {"not in the table": sorted(seen - table), "not in the network": sorted(table - seen)}
    slow = {torch._C._ConvBackend.Slow2d}
    for name, (Cin, Cout, k, s, bias, H, W) in _TABLE.items():
        for dtype in (torch.float64, torch.float32):
            x = torch.empty(1, Cin, H, W, dtype=dtype, device="cuda")
            w = torch.empty(Cout, Cin, k, k, dtype=dtype, device="cuda")
            p = [0, 0] if name in _DECODER else [(k - 1) // 2] * 2        # (the decoder's reference: valid convolution of the padded input)
            with _aten32():
                be = torch._C._select_conv_backend(x, w, None, [s, s], p, [1, 1], False, [0, 0], 1, None)
            assert be in slow, (Cin, Cout, k, H, W, dtype, be)


# ------------------------------------------------------------------------------------------------------------------ 2. every convolution
@pytest.mark.parametrize("name", list(_TABLE))
def test_conv_matches_fp64_at_its_real_shape(name):
    """One standalone layer per table entry against F.conv2d in fp64: output, input gradient (the stem's too, which the step does not
    need), weight gradient, bias gradient.  A decoder entry is the composite the step runs -- pad_cat -> HipConv2d -> crop_act against
    ReflectionPad2d(1) + valid Conv2d + ELU / sigmoid -- with that level's skip and nearest x2; its convolution's upstream gradient has
    the zero ring of the crop, as in the step.  dispconv 0's input gradient is the dense 3x3 convolution with ONE output channel
    (16 <- 1) on the fp32 kernel."""
    import torch
    import torch.nn.functional as F
    from consistent_depth_amd.ops.conv_layer import HipConv2d
    from consistent_depth_amd.ops.resample import HipReflectConv3x3, crop_act, pad_cat
    Cin, Cout, k, s, bias, H, W = _TABLE[name]
    torch.manual_seed(_seed(name))
    g = torch.Generator(device="cuda").manual_seed(_seed(name))
    if name in _DECODER:
        C1, up, C2, _, act, h, w = _DECODER[name]
        mod = HipReflectConv3x3(Cin, Cout).cuda()
        layer = mod.conv
        ins64 = [_rnd(g, N, C1, h, w)] + ([_rnd(g, N, C2, up * h, up * w)] if C2 else [])

        def hip(x, skip=None):
            return crop_act(mod(pad_cat(x, up, skip)), act)

        def aten(wt, b, x, skip=None):
            u = F.interpolate(x, scale_factor=2, mode="nearest") if up == 2 else x
            z = F.conv2d(F.pad(torch.cat([u, skip], 1) if skip is not None else u, (1, 1, 1, 1), mode="reflect"), wt, b)
            return F.elu(z) if act == "elu" else torch.sigmoid(z)
    else:
        layer = hip = HipConv2d(Cin, Cout, k, s, (k - 1) // 2, bias=False).cuda()
        ins64 = [_rnd(g, N, Cin, H, W)]

        def aten(wt, b, x):
            return F.conv2d(x, wt, b, s, (k - 1) // 2)
    params64 = [layer.weight.detach().double()] + ([layer.bias.detach().double()] if bias else [])
    xs = [t.float().requires_grad_(True) for t in ins64]
    y = hip(*xs)
    dy64 = _rnd(g, *y.shape)
    y.backward(dy64.float())
    hip_out = [y] + [t.grad for t in xs] + [layer.weight.grad] + ([layer.bias.grad] if bias else [])

    def reference(dtype):
        ps = [p.detach().to(dtype).requires_grad_(True) for p in params64]
        xr = [t.detach().to(dtype).requires_grad_(True) for t in ins64]
        with _aten32():
            yr = aten(ps[0], ps[1] if bias else None, *xr)
            yr.backward(dy64.to(dtype))
        return [yr.detach()] + [t.grad for t in xr] + [p.grad for p in ps]
    r64 = reference(torch.float64)
    r32 = reference(torch.float32)
    keys = ["y", "dx", "dskip"][:1 + len(ins64)] + ["dw", "db"][:1 + int(bias)]
    got = {k_: _rel(a, b) for k_, a, b in zip(keys, hip_out, r64)}
    ref = {k_: _rel(a, b) for k_, a, b in zip(keys, r32, r64)}
    _check("monodepth2_layer_conv", f"{name} {Cin}->{Cout} k{k} s{s}{' bias' if bias else ''} @{H}x{W}", got, ref, _FLOOR)


# ------------------------------------------------------------------------------------------------------------------ 3. launch shapes
def _tuned_directions(name):
    """The passes of a table entry that HipConv2d routes through ops.conv.tuned_config (conv_layer._dense_cfg: dense, k >= 3, >= 8 input
    channels), as (direction, input channels, output channels)."""
    Cin, Cout, k, _, _, _, _ = _TABLE[name]
    return [(d, ci, co) for d, ci, co in (("forward", Cin, Cout), ("input gradient", Cout, Cin)) if k >= 3 and ci >= 8]


@pytest.mark.parametrize("name", [n for n in _TABLE if _tuned_directions(n)])
def test_every_launch_shape_gives_the_same_bits_at_real_shapes(name):
    """tuned_config picks (tile_rows, co_tiles) by timing on the box and caches it (per process, or on disk): results are box-independent
    only if every admissible launch shape gives the same bits at the step's own shapes -- the decoder's widths 34 .. 1026 leave 2 valid
    columns in the last 32-pixel tile of every row.  Every shape tuned_config would try, forward (with bias) and input gradient
    (transposed filter); the first one also against fp64."""
    import torch
    import torch.nn.functional as F
    from consistent_depth_amd import _native
    from consistent_depth_amd.ops import conv as C
    Cin, Cout, k, s, bias, H, W = _TABLE[name]
    lib = _native.lib()
    g = torch.Generator(device="cuda").manual_seed(_seed(name) + 1)
    w64 = _rnd(g, Cout, Cin, k, k) / np.sqrt(Cin * k * k)
    b64 = _rnd(g, Cout) * 0.1 if bias else None
    for direction, ci, co in _tuned_directions(name):
        fwd = direction == "forward"
        x64 = _rnd(g, N, ci, H, W)
        x = x64.float()
        pk = C.pack_weights(w64.float(), transposed=not fwd)
        b = b64.float() if (fwd and bias) else None
        max_cot = lib.cd_conv2d_packed_co_tiles(co, k)
        first, shapes = None, []
        for ty in C._TILE_HINTS:
            for cot in (1, 2, 4, 8, 16):
                if cot > max_cot or (cot == 16 and ty > 4) or (cot == 8 and ty > 8) or (ty == 32 and cot > 1):
                    continue
                try:
                    out = C.conv2d(x, pk, ci, co, k, bias=b, cfg=(ty, cot))
                except RuntimeError:      # (not available for this filter: tuned_config skips it too)
                    continue
                shapes.append((ty, cot))
                if first is None:
                    first = out
                else:
                    assert torch.equal(out, first), (direction, (ty, cot), shapes[0])
        assert len(shapes) >= 2, (direction, shapes)
        wt = w64 if fwd else w64.transpose(0, 1).flip(2, 3)
        bt = b64 if (fwd and bias) else None
        y64 = F.conv2d(x64, wt, bt, padding=(k - 1) // 2)
        with _aten32():
            y32 = F.conv2d(x, wt.float(), bt.float() if bt is not None else None, padding=(k - 1) // 2)
        _check("monodepth2_launch_shapes", f"{name} {direction} {ci}->{co} k{k} @{H}x{W} shapes={len(shapes)}",
               {"y": _rel(first, y64)}, {"y": _rel(y32, y64)}, _FLOOR)


# ------------------------------------------------------------------------------------------------------------------ 4. BatchNorm blocks
_BN_CASES = {f"{where} {variant}": (shape, relu, res, 0) for where, shape in (("stem", (N, 64, 160, 512)), ("layer1", (N, 64, 80, 256)))
             for variant, relu, res in (("relu", True, False), ("plain", False, False), ("res_relu", True, True))}
_BN_CASES.update({f"stem |mean| = {m} std": ((N, 64, 160, 512), False, False, m) for m in (30, 100)})


@pytest.mark.parametrize("case", list(_BN_CASES))
def test_bn_block_matches_batchnorm_fp64_at_real_counts(case):
    """ops.blocks.bn_act (act(BatchNorm2d_train(x) [+ res]), csrc/bn_block.hip) at the stem's and layer1's real extents -- 655 360 and
    163 840 samples per channel, multi-block statistics (gridDim.x 20 and 5) -- against nn.BatchNorm2d in fp64: output, input and
    residual gradients, d gamma, d beta, running mean / variance and the batch counter.  The upstream gradient is w * y (loss 1/2 w y^2),
    which vanishes where a ReLU decides (a mask flip at |pre-activation| ~ 1e-7 would otherwise be an O(1) difference at one element).
    The |mean| = 30 / 100 std cases hold the statistics to the same rule where E[x^2] - mean^2 cancels."""
    import torch
    import torch.nn as nn
    import torch.nn.functional as F
    from consistent_depth_amd.ops import blocks as B
    shape, relu, with_res, offset = _BN_CASES[case]
    C = shape[1]
    g = torch.Generator(device="cuda").manual_seed(_seed(case))
    std = torch.rand(C, dtype=torch.float64, device="cuda", generator=g) * 1.5 + 0.5
    sign = torch.where(_rnd(g, C) < 0, -1.0, 1.0)
    mean = offset * std * sign if offset else _rnd(g, C) * 0.5
    x64 = (_rnd(g, *shape) * std.view(1, -1, 1, 1) + mean.view(1, -1, 1, 1)).float().double()   # the same input for all three
    r64 = _rnd(g, *shape).float().double() if with_res else None
    wgt = torch.cos(torch.arange(x64.numel(), dtype=torch.float64, device="cuda").reshape(shape) * 0.37)
    bn64 = nn.BatchNorm2d(C).double().cuda().train()
    with torch.no_grad():
        bn64.weight.copy_(torch.rand(C, dtype=torch.float64, device="cuda", generator=g) + 0.5)
        bn64.bias.copy_(_rnd(g, C) * 0.3)
    res = {}
    for tag, dtype in (("hip", torch.float32), ("aten", torch.float32), ("fp64", torch.float64)):
        bn = bn64 if tag == "fp64" else nn.BatchNorm2d(C).cuda().train()
        if tag != "fp64":
            bn.load_state_dict(bn64.state_dict())
        x = x64.detach().to(dtype).requires_grad_(True)
        r = r64.detach().to(dtype).requires_grad_(True) if with_res else None
        with _aten32():
            if tag == "hip":
                y = B.bn_act(x, bn, relu, r)
            else:
                y = bn(x)
                y = y + r if with_res else y
                y = F.relu(y) if relu else y
            (0.5 * wgt.to(dtype) * y * y).sum().backward()
        res[tag] = {"y": y.detach(), "dx": x.grad, "dgamma": bn.weight.grad, "dbeta": bn.bias.grad, "running_mean": bn.running_mean,
                    "running_var": bn.running_var}
        if with_res:
            res[tag]["dres"] = r.grad
        assert int(bn.num_batches_tracked) == 1, tag
    got = {k: _rel(v, res["fp64"][k]) for k, v in res["hip"].items()}
    ref = {k: _rel(v, res["fp64"][k]) for k, v in res["aten"].items()}
    _check("monodepth2_layer_bn", f"{case} {'x'.join(map(str, shape))}", got, ref, _FLOOR)


# ------------------------------------------------------------------------------------------------------------------ 5. max-pool, pad_cat, crop_act
@pytest.mark.parametrize("ties", [False, True], ids=["relu_randn", "tied_windows"])
def test_maxpool_is_bit_identical_at_the_stem(ties):
    """ops.blocks.maxpool3s2 on the stem's output extent (8, 64, 160, 512) against F.max_pool2d(x, 3, 2, 1), forward and backward, bit for
    bit: post-ReLU data (half of it exact zeros), then the same with whole 3x3 windows set to one value (zero or positive) -- where the
    first-index rule alone decides which input gets the gradient."""
    import torch
    import torch.nn.functional as F
    from consistent_depth_amd.ops import blocks as B
    shape = (N, 64, 160, 512)
    Ho, Wo = 80, 256
    g = torch.Generator(device="cuda").manual_seed(11 + ties)
    x = torch.relu(torch.randn(shape, device="cuda", generator=g))
    if ties:
        xp = F.pad(x, (1, 1, 1, 1))          # window (oy, ox) = xp[2 oy : 2 oy + 3, 2 ox : 2 ox + 3]
        sel = torch.zeros(N, 64, Ho, Wo, dtype=torch.bool, device="cuda")
        sel[:, :, ::2, ::2] = torch.rand(N, 64, Ho // 2, Wo // 2, device="cuda", generator=g) < 0.5    # disjoint windows
        val = torch.rand(N, 64, Ho, Wo, device="cuda", generator=g)
        val = torch.where(val < 0.5, torch.zeros_like(val), val)
        for dy in range(3):
            for dx in range(3):
                v = xp[:, :, dy:dy + 2 * Ho:2, dx:dx + 2 * Wo:2]
                v.copy_(torch.where(sel, val, v))
        x = xp[:, :, 1:-1, 1:-1].contiguous()
        win = F.unfold(F.pad(x, (1, 1, 1, 1), value=-1.0), 3, stride=2).view(N, 64, 9, Ho * Wo)
        full = (win == win[:, :, :1]).all(2)
        assert int(full.sum()) > N * 64 * Ho * Wo // 16, int(full.sum())
    x1, x2 = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    y1 = B.maxpool3s2(x1)
    with _aten32():
        y2 = F.max_pool2d(x2, 3, 2, 1)
    assert y1.shape == y2.shape and torch.equal(y1, y2)
    d = torch.randn(y2.shape, device="cuda", generator=g)
    y1.backward(d)
    y2.backward(d)
    assert torch.equal(x1.grad, x2.grad)
    report("monodepth2_layer_maxpool", case="tied_windows" if ties else "relu_randn", zeros=f"{float((x == 0).float().mean()):.3f}",
           bitwise=True)


@pytest.mark.parametrize("name", list(_DECODER))
def test_pad_cat_at_every_decoder_input(name):
    """ops.resample.pad_cat with each decoder convolution's real C1, up and C2: the forward is a pure copy (bit-identical to
    ReflectionPad2d(1)(cat(nearest x2, skip)) in fp32), the backward (the adjoint's sums over the ring and the four up-sampled copies)
    meets the rule against fp64."""
    import torch
    import torch.nn.functional as F
    from consistent_depth_amd.ops.resample import pad_cat
    C1, up, C2, _, _, h, w = _DECODER[name]
    g = torch.Generator(device="cuda").manual_seed(_seed(name) + 2)
    x64 = _rnd(g, N, C1, h, w)
    s64 = _rnd(g, N, C2, up * h, up * w) if C2 else None

    def twin(x, s):
        u = F.interpolate(x, scale_factor=2, mode="nearest") if up == 2 else x
        return F.pad(torch.cat([u, s], 1) if s is not None else u, (1, 1, 1, 1), mode="reflect")
    res = {}
    for tag, dtype in (("hip", torch.float32), ("aten", torch.float32), ("fp64", torch.float64)):
        x = x64.detach().to(dtype).requires_grad_(True)
        s = s64.detach().to(dtype).requires_grad_(True) if C2 else None
        with _aten32():
            out = pad_cat(x, up, s) if tag == "hip" else twin(x, s)
            if tag != "fp64":
                res[tag + "_y"] = out.detach()
            dout = torch.cos(torch.arange(out.numel(), dtype=torch.float64, device="cuda").reshape(out.shape) * 0.61).to(dtype)
            out.backward(dout)
        res[tag] = {"dx": x.grad, **({"dskip": s.grad} if C2 else {})}
    assert torch.equal(res["hip_y"], res["aten_y"])
    got = {k: _rel(v, res["fp64"][k]) for k, v in res["hip"].items()}
    ref = {k: _rel(v, res["fp64"][k]) for k, v in res["aten"].items()}
    _check("monodepth2_layer_pad_cat", f"{name} x {(N, C1, h, w)} up {up} skip {C2}", got, ref, _FLOOR)


@pytest.mark.parametrize("name", list(_DECODER))
def test_crop_act_at_every_decoder_output(name):
    """ops.resample.crop_act at each decoder convolution's real padded output (ELU at the ten upconvs, sigmoid at dispconv 0's
    (8, 1, 320, 1024)): output and input gradient against fp64, the input gradient's ring exactly zero."""
    import torch
    import torch.nn.functional as F
    from consistent_depth_amd.ops.resample import crop_act
    _, up, _, Cout, act, h, w = _DECODER[name]
    H, W = up * h, up * w
    fn = F.elu if act == "elu" else torch.sigmoid
    g = torch.Generator(device="cuda").manual_seed(_seed(name) + 3)
    xp64 = 2 * _rnd(g, N, Cout, H + 2, W + 2)
    dy64 = _rnd(g, N, Cout, H, W)
    res = {}
    for tag, dtype in (("hip", torch.float32), ("aten", torch.float32), ("fp64", torch.float64)):
        xp = xp64.detach().to(dtype).requires_grad_(True)
        y = crop_act(xp, act) if tag == "hip" else fn(xp[:, :, 1:-1, 1:-1])
        y.backward(dy64.to(dtype))
        res[tag] = {"y": y.detach(), "dx": xp.grad}
    ring = res["hip"]["dx"].clone()
    ring[:, :, 1:-1, 1:-1] = 0
    assert not ring.any()
    got = {k: _rel(v, res["fp64"][k]) for k, v in res["hip"].items()}
    ref = {k: _rel(v, res["fp64"][k]) for k, v in res["aten"].items()}
    _check("monodepth2_layer_crop_act", f"{name} {act} {(N, Cout, H, W)}", got, ref, _FLOOR)


# ------------------------------------------------------------------------------------------------------------------ 6. blocks
_BLOCKS = {
    "layer1.0 @80x256": ("encoder.encoder.layer1.0", [(N, 64, 80, 256)]),
    "layer2.0 (stride 2, 1x1 shortcut) @80x256": ("encoder.encoder.layer2.0", [(N, 64, 80, 256)]),
    "layer3.0 (stride 2, 1x1 shortcut) @40x128": ("encoder.encoder.layer3.0", [(N, 128, 40, 128)]),
    "layer4.0 (stride 2, 1x1 shortcut) @20x64": ("encoder.encoder.layer4.0", [(N, 256, 20, 64)]),
    "decoder (4, *) @10x32, skip @20x64": ((0, 1), [(N, 512, 10, 32), (N, 256, 20, 64)]),
    "decoder (0, *) + dispconv 0 @160x512": ((8, 9, 10), [(N, 32, 160, 512)]),
}


def _block(net, name, hip):
    """(module holding the block's parameters, callable) of one block of the HIP network (hip=True) or of the ATen twin."""
    import torch
    import torch.nn.functional as F
    from consistent_depth_amd.ops.resample import crop_act, pad_cat
    spec, _ = _BLOCKS[name]
    if isinstance(spec, str):
        m = net.get_submodule(spec)
        return m, m
    dec = net.depth_decoder.decoder
    mods = torch.nn.ModuleList([dec[j] for j in spec])
    up = lambda t: F.interpolate(t, scale_factor=2, mode="nearest")  # noqa: E731
    if spec == (0, 1):
        if hip:
            return mods, lambda x, s: dec[1](pad_cat(dec[0](pad_cat(x)), 2, s))
        return mods, lambda x, s: dec[1](torch.cat([up(dec[0](x)), s], 1))
    if hip:
        return mods, lambda x: crop_act(dec[10](pad_cat(dec[9](pad_cat(dec[8](pad_cat(x)), 2)))), "sigmoid")
    return mods, lambda x: torch.sigmoid(dec[10](dec[9](up(dec[8](x)))))


@pytest.mark.parametrize("name", list(_BLOCKS))
def test_block_matches_fp64_per_tensor(name):
    """Single blocks of Monodepth2Net at their real extents (N = 8) against the same block of the ATen twin in fp64: the output, every
    input gradient and EVERY parameter gradient on its own (relative L2), each within 4x the ATen fp32 twin's distance.  A stride-2
    shortcut sampled at the wrong phase, one BatchNorm's d gamma or one bias gradient scaled wrongly is an error of its own tensor here,
    where the whole-network test sees it through the norm of all 14.8 M gradients.  Loss 1/2 w y^2 (the output's own ReLU flips do not
    reach the gradients)."""
    import torch
    from consistent_depth_amd.monodepth.monodepth2_net import Monodepth2Net
    from tests.monodepth2_twin import twin
    torch.manual_seed(_seed(name))
    net = Monodepth2Net(FEED).cuda().train()
    nets = {"hip": net}
    for tag in ("aten", "fp64"):
        t = twin(FEED)
        t.encoder.load_state_dict(net.encoder.state_dict())
        t.depth_decoder.load_state_dict(net.depth_decoder.state_dict())
        nets[tag] = (t.cuda().double() if tag == "fp64" else t.cuda()).train()
    g = torch.Generator(device="cuda").manual_seed(_seed(name) + 4)
    _, shapes = _BLOCKS[name]
    ins64 = [_rnd(g, *s) for s in shapes]
    if isinstance(_BLOCKS[name][0], str):
        ins64[0] = torch.relu(ins64[0])       # an encoder block reads post-ReLU features
    res = {}
    for tag, dtype in (("hip", torch.float32), ("aten", torch.float32), ("fp64", torch.float64)):
        mods, fn = _block(nets[tag], name, tag == "hip")
        if tag == "hip":
            net._pack_pool.invalidate()       # a pooled layer called outside the network's forward re-packs the pool
        xs = [t.detach().to(dtype).requires_grad_(True) for t in ins64]
        with _aten32():
            y = fn(*xs)
            w = torch.cos(torch.arange(y.numel(), dtype=torch.float64, device="cuda").reshape(y.shape) * 0.37).to(dtype)
            (0.5 * w * y * y).sum().backward()
        res[tag] = {"y": y.detach(), **{f"d_in{i}": t.grad for i, t in enumerate(xs)},
                    **{k: p.grad for k, p in mods.named_parameters() if p.grad is not None}}
    assert set(res["hip"]) == set(res["fp64"]) == set(res["aten"])
    assert sum(1 for k in res["fp64"] if k.endswith("weight")) >= 2
    got = {k: _rel2(v, res["fp64"][k]) for k, v in res["hip"].items()}
    ref = {k: _rel2(v, res["fp64"][k]) for k, v in res["aten"].items()}
    _check("monodepth2_layer_block", name, got, ref, _BLOCK_FLOOR, {k: v for (b, k), v in _BLOCK_BOUND.items() if b == name})
