"""The native stride-2 convolution (csrc/conv_strided.hip) on the GPU, through the C ABI via the ops.conv wrappers: forward, input
gradient and weight gradient of nn.Conv2d(k = 3, stride = 2, padding = 1), dense and grouped, against fp64 autograd with the
project's yardstick (relative max error <= max(4 x the distance of ATen's own fp32 evaluation to the same fp64 result, 2e-6));
the 2x2 sub-sampling helpers of the 1x1 / 2 shortcuts; refusals; the HipConv2d layer (only cd:: kernels; the old path behind
CD_AMD_CONV_STRIDED=0 still alive).  Outputs are pre-filled with NaN and followed by a guard region that must stay untouched.
References are computed on the device in fp64 and fp32 with MIOpen off, as tests/test_monodepth2_layers_gpu.py does."""
import json
import os
import subprocess
import sys

import pytest

from tests.gpu_util import report

pytestmark = [pytest.mark.gpu]

GUARD = 256
FLOOR = 2e-6

# (cin_g, cout_g, groups, N, H, W): the stage entries of ResNet-18 at the KITTI feed and the strided grouped 3x3 of ResNeXt-101 32x8d
NETWORK = [
    (64, 128, 1, 8, 80, 256), (128, 256, 1, 8, 40, 128), (256, 512, 1, 8, 20, 64),
    (16, 16, 32, 8, 96, 96), (32, 32, 32, 8, 48, 48), (64, 64, 32, 8, 24, 24),
]
_COUT_OF = {8: 40, 16: 24, 24: 16, 40: 8}
SMALL = [(c, _COUT_OF[c], g, 2, h, w, b) for (h, w) in [(13, 7), (1, 5), (2, 2), (17, 33), (16, 64), (9, 65)]
         for c in (8, 16, 24, 40) for g in (1, 4) for b in (False, True)]


def _guarded(shape, fill=float("nan")):
    import torch
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + GUARD,), fill, dtype=torch.float32, device="cuda")
    buf[n:] = 12345.0
    return buf, buf[:n].view(shape)


def _guard_ok(buf):
    return bool((buf[-GUARD:] == 12345.0).all())


def _packs(w, G, transposed):
    """The packed filters of all groups side by side (equal, 64-float aligned parts)."""
    import torch
    from consistent_depth_amd.ops import conv as C
    cout_g = w.shape[0] // G
    parts = [C.pack_weights(w[g * cout_g:(g + 1) * cout_g].contiguous(), transposed) for g in range(G)]
    n = (parts[0].numel() + 63) // 64 * 64
    arena = torch.zeros(G * n, dtype=torch.float32, device=w.device)
    for g, p in enumerate(parts):
        arena[g * n:g * n + p.numel()] = p
    return arena


def _rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)


def _inputs(cin_g, cout_g, G, N, H, W, bias, seed):
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    r = lambda *s: torch.randn(s, dtype=torch.float32, device="cuda", generator=g)  # noqa: E731
    return r(N, G * cin_g, H, W), r(G * cout_g, cin_g, 3, 3) * 0.1, (r(G * cout_g) if bias else None), r(N, G * cout_g, Ho, Wo)


def _references(x, w, b, dy, G):
    """(y, dx, dw, db) in fp64 and in ATen's fp32, on the device, MIOpen off."""
    import torch
    import torch.nn.functional as F
    out = []
    with torch.backends.cudnn.flags(enabled=False):
        for dt in (torch.float64, torch.float32):
            xx, ww = x.to(dt).requires_grad_(True), w.to(dt).requires_grad_(True)
            bb = b.to(dt).requires_grad_(True) if b is not None else None
            y = F.conv2d(xx, ww, bb, 2, 1, 1, G)
            y.backward(dy.to(dt))
            out.append((y.detach(), xx.grad, ww.grad, bb.grad if bb is not None else None))
    return out


def _native_passes(x, w, b, dy, cin_g, cout_g, G, prev_y=None, prev_dx=None):
    """y, dx, dw (and db) by the strided entries; outputs NaN-prefilled (or `prev` for accumulate) with guards."""
    import torch
    from consistent_depth_amd.ops import conv as C
    from consistent_depth_amd.ops.layers import channel_sum
    pk, pkT = _packs(w, G, False), _packs(w, G, True)
    ybuf, y = _guarded(tuple(dy.shape))
    dxbuf, dx = _guarded(tuple(x.shape))
    dwbuf, dw = _guarded(tuple(w.shape))
    if prev_y is not None:
        y.copy_(prev_y)
    if prev_dx is not None:
        dx.copy_(prev_dx)
    C.conv2d_strided(x, pk, cin_g, cout_g, 3, groups=G, bias=b, out=y, accumulate=prev_y is not None)
    C.conv2d_dgrad_strided(dy, pkT, cin_g, cout_g, 3, dx, groups=G, accumulate=prev_dx is not None)
    n = (C.wgrad_workspace_floats(cout_g, cin_g, 3) + 63) // 64 * 64
    ws = torch.empty(G * n, dtype=torch.float32, device="cuda")
    C.conv2d_wgrad_strided(x, dy, cin_g, cout_g, 3, dw, ws, groups=G)
    db = None
    if b is not None:
        db = torch.empty_like(b)
        channel_sum(dy, 0, dy.shape[1], db)
    torch.cuda.synchronize()
    assert _guard_ok(ybuf) and _guard_ok(dxbuf) and _guard_ok(dwbuf), "a guard region was written"
    return y, dx, dw, db


def _parity(test, case, cin_g, cout_g, G, N, H, W, bias, accumulate=False):
    import torch
    x, w, b, dy = _inputs(cin_g, cout_g, G, N, H, W, bias, seed=cin_g * 7 + cout_g * 3 + G + H * 131 + W)
    prev_y = torch.randn_like(dy) if accumulate else None
    prev_dx = torch.randn_like(x) if accumulate else None
    y, dx, dw, db = _native_passes(x, w, b, dy, cin_g, cout_g, G, prev_y, prev_dx)
    # the input gradient writes every element (the NaN pre-fill is gone everywhere), and so do the others
    for name, t in (("y", y), ("dx", dx), ("dw", dw)):
        assert not bool(torch.isnan(t).any()), f"{name}: elements left unwritten"
    (y64, dx64, dw64, db64), (y32, dx32, dw32, db32) = _references(x, w, b, dy, G)
    if accumulate:
        y64, y32 = y64 + prev_y.double(), y32 + prev_y
        dx64, dx32 = dx64 + prev_dx.double(), dx32 + prev_dx
    got = {"y": _rel(y, y64), "dx": _rel(dx, dx64), "dw": _rel(dw, dw64)}
    ref = {"y": _rel(y32, y64), "dx": _rel(dx32, dx64), "dw": _rel(dw32, dw64)}
    if bias:
        got["db"], ref["db"] = _rel(db, db64), _rel(db32, db64)
    report(test, case=case, **{k: f"{v:.2e}" for k, v in got.items()}, **{"ref_" + k: f"{v:.2e}" for k, v in ref.items()})
    bad = {k: (v, ref[k]) for k, v in got.items() if not v <= max(4 * ref[k], FLOOR)}
    assert not bad, bad


@pytest.mark.parametrize("case", NETWORK, ids=lambda c: "x".join(map(str, c)))
def test_network_shapes_match_fp64(case):
    cin_g, cout_g, G, N, H, W = case
    _parity("conv_strided_network", "x".join(map(str, case)), cin_g, cout_g, G, N, H, W, bias=False)


@pytest.mark.parametrize("case", SMALL, ids=lambda c: "x".join(map(str, c)))
def test_small_shapes_match_fp64(case):
    cin_g, cout_g, G, N, H, W, bias = case
    _parity("conv_strided_small", "x".join(map(str, case)), cin_g, cout_g, G, N, H, W, bias)


@pytest.mark.parametrize("case", [(16, 24, 4, 2, 13, 7), (24, 16, 1, 2, 17, 33), (40, 40, 1, 2, 16, 64), (8, 40, 4, 2, 9, 65)],
                         ids=lambda c: "x".join(map(str, c)))
def test_accumulate_adds_to_the_previous_content(case):
    cin_g, cout_g, G, N, H, W = case
    _parity("conv_strided_accumulate", "x".join(map(str, case)), cin_g, cout_g, G, N, H, W, bias=True, accumulate=True)


@pytest.mark.parametrize("case", [(64, 128, 1, 8, 80, 256), (16, 16, 32, 8, 96, 96), (24, 16, 4, 2, 13, 7)], ids=lambda c: "x".join(map(str, c)))
def test_every_pass_is_bit_reproducible(case):
    """Each pass twice on the same inputs gives the same bits (the kernels take no launch-shape hints: one shape per geometry)."""
    import torch
    cin_g, cout_g, G, N, H, W = case
    x, w, b, dy = _inputs(cin_g, cout_g, G, N, H, W, True, seed=5)
    first = _native_passes(x, w, b, dy, cin_g, cout_g, G)
    second = _native_passes(x, w, b, dy, cin_g, cout_g, G)
    for name, p, q in zip(("y", "dx", "dw"), first, second):
        assert torch.equal(p, q), name


@pytest.mark.parametrize("shape", [(2, 5, 12, 12), (1, 3, 7, 9), (2, 4, 1, 6), (8, 64, 80, 256)], ids=lambda s: "x".join(map(str, s)))
def test_subsample2_is_the_strided_slice_and_its_adjoint(shape):
    import torch
    from consistent_depth_amd.ops import conv as C
    N, Cc, H, W = shape
    x = torch.randn(shape, device="cuda")
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    ybuf, y = _guarded((N, Cc, Ho, Wo))
    C.subsample2(x, out=y)
    assert torch.equal(y, x[:, :, ::2, ::2]) and _guard_ok(ybuf)
    dy = torch.randn(N, Cc, Ho, Wo, device="cuda")
    dxbuf, dx = _guarded(shape)
    C.subsample2_bwd(dy, dx)
    want = torch.zeros(shape, device="cuda")
    want[:, :, ::2, ::2] = dy
    assert torch.equal(dx, want) and _guard_ok(dxbuf)
    # a channel slice of a wider buffer: the other channels stay untouched
    wide = torch.randn(N, Cc + 3, H, W, device="cuda")
    assert torch.equal(C.subsample2(wide, C=Cc, coff=2), wide[:, 2:2 + Cc, ::2, ::2])
    keep = wide.clone()
    C.subsample2_bwd(dy, wide, coff=2)
    assert torch.equal(wide[:, 2:2 + Cc], want) and torch.equal(wide[:, :2], keep[:, :2]) and torch.equal(wide[:, 2 + Cc:], keep[:, 2 + Cc:])


def test_refusals_leave_the_outputs_untouched():
    """stride 3, arithmetic mode 0 and k = 5 return CD_ERR_UNSUPPORTED and launch nothing: the NaN pre-fill is intact."""
    import torch
    from consistent_depth_amd import _native
    from consistent_depth_amd.ops import conv as C
    lib = _native.lib()
    cin_g = cout_g = 16
    x, w, _, dy = _inputs(cin_g, cout_g, 1, 2, 12, 12, False, seed=3)
    pk, pkT = _packs(w, 1, False), _packs(w, 1, True)
    ws = torch.empty(C.wgrad_workspace_floats(cout_g, cin_g, 3), dtype=torch.float32, device="cuda")
    w5 = torch.randn(cout_g, cin_g, 5, 5, device="cuda")
    pk5, pk5T = _packs(w5, 1, False), _packs(w5, 1, True)
    ws5 = torch.empty(C.wgrad_workspace_floats(cout_g, cin_g, 5), dtype=torch.float32, device="cuda")

    def all_refused(ks, stride, p, pT, wsp, wshape):
        ybuf, y = _guarded(tuple(dy.shape))
        dxbuf, dx = _guarded(tuple(x.shape))
        dwbuf, dw = _guarded(wshape)
        for call in (lambda: C.conv2d_strided(x, p, cin_g, cout_g, ks, out=y, stride=stride),
                     lambda: C.conv2d_dgrad_strided(dy, pT, cin_g, cout_g, ks, dx, stride=stride),
                     lambda: C.conv2d_wgrad_strided(x, dy, cin_g, cout_g, ks, dw, wsp, stride=stride)):
            with pytest.raises(RuntimeError, match="CD_ERR_UNSUPPORTED"):
                call()
        torch.cuda.synchronize()
        for buf in (ybuf, dxbuf, dwbuf):
            assert bool(torch.isnan(buf[:-GUARD]).all()) and _guard_ok(buf)

    all_refused(3, 3, pk, pkT, ws, tuple(w.shape))
    all_refused(5, 2, pk5, pk5T, ws5, tuple(w5.shape))
    mode = lib.cd_get_conv_arith()
    try:
        assert lib.cd_set_conv_arith(0) == 0
        all_refused(3, 2, pk, pkT, ws, tuple(w.shape))
    finally:
        lib.cd_set_conv_arith(mode)


LAYERS = [(64, 128, 3, 1), (128, 128, 3, 8), (64, 128, 1, 1)]    # (Cin, Cout, k, groups), all stride 2


def _layer_parity(Cin, Cout, k, G):
    """got / ref distances of a stride-2 HipConv2d forward + backward (the layer as the networks use it)."""
    import torch
    import torch.nn.functional as F
    from consistent_depth_amd.ops.conv_layer import HipConv2d
    torch.manual_seed(Cin + Cout + k + G)
    layer = HipConv2d(Cin, Cout, k, 2, (k - 1) // 2, groups=G, bias=True).cuda()
    x = torch.randn(2, Cin, 17, 33, device="cuda", requires_grad=True)
    y = layer(x)
    dy = torch.randn_like(y)
    y.backward(dy)
    res = {}
    with torch.backends.cudnn.flags(enabled=False):
        outs = []
        for dt in (torch.float64, torch.float32):
            xx = x.detach().to(dt).requires_grad_(True)
            ww, bb = layer.weight.detach().to(dt).requires_grad_(True), layer.bias.detach().to(dt).requires_grad_(True)
            yy = F.conv2d(xx, ww, bb, 2, (k - 1) // 2, 1, G)
            yy.backward(dy.to(dt))
            outs.append((yy.detach(), xx.grad, ww.grad, bb.grad))
    for name, got, r64, r32 in zip(("y", "dx", "dw", "db"), (y, x.grad, layer.weight.grad, layer.bias.grad), *outs):
        res[name] = (_rel(got, r64), _rel(r32, r64))
    return res


def test_the_strided_layer_launches_no_framework_kernels():
    """A stride-2 HipConv2d (3x3 dense, 3x3 grouped, 1x1) forward + backward launches only this package's kernels -- same method and
    skip rule as tests/test_finetune_gpu.py::test_the_step_launches_no_framework_kernels.  Without the native strided path the layer
    launches ATen copy / fill kernels (the sub-sampling copy, torch.zeros + the strided scatter)."""
    import torch
    from consistent_depth_amd.ops.conv_layer import HipConv2d
    torch.manual_seed(0)
    layers = [HipConv2d(Cin, Cout, k, 2, (k - 1) // 2, groups=G, bias=False).cuda() for Cin, Cout, k, G in LAYERS]
    xs = [torch.randn(2, l.in_channels, 16, 32, device="cuda", requires_grad=True) for l in layers]
    dys = [torch.randn(2, l.out_channels, 8, 16, device="cuda") for l in layers]

    def run():
        for l, x, dy in zip(layers, xs, dys):
            x.grad = None
            l.weight.grad = None
            torch.autograd.backward(l(x), dy)

    for _ in range(2):
        run()
    torch.cuda.synchronize()
    from torch.profiler import ProfilerActivity, profile
    try:
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            run()
            torch.cuda.synchronize()
        events = list(prof.events())
    except Exception as e:   # noqa: BLE001 -- the tracer, not the layer (it ran twice above)
        pytest.skip(f"torch.profiler is not usable on this stack: {type(e).__name__}: {e}")
    kernels = [e.name for e in events if str(getattr(e, "device_type", "")).endswith("CUDA") and e.name
               and not getattr(e, "is_user_annotation", False) and "#" not in e.name]
    if not any("cd::" in k for k in kernels):
        pytest.skip(f"torch.profiler reports no device kernels of this package on this stack ({len(kernels)} device events)")
    foreign = sorted({k for k in kernels if "cd::" not in k and "rocclr" not in k.lower() and not k.lower().startswith(("memcpy", "memset"))})
    assert not foreign, foreign
    assert any("conv_s2_fwd" in k for k in kernels) and any("conv_s2_dgrad" in k for k in kernels) and any("conv_s2_wgrad" in k for k in kernels)
    assert any("subsample2_fwd" in k for k in kernels) and any("subsample2_bwd" in k for k in kernels)


@pytest.mark.parametrize("case", LAYERS, ids=lambda c: "x".join(map(str, c)))
def test_the_strided_layer_matches_fp64(case):
    res = _layer_parity(*case)
    report("conv_strided_layer", case="x".join(map(str, case)), **{k: f"{g:.2e}/{r:.2e}" for k, (g, r) in res.items()})
    bad = {k: v for k, v in res.items() if not v[0] <= max(4 * v[1], FLOOR)}
    assert not bad, bad


def test_the_switch_keeps_the_old_path_alive():
    """CD_AMD_CONV_STRIDED=0 in a fresh child process: the same layers on the stride-1-plus-sub-sampling path, within the same bound."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import json, sys; sys.path.insert(0, %r); import tests.test_conv_strided_gpu as t; "
            "from consistent_depth_amd.ops import conv as C; assert not C.strided_enabled(); "
            "print('RESULT ' + json.dumps([t._layer_parity(*c) for c in t.LAYERS]))" % root)
    env = dict(os.environ, CD_AMD_CONV_STRIDED="0")
    p = subprocess.run([sys.executable, "-c", code], env=env, cwd=root, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1]
    for case, res in zip(LAYERS, json.loads(line[7:])):
        report("conv_strided_switch_off", case="x".join(map(str, case)), **{k: f"{g:.2e}/{r:.2e}" for k, (g, r) in res.items()})
        bad = {k: v for k, v in res.items() if not v[0] <= max(4 * v[1], FLOOR)}
        assert not bad, (case, bad)
