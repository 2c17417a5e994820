"""The native 7x7 / 2 RGB stem (csrc/conv_stem.hip) on the GPU, through the C ABI via the ops.conv wrappers: forward and weight
gradient of nn.Conv2d(cin <= 4, cout, 7, stride = 2, padding = 3) against fp64 autograd with the project's yardstick (relative max
error <= max(4 x the distance of ATen's own fp32 evaluation to the same fp64 result, 2e-6)); channel slices, accumulate, bit
reproducibility, refusals; the HipConv2d layer (only cd:: kernels, the old path behind CD_AMD_CONV_STEM=0 still alive, graph
capture).  Outputs are pre-filled with NaN and followed by a guard region that must stay untouched.  References are computed on the
device in fp64 and fp32 with MIOpen off, as tests/test_conv_strided_gpu.py does."""
import json
import os
import subprocess
import sys

import pytest

from tests.gpu_util import report

pytestmark = [pytest.mark.gpu]

GUARD = 256
FLOOR = 2e-6

# (cin, cout, N, H, W): the stems of monodepth2 (ResNet-18 at the KITTI feed) and midas2 (ResNeXt-101 at 384 x 384)
NETWORK = [(3, 64, 8, 320, 1024), (3, 64, 16, 384, 384)]
SMALL = [(cin, cout, 2, h, w, b) for (h, w) in [(13, 7), (1, 5), (2, 2), (17, 33), (16, 64), (9, 65)]
         for cin in (1, 3, 4) for cout in (8, 24, 40, 64) for b in (False, True)]


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


def _rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)


def _inputs(cin, cout, N, H, W, bias, seed, ks=7):
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    r = lambda *s: torch.randn(s, dtype=torch.float32, device="cuda", generator=g)  # noqa: E731
    return r(N, cin, H, W), r(cout, cin, ks, ks) * 0.1, (r(cout) if bias else None), r(N, cout, Ho, Wo)


def _references(x, w, b, dy, need_dx=False):
    """(y, dx, dw, db) in fp64 and in ATen's fp32, on the device, MIOpen off."""
    import torch
    import torch.nn.functional as F
    out = []
    with torch.backends.cudnn.flags(enabled=False):
        for dt in (torch.float64, torch.float32):
            xx, ww = x.to(dt).requires_grad_(need_dx), w.to(dt).requires_grad_(True)
            bb = b.to(dt).requires_grad_(True) if b is not None else None
            y = F.conv2d(xx, ww, bb, 2, 3)
            y.backward(dy.to(dt))
            out.append((y.detach(), xx.grad, ww.grad, bb.grad if bb is not None else None))
    return out


def _workspace(cout, cin):
    import torch
    from consistent_depth_amd.ops import conv as C
    return torch.empty(C.stem_wgrad_workspace_floats(cout, cin), dtype=torch.float32, device="cuda")


def _native_passes(x, w, b, dy, prev_dw=None):
    """y, dw (and db) by the stem entries; outputs NaN-prefilled (or `prev_dw` for accumulate) with guards."""
    import torch
    from consistent_depth_amd.ops import conv as C
    from consistent_depth_amd.ops.layers import channel_sum
    cout, cin = w.shape[:2]
    ybuf, y = _guarded(tuple(dy.shape))
    dwbuf, dw = _guarded(tuple(w.shape))
    if prev_dw is not None:
        dw.copy_(prev_dw)
    C.conv2d_stem(x, w, bias=b, out=y)
    C.conv2d_stem_wgrad(x, dy, dw, _workspace(cout, cin), accumulate=prev_dw is not None)
    db = None
    if b is not None:
        db = torch.empty_like(b)
        channel_sum(dy, 0, dy.shape[1], db)
    torch.cuda.synchronize()
    assert _guard_ok(ybuf) and _guard_ok(dwbuf), "a guard region was written"
    return y, dw, db


def _parity(test, case, cin, cout, N, H, W, bias, accumulate=False):
    import torch
    x, w, b, dy = _inputs(cin, cout, N, H, W, bias, seed=cin * 7 + cout * 3 + H * 131 + W)
    prev_dw = torch.randn_like(w) if accumulate else None
    y, dw, db = _native_passes(x, w, b, dy, prev_dw)
    for name, t in (("y", y), ("dw", dw)):
        assert not bool(torch.isnan(t).any()), f"{name}: elements left unwritten"
    (y64, _, dw64, db64), (y32, _, dw32, db32) = _references(x, w, b, dy)
    if accumulate:
        dw64, dw32 = dw64 + prev_dw.double(), dw32 + prev_dw
    got = {"y": _rel(y, y64), "dw": _rel(dw, dw64)}
    ref = {"y": _rel(y32, y64), "dw": _rel(dw32, dw64)}
    if bias:
        got["db"], ref["db"] = _rel(db, db64), _rel(db32, db64)
    report(test, case=case, **{k: f"{v:.2e}" for k, v in got.items()}, **{"ref_" + k: f"{v:.2e}" for k, v in ref.items()})
    bad = {k: (v, ref[k]) for k, v in got.items() if not v <= max(4 * ref[k], FLOOR)}
    assert not bad, bad


@pytest.mark.parametrize("case", NETWORK, ids=lambda c: "x".join(map(str, c)))
def test_network_shapes_match_fp64(case):
    cin, cout, N, H, W = case
    _parity("conv_stem_network", "x".join(map(str, case)), cin, cout, N, H, W, bias=True)


@pytest.mark.parametrize("case", SMALL, ids=lambda c: "x".join(map(str, c)))
def test_small_shapes_match_fp64(case):
    cin, cout, N, H, W, bias = case
    _parity("conv_stem_small", "x".join(map(str, case)), cin, cout, N, H, W, bias)


@pytest.mark.parametrize("case", [(3, 64, 2, 13, 7), (1, 24, 2, 17, 33), (4, 40, 2, 16, 64), (3, 8, 2, 9, 65)], ids=lambda c: "x".join(map(str, c)))
def test_accumulate_adds_to_the_previous_content(case):
    cin, cout, N, H, W = case
    _parity("conv_stem_accumulate", "x".join(map(str, case)), cin, cout, N, H, W, bias=True, accumulate=True)


@pytest.mark.parametrize("case", [(3, 24, 2, 17, 33), (4, 40, 2, 16, 64), (1, 64, 2, 9, 65)], ids=lambda c: "x".join(map(str, c)))
def test_a_channel_slice_leaves_the_other_channels_untouched(case):
    """x and dy / y are channel slices (x_coff, y_coff) of wider buffers: same bits as on tight tensors, nothing else written."""
    import torch
    from consistent_depth_amd.ops import conv as C
    cin, cout, N, H, W = case
    x, w, b, dy = _inputs(cin, cout, N, H, W, True, seed=11)
    y_t, dw_t, _ = _native_passes(x, w, b, dy)
    Ho, Wo = dy.shape[2:]
    xw = torch.randn(N, cin + 3, H, W, device="cuda")
    xw[:, 2:2 + cin] = x
    dyw = torch.randn(N, cout + 5, Ho, Wo, device="cuda")
    dyw[:, 4:4 + cout] = dy
    ybuf, yw = _guarded((N, cout + 5, Ho, Wo))
    C.conv2d_stem(xw, w, bias=b, out=yw, x_coff=2, y_coff=4)
    dwbuf, dw = _guarded(tuple(w.shape))
    C.conv2d_stem_wgrad(xw, dyw, dw, _workspace(cout, cin), x_coff=2, dy_coff=4)
    torch.cuda.synchronize()
    assert _guard_ok(ybuf) and _guard_ok(dwbuf)
    assert torch.equal(yw[:, 4:4 + cout], y_t) and torch.equal(dw, dw_t)
    assert bool(torch.isnan(yw[:, :4]).all()) and bool(torch.isnan(yw[:, 4 + cout:]).all())


@pytest.mark.parametrize("case", [(3, 64, 8, 320, 1024), (3, 64, 16, 384, 384), (4, 40, 2, 13, 7)], ids=lambda c: "x".join(map(str, c)))
def test_every_pass_is_bit_reproducible(case):
    import torch
    cin, cout, N, H, W = case
    x, w, b, dy = _inputs(cin, cout, N, H, W, True, seed=5)
    first = _native_passes(x, w, b, dy)
    second = _native_passes(x, w, b, dy)
    for name, p, q in zip(("y", "dw"), first, second):
        assert torch.equal(p, q), name


def test_refusals_leave_the_outputs_untouched():
    """stride 3, k = 3, 8 input channels and arithmetic mode 0 return CD_ERR_UNSUPPORTED and launch nothing: the NaN pre-fill is intact."""
    import torch
    from consistent_depth_amd import _native
    from consistent_depth_amd.ops import conv as C
    lib = _native.lib()

    def all_refused(cin, ks, stride):
        x, w, _, dy = _inputs(cin, 16, 2, 12, 12, False, seed=3, ks=ks)
        ws = torch.empty(max(C.stem_wgrad_workspace_floats(16, 3), 1), dtype=torch.float32, device="cuda")
        ybuf, y = _guarded(tuple(dy.shape))
        dwbuf, dw = _guarded(tuple(w.shape))
        for call in (lambda: C.conv2d_stem(x, w, out=y, stride=stride), lambda: C.conv2d_stem_wgrad(x, dy, dw, ws, stride=stride)):
            with pytest.raises(RuntimeError, match="CD_ERR_UNSUPPORTED"):
                call()
        torch.cuda.synchronize()
        for buf in (ybuf, dwbuf):
            assert bool(torch.isnan(buf[:-GUARD]).all()) and _guard_ok(buf)

    all_refused(3, 7, 3)
    all_refused(3, 3, 2)
    all_refused(8, 7, 2)
    mode = lib.cd_get_conv_arith()
    try:
        assert lib.cd_set_conv_arith(0) == 0
        all_refused(3, 7, 2)
    finally:
        lib.cd_set_conv_arith(mode)


def _layer_parity(need_dx):
    """got / ref distances of the stem HipConv2d forward + backward (the layer as the networks use it)."""
    import torch
    from consistent_depth_amd.ops.conv_layer import HipConv2d
    torch.manual_seed(7)
    layer = HipConv2d(3, 64, 7, 2, 3, bias=True).cuda()
    x = torch.randn(2, 3, 34, 66, device="cuda", requires_grad=need_dx)
    y = layer(x)
    dy = torch.randn_like(y)
    y.backward(dy)
    outs = _references(x.detach(), layer.weight.detach(), layer.bias.detach(), dy, need_dx=need_dx)
    res = {}
    for name, got, r64, r32 in zip(("y", "dx", "dw", "db"), (y, x.grad, layer.weight.grad, layer.bias.grad), *outs):
        if got is not None:
            res[name] = (_rel(got, r64), _rel(r32, r64))
    return res


def _check_layer(test, res, case):
    report(test, case=case, **{k: f"{g:.2e}/{r:.2e}" for k, (g, r) in res.items()})
    bad = {k: v for k, v in res.items() if not v[0] <= max(4 * v[1], FLOOR)}
    assert not bad, bad


def test_the_stem_layer_launches_no_framework_kernels():
    """HipConv2d(3, 64, 7, 2, 3) forward + backward on an input that needs no gradient launches only this package's kernels -- same
    method and skip rule as tests/test_conv_strided_gpu.py::test_the_strided_layer_launches_no_framework_kernels.  Without the stem
    kernels the layer launches ATen copy / fill kernels (the sub-sampling copy, torch.zeros + the strided scatter)."""
    import torch
    from consistent_depth_amd.ops.conv_layer import HipConv2d
    torch.manual_seed(0)
    layer = HipConv2d(3, 64, 7, 2, 3, bias=False).cuda()
    x = torch.randn(2, 3, 32, 64, device="cuda")
    dy = torch.randn(2, 64, 16, 32, device="cuda")

    def run():
        layer.weight.grad = None
        torch.autograd.backward(layer(x), dy)

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
    assert any("conv_stem_s2_fwd_kernel" in k for k in kernels) and any("conv_stem_s2_wgrad_kernel" in k for k in kernels), sorted(set(kernels))


def test_the_stem_layer_matches_fp64():
    _check_layer("conv_stem_layer", _layer_parity(False), "no_dx")


def test_an_input_that_needs_a_gradient_still_gets_dx():
    """x.requires_grad: y and dw on the stem kernels, dx from the zero-stuffed dy + stride-1 path -- within the parity rule."""
    res = _layer_parity(True)
    assert "dx" in res
    _check_layer("conv_stem_layer", res, "dx")


def test_the_switch_keeps_the_old_path_alive():
    """CD_AMD_CONV_STEM=0 in a fresh child process: the same layer on the stride-1-plus-sub-sampling path, within the same bound."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import json, sys; sys.path.insert(0, %r); import tests.test_conv_stem_gpu as t; "
            "from consistent_depth_amd.ops import conv as C; assert not C.stem_enabled(); "
            "print('RESULT ' + json.dumps([t._layer_parity(False), t._layer_parity(True)]))" % root)
    env = dict(os.environ, CD_AMD_CONV_STEM="0")
    p = subprocess.run([sys.executable, "-c", code], env=env, cwd=root, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1]
    for case, res in zip(("no_dx", "dx"), json.loads(line[7:])):
        _check_layer("conv_stem_switch_off", res, case)


def test_a_captured_graph_replays_the_bits_of_the_eager_run():
    """Forward + backward of the layer captured in a torch.cuda.graph: the replay gives the eager bits (no allocation-dependent state,
    no host synchronisation in the entries)."""
    import torch
    from consistent_depth_amd.ops.conv_layer import HipConv2d
    torch.manual_seed(3)
    layer = HipConv2d(3, 64, 7, 2, 3, bias=True).cuda()
    x = torch.randn(2, 3, 34, 66, device="cuda")
    dy = torch.randn(2, 64, 17, 33, device="cuda")

    def run():
        layer.weight.grad = layer.bias.grad = None
        y = layer(x)
        torch.autograd.backward(y, dy)
        return y, layer.weight.grad, layer.bias.grad

    # Everything on ONE side stream, the eager run included: autograd's AccumulateGrad nodes remember the stream they were created
    # under, and a backward captured on another stream than theirs would wait on the default stream inside the capture (which the
    # runtime does not survive).  Otherwise as engine.GraphedFineTuneStep captures: errors of other threads kept out.
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        eager = [t.clone() for t in run()]
        side.synchronize()
        layer.weight.grad = layer.bias.grad = None
        with torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):
            outs = run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for t in outs:
        t.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    for name, e, r in zip(("y", "dw", "db"), eager, outs):
        assert torch.equal(e, r), name
