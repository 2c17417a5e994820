"""The stride-1 grouped convolution on the GPU, through the ops.conv wrappers: cd_conv2d_fwd_grouped (forward, and the input gradient on
the transposed packs) and cd_conv2d_wgrad_grouped -- all groups in one launch of the split-bf16 kernels (csrc/conv_split.hip,
csrc/wgrad_split.hip with a group grid dimension), or group by group on the dense kernels (fewer than 8 input channels per group, 1x1,
arithmetic mode 0).  Every test runs under the three arithmetic modes.

Two yardsticks:
  * fp64: torch.nn.functional.conv2d(groups=G) and its autograd in fp64 on the CPU; each of y, dx, dw, db must be within
    max(4 x the distance of ATen's own fp32 convolution (on the device, MIOpen off: no kernel is compiled for these shapes) from the same
    fp64 result, 2e-6) in max-abs over max-abs -- the rule of tests/test_midas_gpu.py::test_hip_conv_layer_matches_fp64;
  * the dense entry points: group g alone by conv2d / conv2d_wgrad on the channel slices is BITWISE the grouped result.  The
    accumulation order of the split kernels depends on (Cin, k, Cout <= 16) only, the weight gradient's packed layout and split count on
    (cout_g, cin_g, k, N, H, W) only, and the fallback calls the dense entry itself: a mis-addressed group cannot hide behind a tolerance.
Shapes: both sides of the launch-shape rule N*H*W <= 43008 (and the value itself), odd extents (the scalar staging path) and widths
that are a multiple of 4 (the vector path), every channels-per-group class of the launch dispatch, channel counts that are no multiple
of the 8-channel chunk.  Outputs are pre-filled with NaN and followed by a guard region that must stay untouched."""
import pytest

from tests.gpu_util import report

pytestmark = [pytest.mark.gpu]

GUARD = 256
FLOOR = 2e-6


@pytest.fixture(autouse=True, params=["split", "split3", "fp32"])
def arith(request):
    """Arithmetic modes 2, 1 and 0 (cd_set_conv_arith), the previous one restored afterwards."""
    from consistent_depth_amd import _native
    lib = _native.lib()
    before = lib.cd_get_conv_arith()
    assert lib.cd_set_conv_arith({"fp32": 0, "split3": 1, "split": 2}[request.param]) == 0
    yield request.param
    lib.cd_set_conv_arith(before)


@pytest.fixture(autouse=True, scope="module")
def _drop_references():
    yield
    _REFS.clear()


# (cin_g, cout_g, groups): the classes of launch_conv_split's dispatch (cout_g <= 16: 16 channels x 2 rows per column tile; 32: one
# column tile; > 32: two), their transposes for the input gradient, and channel counts that straddle the 8-channel chunk.  Three groups
# where a group is 8 or 16 channels wide: a power-of-two assumption shows.
CLASSES = [(8, 8, 3), (16, 16, 3), (32, 32, 2), (64, 64, 2), (8, 24, 3), (24, 8, 3), (12, 12, 3), (16, 40, 3)]
SMALL_HW = [(2, 13, 7), (2, 17, 33), (2, 12, 16)]     # (N, H, W): one tile / several tiles, odd; a width the vector staging takes
LARGE_HW = (1, 209, 207)                              # 43263 pixels: just above the rule's 8 * 96 * 56 = 43008
EDGE_HW = (1, 192, 224)                               # exactly 43008: still the small side
# (cin_g, cout_g, groups, ks, N, H, W)
MAIN = ([c + (3,) + hw for c in CLASSES for hw in SMALL_HW] + [c + (3,) + LARGE_HW for c in CLASSES] + [(16, 40, 2, 3) + EDGE_HW])
# the group-by-group path in every mode: fewer than 8 input channels per group, and 1x1
FALLBACK = [c + hw for c in [(4, 4, 5, 3), (4, 12, 5, 3), (16, 16, 4, 1)] for hw in SMALL_HW[:2]]
OTHER_K = [(16, 16, 2, 5, 2, 17, 33), (16, 16, 2, 7, 2, 17, 33), (16, 16, 2, 11, 2, 17, 33), (8, 8, 2, 11, 2, 13, 7)]
ALL = MAIN + FALLBACK + OTHER_K
_id = lambda c: "x".join(map(str, c))  # noqa: E731


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


def _group_packs(w, G, transposed):
    from consistent_depth_amd.ops import conv as C
    cout_g = w.shape[0] // G
    return [C.pack_weights(w[g * cout_g:(g + 1) * cout_g].contiguous(), transposed) for g in range(G)]


def _side_by_side(parts):
    """The packed filters of all groups side by side (equal, 64-float aligned parts; the padding between them is zero)."""
    import torch
    n = (parts[0].numel() + 63) // 64 * 64
    arena = torch.zeros(len(parts) * n, dtype=torch.float32, device=parts[0].device)
    for g, p in enumerate(parts):
        arena[g * n:g * n + p.numel()] = p
    return arena


def _workspace(cin_g, cout_g, ks, G):
    import torch
    from consistent_depth_amd.ops import conv as C
    n = (C.wgrad_workspace_floats(cout_g, cin_g, ks) + 63) // 64 * 64
    return torch.empty(G * n, dtype=torch.float32, device="cuda")


def _rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)


def _inputs(case, bias=True):
    """x with a non-zero mean, filters of unit output variance, a random dy -- seeded by the case, generated on the host."""
    import torch
    cin_g, cout_g, G, ks, N, H, W = case
    g = torch.Generator().manual_seed(1000003 * cin_g + 10007 * cout_g + 101 * G + 13 * ks + 7 * H + W)
    r = lambda *s: torch.randn(s, dtype=torch.float32, generator=g)  # noqa: E731
    x = torch.relu(r(N, G * cin_g, H, W) + 0.5)
    w = r(G * cout_g, cin_g, ks, ks) / float(cin_g * ks * ks) ** 0.5
    b = r(G * cout_g) if bias else None
    dy = r(N, G * cout_g, H, W)
    return tuple(t.cuda() if t is not None else None for t in (x, w, b, dy))


def _references(x, w, b, dy, G, prev_y=None, prev_dx=None, prev_dw=None):
    """(y, dx, dw, db) in fp64 (CPU, returned on the device) and the distances of ATen's fp32 evaluation (device, MIOpen off) from it.
    prev_*: the previous content of an accumulated output, added to both."""
    import torch
    import torch.nn.functional as F
    pad = (w.shape[-1] - 1) // 2

    def run(dt, dev):
        xx, ww = x.to(dev, dt).requires_grad_(True), w.to(dev, dt).requires_grad_(True)
        bb = b.to(dev, dt).requires_grad_(True) if b is not None else None
        y = F.conv2d(xx, ww, bb, 1, pad, 1, G)
        y.backward(dy.to(dev, dt))
        out = {"y": y.detach(), "dx": xx.grad, "dw": ww.grad}
        if bb is not None:
            out["db"] = bb.grad
        for name, prev in (("y", prev_y), ("dx", prev_dx), ("dw", prev_dw)):
            if prev is not None:
                out[name] = out[name] + prev.to(dev, dt)
        return out

    r64 = {k: v.cuda() for k, v in run(torch.float64, "cpu").items()}
    with torch.backends.cudnn.flags(enabled=False):
        r32 = run(torch.float32, "cuda")
    return r64, {k: _rel(r32[k], r64[k]) for k in r64}


_REFS = {}


def _case_data(case):
    """Inputs and references of a case, computed once and shared by the arithmetic modes and the tests (never modified)."""
    if case not in _REFS:
        x, w, b, dy = _inputs(case)
        _REFS[case] = (x, w, b, dy) + _references(x, w, b, dy, case[2])
    return _REFS[case]


def _grouped_passes(case, x, w, b, dy, prev=None):
    """y, dx, dw (and db) by the grouped entries; outputs NaN-prefilled (or `prev` = (y, dx, dw) for accumulate) with guards."""
    import torch
    from consistent_depth_amd.ops import conv as C
    from consistent_depth_amd.ops.layers import channel_sum
    cin_g, cout_g, G, ks = case[:4]
    pk, pkT = _side_by_side(_group_packs(w, G, False)), _side_by_side(_group_packs(w, G, True))
    ybuf, y = _guarded(tuple(dy.shape))
    dxbuf, dx = _guarded(tuple(x.shape))
    dwbuf, dw = _guarded(tuple(w.shape))
    if prev is not None:
        y.copy_(prev[0]), dx.copy_(prev[1]), dw.copy_(prev[2])
    acc = prev is not None
    C.conv2d_grouped(x, pk, cin_g, cout_g, ks, G, bias=b, out=y, accumulate=acc)
    C.conv2d_grouped(dy, pkT, cout_g, cin_g, ks, G, out=dx, accumulate=acc)      # the input gradient, as HipConv2d issues it
    C.conv2d_wgrad_grouped(x, dy, cin_g, cout_g, ks, dw, _workspace(cin_g, cout_g, ks, G), G, accumulate=acc)
    out = {"y": y, "dx": dx, "dw": dw}
    if b is not None:
        out["db"] = torch.empty_like(b)
        channel_sum(dy, 0, dy.shape[1], out["db"])
    torch.cuda.synchronize()
    assert _guard_ok(ybuf) and _guard_ok(dxbuf) and _guard_ok(dwbuf), "a guard region was written"
    for name, t in out.items():
        assert not bool(torch.isnan(t).any()), f"{name}: elements left unwritten"
    return out


def _dense_passes(case, x, w, b, dy):
    """The same results group by group on the DENSE entry points (conv2d / conv2d_wgrad on channel slices of the same buffers)."""
    import torch
    from consistent_depth_amd.ops import conv as C
    cin_g, cout_g, G, ks = case[:4]
    pks, pkTs = _group_packs(w, G, False), _group_packs(w, G, True)
    ybuf, y = _guarded(tuple(dy.shape))
    dxbuf, dx = _guarded(tuple(x.shape))
    dwbuf, dw = _guarded(tuple(w.shape))
    ws = _workspace(cin_g, cout_g, ks, 1)
    for g in range(G):
        C.conv2d(x, pks[g], cin_g, cout_g, ks, bias=b[g * cout_g:(g + 1) * cout_g] if b is not None else None, x_coff=g * cin_g, out=y,
                 y_coff=g * cout_g)
        C.conv2d(dy, pkTs[g], cout_g, cin_g, ks, x_coff=g * cout_g, out=dx, y_coff=g * cin_g)
        C.conv2d_wgrad(x, dy, cin_g, cout_g, ks, dw[g * cout_g:(g + 1) * cout_g], ws, x_coff=g * cin_g, dy_coff=g * cout_g)
    torch.cuda.synchronize()
    assert _guard_ok(ybuf) and _guard_ok(dxbuf) and _guard_ok(dwbuf), "a guard region was written"
    return {"y": y, "dx": dx, "dw": dw}


def _held_to_the_yardstick(test, case, got, r64, ref, arith):
    dist = {k: _rel(v, r64[k]) for k, v in got.items()}
    report(test, case=_id(case), arith=arith, **{k: f"{v:.2e}" for k, v in dist.items()}, **{"ref_" + k: f"{ref[k]:.2e}" for k in dist})
    bad = {k: (v, ref[k]) for k, v in dist.items() if not v <= max(4 * ref[k], FLOOR)}
    assert not bad, bad


@pytest.mark.parametrize("case", ALL, ids=_id)
def test_every_pass_matches_fp64(case, arith):
    """(a), (c), (d): forward with bias, input gradient, weight gradient and bias gradient against fp64."""
    x, w, b, dy, r64, ref = _case_data(case)
    _held_to_the_yardstick("conv_grouped", case, _grouped_passes(case, x, w, b, dy), r64, ref, arith)


@pytest.mark.parametrize("case", ALL, ids=_id)
def test_grouped_equals_dense_bit_for_bit(case, arith):
    """(b): every pass of every case is bitwise the dense entry points' result on the channel slices, in every arithmetic mode."""
    import torch
    x, w, b, dy = _inputs(case)
    grouped, dense = _grouped_passes(case, x, w, b, dy), _dense_passes(case, x, w, b, dy)
    G = case[2]
    for name in ("y", "dx", "dw"):
        a, d = grouped[name], dense[name]
        if torch.equal(a, d):
            continue
        per = a.shape[0] // G if name == "dw" else a.shape[1] // G
        groups = [g for g in range(G) if not torch.equal(a.narrow(0 if name == "dw" else 1, g * per, per), d.narrow(0 if name == "dw" else 1, g * per, per))]
        raise AssertionError(f"{name}: groups {groups} differ from the dense kernels, max |diff| {float((a - d).abs().max()):.3e}")


SLICES = [(12, 12, 3, 3, 2, 13, 7), (8, 24, 3, 3, 2, 17, 33), (32, 32, 2, 3, 2, 12, 16), (64, 64, 2, 3, 2, 13, 7), (4, 12, 5, 3, 2, 13, 7),
          (8, 8, 3, 3) + LARGE_HW]


def _wide(t, below, above, fill):
    """t (N, C, H, W) as the channel slice [below, below + C) of a wider buffer whose other channels hold `fill` (a tensor or a number)."""
    import torch
    N, Cc, H, W = t.shape
    wide = torch.empty(N, below + Cc + above, H, W, dtype=torch.float32, device=t.device)
    if isinstance(fill, torch.Tensor):
        wide.copy_(fill)
    else:
        wide.fill_(fill)
    wide[:, below:below + Cc] = t
    return wide


def _outside_untouched(wide, before, lo, n):
    import torch
    return torch.equal(wide[:, :lo], before[:, :lo]) and torch.equal(wide[:, lo + n:], before[:, lo + n:])


@pytest.mark.parametrize("case", SLICES, ids=_id)
def test_a_channel_slice_leaves_the_other_channels_untouched(case, arith):
    """(e): operands and results are channel slices of wider buffers (x_ctot, y_ctot, dy_ctot > groups * channels per group, non-zero
    offsets).  The results are those of the tight buffers bit for bit (hence within the fp64 bound, checked too), and every channel
    outside the written slice keeps its previous bits."""
    import torch
    from consistent_depth_amd.ops import conv as C
    cin_g, cout_g, G, ks, N, H, W = case
    x, w, b, dy = _inputs(case)
    tight = _grouped_passes(case, x, w, b, dy)
    pk, pkT = _side_by_side(_group_packs(w, G, False)), _side_by_side(_group_packs(w, G, True))
    gen = torch.Generator(device="cuda").manual_seed(11)
    xw, dyw = _wide(x, 3, 2, 7.5), _wide(dy, 5, 3, -3.25)
    ybuf, yw = _guarded((N, 5 + G * cout_g + 3, H, W))
    dxbuf, dxw = _guarded((N, 3 + G * cin_g + 2, H, W))
    yw.copy_(torch.randn(yw.shape, device="cuda", generator=gen)), dxw.copy_(torch.randn(dxw.shape, device="cuda", generator=gen))
    y0, dx0 = yw.clone(), dxw.clone()
    dwbuf, dw = _guarded(tuple(w.shape))
    C.conv2d_grouped(xw, pk, cin_g, cout_g, ks, G, bias=b, x_coff=3, out=yw, y_coff=5)
    C.conv2d_grouped(dyw, pkT, cout_g, cin_g, ks, G, x_coff=5, out=dxw, y_coff=3)
    C.conv2d_wgrad_grouped(xw, dyw, cin_g, cout_g, ks, dw, _workspace(cin_g, cout_g, ks, G), G, x_coff=3, dy_coff=5)
    torch.cuda.synchronize()
    assert _guard_ok(ybuf) and _guard_ok(dxbuf) and _guard_ok(dwbuf), "a guard region was written"
    assert _outside_untouched(yw, y0, 5, G * cout_g), "y: channels outside the slice were written"
    assert _outside_untouched(dxw, dx0, 3, G * cin_g), "dx: channels outside the slice were written"
    got = {"y": yw[:, 5:5 + G * cout_g], "dx": dxw[:, 3:3 + G * cin_g], "dw": dw}
    for name, t in got.items():
        assert torch.equal(t, tight[name]), f"{name}: the slice of the wide buffer differs from the tight buffers' result"
    r64, ref = _references(x, w, b, dy, G)
    _held_to_the_yardstick("conv_grouped_slice", case, got, r64, ref, arith)


@pytest.mark.parametrize("case", SLICES, ids=_id)
def test_accumulate_adds_to_the_previous_content(case, arith):
    """(e): accumulate = 1 gives previous content + result -- against the fp64 sum at the same bound, and bitwise prev + (the kernel's own
    non-accumulated result): the epilogues of conv_split.hip / conv_mfma.hip add the loaded old value ONCE to (sum + bias), and
    unpack_rows writes *d + v with v the finished fp32 sum of the slices."""
    import torch
    cin_g, cout_g, G, ks, N, H, W = case
    x, w, b, dy = _inputs(case)
    gen = torch.Generator(device="cuda").manual_seed(12)
    prev = tuple(torch.randn(t.shape, device="cuda", generator=gen) for t in (dy, x, w))
    plain = _grouped_passes(case, x, w, b, dy)
    got = _grouped_passes(case, x, w, b, dy, prev=prev)
    for name, p in zip(("y", "dx", "dw"), prev):
        assert torch.equal(got[name], p + plain[name]), f"{name}: not previous content + result"
    r64, ref = _references(x, w, b, dy, G, *prev)
    _held_to_the_yardstick("conv_grouped_accumulate", case, {k: got[k] for k in ("y", "dx", "dw")}, r64, ref, arith)


APART = [c + hw for c in [(12, 12, 3, 3), (24, 8, 3, 3), (8, 24, 3, 3), (8, 8, 3, 3)] for hw in [(2, 13, 7), (2, 12, 16)]]


@pytest.mark.parametrize("case", APART, ids=_id)
def test_groups_stay_apart(case, arith):
    """(f): where an 8-channel chunk of the split kernels straddles the next group (12, 24 channels per group) or the end of the slice,
    only the zero padding of the packed filter and the staging mask keep foreign channels out.  NaN in every channel a call must not
    read (below and above the slice, in x and in dy) changes no bit of any result; NaN in ONE group's input channels turns exactly that
    group's outputs into NaN and leaves every other group's bits alone.  All addresses are inside the tensors allocated here."""
    import torch
    from consistent_depth_amd.ops import conv as C
    cin_g, cout_g, G, ks, N, H, W = case
    x, w, b, dy = _inputs(case)
    pk, pkT = _side_by_side(_group_packs(w, G, False)), _side_by_side(_group_packs(w, G, True))
    ws = _workspace(cin_g, cout_g, ks, G)
    XO, YO = 9, 5      # (odd offsets: the slices start inside an 8-channel chunk of the buffer)

    def run(xw, dyw):
        ybuf, y = _guarded(tuple(dy.shape))
        dxbuf, dx = _guarded(tuple(x.shape))
        dwbuf, dw = _guarded(tuple(w.shape))
        C.conv2d_grouped(xw, pk, cin_g, cout_g, ks, G, bias=b, x_coff=XO, out=y)
        C.conv2d_grouped(dyw, pkT, cout_g, cin_g, ks, G, x_coff=YO, out=dx)
        C.conv2d_wgrad_grouped(xw, dyw, cin_g, cout_g, ks, dw, ws, G, x_coff=XO, dy_coff=YO)
        torch.cuda.synchronize()
        assert _guard_ok(ybuf) and _guard_ok(dxbuf) and _guard_ok(dwbuf), "a guard region was written"
        return {"y": y, "dx": dx, "dw": dw}

    clean = run(_wide(x, XO, 11, 0.0), _wide(dy, YO, 13, 0.0))
    dirty = run(_wide(x, XO, 11, float("nan")), _wide(dy, YO, 13, float("nan")))
    for name in clean:
        assert bool(torch.isfinite(dirty[name]).all()), f"{name}: a channel outside the slice was read"
        assert torch.equal(clean[name], dirty[name]), f"{name}: depends on channels outside the slice"
    # NaN in group 1's own channels (x for y and dw, dy for dx and dw): that group's results and no others
    g = 1
    xn, dyn = x.clone(), dy.clone()
    xn[:, g * cin_g:(g + 1) * cin_g] = float("nan")
    dyn[:, g * cout_g:(g + 1) * cout_g] = float("nan")
    hit_x = run(_wide(xn, XO, 11, float("nan")), _wide(dy, YO, 13, float("nan")))
    hit_dy = run(_wide(x, XO, 11, float("nan")), _wide(dyn, YO, 13, float("nan")))
    for name, res, per, dim in (("y", hit_x["y"], cout_g, 1), ("dw", hit_x["dw"], cout_g, 0), ("dx", hit_dy["dx"], cin_g, 1),
                                ("dw", hit_dy["dw"], cout_g, 0)):
        for h in range(G):
            part, base = res.narrow(dim, h * per, per), clean[name].narrow(dim, h * per, per)
            if h == g:
                assert bool(torch.isnan(part).all()), f"{name}: group {g} did not read all of its own channels"
            else:
                assert torch.equal(part, base), f"{name}: group {h} read channels of group {g}"
    # (and the passes that do not read the poisoned operand are unchanged as a whole)
    assert torch.equal(hit_x["dx"], clean["dx"]) and torch.equal(hit_dy["y"], clean["y"])


@pytest.mark.parametrize("case", [(16, 40, 3, 3) + LARGE_HW, (12, 12, 3, 3, 2, 17, 33)], ids=_id)
def test_every_pass_is_bit_reproducible(case, arith):
    """(g): each pass twice on the same inputs gives the same bits (the weight gradient sums its slices in a fixed order)."""
    import torch
    x, w, b, dy = _inputs(case)
    first, second = _grouped_passes(case, x, w, b, dy), _grouped_passes(case, x, w, b, dy)
    for name in ("y", "dx", "dw"):
        assert torch.equal(first[name], second[name]), name


def test_refusals_leave_the_outputs_untouched(arith):
    """(h): slices beyond the buffer, a packed-filter stride below cd_conv2d_packed_weight_floats or no multiple of 4, a workspace stride
    below cd_conv2d_wgrad_workspace_floats and null pointers are CD_ERR_INVALID_ARG, k = 9 is CD_ERR_UNSUPPORTED; nothing is launched:
    the NaN pre-fill of every output is intact."""
    import torch
    from consistent_depth_amd import _native
    from consistent_depth_amd.ops import conv as C
    lib, stream = _native.lib(), _native.stream_ptr(torch.device("cuda"))
    case = (16, 24, 3, 3, 2, 13, 7)
    cin_g, cout_g, G, ks, N, H, W = case
    x, w, b, dy = _inputs(case)
    parts = _group_packs(w, G, False)
    pk = _side_by_side(parts)
    need = lib.cd_conv2d_packed_weight_floats(cout_g, cin_g, ks, 0)
    assert parts[0].numel() == need and need % 4 == 0
    wsf = C.wgrad_workspace_floats(cout_g, cin_g, ks)
    ws = _workspace(cin_g, cout_g, ks, G)
    ybuf, y = _guarded(tuple(dy.shape))
    dwbuf, dw = _guarded(tuple(w.shape))
    invalid, unsupported = "CD_ERR_INVALID_ARG", "CD_ERR_UNSUPPORTED"
    refused = [
        (invalid, lambda: C.conv2d_grouped(x, pk, cin_g, cout_g, ks, G, bias=b, x_coff=1, out=y)),                 # x_coff + G cin_g > x_ctot
        (invalid, lambda: C.conv2d_grouped(x, pk, cin_g, cout_g, ks, G, bias=b, out=y, y_coff=1)),
        (invalid, lambda: C.conv2d_grouped(x, pk, cin_g, cout_g, ks, G, bias=b, x_coff=-1, out=y)),
        (invalid, lambda: C.conv2d_grouped(x, pk[:G * (need - 4)], cin_g, cout_g, ks, G, out=y)),                  # stride < one packed filter
        (invalid, lambda: C.conv2d_grouped(x, torch.zeros(G * (need + 2), device="cuda"), cin_g, cout_g, ks, G, out=y)),   # stride % 4 != 0
        (invalid, lambda: C.conv2d_wgrad_grouped(x, dy, cin_g, cout_g, ks, dw, ws, G, x_coff=1)),
        (invalid, lambda: C.conv2d_wgrad_grouped(x, dy, cin_g, cout_g, ks, dw, ws, G, dy_coff=1)),
        (invalid, lambda: C.conv2d_wgrad_grouped(x, dy, cin_g, cout_g, ks, dw, ws[:G * (wsf - 1)], G)),             # stride < one workspace
        (unsupported, lambda: C.conv2d_grouped(x, pk, cin_g, cout_g, 9, G, out=y)),
        (unsupported, lambda: C.conv2d_wgrad_grouped(x, dy, cin_g, cout_g, 9, dw, ws, G)),
    ]
    for what, call in refused:
        with pytest.raises(RuntimeError, match=what):
            call()
    # null pointers: straight through the C ABI (the wrappers refuse None themselves)
    stride = pk.numel() // G
    fwd = [x.data_ptr(), G * cin_g, 0, cin_g, pk.data_ptr(), stride, b.data_ptr(), y.data_ptr(), G * cout_g, 0, cout_g, G, 0, N, H, W, ks, stream]
    for i in (0, 4, 7):
        args = list(fwd)
        args[i] = None
        assert lib.cd_conv2d_fwd_grouped(*args) == -1
    wg = [x.data_ptr(), G * cin_g, 0, cin_g, dy.data_ptr(), G * cout_g, 0, cout_g, G, dw.data_ptr(), 0, ws.data_ptr(), ws.numel() // G, N, H, W, ks, stream]
    for i in (0, 4, 9, 11):
        args = list(wg)
        args[i] = None
        assert lib.cd_conv2d_wgrad_grouped(*args) == -1
    torch.cuda.synchronize()
    for buf in (ybuf, dwbuf):
        assert bool(torch.isnan(buf[:-GUARD]).all()) and _guard_ok(buf)
