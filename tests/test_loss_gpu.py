"""GPU parity of the fused HIP loss (through the C ABI) against
  (1) golden vectors produced by the reference itself (tests/golden),
  (2) the CPU oracle on seeded inputs at BASELINE sizes (B=4, 384x224),
  (3) size-independent properties (pair-swap symmetry, lambda linearity, autograd scaling).

Tolerances (fp32 kernel vs the fp64 reference): loss values 1e-6 relative; depth gradient within 4x of the
distance the REFERENCE's own fp32 arithmetic has to its fp64 self on the same inputs (torch fp32 for the goldens,
the fp32 build of the oracle elsewhere; floor 2e-6).  Every test prints its measured distances (`PARITY ...`,
also appended to gpurun_out/parity_log.txt; a run is committed as profiles/parity_loss_r02.txt): the kernels sit
at 0.7-1.4x the reference's fp32 distance on every case, the `stress` golden included.
"""
import numpy as np
import pytest

from conftest import golden_loss_cases, load_loss_case
from gpu_util import Opt, metadata_of, report, to_dev

pytestmark = pytest.mark.gpu

LOSS_RTOL = 1e-6
GRAD_X_REF = 4.0     # allowed multiple of the reference's own fp32-vs-fp64 gradient distance
GRAD_FLOOR = 2e-6


def grad_tol(ref_fp32_dist):
    return max(GRAD_X_REF * ref_fp32_dist, GRAD_FLOOR)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def _run(torch, batch, lr, lb, mode=0, mask_sums=None):
    from consistent_depth_amd.loss import consistency_loss as CL
    d = to_dev(batch, torch)
    depth = d["depth"].clone().requires_grad_(True)
    total, reproj, disp = CL.consistency_loss(depth, d["flows"], d["masks"], d["intrinsics"], d["extrinsics"],
                                              lr, lb, mask_sums=mask_sums, depth_mode=mode)
    if total.requires_grad:
        total.backward()
    g = depth.grad.cpu().numpy() if depth.grad is not None else np.zeros_like(batch["depth"])
    return total.item(), reproj.cpu().numpy(), disp.cpu().numpy(), g


@pytest.fixture(params=[4, 3], ids=["sweep", "slab"])
def variant(request):
    """Every formulation of the gradient kernel: v4 row sweep (one workgroup per pair; the default for large batches),
    v3 evaluate-once + slab reduce (the default for small batches).  (Round 1's v2 "owner-computes" kernel was removed in
    round 4: never the dispatch choice, its exact fallback role is v1's.)"""
    from consistent_depth_amd import _native
    lib = _native.lib()
    assert lib.cd_debug_set_loss_variant(request.param) == 0
    yield request.param
    lib.cd_debug_set_loss_variant(0)


@pytest.mark.parametrize("name", golden_loss_cases())
def test_golden_vectors(torch_cuda, oracle, name, variant):
    batch, lr, lb, ref64, ref32 = load_loss_case(name)
    total, reproj, disp, grad = _run(torch_cuda, batch, lr, lb)
    report(f"golden[{name},v{variant}]", loss_rel=abs(total - ref64["total"][0]) / abs(ref64["total"][0]),
           grad_rel_l1=oracle.rel_l1(grad, ref64["grad_depth"]),
           ref_fp32_grad_rel_l1=oracle.rel_l1(ref32["grad_depth"], ref64["grad_depth"]),
           ref_fp32_loss_rel=abs(float(ref32["total"][0]) - ref64["total"][0]) / abs(ref64["total"][0]))
    np.testing.assert_allclose(total, ref64["total"][0], rtol=LOSS_RTOL)
    np.testing.assert_allclose(reproj, ref64["reprojection"], rtol=LOSS_RTOL, atol=1e-7)
    np.testing.assert_allclose(disp, ref64["disparity"], rtol=LOSS_RTOL, atol=1e-7)
    assert oracle.rel_l1(grad, ref64["grad_depth"]) < grad_tol(oracle.rel_l1(ref32["grad_depth"], ref64["grad_depth"]))


@pytest.mark.parametrize("gen", ["scene", "unrelated"])
@pytest.mark.parametrize("H,W", [(384, 224), (224, 384)])
def test_baseline_size_vs_oracle(torch_cuda, oracle, H, W, gen, variant):
    """BASELINE size (B=4, 384x224 and its transpose) on consistent-scene data (what real video looks
    like: the tile windows cover every source) and on the adversarial generator (unrelated
    depth per frame: a few % of the scatter goes through the overflow list)."""
    from consistent_depth_amd import synthetic
    batch = (synthetic.make_scene_batch if gen == "scene" else synthetic.make_pair_batch)(4, H, W, seed=11)
    ref = oracle.consistency_loss(batch["depth"], batch["flows"], batch["masks"], batch["intrinsics"],
                                  batch["extrinsics"], 1.0, 0.1, dtype=np.float64)
    total, reproj, disp, grad = _run(torch_cuda, batch, 1.0, 0.1)
    r32 = oracle.consistency_loss(batch["depth"], batch["flows"], batch["masks"], batch["intrinsics"],
                                  batch["extrinsics"], 1.0, 0.1, dtype=np.float32)
    report(f"baseline_size[{gen},{H}x{W},v{variant}]", loss_rel=abs(total - ref["total"][0]) / abs(ref["total"][0]),
           grad_rel_l1=oracle.rel_l1(grad, ref["grad_depth"]),
           ref_fp32_grad_rel_l1=oracle.rel_l1(r32["grad_depth"], ref["grad_depth"]),
           ref_fp32_loss_rel=abs(float(r32["total"][0]) - ref["total"][0]) / abs(ref["total"][0]))
    np.testing.assert_allclose(total, ref["total"][0], rtol=LOSS_RTOL)
    np.testing.assert_allclose(reproj, ref["reprojection"], rtol=LOSS_RTOL)
    np.testing.assert_allclose(disp, ref["disparity"], rtol=LOSS_RTOL)
    assert oracle.rel_l1(grad, ref["grad_depth"]) < grad_tol(oracle.rel_l1(r32["grad_depth"], ref["grad_depth"]))


@pytest.mark.parametrize("mode", [1, 2])
def test_fused_depth_heads(torch_cuda, oracle, mode, variant):
    """depth = exp(x) (mc) / 1/x (midas) fused into the kernel, gradient w.r.t. x."""
    from consistent_depth_amd import synthetic
    batch = synthetic.make_pair_batch(2, 64, 96, seed=5)
    depth = batch["depth"].astype(np.float64)
    x = np.log(depth) if mode == 1 else 1.0 / depth
    jac = depth if mode == 1 else -depth * depth
    ref = oracle.consistency_loss(depth, batch["flows"], batch["masks"], batch["intrinsics"], batch["extrinsics"],
                                  1.0, 0.1, dtype=np.float64)
    b2 = dict(batch, depth=x.astype(np.float32))
    total, reproj, disp, grad = _run(torch_cuda, b2, 1.0, 0.1, mode=mode)
    report(f"fused_head[mode{mode},v{variant}]", loss_rel=abs(total - ref["total"][0]) / abs(ref["total"][0]),
           grad_rel_l1=oracle.rel_l1(grad, ref["grad_depth"] * jac))
    np.testing.assert_allclose(total, ref["total"][0], rtol=LOSS_RTOL)
    assert oracle.rel_l1(grad, ref["grad_depth"] * jac) < 1e-5


def test_forward_only_and_cached_mask_sums(torch_cuda):
    torch = torch_cuda
    from consistent_depth_amd import synthetic
    from consistent_depth_amd.loss import consistency_loss as CL
    d = to_dev(synthetic.make_pair_batch(3, 48, 64, seed=2), torch)
    msum = CL.mask_sums(d["masks"][0], d["masks"][1])
    np.testing.assert_array_equal(msum.cpu().numpy()[:, 0], d["masks"][0].sum((1, 2, 3)).cpu().numpy())
    depth = d["depth"].clone().requires_grad_(True)
    a = CL.consistency_loss(depth, d["flows"], d["masks"], d["intrinsics"], d["extrinsics"], 1.0, 0.1)
    with torch.no_grad():
        b = CL.consistency_loss(depth, d["flows"], d["masks"], d["intrinsics"], d["extrinsics"], 1.0, 0.1)
    c = CL.consistency_loss(depth, d["flows"], d["masks"], d["intrinsics"], d["extrinsics"], 1.0, 0.1, mask_sums=msum)
    # forward-only and forward+backward are different template instantiations (different FMA
    # contraction), so they agree to fp32 rounding, not bitwise; cached sums are bit-identical
    for u, v in zip(a, b):
        torch.testing.assert_close(u.detach(), v.detach(), rtol=2e-6, atol=0)
    for u, v in zip(a, c):
        assert torch.equal(u.detach(), v.detach())
    assert not b[0].requires_grad and a[0].requires_grad


@pytest.mark.parametrize("cap", [0, 7, 1000])
@pytest.mark.parametrize("name", ["stress_b2_32x48", "basic_b3_48x40"])
def test_overflow_list_and_device_fallback(torch_cuda, oracle, name, cap, variant):
    """The gradient kernels are exact for ANY flow: taps outside the staged windows go
    through the overflow list (cap large), and when the list itself overflows (cap tiny) the
    device-side fallback recomputes the gradient.  Forced here with the debug capacity hook."""
    from consistent_depth_amd import _native
    batch, lr, lb, ref64, ref32 = load_loss_case(name)
    lib = _native.lib()
    try:
        assert lib.cd_debug_set_overflow_capacity(cap) == 0
        total, reproj, disp, grad = _run(torch_cuda, batch, lr, lb)
    finally:
        lib.cd_debug_set_overflow_capacity(-1)
    report(f"overflow[{name},cap{cap},v{variant}]", loss_rel=abs(total - ref64["total"][0]) / abs(ref64["total"][0]),
           grad_rel_l1=oracle.rel_l1(grad, ref64["grad_depth"]))
    np.testing.assert_allclose(total, ref64["total"][0], rtol=LOSS_RTOL)
    assert oracle.rel_l1(grad, ref64["grad_depth"]) < grad_tol(oracle.rel_l1(ref32["grad_depth"], ref64["grad_depth"]))


def test_wild_flow_full_size_vs_oracle(torch_cuda, oracle, variant):
    """Flows with +-40 px noise and strong in-tile variation: windows get capped, most scatter goes
    through the overflow list (or the fallback) -- still the reference's numbers."""
    from consistent_depth_amd import synthetic
    batch = synthetic.make_pair_batch(2, 384, 224, seed=21, noise_px=40.0)
    ref = oracle.consistency_loss(batch["depth"], batch["flows"], batch["masks"], batch["intrinsics"],
                                  batch["extrinsics"], 1.0, 0.1, dtype=np.float64)
    total, reproj, disp, grad = _run(torch_cuda, batch, 1.0, 0.1)
    r32 = oracle.consistency_loss(batch["depth"], batch["flows"], batch["masks"], batch["intrinsics"],
                                  batch["extrinsics"], 1.0, 0.1, dtype=np.float32)
    report(f"wild_flow[v{variant}]", loss_rel=abs(total - ref["total"][0]) / abs(ref["total"][0]),
           grad_rel_l1=oracle.rel_l1(grad, ref["grad_depth"]),
           ref_fp32_grad_rel_l1=oracle.rel_l1(r32["grad_depth"], ref["grad_depth"]))
    np.testing.assert_allclose(total, ref["total"][0], rtol=LOSS_RTOL)
    assert oracle.rel_l1(grad, ref["grad_depth"]) < grad_tol(oracle.rel_l1(r32["grad_depth"], ref["grad_depth"]))


@pytest.mark.parametrize("pxt", [1, 4])
@pytest.mark.parametrize("name", ["basic_b3_48x40", "stress_b2_32x48"])
def test_sweep_pixels_per_thread(torch_cuda, oracle, name, pxt):
    """The row sweep with 1 and 4 columns per thread (2 is the default covered above): other rows per item, other plans."""
    from consistent_depth_amd import _native
    batch, lr, lb, ref64, ref32 = load_loss_case(name)
    lib = _native.lib()
    try:
        assert lib.cd_debug_set_loss_variant(4) == 0 and lib.cd_debug_set_loss_sweep(pxt) == 0
        total, reproj, disp, grad = _run(torch_cuda, batch, lr, lb)
    finally:
        lib.cd_debug_set_loss_sweep(0)
        lib.cd_debug_set_loss_variant(0)
    report(f"sweep_pxt[{name},pxt{pxt}]", loss_rel=abs(total - ref64["total"][0]) / abs(ref64["total"][0]),
           grad_rel_l1=oracle.rel_l1(grad, ref64["grad_depth"]))
    np.testing.assert_allclose(total, ref64["total"][0], rtol=LOSS_RTOL)
    assert oracle.rel_l1(grad, ref64["grad_depth"]) < grad_tol(oracle.rel_l1(ref32["grad_depth"], ref64["grad_depth"]))


def test_stale_plan_falls_back_to_the_exact_path(torch_cuda, oracle):
    """A cached record blob (PairStore keeps one per dataset) whose row-sweep plan was made for another geometry -- here: the
    pixels-per-thread debug hook changed after the blob was built -- must not poison the step with a NaN loss (round 2 did, the
    device-side NaN guard then skipped every step holding such a pair): the sweep raises the degenerate flag and the guarded v1
    pass recomputes loss and gradient exactly.  The record stride does not depend on the hook, so the tile kernels keep reading
    their windows from the same blob."""
    from consistent_depth_amd import _native
    from consistent_depth_amd.loss import consistency_loss as CL
    torch = torch_cuda
    batch, lr, lb, ref64, ref32 = load_loss_case("basic_b3_48x40")
    lib = _native.lib()
    d = to_dev(batch, torch)
    nbytes = lib.cd_tile_windows_bytes(3, 48, 40)
    blob = CL.tile_windows(d["flows"], d["masks"])          # plans for the default geometry (2 pixels per thread)
    try:
        for variant, pxt in ((4, 4), (4, 1), (3, 4)):
            assert lib.cd_debug_set_loss_variant(variant) == 0 and lib.cd_debug_set_loss_sweep(pxt) == 0
            assert lib.cd_tile_windows_bytes(3, 48, 40) == nbytes
            depth = d["depth"].clone().requires_grad_(True)
            total, _, _ = CL.consistency_loss(depth, d["flows"], d["masks"], d["intrinsics"], d["extrinsics"], lr, lb, tile_windows=blob)
            total.backward()
            np.testing.assert_allclose(total.item(), ref64["total"][0], rtol=LOSS_RTOL)
            assert oracle.rel_l1(depth.grad.cpu().numpy(), ref64["grad_depth"]) < grad_tol(oracle.rel_l1(ref32["grad_depth"], ref64["grad_depth"]))
        assert lib.cd_debug_set_loss_variant(2) != 0       # the removed owner-computes variant is refused, not silently remapped
    finally:
        lib.cd_debug_set_loss_sweep(0)
        lib.cd_debug_set_loss_variant(0)


def test_foreign_tile_windows_degrade_to_the_general_pass(torch_cuda, oracle):
    """A tile_windows blob that belongs to OTHER flows / masks of the same shape (a caller's cache gone stale): the row-sweep plan's
    promise "the taps of this row group's valid sources are resident" (Rec::inw, trusted by round 5's fast source pass without clamp or
    vote) does not hold for the flows of the call.  Round 6: the plan carries a fingerprint of the flows / masks it was made from, the
    sweep kernel recomputes it from the samples it reads anyway and, on a mismatch, believes no inw -- the general pass routes taps
    outside the rings through the overflow list: the gradient is the oracle's, as it was before the fast pass existed."""
    from consistent_depth_amd import _native, synthetic
    from consistent_depth_amd.loss import consistency_loss as CL
    torch = torch_cuda
    lib = _native.lib()
    H, W = 384, 224
    a = to_dev(synthetic.make_scene_batch(2, H, W, seed=3), torch)
    batch = synthetic.make_pair_batch(2, H, W, seed=8)          # unrelated depth per frame: flows with a wide vertical spread
    d = to_dev(batch, torch)
    foreign = CL.tile_windows(a["flows"], a["masks"])
    own = CL.tile_windows(d["flows"], d["masks"])
    ref = oracle.consistency_loss(batch["depth"], batch["flows"], batch["masks"], batch["intrinsics"], batch["extrinsics"], 1.0, 0.1, dtype=np.float64)
    r32 = oracle.consistency_loss(batch["depth"], batch["flows"], batch["masks"], batch["intrinsics"], batch["extrinsics"], 1.0, 0.1, dtype=np.float32)
    assert lib.cd_debug_set_loss_variant(4) == 0
    try:
        res = {}
        for name, blob in (("own", own), ("foreign", foreign)):
            depth = d["depth"].clone().requires_grad_(True)
            total, _, _ = CL.consistency_loss(depth, d["flows"], d["masks"], d["intrinsics"], d["extrinsics"], 1.0, 0.1, tile_windows=blob)
            total.backward()
            res[name] = (total.item(), oracle.rel_l1(depth.grad.cpu().numpy(), ref["grad_depth"]))
    finally:
        lib.cd_debug_set_loss_variant(0)
    report("foreign_tile_windows", own_grad_rel_l1=res["own"][1], foreign_grad_rel_l1=res["foreign"][1],
           ref_fp32_grad_rel_l1=oracle.rel_l1(r32["grad_depth"], ref["grad_depth"]))
    for name, (total, dist) in res.items():
        np.testing.assert_allclose(total, ref["total"][0], rtol=LOSS_RTOL)
        assert dist < grad_tol(oracle.rel_l1(r32["grad_depth"], ref["grad_depth"])), (name, dist)


@pytest.mark.parametrize("force", [0, 3], ids=["default_dispatch", "slab_chunked"])
def test_roofline_launch_vs_oracle(torch_cuda, oracle, force):
    """The launch bench.py's roofline number is taken on -- B = 256 pairs of 384x224 in ONE call (0.88 GB, beyond the
    Infinity Cache) -- against the fp64 oracle: the default dispatch (row sweep, one workgroup per pair) and the tile
    kernels' chunked path (2 x 128 pairs)."""
    from consistent_depth_amd import _native, synthetic
    base = synthetic.make_scene_batch(16, 384, 224, seed=31)
    rng = np.random.default_rng(0)
    B = 256
    batch = {"depth": np.concatenate([base["depth"] * np.exp(rng.normal(0, 0.01, base["depth"].shape)).astype(np.float32)
                                      for _ in range(B // 16)]),
             "flows": [np.tile(f, (B // 16, 1, 1, 1)) for f in base["flows"]],
             "masks": [np.tile(m, (B // 16, 1, 1, 1)) for m in base["masks"]],
             "intrinsics": np.tile(base["intrinsics"], (B // 16, 1, 1)),
             "extrinsics": np.tile(base["extrinsics"], (B // 16, 1, 1, 1))}
    ref = oracle.consistency_loss(batch["depth"], batch["flows"], batch["masks"], batch["intrinsics"], batch["extrinsics"],
                                  1.0, 0.1, dtype=np.float64)
    lib = _native.lib()
    try:
        assert lib.cd_debug_set_loss_variant(force) == 0
        total, reproj, disp, grad = _run(torch_cuda, batch, 1.0, 0.1)
    finally:
        lib.cd_debug_set_loss_variant(0)
    # the reference's own fp32 distance on this generator at this size: 8.9e-6 (baseline_size[scene] above)
    report(f"roofline_launch_b256[variant{force}]", loss_rel=abs(total - ref["total"][0]) / abs(ref["total"][0]),
           grad_rel_l1=oracle.rel_l1(grad, ref["grad_depth"]),
           worst_pair_grad_rel_l1=max(oracle.rel_l1(grad[b], ref["grad_depth"][b]) for b in range(B)))
    np.testing.assert_allclose(total, ref["total"][0], rtol=LOSS_RTOL)
    np.testing.assert_allclose(reproj, ref["reprojection"], rtol=2 * LOSS_RTOL)
    np.testing.assert_allclose(disp, ref["disparity"], rtol=2 * LOSS_RTOL)
    assert oracle.rel_l1(grad, ref["grad_depth"]) < 4e-5
    assert max(oracle.rel_l1(grad[b], ref["grad_depth"][b]) for b in range(B)) < 1e-4


def test_midas_scale_vs_oracle(torch_cuda, oracle, variant):
    """BASELINE configs[4] settings: lambda_view_baseline 1e-4, 384x384, B = 8, reciprocal head -- the gradient scale is
    ~1e-3 of the mc case; the accumulators count in O(1) units (sweep) / 2^-40 fixed point (tile kernels)."""
    from consistent_depth_amd import synthetic
    batch = synthetic.make_scene_batch(8, 384, 384, seed=17)
    depth = batch["depth"].astype(np.float64)
    args = (depth, batch["flows"], batch["masks"], batch["intrinsics"], batch["extrinsics"], 1.0, 1e-4)
    ref = oracle.consistency_loss(*args, dtype=np.float64)
    r32 = oracle.consistency_loss(*args, dtype=np.float32)
    b2 = dict(batch, depth=(1.0 / depth).astype(np.float32))
    total, reproj, disp, grad = _run(torch_cuda, b2, 1.0, 1e-4, mode=2)
    want = ref["grad_depth"] * (-depth * depth)
    report(f"midas_scale[v{variant}]", loss_rel=abs(total - ref["total"][0]) / abs(ref["total"][0]),
           grad_rel_l1=oracle.rel_l1(grad, want), ref_fp32_grad_rel_l1=oracle.rel_l1(r32["grad_depth"], ref["grad_depth"]))
    np.testing.assert_allclose(total, ref["total"][0], rtol=LOSS_RTOL)
    assert oracle.rel_l1(grad, want) < grad_tol(oracle.rel_l1(r32["grad_depth"], ref["grad_depth"]))


def test_sweep_degenerate_depth_takes_the_exact_path(torch_cuda, oracle):
    """A zero depth makes 1/zs infinite for whoever samples it -- also for masked-out sources (0 * inf = NaN in the
    reference).  The row sweep lets masked-out sources with far-away taps sample a resident row instead; it is exact
    because any depth that is not a positive finite number sends the whole call to the exact v1 kernels (gradient AND loss)."""
    from consistent_depth_amd import _native, synthetic
    lib = _native.lib()
    batch = synthetic.make_scene_batch(2, 96, 128, seed=4)
    batch["depth"][1, 1, 40:44, 60:64] = 0.0
    args = (batch["depth"], batch["flows"], batch["masks"], batch["intrinsics"], batch["extrinsics"], 1.0, 0.1)
    ref = oracle.consistency_loss(*args, dtype=np.float64)
    r32 = oracle.consistency_loss(*args, dtype=np.float32)
    try:
        assert lib.cd_debug_set_loss_variant(4) == 0
        total, reproj, disp, grad = _run(torch_cuda, batch, 1.0, 0.1)
    finally:
        lib.cd_debug_set_loss_variant(0)
    assert np.isfinite(ref["reprojection"][0]) and np.isfinite(reproj[0])
    np.testing.assert_allclose(reproj[0], ref["reprojection"][0], rtol=LOSS_RTOL)
    np.testing.assert_array_equal(np.isfinite(disp), np.isfinite(ref["disparity"]))
    np.testing.assert_array_equal(np.isfinite(grad), np.isfinite(ref["grad_depth"]))
    # sources that sample next to the zero block see 1/zs^2 blow up: ill-conditioned for ANY fp32 arithmetic, so the yardstick
    # is again the reference's own fp32 run (same finite / non-finite pattern required above)
    fin = np.isfinite(ref["grad_depth"]) & np.isfinite(r32["grad_depth"])
    ref_dist = oracle.rel_l1(r32["grad_depth"][fin], ref["grad_depth"][fin])
    report("degenerate_depth[sweep]", grad_rel_l1=oracle.rel_l1(grad[fin], ref["grad_depth"][fin]), ref_fp32_grad_rel_l1=ref_dist)
    assert oracle.rel_l1(grad[fin], ref["grad_depth"][fin]) < grad_tol(ref_dist)


def test_sweep_is_bit_reproducible(torch_cuda):
    """Integer LDS accumulation: two runs of the row sweep give the same bits (no overflow-list traffic on consistent scenes)."""
    from consistent_depth_amd import _native, synthetic
    lib = _native.lib()
    batch = synthetic.make_scene_batch(6, 384, 224, seed=8)
    try:
        assert lib.cd_debug_set_loss_variant(4) == 0
        a = _run(torch_cuda, batch, 1.0, 0.1, mode=1)
        b = _run(torch_cuda, batch, 1.0, 0.1, mode=1)
    finally:
        lib.cd_debug_set_loss_variant(0)
    assert a[0] == b[0]
    np.testing.assert_array_equal(a[3], b[3])


def test_cached_tile_windows_bitwise(torch_cuda):
    torch = torch_cuda
    from consistent_depth_amd import synthetic
    from consistent_depth_amd.loss import consistency_loss as CL
    d = to_dev(synthetic.make_pair_batch(3, 96, 80, seed=12), torch)
    tw = CL.tile_windows(d["flows"], d["masks"])
    outs = []
    for kw in ({}, {"tile_windows": tw}):
        x = d["depth"].clone().requires_grad_(True)
        t, _, _ = CL.consistency_loss(x, d["flows"], d["masks"], d["intrinsics"], d["extrinsics"], 1.0, 0.1, **kw)
        t.backward()
        outs.append((t.detach(), x.grad))
    assert torch.equal(outs[0][0], outs[1][0])
    # only LDS-atomic ordering inside a tile differs between two runs
    rel = (outs[0][1] - outs[1][1]).abs().sum() / outs[0][1].abs().sum()
    assert rel.item() < 1e-6


def test_module_surface_and_autograd_scaling(torch_cuda):
    """ConsistencyLoss(opt)(depths, metadata) like the reference; upstream grad scales the result."""
    torch = torch_cuda
    from consistent_depth_amd import synthetic
    from consistent_depth_amd.loss.consistency_loss import ConsistencyLoss
    from consistent_depth_amd.loss.joint_loss import JointLoss
    d = to_dev(synthetic.make_pair_batch(2, 32, 48, seed=3), torch)
    crit = ConsistencyLoss(Opt())
    x1 = d["depth"].clone().requires_grad_(True)
    loss, parts = crit(x1, metadata_of(d))
    assert loss.dim() == 0 and set(parts) == {"reprojection", "disparity"} and parts["disparity"].shape == (2,)
    loss.backward()
    x2 = d["depth"].clone().requires_grad_(True)
    jl, jparts = JointLoss(Opt())(x2, metadata_of(d))
    assert jl.shape == (1,) and set(jparts) == {"reprojection", "disparity"}
    (3.0 * jl).sum().backward()
    torch.testing.assert_close(x2.grad, 3.0 * x1.grad, rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(loss.item(), (parts["reprojection"] + parts["disparity"]).mean().item(), rtol=1e-6)


def test_pair_swap_symmetry_full_size(torch_cuda):
    """Swapping the two frames of every pair (and fwd/bwd flows+masks) leaves the loss unchanged
    and swaps the gradient planes -- a size-independent property, checked at 8 x 384 x 224."""
    torch = torch_cuda
    from consistent_depth_amd import synthetic
    from consistent_depth_amd.loss import consistency_loss as CL
    d = to_dev(synthetic.make_pair_batch(8, 384, 224, seed=4), torch)

    def run(depth, flows, masks, intr, extr):
        x = depth.clone().requires_grad_(True)
        t, r, q = CL.consistency_loss(x, flows, masks, intr, extr, 1.0, 0.1)
        t.backward()
        return t.detach(), r, q, x.grad

    t1, r1, q1, g1 = run(d["depth"], d["flows"], d["masks"], d["intrinsics"], d["extrinsics"])
    t2, r2, q2, g2 = run(d["depth"].flip(1).contiguous(), d["flows"][::-1], d["masks"][::-1],
                         d["intrinsics"].flip(1).contiguous(), d["extrinsics"].flip(1).contiguous())
    torch.testing.assert_close(t1, t2, rtol=1e-6, atol=0)
    torch.testing.assert_close(r1, r2, rtol=1e-6, atol=0)
    torch.testing.assert_close(q1, q2, rtol=1e-6, atol=0)
    rel = (g1 - g2.flip(1)).abs().sum() / g1.abs().sum()
    assert rel.item() < 1e-5  # only the atomic accumulation order differs


def test_lambda_linearity_full_size(torch_cuda):
    torch = torch_cuda
    from consistent_depth_amd import synthetic
    from consistent_depth_amd.loss import consistency_loss as CL
    d = to_dev(synthetic.make_pair_batch(4, 384, 224, seed=6), torch)

    def run(lr, lb):
        x = d["depth"].clone().requires_grad_(True)
        t, _, _ = CL.consistency_loss(x, d["flows"], d["masks"], d["intrinsics"], d["extrinsics"], lr, lb)
        t.backward()
        return t.detach(), x.grad

    t_r, g_r = run(1.0, 0.0)
    t_b, g_b = run(0.0, 1.0)
    t, g = run(0.7, 0.3)
    torch.testing.assert_close(t, 0.7 * t_r + 0.3 * t_b, rtol=2e-6, atol=0)
    rel = (g - (0.7 * g_r + 0.3 * g_b)).abs().sum() / g.abs().sum()
    assert rel.item() < 1e-5


def test_nan_propagates_like_reference(torch_cuda):
    """mask * NaN = NaN even where mask == 0 (the reference multiplies, never selects), so the
    NaN guard of depth_fine_tuning.py:278-280 fires identically."""
    torch = torch_cuda
    from consistent_depth_amd import synthetic
    from consistent_depth_amd.loss import consistency_loss as CL
    d = to_dev(synthetic.make_pair_batch(2, 32, 32, seed=8), torch)
    d["masks"][0][0, 0, 5, 5] = 0
    d["depth"][0, 0, 5, 5] = float("nan")
    t, r, q = CL.consistency_loss(d["depth"], d["flows"], d["masks"], d["intrinsics"], d["extrinsics"], 1.0, 0.1)
    assert torch.isnan(t) and torch.isnan(r[0]) and not torch.isnan(r[1])


def test_rejects_cpu_tensors(torch_cuda):
    import torch
    from consistent_depth_amd import synthetic
    from consistent_depth_amd.loss import consistency_loss as CL
    b = synthetic.make_pair_batch(1, 16, 16, seed=0)
    t = lambda a: torch.tensor(a)  # noqa: E731
    with pytest.raises(RuntimeError, match="HIP device"):
        CL.consistency_loss(t(b["depth"]), [t(f) for f in b["flows"]], [t(m) for m in b["masks"]],
                            t(b["intrinsics"]), t(b["extrinsics"]), 1.0, 0.1)


def test_chunked_launches_are_bit_identical(torch_cuda):
    """The evaluate-once kernel processes pairs in chunks (bounded slab scratch); pairs are independent and
    the order of summation inside a pair is fixed, so chunking must not change a single bit."""
    from consistent_depth_amd import _native, synthetic
    lib = _native.lib()
    batch = synthetic.make_scene_batch(7, 96, 128, seed=3)
    try:
        assert lib.cd_debug_set_loss_chunk(7) == 0
        one = _run(torch_cuda, batch, 1.0, 0.1)
        assert lib.cd_debug_set_loss_chunk(3) == 0          # chunks of 3, 3, 1
        three = _run(torch_cuda, batch, 1.0, 0.1)
    finally:
        lib.cd_debug_set_loss_chunk(0)
    assert one[0] == three[0]
    np.testing.assert_array_equal(one[1], three[1])
    np.testing.assert_array_equal(one[2], three[2])
    np.testing.assert_array_equal(one[3], three[3])


def _raw_fwd_bwd(torch, d, ws, lr=1.0, lb=0.1):
    """cd_consistency_loss_fwd_bwd on a caller-owned workspace (row sweep forced), straight through ctypes."""
    from consistent_depth_amd import _native
    lib = _native.lib()
    depth = d["depth"].contiguous()
    B, _, H, W = depth.shape
    out = torch.zeros(2 * B + 1, device=depth.device)
    grad = torch.empty_like(depth)
    rc = lib.cd_consistency_loss_fwd_bwd(depth.data_ptr(), d["flows"][0].data_ptr(), d["flows"][1].data_ptr(), d["masks"][0].data_ptr(),
                                         d["masks"][1].data_ptr(), None, None, d["intrinsics"].data_ptr(), d["extrinsics"].data_ptr(),
                                         lr, lb, 0, B, H, W, out[:B].data_ptr(), out[B:2 * B].data_ptr(), out[2 * B:].data_ptr(),
                                         grad.data_ptr(), ws.data_ptr(), ws.numel(), _native.stream_ptr(depth.device))
    assert rc == 0
    return out, grad


def test_sweep_workspace_header(torch_cuda, variant):
    """ABI 9: the row sweep keeps its finished-workgroup counter in the workspace header BETWEEN calls (the workgroup that finishes last
    puts it back to zero; no per-call reset dispatch).  (1) A workspace that was never initialised gives total = NaN, not a stale
    number; (2) after cd_consistency_loss_workspace_init the same buffer serves calls of DIFFERENT batch sizes back to back, `total` is
    the mean of the per-pair losses every time and the counter is zero after every call.  (The advisor's stress test of the fence-free
    hand-off of the per-pair losses: 60 launches.)"""
    torch = torch_cuda
    from consistent_depth_amd import _native, synthetic
    lib = _native.lib()
    H, W = 64, 96
    batches = {B: to_dev(synthetic.make_scene_batch(B, H, W, seed=20 + B), torch) for B in (7, 3, 12)}
    ws = torch.full((lib.cd_consistency_loss_workspace_bytes(12, H, W),), 0x5a, dtype=torch.uint8, device="cuda")
    if variant != 4:
        # the header is the row sweep's: the slab formulation neither needs nor touches it.  On a workspace that was never initialised
        # its total is the mean of the per-pair losses and the header's 256 bytes stay as they were; after
        # cd_consistency_loss_workspace_init the header keeps what the init wrote (counter 0) and every call of the same batch size is
        # bitwise the one on the uninitialised buffer.
        first = {}
        for B in (7, 3, 12):
            out, grad = _raw_fwd_bwd(torch, batches[B], ws)
            torch.cuda.synchronize()
            per_pair = (out[:B].double() + out[B:2 * B].double()).mean().item()
            assert abs(out[-1].item() - per_pair) <= 2e-7 * abs(per_pair), (B, out[-1].item(), per_pair)
            first[B] = (out.clone(), grad.clone())
        assert bool((ws[:256] == 0x5a).all()), ws[:8]
        assert lib.cd_consistency_loss_workspace_init(ws.data_ptr(), ws.numel(), _native.stream_ptr(ws.device)) == 0
        torch.cuda.synchronize()
        hdr = ws[:256].view(torch.int32)
        hdr0 = hdr.clone()
        assert int(hdr0[1]) == 0
        for it in range(12):
            B = (7, 3, 12)[it % 3]
            out, grad = _raw_fwd_bwd(torch, batches[B], ws)
            torch.cuda.synchronize()
            assert torch.equal(hdr, hdr0), (it, B, hdr[:2].tolist())
            assert torch.equal(first[B][0], out) and torch.equal(first[B][1], grad), (it, B)
        return
    out, _ = _raw_fwd_bwd(torch, batches[7], ws)
    torch.cuda.synchronize()
    assert torch.isnan(out[-1]), "an uninitialised workspace must not report a mean loss"
    assert lib.cd_consistency_loss_workspace_init(ws.data_ptr(), ws.numel(), _native.stream_ptr(ws.device)) == 0
    hdr = ws[:8].view(torch.int32)
    ref = {}
    for it in range(60):
        B = (7, 3, 12)[it % 3]
        out, grad = _raw_fwd_bwd(torch, batches[B], ws)
        torch.cuda.synchronize()
        assert int(hdr[1]) == 0, (it, B, int(hdr[1]))
        per_pair = (out[:B].double() + out[B:2 * B].double()).mean().item()
        assert abs(out[-1].item() - per_pair) <= 2e-7 * abs(per_pair), (it, B, out[-1].item(), per_pair)
        if B in ref:        # integer accumulation: every repeat is bitwise the first call
            assert torch.equal(ref[B][0], out) and torch.equal(ref[B][1], grad), (it, B)
        else:
            ref[B] = (out.clone(), grad.clone())
