"""CPU: the depth previews' fixed parts against the reference's own output (tests/golden/vis_reference.npz, vis_loop_6f_64x48.npz,
written by tools/gen_golden_visualization.py from the unmodified reference with a recording cv2 stub) -- the committed colour table,
the numpy restatement of the formula that the GPU tests use as their yardstick (tests/vis_util.py), the host-side percentile
interpolation, the live reference where it exists, and the surface of utils/visualization.py that needs no device."""
import os
import sys

import numpy as np
import pytest

from conftest import REPO

import vis_util as V

from oracle import ref_loop

needs_reference = pytest.mark.skipif(not ref_loop.available(), reason="reference checkout not present")


def _tool(name):
    sys.path.insert(0, os.path.join(REPO, "tools"))
    return __import__(name)


def test_committed_table_is_the_reference_table():
    from consistent_depth_amd.utils import visualization as vis
    g = V.golden()
    table = vis.color_table()
    assert table.shape == (256, 3) and table.dtype == np.uint8
    assert np.array_equal(table[:, ::-1], g["table_bgr"])            # the reference's arrays are B,G,R
    try:
        import matplotlib
    except ImportError:
        return
    magma = (np.asarray(matplotlib.colormaps["magma"].colors) * 255).astype(np.uint8)
    assert np.array_equal(table, vis.gamma_table(magma))
    # the closest an entry comes to a rounding tie: rint vs any other rounding of the writer cannot matter
    exact = ((magma / 255) ** 2.2) * 255
    assert np.abs(np.abs(exact - np.floor(exact)) - 0.5).min() > 5e-4


def test_generator_tool_reproduces_the_committed_table():
    from consistent_depth_amd.utils import visualization as vis
    gen = _tool("gen_magma_table")
    assert np.array_equal(gen.generate(), vis.color_table())
    assert np.array_equal(np.loadtxt(gen.TABLE, dtype=np.uint8), vis.color_table())


def test_numpy_restatement_matches_every_reference_plane():
    """tests/vis_util.py::preview_pixels is what the GPU tests compare the kernel with where the reference is absent."""
    g = V.golden()
    for name in g["vd_names"]:
        d, (lo, hi) = g[f"vd_{name}_in"], g[f"vd_{name}_range"]
        if bool(g[f"vd_{name}_auto"]):
            lo, hi = np.amin(d), np.amax(d)
        assert np.array_equal(V.preview_pixels(d, lo, hi, g["table_bgr"]), g[f"vd_{name}_out"]), name
    # the wrap table of the issue, as recorded on the x86 host
    idx = V.preview_indices(g["vd_wrap_in"], 0, 1).ravel()[:12]
    assert idx[0] == 0 and idx[1] == 0 and idx[2] == 0 and idx[3] == 0 and idx[6] == 24 and idx[7] == 254 and idx[8] == 64, idx


def test_directory_goldens_follow_the_range_rule():
    """0 / 100: the recorded pixels are the formula under min / max of the finite values over ALL files (the all-NaN frame takes no
    part and is still rendered, the stale file of another size joins)."""
    g = V.golden()
    planes = [g[f"dir_in_{k}"] for k in range(len(g["dir_names"]))]
    finite = [p[np.isfinite(p)] for p in planes]
    lo = min(f.min() for f in finite if f.size)
    hi = max(f.max() for f in finite if f.size)
    for k, p in enumerate(planes):
        assert np.array_equal(V.preview_pixels(p, lo, hi, g["table_bgr"]), g[f"dir_out_0_100_{k}"]), k
    hi99 = max(np.percentile(f, 99) for f in finite if f.size)
    assert hi99 < hi
    for k, p in enumerate(planes):
        assert np.array_equal(V.preview_pixels(p, lo, hi99, g["table_bgr"]), g[f"dir_out_0_99_{k}"]), k


def _percentile_inputs():
    rng = np.random.default_rng(5)
    out = []
    for n in (2, 3, 17, 384, 4801, 86016):
        out.append(rng.uniform(0.01, 4.0, n).astype(np.float32))
        out.append((rng.standard_normal(n) * 3).astype(np.float32))
        out.append(np.round(rng.uniform(0, 8, n)).astype(np.float32))                 # many duplicates
    return out


def test_host_interpolation_within_the_references_own_spread():
    """Percentiles other than 0 / 100: not bit equality.  U = the float32-ulp distance between np.percentile(v) and
    float32(np.percentile(v in float64)), the reference's own spread over these inputs; the product's value -- interpolated from
    the two order statistics the kernel selects -- must stay within max(1, U) ulp of np.percentile(v) and inside [a, b]."""
    from consistent_depth_amd.utils import visualization as vis
    worst_u, worst_mine = 0, 0
    for v in _percentile_inputs():
        s = np.sort(v)
        for q in (1, 5, 25, 50, 75, 95, 99, 99.9):
            want = np.percentile(v, q)
            assert want.dtype == np.float32
            u = V.ulp_distance(want, np.float32(np.percentile(v.astype(np.float64), q)))
            # what cd_depth_range selects: the neighbours of numpy's float32 virtual index
            last = np.float32(v.size - 1)
            vi = last * vis.quantile32(q)
            k = v.size - 1 if vi >= last else int(np.floor(vi))
            a, b = s[k], s[min(k + 1, v.size - 1)]
            got = vis.interpolate_percentile(v.size, a, b, q)
            assert got.dtype == np.float32 and a <= got <= b, (v.size, q, a, got, b)
            mine = V.ulp_distance(got, want)
            worst_u, worst_mine = max(worst_u, u), max(worst_mine, mine)
            assert mine <= max(1, u), (v.size, q, got, want, mine, u)
    print(f"percentile interpolation: reference's own spread U = {worst_u} ulp, product vs np.percentile = {worst_mine} ulp")
    v = _percentile_inputs()[4]
    s = np.sort(v)
    assert vis.interpolate_percentile(v.size, s[0], s[min(1, v.size - 1)], 0) == np.percentile(v, 0)
    assert vis.interpolate_percentile(v.size, s[-1], s[-1], 100) == np.percentile(v, 100)


def test_loop_golden_pins_the_two_ranges():
    """eval/: range [0, max of the FIRST validation batch of the first sweep], also for the sweep after the epoch; depth/: min / max
    over the directory.  Checked on the reference's recorded pixels and the `.raw` planes it rendered them from."""
    g, ref = V.golden("vis_loop_6f_64x48.npz"), V.golden()
    names = [str(n) for n in g["names"]]
    raws = {n: g[f"raw_{i}"] for i, n in enumerate(names)}
    first = [n for n in names if n.startswith("eval") and "_e0000_" in n and int(os.path.basename(n)[6:12]) in set(g["first_batch_frames"].tolist())]
    assert first
    scale = max(raws[n].max() for n in first)
    depth = [n for n in names if n.startswith("depth")]
    lo, hi = min(raws[n].min() for n in depth), max(raws[n].max() for n in depth)
    assert len(depth) == 6 and len(names) == 6 * (int(g["epochs"]) + 1) + 6
    for i, n in enumerate(names):
        want = V.preview_pixels(raws[n], lo, hi, ref["table_bgr"]) if n.startswith("depth") else V.preview_pixels(raws[n], 0, scale, ref["table_bgr"])
        assert np.array_equal(g[f"png_{i}"], want), n


def test_apply_mask_and_scope():
    from consistent_depth_amd.utils import visualization as vis
    rng = np.random.default_rng(0)
    im, mask = rng.uniform(0, 255, (5, 7, 3)), rng.integers(0, 2, (5, 7))
    out = vis.apply_mask(im, mask)
    assert out.shape == (5, 7, 3)
    assert np.allclose(out[mask > 0], 0.7 * im[mask > 0]) and np.allclose(out[mask == 0], 0.7 * im[mask == 0] + 0.3 * np.array([0, 255, 0]))
    grey = vis.apply_mask(im[..., 0], mask)
    assert grey.shape == (5, 7) and np.allclose(grey, 0.7 * im[..., 0] + 0.3 * (mask == 0))
    with pytest.raises(NotImplementedError):
        vis.visualize_depth_dir(".", ".", extension=".png")
    with pytest.raises(RuntimeError, match="HIP device"):
        import torch
        vis.visualize_depth(torch.zeros(4, 4))
    assert vis.previews_enabled() == (os.environ.get("CD_AMD_PREVIEWS", "1") != "0")


@needs_reference
def test_live_reference_equals_the_goldens():
    gen = _tool("gen_golden_visualization")
    g, live = V.golden(), gen.reference_outputs()
    assert sorted(g) == sorted(live)
    for k in g:
        assert np.array_equal(g[k], live[k], equal_nan=True) if g[k].dtype.kind == "f" else np.array_equal(g[k], live[k]), k
    from consistent_depth_amd.utils import visualization as vis
    with gen.recording_reference():
        from utils import visualization as ref_vis
        rng = np.random.default_rng(1)
        im, mask = rng.uniform(0, 255, (6, 5, 3)), rng.integers(0, 2, (6, 5))
        assert np.array_equal(vis.apply_mask(im, mask), ref_vis.apply_mask(im, mask))
        assert np.array_equal(vis.apply_mask(im[..., 0], mask), ref_vis.apply_mask(im[..., 0], mask))


@needs_reference
def test_live_reference_loop_equals_the_loop_golden():
    """The reference's loop with the recording stub (native fp32, one epoch).  fp32 sums depend on the OpenMP team size in their last
    bits, so the pixels are compared wherever the live `.raw` plane equals the golden's bit for bit (every pixel on the host that
    wrote the golden), and the live pixels must in any case be the formula applied to the live planes under the live ranges."""
    gen = _tool("gen_golden_visualization")
    g, live, ref = V.golden("vis_loop_6f_64x48.npz"), gen.loop_outputs(), V.golden()
    names = [str(n) for n in live["names"]]
    assert names == [str(n) for n in g["names"]] and np.array_equal(live["first_batch_frames"], g["first_batch_frames"])
    raws = {n: live[f"raw_{i}"] for i, n in enumerate(names)}
    first = [n for n in names if n.startswith("eval") and "_e0000_" in n and int(os.path.basename(n)[6:12]) in set(live["first_batch_frames"].tolist())]
    scale = max(raws[n].max() for n in first)
    depth = [n for n in names if n.startswith("depth")]
    lo, hi = min(raws[n].min() for n in depth), max(raws[n].max() for n in depth)
    for i, n in enumerate(names):
        want = V.preview_pixels(raws[n], lo, hi, ref["table_bgr"]) if n.startswith("depth") else V.preview_pixels(raws[n], 0, scale, ref["table_bgr"])
        assert np.array_equal(live[f"png_{i}"], want), n
    if all(np.array_equal(live[f"raw_{i}"], g[f"raw_{i}"]) for i in range(len(names))):
        for i, n in enumerate(names):
            assert np.array_equal(live[f"png_{i}"], g[f"png_{i}"]), n
