"""GPU: the depth previews (csrc/visualize.hip, utils/visualization.py) -- the colourise kernel bit for bit against the reference's
recorded pixels (tests/golden/vis_reference.npz), the range kernel against numpy, `visualize_depth_dir` on the golden directory,
the PNGs of a short fine-tuning run with the previews on and off, two ranks against one process, and the kernels the profiler sees.
Where the GPU box has no reference the yardstick is tests/vis_util.py::preview_pixels, pinned to the reference by the CPU tests."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, REPO

import vis_util as V

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def _scalar(torch, v):
    return torch.full((1,), float(v), dtype=torch.float32, device="cuda")


def test_colorize_kernel_is_bit_exact(torch_cuda):
    torch = torch_cuda
    from consistent_depth_amd.utils import visualization as vis
    g = V.golden()
    for name in g["vd_names"]:
        d, (lo, hi) = g[f"vd_{name}_in"], g[f"vd_{name}_range"]
        x = torch.as_tensor(d).cuda()
        if bool(g[f"vd_{name}_auto"]):
            got = vis.visualize_depth(x)
        else:
            got = vis.visualize_depth(x, _scalar(torch, lo), float(hi))
        assert got.dtype == torch.uint8 and tuple(got.shape) == d.shape + (3,)
        assert np.array_equal(got.cpu().numpy(), g[f"vd_{name}_out"]), name
        rgb = vis.visualize_depth(x, None if bool(g[f"vd_{name}_auto"]) else float(lo), None if bool(g[f"vd_{name}_auto"]) else float(hi), bgr=False)
        assert np.array_equal(rgb.cpu().numpy(), g[f"vd_{name}_out"][..., ::-1]), name
    # an unaligned view (base 4 bytes past a 16-byte boundary, odd element count): the scalar path; and a batch of planes
    d = g["vd_odd_37x53_in"]
    buf = torch.zeros(d.size + 5, device="cuda")
    view = buf[1:1 + d.size].view(37, 53)
    view.copy_(torch.as_tensor(d))
    assert view.data_ptr() % 16 == 4
    lo, hi = g["vd_odd_37x53_range"]
    assert np.array_equal(vis.colorize(view, _scalar(torch, lo), _scalar(torch, hi), bgr=True).cpu().numpy(), g["vd_odd_37x53_out"])
    w = g["vd_wrap_in"]
    batch = torch.as_tensor(np.stack([w, w[::-1].copy(), w * 2])).cuda()
    got = vis.colorize(batch, _scalar(torch, 0), _scalar(torch, 1), bgr=True).cpu().numpy()
    for k, p in enumerate((w, w[::-1], w * 2)):
        assert np.array_equal(got[k], V.preview_pixels(p, 0, 1, g["table_bgr"])), k
    assert np.array_equal(got[0], g["vd_wrap_out"])
    # large in-range plane at the headline size
    rng = np.random.default_rng(3)
    big = rng.uniform(0, 2.5, (4, 384, 224)).astype(np.float32)
    got = vis.colorize(torch.as_tensor(big).cuda(), _scalar(torch, 0), _scalar(torch, 2.5), bgr=True).cpu().numpy()
    assert np.array_equal(got, V.preview_pixels(big, 0, 2.5, g["table_bgr"]))


def _same(a, b):
    """Equal as float32 values, NaN == NaN.  (-0.0 and +0.0 are the same value: numpy's min / max / sort do not order them either.)"""
    return np.array_equal(np.float32(a), np.float32(b), equal_nan=True)


def _range_cases():
    rng = np.random.default_rng(7)
    big = rng.uniform(0.01, 4.0, (384, 224)).astype(np.float32)
    big[rng.random(big.shape) > 0.7] = np.nan
    big[3, 3], big[4, 4] = np.inf, -np.inf
    dup = np.round(rng.uniform(0, 6, (64, 48))).astype(np.float32)
    zeros = rng.standard_normal((37, 53)).astype(np.float32)
    zeros[::3] = 0.0
    zeros[1::3] = -0.0
    one = np.full((16, 16), np.nan, np.float32)
    one[5, 6] = 0.5
    two = one.copy()
    two[7, 7] = -2.0
    return {"384x224": big, "dense": rng.standard_normal((384, 224)).astype(np.float32), "duplicates": dup, "signed_zeros": zeros,
            "all_nan": np.full((24, 20), np.nan, np.float32), "one": one, "two": two}


def test_range_kernel_matches_numpy(torch_cuda):
    torch = torch_cuda
    from consistent_depth_amd.utils import visualization as vis
    for name, p in _range_cases().items():
        x = torch.as_tensor(p[None]).cuda()
        f = p[np.isfinite(p)]
        counts, stats = vis.depth_range(x, vis.RANGE_MINMAX)
        c, s = int(counts.item()), stats.cpu().numpy()[0]
        assert c == f.size, name
        if f.size:
            assert _same(s[0], f.min()) and _same(s[1], f.min()) and _same(s[2], f.max()) and _same(s[3], f.max()), (name, s)
        else:
            assert np.isnan(s).all(), name
        # NaN-propagating min / max over everything (np.amin / np.amax)
        counts, stats = vis.depth_range(x, vis.RANGE_NANMAX)
        s = stats.cpu().numpy()[0]
        with np.errstate(all="ignore"):
            assert int(counts.item()) == p.size and _same(s[0], np.amin(p)) and _same(s[3], np.amax(p)), (name, s)
        assert _same(vis.nan_max(x).item(), np.amax(p))
        # order statistics around numpy's float32 virtual index
        srt = np.sort(f)
        for q_lo, q_hi in ((0, 99), (1, 50), (25, 99.9), (5, 100)):
            counts, stats = vis.depth_range(x, vis.RANGE_PERCENTILE, float(vis.quantile32(q_lo)), float(vis.quantile32(q_hi)))
            s = stats.cpu().numpy()[0]
            assert int(counts.item()) == f.size
            if not f.size:
                assert np.isnan(s).all()
                continue
            for j, q in enumerate((q_lo, q_hi)):
                last = np.float32(f.size - 1)
                vi = last * vis.quantile32(q)
                k = f.size - 1 if vi >= last else int(np.floor(vi))
                assert _same(s[2 * j], srt[k]) and _same(s[2 * j + 1], srt[min(k + 1, f.size - 1)]), (name, q, s, srt[k])
                got = vis.interpolate_percentile(f.size, s[2 * j], s[2 * j + 1], q)
                want = np.percentile(f, q)
                u = V.ulp_distance(want, np.float32(np.percentile(f.astype(np.float64), q)))
                assert srt[k] <= got <= srt[min(k + 1, f.size - 1)] and V.ulp_distance(got, want) <= max(1, u), (name, q, got, want, u)
    # a batch in one launch + the fold on the device
    cases = _range_cases()
    stack = np.stack([cases["384x224"], cases["dense"], np.full((384, 224), np.nan, np.float32)])
    counts, stats = vis.depth_range(torch.as_tensor(stack).cuda(), vis.RANGE_MINMAX)
    dmin, dmax = vis.fold_range(counts, stats)
    fin = stack[np.isfinite(stack)]
    assert _same(dmin.item(), fin.min()) and _same(dmax.item(), max(np.float32(0), fin.max()))
    counts, stats = vis.depth_range(torch.as_tensor(stack[2:]).cuda(), vis.RANGE_MINMAX)     # nothing finite: float32 of the reference's start values
    dmin, dmax = vis.fold_range(counts, stats)
    assert dmin.item() == np.inf and dmax.item() == 0.0


def _write_golden_dir(g, path):
    from consistent_depth_amd.utils import image_io
    os.makedirs(path, exist_ok=True)
    for k, name in enumerate(g["dir_names"]):
        image_io.save_raw_float32_image(os.path.join(path, str(name)), g[f"dir_in_{k}"])


def test_visualize_depth_dir_on_the_golden_directory(torch_cuda, tmp_path):
    torch = torch_cuda
    from consistent_depth_amd.utils import visualization as vis
    g = V.golden()
    src = str(tmp_path / "dir")
    _write_golden_dir(g, src)
    vis.visualize_depth_dir(src, src, force=True)
    pngs = sorted(os.path.basename(p) for p in glob.glob(os.path.join(src, "*.png")))
    assert pngs == sorted(os.path.splitext(str(n))[0] + ".png" for n in g["dir_names"])
    for k, name in enumerate(g["dir_names"]):
        got = V.read_png(os.path.join(src, os.path.splitext(str(name))[0] + ".png"))
        assert np.array_equal(got[..., ::-1], g[f"dir_out_0_100_{k}"]), name
    # not forced and everything there: nothing is rewritten
    stamp = {p: os.path.getmtime(os.path.join(src, p)) for p in pngs}
    vis.visualize_depth_dir(src, src)
    assert stamp == {p: os.path.getmtime(os.path.join(src, p)) for p in pngs}
    # 0 / 99 into another directory: the pixels are the formula under the product's OWN range (bit-exact whatever the interpolation
    # did); the range itself is held to the percentile tolerance of the issue
    dst = str(tmp_path / "p99")
    vis.visualize_depth_dir(src, dst, min_percentile=0, max_percentile=99)
    planes = [g[f"dir_in_{k}"] for k in range(len(g["dir_names"]))]
    shapes = sorted({p.shape for p in planes})
    groups = [torch.as_tensor(np.stack([p for p in planes if p.shape == s])).cuda() for s in shapes]
    dmin, dmax, _ = vis.directory_range(groups, 0, 99)
    lo, hi = np.float32(dmin.item()), np.float32(dmax.item())
    finite = [p[np.isfinite(p)] for p in planes if np.isfinite(p).any()]
    want_lo, want_hi = min(np.percentile(f, 0) for f in finite), max(np.percentile(f, 99) for f in finite)
    u = max(V.ulp_distance(np.percentile(f, 99), np.float32(np.percentile(f.astype(np.float64), 99))) for f in finite)
    print(f"0 / 99 range: product [{lo}, {hi}], numpy [{want_lo}, {want_hi}], reference's own spread {u} ulp")
    assert lo == want_lo and V.ulp_distance(hi, want_hi) <= max(1, u)
    differs = 0
    for k, name in enumerate(g["dir_names"]):
        got = V.read_png(os.path.join(dst, os.path.splitext(str(name))[0] + ".png"))
        assert np.array_equal(got[..., ::-1], V.preview_pixels(planes[k], lo, hi, g["table_bgr"])), name
        differs += int((got[..., ::-1] != g[f"dir_out_0_99_{k}"]).any(-1).sum())
    print(f"0 / 99: {differs} pixels differ from the reference's recorded PNGs")


def _run_finetune(tmp_path, tag, previews):
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import make_synthetic_dataset as msd
    from consistent_depth_amd.depth_fine_tuning import DepthFineTuner
    from consistent_depth_amd.params import Video3dParamsParser
    path = str(tmp_path / tag)
    range_dir, pairs = msd.write_dataset(path, n_frames=6, H=64, W=48, seed=3)
    params = Video3dParamsParser().parse(["--path", path, "--num_epochs", "1", "--batch_size", "4", "--print_freq", "0"])
    old = os.environ.get("CD_AMD_PREVIEWS")
    os.environ["CD_AMD_PREVIEWS"] = "1" if previews else "0"
    try:
        ft = DepthFineTuner(range_dir, list(range(6)), params)
        ft.fine_tune()
        ft.save_depth()
    finally:
        if old is None:
            del os.environ["CD_AMD_PREVIEWS"]
        else:
            os.environ["CD_AMD_PREVIEWS"] = old
    return ft, pairs


def _files(root, pattern):
    return sorted(os.path.relpath(p, root) for p in glob.glob(os.path.join(root, "*", pattern)))


def test_previews_of_a_short_finetune_on_and_off(torch_cuda, tmp_path):
    from consistent_depth_amd.utils import image_io
    table = V.golden()["table_bgr"][:, ::-1]            # R,G,B: what PIL decodes
    on, pairs = _run_finetune(tmp_path, "on", True)
    off, _ = _run_finetune(tmp_path, "off", False)
    raws, pngs = _files(on.out_dir, "*.raw"), _files(on.out_dir, "*.png")
    assert len(raws) == 2 * 6 + 6 and pngs == [os.path.splitext(r)[0] + ".png" for r in raws]
    # the validation scale: the maximum of the first batch (pairs 0..3) of the FIRST sweep, kept for the sweep after the epoch
    first_frames = sorted({f for p in pairs[:4] for f in p})
    load = lambda rel: image_io.load_raw_float32_image(os.path.join(on.out_dir, rel))      # noqa: E731
    scale = max(load(os.path.join("eval", f"depth_{f:06d}_e0000_iter000000.raw")).max() for f in first_frames)
    assert np.float32(on.vis_depth_scale.item()) == np.float32(scale)
    depth = [load(r) for r in raws if r.startswith("depth")]
    lo, hi = min(d.min() for d in depth), max(d.max() for d in depth)
    for r in raws:
        got = V.read_png(os.path.join(on.out_dir, os.path.splitext(r)[0] + ".png"))
        want = V.preview_pixels(load(r), lo, hi, table) if r.startswith("depth") else V.preview_pixels(load(r), 0, scale, table)
        assert np.array_equal(got, want), r
    # previews off: no PNG, every other artefact byte for byte
    assert _files(off.out_dir, "*.png") == [] and _files(off.out_dir, "*.raw") == raws
    for rel in raws + _files(on.out_dir, "*.json"):
        with open(os.path.join(on.out_dir, rel), "rb") as a, open(os.path.join(off.out_dir, rel), "rb") as b:
            assert a.read() == b.read(), rel
    assert _files(off.out_dir, "*.json") == _files(on.out_dir, "*.json") and len(_files(on.out_dir, "*.json")) == 2


def test_stale_raw_files_join_the_range_of_save_depth(torch_cuda, tmp_path):
    """A `.raw` left in depth/ by an earlier run takes part in the range and is rendered again (force=True in the reference)."""
    from consistent_depth_amd.utils import image_io
    table = V.golden()["table_bgr"][:, ::-1]
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import make_synthetic_dataset as msd
    from consistent_depth_amd.depth_fine_tuning import DepthFineTuner
    from consistent_depth_amd.loaders.pair_store import PairStore
    from consistent_depth_amd.params import Video3dParamsParser
    path = str(tmp_path / "clip")
    range_dir, _ = msd.write_dataset(path, n_frames=4, H=64, W=48, seed=5)
    params = Video3dParamsParser().parse(["--path", path, "--num_epochs", "1", "--batch_size", "4"])
    ft = DepthFineTuner(range_dir, list(range(4)), params)
    ft.store = PairStore.from_directory(path, os.path.join(range_dir, "metadata_scaled.npz"))
    out = str(tmp_path / "export")
    os.makedirs(os.path.join(out, "depth"))
    stale = np.random.default_rng(0).uniform(0.0, 50.0, (20, 30)).astype(np.float32)
    image_io.save_raw_float32_image(os.path.join(out, "depth", "frame_000077.raw"), stale)
    ft.save_depth(out)
    names = sorted(os.listdir(os.path.join(out, "depth")))
    assert names == sorted([f"frame_{i:06d}.{e}" for i in (0, 1, 2, 3, 77) for e in ("png", "raw")])
    planes = {n: image_io.load_raw_float32_image(os.path.join(out, "depth", n)) for n in names if n.endswith(".raw")}
    lo, hi = min(p.min() for p in planes.values()), max(p.max() for p in planes.values())
    assert hi == stale.max()
    for n, p in planes.items():
        assert np.array_equal(V.read_png(os.path.join(out, "depth", n[:-4] + ".png")), V.preview_pixels(p, lo, hi, table)), n


def test_scale_calibration_writes_the_previews_of_the_scaled_maps(torch_cuda, tmp_path, monkeypatch):
    """depth_scaled_by_colmap_dense/depth gets a PNG per `.raw` (the planes of the call stay on the device; a stale file of an
    earlier run is read from disk), all under the directory's minimum / maximum; CD_AMD_PREVIEWS=0 writes the same `.raw` and no PNG."""
    from consistent_depth_amd import scale_calibration as SC
    from consistent_depth_amd.utils import image_io
    from oracle import scale_oracle as S
    table = V.golden()["table_bgr"][:, ::-1]
    z = np.load(os.path.join(GOLDEN, "scale_stage_6f_48x40.npz"))
    inv_src, inv_cmp, intr, extr = S.make_case(int(z["seed"]))
    dirs = {}
    for tag, mode in (("on", "1"), ("off", "0")):
        monkeypatch.setenv("CD_AMD_PREVIEWS", mode)
        path, out = str(tmp_path / f"clip_{tag}"), str(tmp_path / f"out_{tag}")
        S.write_case(path, out, inv_src, inv_cmp, intr, extr)
        dirs[tag] = os.path.join(out, "depth_scaled_by_colmap_dense", "depth")
        os.makedirs(dirs[tag])
        stale = np.random.default_rng(1).uniform(0.0, 9.0, (20, 30)).astype(np.float32)
        stale[2, 3] = np.nan
        image_io.save_raw_float32_image(os.path.join(dirs[tag], "frame_000077.raw"), stale)
        assert SC.calibrate_scale(path, out, sorted(inv_src)) == {0, 1, 2, 4}
    names = sorted(os.listdir(dirs["on"]))
    assert names == sorted([f"frame_{i:06d}.{e}" for i in (0, 1, 2, 4, 77) for e in ("png", "raw")])
    assert sorted(os.listdir(dirs["off"])) == [n for n in names if n.endswith(".raw")]
    planes = {n: image_io.load_raw_float32_image(os.path.join(dirs["on"], n)) for n in names if n.endswith(".raw")}
    for i, want in zip(z["scaled_frames"].tolist(), z["scaled"]):
        assert np.array_equal(planes[f"frame_{i:06d}.raw"], want, equal_nan=True), i
    lo = min(p[np.isfinite(p)].min() for p in planes.values())
    hi = max(p[np.isfinite(p)].max() for p in planes.values())
    for n, p in planes.items():
        assert np.array_equal(V.read_png(os.path.join(dirs["on"], n[:-4] + ".png")), V.preview_pixels(p, lo, hi, table)), n
        with open(os.path.join(dirs["on"], n), "rb") as a, open(os.path.join(dirs["off"], n), "rb") as b:
            assert a.read() == b.read(), n


TWO_RANK_WORKER = r"""
import os, sys, torch
sys.path.insert(0, %(repo)r)
from consistent_depth_amd import parallel
from consistent_depth_amd.depth_fine_tuning import DepthFineTuner
from consistent_depth_amd.params import Video3dParamsParser
rank, local_rank, world = parallel.init()
torch.cuda.set_device(parallel.local_device(local_rank))
params = Video3dParamsParser().parse(["--path", %(path)r, "--num_epochs", "0", "--batch_size", "2", "--print_freq", "0"])
ft = DepthFineTuner(%(range_dir)r, list(range(6)), params)
ft.fine_tune()
torch.cuda.synchronize()
if world > 1:
    torch.distributed.barrier(); torch.distributed.destroy_process_group()
if rank == 0:
    print("RESULT " + ft.out_dir)
"""


def test_two_ranks_render_the_same_previews_as_one_process(torch_cuda, tmp_path):
    """The validation sweep sharded over two ranks (gloo, both on this GPU): rank 0 owns the first batch, fixes the scale and
    broadcasts it before rank 1 renders.  Same PNG pixels as one process."""
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import make_synthetic_dataset as msd
    outs = {}
    for world in (1, 2):
        path = str(tmp_path / f"clip{world}")
        range_dir, _ = msd.write_dataset(path, n_frames=6, H=64, W=48, seed=3)
        script = tmp_path / f"worker{world}.py"
        script.write_text(TWO_RANK_WORKER % {"repo": REPO, "path": path, "range_dir": range_dir})
        env = dict(os.environ, CD_AMD_DIST_BACKEND="gloo", MASTER_ADDR="127.0.0.1", CD_AMD_PREVIEWS="1")
        for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE"):
            env.pop(k, None)
        cmd = [sys.executable, str(script)] if world == 1 else [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                                                                 "--master-addr", "127.0.0.1", "--master-port", "29561", str(script)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        assert lines, r.stdout[-2000:] + r.stderr[-3000:]
        outs[world] = lines[-1][len("RESULT "):]
    one, two = _files(outs[1], "*.png"), _files(outs[2], "*.png")
    assert one == two and len(one) == 6
    for rel in one:
        assert np.array_equal(V.read_png(os.path.join(outs[1], rel)), V.read_png(os.path.join(outs[2], rel))), rel


def test_only_this_packages_kernels_between_depth_and_host_copy(torch_cuda):
    torch = torch_cuda
    from consistent_depth_amd.utils import visualization as vis
    x = torch.rand(8, 384, 224, device="cuda")
    zero = torch.zeros(1, device="cuda")

    def run():
        counts, stats = vis.depth_range(x, vis.RANGE_MINMAX)
        dmin, dmax = vis.fold_range(counts, stats)
        a = vis.colorize(x, dmin, dmax)
        b = vis.colorize(x, zero, vis.nan_max(x))
        return a.cpu(), b.cpu()

    run()
    torch.cuda.synchronize()
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        run()
        torch.cuda.synchronize()
    kernels = [e.name for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA") and e.name
               and not getattr(e, "is_user_annotation", False) and "#" not in e.name]
    assert any("cd::" in k for k in kernels), f"no kernel of this package among the {len(kernels)} device events: {sorted(set(kernels))}"
    foreign = sorted({k for k in kernels if "cd::" not in k and "rocclr" not in k.lower() and not k.lower().startswith(("memcpy", "memset"))})
    assert not foreign, foreign
    for want in ("depth_range_kernel", "depth_range_fold_kernel", "depth_colorize_kernel"):
        assert any(want in k for k in kernels), sorted(set(kernels))
