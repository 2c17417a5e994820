"""GPU: the flow stage in front of fine-tuning -- cd_flow_stage_masks (masks in the pair store's layout + valid-pixel counts),
consistent_depth_amd/flow.py::Flow on files, PairStore.from_flow_directory and the `--op all` wiring -- against the golden masks
the reference produced, the existing mask kernel, and the numpy oracle.  Boolean / integer outputs: everything is compared exactly."""
import glob
import json
import os
import shutil
import sys

import numpy as np
import pytest

from conftest import REPO
from test_masks_cpu import GOLDEN, load

pytestmark = pytest.mark.gpu


def chw(a):
    return np.ascontiguousarray(np.asarray(a, np.float32).transpose(2, 0, 1))


def raw_call(flows, color, pair_frames, rev, ft, ct):
    """The C entry itself on host arrays, with `masks` pre-filled with 0xAB and `counts` with garbage: every byte and count must be
    overwritten.  -> (masks (P,2,1,H,W) uint8, counts (P,2) int32) as numpy."""
    import torch
    from consistent_depth_amd import _native
    fl = torch.from_numpy(np.ascontiguousarray(flows, dtype=np.float32)).cuda()
    co = torch.from_numpy(np.ascontiguousarray(color, dtype=np.float32)).cuda()
    pf = torch.tensor(pair_frames, dtype=torch.int64).cuda()
    P, _, _, H, W = fl.shape
    masks = torch.full((P, 2, 1, H, W), 0xAB, dtype=torch.uint8, device="cuda")
    counts = torch.full((P, 2), -123456789, dtype=torch.int32, device="cuda")
    rc = _native.lib().cd_flow_stage_masks(fl.data_ptr(), co.data_ptr(), pf.data_ptr(), co.shape[1], rev, ft, ct, P, co.shape[0], H, W,
                                           masks.data_ptr(), counts.data_ptr(), _native.stream_ptr(fl.device))
    assert rc == 0
    torch.cuda.synchronize()
    return masks.cpu().numpy(), counts.cpu().numpy()


# ------------------------------------------------------------------------------------------------ kernel vs the reference's goldens
@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p)[:-4] for p in GOLDEN])
def test_kernel_reproduces_the_golden_masks_and_counts(path):
    """Two pairs over two frames: (0,1) with (fwd, bwd) and (1,0) with (bwd, fwd).  Odd widths, H*W % 4 != 0 (33x47), flows that
    leave the image (wild), the frame indirection."""
    flows, colors, ft, ct, ref = load(path)
    f = [chw(flows[0]), chw(flows[1])]
    store_flows = np.stack([np.stack([f[0], f[1]]), np.stack([f[1], f[0]])])
    color = np.stack([chw(colors[0]), chw(colors[1])])
    masks, counts = raw_call(store_flows, color, [[0, 1], [1, 0]], 0, ft, ct)
    assert set(np.unique(masks)) <= {0, 1}
    for k in range(2):
        np.testing.assert_array_equal(masks[0, k, 0], ref[k].astype(np.uint8))
        np.testing.assert_array_equal(masks[1, k, 0], masks[0, 1 - k, 0])
    want = [int(ref[0].sum()), int(ref[1].sum())]
    assert counts.tolist() == [want, want[::-1]]


# ------------------------------------------------------------------------------------------------ kernel vs the existing kernel
@pytest.fixture(scope="module")
def rebuilt_store():
    from consistent_depth_amd.loaders.pair_store import PairStore
    return PairStore.synthetic(6, 32, 48, seed=3).rebuild_masks(1.0, 1.0)


def test_kernel_gives_the_bytes_of_rebuild_masks(rebuilt_store):
    s = rebuilt_store
    assert len(s) > 2
    masks, counts = raw_call(s.flows.cpu().numpy(), s.color.cpu().numpy(), s.pair_frames.cpu().numpy().tolist(), 0, 1.0, 1.0)
    np.testing.assert_array_equal(masks, s.masks.cpu().numpy())
    np.testing.assert_array_equal(counts, s.mask_sums.cpu().numpy().astype(np.int64))
    assert 0 < counts.min() and counts.max() < 32 * 48


def test_python_entry_crosses_chunk_borders(rebuilt_store):
    import torch
    from consistent_depth_amd.utils import consistency
    s = rebuilt_store
    out = torch.full_like(s.masks, 0xAB)
    masks, counts = consistency.flow_stage_masks(s.flows, s.color, s.pair_frames, 1.0, 1.0, reverse_channels=False, masks=out, chunk=2)
    assert masks is out and masks.dtype == torch.uint8 and counts.dtype == torch.int32
    assert torch.equal(masks, s.masks)
    assert torch.equal(counts.float(), s.mask_sums)


# ------------------------------------------------------------------------------------------------ channel order
def test_the_colour_sum_follows_the_requested_channel_order():
    """(d0^2 + d1^2) + d2^2 in fp32 depends on the order.  A pixel that passes the flow test and whose two sums differ, with the
    threshold put on the larger sum, is valid in one order and not in the other: reverse_channels = 1 on the reversed (R,G,B)
    colours must give the masks of the file order, 0 those of the R,G,B order."""
    from oracle import masks_oracle
    from oracle.gen_golden_masks_inputs import make_case
    flows, colors = make_case(24, 40, seed=0)
    rgb = [np.ascontiguousarray(c[..., ::-1]) for c in colors]
    found = None
    for k in range(2):
        flow_ok, _ = masks_oracle.consistency_mask(flows[k], -flows[1 - k], flows[k], 1.0)
        _, s_file = masks_oracle.consistency_mask(colors[k], colors[1 - k], flows[k], 3.0)
        _, s_rgb = masks_oracle.consistency_mask(rgb[k], rgb[1 - k], flows[k], 3.0)
        for y, x in zip(*np.nonzero(flow_ok & (s_file != s_rgb))):
            lo, hi = sorted((float(s_file[y, x]), float(s_rgb[y, x])))
            ct = float(np.sqrt(hi / 3.0))
            thr = np.float32(3 * ct ** 2)
            if np.float32(lo) < thr <= np.float32(hi):          # the fp32 threshold separates the two sums
                found = (k, y, x, ct)
                break
        if found:
            break
    assert found is not None, "no pixel with order-dependent colour sums passes the flow test"
    k, y, x, ct = found
    print(f"direction {k} pixel ({y},{x}): color_thresh {ct!r}")
    want_file, _ = masks_oracle.consistent_flow_masks(flows, colors, 1.0, ct)
    want_rgb, _ = masks_oracle.consistent_flow_masks(flows, rgb, 1.0, ct)
    assert want_file[k][y, x] != want_rgb[k][y, x]
    store_flows = np.stack([np.stack([chw(flows[0]), chw(flows[1])])])
    color = np.stack([chw(rgb[0]), chw(rgb[1])])
    for rev, want in ((1, want_file), (0, want_rgb)):
        masks, counts = raw_call(store_flows, color, [[0, 1]], rev, 1.0, ct)
        for d in range(2):
            np.testing.assert_array_equal(masks[0, d, 0], want[d].astype(np.uint8))
            assert counts[0, d] == int(want[d].sum())


# ------------------------------------------------------------------------------------------------ the stage on files
PAIRS3 = [(0, 1), (1, 2), (0, 2)]


@pytest.fixture(scope="module")
def clip3(tmp_path_factory):
    """Three 24x40 frames, flows of (0,1), (1,2), (0,2) in both directions, colours as B,G,R .raw files; the oracle's masks of the
    files' own arrays, and an overlap threshold between the lowest and the middle per-pair minimum ratio."""
    from consistent_depth_amd.utils import image_io
    from oracle import masks_oracle
    from oracle.gen_golden_masks_inputs import make_case
    path = str(tmp_path_factory.mktemp("flow_stage") / "clip")
    for d in ("color_down", "flow", "out"):
        os.makedirs(os.path.join(path, d))
    cases = [make_case(24, 40, seed=40), make_case(24, 40, seed=41), make_case(24, 40, seed=42, wild=True)]
    colors = [cases[0][1][0], cases[0][1][1], cases[1][1][1]]
    for f, c in enumerate(colors):
        image_io.save_raw_float32_image(os.path.join(path, "color_down", f"frame_{f:06d}.raw"), c)
    want, ratio = {}, {}
    for (i, j), (flows, _) in zip(PAIRS3, cases):
        for (a, b), fl in (((i, j), flows[0]), ((j, i), flows[1])):
            image_io.save_raw_float32_image(os.path.join(path, "flow", f"flow_{a:06d}_{b:06d}.raw"), fl)
        m, _ = masks_oracle.consistent_flow_masks(flows, [colors[i], colors[j]], 1.0, 1.0)
        want[(i, j)], want[(j, i)] = m
        ratio[(i, j)] = min(float(m[0].sum()) / (24 * 40), float(m[1].sum()) / (24 * 40))
    mins = sorted(ratio.values())
    assert mins[0] < mins[1] < mins[2], mins
    overlap = (mins[0] + mins[1]) / 2
    frame_pairs = [(0, 1), (1, 0), (1, 2), (2, 1), (0, 2), (2, 0)]
    good = [p for p in PAIRS3 if ratio[p] >= overlap]
    assert 0 < len(good) < 3
    np.savez(os.path.join(path, "out", "metadata_scaled.npz"), intrinsics=np.tile(np.float32([30, 30, 20, 12]), (3, 1)),
             extrinsics=np.tile(np.eye(3, 4, dtype=np.float32), (3, 1, 1)))
    return dict(path=path, out=os.path.join(path, "out"), want=want, overlap=overlap, frame_pairs=frame_pairs,
                expected_list=[list(q) for p in good for q in (p, p[::-1])])


def _mtimes(*patterns):
    return {f: os.stat(f).st_mtime_ns for pat in patterns for f in sorted(glob.glob(pat))}


def test_stage_on_files(clip3):
    from PIL import Image
    from consistent_depth_amd.flow import Flow
    from consistent_depth_amd.loaders.pair_store import PairStore
    import torch
    c = clip3
    flow = Flow(c["path"], c["out"])
    flow.mask_valid_correspondences(chunk=2)
    for (a, b), m in c["want"].items():
        with Image.open(os.path.join(c["path"], "mask", f"mask_{a:06d}_{b:06d}.png")) as im:
            got = np.asarray(im)
        assert got.dtype == np.uint8 and got.ndim == 2
        np.testing.assert_array_equal(got, m.astype(np.uint8) * 255)
    fn = flow.check_good_flow_pairs(c["frame_pairs"], c["overlap"])
    assert fn == os.path.join(c["out"], "flow_list_%.2f.json" % c["overlap"])
    assert json.load(open(fn)) == c["expected_list"]
    # the same list from the PNGs alone (a fresh object has no counts of its own)
    os.rename(fn, fn + ".first")
    assert json.load(open(Flow(c["path"], c["out"]).check_good_flow_pairs(c["frame_pairs"], c["overlap"]))) == c["expected_list"]
    os.remove(fn + ".first")
    # a second run writes nothing
    before = _mtimes(os.path.join(c["path"], "mask", "*"), os.path.join(c["out"], "flow_list_*"))
    again = Flow(c["path"], c["out"])
    again.mask_valid_correspondences(chunk=2)
    assert again.check_good_flow_pairs(c["frame_pairs"], c["overlap"]) == fn
    assert _mtimes(os.path.join(c["path"], "mask", "*"), os.path.join(c["out"], "flow_list_*")) == before and len(before) == 7
    # the store built from colours and flows alone = the store loaded from what the stage wrote
    shutil.copyfile(fn, os.path.join(c["path"], "flow_list.json"))
    meta = os.path.join(c["out"], "metadata_scaled.npz")
    a = PairStore.from_directory(c["path"], meta)
    b = PairStore.from_flow_directory(c["path"], meta, c["frame_pairs"], c["overlap"])
    assert len(a) == len(c["expected_list"]) // 2 and a.frame_ids == b.frame_ids and a.pair_indices() == b.pair_indices()
    for name in ("masks", "pair_frames", "mask_sums", "flows", "color", "intrinsics", "extrinsics"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert b.masks.dtype == torch.uint8


def test_a_pair_with_one_direction_only_is_an_error(tmp_path):
    from consistent_depth_amd.flow import Flow
    from consistent_depth_amd.utils import image_io
    path = str(tmp_path)
    os.makedirs(os.path.join(path, "flow"))
    image_io.save_raw_float32_image(os.path.join(path, "flow", "flow_000000_000001.raw"), np.zeros((8, 8, 2), np.float32))
    with pytest.raises(FileNotFoundError, match="flow_000001_000000.raw"):
        Flow(path, path).mask_valid_correspondences()


# ------------------------------------------------------------------------------------------------ argument checks
def test_bad_arguments_are_rejected_before_any_launch():
    import torch
    from consistent_depth_amd import _native
    from consistent_depth_amd.utils import consistency
    fl, co = torch.zeros(2, 2, 2, 8, 8), torch.zeros(2, 3, 8, 8)
    pf = torch.tensor([[0, 1], [1, 0]])
    with pytest.raises(RuntimeError, match="HIP device"):
        consistency.flow_stage_masks(fl, co, pf)
    with pytest.raises(TypeError):
        consistency.flow_stage_masks(None, co.cuda(), pf.cuda())
    with pytest.raises(ValueError, match="P > 0"):
        consistency.flow_stage_masks(fl[:0].cuda(), co.cuda(), pf[:0].cuda())
    for bad in ([[0, 2], [1, 0]], [[0, 1], [-1, 0]]):
        with pytest.raises(ValueError, match="pair_frames holds rows"):
            consistency.flow_stage_masks(fl.cuda(), co.cuda(), torch.tensor(bad).cuda())
    with pytest.raises(ValueError):
        consistency.flow_stage_masks(fl.cuda(), torch.zeros(2, 3, 8, 9).cuda(), pf.cuda())
    # the C entry: null pointers, non-positive sizes, W < 2, a mask pointer off the word grid
    lib, m, c = _native.lib(), torch.zeros(2, 2, 1, 8, 8, dtype=torch.uint8).cuda(), torch.zeros(2, 2, dtype=torch.int32).cuda()
    f, k, p = fl.cuda(), co.cuda(), pf.cuda()
    call = lambda *a: lib.cd_flow_stage_masks(*a, _native.stream_ptr(f.device))  # noqa: E731
    assert call(f.data_ptr(), k.data_ptr(), p.data_ptr(), 3, 0, 1.0, 1.0, 2, 2, 8, 8, m.data_ptr(), c.data_ptr()) == 0
    assert call(None, k.data_ptr(), p.data_ptr(), 3, 0, 1.0, 1.0, 2, 2, 8, 8, m.data_ptr(), c.data_ptr()) == -1
    assert call(f.data_ptr(), k.data_ptr(), p.data_ptr(), 3, 0, 1.0, 1.0, 2, 2, 8, 8, m.data_ptr(), None) == -1
    assert call(f.data_ptr(), k.data_ptr(), p.data_ptr(), 3, 0, 1.0, 1.0, 0, 2, 8, 8, m.data_ptr(), c.data_ptr()) == -1
    assert call(f.data_ptr(), k.data_ptr(), p.data_ptr(), 3, 0, 1.0, 1.0, 2, 2, 64, 1, m.data_ptr(), c.data_ptr()) == -1
    assert call(f.data_ptr(), k.data_ptr(), p.data_ptr(), 3, 2, 1.0, 1.0, 2, 2, 8, 8, m.data_ptr(), c.data_ptr()) == -1
    assert call(f.data_ptr(), k.data_ptr(), p.data_ptr(), 3, 0, 1.0, 1.0, 1, 2, 8, 8, m.data_ptr() + 1, c.data_ptr()) == -1
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ end to end
def _write_clip(path):
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import make_synthetic_dataset as msd
    return msd.write_dataset(path, n_frames=6, H=64, W=48)


def _run(path):
    from consistent_depth_amd.params import Video3dParamsParser
    from consistent_depth_amd.process import DatasetProcessor
    return DatasetProcessor().process(Video3dParamsParser().parse(["--path", path, "--num_epochs", "1", "--batch_size", "4"]))


def test_op_all_builds_the_masks_and_the_pair_list_it_lacks(tmp_path):
    from PIL import Image
    from consistent_depth_amd.utils import image_io
    from oracle import masks_oracle
    path = str(tmp_path / "clip")
    range_dir, pairs = _write_clip(path)
    shutil.rmtree(os.path.join(path, "mask"))
    os.remove(os.path.join(path, "flow_list.json"))
    _, out_dir, frames = _run(path)
    ratios = {}
    for i, j in pairs:
        flows = [image_io.load_raw_float32_image(os.path.join(path, "flow", f"flow_{a:06d}_{b:06d}.raw")) for a, b in ((i, j), (j, i))]
        colors = [image_io.load_raw_float32_image(os.path.join(path, "color_down", f"frame_{a:06d}.raw")) for a in (i, j)]
        want, _ = masks_oracle.consistent_flow_masks(flows, colors, 1.0, 1.0)
        for (a, b), m in zip(((i, j), (j, i)), want):
            with Image.open(os.path.join(path, "mask", f"mask_{a:06d}_{b:06d}.png")) as im:
                np.testing.assert_array_equal(np.asarray(im), m.astype(np.uint8) * 255)
        ratios[(i, j)] = min(float(m.sum()) / m.size for m in want)
    assert len(glob.glob(os.path.join(path, "mask", "*.png"))) == 2 * len(pairs)
    listed = json.load(open(os.path.join(path, "flow_list.json")))
    assert listed == json.load(open(os.path.join(range_dir, "flow_list_0.20.json")))
    assert {tuple(sorted(p)) for p in listed} == {p for p, r in ratios.items() if r >= 0.2} and len(listed) == 2 * len({tuple(sorted(p)) for p in listed})
    assert frames and len(glob.glob(os.path.join(out_dir, "depth", "frame_*.raw"))) == len(frames)
    for fr in frames:
        inv = image_io.load_raw_float32_image(os.path.join(out_dir, "depth", f"frame_{fr:06d}.raw"))
        assert inv.shape == (64, 48) and np.isfinite(inv).all()


def test_op_all_leaves_a_complete_clip_alone(tmp_path):
    path = str(tmp_path / "clip")
    range_dir, _ = _write_clip(path)
    before = _mtimes(os.path.join(path, "mask", "*"), os.path.join(path, "flow_list.json"))
    _run(path)
    assert _mtimes(os.path.join(path, "mask", "*"), os.path.join(path, "flow_list.json")) == before
    assert not glob.glob(os.path.join(path, "**", "flow_list_*.json"), recursive=True)
