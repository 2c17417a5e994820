"""CPU: the good-pair filter of the flow stage (consistent_depth_amd/flow.py::Flow.check_good_flow_pairs) on mask PNGs written
from the golden masks the reference itself produced (tests/golden/masks_*.npz), one clip per size.  Valid fractions of those
goldens (forward / backward): basic 24x40 0.254 / 0.227, size 96x128 0.843 / 0.689, tight 33x47 0.124 / 0.085,
wild 32x32 0.021 / 0.019 -- at the default overlap ratio 0.2 basic and size pass, at the KITTI preset's 0.5 only size does."""
import json
import os
import sys
import types

import numpy as np
import pytest

from test_masks_cpu import GOLDEN

NAMES = [os.path.basename(p).split("_")[1] for p in GOLDEN]      # masks_<name>_<H>x<W>.npz
RATIOS = {"basic": (0.254, 0.227), "size": (0.843, 0.689), "tight": (0.124, 0.085), "wild": (0.021, 0.019)}
PAIR = (3, 7)


def make_clip(root, name):
    """<root>/<name>: mask/mask_000003_000007.png (forward) and mask_000007_000003.png (backward) of one golden."""
    from consistent_depth_amd.utils import image_io
    d = np.load(GOLDEN[NAMES.index(name)])
    path = os.path.join(str(root), name)
    os.makedirs(os.path.join(path, "mask"))
    os.makedirs(os.path.join(path, "out"))
    for (a, b), key in ((PAIR, "mask_fwd"), (PAIR[::-1], "mask_bwd")):
        image_io.save_mask_png(os.path.join(path, "mask", f"mask_{a:06d}_{b:06d}.png"), d[key])
    return path


def flow_of(path):
    from consistent_depth_amd.flow import Flow
    return Flow(path, os.path.join(path, "out"))


def test_the_goldens_have_the_stated_ratios():
    assert sorted(NAMES) == sorted(RATIOS)
    for name, path in zip(NAMES, GOLDEN):
        d = np.load(path)
        for key, want in zip(("mask_fwd", "mask_bwd"), RATIOS[name]):
            assert abs(float(d[key].mean()) - want) < 5e-4, (name, key, float(d[key].mean()))


@pytest.mark.parametrize("ratio,passing", [(0.2, {"basic", "size"}), (0.5, {"size"})], ids=["default", "kitti"])
@pytest.mark.parametrize("name", sorted(RATIOS))
def test_pairs_pass_or_fail_by_both_directions(tmp_path, name, ratio, passing):
    path = make_clip(tmp_path, name)
    flow = flow_of(path)
    if name not in passing:
        with pytest.raises(Exception, match="No good frame pairs are found."):
            flow.check_good_flow_pairs([PAIR], ratio)
        assert not os.listdir(os.path.join(path, "out"))
        return
    fn = flow.check_good_flow_pairs([PAIR], ratio)
    assert fn == os.path.join(path, "out", "flow_list_%.2f.json" % ratio)
    assert json.load(open(fn)) == [list(PAIR), list(PAIR[::-1])]


def test_list_name_content_and_reuse(tmp_path):
    path = make_clip(tmp_path, "size")
    fn = flow_of(path).check_good_flow_pairs([PAIR], 0.2)
    assert os.path.basename(fn) == "flow_list_0.20.json"
    assert open(fn).read() == "[[3, 7], [7, 3]]"
    # an existing list is returned as it is: not rewritten, not even when the pairs would fail now
    with open(fn, "w") as f:
        f.write("[[1, 2], [2, 1]]")
    before = os.stat(fn).st_mtime_ns
    assert flow_of(path).check_good_flow_pairs([(8, 9)], 0.2) == fn
    assert os.stat(fn).st_mtime_ns == before and open(fn).read() == "[[1, 2], [2, 1]]"


def test_a_repeated_or_reversed_pair_is_visited_once(tmp_path, monkeypatch):
    path = make_clip(tmp_path, "size")
    flow = flow_of(path)
    visited = []
    ratio = flow.mask_ratio
    monkeypatch.setattr(flow, "mask_ratio", lambda i, j: visited.append((i, j)) or ratio(i, j))
    fn = flow.check_good_flow_pairs([PAIR, PAIR[::-1], list(PAIR), PAIR], 0.2)
    assert visited == [PAIR, PAIR[::-1]]
    assert json.load(open(fn)) == [[3, 7], [7, 3]]


def test_the_reversed_pair_first_keeps_its_order(tmp_path):
    path = make_clip(tmp_path, "size")
    fn = flow_of(path).check_good_flow_pairs([PAIR[::-1], PAIR], 0.2)
    assert json.load(open(fn)) == [[7, 3], [3, 7]]


def test_one_failing_direction_drops_the_pair(tmp_path):
    """size: forward 0.843, backward 0.689 -- between them the pair fails although one direction passes."""
    path = make_clip(tmp_path, "size")
    with pytest.raises(Exception, match="No good frame pairs"):
        flow_of(path).check_good_flow_pairs([PAIR], 0.75)


def test_compute_flow_is_an_input_and_flow_files_are_checked(tmp_path):
    path = make_clip(tmp_path, "basic")
    flow = flow_of(path)
    with pytest.raises(NotImplementedError, match="input"):
        flow.compute_flow([PAIR], "FlowNet2")
    os.makedirs(os.path.join(path, "flow"))
    assert not flow.check_flow_files([PAIR])
    open(os.path.join(path, "flow", "flow_000003_000007.raw"), "wb").close()
    assert flow.check_flow_files([PAIR]) and not flow.check_flow_files([PAIR, PAIR[::-1]])
    assert flow.flow_pairs() == [PAIR]
    assert flow.max_size() == 1024


def test_importing_the_stage_needs_no_gpu():
    import consistent_depth_amd.flow as F
    assert "torch" not in F.__dict__


REF = "/root/reference"


@pytest.mark.skipif(not os.path.isfile(os.path.join(REF, "flow.py")), reason="reference checkout not present")
def test_list_file_equals_the_live_reference_byte_for_byte(tmp_path):
    """The reference's own Flow.check_good_flow_pairs, imported unmodified through the stub set of the live-reference tests
    (cv2.imread = PIL), on the same directories."""
    from oracle import ref_loop
    frame_pairs = [PAIR, PAIR[::-1], PAIR]
    ours = {}
    for name in ("basic", "size"):
        for ratio in (0.2, 0.5):
            path = make_clip(tmp_path / f"ours_{ratio}", name)
            try:
                ours[(name, ratio)] = open(flow_of(path).check_good_flow_pairs(frame_pairs, ratio)).read()
            except Exception as e:   # noqa: BLE001
                ours[(name, ratio)] = str(e)
    extra = {"third_party": types.ModuleType("third_party"), "third_party.OpticalFlowToolkit": types.ModuleType("third_party.OpticalFlowToolkit"),
             "third_party.OpticalFlowToolkit.lib": types.ModuleType("third_party.OpticalFlowToolkit.lib"),
             "third_party.OpticalFlowToolkit.lib.flowlib": types.ModuleType("third_party.OpticalFlowToolkit.lib.flowlib"),
             "optical_flow_flownet2_homography": types.ModuleType("optical_flow_flownet2_homography")}
    for k in list(extra)[:3]:
        extra[k].__path__ = []
    extra["third_party.OpticalFlowToolkit.lib"].flowlib = extra["third_party.OpticalFlowToolkit.lib.flowlib"]
    saved = {k: sys.modules.pop(k) for k in list(sys.modules) if k in extra or k == "flow"}
    theirs = {}
    try:
        with ref_loop.reference_modules():
            sys.modules.update(extra)
            import flow as ref_flow
            assert ref_flow.__file__.startswith(REF)
            for name in ("basic", "size"):
                for ratio in (0.2, 0.5):
                    path = make_clip(tmp_path / f"ref_{ratio}", name)
                    try:
                        theirs[(name, ratio)] = open(ref_flow.Flow(path, os.path.join(path, "out")).check_good_flow_pairs(frame_pairs, ratio)).read()
                    except Exception as e:   # noqa: BLE001
                        theirs[(name, ratio)] = str(e)
    finally:
        for k in list(extra) + ["flow"]:
            sys.modules.pop(k, None)
        sys.modules.update(saved)
    assert ours == theirs
    assert ours[("size", 0.5)] == "[[3, 7], [7, 3]]" and ours[("basic", 0.5)] == "No good frame pairs are found."
