#!/usr/bin/env python3
"""BUILD CONTAINER ONLY.  Writes tests/golden/vis_reference.npz and tests/golden/vis_loop_6f_64x48.npz: what the reference's OWN
utils/visualization.py and depth_fine_tuning.py hand to cv2.imwrite, recorded by importing the reference unmodified (oracle/ref_loop.py)
with a `cv2` stub whose `applyColorMap` is a table gather and whose `imwrite` records `rint` of its argument (OpenCV rounds to
nearest-even when it converts a float image to 8 bits).  `imread` is never called.  Pixel arrays are B,G,R, as the reference builds them.

    python tools/gen_golden_visualization.py

vis_reference.npz: the final 256 x 3 table; `visualize_depth` on small planes, in range and out of range (the out-of-range indices are
data of the x86 host the file was made on); `visualize_depth_dir` on a 6-frame directory with NaN pixels, an all-NaN frame and a
stale file of another size, at percentiles 0 / 100 and 0 / 99.  vis_loop_6f_64x48.npz: the eval/ and depth/ PNG pixels of one epoch
of the reference's loop on the clip of oracle/gen_golden_loop.py (native fp32), next to the `.raw` planes they were rendered from.
"""
import contextlib
import glob
import os
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

GOLDEN = os.path.join(REPO, "tests", "golden")
SEED = 11
LOOP_EPOCHS = 1


@contextlib.contextmanager
def recording_stub():
    """oracle/ref_loop.py's stub set with the recording cv2 in place of its no-op one.  Yields {path: uint8 B,G,R image}."""
    from oracle import ref_loop
    written = {}
    plain = ref_loop._stub_modules

    def stubs(dtype):
        s = plain(dtype)
        s["cv2"].applyColorMap = lambda img, cm: np.asarray(cm).reshape(256, 3)[np.asarray(img)]
        s["cv2"].imwrite = lambda path, img, *a: written.__setitem__(path, np.rint(np.asarray(img)).astype(np.uint8)) or True
        return s
    ref_loop._stub_modules = stubs
    try:
        yield written
    finally:
        ref_loop._stub_modules = plain


@contextlib.contextmanager
def recording_reference():
    """The reference importable as top-level packages, with the recording stub, for the duration of the block."""
    import torch
    from oracle import ref_loop
    with recording_stub() as written, ref_loop.reference_modules(torch.float32):
        yield written


def plane_cases(rng):
    """[(name, plane, dmin, dmax)]: the inputs of the `visualize_depth` goldens."""
    cases = []
    ramp = (((np.arange(256) + 0.5) / 255) ** 2).astype(np.float32).reshape(16, 16)
    cases.append(("ramp", ramp, np.float32(0), np.float32(1)))                       # index i at position i: reads the table out
    a = rng.uniform(0.05, 3.0, (37, 53)).astype(np.float32)
    cases.append(("odd_37x53", a, np.float32(0), a.max()))
    cases.append(("odd_37x53_inner", a, np.float32(0.5), np.float32(2.0)))           # below dmin (sqrt of a negative) and above dmax
    b = rng.uniform(0.0, 1.0, (24, 20)).astype(np.float32)
    b.flat[:12] = [np.nan, np.inf, -np.inf, -1.0, -0.0, 0.0, (280.5 / 255) ** 2, 4.0, (4416.73 / 255) ** 2, 1e30, 3e38, 1.0]
    cases.append(("wrap", b, np.float32(0), np.float32(1)))
    cases.append(("wrap_huge_scale", (b * np.float32(1e30)).astype(np.float32), np.float32(0), np.float32(1e-8)))
    cases.append(("flat", np.full((8, 12), 0.75, np.float32), np.float32(0.75), np.float32(0.75)))      # dmax == dmin: 0 / 0
    cases.append(("flat_mixed", b, np.float32(0.25), np.float32(0.25)))                                # x / 0: +-inf and NaN
    cases.append(("nan_max", b, np.float32(0), np.float32(np.nan)))
    c = rng.uniform(0.2, 1.5, (5, 7)).astype(np.float32)
    cases.append(("auto_range", c, None, None))                                                       # np.amin / np.amax
    return cases


def directory_case(rng):
    """{file name: plane}: 6 frames of 24 x 20 with NaN pixels, one of them all NaN, and a stale file of another size."""
    files = {}
    for i in range(6):
        p = rng.uniform(0.1 + 0.05 * i, 2.0 + 0.3 * i, (24, 20)).astype(np.float32)
        p[rng.random(p.shape) > 0.8] = np.nan
        if i == 1:
            p[3, 4] = np.inf                       # not finite: takes no part in the range
        if i == 2:
            p[0, :2] = 40.0                        # a few outliers: 0 / 99 cuts them off, 0 / 100 does not
        if i == 4:
            p[:] = np.nan
        files[f"frame_{i:06d}.raw"] = p
    files["frame_000099.raw"] = rng.uniform(0.02, 5.0, (10, 12)).astype(np.float32)     # left over from an earlier run
    return files


def reference_outputs():
    out = {}
    rng = np.random.default_rng(SEED)
    with recording_reference() as written:
        from utils import image_io as ref_io, visualization as ref_vis
        with np.errstate(all="ignore"):
            names = []
            for name, plane, lo, hi in plane_cases(rng):
                names.append(name)
                out[f"vd_{name}_in"] = plane
                out[f"vd_{name}_range"] = np.array([np.nan if lo is None else lo, np.nan if hi is None else hi], np.float32)
                out[f"vd_{name}_auto"] = np.array(lo is None)
                out[f"vd_{name}_out"] = np.rint(ref_vis.visualize_depth(plane, lo, hi)).astype(np.uint8)
            out["vd_names"] = np.array(names)
            ramp = out["vd_ramp_out"].reshape(256, 3)
            out["table_bgr"] = ramp
            files = directory_case(rng)
            out["dir_names"] = np.array(list(files))
            for (lo, hi) in ((0, 100), (0, 99)):
                tmp = tempfile.mkdtemp()
                for name, plane in files.items():
                    ref_io.save_raw_float32_image(os.path.join(tmp, name), plane)
                written.clear()
                with contextlib.redirect_stdout(open(os.devnull, "w")):
                    ref_vis.visualize_depth_dir(tmp, tmp, force=True, min_percentile=lo, max_percentile=hi)
                assert sorted(os.path.basename(p) for p in written) == sorted(os.path.splitext(n)[0] + ".png" for n in files)
                for k, name in enumerate(files):
                    out[f"dir_in_{k}"] = files[name]
                    out[f"dir_out_{lo}_{hi}_{k}"] = written[os.path.join(tmp, os.path.splitext(name)[0] + ".png")]
    return out


def loop_outputs():
    """One epoch of the reference's loop (native fp32) + save_depth with the recording cv2."""
    import make_synthetic_dataset as msd
    import torch
    from consistent_depth_amd.utils import image_io
    from oracle import gen_golden_loop as G, ref_loop
    tmp = tempfile.mkdtemp()
    clip = os.path.join(tmp, "clip")
    range_dir, _ = msd.write_dataset(clip, **G.CLIP)
    with recording_stub() as written:      # (ref_loop.run enters reference_modules itself)
        run = ref_loop.run(clip, range_dir, list(range(G.CLIP["n_frames"])), G.initial_state(), os.path.join(tmp, "work"), dtype=torch.float32,
                           num_epochs=LOOP_EPOCHS, seed=G.LOOP_SEED)
    # the frames of the validation sweep's first batch (4 pairs): their maximum inverse depth is the scale of every eval/ preview
    out = {"epochs": np.array(LOOP_EPOCHS), "first_batch_frames": np.array(sorted({f for pair in run["flow_indices"][:4] for f in pair}))}
    names = []
    for path in sorted(written):
        rel = os.path.relpath(path, run["out_dir"])
        raw = os.path.splitext(path)[0] + ".raw"
        assert os.path.exists(raw), raw
        names.append(rel)
        out[f"png_{len(names) - 1}"] = written[path]
        out[f"raw_{len(names) - 1}"] = image_io.load_raw_float32_image(raw)
    out["names"] = np.array(names)
    assert len(names) == (LOOP_EPOCHS + 1) * G.CLIP["n_frames"] + G.CLIP["n_frames"], names
    return out


def main():
    for name, fn in (("vis_reference.npz", reference_outputs), ("vis_loop_6f_64x48.npz", loop_outputs)):
        dst = os.path.join(GOLDEN, name)
        np.savez_compressed(dst, **fn())
        print("wrote", dst, os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    main()
