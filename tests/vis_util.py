"""Shared by tests/test_visualization_cpu.py and tests/test_visualization_gpu.py: the reference's preview formula restated in numpy
(pinned to the reference's own output by the CPU tests, used as the yardstick where the GPU box has no reference) and golden access."""
import os

import numpy as np

from conftest import GOLDEN


def golden(name="vis_reference.npz"):
    with np.load(os.path.join(GOLDEN, name)) as z:
        return {k: z[k] for k in z.files}


def preview_indices(depth, dmin, dmax):
    """uint8(sqrt((d - dmin) / (dmax - dmin)) * 255) as the reference's x86 host computes it: float32 steps, then the low byte of the
    int32 truncation, 0 for NaN and for values outside int32."""
    d, lo, hi = np.asarray(depth, np.float32), np.float32(dmin), np.float32(dmax)
    with np.errstate(all="ignore"):
        v = np.sqrt((d - lo) / (hi - lo)) * np.float32(255)
        ok = np.abs(v) < np.float32(2 ** 31)           # False for NaN
        return np.where(ok, np.trunc(np.where(ok, v, 0)).astype(np.int64) & 255, 0).astype(np.uint8)


def preview_pixels(depth, dmin, dmax, table):
    """table: (256, 3) in the channel order wanted."""
    return np.asarray(table)[preview_indices(depth, dmin, dmax)]


def ulp_distance(a, b):
    """Distance of two float32 values in units of the last place (adjacent floats are 1 apart; the same value is 0)."""
    def key(x):
        i = int(np.float32(x).view(np.int32))
        return i if i >= 0 else -(i & 0x7fffffff)
    return abs(key(a) - key(b))


def read_png(path):
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im.convert("RGB"))
