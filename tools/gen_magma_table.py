"""Generates consistent_depth_amd/utils/magma_gamma22_u8.txt, the 256 x 3 byte table of the depth previews (R G B per line), from
matplotlib's `magma` and the formula of consistent_depth_amd/utils/visualization.py:

    entry = rint(((uint8(magma(i) * 255) / 255) ** 2.2) * 255)           i = 0..255, float64, round half to even

The product never imports matplotlib: the table is committed data.  `--check` regenerates and compares without writing.

    python tools/gen_magma_table.py [--check]
"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(REPO, "consistent_depth_amd", "utils", "magma_gamma22_u8.txt")


def magma_u8() -> np.ndarray:
    """matplotlib's 256 magma colours as truncated bytes, (256, 3) R,G,B."""
    import matplotlib
    colors = np.asarray(matplotlib.colormaps["magma"].colors, dtype=np.float64)
    assert colors.shape == (256, 3)
    return (colors * 255).astype(np.uint8)


def generate() -> np.ndarray:
    sys.path.insert(0, REPO)
    from consistent_depth_amd.utils.visualization import gamma_table
    return gamma_table(magma_u8())


def write(path: str = TABLE) -> None:
    np.savetxt(path, generate(), fmt="%d", header="depth preview table: rint(((uint8(magma * 255) / 255) ** 2.2) * 255), one 'R G B' line per index "
               "(tools/gen_magma_table.py)")


if __name__ == "__main__":
    if "--check" in sys.argv:
        have = np.loadtxt(TABLE, dtype=np.uint8)
        ok = np.array_equal(have, generate())
        print("table matches" if ok else "table DIFFERS")
        sys.exit(0 if ok else 1)
    write()
    print("wrote", TABLE)
