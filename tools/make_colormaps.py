#!/usr/bin/env python
"""Write gscream_amd/colormaps.json: the two 256-entry byte tables gscream_amd.frames colours depth with (RGB), as text: per table,
rows of 16 colours as "rrggbb" hex digits (gscream_amd.frames.load_colormaps reads them back as uint8 [2, 256, 3]).

    python tools/make_colormaps.py [--check]

Both come from the installed matplotlib's listed colours (256 fp64 RGB triples each):
    [0] inferno   round(255 c): what OpenCV's table-to-bytes conversion does to the same listed colours (COLORMAP_INFERNO, as RGB).
                  Not pinned by a run of cv2 (it is not on this stack); the closest any 255 c comes to a rounding tie is printed.
    [1] viridis   trunc(255 c): the bytes plt.imsave(cmap="viridis") writes, (lut * 255).astype(uint8); pinned by tests/golden/ref_frames.npz.
--check compares the committed file with what this would write and changes nothing."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(ROOT, "gscream_amd", "colormaps.json")
NAMES = ("inferno", "viridis")


def listed(name):
    import matplotlib
    c = np.asarray(matplotlib.colormaps[name].colors, dtype=np.float64)
    assert c.shape == (256, 3) and c.min() >= 0.0 and c.max() <= 1.0
    return c


def tables():
    inferno, viridis = listed("inferno") * 255.0, listed("viridis") * 255.0
    tie = np.abs(inferno - np.floor(inferno) - 0.5).min()
    return np.stack([np.floor(inferno + 0.5).astype(np.uint8), viridis.astype(np.uint8)]), tie


def main():
    import matplotlib
    lut, tie = tables()
    print(f"matplotlib {matplotlib.__version__}: inferno's 255 c comes no closer than {tie:.3g} to a rounding tie")
    if "--check" in sys.argv:
        sys.path.insert(0, ROOT)
        from gscream_amd.frames import load_colormaps
        same = np.array_equal(load_colormaps(), lut)
        print(PATH, "matches" if same else "DIFFERS")
        sys.exit(0 if same else 1)
    with open(PATH, "w") as f:
        f.write("{\n")
        for k, name in enumerate(NAMES):
            rows = [lut[k, r:r + 16].tobytes().hex() for r in range(0, 256, 16)]
            f.write(f' "{name}": [\n' + ",\n".join(f'  "{row}"' for row in rows) + "\n ]" + ("," if k == 0 else "") + "\n")
        f.write("}\n")
    print(PATH, os.path.getsize(PATH), "bytes")


if __name__ == "__main__":
    main()
