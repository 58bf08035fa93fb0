"""Generate the cross-based matcher's golden fixtures from the reference's own data files.

    python tests/golden/make_golden_cross.py [REFERENCE_DIR/stereo_matching]

(the directory may also come from the environment variable STEREO_REFERENCE).  For each
scene of the reference's pics.txt it stores, in ``tests/golden/cross_<scene>.npz``:

* ``initial``: the device-produced ``cross_based_initial.png`` (main.cpp:357-359), the
  image Init_disparity writes, as uint8 [H][W] grey values;
* ``final``: ``cross_based_disparity.png`` (main.cpp:361-363), the 3x3 median of the
  Disparity vote, likewise;
* ``source``: the two paths.

The PNGs are decoded through RGBA and channel 0 is kept: art's
cross_based_disparity.png is a palette PNG, whose raw samples are palette indices and not
grey values.  Every image is grey (R = G = B, checked).  The inputs of a scene are the
``left`` / ``right`` arrays of the existing ``<scene>.npz`` (make_golden.py).

These are data (expected outputs), not reference source.  PNG decoding uses PIL, which is
only needed to regenerate the fixtures.
"""
from __future__ import annotations

import os
import sys

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))


def main(argv) -> int:
    from PIL import Image

    ref = argv[1] if len(argv) > 1 else os.environ.get("STEREO_REFERENCE", "")
    if not os.path.isdir(ref):
        print("usage: make_golden_cross.py REFERENCE_DIR/stereo_matching", file=sys.stderr)
        return 1
    with open(os.path.join(ref, "pics.txt")) as f:
        lines = [ln.strip() for ln in f if ln.strip()]
    for lp in lines[0::2]:
        scene = lp.split("/")[0]
        grey = {}
        for key, name in (("initial", "cross_based_initial.png"), ("final", "cross_based_disparity.png")):
            rgba = np.array(Image.open(os.path.join(ref, scene, name)).convert("RGBA"))
            assert (rgba[..., 0] == rgba[..., 1]).all() and (rgba[..., 1] == rgba[..., 2]).all(), (scene, name)
            grey[key] = np.ascontiguousarray(rgba[..., 0])
        pair = np.load(os.path.join(OUT, f"{scene}.npz"))
        assert grey["initial"].shape == grey["final"].shape == pair["left"].shape[:2], scene
        np.savez_compressed(os.path.join(OUT, f"cross_{scene}.npz"), initial=grey["initial"], final=grey["final"],
                            source=np.array(f"{scene}/cross_based_initial.png {scene}/cross_based_disparity.png"))
        print(scene, grey["initial"].shape, len(np.unique(grey["initial"])), len(np.unique(grey["final"])))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
