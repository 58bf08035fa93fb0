"""asw_timings.refine of the refinement loops through the frame API (asw_match), on one GPU.

C4 (1920x1080, D 256, T 35, r 7): the 8-bit loop (ASW_LR_U8, asw_set_refine) and the native
loop (ASW_LR_NATIVE, asw_set_refine_native) on the same synthetic pair, in two contexts
matched alternately in one process, so both see the same box at the same time.
C5 (3840x2160, D 512, T 51, r 7): the native loop (the 8-bit one is not built for D 512).
Each prints one JSON line: the median, minimum and maximum of `refine` (HIP events around
the loop and the median, asw_frame.cpp) and of `total` over the timed frames.

    python tools/refine_bench.py [--k 6] [--frames 8] [--warmup 2] [--skip-c5]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from stereo_matchin_amd import FrameContext, _lib, make_params  # noqa: E402
from stereo_matchin_amd.synthetic import make_pair  # noqa: E402


def stats(xs):
    return {"median_ms": round(float(np.median(xs)), 4), "min_ms": round(float(np.min(xs)), 4),
            "max_ms": round(float(np.max(xs)), 4), "frames": len(xs)}


def run(name, W, H, D, T, modes, k, frames, warmup):
    Lh, Rh, _ = make_pair(W, H, D, 0)
    rp = _lib.default_refine_params(iters=k)
    ctxs = {m: FrameContext(make_params(W, H, ndisp=D, taps=T, iters=7, lr_mode=lr), refine=rp)
            for m, lr in modes.items()}
    times = {m: {"refine": [], "total": []} for m in ctxs}
    try:
        for i in range(warmup + frames):
            for m, fc in ctxs.items():  # alternating
                t = fc.match(Lh, Rh)["timings"]
                if i >= warmup:
                    times[m]["refine"].append(t["refine"])
                    times[m]["total"].append(t["total"])
    finally:
        for fc in ctxs.values():
            fc.close()
    for m in ctxs:
        print(json.dumps({"workload": name, "shape": [W, H, D, T], "loop": m, "k": k,
                          "native": ctxs[m].refine_native is not None, "refine": stats(times[m]["refine"]),
                          "total": stats(times[m]["total"])}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=6)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--skip-c5", action="store_true")
    a = ap.parse_args()
    run("c4", 1920, 1080, 256, 35, {"u8": _lib.LR_U8, "native": _lib.LR_NATIVE}, a.k, a.frames, a.warmup)
    if not a.skip_c5:
        run("c5", 3840, 2160, 512, 51, {"native": _lib.LR_NATIVE}, a.k, a.frames, a.warmup)


if __name__ == "__main__":
    main()
