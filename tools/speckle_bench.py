"""Speckle filter timing (GPU): asw_speckle on four inputs at C4 (1920x1080) and C5 (3840x2160),
and the whole frame with the filter off and on in one session.

    python tools/speckle_bench.py [--warmup 3] [--reps 20] [--small] [--no-frame] [--out FILE]

Inputs: (a) the LR-masked d_ref of a synthetic pair's frame (SGM on the census cost, D 64: the
map depends on the image size alone, not on the aggregator's cost), (b) a checkerboard (S
components), (c) a constant map (one component of S pixels), (d) the serpentine of
tests/speckle_ref.py (one corridor through every row).  One process, HIP events around every
asw_speckle call (its memset and four launches), ``--warmup`` untimed and ``--reps`` timed calls each;
prints one JSON line (medians and minima in ms) and writes it to ``--out`` when given.  The frame
is ``FrameContext.match`` at C4 (D 256, T 35, r 7), timed by asw_timings.total.  ``--small`` runs
320x240 (a functional check).
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import speckle_ref as SK  # noqa: E402
from stereo_matchin_amd import FrameContext, default_speckle_params, make_params  # noqa: E402
from stereo_matchin_amd import kernels as K  # noqa: E402
from stereo_matchin_amd.synthetic import make_pair  # noqa: E402


def timed(fn, warmup, reps):
    ts = []
    for r in range(warmup + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if r >= warmup:
            ts.append(e0.elapsed_time(e1))
    return {"ms_median": round(float(np.median(ts)), 4), "ms_min": round(min(ts), 4)}


def frame_map(W, H, D=64):
    """(d_ref int32, valid uint8) of a synthetic pair's frame: SGM on the census cost, LR check."""
    Lh, Rh, _ = make_pair(W, H, D, 0)
    with FrameContext(make_params(W, H, ndisp=D, taps=35, iters=7), sgm=True, census=True) as fc:
        out = fc.match(Lh, Rh, want16=True)
    return out["d_ref"], (out["lr16"] != 0xFFFF).astype(np.uint8)


def stage_times(W, H, a, dev):
    p = make_params(W, H, ndisp=64)
    sp = default_speckle_params()
    ws = K.speckle_workspace(p, dev)
    d_frame, v_frame = frame_map(W, H)
    cases = {"a_frame_lr_masked": (d_frame, v_frame), "b_checker": SK.checker(H, W),
             "c_one_component": (np.zeros((H, W), np.int32), None), "d_serpentine": SK.serpentine(H, W)}
    out = {}
    for name, (d, valid) in cases.items():
        dd = torch.from_numpy(np.ascontiguousarray(d)).to(dev)
        vv = None if valid is None else torch.from_numpy(valid).to(dev)
        t = timed(lambda: K.speckle(p, sp, dd, vv, workspace=ws), a.warmup, a.reps)
        _, size, keep, status = K.speckle(p, sp, dd, vv, workspace=ws, return_status=True)
        t.update(status=status, kept_share=round(float(keep.float().mean()), 4), largest=int(size.max()))
        out[name] = t
    return out


def frame_times(a):
    W, H, D, T, r = (320, 240, 64, 35, 7) if a.small else (1920, 1080, 256, 35, 7)
    Lh, Rh, _ = make_pair(W, H, D, 0)
    out = {"shape": {"W": W, "H": H, "D": D, "T": T, "iters": r}}
    for name, speckle in (("off", None), ("on", True), ("off_again", None)):
        with FrameContext(make_params(W, H, ndisp=D, taps=T, iters=r), speckle=speckle) as fc:
            ts = [fc.match(Lh, Rh)["timings"]["total"] for _ in range(a.warmup + a.reps)][a.warmup:]
        out[name] = {"ms_median": round(float(np.median(ts)), 4), "ms_min": round(min(ts), 4)}
    out["on_minus_off_ms"] = round(out["on"]["ms_median"] - out["off"]["ms_median"], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--small", action="store_true", help="320x240 only")
    ap.add_argument("--no-frame", action="store_true", help="the stage times only")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {"warmup": a.warmup, "reps": a.reps, "device": torch.cuda.get_device_name(dev),
           "speckle": {"min_size": 32, "max_diff": 1}}
    for name, (W, H) in ({"small": (320, 240)} if a.small else {"c4": (1920, 1080), "c5": (3840, 2160)}).items():
        out[name] = dict(stage_times(W, H, a, dev), shape={"W": W, "H": H})
    if not a.no_frame:
        out["frame"] = frame_times(a)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
