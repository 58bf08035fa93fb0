"""Census cost timing (GPU): the AD raw cost against the census transform and cost, and
the whole frame with census off and on, at C4 (1920x1080, D 256, T 35, r 7).

    python tools/census_bench.py [--warmup 3] [--reps 20] [--small]

One process, HIP events around every launch (the whole ``StereoMatcher.match`` for the
two frames), ``--warmup`` untimed and ``--reps`` timed launches each; prints one JSON line
(medians and minima in ms).  ``--small`` runs 320x240, D 64 (a functional check).
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from stereo_matchin_amd import StereoMatcher, default_census_params, make_params  # noqa: E402
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--small", action="store_true", help="320x240, D 64")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    W, H, D, T, r = (320, 240, 64, 35, 7) if a.small else (1920, 1080, 256, 35, 7)
    Lh, Rh, _ = make_pair(W, H, D, 0)
    p = make_params(W, H, ndisp=D, taps=T, iters=r)
    cp = default_census_params()
    L, R = torch.from_numpy(Lh).to(dev), torch.from_numpy(Rh).to(dev)
    c16 = torch.empty(K.cost_shape(p), dtype=torch.int16, device=dev)
    cl, cr = K.census(p, cp, L), K.census(p, cp, R)
    out = {"shape": {"W": W, "H": H, "D": D, "T": T, "iters": r}, "warmup": a.warmup, "reps": a.reps,
           "census": {"win_w": cp.win_w, "win_h": cp.win_h, "ad_weight": cp.ad_weight,
                      "census_weight": cp.census_weight},
           "device": torch.cuda.get_device_name(dev)}
    out["asw_raw_cost16"] = timed(lambda: K.asw_Aggr16(p, L, R, out=c16), a.warmup, a.reps)
    out["asw_census"] = timed(lambda: K.census(p, cp, L, out=cl), a.warmup, a.reps)
    out["asw_census_cost16"] = timed(lambda: K.census_cost16(p, cp, L, R, cl, cr, out=c16), a.warmup, a.reps)
    del c16
    for name, census in (("match_census_off", None), ("match_census_on", cp)):
        m = StereoMatcher(p, dev, census=census)
        out[name] = timed(lambda: m.match(L, R), a.warmup, a.reps)
        del m
    out["census_cost16_over_raw_cost16"] = round(out["asw_census_cost16"]["ms_median"] /
                                                 out["asw_raw_cost16"]["ms_median"], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
