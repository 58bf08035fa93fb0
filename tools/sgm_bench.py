"""Semi-global matching timing (GPU): every asw_sgm_path, asw_sgm at 4 and 8 paths, and the
whole frame with SGM off and on in one session, at C4 (1920x1080, D 256, T 35, r 7) on the
default census cost.

    python tools/sgm_bench.py [--warmup 3] [--reps 20] [--small] [--out FILE]

One process, HIP events around every launch (the whole ``StereoMatcher.match`` for the
frames), ``--warmup`` untimed and ``--reps`` timed launches each; prints one JSON line (medians
and minima in ms, the bytes each launch must move by the layout and the TB/s that implies) and
writes it to ``--out`` when given.  ``--small`` runs 320x240, D 64 (a functional check).
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from stereo_matchin_amd import StereoMatcher, default_census_params, default_sgm_params, make_params  # noqa: E402
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


def with_traffic(t, nbytes):
    t["bytes"] = int(nbytes)
    t["tb_per_s"] = round(nbytes / (t["ms_median"] * 1e-3) / 1e12, 3)
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--small", action="store_true", help="320x240, D 64")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    W, H, D, T, r = (320, 240, 64, 35, 7) if a.small else (1920, 1080, 256, 35, 7)
    Lh, Rh, _ = make_pair(W, H, D, 0)
    p = make_params(W, H, ndisp=D, taps=T, iters=r)
    cp = default_census_params()
    L, R = torch.from_numpy(Lh).to(dev), torch.from_numpy(Rh).to(dev)
    cl, cr = K.census(p, cp, L), K.census(p, cp, R)
    c16 = K.census_cost16(p, cp, L, R, cl, cr)
    S = torch.zeros(K.cost_shape(p), dtype=torch.float32, device=dev)
    Dp = K.cost_shape(p)[2]
    cost_bytes, sum_bytes = W * H * Dp * 2, W * H * Dp * 4
    out = {"shape": {"W": W, "H": H, "D": D, "T": T, "iters": r}, "warmup": a.warmup, "reps": a.reps,
           "census": {"win_w": cp.win_w, "win_h": cp.win_h, "ad_weight": cp.ad_weight,
                      "census_weight": cp.census_weight},
           "device": torch.cuda.get_device_name(dev), "cost16_bytes": cost_bytes, "sum_bytes": sum_bytes}
    sp = default_sgm_params()
    for k in range(8):  # a path that writes reads C and writes S; one that accumulates also reads S
        out[f"asw_sgm_path_{k}_write"] = with_traffic(
            timed(lambda: K.sgm_path(p, sp, k, c16, out=S), a.warmup, a.reps), cost_bytes + sum_bytes)
        out[f"asw_sgm_path_{k}_accumulate"] = with_traffic(
            timed(lambda: K.sgm_path(p, sp, k, c16, out=S, accumulate=True), a.warmup, a.reps),
            cost_bytes + 2 * sum_bytes)
        S.zero_()  # keep the sums exact integers below 2^24
    for n in (4, 8):
        spn = default_sgm_params(paths=n)
        out[f"asw_sgm_{n}"] = with_traffic(timed(lambda: K.sgm(p, spn, c16, out=S), a.warmup, a.reps),
                                           n * cost_bytes + (2 * n - 1) * sum_bytes)
    del c16, S
    for name, census, sgm in (("match_asw_ad", None, None), ("match_sgm_off", cp, None), ("match_sgm_on", cp, sp)):
        m = StereoMatcher(p, dev, census=census, sgm=sgm)
        out[name] = timed(lambda: m.match(L, R), a.warmup, a.reps)
        del m
    out["sgm_frame_over_asw_frame"] = round(out["match_sgm_on"]["ms_median"] / out["match_sgm_off"]["ms_median"], 3)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
