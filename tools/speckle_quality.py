"""The quality table of DESIGN.md §Speckle: the bad-pixel rate among the pixels the speckle filter
keeps against the rate among all of them (CPU: tests/census_ref.py's default cost, tests/sgm_ref.py
at its defaults, a first-argmin, tests/speckle_ref.py at its defaults) on the three synthetic pairs
of tests/test_sgm.py, unchanged and with a gain / offset on the right image; every pixel valid, and
valid where the left-right check passes (tests/wta_shard_ref.py's WTA of both views and
tests/subpixel_ref.py's rule on the 8-bit codes).

    python tools/speckle_quality.py [--min-size 32] [--max-diff 1]      # markdown rows on stdout
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import census_ref as CR  # noqa: E402
import sgm_ref as SG  # noqa: E402
import speckle_ref as SK  # noqa: E402
import subpixel_ref as SR  # noqa: E402
import wta_shard_ref as WR  # noqa: E402
from stereo_matchin_amd.synthetic import make_pair  # noqa: E402

PAIRS = [(160, 96, 32, 7), (128, 64, 24, 3), (192, 64, 32, 5)]


def code_u8(d, D):
    """The 8-bit code of a disparity index (code_u8 of asw_common.h)."""
    return np.clip((510 * d.astype(np.int64) + (D - 2)) // (2 * (D - 1)), 0, 255).astype(np.uint8)


def rates(d, gt, D, valid, min_size, max_diff):
    """(bad rate among the valid pixels, among the kept ones, kept share of the valid ones), x >= D."""
    keep = SK.components(d, valid, min_size, max_diff)[2][:, D:] != 0
    ok = np.ones(keep.shape, bool) if valid is None else valid[:, D:] != 0
    bad = (np.abs(d.astype(np.int64) - gt) > 1)[:, D:]
    return float(bad[ok].mean()), float(bad[keep].mean()), float(keep.sum() / ok.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--min-size", type=int, default=SK.DEFAULT["min_size"])
    ap.add_argument("--max-diff", type=int, default=SK.DEFAULT["max_diff"])
    a = ap.parse_args()
    print("| pair | right image | valid | before | after | kept share |")
    print("|---|---|---|---|---|---|")
    for W, H, D, seed in PAIRS:
        L, R, gt = make_pair(W, H, D, seed)
        for label, Rv in (("unchanged", R), ("0.7 R + 40", CR.gain_offset(R))):
            S = SG.sgm(CR.cost_u16(L, Rv, D), **SG.DEFAULT)
            d = SG.first_argmin(S)
            d_ref, _, d_tar, _ = WR.wta(S.astype(np.float32))
            assert np.array_equal(d_ref, d)
            lr = SR.lr_pass(d_ref, d_tar, code_u8(d_ref, D), code_u8(d_tar, D), D, 0).astype(np.uint8)
            for name, valid in (("every pixel", None), ("LR check", lr)):
                b, k, s = rates(d, gt, D, valid, a.min_size, a.max_diff)
                print(f"| ({W}, {H}, {D}, {seed}) | {label} | {name} | {b:.3f} | {k:.3f} | {s:.3f} |")


if __name__ == "__main__":
    main()
