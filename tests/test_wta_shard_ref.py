"""The numpy restatement of the WTA stage functions (tests/wta_shard_ref.py) against the
C oracle (oracle_wta, oracle_wta_ref: the reference's loops, pinned to its images in
test_oracle_golden.py), bit for bit, on the well volumes (no GPU).

tests/test_gpu_wta_shard.py compares the HIP stage kernels with this restatement; what is
checked here is that a disagreement there is the device's.  The inputs are asserted to
separate the rules (shares of the pixels computed from the reference results): a
restatement with `<=` for `<`, with `second` always offering m1, or without the
max(x - i, 0) clamp fails these tests.
"""
import numpy as np
import pytest

import wta_shard_ref as R
from wta_shard_ref import CASES, case_id, shard_case

SHAPES = sorted({c[:3] for c in CASES} | {(61, 5, 67), (300, 3, 200), (256, 13, 129)})


def _eq(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


@pytest.mark.parametrize("D,H,W", SHAPES)
def test_whole_volume_forms_equal_oracle(oracle, D, H, W):
    seed = R.case_seed(D, H, W)
    C = R.well_volume(D, H, W, seed)
    ref_l, ref_r = R.refine_estimates(H, W, D, seed + 1)
    for name, got, want in zip(("d_ref", "conf_ref", "d_tar", "conf_tar"), R.wta(C), oracle.wta(C)):
        assert _eq(got, want), name
    for name, got, want in zip(("d_ref", "d_tar", "conf_ref"), R.wta_ref(C, ref_l, ref_r),
                               oracle.wta_ref(C, ref_l, ref_r)):
        assert _eq(got, want), name
    # ... and on the volume kind of the older tests (few levels, ties everywhere)
    rng = np.random.default_rng(seed)
    L = np.ascontiguousarray(rng.integers(1, 9, (D, H, W)).astype(np.float32))
    for name, got, want in zip(("d_ref", "conf_ref", "d_tar", "conf_tar"), R.wta(L), oracle.wta(L)):
        assert _eq(got, want), name


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_shard_ops_equal_oracle(oracle, case):
    c = shard_case(*case)
    c.assert_conditions()
    for name, got, want in zip(("d_ref", "conf_ref", "d_tar", "conf_tar"), c.final, oracle.wta(c.C)):
        assert _eq(got, want), name
    for name, got, want in zip(("d_ref", "d_tar", "conf_ref"), c.rfinal, oracle.wta_ref(c.C, c.ref_l, c.ref_r)):
        assert _eq(got, want), name


def test_well_volume_recipe():
    C = R.well_volume(70, 7, 20, 3)
    assert C.dtype == np.float32 and C.shape == (70, 7, 20)
    assert np.array_equal(C * 4, np.round(C * 4))  # multiples of 0.25: exact ties
    assert (C[:, 0, :3] == 5.0).all() and (C[:, 1, 0] == 100000.0).all() and (C[:, 1, 1] == 250000.0).all()
    body = C[:, 2:]
    assert body.min() >= 0.25 and body.max() <= 2.25
    wells = (body == body.min(axis=0)).sum(axis=0)
    assert set(np.unique(wells)) == {1, 2} and 0.15 <= np.mean(wells == 2) <= 0.45
    assert R.well_volume(9, 5, 1, 1).shape == (9, 5, 1)  # W = 1: the fixed pixels fit
    ref_l, ref_r = R.refine_estimates(7, 20, 70, 4)
    assert ref_l.shape == ref_r.shape == (2, 7, 20) and ref_l.dtype == np.float32
    assert set(np.unique(ref_l[1])) <= {np.float32(v) for v in (0, 1e-5, 0.5, 1, 4, 64, 3e7)}
    assert ref_l[0].min() >= -2.0 and ref_l[0].max() < 72.0 and not np.array_equal(ref_l, ref_r)
