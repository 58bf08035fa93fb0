"""The cones of tests/far_ref.py, proven on the CPU: for every stage function, at small
shapes, reference(cone)[crop] == reference(whole problem)[crop] bit for bit, at the first
rows, an interior band and the last rows.  The whole-problem reference is the same function
on the region of every row (its cone is then the whole input, handed to the reference module
as it is).  Negative controls: a cone one row or one column too small on its upstream side
must differ, for every stage that recurs along a line (the two integrals, the eight SGM
paths) and for the window stages whose window is the cone.  No tolerance anywhere.
"""
import functools

import numpy as np
import pytest

import far_ref as F

SHAPES = [(19, 23, 7), (40, 31, 12), (8, 33, 6)]  # (W, H, D); W = 8: the diagonal cones are 7 rows
TAPS = 5
ARM_MAX, TAU = 3, 60


def bands_of(H):
    return [(0, 2), (H // 2 - 1, H // 2 + 2), (H - 2, H)]


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return a.tobytes() == b.tobytes()  # bit patterns: NaNs and signed zeros included


@functools.lru_cache(maxsize=None)
def inputs(W, H, D):
    r = np.random.default_rng(1000 * W + H)
    # blocky images: arms, supports and census codes with structure, not noise alone
    def img():
        base = r.integers(0, 256, (H // 4 + 1, W // 4 + 1, 4), dtype=np.uint8).repeat(4, 0).repeat(4, 1)[:H, :W]
        return np.ascontiguousarray(np.clip(base.astype(np.int32) + r.integers(-20, 21, (H, W, 4)), 0, 255)
                                    .astype(np.uint8))
    z = {"L": img(), "R": img()}
    Dp = 16
    # quarter steps: exact ties for the first-argmin and second-minimum rules
    z["C"] = (r.integers(0, 2800, (H, W, Dp)).astype(np.float32) / np.float32(4.0))
    z["C16"] = r.integers(0, 765, (H, W, Dp)).astype(np.uint16)
    z["sL"] = r.random((H, W, 12), dtype=np.float32)
    z["sR"] = r.random((H, W, 12), dtype=np.float32)
    z["conf_ref"] = r.random((H, W), dtype=np.float32)
    z["conf_tar"] = r.random((H, W), dtype=np.float32)
    z["est"] = r.integers(0, D, (H, W)).astype(np.int32)
    z["d_tar"] = np.clip(z["est"] + r.integers(-2, 3, (H, W)), 0, D - 1).astype(np.int32)
    z["ref_l"] = np.stack([r.random((H, W), dtype=np.float32) * np.float32(D), r.random((H, W), dtype=np.float32)])
    z["ref_r"] = np.stack([r.random((H, W), dtype=np.float32) * np.float32(D), r.random((H, W), dtype=np.float32)])
    disp = r.random((H, W), dtype=np.float32) * np.float32(D)
    disp[r.random((H, W)) < 0.4] = np.nan
    disp[H // 2] = np.nan  # a row without a valid pixel
    z["disp_lr"] = disp
    for a in z.values():
        a.setflags(write=False)
    return z


@functools.lru_cache(maxsize=None)
def stages(W, H, D):
    """name -> fn(y0, y1, trim): every far_ref stage function that takes a row region."""
    z = inputs(W, H, D)
    L, R, C, C16 = z["L"], z["R"], z["C"], z["C16"]
    b, e = D // 3, D - 1  # a shard
    Cl = C[:, :, b:e]
    key = F.wta_local(C, 0, D, D, 0, H)[0]
    key_l, m1, m2 = F.wta_local(Cl, b, e, D, 0, H)
    tkey, t1, t2 = F.wta_target_local(C, key, 0, D, D, 0, H)
    nb = F.subpixel_local(C, key, 0, D, D, 0, H)
    med_l, med_r = F.median3_rgba(L, 0, H), F.median3_rgba(R, 0, H)
    al, ar = F.cross_arms(med_l, ARM_MAX, TAU, 0, H), F.cross_arms(med_r, ARM_MAX, TAU, 0, H)
    code0 = F.cross_init(C, D, 0, H)[1]
    est_v = F.ref_v_native(L, z["est"], z["conf_ref"], TAPS, 0, H)
    code_a, code_b = F.O.code_u8(z["est"], D), F.O.code_u8(z["d_tar"], D)
    cen = dict(tad_tau=40.0, win_w=5, win_h=7, ad_weight=2, census_weight=3)
    s = {
        "raw_cost": lambda y0, y1, t: F.raw_cost(L, R, D, y0, y1),
        "raw_cost_shard": lambda y0, y1, t: F.raw_cost(L, R, D, y0, y1, b, e),
        "raw_cost16": lambda y0, y1, t: F.raw_cost16(L, R, D, y0, y1),
        "census": lambda y0, y1, t: F.census(L, y0, y1, 5, 7, trim=t),
        "census_cost": lambda y0, y1, t: F.census_cost(L, R, D, y0, y1, trim=t, **cen),
        "census_cost16": lambda y0, y1, t: F.census_cost(L, R, D, y0, y1, u16=True, d_begin=b, d_end=e, trim=t, **cen),
        "support_v": lambda y0, y1, t: F.support(L, TAPS, 0, y0, y1, trim=t),
        "support_h": lambda y0, y1, t: F.support(L, TAPS, 1, y0, y1),
        "pass_v": lambda y0, y1, t: F.aggregate_pass(z["sL"], z["sR"], C, D, TAPS, 0, y0, y1, trim=t),
        "pass_h": lambda y0, y1, t: F.aggregate_pass(z["sL"], z["sR"], C, D, TAPS, 1, y0, y1),
        "pass_v_shard": lambda y0, y1, t: F.aggregate_pass(z["sL"], z["sR"], Cl, D, TAPS, 0, y0, y1, b, e, trim=t),
        "wta": lambda y0, y1, t: F.wta(C, D, y0, y1),
        "wta_ref": lambda y0, y1, t: F.wta_ref(C, z["ref_l"], z["ref_r"], D, y0, y1),
        "wta_local": lambda y0, y1, t: F.wta_local(Cl, b, e, D, y0, y1),
        "wta_target_local": lambda y0, y1, t: F.wta_target_local(Cl, key, b, e, D, y0, y1),
        "wta_second": lambda y0, y1, t: F.wta_second(key, key_l, m1, m2, y0, y1),
        "wta_finalize": lambda y0, y1, t: F.wta_finalize(key, m2, tkey, t2, D, y0, y1),
        "wta_ref_local": lambda y0, y1, t: F.wta_ref_local(Cl, z["ref_l"], b, e, D, y0, y1),
        "wta_ref_target_local": lambda y0, y1, t: F.wta_ref_target_local(Cl, z["ref_r"], key, b, e, D, y0, y1),
        "wta_ref_finalize": lambda y0, y1, t: F.wta_ref_finalize(key, tkey, t2, D, y0, y1),
        "consistency_u8": lambda y0, y1, t: F.consistency(code_a, code_b, z["conf_ref"], z["conf_tar"], D, y0, y1),
        "subpixel": lambda y0, y1, t: F.subpixel(C, z["est"], D, y0, y1),
        "subpixel_local": lambda y0, y1, t: np.moveaxis(F.subpixel_local(Cl, key, b, e, D, y0, y1), 0, 1),
        "subpixel_finalize": lambda y0, y1, t: F.subpixel_finalize(key, nb, D, y0, y1),
        "disp_mask": lambda y0, y1, t: F.disp_mask(z["disp_lr"], z["est"], z["d_tar"], None, None, D, 1, y0, y1),
        "disp_fill": lambda y0, y1, t: F.disp_fill(z["disp_lr"], y0, y1),
        "median3": lambda y0, y1, t: F.median3(z["est"], y0, y1, trim=t),
        "ref_v_native": lambda y0, y1, t: np.moveaxis(F.ref_v_native(L, z["est"], z["conf_ref"], TAPS, y0, y1, trim=t), 0, 1),
        "ref_h": lambda y0, y1, t: np.moveaxis(F.ref_h(L, z["conf_ref"], est_v, TAPS, y0, y1), 0, 1),
        "consistency_native": lambda y0, y1, t: F.consistency_native(z["est"], z["d_tar"], y0, y1),
        "refine_native": lambda y0, y1, t: tuple(v for _, v in sorted(F.refine_native(
            L, R, D, C, z["est"], z["d_tar"], z["conf_ref"], z["conf_tar"], 2, TAPS, y0, y1, trim=t).items())),
        "median3_rgba": lambda y0, y1, t: F.median3_rgba(L, y0, y1, trim=t),
        "cross_arms": lambda y0, y1, t: F.cross_arms(med_l, ARM_MAX, TAU, y0, y1, trim=t),
        "cross_cost": lambda y0, y1, t: F.cross_cost(med_l, med_r, D, y0, y1),
        "cross_integral_h": lambda y0, y1, t: F.cross_integral_h(C, D, y0, y1),
        "cross_oii_h": lambda y0, y1, t: F.cross_oii(C, al, ar, D, "h", ARM_MAX, y0, y1),
        "cross_oii_v": lambda y0, y1, t: F.cross_oii(C, al, ar, D, "v", ARM_MAX, y0, y1, trim=t),
        "cross_init": lambda y0, y1, t: F.cross_init(C, D, y0, y1),
        "cross_vote": lambda y0, y1, t: F.cross_vote(code0, al, D, ARM_MAX, y0, y1, trim=t),
    }
    for k in range(8):
        s[f"sgm_path{k}"] = lambda y0, y1, t, k=k: F.sgm_path(C16, k, 16, 128, D, (y0, y1), (0, W), trim=t)
    s["sgm"] = lambda y0, y1, t: F.sgm(C16, 8, 16, 128, D, (y0, y1), (0, W))
    return s


STAGES = ["raw_cost", "raw_cost_shard", "raw_cost16", "census", "census_cost", "census_cost16", "support_v", "support_h",
          "pass_v", "pass_h", "pass_v_shard", "wta", "wta_ref", "wta_local", "wta_target_local", "wta_second",
          "wta_finalize", "subpixel", "subpixel_local", "subpixel_finalize", "disp_mask", "disp_fill", "median3",
          "ref_v_native", "ref_h", "consistency_native", "refine_native", "median3_rgba", "cross_arms", "cross_cost",
          "cross_integral_h", "cross_oii_h", "cross_oii_v", "cross_init", "cross_vote", "sgm", "wta_ref_local",
          "wta_ref_target_local", "wta_ref_finalize", "consistency_u8"] + [
              f"sgm_path{k}" for k in range(8)]
# window stages: the window is the cone, so one row less must show
WINDOWED = ["census", "census_cost", "support_v", "pass_v", "pass_v_shard", "median3", "ref_v_native", "median3_rgba"]


def test_every_stage_is_listed():
    assert sorted(STAGES) == sorted(stages(*SHAPES[0]))


def tup(v):
    return v if isinstance(v, tuple) else (v,)


@functools.lru_cache(maxsize=None)
def whole(shape, name):
    return tup(stages(*shape)[name](0, shape[1], 0))


@pytest.mark.parametrize("name", STAGES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_cone_equals_whole(shape, name):
    H = shape[1]
    for y0, y1 in bands_of(H):
        got = tup(stages(*shape)[name](y0, y1, 0))
        want = whole(shape, name)
        assert len(got) == len(want)
        for g, w in zip(got, want):
            assert same(g, w[y0:y1]), (name, y0, y1)


@pytest.mark.parametrize("name", WINDOWED)
def test_window_one_row_short_differs(name):
    shape = SHAPES[1]
    H = shape[1]
    y0, y1 = H // 2 - 1, H // 2 + 2  # interior: the window is not clamped, so the trim bites
    got = tup(stages(*shape)[name](y0, y1, 1))
    want = whole(shape, name)
    assert not all(same(g, w[y0:y1]) for g, w in zip(got, want)), name


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_column_crops(shape):
    """The column-recursive stages: a pair of columns over every row."""
    W, H, D = shape
    z = inputs(*shape)
    for x0, x1 in ((0, 2), (W // 2, W // 2 + 2), (W - 2, W)):
        assert same(F.cross_integral_v(z["C"], D, x0, x1), F.cross_integral_v(z["C"], D, 0, W)[:, x0:x1])
        for k in (2, 3):
            got = F.sgm_path(z["C16"], k, 16, 128, D, (0, H), (x0, x1))
            assert same(got, F.sgm_path(z["C16"], k, 16, 128, D, (0, H), (0, W))[:, x0:x1]), k
        # and a region of both a few rows and a few columns, every path and their sum
        y0, y1 = H - 3, H
        for k in range(8):
            got = F.sgm_path(z["C16"], k, 16, 128, D, (y0, y1), (x0, x1))
            assert same(got, F.sgm_path(z["C16"], k, 16, 128, D, (0, H), (0, W))[y0:y1, x0:x1]), k
        assert same(F.sgm(z["C16"], 8, 16, 128, D, (y0, y1), (x0, x1)),
                    F.sgm(z["C16"], 8, 16, 128, D, (0, H), (0, W))[y0:y1, x0:x1])


# Negative controls of the recursive stages.  The penalties 2^20 keep min(...) on L(q, d) for
# these short paths, so L(p, d) = C(p, d) + L(q, d) - m carries every pixel of the path: a
# cone that starts one pixel late changes the whole line after it.
BIG = 1 << 20


@pytest.mark.parametrize("k", range(8))
def test_sgm_cone_one_short_differs(k):
    W, H, D = SHAPES[2]
    C16 = inputs(W, H, D)["C16"]
    dx, dy = F.sgm_ref.STEPS[k]
    if dy == 0:
        rows, cols = (H // 2, H // 2 + 2), ((2, W) if dx > 0 else (0, W - 2))
    elif dx == 0:
        rows, cols = ((2, H) if dy > 0 else (0, H - 2)), (W // 2, W // 2 + 2)
    else:  # an interior band whose cone of W - 1 rows is not clamped by the image
        rows, cols = ((H - 12, H - 10) if dy > 0 else (10, 12)), (0, W)
    full = F.sgm_path(C16, k, BIG, BIG, D, (0, H), (0, W))[rows[0]:rows[1], cols[0]:cols[1]]
    assert same(F.sgm_path(C16, k, BIG, BIG, D, rows, cols), full)
    assert not same(F.sgm_path(C16, k, BIG, BIG, D, rows, cols, trim=1), full)


def test_oii_v_cone_one_short_differs():
    """oii-V reads row y + m - 1 with m >= -arm_max: the full reach needs both views' upper
    arms at their maximum, so the control uses uniform full-length arms."""
    W, H, D = SHAPES[1]
    C = inputs(W, H, D)["C"]
    arms = np.empty((H, W, 4), np.int8)
    arms[...] = (-ARM_MAX, ARM_MAX, -ARM_MAX, ARM_MAX)
    y0, y1 = H // 2 - 1, H // 2 + 2
    full = F.cross_oii(C, arms, arms, D, "v", ARM_MAX, 0, H)[y0:y1]
    assert same(F.cross_oii(C, arms, arms, D, "v", ARM_MAX, y0, y1), full)
    assert not same(F.cross_oii(C, arms, arms, D, "v", ARM_MAX, y0, y1, trim=1), full)


def test_integral_cone_one_short_differs():
    W, H, D = SHAPES[0]
    C = inputs(W, H, D)["C"]
    y0, y1 = H // 2, H // 2 + 2
    assert not same(F.cross_integral_h(C, D, y0, y1, trim=1), F.cross_integral_h(C, D, 0, H)[y0:y1, 1:])
    x0, x1 = W // 2, W // 2 + 2
    assert not same(F.cross_integral_v(C, D, x0, x1, trim=1), F.cross_integral_v(C, D, 0, W)[1:, x0:x1])


def test_bands_straddle_their_limits():
    """far_ref.bands: every straddle band holds offsets on both sides of each of its limits,
    for the volume kinds of tests/test_gpu_far.py (no allocation: arithmetic only)."""
    for H, row, item in ((4112, 1021 * 256, 4), (4112, 1021 * 256, 2), (8200, 1024 * 512, 4), (8200, 1024 * 512, 2),
                         (65600, 256 * 256, 4), (65600, 256 * 256, 2), (4096, 1024 * 256, 4), (64, 64, 4)):
        bs = F.bands(H, row, item)
        assert bs[0][1] == 0 and bs[-1][2] == H
        seen = []
        for name, y0, y1, limits in bs:
            assert 0 <= y0 < y1 <= H
            for limit, unit in limits:
                assert y0 * row * unit < limit < y1 * row * unit, name
                seen.append((limit, unit))
        total = H * row
        want = [(lim, u) for lim, u in ((1 << 31, item), (1 << 32, item), (1 << 31, 1), (1 << 32, 1)) if total * u > lim]
        assert sorted(seen) == sorted(want)
