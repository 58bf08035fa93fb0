"""The census / AD-census cost on the CPU: known answers that pin tests/census_ref.py (the
oracle of the kernels, tests/test_gpu_census.py), the host-side half of the C-ABI
(asw_census_params_check, asw_census16_supported, null-pointer rejection: no launch), and
the quality claim of DESIGN.md §Census through the CPU oracle."""
import ctypes

import numpy as np
import pytest

import census_ref as CR

FULL_9x7 = (1 << 62) - 1


def _grey(Y):
    Y = np.asarray(Y, np.uint8)
    return np.ascontiguousarray(np.stack([Y, Y, Y, np.full_like(Y, 255)], -1))


@pytest.fixture(scope="module")
def L():
    import stereo_matchin_amd._lib as L
    L.lib()
    return L


# ------------------------------------------------------------------ the restatement

def test_luma_of_grey_is_identity_and_alpha_ignored():
    Y = np.arange(256, dtype=np.uint8).reshape(16, 16)
    img = _grey(Y)
    assert np.array_equal(CR.luma(img), Y)  # 77 + 150 + 29 = 256
    img[..., 3] = 7
    assert np.array_equal(CR.luma(img), Y)
    assert CR.luma(np.array([[[255, 0, 0, 255], [0, 255, 0, 255], [0, 0, 255, 255]]], np.uint8)).tolist() == \
        [[(77 * 255 + 128) >> 8, (150 * 255 + 128) >> 8, (29 * 255 + 128) >> 8]]


def test_constant_image_gives_zero():
    for w, h in ((9, 7), (3, 3), (7, 9)):
        assert not CR.census_luma(np.full((11, 13), 90), w, h).any()


def test_single_bright_pixel():
    Y = np.full((15, 21), 50)
    Y[7, 10] = 200
    c = CR.census_luma(Y)
    assert int(c[7, 10]) == FULL_9x7
    c[7, 10] = 0
    assert not c.any()  # strict '<': the bright pixel is darker than nobody, and ties set no bit


def test_bit_order():
    for w, h in ((9, 7), (5, 3), (3, 9)):
        rw, rh = w // 2, h // 2
        for (dx, dy), bit in (((-rw, -rh), 0), ((rw, rh), w * h - 2), ((-1, 0), (w * h - 1) // 2 - 1),
                              ((1, 0), (w * h - 1) // 2), ((rw, -rh), w - 1)):
            Y = np.full((21, 21), 100)
            Y[10 + dy, 10 + dx] = 10
            assert int(CR.census_luma(Y, w, h)[10, 10]) == 1 << bit, (w, h, dx, dy)


def test_small_image_equals_the_per_pixel_loop():
    rng = np.random.default_rng(1)
    Y = rng.integers(0, 256, (3, 5))
    got = CR.census_luma(Y, 9, 7)
    for y in range(3):
        for x in range(5):
            code, n = 0, 0
            for dy in range(-3, 4):
                for dx in range(-4, 5):
                    if dx == 0 and dy == 0:
                        continue
                    if Y[min(max(y + dy, 0), 2), min(max(x + dx, 0), 4)] < Y[y, x]:
                        code |= 1 << n
                    n += 1
            assert n == 62 and int(got[y, x]) == code


def test_invariant_under_an_increasing_luma_map():
    """Y -> 2Y/3 + 20 (integer division) on a grey image whose values are the multiples of
    3 from 0 to 252: there the map is 2k + 20 for Y = 3k, strictly increasing."""
    rng = np.random.default_rng(2)
    Y = 3 * rng.integers(0, 85, (24, 40))
    Z = 2 * Y // 3 + 20
    assert len(np.unique(Y)) == len(np.unique(Z)) > 50 and Z.max() <= 255
    for w, h in ((9, 7), (5, 5)):
        a, b = CR.census(_grey(Y), w, h), CR.census(_grey(Z), w, h)
        assert a.any() and np.array_equal(a, b)


def test_popcount64():
    v = np.array([0, 1, FULL_9x7, (1 << 64) - 1, 0x8000000000000001], np.uint64)
    assert CR.popcount64(v).tolist() == [0, 1, 62, 64, 2]


def test_crafted_maximum_pair():
    Lh, Rh = CR.crafted_max_pair()
    ad, ham = CR.terms(Lh, Rh, CR.census(Lh), CR.census(Rh), 4)
    assert ham[0, 4, 8] == 62 and ad[0, 4, 8] == 765
    f = CR.cost_f32(Lh, Rh, 4, ad_weight=3, census_weight=1000)
    u = CR.cost_u16(Lh, Rh, 4, ad_weight=3, census_weight=1000)
    assert f[0, 4, 8] == 64295.0 and u[0, 4, 8] == 64295 and u.max() == 64295
    assert CR.same_bits(u.astype(np.float32), f)


def test_uint16_form_equals_float_form():
    rng = np.random.default_rng(3)
    Lh = rng.integers(0, 256, (6, 40, 4), dtype=np.uint8)
    Rh = rng.integers(0, 256, (6, 40, 4), dtype=np.uint8)
    for tau, wa, wc in ((765.0, 1, 8), (40.0, 64, 17), (40.5, 0, 1024), (0.0, 5, 1)):
        f = CR.cost_f32(Lh, Rh, 12, tau, 9, 7, wa, wc)
        assert CR.same_bits(CR.cost_u16(Lh, Rh, 12, tau, 9, 7, wa, wc).astype(np.float32), f)
    assert CR.cost_u16(Lh, Rh, 12, 40.5, 9, 7, 1, 8) is None
    part = CR.cost_f32(Lh, Rh, 12, 40.5, 7, 9, 2, 3, d_begin=5, d_end=9)
    assert CR.same_bits(part, CR.cost_f32(Lh, Rh, 12, 40.5, 7, 9, 2, 3)[5:9])


# ------------------------------------------------------------------ host-side C-ABI

def _chk(L, p, **kw):
    cp = L.default_census_params(**kw)
    return L.lib().asw_census_params_check(ctypes.byref(p), ctypes.byref(cp))


def test_params_check(L):
    p = L.default_params(64, 32, ndisp=64, taps=35)
    cp = L.default_census_params()
    assert (cp.win_w, cp.win_h, cp.ad_weight, cp.census_weight) == (9, 7, 1, 8)
    assert _chk(L, p) == L.ASW_OK
    for w in CR.SIZES:
        for h in CR.SIZES:
            assert _chk(L, p, win_w=w, win_h=h) == (L.ASW_OK if (w, h) != (9, 9) else L.ASW_E_INVALID)
    for bad in (dict(win_w=4), dict(win_h=6), dict(win_w=8, win_h=8), dict(win_w=1), dict(win_h=11),
                dict(census_weight=0), dict(census_weight=1025), dict(ad_weight=65), dict(ad_weight=-1),
                dict(ad_weight=64, census_weight=1024)):
        assert _chk(L, p, **bad) == L.ASW_E_INVALID, bad
    assert _chk(L, p, ad_weight=64, census_weight=256) == L.ASW_OK       # 48960 + 15872 = 64832
    assert _chk(L, p, ad_weight=64, census_weight=268) == L.ASW_E_INVALID  # 48960 + 16616 = 65576
    neg = L.default_params(64, 32, ndisp=64, taps=35, tad_tau=-1.0)
    assert _chk(L, neg) == L.ASW_E_INVALID
    assert _chk(L, neg, ad_weight=0) == L.ASW_OK  # tau is not read
    # ceil(tau) bounds the AD term: 64 * 41 + 1014 * 62 = 65492, 64 * 42 + 1014 * 62 = 65556
    assert _chk(L, L.default_params(64, 32, tad_tau=40.5), ad_weight=64, census_weight=1014) == L.ASW_OK
    assert _chk(L, L.default_params(64, 32, tad_tau=41.5), ad_weight=64, census_weight=1014) == L.ASW_E_INVALID
    assert _chk(L, L.default_params(0, 32)) == L.ASW_E_INVALID  # asw_params_check first
    assert L.lib().asw_census_params_check(None, ctypes.byref(cp)) == L.ASW_E_INVALID
    assert L.lib().asw_census_params_check(ctypes.byref(p), None) == L.ASW_E_INVALID
    # the numpy rule is the same one
    for tau, w, h, a, c in ((765.0, 9, 7, 1, 8), (765.0, 9, 9, 1, 8), (40.5, 9, 7, 64, 1014), (41.5, 9, 7, 64, 1014),
                            (-1.0, 9, 7, 0, 8), (-1.0, 9, 7, 1, 8), (765.0, 3, 3, 64, 1024)):
        q = L.default_params(64, 32, tad_tau=tau)
        assert (_chk(L, q, win_w=w, win_h=h, ad_weight=a, census_weight=c) == L.ASW_OK) == CR.params_ok(tau, w, h, a, c)
    assert L.lib().asw_census_bytes(ctypes.byref(p)) == 64 * 32 * 8


def test_census16_supported(L):
    sup = L.lib().asw_census16_supported

    def s(p, **kw):
        return sup(ctypes.byref(p), ctypes.byref(L.default_census_params(**kw)))
    frac = L.default_params(64, 32, ndisp=64, taps=35, tad_tau=40.5)
    assert s(L.default_params(64, 32, ndisp=64, taps=35)) == 1
    assert s(L.default_params(64, 32, ndisp=64, taps=35, tad_tau=40.0)) == 1
    assert s(frac, ad_weight=0) == 1
    assert s(frac, ad_weight=1) == 0
    assert s(L.default_params(64, 32, ndisp=64, taps=11)) == 0  # no ring kernel
    assert s(L.default_params(64, 32, ndisp=64, taps=35, iters=0)) == 0
    assert s(L.default_params(64, 32, ndisp=64, taps=35), win_w=9, win_h=9) == 0
    assert s(L.default_params(64, 32, ndisp=256, taps=35, d_begin=32, d_end=64)) == 1  # a 32-plane shard


def test_stage_calls_validate_before_any_launch(L):
    lib = L.lib()
    p = L.default_params(64, 32, ndisp=64, taps=35)
    cp = L.default_census_params()
    x, y = ctypes.c_void_p(8), ctypes.c_void_p(16)
    P, C = ctypes.byref(p), ctypes.byref(cp)
    assert lib.asw_census(P, C, None, y, None) == L.ASW_E_INVALID
    assert lib.asw_census(P, C, x, None, None) == L.ASW_E_INVALID
    assert lib.asw_census(P, None, x, y, None) == L.ASW_E_INVALID
    assert lib.asw_census(None, C, x, y, None) == L.ASW_E_INVALID
    for fn in (lib.asw_census_cost, lib.asw_census_cost16):
        for hole in range(5):
            args = [x, x, x, x, y]
            args[hole] = None
            assert fn(P, C, *args, None) == L.ASW_E_INVALID
        assert fn(P, None, x, x, x, x, y, None) == L.ASW_E_INVALID
    bad = L.default_census_params(win_w=9, win_h=9)
    assert lib.asw_census(P, ctypes.byref(bad), x, y, None) == L.ASW_E_INVALID
    assert lib.asw_census_cost16(P, ctypes.byref(bad), x, x, x, x, y, None) == L.ASW_E_INVALID
    frac = L.default_params(64, 32, ndisp=64, taps=35, tad_tau=40.5)
    assert lib.asw_census_cost16(ctypes.byref(frac), C, x, x, x, x, y, None) == L.ASW_E_UNSUPPORTED
    assert lib.asw_set_census(None, C) == L.ASW_E_INVALID


def test_abi_revision_is_unchanged(L):
    assert L.lib().asw_abi_version() == 4 and L.ABI_VERSION == 4
    import stereo_matchin_amd as pkg
    assert pkg.AswCensusParams is L.AswCensusParams and pkg.default_census_params is L.default_census_params


# ------------------------------------------------------------------ the quality claim

def test_census_survives_a_gain_and_offset_where_ad_does_not(oracle):
    """DESIGN.md §Census, measured through the CPU oracle on make_pair(160, 96, 32, 7), T 9,
    r 2, right image clip(rint(0.7 R + 40)): AD 0.856, census 9x7 only 0.118, AD + 8 census
    0.064 (unchanged right image: 0.050, 0.106, 0.059).  The bounds leave a factor of
    about 2 on each side; they are conditions on the definition."""
    from stereo_matchin_amd.synthetic import make_pair
    W, H, D, T, r = 160, 96, 32, 9, 2
    Lh, Rh, gt = make_pair(W, H, D, 7)
    Rg = CR.gain_offset(Rh)
    # the harness is oracle.match when fed the oracle's own raw cost
    ref = oracle.match(Lh, Rh, D, T, r, want_cost=True)
    own = CR.match(oracle, Lh, Rh, D, T, r, oracle.raw_cost(Lh, Rh, D))
    for k in ("d_ref", "d_tar", "lr_red_rgba", "cost"):
        assert np.array_equal(own[k], ref[k]), k
    assert CR.bad_rate(ref["d_ref"], gt, D) < 0.1
    ad = CR.bad_rate(oracle.match(Lh, Rg, D, T, r)["d_ref"], gt, D)
    cen = CR.bad_rate(CR.match(oracle, Lh, Rg, D, T, r, CR.cost_f32(Lh, Rg, D, ad_weight=0, census_weight=1))["d_ref"],
                      gt, D)
    both = CR.bad_rate(CR.match(oracle, Lh, Rg, D, T, r, CR.cost_f32(Lh, Rg, D))["d_ref"], gt, D)
    print(f"bad-pixel rates under gain 0.7 / +40: AD {ad:.3f}, census {cen:.3f}, AD + 8 census {both:.3f}")
    assert ad > 0.5
    assert cen < 0.25
    assert both < 0.25
