"""Semi-global matching on the CPU: a naive restatement and closed forms that pin
tests/sgm_ref.py (the oracle of the kernels, tests/test_gpu_sgm.py), the host-side half of the
C-ABI (asw_sgm_params_check, null-pointer rejection: no launch), and the quality claim of
DESIGN.md §SGM through the reference and a first-argmin."""
import ctypes

import numpy as np
import pytest

import census_ref as CR
import sgm_ref as SG

PENALTIES = [(0, 0), (5, 5), (100, 20000), (1048576, 1048576)]
SHAPES = [(1, 3, 4), (2, 5, 3), (7, 6, 9)]  # (D, H, W)


@pytest.fixture(scope="module")
def L():
    import stereo_matchin_amd._lib as L
    L.lib()
    return L


def _costs(D, H, W, seed=0):
    """Costs over the full uint16 range, 0 and 65535 among them."""
    rng = np.random.default_rng(seed + 1000 * D + 10 * H + W)
    c = rng.integers(0, 65536, (D, H, W))
    c.reshape(-1)[:: 7] = 65535
    c.reshape(-1)[3:: 11] = 0
    return c


def naive_path(C, k, p1, p2):
    """The recurrence of include/asw.h §SGM, pixel by pixel and plane by plane."""
    D, H, W = C.shape
    dx, dy = SG.STEPS[k]
    L = np.zeros((D, H, W), np.int64)
    ys = range(H) if dy >= 0 else range(H - 1, -1, -1)
    xs = range(W) if dx >= 0 else range(W - 1, -1, -1)
    for y in ys:
        for x in xs:
            qx, qy = x - dx, y - dy
            if not (0 <= qx < W and 0 <= qy < H):
                for d in range(D):
                    L[d, y, x] = int(C[d, y, x])
                continue
            m = min(int(L[j, qy, qx]) for j in range(D))
            for d in range(D):
                terms = [int(L[d, qy, qx]), m + p2]
                if d > 0:
                    terms.append(int(L[d - 1, qy, qx]) + p1)
                if d < D - 1:
                    terms.append(int(L[d + 1, qy, qx]) + p1)
                L[d, y, x] = int(C[d, y, x]) + min(terms) - m
    return L


# ------------------------------------------------------------------ the restatement

@pytest.mark.parametrize("D,H,W", SHAPES)
def test_reference_equals_the_naive_loops(D, H, W):
    C = _costs(D, H, W)
    for p1, p2 in PENALTIES:
        paths = [SG.path(C, k, p1, p2) for k in range(8)]
        for k in range(8):
            assert np.array_equal(paths[k], naive_path(C, k, p1, p2)), (k, p1, p2)
        assert np.array_equal(SG.sgm(C, 4, p1, p2), sum(paths[:4]))
        assert np.array_equal(SG.sgm(C, 8, p1, p2), sum(paths))


def test_zero_p2_is_the_raw_cost():
    C = _costs(7, 6, 9, 1)
    for k in range(8):
        assert np.array_equal(SG.path(C, k, 0, 0), C)
    assert np.array_equal(SG.sgm(C, 4, 0, 0), 4 * C)
    assert np.array_equal(SG.sgm(C, 8, 0, 0), 8 * C)


@pytest.mark.parametrize("D,H,W", SHAPES + [(16, 9, 12)])
def test_path_cost_bounds(D, H, W):
    C = _costs(D, H, W, 2)
    for p1, p2 in PENALTIES + [(16, 128)]:
        for k in range(8):
            Lk = SG.path(C, k, p1, p2)
            assert (Lk >= C).all() and (Lk <= C + p2).all(), (k, p1, p2)


def test_huge_penalties_give_a_rebased_running_sum():
    """Costs <= 100 and at most 64 steps per path: the sum along a path stays far below P1 = P2
    = 2^20, so the minimum is always the d term: L(p, d) = C(p, d) + L(q, d) - m, the running
    sum along the path minus the minima met on the way."""
    D, H, W = 5, 40, 64
    rng = np.random.default_rng(3)
    C = rng.integers(0, 101, (D, H, W))
    P = 1048576
    # path 0 (left to right): cumsum along x; m of pixel x-1 is the minimum over d of L there
    L0 = SG.path(C, 0, P, P)
    run = np.cumsum(C, axis=2)
    want = np.empty_like(run)
    want[:, :, 0] = C[:, :, 0]
    base = np.zeros((H,), np.int64)  # the minima subtracted so far
    for x in range(1, W):
        base = base + (run[:, :, x - 1] - base).min(axis=0)
        want[:, :, x] = run[:, :, x] - base
    assert np.array_equal(L0, want)
    # path 1 is path 0 of the mirrored image, paths 2 and 3 the same along y
    assert np.array_equal(SG.path(C, 1, P, P), SG.path(C[:, :, ::-1], 0, P, P)[:, :, ::-1])
    Ct = np.transpose(C, (0, 2, 1))
    assert np.array_equal(SG.path(C, 2, P, P), np.transpose(SG.path(Ct, 0, P, P), (0, 2, 1)))
    assert np.array_equal(SG.path(C, 3, P, P), np.transpose(SG.path(Ct, 1, P, P), (0, 2, 1)))
    # a diagonal: the running sum along each diagonal, restarted at the border
    L4 = SG.path(C, 4, P, P)
    for x0, y0 in ((0, 0), (10, 0), (0, 7), (63, 0), (0, 39)):
        n = min(W - x0, H - y0)
        seg = np.stack([C[:, y0 + i, x0 + i] for i in range(n)], 1)  # [D][n]
        got = np.stack([L4[:, y0 + i, x0 + i] for i in range(n)], 1)
        assert np.array_equal(got, SG.path(seg[:, None, :], 0, P, P)[:, 0, :])


def test_sum_is_exact_in_float32_at_the_extremes():
    C = np.full((3, 4, 5), 65535)
    C[1] = 0
    S = SG.sgm(C, 8, 1048576, 1048576)
    assert S.max() < 2 ** 24
    assert S.max() <= 8 * (65535 + 1048576)
    assert np.array_equal(S.astype(np.float32).astype(np.int64), S)


# ------------------------------------------------------------------ host-side C-ABI

def _chk(L, p, **kw):
    sp = L.default_sgm_params(**kw)
    return L.lib().asw_sgm_params_check(ctypes.byref(p), ctypes.byref(sp))


def test_params_check(L):
    p = L.default_params(64, 32, ndisp=64, taps=35)
    sp = L.default_sgm_params()
    assert (sp.paths, sp.p1, sp.p2) == (8, 16, 128)
    assert _chk(L, p) == L.ASW_OK
    for paths, p1, p2 in ((4, 0, 0), (8, 0, 0), (8, 7, 7), (4, 1048576, 1048576), (8, 0, 1048576), (5, 16, 128),
                          (0, 16, 128), (16, 16, 128), (8, -1, 128), (8, 129, 128), (8, 16, 1048577), (8, 16, -1)):
        assert (_chk(L, p, paths=paths, p1=p1, p2=p2) == L.ASW_OK) == SG.params_ok(paths, p1, p2), (paths, p1, p2)
        if not SG.params_ok(paths, p1, p2):
            assert _chk(L, p, paths=paths, p1=p1, p2=p2) == L.ASW_E_INVALID
    assert _chk(L, L.default_params(0, 32)) == L.ASW_E_INVALID  # asw_params_check first
    # a d-shard cannot compute m
    assert _chk(L, L.default_params(64, 32, ndisp=64, d_begin=0, d_end=32)) == L.ASW_E_INVALID
    assert _chk(L, L.default_params(64, 32, ndisp=64, d_begin=32, d_end=64)) == L.ASW_E_INVALID
    assert _chk(L, L.default_params(64, 32, ndisp=64, d_begin=0, d_end=64)) == L.ASW_OK
    # taps and iters are not SGM's: any accepted asw_params will do
    assert _chk(L, L.default_params(64, 32, ndisp=300, taps=11, iters=0)) == L.ASW_OK
    assert L.lib().asw_sgm_params_check(None, ctypes.byref(sp)) == L.ASW_E_INVALID
    assert L.lib().asw_sgm_params_check(ctypes.byref(p), None) == L.ASW_E_INVALID


def test_stage_calls_validate_before_any_launch(L):
    lib = L.lib()
    p = L.default_params(64, 32, ndisp=64, taps=35)
    sp = L.default_sgm_params()
    x, y = ctypes.c_void_p(256), ctypes.c_void_p(512)
    P, S = ctypes.byref(p), ctypes.byref(sp)
    assert lib.asw_sgm_path(P, S, 0, None, y, 0, None) == L.ASW_E_INVALID
    assert lib.asw_sgm_path(P, S, 0, x, None, 0, None) == L.ASW_E_INVALID
    assert lib.asw_sgm_path(P, None, 0, x, y, 0, None) == L.ASW_E_INVALID
    assert lib.asw_sgm_path(None, S, 0, x, y, 0, None) == L.ASW_E_INVALID
    assert lib.asw_sgm_path(P, S, -1, x, y, 0, None) == L.ASW_E_INVALID
    assert lib.asw_sgm_path(P, S, 8, x, y, 0, None) == L.ASW_E_INVALID
    assert lib.asw_sgm_path(P, S, 0, x, x, 0, None) == L.ASW_E_INVALID  # aliased
    assert lib.asw_sgm(P, S, None, y, None, None) == L.ASW_E_INVALID
    assert lib.asw_sgm(P, S, x, None, None, None) == L.ASW_E_INVALID
    assert lib.asw_sgm(P, S, x, x, None, None) == L.ASW_E_INVALID
    bad = L.default_sgm_params(paths=5)
    assert lib.asw_sgm_path(P, ctypes.byref(bad), 0, x, y, 0, None) == L.ASW_E_INVALID
    assert lib.asw_sgm(P, ctypes.byref(bad), x, y, None, None) == L.ASW_E_INVALID
    shard = L.default_params(64, 32, ndisp=64, d_begin=0, d_end=32)
    assert lib.asw_sgm(ctypes.byref(shard), S, x, y, None, None) == L.ASW_E_INVALID
    assert lib.asw_set_sgm(None, S) == L.ASW_E_INVALID
    assert lib.asw_sgm_workspace_bytes(P, S) >= 0


def test_shape_limits_are_checked_on_the_host(L):
    """A pitch above 65536 planes is ASW_E_UNSUPPORTED before any launch; 65536 planes pass the
    check (the pointers below are never dereferenced: the parameter errors come first)."""
    lib = L.lib()
    sp = L.default_sgm_params()
    x, y = ctypes.c_void_p(256), ctypes.c_void_p(512)
    big = L.default_params(2, 1, ndisp=65537)
    assert lib.asw_sgm_params_check(ctypes.byref(big), ctypes.byref(sp)) == L.ASW_OK
    assert lib.asw_sgm_path(ctypes.byref(big), ctypes.byref(sp), 0, x, y, 0, None) == L.ASW_E_UNSUPPORTED
    assert lib.asw_sgm(ctypes.byref(big), ctypes.byref(sp), x, y, None, None) == L.ASW_E_UNSUPPORTED
    # the uint16 cost kernels stage a pitch in LDS: the predicates know that bound too
    wide = L.default_params(64, 32, ndisp=20000, taps=35)
    assert lib.asw_raw16_supported(ctypes.byref(L.default_params(64, 32, ndisp=4096, taps=35))) == 1
    assert lib.asw_raw16_supported(ctypes.byref(wide)) == 0
    assert lib.asw_raw_cost16(ctypes.byref(wide), x, x, y, None) == L.ASW_E_UNSUPPORTED
    cp = L.default_census_params()
    assert lib.asw_census16_supported(ctypes.byref(wide), ctypes.byref(cp)) == 0
    assert lib.asw_census_cost16(ctypes.byref(wide), ctypes.byref(cp), x, x, x, x, y, None) == L.ASW_E_UNSUPPORTED


def test_abi_revision_is_unchanged(L):
    assert L.lib().asw_abi_version() == 4 and L.ABI_VERSION == 4
    import stereo_matchin_amd as pkg
    assert pkg.AswSgmParams is L.AswSgmParams and pkg.default_sgm_params is L.default_sgm_params
    assert ctypes.sizeof(L.AswSgmParams) == 12


# ------------------------------------------------------------------ the quality claim

PAIRS = [(160, 96, 32, 7), (128, 64, 24, 3), (192, 64, 32, 5)]


@pytest.mark.parametrize("W,H,D,seed", PAIRS)
@pytest.mark.parametrize("gain", [False, True])
def test_sgm_beats_the_raw_argmin(W, H, D, seed, gain):
    """on each synthetic pair, unchanged and with clip(rint(0.7 R + 40)) on the
    right image, the bad-pixel rate of SGM at its defaults (8 paths, 16 / 128) on the default
    census cost is below the rate of the first-argmin of that raw volume itself.  Measured
    raw -> SGM: (160, 96, 32, 7) 0.105 -> 0.080, gain 0.192 -> 0.108; (128, 64, 24, 3)
    0.166 -> 0.147, gain 0.234 -> 0.176; (192, 64, 32, 5) 0.101 -> 0.081, gain 0.192 -> 0.096."""
    from stereo_matchin_amd.synthetic import make_pair
    Lh, Rh, gt = make_pair(W, H, D, seed)
    if gain:
        Rh = CR.gain_offset(Rh)
    C = CR.cost_u16(Lh, Rh, D)
    raw = CR.bad_rate(SG.first_argmin(C), gt, D)
    got = CR.bad_rate(SG.first_argmin(SG.sgm(C, **SG.DEFAULT)), gt, D)
    print(f"bad-pixel rate ({W}, {H}, {D}, {seed}){' gain/offset' if gain else ''}: raw {raw:.3f} -> SGM {got:.3f}")
    assert got < raw
