"""The speckle filter on the CPU: tests/speckle_ref.py (the oracle of tests/test_gpu_speckle.py)
pinned against an independent fixpoint iteration and hand-written answers, the generators'
own claims, the host-side half of the C-ABI (parameter checks, the 2^31 - 1 pixel limit, null
pointers: no launch), and the quality claim of DESIGN.md §Speckle through the references."""
import ctypes

import numpy as np
import pytest

import census_ref as CR
import sgm_ref as SG
import speckle_ref as SK


@pytest.fixture(scope="module")
def L():
    import stereo_matchin_amd._lib as L
    L.lib()
    return L


def fixpoint(d, valid=None, min_size=32, max_diff=1):
    """An implementation that shares nothing with the flood fill: every valid pixel starts with
    its own flat index and takes the minimum over its linked neighbours until nothing changes;
    the sizes are a histogram of the final labels."""
    d = np.asarray(d).astype(np.int64)
    H, W = d.shape
    ok = np.ones((H, W), bool) if valid is None else np.asarray(valid) != 0
    big = H * W
    lab = np.where(ok, np.arange(big).reshape(H, W), big)
    link_r = ok[:, :-1] & ok[:, 1:] & (np.abs(d[:, :-1] - d[:, 1:]) <= max_diff)
    link_d = ok[:-1, :] & ok[1:, :] & (np.abs(d[:-1, :] - d[1:, :]) <= max_diff)
    while True:
        new = lab.copy()
        new[:, :-1] = np.where(link_r, np.minimum(new[:, :-1], lab[:, 1:]), new[:, :-1])
        new[:, 1:] = np.where(link_r, np.minimum(new[:, 1:], lab[:, :-1]), new[:, 1:])
        new[:-1, :] = np.where(link_d, np.minimum(new[:-1, :], lab[1:, :]), new[:-1, :])
        new[1:, :] = np.where(link_d, np.minimum(new[1:, :], lab[:-1, :]), new[1:, :])
        if np.array_equal(new, lab):
            break
        lab = new
    counts = np.bincount(lab[ok], minlength=big + 1)
    size = np.where(ok, counts[lab], 0)
    label = np.where(ok, lab, -1)
    return label.astype(np.int32), size.astype(np.int32), (ok & (size >= min_size)).astype(np.uint8)


def _same(a, b):
    return all(x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(a, b))


# ------------------------------------------------------------------ the reference

@pytest.mark.parametrize("H,W", [(1, 1), (3, 5), (17, 65), (23, 40)])
def test_flood_fill_equals_the_fixpoint_on_random_maps(H, W):
    for seed in range(4):
        for levels, holes in ((2, 0.0), (3, 0.3), (6, 0.1)):
            d, valid = SK.random(H, W, seed, levels, holes)
            for min_size, max_diff in SK.PARAMS:
                assert _same(SK.components(d, valid, min_size, max_diff), fixpoint(d, valid, min_size, max_diff))
            assert _same(SK.components(d, None, 2, 0), fixpoint(d, None, 2, 0))


@pytest.mark.parametrize("name", sorted(SK.GENERATORS))
def test_flood_fill_equals_the_fixpoint_on_every_generator(name):
    for H, W in SK.SHAPES:
        d, valid = SK.GENERATORS[name](H, W)
        assert d.dtype == np.int32 and d.shape == (H, W)
        for min_size, max_diff in SK.PARAMS:
            assert _same(SK.components(d, valid, min_size, max_diff), fixpoint(d, valid, min_size, max_diff)), \
                (H, W, min_size, max_diff)


def test_known_answers_5x7():
    d = np.array([[1, 1, 5, 5, 5, 9, 9],
                  [1, 2, 5, 0, 5, 9, 7],
                  [3, 2, 5, 5, 5, 0, 7],
                  [3, 3, 0, 0, 0, 0, 7],
                  [8, 3, 3, 4, 5, 6, 7]], np.int32)
    valid = np.ones((5, 7), np.uint8)
    valid[2, 5] = 0  # the 0 between the 9s and the bottom 0s
    # max_diff 0: the 1s {0, 1, 7}; the 2s {8, 15}; the ring of 5s (8 pixels, label 2); the 0 inside
    # the ring (10); the 9s {5, 6, 12}; the 7s {13, 20, 27, 34}; the 3s {14, 21, 22, 29, 30}; the 0s
    # of row 3 {23, 24, 25, 26}; 8, 4, 5, 6 of the bottom row alone
    want_label = np.array([[0, 0, 2, 2, 2, 5, 5],
                           [0, 8, 2, 10, 2, 5, 13],
                           [14, 8, 2, 2, 2, -1, 13],
                           [14, 14, 23, 23, 23, 23, 13],
                           [28, 14, 14, 31, 32, 33, 13]], np.int32)
    want_size = np.array([[3, 3, 8, 8, 8, 3, 3],
                          [3, 2, 8, 1, 8, 3, 4],
                          [5, 2, 8, 8, 8, 0, 4],
                          [5, 5, 4, 4, 4, 4, 4],
                          [1, 5, 5, 1, 1, 1, 4]], np.int32)
    label, size, keep = SK.components(d, valid, min_size=4, max_diff=0)
    assert np.array_equal(label, want_label)
    assert np.array_equal(size, want_size)
    assert np.array_equal(keep, (want_size >= 4).astype(np.uint8))
    # max_diff 1 is transitive: 1-2-3-3-4-5-6-7 along the left edge and the bottom row join the
    # 1s, 2s, 3s, the 4-5-6 of the bottom row and the 7s (3 + 2 + 5 + 3 + 4 = 17); 8 stays alone (3
    # and 8 differ by 5); the row-3 0s do not reach the 0 inside the ring (5 against 0)
    label, size, keep = SK.components(d, valid, min_size=17, max_diff=1)
    assert size[0, 0] == 17 and label[4, 6] == 0 and label[1, 6] == 0 and keep[4, 3] == 1
    assert size[4, 0] == 1 and label[4, 0] == 28 and keep[4, 0] == 0
    assert size[1, 3] == 1 and size[3, 2] == 4 and label[3, 5] == 23
    assert label[2, 5] == -1 and size[2, 5] == 0 and keep[2, 5] == 0
    assert size[0, 2] == 8 and keep[0, 2] == 0


def test_generators_do_what_they_say():
    H, W = 50, 200
    S = H * W
    d, v = SK.checker(H, W)
    assert (SK.components(d, v, 1, 1)[1] == 1).all()
    assert (SK.components(d, v, 1, 2)[1] == S).all()
    d, v = SK.ramp(H, W)
    label, size, _ = SK.components(d, v, 1, 1)
    assert (size == S).all() and (label == 0).all()
    label, size, _ = SK.components(d, v, 1, 0)
    assert (size == H).all() and np.array_equal(label, np.broadcast_to(np.arange(W), (H, W)))
    d, v = SK.serpentine(H, W)
    label, size, _ = SK.components(d, v, 1, 1)
    assert label[0, 0] == 0 and label[H - 2, W // 2] == 0 and size[0, 0] == (H // 2) * W + H // 2
    d, v = SK.spiral(H, W)
    label, size, _ = SK.components(d, v, 1, 1)
    assert label[0, 0] == 0 and size[0, 0] == (d >= 100).sum() > S // 3 and (label[d >= 100] == 0).all()
    d, v = SK.ushape(H, W, 1)
    label, size, _ = SK.components(d, v, 1, 1)
    assert label[0, W - 1] == 0 and size[0, 0] == 2 * H + W - 2 and label[0, 1] == 1 and size[0, 1] == H - 1
    d, v = SK.blobs(H, W, 6)
    label, size, keep = SK.components(d, v, 6, 1)
    assert size[SK.TILE_H, 0] == 5 and size[SK.TILE_H - 1, 0] == 5 and keep[SK.TILE_H, 0] == 0
    assert size[0, SK.TILE_W] == 6 and size[0, SK.TILE_W - 1] == 6 and keep[0, SK.TILE_W] == 1
    d, v = SK.extremes(H, W)
    _, size, _ = SK.components(d, v, 1, 65535)
    assert (size == 1).all() and d.min() == SK.I32_MIN and d.max() == SK.I32_MAX
    d, v = SK.all_invalid(H, W)
    label, size, keep = SK.components(d, v, 1, 1)
    assert (label == -1).all() and not size.any() and not keep.any()
    d, v = SK.one_valid(H, W)
    label, size, keep = SK.components(d, v, 1, 1)
    assert size.sum() == 1 and keep.sum() == 1 and label[H // 2, W // 2] == (H // 2) * W + W // 2


def test_masks():
    d = np.array([[3, 70000], [5, -1]], np.int32)
    keep = np.array([[1, 1], [0, 1]], np.uint8)
    assert np.array_equal(SK.mask16(d, keep), np.array([[3, 70000 & 0xFFFF], [0xFFFF, 0xFFFF]], np.uint16))
    f = SK.mask_f32(np.array([[1.5, 2.5], [3.5, 4.5]], np.float32), keep)
    assert f.dtype == np.float32 and np.isnan(f[1, 0]) and f[0, 1] == 2.5


# ------------------------------------------------------------------ host-side C-ABI

def _chk(L, p, **kw):
    sp = L.default_speckle_params(**kw)
    return L.lib().asw_speckle_params_check(ctypes.byref(p), ctypes.byref(sp))


def test_params_check(L):
    p = L.default_params(64, 32, ndisp=64, taps=35)
    sp = L.default_speckle_params()
    assert (sp.min_size, sp.max_diff) == (SK.DEFAULT["min_size"], SK.DEFAULT["max_diff"]) == (32, 1)
    assert _chk(L, p) == L.ASW_OK
    for min_size, max_diff in ((1, 0), (2 ** 31 - 1, 65535), (0, 1), (-5, 1), (32, -1), (32, 65536), (1, 65535)):
        want = L.ASW_OK if SK.params_ok(min_size, max_diff) else L.ASW_E_INVALID
        assert _chk(L, p, min_size=min_size, max_diff=max_diff) == want, (min_size, max_diff)
    assert _chk(L, L.default_params(0, 32)) == L.ASW_E_INVALID  # asw_params_check first
    # only width and height are read: a shard and any ndisp are fine
    assert _chk(L, L.default_params(64, 32, ndisp=64, d_begin=32, d_end=64)) == L.ASW_OK
    assert _chk(L, L.default_params(64, 32, ndisp=70000)) == L.ASW_OK
    assert L.lib().asw_speckle_params_check(None, ctypes.byref(sp)) == L.ASW_E_INVALID
    assert L.lib().asw_speckle_params_check(ctypes.byref(p), None) == L.ASW_E_INVALID
    assert L.speckle_params_of(None) is None and L.speckle_params_of(False) is None
    assert L.speckle_params_of(True).min_size == 32
    mine = L.default_speckle_params(min_size=7)
    assert L.speckle_params_of(mine).min_size == 7 and L.speckle_params_of(mine) is not mine


def test_more_than_int32_pixels_is_unsupported_before_any_launch(L):
    """Labels are int32 pixel indices: more than 2^31 - 1 pixels are ASW_E_UNSUPPORTED, and the
    stage then launches nothing (the pointers below are never dereferenced).  Up to 2^31 - 1 pixels
    the answer is asw_params_check's, whose own limit is 2^25 pixels."""
    lib = L.lib()
    sp = L.default_speckle_params()
    x, y, z = ctypes.c_void_p(256), ctypes.c_void_p(1 << 40), ctypes.c_void_p(1 << 41)
    for w, h, want in ((8192, 4096, L.ASW_OK), (2 ** 25, 1, L.ASW_OK), (2 ** 25 + 1, 1, L.ASW_E_INVALID),
                       (2 ** 31 - 1, 1, L.ASW_E_INVALID), (46341, 46340, L.ASW_E_INVALID)):
        p = L.default_params(w, h)
        assert L.params_check(p) == want
        assert lib.asw_speckle_params_check(ctypes.byref(p), ctypes.byref(sp)) == want, (w, h)
    for w, h in ((65536, 32768), (2 ** 31 - 1, 2), (46341, 46341), (2 ** 31 - 1, 2 ** 31 - 1)):
        big = L.default_params(w, h)
        assert lib.asw_speckle_params_check(ctypes.byref(big), ctypes.byref(sp)) == L.ASW_E_UNSUPPORTED
        assert lib.asw_speckle(ctypes.byref(big), ctypes.byref(sp), x, None, y, z, None, None, None) \
            == L.ASW_E_UNSUPPORTED


def test_stage_calls_validate_before_any_launch(L):
    lib = L.lib()
    p = L.default_params(64, 32, ndisp=64, taps=35)
    sp = L.default_speckle_params()
    P, S = ctypes.byref(p), ctypes.byref(sp)
    ws_bytes = lib.asw_speckle_workspace_bytes(P)
    assert ws_bytes >= 2 * 4 * 64 * 32 + 4 and lib.asw_speckle_workspace_bytes(None) == 0
    assert L.SPECKLE_STATUS_OFFSET + 4 <= ws_bytes
    ws = 1 << 40
    x, y = ctypes.c_void_p(256), ctypes.c_void_p(1 << 30)
    W = ctypes.c_void_p(ws)
    assert lib.asw_speckle(P, S, None, None, W, y, None, None, None) == L.ASW_E_INVALID
    assert lib.asw_speckle(P, S, x, None, None, y, None, None, None) == L.ASW_E_INVALID
    assert lib.asw_speckle(P, None, x, None, W, y, None, None, None) == L.ASW_E_INVALID
    assert lib.asw_speckle(None, S, x, None, W, y, None, None, None) == L.ASW_E_INVALID
    bad = L.default_speckle_params(min_size=0)
    assert lib.asw_speckle(P, ctypes.byref(bad), x, None, W, y, None, None, None) == L.ASW_E_INVALID
    # the input, the validity map and every output must lie outside the workspace
    inside = ctypes.c_void_p(ws + ws_bytes - 1)
    before = ctypes.c_void_p(ws - 4)  # an int32 map that ends inside it
    assert lib.asw_speckle(P, S, inside, None, W, y, None, None, None) == L.ASW_E_INVALID
    assert lib.asw_speckle(P, S, x, inside, W, y, None, None, None) == L.ASW_E_INVALID
    assert lib.asw_speckle(P, S, x, None, W, inside, None, None, None) == L.ASW_E_INVALID
    assert lib.asw_speckle(P, S, x, None, W, None, before, None, None) == L.ASW_E_INVALID
    assert lib.asw_speckle(P, S, x, None, W, None, None, W, None) == L.ASW_E_INVALID
    # the helpers
    assert lib.asw_lr_valid(P, None, x, x, x, y, None) == L.ASW_E_INVALID
    assert lib.asw_lr_valid(P, x, None, x, x, y, None) == L.ASW_E_INVALID
    assert lib.asw_lr_valid(P, x, x, x, x, None, None) == L.ASW_E_INVALID
    assert lib.asw_lr_valid(P, x, x, None, x, y, None) == L.ASW_E_INVALID  # ASW_LR_U8 reads the codes
    assert lib.asw_lr_valid(None, x, x, x, x, y, None) == L.ASW_E_INVALID
    assert lib.asw_speckle_mask16(P, None, x, y, None) == L.ASW_E_INVALID
    assert lib.asw_speckle_mask16(P, x, None, y, None) == L.ASW_E_INVALID
    assert lib.asw_speckle_mask16(P, x, x, None, None) == L.ASW_E_INVALID
    wide = L.default_params(64, 32, ndisp=65536)
    assert lib.asw_speckle_mask16(ctypes.byref(wide), x, x, y, None) == L.ASW_E_INVALID
    assert lib.asw_speckle_mask_f32(P, None, x, y, None) == L.ASW_E_INVALID
    assert lib.asw_speckle_mask_f32(P, x, None, y, None) == L.ASW_E_INVALID
    assert lib.asw_speckle_mask_f32(P, x, x, None, None) == L.ASW_E_INVALID
    assert lib.asw_set_speckle(None, S, None) == L.ASW_E_INVALID


def test_abi_revision_is_unchanged(L):
    assert L.lib().asw_abi_version() == 4 and L.ABI_VERSION == 4
    import stereo_matchin_amd as pkg
    assert pkg.AswSpeckleParams is L.AswSpeckleParams and pkg.default_speckle_params is L.default_speckle_params
    assert ctypes.sizeof(L.AswSpeckleParams) == 8
    assert ctypes.sizeof(L.AswSpeckleOutputs) == 5 * ctypes.sizeof(ctypes.c_void_p)


# ------------------------------------------------------------------ the quality claim

PAIRS = [(160, 96, 32, 7), (128, 64, 24, 3), (192, 64, 32, 5)]  # tests/test_sgm.py's


@pytest.mark.parametrize("W,H,D,seed", PAIRS)
@pytest.mark.parametrize("gain", [False, True])
def test_filter_lowers_the_bad_rate_of_sgm(W, H, D, seed, gain):
    """on each synthetic pair, unchanged and with clip(rint(0.7 R + 40)) on the
    right image, SGM at its defaults on the default census cost followed by a first-argmin, every
    pixel valid, then the filter at its defaults (32, 1): among the pixels of the columns x >= D
    the bad rate (census_ref.bad_rate's rule) of the kept ones is below the rate of all of them,
    and at least 0.90 of them are kept (the reference keeps >= 0.943 on every variant)."""
    from stereo_matchin_amd.synthetic import make_pair
    Lh, Rh, gt = make_pair(W, H, D, seed)
    if gain:
        Rh = CR.gain_offset(Rh)
    d = SG.first_argmin(SG.sgm(CR.cost_u16(Lh, Rh, D), **SG.DEFAULT))
    _, _, keep = SK.components(d, None, **SK.DEFAULT)
    bad = (np.abs(d.astype(np.int64) - gt) > 1)[:, D:]
    kept = keep[:, D:] != 0
    before, after, share = float(bad.mean()), float(bad[kept].mean()), float(kept.mean())
    assert before == CR.bad_rate(d, gt, D)
    print(f"bad-pixel rate ({W}, {H}, {D}, {seed}){' gain/offset' if gain else ''}: all {before:.3f} -> kept "
          f"{after:.3f}, kept share {share:.3f}")
    assert after < before
    assert share >= 0.90
