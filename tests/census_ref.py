"""numpy restatement of the census / AD-census matching cost (include/asw.h §census,
DESIGN.md §Census): the oracle of the kernels in stereo_matchin_amd/csrc/asw_census.hip.

Every operation is an integer one, except the float form's one multiply and one add.

  luma    Y = (77 R + 150 G + 29 B + 128) >> 8
  census  neighbours row-major (dy = -rh..rh, dx = -rw..rw, centre skipped); neighbour n
          sets bit n (LSB first) when Y(clamp(x+dx), clamp(y+dy)) < Y(x, y)
  cost    xr = max(x - d, 0); AD = |dR|+|dG|+|dB|; ham = popcount(cenL(x, y) ^ cenR(xr, y))
          float   fminf(AD, tau) * w_a + (float)(w_c * ham)   (w_a = 0: (float)(w_c * ham))
          uint16  w_a * min(AD, tau) + w_c * ham

tests/test_census.py pins this file (known answers, a per-pixel loop, the quality claim).
"""
import numpy as np

F = np.float32
SIZES = (3, 5, 7, 9)
DEFAULT = dict(win_w=9, win_h=7, ad_weight=1, census_weight=8)


def luma(img):
    """uint8 [H][W] luma of an RGBA8 / RGB image (alpha ignored)."""
    a = np.asarray(img).astype(np.int64)
    return ((77 * a[..., 0] + 150 * a[..., 1] + 29 * a[..., 2] + 128) >> 8).astype(np.uint8)


def window_ok(win_w, win_h):
    return win_w in SIZES and win_h in SIZES and win_w * win_h - 1 <= 64


def params_ok(tad_tau, win_w, win_h, ad_weight, census_weight):
    """The parameter rule of asw_census_params_check (given a valid asw_params)."""
    if not window_ok(win_w, win_h) or not 0 <= ad_weight <= 64 or not 1 <= census_weight <= 1024:
        return False
    ad_max = 0
    if ad_weight > 0:
        if not tad_tau >= 0:
            return False
        ad_max = 765 if tad_tau >= 765 else int(np.ceil(tad_tau))
    return ad_weight * ad_max + census_weight * (win_w * win_h - 1) <= 65535


def census_luma(Y, win_w=9, win_h=7):
    """uint64 [H][W] census codes of a luma image."""
    assert window_ok(win_w, win_h)
    Y = np.asarray(Y).astype(np.int64)
    H, W = Y.shape
    rw, rh = win_w // 2, win_h // 2
    ys, xs = np.arange(H), np.arange(W)
    code = np.zeros((H, W), np.uint64)
    n = 0
    for dy in range(-rh, rh + 1):
        for dx in range(-rw, rw + 1):
            if dx == 0 and dy == 0:
                continue
            nb = Y[np.clip(ys + dy, 0, H - 1)][:, np.clip(xs + dx, 0, W - 1)]
            code |= (nb < Y).astype(np.uint64) << np.uint64(n)
            n += 1
    return code


def census(img, win_w=9, win_h=7):
    return census_luma(luma(img), win_w, win_h)


def popcount64(v):
    v = np.ascontiguousarray(v, np.uint64)
    return np.unpackbits(v.view(np.uint8).reshape(v.shape + (8,)), axis=-1).sum(-1).astype(np.int64)


def terms(L, R, cenL, cenR, D, d_begin=0, d_end=None):
    """(AD, ham) int64 [n][H][W] of planes d = d_begin .. d_end-1 (plane-major, the
    oracle's layout)."""
    d_end = D if d_end is None else d_end
    L = np.asarray(L).astype(np.int64)[..., :3]
    R = np.asarray(R).astype(np.int64)[..., :3]
    H, W = L.shape[:2]
    xs = np.arange(W)
    ad = np.empty((d_end - d_begin, H, W), np.int64)
    ham = np.empty_like(ad)
    for k, d in enumerate(range(d_begin, d_end)):
        xr = np.maximum(xs - d, 0)
        ad[k] = np.abs(L - R[:, xr]).sum(-1)
        ham[k] = popcount64(cenL ^ cenR[:, xr])
    return ad, ham


def cost_f32(L, R, D, tad_tau=765.0, win_w=9, win_h=7, ad_weight=1, census_weight=8, d_begin=0, d_end=None):
    """The float form, float32 [n][H][W]."""
    ad, ham = terms(L, R, census(L, win_w, win_h), census(R, win_w, win_h), D, d_begin, d_end)
    hc = (census_weight * ham).astype(F)
    if ad_weight == 0:
        return hc
    t = np.minimum(ad.astype(F), F(tad_tau))   # fminf((float)AD, tau)
    t = (t * F(ad_weight)).astype(F)           # one float multiply
    return (t + hc).astype(F)                  # one float add


def cost_u16(L, R, D, tad_tau=765.0, win_w=9, win_h=7, ad_weight=1, census_weight=8, d_begin=0, d_end=None):
    """The uint16 form, uint16 [n][H][W]; None where it is not defined."""
    if ad_weight and not (tad_tau >= 765 or tad_tau == np.floor(tad_tau)):
        return None
    ad, ham = terms(L, R, census(L, win_w, win_h), census(R, win_w, win_h), D, d_begin, d_end)
    c = census_weight * ham
    if ad_weight:
        c = c + ad_weight * np.minimum(ad, 765 if tad_tau >= 765 else int(tad_tau))
    assert c.max() <= 65535
    return c.astype(np.uint16)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def crafted_max_pair(H=9, W=16, y=4, x=8):
    """L flat 100 with (255, 255, 255) at (x, y), R flat 100 with (0, 0, 0) there: at d = 0
    that pixel has ham = 62 (9 x 7) and AD = 765, the largest cost of a weight pair."""
    L = np.full((H, W, 4), 100, np.uint8)
    R = L.copy()
    L[y, x, :3] = 255
    R[y, x, :3] = 0
    L[..., 3] = R[..., 3] = 255
    return L, R


def gain_offset(img, gain=0.7, offset=40.0):
    """clip(rint(gain * c + offset)) per colour channel, alpha kept."""
    out = np.array(img, np.uint8)
    out[..., :3] = np.clip(np.rint(gain * out[..., :3].astype(np.float64) + offset), 0, 255).astype(np.uint8)
    return out


def bad_rate(d_ref, gt, D):
    """Share of the pixels with x >= D whose |d_ref - gt| exceeds 1."""
    return float((np.abs(d_ref[:, D:].astype(np.int64) - gt[:, D:]) > 1).mean())


def match(oracle, L, R, D, T, iters, cost):
    """The oracle's supports, passes, WTA and consistency on a raw cost volume [D][H][W]
    (oracle.match with another raw cost): d_ref, d_tar, lr_rgba, lr_red_rgba, cost."""
    sv = [oracle.support(im, T, 0) for im in (L, R)]
    sh = [oracle.support(im, T, 1) for im in (L, R)]
    c = np.ascontiguousarray(cost, F)
    for _ in range(iters):
        c = oracle.aggregate_pass(sv[0], sv[1], c, T, 0)
        c = oracle.aggregate_pass(sh[0], sh[1], c, T, 1)
    dr, cr, dt, ct = oracle.wta(c)
    lr, red, cr2, ct2 = oracle.consistency(oracle.code_u8(dr, D), oracle.code_u8(dt, D), cr, ct, D)
    return {"d_ref": dr, "d_tar": dt, "conf_ref": cr, "conf_tar": ct, "lr_rgba": lr, "lr_red_rgba": red, "cost": c}
