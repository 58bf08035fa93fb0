"""Numpy restatement of the refinement loop (main.cpp:540-623: asw_ref_v, asw_ref_h,
asw_WTA_REF, Constistency, Median), parametrised on how an estimate map is decoded and on
the left-right rule:

* ``mode="u8"``: the reference's loop.  Estimates are 8-bit codes read back as
  ``(code/255)*(D-1)``, consistency is K/consist.cl's ``|q_tar - q_ref| < 1.001f`` on the
  codes, the outputs are RGBA8 images.  tests/test_refine_native.py pins this mode to
  ``oracle.refine`` bit for bit, and ``oracle.refine`` is pinned to the reference's committed
  asw_disparity.png: that ties the operation order below to the reference project.
* ``mode="native"``: include/asw.h §native refinement.  Estimates are int32 disparity
  indices decoded as ``(float)est``, consistency is ``|d_ref - d_tar| <= 1``, the outputs
  are uint16 maps.  Nothing else differs.

Every array is float32 and every tap is one vector operation per product and per sum, so
each rounds separately (numpy never fuses): the products and sums of asw_ref_v /
asw_ref_h in their tap order.  The weights come from ``oracle.support_weight`` (the
refinement falloffs 10.94 / 118.78), the volume scan from ``oracle.wta_ref``.
"""
import functools

import numpy as np

from oracle import oracle as O

REF_GC, REF_GG = 10.94, 118.78  # K/asw_refinement_v.cl:6-7
EPS = np.float32(0.00001)
INVALID16 = 0xFFFF


@functools.lru_cache(maxsize=None)
def weight_lut(taps: int) -> np.ndarray:
    """[(R+1)][766] float32: exp(-sad/10.94 - dist/118.78) of every (dist, SAD)."""
    R = taps // 2
    lut = np.empty((R + 1, 766), np.float32)
    for dist in range(R + 1):
        for sad in range(766):
            lut[dist, sad] = O.support_weight(sad, dist, REF_GC, REF_GG)
    lut.setflags(write=False)
    return lut


def _sad(a, b):
    return np.abs(a[..., :3].astype(np.int32) - b[..., :3].astype(np.int32)).sum(-1)


def decode(est, D: int, mode: str) -> np.ndarray:
    if mode == "u8":
        return (est.astype(np.float32) / np.float32(255.0)) * np.float32(D - 1)
    return est.astype(np.float32)


def ref_v(img, Dv, conf, taps: int) -> np.ndarray:
    """asw_ref_v on decoded estimates Dv: [2][H][W] = (num/den, den)."""
    H, W = conf.shape
    lut, Rr = weight_lut(taps), taps // 2
    ys = np.arange(H)
    num = np.full((H, W), EPS, np.float32)
    den = np.full((H, W), EPS, np.float32)
    for i in range(taps):
        qy = np.clip(ys + i - Rr, 0, H - 1)
        w = lut[np.abs(ys - qy)[:, None], _sad(img, img[qy])]
        t = w * conf[qy]
        num = num + t * Dv[qy]
        den = den + t
    out = np.stack([num / den, den])
    assert out.dtype == np.float32
    return out


def ref_h(img, conf, est_v, taps: int) -> np.ndarray:
    """asw_ref_h on asw_ref_v's output."""
    H, W = conf.shape
    lut, Rr = weight_lut(taps), taps // 2
    xs = np.arange(W)
    num = np.full((H, W), EPS, np.float32)
    den = np.full((H, W), EPS, np.float32)
    for i in range(taps):
        qx = np.clip(xs + i - Rr, 0, W - 1)
        w = lut[np.abs(xs - qx)[None, :], _sad(img, img[:, qx])]
        t = w * conf[:, qx]
        tr = t * est_v[0][:, qx]
        n = est_v[1][:, qx]
        num = num + tr * n
        den = den + t * n
    out = np.stack([num / den, den])
    assert out.dtype == np.float32
    return out


def median3(a: np.ndarray) -> np.ndarray:
    """3x3 median, clamp-to-edge."""
    H, W = a.shape
    ys, xs = np.arange(H), np.arange(W)
    nb = [a[np.clip(ys + dy, 0, H - 1)][:, np.clip(xs + dx, 0, W - 1)] for dy in (-1, 0, 1) for dx in (-1, 0, 1)]
    return np.sort(np.stack(nb), axis=0)[4]


def consistent(a, b, D: int, mode: str) -> np.ndarray:
    """The LR rule on two maps (codes in u8 mode, indices in native mode)."""
    if mode == "u8":
        return np.abs(decode(b, D, mode) - decode(a, D, mode)) < np.float32(1.001)
    return np.abs(a.astype(np.int64) - b.astype(np.int64)) <= 1


def native_est_left(d_ref, d_tar):
    """est_left and post16 of asw_consistency_native."""
    cons = consistent(d_ref, d_tar, 0, "native")
    return (np.where(cons, d_ref, d_tar).astype(np.int32),
            np.where(cons, d_ref, INVALID16).astype(np.uint16), cons)


def refine(L, R, D: int, cost, est_left, est_right, conf_ref, conf_tar, k: int, taps: int = 33,
           mode: str = "native") -> dict:
    """The loop on a plane-major volume ``cost`` [D][H][W].  est_left / est_right: the
    estimates of the two views entering the first iteration (u8 codes, or int32 indices in
    native mode); conf_ref / conf_tar: the confidences after the pre-refinement consistency
    check.  Inputs are not modified."""
    assert mode in ("u8", "native")
    H, W = conf_ref.shape
    cost = np.ascontiguousarray(cost, np.float32)
    el, er = est_left.copy(), est_right.copy()
    cr, ct = conf_ref.astype(np.float32).copy(), conf_tar.astype(np.float32).copy()
    dr = dt = None
    post = np.zeros((H, W, 4), np.uint8) if mode == "u8" else np.full((H, W), INVALID16, np.uint16)
    for _ in range(k):
        vl = ref_v(L, decode(el, D, mode), cr, taps)
        vr = ref_v(R, decode(er, D, mode), ct, taps)
        hl = ref_h(L, cr, vl, taps)
        hr = ref_h(R, ct, vr, taps)
        dr, dt, cr = O.wta_ref(cost, np.ascontiguousarray(hl), np.ascontiguousarray(hr))  # cr <- target confidence
        if mode == "u8":
            kl, er = O.code_u8(dr, D), O.code_u8(dt, D)
            cons = consistent(kl, er, D, mode)
            el = np.where(cons, kl, er)
            post = np.stack([np.where(cons, kl, 255), np.where(cons, kl, 0), np.where(cons, kl, 0),
                             np.full((H, W), 255)], axis=-1).astype(np.uint8)
        else:
            er = dt
            el, post, cons = native_est_left(dr, dt)
        cr = np.where(cons, cr, np.float32(0.0)).astype(np.float32)
        ct = np.where(cons, ct, np.float32(0.0)).astype(np.float32)
    med = median3(el)
    out = {"ref_d_ref": dr, "ref_d_tar": dt, "ref_conf_ref": cr, "ref_conf_tar": ct, "est_left": el}
    if mode == "u8":
        out["final_rgba"] = np.stack([med, med, med, np.full((H, W), 255, np.uint8)], axis=-1).astype(np.uint8)
        out["post_red_rgba"] = post
    else:
        out["final16"] = med.astype(np.uint16)
        out["post16"] = post
    return out


def refine_native_from_wta(L, R, D: int, cost, d_ref, d_tar, conf_ref, conf_tar, k: int, taps: int = 33) -> dict:
    """The native loop from pre-refinement maps: est_left by the native rule from the WTA's
    d_ref / d_tar, the right estimate d_tar, the confidences as given (after asw_consistency)."""
    el, _, _ = native_est_left(d_ref, d_tar)
    return refine(L, R, D, cost, el, d_tar.astype(np.int32), conf_ref, conf_tar, k, taps, "native")
