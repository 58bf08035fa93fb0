"""numpy restatement of the reference's cross-based matcher (main.cpp:243-411), the CPU
oracle of stereo_matchin_amd/csrc/asw_cross.hip.

Every float operation is an IEEE float32 one in the reference's order (DESIGN.md
§Cross-based); ``np.add.accumulate(..., dtype=float32)`` is the serial running sum of the
two integral kernels.  Volumes are [H][W][D] float32 (the device layout without its pitch
padding), arm maps int8 [H][W][4] = (h-, h+, v-, v+), images uint8 [H][W][4].
"""
from __future__ import annotations

import numpy as np

F = np.float32


def code_u8(d, D: int):
    """8-bit code of index d for D levels (round-half-down of 255 d / (D-1), asw_common.h)."""
    d = np.asarray(d, np.int64)
    return np.clip((510 * d + (D - 2)) // (2 * (D - 1)), 0, 255).astype(np.uint8)


def code_index(c, D: int):
    """K/disparity.cl:28-29: (int)(((float)c / 255.0f) * (float)(D-1)), truncated."""
    c = np.asarray(c)
    return ((c.astype(F) / F(255.0)) * F(D - 1)).astype(np.int32)


def _neighbourhood(a: np.ndarray):
    """the 9 clamp-to-edge 3x3 neighbours of every pixel, stacked on a new first axis"""
    H, W = a.shape[:2]
    ys = np.clip(np.arange(H)[:, None] + np.array([-1, 0, 1])[None, :], 0, H - 1)  # [H][3]
    xs = np.clip(np.arange(W)[:, None] + np.array([-1, 0, 1])[None, :], 0, W - 1)
    return np.stack([a[ys[:, i]][:, xs[:, j]] for i in range(3) for j in range(3)])


def median3_rgba(img: np.ndarray) -> np.ndarray:
    """Median (K/median.cl:58-88): per-channel 3x3 median, clamp-to-edge, alpha 255."""
    out = np.sort(_neighbourhood(np.asarray(img, np.uint8)), axis=0)[4]
    out[..., 3] = 255
    return np.ascontiguousarray(out)


def median3_codes(codes: np.ndarray) -> np.ndarray:
    """The same median of a one-channel code image (the final Median, main.cpp:352-354)."""
    return np.ascontiguousarray(np.sort(_neighbourhood(np.asarray(codes, np.uint8)), axis=0)[4])


def cross_arms(med: np.ndarray, arm_max: int = 25, tau: int = 25) -> np.ndarray:
    """Cross (K/cross.cl): per direction a = 1; for k = 1..arm_max the pixel at distance
    k+1 is accepted (a = k) when it is inside the image, k - a <= 1 and every colour
    channel is within tau of the ANCHOR pixel."""
    m = np.asarray(med, np.uint8)[..., :3].astype(np.int32)
    H, W = m.shape[:2]
    yy, xx = np.mgrid[0:H, 0:W]
    arms = np.empty((H, W, 4), np.int8)
    for slot, (dx, dy, sign) in enumerate(((-1, 0, -1), (1, 0, 1), (0, -1, -1), (0, 1, 1))):
        a = np.ones((H, W), np.int32)
        for k in range(1, arm_max + 1):
            qx, qy = xx + (k + 1) * dx, yy + (k + 1) * dy
            inside = (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
            q = m[np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)]
            similar = (np.abs(q - m) <= tau).all(-1)
            a = np.where(inside & similar & (k - a <= 1), k, a)
        arms[..., slot] = sign * a
    return arms


def cost_volume(med_l: np.ndarray, med_r: np.ndarray, D: int) -> np.ndarray:
    """Aggregation (K/aggregation.cl): (|dr| + |dg|) + |db| of the channels / 255."""
    l = np.asarray(med_l, np.uint8)[..., :3].astype(F) / F(255.0)
    r = np.asarray(med_r, np.uint8)[..., :3].astype(F) / F(255.0)
    H, W = l.shape[:2]
    C = np.empty((H, W, D), F)
    x = np.arange(W)
    for d in range(D):
        diff = np.abs(l - r[:, np.maximum(x - d, 0)])
        C[:, :, d] = (diff[..., 0] + diff[..., 1]) + diff[..., 2]
    return C


def integral(vol: np.ndarray, direction: str) -> np.ndarray:
    """Integral_h ('h': along x from x = 0) / Integral_v ('v': along y from y = 0)."""
    return np.add.accumulate(np.asarray(vol, F), axis=1 if direction == "h" else 0, dtype=F)


def oii(vol: np.ndarray, arms_l: np.ndarray, arms_r: np.ndarray, direction: str) -> np.ndarray:
    """Oii_hcross / Oii_vcross (K/oii_hcross.cl:13-31) of an integral volume."""
    H, W, D = vol.shape
    lo_slot, hi_slot = (0, 1) if direction == "h" else (2, 3)
    y, x, d = np.meshgrid(np.arange(H), np.arange(W), np.arange(D), indexing="ij")
    xr = np.maximum(x - d, 0)
    al, ar = arms_l.astype(np.int32), arms_r.astype(np.int32)
    m = np.maximum(ar[y, xr, lo_slot], al[y, x, lo_slot])
    pl = np.minimum(ar[y, xr, hi_slot], al[y, x, hi_slot])
    if direction == "h":
        a = vol[y, np.minimum(W - 1, x + pl), d]
        b = vol[y, np.maximum(0, x + m - 1), d]
    else:
        a = vol[np.minimum(H - 1, y + pl), x, d]
        b = vol[np.maximum(0, y + m - 1), x, d]
    return ((a - b).astype(F) / (pl - m).astype(F)).astype(F)


def init_disparity(vol: np.ndarray):
    """Init_disparity: the first strict minimum over d, and its code."""
    d0 = np.argmin(vol, axis=2).astype(np.int32)
    return d0, code_u8(d0, vol.shape[2])


def vote(code0: np.ndarray, arms_l: np.ndarray, D: int):
    """Disparity (K/disparity.cl): histogram of idx(code0) over the cross region of every
    pixel, the LAST bin with the largest count.  Vectorised over pixels: one step per
    (row offset, column offset) pair inside the largest arms."""
    H, W = code0.shape
    a = arms_l.astype(np.int32)
    idx = code_index(code0, D)
    tab = np.zeros((H, W, D), np.int32)
    yy, xx = np.mgrid[0:H, 0:W]
    flat = (yy * W + xx) * D
    tabf = tab.reshape(-1)
    for i in range(int(a[..., 2].min()), int(a[..., 3].max()) + 1):
        rows = (i >= a[..., 2]) & (i <= a[..., 3])
        if not rows.any():
            continue
        yc = np.clip(yy + i, 0, H - 1)
        hm, hp = a[yc, xx, 0], a[yc, xx, 1]
        for j in range(int(hm[rows].min()), int(hp[rows].max()) + 1):
            sel = rows & (j >= hm) & (j <= hp)
            if not sel.any():
                continue
            b = idx[yc, np.clip(xx + j, 0, W - 1)]
            tabf[(flat + b)[sel]] += 1  # one entry per pixel: no duplicate index in a step
    d1 = (D - 1 - np.argmax(tab[:, :, ::-1], axis=2)).astype(np.int32)
    return d1, code_u8(d1, D)


def match(left: np.ndarray, right: np.ndarray, D: int = 61, arm_max: int = 25, tau: int = 25,
          want_volumes: bool = False) -> dict:
    """The whole sequence on an RGBA8 pair."""
    ml, mr = median3_rgba(left), median3_rgba(right)
    al, ar = cross_arms(ml, arm_max, tau), cross_arms(mr, arm_max, tau)
    C = cost_volume(ml, mr, D)
    Ih = integral(C, "h")
    T = oii(Ih, al, ar, "h")
    Iv = integral(T, "v")
    A = oii(Iv, al, ar, "v")
    d0, code0 = init_disparity(A)
    d1, code1 = vote(code0, al, D)
    out = {"median_l": ml, "median_r": mr, "arms_l": al, "arms_r": ar, "d_initial": d0, "code_initial": code0,
           "d_final": d1, "code_final": code1, "final": median3_codes(code1)}
    if want_volumes:
        out.update(cost=C, integral_h=Ih, oii_h=T, integral_v=Iv, oii_v=A)
    return out
