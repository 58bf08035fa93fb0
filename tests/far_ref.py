"""Crop references: the CPU reference of a stage on a pixel region, computed from the
region's CONE (the bounded part of the inputs the region depends on) instead of the whole
problem.  tests/test_gpu_far.py compares them with the far end of volumes of many GB, where
a whole-problem reference is out of reach; tests/test_far_ref.py proves every cone against
the whole-problem reference at small shapes (DESIGN.md §Far addressing).

Every function takes the FULL-PROBLEM inputs in the device layouts of include/asw.h (images
[H][W][4] uint8, volumes [H][W][>=D], supports [H][W][>=T], maps [H][W], estimates [2][H][W])
and a region, rows [y0, y1) (``cols=(x0, x1)`` where a stage recurs along y).  Inputs are
only ever sliced, then converted: a numpy array or a torch tensor on any device works, and of
a device tensor only the cone is copied to the host.  The arithmetic is that of the existing
reference modules (oracle, census_ref, cross_ref, sgm_ref, subpixel_ref, refine_native_ref,
wta_shard_ref): nothing is restated here but the cones.  Outputs are in the device layout,
restricted to the region and to the valid planes.

The cones are derived from the reference code:
  per pixel / row-local   the same rows (raw, census and cross costs, the H pass and support,
                          the H integral and oii-H, WTA own and target scans: xq <= x of the same
                          row, sub-pixel, fill, init, SGM paths 0 and 1)
  window                  rows [y0 - r, y1 + r) clamped into the image: r = R for the V pass and
                          support, the window's half height for census, 1 for the medians, Rr for
                          the V estimate, iters * Rr + 1 for the native loop, arm_max (+ 1 below)
                          for arms, vote and oii-V
  column-recursive        the same columns, every row (the V integral, SGM paths 2 and 3)
  SGM diagonals           a walker restarts where its column wraps, so (x, y) depends on the
                          W - 1 rows before it along the path: rows [y0 - (W-1), y1) for dy > 0,
                          [y0, y1 + (W-1)) for dy < 0, every column

``trim`` (negative controls only) makes a cone one row or column too small on its upstream
side; 0 everywhere else.
"""
from __future__ import annotations

import numpy as np

import census_ref
import cross_ref
import refine_native_ref
import sgm_ref
import subpixel_ref
import wta_shard_ref
from oracle import oracle as O


def host(a):
    """A contiguous numpy copy of an (already sliced) numpy array or torch tensor."""
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a)


def window(y0, y1, r, H, trim=0):
    """Rows [a, b) of the cone of rows [y0, y1) under a clamped +-r window, and the offset of
    y0 in it.  trim > 0 cuts the cone at its upper (smaller y) end."""
    a, b = max(0, y0 - r) + trim, min(H, y1 + r)
    return a, b, y0 - a


def _planes(vol, D):
    """device [h][w][>=D] -> the oracle's [D][h][w]"""
    return np.ascontiguousarray(np.transpose(host(vol)[:, :, :D], (2, 0, 1)))


def _pixels(vol):
    """[n][h][w] -> [h][w][n]"""
    return np.ascontiguousarray(np.transpose(vol, (1, 2, 0)))


def _u16(vol):
    v = host(vol)
    return v.view(np.uint16) if v.dtype == np.int16 else v


# ------------------------------------------------------------------ raw and census costs

def raw_cost(L, R, D, y0, y1, d_begin=0, d_end=None):
    """asw_raw_cost (untruncated AD): float32 [rows][W][d_end - d_begin]."""
    d_end = D if d_end is None else d_end
    return _pixels(O.raw_cost(host(L[y0:y1]), host(R[y0:y1]), D)[d_begin:d_end])


def raw_cost16(L, R, D, y0, y1, d_begin=0, d_end=None):
    """asw_raw_cost16: the same integers as uint16."""
    c = raw_cost(L, R, D, y0, y1, d_begin, d_end)
    assert c.max() <= 765 and np.array_equal(c, np.floor(c))
    return c.astype(np.uint16)


def census(img, y0, y1, win_w=9, win_h=7, trim=0):
    """asw_census: uint64 [rows][W]."""
    a, b, o = window(y0, y1, win_h // 2, img.shape[0], trim)
    return census_ref.census(host(img[a:b]), win_w, win_h)[o:o + y1 - y0]


def census_cost(L, R, D, y0, y1, u16=False, d_begin=0, d_end=None, trim=0, **cp):
    """asw_census_cost / asw_census_cost16 (u16): [rows][W][d_end - d_begin].  cp: tad_tau,
    win_w, win_h, ad_weight, census_weight of census_ref."""
    a, b, o = window(y0, y1, cp.get("win_h", 7) // 2, L.shape[0], trim)
    fn = census_ref.cost_u16 if u16 else census_ref.cost_f32
    return _pixels(fn(host(L[a:b]), host(R[a:b]), D, d_begin=d_begin, d_end=d_end, **cp)[:, o:o + y1 - y0])


# ------------------------------------------------------------------ supports and passes

def support(img, T, direction, y0, y1, trim=0):
    """asw_support (RGB): float32 [rows][W][T].  direction 0 = V, 1 = H."""
    a, b, o = window(y0, y1, T // 2 if direction == 0 else 0, img.shape[0], trim)
    return _pixels(O.support(host(img[a:b]), T, direction)[:, o:o + y1 - y0])


def aggregate_pass(sL, sR, cin, D, T, direction, y0, y1, d_begin=0, d_end=None, trim=0):
    """One aggregation pass over the planes [d_begin, d_end) that cin holds: float32
    [rows][W][d_end - d_begin].  sL / sR: supports [H][W][>=T]; cin: [H][W][>=n]."""
    d_end = D if d_end is None else d_end
    a, b, o = window(y0, y1, T // 2 if direction == 0 else 0, cin.shape[0], trim)
    out = O.aggregate_pass(_planes(sL[a:b], T), _planes(sR[a:b], T), _planes(cin[a:b], d_end - d_begin), T,
                           direction, d_begin, d_end, d_begin)
    return _pixels(out[:, o:o + y1 - y0])


# ------------------------------------------------------------------ WTA

def wta(C, D, y0, y1):
    """asw_wta: (d_ref, conf_ref, d_tar, conf_tar) of the rows."""
    return O.wta(_planes(C[y0:y1], D))


def wta_ref(C, ref_l, ref_r, D, y0, y1):
    """asw_wta_ref: (d_ref, d_tar, conf_ref <- the target confidence) of the rows."""
    return O.wta_ref(_planes(C[y0:y1], D), host(ref_l[:, y0:y1]), host(ref_r[:, y0:y1]))


def _t(a):
    import torch
    return torch.from_numpy(host(a))


def wta_local(Cl, b, e, D, y0, y1):
    """asw_wta_local of the shard [b, e) (Cl: its local planes): (key, m1, m2)."""
    return tuple(t.numpy() for t in wta_shard_ref.CpuShardOps(b, e, D).local(_t(Cl[y0:y1, :, :e - b])))


def wta_target_local(Cl, key_ref, b, e, D, y0, y1):
    """asw_wta_target_local: (tkey, t1, t2)."""
    ops = wta_shard_ref.CpuShardOps(b, e, D)
    return tuple(t.numpy() for t in ops.target_local(_t(Cl[y0:y1, :, :e - b]), _t(key_ref[y0:y1])))


def wta_second(key_g, key_l, m1, m2, y0, y1):
    """asw_wta_second."""
    return wta_shard_ref.CpuShardOps(0, 0, 0).second(*(_t(a[y0:y1]) for a in (key_g, key_l, m1, m2))).numpy()


def wta_finalize(key, m2, tkey, t2, D, y0, y1):
    """asw_wta_finalize: (d_ref, conf_ref, d_tar, conf_tar)."""
    return wta_shard_ref.CpuShardOps(0, D, D).finalize(*(_t(a[y0:y1]) for a in (key, m2, tkey, t2)))


def wta_ref_local(Cl, ref_l, b, e, D, y0, y1):
    """asw_wta_ref_local of the shard [b, e): (key, m1, m2) of the penalised values."""
    rl = host(ref_l[:, y0:y1])
    return tuple(t.numpy() for t in wta_shard_ref.CpuRefShardOps(b, e, D, rl, rl).ref_local(_t(Cl[y0:y1, :, :e - b])))


def wta_ref_target_local(Cl, ref_r, key_ref, b, e, D, y0, y1):
    """asw_wta_ref_target_local: (tkey, t1, t2)."""
    rr = host(ref_r[:, y0:y1])
    ops = wta_shard_ref.CpuRefShardOps(b, e, D, rr, rr)
    return tuple(t.numpy() for t in ops.ref_target_local(_t(Cl[y0:y1, :, :e - b]), _t(key_ref[y0:y1])))


def wta_ref_finalize(key, tkey, t2, D, y0, y1):
    """asw_wta_ref_finalize: (d_ref, d_tar, conf_ref <- the target confidence)."""
    ops = wta_shard_ref.CpuRefShardOps(0, D, D, None, None)
    return ops.ref_finalize(*(_t(a[y0:y1]) for a in (key, tkey, t2)))


def consistency(code_ref, code_tar, conf_ref, conf_tar, D, y0, y1):
    """asw_consistency with the 8-bit rule (ASW_LR_U8): (out_rgba, out_red_rgba, conf_ref,
    conf_tar) of the rows; the confidences are the zeroed copies."""
    return O.consistency(host(code_ref[y0:y1]), host(code_tar[y0:y1]), host(conf_ref[y0:y1]), host(conf_tar[y0:y1]), D)


# ------------------------------------------------------------------ sub-pixel maps

def subpixel(C, d_ref, D, y0, y1):
    return subpixel_ref.subpixel_D(host(C[y0:y1]), host(d_ref[y0:y1]), D)


def subpixel_local(Cl, key_g, b, e, D, y0, y1):
    return subpixel_ref.local_neighbours(host(Cl[y0:y1]), host(key_g[y0:y1]), b, e, D)


def subpixel_finalize(key_g, nb, D, y0, y1):
    return subpixel_ref.finalize(host(key_g[y0:y1]), host(nb[:, y0:y1]), D)


def disp_mask(disp, d_ref, d_tar, code_ref, code_tar, D, mode, y0, y1):
    ok = subpixel_ref.lr_pass(*(None if a is None else host(a[y0:y1]) for a in (d_ref, d_tar, code_ref, code_tar)),
                              D, mode)
    return subpixel_ref.mask(host(disp[y0:y1]), ok)


def disp_fill(disp_lr, y0, y1):
    return subpixel_ref.fill(host(disp_lr[y0:y1]))


# ------------------------------------------------------------------ native refinement

def median3(a, y0, y1, trim=0):
    """asw_median3_u16 / asw_median3 of a map [H][W]: the 3x3 clamp-to-edge median."""
    lo, hi, o = window(y0, y1, 1, a.shape[0], trim)
    return refine_native_ref.median3(host(a[lo:hi]))[o:o + y1 - y0]


def ref_v_native(img, est, conf, taps, y0, y1, trim=0):
    """asw_ref_v_native: float32 [2][rows][W]."""
    a, b, o = window(y0, y1, taps // 2, conf.shape[0], trim)
    out = refine_native_ref.ref_v(host(img[a:b]), host(est[a:b]).astype(np.float32), host(conf[a:b]), taps)
    return out[:, o:o + y1 - y0]


def ref_h(img, conf, est_v, taps, y0, y1):
    """asw_ref_h: float32 [2][rows][W]."""
    return refine_native_ref.ref_h(host(img[y0:y1]), host(conf[y0:y1]), host(est_v[:, y0:y1]), taps)


def consistency_native(d_ref, d_tar, y0, y1):
    """asw_consistency_native: (est_left, post16, cons)."""
    return refine_native_ref.native_est_left(host(d_ref[y0:y1]), host(d_tar[y0:y1]))


def refine_native(L, R, D, cost, est_left, d_tar, conf_ref, conf_tar, iters, taps, y0, y1, trim=0):
    """asw_refine_native: the dict of refine_native_ref.refine, every map cut to the rows.
    Each iteration widens the cone by the V estimate's half window, the final median by 1."""
    a, b, o = window(y0, y1, iters * (taps // 2) + 1, conf_ref.shape[0], trim)
    res = refine_native_ref.refine(host(L[a:b]), host(R[a:b]), D, _planes(cost[a:b], D), host(est_left[a:b]),
                                   host(d_tar[a:b]), host(conf_ref[a:b]), host(conf_tar[a:b]), iters, taps, "native")
    return {k: v[o:o + y1 - y0] for k, v in res.items() if v is not None}


# ------------------------------------------------------------------ cross-based matcher

def median3_rgba(img, y0, y1, trim=0):
    a, b, o = window(y0, y1, 1, img.shape[0], trim)
    return cross_ref.median3_rgba(host(img[a:b]))[o:o + y1 - y0]


def cross_arms(med, arm_max, tau, y0, y1, trim=0):
    """asw_cross_arms: a vertical arm tests pixels up to arm_max + 1 rows away."""
    a, b, o = window(y0, y1, arm_max + 1, med.shape[0], trim)
    return cross_ref.cross_arms(host(med[a:b]), arm_max, tau)[o:o + y1 - y0]


def cross_cost(ml, mr, D, y0, y1):
    return cross_ref.cost_volume(host(ml[y0:y1]), host(mr[y0:y1]), D)


def cross_integral_h(vol, D, y0, y1, trim=0):
    """Integral_h of the rows: [rows][W - trim][D] (trim drops the first columns: the sums
    then start too late)."""
    return cross_ref.integral(host(vol[y0:y1, trim:, :D]), "h")


def cross_integral_v(vol, D, x0, x1, trim=0):
    """Integral_v of the columns [x0, x1), every row: [H - trim][cols][D]."""
    return cross_ref.integral(host(vol[trim:, x0:x1, :D]), "v")


def cross_oii(vol, arms_l, arms_r, D, direction, arm_max, y0, y1, trim=0):
    """asw_cross_oii: 'h' is row-local; 'v' reads rows y + pl <= y + arm_max and
    y + m - 1 >= y - arm_max - 1."""
    a, b, o = window(y0, y1, arm_max + 1 if direction == "v" else 0, vol.shape[0], trim)
    out = cross_ref.oii(host(vol[a:b, :, :D]), host(arms_l[a:b]), host(arms_r[a:b]), direction)
    return out[o:o + y1 - y0]


def cross_init(vol, D, y0, y1):
    return cross_ref.init_disparity(host(vol[y0:y1, :, :D]))


def cross_vote(code0, arms_l, D, arm_max, y0, y1, trim=0):
    """asw_cross_vote: the region rows y + i, |i| <= arm_max, every column."""
    a, b, o = window(y0, y1, arm_max, code0.shape[0], trim)
    d1, c1 = cross_ref.vote(host(code0[a:b]), host(arms_l[a:b]), D)
    return d1[o:o + y1 - y0], c1[o:o + y1 - y0]


# ------------------------------------------------------------------ semi-global matching

def sgm_path(C16, k, p1, p2, D, rows, cols, trim=0):
    """L_k of asw_sgm_path on the region rows x cols: int64 [rows][cols][D].  C16: the uint16
    raw costs [H][W][>=D] (int16 storage accepted)."""
    (y0, y1), (x0, x1) = rows, cols
    H, W = C16.shape[:2]
    dx, dy = sgm_ref.STEPS[k]
    if dy == 0:  # row walkers: the rows, every column; upstream is x = 0 (dx > 0) or x = W - 1
        xa, xb = (trim, W) if dx > 0 else (0, W - trim)
        L = sgm_ref.path(_planes(_u16(C16[y0:y1, xa:xb]), D), k, p1, p2)
        return _pixels(L)[:, x0 - xa:x1 - xa]
    if dx == 0:  # column walkers: the columns, every row; upstream is y = 0 (dy > 0) or y = H - 1
        ya, yb = (trim, H) if dy > 0 else (0, H - trim)
        L = sgm_ref.path(_planes(_u16(C16[ya:yb, x0:x1]), D), k, p1, p2)
        return _pixels(L)[y0 - ya:y1 - ya]
    # diagonal walkers restart where the column wraps: at most W - 1 steps back along the path
    if dy > 0:
        ya, yb = max(0, y0 - (W - 1)) + trim, y1
    else:
        ya, yb = y0, min(H, y1 + (W - 1)) - trim
    L = sgm_ref.path(_planes(_u16(C16[ya:yb]), D), k, p1, p2)
    return _pixels(L)[y0 - ya:y1 - ya, x0:x1]


def sgm(C16, paths, p1, p2, D, rows, cols):
    """S of asw_sgm on the region: int64 [rows][cols][D]."""
    assert sgm_ref.params_ok(paths, p1, p2)
    return sum(sgm_path(C16, k, p1, p2, D, rows, cols) for k in range(paths))


# ------------------------------------------------------------------ bands

def bands(H, row_elems, itemsize, nrows=2):
    """The row bands a far test compares: the first rows, the rows straddling each 32-bit
    limit the [H][row_elems] volume of `itemsize`-byte elements crosses, and the last rows.
    Returns [(name, y0, y1, limits)], limits = [(limit, bytes per counted unit)]: the band holds
    offsets on both sides of every one of them (limits that fall into the same rows share a
    band)."""
    total = H * row_elems
    out = {(0, min(nrows, H)): ["first", []]}
    for name, limit, unit in (("byte 2^31", 1 << 31, itemsize), ("byte 2^32", 1 << 32, itemsize),
                              ("element 2^31", 1 << 31, 1), ("element 2^32", 1 << 32, 1)):
        if total * unit <= limit:
            continue
        row = row_elems * unit
        y = limit // row  # the row that holds the limit (or starts at it: then the row before too)
        y0 = max(0, min(y - (nrows - 1) // 2 - (1 if limit % row == 0 else 0), H - nrows))
        y1 = y0 + nrows
        assert y0 * row < limit < y1 * row, (name, y0, y1)
        ent = out.setdefault((y0, y1), [name, []])
        if ent[1] and name not in ent[0]:
            ent[0] += " + " + name
        elif not ent[1] and ent[0] != name:
            ent[0] += " + " + name
        ent[1].append((limit, unit))
    ent = out.setdefault((max(0, H - nrows), H), ["last", []])
    if ent[0] != "last":
        ent[0] += " + last"
    return [(n, y0, y1, lim) for (y0, y1), (n, lim) in sorted(out.items())]
