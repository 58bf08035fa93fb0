"""Every stage kernel past the 2^31 / 2^32 byte and element limits — run on an MI355X.

Volumes here are 4 to 17 GB: the index ((y*W + x)*Dp + d) crosses byte offset 2^31 and 2^32
and element index 2^31 and 2^32.  A whole-problem CPU reference is out of reach, so each
stage is compared bit for bit with its crop reference (tests/far_ref.py, proven on the CPU by
tests/test_far_ref.py) on a few row bands: the first rows, the rows straddling every limit
the volume crosses, and the last rows (DESIGN.md §Far addressing).  Inputs are made on the
device from a seeded generator; only cones and crops are copied to the host.

Tiers (the smallest shapes that cross the limits, within what the entry points accept):
  1  1021 x 4112, D 250 (Dp 256): 1.07 G elements; float32 4.3 GB crosses byte 2^31 and 2^32,
     uint16 2.1 GB crosses byte 2^31
  2  1024 x 8200, D 500 (Dp 512), or 1024 x 16400, D 250 (Dp 256) for the stages built for
     pitches up to 256: 4.3 G elements; float32 17.2 GB and uint16 8.6 GB cross all four limits
SGM uses narrow shapes (256 x 16400 and 256 x 65600, D 250) so that a diagonal cone is 255 rows.

What cannot reach a limit, and is therefore not here: every stage that reads and writes maps
only (consistency, asw_disp_mask / _fill, the medians, asw_ref_v_native, asw_ref_h,
asw_consistency_native, asw_cross_arms, asw_cross_vote, asw_wta_second / _finalize,
asw_subpixel_finalize): W * H <= 2^25 pixels of at most 16 bytes stay below 2^29 bytes.
asw_cross_cost and asw_cross_oii launch one work-item per element and are rejected from
2^32 - 255 elements on (test_cross_rejects_what_a_launch_cannot_hold): they run at tier 1 and
at 1024 x 8200 x 256, past element 2^31; the integrals and asw_cross_init hold more and run
past 2^32 elements too.  The 32-plane shard passes hold at most 2^25 pixels * 32 planes * 4 bytes = exactly 2^32 bytes: they
cross byte 2^31 and end at byte 2^32.
"""
import ctypes

import numpy as np
import pytest

import far_ref as F
from guarded import guarded_kernels  # noqa: F401  (a fixture, used by name)

# every map or volume the wrappers allocate is guarded and poisoned (tests/guarded.py); the
# volumes allocated here are filled with NaN (or 0xFFFF) before the kernel under test runs, so
# a far row that a wrapped offset left unwritten cannot pass
pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("guarded_kernels")]

TIER1 = (1021, 4112, 250)
TIER2_DEEP = (1024, 8200, 500)
TIER2_256 = (1024, 16400, 250)
NROWS = 2


def _torch():
    import torch
    return torch


def params(W, H, D, T=5, **kw):
    from stereo_matchin_amd import _lib
    return _lib.default_params(W, H, ndisp=D, taps=T, iters=1, **kw)


def need(nbytes):
    """The one permitted skip: a busy shared card with less free memory than the case holds."""
    assert nbytes <= 64 << 30, "no case may hold more than 64 GiB"
    free, _ = _torch().cuda.mem_get_info()
    if free < nbytes + (1 << 30):
        pytest.skip(f"needs {nbytes + (1 << 30)} bytes of device memory, {free} bytes are free")


def release():
    import gc
    gc.collect()
    _torch().cuda.empty_cache()


def gen(dev, seed):
    g = _torch().Generator(device=dev)
    g.manual_seed(seed)
    return g


def fill(t, g, hi, scale=None):
    """t <- random integers in [0, hi) (times scale for floats), in slabs of 2^27 elements."""
    torch = _torch()
    flat = t.view(-1)
    step = 1 << 27
    for o in range(0, flat.numel(), step):
        v = flat[o:o + step]
        r = torch.randint(0, hi, (v.numel(),), generator=g, device=t.device, dtype=torch.int32)
        v.copy_(r.to(t.dtype) * scale if scale is not None else r)
    return t


def cost_f32(shape, dev, g):
    """random float costs in [0, 700), quarter steps (exact ties), padding planes included"""
    return fill(_torch().empty(shape, dtype=_torch().float32, device=dev), g, 2800, 0.25)


def cost_u16(shape, dev, g):
    """random uint16 costs below 765 (int16 storage)"""
    return fill(_torch().empty(shape, dtype=_torch().int16, device=dev), g, 765)


def image(H, W, dev, g):
    return _torch().randint(0, 256, (H, W, 4), generator=g, device=dev, dtype=_torch().uint8)


def unit(H, W, n, dev, g):
    """random floats in (0, 1]: supports and confidences"""
    t = _torch().empty((H, W, n) if n else (H, W), dtype=_torch().float32, device=dev)
    return fill(t, g, 1 << 20, 1.0 / (1 << 20)).add_(1.0 / (1 << 20))


def far_bands(shape, itemsize, want_limits):
    """The bands of a [H][W][Dp] volume; asserts that it crosses exactly `want_limits` of
    ('b31', 'b32', 'e31', 'e32') and that each straddle band spans its limit."""
    H, W, Dp = shape
    bs = F.bands(H, W * Dp, itemsize, NROWS)
    names = {(1 << 31, itemsize): "b31", (1 << 32, itemsize): "b32", (1 << 31, 1): "e31", (1 << 32, 1): "e32"}
    seen = set()
    for name, y0, y1, limits in bs:
        for limit, u in limits:
            first, last = y0 * W * Dp * u, (y1 * W * Dp - 1) * u  # offsets of the band's first and last element
            assert first < limit <= last, (name, y0, y1)
            seen.add(names[(limit, u)])
    assert seen == set(want_limits), (seen, want_limits)
    assert bs[-1][2] == H
    return [(name, y0, y1) for name, y0, y1, _ in bs]


def bits(a):
    a = np.ascontiguousarray(F.host(a))
    return a.view(np.uint8).reshape(-1)


def same(got, want, what):
    got, want = np.ascontiguousarray(F.host(got)), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if not np.array_equal(bits(got), bits(want)):
        bad = np.argwhere(got != want)
        raise AssertionError(f"{what}: {len(bad)} elements differ, first at {bad[:4].tolist()}")


def padding_is_zero(vol, n, y0, y1, what):
    pad = vol[y0:y1, :, n:]
    assert pad.numel() == 0 or int(_torch().count_nonzero(pad.view(_torch().int16 if pad.dtype == _torch().int16
                                                                    else _torch().int32))) == 0, what


LIMITS_F32 = {TIER1: ("b31", "b32"), TIER2_DEEP: ("b31", "b32", "e31", "e32"), TIER2_256: ("b31", "b32", "e31", "e32")}
LIMITS_U16 = {TIER1: ("b31",), TIER2_DEEP: ("b31", "b32", "e31", "e32"), TIER2_256: ("b31", "b32", "e31", "e32")}
ids = lambda s: "x".join(map(str, s))  # noqa: E731


# ------------------------------------------------------------------ raw and census costs

@pytest.mark.parametrize("shape", [TIER1, TIER2_DEEP], ids=ids)
def test_raw_and_census_costs(gpu, oracle, shape):
    """asw_raw_cost, asw_raw_cost16, asw_census_cost and asw_census_cost16, one volume at a time."""
    import stereo_matchin_amd.kernels as K
    from stereo_matchin_amd import _lib
    torch = _torch()
    W, H, D = shape
    p = params(W, H, D)
    vs = K.cost_shape(p)
    need(vs[0] * vs[1] * vs[2] * 4 + (64 << 20) * 4)
    g = gen(gpu, 11)
    L, R = image(H, W, gpu, g), image(H, W, gpu, g)
    cen = dict(tad_tau=765.0, win_w=9, win_h=7, ad_weight=1, census_weight=8)
    cp = _lib.default_census_params()
    try:
        cl, cr = K.census(p, cp, L), K.census(p, cp, R)
        for y0, y1 in ((0, NROWS), (H // 2, H // 2 + NROWS), (H - NROWS, H)):  # (a map: no limit to cross)
            same(cl[y0:y1].view(torch.uint8), F.census(L, y0, y1).view(np.uint8), f"census rows {y0}")
        for kind in ("raw", "raw16", "census", "census16"):
            u16 = kind.endswith("16")
            out = torch.full(vs, -1 if u16 else float("nan"), dtype=torch.int16 if u16 else torch.float32, device=gpu)
            if kind == "raw":
                K.asw_Aggr(p, L, R, out)
            elif kind == "raw16":
                K.asw_Aggr16(p, L, R, out)
            elif kind == "census":
                K.census_cost(p, cp, L, R, cl, cr, out)
            else:
                K.census_cost16(p, cp, L, R, cl, cr, out)
            for name, y0, y1 in far_bands(vs, 2 if u16 else 4, (LIMITS_U16 if u16 else LIMITS_F32)[shape]):
                if kind.startswith("raw"):
                    want = (F.raw_cost16 if u16 else F.raw_cost)(L, R, D, y0, y1)
                else:
                    want = F.census_cost(L, R, D, y0, y1, u16=u16, **cen)
                got = F.host(out[y0:y1, :, :D])
                same(got.view(np.uint16) if u16 else got, want, f"{kind} {name} rows {y0}..{y1}")
                padding_is_zero(out, D, y0, y1, f"{kind} {name} padding planes")
            del out
            release()
    finally:
        del L, R
        release()


def test_tall_image_rows_past_65535(gpu, oracle):
    """The row-per-block kernels put the image row in the grid's y: a tall frame (legal:
    W * H <= 2^25) has more than 65535 rows."""
    import stereo_matchin_amd.kernels as K
    W, H, D = 64, 65600, 16
    p = params(W, H, D)
    g = gen(gpu, 12)
    L, R = image(H, W, gpu, g), image(H, W, gpu, g)
    try:
        out = K.asw_Aggr16(p, L, R)
        for y0, y1 in ((0, 2), (65534, 65537), (H - 2, H)):
            same(F.host(out[y0:y1, :, :D]).view(np.uint16), F.raw_cost16(L, R, D, y0, y1), f"rows {y0}")
        sup = K.asw_vSupport(p, L)
        for y0, y1 in ((65534, 65537), (H - 2, H)):
            same(sup[y0:y1, :, :5], F.support(L, 5, 0, y0, y1), f"support rows {y0}")
    finally:
        del L, R
        release()


# ------------------------------------------------------------------ aggregation passes

def expected_kernel(direction, T, dm, c16=False):
    nt = ",nt"  # every far volume is past the 256 MB streaming threshold
    if direction == 0:
        shape = "NW=16" if T <= 35 else "NW=12,NPH=3,TK=4"
        return f"{'k_vpass10_c16' if c16 else 'k_vpass10'}<T={T},{shape},DM={dm}{nt}>"
    if T <= 35:
        return f"k_hpass11<T={T},NKW=4,DM={dm}{nt}>"
    return f"k_hpass11<T={T},{'NKW=2,PX=24' if dm == 2 else 'NKW=2'},DM={dm}{nt}>"


@pytest.mark.parametrize("T", [5, 35, 51])
@pytest.mark.parametrize("shape", [TIER1, TIER2_DEEP], ids=ids)
def test_ring_passes(gpu, oracle, shape, T):
    """V and H ring passes in the three den modes, and the uint16 first V pass, each against
    the same crop reference; the kernel forms are asserted by name."""
    import stereo_matchin_amd.kernels as K
    from stereo_matchin_amd import _lib
    torch = _torch()
    W, H, D = shape
    p = params(W, H, D, T)
    vs, ss = K.cost_shape(p), K.support_shape(p)
    vol = vs[0] * vs[1] * vs[2] * 4
    need(3 * vol + 2 * ss[0] * ss[1] * ss[2] * 4 + (1 << 30))
    g = gen(gpu, 20 + T)
    try:
        wl, wr = unit(H, W, ss[2], gpu, g), unit(H, W, ss[2], gpu, g)
        cin = cost_f32(vs, gpu, g)
        out = torch.empty(vs, dtype=torch.float32, device=gpu)
        den = torch.empty(vs, dtype=torch.float32, device=gpu)
        bands = far_bands(vs, 4, LIMITS_F32[shape])
        for direction in (0, 1):
            fn = K.asw_vCostAggregation if direction == 0 else K.asw_hCostAggregation
            want = {}
            for dm in (_lib.DEN_WRITE, _lib.DEN_READ, _lib.DEN_NONE):
                out.fill_(float("nan"))
                fn(p, wl, wr, cin, out, den if dm else None, dm)
                assert K.pass_kernel(direction, dm) == expected_kernel(direction, T, dm)
                for name, y0, y1 in bands:
                    if name not in want:
                        want[name] = F.aggregate_pass(wl, wr, cin, D, T, direction, y0, y1)
                    same(out[y0:y1, :, :D], want[name], f"dir {direction} den mode {dm} {name} rows {y0}..{y1}")
        # the first V pass over a uint16 volume: the same pass over the float values of the integers
        c16 = K.cost16_view(den)  # (the den volume's memory: DEN_NONE does not touch it)
        fill(c16, g, 765)
        for y0 in range(0, H, 512):  # cin <- (float)c16, in row slabs
            cin[y0:y0 + 512].copy_(c16[y0:y0 + 512].view(torch.int16))
        out.fill_(float("nan"))
        K.asw_vCostAggregation16(p, wl, wr, c16, out)
        assert K.pass_kernel(0, 0) == expected_kernel(0, T, 0, c16=True)
        for name, y0, y1 in bands:
            same(out[y0:y1, :, :D], F.aggregate_pass(wl, wr, cin, D, T, 0, y0, y1), f"uint16 first pass {name}")
        # its own volume crosses its own limits at other rows
        for name, y0, y1 in far_bands(vs, 2, LIMITS_U16[shape]):
            same(out[y0:y1, :, :D], F.aggregate_pass(wl, wr, cin, D, T, 0, y0, y1), f"uint16 first pass, its {name}")
    finally:
        wl = wr = cin = out = den = c16 = None
        release()


@pytest.mark.parametrize("shape", [TIER1, TIER2_DEEP], ids=ids)
def test_hpass9_streaming_form(gpu, oracle, tune_variant, shape):
    """k_hpass9 with nt streams: the default dispatch gives every far volume to k_hpass11, so
    the form is selected through the tuning hook (variant bit 128)."""
    import stereo_matchin_amd.kernels as K
    torch = _torch()
    W, H, D = shape
    T = 35
    p = params(W, H, D, T)
    vs, ss = K.cost_shape(p), K.support_shape(p)
    need(2 * vs[0] * vs[1] * vs[2] * 4 + 2 * ss[0] * ss[1] * ss[2] * 4 + (1 << 30))
    g = gen(gpu, 29)
    try:
        wl, wr = unit(H, W, ss[2], gpu, g), unit(H, W, ss[2], gpu, g)
        cin = cost_f32(vs, gpu, g)
        out = torch.full(vs, float("nan"), dtype=torch.float32, device=gpu)
        tune_variant(128)
        K.asw_hCostAggregation(p, wl, wr, cin, out)
        assert K.pass_kernel(1, 0) == f"k_hpass9<T={T},NW=4,DM=0,nt>"
        for name, y0, y1 in far_bands(vs, 4, LIMITS_F32[shape]):
            same(out[y0:y1, :, :D], F.aggregate_pass(wl, wr, cin, D, T, 1, y0, y1), name)
    finally:
        wl = wr = cin = out = None
        release()


@pytest.mark.parametrize("shape", [TIER1, TIER2_DEEP], ids=ids)
def test_generic_pass(gpu, oracle, shape):
    """k_pass_any (a tap count without a ring kernel), V and H."""
    import stereo_matchin_amd.kernels as K
    torch = _torch()
    W, H, D = shape
    T = 11
    p = params(W, H, D, T)
    vs, ss = K.cost_shape(p), K.support_shape(p)
    need(2 * vs[0] * vs[1] * vs[2] * 4 + 2 * ss[0] * ss[1] * ss[2] * 4 + (1 << 30))
    g = gen(gpu, 31)
    try:
        wl, wr = unit(H, W, ss[2], gpu, g), unit(H, W, ss[2], gpu, g)
        cin = cost_f32(vs, gpu, g)
        out = torch.empty(vs, dtype=torch.float32, device=gpu)
        for direction in (0, 1):
            out.fill_(float("nan"))
            (K.asw_vCostAggregation if direction == 0 else K.asw_hCostAggregation)(p, wl, wr, cin, out)
            for name, y0, y1 in far_bands(vs, 4, LIMITS_F32[shape]):
                same(out[y0:y1, :, :D], F.aggregate_pass(wl, wr, cin, D, T, direction, y0, y1),
                     f"dir {direction} {name}")
    finally:
        wl = wr = cin = out = None
        release()


def test_pitch32_passes(gpu, oracle):
    """The half-wave passes of a 32-plane shard.  2^25 pixels * 32 planes * 4 bytes is exactly
    2^32 bytes: the volume crosses byte 2^31 and its last element ends at byte 2^32."""
    import stereo_matchin_amd.kernels as K
    from stereo_matchin_amd import _lib
    torch = _torch()
    W, H, D, T = 2048, 16384, 96, 9
    b, e = 40, 72
    p = params(W, H, D, T, d_begin=b, d_end=e)
    vs, ss = K.cost_shape(p), K.support_shape(p)
    assert vs[2] == 32 and vs[0] * vs[1] * vs[2] * 4 == 1 << 32
    need(3 * (1 << 32) + 2 * ss[0] * ss[1] * ss[2] * 4 + (1 << 30))
    g = gen(gpu, 37)
    try:
        wl, wr = unit(H, W, ss[2], gpu, g), unit(H, W, ss[2], gpu, g)
        cin = cost_f32(vs, gpu, g)
        out = torch.empty(vs, dtype=torch.float32, device=gpu)
        den = torch.empty(vs, dtype=torch.float32, device=gpu)
        bands = far_bands(vs, 4, ("b31",))
        for direction in (0, 1):
            fn = K.asw_vCostAggregation if direction == 0 else K.asw_hCostAggregation
            want = {}
            for dm in (_lib.DEN_WRITE, _lib.DEN_READ, _lib.DEN_NONE):
                out.fill_(float("nan"))
                fn(p, wl, wr, cin, out, den if dm else None, dm)
                assert K.pass_kernel(direction, dm).startswith(("k_vpass32<", "k_hpass32<")[direction])
                for name, y0, y1 in bands:
                    if name not in want:
                        want[name] = F.aggregate_pass(wl, wr, cin, D, T, direction, y0, y1, b, e)
                    same(out[y0:y1], want[name], f"dir {direction} den mode {dm} {name}")
    finally:
        wl = wr = cin = out = den = None
        release()


# ------------------------------------------------------------------ WTA, sub-pixel, asw_wta_ref

@pytest.mark.parametrize("shape", [TIER1, TIER2_256, TIER2_DEEP], ids=ids)
def test_wta_family(gpu, oracle, shape):
    """On one volume: asw_wta by the scan and (pitches up to 256) by the row sweep, asw_wta_ref
    (the native refinement loop's volume stage), asw_subpixel, and, reading the same memory as
    the local planes of a shard, asw_wta_local, asw_wta_target_local and asw_subpixel_local."""
    import stereo_matchin_amd.kernels as K
    from stereo_matchin_amd import _lib
    torch = _torch()
    W, H, D = shape
    p = params(W, H, D)
    vs = K.cost_shape(p)
    need(vs[0] * vs[1] * vs[2] * 4 + (2 << 30))
    g = gen(gpu, 41)
    L = _lib.lib()
    try:
        C = cost_f32(vs, gpu, g)
        bands = far_bands(vs, 4, LIMITS_F32[shape])
        want = {name: F.wta(C, D, y0, y1) for name, y0, y1 in bands}
        for variant in ((0, 2) if vs[2] <= 256 else (0,)):
            old = L.asw_tune_set(2, variant)
            try:
                got = K.asw_WTA(p, C)
            finally:
                L.asw_tune_set(2, old)
            for name, y0, y1 in bands:
                for i, w in enumerate(want[name]):
                    same(got[i][y0:y1], w, f"asw_wta variant {variant} output {i} {name}")
        d_ref = got[0]
        # sub-pixel map of the winner
        disp = K.subpixel(p, C, d_ref)
        for name, y0, y1 in bands:
            same(disp[y0:y1], F.subpixel(C, d_ref, D, y0, y1), f"asw_subpixel {name}")
        # asw_wta_ref with random estimates
        ref_l = torch.stack([unit(H, W, 0, gpu, g) * float(D), unit(H, W, 0, gpu, g)])
        ref_r = torch.stack([unit(H, W, 0, gpu, g) * float(D), unit(H, W, 0, gpu, g)])
        conf = torch.empty((H, W), dtype=torch.float32, device=gpu)
        dr, dt, _, _ = K.asw_WTA_REF(p, C, ref_l, ref_r, conf)
        for name, y0, y1 in bands:
            w = F.wta_ref(C, ref_l, ref_r, D, y0, y1)
            for i, (gt, wt) in enumerate(zip((dr, dt, conf), w)):
                same(gt[y0:y1], wt, f"asw_wta_ref output {i} {name}")
        # the same memory as the local planes [b, e) of a shard of a deeper range
        b = 100
        e, D2 = b + D, D + 150
        ps = params(W, H, D2, d_begin=b, d_end=e)
        assert K.cost_shape(ps) == vs
        key, m1, m2 = K.wta_local(ps, C)
        tkey, t1, t2 = K.wta_target_local(ps, C, key)
        nb = K.subpixel_local(ps, C, key)
        for name, y0, y1 in bands:
            for i, (gt, wt) in enumerate(zip((key, m1, m2), F.wta_local(C, b, e, D2, y0, y1))):
                same(gt[y0:y1], wt, f"asw_wta_local output {i} {name}")
            for i, (gt, wt) in enumerate(zip((tkey, t1, t2), F.wta_target_local(C, key, b, e, D2, y0, y1))):
                same(gt[y0:y1], wt, f"asw_wta_target_local output {i} {name}")
            same(nb[:, y0:y1], F.subpixel_local(C, key, b, e, D2, y0, y1), f"asw_subpixel_local {name}")
        # the penalised forms of the two scans (asw_wta_ref_local / _target_local) on the same shard
        rkey, rm1, rm2 = K.wta_ref_local(ps, C, ref_l)
        rtkey, rt1, rt2 = K.wta_ref_target_local(ps, C, ref_r, rkey)
        rfin = K.wta_ref_finalize(ps, rkey, rtkey, rt2)
        for name, y0, y1 in bands:
            for i, (gt, wt) in enumerate(zip((rkey, rm1, rm2), F.wta_ref_local(C, ref_l, b, e, D2, y0, y1))):
                same(gt[y0:y1], wt, f"asw_wta_ref_local output {i} {name}")
            w = F.wta_ref_target_local(C, ref_r, rkey, b, e, D2, y0, y1)
            for i, (gt, wt) in enumerate(zip((rtkey, rt1, rt2), w)):
                same(gt[y0:y1], wt, f"asw_wta_ref_target_local output {i} {name}")
            for i, wt in enumerate(F.wta_ref_finalize(rkey, rtkey, rt2, D2, y0, y1)):
                same(rfin[i][y0:y1], wt, f"asw_wta_ref_finalize output {i} {name}")
        # the map-only halves of the protocol, on the far shard's maps (one shard: its own keys)
        contrib = K.wta_second(ps, key, key, m1, m2)
        fin = K.wta_finalize(ps, key, m2, tkey, t2)
        sub = K.subpixel_finalize(ps, key, nb)
        for name, y0, y1 in bands:
            same(contrib[y0:y1], F.wta_second(key, key, m1, m2, y0, y1), f"asw_wta_second {name}")
            for i, wt in enumerate(F.wta_finalize(key, m2, tkey, t2, D2, y0, y1)):
                same(fin[i][y0:y1], wt, f"asw_wta_finalize output {i} {name}")
            same(sub[y0:y1], F.subpixel_finalize(key, nb, D2, y0, y1), f"asw_subpixel_finalize {name}")
    finally:
        C = got = disp = ref_l = ref_r = None
        release()


@pytest.mark.parametrize("shape", [TIER1, TIER2_DEEP], ids=ids)
def test_native_refinement_loop(gpu, oracle, shape):
    """asw_refine_native (2 iterations, 5 taps) on a far volume: its map stages cannot reach a
    limit themselves, its volume scan does.  Every map it returns or updates, on the bands."""
    import stereo_matchin_amd.kernels as K
    from stereo_matchin_amd import _lib
    torch = _torch()
    W, H, D = shape
    iters, taps = 2, 5
    p = params(W, H, D, lr_mode=_lib.LR_NATIVE)
    rp = _lib.default_refine_params(iters=iters, taps=taps)
    vs = K.cost_shape(p)
    need(vs[0] * vs[1] * vs[2] * 4 + (2 << 30))
    g = gen(gpu, 47)
    try:
        C = cost_f32(vs, gpu, g)
        L, R = image(H, W, gpu, g), image(H, W, gpu, g)
        est = torch.randint(0, D, (H, W), generator=g, device=gpu, dtype=torch.int32)
        d_tar = (est + torch.randint(-2, 3, (H, W), generator=g, device=gpu, dtype=torch.int32)).clamp_(0, D - 1)
        conf_ref, conf_tar = unit(H, W, 0, gpu, g), unit(H, W, 0, gpu, g)
        bands = far_bands(vs, 4, LIMITS_F32[shape])
        want = {name: F.refine_native(L, R, D, C, est, d_tar, conf_ref, conf_tar, iters, taps, y0, y1)
                for name, y0, y1 in bands}  # (before the call: the loop updates its inputs in place)
        res = K.refine_native(p, rp, L, R, C, est, d_tar, conf_ref, conf_tar)
        for name, y0, y1 in bands:
            w = want[name]
            same(res["d_ref"][y0:y1], w["ref_d_ref"], f"d_ref {name}")
            same(res["d_tar"][y0:y1], w["ref_d_tar"], f"d_tar {name}")
            same(res["est_left"][y0:y1], w["est_left"], f"est_left {name}")
            same(F.host(res["post16"][y0:y1]).view(np.uint16), w["post16"], f"post16 {name}")
            same(F.host(res["final16"][y0:y1]).view(np.uint16), w["final16"], f"final16 {name}")
            same(conf_ref[y0:y1], w["ref_conf_ref"], f"conf_ref {name}")
            same(conf_tar[y0:y1], w["ref_conf_tar"], f"conf_tar {name}")
    finally:
        C = L = R = res = None
        release()


def test_wta_target_scan_rejects_rows_past_2_gib(gpu):
    """The target scan's 32-bit offsets reach one row plus 64 pixels: the boundary shape is
    rejected by every entry point that runs it, and no kernel is launched (the pointers are
    one small buffer)."""
    from stereo_matchin_amd import _lib
    torch = _torch()
    L = _lib.lib()
    buf = torch.zeros(1024, dtype=torch.uint8, device=gpu)
    q = ctypes.c_void_p(buf.data_ptr())
    Dp = 256
    w_bad = (1 << 31) // (Dp * 4) - 64  # (W + 64) * Dp * 4 == 2^31
    p = params(w_bad, 4, 250)
    assert _lib.params_check(p) == _lib.ASW_OK and _lib.disp_pitch(p) == Dp
    P, status = ctypes.byref(p), _lib.ASW_E_UNSUPPORTED
    assert L.asw_wta(P, q, q, q, q, q, q, q, None) == status
    assert L.asw_wta_ref(P, q, q, q, q, q, q, q, q, None) == status
    assert L.asw_wta_target_local(P, q, q, q, q, q, None) == status
    assert L.asw_wta_ref_target_local(P, q, q, q, q, q, q, None) == status
    torch.cuda.synchronize()
    assert int(buf.sum()) == 0


def test_support_rejects_rows_past_int_max(gpu):
    """The support kernels index a row's W * Tp floats, rounded up to blocks of 256, in 32
    bits: the first width at which W * 68 + 255 passes 2^31 - 1 is rejected by the three entry
    points, no kernel launched (one column less is the largest accepted row: 8.6 GB of weights,
    not launched here)."""
    from stereo_matchin_amd import _lib
    torch = _torch()
    L = _lib.lib()
    buf = torch.zeros(1024, dtype=torch.uint8, device=gpu)
    q, q2 = ctypes.c_void_p(buf.data_ptr()), ctypes.c_void_p(buf.data_ptr() + 512)
    w_bad = ((1 << 31) - 1 - 255) // 68 + 1
    assert (w_bad - 1) * 68 + 255 <= (1 << 31) - 1 < w_bad * 68 + 255 and w_bad <= 1 << 25
    p = params(w_bad, 1, 16, T=65)
    assert _lib.params_check(p) == _lib.ASW_OK and _lib.tap_pitch(p) == 68
    P = ctypes.byref(p)
    assert L.asw_support(P, 0, q, q, q2, None) == _lib.ASW_E_UNSUPPORTED
    assert L.asw_support_all(P, q, q, q, q2, q2, q2, q2, None) == _lib.ASW_E_UNSUPPORTED
    p.color_space = _lib.COLOR_LAB
    assert L.asw_support_lab(P, 1, q, q2, None) == _lib.ASW_E_UNSUPPORTED
    torch.cuda.synchronize()
    assert int(buf.sum()) == 0


# ------------------------------------------------------------------ cross-based matcher

CROSS_E31 = (1024, 8200, 250)  # 2.15 G elements, 8.6 GB: the most asw_cross_cost / _oii hold is 2^32 - 256
LIMITS_CROSS = {TIER1: ("b31", "b32"), CROSS_E31: ("b31", "b32", "e31")}


@pytest.mark.parametrize("shape", [TIER1, CROSS_E31], ids=ids)
def test_cross_volume_stages(gpu, oracle, shape):
    """asw_cross_cost, both integrals, both oii and asw_cross_init, at tier 1 and past element
    2^31 (where a 32-bit linear id of the (pixel, plane) decoding would wrap; cost and oii
    launch a work-item per element and stop below 2^32 elements).  Each stage's reference
    starts from the device's input of that stage."""
    import stereo_matchin_amd.kernels as K
    from stereo_matchin_amd import _lib
    torch = _torch()
    W, H, D = shape
    p = params(W, H, D)
    cp = _lib.default_cross_params()
    vs = K.cost_shape(p)
    need(2 * vs[0] * vs[1] * vs[2] * 4 + (1 << 30))
    g = gen(gpu, 51)
    DIR_V, DIR_H = 0, 1
    try:
        # blocky images: long and short arms
        def img():
            base = image(H // 8 + 1, W // 8 + 1, gpu, g).repeat_interleave(8, 0).repeat_interleave(8, 1)[:H, :W]
            return ((base.to(torch.int16) + torch.randint(-12, 13, (H, W, 4), generator=g, device=gpu,
                                                          dtype=torch.int16)).clamp_(0, 255)).to(torch.uint8).contiguous()
        ml, mr = K.Median_rgba(p, img()), K.Median_rgba(p, img())
        al, ar = K.Cross(p, cp, ml), K.Cross(p, cp, mr)
        bands = far_bands(vs, 4, LIMITS_CROSS[shape])
        a = torch.full(vs, float("nan"), dtype=torch.float32, device=gpu)
        K.Aggregation(p, ml, mr, a)
        for name, y0, y1 in bands:
            same(a[y0:y1, :, :D], F.cross_cost(ml, mr, D, y0, y1), f"asw_cross_cost {name}")
            padding_is_zero(a, D, y0, y1, f"asw_cross_cost {name} padding planes")
        want = {name: F.cross_integral_h(a, D, y0, y1) for name, y0, y1 in bands}
        K.Integral(p, DIR_H, a)
        for name, y0, y1 in bands:
            same(a[y0:y1, :, :D], want[name], f"Integral_h {name}")
        t = torch.full(vs, float("nan"), dtype=torch.float32, device=gpu)
        K.Oii_cross(p, DIR_H, al, ar, a, t)
        for name, y0, y1 in bands:
            same(t[y0:y1, :, :D], F.cross_oii(a, al, ar, D, "h", cp.arm_max, y0, y1), f"Oii_hcross {name}")
            padding_is_zero(t, D, y0, y1, f"Oii_hcross {name} padding planes")
        # the V integral recurs down the columns: a pair of columns, every row (the far rows
        # of those columns are the test)
        cols = ((0, 2), (W // 2, W // 2 + 2), (W - 2, W))
        want = [F.cross_integral_v(t, D, x0, x1) for x0, x1 in cols]
        K.Integral(p, DIR_V, t)
        for (x0, x1), w in zip(cols, want):
            same(t[:, x0:x1, :D], w, f"Integral_v columns {x0}..{x1}")
        a.fill_(float("nan"))
        K.Oii_cross(p, DIR_V, al, ar, t, a)
        for name, y0, y1 in bands:
            same(a[y0:y1, :, :D], F.cross_oii(t, al, ar, D, "v", cp.arm_max, y0, y1), f"Oii_vcross {name}")
        d0, code0 = K.Init_disparity(p, a)
        for name, y0, y1 in bands:
            w = F.cross_init(a, D, y0, y1)
            same(d0[y0:y1], w[0], f"Init_disparity d0 {name}")
            same(code0[y0:y1], w[1], f"Init_disparity code0 {name}")
    finally:
        a = t = ml = mr = al = ar = None
        release()


def test_cross_integrals_and_init_past_2_32_elements(gpu, oracle):
    """Integral_h, Integral_v and Init_disparity launch a wave per 64 planes of a line or per
    pixel, so they hold volumes past 2^32 elements: a random 17 GB volume, all four limits.
    Row bands for the H integral and init, column pairs over every row for the V integral."""
    import stereo_matchin_amd.kernels as K
    torch = _torch()
    W, H, D = TIER2_256
    p = params(W, H, D)
    vs = K.cost_shape(p)
    need(vs[0] * vs[1] * vs[2] * 4 + (2 << 30))
    g = gen(gpu, 53)
    try:
        v = cost_f32(vs, gpu, g)
        bands = far_bands(vs, 4, LIMITS_F32[TIER2_256])
        d0, code0 = K.Init_disparity(p, v)
        for name, y0, y1 in bands:
            w = F.cross_init(v, D, y0, y1)
            same(d0[y0:y1], w[0], f"Init_disparity d0 {name}")
            same(code0[y0:y1], w[1], f"Init_disparity code0 {name}")
        want = {name: F.cross_integral_h(v, D, y0, y1) for name, y0, y1 in bands}
        pad = {name: F.host(v[y0:y1, :, D:]) for name, y0, y1 in bands}
        K.Integral(p, 1, v)
        for name, y0, y1 in bands:
            same(v[y0:y1, :, :D], want[name], f"Integral_h {name}")
            same(v[y0:y1, :, D:], pad[name], f"Integral_h {name}: padding planes are not written")
        cols = ((0, 2), (W // 2, W // 2 + 2), (W - 2, W))
        want = [F.cross_integral_v(v, D, x0, x1) for x0, x1 in cols]
        K.Integral(p, 0, v)
        for (x0, x1), w in zip(cols, want):
            same(v[:, x0:x1, :D], w, f"Integral_v columns {x0}..{x1}")
    finally:
        v = None
        release()


def test_sgm_rejects_what_a_launch_cannot_hold(gpu):
    """A walker is one block, of 1024 threads at 4096 planes: 2^22 rows of them are 2^32
    work-items, one more than a launch holds.  ASW_E_UNSUPPORTED, no kernel launched."""
    from stereo_matchin_amd import _lib
    torch = _torch()
    L = _lib.lib()
    buf = torch.zeros(1024, dtype=torch.uint8, device=gpu)
    q, q2 = ctypes.c_void_p(buf.data_ptr()), ctypes.c_void_p(buf.data_ptr() + 512)
    p = params(1, 1 << 22, 4096)
    sp = _lib.default_sgm_params()
    assert L.asw_sgm_params_check(ctypes.byref(p), ctypes.byref(sp)) == _lib.ASW_OK and _lib.disp_pitch(p) == 4096
    for k in range(8):
        assert L.asw_sgm_path(ctypes.byref(p), ctypes.byref(sp), k, q, q2, 0, None) == _lib.ASW_E_UNSUPPORTED
    assert L.asw_sgm(ctypes.byref(p), ctypes.byref(sp), q, q2, None, None) == _lib.ASW_E_UNSUPPORTED
    torch.cuda.synchronize()
    assert int(buf.sum()) == 0


def test_cross_rejects_what_a_launch_cannot_hold(gpu):
    """One work-item per element: 4096 x 4096 x 256 = 2^32 elements is the first shape past
    the 2^32 - 1 work-items of a launch.  ASW_E_UNSUPPORTED, no kernel launched."""
    from stereo_matchin_amd import _lib
    torch = _torch()
    L = _lib.lib()
    buf = torch.zeros(1024, dtype=torch.uint8, device=gpu)
    q, q2 = ctypes.c_void_p(buf.data_ptr()), ctypes.c_void_p(buf.data_ptr() + 512)
    p = params(4096, 4096, 256)
    assert _lib.params_check(p) == _lib.ASW_OK
    P = ctypes.byref(p)
    assert L.asw_cross_cost(P, q, q, q, None) == _lib.ASW_E_UNSUPPORTED
    assert L.asw_cross_oii(P, 0, q, q, q, q2, None) == _lib.ASW_E_UNSUPPORTED
    assert L.asw_cross_oii(P, 1, q, q, q, q2, None) == _lib.ASW_E_UNSUPPORTED
    # the integral launches a wave per 64 planes of a line: 2^25 columns of 256 planes
    p = params(1 << 25, 1, 256)
    assert _lib.params_check(p) == _lib.ASW_OK
    assert L.asw_cross_integral(ctypes.byref(p), 0, q, None) == _lib.ASW_E_UNSUPPORTED
    torch.cuda.synchronize()
    assert int(buf.sum()) == 0


# ------------------------------------------------------------------ semi-global matching

@pytest.mark.parametrize("shape", [(256, 16400, 250), (256, 13200, 300), (256, 65600, 250)], ids=ids)
def test_sgm_paths(gpu, shape):
    """asw_sgm_path for all eight k with accumulate 0 and 1, then asw_sgm.  Row bands with every
    column for the horizontal and diagonal paths (a diagonal cone is 255 rows), a column pair
    over every row for the vertical ones.  D 300 (Dp 320) is the several-wave form."""
    import stereo_matchin_amd.kernels as K
    from stereo_matchin_amd import _lib
    torch = _torch()
    W, H, D = shape
    p = params(W, H, D)
    sp = _lib.default_sgm_params()
    vs = K.cost_shape(p)
    n = vs[0] * vs[1] * vs[2]
    need(n * 6 + (1 << 30))
    tier2 = n > 1 << 32
    g = gen(gpu, 61)
    try:
        C = cost_u16(vs, gpu, g)
        S = torch.full(vs, float("nan"), dtype=torch.float32, device=gpu)
        bands = far_bands(vs, 4, ("b31", "b32", "e31", "e32") if tier2 else ("b31", "b32"))
        bands16 = far_bands(vs, 2, ("b31", "b32", "e31", "e32") if tier2 else ("b31",))
        rows = sorted({b[1:] for b in bands} | {b[1:] for b in bands16})
        cols = (W - 2, W)
        total = {r: 0 for r in rows}
        for k in range(8):
            vertical = sgm_vertical(k)
            K.sgm_path(p, sp, k, C, S)
            if vertical:
                want_cols = F.sgm_path(C, k, sp.p1, sp.p2, D, (0, H), cols).astype(np.float32)
                same(S[:, cols[0]:cols[1], :D], want_cols, f"path {k} columns")
            want = {}
            for y0, y1 in rows:
                if vertical:
                    want[y0, y1] = want_cols[y0:y1]
                    total[y0, y1] = total[y0, y1] + want[y0, y1]
                    continue
                full = F.sgm_path(C, k, sp.p1, sp.p2, D, (y0, y1), (0, W)).astype(np.float32)
                same(S[y0:y1, :, :D], full, f"path {k} rows {y0}..{y1}")
                padding_is_zero(S, D, y0, y1, f"path {k} rows {y0} padding planes")
                want[y0, y1] = full[:, cols[0]:cols[1]]
                total[y0, y1] = total[y0, y1] + want[y0, y1]
            K.sgm_path(p, sp, k, C, S, accumulate=True)  # S <- L + L
            for y0, y1 in rows:
                same(S[y0:y1, cols[0]:cols[1], :D], want[y0, y1] * np.float32(2.0), f"path {k} accumulate rows {y0}")
        S.fill_(float("nan"))
        K.sgm(p, sp, C, S)
        for y0, y1 in rows:
            assert float(total[y0, y1].max()) < 1 << 24
            same(S[y0:y1, cols[0]:cols[1], :D], total[y0, y1], f"asw_sgm rows {y0}..{y1}")
            padding_is_zero(S, D, y0, y1, f"asw_sgm rows {y0} padding planes")
    finally:
        C = S = None
        release()


def sgm_vertical(k):
    return k in (2, 3)
