"""Every stage kernel in guard-banded, poisoned buffers (tests/guarded.py) — run on an MI355X.

The value tests compare results; these cases check memory.  Every input lies in a guarded
buffer whose padding planes and guards hold what the consumer must not let through (NaN
for arithmetic, -inf for a minimum, 0xFFFF for uint16 volumes), every output in a guarded
buffer poisoned with 0xFF and then with 0x5A.  A case passes when no guard byte changed,
every valid element (and every specified padding element) is byte-identical under both
poisons, and the valid region equals the CPU reference of the stage.  Every case is a
valid call on a valid shape: the smallest shapes that reach each kernel's edges.

Padding that include/asw.h leaves unspecified (the pass outputs' planes >= d_end - d_begin)
is not compared.  A finding is kept as a comment next to its case; when this module was
written every case passed on the first run, so there is none.
"""
import ctypes

import numpy as np
import pytest

import guarded as G
from conftest import pixel_major, plane_major

pytestmark = pytest.mark.gpu

F = np.float32


def _np(t):
    return t.detach().cpu().numpy()


def _params(W, H, D, T=5, iters=1, **kw):
    from stereo_matchin_amd import make_params
    return make_params(W, H, ndisp=D, taps=T, iters=iters, **kw)


def _pair(seed, H, W, shift=4):
    """A shifted, perturbed random pair with random alpha bytes (never read)."""
    rng = np.random.default_rng(seed)
    L = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
    R = np.roll(L, -min(shift, W - 1), axis=1).copy()
    R[..., :3] = np.clip(R[..., :3].astype(int) + rng.integers(-9, 10, (H, W, 3)), 0, 255).astype(np.uint8)
    return np.ascontiguousarray(L), np.ascontiguousarray(R)


def _twice(gpu, stage, specs=None):
    """stage(arena) under both poisons, the library's own allocations guarded too."""

    def run(arena):
        with G.patched(arena):
            return stage(arena)

    return G.run_twice(run, specs, device=gpu)


def _put_cost(arena, name, c_dhw, Dp, fill=G.NAN):
    """A plane-major [n][H][W] volume as the device [H][W][Dp] one, padding planes = fill."""
    n = c_dhw.shape[0]
    a = pixel_major(c_dhw, Dp)
    if fill == G.U16_MAX:
        a = a.astype(np.uint16).view(np.int16)
    return arena.put(name, a, fill=fill, valid=np.s_[:, :, :n])


def _put_support(arena, name, s_thw, Tp):
    """oracle.support's [T][H][W] as [H][W][Tp]: the padding taps stay the specified zero,
    the guards are NaN (the passes multiply by the weights)."""
    T, H, W = s_thw.shape
    a = np.zeros((H, W, Tp), F)
    a[:, :, :T] = np.transpose(s_thw, (1, 2, 0))
    return arena.put(name, a, fill=G.NAN)


def _bits_equal(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    u = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    ne = got.view(u) != want.view(u)
    if got.dtype.kind == "f":  # the references do not pin a NaN's payload
        ne &= ~(np.isnan(got) & np.isnan(want))
    bad = np.argwhere(ne)
    assert bad.size == 0, (what, len(bad), bad[:5].tolist())


def _planes(n, pad=G.UNSPECIFIED, finite=True):
    return G.Out(valid=np.s_[:, :, :n], pad=pad, finite=finite)


# ------------------------------------------------------------------ the harness on the device

def _defects():
    from test_guarded import DEFECTS
    return DEFECTS


@pytest.mark.parametrize("defect,report", [(None, None)] + _defects(),
                         ids=["correct"] + [d.replace(" ", "-") for d, _ in _defects()])
def test_harness_on_device(gpu, defect, report):
    """test_guarded's fake stage (torch operations, no kernel of the library) on device
    tensors: the planted defects are reported there as on the CPU; every planted write
    lands in a guard the arena owns."""
    from test_guarded import SPEC, _stage
    if defect is None:
        G.run_twice(_stage(), SPEC, device=gpu)
        return
    with pytest.raises(G.GuardError) as e:
        G.run_twice(_stage(defect), SPEC, device=gpu)
    assert report in str(e.value), str(e.value)


# ------------------------------------------------------------------ passes

# (H, W, D, d0, d1, pass variant): smaller than every block in both axes with 55 padding
# planes; W ragged for the 12-, 16- and 40-column blocks; a shard with d_begin > 0; pitch 32
# (k_vpass32 / k_hpass32) in both nt policies (variant bit 26); tall, the unclamped chunks
PASS_CASES = [(3, 5, 9, 0, 9, 0), (37, 91, 70, 0, 70, 0), (23, 150, 200, 70, 135, 0), (9, 331, 256, 224, 256, 0),
              (9, 331, 256, 224, 256, 1 << 26), (150, 70, 64, 0, 64, 0)]
# k_hpass11 (variant 4096): NKW = 4 with a ragged last segment, NKW = 1
H11_CASES = [(4, 290, 300, 40, 296, 4096), (3, 150, 64, 0, 50, 4096)]
_pass_refs = {}


def _pass_ref(oracle, T, direction, H, W, D, d0, d1):
    """(sl, sr, cin, want): one oracle pass per case, computed once and read only."""
    key = (T, direction, H, W, D, d0, d1)
    if key not in _pass_refs:
        Lh, Rh = _pair(T * 7 + direction + W, H, W, shift=6)
        sl, sr = oracle.support(Lh, T, direction), oracle.support(Rh, T, direction)
        rng = np.random.default_rng(T + D + H)
        cin = np.floor(rng.random((d1 - d0, H, W)) * 766).astype(F)  # integers <= 765: a uint16 form exists
        want = oracle.aggregate_pass(sl, sr, cin, T, direction, d0=d0, d1=d1, plane_base=d0)
        for a in (sl, sr, cin, want):
            a.setflags(write=False)
        _pass_refs[key] = sl, sr, cin, want
    return _pass_refs[key]


@pytest.mark.parametrize("T", [5, 11, 35, 51])  # 11: k_pass_any
@pytest.mark.parametrize("direction,H,W,D,d0,d1,variant",
                         [(d,) + c for c in PASS_CASES for d in (0, 1)] + [(1,) + c for c in H11_CASES])
def test_pass(gpu, oracle, tune_variant, T, direction, H, W, D, d0, d1, variant):
    """asw_aggregate_pass_den: DEN_NONE, then DEN_WRITE and DEN_READ on one den buffer.
    cin's padding planes are NaN; the last row and column of cout and den end at a guard."""
    import torch

    import stereo_matchin_amd.kernels as K
    from stereo_matchin_amd import _lib
    p = _params(W, H, D, T, d_begin=d0, d_end=d1)
    _, _, Dp = K.cost_shape(p)
    Tp = K.support_shape(p)[2]
    n = d1 - d0
    sl, sr, cin, want = _pass_ref(oracle, T, direction, H, W, D, d0, d1)
    g = K.asw_vCostAggregation if direction == 0 else K.asw_hCostAggregation
    if variant:
        tune_variant(variant)

    def stage(arena):
        wl, wr = _put_support(arena, "wl", sl, Tp), _put_support(arena, "wr", sr, Tp)
        c = _put_cost(arena, "cin", cin, Dp)
        den = arena.out("den", (H, W, Dp), torch.float32)  # 0xFF: NaN
        return {"cout_none": g(p, wl, wr, c),
                "cout_write": g(p, wl, wr, c, den=den, den_mode=_lib.DEN_WRITE),
                "cout_read": g(p, wl, wr, c, den=den, den_mode=_lib.DEN_READ), "den": den}

    for res in _twice(gpu, stage, {k: _planes(n) for k in ("cout_none", "cout_write", "cout_read", "den")}):
        for k in ("cout_none", "cout_write", "cout_read"):
            _bits_equal(plane_major(_np(res[k]), n), want, (k, K.pass_kernel(direction, 0)))
    if Dp == 32 and T != 11:
        name = K.pass_kernel(direction, _lib.DEN_NONE)
        assert name.startswith("k_vpass32<" if direction == 0 else "k_hpass32<"), name
    if variant == 4096 and T != 11:
        assert K.pass_kernel(1, _lib.DEN_NONE).startswith(f"k_hpass11<T={T},"), K.pass_kernel(1, 0)
    if T == 11:
        assert K.pass_kernel(direction, _lib.DEN_NONE).startswith("k_pass_any<"), K.pass_kernel(direction, 0)


@pytest.mark.parametrize("T", [5, 35, 51])
@pytest.mark.parametrize("H,W,D,d0,d1", [c[:5] for c in (PASS_CASES[0], PASS_CASES[1], PASS_CASES[3])])
def test_pass16(gpu, oracle, T, H, W, D, d0, d1):
    """asw_aggregate_pass_den16 (NONE, WRITE) over a uint16 volume with 0xFFFF padding planes
    and guards, against the float pass (and the oracle) on the same costs."""
    import torch

    import stereo_matchin_amd.kernels as K
    from stereo_matchin_amd import _lib
    p = _params(W, H, D, T, d_begin=d0, d_end=d1)
    assert K.raw16_supported(p)
    _, _, Dp = K.cost_shape(p)
    Tp = K.support_shape(p)[2]
    n = d1 - d0
    sl, sr, cin, want = _pass_ref(oracle, T, 0, H, W, D, d0, d1)

    def stage(arena):
        wl, wr = _put_support(arena, "wl", sl, Tp), _put_support(arena, "wr", sr, Tp)
        c16 = _put_cost(arena, "cin16", cin, Dp, fill=G.U16_MAX)
        c32 = _put_cost(arena, "cin", cin, Dp)
        den = arena.out("den", (H, W, Dp), torch.float32)
        den32 = arena.out("den32", (H, W, Dp), torch.float32)
        return {"float": K.asw_vCostAggregation(p, wl, wr, c32, den=den32, den_mode=_lib.DEN_WRITE),
                "cout_none": K.asw_vCostAggregation16(p, wl, wr, c16),
                "cout_write": K.asw_vCostAggregation16(p, wl, wr, c16, den=den, den_mode=_lib.DEN_WRITE),
                "den": den, "den32": den32}

    names = ("cout_none", "cout_write", "den", "den32", "float")
    for res in _twice(gpu, stage, {k: _planes(n) for k in names}):
        for k in ("cout_none", "cout_write"):
            _bits_equal(plane_major(_np(res[k]), n), want, k)
            _bits_equal(_np(res[k])[:, :, :n], _np(res["float"])[:, :, :n], k + " against the float pass")
        _bits_equal(_np(res["den"])[:, :, :n], _np(res["den32"])[:, :, :n], "den")
    kern = "k_vpass32_c16<" if Dp == 32 else "k_vpass10_c16<"
    for mode in (_lib.DEN_NONE, _lib.DEN_WRITE):
        assert K.pass_kernel(0, mode).startswith(kern + f"T={T},"), K.pass_kernel(0, mode)


# ------------------------------------------------------------------ raw cost

@pytest.mark.parametrize("W,H,D,d0,d1,tau", [(5, 3, 9, 0, 9, 765.0), (97, 13, 70, 0, 70, 765.0),
                                             (150, 9, 200, 64, 160, 90.0), (131, 41, 256, 96, 128, 765.0),
                                             (70, 4, 512, 0, 512, 40.5)])
def test_raw_cost(gpu, oracle, W, H, D, d0, d1, tau):
    """asw_raw_cost and asw_raw_cost16 (none at the non-integral tau): padding planes are
    specified zero; the uint16 volume is half the float volume's bytes, its guard right
    behind it."""
    import stereo_matchin_amd.kernels as K
    Lh, Rh = _pair(W + H + D, H, W, shift=5)
    p = _params(W, H, D, d_begin=d0, d_end=d1, tad_tau=tau)
    n = d1 - d0
    want = np.minimum(oracle.raw_cost(Lh, Rh, D)[d0:d1], F(tau))
    has16 = K.raw16_supported(p)
    assert has16 == (tau == int(tau))

    def stage(arena):
        L, R = arena.put("left", Lh), arena.put("right", Rh)
        out = {"cost": K.asw_Aggr(p, L, R)}
        if has16:
            out["cost16"] = K.asw_Aggr16(p, L, R)
            assert arena.find(out["cost16"]).nbytes * 2 == arena.find(out["cost"]).nbytes
        return out

    for res in _twice(gpu, stage, {"cost": _planes(n, pad=0), "cost16": _planes(n, pad=0, finite=False)}):
        _bits_equal(plane_major(_np(res["cost"]), n), want, "asw_raw_cost")
        if has16:
            _bits_equal(plane_major(_np(res["cost16"]).view(np.uint16), n), want.astype(np.uint16), "asw_raw_cost16")


# ------------------------------------------------------------------ census

@pytest.mark.parametrize("H,W", [(3, 5), (9, 70), (5, 257)])
@pytest.mark.parametrize("win", [(9, 7), (5, 5)])
def test_census(gpu, H, W, win):
    import census_ref as CR
    import stereo_matchin_amd.kernels as K
    from stereo_matchin_amd import default_census_params
    img = np.random.default_rng(H * 1000 + W).integers(0, 256, (H, W, 4), dtype=np.uint8)
    p, cp = _params(W, H, 8), default_census_params(win_w=win[0], win_h=win[1])
    for res in _twice(gpu, lambda arena: {"census": K.census(p, cp, arena.put("img", img))}):
        _bits_equal(_np(res["census"]).view(np.uint64), CR.census(img, *win), "asw_census")


def _census_cost_shapes():
    from test_gpu_census import COST_SHAPES
    return COST_SHAPES


@pytest.mark.parametrize("W,H,D,d0,d1", _census_cost_shapes())
def test_census_cost(gpu, W, H, D, d0, d1):
    """asw_census_cost / asw_census_cost16 at test_gpu_census.COST_SHAPES: padding planes
    are specified zero."""
    import census_ref as CR
    import stereo_matchin_amd.kernels as K
    from stereo_matchin_amd import default_census_params
    from test_gpu_census import _rand_pair
    Lh, Rh = _rand_pair(W + D + d0, H, W)
    n = d1 - d0
    for tau, (w, h), wa, wc in ((765.0, (9, 7), 1, 8), (90.0, (9, 3), 64, 700)):
        p = _params(W, H, D, d_begin=d0, d_end=d1, tad_tau=tau)
        cp = default_census_params(win_w=w, win_h=h, ad_weight=wa, census_weight=wc)
        assert K.census16_supported(p, cp)
        cl_h, cr_h = CR.census(Lh, w, h).view(np.int64), CR.census(Rh, w, h).view(np.int64)

        def stage(arena):
            L, R = arena.put("left", Lh), arena.put("right", Rh)
            cl, cr = arena.put("cen_left", cl_h), arena.put("cen_right", cr_h)
            return {"cost": K.census_cost(p, cp, L, R, cl, cr), "cost16": K.census_cost16(p, cp, L, R, cl, cr)}

        for res in _twice(gpu, stage, {"cost": _planes(n, pad=0), "cost16": _planes(n, pad=0, finite=False)}):
            _bits_equal(plane_major(_np(res["cost"]), n), CR.cost_f32(Lh, Rh, D, tau, w, h, wa, wc, d0, d1), "f32")
            _bits_equal(plane_major(_np(res["cost16"]).view(np.uint16), n),
                        CR.cost_u16(Lh, Rh, D, tau, w, h, wa, wc, d0, d1), "u16")


# ------------------------------------------------------------------ supports

@pytest.mark.parametrize("T", [1, 5, 35, 51, 71])  # Q = 1, 3, 9, 13 and k_support_any
@pytest.mark.parametrize("H,W", [(45, 67), (3, 5)])
def test_support(gpu, oracle, T, H, W):
    """asw_support in both directions and asw_support_all (four jobs in one launch): the
    padding taps are specified zero."""
    import torch

    import stereo_matchin_amd.kernels as K
    Lh, Rh = _pair(T + H, H, W)
    p = _params(W, H, 16, T)
    shape = K.support_shape(p)
    want_lut = np.array([[oracle.support_weight(s, d) for s in range(766)] for d in range(T // 2 + 1)], F)
    want = {(i, d): np.transpose(oracle.support(img, T, d), (1, 2, 0)) for i, img in enumerate((Lh, Rh)) for d in (0, 1)}

    def stage(arena):
        L, R = arena.put("left", Lh), arena.put("right", Rh)
        lut = K.support_lut(p, gpu)
        out = {"lut": lut, "v": K.asw_vSupport(p, L, lut), "h": K.asw_hSupport(p, L, lut)}
        four = [arena.out(k, shape, torch.float32) for k in ("wvl", "whl", "wvr", "whr")]
        K.support_all(p, L, R, lut, *four)
        out.update(zip(("wvl", "whl", "wvr", "whr"), four))
        return out

    specs = {k: _planes(T, pad=0) for k in ("v", "h", "wvl", "whl", "wvr", "whr")}
    specs["lut"] = G.Out(finite=True)
    for res in _twice(gpu, stage, specs):
        _bits_equal(_np(res["lut"]), want_lut, "asw_support_lut")
        for k, key in (("v", (0, 0)), ("h", (0, 1)), ("wvl", (0, 0)), ("whl", (0, 1)), ("wvr", (1, 0)), ("whr", (1, 1))):
            _bits_equal(_np(res[k])[:, :, :T], want[key], k)


@pytest.mark.parametrize("T", [5, 35])
def test_support_lab(gpu, oracle, T):
    import stereo_matchin_amd.kernels as K
    H, W = 9, 70
    img, _ = _pair(T, H, W)
    p = _params(W, H, 16, T, color_space=1)
    lab_ref = oracle.lab(img)

    def stage(arena):
        lab = K.lab_image(p, arena.put("img", img))
        return {"lab": lab, "v": K.support_lab(p, 0, lab), "h": K.support_lab(p, 1, lab)}

    for res in _twice(gpu, stage, {"lab": G.Out(finite=True), "v": _planes(T, pad=0), "h": _planes(T, pad=0)}):
        _bits_equal(_np(res["lab"]), lab_ref, "asw_lab")
        for k, d in (("v", 0), ("h", 1)):
            _bits_equal(_np(res[k])[:, :, :T], np.transpose(oracle.support_lab(lab_ref, T, d), (1, 2, 0)), k)


# ------------------------------------------------------------------ WTA

_WTA_NAMES = ("d_ref", "conf_ref", "d_tar", "conf_tar", "code_ref", "code_tar")


@pytest.mark.parametrize("variant", [0, 2])  # the lane-per-pixel scan; the row sweep (Dp 64, 128, 256)
@pytest.mark.parametrize("D,H,W", [(61, 5, 67), (128, 4, 70), (256, 13, 129), (300, 3, 200)])
def test_wta(gpu, oracle, variant, D, H, W):
    """asw_wta on the deep-tied well volume; the padding planes and the guards are -inf (a
    minimum ignores NaN).  ASW_TUNE_WTA_VARIANT as test_wta_variants_on_random_volume."""
    import stereo_matchin_amd.kernels as K
    from stereo_matchin_amd import _lib
    from wta_shard_ref import case_seed, well_volume
    C = well_volume(D, H, W, case_seed(D, H, W))
    want = oracle.wta(C) + ((oracle.code_u8(oracle.wta(C)[0], D), oracle.code_u8(oracle.wta(C)[2], D))
                            if D <= 256 else ())
    p = _params(W, H, D, 3)
    Dp = K.cost_shape(p)[2]
    old = _lib.lib().asw_tune_set(2, variant)
    try:
        runs = _twice(gpu, lambda arena: dict(zip(_WTA_NAMES, K.asw_WTA(p, _put_cost(arena, "cost", C, Dp, G.NEG_INF)))))
    finally:
        _lib.lib().asw_tune_set(2, old)
    for res in runs:
        for k, w in zip(_WTA_NAMES, want):
            _bits_equal(_np(res[k]), w, k)


def _shard_case(D, H, W, nshards):
    from stereo_matchin_amd.distributed import shard_range
    from wta_shard_ref import shard_case
    return shard_case(D, H, W, tuple(shard_range(D, r, nshards) for r in range(nshards)))


@pytest.mark.parametrize("D,H,W,nshards", [(61, 5, 67, 3), (300, 3, 200, 8)])  # pitch 32; pitch 64
def test_wta_sharded(gpu, oracle, D, H, W, nshards):
    """asw_wta_local, asw_wta_target_local, asw_wta_second, asw_wta_finalize and the three
    asw_wta_ref_* entries, shard by shard against wta_shard_ref, -inf padding planes."""
    import stereo_matchin_amd.kernels as K
    c = _shard_case(D, H, W, nshards)
    ps = [_params(W, H, D, 3, d_begin=b, d_end=e) for b, e in c.spans]
    assert {K.cost_shape(p)[2] for p in ps} == ({32} if D == 61 else {64})
    kg, m2g, tkg, t2g = (t.numpy() for t in (c.key_g, c.m2_g, c.tkey_g, c.t2_g))
    rkg, rtkg, rt2g = (t.numpy() for t in (c.rkey_g, c.rtkey_g, c.rt2_g))

    def stage(arena):
        out = {}
        key_g, tkey_g = arena.put("key_g", kg), arena.put("tkey_g", tkg)
        rkey_g, rtkey_g = arena.put("rkey_g", rkg), arena.put("rtkey_g", rtkg)
        ref_l, ref_r = arena.put("ref_l", c.ref_l, fill=G.NAN), arena.put("ref_r", c.ref_r, fill=G.NAN)
        for s, (p, (b, e)) in enumerate(zip(ps, c.spans)):
            cost = _put_cost(arena, f"cost{s}", c.C[b:e], K.cost_shape(p)[2], G.NEG_INF)
            loc = K.wta_local(p, cost)
            tar = K.wta_target_local(p, cost, key_g)
            rloc = K.wta_ref_local(p, cost, ref_l)
            rtar = K.wta_ref_target_local(p, cost, ref_r, rkey_g)
            out.update({f"local{s}.{i}": t for i, t in enumerate(loc)})
            out.update({f"target{s}.{i}": t for i, t in enumerate(tar)})
            out.update({f"rlocal{s}.{i}": t for i, t in enumerate(rloc)})
            out.update({f"rtarget{s}.{i}": t for i, t in enumerate(rtar)})
            out[f"second{s}"] = K.wta_second(p, key_g, *loc)
            out[f"tsecond{s}"] = K.wta_second(p, tkey_g, *tar)
            out[f"rtsecond{s}"] = K.wta_second(p, rtkey_g, *rtar)
        fin = K.wta_finalize(ps[0], key_g, arena.put("m2_g", m2g), tkey_g, arena.put("t2_g", t2g))
        rfin = K.wta_ref_finalize(ps[0], rkey_g, rtkey_g, arena.put("rt2_g", rt2g))
        out.update({f"final.{i}": t for i, t in enumerate(fin)})
        out.update({f"rfinal.{i}": t for i, t in enumerate(rfin)})
        return out

    for res in _twice(gpu, stage):
        for s in range(nshards):
            for name, want in (("local", c.local[s]), ("target", c.target[s]), ("rlocal", c.rlocal[s]),
                               ("rtarget", c.rtarget[s])):
                for i in range(3):
                    _bits_equal(_np(res[f"{name}{s}.{i}"]), want[i].numpy(), (name, s, i))
            for name, want in (("second", c.second[s]), ("tsecond", c.tsecond[s]), ("rtsecond", c.rtsecond[s])):
                _bits_equal(_np(res[name + str(s)]), want.numpy(), (name, s))
        for i, w in enumerate(c.final):
            _bits_equal(_np(res[f"final.{i}"]), w, ("asw_wta_finalize", i))
        for i, w in enumerate(c.rfinal):
            _bits_equal(_np(res[f"rfinal.{i}"]), w, ("asw_wta_ref_finalize", i))


# ------------------------------------------------------------------ sub-pixel

def _put_vol(arena, name, vol_hwd, Dp, fill=G.NAN):
    """A pixel-major [H][W][n] volume as [H][W][Dp], padding planes and guards = fill."""
    H, W, n = vol_hwd.shape
    a = np.zeros((H, W, Dp), F)
    a[:, :, :n] = vol_hwd
    return arena.put(name, a, fill=fill, valid=np.s_[:, :, :n])


@pytest.mark.parametrize("H,W,D,nshards", [(4, 70, 16, 1), (2, 64, 65, 1), (2, 64, 65, 3)])
def test_subpixel(gpu, H, W, D, nshards):
    """asw_subpixel, or asw_subpixel_local on every shard and asw_subpixel_finalize, then
    asw_disp_mask in both LR modes (NULL codes with the native one); NaN padding planes."""
    import subpixel_ref as SR
    import stereo_matchin_amd.kernels as K
    from stereo_matchin_amd.distributed import shard_range
    from test_gpu_subpixel import _crafted
    p = _params(W, H, D)
    Dp = K.cost_shape(p)[2]
    cost, d_ref = (t.cpu().numpy() for t in _crafted(gpu, H, W, D, Dp))
    C = cost[:, :, :D]
    want = SR.subpixel_D(cost, d_ref, D)
    rng = np.random.default_rng(D)
    d_tar = np.clip(d_ref + rng.integers(-2, 3, d_ref.shape), 0, D - 1).astype(np.int32)
    code_ref, code_tar = (np.ascontiguousarray(cross_code(d, D)) for d in (d_ref, d_tar))
    key = ((C.min(axis=2).view(np.uint32).astype(np.int64) << 32) | d_ref).astype(np.int64)
    spans = [shard_range(D, r, nshards) for r in range(nshards)]

    def stage(arena):
        dr, dt = arena.put("d_ref", d_ref), arena.put("d_tar", d_tar)
        out = {}
        if nshards == 1:
            out["disp"] = K.subpixel(p, _put_vol(arena, "cost", C, Dp), dr)
        else:
            kg = arena.put("key_g", key)
            nb = None
            for s, (b, e) in enumerate(spans):
                ps = p.copy()
                ps.d_begin, ps.d_end = b, e
                out[f"nb{s}"] = K.subpixel_local(ps, _put_vol(arena, f"cost{s}", C[:, :, b:e], K.cost_shape(ps)[2]), kg)
                nb = out[f"nb{s}"] if nb is None else K.torch.minimum(nb, out[f"nb{s}"])
            out["disp"] = K.subpixel_finalize(p, kg, arena.put("nb", _np(nb), fill=G.NAN))
        disp = arena.put("disp_in", want, fill=G.NAN)
        q = p.copy()
        q.lr_mode = 1
        out["lr_u8"] = K.disp_mask(p, disp, dr, dt, arena.put("code_ref", code_ref), arena.put("code_tar", code_tar))
        out["lr_native"] = K.disp_mask(q, disp, dr, dt)
        return out

    for res in _twice(gpu, stage, {"disp": G.Out(finite=True)}):
        _bits_equal(_np(res["disp"]), want, "disp")
        for s, (b, e) in enumerate(spans if nshards > 1 else ()):
            _bits_equal(_np(res[f"nb{s}"]), SR.local_neighbours(C[:, :, b:e], key, b, e, D), ("nb", s))
        for k, mode in (("lr_u8", 0), ("lr_native", 1)):
            ok = SR.lr_pass(d_ref, d_tar, code_ref, code_tar, D, mode)
            assert not ok.all() and ok.any()
            _bits_equal(_np(res[k]), SR.mask(want, ok), k)


def cross_code(d, D):
    from cross_ref import code_u8
    return code_u8(d, D)


@pytest.mark.parametrize("W", [1, 63, 65, 257])
def test_disp_fill(gpu, W):
    import subpixel_ref as SR
    import stereo_matchin_amd.kernels as K
    from test_gpu_subpixel import _fill_rows
    rows = _fill_rows(W, np.random.default_rng(W))
    img = np.stack(rows)
    p = _params(W, len(rows), 16)
    for res in _twice(gpu, lambda arena: {"filled": K.disp_fill(p, arena.put("disp_lr", img, fill=G.NAN))},
                      {"filled": G.Out(finite=True)}):
        _bits_equal(_np(res["filled"]), SR.fill(img), "asw_disp_fill")


# ------------------------------------------------------------------ consistency

@pytest.mark.parametrize("lr_mode", [0, 1])
@pytest.mark.parametrize("drop", [None, "out_rgba", "out_red_rgba"])
def test_consistency(gpu, oracle, lr_mode, drop):
    """asw_consistency in both modes, each optional output NULL in turn; the confidences
    are updated in place: guarded, not poisoned."""
    import torch

    import stereo_matchin_amd.kernels as K
    from stereo_matchin_amd import _lib
    W, H, D = 67, 9, 61
    rng = np.random.default_rng(5 + lr_mode)
    d_ref = rng.integers(2, D - 2, (H, W)).astype(np.int32)
    d_tar = (d_ref + rng.integers(-2, 3, (H, W))).astype(np.int32)
    k_ref, k_tar = oracle.code_u8(d_ref, D), oracle.code_u8(d_tar, D)
    cr, ct = rng.random((H, W), dtype=F) + 1, rng.random((H, W), dtype=F) + 1
    p = _params(W, H, D, lr_mode=lr_mode)
    if lr_mode == 0:
        o, r, wcr, wct = oracle.consistency(k_ref, k_tar, cr, ct, D)
    else:
        cons = np.abs(d_ref - d_tar) <= 1
        grey = np.stack([k_ref, k_ref, k_ref, np.full_like(k_ref, 255)], -1)
        r = np.where(cons[..., None], grey, np.array([255, 0, 0, 255], np.uint8)).astype(np.uint8)
        o = None  # lr_rgba of the native mode: compared between the poisons only
        wcr, wct = np.where(cons, cr, F(0)), np.where(cons, ct, F(0))

    def stage(arena):
        a = {k: arena.put(k, v) for k, v in (("d_ref", d_ref), ("d_tar", d_tar), ("code_ref", k_ref),
                                             ("code_tar", k_tar), ("conf_ref", cr), ("conf_tar", ct))}
        out = {k: None if k == drop else arena.out(k, (H, W, 4), torch.uint8) for k in ("out_rgba", "out_red_rgba")}
        _lib.check(_lib.lib().asw_consistency(ctypes.byref(p), *(K._ptr(a[k]) for k in (
            "d_ref", "d_tar", "code_ref", "code_tar", "conf_ref", "conf_tar")), K._ptr(out["out_rgba"]),
            K._ptr(out["out_red_rgba"]), K._stream(gpu)), "asw_consistency")
        return dict(out, conf_ref=a["conf_ref"], conf_tar=a["conf_tar"])

    for res in _twice(gpu, stage):
        _bits_equal(_np(res["conf_ref"]), wcr, "conf_ref")
        _bits_equal(_np(res["conf_tar"]), wct, "conf_tar")
        if drop != "out_red_rgba":
            _bits_equal(_np(res["out_red_rgba"]), r, "out_red_rgba")
        if drop != "out_rgba" and o is not None:
            _bits_equal(_np(res["out_rgba"]), o, "out_rgba")


@pytest.mark.parametrize("drop", [None, "conf_ref", "conf_tar", "est_left", "post16"])
def test_consistency_native(gpu, drop):
    import torch

    import refine_native_ref as RN
    import stereo_matchin_amd.kernels as K
    from stereo_matchin_amd import _lib
    W, H, D = 67, 9, 700
    rng = np.random.default_rng(3)
    d_ref = rng.integers(2, D - 2, (H, W)).astype(np.int32)
    d_tar = (d_ref + rng.integers(-2, 3, (H, W))).astype(np.int32)
    cr, ct = rng.random((H, W), dtype=F) + 1, rng.random((H, W), dtype=F) + 1
    est, post, cons = RN.native_est_left(d_ref, d_tar)
    p = _params(W, H, D, lr_mode=1)

    def stage(arena):
        a = {"d_ref": arena.put("d_ref", d_ref), "d_tar": arena.put("d_tar", d_tar),
             "conf_ref": arena.put("conf_ref", cr), "conf_tar": arena.put("conf_tar", ct),
             "est_left": arena.out("est_left", (H, W), torch.int32), "post16": arena.out("post16", (H, W), torch.int16)}
        a[drop] = None
        _lib.check(_lib.lib().asw_consistency_native(ctypes.byref(p), *(K._ptr(a[k]) for k in (
            "d_ref", "d_tar", "conf_ref", "conf_tar", "est_left", "post16")), K._stream(gpu)), "asw_consistency_native")
        return {k: a[k] for k in ("conf_ref", "conf_tar", "est_left", "post16")}

    want = {"conf_ref": np.where(cons, cr, F(0)), "conf_tar": np.where(cons, ct, F(0)), "est_left": est,
            "post16": post.view(np.int16)}
    for res in _twice(gpu, stage):
        for k, w in want.items():
            if k != drop:
                _bits_equal(_np(res[k]), w, k)


# ------------------------------------------------------------------ refinement

def _refine_inputs(W, H, D, seed):
    from test_gpu_refine_native import _stage_inputs
    return _stage_inputs(W, H, D, seed)


@pytest.mark.parametrize("W,H,Tr", [(3, 5, 33), (19, 7, 1), (300, 3, 9)])
def test_ref_v_h(gpu, W, H, Tr):
    """asw_refine_lut / asw_refine_native_lut, asw_ref_v at code strides 1 and 4,
    asw_ref_v_native and asw_ref_h; the estimates entering asw_ref_h lie between NaN guards."""
    import refine_native_ref as RN
    import stereo_matchin_amd.kernels as K
    from stereo_matchin_amd import _lib
    D = 200
    p, rp = _params(W, H, D), _lib.default_refine_params(taps=Tr)
    img, est, conf = _refine_inputs(W, H, D, 7 * W + Tr)
    codes = (est % 256).astype(np.uint8)
    rgba = np.ascontiguousarray(np.stack([codes, 255 - codes, codes // 2, np.full_like(codes, 255)], -1))
    want_v8 = RN.ref_v(img, RN.decode(codes, D, "u8"), conf, Tr)
    want_vn = RN.ref_v(img, est.astype(F), conf, Tr)
    want_h = RN.ref_h(img, conf, want_vn, Tr)

    def stage(arena):
        im, cf = arena.put("img", img), arena.put("conf", conf, fill=G.NAN)
        lut, lutn = K.refine_lut(p, rp, gpu), K.refine_native_lut(p, rp, gpu)
        out = {"lut": lut, "lut_native": lutn,
               "v_stride1": K.asw_ref_v(p, rp, im, arena.put("codes", codes), cf, lut),
               "v_stride4": K.asw_ref_v(p, rp, im, arena.put("rgba", rgba), cf, lut),
               "v_native": K.asw_ref_v_native(p, rp, im, arena.put("est", est), cf, lutn)}
        out["h"] = K.asw_ref_h(p, rp, im, cf, arena.put("est_v", want_vn, fill=G.NAN), lut)
        return out

    for res in _twice(gpu, stage, {k: G.Out(finite=True) for k in ("lut", "lut_native", "v_stride1", "v_stride4",
                                                                  "v_native", "h")}):
        for k, w in (("lut", RN.weight_lut(Tr)), ("lut_native", RN.weight_lut(Tr)), ("v_stride1", want_v8),
                     ("v_stride4", want_v8), ("v_native", want_vn), ("h", want_h)):
            _bits_equal(_np(res[k]), w, k)


@pytest.mark.parametrize("W,H", [(1, 1), (1, 4), (37, 5)])
def test_median(gpu, W, H):
    """asw_median3 at strides 1 and 4 and asw_median3_u16."""
    import refine_native_ref as RN
    import stereo_matchin_amd.kernels as K
    rng = np.random.default_rng(W + H)
    a = rng.integers(0, 65535, (H, W)).astype(np.int32)
    codes = rng.integers(0, 256, (H, W), dtype=np.uint8)
    rgba = np.ascontiguousarray(np.stack([codes, 255 - codes, codes // 2, codes], -1))
    p = _params(W, H, 65535, lr_mode=1)
    med = RN.median3(codes)
    want8 = np.stack([med, med, med, np.full_like(med, 255)], -1)

    def stage(arena):
        return {"stride1": K.Median(p, arena.put("codes", codes)), "stride4": K.Median(p, arena.put("rgba", rgba)),
                "u16": K.Median16(p, arena.put("est", a))}

    for res in _twice(gpu, stage):
        _bits_equal(_np(res["stride1"]), want8, "stride 1")
        _bits_equal(_np(res["stride4"]), want8, "stride 4")
        _bits_equal(_np(res["u16"]).view(np.uint16), RN.median3(a).astype(np.uint16), "u16")


def _pre(oracle, W, H, D, seed):
    """The pre-refinement state of a synthetic pair from the oracle (taps 5, one iteration)."""
    from stereo_matchin_amd.synthetic import make_pair
    Lh, Rh, _ = make_pair(W, H, max(2, W // 3), seed, regions=6)
    Lh, Rh = np.ascontiguousarray(Lh), np.ascontiguousarray(Rh)
    return Lh, Rh, oracle.match(Lh, Rh, D, 5, 1, want_cost=True)


def test_refine_loop(gpu, oracle):
    """asw_refine (70 x 40, D 61, k 2): the workspace is a guarded buffer of exactly
    asw_refine_workspace_bytes (the wrapper's allocation), so the last carve-out of the
    launcher must end inside it.  The in-place buffers are guarded, not poisoned."""
    import stereo_matchin_amd.kernels as K
    from stereo_matchin_amd import _lib
    W, H, D, k = 70, 40, 61, 2
    Lh, Rh, pre = _pre(oracle, W, H, D, 3)
    want = oracle.refine(Lh, Rh, D, pre["cost"], pre, k, 33)
    p, rp = _params(W, H, D), _lib.default_refine_params(iters=k, taps=33)
    nws = int(_lib.lib().asw_refine_workspace_bytes(ctypes.byref(p), ctypes.byref(rp)))
    assert nws > 0

    def stage(arena):
        a = {"est_left_rgba": arena.put("est_left_rgba", pre["lr_rgba"]),
             "code_tar": arena.put("code_tar", oracle.code_u8(pre["d_tar"], D)),
             "conf_ref": arena.put("conf_ref", pre["conf_ref"]), "conf_tar": arena.put("conf_tar", pre["conf_tar"])}
        out = K.refine(p, rp, arena.put("left", Lh), arena.put("right", Rh),
                       _put_cost(arena, "cost", pre["cost"], K.cost_shape(p)[2], G.NEG_INF), *a.values())
        assert any(b.nbytes == nws and b.body.dim() == 1 for b in arena.buffers), "the workspace is guarded"
        return dict(out, **a)

    for res in _twice(gpu, stage):
        for g, w in (("final_rgba", "final_rgba"), ("post_red_rgba", "post_red_rgba"), ("d_ref", "ref_d_ref"),
                     ("d_tar", "ref_d_tar"), ("conf_ref", "ref_conf_ref"), ("conf_tar", "ref_conf_tar")):
            _bits_equal(_np(res[g]), want[w], g)


def test_refine_native_loop(gpu, oracle):
    """asw_refine_native (96 x 24, D 512, k 1) in a workspace of exactly
    asw_refine_native_workspace_bytes."""
    import refine_native_ref as RN
    import stereo_matchin_amd.kernels as K
    from stereo_matchin_amd import _lib
    W, H, D, k = 96, 24, 512, 1
    Lh, Rh, pre = _pre(oracle, W, H, D, 5)
    dr, cr, dt, ct = oracle.wta(pre["cost"])
    el, _, cons = RN.native_est_left(dr, dt)
    cr, ct = np.where(cons, cr, F(0)), np.where(cons, ct, F(0))
    want = RN.refine(Lh, Rh, D, pre["cost"], el, dt, cr, ct, k, 33, "native")
    p, rp = _params(W, H, D, lr_mode=1), _lib.default_refine_params(iters=k, taps=33)
    nws = int(_lib.lib().asw_refine_native_workspace_bytes(ctypes.byref(p), ctypes.byref(rp)))
    assert nws > 0

    def stage(arena):
        a = [arena.put("est_left", el), arena.put("d_tar", dt), arena.put("conf_ref", cr), arena.put("conf_tar", ct)]
        out = K.refine_native(p, rp, arena.put("left", Lh), arena.put("right", Rh),
                              _put_cost(arena, "cost", pre["cost"], K.cost_shape(p)[2], G.NEG_INF), *a)
        assert any(b.nbytes == nws and b.body.dim() == 1 for b in arena.buffers), "the workspace is guarded"
        return dict(out, conf_ref=a[2], conf_tar=a[3])

    for res in _twice(gpu, stage):
        for g, w in (("d_ref", "ref_d_ref"), ("d_tar", "ref_d_tar"), ("conf_ref", "ref_conf_ref"),
                     ("conf_tar", "ref_conf_tar"), ("est_left", "est_left")):
            _bits_equal(_np(res[g]), want[w], g)
        for g in ("post16", "final16"):
            _bits_equal(_np(res[g]).view(np.uint16), want[g], g)


# ------------------------------------------------------------------ cross-based

@pytest.mark.parametrize("W,H,D", [(7, 5, 4), (70, 9, 61), (33, 40, 65), (40, 12, 256)])
def test_cross(gpu, W, H, D):
    """The nine entry points of asw_cross.hip.  The cost and OII outputs' padding planes are
    written zero; the integral runs in place (guarded, NaN padding planes neither read nor
    written); asw_cross_init's volume has -inf padding planes."""
    import stereo_matchin_amd.kernels as K
    from stereo_matchin_amd import _lib
    from test_gpu_cross import _ref
    L, R, ref = _ref(W, H, D, "piecewise")
    p, cp = _lib.default_params(W, H, ndisp=D), _lib.default_cross_params()
    Dp = _lib.disp_pitch(p)

    def stage(arena):
        ml, mr = arena.put("median_l", ref["median_l"]), arena.put("median_r", ref["median_r"])
        al, ar = arena.put("arms_l", ref["arms_l"]), arena.put("arms_r", ref["arms_r"])
        out = {"median_l": K.Median_rgba(p, arena.put("left", L)), "median_r": K.Median_rgba(p, arena.put("right", R)),
               "arms_l": K.Cross(p, cp, ml), "arms_r": K.Cross(p, cp, mr), "cost": K.Aggregation(p, ml, mr)}
        for direction, src, integ, oii in ((_lib.DIR_H, "cost", "integral_h", "oii_h"),
                                           (_lib.DIR_V, "oii_h", "integral_v", "oii_v")):
            out[integ] = K.Integral(p, direction, _put_vol(arena, integ, ref[src], Dp))
            out[oii] = K.Oii_cross(p, direction, al, ar, _put_vol(arena, integ + "_in", ref[integ], Dp))
        out["d_initial"], out["code_initial"] = K.Init_disparity(p, _put_vol(arena, "oii_v_in", ref["oii_v"], Dp,
                                                                             G.NEG_INF))
        out["d_final"], out["code_final"] = K.Disparity(p, arena.put("code0", ref["code_initial"]), al)
        out["final"] = K.Median(p, arena.put("code1", ref["code_final"]))
        return out

    specs = {k: _planes(D, pad=0) for k in ("cost", "oii_h", "oii_v")}
    specs.update({k: _planes(D) for k in ("integral_h", "integral_v")})
    for res in _twice(gpu, stage, specs):
        for k in ("median_l", "median_r", "arms_l", "arms_r", "d_initial", "code_initial", "d_final", "code_final"):
            _bits_equal(_np(res[k]), ref[k], k)
        for k in ("cost", "integral_h", "oii_h", "integral_v", "oii_v"):
            _bits_equal(_np(res[k])[:, :, :D], ref[k], k)
        for k in ("integral_h", "integral_v"):
            assert np.isnan(_np(res[k])[:, :, D:]).all(), k + " padding"
        _bits_equal(_np(res["final"])[..., 0], ref["final"], "final")


# ------------------------------------------------------------------ the tiled V pass, ragged

@pytest.mark.slow
def test_vpass_tiled_ragged(gpu, oracle):
    """k_vpass10<..,TK=4> (XCD-round tiles of 4 plane blocks, launch_dm: T > 35, a volume of
    at least 256 MiB, v12_tiles) where its tiles are partial: Dp = 320 is 5 plane blocks
    (the second tile holds one: kbi >= nkb), 59 column groups are 8 per XCD (the last XCD
    has 3 live ones: cgl >= xg_per_xcd), and the 300 rows are two strips of 168 and 132
    (strip = rest / ntc; the second no whole number of 56-row chunks).  700*300*320*4 B is
    just over 256 MiB: nothing smaller reaches this branch.  NONE, WRITE then READ, and the
    uint16 NONE and WRITE passes against one oracle pass, compared on the GPU."""
    import torch

    import stereo_matchin_amd.kernels as K
    from stereo_matchin_amd import _lib
    from test_gpu_parity import _cost_equal_on_gpu
    W, H, D, T = 700, 300, 300, 51
    p = _params(W, H, D, T)
    Dp = K.cost_shape(p)[2]
    Tp = K.support_shape(p)[2]
    assert Dp == 320 and H * W * Dp * 4 >= 256 << 20
    Lh, Rh = _pair(51, H, W, shift=9)
    sl, sr = oracle.support(Lh, T, 0), oracle.support(Rh, T, 0)
    rng = np.random.default_rng(700)
    cin = rng.integers(0, 766, (D, H, W)).astype(F)
    want = oracle.aggregate_pass(sl, sr, cin, T, 0)
    c32 = np.full((H, W, Dp), np.nan, F)  # the 20 padding planes: NaN
    c32[:, :, :D] = np.transpose(cin, (1, 2, 0))
    c16 = np.full((H, W, Dp), -1, np.int16)  # 0xFFFF
    c16[:, :, :D] = c32[:, :, :D].astype(np.int16)
    del cin
    names = {}

    def stage(arena):
        wl, wr = _put_support(arena, "wl", sl, Tp), _put_support(arena, "wr", sr, Tp)
        c = arena.put("cin", c32, fill=G.NAN)
        h = arena.put("cin16", c16, fill=G.U16_MAX)
        den, den16 = (arena.out(k, (H, W, Dp), torch.float32) for k in ("den", "den16"))
        out = {"den": den, "den16": den16}
        for key, fn, src, kw in (("none", K.asw_vCostAggregation, c, {}),
                                 ("write", K.asw_vCostAggregation, c, dict(den=den, den_mode=_lib.DEN_WRITE)),
                                 ("read", K.asw_vCostAggregation, c, dict(den=den, den_mode=_lib.DEN_READ)),
                                 ("none16", K.asw_vCostAggregation16, h, {}),
                                 ("write16", K.asw_vCostAggregation16, h, dict(den=den16, den_mode=_lib.DEN_WRITE))):
            out[key] = fn(p, wl, wr, src, **kw)
            names[key] = K.pass_kernel(0, kw.get("den_mode", 0))
        return out

    keys = ("none", "write", "read", "none16", "write16")
    for res in _twice(gpu, stage, {k: _planes(D) for k in keys + ("den", "den16")}):
        for k in keys:
            _cost_equal_on_gpu(gpu, res[k], want)
        assert torch.equal(res["den"][:, :, :D], res["den16"][:, :, :D])
    for k, dm in (("none", 0), ("write", 1), ("read", 2)):
        assert names[k] == f"k_vpass10<T=51,NW=12,NPH=3,TK=4,DM={dm},nt>", names
    for k, dm in (("none16", 0), ("write16", 1)):
        assert names[k] == f"k_vpass10_c16<T=51,NW=12,NPH=3,TK=4,DM={dm},nt>", names


# ------------------------------------------------------------------ host outputs of a batch

_HOST_GUARD = 4096


def _host(shape, dtype):
    """A numpy array inside a larger one, 0xA5 guard bytes on both sides, the body 0x5A."""
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    base = np.full(n + 2 * _HOST_GUARD, 0xA5, np.uint8)
    base[_HOST_GUARD:_HOST_GUARD + n] = 0x5A
    return base, base[_HOST_GUARD:_HOST_GUARD + n].view(dtype).reshape(shape)


def _host_guards_intact(arrays):
    for name, (base, body) in arrays.items():
        for side, g in (("front", base[:_HOST_GUARD]), ("back", base[_HOST_GUARD + body.nbytes:])):
            bad = np.flatnonzero(g != 0xA5)
            assert bad.size == 0, f"host guard of '{name}' damaged: {side} guard, first at byte {bad[0]}"


def _match_batch(ctx, p, rp, cp, lefts, rights):
    """asw_match_batch of B pairs with the sub-pixel, native-refinement and cross outputs
    registered: every host array guarded.  The registered arrays hold the B pairs at
    pair * S offsets, so pair B-1's copy ends exactly at the array's end."""
    from stereo_matchin_amd import _lib
    lib = _lib.lib()
    B, H, W = lefts.shape[:3]
    arrays, outs = {}, []
    for b in range(B):
        shapes = {"d_ref": ((H, W), np.int32), "d_tar": ((H, W), np.int32), "conf_ref": ((H, W), F),
                  "conf_tar": ((H, W), F), "disp_rgba": ((H, W, 4), np.uint8), "lr_rgba": ((H, W, 4), np.uint8),
                  "lr_red_rgba": ((H, W, 4), np.uint8), "cost": ((H, W, _lib.disp_pitch(p)), F),
                  "disp16": ((H, W), np.uint16), "lr16": ((H, W), np.uint16)}
        for k, (s, t) in shapes.items():
            arrays[f"{k}[{b}]"] = _host(s, t)
        outs.append(_lib.AswOutputs(*[arrays[f"{k}[{b}]"][1].ctypes.data if k in shapes else None
                                      for k, _ in _lib.AswOutputs._fields_]))
    reg = {"disp_sub": F, "disp_sub_lr": F, "disp_sub_filled": F, "final16": np.uint16, "post16": np.uint16,
           "refine_d_ref": np.int32, "refine_d_tar": np.int32, "cross_d_initial": np.int32}
    for k, t in reg.items():
        arrays[k] = _host((B, H, W), t)
    for k in ("cross_initial_rgba", "cross_final_rgba", "cross_median_rgba"):
        arrays[k] = _host((B, H, W, 4), np.uint8)
    ptr = lambda k: arrays[k][1].ctypes.data  # noqa: E731
    so = _lib.AswSubpixelOutputs(ptr("disp_sub"), ptr("disp_sub_lr"), ptr("disp_sub_filled"))
    no = _lib.AswRefineNativeOutputs(ptr("final16"), ptr("post16"), ptr("refine_d_ref"), ptr("refine_d_tar"))
    co = _lib.AswCrossOutputs(ptr("cross_initial_rgba"), ptr("cross_final_rgba"), ptr("cross_median_rgba"),
                              ptr("cross_d_initial"), None)
    _lib.check(lib.asw_set_subpixel(ctx, ctypes.byref(so)), "asw_set_subpixel")
    _lib.check(lib.asw_set_refine_native(ctx, ctypes.byref(rp), ctypes.byref(no)), "asw_set_refine_native")
    _lib.check(lib.asw_set_cross(ctx, ctypes.byref(cp), ctypes.byref(co)), "asw_set_cross")
    try:
        _lib.check(lib.asw_match_batch(ctx, lefts.ctypes.data, rights.ctypes.data, B,
                                       (_lib.AswOutputs * B)(*outs), None), "asw_match_batch")
    finally:  # this call's arrays leave the context
        lib.asw_set_subpixel(ctx, None)
        lib.asw_set_refine_native(ctx, None, None)
        lib.asw_set_cross(ctx, None, None)
    _host_guards_intact(arrays)
    return {k: body for k, (_, body) in arrays.items()}


def test_batch_host_outputs(gpu, oracle):
    """asw_match_batch, batch = 2 on 70 x 40, D 61: every host output between guard bytes;
    the batch equals the two pairs matched alone, and the oracle's maps."""
    from stereo_matchin_amd import _lib
    W, H, D = 70, 40, 61
    pairs = [_pre(oracle, W, H, D, seed) for seed in (3, 4)]
    lefts = np.ascontiguousarray(np.stack([L for L, _, _ in pairs]))
    rights = np.ascontiguousarray(np.stack([R for _, R, _ in pairs]))
    p = _params(W, H, D)
    rp, cp = _lib.default_refine_params(iters=1, taps=9), _lib.default_cross_params()
    lib = _lib.lib()
    ctx = ctypes.c_void_p()
    _lib.check(lib.asw_create(ctypes.byref(p), 0, ctypes.byref(ctx)), "asw_create")
    try:
        both = _match_batch(ctx, p, rp, cp, lefts, rights)
        single = [_match_batch(ctx, p, rp, cp, lefts[b:b + 1], rights[b:b + 1]) for b in range(2)]
    finally:
        lib.asw_destroy(ctx)
    for b in range(2):
        for k, v in single[b].items():
            got = both[k.replace("[0]", f"[{b}]")] if k.endswith("[0]") else both[k][b]
            _bits_equal(got, v if k.endswith("[0]") else v[0], (k, b))
        for k in ("d_ref", "d_tar", "lr_red_rgba"):
            _bits_equal(both[f"{k}[{b}]"], pairs[b][2][k], (k, b))
        _bits_equal(plane_major(both[f"cost[{b}]"], D), pairs[b][2]["cost"], ("cost", b))
    assert not np.array_equal(both["disp_sub"][0], both["disp_sub"][1])
