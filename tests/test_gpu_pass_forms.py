"""Every compiled form of the 64-lane aggregation passes, at every ring tap count — run on an MI355X.

k_vpass10, k_vpass10_c16, k_hpass9 and k_hpass11 are compiled once per tap count T in
{3, 5, 7, 9, 15, 33, 35, 51} and den mode, in several block shapes and two cache policies
(tests/pass_forms.py lists the names: CATALOGUE).  The window period, the refill batch, the
ring lengths and the phase split are compile-time functions of T, so a form that passes at one
T says little about the next.  CASES below holds the smallest shapes at which each path of each
form exists, at all eight T; tests/test_pass_forms.py proves on the CPU that the names CASES
maps to are exactly the catalogue, and every test here asserts after each launch that the
library ran the form the case stands for.

Every output is compared bit for bit (no tolerance) with the oracle's pass over the whole
volume; the three shapes at the 256 MiB policy threshold are compared on row bands with the crop
reference (tests/far_ref.py) and across den modes over the whole volume.  Variant bit 26 flips the
cache policy, so the nt forms run at shapes the oracle can cover.
"""
from collections import namedtuple

import numpy as np
import pytest

import pass_forms as PF
from conftest import pixel_major
from guarded import guarded_kernels  # noqa: F401  (a fixture, used by name)

# every output the wrappers allocate is guarded and poisoned (tests/guarded.py)
pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("guarded_kernels")]

ALL = (PF.DEN_NONE, PF.DEN_WRITE, PF.DEN_READ)
FIRST = (PF.DEN_NONE, PF.DEN_WRITE)  # the uint16 form is a first pass: there is no den to read yet
FLIP = PF.BIT_NT_FLIP

# shapes are (H, W, D, d_begin, d_end); modes: the den modes run, in this order, on one den buffer
Case = namedtuple("Case", "family T H W D d0 d1 direction c16 variant modes")


def _v_shapes(T):
    # two or more strips with a ragged last chunk and unclamped interior chunks, W ragged for the
    # 16- and 12-column blocks, 58 padding planes; a shard with Dp = 192; smaller than a block
    return [(4 * T + 13, 37, 70, 0, 70), (4 * T + 13, 70, 200, 10, 140), (3, 5, 9, 0, 9)]


# TK = 4 tiles (T = 51, nt): 65 column groups (9 per XCD: 2 tile columns, the second partial) and
# 5 plane blocks (2 tile rows, the second partial); two strips through the tile order
TILE_SHAPES = [(8, 780, 320, 0, 320), (217, 780, 256, 0, 256)]
# k_hpass11: NKW = 4 with three segments and a ragged last; NKW = 4 with d_begin > 0; nkb = 6 (NKW = 2,
# three groups); NKW = 2; nkb = 3 (NKW = 1, three groups); NKW = 1; W below most T (every tap clamps);
# a shard with x - d < 0 everywhere (the right column is always 0: ring_off)
H11_SHAPES = [(7, 530, 256, 0, 256), (4, 290, 300, 40, 296), (3, 300, 384, 0, 384), (5, 410, 128, 0, 128),
              (6, 333, 200, 8, 200), (3, 150, 64, 0, 50), (2, 5, 64, 0, 64), (3, 150, 600, 448, 512)]
# the segment override (2 and 1 window periods per segment: at T = 51 den-read, PX = 24, not a whole
# number of the 80-step periods the kernel sweeps in), NKW = 4 | 2, 2 and 1
H11_SEG_SHAPES = [H11_SHAPES[0], H11_SHAPES[2], H11_SHAPES[4]]
H9_SHAPES = [(9, 331, 256, 0, 256), (6, 47, 128, 0, 128), (5, 161, 300, 40, 168), (2, 5, 64, 0, 64)]


def _cases():
    cs = []
    for T in PF.RING_TAPS:
        for shape in _v_shapes(T):
            cs += [Case("v", T, *shape, PF.DIR_V, False, v, ALL) for v in (0, FLIP)]
        for shape in _v_shapes(T)[:2]:
            cs += [Case("v16", T, *shape, PF.DIR_V, True, v, FIRST) for v in (0, FLIP)]
    cs += [Case("v-tiles", 51, *shape, PF.DIR_V, False, FLIP, ALL) for shape in TILE_SHAPES]
    cs += [Case("v16-tiles", 51, *TILE_SHAPES[0], PF.DIR_V, True, FLIP, FIRST)]
    for T in PF.RING_TAPS:
        cs += [Case("h11", T, *shape, PF.DIR_H, False, PF.BIT_H11, ALL) for shape in H11_SHAPES]
    for T in (7, 51):
        for shape in H11_SEG_SHAPES:
            cs += [Case("h11-seg", T, *shape, PF.DIR_H, False, PF.BIT_H11 + (n << PF.SEG_SHIFT), ALL) for n in (2, 1)]
    for T in PF.RING_TAPS:
        for shape in H9_SHAPES:
            cs += [Case("h9", T, *shape, PF.DIR_H, False, v, ALL) for v in (PF.BIT_H9, PF.BIT_H9 | FLIP)]
    # the default dispatch at its thresholds (no variant): exactly 8192 waves, and one row less
    cs += [Case("waves", 7, H, 8, 64, 0, 64, PF.DIR_H, False, 0, ALL) for H in (8192, 8191)]
    return cs


# the default dispatch at the 256 MiB policy threshold (no variant): exactly 2^28 bytes, one row
# less, and past it with fewer than 8192 H waves (k_hpass9 nt; T = 51: the untiled 12-column nt form)
LARGE_CASES = [Case("large", T, H, W, 256, 0, 256, direction, False, 0, ALL)
               for T, H, W in ((9, 512, 512), (9, 511, 512), (3, 1200, 224), (51, 1200, 224))
               for direction in (PF.DIR_V, PF.DIR_H)]
CASES = _cases() + LARGE_CASES


def case_id(c):
    return f"{c.family}-T{c.T}-{c.H}x{c.W}x{c.D}-{c.d0}_{c.d1}-v{c.variant:#x}" + ("-H" if c.direction else "-V")


def case_names(c):
    """The catalogue names the case must run, one per den mode."""
    return [PF.expected_name(c.W, c.H, c.d0, c.d1, c.D, c.T, c.direction, m, c.c16, c.variant) for m in c.modes]


def _t(a, dev):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.flags.writeable else a.copy()).to(dev)  # (the shared references are read-only)


def _params(c):
    from stereo_matchin_amd import make_params
    return make_params(c.W, c.H, ndisp=c.D, taps=c.T, iters=1, d_begin=c.d0, d_end=c.d1)


def _pair(seed, H, W):
    """A shifted, perturbed random pair (ragged: no size here is a multiple of a block)."""
    rng = np.random.default_rng(seed)
    L = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
    R = np.roll(L, -min(6, W - 1), axis=1).copy()
    R[..., :3] = np.clip(R[..., :3].astype(int) + rng.integers(-9, 10, (H, W, 3)), 0, 255).astype(np.uint8)
    L[..., 3] = R[..., 3] = 255
    return np.ascontiguousarray(L), np.ascontiguousarray(R)


_ref = {}


def _pass_ref(oracle, c):
    """(Lh, Rh, cin, want) of a case: one oracle pass per (T, direction, shape, integer costs),
    computed once, read only, shared by the policies, variants and den modes that follow it in
    CASES (only the latest is kept: the largest holds 43 M voxels)."""
    key = (c.T, c.direction, c.H, c.W, c.D, c.d0, c.d1, c.c16)
    if key not in _ref:
        _ref.clear()
        Lh, Rh = _pair(c.T * 7 + c.direction + c.W, c.H, c.W)
        sl, sr = oracle.support(Lh, c.T, c.direction), oracle.support(Rh, c.T, c.direction)
        rng = np.random.default_rng(c.T + c.D + c.H)
        cin = rng.random((c.d1 - c.d0, c.H, c.W), dtype=np.float32)
        # uint16 form: integers <= 765, the raw costs' range; else floats in [0, 700)
        cin = np.floor(cin * np.float32(766)) if c.c16 else cin * np.float32(700)
        want = oracle.aggregate_pass(sl, sr, cin, c.T, c.direction, d0=c.d0, d1=c.d1, plane_base=c.d0)
        for a in (Lh, Rh, cin, want):
            a.setflags(write=False)
        _ref[key] = Lh, Rh, cin, want
    return _ref[key]


def _same_bits(got_hwd, want_hwd, what):
    """Two device [H][W][n] float volumes, bit for bit."""
    import torch
    ne = got_hwd.view(torch.int32) != want_hwd.view(torch.int32)
    if bool(ne.any()):
        bad = torch.nonzero(ne)
        raise AssertionError(f"{what}: {len(bad)} voxels differ, first (y, x, k) {bad[:5].tolist()}")


def _supports(K, p, c, Lh, Rh, gpu):
    f = K.asw_vSupport if c.direction == PF.DIR_V else K.asw_hSupport
    return f(p, _t(Lh, gpu)), f(p, _t(Rh, gpu))


@pytest.mark.parametrize("c", [c for c in CASES if not c.c16 and c.family != "large"], ids=case_id)
def test_float_pass(gpu, oracle, tune_variant, c):
    """DEN_NONE, DEN_WRITE, then DEN_READ on one den buffer (NaN before): each output equals the
    oracle's pass over the whole volume, each launch ran the form the case names."""
    import torch

    import stereo_matchin_amd.kernels as K
    p = _params(c)
    Dp, n = K.cost_shape(p)[2], c.d1 - c.d0
    assert Dp == PF.pitch(c.d0, c.d1, c.D)
    Lh, Rh, cin, want = _pass_ref(oracle, c)
    wl, wr = _supports(K, p, c, Lh, Rh, gpu)
    cin_d = _t(pixel_major(cin, Dp), gpu)
    want_d = _t(want, gpu).permute(1, 2, 0)
    den = torch.full(K.cost_shape(p), float("nan"), dtype=torch.float32, device=gpu)
    g = K.asw_vCostAggregation if c.direction == PF.DIR_V else K.asw_hCostAggregation
    tune_variant(c.variant)
    for mode, name in zip(c.modes, case_names(c)):
        out = g(p, wl, wr, cin_d, den=den if mode else None, den_mode=mode)
        assert K.pass_kernel(c.direction, mode) == name
        _same_bits(out[:, :, :n], want_d, name)


@pytest.mark.parametrize("c", [c for c in CASES if c.c16], ids=case_id)
def test_first_pass16(gpu, oracle, tune_variant, c):
    """The first V pass over uint16 costs: the oracle's pass over the same integers as floats,
    and the den it writes equals the float pass's."""
    import torch

    import stereo_matchin_amd.kernels as K
    p = _params(c)
    assert K.raw16_supported(p)
    Dp, n = K.cost_shape(p)[2], c.d1 - c.d0
    Lh, Rh, cin, want = _pass_ref(oracle, c)
    assert cin.max() <= 765 and np.array_equal(cin, np.floor(cin))
    wl, wr = _supports(K, p, c, Lh, Rh, gpu)
    cin_h = pixel_major(cin, Dp)
    c32, c16 = _t(cin_h, gpu), _t(cin_h.astype(np.uint16).view(np.int16), gpu)
    want_d = _t(want, gpu).permute(1, 2, 0)
    den32 = torch.full(K.cost_shape(p), float("nan"), dtype=torch.float32, device=gpu)
    den16 = den32.clone()
    tune_variant(c.variant)
    K.asw_vCostAggregation(p, wl, wr, c32, den=den32, den_mode=PF.DEN_WRITE)
    for mode, name in zip(c.modes, case_names(c)):
        out = K.asw_vCostAggregation16(p, wl, wr, c16, den=den16 if mode else None, den_mode=mode)
        assert K.pass_kernel(PF.DIR_V, mode) == name
        _same_bits(out[:, :, :n], want_d, name)
    _same_bits(den16[:, :, :n], den32[:, :, :n], "den of " + name)


def large_bands(c):
    """Rows 0..4, the rows either side of each V strip boundary, the last 4 rows."""
    rows, nstrip = PF.v_strips(c.W, c.H, PF.pitch(c.d0, c.d1, c.D), c.T)
    return [(0, 4)] + [(s * rows - 1, s * rows + 1) for s in range(1, nstrip)] + [(c.H - 4, c.H)]


@pytest.mark.parametrize("c", LARGE_CASES, ids=case_id)
def test_policy_threshold(gpu, oracle, c):
    """The unforced dispatch at 256 MiB of volume.  A whole-volume oracle pass is out of reach:
    row bands against the crop reference, and the three den modes equal over the whole volume."""
    import torch

    import far_ref as F
    import stereo_matchin_amd.kernels as K
    p = _params(c)
    vs = K.cost_shape(p)
    assert vs == (c.H, c.W, c.D)
    assert (c.W * c.H * c.D * 4 >= 1 << 28) == case_names(c)[0].endswith(",nt>")
    Lh, Rh = _pair(c.T + c.H, c.H, c.W)
    wl, wr = _supports(K, p, c, Lh, Rh, gpu)
    cin = _t(np.random.default_rng(c.T + c.W).random(vs, dtype=np.float32) * np.float32(700), gpu)
    den = torch.full(vs, float("nan"), dtype=torch.float32, device=gpu)
    g = K.asw_vCostAggregation if c.direction == PF.DIR_V else K.asw_hCostAggregation
    outs = []
    for mode, name in zip(c.modes, case_names(c)):
        outs.append(g(p, wl, wr, cin, den=den if mode else None, den_mode=mode))
        assert K.pass_kernel(c.direction, mode) == name
    for y0, y1 in large_bands(c):
        want = _t(F.aggregate_pass(wl, wr, cin, c.D, c.T, c.direction, y0, y1), gpu)
        _same_bits(outs[0][y0:y1], want, f"{case_names(c)[0]} rows {y0}..{y1}")
    for out, name in zip(outs[1:], case_names(c)[1:]):
        assert torch.equal(out, outs[0]), name
