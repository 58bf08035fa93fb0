"""Semi-global matching on the GPU (include/asw.h: asw_sgm_path, asw_sgm, asw_set_sgm;
stereo_matchin_amd/csrc/asw_sgm.hip).

Every comparison with tests/sgm_ref.py (pinned by tests/test_sgm.py) is exact: array_equal on
integers, float32 bit patterns on volumes.
"""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

import census_ref as CR
import sgm_ref as SG
import subpixel_ref as SR
from conftest import ROOT, plane_major
from guarded import guarded_kernels  # noqa: F401  (a fixture, used by name)

# every output the wrappers allocate is guarded and poisoned (tests/guarded.py)
pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("guarded_kernels")]

F = np.float32
PKG = os.path.join(ROOT, "stereo_matchin_amd")
CLI = os.path.join(PKG, "asw_stereo")
# (W, H, D): a one-pixel image; W < H and H < W (a diagonal restarts on a side border before
# and after a top / bottom one); one wave with 1, 2 and 4 planes per lane, ragged lanes, the
# 64-lane seam (D 65: pitch 128), several waves per pixel (D 300: pitch 320, not a power of two);
# and tiny images with a ragged D above 4096, 16384 and 32768 planes of pitch: the forms with
# 16, 32 and 64 planes per thread (sums read and written inside the step, costs loaded in
# 8-plane chunks inside the chain, the one form with scratch), on row, column and diagonal paths
SHAPES = [(1, 1, 1), (5, 3, 2), (70, 4, 16), (4, 70, 61), (66, 37, 64), (9, 6, 65), (20, 5, 256), (7, 3, 300),
          (3, 2, 4999), (2, 3, 19999), (3, 2, 39999)]
PENALTIES = [(0, 0), (16, 128), (100, 20000), (1048576, 1048576)]
FRAME_KEYS = ("d_ref", "d_tar", "lr_red_rgba")


def _t(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _np(t):
    return t.detach().cpu().numpy()


def _p(W, H, D, T=5, iters=1, **kw):
    from stereo_matchin_amd import make_params
    return make_params(W, H, ndisp=D, taps=T, iters=iters, **kw)


def _cp(**kw):
    from stereo_matchin_amd import default_census_params
    return default_census_params(**kw)


def _sp(**kw):
    from stereo_matchin_amd import default_sgm_params
    return default_sgm_params(**kw)


@functools.lru_cache(maxsize=None)
def _costs(W, H, D):
    """uint16 [D][H][W] over the full range, with blocks of 0 and of 65535 (read-only)."""
    rng = np.random.default_rng(W * 10007 + H * 101 + D)
    c = rng.integers(0, 65536, (D, H, W)).astype(np.uint16)
    c[: (D + 1) // 2, : (H + 1) // 2, : (W + 2) // 3] = 0
    c[D // 2:, H // 2:, W // 2:] = 65535
    if D * H * W > 4:
        c[0, 0, 0], c[-1, -1, -1] = 12345, 54321
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def _paths(W, H, D, p1, p2):
    """The eight reference path volumes of a shape, computed once and shared (read-only)."""
    out = tuple(SG.path(_costs(W, H, D), k, p1, p2) for k in range(8))
    for a in out:
        a.setflags(write=False)
    return out


def _device_cost(gpu, W, H, D, Dp, pad):
    """int16 storage [H][W][Dp] of the shape's costs, padding planes set to ``pad``."""
    c = np.full((H, W, Dp), pad, np.uint16)
    c[:, :, :D] = np.transpose(_costs(W, H, D), (1, 2, 0))
    return _t(c.view(np.int16), gpu)


def _bits_equal(got_hwd, want_dhw, D):
    return CR.same_bits(plane_major(got_hwd, D), want_dhw.astype(F))


# ------------------------------------------------------------------ paths

@pytest.mark.parametrize("W,H,D", SHAPES)
def test_paths(gpu, W, H, D):
    """asw_sgm_path for every k: written into a NaN-filled volume (padding exactly +0) and
    accumulated onto a known integer volume (padding kept); once with the padding planes of C
    at 0 and once at 0xFFFF: padding that reaches m or a d+1 neighbour fails one of the two."""
    import torch
    from stereo_matchin_amd import kernels as K
    p = _p(W, H, D)
    Dp = K.cost_shape(p)[2]
    assert Dp == -(-D // 64) * 64
    rng = np.random.default_rng(D)
    base = rng.integers(0, 1 << 20, (H, W, Dp)).astype(F)
    base[:, :, D:] = -7.5  # padding of the accumulated volume: left as it is
    for pad in (0, 0xFFFF):
        c16 = _device_cost(gpu, W, H, D, Dp, pad)
        for p1, p2 in PENALTIES:
            sp = _sp(p1=p1, p2=p2)
            want = _paths(W, H, D, p1, p2)
            for k in range(8):
                out = torch.full(K.cost_shape(p), float("nan"), dtype=torch.float32, device=gpu)
                got = _np(K.sgm_path(p, sp, k, c16, out=out))
                assert _bits_equal(got, want[k], D), (pad, p1, p2, k, np.argwhere(plane_major(got, D) != want[k])[:5])
                assert (got[:, :, D:].view(np.uint32) == 0).all(), (pad, p1, p2, k)  # exactly +0
                acc = _np(K.sgm_path(p, sp, k, c16, out=_t(base, gpu), accumulate=True))
                assert _bits_equal(acc, plane_major(base, D).astype(np.int64) + want[k], D), (pad, p1, p2, k)
                assert CR.same_bits(acc[:, :, D:], base[:, :, D:]), (pad, p1, p2, k)
            # a guarded, poisoned output of the wrapper's own (the fixture checks its guards)
            got = _np(K.sgm_path(p, sp, 4, c16))
            assert _bits_equal(got, want[4], D) and (got[:, :, D:].view(np.uint32) == 0).all()


@pytest.mark.parametrize("W,H,D", SHAPES)
def test_sum(gpu, W, H, D):
    """asw_sgm for 4 and 8 paths into a poisoned volume: S on the valid planes, +0 on padding."""
    from stereo_matchin_amd import kernels as K
    p = _p(W, H, D)
    Dp = K.cost_shape(p)[2]
    for pad in (0, 0xFFFF):
        c16 = _device_cost(gpu, W, H, D, Dp, pad)
        for p1, p2 in PENALTIES:
            want = _paths(W, H, D, p1, p2)
            for n in (4, 8):
                got = _np(K.sgm(p, _sp(paths=n, p1=p1, p2=p2), c16))
                S = sum(want[:n])
                assert S.max() < 2 ** 24
                assert _bits_equal(got, S, D), (pad, p1, p2, n, np.argwhere(plane_major(got, D) != S)[:5])
                assert (got[:, :, D:].view(np.uint32) == 0).all(), (pad, p1, p2, n)


def test_absent_neighbour_terms(gpu):
    """D = 1 (only the d and the m + P2 terms: L = C) and D = 2 against closed forms."""
    from stereo_matchin_amd import kernels as K
    W, H = 5, 3
    for D in (1, 2):
        p = _p(W, H, D)
        c16 = _device_cost(gpu, W, H, D, 64, 0xFFFF)
        C = _costs(W, H, D).astype(np.int64)
        for k in range(8):
            got = plane_major(_np(K.sgm_path(p, _sp(p1=3, p2=9), k, c16)), D)
            if D == 1:  # m = L(q, 0): min(L, m + P2) - m = 0
                assert np.array_equal(got, C.astype(F)), k
            else:
                assert np.array_equal(got, SG.path(C, k, 3, 9).astype(F)), k


def test_rejections(gpu):
    import torch
    from stereo_matchin_amd import _lib
    from stereo_matchin_amd import kernels as K
    p = _p(8, 4, 16)
    c16 = _device_cost(gpu, 8, 4, 16, 64, 0)
    out = torch.zeros(K.cost_shape(p), dtype=torch.float32, device=gpu)
    for k in (-1, 8):
        with pytest.raises(_lib.AswError) as e:
            K.sgm_path(p, _sp(), k, c16, out=out)
        assert e.value.status == _lib.ASW_E_INVALID
    with pytest.raises(_lib.AswError) as e:
        K.sgm(p, _sp(paths=5), c16, out=out)
    assert e.value.status == _lib.ASW_E_INVALID
    with pytest.raises(_lib.AswError) as e:
        K.sgm(_p(8, 4, 16, d_begin=0, d_end=8), _sp(), c16[:, :, :32].contiguous())
    assert e.value.status == _lib.ASW_E_INVALID
    assert (out == 0).all()
    # k >= 4 is allowed whatever sp.paths says
    got = _np(K.sgm_path(p, _sp(paths=4), 6, c16))
    assert _bits_equal(got, _paths(8, 4, 16, 16, 128)[6], 16)


# ------------------------------------------------------------------ frame

W0, H0, D0, T0, R0 = 160, 96, 32, 9, 2


def _ad_u16(Lh, Rh, D):
    z = np.zeros(Lh.shape[:2], np.uint64)
    return CR.terms(Lh, Rh, z, z, D)[0]


def _want_frame(oracle, C, sp=None):
    """sgm_ref -> oracle WTA -> oracle consistency on an integer raw cost [D][H][W]."""
    kw = SG.DEFAULT if sp is None else dict(paths=sp.paths, p1=sp.p1, p2=sp.p2)
    S = np.ascontiguousarray(SG.sgm(C, **kw).astype(F))
    dr, cr, dt, ct = oracle.wta(S)
    D = S.shape[0]
    lr, red, _, _ = oracle.consistency(oracle.code_u8(dr, D), oracle.code_u8(dt, D), cr, ct, D)
    return {"d_ref": dr, "d_tar": dt, "lr_rgba": lr, "lr_red_rgba": red, "cost": S}


@pytest.fixture(scope="module")
def frame(gpu, oracle):
    """The (160, 96, 32) pair 7: the reference frames on the AD and the default census cost, the
    SGM frames of a one-shard context and the plain ASW frame; shared by the frame tests."""
    from stereo_matchin_amd import FrameContext
    from stereo_matchin_amd.synthetic import make_pair
    Lh, Rh, gt = make_pair(W0, H0, D0, 7)
    p = _p(W0, H0, D0, T0, R0)
    want = {False: _want_frame(oracle, _ad_u16(Lh, Rh, D0)), True: _want_frame(oracle, CR.cost_u16(Lh, Rh, D0))}
    got = {}
    for census in (False, True):
        with FrameContext(p, census=census or None, sgm=True) as fc:
            got[census] = fc.match(Lh, Rh, want_cost=True, want16=True)
    with FrameContext(p) as fc:
        plain = fc.match(Lh, Rh, want_cost=True, want16=True)
    return {"L": Lh, "R": Rh, "gt": gt, "p": p, "want": want, "got": got, "plain": plain}


def _same_frame(got, want, cost=True):
    for k in FRAME_KEYS:
        assert np.array_equal(got[k], want[k]), k
    if cost:
        c = want["cost"]
        c = c if c.shape[0] == D0 else plane_major(c, D0)
        assert CR.same_bits(plane_major(got["cost"], D0), c)


@pytest.mark.parametrize("census", [False, True])
def test_frame_equals_reference(gpu, frame, census):
    got = frame["got"][census]
    _same_frame(got, frame["want"][census])
    assert (got["cost"][:, :, D0:].view(np.uint32) == 0).all()
    assert not np.array_equal(got["d_ref"], frame["plain"]["d_ref"])  # another aggregator than ASW
    t = got["timings"]
    assert t["aggregation_total"] > 0 and t["support"] == 0
    assert t["v_pass_mean"] == 0 and t["h_pass_mean"] == 0 and t["total"] >= t["aggregation_total"]


@pytest.mark.parametrize("census", [False, True])
def test_stage_pipeline_equals_reference(gpu, frame, census):
    from stereo_matchin_amd import StereoMatcher
    f = frame
    for flags in (0, 0x40):  # ASW_FLAG_RAW_F32 is ignored while SGM is on
        m = StereoMatcher(_p(W0, H0, D0, T0, R0, flags=flags), gpu, census=census or None, sgm=True)
        res = m.match(_t(f["L"], gpu), _t(f["R"], gpu))
        got = {"d_ref": _np(res.d_ref), "d_tar": _np(res.d_tar), "lr_red_rgba": _np(res.lr_red_rgba),
               "cost": _np(res.cost)}
        _same_frame(got, f["want"][census])


def test_frame_raw_f32_flag_is_ignored(gpu, frame):
    from stereo_matchin_amd import FrameContext, _lib
    with FrameContext(_p(W0, H0, D0, T0, R0, flags=_lib.FLAG_RAW_F32), sgm=True) as fc:
        _same_frame(fc.match(frame["L"], frame["R"], want_cost=True), frame["want"][False])


@pytest.mark.parametrize("T,iters", [(11, 2), (9, 0), (11, 0)])
def test_frame_reads_neither_taps_nor_iters(gpu, frame, T, iters):
    """A tap count without a ring kernel and iters = 0 work: no pass is launched."""
    from stereo_matchin_amd import FrameContext
    with FrameContext(_p(W0, H0, D0, T, iters), sgm=True) as fc:
        got = fc.match(frame["L"], frame["R"], want_cost=True)
    _same_frame(got, frame["want"][False])
    assert got["timings"]["aggregation_total"] > 0


def test_frame_other_parameters(gpu, oracle, frame):
    from stereo_matchin_amd import FrameContext
    sp = _sp(paths=4, p1=8, p2=64)
    C = CR.cost_u16(frame["L"], frame["R"], D0)
    with FrameContext(frame["p"], census=True, sgm=sp) as fc:
        _same_frame(fc.match(frame["L"], frame["R"], want_cost=True), _want_frame(oracle, C, sp))


def test_set_sgm_rejections(gpu, frame):
    from stereo_matchin_amd import FrameContext, _lib
    f = frame
    sp = _sp()
    # a fractional tau with an AD term has no uint16 cost: refused, the context keeps working
    with FrameContext(_p(W0, H0, D0, T0, R0, tad_tau=40.5)) as fc:
        assert fc.L.asw_set_sgm(fc.ctx, ctypes.byref(sp)) == _lib.ASW_E_UNSUPPORTED
        with FrameContext(_p(W0, H0, D0, T0, R0, tad_tau=40.5)) as never:
            want = never.match(f["L"], f["R"], want_cost=True)
        _same_frame(fc.match(f["L"], f["R"], want_cost=True), want)
        fc.set_census(_cp(ad_weight=0, census_weight=1))  # census only: tau is not read
        fc.set_sgm(True)
        assert fc.L.asw_set_census(fc.ctx, ctypes.byref(_cp())) == _lib.ASW_E_UNSUPPORTED  # back to an AD term
        assert fc.L.asw_set_census(fc.ctx, None) == _lib.ASW_E_UNSUPPORTED
        fc.match(f["L"], f["R"])
    with FrameContext(f["p"], devices=(0, 0)) as fc:  # more than one shard
        assert fc.L.asw_set_sgm(fc.ctx, ctypes.byref(sp)) == _lib.ASW_E_UNSUPPORTED
        _same_frame(fc.match(f["L"], f["R"], want_cost=True), f["plain"])
    with pytest.raises(_lib.AswError) as e:
        FrameContext(f["p"], devices=(0, 0), sgm=True)
    assert e.value.status == _lib.ASW_E_UNSUPPORTED
    # a pitch asw_raw_cost16's LDS stage does not hold: refused at the setter, not at the first match
    with FrameContext(_p(4, 2, 20000, 5, 1, lr_mode=_lib.LR_NATIVE)) as fc:
        assert fc.L.asw_set_sgm(fc.ctx, ctypes.byref(sp)) == _lib.ASW_E_UNSUPPORTED
    with FrameContext(f["p"]) as fc:
        bad = _sp(p1=200)
        assert fc.L.asw_set_sgm(fc.ctx, ctypes.byref(bad)) == _lib.ASW_E_INVALID
        _same_frame(fc.match(f["L"], f["R"], want_cost=True), f["plain"])  # still off


def test_frame_graph_and_switching(gpu, frame):
    """Graph on: SGM inside the captured frame (capture, replay); set_sgm(None) drops the graph
    and the next frames equal a context that never had it; on again equals the reference."""
    from stereo_matchin_amd import FrameContext
    f = frame
    with FrameContext(f["p"], graph=True, sgm=True) as fc:
        for _ in range(2):
            _same_frame(fc.match(f["L"], f["R"], want_cost=True), f["want"][False])
        fc.set_sgm(None)
        for _ in range(2):
            _same_frame(fc.match(f["L"], f["R"], want_cost=True), f["plain"])
        fc.set_sgm(_sp())
        _same_frame(fc.match(f["L"], f["R"], want_cost=True), f["want"][False])
    with FrameContext(f["p"], sgm=True) as fc:  # and without a graph
        fc.set_sgm(None)
        off = fc.match(f["L"], f["R"], want_cost=True, want16=True)
    for k in ("d_ref", "d_tar", "conf_ref", "conf_tar", "disp_rgba", "lr_rgba", "lr_red_rgba", "disp16", "lr16"):
        assert np.array_equal(off[k], f["plain"][k]), k
    assert CR.same_bits(off["cost"], f["plain"]["cost"])


def test_frame_batch(gpu, frame):
    from stereo_matchin_amd import FrameContext
    from stereo_matchin_amd.synthetic import make_pair
    f = frame
    L2, R2, _ = make_pair(W0, H0, D0, 3)
    with FrameContext(f["p"], sgm=True) as fc:
        batch = fc.match_batch(np.stack([f["L"], L2]), np.stack([f["R"], R2]), want_cost=True)
        single = fc.match(L2, R2, want_cost=True)
    assert len(batch) == 2
    _same_frame(batch[0], f["want"][False])
    _same_frame(batch[1], single)
    assert not np.array_equal(batch[0]["d_ref"], batch[1]["d_ref"])


def test_frame_subpixel(gpu, frame):
    from stereo_matchin_amd import FrameContext
    f = frame
    with FrameContext(f["p"], census=True, sgm=True) as fc:
        got = fc.match(f["L"], f["R"], want_cost=True, want16=True, subpixel=True)
    _same_frame(got, f["want"][True])
    want = SR.subpixel_D(got["cost"], got["d_ref"], D0)
    assert SR.same_bits(got["disp_sub"], want)
    holes = got["lr16"] == 0xFFFF
    assert holes.any()
    assert SR.same_bits(got["disp_sub_lr"], SR.mask(want, ~holes))
    assert SR.same_bits(got["disp_sub_filled"], SR.fill(SR.mask(want, ~holes)))


def test_frame_native_refinement(gpu, frame):
    """The native loop with iters = 2 runs on the sums and leaves the pre-refinement maps."""
    from stereo_matchin_amd import FrameContext, _lib
    f = frame
    rp = _lib.default_refine_params(iters=2)
    p = _p(W0, H0, D0, T0, R0, lr_mode=_lib.LR_NATIVE)
    with FrameContext(p, sgm=True) as fc:
        pre = fc.match(f["L"], f["R"], want_cost=True, want16=True)
    with FrameContext(p, refine=rp, sgm=True) as fc:
        assert fc.refine_native is not None
        out = fc.match(f["L"], f["R"], want_cost=True, want16=True)
    for k in ("d_ref", "d_tar", "conf_ref", "conf_tar", "disp_rgba", "lr_rgba", "lr_red_rgba", "disp16", "lr16"):
        assert np.array_equal(out[k], pre[k]), k
    assert np.array_equal(out["d_ref"], f["want"][False]["d_ref"])
    assert CR.same_bits(out["cost"], pre["cost"])
    assert out["final16"].max() < D0 and out["timings"]["refine"] > 0


def test_frame_with_cross(gpu, frame):
    """asw_set_cross runs ahead in the same two volumes; the SGM frame is unchanged."""
    from stereo_matchin_amd import FrameContext
    f = frame
    with FrameContext(f["p"], sgm=True) as fc:
        fc.set_cross(True)
        got = fc.match(f["L"], f["R"], want_cost=True)
    _same_frame(got, f["want"][False])
    assert "cross_final_rgba" in got


# ------------------------------------------------------------------ CLI

def test_cli_sgm(gpu, frame, tmp_path):
    PIL = pytest.importorskip("PIL.Image")
    f = frame
    d = tmp_path / "pair"
    d.mkdir()
    PIL.fromarray(f["L"][..., :3]).save(d / "left.png")
    PIL.fromarray(f["R"][..., :3]).save(d / "right.png")
    (tmp_path / "pics.txt").write_text("pair/left.png\npair/right.png\n")
    base = [CLI, "--pics", str(tmp_path / "pics.txt"), "--runs", "1", "--ndisp", str(D0), "--taps", str(T0),
            "--iters", str(R0), "--refine", "0", "--tsv", str(tmp_path / "t.tsv")]
    r = subprocess.run(base + ["--sgm"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    png = np.asarray(PIL.open(d / "asw_wta_disparity.png").convert("RGBA"))
    assert np.array_equal(png, f["got"][False]["disp_rgba"])
    assert not np.array_equal(png, f["plain"]["disp_rgba"])
    header = [ln for ln in (tmp_path / "t.tsv").read_text().splitlines() if ln.startswith("id\t")]
    assert header == ["id\taggr\tsupp_w\tv_aggr_mean\th_aggr_mean\ttotal aggregation\twta\tconsistency\ttotal\t"
                      "refine\th2d\td2h\texchange"]
    r = subprocess.run(base + ["--sgm-paths", "5"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "asw_set_sgm" in r.stderr
    r = subprocess.run(base + ["--sgm-penalties", "7"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "usage" in r.stderr
    for bad in (["--sgm-paths", "-3"], ["--sgm-penalties", "-1,5"]):  # well-formed: the library's to reject
        r = subprocess.run(base + bad, capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "asw_set_sgm" in r.stderr, bad
