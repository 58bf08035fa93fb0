"""The census / AD-census cost on the GPU (include/asw.h: asw_census, asw_census_cost,
asw_census_cost16, asw_set_census; stereo_matchin_amd/csrc/asw_census.hip).

Every comparison with tests/census_ref.py (pinned by tests/test_census.py) is exact:
array_equal on integers, float32 bit patterns on floats.
"""
import os
import subprocess

import numpy as np
import pytest

import census_ref as CR
import subpixel_ref as SR
from conftest import ROOT, plane_major
from guarded import guarded_kernels  # noqa: F401  (a fixture, used by name)

# every output the wrappers allocate is guarded and poisoned (tests/guarded.py)
pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("guarded_kernels")]

F = np.float32
PKG = os.path.join(ROOT, "stereo_matchin_amd")
CLI = os.path.join(PKG, "asw_stereo")
WINDOWS = [(9, 7), (7, 9), (5, 5), (3, 3), (9, 3)]
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


def _rand_pair(seed, H, W, shift=4):
    """A shifted, perturbed random pair; the alpha bytes are random too (never read)."""
    rng = np.random.default_rng(seed)
    L = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
    R = np.roll(L, -shift, axis=1).copy()
    R[..., :3] = np.clip(R[..., :3].astype(int) + rng.integers(-20, 21, (H, W, 3)), 0, 255).astype(np.uint8)
    R[..., 3] = rng.integers(0, 256, (H, W), dtype=np.uint8)
    return np.ascontiguousarray(L), np.ascontiguousarray(R)


def _census_gpu(gpu, p, cp, img):
    """asw_census into a pre-filled buffer (an unwritten pixel keeps the pattern)."""
    import torch
    from stereo_matchin_amd import kernels as K
    out = torch.full((p.height, p.width), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=gpu)
    K.census(p, cp, _t(img, gpu), out=out)
    return out


# ------------------------------------------------------------------ transform

@pytest.mark.parametrize("H,W", [(3, 5), (7, 9), (9, 70), (5, 257), (8, 128), (37, 66)])
def test_census_transform(gpu, H, W):
    """Images smaller than the window (every neighbour clamped), widths around the 64-pixel
    tile and (37, 66): more than one tile in both directions, ragged in both."""
    rng = np.random.default_rng(H * 1000 + W)
    rand = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
    two = np.full((H, W, 4), 100, np.uint8)  # two levels: ties dominate, the strict '<' decides
    two[..., :3] += rng.integers(0, 2, (H, W, 1), dtype=np.uint8)
    assert set(np.unique(CR.luma(two))) <= {100, 101}
    p = _p(W, H, 8)
    for w, h in WINDOWS:
        cp = _cp(win_w=w, win_h=h)
        for img in (rand, two):
            got = _np(_census_gpu(gpu, p, cp, img)).view(np.uint64)
            want = CR.census(img, w, h)
            assert np.array_equal(got, want), (w, h, np.argwhere(got != want)[:5])
        assert want.any() and (want >> np.uint64(w * h - 1) == 0).all()  # the upper bits are 0


# ------------------------------------------------------------------ cost

COST_SHAPES = [(70, 4, 16, 0, 16), (257, 3, 61, 0, 61), (64, 2, 65, 0, 65), (70, 4, 256, 0, 256),
               (10, 3, 61, 0, 61),  # W < D: xr clamps to 0 on most planes
               (70, 4, 256, 64, 128), (70, 4, 256, 0, 32), (70, 4, 256, 250, 256)]  # shards; the last two: pitch 32
# (tad_tau, window, w_a, w_c, has a uint16 form)
COST_FORMS = [(765.0, (9, 7), 1, 8, True), (40.5, (9, 7), 0, 8, True), (40.0, (7, 9), 1, 8, True),
              (40.5, (5, 5), 1, 8, False), (90.0, (9, 3), 64, 700, True)]


@pytest.mark.parametrize("W,H,D,d0,d1", COST_SHAPES)
def test_census_cost(gpu, W, H, D, d0, d1):
    import torch
    from stereo_matchin_amd import _lib
    from stereo_matchin_amd import kernels as K
    Lh, Rh = _rand_pair(W + D + d0, H, W)
    n = d1 - d0
    for tau, (w, h), wa, wc, has16 in COST_FORMS:
        p = _p(W, H, D, d_begin=d0, d_end=d1, tad_tau=tau)
        cp = _cp(win_w=w, win_h=h, ad_weight=wa, census_weight=wc)
        Dp = K.cost_shape(p)[2]
        assert Dp == (32 if (d0, d1) in ((0, 32), (250, 256)) else -(-n // 64) * 64)
        L, R = _t(Lh, gpu), _t(Rh, gpu)
        cl, cr = _census_gpu(gpu, p, cp, Lh), _census_gpu(gpu, p, cp, Rh)
        assert np.array_equal(_np(cl).view(np.uint64), CR.census(Lh, w, h))
        want = CR.cost_f32(Lh, Rh, D, tau, w, h, wa, wc, d0, d1)
        cost = torch.full(K.cost_shape(p), float("nan"), dtype=torch.float32, device=gpu)
        got = _np(K.census_cost(p, cp, L, R, cl, cr, out=cost))
        assert CR.same_bits(plane_major(got, n), want), np.argwhere(plane_major(got, n) != want)[:5]
        assert (got[:, :, n:].view(np.uint32) == 0).all()  # padding planes: exactly +0
        c16 = torch.full(K.cost_shape(p), -1, dtype=torch.int16, device=gpu)  # 0xFFFF
        assert K.census16_supported(p, cp) == has16
        if not has16:
            with pytest.raises(_lib.AswError) as e:
                K.census_cost16(p, cp, L, R, cl, cr, out=c16)
            assert e.value.status == _lib.ASW_E_UNSUPPORTED
            assert (c16 == -1).all()
            continue
        got16 = _np(K.census_cost16(p, cp, L, R, cl, cr, out=c16)).view(np.uint16)
        assert np.array_equal(plane_major(got16, n), CR.cost_u16(Lh, Rh, D, tau, w, h, wa, wc, d0, d1))
        assert (got16[:, :, n:] == 0).all()
        assert CR.same_bits(got16.astype(F), got)  # the two forms against each other, padding too


def test_census_cost_crafted_maximum(gpu):
    """L flat 100 with one white pixel, R flat 100 with a black one at the same place:
    ham 62, AD 765 at d = 0; with (w_a, w_c) = (3, 1000) the cost is 64295."""
    from stereo_matchin_amd import kernels as K
    Lh, Rh = CR.crafted_max_pair()
    H, W = Lh.shape[:2]
    p, cp = _p(W, H, 4), _cp(ad_weight=3, census_weight=1000)
    L, R = _t(Lh, gpu), _t(Rh, gpu)
    cl, cr = K.census(p, cp, L), K.census(p, cp, R)
    f = _np(K.census_cost(p, cp, L, R, cl, cr))
    u = _np(K.census_cost16(p, cp, L, R, cl, cr)).view(np.uint16)
    assert f[4, 8, 0] == 64295.0 and u[4, 8, 0] == 64295 and u.max() == 64295
    assert CR.same_bits(plane_major(f, 4), CR.cost_f32(Lh, Rh, 4, ad_weight=3, census_weight=1000))
    assert CR.same_bits(u.astype(F), f)


# ------------------------------------------------------------------ first pass on large costs

@pytest.mark.parametrize("T", [9, 35])
@pytest.mark.parametrize("D,d0,d1", [(16, 0, 16), (256, 32, 64)])
def test_first_pass_on_large_costs(gpu, oracle, T, D, d0, d1):
    """div_pos's operand range (asw_aggregate_impl.h): uint16 costs up to 65535 (the census
    maximum 64295 of the crafted pair, 65535 and 0 in blocks, random values between) through
    asw_aggregate_pass_den16 (den none and den write) and one float H pass, bit for bit
    against the oracle's passes on the same values; once on a 32-plane shard."""
    import torch
    from stereo_matchin_amd import _lib
    from stereo_matchin_amd import kernels as K
    W, H = 70, 40
    n = d1 - d0
    Lh, Rh = _rand_pair(T + D, H, W, shift=3)
    p = _p(W, H, D, T, d_begin=d0, d_end=d1)
    Dp = K.cost_shape(p)[2]
    assert Dp == (32 if D == 256 else 64)
    rng = np.random.default_rng(T * D)
    c = rng.integers(0, 65536, (n, H, W)).astype(np.uint16)
    c[:, 5:15, 10:40] = 64295
    c[: n // 2, 20:30, 30:60] = 65535
    c[:, 30:35, 0:20] = 0
    c[n // 2:, 0:5, :] = rng.choice(np.array([64295, 65535], np.uint16), (n - n // 2, 5, W))
    cin = c.astype(F)
    c16 = np.zeros((H, W, Dp), np.uint16)
    c16[:, :, :n] = np.transpose(c, (1, 2, 0))
    sv = [oracle.support(im, T, 0) for im in (Lh, Rh)]
    sh = [oracle.support(im, T, 1) for im in (Lh, Rh)]
    want_v = oracle.aggregate_pass(sv[0], sv[1], cin, T, 0, d0=d0, d1=d1, plane_base=d0)
    want_h = oracle.aggregate_pass(sh[0], sh[1], want_v, T, 1, d0=d0, d1=d1, plane_base=d0)
    assert want_v.max() > 60000.0
    L, R = _t(Lh, gpu), _t(Rh, gpu)
    wvl, wvr, whl, whr = K.asw_vSupport(p, L), K.asw_vSupport(p, R), K.asw_hSupport(p, L), K.asw_hSupport(p, R)
    dev16 = _t(c16.view(np.int16), gpu)
    for mode in (_lib.DEN_NONE, _lib.DEN_WRITE):
        den = torch.full(K.cost_shape(p), float("nan"), dtype=torch.float32, device=gpu)
        v = K.asw_vCostAggregation16(p, wvl, wvr, dev16, den=den if mode else None, den_mode=mode)
        got_v = plane_major(_np(v), n)
        assert CR.same_bits(got_v, want_v), (mode, np.argwhere(got_v != want_v)[:5])
        got_h = plane_major(_np(K.asw_hCostAggregation(p, whl, whr, v)), n)
        assert CR.same_bits(got_h, want_h), (mode, np.argwhere(got_h != want_h)[:5])


# ------------------------------------------------------------------ frame

W0, H0, D0, T0, R0 = 160, 96, 32, 9, 2


@pytest.fixture(scope="module")
def frame(gpu, oracle):
    """The (160, 96, 32) pair, T 9, r 2: census_ref cost -> oracle supports, passes, WTA and
    consistency, and a census frame of the one-shard context; shared by the frame tests."""
    from stereo_matchin_amd import FrameContext
    from stereo_matchin_amd.synthetic import make_pair
    Lh, Rh, gt = make_pair(W0, H0, D0, 7)
    want = CR.match(oracle, Lh, Rh, D0, T0, R0, CR.cost_f32(Lh, Rh, D0))
    p = _p(W0, H0, D0, T0, R0)
    with FrameContext(p, census=True) as fc:
        one = fc.match(Lh, Rh, want_cost=True, want16=True)
    with FrameContext(p) as fc:
        plain = fc.match(Lh, Rh, want_cost=True, want16=True)
    return {"L": Lh, "R": Rh, "gt": gt, "want": want, "p": p, "one": one, "plain": plain}


def _same_frame(got, want, cost=True):
    for k in FRAME_KEYS:
        assert np.array_equal(got[k], want[k]), k
    if cost:
        c = want["cost"]
        c = c if c.shape[0] == D0 else plane_major(c, D0)
        assert CR.same_bits(plane_major(got["cost"], D0), c)


def test_stage_pipeline_equals_reference(gpu, frame):
    from stereo_matchin_amd import StereoMatcher
    f = frame
    for flags in (0, 0x40):
        m = StereoMatcher(_p(W0, H0, D0, T0, R0, flags=flags), gpu, census=True)
        assert m.raw16 == (flags == 0)
        res = m.match(_t(f["L"], gpu), _t(f["R"], gpu))
        got = {"d_ref": _np(res.d_ref), "d_tar": _np(res.d_tar), "lr_red_rgba": _np(res.lr_red_rgba),
               "cost": _np(res.cost)}
        _same_frame(got, f["want"])
    assert not np.array_equal(got["d_ref"], f["plain"]["d_ref"])  # another cost than the AD frame's


def test_frame_equals_reference(gpu, frame):
    _same_frame(frame["one"], frame["want"])
    t = frame["one"]["timings"]
    assert t["raw_cost"] > 0 and t["total"] > t["raw_cost"]


@pytest.mark.parametrize("devices", [(0, 0), (0, 0, 0)])
def test_frame_sharded(gpu, frame, devices):
    from stereo_matchin_amd import FrameContext
    with FrameContext(frame["p"], devices=devices, census=True) as fc:
        assert len(fc.shards()) == len(devices)
        got = fc.match(frame["L"], frame["R"], want_cost=True)
    _same_frame(got, frame["want"])


def test_frame_rank_context(gpu, frame):
    from stereo_matchin_amd import FrameContext, comm_unique_id
    with FrameContext(frame["p"], devices=[0], rank=0, nranks=1, comm_id=comm_unique_id(), census=True) as fc:
        got = fc.match(frame["L"], frame["R"], want_cost=True)
    _same_frame(got, frame["want"])


def test_frame_float_volume(gpu, frame):
    """ASW_FLAG_RAW_F32, a fractional tau with w_a = 1 and a tap count without a ring kernel
    take asw_census_cost; the first gives the uint16 frame's results."""
    from stereo_matchin_amd import FrameContext, _lib
    with FrameContext(_p(W0, H0, D0, T0, R0, flags=_lib.FLAG_RAW_F32), census=True) as fc:
        _same_frame(fc.match(frame["L"], frame["R"], want_cost=True), frame["want"])


@pytest.mark.parametrize("tau,T,cen", [(40.5, 9, dict()), (765.0, 11, dict(win_w=5, win_h=5, ad_weight=2))])
def test_frame_float_path_parameters(gpu, oracle, frame, tau, T, cen):
    from stereo_matchin_amd import FrameContext
    from stereo_matchin_amd import kernels as K
    p, cp = _p(W0, H0, D0, T, R0, tad_tau=tau), _cp(**cen)
    assert not K.census16_supported(p, cp)
    Lh, Rh = frame["L"], frame["R"]
    want = CR.match(oracle, Lh, Rh, D0, T, R0, CR.cost_f32(Lh, Rh, D0, tau, cp.win_w, cp.win_h, cp.ad_weight,
                                                           cp.census_weight))
    with FrameContext(p, census=cp) as fc:
        _same_frame(fc.match(Lh, Rh, want_cost=True), want)


def test_frame_graph_and_switching(gpu, frame):
    """Graph on: census inside the captured frame (capture, replay); set_census(None) drops
    the captured graph and the next frames equal a context that never had census on; on
    again equals the reference again."""
    from stereo_matchin_amd import FrameContext
    f = frame
    with FrameContext(f["p"], graph=True, census=True) as fc:
        for _ in range(2):
            _same_frame(fc.match(f["L"], f["R"], want_cost=True), f["want"])
        fc.set_census(None)
        for _ in range(2):
            _same_frame(fc.match(f["L"], f["R"], want_cost=True), f["plain"])
        fc.set_census(_cp())
        _same_frame(fc.match(f["L"], f["R"], want_cost=True), f["want"])
    with FrameContext(f["p"], census=True) as fc:  # and without a graph
        fc.set_census(None)
        off = fc.match(f["L"], f["R"], want_cost=True, want16=True)
    for k in ("d_ref", "d_tar", "conf_ref", "conf_tar", "disp_rgba", "lr_rgba", "lr_red_rgba", "disp16", "lr16"):
        assert np.array_equal(off[k], f["plain"][k]), k
    assert CR.same_bits(off["cost"], f["plain"]["cost"])


def test_frame_batch(gpu, oracle, frame):
    from stereo_matchin_amd import FrameContext
    from stereo_matchin_amd.synthetic import make_pair
    f = frame
    L2, R2, _ = make_pair(W0, H0, D0, 3)
    with FrameContext(f["p"], census=True) as fc:
        batch = fc.match_batch(np.stack([f["L"], L2]), np.stack([f["R"], R2]), want_cost=True)
        single = fc.match(L2, R2, want_cost=True)
    assert len(batch) == 2
    _same_frame(batch[0], f["want"])
    _same_frame(batch[1], single)
    assert not np.array_equal(batch[0]["d_ref"], batch[1]["d_ref"])


def test_frame_refinement(gpu, frame):
    from stereo_matchin_amd import FrameContext, _lib
    f = frame
    rp = _lib.default_refine_params(iters=2)
    outs = []
    for devices in ((0,), (0, 0)):
        with FrameContext(f["p"], devices=devices, refine=rp, census=True) as fc:
            outs.append(fc.match(f["L"], f["R"]))
        _same_frame(outs[-1], f["want"], cost=False)  # the maps stay pre-refinement results
    assert np.array_equal(outs[0]["final_rgba"], outs[1]["final_rgba"])
    assert np.array_equal(outs[0]["post_red_rgba"], outs[1]["post_red_rgba"])


@pytest.mark.parametrize("devices", [(0,), (0, 0)])
def test_frame_subpixel(gpu, frame, devices):
    from stereo_matchin_amd import FrameContext
    f = frame
    with FrameContext(f["p"], devices=devices, census=True) as fc:
        got = fc.match(f["L"], f["R"], want_cost=True, want16=True, subpixel=True)
    _same_frame(got, f["want"])
    want = SR.subpixel_D(got["cost"], got["d_ref"], D0)
    assert SR.same_bits(got["disp_sub"], want)
    holes = got["lr16"] == 0xFFFF
    assert holes.any()
    assert SR.same_bits(got["disp_sub_lr"], SR.mask(want, ~holes))
    assert SR.same_bits(got["disp_sub_filled"], SR.fill(SR.mask(want, ~holes)))


def test_set_census_rejects_bad_parameters(gpu, frame):
    import ctypes
    from stereo_matchin_amd import FrameContext, _lib
    with FrameContext(frame["p"]) as fc:
        bad = _cp(win_w=9, win_h=9)
        assert fc.L.asw_set_census(fc.ctx, ctypes.byref(bad)) == _lib.ASW_E_INVALID
        _same_frame(fc.match(frame["L"], frame["R"], want_cost=True), frame["plain"])  # still off


# ------------------------------------------------------------------ robustness on the device

def test_gain_and_offset_on_the_device(gpu, frame):
    """The three rates of tests/test_census.py from the GPU's d_ref (AD through the ordinary
    path): it follows from parity and is asserted directly."""
    from stereo_matchin_amd import StereoMatcher
    f = frame
    L, Rg = _t(f["L"], gpu), _t(CR.gain_offset(f["R"]), gpu)
    rates = []
    for census in (None, _cp(ad_weight=0, census_weight=1), True):
        res = StereoMatcher(f["p"], gpu, census=census).match(L, Rg)
        rates.append(CR.bad_rate(_np(res.d_ref), f["gt"], D0))
    print("bad-pixel rates under gain 0.7 / +40 on the device: AD %.3f, census %.3f, AD + 8 census %.3f" % tuple(rates))
    assert rates[0] > 0.5
    assert rates[1] < 0.25
    assert rates[2] < 0.25


# ------------------------------------------------------------------ CLI

def test_cli_census(gpu, frame, tmp_path):
    PIL = pytest.importorskip("PIL.Image")
    f = frame
    d = tmp_path / "pair"
    d.mkdir()
    PIL.fromarray(f["L"][..., :3]).save(d / "left.png")
    PIL.fromarray(f["R"][..., :3]).save(d / "right.png")
    (tmp_path / "pics.txt").write_text("pair/left.png\npair/right.png\n")
    base = [CLI, "--pics", str(tmp_path / "pics.txt"), "--runs", "1", "--ndisp", str(D0), "--taps", str(T0),
            "--iters", str(R0), "--refine", "0", "--tsv", str(tmp_path / "t.tsv")]
    r = subprocess.run(base + ["--census"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    png = np.asarray(PIL.open(d / "asw_wta_disparity.png").convert("RGBA"))
    assert np.array_equal(png, f["one"]["disp_rgba"])
    assert not np.array_equal(png, f["plain"]["disp_rgba"])
    pre = np.asarray(PIL.open(d / "asw_consistency_pre-reff.png").convert("RGBA"))
    assert np.array_equal(pre, f["one"]["lr_red_rgba"])
    header = [ln for ln in (tmp_path / "t.tsv").read_text().splitlines() if ln.startswith("id\t")]
    assert header == ["id\taggr\tsupp_w\tv_aggr_mean\th_aggr_mean\ttotal aggregation\twta\tconsistency\ttotal\t"
                      "refine\th2d\td2h\texchange"]
    r = subprocess.run(base + ["--census-win", "9x9"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "asw_set_census" in r.stderr
    r = subprocess.run(base + ["--census-weights", "7"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "usage" in r.stderr
