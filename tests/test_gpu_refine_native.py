"""The native refinement loop (include/asw.h §native refinement) on an MI355X: the three
new stage kernels, asw_refine_native, the frame API (asw_set_refine_native: eager, graphed,
d-sharded) and the CLI, all bit-exact against the numpy restatement
tests/refine_native_ref.py (pinned to the C oracle by tests/test_refine_native.py)."""
import os
import subprocess

import numpy as np
import pytest

import refine_native_ref as RN
from conftest import plane_major
from guarded import guarded_kernels  # noqa: F401  (a fixture, used by name)

# every output the wrappers allocate is guarded and poisoned (tests/guarded.py)
pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("guarded_kernels")]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "stereo_matchin_amd", "asw_stereo")


def _t(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _np(t):
    return t.detach().cpu().numpy()


def _u16(t):
    return _np(t).view(np.uint16)


def _params(W, H, D, **kw):
    from stereo_matchin_amd import _lib, make_params
    kw.setdefault("lr_mode", _lib.LR_NATIVE)
    return make_params(W, H, ndisp=D, taps=5, iters=1, **kw)


def _pair(W, H, seed):
    from stereo_matchin_amd.synthetic import make_pair
    Lh, Rh, _ = make_pair(W, H, max(2, W // 3), seed, regions=6)
    return np.ascontiguousarray(Lh), np.ascontiguousarray(Rh)


def _same(got, want, name):
    assert got.dtype == want.dtype and got.shape == want.shape, (name, got.dtype, want.dtype)
    assert np.array_equal(got, want, equal_nan=True), (name, np.argwhere(got != want)[:5])


def _stage_inputs(W, H, D, seed):
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
    img[..., :3] //= 4  # small colour differences: weights well above zero
    img[..., 3] = 255
    est = rng.integers(0, D, (H, W)).astype(np.int32)
    conf = rng.random((H, W), dtype=np.float32)
    conf[rng.random((H, W)) < 0.3] = 0.0  # exact zeros
    return img, est, conf


# ------------------------------------------------------------------------ stage kernels

@pytest.mark.parametrize("W,H,Tr", [(70, 40, 33), (3, 5, 33), (19, 7, 1), (300, 3, 9)])
def test_v_and_h_estimates(gpu, oracle, W, H, Tr):
    """asw_ref_v_native on an int32 map of indices up to 599, and asw_ref_h at D 600 (the
    8-bit check refuses that D).  70 is no multiple of 64: the waves of the flattened image
    straddle rows; 3 x 5 is smaller than the window and than a wave; Tr 1 is the centre tap
    alone; 300 x 3 has more than one block."""
    import stereo_matchin_amd.kernels as K
    from stereo_matchin_amd import _lib
    D = 600
    p, rp = _params(W, H, D), _lib.default_refine_params(taps=Tr)
    img, est, conf = _stage_inputs(W, H, D, 7 * W + Tr)
    assert (conf == 0).any() or W * H < 20
    lut = K.refine_native_lut(p, rp, gpu)
    _same(_np(lut), RN.weight_lut(Tr), "lut")
    want_v = RN.ref_v(img, est.astype(np.float32), conf, Tr)
    got_v = K.asw_ref_v_native(p, rp, _t(img, gpu), _t(est, gpu), _t(conf, gpu), lut)
    _same(_np(got_v), want_v, "v")
    got_h = K.asw_ref_h(p, rp, _t(img, gpu), _t(conf, gpu), got_v, lut)
    _same(_np(got_h), RN.ref_h(img, conf, want_v, Tr), "h")


def test_consistency_native(gpu):
    """|d_ref - d_tar| of 0, 1 and 2 in both directions, indices above 255."""
    import stereo_matchin_amd.kernels as K
    W, H, D = 67, 9, 700
    rng = np.random.default_rng(3)
    d_ref = rng.integers(2, D - 2, (H, W)).astype(np.int32)
    delta = rng.integers(-2, 3, (H, W)).astype(np.int32)
    d_tar = d_ref + delta
    assert set(np.unique(delta)) == {-2, -1, 0, 1, 2}
    cr, ct = rng.random((H, W), dtype=np.float32) + 1, rng.random((H, W), dtype=np.float32) + 1
    p = _params(W, H, D)
    gcr, gct = _t(cr, gpu), _t(ct, gpu)
    est, post = K.consistency_native(p, _t(d_ref, gpu), _t(d_tar, gpu), gcr, gct)
    cons = np.abs(delta) <= 1
    _same(_np(est), np.where(cons, d_ref, d_tar).astype(np.int32), "est_left")
    _same(_u16(post), np.where(cons, d_ref, 0xFFFF).astype(np.uint16), "post16")
    _same(_np(gcr), np.where(cons, cr, 0).astype(np.float32), "conf_ref")
    _same(_np(gct), np.where(cons, ct, 0).astype(np.float32), "conf_tar")
    want = RN.native_est_left(d_ref, d_tar)
    _same(_np(est), want[0], "est_left (restatement)")
    _same(_u16(post), want[1], "post16 (restatement)")
    # without confidences (the pre-refinement est_left): the same maps
    est2, _ = K.consistency_native(p, _t(d_ref, gpu), _t(d_tar, gpu))
    _same(_np(est2), want[0], "est_left, no confidences")


@pytest.mark.parametrize("W,H", [(37, 5), (1, 1), (1, 4), (300, 2)])
def test_median16(gpu, W, H):
    """Values above 255 everywhere, the borders included (clamp-to-edge)."""
    import stereo_matchin_amd.kernels as K
    a = np.random.default_rng(W + H).integers(0, 65535, (H, W)).astype(np.int32)
    a[0, :] |= 0x4000
    a[:, -1] |= 0x8000
    got = _u16(K.Median16(_params(W, H, 65535), _t(a, gpu)))
    _same(got, RN.median3(a).astype(np.uint16), "median")
    assert got.max() > 255


# --------------------------------------------------------------------------- whole loop

_loops = {}


def _loop(gpu, D, W, H, k):
    """One (shape, k): the pre-refinement maps of a real aggregated volume (StereoMatcher at
    taps 5, iters 1), the asw_refine_native result from them and the restatement's, computed
    once and read only."""
    key = (D, W, H, k)
    if key not in _loops:
        from stereo_matchin_amd import StereoMatcher, _lib
        Lh, Rh = _pair(W, H, D + W)
        p = _params(W, H, D)
        rp = _lib.default_refine_params(iters=k)
        m = StereoMatcher(p, gpu)
        L, R = _t(Lh, gpu), _t(Rh, gpu)
        res = m.match(L, R)
        pre = {n: _np(getattr(res, n)).copy() for n in ("d_ref", "d_tar", "conf_ref", "conf_tar")}
        pre["cost"] = plane_major(_np(res.cost), D)
        out = m.refine(res, L, R, rp)
        got = {"d_ref": _np(out["d_ref"]), "d_tar": _np(out["d_tar"]), "conf_ref": _np(res.conf_ref),
               "conf_tar": _np(res.conf_tar), "est_left": _np(out["est_left"]), "post16": _u16(out["post16"]),
               "final16": _u16(out["final16"]), "pre_d_tar_after": _np(res.d_tar)}
        want = RN.refine_native_from_wta(Lh, Rh, D, pre["cost"], pre["d_ref"], pre["d_tar"], pre["conf_ref"],
                                         pre["conf_tar"], k)
        _loops[key] = dict(Lh=Lh, Rh=Rh, p=p, rp=rp, pre=pre, got=got, want=want)
    return _loops[key]


@pytest.mark.parametrize("D,W,H,k", [(300, 70, 40, 2), (512, 96, 24, 1)])
def test_whole_loop(gpu, oracle, D, W, H, k):
    """asw_refine_native against the restatement.  D 300 has pitch 320: padding planes are
    present and never scanned."""
    import stereo_matchin_amd.kernels as K
    c = _loop(gpu, D, W, H, k)
    assert K.cost_shape(c["p"])[2] == (320 if D == 300 else 512)
    got, want = c["got"], c["want"]
    for g, w in (("d_ref", "ref_d_ref"), ("d_tar", "ref_d_tar"), ("conf_ref", "ref_conf_ref"),
                 ("conf_tar", "ref_conf_tar"), ("est_left", "est_left"), ("post16", "post16"),
                 ("final16", "final16")):
        _same(got[g], want[w], g)
    _same(got["pre_d_tar_after"], c["pre"]["d_tar"], "the matcher's d_tar stays the pre-refinement map")
    # the loop did something: maps moved, and some pixels are inconsistent
    assert not np.array_equal(got["d_ref"], c["pre"]["d_ref"])
    assert (got["post16"] == 0xFFFF).any() and (got["post16"] != 0xFFFF).any()


# ---------------------------------------------------------------------------- frame API

PRE = ("d_ref", "d_tar", "conf_ref", "conf_tar", "disp_rgba", "lr_rgba", "lr_red_rgba", "disp16", "lr16")
FRAME = (300, 70, 40, 2)


def _frame_equals_stage(out, c):
    _same(out["final16"], c["got"]["final16"], "final16")
    _same(out["post16"], c["got"]["post16"], "post16")
    _same(out["refine_d_ref"], c["got"]["d_ref"], "refine_d_ref")
    _same(out["refine_d_tar"], c["got"]["d_tar"], "refine_d_tar")
    for n in ("d_ref", "d_tar"):
        _same(out[n], c["pre"][n], n)


def test_match_frame_equals_stage_loop(gpu, oracle):
    from stereo_matchin_amd import match_frame
    c = _loop(gpu, *FRAME)
    out = match_frame(c["p"], c["Lh"], c["Rh"], refine=c["rp"], want16=True)
    _frame_equals_stage(out, c)
    assert "final_rgba" not in out  # the 8-bit loop did not run
    assert out["timings"]["refine"] > 0


def test_frame_setter_leaves_pre_refinement_outputs(gpu, oracle):
    from stereo_matchin_amd import FrameContext
    c = _loop(gpu, *FRAME)
    with FrameContext(c["p"]) as plain, FrameContext(c["p"], refine=c["rp"]) as fc:
        a = plain.match(c["Lh"], c["Rh"], want16=True)
        b = fc.match(c["Lh"], c["Rh"], want16=True)
    assert a["timings"]["refine"] == 0 and "final16" not in a
    for n in PRE:
        _same(b[n], a[n], n)


def test_frame_graph_equals_eager(gpu, oracle):
    from stereo_matchin_amd import FrameContext
    c = _loop(gpu, *FRAME)
    with FrameContext(c["p"], refine=c["rp"], graph=True) as fc:
        outs = [fc.match(c["Lh"], c["Rh"], want16=True) for _ in range(2)]  # capture, then replay
    for out in outs:
        _frame_equals_stage(out, c)
        assert out["timings"]["refine"] > 0


def test_frame_three_shards_equal_one(gpu, oracle):
    """asw_create_multi with a repeated id: three d-shards on one device, the loop's scan
    through the asw_wta_ref_local protocol."""
    from stereo_matchin_amd import FrameContext
    c = _loop(gpu, *FRAME)
    with FrameContext(c["p"], devices=[0, 0, 0], refine=c["rp"]) as fc:
        assert len(fc.shards()) == 3
        out = fc.match(c["Lh"], c["Rh"], want16=True)
    _frame_equals_stage(out, c)
    assert out["timings"]["refine"] > 0


def test_one_loop_per_context(gpu):
    """asw_set_refine and asw_set_refine_native exclude each other; the 8-bit setter still
    refuses D 300."""
    import ctypes

    from stereo_matchin_amd import FrameContext, _lib
    rp = _lib.default_refine_params(iters=1)
    with FrameContext(_params(32, 16, 300)) as fc:
        assert fc.L.asw_set_refine(fc.ctx, ctypes.byref(rp)) == _lib.ASW_E_UNSUPPORTED
        assert fc.L.asw_set_refine_native(fc.ctx, ctypes.byref(rp), None) == _lib.ASW_E_INVALID
    with FrameContext(_params(32, 16, 61, lr_mode=_lib.LR_U8), refine=rp) as fc:
        assert fc.refine and fc.refine_native is None  # the 8-bit loop where it is built
        no = _lib.AswRefineNativeOutputs()
        assert fc.L.asw_set_refine_native(fc.ctx, ctypes.byref(rp), ctypes.byref(no)) == _lib.ASW_E_INVALID
        assert fc.L.asw_set_refine(fc.ctx, None) == _lib.ASW_OK
        assert fc.L.asw_set_refine_native(fc.ctx, ctypes.byref(rp), ctypes.byref(no)) == _lib.ASW_OK
        assert fc.L.asw_set_refine(fc.ctx, ctypes.byref(rp)) == _lib.ASW_E_INVALID


# ---------------------------------------------------------------------------------- CLI

def test_cli_writes_the_native_maps(gpu, oracle, tmp_path):
    """asw_stereo --ndisp 300 --refine 1 runs the native loop instead of skipping it and
    writes asw_disparity16.png / asw_consistency_post16.png: the frame API's maps."""
    import PIL.Image as PIL

    from stereo_matchin_amd import _lib, match_frame
    W, H, D = 70, 40, 300
    Lh, Rh = _pair(W, H, 11)
    d = tmp_path / "syn"
    d.mkdir()
    PIL.fromarray(Lh[..., :3]).save(d / "im0.png")
    PIL.fromarray(Rh[..., :3]).save(d / "im1.png")
    (tmp_path / "pics.txt").write_text("syn/im0.png\nsyn/im1.png\n")
    r = subprocess.run([CLI, "--pics", str(tmp_path / "pics.txt"), "--runs", "1", "--ndisp", str(D), "--taps", "5",
                        "--iters", "1", "--refine", "1", "--tsv", str(tmp_path / "t.tsv")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "skipped" not in r.stderr
    want = match_frame(_params(W, H, D), Lh, Rh, refine=_lib.default_refine_params(iters=1))
    for name, key in (("asw_disparity16.png", "final16"), ("asw_consistency_post16.png", "post16")):
        im = PIL.open(d / name)
        assert im.mode.startswith("I"), name
        _same(np.asarray(im).astype(np.uint16), want[key], name)
    assert not (d / "asw_disparity.png").exists()  # the 8-bit images belong to the 8-bit loop
    row = [ln for ln in (tmp_path / "t.tsv").read_text().splitlines() if ln[:1].isdigit()][0].split("\t")
    assert float(row[9]) > 0  # the refine column
