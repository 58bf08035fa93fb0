"""The speckle filter on the GPU (include/asw.h: asw_speckle, asw_lr_valid, asw_speckle_mask16,
asw_speckle_mask_f32, asw_set_speckle).

Every output is an integer function of the input alone, so every comparison is exact, against
the flood fill of tests/speckle_ref.py (pinned by tests/test_speckle.py).  The stage runs in
guard-banded buffers under both poisons (tests/guarded.py), workspace included.
"""
import os
import subprocess

import numpy as np
import pytest

import guarded as G
import speckle_ref as SK
import subpixel_ref as SR
from conftest import ROOT
from guarded import guarded_kernels  # noqa: F401  (a fixture, used by name)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("guarded_kernels")]

PKG = os.path.join(ROOT, "stereo_matchin_amd")
CLI = os.path.join(PKG, "asw_stereo")
KEYS = ("d_ref", "d_tar", "conf_ref", "conf_tar", "disp_rgba", "lr_rgba", "lr_red_rgba", "disp16", "lr16")
NO_LR_KEYS = tuple(k for k in KEYS if not k.startswith("lr"))  # a context without the check leaves those alone
SPK_KEYS = ("speckle_filtered16", "speckle_size", "speckle_keep")


def _p(W, H, D=16, T=5, iters=1, **kw):
    from stereo_matchin_amd import make_params
    return make_params(W, H, ndisp=D, taps=T, iters=iters, **kw)


def _sp(min_size, max_diff):
    from stereo_matchin_amd import default_speckle_params
    return default_speckle_params(min_size=min_size, max_diff=max_diff)


_REF = {}


def _ref(name, H, W, min_size, max_diff):
    """The generator's map and the reference's answer, computed once per case and shared."""
    key = (name, H, W, min_size, max_diff)
    if key not in _REF:
        d, valid = SK.GENERATORS[name](H, W)
        _REF[key] = (d, valid) + SK.components(d, valid, min_size, max_diff)
    return _REF[key]


# ------------------------------------------------------------------ the stage

@pytest.mark.parametrize("H,W", SK.SHAPES)
@pytest.mark.parametrize("name", sorted(SK.GENERATORS))
def test_stage_equals_the_reference_under_both_poisons(gpu, name, H, W):
    """label, size and keep equal the flood fill exactly for every (min_size, max_diff) pair, the
    status word is 0, and with the workspace and the outputs poisoned 0xFF and 0x5A every guard
    stays intact and every output element is the same."""
    import torch
    from stereo_matchin_amd import kernels as K
    p = _p(W, H)
    for min_size, max_diff in SK.PARAMS:
        d, valid, want_label, want_size, want_keep = _ref(name, H, W, min_size, max_diff)
        sp = _sp(min_size, max_diff)
        status = []

        def run(arena):
            with G.patched(arena):
                dd = arena.put("d", d)
                vv = None if valid is None else arena.put("valid", valid)
                label, size, keep, st = K.speckle(p, sp, dd, vv, return_status=True)
            status.append(st)
            return {"label": label, "size": size, "keep": keep}

        for got in G.run_twice(run, device=gpu):
            assert np.array_equal(got["label"].cpu().numpy(), want_label), (min_size, max_diff)
            assert np.array_equal(got["size"].cpu().numpy(), want_size), (min_size, max_diff)
            assert np.array_equal(got["keep"].cpu().numpy(), want_keep), (min_size, max_diff)
            assert got["label"].dtype == torch.int32 and got["keep"].dtype == torch.uint8
        assert status == [0, 0]


@pytest.mark.parametrize("H,W", [(17, 65), (50, 200)])
def test_null_valid_is_an_all_ones_map_and_null_outputs_are_accepted(gpu, H, W):
    import torch
    from stereo_matchin_amd import kernels as K
    p, sp = _p(W, H), _sp(3, 1)
    d = torch.from_numpy(SK.random(H, W, 11, 3, 0.0)[0]).to(gpu)
    ones = torch.ones((H, W), dtype=torch.uint8, device=gpu)
    full = K.speckle(p, sp, d, None, return_status=True)
    assert full[3] == 0
    want = SK.components(d.cpu().numpy(), None, 3, 1)
    for a, b, c in zip(full[:3], K.speckle(p, sp, d, ones), want):
        assert torch.equal(a, b) and np.array_equal(a.cpu().numpy(), c)
    names = ("label", "size", "keep")
    for mask in range(8):  # every combination of NULL outputs, none included
        sel = tuple(n for i, n in enumerate(names) if mask >> i & 1)
        got = K.speckle(p, sp, d, None, want=sel, return_status=True)
        assert got[3] == 0
        for i, n in enumerate(names):
            assert (got[i] is None) == (n not in sel)
            if got[i] is not None:
                assert torch.equal(got[i], full[i]), (sel, n)


# ------------------------------------------------------------------ the helpers

def _matched(gpu, p, seed=7):
    import torch
    from stereo_matchin_amd import StereoMatcher
    from stereo_matchin_amd.synthetic import make_pair
    Lh, Rh, _ = make_pair(p.width, p.height, p.ndisp, seed)
    return StereoMatcher(p, gpu).match(torch.from_numpy(Lh).to(gpu), torch.from_numpy(Rh).to(gpu), subpixel=True)


@pytest.mark.parametrize("lr_mode", [0, 1])
def test_lr_valid_is_the_lr_rule(gpu, lr_mode):
    from stereo_matchin_amd import kernels as K
    p = _p(160, 96, 32, lr_mode=lr_mode)
    res = _matched(gpu, p)
    if lr_mode == 1:  # the native rule does not read the codes
        got = K.lr_valid(p, res.d_ref, res.d_tar).cpu().numpy()
    else:
        got = K.lr_valid(p, res.d_ref, res.d_tar, res.code_ref, res.code_tar).cpu().numpy()
    want = SR.lr_pass(res.d_ref.cpu().numpy(), res.d_tar.cpu().numpy(), res.code_ref.cpu().numpy(),
                      res.code_tar.cpu().numpy(), 32, lr_mode)
    assert got.dtype == np.uint8 and np.array_equal(got, want.astype(np.uint8))
    assert want.any() and not want.all()


def test_masks_by_bits(gpu):
    import torch
    from stereo_matchin_amd import kernels as K
    H, W = 17, 65
    p = _p(W, H, 300)
    rng = np.random.default_rng(5)
    d = rng.integers(0, 300, (H, W)).astype(np.int32)
    d[0, 0], d[0, 1] = 70000, -1  # only the low 16 bits are stored
    keep = (rng.random((H, W)) < 0.6).astype(np.uint8) * rng.integers(1, 256, (H, W)).astype(np.uint8)
    disp = rng.uniform(0, 300, (H, W)).astype(np.float32)
    disp[1, 0] = np.float32(np.nan)
    dk = torch.from_numpy(keep).to(gpu)
    got16 = K.speckle_mask16(p, torch.from_numpy(d).to(gpu), dk).cpu().numpy().view(np.uint16)
    assert np.array_equal(got16, SK.mask16(d, keep))
    gotf = K.speckle_mask_f32(p, torch.from_numpy(disp).to(gpu), dk).cpu().numpy()
    want = disp.view(np.uint32).copy()
    want[keep == 0] = 0x7FC00000  # asw_disp_mask's quiet NaN
    assert np.array_equal(gotf.view(np.uint32), want)
    with pytest.raises(Exception):
        K.speckle_mask16(_p(W, H, 65536), torch.from_numpy(d).to(gpu), dk)


# ------------------------------------------------------------------ the frame API

def _stage_path(gpu, p, sp, frame):
    """The stage path on a frame's own d_ref and validity (its lr16 holes, when it has the check)."""
    import torch
    from stereo_matchin_amd import kernels as K
    d = torch.from_numpy(frame["d_ref"]).to(gpu)
    valid = None
    if p.lr_check:
        valid = torch.from_numpy((frame["lr16"] != 0xFFFF).astype(np.uint8)).to(gpu)
    _, size, keep, st = K.speckle(p, sp, d, valid, want=("size", "keep"), return_status=True)
    assert st == 0
    out = {"speckle_size": size.cpu().numpy(), "speckle_keep": keep.cpu().numpy()}
    if p.ndisp <= 65535:
        out["speckle_filtered16"] = K.speckle_mask16(p, d, keep).cpu().numpy().view(np.uint16)
    return out


def _check_frame(gpu, p, speckle, Lh, Rh, **ctx):
    """FrameContext(speckle=...) equals the stage path and the reference; every other output is
    byte-identical to the same context without the filter."""
    from stereo_matchin_amd import FrameContext, _lib
    sp = _lib.speckle_params_of(speckle)
    with FrameContext(p, **ctx) as fc:
        off = fc.match(Lh, Rh, want16=True)
    with FrameContext(p, speckle=speckle, **ctx) as fc:
        on = fc.match(Lh, Rh, want16=True)
        again = fc.match(Lh, Rh, want16=True)  # a graph context: capture, then replay
        fc.set_speckle(None)
        switched_off = fc.match(Lh, Rh, want16=True)
    assert not any(k.startswith("speckle_") for k in off) and not any(k.startswith("speckle_") for k in switched_off)
    for k in KEYS if p.lr_check else NO_LR_KEYS:
        assert np.array_equal(on[k], off[k], equal_nan=True), k
        assert np.array_equal(switched_off[k], off[k], equal_nan=True), k
    stage = _stage_path(gpu, p, sp, on)
    valid = on["lr16"] != 0xFFFF if p.lr_check else None
    _, want_size, want_keep = SK.components(on["d_ref"], valid, sp.min_size, sp.max_diff)
    for got in (on, again):
        assert np.array_equal(got["speckle_size"], want_size) and np.array_equal(got["speckle_keep"], want_keep)
        assert np.array_equal(got["speckle_filtered16"], SK.mask16(on["d_ref"], want_keep))
        for k in stage:
            assert got[k].dtype == stage[k].dtype and np.array_equal(got[k], stage[k]), k
    assert on["timings"]["total"] > 0
    return on


@pytest.fixture(scope="module")
def pair():
    from stereo_matchin_amd.synthetic import make_pair
    return make_pair(160, 96, 32, 7)[:2]


def test_frame_equals_the_stage_path(gpu, pair):
    on = _check_frame(gpu, _p(160, 96, 32, 9, 2), True, *pair)
    keep = on["speckle_keep"]
    assert keep.any() and not keep.all()
    assert (on["speckle_size"][(keep == 0) & (on["lr16"] != 0xFFFF)] < 32).all()  # removed, not merely inconsistent
    assert ((keep == 0) & (on["lr16"] != 0xFFFF)).any()


def test_frame_with_graph(gpu, pair):
    _check_frame(gpu, _p(160, 96, 32, 9, 2), True, *pair, graph=True)


def test_frame_with_sgm_and_census(gpu, pair):
    from stereo_matchin_amd import default_speckle_params
    _check_frame(gpu, _p(160, 96, 32, 9, 2), default_speckle_params(min_size=20, max_diff=2), *pair, sgm=True,
                 census=True)


def test_frame_without_lr_check(gpu, pair):
    on = _check_frame(gpu, _p(160, 96, 32, 9, 2, lr_check=0), True, *pair)
    assert (on["speckle_size"] > 0).all()  # every pixel is valid


def test_frame_d300_native_lr(gpu):
    from stereo_matchin_amd.synthetic import make_pair
    Lh, Rh, _ = make_pair(400, 32, 300, 5)
    on = _check_frame(gpu, _p(400, 32, 300, 9, 1, lr_mode=1), True, Lh, Rh)
    assert on["d_ref"].max() > 256


def test_frame_two_shards_equal_one(gpu, pair):
    p = _p(160, 96, 32, 9, 2)
    one = _check_frame(gpu, p, True, *pair)
    two = _check_frame(gpu, p, True, *pair, devices=(0, 0))
    for k in SPK_KEYS + KEYS:
        assert np.array_equal(one[k], two[k], equal_nan=True), k


def test_frame_batch_lands_at_the_right_offsets(gpu, pair):
    from stereo_matchin_amd import FrameContext
    from stereo_matchin_amd.synthetic import make_pair
    pairs = [pair, make_pair(160, 96, 32, 11)[:2]]
    with FrameContext(_p(160, 96, 32, 9, 2), speckle=True) as fc:
        single = [fc.match(L, R) for L, R in pairs]
        batch = fc.match_batch(np.stack([L for L, _ in pairs]), np.stack([R for _, R in pairs]))
    assert len(batch) == 2
    for a, b in zip(batch, single):
        for k in SPK_KEYS + ("d_ref",):
            assert np.array_equal(a[k], b[k]), k
    assert not np.array_equal(batch[0]["speckle_size"], batch[1]["speckle_size"])


@pytest.mark.parametrize("devices", [(0,), (0, 0)])
def test_frame_float_maps(gpu, pair, devices):
    """With subpixel=True the two float maps are mask_f32 of the frame's disp under the frame's
    keep, and subpixel_ref.fill of that; the sub-pixel maps themselves are those of a context
    without the filter."""
    import torch
    from stereo_matchin_amd import FrameContext
    from stereo_matchin_amd import kernels as K
    p = _p(160, 96, 32, 9, 2)
    with FrameContext(p, devices=devices) as fc:
        off = fc.match(*pair, want16=True, subpixel=True)
    with FrameContext(p, devices=devices, speckle=True) as fc:
        on = fc.match(*pair, want16=True, subpixel=True)
        plain = fc.match(*pair, want16=True)
    assert "speckle_disp_lr" not in plain and "speckle_disp_lr" not in off
    for k in KEYS + ("disp_sub", "disp_sub_lr", "disp_sub_filled"):
        assert np.array_equal(on[k], off[k], equal_nan=True), k
    for k in SPK_KEYS:
        assert np.array_equal(on[k], plain[k]), k
    masked = K.speckle_mask_f32(p, torch.from_numpy(on["disp_sub"]).to(gpu),
                                torch.from_numpy(on["speckle_keep"]).to(gpu)).cpu().numpy()
    assert np.array_equal(masked.view(np.uint32), SK.mask_f32(on["disp_sub"], on["speckle_keep"]).view(np.uint32))
    assert np.array_equal(on["speckle_disp_lr"].view(np.uint32), masked.view(np.uint32))
    assert SR.same_bits(on["speckle_disp_filled"], SR.fill(masked))
    assert np.isnan(on["speckle_disp_lr"]).sum() > np.isnan(on["disp_sub_lr"]).sum()


@pytest.mark.parametrize("lr_check", [1, 0])
def test_stereo_matcher_fields(gpu, pair, lr_check):
    """StereoMatcher(speckle=...) fills speckle_keep / speckle_size / filtered16 from its own d_ref
    and LR rule; without the keyword the fields stay None and the maps are the same."""
    import torch
    from stereo_matchin_amd import StereoMatcher, default_speckle_params
    p = _p(160, 96, 32, 9, 2, lr_check=lr_check)
    L, R = (torch.from_numpy(x).to(gpu) for x in pair)
    off = StereoMatcher(p, gpu).match(L, R)
    assert off.speckle_keep is None and off.speckle_size is None and off.filtered16 is None
    on = StereoMatcher(p, gpu, speckle=default_speckle_params(min_size=20)).match(L, R)
    assert torch.equal(on.d_ref, off.d_ref) and torch.equal(on.d_tar, off.d_tar)
    d = on.d_ref.cpu().numpy()
    valid = None
    if lr_check:
        valid = SR.lr_pass(d, on.d_tar.cpu().numpy(), on.code_ref.cpu().numpy(), on.code_tar.cpu().numpy(), 32, 0)
    _, want_size, want_keep = SK.components(d, valid, 20, 1)
    assert np.array_equal(on.speckle_size.cpu().numpy(), want_size)
    assert np.array_equal(on.speckle_keep.cpu().numpy(), want_keep)
    assert np.array_equal(on.filtered16.cpu().numpy().view(np.uint16), SK.mask16(d, want_keep))


def test_set_speckle_argument_rules(gpu):
    import ctypes
    from stereo_matchin_amd import FrameContext, _lib
    sp = _lib.default_speckle_params()
    with FrameContext(_p(64, 16, 16)) as fc:
        assert fc.L.asw_set_speckle(fc.ctx, ctypes.byref(sp), None) == _lib.ASW_E_INVALID
        bad = _lib.default_speckle_params(min_size=0)
        empty = _lib.AswSpeckleOutputs()
        assert fc.L.asw_set_speckle(fc.ctx, ctypes.byref(bad), ctypes.byref(empty)) == _lib.ASW_E_INVALID
        assert fc.L.asw_set_speckle(fc.ctx, None, None) == _lib.ASW_OK


# ------------------------------------------------------------------ CLI

def test_cli_speckle_png16(gpu, pair, tmp_path):
    PIL = pytest.importorskip("PIL.Image")
    from stereo_matchin_amd import FrameContext
    Lh, Rh = pair
    d = tmp_path / "syn"
    d.mkdir()
    PIL.fromarray(Lh[..., :3]).save(d / "im1.png")
    PIL.fromarray(Rh[..., :3]).save(d / "im5.png")
    (tmp_path / "pics.txt").write_text("syn/im1.png\nsyn/im5.png\n")
    r = subprocess.run([CLI, "--pics", str(tmp_path / "pics.txt"), "--runs", "1", "--ndisp", "32", "--taps", "9",
                        "--iters", "2", "--refine", "0", "--speckle", "--png16", "--tsv", str(tmp_path / "t.tsv")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    with FrameContext(_p(160, 96, 32, 9, 2), speckle=True) as fc:
        want = fc.match(Lh, Rh, want16=True)
    png = np.asarray(PIL.open(d / "asw_speckle16.png")).astype(np.int64)
    assert np.array_equal(png, want["speckle_filtered16"].astype(np.int64))
    assert (png == 0xFFFF).any() and (png != 0xFFFF).any()
    lr16 = np.asarray(PIL.open(d / "asw_consistency16.png")).astype(np.int64)
    assert np.array_equal(lr16, want["lr16"].astype(np.int64))
