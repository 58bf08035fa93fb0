"""The guard-band harness (tests/guarded.py) on CPU tensors: fake stages, written in Python,
each with one planted defect of the kind a subtly wrong kernel has.  The harness must
report every one of them with the buffer's name and the offset, and pass the correct
stage: this is how it is shown to catch a wrong kernel without running one on a GPU."""
import numpy as np
import pytest
import torch

import guarded as G
from guarded import guarded_kernels  # noqa: F401  (a fixture, used by name)

H, W, D, DP = 3, 5, 9, 16  # a [H][W][DP] volume with D valid planes: 7 padding planes


def _cin():
    rng = np.random.default_rng(1)
    c = np.zeros((H, W, DP), np.float32)
    c[:, :, :D] = rng.random((H, W, D), dtype=np.float32) * 700
    return c


def _stage(defect=None):
    """out[y][x][d] = 2 * cin[y][x][d] for d < D, padding planes zero."""

    def fn(arena):
        cin = arena.put("cin", _cin(), fill=G.NAN, valid=np.s_[:, :, :D])
        out = arena.out("cout", (H, W, DP), torch.float32, row_bytes=W * DP * 4)
        before = out.clone()
        flat = arena.find(out).base[arena.find(out).off:].view(torch.float32)  # the body and what follows
        front = arena.find(out).base[:arena.find(out).off].view(torch.float32)
        out[:, :, :D] = 2 * cin[:, :, :D]
        out[:, :, D:] = 0
        if defect == "one past the end":
            flat[H * W * DP] = 1.0
        elif defect == "one before the start":
            front[-1] = 1.0
        elif defect == "a row past the end":
            flat[H * W * DP + W * DP - 1] = 1.0
        elif defect == "unwritten":
            out[1, 2, 3] = before[1, 2, 3]
        elif defect == "previous contents":
            out[2, 4, 8] = before[2, 4, 7] * 0.5 if torch.isfinite(before[2, 4, 7]) else before[2, 4, 7]
        elif defect == "input padding":
            out[0, 1, D - 1] = cin[0, 1, D - 1] + cin[0, 1, D]
        elif defect == "padding unwritten":
            out[2, 0, D + 1] = before[2, 0, D + 1]
        return {"cout": out}

    return fn


SPEC = {"cout": G.Out(valid=np.s_[:, :, :D], pad=0, finite=True)}


def _elem(y, x, d):
    return f"'cout' element ({y}, {x}, {d}) (byte offset {((y * W + x) * DP + d) * 4},"


def test_correct_stage_passes():
    a, b = G.run_twice(_stage(), SPEC)
    assert torch.equal(a["cout"], b["cout"])
    assert np.array_equal(a["cout"].numpy()[:, :, :D], 2 * _cin()[:, :, :D])


DEFECTS = [
    ("one past the end", f"guard of 'cout' damaged: back guard, first at byte offset {H * W * DP * 4} "),
    ("one before the start", "guard of 'cout' damaged: front guard, first at byte offset -4 "),
    ("a row past the end", f"guard of 'cout' damaged: back guard, first at byte offset {(H + 1) * W * DP * 4 - 4} "),
    ("unwritten", "valid region depends on the previous contents (unwritten, or computed from them): "
     + _elem(1, 2, 3)),
    ("previous contents", "valid region depends on the previous contents (unwritten, or computed from them): "
     + _elem(2, 4, 8)),
    ("input padding", "valid region is not finite (computed from an input's padding, its guard or the poison): "
     + _elem(0, 1, D - 1)),
    ("padding unwritten", "specified padding depends on the previous contents (unwritten): " + _elem(2, 0, D + 1)),
]


@pytest.mark.parametrize("defect,report", DEFECTS, ids=[d.replace(" ", "-") for d, _ in DEFECTS])
def test_planted_defect_is_reported(defect, report):
    with pytest.raises(G.GuardError) as e:
        G.run_twice(_stage(defect), SPEC)
    assert report in str(e.value), str(e.value)


def test_unspecified_padding_is_not_compared():
    spec = {"cout": G.Out(valid=np.s_[:, :, :D], pad=G.UNSPECIFIED, finite=True)}
    G.run_twice(_stage("padding unwritten"), spec)
    with pytest.raises(G.GuardError):
        G.run_twice(_stage("unwritten"), spec)


def test_specified_padding_value_is_checked():
    def fn(arena):
        out = _stage()(arena)["cout"]
        out[1, 1, D] = 3.0  # written, the same in both runs, but not the specified zero
        return {"cout": out}

    with pytest.raises(G.GuardError) as e:
        G.run_twice(fn, SPEC)
    assert "specified padding is not 0: " + _elem(1, 1, D) in str(e.value)


@pytest.mark.parametrize("shape,dtype,row", [((3, 5, 64), torch.float32, None), ((1, 1), torch.uint8, None),
                                             ((7, 300, 32), torch.int16, 300 * 32 * 2), ((0,), torch.uint8, None),
                                             ((4097,), torch.uint8, None), ((2, 3, 5), torch.int64, None)])
def test_allocation_layout(shape, dtype, row):
    arena = G.Arena("cpu", 0x5A)
    t = arena.out("t", shape, dtype, row_bytes=row)
    b = arena.find(t) if t.numel() else arena.buffers[0]
    assert t.data_ptr() % 256 == 0 and t.is_contiguous() and tuple(t.shape) == shape and t.dtype == dtype
    rowb = row if row is not None else int(np.prod(shape[1:])) * t.element_size() if len(shape) > 1 else 0
    assert b.guard >= max(4096, rowb)
    assert b.off >= b.guard and b.off + b.nbytes + b.guard <= b.base.numel()  # both bands inside the allocation
    assert (b.base[b.off:b.off + b.nbytes] == 0x5A).all()
    assert (b.base[:b.off] == 0xA5).all() and (b.base[b.off + b.nbytes:b.off + b.nbytes + b.guard] == 0xA5).all()
    assert arena.damaged() == []


def test_poison_values():
    arena = G.Arena("cpu", 0xFF)
    assert torch.isnan(arena.out("f", (4,), torch.float32)).all()
    assert (arena.out("i", (4,), torch.int32) == -1).all() and (arena.out("b", (4,), torch.uint8) == 255).all()
    arena = G.Arena("cpu", 0x5A)
    f = arena.out("f", (4,), torch.float32)
    assert torch.isfinite(f).all() and (f > 1e16).all()


@pytest.mark.parametrize("fill,dtype,bad", [(G.NAN, np.float32, np.isnan), (G.NEG_INF, np.float32, np.isneginf),
                                           (G.U16_MAX, np.uint16, lambda a: a == 0xFFFF)])
def test_put_fills_padding_and_guards(fill, dtype, bad):
    arena = G.Arena("cpu")
    a = np.arange(H * W * DP).reshape(H, W, DP).astype(dtype)
    if dtype == np.uint16:
        a = a.view(np.int16)  # torch has no uint16 arithmetic: int16 storage, as the library uses
    t = arena.put("cin", a, fill=fill, valid=np.s_[:, :, :D])
    got = t.numpy().view(dtype)
    assert np.array_equal(got[:, :, :D], a.view(dtype)[:, :, :D]) and bad(got[:, :, D:]).all()
    b = arena.find(t)
    for _, region, _ in b.sides():
        assert bad(region.numpy().view(dtype)).all()
    assert arena.damaged() == []
    b.base[b.off + b.nbytes + 6] ^= 1  # the guard right after the body
    assert arena.damaged() == [("cin", "back", b.nbytes + 6, 1)]


def test_put_keeps_specified_padding():
    """Support arrays keep their zero padding taps: no fill, plain guards."""
    arena = G.Arena("cpu")
    w = np.zeros((2, 3, 8), np.float32)
    w[:, :, :5] = 1
    t = arena.put("w", w)
    assert np.array_equal(t.numpy(), w) and arena.find(t).pattern == G.GUARD


def test_proxy_hands_out_guarded_poisoned_allocations():
    arena = G.Arena("cpu", 0xFF)
    proxy = G.TorchProxy(torch, arena)
    e = proxy.empty((3, 5), dtype=torch.float32, device="cpu")
    e1 = proxy.empty(7, dtype=torch.uint8, device=torch.device("cpu"))
    el = proxy.empty_like(e)
    z = proxy.zeros((2, 2, 4), dtype=torch.uint8, device="cpu")
    f = proxy.full((2, 3), -1, dtype=torch.int16, device="cpu")
    assert [arena.find(t) is not None for t in (e, e1, el, z, f)] == [True] * 5
    assert torch.isnan(e).all() and (e1 == 255).all() and torch.isnan(el).all() and el.shape == e.shape
    assert (z == 0).all() and (f == -1).all()
    assert proxy.float32 is torch.float32 and proxy.Tensor is torch.Tensor and proxy.cuda is torch.cuda
    arena.verify()
    b = arena.find(f)
    b.base[b.off - 1] = 0
    with pytest.raises(G.GuardError) as err:
        arena.verify()
    assert f"guard of '{b.name}' damaged: front guard, first at byte offset -1 " in str(err.value)


def test_fixture_patches_library_and_verifies_on_teardown(guarded_kernels):
    import stereo_matchin_amd.kernels as K
    import stereo_matchin_amd.pipeline as P
    assert isinstance(K.torch, G.TorchProxy) and isinstance(P.torch, G.TorchProxy)
    assert K.torch.arena is guarded_kernels and P.torch.arena is guarded_kernels
    t = K.torch.empty((2, 3), dtype=torch.int32, device="cpu")
    assert (t == -1).all() and guarded_kernels.find(t) is not None


def test_fixture_is_undone():
    import stereo_matchin_amd.kernels as K
    import stereo_matchin_amd.pipeline as P
    assert K.torch is torch and P.torch is torch
