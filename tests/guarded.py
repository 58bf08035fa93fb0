"""Guard-banded, poisoned buffers for the stage kernels (CPU and device tensors).

A value test cannot see memory: a kernel that writes past its output, leaves a valid
element unwritten, or lets the previous contents of its output or an input's padding
plane reach a result.  This module is the device-side memory check the project has:

* :meth:`Arena.alloc` returns a contiguous tensor that is the 256-byte aligned middle
  of a larger uint8 allocation.  On each side lies a guard band of at least
  ``max(4 KiB, one image row of the buffer)`` filled with a fixed pattern, so an overrun
  of up to a row lands in memory the arena owns and :meth:`Arena.damage` reports the
  first damaged byte relative to the body and its side.
* Output bodies are pre-filled with a poison byte: 0xFF (float NaN, integer -1, 255) or
  0x5A (a large finite float, 1.5e16).  In-place buffers are guarded, not poisoned.
* :func:`run_twice` runs a stage once under each poison and asserts that every guard is
  intact and that each output's valid region (and its padding, where specified) is
  byte-identical in both runs: every such element was written and none depends on what
  the buffer held before.
* :meth:`Arena.put` places a numpy array in a guarded buffer with a chosen fill of its
  padding region and of its guards (NAN where the consumer does arithmetic, NEG_INF
  where it takes a minimum, U16_MAX for uint16 volumes).
* the ``guarded_kernels`` fixture makes every ``torch.empty / empty_like / zeros / full``
  of ``stereo_matchin_amd.kernels`` and ``.pipeline`` a guarded allocation for one test.
"""
from __future__ import annotations

import math
import struct

import numpy as np
import pytest

ALIGN = 256
MIN_GUARD = 4096
GUARD = b"\xa5"  # guard bytes of outputs and in-place buffers
POISONS = (0xFF, 0x5A)
NAN = struct.pack("<f", float("nan"))
NEG_INF = struct.pack("<f", float("-inf"))
U16_MAX = b"\xff\xff"
UNSPECIFIED = object()  # an output's padding that the entry point does not define

_BITS = {1: "uint8", 2: "int16", 4: "int32", 8: "int64"}


class GuardError(AssertionError):
    pass


def _torch():
    import torch
    return torch


def _pattern(pattern: bytes, device):
    torch = _torch()
    return torch.tensor(list(pattern), dtype=torch.uint8, device=device)


def _fill(region, pattern: bytes):
    """region: 1-D uint8, a multiple of len(pattern) long."""
    if len(pattern) == 1:
        region.fill_(pattern[0])
    elif region.numel():
        region.view(-1, len(pattern)).copy_(_pattern(pattern, region.device).expand(region.numel() // len(pattern), -1))


def _bits(t):
    """The elements of t as integers of the same width: exact comparisons, NaN included."""
    torch = _torch()
    return t.view(getattr(torch, _BITS[t.element_size()]))


class Buffer:
    """One guarded allocation: ``body`` is base[off : off + nbytes] viewed as (shape, dtype)."""

    def __init__(self, name, base, off, nbytes, guard, pattern, body):
        self.name, self.base, self.off, self.nbytes, self.guard, self.pattern, self.body = \
            name, base, off, nbytes, guard, pattern, body

    def sides(self):
        end = self.off + self.nbytes
        return (("front", self.base[self.off - self.guard:self.off], -self.guard),
                ("back", self.base[end:end + self.guard], self.nbytes))

    def bad(self, region):
        """bool [n]: guard bytes that no longer hold the pattern."""
        L = len(self.pattern)
        return (region.view(-1, L) != _pattern(self.pattern, region.device)).view(-1)

    def damage(self):
        """None, or (side, byte offset relative to the body's first byte, damaged bytes) of the
        first damaged guard byte: negative in the front guard, >= nbytes in the back guard."""
        for side, region, rel in self.sides():
            bad = self.bad(region)
            n = int(bad.sum())
            if n:
                return side, rel + int(bad.to(_torch().uint8).argmax()), n
        return None


class Arena:
    """Hands out guarded buffers on one device and verifies their guards."""

    def __init__(self, device="cpu", poison: int | None = POISONS[0]):
        self.device = device
        self.poison = poison
        self.buffers: list[Buffer] = []

    # -- allocation
    def alloc(self, name, shape, dtype, row_bytes: int | None = None, pattern: bytes = GUARD,
              poison: int | None = None, device=None):
        """A guarded tensor.  row_bytes: bytes of one image row of the buffer (W * pitch *
        itemsize); by default everything below the first axis.  poison: a byte to pre-fill
        the body with, or None to leave the body as allocated (fill it yourself)."""
        torch = _torch()
        shape = (int(shape),) if isinstance(shape, (int, np.integer)) else tuple(int(s) for s in shape)
        item = torch.empty((), dtype=dtype).element_size()
        nbytes = math.prod(shape) * item
        if row_bytes is None:
            row_bytes = math.prod(shape[1:]) * item if len(shape) > 1 else 0
        guard = -(-max(MIN_GUARD, int(row_bytes)) // ALIGN) * ALIGN
        assert guard % len(pattern) == 0 and nbytes % len(pattern) == 0, (name, pattern)
        base = torch.empty(2 * guard + nbytes + ALIGN, dtype=torch.uint8, device=device or self.device)
        off = guard + (-(base.data_ptr() + guard)) % ALIGN
        body = base[off:off + nbytes].view(dtype).view(shape)
        assert body.data_ptr() % ALIGN == 0 and body.is_contiguous()
        _fill(base[:off], pattern)
        _fill(base[off + nbytes:off + nbytes + guard], pattern)
        if poison is not None:
            base[off:off + nbytes].fill_(poison)
        buf = Buffer(name or f"#{len(self.buffers)}", base, off, nbytes, guard, pattern, body)
        self.buffers.append(buf)
        return body

    def out(self, name, shape, dtype, row_bytes=None):
        """An output: guarded and poisoned with the arena's byte."""
        return self.alloc(name, shape, dtype, row_bytes, poison=self.poison)

    def put(self, name, array, fill: bytes | None = None, valid=None, row_bytes=None):
        """An input or in-place buffer holding ``array`` (numpy).  ``fill`` (NAN, NEG_INF,
        U16_MAX, ...) is written to the guards and, where ``valid`` (an index expression)
        is given, over every element outside ``array[valid]``: the padding the consumer
        must not let reach a result.  fill None: plain guards, the array as it is."""
        torch = _torch()
        a = np.ascontiguousarray(array)
        src = torch.from_numpy(a)
        body = self.alloc(name, a.shape, src.dtype, row_bytes, pattern=fill or GUARD)
        if valid is not None and fill is not None:
            assert a.dtype.itemsize == len(fill), (name, a.dtype, fill)
            a = a.copy()
            pad = np.ones(a.shape, bool)
            pad[valid] = False
            a[pad] = np.frombuffer(fill, a.dtype)[0]
            src = torch.from_numpy(a)
        body.copy_(src)
        return body

    # -- verification
    def find(self, tensor) -> Buffer | None:
        for b in self.buffers:
            if b.body.data_ptr() == tensor.data_ptr() and b.body.shape == tensor.shape:
                return b
        return None

    def damaged(self):
        """[(name, side, offset, nbytes damaged)] of every buffer with a damaged guard."""
        torch = _torch()
        if not self.buffers:
            return []
        flags = {}
        for b in self.buffers:
            flags.setdefault(b.base.device, []).extend(b.bad(r).any() for _, r, _ in b.sides())
        if not any(bool(torch.stack(f).any()) for f in flags.values()):  # one synchronisation per device
            return []
        return [(b.name,) + d for b in self.buffers for d in (b.damage(),) if d]

    def verify(self):
        bad = self.damaged()
        if bad:
            raise GuardError("; ".join(
                f"guard of '{n}' damaged: {side} guard, first at byte offset {off} relative to the body "
                f"({cnt} bytes)" for n, side, off, cnt in bad))

    def release(self):
        self.buffers.clear()


class Out:
    """How run_twice checks one output: ``valid`` is an index expression of the region the
    stage defines (default: everything); ``pad`` the value of every other element, or
    UNSPECIFIED; ``finite``: the valid region holds no NaN / inf (a float output whose
    inputs' padding and guards are NaN or -inf: a non-finite value came from there)."""

    def __init__(self, valid=None, pad=UNSPECIFIED, finite=False):
        self.valid, self.pad, self.finite = valid, pad, finite


def _first(mask):
    """(flat index, unravelled index, count) of the first True element."""
    flat = int(mask.reshape(-1).to(_torch().uint8).argmax())
    return flat, tuple(int(i) for i in np.unravel_index(flat, tuple(mask.shape))), int(mask.sum())


def _where(name, t, mask):
    flat, idx, n = _first(mask)
    return f"'{name}' element {idx} (byte offset {flat * t.element_size()}, {n} elements)"


def check_outputs(runs, specs=None):
    """runs: [(arena, {name: tensor})] of the same stage under different poisons."""
    torch = _torch()
    specs = specs or {}
    for arena, _ in runs:
        arena.verify()
    (_, first), rest = runs[0], runs[1:]
    for name, a in first.items():
        if a is None:
            continue
        spec = specs.get(name) or Out()
        valid = torch.ones(a.shape, dtype=torch.bool, device=a.device)
        if spec.valid is not None:
            valid.zero_()
            valid[spec.valid] = True
        for _, other in rest:
            b = other[name]
            diff = _bits(a) != _bits(b)
            if bool((diff & valid).any()):
                raise GuardError("valid region depends on the previous contents (unwritten, or computed "
                                 "from them): " + _where(name, a, diff & valid))
            if spec.pad is not UNSPECIFIED and bool((diff & ~valid).any()):
                raise GuardError("specified padding depends on the previous contents (unwritten): "
                                 + _where(name, a, diff & ~valid))
        if spec.pad is not UNSPECIFIED:
            for _, res in runs:
                wrong = (res[name] != spec.pad) & ~valid
                if bool(wrong.any()):
                    raise GuardError(f"specified padding is not {spec.pad}: " + _where(name, a, wrong))
        if spec.finite:
            for _, res in runs:
                wrong = ~torch.isfinite(res[name]) & valid
                if bool(wrong.any()):
                    raise GuardError("valid region is not finite (computed from an input's padding, its guard "
                                     "or the poison): " + _where(name, a, wrong))


def run_twice(fn, specs=None, device="cpu"):
    """Run ``fn(arena) -> {name: output tensor}`` once under each poison, every input placed
    with arena.put and every output allocated with arena.out (or by the library under
    :func:`patched`), then check guards and outputs (:func:`check_outputs`).  Returns
    the two result dicts."""
    runs = []
    for poison in POISONS:
        arena = Arena(device, poison)
        runs.append((arena, fn(arena)))
    if str(device) != "cpu":
        _torch().cuda.synchronize()
    check_outputs(runs, specs)
    return [r for _, r in runs]


# ------------------------------------------------------------------ the torch proxy

class TorchProxy:
    """``torch`` with guarded ``empty / empty_like / zeros / full``; all else is forwarded."""

    def __init__(self, real, arena: Arena):
        self._real, self.arena = real, arena

    def __getattr__(self, name):
        return getattr(self._real, name)

    def _new(self, size, dtype, device, kw, poison):
        if kw or (len(size) == 1 and isinstance(size[0], self._real.Tensor)):
            return None  # a form this proxy does not know: the plain allocation
        if len(size) == 1 and not isinstance(size[0], (int, np.integer)):
            size = tuple(size[0])
        dtype = dtype or self._real.get_default_dtype()
        return self.arena.alloc(None, size, dtype, poison=poison, device=device or "cpu")

    def empty(self, *size, dtype=None, device=None, **kw):
        t = self._new(size, dtype, device, kw, self.arena.poison)
        return self._real.empty(*size, dtype=dtype, device=device, **kw) if t is None else t

    def empty_like(self, t, **kw):
        if kw or not t.is_contiguous():
            return self._real.empty_like(t, **kw)
        return self.arena.alloc(None, t.shape, t.dtype, poison=self.arena.poison, device=t.device)

    def zeros(self, *size, dtype=None, device=None, **kw):
        t = self._new(size, dtype, device, kw, None)
        return self._real.zeros(*size, dtype=dtype, device=device, **kw) if t is None else t.zero_()

    def full(self, size, fill_value, dtype=None, device=None, **kw):
        if dtype is None:
            return self._real.full(size, fill_value, device=device, **kw)
        t = self._new((size,), dtype, device, kw, None)
        return self._real.full(size, fill_value, dtype=dtype, device=device, **kw) if t is None \
            else t.fill_(fill_value)


class patched:
    """Context manager: the ``torch`` of stereo_matchin_amd.kernels and .pipeline allocates
    from ``arena`` (what the guarded_kernels fixture does for a whole test)."""

    def __init__(self, arena: Arena):
        self.arena = arena

    def __enter__(self):
        import stereo_matchin_amd.kernels as K
        import stereo_matchin_amd.pipeline as P
        self.saved = [(m, m.torch) for m in (K, P)]
        for m, real in self.saved:
            m.torch = TorchProxy(real, self.arena)
        return self.arena

    def __exit__(self, *exc):
        for m, real in self.saved:
            m.torch = real
        return False


@pytest.fixture
def guarded_kernels():
    """Every output the library wrappers allocate in this test is guarded and poisoned
    (0xFF); every guard handed out is verified on teardown."""
    arena = Arena("cpu", POISONS[0])
    with patched(arena):
        yield arena
    try:
        arena.verify()
    finally:
        arena.release()
