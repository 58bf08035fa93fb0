"""The compiled forms of the 64-lane aggregation passes, restated in Python (no GPU).

`expected_name` says which instantiation `asw_aggregate_pass_den` / `_den16` must run for a
shape, a tap count and a tuning variant, as the string `asw_pass_kernel` reports; `CATALOGUE`
is every such string the dispatch can produce.  Both are written from the dispatch rules
(launch_pass_t / launch_dm in csrc), not read from the library: tests/test_pass_forms.py holds
the GPU matrix (tests/test_gpu_pass_forms.py) against them, so a form that is compiled and
never run, or a case that runs another form than it says, fails on the CPU.
"""

RING_TAPS = (3, 5, 7, 9, 15, 33, 35, 51)  # the tap counts with ring kernels (any other odd T: k_pass_any)
DIR_V, DIR_H = 0, 1
DEN_NONE, DEN_WRITE, DEN_READ = 0, 1, 2

BIT_H9 = 128          # H by k_hpass9 at any frame size
BIT_H11 = 4096        # H by k_hpass11 at any frame size
SEG_SHIFT = 8         # bits 8..11: k_hpass11's segment length in window periods
BIT_NT_FLIP = 1 << 26  # the other cache policy (k_hpass11 is nt in both)

STREAM_BYTES = 256 << 20  # volumes from here on stream nt
H11_WAVES = 8192          # H grids from here on run k_hpass11


def ceil_div(a, b):
    return -(-a // b)


def pitch(d_begin, d_end, D):
    """Planes per pixel of the device volume: whole 64-plane blocks, 32 for a shard of <= 32 planes."""
    n = d_end - d_begin
    if n <= 32 and (d_begin > 0 or d_end < D):
        return 32
    return ceil_div(n, 64) * 64


def period(T):
    """The window period U: the smallest multiple of 4 from T + 3 on."""
    return ceil_div(T + 3, 4) * 4


def h11_seg_len(T, variant):
    """Columns per k_hpass11 sweep: the multiple of U nearest 240, or the variant's count of periods."""
    U = period(T)
    n = (variant >> SEG_SHIFT) & 15
    return (n if n else (240 + U // 2) // U) * U


def streams(W, H, Dp, variant):
    nt = W * H * Dp * 4 >= STREAM_BYTES
    return nt != bool(variant & BIT_NT_FLIP)


def v12_tiles(W, Dp):
    """T = 51, nt: the 12-column blocks in XCD-round tiles of 4 plane blocks x 8 column groups."""
    return Dp // 64 >= 4 and ceil_div(ceil_div(W, 12), 8) >= 8


def h11_selected(W, H, Dp, T, variant):
    waves = H * ceil_div(W, h11_seg_len(T, variant)) * (Dp // 64)
    return not variant & BIT_H9 and (waves >= H11_WAVES or bool(variant & BIT_H11))


def _name(kernel, T, shape, den_mode, nt):
    return f"{kernel}<T={T},{shape},DM={den_mode}{',nt' if nt else ''}>"


def expected_name(W, H, d_begin, d_end, D, T, direction, den_mode, c16, variant):
    """The instantiation a pass over this (shard of a) W x H x D problem runs."""
    if T not in RING_TAPS:
        raise ValueError(f"T = {T} has no ring kernel")
    Dp = pitch(d_begin, d_end, D)
    if Dp == 32:
        raise ValueError("a 32-plane shard runs the half-wave passes, not these")
    if den_mode not in (DEN_NONE, DEN_WRITE, DEN_READ):
        raise ValueError(den_mode)
    if c16 and (direction != DIR_V or den_mode == DEN_READ):
        raise ValueError("the uint16 form is the first V pass: den-none or den-write")
    nt = streams(W, H, Dp, variant)
    nkb = Dp // 64
    if direction == DIR_V:
        kernel = "k_vpass10_c16" if c16 else "k_vpass10"
        if T <= 35:
            shape = "NW=16"
        elif nt and v12_tiles(W, Dp):
            shape = "NW=12,NPH=3,TK=4"
        else:
            shape = "NW=12,NPH=3"
        return _name(kernel, T, shape, den_mode, nt)
    if not h11_selected(W, H, Dp, T, variant):
        return _name("k_hpass9", T, "NW=4", den_mode, nt)
    if T <= 35:
        nkw = 4 if nkb % 4 == 0 else 2 if nkb % 2 == 0 else 1
    else:
        nkw = 2 if nkb % 2 == 0 else 1
    shape = f"NKW={nkw}"
    if T == 51 and den_mode == DEN_READ and nkw == 2:
        shape += ",PX=24"
    return _name("k_hpass11", T, shape, den_mode, True)


def _catalogue():
    names = []
    for T in RING_TAPS:
        # V: 16 columns up to T = 35 in both policies; 12 columns in 3 phases past it, cached,
        # nt and nt in tiles
        v_forms = [("NW=16", False), ("NW=16", True)] if T <= 35 else \
            [("NW=12,NPH=3", False), ("NW=12,NPH=3", True), ("NW=12,NPH=3,TK=4", True)]
        for shape, nt in v_forms:
            names += [_name("k_vpass10", T, shape, dm, nt) for dm in (DEN_NONE, DEN_WRITE, DEN_READ)]
            names += [_name("k_vpass10_c16", T, shape, dm, nt) for dm in (DEN_NONE, DEN_WRITE)]
        for dm in (DEN_NONE, DEN_WRITE, DEN_READ):
            # H rings: 4, 2 or 1 plane blocks per block up to T = 35, 2 or 1 past it (den-read: PX = 24)
            if T <= 35:
                h_forms = ["NKW=4", "NKW=2", "NKW=1"]
            else:
                h_forms = ["NKW=2,PX=24" if dm == DEN_READ else "NKW=2", "NKW=1"]
            names += [_name("k_hpass11", T, shape, dm, True) for shape in h_forms]
            names += [_name("k_hpass9", T, "NW=4", dm, nt) for nt in (False, True)]
    return tuple(names)


CATALOGUE = _catalogue()


def v_strips(W, H, Dp, T):
    """(rows per strip, strips) of the V pass's grid: enough blocks to fill the CUs several
    times, strips of whole U-row chunks and at least 2T rows."""
    U = period(T)
    blocks = ceil_div(W, 16 if T <= 35 else 12) * (Dp // 64)
    nstrip = max(1, min(ceil_div(2048, blocks), max(1, H // (2 * T))))
    rows = ceil_div(ceil_div(H, nstrip), U) * U
    return rows, ceil_div(H, rows)


def v_lookahead(T):
    """Rows past its own that a V step touches (the window's newest row; staging 3 + 4 rows ahead)."""
    return max(T // 2 + period(T) - T, 7)
