"""The catalogue of 64-lane pass forms against the GPU matrix's case list (no GPU).

tests/test_gpu_pass_forms.py asserts on the device that every launch ran the form its case
names; this module proves that those names are every name the dispatch can produce.
"""
from collections import Counter

import pass_forms as PF
import test_gpu_pass_forms as M


def test_catalogue_size_and_no_duplicates():
    assert len(set(PF.CATALOGUE)) == len(PF.CATALOGUE) == 202
    per_kernel = Counter(name.split("<")[0] for name in PF.CATALOGUE)
    assert per_kernel == {"k_vpass10": 51, "k_vpass10_c16": 34, "k_hpass11": 69, "k_hpass9": 48}


def test_every_case_maps_to_a_catalogue_entry():
    ids = [M.case_id(c) for c in M.CASES]
    assert len(set(ids)) == len(ids)
    for c in M.CASES:
        assert c.T in PF.RING_TAPS and PF.pitch(c.d0, c.d1, c.D) >= 64, c
        assert c.modes == ((PF.DEN_NONE, PF.DEN_WRITE) if c.c16 else (PF.DEN_NONE, PF.DEN_WRITE, PF.DEN_READ)), c
        for name in M.case_names(c):
            assert name in PF.CATALOGUE, (c, name)


def test_the_cases_run_the_whole_catalogue():
    """Nothing left out, nothing besides: the union over the case list is the catalogue."""
    ran = {name for c in M.CASES for name in M.case_names(c)}
    assert ran == set(PF.CATALOGUE), (sorted(set(PF.CATALOGUE) - ran), sorted(ran - set(PF.CATALOGUE)))


def test_every_family_runs_every_tap_count():
    for family in ("v", "v16", "h11", "h9"):
        for v in {c.variant for c in M.CASES if c.family == family}:
            taps = {c.T for c in M.CASES if c.family == family and c.variant == v}
            assert taps == set(PF.RING_TAPS), (family, v)


def test_names_at_the_dispatch_thresholds():
    """The restated dispatch against names written out by hand."""
    e = PF.expected_name
    # exactly 8192 H waves: k_hpass11; one row less: k_hpass9 (16 MB volumes: not nt)
    assert [e(8, 8192, 0, 64, 64, 7, 1, m, False, 0) for m in (0, 1, 2)] == \
        [f"k_hpass11<T=7,NKW=1,DM={m},nt>" for m in (0, 1, 2)]
    assert e(8, 8191, 0, 64, 64, 7, 1, 2, False, 0) == "k_hpass9<T=7,NW=4,DM=2>"
    # exactly 2^28 bytes: nt; one row less: not
    assert e(512, 512, 0, 256, 256, 9, 0, 1, False, 0) == "k_vpass10<T=9,NW=16,DM=1,nt>"
    assert e(512, 511, 0, 256, 256, 9, 0, 1, False, 0) == "k_vpass10<T=9,NW=16,DM=1>"
    assert e(512, 512, 0, 256, 256, 9, 1, 0, False, 0) == "k_hpass9<T=9,NW=4,DM=0,nt>"
    # past 256 MiB and under 8192 waves
    assert e(224, 1200, 0, 256, 256, 3, 1, 2, False, 0) == "k_hpass9<T=3,NW=4,DM=2,nt>"
    assert e(224, 1200, 0, 256, 256, 3, 0, 0, False, 0) == "k_vpass10<T=3,NW=16,DM=0,nt>"
    assert e(224, 1200, 0, 256, 256, 51, 0, 2, False, 0) == "k_vpass10<T=51,NW=12,NPH=3,DM=2,nt>"
    # the flagship frames (asserted on the device by tests/test_gpu_parity.py)
    assert e(1920, 1080, 0, 256, 256, 35, 0, 1, True, 0) == "k_vpass10_c16<T=35,NW=16,DM=1,nt>"
    assert e(1920, 1080, 0, 256, 256, 35, 1, 2, False, 0) == "k_hpass11<T=35,NKW=4,DM=2,nt>"
    assert e(3840, 270, 0, 512, 512, 51, 0, 2, False, 0) == "k_vpass10<T=51,NW=12,NPH=3,TK=4,DM=2,nt>"
    assert e(3840, 270, 0, 512, 512, 51, 1, 2, False, 0) == "k_hpass11<T=51,NKW=2,PX=24,DM=2,nt>"
    assert e(3840, 270, 0, 512, 512, 51, 1, 1, False, 0) == "k_hpass11<T=51,NKW=2,DM=1,nt>"
    # bit 26 flips V and k_hpass9, never k_hpass11
    assert e(37, 25, 0, 70, 70, 3, 0, 0, False, PF.BIT_NT_FLIP) == "k_vpass10<T=3,NW=16,DM=0,nt>"
    assert e(1920, 1080, 0, 256, 256, 35, 0, 2, False, PF.BIT_NT_FLIP) == "k_vpass10<T=35,NW=16,DM=2>"
    assert e(331, 9, 0, 256, 256, 15, 1, 0, False, 128 | PF.BIT_NT_FLIP) == "k_hpass9<T=15,NW=4,DM=0,nt>"
    assert e(530, 7, 0, 256, 256, 15, 1, 0, False, 4096 | PF.BIT_NT_FLIP) == "k_hpass11<T=15,NKW=4,DM=0,nt>"


def test_the_shapes_reach_the_paths_they_are_there_for():
    """What the case list's comments claim about its shapes, from the launch geometry."""
    for c in M.CASES:
        Dp = PF.pitch(c.d0, c.d1, c.D)
        if c.family in ("v", "v16") and c.H > 3:
            U, la = PF.period(c.T), PF.v_lookahead(c.T)
            rows, nstrip = PF.v_strips(c.W, c.H, Dp, c.T)
            assert nstrip >= 2 and c.H % U != 0, c                  # several strips, a partial last chunk
            assert U <= rows and U + la <= c.H, c                   # an unclamped whole chunk
            assert c.W % 16 and c.W % 12, c
        if c.family == "h11":
            assert PF.h11_selected(c.W, c.H, Dp, c.T, c.variant) and not PF.h11_selected(c.W, c.H, Dp, c.T, 0), c
    # the TK = 4 tile order: a partial tile in both axes
    H, W, D = M.TILE_SHAPES[0][:3]
    per_xcd, nkb = PF.ceil_div(PF.ceil_div(W, 12), 8), PF.pitch(0, D, D) // 64
    assert PF.v12_tiles(W, D) and per_xcd % 8 and per_xcd > 8 and nkb % 4 and nkb > 4
    assert PF.v_strips(M.TILE_SHAPES[1][1], M.TILE_SHAPES[1][0], 256, 51)[1] == 2
    # the segment override at T = 51 den-read: segments that are no whole number of 80-step periods
    assert {PF.h11_seg_len(51, c.variant) % (PF.period(51) + 24) for c in M.CASES if c.family == "h11-seg"
            and c.T == 51} == {56 % 80, 112 % 80}
    # the large shapes: 2^28 bytes exactly, one row less, and past it under 8192 H waves
    sizes = sorted({(c.W * c.H * c.D * 4, c.H) for c in M.LARGE_CASES})
    assert sizes[0][0] < 1 << 28 and sizes[1][0] == 1 << 28 and sizes[2][0] > 1 << 28
    for c in M.LARGE_CASES:
        assert not PF.h11_selected(c.W, c.H, c.D, c.T, 0) and len(M.large_bands(c)) >= 3
