"""Numpy restatement of the WTA stage functions (include/asw.h: asw_wta_local /
_target_local / _second / _finalize and their penalised asw_wta_ref_* forms), the
whole-volume forms they must add up to, and the crafted inputs of
tests/test_wta_shard_ref.py, tests/test_distributed.py and tests/test_gpu_wta_shard.py.

The rules are the reference's (K/asw_wta.cl:12-82, K/asw_wta_ref.cl:2-68):
a sequential strict-< scan that keeps the first minimum and the second smallest value of
the multiset; the target scan over i = 0..md-1 of C[md + max(x-i, 0) - x][y][max(x-i, 0)].
The penalised forms scan (0.085f*den) * |val - (float)i| + c, every operation a float32 one
(numpy's are correctly rounded and never fused), i being the global plane index in the
own scan and the scan index in the target scan.  tests/test_wta_shard_ref.py pins all of
it to the C oracle (oracle_wta, oracle_wta_ref) bit for bit.
"""
import functools

import numpy as np
import torch

from stereo_matchin_amd.distributed import shard_range

INIT = np.float32(100000.0)  # K/asw_wta.cl:25-26
NOKEY = np.int64(0x7FFFFFFFFFFFFFFF)
ALPHA = np.float32(0.085)  # K/asw_wta_ref.cl:28


def _key(v: np.ndarray, idx: np.ndarray) -> np.ndarray:
    bits = v.astype(np.float32).view(np.uint32).astype(np.uint64)
    return ((bits << np.uint64(32)) | idx.astype(np.uint64)).astype(np.int64)


def _top2(cands: np.ndarray, ids: np.ndarray):
    """Sequential strict-< scan of K/asw_wta.cl:25-47 over the last axis."""
    m1 = np.full(cands.shape[:-1], INIT, np.float32)
    m2 = np.full(cands.shape[:-1], INIT, np.float32)
    idx = np.full(cands.shape[:-1], -1, np.int64)
    for j in range(cands.shape[-1]):
        t = cands[..., j]
        ok = ~np.isnan(t)
        lt2 = ok & (t < m2)
        m2 = np.where(lt2, t, m2)
        lt1 = ok & (t < m1)
        m2 = np.where(lt1, m1, m2)
        idx = np.where(lt1, ids[..., j], idx)
        m1 = np.where(lt1, t, m1)
    return m1, m2, idx


class CpuShardOps:
    """CPU restatement of the per-shard stage functions (test infrastructure)."""

    def __init__(self, d_begin: int, d_end: int, D: int):
        self.b, self.e, self.D = d_begin, d_end, D

    def local(self, cost):  # cost: [H][W][n] local planes, pixel-major like the product
        c = cost.numpy()
        ids = np.broadcast_to(np.arange(self.b, self.e), c.shape)
        m1, m2, idx = _top2(c, ids)
        key = np.where(idx < 0, NOKEY, _key(m1, np.maximum(idx, 0)))
        return torch.from_numpy(key), torch.from_numpy(m1), torch.from_numpy(m2)

    def target_local(self, cost, key_ref):
        c = cost.numpy()
        H, W, _ = c.shape
        kr = key_ref.numpy()
        md = np.where(kr == NOKEY, 0, kr & 0xFFFFFFFF).astype(np.int64)
        x = np.broadcast_to(np.arange(W), (H, W))
        y = np.broadcast_to(np.arange(H)[:, None], (H, W))
        Dmax = self.D
        i = np.arange(Dmax)
        xq = np.maximum(x[..., None] - i, 0)
        b = md[..., None] + xq - x[..., None]
        valid = (i < md[..., None]) & (b >= self.b) & (b < self.e)
        cand = np.full((H, W, Dmax), np.nan, np.float32)
        yy = np.broadcast_to(y[..., None], cand.shape)
        cand[valid] = c[yy[valid], xq[valid], (b - self.b)[valid]]
        m1, m2, idx = _top2(cand, np.broadcast_to(i, cand.shape))
        tkey = np.where(idx < 0, NOKEY, _key(m1, np.maximum(idx, 0)))
        return torch.from_numpy(tkey), torch.from_numpy(m1), torch.from_numpy(m2)

    def second(self, key_g, key_l, m1, m2):
        return torch.where(key_l == key_g, m2, m1)

    def finalize(self, key, m2, tkey, t2):
        k, tk = key.numpy(), tkey.numpy()
        H, W = k.shape
        x = np.broadcast_to(np.arange(W), (H, W))
        md = np.where(k == NOKEY, 0, k & 0xFFFFFFFF).astype(np.int32)
        m1 = np.where(k == NOKEY, INIT, (k.astype(np.uint64) >> np.uint64(32)).astype(np.uint32).view(np.float32))
        ti = (tk & 0xFFFFFFFF).astype(np.int64)
        mdr = np.where(tk == NOKEY, md, md + np.maximum(x - ti, 0) - x).astype(np.int32)
        tm1 = np.where(tk == NOKEY, INIT,
                       (tk.astype(np.uint64) >> np.uint64(32)).astype(np.uint32).view(np.float32))
        with np.errstate(invalid="ignore", divide="ignore"):
            conf_ref = (m2.numpy() - m1) / m2.numpy()
            conf_tar = (t2.numpy() - tm1) / t2.numpy()
        return md, conf_ref.astype(np.float32), mdr, conf_tar.astype(np.float32)


def penalty(den, val, i, c):
    """(0.085f*den) * |val - (float)i| + c in float32 steps (penalty() of asw_refine.hip,
    the oracle's policy REF_POL = 0).  NaN candidates (planes not scanned) stay NaN."""
    a = ALPHA * np.asarray(den, np.float32)
    b = np.abs(np.asarray(val, np.float32) - np.asarray(i).astype(np.float32))
    out = a * b + np.asarray(c, np.float32)
    assert out.dtype == np.float32
    return out


class CpuRefShardOps(CpuShardOps):
    """The penalised stage functions (asw_wta_ref_local / _target_local / _finalize) of one
    shard; ref_l / ref_r: [2][H][W] float32 (value plane, den plane) of each view."""

    def __init__(self, d_begin: int, d_end: int, D: int, ref_l: np.ndarray, ref_r: np.ndarray):
        super().__init__(d_begin, d_end, D)
        self.ref_l, self.ref_r = ref_l, ref_r

    def ref_local(self, cost):
        c = cost.numpy()
        ids = np.broadcast_to(np.arange(self.b, self.e), c.shape)
        pen = penalty(self.ref_l[1][..., None], self.ref_l[0][..., None], ids, c)
        m1, m2, idx = _top2(pen, ids)
        key = np.where(idx < 0, NOKEY, _key(m1, np.maximum(idx, 0)))
        return torch.from_numpy(key), torch.from_numpy(m1), torch.from_numpy(m2)

    def ref_target_local(self, cost, key_ref):
        c = cost.numpy()
        H, W, _ = c.shape
        kr = key_ref.numpy()
        md = np.where(kr == NOKEY, 0, kr & 0xFFFFFFFF).astype(np.int64)
        x = np.broadcast_to(np.arange(W), (H, W))
        y = np.broadcast_to(np.arange(H)[:, None], (H, W))
        i = np.arange(self.D)
        xq = np.maximum(x[..., None] - i, 0)
        b = md[..., None] + xq - x[..., None]
        valid = (i < md[..., None]) & (b >= self.b) & (b < self.e)
        cand = np.full((H, W, self.D), np.nan, np.float32)
        yy = np.broadcast_to(y[..., None], cand.shape)
        cand[valid] = c[yy[valid], xq[valid], (b - self.b)[valid]]
        ii = np.broadcast_to(i, cand.shape)
        pen = penalty(self.ref_r[1][..., None], self.ref_r[0][..., None], ii, cand)  # i: the scan index
        m1, m2, idx = _top2(pen, ii)
        tkey = np.where(idx < 0, NOKEY, _key(m1, np.maximum(idx, 0)))
        return torch.from_numpy(tkey), torch.from_numpy(m1), torch.from_numpy(m2)

    def ref_finalize(self, key, tkey, t2):
        """(d_ref, d_tar, conf_ref): conf_ref receives the TARGET confidence, the left
        second minimum is not used (K/asw_wta_ref.cl:64-66)."""
        k, tk = key.numpy(), tkey.numpy()
        H, W = k.shape
        x = np.broadcast_to(np.arange(W), (H, W))
        md = np.where(k == NOKEY, 0, k & 0xFFFFFFFF).astype(np.int32)
        ti = (tk & 0xFFFFFFFF).astype(np.int64)
        mdr = np.where(tk == NOKEY, md, md + np.maximum(x - ti, 0) - x).astype(np.int32)
        tm1 = np.where(tk == NOKEY, INIT,
                       (tk.astype(np.uint64) >> np.uint64(32)).astype(np.uint32).view(np.float32))
        with np.errstate(invalid="ignore", divide="ignore"):
            conf_ref = (t2.numpy() - tm1) / t2.numpy()
        return md, mdr, conf_ref.astype(np.float32)


# ------------------------------------------------------------------ whole-volume forms

def _whole(C, ref_l=None, ref_r=None):
    """The reference's loops on a plane-major volume [D][H][W], written without keys or
    shards: own scan over d, target scan over i with the winner recorded as the plane b."""
    C = np.asarray(C, np.float32)
    D, H, W = C.shape
    own = np.ascontiguousarray(C.transpose(1, 2, 0))
    d = np.broadcast_to(np.arange(D), own.shape)
    if ref_l is not None:
        own = penalty(ref_l[1][..., None], ref_l[0][..., None], d, own)
    m1, m2, idx = _top2(own, d)
    md = np.maximum(idx, 0)
    x = np.broadcast_to(np.arange(W), (H, W))[..., None]
    y = np.broadcast_to(np.arange(H)[:, None], (H, W))[..., None]
    i = np.broadcast_to(np.arange(D), (H, W, D))
    xq = np.maximum(x - i, 0)
    b = md[..., None] + xq - x
    valid = i < md[..., None]
    cand = np.where(valid, C[np.where(valid, b, 0), y, xq], np.float32(np.nan)).astype(np.float32)
    if ref_r is not None:
        cand = penalty(ref_r[1][..., None], ref_r[0][..., None], i, cand)
    t1, t2, bidx = _top2(cand, b)
    mdr = np.where(bidx < 0, md, bidx)
    with np.errstate(invalid="ignore", divide="ignore"):
        conf_ref = ((m2 - m1) / m2).astype(np.float32)
        conf_tar = ((t2 - t1) / t2).astype(np.float32)
    return md.astype(np.int32), conf_ref, mdr.astype(np.int32), conf_tar


def wta(C):
    """asw_WTA on [D][H][W]: (d_ref, conf_ref, d_tar, conf_tar), as oracle.wta."""
    return _whole(C)


def wta_ref(C, ref_l, ref_r):
    """asw_WTA_REF on [D][H][W]: (d_ref, d_tar, conf_ref), as oracle.wta_ref."""
    md, _, mdr, conf_tar = _whole(C, ref_l, ref_r)
    return md, mdr, conf_tar


# ------------------------------------------------------------------------------ inputs

def well_volume(D, H, W, seed):
    """[D][H][W] float32, every value a multiple of 0.25 (exact ties): a per-pixel depth
    `base`, a background of base + 0.25..1.25, one well of depth `base` at a plane drawn
    over the whole range and, for 30 % of the pixels, a second equal well at another
    plane (a tie of the minimum, often across shards).  A pixel with a high base sees
    lower values along its diagonal, so its target scan leaves d_ref.  Row 0 starts with
    all-equal pixels; row 1 with pixels that hold nothing below the 100000 sentinel."""
    rng = np.random.default_rng(seed)
    q = np.float32(0.25)
    base = (rng.integers(0, 4, (H, W)) + 1).astype(np.float32) * q
    C = base + rng.integers(1, 6, (D, H, W)).astype(np.float32) * q
    y, x = np.mgrid[0:H, 0:W]
    md = rng.integers(0, D, (H, W))
    C[md, y, x] = base
    if D > 1:
        twice = rng.random((H, W)) < 0.3
        md2 = (md + rng.integers(1, D, (H, W))) % D  # uniform over the other planes
        C[md2[twice], y[twice], x[twice]] = base[twice]
    C[:, 0, :3] = 5.0
    if H > 1:
        C[:, 1, 0] = 100000.0
        C[:, 1, 1:2] = 250000.0
    assert C.dtype == np.float32
    return np.ascontiguousarray(C)


def refine_estimates(H, W, D, seed):
    """(ref_l, ref_r), each [2][H][W] float32 = (value plane, den plane) like asw_ref_h's
    output: values on the 0.25 grid from -2 to past D; den 0 switches the penalty off
    (the ties come back), 3e7 lifts most or all planes above the sentinel."""
    rng = np.random.default_rng(seed)
    dens = np.array([0, 1e-5, 0.5, 1, 4, 64, 3e7], np.float32)
    prob = [.2, .1, .2, .2, .15, .1, .05]

    def one():
        val = rng.integers(-8, 4 * (D + 2), (H, W)).astype(np.float32) * np.float32(0.25)
        den = rng.choice(dens, size=(H, W), p=prob).astype(np.float32)
        return np.ascontiguousarray(np.stack([val, den]))

    return one(), one()


def _even(D, n):
    return tuple(shard_range(D, r, n) for r in range(n))


# (D, H, W, ((d_begin, d_end), ...)): each the smallest shape that reaches its edge
CASES = [
    (70, 7, 20, ((0, 24), (24, 47), (47, 70))),       # pitch 32 everywhere, waves over 3-4 rows, S % 64 != 0
    (200, 3, 150, ((0, 70), (70, 135), (135, 200))),  # pitch 128
    (200, 3, 150, _even(200, 8)),                     # pitch 32
    (512, 2, 300, _even(512, 8)),                     # D > 256, md > W
    (512, 2, 300, ((0, 33), (33, 300), (300, 512))),  # pitches 64 / 320 / 256 in one frame
    (256, 2, 130, _even(256, 8)),                     # the eight-way 32-plane shard shape
    (33, 1, 64, ((0, 32), (32, 33))),                 # a one-plane shard, exactly one wave
    (9, 5, 1, ((0, 5), (5, 9))),                      # W = 1: every scan step is clamped
]


def case_id(case):
    D, H, W, spans = case
    return f"D{D}-H{H}-W{W}-" + "_".join(str(b) for b, _ in spans)


def case_seed(D, H, W):
    return 7919 * D + 131 * H + W


def local_cost(C, b, e):
    """Planes [b, e) of a plane-major volume as the pixel-major [H][W][n] tensor of a shard."""
    return torch.from_numpy(np.ascontiguousarray(C[b:e].transpose(1, 2, 0)))


def _min(ts):
    return functools.reduce(torch.minimum, ts)


class ShardCase:
    """One (shape, split): the inputs, every stage result of every shard and the combined
    results, plain and penalised, all from the numpy restatement.  Shared (see
    :func:`shard_case`) and read-only."""

    def __init__(self, D, H, W, spans):
        self.D, self.H, self.W, self.spans = D, H, W, spans
        seed = case_seed(D, H, W)
        self.C = well_volume(D, H, W, seed)
        self.ref_l, self.ref_r = refine_estimates(H, W, D, seed + 1)
        self.ops = [CpuRefShardOps(b, e, D, self.ref_l, self.ref_r) for b, e in spans]
        self.costs = [local_cost(self.C, b, e) for b, e in spans]
        # plain protocol (sharded_wta's sequence)
        self.local = [o.local(c) for o, c in zip(self.ops, self.costs)]
        self.key_g = _min([k for k, _, _ in self.local])
        self.second = [o.second(self.key_g, *l) for o, l in zip(self.ops, self.local)]
        self.m2_g = _min(self.second)
        self.target = [o.target_local(c, self.key_g) for o, c in zip(self.ops, self.costs)]
        self.tkey_g = _min([k for k, _, _ in self.target])
        self.tsecond = [o.second(self.tkey_g, *t) for o, t in zip(self.ops, self.target)]
        self.t2_g = _min(self.tsecond)
        self.final = self.ops[0].finalize(self.key_g, self.m2_g, self.tkey_g, self.t2_g)
        # penalised protocol (asw_wta_ref_local's sequence)
        self.rlocal = [o.ref_local(c) for o, c in zip(self.ops, self.costs)]
        self.rkey_g = _min([k for k, _, _ in self.rlocal])
        self.rtarget = [o.ref_target_local(c, self.rkey_g) for o, c in zip(self.ops, self.costs)]
        self.rtkey_g = _min([k for k, _, _ in self.rtarget])
        self.rtsecond = [o.second(self.rtkey_g, *t) for o, t in zip(self.ops, self.rtarget)]
        self.rt2_g = _min(self.rtsecond)
        self.rfinal = self.ops[0].ref_finalize(self.rkey_g, self.rtkey_g, self.rt2_g)

    def _owner(self, d):
        own = np.full(d.shape, -1)
        for s, (b, e) in enumerate(self.spans):
            own[(d >= b) & (d < e)] = s
        return own

    def shares(self):
        """The input conditions, from the reference results alone (shares of the pixels)."""
        dr, _, dt, _ = self.final
        rdr, rdt, _ = self.rfinal
        gmin = _min([m1 for _, m1, _ in self.local]).numpy()
        attained = sum((m1.numpy() == gmin) & (k.numpy() != NOKEY) for k, m1, _ in self.local)
        x = np.broadcast_to(np.arange(self.W), dr.shape)
        own = self._owner(dr)
        rown = self._owner(rdr)
        n = len(self.spans)
        return {
            "min_in_two_shards": float(np.mean(attained >= 2)),
            "tar_ne_ref": float(np.mean(dt != dr)),
            "tar_ne_ref_pen": float(np.mean(rdt != rdr)),
            "tar_other_shard": float(np.mean(self._owner(dt) != own)),
            "tar_other_shard_pen": float(np.mean(self._owner(rdt) != rown)),
            "ref_gt_x": float(np.mean(dr > x)),
            "ref_gt_x_pen": float(np.mean(rdr > x)),
            "min_shard_owns": float(min(np.mean(own == s) for s in range(n))),
            "min_shard_owns_pen": float(min(np.mean(rown == s) for s in range(n))),
        }

    def checked(self):
        """W >= 100 and at least 3 shards: the cases that must meet REQUIRED."""
        return self.W >= 100 and len(self.spans) >= 3

    def assert_conditions(self):
        """The inputs still separate the rules under test (about half of what the recipe
        gives, so another seed passes but an emptied case does not)."""
        if not self.checked():
            return None
        s = self.shares()
        print(case_id((self.D, self.H, self.W, self.spans)), {k: round(v, 3) for k, v in s.items()})
        for name, need in REQUIRED.items():
            assert s[name] >= need, (name, s[name], need)
        return s


REQUIRED = {
    "min_in_two_shards": 0.10,
    "tar_ne_ref": 0.25,
    "tar_ne_ref_pen": 0.25,
    "tar_other_shard": 0.03,
    "ref_gt_x": 0.30,
    "min_shard_owns": 0.01,
}


@functools.lru_cache(maxsize=None)
def shard_case(D, H, W, spans) -> ShardCase:
    return ShardCase(D, H, W, spans)
