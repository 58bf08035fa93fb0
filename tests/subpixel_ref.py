"""Numpy float32 restatement of the sub-pixel maps (include/asw.h):
the oracle of tests/test_subpixel.py and tests/test_gpu_subpixel.py.

Every operation is an IEEE float32 one in the order the header states; numpy's float32
`-`, `+`, `*` and `/` are correctly rounded, so the GPU maps must equal these bit for bit.
"""
import numpy as np

F = np.float32
NOKEY = np.int64(0x7FFFFFFFFFFFFFFF)


def subpixel(C, d_ref):
    """C: [H][W][>=D] float32 (pixel-major, planes >= D never read), d_ref: int [H][W]."""
    return subpixel_D(C, d_ref, C.shape[2])


def subpixel_D(C, d_ref, D):
    C = np.asarray(C, F)
    d = np.asarray(d_ref).astype(np.int64)
    inner = (d > 0) & (d < D - 1)
    dc = np.where(inner, d, 1)  # a safe index where the neighbours are not read
    take = lambda k: np.take_along_axis(C, (dc + k)[..., None], axis=2)[..., 0]  # noqa: E731
    return from_neighbours(d, D, take(-1), take(0), take(1))


def from_neighbours(d, D, cm, c0, cp):
    d = np.asarray(d).astype(np.int64)
    inner = (d > 0) & (d < D - 1)
    with np.errstate(invalid="ignore", divide="ignore"):
        a = cm.astype(F) - c0.astype(F)
        b = cp.astype(F) - c0.astype(F)
        off = (a - b) / (F(2.0) * (a + b))
        assert off.dtype == F
        return np.where(inner, d.astype(F) + off, d.astype(F)).astype(F)


def lr_pass(d_ref, d_tar, code_ref, code_tar, D, mode):
    """The LR rule of asw_outputs.lr16: mode 0 = 8-bit codes (K/consist.cl:20-30), 1 = indices."""
    if mode == 0:
        scale = F(D - 1)
        qr = (code_ref.astype(F) / F(255.0)) * scale
        qt = (code_tar.astype(F) / F(255.0)) * scale
        return np.abs(qt - qr) < F(1.001)
    dd = d_ref.astype(np.int64) - d_tar.astype(np.int64)
    return (dd <= 1) & (dd >= -1)


def mask(disp, ok):
    return np.where(ok, disp, F(np.nan)).astype(F)


def fill(disp_lr):
    """Background fill per row, written as the definition (a loop over pixels)."""
    src = np.asarray(disp_lr, F)
    H, W = src.shape
    out = np.empty_like(src)
    for y in range(H):
        valid = ~np.isnan(src[y])
        cols = np.flatnonzero(valid)
        for x in range(W):
            if valid[x]:
                out[y, x] = src[y, x]
                continue
            left = cols[cols < x]
            right = cols[cols > x]
            if len(left) and len(right):
                out[y, x] = min(src[y, left[-1]], src[y, right[0]])
            elif len(left):
                out[y, x] = src[y, left[-1]]
            elif len(right):
                out[y, x] = src[y, right[0]]
            else:
                out[y, x] = F(0.0)
    return out


def key_index(key):
    key = np.asarray(key)
    return np.where(key == NOKEY, 0, key & 0xFFFFFFFF).astype(np.int64)


def local_neighbours(C_local, key_g, b, e, D):
    """asw_subpixel_local of the shard [b, e): C_local is [H][W][>= e-b]; returns [3][H][W]."""
    d = key_index(key_g)
    H, W = d.shape
    nb = np.full((3, H, W), np.inf, F)
    for j in range(3):
        pl = d - 1 + j
        own = (pl >= b) & (pl < e) & (pl >= 0) & (pl < D)
        idx = np.where(own, pl - b, 0)
        v = np.take_along_axis(np.asarray(C_local, F), idx[..., None], axis=2)[..., 0] if e > b else nb[j]
        nb[j] = np.where(own, v, F(np.inf))
    return nb


def finalize(key_g, nb, D):
    return from_neighbours(key_index(key_g), D, nb[0], nb[1], nb[2])


def same_bits(a, b):
    """Equal float32 bit patterns, NaN positions compared separately (any NaN payload)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != F or b.dtype != F or a.shape != b.shape:
        return False
    na, nb_ = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb_) and np.array_equal(a[~na].view(np.uint32), b[~nb_].view(np.uint32)))


def read_pfm(path):
    """One-channel PFM -> float32 [H][W] with the top row first."""
    with open(path, "rb") as f:
        assert f.readline().strip() == b"Pf"
        w, h = map(int, f.readline().split())
        scale = float(f.readline())
        data = np.frombuffer(f.read(), "<f4" if scale < 0 else ">f4")
    assert data.size == w * h
    return np.ascontiguousarray(data.reshape(h, w)[::-1]).astype(F), scale
