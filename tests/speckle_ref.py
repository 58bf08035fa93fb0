"""Numpy restatement of the speckle filter (include/asw.h §speckle): the
oracle of tests/test_speckle.py and tests/test_gpu_speckle.py, and the generators both share.

Pixels p and q are linked when they are 4-neighbours, both valid and |d[p] - d[q]| <= max_diff
(in 64 bits).  components() is a flood fill in flat order, so the first pixel it meets of a
component is the component's smallest flat index.
"""
import numpy as np

I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
TILE_W, TILE_H = 64, 16  # the tile of k_speckle_tile: the generators put their seams there
DEFAULT = dict(min_size=32, max_diff=1)


def params_ok(min_size, max_diff):
    """The parameter rule of asw_speckle_params_check (given a valid asw_params)."""
    return 1 <= min_size <= I32_MAX and 0 <= max_diff <= 65535


def _valid(d, valid):
    return np.ones(d.shape, bool) if valid is None else np.asarray(valid) != 0


def components(d, valid=None, min_size=32, max_diff=1):
    """(label int32, size int32, keep uint8) [H][W]."""
    d = np.asarray(d).astype(np.int64)
    H, W = d.shape
    ok = _valid(d, valid)
    label = np.full((H, W), -1, np.int64)
    size = np.zeros((H, W), np.int64)
    for y0 in range(H):
        for x0 in range(W):
            if not ok[y0, x0] or label[y0, x0] >= 0:
                continue
            root = y0 * W + x0
            label[y0, x0] = root
            stack, members = [(y0, x0)], []
            while stack:
                y, x = stack.pop()
                members.append((y, x))
                for ny, nx in ((y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1)):
                    if 0 <= ny < H and 0 <= nx < W and ok[ny, nx] and label[ny, nx] < 0 \
                            and abs(int(d[y, x]) - int(d[ny, nx])) <= max_diff:
                        label[ny, nx] = root
                        stack.append((ny, nx))
            ys, xs = zip(*members)
            size[ys, xs] = len(members)
    keep = (ok & (size >= min_size)).astype(np.uint8)
    return label.astype(np.int32), size.astype(np.int32), keep


def mask16(d, keep):
    return np.where(np.asarray(keep) != 0, np.asarray(d).astype(np.int64) & 0xFFFF, 0xFFFF).astype(np.uint16)


def mask_f32(disp, keep):
    return np.where(np.asarray(keep) != 0, disp, np.float32(np.nan)).astype(np.float32)


# ------------------------------------------------------------------ generators: (d int32, valid uint8 | None)

def _i32(a):
    return np.ascontiguousarray(a, np.int32)


def random(H, W, seed=0, levels=4, hole_share=0.2):
    rng = np.random.default_rng(seed + 7919 * H + W)
    d = rng.integers(0, levels, (H, W))
    valid = (rng.random((H, W)) >= hole_share).astype(np.uint8)
    return _i32(d), valid


def checker(H, W, step=2):
    """Singletons at max_diff < step, one component at max_diff >= step."""
    y, x = np.mgrid[0:H, 0:W]
    return _i32(((x + y) & 1) * step), None


def ramp(H, W):
    """d = x: one component at max_diff >= 1, the columns at max_diff 0."""
    return _i32(np.broadcast_to(np.arange(W), (H, W))), None


def serpentine(H, W):
    """Even rows are a corridor (5), odd rows walls (1000) with one gap at alternating ends: one
    component of about half the pixels with label 0 that crosses every seam."""
    d = np.full((H, W), 5, np.int64)
    for y in range(1, H, 2):
        d[y] = 1000
        d[y, W - 1 if y % 4 == 1 else 0] = 5
    return _i32(d), None


def spiral(H, W):
    """A one-pixel path that winds inwards, its value rising by one every second step, between
    one-pixel walls of 0."""
    d = np.zeros((H, W), np.int64)
    on = np.zeros((H, W), bool)
    y = x = 0
    dy, dx = 0, 1
    on[0, 0] = True
    d[0, 0] = 100
    k = 0
    inside = lambda a, b: 0 <= a < H and 0 <= b < W  # noqa: E731
    while True:
        for _ in range(2):
            ny, nx, my, mx = y + dy, x + dx, y + 2 * dy, x + 2 * dx
            if inside(ny, nx) and not on[ny, nx] and not (inside(my, mx) and on[my, mx]):
                break
            dy, dx = dx, -dy
        else:
            break
        y, x, k = ny, nx, k + 1
        on[y, x] = True
        d[y, x] = 100 + k // 2
    return _i32(d), None


def ushape(H, W, max_diff=1):
    """Two bars (50) in the first and the last column, joined only along the bottom row, on a
    background of 10000; beside the first bar a decoy bar of 50 + max_diff + 1."""
    d = np.full((H, W), 10000, np.int64)
    d[:, 0] = 50
    d[:, W - 1] = 50
    d[H - 1, :] = 50
    if W > 2 and H > 1:
        d[:H - 1, 1] = 50 + max_diff + 1
    return _i32(d), None


def blobs(H, W, min_size=6):
    """On a background of 0: a vertical strip (50) of min_size - 1 pixels in column 0 that ends
    one row below the first horizontal tile seam, and a horizontal strip (90) of min_size pixels
    in row 0 that ends one column right of the first vertical tile seam (clipped to the image)."""
    d = np.zeros((H, W), np.int64)
    n = min_size - 1
    d[max(1, TILE_H + 1 - n):min(H, TILE_H + 1), 0] = 50
    n = min_size
    d[0, max(1, TILE_W + 1 - n):min(W, TILE_W + 1)] = 90
    return _i32(d), None


def extremes(H, W):
    """A checkerboard of INT32_MIN and INT32_MAX: every pair of neighbours differs by 2^32 - 1,
    which no max_diff links (and a 32-bit difference would wrap to -1): singletons."""
    y, x = np.mgrid[0:H, 0:W]
    return _i32(np.where((x + y) & 1, I32_MIN, I32_MAX)), None


def all_invalid(H, W):
    return random(H, W, 3)[0], np.zeros((H, W), np.uint8)


def one_valid(H, W):
    valid = np.zeros((H, W), np.uint8)
    valid[H // 2, W // 2] = 1
    return random(H, W, 4)[0], valid


GENERATORS = {
    "random": random,
    "random_dense": lambda H, W: random(H, W, 1, 2, 0.05),
    "checker": checker,
    "ramp": ramp,
    "serpentine": serpentine,
    "spiral": spiral,
    "ushape": ushape,
    "blobs": blobs,
    "extremes": extremes,
    "all_invalid": all_invalid,
    "one_valid": one_valid,
}
# (min_size, max_diff) pairs of the stage tests; blobs() is built for min_size 6
PARAMS = [(1, 0), (6, 1), (32, 1), (3, 2)]
# the smallest shapes (H, W) that straddle the 64 x 16 tile: one pixel, one row, one column, one
# exact tile, a tile plus one pixel each way, four ragged tiles each way
SHAPES = [(1, 1), (1, 200), (40, 1), (16, 64), (17, 65), (50, 200)]
