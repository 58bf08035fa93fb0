// asw_speckle.hip — speckle filter: connected components of similar disparity on an int32 map
// (include/asw.h §speckle).  The reference has no counterpart.
//
// Pixels are linked when they are 4-neighbours, both valid and |d[p] - d[q]| <= max_diff (in
// 64 bits).  Every valid pixel receives the smallest flat index of its component (label), the
// component's pixel count (size) and size >= min_size (keep): functions of the input alone.
//
// Four launches on a label array L and a count array C in the workspace:
//   k_speckle_tile   one block per 64 x 16 tile: horizontal runs by ballot, vertical links by a
//                    union-find in LDS, counts per tile-local root; L[p] = the global index of
//                    p's tile-local root, C[p] = its count at a tile-local root, 0 elsewhere
//   k_speckle_seam   one thread per pixel pair across a tile seam: union on L in global memory
//   k_speckle_count  every tile-local root that is no global root points itself at its global
//                    root and adds its count there: one atomic per (tile, component)
//   k_speckle_apply  label / size / keep of every pixel (at most three loads of L)
//
// Union-find invariants: a stored label never increases and L[i] <= i, so a find strictly
// descends and a union retries only after another thread lowered a value.  Every loop that
// follows links also stops after S = W * H steps and then sets the status word (offset
// ASW_SPECKLE_STATUS_OFFSET of the workspace) to a non-zero value.
//
// Visibility: in k_speckle_seam and k_speckle_count other workgroups write L during the launch;
// every value of L those kernels act on is the return value of an atomic or a relaxed agent-scope
// atomic load (served by L2, never by a CU's L1).  The tile kernel's unions are in LDS.  All other
// loads read bytes written before the launch (kernel boundaries order them).
#include <hip/hip_runtime.h>

#include "asw_common.h"

namespace asw {
namespace {

constexpr int kTW = 64;   // tile columns = lanes of a wave
constexpr int kTH = 16;   // tile rows
constexpr int kTileThreads = 256;
constexpr int kTileWaves = kTileThreads / kWave;
constexpr int kRowsPerWave = kTH / kTileWaves;
constexpr unsigned kMaxTileBlocks = 1u << 22;  // more tiles than this: a block walks several
constexpr size_t kStatusBytes = 256;           // the status word's block at the workspace's start

constexpr int kFailTile = 1, kFailSeam = 2, kFailCount = 4, kFailApply = 8;  // status bits

__device__ __forceinline__ bool similar(int a, int b, int max_diff) {
    const long long dd = (long long)a - (long long)b;
    return dd <= (long long)max_diff && dd >= -(long long)max_diff;
}

// ---- union-find on tile-local indices in LDS (workgroup scope)
__device__ __forceinline__ int lds_find(int *lab, int x, int lim, bool &fail) {
    for (int n = 0;; ++n) {
        const int q = __hip_atomic_load(&lab[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (q == x) return x;
        if (n >= lim) {
            fail = true;
            return x;
        }
        x = q;
    }
}

__device__ __forceinline__ void lds_union(int *lab, int a, int b, int lim, bool &fail) {
    for (int n = 0;; ++n) {
        a = lds_find(lab, a, lim, fail);
        b = lds_find(lab, b, lim, fail);
        if (fail || a == b) return;
        const int hi = a > b ? a : b, lo = a > b ? b : a;
        const int old = atomicMin(&lab[hi], lo);  // the larger root under the smaller
        if (old == hi) return;
        if (n >= lim) {
            fail = true;
            return;
        }
        a = old;  // hi was no root any more: its other parent joins lo
        b = lo;
    }
}

// ---- union-find on flat pixel indices in global memory (agent scope)
__device__ __forceinline__ int glb_load(const int *L, long long i) {
    return __hip_atomic_load(L + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ int glb_find(const int *L, int x, int lim, bool &fail) {
    for (int n = 0;; ++n) {
        const int q = glb_load(L, x);
        if (q == x) return x;
        if (n >= lim) {
            fail = true;
            return x;
        }
        x = q;
    }
}

__device__ __forceinline__ void glb_union(int *L, int a, int b, int lim, bool &fail) {
    for (int n = 0;; ++n) {
        a = glb_find(L, a, lim, fail);
        b = glb_find(L, b, lim, fail);
        if (fail || a == b) return;
        const int hi = a > b ? a : b, lo = a > b ? b : a;
        const int old = atomicMin(&L[hi], lo);
        if (old == hi) return;
        if (n >= lim) {
            fail = true;
            return;
        }
        a = old;
        b = lo;
    }
}

// One 64 x 16 tile per block turn; wave w owns rows 4w..4w+3, lane = column.  Pixels outside
// the image and invalid pixels are singletons that nothing links to.
__global__ __launch_bounds__(kTileThreads) void k_speckle_tile(int W, int H, int max_diff, unsigned tiles_x,
                                                               unsigned ntiles, const int32_t *__restrict__ d,
                                                               const uint8_t *__restrict__ valid, int *label_g,
                                                               int *cnt_g, int lim, int *status) {
    __shared__ int s_lab[kTW * kTH];
    __shared__ int s_cnt[kTW * kTH];
    __shared__ int s_d[kTW * kTH];
    __shared__ uint8_t s_fl[kTW * kTH];  // bit 0: linked to the left neighbour, bit 1: valid
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const unsigned long long upto = lane == kWave - 1 ? ~0ull : (2ull << lane) - 1;  // bits 0..lane
    bool fail = false;
    for (unsigned tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int x0 = (int)(tile % tiles_x) * kTW, y0 = (int)(tile / tiles_x) * kTH;
        const int x = x0 + lane;
        // 1. horizontal runs: the run start of a lane is the last lane <= it that is not
        //    linked to its left neighbour
#pragma unroll
        for (int j = 0; j < kRowsPerWave; ++j) {
            const int r = wave * kRowsPerWave + j, y = y0 + r, idx = r * kTW + lane;
            const bool in = x < W && y < H;
            const long long gp = (long long)y * W + x;
            const int dv = in ? d[gp] : 0;
            const bool ok = in && (!valid || valid[gp] != 0);
            const int dl = __shfl_up(dv, 1, kWave);
            const int okl = __shfl_up((int)ok, 1, kWave);
            const bool link_l = ok && lane > 0 && okl && similar(dv, dl, max_diff);
            const unsigned long long starts = ~__ballot(link_l);  // bit 0 is always set
            s_lab[idx] = r * kTW + (63 - __clzll((long long)(starts & upto)));
            s_cnt[idx] = 0;
            s_d[idx] = dv;
            s_fl[idx] = (uint8_t)((link_l ? 1 : 0) | (ok ? 2 : 0));
        }
        __syncthreads();
        // 2. vertical links.  A link whose left neighbours are linked to each other and to
        //    both of its ends follows from theirs: one union per pair of overlapping runs.
#pragma unroll
        for (int j = 0; j < kRowsPerWave; ++j) {
            const int r = wave * kRowsPerWave + j, idx = r * kTW + lane;
            if (r == 0) continue;  // wave-uniform
            const int fl = s_fl[idx], flu = s_fl[idx - kTW];
            const bool link_u = (fl & 2) && (flu & 2) && similar(s_d[idx], s_d[idx - kTW], max_diff);
            const unsigned long long mu = __ballot(link_u);
            const bool implied = (fl & 1) && (flu & 1) && ((mu >> (lane > 0 ? lane - 1 : 0)) & 1);
            if (link_u && !implied) lds_union(s_lab, idx, idx - kTW, lim, fail);
        }
        __syncthreads();
        // 3. every pixel's tile-local root; a run's first lane adds the run's length to it
        int root[kRowsPerWave];
#pragma unroll
        for (int j = 0; j < kRowsPerWave; ++j) {
            const int r = wave * kRowsPerWave + j, idx = r * kTW + lane;
            const int fl = s_fl[idx];
            const unsigned long long starts = ~__ballot(fl & 1);
            root[j] = lds_find(s_lab, idx, lim, fail);
            if ((fl & 2) && !(fl & 1)) {
                const unsigned long long later = lane == kWave - 1 ? 0ull : starts >> (lane + 1);
                const int len = later ? __ffsll((long long)later) : kWave - lane;
                atomicAdd(&s_cnt[root[j]], len);
            }
        }
        __syncthreads();
        // 4. row-major order inside the tile agrees with the flat order: the local minimum
        //    is the component's smallest flat index within the tile
#pragma unroll
        for (int j = 0; j < kRowsPerWave; ++j) {
            const int r = wave * kRowsPerWave + j, y = y0 + r, idx = r * kTW + lane;
            if (x < W && y < H) {
                const long long gp = (long long)y * W + x;
                const int rr = root[j] / kTW, rc = root[j] % kTW;
                label_g[gp] = (int)((long long)(y0 + rr) * W + (x0 + rc));
                cnt_g[gp] = root[j] == idx ? s_cnt[idx] : 0;
            }
        }
        __syncthreads();  // the next tile reuses the arrays
    }
    if (fail) atomicOr(status, kFailTile);
}

struct SeamInput {
    const int32_t *d;
    const uint8_t *valid;
    int max_diff;
    __device__ __forceinline__ bool ok(long long p) const { return !valid || valid[p] != 0; }
    __device__ __forceinline__ bool link(long long p, long long q) const {
        return ok(p) && ok(q) && similar(d[p], d[q], max_diff);
    }
};

// Threads [0, n_h): pixel x of horizontal seam s (rows 16s+15 | 16s+16) and the pixel below it;
// threads [n_h, n): pixel y of vertical seam s (columns 64s+63 | 64s+64) and the pixel right of it.
// A link is skipped when the same link one step back along the seam, inside the same tile, exists
// together with the two links that join the pairs: the tile kernel made those two, the thread one
// step back makes (or was itself spared) the third.  The first pair of a tile is never skipped.
__global__ __launch_bounds__(256) void k_speckle_seam(int W, int H, SeamInput in, int *L, long long n_h, long long n,
                                                      int lim, int *status) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    long long a, step, back;
    bool first;
    if (t < n_h) {
        const long long s = t / W;
        const int x = (int)(t - s * W);
        a = (s * kTH + kTH - 1) * W + x;
        step = W;
        back = 1;
        first = x % kTW == 0;
    } else {
        const long long u = t - n_h, s = u / H;
        const int y = (int)(u - s * H);
        a = (long long)y * W + (s * kTW + kTW - 1);
        step = 1;
        back = W;
        first = y % kTH == 0;
    }
    const long long b = a + step;
    if (!in.link(a, b)) return;
    if (!first && in.link(a - back, a) && in.link(b - back, b) && in.link(a - back, b - back)) return;
    bool fail = false;
    glb_union(L, (int)a, (int)b, lim, fail);
    if (fail) atomicOr(status, kFailSeam);
}

// Givers (tile-local roots with a smaller global root) are never receivers (global roots), so the
// count a giver reads is final.  The giver's label drops to its global root: k_speckle_apply then
// walks at most pixel -> tile-local root -> global root.
__global__ __launch_bounds__(256) void k_speckle_count(long long n, int *L, int *cnt_g, int lim, int *status) {
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const int c = cnt_g[p];
    if (c <= 0) return;  // no tile-local root of a valid component
    bool fail = false;
    const int r = glb_find(L, (int)p, lim, fail);
    if (fail) {
        atomicOr(status, kFailCount);
        return;
    }
    if (r != (int)p) {
        __hip_atomic_store(L + p, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        atomicAdd(&cnt_g[r], c);
    }
}

__global__ __launch_bounds__(256) void k_speckle_apply(long long n, int min_size, const uint8_t *__restrict__ valid,
                                                       const int *__restrict__ L, const int *__restrict__ cnt_g,
                                                       int32_t *__restrict__ label, int32_t *__restrict__ size,
                                                       uint8_t *__restrict__ keep, int lim, int *status) {
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    int lab = -1, sz = 0;
    if (!valid || valid[p] != 0) {
        int r = L[p];
        bool fail = false;
        for (int k = 0;; ++k) {
            const int q = L[r];
            if (q == r) break;
            if (k >= lim) {
                fail = true;
                break;
            }
            r = q;
        }
        if (fail) atomicOr(status, kFailApply);
        lab = r;
        sz = cnt_g[r];
    }
    if (label) label[p] = lab;
    if (size) size[p] = sz;
    if (keep) keep[p] = sz >= min_size ? 1 : 0;
}

__global__ __launch_bounds__(256) void k_lr_valid(long long n, int D, int mode, const int32_t *__restrict__ d_ref,
                                                  const int32_t *__restrict__ d_tar,
                                                  const uint8_t *__restrict__ code_ref,
                                                  const uint8_t *__restrict__ code_tar, uint8_t *__restrict__ valid) {
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    valid[p] = lr_consistent(mode, D, p, d_ref[p], d_tar, code_ref, code_tar) ? 1 : 0;
}

__global__ __launch_bounds__(256) void k_speckle_mask16(long long n, const int32_t *__restrict__ d,
                                                        const uint8_t *__restrict__ keep, uint16_t *__restrict__ out) {
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    out[p] = keep[p] ? (uint16_t)d[p] : (uint16_t)ASW_DISP16_INVALID;
}

__global__ __launch_bounds__(256) void k_speckle_mask_f32(long long n, const float *__restrict__ disp,
                                                          const uint8_t *__restrict__ keep, float *__restrict__ out) {
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    out[p] = keep[p] ? disp[p] : __uint_as_float(0x7fc00000u);  // asw_disp_mask's quiet NaN
}

inline int finish_launch() {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_hip_error(e);
        return ASW_E_HIP;
    }
    return ASW_OK;
}

inline dim3 pixel_grid(long long n) { return dim3((unsigned)((n + 255) / 256)); }

inline size_t map_bytes(long long n) { return ((size_t)n * 4 + 255) / 256 * 256; }

// [a, a + na) and [b, b + nb) share a byte
inline bool overlaps(const void *a, size_t na, const void *b, size_t nb) {
    if (!a || !b) return false;
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}

}  // namespace
}  // namespace asw

using namespace asw;

#define ASW_CHECK_PARAMS(p)                 \
    do {                                    \
        const int _s = asw_params_check(p); \
        if (_s != ASW_OK) return _s;        \
    } while (0)

extern "C" {

void asw_speckle_params_default(asw_speckle_params *sp) {
    if (!sp) return;
    sp->min_size = 32;
    sp->max_diff = 1;
}

int asw_speckle_params_check(const asw_params *p, const asw_speckle_params *sp) {
    if (!p || !sp) return ASW_E_INVALID;
    // labels are int32 pixel indices; ahead of asw_params_check, whose own pixel limit is lower
    if (p->width >= 1 && p->height >= 1 && (long long)p->width * p->height > 0x7fffffffLL) return ASW_E_UNSUPPORTED;
    if (asw_params_check(p) != ASW_OK) return ASW_E_INVALID;
    if (sp->min_size < 1 || sp->max_diff < 0 || sp->max_diff > 65535) return ASW_E_INVALID;
    return ASW_OK;
}

size_t asw_speckle_workspace_bytes(const asw_params *p) {
    if (!p || p->width < 1 || p->height < 1) return 0;
    return kStatusBytes + 2 * map_bytes((long long)p->width * p->height);
}

int asw_lr_valid(const asw_params *p, const int32_t *d_ref, const int32_t *d_tar, const uint8_t *code_ref,
                 const uint8_t *code_tar, uint8_t *valid, void *stream) {
    ASW_CHECK_PARAMS(p);
    if (!d_ref || !d_tar || !valid) return ASW_E_INVALID;
    if (p->lr_mode == ASW_LR_U8 && (!code_ref || !code_tar)) return ASW_E_INVALID;
    const long long n = (long long)p->width * p->height;
    hipLaunchKernelGGL(k_lr_valid, pixel_grid(n), dim3(256), 0, (hipStream_t)stream, n, p->ndisp, p->lr_mode, d_ref,
                       d_tar, code_ref, code_tar, valid);
    return finish_launch();
}

int asw_speckle(const asw_params *p, const asw_speckle_params *sp, const int32_t *d, const uint8_t *valid,
                void *workspace, int32_t *label, int32_t *size, uint8_t *keep, void *stream) {
    if (const int s = asw_speckle_params_check(p, sp)) return s;
    if (!d || !workspace) return ASW_E_INVALID;
    const int W = p->width, H = p->height;
    const long long n = (long long)W * H;
    const size_t ws_bytes = asw_speckle_workspace_bytes(p);
    if (overlaps(workspace, ws_bytes, d, (size_t)n * 4) || overlaps(workspace, ws_bytes, valid, (size_t)n) ||
        overlaps(workspace, ws_bytes, label, (size_t)n * 4) || overlaps(workspace, ws_bytes, size, (size_t)n * 4) ||
        overlaps(workspace, ws_bytes, keep, (size_t)n))
        return ASW_E_INVALID;
    hipStream_t st = (hipStream_t)stream;
    char *ws = static_cast<char *>(workspace);
    int *status = reinterpret_cast<int *>(ws + ASW_SPECKLE_STATUS_OFFSET);
    int *L = reinterpret_cast<int *>(ws + kStatusBytes);
    int *cnt = reinterpret_cast<int *>(ws + kStatusBytes + map_bytes(n));
    const int lim = (int)n;
    if (const hipError_t e = hipMemsetAsync(ws, 0, kStatusBytes, st); e != hipSuccess) {
        set_hip_error(e);
        return ASW_E_HIP;
    }

    const unsigned tiles_x = (unsigned)((W + kTW - 1) / kTW);
    // at most 2^31 / 16 tiles (width 1): the product fits 32 bits
    const unsigned ntiles = tiles_x * (unsigned)((H + kTH - 1) / kTH);
    hipLaunchKernelGGL(k_speckle_tile, dim3(ntiles < kMaxTileBlocks ? ntiles : kMaxTileBlocks), dim3(kTileThreads), 0,
                       st, W, H, sp->max_diff, tiles_x, ntiles, d, valid, L, cnt, lim, status);
    if (const int s = finish_launch()) return s;

    const long long n_h = (long long)((H - 1) / kTH) * W, n_v = (long long)((W - 1) / kTW) * H;
    if (n_h + n_v > 0) {
        const SeamInput in{d, valid, sp->max_diff};
        hipLaunchKernelGGL(k_speckle_seam, pixel_grid(n_h + n_v), dim3(256), 0, st, W, H, in, L, n_h, n_h + n_v, lim,
                           status);
        if (const int s = finish_launch()) return s;
        hipLaunchKernelGGL(k_speckle_count, pixel_grid(n), dim3(256), 0, st, n, L, cnt, lim, status);
        if (const int s = finish_launch()) return s;
    }
    if (label || size || keep) {
        hipLaunchKernelGGL(k_speckle_apply, pixel_grid(n), dim3(256), 0, st, n, sp->min_size, valid, L, cnt, label,
                           size, keep, lim, status);
        if (const int s = finish_launch()) return s;
    }
    return ASW_OK;
}

int asw_speckle_mask16(const asw_params *p, const int32_t *d, const uint8_t *keep, uint16_t *out, void *stream) {
    ASW_CHECK_PARAMS(p);
    if (p->ndisp > 65535 || !d || !keep || !out) return ASW_E_INVALID;
    const long long n = (long long)p->width * p->height;
    hipLaunchKernelGGL(k_speckle_mask16, pixel_grid(n), dim3(256), 0, (hipStream_t)stream, n, d, keep, out);
    return finish_launch();
}

int asw_speckle_mask_f32(const asw_params *p, const float *disp, const uint8_t *keep, float *out, void *stream) {
    ASW_CHECK_PARAMS(p);
    if (!disp || !keep || !out) return ASW_E_INVALID;
    const long long n = (long long)p->width * p->height;
    hipLaunchKernelGGL(k_speckle_mask_f32, pixel_grid(n), dim3(256), 0, (hipStream_t)stream, n, disp, keep, out);
    return finish_launch();
}

}  // extern "C"
