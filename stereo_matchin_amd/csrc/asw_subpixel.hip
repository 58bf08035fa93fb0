// asw_subpixel.hip — sub-pixel float disparity maps (include/asw.h):
// the parabola offset of the WTA winner from its two neighbouring planes of the final
// aggregated volume, its LR-masked form (NaN holes) and the row-wise background fill.
// The reference has no counterpart (it writes 8-bit codes only).
//
// Every float operation is written once (subpixel_value) and shared by the whole-volume
// kernel and the d-sharded finalize, so the two are bit-identical given the same three
// floats; -ffp-contract=off keeps the compiler from fusing any of it.
#include <hip/hip_runtime.h>

#include "asw_common.h"

namespace asw {
namespace {

constexpr long long kNoKey = 0x7fffffffffffffffLL;  // asw_wta_local's "no plane" sentinel
constexpr int kFillThreads = 256;
constexpr int kFillWaves = kFillThreads / kWave;

__device__ __forceinline__ float quiet_nan() { return __uint_as_float(0x7fc00000u); }
__device__ __forceinline__ float pos_inf() { return __uint_as_float(0x7f800000u); }

// the winner index of a global WTA key (k_wta_finalize's rule: no key -> 0)
__device__ __forceinline__ int key_index(long long k) { return k == kNoKey ? 0 : (int)(unsigned)(k & 0xffffffffLL); }

// d + (a - b) / (2 (a + b)), a = cm - c0, b = cp - c0; the quotient is the correctly
// rounded IEEE one (hipcc's default for `/`)
__device__ __forceinline__ float subpixel_value(int d, float cm, float c0, float cp) {
    const float a = cm - c0;
    const float b = cp - c0;
    const float off = (a - b) / (2.0f * (a + b));
    return (float)d + off;
}

// lane per pixel; the three neighbours are 12 contiguous bytes of [H][W][Dp]
__global__ __launch_bounds__(256) void k_subpixel(long long n, int D, int Dp, const float *__restrict__ cost,
                                                  const int32_t *__restrict__ d_ref, float *__restrict__ disp) {
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const int d = d_ref[p];
    float v = (float)d;
    if (d > 0 && d < D - 1) {  // also keeps an out-of-range index away from the volume
        const float *c = cost + p * (long long)Dp + d;
        v = subpixel_value(d, c[-1], c[0], c[1]);
    }
    disp[p] = v;
}

// shard [b, e): nb[j][p] = C[p][d-1+j] where the shard owns that plane, +INF elsewhere
__global__ __launch_bounds__(256) void k_subpixel_local(long long n, int D, int Dp, int b, int e,
                                                        const float *__restrict__ cost,
                                                        const long long *__restrict__ key_global,
                                                        float *__restrict__ nb) {
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const int d = key_index(key_global[p]);
    const float *c = cost + p * (long long)Dp;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int pl = d - 1 + j;
        float v = pos_inf();
        if (pl >= b && pl < e && pl >= 0 && pl < D) v = c[pl - b];
        nb[(long long)j * n + p] = v;
    }
}

__global__ __launch_bounds__(256) void k_subpixel_finalize(long long n, int D,
                                                           const long long *__restrict__ key_global,
                                                           const float *__restrict__ nb, float *__restrict__ disp) {
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const int d = key_index(key_global[p]);
    float v = (float)d;
    if (d > 0 && d < D - 1) v = subpixel_value(d, nb[p], nb[n + p], nb[2 * n + p]);
    disp[p] = v;
}

// the LR rule of k_disp16 / k_consistency on a float map: NaN where it fails
__global__ __launch_bounds__(256) void k_disp_mask(long long n, int D, int mode, const float *__restrict__ disp,
                                                   const int32_t *__restrict__ d_ref,
                                                   const int32_t *__restrict__ d_tar,
                                                   const uint8_t *__restrict__ code_ref,
                                                   const uint8_t *__restrict__ code_tar,
                                                   float *__restrict__ disp_lr) {
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const bool cons = lr_consistent(mode, D, p, d_ref[p], d_tar, code_ref, code_tar);
    disp_lr[p] = cons ? disp[p] : quiet_nan();
}

// ---------------------------------------------------------------------------
// background fill: one 256-thread block per row, the row in chunks of 256 columns.
// "Nearest valid column <= x" is an inclusive max-scan of (valid ? x : -1), "nearest
// valid column >= x" the mirrored (suffix) min-scan of (valid ? x : INT_MAX): wave64
// shuffles inside a wave, the four wave totals and the carry of the chunks already
// scanned through LDS.  Every thread of the block runs every shuffle and barrier: a
// tail lane (x >= W) takes part as an invalid pixel and only skips its load and store.
// ---------------------------------------------------------------------------
constexpr int kNoLeft = -1;
constexpr int kNoRight = 0x7fffffff;

__device__ __forceinline__ int wave_prefix_max(int v, int lane) {
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
        const int o = __shfl_up(v, off, kWave);
        if (lane >= off) v = o > v ? o : v;
    }
    return v;
}

__device__ __forceinline__ int wave_suffix_min(int v, int lane) {
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
        const int o = __shfl_down(v, off, kWave);
        if (lane + off < kWave) v = o < v ? o : v;
    }
    return v;
}

__global__ __launch_bounds__(kFillThreads) void k_disp_fill(int W, const float *__restrict__ in,
                                                            float *__restrict__ out) {
    __shared__ int s_wave[kFillWaves];
    __shared__ int s_carry;
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const long long row = (long long)blockIdx.x * W;
    const float *src = in + row;
    float *dst = out + row;
    const int nchunks = (W + kFillThreads - 1) / kFillThreads;

    // right to left: out[x] = the value at the nearest valid column >= x (NaN: none)
    if (tid == 0) s_carry = kNoRight;
    __syncthreads();
    for (int ch = nchunks - 1; ch >= 0; --ch) {
        const int x = ch * kFillThreads + tid;
        const bool in_row = x < W;
        const float v = in_row ? src[x] : quiet_nan();
        const bool valid = v == v;
        int r = wave_suffix_min(valid ? x : kNoRight, lane);
        if (lane == 0) s_wave[wave] = r;
        __syncthreads();
        int beyond = s_carry, total = s_carry;
#pragma unroll
        for (int w = 0; w < kFillWaves; ++w) {
            const int t = s_wave[w];
            total = t < total ? t : total;
            if (w > wave) beyond = t < beyond ? t : beyond;
        }
        r = beyond < r ? beyond : r;
        if (in_row) dst[x] = valid ? v : (r != kNoRight ? src[r] : quiet_nan());
        __syncthreads();
        if (tid == 0) s_carry = total;
    }
    __syncthreads();

    // left to right: the nearest valid column <= x, and the fill rule.  Thread tid
    // reads back the out[x] it wrote itself in the first sweep (same chunking).
    if (tid == 0) s_carry = kNoLeft;
    __syncthreads();
    for (int ch = 0; ch < nchunks; ++ch) {
        const int x = ch * kFillThreads + tid;
        const bool in_row = x < W;
        const float v = in_row ? src[x] : quiet_nan();
        const bool valid = v == v;
        int l = wave_prefix_max(valid ? x : kNoLeft, lane);
        if (lane == kWave - 1) s_wave[wave] = l;
        __syncthreads();
        int before = s_carry, total = s_carry;
#pragma unroll
        for (int w = 0; w < kFillWaves; ++w) {
            const int t = s_wave[w];
            total = t > total ? t : total;
            if (w < wave) before = t > before ? t : before;
        }
        l = before > l ? before : l;
        if (in_row && !valid) {
            const float rv = dst[x];
            const bool has_r = rv == rv, has_l = l != kNoLeft;
            float f = 0.0f;
            if (has_l) {
                const float lv = src[l];
                f = has_r ? (lv < rv ? lv : rv) : lv;
            } else if (has_r) {
                f = rv;
            }
            dst[x] = f;
        }
        __syncthreads();
        if (tid == 0) s_carry = total;
    }
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

}  // namespace
}  // namespace asw

using namespace asw;

#define ASW_CHECK_PARAMS(p)                 \
    do {                                    \
        const int _s = asw_params_check(p); \
        if (_s != ASW_OK) return _s;        \
    } while (0)

extern "C" {

int asw_subpixel(const asw_params *p, const float *cost, const int32_t *d_ref, float *disp, void *stream) {
    ASW_CHECK_PARAMS(p);
    if (p->d_begin != 0 || d_end_of_p(p) != p->ndisp) return ASW_E_INVALID;  // sharded: asw_subpixel_local & co.
    if (!cost || !d_ref || !disp) return ASW_E_INVALID;
    const long long n = (long long)p->width * p->height;
    hipLaunchKernelGGL(k_subpixel, pixel_grid(n), dim3(256), 0, (hipStream_t)stream, n, p->ndisp, asw_disp_pitch(p),
                       cost, d_ref, disp);
    return finish_launch();
}

int asw_subpixel_local(const asw_params *p, const float *cost, const int64_t *key_global, float *nb, void *stream) {
    ASW_CHECK_PARAMS(p);
    if (!cost || !key_global || !nb) return ASW_E_INVALID;
    const long long n = (long long)p->width * p->height;
    hipLaunchKernelGGL(k_subpixel_local, pixel_grid(n), dim3(256), 0, (hipStream_t)stream, n, p->ndisp,
                       asw_disp_pitch(p), p->d_begin, d_end_of_p(p), cost,
                       reinterpret_cast<const long long *>(key_global), nb);
    return finish_launch();
}

int asw_subpixel_finalize(const asw_params *p, const int64_t *key_global, const float *nb, float *disp,
                          void *stream) {
    ASW_CHECK_PARAMS(p);
    if (!key_global || !nb || !disp) return ASW_E_INVALID;
    const long long n = (long long)p->width * p->height;
    hipLaunchKernelGGL(k_subpixel_finalize, pixel_grid(n), dim3(256), 0, (hipStream_t)stream, n, p->ndisp,
                       reinterpret_cast<const long long *>(key_global), nb, disp);
    return finish_launch();
}

int asw_disp_mask(const asw_params *p, const float *disp, const int32_t *d_ref, const int32_t *d_tar,
                  const uint8_t *code_ref, const uint8_t *code_tar, float *disp_lr, void *stream) {
    ASW_CHECK_PARAMS(p);
    if (!disp || !d_ref || !d_tar || !disp_lr) return ASW_E_INVALID;
    if (p->lr_mode == ASW_LR_U8 && (!code_ref || !code_tar)) return ASW_E_INVALID;
    const long long n = (long long)p->width * p->height;
    hipLaunchKernelGGL(k_disp_mask, pixel_grid(n), dim3(256), 0, (hipStream_t)stream, n, p->ndisp, p->lr_mode, disp,
                       d_ref, d_tar, code_ref, code_tar, disp_lr);
    return finish_launch();
}

int asw_disp_fill(const asw_params *p, const float *disp_lr, float *disp_filled, void *stream) {
    ASW_CHECK_PARAMS(p);
    if (!disp_lr || !disp_filled || disp_lr == disp_filled) return ASW_E_INVALID;
    hipLaunchKernelGGL(k_disp_fill, dim3((unsigned)p->height), dim3(kFillThreads), 0, (hipStream_t)stream, p->width,
                       disp_lr, disp_filled);
    return finish_launch();
}

}  // extern "C"
