// asw_cross.hip — the reference's cross-based matcher with orthogonal integral images
// (main.cpp:243-411; K/median.cl, cross.cl, aggregation.cl, integral_h.cl, oii_hcross.cl,
// integral_v.cl, oii_vcross.cl, init_disparity.cl, disparity.cl), one entry point per
// reference kernel (include/asw.h §Cross-based).
//
// Every float operation is an IEEE float32 one in the reference's order
// (-ffp-contract=off, `/` correctly rounded).  The two integrals add serially from the
// image edge: a tree or wave scan would round differently.  The [H][W][Dp] layout makes
// the serial order cheap: a wave holds 64 consecutive planes in its lanes and walks x
// (or y), one coalesced 256-byte load and store per step.
#include <hip/hip_runtime.h>

#include "asw_common.h"

namespace asw {
namespace {

static_assert((char)-1 < 0, "the arm maps are signed bytes (char4)");

constexpr int kIntegralUnroll = 8;  // loads in flight ahead of the add chain
constexpr int kVoteWaves = 4;       // pixels per vote block (one wave each)
constexpr int kVoteBins = 256;      // ndisp <= 256

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__device__ __forceinline__ void cswap(int &a, int &b) {
    const int lo = min(a, b), hi = max(a, b);
    a = lo;
    b = hi;
}

// exact median of 9 (Paeth's exchange network, as k_median3 of asw_refine.hip)
__device__ __forceinline__ int median9(int v[9]) {
    cswap(v[1], v[2]); cswap(v[4], v[5]); cswap(v[7], v[8]);
    cswap(v[0], v[1]); cswap(v[3], v[4]); cswap(v[6], v[7]);
    cswap(v[1], v[2]); cswap(v[4], v[5]); cswap(v[7], v[8]);
    cswap(v[0], v[3]); cswap(v[5], v[8]); cswap(v[4], v[7]);
    cswap(v[3], v[6]); cswap(v[1], v[4]); cswap(v[2], v[5]);
    cswap(v[4], v[7]); cswap(v[4], v[2]); cswap(v[6], v[4]);
    cswap(v[4], v[2]);
    return v[4];
}

// Median (K/median.cl:58-88) of an RGBA8 image: per channel, clamp-to-edge, alpha 255
__global__ __launch_bounds__(256) void k_median3_rgba(const uchar4 *__restrict__ in, int W, int H,
                                                      uchar4 *__restrict__ out) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= W) return;
    int r[9], g[9], b[9];
    int n = 0;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            const uchar4 v = in[(long long)clampi(y + dy, 0, H - 1) * W + clampi(x + dx, 0, W - 1)];
            r[n] = v.x;
            g[n] = v.y;
            b[n] = v.z;
            ++n;
        }
    out[(long long)y * W + x] =
        make_uchar4((unsigned char)median9(r), (unsigned char)median9(g), (unsigned char)median9(b), 255);
}

// one arm of Cross (K/cross.cl:3-82): k = 1..arm_max tests the pixel at distance k+1
// against the anchor; accepted only inside the image, within one step of the arm so far
// and with every channel within tau
__device__ __forceinline__ int cross_arm(const uchar4 *__restrict__ img, int W, int H, int x, int y, int dx, int dy,
                                         int arm_max, int tau, uchar4 c) {
    int a = 1;
    for (int k = 1; k <= arm_max; ++k) {
        if (k - a > 1) break;  // two consecutive failures: nothing later can be accepted
        const int qx = x + (k + 1) * dx, qy = y + (k + 1) * dy;
        if (qx < 0 || qx >= W || qy < 0 || qy >= H) break;  // and stays outside from here on
        const uchar4 q = img[(long long)qy * W + qx];
        const int dr = abs((int)q.x - (int)c.x), dg = abs((int)q.y - (int)c.y), db = abs((int)q.z - (int)c.z);
        if (dr <= tau && dg <= tau && db <= tau) a = k;
    }
    return a;
}

__global__ __launch_bounds__(256) void k_cross_arms(const uchar4 *__restrict__ img, int W, int H, int arm_max,
                                                    int tau, char4 *__restrict__ arms) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= W) return;
    const uchar4 c = img[(long long)y * W + x];
    const int hm = cross_arm(img, W, H, x, y, -1, 0, arm_max, tau, c);
    const int hp = cross_arm(img, W, H, x, y, 1, 0, arm_max, tau, c);
    const int vm = cross_arm(img, W, H, x, y, 0, -1, arm_max, tau, c);
    const int vp = cross_arm(img, W, H, x, y, 0, 1, arm_max, tau, c);
    arms[(long long)y * W + x] = make_char4((signed char)-hm, (signed char)hp, (signed char)-vm, (signed char)vp);
}

__device__ __forceinline__ float unorm(unsigned char c) { return (float)c / 255.0f; }

// Aggregation (K/aggregation.cl): lane per (pixel, plane) of [H][W][Dp]; padding planes 0
__global__ __launch_bounds__(256) void k_cross_cost(long long total, int W, int D, int Dp,
                                                    const uchar4 *__restrict__ ml, const uchar4 *__restrict__ mr,
                                                    float *__restrict__ cost) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const long long pix = i / Dp;
    const int d = (int)(i - pix * Dp);
    float v = 0.0f;
    if (d < D) {
        const int x = (int)(pix % W);
        const int xr = x - d > 0 ? x - d : 0;
        const uchar4 l = ml[pix], r = mr[pix - x + xr];
        v = (fabsf(unorm(l.x) - unorm(r.x)) + fabsf(unorm(l.y) - unorm(r.y))) + fabsf(unorm(l.z) - unorm(r.z));
    }
    cost[i] = v;
}

// Integral_h / Integral_v (K/integral_h.cl, K/integral_v.cl), in place.  Wave w owns the
// 64 planes [64 c, 64 c + 64) of line l (a row for H, a column for V), w = l * (Dp/64) + c,
// and adds serially along the line: `count` steps of `step` floats from `base`.  Lanes of
// padding planes neither load nor store.  kIntegralUnroll loads are issued before the
// dependent adds of a group.
__global__ __launch_bounds__(256) void k_cross_integral(float *__restrict__ vol, long long nwaves, int chunks, int D,
                                                        long long line_stride, long long step, int count) {
    const long long w = (long long)blockIdx.x * (blockDim.x / kWave) + threadIdx.x / kWave;
    if (w >= nwaves) return;
    const int lane = threadIdx.x & (kWave - 1);
    const long long line = w / chunks;
    const int plane = (int)(w - line * chunks) * kWave + lane;
    if (plane >= D) return;
    float *p = vol + line * line_stride + plane;
    float acc = 0.0f;
    int i = 0;
    for (; i + kIntegralUnroll <= count; i += kIntegralUnroll) {
        float v[kIntegralUnroll];
#pragma unroll
        for (int u = 0; u < kIntegralUnroll; ++u) v[u] = p[(long long)u * step];
#pragma unroll
        for (int u = 0; u < kIntegralUnroll; ++u) {
            acc = acc + v[u];
            p[(long long)u * step] = acc;
        }
        p += (long long)kIntegralUnroll * step;
    }
    for (; i < count; ++i) {
        acc = acc + *p;
        *p = acc;
        p += step;
    }
}

// Oii_hcross / Oii_vcross (K/oii_hcross.cl:13-31, K/oii_vcross.cl): lane per (pixel, plane).
// The combined arm is max of the minus arms and min of the plus arms of L(x, y) and
// R(max(x-d, 0), y); the reference's off-by-one at the lower end and its division by
// hp - hm (not the pixel count) are kept.  Both window ends are clamped into the line, so
// no arm value can take a read outside the volume.  Padding planes: written 0, never read.
template <int DIR>
__global__ __launch_bounds__(256) void k_cross_oii(long long total, int W, int H, int D, int Dp,
                                                   const char4 *__restrict__ al, const char4 *__restrict__ ar,
                                                   const float *__restrict__ in, float *__restrict__ out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const long long pix = i / Dp;
    const int d = (int)(i - pix * Dp);
    float v = 0.0f;
    if (d < D) {
        const int x = (int)(pix % W), y = (int)(pix / W);
        const int xr = x - d > 0 ? x - d : 0;
        const char4 l = al[pix], r = ar[pix - x + xr];
        const int lm = DIR == ASW_DIR_H ? l.x : l.z, lp = DIR == ASW_DIR_H ? l.y : l.w;
        const int rm = DIR == ASW_DIR_H ? r.x : r.z, rp = DIR == ASW_DIR_H ? r.y : r.w;
        const int m = rm > lm ? rm : lm, pl = rp < lp ? rp : lp;
        long long hi, lo;
        if (DIR == ASW_DIR_H) {
            hi = pix - x + clampi(x + pl, 0, W - 1);
            lo = pix - x + clampi(x + m - 1, 0, W - 1);
        } else {
            hi = (long long)clampi(y + pl, 0, H - 1) * W + x;
            lo = (long long)clampi(y + m - 1, 0, H - 1) * W + x;
        }
        v = (in[hi * Dp + d] - in[lo * Dp + d]) / (float)(pl - m);
    }
    out[i] = v;
}

// Init_disparity (K/init_disparity.cl): wave per pixel, lanes over the planes.  The first
// strict minimum over d is the smallest index that attains the minimum: a lane keeps the
// first of its own planes (ascending), the wave keeps the smaller index among equal values.
__global__ __launch_bounds__(256) void k_cross_init(long long npix, int D, int Dp, const float *__restrict__ vol,
                                                    int32_t *__restrict__ d0, uint8_t *__restrict__ code0) {
    const long long pix = (long long)blockIdx.x * (blockDim.x / kWave) + threadIdx.x / kWave;
    if (pix >= npix) return;
    const int lane = threadIdx.x & (kWave - 1);
    const float *c = vol + pix * Dp;
    float best = __uint_as_float(0x7f800000u);
    int bi = 0x7fffffff;
    for (int d = lane; d < D; d += kWave) {
        const float v = c[d];
        if (bi == 0x7fffffff || v < best) {
            best = v;
            bi = d;
        }
    }
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) {
        const float ov = __shfl_xor(best, off, kWave);
        const int oi = __shfl_xor(bi, off, kWave);
        const bool take = oi != 0x7fffffff && (bi == 0x7fffffff || ov < best || (ov == best && oi < bi));
        if (take) {
            best = ov;
            bi = oi;
        }
    }
    if (lane == 0) {
        if (d0) d0[pix] = bi;
        if (code0) code0[pix] = (uint8_t)code_u8(bi, D);
    }
}

// Disparity (K/disparity.cl): the histogram of the initial codes over the pixel's cross
// region, the last bin with the largest count wins.  One wave per pixel, a per-wave
// histogram in LDS (ds_add_u32; integer counts: any order is exact).  The wave works on
// four region rows at a time, 16 lanes striding over the columns of each row.  Every
// thread of the block reaches both barriers: a wave without a pixel only skips the work.
__global__ __launch_bounds__(kVoteWaves *kWave) void k_cross_vote(int W, int H, int D,
                                                                  const uint8_t *__restrict__ code0,
                                                                  const char4 *__restrict__ arms,
                                                                  int32_t *__restrict__ d1,
                                                                  uint8_t *__restrict__ code1) {
    __shared__ unsigned int s_tab[kVoteWaves][kVoteBins];
    const int wave = threadIdx.x / kWave, lane = threadIdx.x & (kWave - 1);
    const long long npix = (long long)W * H;
    const long long pix = (long long)blockIdx.x * kVoteWaves + wave;
    const bool live = pix < npix;
    unsigned int *tab = s_tab[wave];
    for (int b = lane; b < kVoteBins; b += kWave) tab[b] = 0u;
    __syncthreads();
    if (live) {
        const int x = (int)(pix % W), y = (int)(pix / W);
        const char4 own = arms[pix];
        const float scale = (float)(D - 1);
        const int sub = lane >> 4, col = lane & 15;
        for (int i = own.z + sub; i <= own.w; i += 4) {
            const int yc = clampi(y + i, 0, H - 1);
            const long long row = (long long)yc * W;
            const char4 a = arms[row + x];
            for (int j = a.x + col; j <= a.y; j += 16) {
                const unsigned char c = code0[row + clampi(x + j, 0, W - 1)];
                int bin = (int)(((float)c / 255.0f) * scale);
                bin = clampi(bin, 0, kVoteBins - 1);
                atomicAdd(&tab[bin], 1u);
            }
        }
    }
    __syncthreads();
    if (live) {
        int best = -1, bi = 0;
        for (int b = lane; b < D; b += kWave) {
            const int n = (int)tab[b];
            if (n >= best) {
                best = n;
                bi = b;
            }
        }
#pragma unroll
        for (int off = kWave / 2; off > 0; off >>= 1) {
            const int on = __shfl_xor(best, off, kWave);
            const int oi = __shfl_xor(bi, off, kWave);
            if (on > best || (on == best && oi > bi)) {
                best = on;
                bi = oi;
            }
        }
        if (lane == 0) {
            if (d1) d1[pix] = bi;
            if (code1) code1[pix] = (uint8_t)code_u8(bi, D);
        }
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

// whole-volume p with 8-bit codes: what every volume stage of the matcher needs
inline int cross_shape_check(const asw_params *p) {
    const int s = asw_params_check(p);
    if (s != ASW_OK) return s;
    if (p->d_begin != 0 || d_end_of_p(p) != p->ndisp) return ASW_E_INVALID;
    if (p->ndisp < 2 || p->ndisp > 256) return ASW_E_UNSUPPORTED;
    return ASW_OK;
}

inline dim3 row_grid(const asw_params *p) { return dim3((unsigned)((p->width + 255) / 256), (unsigned)p->height); }

// blocks of kFlatThreads threads over n items; ASW_E_UNSUPPORTED past the grid limit: a
// dispatch holds its work-item count per dimension in 32 bits, so blocks * kFlatThreads
// must stay below 2^32 (a launch past it fails, it never runs with a wrapped grid)
constexpr long long kFlatThreads = 256;
inline int flat_grid(long long n, long long per_block, dim3 *g) {
    const long long blocks = (n + per_block - 1) / per_block;
    if (blocks * kFlatThreads > 0xffffffffLL) return ASW_E_UNSUPPORTED;
    *g = dim3((unsigned)blocks);
    return ASW_OK;
}

}  // namespace
}  // namespace asw

using namespace asw;

#define ASW_CROSS_CHECK(expr)        \
    do {                             \
        const int _s = (expr);       \
        if (_s != ASW_OK) return _s; \
    } while (0)

extern "C" {

void asw_cross_params_default(asw_cross_params *cp) {
    if (!cp) return;
    cp->arm_max = 25;  // K/cross.cl:32-80: 25 unrolled steps
    cp->tau = 25;      // K/cross.cl:11-13: |delta| / 255 < 0.10f  <=>  |delta| <= 25
}

int asw_cross_params_check(const asw_params *p, const asw_cross_params *cp) {
    if (!p || !cp) return ASW_E_INVALID;
    ASW_CROSS_CHECK(cross_shape_check(p));
    if (cp->arm_max < 1 || cp->arm_max > 127) return ASW_E_INVALID;  // signed bytes
    if (cp->tau < 0 || cp->tau > 255) return ASW_E_INVALID;
    return ASW_OK;
}

size_t asw_cross_arm_bytes(const asw_params *p) {
    if (!p || p->width <= 0 || p->height <= 0) return 0;
    return (size_t)p->width * (size_t)p->height * 4;
}

int asw_median3_rgba(const asw_params *p, const uint8_t *in_rgba, uint8_t *out_rgba, void *stream) {
    if (!p) return ASW_E_INVALID;
    ASW_CROSS_CHECK(asw_params_check(p));
    if (!in_rgba || !out_rgba || in_rgba == out_rgba) return ASW_E_INVALID;
    hipLaunchKernelGGL(k_median3_rgba, row_grid(p), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const uchar4 *>(in_rgba), p->width, p->height,
                       reinterpret_cast<uchar4 *>(out_rgba));
    return finish_launch();
}

int asw_cross_arms(const asw_params *p, const asw_cross_params *cp, const uint8_t *med_rgba, int8_t *arms,
                   void *stream) {
    ASW_CROSS_CHECK(asw_cross_params_check(p, cp));
    if (!med_rgba || !arms) return ASW_E_INVALID;
    hipLaunchKernelGGL(k_cross_arms, row_grid(p), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const uchar4 *>(med_rgba), p->width, p->height, cp->arm_max, cp->tau,
                       reinterpret_cast<char4 *>(arms));
    return finish_launch();
}

int asw_cross_cost(const asw_params *p, const uint8_t *med_left_rgba, const uint8_t *med_right_rgba, float *cost,
                   void *stream) {
    if (!p) return ASW_E_INVALID;
    ASW_CROSS_CHECK(cross_shape_check(p));
    if (!med_left_rgba || !med_right_rgba || !cost) return ASW_E_INVALID;
    const int Dp = asw_disp_pitch(p);
    const long long total = (long long)p->width * p->height * Dp;
    dim3 g;
    ASW_CROSS_CHECK(flat_grid(total, 256, &g));
    hipLaunchKernelGGL(k_cross_cost, g, dim3(256), 0, (hipStream_t)stream, total, p->width, p->ndisp, Dp,
                       reinterpret_cast<const uchar4 *>(med_left_rgba),
                       reinterpret_cast<const uchar4 *>(med_right_rgba), cost);
    return finish_launch();
}

int asw_cross_integral(const asw_params *p, int dir, float *vol, void *stream) {
    if (!p) return ASW_E_INVALID;
    ASW_CROSS_CHECK(cross_shape_check(p));
    if (!vol || (dir != ASW_DIR_H && dir != ASW_DIR_V)) return ASW_E_INVALID;
    const int Dp = asw_disp_pitch(p), chunks = Dp / kWave;
    const long long W = p->width, H = p->height;
    // H: line = row y, steps of one pixel; V: line = column x, steps of one row
    const long long lines = dir == ASW_DIR_H ? H : W;
    const long long line_stride = dir == ASW_DIR_H ? W * Dp : Dp;
    const long long step = dir == ASW_DIR_H ? Dp : W * Dp;
    const int count = dir == ASW_DIR_H ? p->width : p->height;
    const long long nwaves = lines * chunks;
    dim3 g;
    ASW_CROSS_CHECK(flat_grid(nwaves, 256 / kWave, &g));
    hipLaunchKernelGGL(k_cross_integral, g, dim3(256), 0, (hipStream_t)stream, vol, nwaves, chunks, p->ndisp,
                       line_stride, step, count);
    return finish_launch();
}

int asw_cross_oii(const asw_params *p, int dir, const int8_t *arms_left, const int8_t *arms_right, const float *in,
                  float *out, void *stream) {
    if (!p) return ASW_E_INVALID;
    ASW_CROSS_CHECK(cross_shape_check(p));
    if (!arms_left || !arms_right || !in || !out || in == out) return ASW_E_INVALID;
    if (dir != ASW_DIR_H && dir != ASW_DIR_V) return ASW_E_INVALID;
    const int Dp = asw_disp_pitch(p);
    const long long total = (long long)p->width * p->height * Dp;
    dim3 g;
    ASW_CROSS_CHECK(flat_grid(total, 256, &g));
    const char4 *al = reinterpret_cast<const char4 *>(arms_left), *ar = reinterpret_cast<const char4 *>(arms_right);
    if (dir == ASW_DIR_H)
        hipLaunchKernelGGL(k_cross_oii<ASW_DIR_H>, g, dim3(256), 0, (hipStream_t)stream, total, p->width, p->height,
                           p->ndisp, Dp, al, ar, in, out);
    else
        hipLaunchKernelGGL(k_cross_oii<ASW_DIR_V>, g, dim3(256), 0, (hipStream_t)stream, total, p->width, p->height,
                           p->ndisp, Dp, al, ar, in, out);
    return finish_launch();
}

int asw_cross_init(const asw_params *p, const float *vol, int32_t *d0, uint8_t *code0, void *stream) {
    if (!p) return ASW_E_INVALID;
    ASW_CROSS_CHECK(cross_shape_check(p));
    if (!vol || (!d0 && !code0)) return ASW_E_INVALID;
    const long long npix = (long long)p->width * p->height;
    dim3 g;
    ASW_CROSS_CHECK(flat_grid(npix, 256 / kWave, &g));
    hipLaunchKernelGGL(k_cross_init, g, dim3(256), 0, (hipStream_t)stream, npix, p->ndisp, asw_disp_pitch(p), vol, d0,
                       code0);
    return finish_launch();
}

int asw_cross_vote(const asw_params *p, const uint8_t *code0, const int8_t *arms_left, int32_t *d1, uint8_t *code1,
                   void *stream) {
    if (!p) return ASW_E_INVALID;
    ASW_CROSS_CHECK(cross_shape_check(p));
    if (!code0 || !arms_left || (!d1 && !code1) || code0 == code1) return ASW_E_INVALID;
    const long long npix = (long long)p->width * p->height;
    dim3 g;
    ASW_CROSS_CHECK(flat_grid(npix, kVoteWaves, &g));
    hipLaunchKernelGGL(k_cross_vote, g, dim3(kVoteWaves * kWave), 0, (hipStream_t)stream, p->width, p->height,
                       p->ndisp, code0, reinterpret_cast<const char4 *>(arms_left), d1, code1);
    return finish_launch();
}

}  // extern "C"
