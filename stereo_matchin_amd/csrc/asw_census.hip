// asw_census.hip — the census / AD-census matching cost (include/asw.h §census,
// DESIGN.md §Census).  No reference counterpart: the reference's only raw cost is the
// RGB absolute difference (K/asw_aggr.cl), which assumes both cameras see the same
// brightness.  The census code of a pixel depends only on the ORDER of the lumas in its
// window, so a gain or offset between the two views leaves the Hamming cost unchanged.
//
// Every operation is an integer one, except the float form's one multiply and one add
// (-ffp-contract=off: never fused).  Two kernels:
//   k_census       luma + census code of one image, uint64 [H][W]
//   k_census_cost  the cost volume [H][W][Dp] (float, or uint16 for the first V pass
//                  asw_aggregate_pass_den16), k_raw_cost's structure with the census
//                  codes staged next to the right-image pixels
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "asw_common.h"

namespace asw {
namespace {

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// ---------------------------------------------------------------------------
// Census transform.  Block = 4 waves on a 64 x 16 pixel tile; its lumas
// Y = (77 R + 150 G + 29 B + 128) >> 8 with a halo of RW columns and RH rows on each
// side (clamp-to-edge, so an image smaller than the window needs no special case) are
// staged once in LDS as bytes: the lanes of a read are consecutive bytes of one tile row
// (four lanes per dword: broadcast, no bank conflict).  A lane owns one column and four
// rows of the tile.  The window is a template parameter: the (2RW+1)(2RH+1) - 1
// comparisons unroll, each bit position is a constant, the code is built in two 32-bit
// halves and leaves as one 8-byte store.  The only barrier precedes any divergent flow.
// ---------------------------------------------------------------------------
constexpr int kCenTX = 64, kCenTY = 16;
template <int RW, int RH>
__global__ __launch_bounds__(256) void k_census(const uchar4 *__restrict__ img, int W, int H,
                                                unsigned long long *__restrict__ out) {
    static_assert(RW >= 1 && RW <= 4 && RH >= 1 && RH <= 4, "halo of at most 4 columns and 4 rows");
    static_assert((2 * RW + 1) * (2 * RH + 1) - 1 <= 64, "the code is 64 bits");
    constexpr int TW = kCenTX + 2 * RW, TH = kCenTY + 2 * RH;
    __shared__ unsigned char luma[TH * TW];
    const int x0 = blockIdx.x * kCenTX, y0 = blockIdx.y * kCenTY;
    for (int t = threadIdx.x; t < TH * TW; t += 256) {
        const int r = t / TW, c = t - r * TW;
        const int gx = clampi(x0 - RW + c, 0, W - 1), gy = clampi(y0 - RH + r, 0, H - 1);
        const uchar4 v = img[(long long)gy * W + gx];
        luma[t] = (unsigned char)((77u * v.x + 150u * v.y + 29u * v.z + 128u) >> 8);
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x = x0 + lane;
    if (x >= W) return;
#pragma unroll
    for (int j = 0; j < kCenTY / 4; ++j) {
        const int ly = wave * (kCenTY / 4) + j, y = y0 + ly;
        if (y >= H) break;
        // tile position of (x, y): column lane + RW, row ly + RH
        const unsigned char *row0 = &luma[ly * TW + lane];
        const unsigned c = row0[RH * TW + RW];
        unsigned lo = 0u, hi = 0u;
        int n = 0;
#pragma unroll
        for (int dy = 0; dy <= 2 * RH; ++dy)
#pragma unroll
            for (int dx = 0; dx <= 2 * RW; ++dx) {
                if (dy == RH && dx == RW) continue;  // the centre is skipped
                const unsigned bit = row0[dy * TW + dx] < c ? 1u : 0u;  // strict
                if (n < 32) lo |= bit << (n & 31);
                else hi |= bit << (n & 31);
                ++n;
            }
        out[(long long)y * W + x] = ((unsigned long long)hi << 32) | lo;
    }
}

// ---------------------------------------------------------------------------
// Census / AD-census cost: k_raw_cost (asw_kernels.hip) with twelve bytes per staged
// element.  Block = 4 waves on row blockIdx.y, 4 * 16 consecutive pixels; the right-image
// elements they reach (columns x - d, clamped to [0, W-1]: xr = max(x - d, 0)) are staged
// once in LDS as three dword arrays (pixel, low and high half of the census code), each in
// k_raw_cost's 4-phase layout: element t at (t & 3) * s4 + (t >> 2).  The lanes of a read
// are 4 elements apart (planes 4q..4q+3 of lane q), so they read consecutive dwords of one
// phase, and s4 = 8 (mod 32) spreads the staging writes of 32 consecutive t over 32 banks;
// each array starts a multiple of 32 dwords after the one before, so all three behave alike.
// Per element: v_sad_u8 for the AD, two xors and two accumulating popcounts for the
// Hamming distance, the clamp and one integer multiply-add per weight.  Every store is a
// float4 (or 4 x uint16) per lane, nontemporal: the volume is a write-once stream.
// ---------------------------------------------------------------------------
constexpr int kCcPPW = 16;            // pixels per wave
constexpr int kCcSpan = 4 * kCcPPW;   // pixels per block
__host__ __device__ constexpr int cc_phase_stride(int Dp) { return ((kCcSpan + Dp - 1 + 3) / 4 + 31) / 32 * 32 + 8; }

template <bool U16>
__global__ __launch_bounds__(256) void k_census_cost(const uchar4 *__restrict__ L, const uchar4 *__restrict__ R,
                                                      const unsigned long long *__restrict__ CL,
                                                      const unsigned long long *__restrict__ CR,
                                                      void *__restrict__ cost_v, int W, int Dp, int nloc, int d_begin,
                                                      float tau, unsigned tau_u, unsigned wa, unsigned wc) {
    using f4 = float __attribute__((ext_vector_type(4)));
    using u4 = unsigned short __attribute__((ext_vector_type(4)));
    extern __shared__ unsigned stage[];
    const int s4 = cc_phase_stride(Dp);
    unsigned *rpix = stage, *rlo = stage + 4 * s4, *rhi = stage + 8 * s4;
    auto slot = [s4](int t) __attribute__((always_inline)) { return (t & 3) * s4 + (t >> 2); };
    const int y = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long row = (long long)y * W;
    const unsigned *Lrow = reinterpret_cast<const unsigned *>(L + row);
    const unsigned *Rrow = reinterpret_cast<const unsigned *>(R + row);
    const uint2 *CLrow = reinterpret_cast<const uint2 *>(CL + row);
    const uint2 *CRrow = reinterpret_cast<const uint2 *>(CR + row);
    const int x0 = blockIdx.x * kCcSpan;
    const int xlo = x0 - (d_begin + Dp - 1);  // smallest x - d of the block (staged clamped to [0, W-1])
    const int nr = kCcSpan + Dp - 1;
    for (int t = threadIdx.x; t < nr; t += 256) {
        const int xr = clampi(xlo + t, 0, W - 1);
        const uint2 cen = CRrow[xr];
        const int s = slot(t);
        rpix[s] = Rrow[xr] & 0xFFFFFFu;  // (alpha cleared: v_sad_u8 then sums |dR| + |dG| + |dB|)
        rlo[s] = cen.x;
        rhi[s] = cen.y;
    }
    const int xa = x0 + wave * kCcPPW;
    const int xb = min(xa + kCcPPW, W);
    // the wave's 16 left pixels and codes in one load each (lane i: pixel xa + i), taken by
    // the lanes that need them through lane permutes
    const int xl = min(xa + (lane & (kCcPPW - 1)), W - 1);
    const unsigned lw = Lrow[xl] & 0xFFFFFFu;
    const uint2 lcen = CLrow[xl];
    __syncthreads();
    const int nq = Dp >> 2;
    // Dp < 256 (narrow shards): 64/nq pixels per wave iteration, so no lane idles
    const int ppi = (nq < 64 && 64 % nq == 0) ? 64 / nq : 1;
    const int lpp = ppi > 1 ? nq : 64;  // lanes per pixel
    // (a uniform trip count: the permutes read lanes that must all be active; Dp is 32 or
    // a multiple of 64, so ppi <= 8 divides kCcPPW)
    for (int it = 0; it < kCcPPW / ppi; ++it) {
        const int x = xa + lane / lpp + it * ppi;
        const int src = min(x - xa, kCcPPW - 1);
        const unsigned l = (unsigned)__shfl((int)lw, src);
        const unsigned llo = (unsigned)__shfl((int)lcen.x, src), lhi = (unsigned)__shfl((int)lcen.y, src);
        if (x >= xb) continue;
        const long long e0 = (row + x) * Dp;  // first element of pixel x
        for (int q = lane % lpp; q < nq; q += lpp) {
            unsigned ad[4], wh[4];  // AD and w_c * ham of the four planes
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int s = slot(x - (d_begin + 4 * q + j) - xlo);  // = R(max(x-d, 0), y): the stage clamps
                ad[j] = __builtin_amdgcn_sad_u8(l, rpix[s], 0u);  // exact integer AD, <= 765
                wh[j] = wc * (unsigned)(__builtin_popcount(llo ^ rlo[s]) + __builtin_popcount(lhi ^ rhi[s]));
            }
            if constexpr (U16) {
                u4 h;
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    h[j] = 4 * q + j < nloc ? (unsigned short)(wa * min(ad[j], tau_u) + wh[j]) : (unsigned short)0;
                __builtin_nontemporal_store(h, &reinterpret_cast<u4 *>(static_cast<unsigned short *>(cost_v) + e0)[q]);
            } else {
                f4 v;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    // w_a = 0: the AD term is not formed and tau is not read
                    const float c = wa ? fminf((float)ad[j], tau) * (float)wa + (float)wh[j] : (float)wh[j];
                    v[j] = 4 * q + j < nloc ? c : 0.0f;
                }
                __builtin_nontemporal_store(v, &reinterpret_cast<f4 *>(static_cast<float *>(cost_v) + e0)[q]);
            }
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

bool window_size(int v) { return v == 3 || v == 5 || v == 7 || v == 9; }

// the uint16 form is the float form exactly: w_a = 0, or the truncated AD is an integer
bool census16_exact(const asw_params *p, const asw_census_params *cp) {
    return cp->ad_weight == 0 || p->tad_tau >= (float)kSadMax || p->tad_tau == floorf(p->tad_tau);
}

template <int RW>
int launch_census_rw(int rh, dim3 grid, hipStream_t st, const uchar4 *img, int W, int H, unsigned long long *out) {
    switch (rh) {
        case 1: hipLaunchKernelGGL((k_census<RW, 1>), grid, dim3(256), 0, st, img, W, H, out); break;
        case 2: hipLaunchKernelGGL((k_census<RW, 2>), grid, dim3(256), 0, st, img, W, H, out); break;
        case 3: hipLaunchKernelGGL((k_census<RW, 3>), grid, dim3(256), 0, st, img, W, H, out); break;
        case 4:
            if constexpr (RW < 4) hipLaunchKernelGGL((k_census<RW, 4>), grid, dim3(256), 0, st, img, W, H, out);
            else return ASW_E_INVALID;  // 9 x 9: 80 bits
            break;
        default: return ASW_E_INVALID;
    }
    return finish_launch();
}

int launch_census_cost(bool u16, const asw_params *p, const asw_census_params *cp, const uint8_t *left,
                       const uint8_t *right, const uint64_t *cl, const uint64_t *cr, void *cost, void *stream) {
    const int Dp = asw_disp_pitch(p);
    const dim3 grid((unsigned)((p->width + kCcSpan - 1) / kCcSpan), (unsigned)p->height);
    const size_t lds = (size_t)3 * 4 * cc_phase_stride(Dp) * sizeof(unsigned);  // 3 arrays of 4 phases
    if (lds > 64 * 1024) return ASW_E_UNSUPPORTED;
    const uchar4 *l = reinterpret_cast<const uchar4 *>(left), *r = reinterpret_cast<const uchar4 *>(right);
    const unsigned long long *ql = reinterpret_cast<const unsigned long long *>(cl),
                             *qr = reinterpret_cast<const unsigned long long *>(cr);
    const unsigned wa = (unsigned)cp->ad_weight, wc = (unsigned)cp->census_weight;
    // an integral tau below 765 clamps the integer AD (the uint16 form's domain); w_a = 0: unread
    const float tau = wa ? p->tad_tau : 0.0f;
    const unsigned tau_u = !wa ? 0u : (tau >= (float)kSadMax ? (unsigned)kSadMax : (unsigned)tau);
    const int nloc = d_end_of_p(p) - p->d_begin;
    if (u16)
        hipLaunchKernelGGL(k_census_cost<true>, grid, dim3(256), lds, (hipStream_t)stream, l, r, ql, qr, cost,
                           p->width, Dp, nloc, p->d_begin, tau, tau_u, wa, wc);
    else
        hipLaunchKernelGGL(k_census_cost<false>, grid, dim3(256), lds, (hipStream_t)stream, l, r, ql, qr, cost,
                           p->width, Dp, nloc, p->d_begin, tau, tau_u, wa, wc);
    return finish_launch();
}

}  // namespace

int census_cost16_check(const asw_params *p, const asw_census_params *cp) {
    if (!census16_exact(p, cp)) return ASW_E_UNSUPPORTED;
    const size_t lds = (size_t)3 * 4 * cc_phase_stride(asw_disp_pitch(p)) * sizeof(unsigned);
    return lds > 64 * 1024 ? ASW_E_UNSUPPORTED : ASW_OK;
}

}  // namespace asw

using namespace asw;

#define ASW_CENSUS_CHECK(expr)       \
    do {                             \
        const int _s = (expr);       \
        if (_s != ASW_OK) return _s; \
    } while (0)

extern "C" {

void asw_census_params_default(asw_census_params *cp) {
    if (!cp) return;
    cp->win_w = 9;  // 9 x 7: 62 bits
    cp->win_h = 7;
    cp->ad_weight = 1;
    cp->census_weight = 8;
}

int asw_census_params_check(const asw_params *p, const asw_census_params *cp) {
    if (!p || !cp) return ASW_E_INVALID;
    ASW_CENSUS_CHECK(asw_params_check(p));
    if (!window_size(cp->win_w) || !window_size(cp->win_h)) return ASW_E_INVALID;
    const int bits = cp->win_w * cp->win_h - 1;
    if (bits > 64) return ASW_E_INVALID;  // 9 x 9
    if (cp->ad_weight < 0 || cp->ad_weight > 64) return ASW_E_INVALID;
    if (cp->census_weight < 1 || cp->census_weight > 1024) return ASW_E_INVALID;
    int ad_max = 0;
    if (cp->ad_weight > 0) {
        if (!(p->tad_tau >= 0.0f)) return ASW_E_INVALID;
        ad_max = p->tad_tau >= (float)kSadMax ? kSadMax : (int)ceilf(p->tad_tau);
    }
    if (cp->ad_weight * ad_max + cp->census_weight * bits > 65535) return ASW_E_INVALID;  // the uint16 volume
    return ASW_OK;
}

size_t asw_census_bytes(const asw_params *p) {
    if (!p || p->width <= 0 || p->height <= 0) return 0;
    return (size_t)p->width * (size_t)p->height * 8;
}

int asw_census(const asw_params *p, const asw_census_params *cp, const uint8_t *img_rgba, uint64_t *census,
               void *stream) {
    ASW_CENSUS_CHECK(asw_census_params_check(p, cp));
    if (!img_rgba || !census) return ASW_E_INVALID;
    const dim3 grid((unsigned)((p->width + kCenTX - 1) / kCenTX), (unsigned)((p->height + kCenTY - 1) / kCenTY));
    const uchar4 *img = reinterpret_cast<const uchar4 *>(img_rgba);
    unsigned long long *out = reinterpret_cast<unsigned long long *>(census);
    const int rh = cp->win_h / 2;
    const hipStream_t st = (hipStream_t)stream;
    switch (cp->win_w / 2) {
        case 1: return launch_census_rw<1>(rh, grid, st, img, p->width, p->height, out);
        case 2: return launch_census_rw<2>(rh, grid, st, img, p->width, p->height, out);
        case 3: return launch_census_rw<3>(rh, grid, st, img, p->width, p->height, out);
        case 4: return launch_census_rw<4>(rh, grid, st, img, p->width, p->height, out);
        default: return ASW_E_INVALID;
    }
}

int asw_census_cost(const asw_params *p, const asw_census_params *cp, const uint8_t *left_rgba,
                    const uint8_t *right_rgba, const uint64_t *cen_left, const uint64_t *cen_right, float *cost,
                    void *stream) {
    ASW_CENSUS_CHECK(asw_census_params_check(p, cp));
    if (!left_rgba || !right_rgba || !cen_left || !cen_right || !cost) return ASW_E_INVALID;
    return launch_census_cost(false, p, cp, left_rgba, right_rgba, cen_left, cen_right, cost, stream);
}

int asw_census16_supported(const asw_params *p, const asw_census_params *cp) {
    if (asw_census_params_check(p, cp) != ASW_OK) return 0;
    // exact, and read by a ring-kernel first V pass (asw_aggregate_pass_den16)
    return census_cost16_check(p, cp) == ASW_OK && p->iters >= 1 && ring_taps(p->taps) ? 1 : 0;
}

int asw_census_cost16(const asw_params *p, const asw_census_params *cp, const uint8_t *left_rgba,
                      const uint8_t *right_rgba, const uint64_t *cen_left, const uint64_t *cen_right, uint16_t *cost,
                      void *stream) {
    ASW_CENSUS_CHECK(asw_census_params_check(p, cp));
    if (!left_rgba || !right_rgba || !cen_left || !cen_right || !cost) return ASW_E_INVALID;
    ASW_CENSUS_CHECK(census_cost16_check(p, cp));
    return launch_census_cost(true, p, cp, left_rgba, right_rgba, cen_left, cen_right, cost, stream);
}

}  // extern "C"
