// asw_refine_native.hip — the refinement loop of asw_refine.hip (main.cpp:540-623) on
// disparity INDICES: the reference feeds its disparities back through 8-bit images
// ((code/255)*(ndisp-1)), which collide above 256 levels and differ from the indices
// under ASW_LR_NATIVE.  Here the estimates are int32 index maps and the outputs uint16
// maps, at any ndisp <= 65535 (DESIGN.md §Native refinement).  asw_ref_h and the
// asw_WTA_REF scan (k_wta_scan<1>, asw_refine.hip) are shared with the 8-bit loop; this
// file holds the three stages that carried codes: the V estimate, the consistency
// write-back and the median.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "asw_common.h"

namespace asw {
namespace {

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// The V estimate (k_ref_v of asw_refine.hip with the decode replaced): per pixel, over
// the Tr vertical taps q = (x, clamp(y+i-Rr)): w = LUT[|dy|][SAD], Dv = (float)est[q],
// t = w*conf[q]; num = num + t*Dv; den = den + t  (num = den = 1e-5 on entry, i ascending).
// One lane per pixel of the flattened image: a wave's 64 pixels are consecutive in
// memory (they may wrap to the next row of a narrow image), so each tap's three loads
// (image, estimate, confidence: 4 bytes per lane each) are coalesced 256-byte rows.  The
// loads of kBatch taps are issued before their in-order sums.
constexpr int kBatch = 8;

__global__ __launch_bounds__(256) void k_ref_v_native(const uchar4 *__restrict__ img, const int32_t *__restrict__ est,
                                                      const float *__restrict__ conf, const float *__restrict__ lut,
                                                      int W, int H, int Tr, float *__restrict__ out) {
    const long long S = (long long)W * H;
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= S) return;
    const int y = (int)(p / W);
    const int x = (int)(p - (long long)y * W);
    const int Rr = Tr / 2;
    const uchar4 pc = img[p];
    float num = 0.00001f, den = 0.00001f;
    for (int i0 = 0; i0 < Tr; i0 += kBatch) {
        uchar4 qc[kBatch];
        int32_t e[kBatch];
        float f[kBatch];
        int dist[kBatch];
        // a tap past Tr re-reads the last one's (in-bounds) address and is not summed
#pragma unroll
        for (int k = 0; k < kBatch; ++k) {
            const int i = min(i0 + k, Tr - 1);
            const int qy = clampi(y + i - Rr, 0, H - 1);
            const long long q = (long long)qy * W + x;
            qc[k] = img[q];
            e[k] = est[q];
            f[k] = conf[q];
            dist[k] = y > qy ? y - qy : qy - y;
        }
        float w[kBatch];
#pragma unroll
        for (int k = 0; k < kBatch; ++k) {
            const int sad = abs((int)pc.x - qc[k].x) + abs((int)pc.y - qc[k].y) + abs((int)pc.z - qc[k].z);
            w[k] = lut[dist[k] * kLutWidth + sad];
        }
#pragma unroll
        for (int k = 0; k < kBatch; ++k) {
            if (i0 + k < Tr) {
                const float Dv = (float)e[k];
                const float t = w[k] * f[k];
                num = num + t * Dv;
                den = den + t;
            }
        }
    }
    out[p] = num / den;
    out[S + p] = den;
}

// Native consistency: cons = |d_ref - d_tar| <= 1.  Where !cons both confidences are
// zeroed (when given); est_left = cons ? d_ref : d_tar (K/consist.cl writes the target
// value); post16 = cons ? d_ref : ASW_DISP16_INVALID.
__global__ void k_consistency_native(long long n, const int32_t *__restrict__ d_ref, const int32_t *__restrict__ d_tar,
                                     float *__restrict__ conf_ref, float *__restrict__ conf_tar,
                                     int32_t *__restrict__ est_left, uint16_t *__restrict__ post16) {
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const int dr = d_ref[p], dt = d_tar[p];
    const int dd = dr - dt;
    const bool cons = dd <= 1 && dd >= -1;
    if (!cons) {
        if (conf_ref) conf_ref[p] = 0.0f;
        if (conf_tar) conf_tar[p] = 0.0f;
    }
    if (est_left) est_left[p] = cons ? dr : dt;
    if (post16) post16[p] = cons ? (uint16_t)dr : (uint16_t)ASW_DISP16_INVALID;
}

__device__ __forceinline__ void cswap(int &a, int &b) {
    const int lo = min(a, b), hi = max(a, b);
    a = lo;
    b = hi;
}

// 3x3 clamp-to-edge median of an int32 index map, written as uint16 (k_median3's network)
__global__ __launch_bounds__(256) void k_median3_u16(const int32_t *__restrict__ in, int W, int H,
                                                     uint16_t *__restrict__ out) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= W) return;
    int v[9];
    int n = 0;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx)
            v[n++] = in[(long long)clampi(y + dy, 0, H - 1) * W + clampi(x + dx, 0, W - 1)];
    // Paeth's median-of-9 exchange network
    cswap(v[1], v[2]); cswap(v[4], v[5]); cswap(v[7], v[8]);
    cswap(v[0], v[1]); cswap(v[3], v[4]); cswap(v[6], v[7]);
    cswap(v[1], v[2]); cswap(v[4], v[5]); cswap(v[7], v[8]);
    cswap(v[0], v[3]); cswap(v[5], v[8]); cswap(v[4], v[7]);
    cswap(v[3], v[6]); cswap(v[1], v[4]); cswap(v[2], v[5]);
    cswap(v[4], v[7]); cswap(v[4], v[2]); cswap(v[6], v[4]);
    cswap(v[4], v[2]);
    out[(long long)y * W + x] = (uint16_t)v[4];
}

inline int finish() {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_hip_error(e);
        return ASW_E_HIP;
    }
    return ASW_OK;
}

inline size_t lut_slot(const asw_refine_params *rp) { return (asw_refine_lut_bytes(rp) + 255) / 256 * 256; }

}  // namespace
}  // namespace asw

using namespace asw;

extern "C" {

int asw_refine_native_params_check(const asw_params *p, const asw_refine_params *rp) {
    const int s = asw_params_check(p);
    if (s != ASW_OK) return s;
    if (!rp || rp->iters < 0 || rp->taps < 1 || (rp->taps & 1) == 0) return ASW_E_INVALID;
    if (!(rp->gamma_c > 0.0f) || !(rp->gamma_g > 0.0f)) return ASW_E_INVALID;
    if (rp->alpha != 0.085f) return ASW_E_UNSUPPORTED;
    if (p->ndisp > 65535) return ASW_E_INVALID;  // the uint16 maps hold indices below ASW_DISP16_INVALID
    if (p->d_begin != 0 || d_end_of_p(p) != p->ndisp) return ASW_E_INVALID;  // whole volume on one device
    return ASW_OK;
}

int asw_refine_native_lut(const asw_params *p, const asw_refine_params *rp, float *lut, void *stream) {
    const int s = asw_refine_native_params_check(p, rp);
    if (s != ASW_OK) return s;
    asw_params q = *p;  // asw_refine_lut's table: it depends on the window and the falloffs only
    q.taps = rp->taps;
    q.gamma_c = rp->gamma_c;
    q.gamma_g = rp->gamma_g;
    return asw_support_lut(&q, lut, stream);
}

int asw_ref_v_native(const asw_params *p, const asw_refine_params *rp, const uint8_t *img_rgba, const int32_t *est,
                     const float *conf, const float *lut, float *out, void *stream) {
    const int s = asw_refine_native_params_check(p, rp);
    if (s != ASW_OK) return s;
    if (!img_rgba || !est || !conf || !lut || !out) return ASW_E_INVALID;
    const long long S = (long long)p->width * p->height;
    hipLaunchKernelGGL(k_ref_v_native, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const uchar4 *>(img_rgba), est, conf, lut, p->width, p->height, rp->taps, out);
    return finish();
}

int asw_consistency_native(const asw_params *p, const int32_t *d_ref, const int32_t *d_tar, float *conf_ref,
                           float *conf_tar, int32_t *est_left, uint16_t *post16, void *stream) {
    const int s = asw_params_check(p);
    if (s != ASW_OK) return s;
    if (!d_ref || !d_tar || p->ndisp > 65535) return ASW_E_INVALID;
    if (est_left == d_ref || est_left == d_tar) return ASW_E_INVALID;
    const long long n = (long long)p->width * p->height;
    hipLaunchKernelGGL(k_consistency_native, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n,
                       d_ref, d_tar, conf_ref, conf_tar, est_left, post16);
    return finish();
}

int asw_median3_u16(const asw_params *p, const int32_t *in, uint16_t *out, void *stream) {
    const int s = asw_params_check(p);
    if (s != ASW_OK) return s;
    if (!in || !out) return ASW_E_INVALID;
    const dim3 grid((unsigned)((p->width + 255) / 256), (unsigned)p->height);
    hipLaunchKernelGGL(k_median3_u16, grid, dim3(256), 0, (hipStream_t)stream, in, p->width, p->height, out);
    return finish();
}

size_t asw_refine_native_workspace_bytes(const asw_params *p, const asw_refine_params *rp) {
    if (asw_refine_native_params_check(p, rp) != ASW_OK) return 0;
    const size_t S = (size_t)p->width * p->height;
    // lut, 4 x [2][S] f32 (V/H estimates of both views), S int32 (d_ref of the scan)
    return lut_slot(rp) + 4 * 2 * S * 4 + S * 4 + 256;
}

int asw_refine_native(const asw_params *p, const asw_refine_params *rp, const uint8_t *left_rgba,
                      const uint8_t *right_rgba, const float *cost, int32_t *est_left, int32_t *d_tar, float *conf_ref,
                      float *conf_tar, void *workspace, uint16_t *post16, uint16_t *final16, int32_t *d_ref,
                      void *stream) {
    int s = asw_refine_native_params_check(p, rp);
    if (s != ASW_OK) return s;
    if (!left_rgba || !right_rgba || !cost || !est_left || !d_tar || !conf_ref || !conf_tar || !workspace)
        return ASW_E_INVALID;
    const size_t S = (size_t)p->width * p->height;
    char *ws = static_cast<char *>(workspace);
    float *lut = reinterpret_cast<float *>(ws);
    ws += lut_slot(rp);
    float *vl = reinterpret_cast<float *>(ws), *vr = vl + 2 * S, *hl = vr + 2 * S, *hr = hl + 2 * S;
    int32_t *dr = reinterpret_cast<int32_t *>(hr + 2 * S);
    hipStream_t st = (hipStream_t)stream;
    if ((s = asw_refine_native_lut(p, rp, lut, st)) != ASW_OK) return s;
    for (int it = 0; it < rp->iters; ++it) {
        if ((s = asw_ref_v_native(p, rp, left_rgba, est_left, conf_ref, lut, vl, st)) != ASW_OK) return s;
        if ((s = asw_ref_v_native(p, rp, right_rgba, d_tar, conf_tar, lut, vr, st)) != ASW_OK) return s;
        if ((s = asw_ref_h(p, rp, left_rgba, conf_ref, vl, lut, hl, st)) != ASW_OK) return s;
        if ((s = asw_ref_h(p, rp, right_rgba, conf_tar, vr, lut, hr, st)) != ASW_OK) return s;
        // the scan writes the new target map over the one the right V estimate has read
        if ((s = asw_wta_ref(p, cost, hl, hr, dr, d_tar, conf_ref, nullptr, nullptr, st)) != ASW_OK) return s;
        if ((s = asw_consistency_native(p, dr, d_tar, conf_ref, conf_tar, est_left, post16, st)) != ASW_OK) return s;
    }
    if (final16 && (s = asw_median3_u16(p, est_left, final16, st)) != ASW_OK) return s;
    if (d_ref && rp->iters > 0 && hipMemcpyAsync(d_ref, dr, S * 4, hipMemcpyDeviceToDevice, st) != hipSuccess)
        return ASW_E_HIP;
    return ASW_OK;
}

}  // extern "C"
