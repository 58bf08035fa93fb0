// Shared host/device definitions of the ASW matcher (layout pitches, error state).
#pragma once
#include <hip/hip_runtime.h>

#include "asw.h"

namespace asw {

constexpr int kWave = 64;
constexpr int kSadMax = 765;        // 3 * 255: largest RGB SAD
constexpr int kLutWidth = kSadMax + 1;

// Tp: smallest multiple of 4 >= T whose quotient by 4 is odd.  A wave's lanes
// read the support slab at a stride of Tp floats; an odd number of 16-byte
// slots per row keeps ds_read_b128 conflict-free.
__host__ __device__ constexpr int tap_pitch(int T) {
    int k = (T + 3) / 4;
    if ((k & 1) == 0) ++k;
    return 4 * k;
}

__host__ __device__ constexpr int round_up(int v, int m) { return (v + m - 1) / m * m; }

// 8-bit code of disparity index d for D levels: round-half-down of 255*d/(D-1),
// the convention of the reference's write_imagef (K/asw_wta.cl:70-74).
__host__ __device__ inline int code_u8(int d, int D) {
    if (D <= 1) return 0;
    long long c = (510LL * d + (D - 2)) / (2LL * (D - 1));
    return c > 255 ? 255 : (c < 0 ? 0 : (int)c);
}

// The left-right rule of asw_outputs.lr16, asw_disp_mask and asw_lr_valid at pixel p, written
// once: ASW_LR_U8 compares the 8-bit codes like K/consist.cl:20-30, ASW_LR_NATIVE the indices
// (|d_ref - d_tar| <= 1).  dr = d_ref[p]; the code pointers are read with ASW_LR_U8 only.
__device__ __forceinline__ bool lr_consistent(int mode, int D, long long p, int dr, const int32_t *d_tar,
                                              const uint8_t *code_ref, const uint8_t *code_tar) {
    if (mode == ASW_LR_U8) {
        const float scale = (float)(D - 1);
        const float qr = ((float)code_ref[p] / 255.0f) * scale;
        const float qt = ((float)code_tar[p] / 255.0f) * scale;
        return fabsf(qt - qr) < 1.001f;
    }
    const int dd = dr - d_tar[p];
    return dd <= 1 && dd >= -1;
}

void set_hip_error(hipError_t e);

// last plane + 1 of the context's disparity shard (asw_params.d_end < 0: ndisp)
__host__ __device__ inline int d_end_of_p(const asw_params *p) { return p->d_end < 0 ? p->ndisp : p->d_end; }

// the first V pass over the raw costs as uint16 (asw_raw_cost16, asw_aggregate_pass_den16)
struct RawSrc {
    const uint16_t *cost16;
};

// one aggregation pass over every local plane (asw_aggregate.hip)
// den/dm: cached-denominator mode (ASW_DEN_*; den = NULL with ASW_DEN_NONE)
int launch_pass(const asw_params *p, int dir, const float *wl, const float *wr, const float *cin, float *cout,
                float *den, int dm, hipStream_t st, const RawSrc *raw = nullptr);
// the H pass's k_hpass11 segment length (variant bits 8..11: U-step chunks, else the
// multiple of U nearest 240) and its choice against k_hpass9 (launch_dm)
int h11_seg_len(int T, int variant);
bool h11_selected(const asw_params *p, int variant);
// the tap counts with ring kernels (the uint16 first pass needs one)
bool ring_taps(int T);
int set_pass_variant(int v);
// the asw_tune_set(ASW_TUNE_PASS_VARIANT) bits launch_dm reads: 128 = H by k_hpass9,
// 4096 = H by k_hpass11 at any size, 0xF00 = k_hpass11 segment length in U-step chunks
constexpr int kPassVariantBits = 128 | 4096 | 0xF00;
// records the instantiation a pass launch of (dir, dm) runs (asw_pass_kernel)
void note_pass_kernel(int dir, int dm, const char *kernel, int T, const char *shape, bool nt);
// ASW_OK when the pass kernels can address a (shard) context of this shape: they use
// 32-bit buffer offsets of up to ~2T+16 cost rows from a per-chunk base and a support
// array from its base; ASW_E_UNSUPPORTED otherwise (checked at asw_create, before
// any allocation, and by every pass launch)
int pass_shape_check(const asw_params *p);

// ASW_OK when asw_raw_cost16 / asw_census_cost16 is built for p (and cp): the cost has a uint16
// form (the tad_tau rule of include/asw.h) and the kernel's LDS stage holds the pitch; else
// ASW_E_UNSUPPORTED.  The one rule of those entry points, asw_*16_supported and asw_set_sgm;
// p (and cp) have passed their parameter checks.
int raw_cost16_check(const asw_params *p);
int census_cost16_check(const asw_params *p, const asw_census_params *cp);
// ASW_OK when k_sgm_path is built for p's pitch (at most 65536 planes), else ASW_E_UNSUPPORTED
int sgm_shape_check(const asw_params *p);

// lane-per-pixel WTA scan (asw_refine.hip): mode 0 = asw_WTA, 1 = asw_WTA_REF
// lane-per-pixel d-sharded WTA halves (ref = NULL: asw_WTA; else asw_WTA_REF's penalty)
int launch_wta_local_scan(const asw_params *p, const float *cost, const float *ref, long long *key, float *m1,
                          float *m2, hipStream_t st);
int launch_wta_target_local_scan(const asw_params *p, const float *cost, const long long *key_ref, const float *ref,
                                 long long *tkey, float *t1, float *t2, hipStream_t st);
int launch_wta_scan(const asw_params *p, int mode, const float *cost, const float *ref_l, const float *ref_r,
                    int32_t *d_ref, float *conf_ref, int32_t *d_tar, float *conf_tar, uint8_t *code_ref,
                    uint8_t *code_tar, hipStream_t st);

}  // namespace asw
