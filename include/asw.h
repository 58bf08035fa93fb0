/*
 * asw.h — C-ABI of the MI355X-native adaptive-support-weight (ASW) stereo matcher.
 *
 * Drop-in boundary for the reference's OpenCL `kernels/` path
 * (manixq/stereo_matchin, stereo_matching/main.cpp:413-537).  Every entry point
 * is `extern "C"`, takes plain pointers and sizes, returns an int status
 * (ASW_OK or a negative ASW_E_* code; never throws), and names the reference
 * interface it replaces.
 *
 * Two levels:
 *   - STAGE API: device pointers, asynchronous on the caller's HIP stream
 *     (`void* stream` is a hipStream_t; NULL = default stream).  One call per
 *     reference kernel launch, with the same argument meaning.
 *   - FRAME API: host RGBA8 pointers in, host disparity maps out, synchronous
 *     (what main.cpp:183-186 -> :621-631 does for one image pair).
 *
 * Device data layout — NOT the reference's plane-major one:
 *   images   : row-major RGBA8, [H][W][4]                         (as lodepng decodes)
 *   cost     : PIXEL-major, [H][W][Dp] float32, Dp = asw_disp_pitch(p) (64k, or 32)
 *              element (y,x,k) holds disparity d = p->d_begin + k (k < d_end-d_begin)
 *   supports : [H][W][Tp] float32, Tp = asw_tap_pitch(p); element (y,x,i) = tap i
 *   LUT      : [(R+1)][766] float32 support-weight table, R = (taps-1)/2
 *   maps     : [H][W] int32 disparity indices, float32 confidences, u8 codes
 */
#ifndef ASW_H
#define ASW_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes (main.cpp:27-30 ErCheck prints cl_int and continues; we return) ---- */
#define ASW_OK 0
#define ASW_E_INVALID -1     /* bad parameter / shape                         */
#define ASW_E_HIP -2         /* a HIP runtime call failed (asw_last_hip_error) */
#define ASW_E_NOMEM -3       /* device or host allocation failed              */
#define ASW_E_UNSUPPORTED -4 /* parameter combination not built               */
#define ASW_E_COMM -5        /* a collective (RCCL) call failed               */

#define ASW_DIR_V 0 /* vertical pass / support   (asw_vSupport, asw_vCostAggregation) */
#define ASW_DIR_H 1 /* horizontal pass / support (asw_hSupport, asw_hCostAggregation) */

#define ASW_COLOR_RGB 0 /* reference: RGB sum of absolute differences (K/asw_vsupport.cl:22) */
#define ASW_COLOR_LAB 1 /* extension (north star): CIELab Euclidean distance (asw_lab)     */

#define ASW_LR_U8 0     /* parity: compare 8-bit codes like K/consist.cl:20-30 */
#define ASW_LR_NATIVE 1 /* |d_ref - d_tar| <= 1 on integer indices (D > 256)   */

/* Parameters.  asw_params_default() fills the reference values:
 * ndisp 61 (K/asw_aggr.cl:16), taps 33 (K/asw_vcost_aggregation.cl:33), iters 7
 * (main.cpp:177), gamma_c 30.91 / gamma_g 28.21 (K/asw_vsupport.cl:22,24),
 * untruncated AD (tad_tau >= 765), LR check on with 8-bit codes. */
typedef struct asw_params {
    int width, height;   /* image size W, H                                    */
    int ndisp;           /* D: disparity levels 0..D-1                          */
    int taps;            /* T = 2R+1 taps per 1-D pass (odd)                    */
    int iters;           /* r: (V,H) pass pairs                                 */
    float gamma_c;       /* colour falloff                                       */
    float gamma_g;       /* geometric falloff                                    */
    int color_space;     /* ASW_COLOR_*                                          */
    float tad_tau;       /* truncated-AD threshold; >= 765 is plain AD           */
    int lr_check;        /* run the left-right consistency stage                */
    int lr_mode;         /* ASW_LR_*                                             */
    int d_begin, d_end;  /* disparity shard owned by this context [begin, end)  */
    int flags;           /* ASW_FLAG_*: frame-API context options (0 = the default forms) */
} asw_params;

/* asw_params.flags: context options of the frame API (asw_create*).  Every option is
 * bit-identical to the default; asw_params_check rejects unknown bits.  (Round 6 removed
 * the opt-in forms that measured slower in every shape; their bits
 * 0x1, 0x2, 0x4, 0x8, 0x10, 0x80 and 0x100 are no longer accepted.)  The stage API
 * ignores flags. */
#define ASW_FLAG_COMM_LOCAL 0x20     /* asw_create_multi: the device-local exchange even for distinct ids */
#define ASW_FLAG_RAW_F32 0x40        /* keep the float raw-cost volume (asw_raw_cost) where the uint16 one
                                        (asw_raw_cost16 + asw_aggregate_pass_den16) is the default;
                                        ignored while asw_set_sgm is on (SGM reads the uint16 volume) */
#define ASW_FLAG_ALL 0x60

void asw_params_default(asw_params *p);
int asw_params_check(const asw_params *p);
const char *asw_strerror(int status);
int asw_last_hip_error(void); /* hipError_t of the last ASW_E_HIP */
/* ABI revision of this header.  The frame API's caller-allocated structs
 * (asw_outputs, asw_timings) grow between revisions: a host must check
 * asw_abi_version() == ASW_ABI_VERSION before calling asw_match / asw_match_batch,
 * or the library writes past a struct of an older layout.
 *   1: round 1;  2: asw_outputs.disp16 / lr16, asw_timings.exchange;
 *   3: asw_params.flags (the context options that were environment variables);
 *      asw_raw_cost16 / asw_aggregate_pass_den16 (the uint16 raw-cost volume);
 *   4: the measured-negative forms removed with their entry points and flags
 *      (on-the-fly, index-form and fused-raw passes, the fused WTA scan).
 * Additive within revision 4 (no struct above changes its layout, no flag is added):
 *      the sub-pixel entry points asw_subpixel / asw_subpixel_local /
 *      asw_subpixel_finalize / asw_disp_mask / asw_disp_fill and asw_set_subpixel with
 *      its own asw_subpixel_outputs struct; the cross-based matcher's entry points
 *      (asw_median3_rgba, asw_cross_*) and asw_set_cross with its own structs; the census /
 *      AD-census matching cost (asw_census_*, asw_census, asw_census_cost, asw_census_cost16,
 *      asw_census16_supported) and asw_set_census with its own asw_census_params struct; the
 *      native refinement loop (asw_refine_native_*, asw_ref_v_native, asw_consistency_native,
 *      asw_median3_u16, asw_refine_native) and asw_set_refine_native with its own
 *      asw_refine_native_outputs struct; the semi-global matching aggregator (asw_sgm_params_default,
 *      asw_sgm_params_check, asw_sgm_workspace_bytes, asw_sgm_path, asw_sgm) and asw_set_sgm with
 *      its own asw_sgm_params struct; the speckle filter (asw_speckle_params_default,
 *      asw_speckle_params_check, asw_speckle_workspace_bytes, asw_lr_valid, asw_speckle,
 *      asw_speckle_mask16, asw_speckle_mask_f32) and asw_set_speckle with its own asw_speckle_params
 *      and asw_speckle_outputs structs. */
#define ASW_ABI_VERSION 4
int asw_abi_version(void);

/* layout helpers */
/* Dp = round_up(d_end-d_begin, 64); a shard (d_begin > 0 or d_end < ndisp) of at most
 * 32 planes: Dp = 32 (its passes hold two pixels per wave, 32 planes each) */
int asw_disp_pitch(const asw_params *p);
int asw_tap_pitch(const asw_params *p);  /* Tp = smallest 4k >= taps with k odd        */
size_t asw_cost_bytes(const asw_params *p);    /* H*W*Dp*4   */
size_t asw_support_bytes(const asw_params *p); /* H*W*Tp*4   */
size_t asw_lut_bytes(const asw_params *p);     /* (R+1)*766*4 */
size_t asw_lab_bytes(const asw_params *p);     /* H*W*16 (float4 per pixel) */

/* ---------------- STAGE API (device pointers, async on `stream`) ---------------- */

/* replaces asw_Aggr (K/asw_aggr.cl:3-23), launched at main.cpp:463-466:
 * cost[y][x][k] = min(tad_tau, |dR|+|dG|+|dB|) between L(x,y) and R(max(x-d,0),y),
 * d = d_begin + k; padding lanes k >= d_end-d_begin are written 0. */
int asw_raw_cost(const asw_params *p, const uint8_t *left_rgba, const uint8_t *right_rgba, float *cost,
                 void *stream);
/* The same costs as uint16 [H][W][Dp] (half the bytes): |dR|+|dG|+|dB| is an integer
 * <= 765, so min(tad_tau, AD) is one too when tad_tau >= 765 or integral; other
 * tad_tau (or tad_tau < 0): ASW_E_UNSUPPORTED.  asw_aggregate_pass_den16 reads it as the
 * first V pass (main.cpp:494-500); the float values it converts are the ones
 * asw_raw_cost writes, so every output is bit-identical.  asw_raw16_supported: 1 when
 * both are built for p (that tad_tau, a ring tap count, iters >= 1), else 0.  The pass
 * itself never reads tad_tau (it needs a ring tap count and iters >= 1, else
 * ASW_E_UNSUPPORTED): it also reads asw_census_cost16's volume (integers <= 65535). */
int asw_raw_cost16(const asw_params *p, const uint8_t *left_rgba, const uint8_t *right_rgba, uint16_t *cost,
                   void *stream);
int asw_aggregate_pass_den16(const asw_params *p, const float *wvl, const float *wvr, const uint16_t *cin16,
                             float *cout, float *den, int den_mode, void *stream); /* V; den_mode NONE or WRITE */
int asw_raw16_supported(const asw_params *p);

/* ---- census / AD-census matching cost (no reference counterpart: the reference's only
 * raw cost is the RGB AD, which a gain or offset between the two views breaks).  Every
 * operation is an integer one but the two float operations of the float form
 * (DESIGN.md §Census).
 *   luma    Y = (77 R + 150 G + 29 B + 128) >> 8, 0..255 (alpha ignored)
 *   census  uint64 per pixel over a win_w x win_h window (each of 3, 5, 7, 9 with
 *           win_w * win_h - 1 <= 64: every pair but 9x9; default 9x7 = 62 bits).  The
 *           neighbours are enumerated row-major (dy = -rh..rh, within a row dx = -rw..rw,
 *           the centre skipped); neighbour n (0-based) sets bit n (LSB first) when
 *           Y(clamp(x+dx), clamp(y+dy)) < Y(x, y) (strict; clamp-to-edge); upper bits 0.
 *   cost    with xr = max(x - d, 0), d = d_begin + k (as asw_raw_cost),
 *           AD = |dR|+|dG|+|dB| of L(x, y) and R(xr, y), ham = popcount(cenL(x, y) ^ cenR(xr, y))
 *           and the integer weights ad_weight w_a >= 0, census_weight w_c >= 1:
 *     float   cost = fminf((float)AD, tad_tau) * (float)w_a + (float)(w_c * ham)
 *             (one float multiply, then one float add, no fma); w_a = 0: the AD term is
 *             not formed, tad_tau is not read, cost = (float)(w_c * ham)
 *     uint16  w_a * min(AD, tau) + w_c * ham as an integer: defined when w_a = 0 or
 *             tad_tau >= 765 or integral (asw_raw_cost16's rule), else ASW_E_UNSUPPORTED.
 *             Its float value equals the float form bit for bit.
 *           Padding planes k >= d_end - d_begin are written 0.
 * asw_census_params_check (ASW_E_INVALID otherwise): p passes asw_params_check, the window
 * rule, 0 <= w_a <= 64, 1 <= w_c <= 1024, tad_tau >= 0 when w_a > 0, and
 * w_a * min(765, ceil(tad_tau)) + w_c * (win_w * win_h - 1) <= 65535.
 * asw_census16_supported: 1 when asw_census_cost16 and the first V pass over its volume
 * (asw_aggregate_pass_den16) are built for (p, cp): the tau rule above, a ring tap count,
 * iters >= 1 (asw_raw16_supported's conditions), else 0. */
typedef struct asw_census_params {
    int win_w, win_h;   /* census window (odd, 3..9, not 9x9); default 9 x 7            */
    int ad_weight;      /* w_a: 0..64; 0 = census only; default 1                       */
    int census_weight;  /* w_c: 1..1024; default 8                                      */
} asw_census_params;
void asw_census_params_default(asw_census_params *cp);
int asw_census_params_check(const asw_params *p, const asw_census_params *cp);
size_t asw_census_bytes(const asw_params *p); /* H*W*8 */
/* the census codes [H][W] uint64 of an RGBA8 image */
int asw_census(const asw_params *p, const asw_census_params *cp, const uint8_t *img_rgba, uint64_t *census,
               void *stream);
/* the cost volume [H][W][Dp] of p's planes from both images and their census codes */
int asw_census_cost(const asw_params *p, const asw_census_params *cp, const uint8_t *left_rgba,
                    const uint8_t *right_rgba, const uint64_t *cen_left, const uint64_t *cen_right, float *cost,
                    void *stream);
int asw_census_cost16(const asw_params *p, const asw_census_params *cp, const uint8_t *left_rgba,
                      const uint8_t *right_rgba, const uint64_t *cen_left, const uint64_t *cen_right, uint16_t *cost,
                      void *stream);
int asw_census16_supported(const asw_params *p, const asw_census_params *cp);

/* ---- semi-global matching (Hirschmueller 2008) on the uint16 raw-cost volume (no reference
 * counterpart: the reference's only aggregator is the iterated ASW pass).  Every operation is
 * an integer one.  Input: a whole-volume raw cost C, uint16 [H][W][Dp], as
 * asw_raw_cost16 or asw_census_cost16 writes it; padding planes d >= ndisp never reach a
 * result.  Path k has the step (dx, dy); the predecessor of p = (x, y) is q = (x-dx, y-dy):
 *   k  0: (+1, 0)  1: (-1, 0)  2: (0, +1)  3: (0, -1)  4: (+1, +1)  5: (-1, -1)  6: (-1, +1)  7: (+1, -1)
 *   q outside the image:  L_k(p, d) = C(p, d)
 *   else, m = min_{j < ndisp} L_k(q, j):
 *     L_k(p, d) = C(p, d) + min(L_k(q, d), L_k(q, d-1) + P1, L_k(q, d+1) + P1, m + P2) - m
 *     (the d-1 term absent at d = 0, the d+1 term at d = ndisp-1)
 * so C <= L_k <= C + P2.  S(p, d) = sum of L_k over k < paths (4: k = 0..3; 8: k = 0..7) is
 * below 2^24: the output volume, float32 [H][W][Dp], holds (float)S exactly, and every float
 * add of partial sums is exact, so the order of the paths is free.  The first-argmin WTA and
 * everything after it read this volume like an aggregated one.
 * asw_sgm_params_check: ASW_E_INVALID for paths not 4 or 8, penalties outside
 * 0 <= p1 <= p2 <= 1048576, a p that fails asw_params_check, or a shard p (d_begin > 0 or
 * d_end < ndisp: m is a minimum over every disparity).  Offsets are 64-bit: no accepted shape
 * overflows them (a pitch above 65536 planes is ASW_E_UNSUPPORTED at launch, and so is a shape
 * whose walkers, max(width, height) blocks of up to 1024 threads at pitches above 256, exceed
 * the 2^32 - 1 work-items of a launch: e.g. height 2^22 at 4096 planes).
 *   asw_sgm_path: path k alone (0 <= k < 8 whatever sp->paths, else ASW_E_INVALID).
 *     accumulate == 0: sum = (float)L_k on the valid planes, +0 on the padding planes;
 *     accumulate != 0: sum = sum + (float)L_k on the valid planes, padding planes kept.
 *   asw_sgm: the whole S of sp->paths, padding planes +0.  workspace: asw_sgm_workspace_bytes
 *     of device memory (0 today: NULL is accepted then, ASW_E_INVALID otherwise).
 * cost16 and sum must not alias. */
typedef struct asw_sgm_params {
    int paths;   /* 4 or 8; default 8                        */
    int p1, p2;  /* 0 <= p1 <= p2 <= 1048576; default 16, 128 */
} asw_sgm_params;
void asw_sgm_params_default(asw_sgm_params *sp);
int asw_sgm_params_check(const asw_params *p, const asw_sgm_params *sp);
size_t asw_sgm_workspace_bytes(const asw_params *p, const asw_sgm_params *sp);
int asw_sgm_path(const asw_params *p, const asw_sgm_params *sp, int k, const uint16_t *cost16, float *sum,
                 int accumulate, void *stream);
int asw_sgm(const asw_params *p, const asw_sgm_params *sp, const uint16_t *cost16, float *sum, void *workspace,
            void *stream);

/* support-weight table (the exp of K/asw_vsupport.cl:22-25 for every (|delta|, SAD)) */
int asw_support_lut(const asw_params *p, float *lut, void *stream);

/* replaces asw_vSupport / asw_hSupport (K/asw_vsupport.cl:3-27, K/asw_hsupport.cl:3-28),
 * launched at main.cpp:469-484 (once per image and direction).  RGB contexts only
 * (ASW_E_INVALID for ASW_COLOR_LAB: use asw_lab + asw_support_lab).  The padding taps
 * i >= taps of every pixel are written 0 (asw_support_all and asw_support_lab too).
 * A row of width * Tp floats is indexed in 32 bits: width * Tp + 255 > 2^31 - 1 is
 * ASW_E_UNSUPPORTED in all three entry points (no kernel is launched). */
int asw_support(const asw_params *p, int dir, const uint8_t *img_rgba, const float *lut, float *w,
                void *stream);

/* the four support arrays of a frame in one launch (asw_vSupport and asw_hSupport of
 * both images, main.cpp:469-484): bit-identical to four asw_support calls. */
int asw_support_all(const asw_params *p, const uint8_t *left_rgba, const uint8_t *right_rgba, const float *lut,
                    float *wvl, float *whl, float *wvr, float *whr, void *stream);

/* CIELab extension (north star; the reference has no colour conversion, so this
 * is not reference-pinned: the oracle restates the same IEEE double sequence and
 * colorimetric known answers pin the conversion).  With p->color_space ==
 * ASW_COLOR_LAB the support weights use the Euclidean L*a*b* distance in place of
 * the RGB SAD of K/asw_vsupport.cl:19-25; the raw cost stays RGB AD/TAD.
 *   asw_lab:          lab[y][x] = (L*, a*, b*, 0) float4 of an RGBA8 image (sRGB, D65)
 *   asw_support_lab:  the asw_support of a LAB context, from a lab image. */
int asw_lab(const asw_params *p, const uint8_t *img_rgba, float *lab, void *stream);
int asw_support_lab(const asw_params *p, int dir, const float *lab, float *w, void *stream);

/* replaces asw_vCostAggregation / asw_hCostAggregation (K/asw_vcost_aggregation.cl:11-44,
 * K/asw_hcost_aggregation.cl:12-44), launched at main.cpp:494-509.  One pass over
 * every local plane: cout = sum_i wl_i*wr_i(xr)*cin_i / sum_i wl_i*wr_i(xr).
 * The reference's dead `denom` output is not produced.  cin != cout.
 * Padding planes k >= d_end - d_begin of cout are UNSPECIFIED in every pass entry point
 * (asw_aggregate_pass, _den, _den16, asw_aggregate, asw_aggregate_den): the kernels carry
 * them along, computed from cin's padding planes (NaN or 0xFFFF there comes out as NaN or
 * a large value).  No valid plane depends on a padding plane of cin, cout or den. */
int asw_aggregate_pass(const asw_params *p, int dir, const float *wl, const float *wr, const float *cin,
                       float *cout, void *stream);

/* Same pass with a cached denominator volume `den` ([H][W][Dp] float32, the cost
 * layout).  The reference recomputes den = 1e-5 + sum_i wl_i*wr_i(xr) in every pass
 * (K/asw_vcost_aggregation.cl:38, written to its dead asw_denom buffer); it does
 * not depend on the cost, so ASW_DEN_WRITE stores it during a pass and
 * ASW_DEN_READ reuses it in the later passes of the same direction (same
 * supports).  Results are bit-identical in every mode.  The padding planes of `den` are
 * UNSPECIFIED: ASW_DEN_WRITE writes them (the sum at the disparities past d_end, which no
 * valid plane uses) and ASW_DEN_READ reads them into cout's padding planes only. */
#define ASW_DEN_NONE 0  /* compute den, do not touch `den` (may be NULL) */
#define ASW_DEN_WRITE 1 /* compute den and store it to `den`            */
#define ASW_DEN_READ 2  /* take den from `den` (written by a DEN_WRITE pass of this direction) */
int asw_aggregate_pass_den(const asw_params *p, int dir, const float *wl, const float *wr, const float *cin,
                           float *cout, float *den, int den_mode, void *stream);

/* r x (V,H) ping-pong of main.cpp:486-515 on two caller buffers; the result
 * ends in `c0` (c0 holds the raw cost on entry, c1 is scratch). */
int asw_aggregate(const asw_params *p, const float *wvl, const float *wvr, const float *whl, const float *whr,
                  float *c0, float *c1, void *stream);
/* asw_aggregate with cached denominators: den_v, den_h are two more [H][W][Dp]
 * volumes (asw_cost_bytes each); the first iteration writes them, the other r-1
 * read them.  den_v = den_h = NULL is asw_aggregate. */
int asw_aggregate_den(const asw_params *p, const float *wvl, const float *wvr, const float *whl, const float *whr,
                      float *c0, float *c1, float *den_v, float *den_h, void *stream);

/* replaces asw_WTA (K/asw_wta.cl:12-82), launched at main.cpp:517-526, for a context
 * that owns the whole disparity range: left first-argmin + confidence, the
 * bresenham target scan, and the 8-bit codes the reference writes to its images.
 * The target scan (here, in asw_wta_target_local, asw_wta_ref and asw_wta_ref_target_local)
 * gathers with 32-bit byte offsets from the start of a row: (width + 64) * Dp * 4 >= 2^31
 * is ASW_E_UNSUPPORTED (no kernel is launched); asw_wta through the row sweep
 * (ASW_TUNE_WTA_VARIANT 2, Dp 64 / 128 / 256) has no such limit. */
int asw_wta(const asw_params *p, const float *cost, int32_t *d_ref, float *conf_ref, int32_t *d_tar,
            float *conf_tar, uint8_t *code_ref, uint8_t *code_tar, void *stream);

/* replaces Constistency (K/consist.cl:3-34), launched at main.cpp:529-537.
 * conf_ref / conf_tar are zeroed in place where inconsistent (RMW like the
 * reference).  out_rgba / out_red_rgba are [H][W][4]; either may be NULL. */
int asw_consistency(const asw_params *p, const int32_t *d_ref, const int32_t *d_tar, const uint8_t *code_ref,
                    const uint8_t *code_tar, float *conf_ref, float *conf_tar, uint8_t *out_rgba,
                    uint8_t *out_red_rgba, void *stream);

/* ---- d-sharded WTA (no reference counterpart: the reference runs one device) ----
 * key = (float_bits(m1) << 32) | index, reduced with an elementwise MIN across
 * shards (RCCL ncclMin on int64; keys are positive).  Sequence per frame:
 *   asw_wta_local      -> allreduce_min(key)   -> asw_wta_second(ref)  -> allreduce_min(m2)
 *   asw_wta_target_local(key) -> allreduce_min(tkey) -> asw_wta_second(tar) -> allreduce_min(t2)
 *   asw_wta_finalize.
 * Exact: the result equals asw_wta on the unsharded volume bit for bit. */
int asw_wta_local(const asw_params *p, const float *cost, int64_t *key, float *m1, float *m2, void *stream);
int asw_wta_target_local(const asw_params *p, const float *cost, const int64_t *key_ref, int64_t *tkey,
                         float *t1, float *t2, void *stream);
int asw_wta_second(const asw_params *p, const int64_t *key_global, const int64_t *key_local, const float *m1,
                   const float *m2, float *m2_contrib, void *stream);
int asw_wta_finalize(const asw_params *p, const int64_t *key, const float *m2, const int64_t *tkey,
                     const float *t2, int32_t *d_ref, float *conf_ref, int32_t *d_tar, float *conf_tar,
                     uint8_t *code_ref, uint8_t *code_tar, void *stream);

/* ---- sub-pixel float disparity maps (no reference counterpart: the reference writes
 * 8-bit codes only).  Every operation is an IEEE float32 one, in this order
 * (DESIGN.md §Sub-pixel).  With d = d_ref[p] (the first argmin) and c0 = C[p][d],
 * cm = C[p][d-1], cp = C[p][d+1] of the final aggregated volume:
 *   d == 0 or d == ndisp-1:  disp[p] = (float)d
 *   else  a = cm - c0;  b = cp - c0;  disp[p] = (float)d + (a - b) / (2.0f * (a + b))
 * (the quotient correctly rounded; a > 0, b >= 0, so the offset lies in (-0.5, 0.5]).
 * Planes >= ndisp (pitch padding) are never read.
 *   asw_subpixel: whole-volume p only (d_begin = 0, d_end = ndisp), else ASW_E_INVALID.
 * d-sharded (after the first MIN all-reduce of the asw_wta_local protocol):
 *   asw_subpixel_local(key_global) -> allreduce_min(nb) -> asw_subpixel_finalize.
 * nb is [3][S] float32: nb[j][p] = C[p][d-1+j] where this shard owns plane d-1+j (and it
 * lies in [0, ndisp)), +INF elsewhere; d = low 32 bits of key_global[p].  The three
 * floats that survive the MIN are the ones asw_subpixel reads: bit-identical. */
int asw_subpixel(const asw_params *p, const float *cost, const int32_t *d_ref, float *disp, void *stream);
int asw_subpixel_local(const asw_params *p, const float *cost, const int64_t *key_global, float *nb, void *stream);
int asw_subpixel_finalize(const asw_params *p, const int64_t *key_global, const float *nb, float *disp,
                          void *stream);
/* disp_lr[p] = disp[p] where the LR rule of asw_outputs.lr16 passes (ASW_LR_U8: the 8-bit
 * codes of K/consist.cl:20-30; ASW_LR_NATIVE: |d_ref - d_tar| <= 1), else a quiet NaN.
 * code_ref / code_tar may be NULL with ASW_LR_NATIVE. */
int asw_disp_mask(const asw_params *p, const float *disp, const int32_t *d_ref, const int32_t *d_tar,
                  const uint8_t *code_ref, const uint8_t *code_tar, float *disp_lr, void *stream);
/* background fill per row: a valid (non-NaN) pixel is copied; an invalid one takes the
 * smaller of its nearest valid neighbours to the left and to the right in its row (the
 * one that exists at a row end, 0.0f in a row without a valid pixel).  The output holds
 * no NaN.  disp_lr != disp_filled. */
int asw_disp_fill(const asw_params *p, const float *disp_lr, float *disp_filled, void *stream);

/* ---- speckle filter: connected components of similar disparity (no reference counterpart;
 * the post-filter of OpenCV's filterSpeckles and Hirschmueller's peak filter).  Integers only,
 * free of any order.  Input: d, int32 [H][W], any values; valid, uint8
 * [H][W], non-zero = valid, NULL = every pixel valid.  Pixels p and q are LINKED when they are
 * 4-neighbours, both valid and |d[p] - d[q]| <= max_diff (the difference in 64 bits: INT32_MIN
 * beside INT32_MAX is not linked).  A component is a connected component of that graph (a ramp
 * 0, 1, 2, ... is one component at max_diff 1).  Every element of every output is written:
 *   valid p:    label[p] = the smallest flat index y*W + x of p's component,
 *               size[p]  = the component's pixel count, keep[p] = size[p] >= min_size
 *   invalid p:  label[p] = -1, size[p] = 0, keep[p] = 0
 * asw_speckle_params_check: ASW_E_UNSUPPORTED for width * height > 2^31 - 1 (labels are int32
 * pixel indices; nothing is launched; checked first, since asw_params_check has a pixel limit of
 * its own, 2^25 today, and answers ASW_E_INVALID); ASW_E_INVALID for min_size < 1, max_diff
 * outside 0..65535 or a p that fails asw_params_check.  Only width and height of p are read: a
 * shard p and any ndisp are fine.
 *   asw_speckle: label, size and keep may each be NULL.  workspace: asw_speckle_workspace_bytes
 *     of device memory with arbitrary contents (the stage initialises what it reads); d, valid and
 *     the outputs must not overlap it (ASW_E_INVALID).  The int32 at byte ASW_SPECKLE_STATUS_OFFSET
 *     of the workspace is the status word: 0 after a run whose link-following loops all ended by
 *     themselves, non-zero when one ran into its bound of width * height steps (the outputs are
 *     then not to be trusted; it cannot happen unless the kernels are wrong).  All offsets 64-bit.
 *   asw_lr_valid: valid[p] = 1 where the LR rule of asw_outputs.lr16 / asw_disp_mask passes
 *     (p->lr_mode; code_ref / code_tar may be NULL with ASW_LR_NATIVE), else 0.
 *   asw_speckle_mask16: out[p] = (uint16)d[p] where keep[p], else ASW_DISP16_INVALID;
 *     ASW_E_INVALID for ndisp > 65535.
 *   asw_speckle_mask_f32: out[p] = disp[p] where keep[p], else asw_disp_mask's quiet NaN
 *     (0x7fc00000): asw_disp_fill fills it. */
typedef struct asw_speckle_params {
    int min_size;  /* 1..2^31-1: smallest component that is kept; default 32 */
    int max_diff;  /* 0..65535: largest linked difference; default 1         */
} asw_speckle_params;
#define ASW_SPECKLE_STATUS_OFFSET 0
void asw_speckle_params_default(asw_speckle_params *sp);
int asw_speckle_params_check(const asw_params *p, const asw_speckle_params *sp);
size_t asw_speckle_workspace_bytes(const asw_params *p);
int asw_lr_valid(const asw_params *p, const int32_t *d_ref, const int32_t *d_tar, const uint8_t *code_ref,
                 const uint8_t *code_tar, uint8_t *valid, void *stream);
int asw_speckle(const asw_params *p, const asw_speckle_params *sp, const int32_t *d, const uint8_t *valid,
                void *workspace, int32_t *label, int32_t *size, uint8_t *keep, void *stream);
int asw_speckle_mask16(const asw_params *p, const int32_t *d, const uint8_t *keep, uint16_t *out, void *stream);
int asw_speckle_mask_f32(const asw_params *p, const float *disp, const uint8_t *keep, float *out, void *stream);

/* ---- d-sharded asw_WTA_REF (K/asw_wta_ref.cl:2-68): the refinement loop's volume
 * scan over a shard, the asw_wta_local protocol on the penalised values
 * 0.085*den*|val - i| + C (ref_l / ref_r = asw_ref_h's [2][S] output of each view):
 *   asw_wta_ref_local -> allreduce_min(key)
 *   asw_wta_ref_target_local(key) -> allreduce_min(tkey) -> asw_wta_second(tar) -> allreduce_min(t2)
 *   asw_wta_ref_finalize.
 * The left second minimum is not exchanged: the reference's `confidence` receives the
 * target confidence last (K/asw_wta_ref.cl:64-66).  Equals asw_wta_ref bit for bit. */
int asw_wta_ref_local(const asw_params *p, const float *cost, const float *ref_l, int64_t *key, float *m1, float *m2,
                      void *stream);
int asw_wta_ref_target_local(const asw_params *p, const float *cost, const float *ref_r, const int64_t *key_ref,
                             int64_t *tkey, float *t1, float *t2, void *stream);
int asw_wta_ref_finalize(const asw_params *p, const int64_t *key, const int64_t *tkey, const float *t2,
                         int32_t *d_ref, int32_t *d_tar, float *conf_ref, uint8_t *code_ref, uint8_t *code_tar,
                         void *stream);

/* ---- refinement loop (main.cpp:540-623): k x (asw_ref_v, asw_ref_h on both views,
 * asw_WTA_REF, Constistency), then the 3x3 Median -> asw_disparity.png ----
 * Whole-volume contexts only (d_begin = 0, d_end = ndisp), ndisp <= 256, ASW_LR_U8:
 * the loop feeds disparities back through the reference's 8-bit codes. */
typedef struct asw_refine_params {
    int iters;      /* k refinement iterations (main.cpp:178: 6)                      */
    int taps;       /* window of asw_ref_v / asw_ref_h (K/asw_refinement_v.cl:33: 33)  */
    float gamma_c;  /* 10.94 (K/asw_refinement_v.cl:6)                                 */
    float gamma_g;  /* 118.78 (K/asw_refinement_v.cl:7)                                */
    float alpha;    /* penalty slope 0.085 (K/asw_wta_ref.cl:28); only 0.085 is built  */
} asw_refine_params;

void asw_refine_params_default(asw_refine_params *rp);
int asw_refine_params_check(const asw_params *p, const asw_refine_params *rp);
size_t asw_refine_lut_bytes(const asw_refine_params *rp);
/* weight table of the refinement kernels (asw_support_lut with the refinement falloffs) */
int asw_refine_lut(const asw_params *p, const asw_refine_params *rp, float *lut, void *stream);

/* replaces asw_ref_v (K/asw_refinement_v.cl:13-51), main.cpp:547-558.  est: u8
 * disparity codes read at `est_stride` bytes per pixel (4 = channel 0 of an RGBA8
 * image such as consistency_error, 1 = a plain code map).  out: [2][H][W] f32,
 * plane 0 = the refined disparity estimate num/den, plane 1 = den. */
int asw_ref_v(const asw_params *p, const asw_refine_params *rp, const uint8_t *img_rgba, const uint8_t *est,
              int est_stride, const float *conf, const float *lut, float *out, void *stream);
/* replaces asw_ref_h (K/asw_refinement_h.cl:16-53), main.cpp:561-573; in/out [2][H][W].
 * It reads no disparity: also accepted where asw_refine_native_params_check passes. */
int asw_ref_h(const asw_params *p, const asw_refine_params *rp, const uint8_t *img_rgba, const float *conf,
              const float *in, const float *lut, float *out, void *stream);
/* replaces asw_WTA_REF (K/asw_wta_ref.cl:2-68), main.cpp:576-586: first-argmin of
 * 0.085*den*|val - d| + C[d] (left) and the same along the target diagonal.
 * As the reference: conf_ref receives the TARGET confidence (its second store to
 * `confidence`), the target confidence array is not written. */
int asw_wta_ref(const asw_params *p, const float *cost, const float *ref_l, const float *ref_r, int32_t *d_ref,
                int32_t *d_tar, float *conf_ref, uint8_t *code_ref, uint8_t *code_tar, void *stream);
/* replaces Median (K/median.cl:58-88), main.cpp:615-617: 3x3 median of u8 codes
 * (stride 1 or 4 bytes per pixel), clamped borders; out = grey RGBA8. */
int asw_median3(const asw_params *p, const uint8_t *codes, int stride, uint8_t *out_rgba, void *stream);

/* The whole loop on device buffers.  In: the final aggregated volume `cost`, the
 * pre-refinement consistency image est_left_rgba (asw_consistency's out_rgba) and
 * target codes code_tar (asw_wta's), confidences after that consistency check.
 * All four are updated in place, as the reference's buffers are.  Out (any may be
 * NULL): post_red_rgba (asw_consistency_post-reff.png, written when iters > 0),
 * final_rgba (asw_disparity.png), d_ref / d_tar of the last asw_WTA_REF.
 * workspace: asw_refine_workspace_bytes() of device memory. */
size_t asw_refine_workspace_bytes(const asw_params *p, const asw_refine_params *rp);
int asw_refine(const asw_params *p, const asw_refine_params *rp, const uint8_t *left_rgba, const uint8_t *right_rgba,
               const float *cost, uint8_t *est_left_rgba, uint8_t *code_tar, float *conf_ref, float *conf_tar,
               void *workspace, uint8_t *post_red_rgba, uint8_t *final_rgba, int32_t *d_ref, int32_t *d_tar,
               void *stream);

/* ---- native refinement: the loop above on disparity INDICES (no reference counterpart:
 * the reference feeds disparities back through 8-bit images, which collide above 256 levels).
 * The estimates are int32 index maps, the outputs uint16 maps; any ndisp <= 65535, either
 * lr_mode.  Every operation is an IEEE float32 one in the stated order, no contraction: the
 * arithmetic of the 8-bit loop's kernels with the decode replaced (DESIGN.md §Native
 * refinement).  Per iteration, for both views:
 *   1. V estimate (asw_ref_v_native): asw_ref_v with Dv = (float)est[q] in place of
 *      (code/255)*(ndisp-1): over the taps i = 0..taps-1, q = (x, clamp(y+i-R)),
 *      t = w*conf[q]; num = num + t*Dv; den = den + t (num = den = 1e-5f on entry);
 *      out [2][H][W] = num/den, den.  Left view: est = est_left; right view: est = d_tar.
 *   2. H estimate: asw_ref_h, unchanged.
 *   3. asw_wta_ref with NULL code outputs: d_ref, d_tar, conf_ref <- the target confidence.
 *   4. asw_consistency_native: cons = |d_ref[p] - d_tar[p]| <= 1; where !cons both
 *      confidences are set to 0; est_left[p] = cons ? d_ref[p] : d_tar[p] (K/consist.cl
 *      writes the target value); post16[p] = cons ? d_ref[p] : ASW_DISP16_INVALID.
 * After the last iteration final16 = asw_median3_u16(est_left): the 3x3 clamp-to-edge median.
 * The first iteration starts from the pre-refinement maps: est_left built from the WTA's
 * d_ref / d_tar by the rule of step 4 (asw_consistency_native with NULL confidences), the
 * right estimate the WTA's d_tar, the confidences as asw_consistency left them.
 *
 * asw_refine_native_params_check: ASW_E_INVALID for a bad rp, ndisp > 65535 or a shard p
 * (d_begin > 0 or d_end < ndisp); ASW_E_UNSUPPORTED for alpha != 0.085.  asw_ref_h accepts
 * every (p, rp) this check or asw_refine_params_check accepts. */
int asw_refine_native_params_check(const asw_params *p, const asw_refine_params *rp);
/* asw_refine_lut's table (it depends on rp alone) under the native check */
int asw_refine_native_lut(const asw_params *p, const asw_refine_params *rp, float *lut, void *stream);
/* est: int32 [H][W] disparity indices; out: [2][H][W] f32 (num/den, den) */
int asw_ref_v_native(const asw_params *p, const asw_refine_params *rp, const uint8_t *img_rgba, const int32_t *est,
                     const float *conf, const float *lut, float *out, void *stream);
/* step 4.  conf_ref / conf_tar (zeroed in place), est_left and post16 may each be NULL;
 * est_left must not alias d_ref or d_tar.  Reads width, height, ndisp (<= 65535) of p. */
int asw_consistency_native(const asw_params *p, const int32_t *d_ref, const int32_t *d_tar, float *conf_ref,
                           float *conf_tar, int32_t *est_left, uint16_t *post16, void *stream);
/* 3x3 median, clamped borders, of an int32 index map; out: uint16 [H][W].  in != out. */
int asw_median3_u16(const asw_params *p, const int32_t *in, uint16_t *out, void *stream);
/* The whole loop on device buffers.  In: the final aggregated volume `cost`; est_left, the
 * target map d_tar and both confidences as described above, all four updated in place
 * (d_tar ends as the last asw_wta_ref's target map).  Out (any may be NULL): post16
 * (written when iters > 0), final16, d_ref of the last asw_wta_ref (iters > 0).
 * workspace: asw_refine_native_workspace_bytes() of device memory. */
size_t asw_refine_native_workspace_bytes(const asw_params *p, const asw_refine_params *rp);
int asw_refine_native(const asw_params *p, const asw_refine_params *rp, const uint8_t *left_rgba,
                      const uint8_t *right_rgba, const float *cost, int32_t *est_left, int32_t *d_tar, float *conf_ref,
                      float *conf_tar, void *workspace, uint16_t *post16, uint16_t *final16, int32_t *d_ref,
                      void *stream);

/* ---- Cross-based matcher with orthogonal integral images: the reference's first method
 * (main.cpp:243-411; K/median.cl, cross.cl, aggregation.cl, integral_h.cl, oii_hcross.cl,
 * integral_v.cl, oii_vcross.cl, init_disparity.cl, disparity.cl), one call per reference
 * kernel.  IEEE float32 in the reference's order.  Whole-volume
 * p only (d_begin = 0, d_end = ndisp) with 2 <= ndisp <= 256 (8-bit codes); reads width,
 * height and ndisp of p.  Volumes are [H][W][Dp] float32 like every cost volume; an arm
 * map is [H][W] of four signed bytes (h-, h+, v-, v+) = (-a, +a, -a, +a), a in
 * [1, arm_max] (the reference: four int planes).  The volume stages launch one work-item per
 * element (asw_cross_cost, asw_cross_oii) or one wave per 64 planes of a line
 * (asw_cross_integral); a launch holds at most 2^32 - 1 work-items, so width * height * Dp
 * >= 2^32 - 255 elements (or, for the integral, lines * Dp >= 2^32 - 255) is
 * ASW_E_UNSUPPORTED (no kernel is launched). */
typedef struct asw_cross_params {
    int arm_max; /* longest arm (K/cross.cl:32-80: 25), 1..127                            */
    int tau;     /* colour similarity in 8-bit units, 0..255: 25 is exactly the reference's
                    |delta| / 255 < 0.10f (K/cross.cl:11-13)                              */
} asw_cross_params;
void asw_cross_params_default(asw_cross_params *cp);
int asw_cross_params_check(const asw_params *p, const asw_cross_params *cp);
size_t asw_cross_arm_bytes(const asw_params *p); /* H*W*4 */
/* Median (K/median.cl:58-88, main.cpp:272-280) of an RGBA8 image: per channel, 3x3,
 * clamp-to-edge, alpha 255.  in != out. */
int asw_median3_rgba(const asw_params *p, const uint8_t *in_rgba, uint8_t *out_rgba, void *stream);
/* Cross (K/cross.cl, main.cpp:284-292) on a median image.  Per direction: a = 1; for
 * k = 1..arm_max, q = p + (k+1) dir is accepted (a = k) when it lies inside the image,
 * k - a <= 1 and every colour channel is within tau of the ANCHOR p. */
int asw_cross_arms(const asw_params *p, const asw_cross_params *cp, const uint8_t *med_rgba, int8_t *arms,
                   void *stream);
/* Aggregation (K/aggregation.cl, main.cpp:296-299): with f(c) = (float)c / 255.0f,
 * cost[y][x][d] = (|f(Lr)-f(Rr)| + |f(Lg)-f(Rg)|) + |f(Lb)-f(Rb)| between medL(x, y) and
 * medR(max(x-d, 0), y); padding planes are written 0. */
int asw_cross_cost(const asw_params *p, const uint8_t *med_left_rgba, const uint8_t *med_right_rgba, float *cost,
                   void *stream);
/* Integral_h / Integral_v (main.cpp:304-306, :322-324), in place: the serial running sum
 * along x (ASW_DIR_H, from x = 0) or y (ASW_DIR_V, from y = 0) of every plane < ndisp.
 * Padding planes are neither read nor written. */
int asw_cross_integral(const asw_params *p, int dir, float *vol, void *stream);
/* Oii_hcross / Oii_vcross (K/oii_hcross.cl:13-31, main.cpp:312-317, :329-334).  With
 * xr = max(0, x-d), m = max(armsR[y][xr].minus, armsL[y][x].minus) and
 * pl = min(armsR[y][xr].plus, armsL[y][x].plus) of the direction's arms:
 *   H: out[y][x][d] = (in[y][min(W-1, x+pl)][d] - in[y][max(0, x+m-1)][d]) / (float)(pl - m)
 *   V: out[y][x][d] = (in[min(H-1, y+pl)][x][d] - in[max(0, y+m-1)][x][d]) / (float)(pl - m)
 * (the reference's off-by-one at the lower end and its divisor, kept).  Padding planes of
 * `in` are never read, those of `out` are written 0.  in != out. */
int asw_cross_oii(const asw_params *p, int dir, const int8_t *arms_left, const int8_t *arms_right, const float *in,
                  float *out, void *stream);
/* Init_disparity (K/init_disparity.cl, main.cpp:339-341): d0 = the first strict minimum of
 * vol over d in [0, ndisp), code0 = its 8-bit code (the rule of asw_wta).  d0 or code0 may
 * be NULL. */
int asw_cross_init(const asw_params *p, const float *vol, int32_t *d0, uint8_t *code0, void *stream);
/* Disparity (K/disparity.cl, main.cpp:346-349): for pixel (x, y) with its own arms
 * (vm, vp), every row i = vm..vp at yc = clamp(y+i), with (hm, hp) = armsL[yc][x], every
 * j = hm..hp votes bin (int)(((float)code0[yc][clamp(x+j)] / 255.0f) * (float)(ndisp-1));
 * d1 = the LAST bin with the largest count, code1 its 8-bit code.  d1 or code1 may be NULL;
 * code0 != code1. */
int asw_cross_vote(const asw_params *p, const uint8_t *code0, const int8_t *arms_left, int32_t *d1, uint8_t *code1,
                   void *stream);

/* tuning hook (benchmarks / kernel experiments): selects among compiled kernel
 * variants; returns the previous value, or ASW_E_INVALID for an unknown key.
 * Every variant computes bit-identical results. */
#define ASW_TUNE_PASS_VARIANT 1 /* aggregation passes, a bit set: 128 H by k_hpass9, 4096 H by k_hpass11 at any
                                  frame size, 0xF00 k_hpass11's segment length in window periods; bit 26 flips the
                                  cache policy of the cost / den / output streams (nt from 256 MiB of volume on)
                                  in the 64-lane V passes, k_hpass9 and the 32-plane passes (k_hpass11 is nt
                                  always); bits 16-23 the 32-plane passes' strip / segment counts */
#define ASW_TUNE_WTA_VARIANT 2 /* asw_wta: 0 lane-per-pixel scan (default), 2 row sweep (Dp 64/128/256; the
                                  scan elsewhere); 1 (round 1's wave per pixel) is no longer built */
int asw_tune_set(int key, int value);
/* the kernel instantiation the most recent aggregation-pass launch of (dir, den_mode)
 * in this process ran, e.g. "k_vpass10<T=35,NW=16,DM=2,nt>" (NUL-terminated, at most
 * len bytes): lets a test assert which compiled form a shape selects.  ASW_E_INVALID
 * when no such pass has been launched yet. */
int asw_pass_kernel(int dir, int den_mode, char *buf, int len);

/* ---------------- FRAME API (host pointers, synchronous) ---------------- */

typedef struct asw_ctx asw_ctx;

typedef struct asw_outputs { /* caller-owned host arrays; any may be NULL */
    int32_t *d_ref, *d_tar;  /* [H][W] disparity indices (left, right view)     */
    float *conf_ref, *conf_tar;
    uint8_t *disp_rgba;      /* [H][W][4] 8-bit disparity image (asw_left_wta)  */
    uint8_t *lr_rgba;        /* [H][W][4] consistency output ("consistency_error") */
    uint8_t *lr_red_rgba;    /* [H][W][4] asw_consistency_pre-reff.png image    */
    float *cost;             /* [H][W][Dp] final aggregated volume (optional)   */
    uint8_t *final_rgba;     /* [H][W][4] asw_disparity.png (refinement on)     */
    uint8_t *post_red_rgba;  /* [H][W][4] asw_consistency_post-reff.png (refinement on) */
    /* 16-bit disparity images: the 8-bit codes of K/asw_wta.cl:70-74
     * collide above D = 256 (C5: D = 512); these hold the disparity index itself. */
    uint16_t *disp16;        /* [H][W] d_ref                                              */
    uint16_t *lr16;          /* [H][W] d_ref where the LR check passes, else ASW_DISP16_INVALID
                                (the asw_consistency_pre-reff image; lr_check only)        */
} asw_outputs;
#define ASW_DISP16_INVALID 0xFFFF

typedef struct asw_timings { /* milliseconds from HIP events, columns of main.cpp:181 */
    double raw_cost, support, v_pass_mean, h_pass_mean, aggregation_total, wta, consistency, total;
    double h2d, d2h;
    double refine;           /* refinement loop + median (0 when off) */
    double exchange;         /* multi-GPU contexts: the WTA exchange (4 MIN all-reduces) */
} asw_timings;

/* marketing name of a HIP device (the reference names its TSV after the OpenCL
 * device, main.cpp:164-166); writes a NUL-terminated string of at most len bytes. */
int asw_device_name(int hip_device, char *buf, int len);

/* A context owns the device buffers of one image size, sized at create and reused
 * by every asw_match (the reference re-creates its cl_mem objects per run,
 * main.cpp:243-457).  p->d_begin / d_end must cover the whole range: contexts
 * shard the disparity axis themselves.  Shapes whose volume rows or support arrays
 * exceed the pass kernels' 32-bit offsets (e.g. 7680x4320 at D = 512) are rejected
 * here with ASW_E_UNSUPPORTED, before anything is allocated.
 *
 * asw_create: one GPU (HIP device ordinal), the whole disparity range. */
int asw_create(const asw_params *p, int hip_device, asw_ctx **out);
/* One process, n_devices GPUs: [0, ndisp) is split into n_devices
 * contiguous shards, shard i on hip_device_ids[i].  Raw cost, supports and the 2r
 * passes of a shard touch only its planes (no communication); the WTA is the one
 * exchange: 4 elementwise MIN all-reduces of S-element arrays (int64 keys
 * (float_bits(m1) << 32 | d) and float second minima, the asw_wta_local protocol).
 * They run over RCCL (ncclAllReduce / ncclMin in one ncclGroupStart/End, one
 * communicator per device from ncclCommInitAll) when the ids are distinct, and as
 * peer copies + a MIN kernel on hip_device_ids[0] when an id repeats (several
 * shards on one GPU).  The LR check and every output are on hip_device_ids[0];
 * results equal a one-GPU context bit for bit. */
int asw_create_multi(const asw_params *p, const int *hip_device_ids, int n_devices, asw_ctx **out);
/* Multi-process (one process per GPU): this process is shard `rank` of `nranks`,
 * the all-reduces run over an RCCL communicator made from `id` (ncclCommInitRank);
 * asw_comm_unique_id makes the id on one rank (ncclGetUniqueId) and the caller
 * shares it with the others (MPI, torch.distributed, a file).  Every rank returns
 * the whole frame's maps and images; the one exception is asw_outputs.cost, which
 * a rank fills only at its own planes [d_begin, d_end) (asw_ctx_shard) and leaves
 * untouched elsewhere (the volume is never gathered).
 * The cross-device RCCL path (distinct GPUs, nranks > 1, or asw_create_multi with
 * distinct ids) runs the same protocol as the tested one-rank and same-device
 * paths; it has not been executed on a multi-GPU box by this project's tests. */
#define ASW_COMM_ID_BYTES 128
int asw_comm_unique_id(uint8_t id[ASW_COMM_ID_BYTES]);
int asw_create_rank(const asw_params *p, int hip_device, int rank, int nranks, const uint8_t id[ASW_COMM_ID_BYTES],
                    asw_ctx **out);
/* shard layout of a context: number of shards it drives in this process and the
 * [d_begin, d_end) of shard i (ASW_E_INVALID for i out of range) */
int asw_ctx_shard(const asw_ctx *ctx, int i, int *n_shards, int *d_begin, int *d_end);
int asw_destroy(asw_ctx *ctx);
/* One stereo pair, host RGBA8 in, host outputs out (any output pointer may be NULL). */
int asw_match(asw_ctx *ctx, const uint8_t *left_rgba, const uint8_t *right_rgba, asw_outputs *out,
              asw_timings *t);
/* `batch` pairs (SURVEY §8(b) `asw_match(ctx, L, R, batch, ...)`): left_rgba /
 * right_rgba hold `batch` consecutive [H][W][4] images, out[b] and t[b] (t may be
 * NULL) receive pair b.  The pairs stream through the context's one set of
 * volumes (a 3840x2160 D512 pair needs ~75 GB with cached denominators; 8 of them
 * are never resident together). */
int asw_match_batch(asw_ctx *ctx, const uint8_t *left_rgba, const uint8_t *right_rgba, int batch,
                    asw_outputs *out, asw_timings *t);
/* turn the refinement loop on for later asw_match calls (rp = NULL or iters = 0:
 * off, the default).  Needs lr_check.  On a multi-shard context the loop's volume
 * scan (asw_WTA_REF) is d-sharded and exchanged like the WTA (asw_wta_ref_local
 * protocol); the per-pixel stages run on the first shard.  asw_match then
 * fills final_rgba / post_red_rgba; every other output (d_ref, d_tar, conf_*,
 * disp_rgba, lr_rgba, lr_red_rgba, disp16, lr16) stays the pre-refinement result
 * (they are copied out before the loop updates its buffers in place). */
int asw_set_refine(asw_ctx *ctx, const asw_refine_params *rp);
/* The native refinement loop (asw_refine_native) inside asw_match, for the contexts the
 * 8-bit loop is not built for (ndisp > 256, ASW_LR_NATIVE) and any other: caller-owned host
 * arrays, any may be NULL.  asw_set_refine_native checks rp (asw_refine_native_params_check),
 * copies both structs and allocates the loop's device buffers once; every later asw_match
 * runs the loop after the pre-refinement outputs have left and fills the registered arrays
 * (asw_match_batch: pair b at offset b*H*W of each).  rp = NULL or iters = 0: off (the
 * default; a frame then launches and allocates nothing new); o = NULL with the loop on:
 * ASW_E_INVALID.  Needs lr_check; ASW_E_INVALID while asw_set_refine is on (and
 * asw_set_refine returns ASW_E_INVALID while this loop is on): one loop per context.  Its
 * time is asw_timings.refine.  With asw_set_graph on the loop is captured and replayed like
 * the 8-bit one.  Multi-shard contexts run the volume scan through the asw_wta_ref_local
 * protocol and the per-pixel stages on the first shard, bit-identical to one GPU (with
 * asw_create_rank every rank must switch the loop alike: the all-reduces are collective).
 * Every other output stays the pre-refinement result. */
typedef struct asw_refine_native_outputs {
    uint16_t *final16;      /* [H][W] 3x3 median of the last est_left (asw_disparity16.png)          */
    uint16_t *post16;       /* [H][W] d_ref of the last iteration where consistent, else
                               ASW_DISP16_INVALID (asw_consistency_post16.png)                      */
    int32_t *d_ref, *d_tar; /* [H][W] the last asw_wta_ref's maps                                   */
} asw_refine_native_outputs;
int asw_set_refine_native(asw_ctx *ctx, const asw_refine_params *rp, const asw_refine_native_outputs *o);
/* on != 0: from the next asw_match on, the frame's device work (raw cost to the
 * consistency images, and the refinement loop) is captured once into HIP graphs
 * (hipStreamBeginCapture) and replayed: one launch per graph instead of ~25 (+37 for
 * the loop) kernel launches, for small, launch-bound frames.  Same results.  Only
 * the coarse timings (h2d, total, refine, d2h) are measured.  One-shard contexts. */
int asw_set_graph(asw_ctx *ctx, int on);
/* Sub-pixel float maps of the left view (asw_subpixel, asw_disp_mask, asw_disp_fill):
 * caller-owned host [H][W] float32 arrays, any may be NULL.  asw_set_subpixel copies
 * the struct and allocates the device maps once; every later asw_match fills the
 * registered arrays (asw_match_batch: pair b at offset b*H*W of each).  o = NULL: off
 * (the default; a frame then launches nothing new).  disp_lr / disp_filled need
 * lr_check (ASW_E_INVALID without).  The maps are pre-refinement results like every
 * other map.  A multi-shard context runs the asw_subpixel_local protocol: one more MIN
 * all-reduce ([3][S] float32), maps on the first shard, bit-identical to one GPU (with
 * asw_create_rank every rank must turn the maps on or off alike: the all-reduce is
 * collective; every rank then receives the maps).  With
 * asw_set_graph on the kernels run on the stream after the graph replay (not captured).
 * Their time is inside asw_timings.total and in no stage column. */
typedef struct asw_subpixel_outputs {
    float *disp;        /* d_ref + parabola offset                                  */
    float *disp_lr;     /* disp where the LR check passes, else NaN                 */
    float *disp_filled; /* disp_lr with the holes filled from the row's background  */
} asw_subpixel_outputs;
int asw_set_subpixel(asw_ctx *ctx, const asw_subpixel_outputs *o);
/* The cross-based matcher (main.cpp:243-411) inside asw_match: caller-owned host arrays,
 * any may be NULL.  asw_set_cross copies both structs and allocates the two arm maps, the
 * two median images and the code maps once; every later asw_match runs the cross stages
 * BEFORE the ASW stages, as the reference does, in the context's two cost volumes (which
 * the ASW stages overwrite afterwards), and fills the registered arrays (asw_match_batch:
 * pair b at offset b*H*W pixels of each array, timings[b]).  cp = NULL: off (the default;
 * a frame then launches nothing new); o = NULL with cp set: ASW_E_INVALID.  The stages
 * are never captured (asw_set_graph: they run on the stream before the replay) and their
 * time is in no asw_timings column.  One-shard contexts only: asw_create_multi /
 * asw_create_rank contexts with more than one shard return ASW_E_UNSUPPORTED (their
 * volumes are shard-sized). */
typedef struct asw_cross_timings { /* milliseconds, the columns of main.cpp:394-410 */
    double median[2], cross[2];    /* left, right image                               */
    double aggregation, integral_h, oii_h, integral_v, oii_v, init, vote;
    double total;                  /* first median start to vote end                  */
} asw_cross_timings;
typedef struct asw_cross_outputs {
    uint8_t *initial_rgba;      /* [H][W][4] cross_based_initial.png                          */
    uint8_t *final_rgba;        /* [H][W][4] cross_based_disparity.png (3x3 median of the vote) */
    uint8_t *median_left_rgba;  /* [H][W][4] median.png                                        */
    int32_t *d_initial;         /* [H][W] initial disparity indices                            */
    asw_cross_timings *timings;
} asw_cross_outputs;
int asw_set_cross(asw_ctx *ctx, const asw_cross_params *cp, const asw_cross_outputs *o);
/* The census / AD-census cost in place of the AD raw cost of later asw_match calls
 * (cp = NULL: off, the default; a frame then launches and allocates nothing new).
 * asw_set_census checks cp against the context (asw_census_params_check), copies it and
 * allocates the two census maps of every shard once (freed at asw_destroy).  A shard then
 * runs asw_census on both images and asw_census_cost16 into its raw-cost volume where it
 * would have run asw_raw_cost16 (the first V pass stays asw_aggregate_pass_den16), and
 * asw_census_cost elsewhere (ASW_FLAG_RAW_F32, a non-integral tad_tau with w_a > 0, a tap
 * count without a ring kernel).  The three launches are timed in asw_timings.raw_cost.
 * Every context kind works: each shard repeats the d-independent transform and computes its
 * own planes, with no new collective (with asw_create_rank every rank must switch census
 * alike, or the ranks aggregate different costs).  With asw_set_graph on the launches are
 * inside the captured frame: asw_set_census drops a captured frame graph, the next
 * asw_match captures again.  Refinement, the sub-pixel maps, the LR modes and the
 * cross-based stages (which keep their own cost) are untouched. */
int asw_set_census(asw_ctx *ctx, const asw_census_params *cp);
/* Semi-global matching (asw_sgm) in place of the supports and the 2r ASW passes of later
 * asw_match calls (sp = NULL: off, the default; a frame then launches and allocates nothing
 * new).  asw_set_sgm checks sp against the context (asw_sgm_params_check) and copies it; the
 * workspace (asw_sgm_workspace_bytes) is allocated once.  A frame then writes the raw cost in
 * its uint16 form (asw_raw_cost16, or with census on asw_census x 2 and asw_census_cost16)
 * into one of the context's two cost volumes and asw_sgm's sums into the other; the WTA and
 * everything after it (LR check, 16-bit and sub-pixel maps, both refinement loops,
 * asw_outputs.cost) read that volume.  The supports and passes are not launched: taps and
 * iters are not read (any tap count, iters = 0 included), and ASW_FLAG_RAW_F32 is ignored.
 * ASW_E_UNSUPPORTED: a context with more than one shard (m is a minimum over every
 * disparity), and a cost without a uint16 form (asw_raw_cost16's / asw_census_cost16's
 * ASW_E_UNSUPPORTED: a fractional tad_tau below 765 with an AD term); asw_set_census returns
 * ASW_E_UNSUPPORTED for such a form while SGM is on.  The context is unchanged after an error.
 * Timings: the SGM launches are asw_timings.aggregation_total; support, v_pass_mean and
 * h_pass_mean are 0.  With asw_set_graph on the launches are inside the captured frame:
 * asw_set_sgm drops a captured frame graph, the next asw_match captures again.  The
 * refinement penalty 0.085 * den * |val - d| was tuned against ASW-scale costs: the loops
 * run on the sums unchanged, their quality there is not claimed. */
int asw_set_sgm(asw_ctx *ctx, const asw_sgm_params *sp);
/* The speckle filter (asw_speckle) on the frame's pre-refinement d_ref: caller-owned host
 * arrays, any may be NULL.  asw_set_speckle checks sp (asw_speckle_params_check), copies both
 * structs and allocates the device maps and the workspace once; every later asw_match fills the
 * registered arrays (asw_match_batch: pair b at offset b*H*W of each).  sp = NULL: off (the
 * default; a frame then launches and allocates nothing new); o = NULL with sp set:
 * ASW_E_INVALID, and so is filtered16 at ndisp > 65535.  valid is the LR rule (asw_lr_valid)
 * on a context with lr_check, every pixel otherwise.  The kernels run on the first shard's
 * stream after the consistency stage and the sub-pixel work, before the pre-refinement maps
 * leave; with asw_set_graph on they run after the replay (not captured).  Their time is inside
 * asw_timings.total and in no stage column.  disp_lr / disp_filled need the sub-pixel disp: the
 * frame computes it once for asw_set_subpixel and for these outputs (a multi-shard context: the
 * same one extra MIN all-reduce; with asw_create_rank every rank must switch alike).  The filter
 * itself is per-pixel work on maps every rank holds: no new collective.  Works with census, SGM,
 * both LR modes, any ndisp and any number of shards. */
typedef struct asw_speckle_outputs {
    uint16_t *filtered16;   /* [H][W] d_ref where valid and kept, else ASW_DISP16_INVALID            */
    int32_t  *size;         /* [H][W] component size, 0 where invalid                                */
    uint8_t  *keep;         /* [H][W]                                                                */
    float    *disp_lr;      /* [H][W] sub-pixel disp where valid and kept, else NaN                  */
    float    *disp_filled;  /* [H][W] asw_disp_fill of disp_lr                                       */
} asw_speckle_outputs;
int asw_set_speckle(asw_ctx *ctx, const asw_speckle_params *sp, const asw_speckle_outputs *o);

#ifdef __cplusplus
}
#endif
#endif /* ASW_H */
