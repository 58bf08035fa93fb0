// asw_frame.cpp — FRAME half of the C-ABI (include/asw.h): a context owns the
// device buffers of one image size and runs the reference's ASW sequence for a
// stereo pair (main.cpp:243-244 upload, :463-537 kernels, :540-623 refinement,
// :621-631 read-back), with HIP events in place of the reference's OpenCL
// profiling events (main.cpp:634-708).
//
// A context drives one or more SHARDS: contiguous disparity ranges, each with its
// own device, stream and volumes (the reference runs one device per pass of its
// device loop, main.cpp:158-172; it has no multi-device path).  Shards need no
// communication until the WTA, which is the exchange of the d-sharded protocol
// (asw_wta_local ... asw_wta_finalize): four elementwise MIN all-reduces, over
// RCCL when the shards' devices are distinct (one process: ncclCommInitAll; one
// process per GPU: ncclCommInitRank), else over peer copies and a MIN kernel on
// the first shard's device (several shards on one GPU).
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "asw_common.h"

namespace {

constexpr int kMaxShards = 64;

enum CommMode { COMM_NONE = 0, COMM_RCCL = 1, COMM_LOCAL = 2 };

struct Shard {
    int device = 0;
    hipStream_t stream = nullptr;
    asw_params p{};                     // this shard's [d_begin, d_end)
    uint8_t *left = nullptr, *right = nullptr;  // RGBA8 [H][W][4]
    float *lut = nullptr;
    float *lab_l = nullptr, *lab_r = nullptr;  // float4 [H][W] (ASW_COLOR_LAB only)
    float *wvl = nullptr, *wvr = nullptr, *whl = nullptr, *whr = nullptr;  // [H][W][Tp]
    float *c0 = nullptr, *c1 = nullptr;                                    // [H][W][Dp]
    float *den_v = nullptr, *den_h = nullptr;  // cached denominators (iters >= 2)
    bool raw16 = false; // the raw costs as uint16 in c0 (asw_raw_cost16 + asw_aggregate_pass_den16)
    // d-sharded WTA (more than one shard in the frame)
    int64_t *key = nullptr, *key_g = nullptr, *tkey = nullptr, *tkey_g = nullptr;
    float *m1 = nullptr, *m2 = nullptr, *t1 = nullptr, *t2 = nullptr, *m2_g = nullptr, *t2_g = nullptr;
    ncclComm_t comm = nullptr;
    hipEvent_t ready = nullptr;  // COMM_LOCAL: this shard's operand is complete
    float *ref_l = nullptr, *ref_r = nullptr;  // sharded refinement, shards > 0: the per-view estimates
    float *nb = nullptr;  // asw_set_subpixel on a sharded frame: [3][S] neighbour costs of the winner
    uint64_t *cen_l = nullptr, *cen_r = nullptr;  // asw_set_census: the census codes of both images, [H][W]
    bool census16 = false;  // census on: the costs as uint16 in c0 (asw_census_cost16 + asw_aggregate_pass_den16)
};

}  // namespace

struct asw_ctx {
    asw_params p{};          // the whole frame
    int n = 0;               // shards driven by this process
    int rank = 0, nranks = 1;  // multi-process: this process's shard of nranks (n = 1)
    CommMode comm = COMM_NONE;
    Shard sh[kMaxShards];
    void *red_tmp = nullptr;  // COMM_LOCAL: (n-1) x S int64 operands copied to shard 0's device
    hipEvent_t red_done = nullptr;
    // outputs, on shard 0's device
    int32_t *d_ref = nullptr, *d_tar = nullptr;
    float *conf_ref = nullptr, *conf_tar = nullptr;
    uint8_t *code_ref = nullptr, *code_tar = nullptr;
    uint8_t *lr = nullptr, *lr_red = nullptr, *disp = nullptr;  // RGBA8
    uint16_t *disp16 = nullptr, *lr16 = nullptr;
    // refinement loop (asw_set_refine): parameters, workspace, its estimate image
    // (a copy of lr, refined in place) and outputs
    asw_refine_params rp{};
    bool refine = false;
    void *rws = nullptr;
    uint8_t *est = nullptr, *post_red = nullptr, *final_rgba = nullptr;  // RGBA8
    // native refinement loop (asw_set_refine_native): parameters, the registered host arrays,
    // workspace, the int32 estimate / target / reference maps the loop updates and its uint16 outputs
    asw_refine_params nrp{};
    asw_refine_native_outputs nro{};
    bool nrefine = false;
    void *nrws = nullptr;
    int32_t *n_est = nullptr, *n_dt = nullptr, *n_dr = nullptr;
    uint16_t *n_post16 = nullptr, *n_final16 = nullptr;
    std::vector<hipEvent_t> ev;  // timing events on shard 0's stream
    // asw_set_graph: the frame's device work captured once into HIP graphs, replayed
    bool graph = false;
    hipGraph_t g_main = nullptr, g_ref = nullptr;
    hipGraphExec_t gx_main = nullptr, gx_ref = nullptr;
    // asw_set_subpixel: the registered host arrays and their device maps (shard 0's device)
    asw_subpixel_outputs sub{};
    bool sub_on = false;
    float *sp_disp = nullptr, *sp_lr = nullptr, *sp_fill = nullptr;
    // asw_set_cross: the cross-based matcher (main.cpp:243-411) ahead of the ASW stages, in
    // shard 0's two cost volumes; its own maps and images (RGBA8) and timing events
    asw_cross_params cp{};
    asw_cross_outputs cro{};
    bool cross_on = false;
    uint8_t *cr_med_l = nullptr, *cr_med_r = nullptr, *cr_init = nullptr, *cr_final = nullptr;
    int8_t *cr_arms_l = nullptr, *cr_arms_r = nullptr;
    int32_t *cr_d0 = nullptr;
    uint8_t *cr_code0 = nullptr, *cr_code1 = nullptr;
    std::vector<hipEvent_t> cr_ev;
    // asw_set_census: the census / AD-census cost in place of the AD raw cost
    asw_census_params cen{};
    bool census_on = false;
    // asw_set_sgm: semi-global matching in place of the supports and the 2r passes: the raw
    // cost as uint16 in shard 0's c1, asw_sgm's sums in its c0 (what the WTA onwards reads)
    asw_sgm_params sgm{};
    bool sgm_on = false;
    void *sgm_ws = nullptr;
    // asw_set_speckle: the speckle filter on the pre-refinement d_ref: parameters, the registered
    // host arrays, the validity map (lr_check), workspace and device maps (shard 0's device)
    asw_speckle_params spk{};
    asw_speckle_outputs spo{};
    bool spk_on = false;
    uint8_t *spk_valid = nullptr, *spk_keep = nullptr;
    void *spk_ws = nullptr;
    int32_t *spk_size = nullptr;
    uint16_t *spk_f16 = nullptr;
    float *spk_lr = nullptr, *spk_fill = nullptr;
};

namespace {

int hip_fail(hipError_t e) {
    asw::set_hip_error(e);
    return e == hipErrorOutOfMemory ? ASW_E_NOMEM : ASW_E_HIP;
}

#define HIPCHK(expr)                               \
    do {                                           \
        const hipError_t _e = (expr);              \
        if (_e != hipSuccess) return hip_fail(_e); \
    } while (0)

#define ASWCHK(expr)                 \
    do {                             \
        const int _s = (expr);       \
        if (_s != ASW_OK) return _s; \
    } while (0)

#define NCCLCHK(expr)                                \
    do {                                             \
        const ncclResult_t _r = (expr);              \
        if (_r != ncclSuccess) return ASW_E_COMM;    \
    } while (0)

template <class T>
int dev_alloc(T **ptr, size_t bytes) {
    void *v = nullptr;
    HIPCHK(hipMalloc(&v, bytes));
    *ptr = static_cast<T *>(v);
    return ASW_OK;
}

double ms_between(hipEvent_t a, hipEvent_t b) {
    float ms = 0.0f;
    if (hipEventElapsedTime(&ms, a, b) != hipSuccess) return -1.0;
    return (double)ms;
}

// grey RGBA image of the 8-bit codes (asw_left_wta written by K/asw_wta.cl:73)
__global__ void k_codes_to_rgba(long long n, const uint8_t *code, uchar4 *out) {
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p < n) {
        const uint8_t c = code[p];
        out[p] = make_uchar4(c, c, c, 255);
    }
}

// 16-bit disparity images: d_ref, and d_ref where the LR check of asw_consistency
// (same rule: 8-bit codes or native indices) passes, ASW_DISP16_INVALID elsewhere
__global__ void k_disp16(long long n, int D, int mode, int lr, const int32_t *d_ref, const int32_t *d_tar,
                         const uint8_t *code_ref, const uint8_t *code_tar, uint16_t *disp16, uint16_t *lr16) {
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const int dr = d_ref[p];
    if (disp16) disp16[p] = (uint16_t)dr;
    if (!lr16 || !lr) return;
    const bool cons = asw::lr_consistent(mode, D, p, dr, d_tar, code_ref, code_tar);
    lr16[p] = cons ? (uint16_t)dr : (uint16_t)ASW_DISP16_INVALID;
}

// elementwise MIN of n operands (COMM_LOCAL all-reduce), written to out
struct MinOperands {
    const void *p[kMaxShards];
    int n;
};
template <class T>
__global__ void k_min_n(long long count, MinOperands ops, T *out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    T v = static_cast<const T *>(ops.p[0])[i];
    for (int k = 1; k < ops.n; ++k) {
        const T o = static_cast<const T *>(ops.p[k])[i];
        v = o < v ? o : v;
    }
    out[i] = v;
}

size_t frame_pixels(const asw_params *p) { return (size_t)p->width * p->height; }

// In-place elementwise MIN all-reduce of buf(shard) (count elements of T) over
// every shard of the frame.  Stream-ordered on each shard's stream
// (`per_pixel` elements per pixel: 1 for the WTA's maps, 3 for the sub-pixel neighbours).
template <class T>
int allreduce_min(asw_ctx *c, T *(*buf)(Shard &), ncclDataType_t type, int per_pixel = 1) {
    const size_t S = frame_pixels(&c->p) * (size_t)per_pixel;
    if (c->comm == COMM_RCCL) {
        NCCLCHK(ncclGroupStart());
        for (int i = 0; i < c->n; ++i) {
            Shard &s = c->sh[i];
            T *b = buf(s);
            const ncclResult_t r = ncclAllReduce(b, b, S, type, ncclMin, s.comm, s.stream);
            if (r != ncclSuccess) {
                (void)ncclGroupEnd();
                return ASW_E_COMM;
            }
        }
        NCCLCHK(ncclGroupEnd());
        return ASW_OK;
    }
    if (c->comm != COMM_LOCAL) return ASW_OK;  // one shard: nothing to reduce
    Shard &s0 = c->sh[0];
    MinOperands ops{};
    ops.n = c->n;
    for (int i = 0; i < c->n; ++i) {
        Shard &s = c->sh[i];
        HIPCHK(hipSetDevice(s.device));
        HIPCHK(hipEventRecord(s.ready, s.stream));
    }
    HIPCHK(hipSetDevice(s0.device));
    for (int i = 0; i < c->n; ++i) HIPCHK(hipStreamWaitEvent(s0.stream, c->sh[i].ready, 0));
    T *tmp = static_cast<T *>(c->red_tmp);
    for (int i = 0; i < c->n; ++i) {
        Shard &s = c->sh[i];
        if (s.device == s0.device) {
            ops.p[i] = buf(s);  // same device: read in place
        } else {
            T *dst = tmp + (size_t)(i - 1) * S;
            HIPCHK(hipMemcpyPeerAsync(dst, s0.device, buf(s), s.device, S * sizeof(T), s0.stream));
            ops.p[i] = dst;
        }
    }
    hipLaunchKernelGGL(k_min_n<T>, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, s0.stream, (long long)S, ops,
                       buf(s0));
    HIPCHK(hipGetLastError());
    for (int i = 1; i < c->n; ++i) {
        Shard &s = c->sh[i];
        if (s.device == s0.device)
            HIPCHK(hipMemcpyAsync(buf(s), buf(s0), S * sizeof(T), hipMemcpyDeviceToDevice, s0.stream));
        else
            HIPCHK(hipMemcpyPeerAsync(buf(s), s.device, buf(s0), s0.device, S * sizeof(T), s0.stream));
    }
    HIPCHK(hipEventRecord(c->red_done, s0.stream));
    for (int i = 1; i < c->n; ++i) {
        HIPCHK(hipSetDevice(c->sh[i].device));
        HIPCHK(hipStreamWaitEvent(c->sh[i].stream, c->red_done, 0));
    }
    return ASW_OK;
}

int64_t *b_key_g(Shard &s) { return s.key_g; }
int64_t *b_tkey_g(Shard &s) { return s.tkey_g; }
float *b_m2_g(Shard &s) { return s.m2_g; }
float *b_t2_g(Shard &s) { return s.t2_g; }
float *b_nb(Shard &s) { return s.nb; }

void free_shard(Shard &s) {
    if (s.stream == nullptr && s.left == nullptr) return;
    (void)hipSetDevice(s.device);
    void *bufs[] = {s.left, s.right, s.lut, s.lab_l, s.lab_r, s.wvl, s.wvr, s.whl, s.whr, s.c0, s.c1, s.den_v,
                    s.den_h, s.key, s.key_g, s.tkey, s.tkey_g, s.m1, s.m2, s.t1, s.t2, s.m2_g, s.t2_g, s.ref_l,
                    s.ref_r, s.nb, s.cen_l, s.cen_r};
    for (void *b : bufs)
        if (b) (void)hipFree(b);
    if (s.comm) (void)ncclCommDestroy(s.comm);
    if (s.ready) (void)hipEventDestroy(s.ready);
    if (s.stream) (void)hipStreamDestroy(s.stream);
    s = Shard{};
}

int alloc_shard(Shard &s, bool sharded) {
    const asw_params *p = &s.p;
    const size_t S = frame_pixels(p);
    HIPCHK(hipSetDevice(s.device));
    HIPCHK(hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking));
    HIPCHK(hipEventCreateWithFlags(&s.ready, hipEventDisableTiming));
    ASWCHK(dev_alloc(&s.left, S * 4));
    ASWCHK(dev_alloc(&s.right, S * 4));
    ASWCHK(dev_alloc(&s.lut, asw_lut_bytes(p)));
    if (p->color_space == ASW_COLOR_LAB) {
        ASWCHK(dev_alloc(&s.lab_l, asw_lab_bytes(p)));
        ASWCHK(dev_alloc(&s.lab_r, asw_lab_bytes(p)));
    }
    // the raw-cost volume as uint16 (half the bytes written by asw_Aggr and read by the
    // first V pass; bit-identical) where built; ASW_FLAG_RAW_F32 keeps the float volume
    s.raw16 = !(p->flags & ASW_FLAG_RAW_F32) && asw_raw16_supported(p);
    ASWCHK(dev_alloc(&s.wvl, asw_support_bytes(p)));
    ASWCHK(dev_alloc(&s.wvr, asw_support_bytes(p)));
    ASWCHK(dev_alloc(&s.whl, asw_support_bytes(p)));
    ASWCHK(dev_alloc(&s.whr, asw_support_bytes(p)));
    ASWCHK(dev_alloc(&s.c0, asw_cost_bytes(p)));
    ASWCHK(dev_alloc(&s.c1, asw_cost_bytes(p)));
    if (p->iters >= 2 && asw_disp_pitch(p) != 32) {
        // the den of a direction is written by its first pass and read by the r-1 others
        // (a 32-plane shard's passes recompute it: at C4 / 8 k_vpass32 den-none 0.24 against
        // den-read 0.28 ms, k_hpass32 0.30-0.33 against 0.36, profiles/r04/h32_variants_r11d.log;
        // in the shard frame 4.99 against 5.04 ms, profiles/r04/shard_den_h_ab_r11e.log)
        ASWCHK(dev_alloc(&s.den_v, asw_cost_bytes(p)));
        ASWCHK(dev_alloc(&s.den_h, asw_cost_bytes(p)));
    }
    if (sharded) {
        ASWCHK(dev_alloc(&s.key, S * 8));
        ASWCHK(dev_alloc(&s.key_g, S * 8));
        ASWCHK(dev_alloc(&s.tkey, S * 8));
        ASWCHK(dev_alloc(&s.tkey_g, S * 8));
        ASWCHK(dev_alloc(&s.m1, S * 4));
        ASWCHK(dev_alloc(&s.m2, S * 4));
        ASWCHK(dev_alloc(&s.t1, S * 4));
        ASWCHK(dev_alloc(&s.t2, S * 4));
        ASWCHK(dev_alloc(&s.m2_g, S * 4));
        ASWCHK(dev_alloc(&s.t2_g, S * 4));
    }
    return ASW_OK;
}

// contiguous balanced split of [0, D) (stereo_matchin_amd/distributed.py shard_range)
void shard_range(int D, int i, int n, int *b, int *e) {
    const int base = D / n, rem = D % n;
    *b = i * base + (i < rem ? i : rem);
    *e = *b + base + (i < rem ? 1 : 0);
}

int destroy_ctx(asw_ctx *c) {
    if (!c) return ASW_OK;
    for (int i = 0; i < kMaxShards; ++i) free_shard(c->sh[i]);
    (void)hipSetDevice(c->sh[0].device);
    void *bufs[] = {c->red_tmp, c->d_ref, c->d_tar, c->conf_ref, c->conf_tar, c->code_ref, c->code_tar, c->lr,
                    c->lr_red, c->disp, c->disp16, c->lr16, c->rws, c->est, c->post_red, c->final_rgba,
                    c->nrws, c->n_est, c->n_dt, c->n_dr, c->n_post16, c->n_final16,
                    c->sgm_ws, c->sp_disp, c->sp_lr, c->sp_fill, c->cr_med_l, c->cr_med_r, c->cr_init, c->cr_final,
                    c->cr_arms_l, c->cr_arms_r, c->cr_d0, c->cr_code0, c->cr_code1,
                    c->spk_valid, c->spk_keep, c->spk_ws, c->spk_size, c->spk_f16, c->spk_lr, c->spk_fill};
    for (void *b : bufs)
        if (b) (void)hipFree(b);
    for (hipEvent_t e : c->ev)
        if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : c->cr_ev)
        if (e) (void)hipEventDestroy(e);
    if (c->red_done) (void)hipEventDestroy(c->red_done);
    if (c->gx_main) (void)hipGraphExecDestroy(c->gx_main);
    if (c->gx_ref) (void)hipGraphExecDestroy(c->gx_ref);
    if (c->g_main) (void)hipGraphDestroy(c->g_main);
    if (c->g_ref) (void)hipGraphDestroy(c->g_ref);
    delete c;
    return ASW_OK;
}

// Shared constructor.  This process drives shards [shard0, shard0 + n) of `total`
// (devs[i] = the device of its i-th shard); comm selects the exchange.
int create_ctx(const asw_params *p, const int *devs, int n, int shard0, int total, CommMode comm,
               const ncclUniqueId *id, asw_ctx **out) {
    if (!out) return ASW_E_INVALID;
    *out = nullptr;
    ASWCHK(asw_params_check(p));
    if (p->d_begin != 0 || (p->d_end >= 0 && p->d_end != p->ndisp)) return ASW_E_INVALID;  // contexts shard themselves
    if (n < 1 || n > kMaxShards || total < n || total > p->ndisp) return ASW_E_INVALID;
    // a shape the pass kernels cannot address fails here, before any device call or
    // allocation (tens of GB for an 8K frame), not at the first pass
    for (int i = 0; i < n; ++i) {
        asw_params sp = *p;
        sp.d_end = p->ndisp;
        shard_range(p->ndisp, shard0 + i, total, &sp.d_begin, &sp.d_end);
        ASWCHK(asw::pass_shape_check(&sp));
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess) ndev = 0;
    for (int i = 0; i < n; ++i)
        if (devs[i] < 0 || devs[i] >= ndev) return ASW_E_INVALID;
    asw_ctx *c = new (std::nothrow) asw_ctx;
    if (!c) return ASW_E_NOMEM;
    c->p = *p;
    c->p.d_end = p->ndisp;
    c->n = n;
    c->rank = shard0;
    c->nranks = total;
    c->comm = comm;
    const size_t S = frame_pixels(p);
    int s = ASW_OK;
    auto chain = [&](int r) {
        if (s == ASW_OK) s = r;
    };
    for (int i = 0; i < n && s == ASW_OK; ++i) {
        Shard &sh = c->sh[i];
        sh.device = devs[i];
        sh.p = c->p;
        shard_range(p->ndisp, shard0 + i, total, &sh.p.d_begin, &sh.p.d_end);
        chain(alloc_shard(sh, comm != COMM_NONE));
    }
    if (s == ASW_OK && comm == COMM_LOCAL) {
        chain(hipSetDevice(devs[0]) == hipSuccess ? ASW_OK : ASW_E_HIP);
        chain(hipEventCreateWithFlags(&c->red_done, hipEventDisableTiming) == hipSuccess ? ASW_OK : ASW_E_HIP);
        bool peers = false;
        for (int i = 1; i < n; ++i) peers = peers || devs[i] != devs[0];
        if (peers) chain(dev_alloc(&c->red_tmp, (size_t)(n - 1) * S * 8));
    }
    if (s == ASW_OK && comm == COMM_RCCL) {
        ncclComm_t comms[kMaxShards] = {};
        ncclResult_t r = ncclSuccess;
        if (id) {  // one process per GPU
            const hipError_t e = hipSetDevice(devs[0]);
            if (e != hipSuccess) s = hip_fail(e);  // a device-selection failure, not a communicator one
            else r = ncclCommInitRank(&comms[0], total, *id, shard0);
        } else {
            r = ncclCommInitAll(comms, n, devs);
        }
        if (s == ASW_OK && r != ncclSuccess) s = ASW_E_COMM;
        for (int i = 0; i < n; ++i) c->sh[i].comm = comms[i];
    }
    if (s == ASW_OK) {
        chain(hipSetDevice(devs[0]) == hipSuccess ? ASW_OK : ASW_E_HIP);
        chain(dev_alloc(&c->d_ref, S * 4));
        chain(dev_alloc(&c->d_tar, S * 4));
        chain(dev_alloc(&c->conf_ref, S * 4));
        chain(dev_alloc(&c->conf_tar, S * 4));
        chain(dev_alloc(&c->code_ref, S));
        chain(dev_alloc(&c->code_tar, S));
        chain(dev_alloc(&c->lr, S * 4));
        chain(dev_alloc(&c->lr_red, S * 4));
        chain(dev_alloc(&c->disp, S * 4));
        chain(dev_alloc(&c->disp16, S * 2));
        chain(dev_alloc(&c->lr16, S * 2));
        // h2d, raw, support, 2r+1 pass marks, exchange, wta, consistency, refine, d2h, sub-pixel start
        c->ev.assign(2 * (size_t)p->iters + 11, nullptr);
        for (hipEvent_t &e : c->ev)
            if (s == ASW_OK) chain(hipEventCreate(&e) == hipSuccess ? ASW_OK : ASW_E_HIP);
    }
    if (s != ASW_OK) {
        destroy_ctx(c);
        return s;
    }
    *out = c;
    return ASW_OK;
}

// whether the raw cost SGM reads is built: asw_raw_cost16's / asw_census_cost16's own rule
bool cost16_exists(const asw_params *p, const asw_census_params *cen) {
    return (cen ? asw::census_cost16_check(p, cen) : asw::raw_cost16_check(p)) == ASW_OK;
}

// asw_set_sgm on (one shard): the raw cost in its uint16 form into c1, asw_sgm's sums into c0.
// No supports and no passes: taps and iters are not read.  The caller's next event (the WTA's
// start) is the end of asw_timings.aggregation_total.
int sgm_aggregate(asw_ctx *c, const uint8_t *left_rgba, const uint8_t *right_rgba, int e_raw, int e_pass0,
                  bool timed) {
    Shard &s = c->sh[0];
    const asw_params *p = &s.p;
    const size_t S = frame_pixels(p);
    hipStream_t st = s.stream;
    uint16_t *raw = reinterpret_cast<uint16_t *>(s.c1);
    HIPCHK(hipSetDevice(s.device));
    if (left_rgba) {
        HIPCHK(hipMemcpyAsync(s.left, left_rgba, S * 4, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(s.right, right_rgba, S * 4, hipMemcpyHostToDevice, st));
    }
    if (timed) HIPCHK(hipEventRecord(c->ev[e_raw], st));
    if (c->census_on) {
        ASWCHK(asw_census(p, &c->cen, s.left, s.cen_l, st));
        ASWCHK(asw_census(p, &c->cen, s.right, s.cen_r, st));
        ASWCHK(asw_census_cost16(p, &c->cen, s.left, s.right, s.cen_l, s.cen_r, raw, st));
    } else {
        ASWCHK(asw_raw_cost16(p, s.left, s.right, raw, st));
    }
    if (timed) HIPCHK(hipEventRecord(c->ev[e_raw + 1], st));
    if (timed) HIPCHK(hipEventRecord(c->ev[e_pass0], st));
    return asw_sgm(p, &c->sgm, raw, s.c0, c->sgm_ws, st);
}

// raw cost + supports + 2r passes of one shard, asynchronous on its stream.
// Pass-boundary events (timing) are recorded only for shard 0.
int shard_aggregate(asw_ctx *c, int i, const uint8_t *left_rgba, const uint8_t *right_rgba, int e_raw, int e_pass0,
                    bool timing = true) {
    Shard &s = c->sh[i];
    const asw_params *p = &s.p;
    const size_t S = frame_pixels(p);
    hipStream_t st = s.stream;
    const bool timed = i == 0 && timing;
    HIPCHK(hipSetDevice(s.device));
    if (left_rgba) {  // NULL: the images are already on the device (graph replay)
        HIPCHK(hipMemcpyAsync(s.left, left_rgba, S * 4, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(s.right, right_rgba, S * 4, hipMemcpyHostToDevice, st));
    }
    if (timed) HIPCHK(hipEventRecord(c->ev[e_raw], st));
    // the raw cost (uint16 where the first pass reads it so); census on: the transform of
    // both images (d-independent, repeated by every shard) and the census cost in its place
    const bool raw16 = c->census_on ? s.census16 : s.raw16;
    if (c->census_on) {
        ASWCHK(asw_census(p, &c->cen, s.left, s.cen_l, st));
        ASWCHK(asw_census(p, &c->cen, s.right, s.cen_r, st));
        if (raw16)
            ASWCHK(asw_census_cost16(p, &c->cen, s.left, s.right, s.cen_l, s.cen_r, reinterpret_cast<uint16_t *>(s.c0),
                                     st));
        else ASWCHK(asw_census_cost(p, &c->cen, s.left, s.right, s.cen_l, s.cen_r, s.c0, st));
    } else if (raw16) {
        ASWCHK(asw_raw_cost16(p, s.left, s.right, reinterpret_cast<uint16_t *>(s.c0), st));
    } else {
        ASWCHK(asw_raw_cost(p, s.left, s.right, s.c0, st));
    }
    if (timed) HIPCHK(hipEventRecord(c->ev[e_raw + 1], st));
    if (p->color_space == ASW_COLOR_LAB) {
        ASWCHK(asw_lab(p, s.left, s.lab_l, st));
        ASWCHK(asw_lab(p, s.right, s.lab_r, st));
        ASWCHK(asw_support_lab(p, ASW_DIR_V, s.lab_l, s.wvl, st));
        ASWCHK(asw_support_lab(p, ASW_DIR_H, s.lab_l, s.whl, st));
        ASWCHK(asw_support_lab(p, ASW_DIR_V, s.lab_r, s.wvr, st));
        ASWCHK(asw_support_lab(p, ASW_DIR_H, s.lab_r, s.whr, st));
    } else {
        ASWCHK(asw_support_lut(p, s.lut, st));
        ASWCHK(asw_support_all(p, s.left, s.right, s.lut, s.wvl, s.whl, s.wvr, s.whr, st));
    }
    if (timed) HIPCHK(hipEventRecord(c->ev[e_pass0], st));
    for (int it = 0; it < p->iters; ++it) {
        const int dmv = !s.den_v ? ASW_DEN_NONE : (it == 0 ? ASW_DEN_WRITE : ASW_DEN_READ);
        const int dm = !s.den_h ? ASW_DEN_NONE : (it == 0 ? ASW_DEN_WRITE : ASW_DEN_READ);
        if (it == 0 && raw16)
            ASWCHK(asw_aggregate_pass_den16(p, s.wvl, s.wvr, reinterpret_cast<const uint16_t *>(s.c0), s.c1, s.den_v,
                                            dmv, st));
        else ASWCHK(asw_aggregate_pass_den(p, ASW_DIR_V, s.wvl, s.wvr, s.c0, s.c1, s.den_v, dmv, st));
        if (timed) HIPCHK(hipEventRecord(c->ev[e_pass0 + 2 * it + 1], st));
        ASWCHK(asw_aggregate_pass_den(p, ASW_DIR_H, s.whl, s.whr, s.c1, s.c0, s.den_h, dm, st));
        if (timed) HIPCHK(hipEventRecord(c->ev[e_pass0 + 2 * it + 2], st));
    }
    return ASW_OK;
}

// The WTA of a one-shard frame
int single_wta(asw_ctx *c) {
    Shard &s0 = c->sh[0];
    return asw_wta(&s0.p, s0.c0, c->d_ref, c->conf_ref, c->d_tar, c->conf_tar, c->code_ref, c->code_tar, s0.stream);
}

// The d-sharded WTA (asw_wta_local protocol, include/asw.h): maps on shard 0.
int sharded_wta(asw_ctx *c) {
    const size_t S = frame_pixels(&c->p);
    for (int i = 0; i < c->n; ++i) {
        Shard &s = c->sh[i];
        HIPCHK(hipSetDevice(s.device));
        ASWCHK(asw_wta_local(&s.p, s.c0, s.key, s.m1, s.m2, s.stream));
        HIPCHK(hipMemcpyAsync(s.key_g, s.key, S * 8, hipMemcpyDeviceToDevice, s.stream));
    }
    ASWCHK(allreduce_min<int64_t>(c, b_key_g, ncclInt64));
    for (int i = 0; i < c->n; ++i) {
        Shard &s = c->sh[i];
        HIPCHK(hipSetDevice(s.device));
        ASWCHK(asw_wta_second(&s.p, s.key_g, s.key, s.m1, s.m2, s.m2_g, s.stream));
    }
    ASWCHK(allreduce_min<float>(c, b_m2_g, ncclFloat32));
    for (int i = 0; i < c->n; ++i) {
        Shard &s = c->sh[i];
        HIPCHK(hipSetDevice(s.device));
        ASWCHK(asw_wta_target_local(&s.p, s.c0, s.key_g, s.tkey, s.t1, s.t2, s.stream));
        HIPCHK(hipMemcpyAsync(s.tkey_g, s.tkey, S * 8, hipMemcpyDeviceToDevice, s.stream));
    }
    ASWCHK(allreduce_min<int64_t>(c, b_tkey_g, ncclInt64));
    for (int i = 0; i < c->n; ++i) {
        Shard &s = c->sh[i];
        HIPCHK(hipSetDevice(s.device));
        ASWCHK(asw_wta_second(&s.p, s.tkey_g, s.tkey, s.t1, s.t2, s.t2_g, s.stream));
    }
    ASWCHK(allreduce_min<float>(c, b_t2_g, ncclFloat32));
    Shard &s0 = c->sh[0];
    HIPCHK(hipSetDevice(s0.device));
    return asw_wta_finalize(&s0.p, s0.key_g, s0.m2_g, s0.tkey_g, s0.t2_g, c->d_ref, c->conf_ref, c->d_tar,
                            c->conf_tar, c->code_ref, c->code_tar, s0.stream);
}

// asw_WTA_REF of a d-sharded frame from the two views' H estimates hl / hr (on shard 0):
// the scan runs on every shard and is exchanged like the WTA: MIN all-reduces of the left
// key, the target key and the target second minimum (asw_wta_ref_local protocol).  Maps on
// shard 0; kl / kt (the 8-bit codes) may be NULL.
int sharded_wta_ref(asw_ctx *c, const float *hl, const float *hr, int32_t *dr, int32_t *dt, uint8_t *kl,
                    uint8_t *kt) {
    const size_t S = frame_pixels(&c->p);
    Shard &s0 = c->sh[0];
    hipStream_t st = s0.stream;
    for (int i = 1; i < c->n; ++i) {  // the estimates to the other shards' devices
        Shard &s = c->sh[i];
        HIPCHK(hipMemcpyPeerAsync(s.ref_l, s.device, hl, s0.device, 2 * S * 4, st));
        HIPCHK(hipMemcpyPeerAsync(s.ref_r, s.device, hr, s0.device, 2 * S * 4, st));
    }
    if (c->n > 1) {
        HIPCHK(hipEventRecord(c->red_done, st));
        for (int i = 1; i < c->n; ++i) {
            HIPCHK(hipSetDevice(c->sh[i].device));
            HIPCHK(hipStreamWaitEvent(c->sh[i].stream, c->red_done, 0));
        }
    }
    for (int i = 0; i < c->n; ++i) {
        Shard &s = c->sh[i];
        HIPCHK(hipSetDevice(s.device));
        ASWCHK(asw_wta_ref_local(&s.p, s.c0, i ? s.ref_l : hl, s.key, s.m1, s.m2, s.stream));
        HIPCHK(hipMemcpyAsync(s.key_g, s.key, S * 8, hipMemcpyDeviceToDevice, s.stream));
    }
    ASWCHK(allreduce_min<int64_t>(c, b_key_g, ncclInt64));
    for (int i = 0; i < c->n; ++i) {
        Shard &s = c->sh[i];
        HIPCHK(hipSetDevice(s.device));
        ASWCHK(asw_wta_ref_target_local(&s.p, s.c0, i ? s.ref_r : hr, s.key_g, s.tkey, s.t1, s.t2, s.stream));
        HIPCHK(hipMemcpyAsync(s.tkey_g, s.tkey, S * 8, hipMemcpyDeviceToDevice, s.stream));
    }
    ASWCHK(allreduce_min<int64_t>(c, b_tkey_g, ncclInt64));
    for (int i = 0; i < c->n; ++i) {
        Shard &s = c->sh[i];
        HIPCHK(hipSetDevice(s.device));
        ASWCHK(asw_wta_second(&s.p, s.tkey_g, s.tkey, s.t1, s.t2, s.t2_g, s.stream));
    }
    ASWCHK(allreduce_min<float>(c, b_t2_g, ncclFloat32));
    HIPCHK(hipSetDevice(s0.device));
    return asw_wta_ref_finalize(&s0.p, s0.key_g, s0.tkey_g, s0.t2_g, dr, dt, c->conf_ref, kl, kt, st);
}

// The refinement loop (main.cpp:540-617) + median on a d-sharded frame.  The
// per-pixel stages (asw_ref_v / asw_ref_h, consistency, median) run on shard 0 (in
// one process per GPU: on every rank, identically); the volume scan (asw_WTA_REF)
// runs on every shard and is exchanged like the WTA: MIN all-reduces of the left
// key, the target key and the target second minimum (asw_wta_ref_local protocol).
int refine_sharded(asw_ctx *c) {
    const asw_params *p = &c->p;
    const asw_refine_params *rp = &c->rp;
    const size_t S = frame_pixels(p);
    Shard &s0 = c->sh[0];
    hipStream_t st = s0.stream;
    char *ws = static_cast<char *>(c->rws);
    float *lut = reinterpret_cast<float *>(ws);
    ws += (asw_refine_lut_bytes(rp) + 255) / 256 * 256;
    float *vl = reinterpret_cast<float *>(ws), *vr = vl + 2 * S, *hl = vr + 2 * S, *hr = hl + 2 * S;
    int32_t *dr = reinterpret_cast<int32_t *>(hr + 2 * S), *dt = dr + S;
    uint8_t *kl = reinterpret_cast<uint8_t *>(dt + S);
    HIPCHK(hipSetDevice(s0.device));
    ASWCHK(asw_refine_lut(p, rp, lut, st));
    for (int it = 0; it < rp->iters; ++it) {
        HIPCHK(hipSetDevice(s0.device));
        ASWCHK(asw_ref_v(p, rp, s0.left, c->est, 4, c->conf_ref, lut, vl, st));
        ASWCHK(asw_ref_v(p, rp, s0.right, c->code_tar, 1, c->conf_tar, lut, vr, st));
        ASWCHK(asw_ref_h(p, rp, s0.left, c->conf_ref, vl, lut, hl, st));
        ASWCHK(asw_ref_h(p, rp, s0.right, c->conf_tar, vr, lut, hr, st));
        ASWCHK(sharded_wta_ref(c, hl, hr, dr, dt, kl, c->code_tar));
        ASWCHK(asw_consistency(p, dr, dt, kl, c->code_tar, c->conf_ref, c->conf_tar, c->est, c->post_red, st));
    }
    HIPCHK(hipSetDevice(s0.device));
    return asw_median3(p, c->est, 4, c->final_rgba, st);
}

// The device work of a one-shard frame from uploaded images to the consistency
// images (no events): what asw_set_graph captures into one HIP graph.
int main_work_untimed(asw_ctx *c) {
    const asw_params *p = &c->p;
    const size_t S = frame_pixels(p);
    Shard &s0 = c->sh[0];
    hipStream_t st = s0.stream;
    if (c->sgm_on) ASWCHK(sgm_aggregate(c, nullptr, nullptr, 1, 3, false));
    else ASWCHK(shard_aggregate(c, 0, nullptr, nullptr, 1, 3, false));
    ASWCHK(single_wta(c));
    hipLaunchKernelGGL(k_codes_to_rgba, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, st, (long long)S,
                       c->code_ref, reinterpret_cast<uchar4 *>(c->disp));
    HIPCHK(hipGetLastError());
    if (p->lr_check)
        ASWCHK(asw_consistency(p, c->d_ref, c->d_tar, c->code_ref, c->code_tar, c->conf_ref, c->conf_tar, c->lr,
                               c->lr_red, st));
    hipLaunchKernelGGL(k_disp16, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, st, (long long)S, p->ndisp,
                       p->lr_mode, p->lr_check, c->d_ref, c->d_tar, c->code_ref, c->code_tar, c->disp16, c->lr16);
    HIPCHK(hipGetLastError());
    return ASW_OK;
}

int refine_work(asw_ctx *c) {
    const size_t S = frame_pixels(&c->p);
    Shard &s0 = c->sh[0];
    hipStream_t st = s0.stream;
    HIPCHK(hipMemcpyAsync(c->est, c->lr, S * 4, hipMemcpyDeviceToDevice, st));
    if (c->comm == COMM_NONE)
        return asw_refine(&s0.p, &c->rp, s0.left, s0.right, s0.c0, c->est, c->code_tar, c->conf_ref, c->conf_tar,
                          c->rws, c->post_red, c->final_rgba, nullptr, nullptr, st);
    return refine_sharded(c);
}

// The native refinement loop (asw_set_refine_native; include/asw.h §native refinement) of a
// frame: est_left from the WTA's maps by the native rule (the confidences stay as
// asw_consistency left them), the right estimate a copy of d_tar; then asw_refine_native on
// a one-shard frame, and on a d-sharded one its stages on shard 0 around sharded_wta_ref.
int refine_native_work(asw_ctx *c) {
    const asw_params *p = &c->p;
    const asw_refine_params *rp = &c->nrp;
    const size_t S = frame_pixels(p);
    Shard &s0 = c->sh[0];
    hipStream_t st = s0.stream;
    HIPCHK(hipMemcpyAsync(c->n_dt, c->d_tar, S * 4, hipMemcpyDeviceToDevice, st));
    ASWCHK(asw_consistency_native(p, c->d_ref, c->d_tar, nullptr, nullptr, c->n_est, nullptr, st));
    if (c->comm == COMM_NONE)
        return asw_refine_native(&s0.p, rp, s0.left, s0.right, s0.c0, c->n_est, c->n_dt, c->conf_ref, c->conf_tar,
                                 c->nrws, c->n_post16, c->n_final16, c->n_dr, st);
    char *ws = static_cast<char *>(c->nrws);
    float *lut = reinterpret_cast<float *>(ws);
    ws += (asw_refine_lut_bytes(rp) + 255) / 256 * 256;
    float *vl = reinterpret_cast<float *>(ws), *vr = vl + 2 * S, *hl = vr + 2 * S, *hr = hl + 2 * S;
    ASWCHK(asw_refine_native_lut(p, rp, lut, st));
    for (int it = 0; it < rp->iters; ++it) {
        HIPCHK(hipSetDevice(s0.device));
        ASWCHK(asw_ref_v_native(p, rp, s0.left, c->n_est, c->conf_ref, lut, vl, st));
        ASWCHK(asw_ref_v_native(p, rp, s0.right, c->n_dt, c->conf_tar, lut, vr, st));
        ASWCHK(asw_ref_h(p, rp, s0.left, c->conf_ref, vl, lut, hl, st));
        ASWCHK(asw_ref_h(p, rp, s0.right, c->conf_tar, vr, lut, hr, st));
        ASWCHK(sharded_wta_ref(c, hl, hr, c->n_dr, c->n_dt, nullptr, nullptr));
        ASWCHK(asw_consistency_native(p, c->n_dr, c->n_dt, c->conf_ref, c->conf_tar, c->n_est, c->n_post16, st));
    }
    HIPCHK(hipSetDevice(s0.device));
    return asw_median3_u16(p, c->n_est, c->n_final16, st);
}

// The sub-pixel maps (asw_set_subpixel) from the frame's WTA results, on shard 0's
// stream after the consistency stage and before the refinement loop touches anything.
// One shard: asw_subpixel on the volume.  Sharded: every shard offers the neighbour
// planes it owns of the global winner (key_g, still the first all-reduce's result), one
// MIN all-reduce of the [3][S] array, finalize on shard 0 from the same three floats.
int subpixel_work(asw_ctx *c) {
    const asw_params *p = &c->p;
    Shard &s0 = c->sh[0];
    hipStream_t st = s0.stream;
    if (c->comm == COMM_NONE) {
        ASWCHK(asw_subpixel(&s0.p, s0.c0, c->d_ref, c->sp_disp, st));
    } else {
        for (int i = 0; i < c->n; ++i) {
            Shard &s = c->sh[i];
            HIPCHK(hipSetDevice(s.device));
            ASWCHK(asw_subpixel_local(&s.p, s.c0, s.key_g, s.nb, s.stream));
        }
        ASWCHK(allreduce_min<float>(c, b_nb, ncclFloat32, 3));
        HIPCHK(hipSetDevice(s0.device));
        ASWCHK(asw_subpixel_finalize(p, s0.key_g, s0.nb, c->sp_disp, st));
    }
    if (c->sp_lr)
        ASWCHK(asw_disp_mask(p, c->sp_disp, c->d_ref, c->d_tar, c->code_ref, c->code_tar, c->sp_lr, st));
    if (c->sp_fill) ASWCHK(asw_disp_fill(p, c->sp_lr, c->sp_fill, st));
    return ASW_OK;
}

// whether the registered speckle outputs need the sub-pixel disp map (subpixel_work)
bool speckle_wants_disp(const asw_ctx *c) { return c->spk_on && (c->spo.disp_lr || c->spo.disp_filled); }

// The speckle filter (asw_set_speckle) on the frame's d_ref, on shard 0's stream after the
// consistency stage and the sub-pixel work: the LR rule as the validity map (lr_check), the
// components, then the masked maps that were asked for.
int speckle_work(asw_ctx *c) {
    const asw_params *p = &c->p;
    hipStream_t st = c->sh[0].stream;
    const uint8_t *valid = nullptr;
    if (p->lr_check) {
        ASWCHK(asw_lr_valid(p, c->d_ref, c->d_tar, c->code_ref, c->code_tar, c->spk_valid, st));
        valid = c->spk_valid;
    }
    ASWCHK(asw_speckle(p, &c->spk, c->d_ref, valid, c->spk_ws, nullptr, c->spk_size, c->spk_keep, st));
    if (c->spo.filtered16) ASWCHK(asw_speckle_mask16(p, c->d_ref, c->spk_keep, c->spk_f16, st));
    if (speckle_wants_disp(c)) ASWCHK(asw_speckle_mask_f32(p, c->sp_disp, c->spk_keep, c->spk_lr, st));
    if (c->spo.disp_filled) ASWCHK(asw_disp_fill(p, c->spk_lr, c->spk_fill, st));
    return ASW_OK;
}

// The cross-based matcher of a frame (asw_set_cross; main.cpp:272-354), on shard 0's
// stream ahead of the ASW stages: it uploads the pair itself and borrows the shard's two
// cost volumes, which the ASW stages overwrite afterwards.  The registered host arrays
// receive pair `pair` of a batch.  Never captured into a graph.
constexpr int kCrossEvents = 12;  // start + one per column of asw_cross_timings but the total

int cross_work(asw_ctx *c, const uint8_t *left_rgba, const uint8_t *right_rgba, size_t pair) {
    const asw_params *p = &c->p;
    const size_t S = frame_pixels(p);
    Shard &s0 = c->sh[0];
    hipStream_t st = s0.stream;
    std::vector<hipEvent_t> &ev = c->cr_ev;
    const asw_cross_outputs &o = c->cro;
    HIPCHK(hipMemcpyAsync(s0.left, left_rgba, S * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(s0.right, right_rgba, S * 4, hipMemcpyHostToDevice, st));
    int e = 0;
    HIPCHK(hipEventRecord(ev[e++], st));
    ASWCHK(asw_median3_rgba(p, s0.left, c->cr_med_l, st));
    HIPCHK(hipEventRecord(ev[e++], st));
    ASWCHK(asw_median3_rgba(p, s0.right, c->cr_med_r, st));
    HIPCHK(hipEventRecord(ev[e++], st));
    ASWCHK(asw_cross_arms(p, &c->cp, c->cr_med_l, c->cr_arms_l, st));
    HIPCHK(hipEventRecord(ev[e++], st));
    ASWCHK(asw_cross_arms(p, &c->cp, c->cr_med_r, c->cr_arms_r, st));
    HIPCHK(hipEventRecord(ev[e++], st));
    ASWCHK(asw_cross_cost(p, c->cr_med_l, c->cr_med_r, s0.c0, st));
    HIPCHK(hipEventRecord(ev[e++], st));
    ASWCHK(asw_cross_integral(p, ASW_DIR_H, s0.c0, st));
    HIPCHK(hipEventRecord(ev[e++], st));
    ASWCHK(asw_cross_oii(p, ASW_DIR_H, c->cr_arms_l, c->cr_arms_r, s0.c0, s0.c1, st));
    HIPCHK(hipEventRecord(ev[e++], st));
    ASWCHK(asw_cross_integral(p, ASW_DIR_V, s0.c1, st));
    HIPCHK(hipEventRecord(ev[e++], st));
    ASWCHK(asw_cross_oii(p, ASW_DIR_V, c->cr_arms_l, c->cr_arms_r, s0.c1, s0.c0, st));
    HIPCHK(hipEventRecord(ev[e++], st));
    ASWCHK(asw_cross_init(p, s0.c0, c->cr_d0, c->cr_code0, st));
    HIPCHK(hipEventRecord(ev[e++], st));
    ASWCHK(asw_cross_vote(p, c->cr_code0, c->cr_arms_l, nullptr, c->cr_code1, st));
    HIPCHK(hipEventRecord(ev[e++], st));
    if (o.initial_rgba) {
        hipLaunchKernelGGL(k_codes_to_rgba, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, st, (long long)S,
                           c->cr_code0, reinterpret_cast<uchar4 *>(c->cr_init));
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(o.initial_rgba + pair * S * 4, c->cr_init, S * 4, hipMemcpyDeviceToHost, st));
    }
    if (o.final_rgba) {  // main.cpp:352-354: the Median of the voted code image
        ASWCHK(asw_median3(p, c->cr_code1, 1, c->cr_final, st));
        HIPCHK(hipMemcpyAsync(o.final_rgba + pair * S * 4, c->cr_final, S * 4, hipMemcpyDeviceToHost, st));
    }
    if (o.median_left_rgba)
        HIPCHK(hipMemcpyAsync(o.median_left_rgba + pair * S * 4, c->cr_med_l, S * 4, hipMemcpyDeviceToHost, st));
    if (o.d_initial) HIPCHK(hipMemcpyAsync(o.d_initial + pair * S, c->cr_d0, S * 4, hipMemcpyDeviceToHost, st));
    if (o.timings) {
        HIPCHK(hipStreamSynchronize(st));
        asw_cross_timings *t = o.timings + pair;
        t->median[0] = ms_between(ev[0], ev[1]);
        t->median[1] = ms_between(ev[1], ev[2]);
        t->cross[0] = ms_between(ev[2], ev[3]);
        t->cross[1] = ms_between(ev[3], ev[4]);
        t->aggregation = ms_between(ev[4], ev[5]);
        t->integral_h = ms_between(ev[5], ev[6]);
        t->oii_h = ms_between(ev[6], ev[7]);
        t->integral_v = ms_between(ev[7], ev[8]);
        t->oii_v = ms_between(ev[8], ev[9]);
        t->init = ms_between(ev[9], ev[10]);
        t->vote = ms_between(ev[10], ev[11]);
        t->total = ms_between(ev[0], ev[11]);
    }
    return ASW_OK;
}

// capture fn's work on stream st into *g / *gx (once), then launch it
template <class F>
int graph_run(hipStream_t st, hipGraph_t *g, hipGraphExec_t *gx, F &&fn) {
    if (!*gx) {
        HIPCHK(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
        const int s = fn();
        hipGraph_t cap = nullptr;
        const hipError_t e = hipStreamEndCapture(st, &cap);
        if (s != ASW_OK || e != hipSuccess) {
            if (cap) (void)hipGraphDestroy(cap);
            return s != ASW_OK ? s : hip_fail(e);
        }
        const hipError_t ei = hipGraphInstantiate(gx, cap, nullptr, nullptr, 0);
        if (ei != hipSuccess) {  // nothing kept: the next call captures afresh
            (void)hipGraphDestroy(cap);
            *gx = nullptr;
            return hip_fail(ei);
        }
        *g = cap;
    }
    HIPCHK(hipGraphLaunch(*gx, st));
    return ASW_OK;
}

int match_one(asw_ctx *c, const uint8_t *left_rgba, const uint8_t *right_rgba, asw_outputs *o, asw_timings *t,
              size_t pair = 0) {
    const asw_params *p = &c->p;
    const size_t S = frame_pixels(p);
    const int r = p->iters;
    Shard &s0 = c->sh[0];
    hipStream_t st = s0.stream;
    std::vector<hipEvent_t> &ev = c->ev;
    // event slots: 0 h2d start, 1 h2d end = raw start, 2 raw end, 3.. 3+2r pass marks,
    // then exchange end, wta end, consistency end (= end of `total`), pre-refinement d2h end,
    // refine end, d2h end; sub-pixel maps or speckle filter on: their start (they end at
    // "consistency end")
    const int e_pass0 = 3, e_x = e_pass0 + 2 * r + 1, e_wta = e_x + 1, e_cons = e_x + 2, e_pre = e_x + 3,
              e_ref = e_x + 4, e_d2h = e_x + 5, e_sub = e_x + 6;
    const bool graphed = c->graph && c->comm == COMM_NONE;
    HIPCHK(hipSetDevice(s0.device));
    if (c->cross_on) ASWCHK(cross_work(c, left_rgba, right_rgba, pair));  // the reference's order: before ASW
    HIPCHK(hipEventRecord(ev[0], st));
    if (graphed) {
        HIPCHK(hipMemcpyAsync(s0.left, left_rgba, S * 4, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(s0.right, right_rgba, S * 4, hipMemcpyHostToDevice, st));
        HIPCHK(hipEventRecord(ev[1], st));
        ASWCHK(graph_run(st, &c->g_main, &c->gx_main, [&] { return main_work_untimed(c); }));
    } else {
        if (c->sgm_on) ASWCHK(sgm_aggregate(c, left_rgba, right_rgba, 1, e_pass0, true));
        else
            for (int i = 0; i < c->n; ++i) ASWCHK(shard_aggregate(c, i, left_rgba, right_rgba, 1, e_pass0));
        if (c->comm == COMM_NONE) {
            HIPCHK(hipSetDevice(s0.device));
            HIPCHK(hipEventRecord(ev[e_x], st));
            ASWCHK(single_wta(c));
        } else {
            ASWCHK(sharded_wta(c));
            HIPCHK(hipSetDevice(s0.device));
            HIPCHK(hipEventRecord(ev[e_x], st));
        }
        HIPCHK(hipEventRecord(ev[e_wta], st));
        hipLaunchKernelGGL(k_codes_to_rgba, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, st, (long long)S,
                           c->code_ref, reinterpret_cast<uchar4 *>(c->disp));
        HIPCHK(hipGetLastError());
        if (p->lr_check)
            ASWCHK(asw_consistency(p, c->d_ref, c->d_tar, c->code_ref, c->code_tar, c->conf_ref, c->conf_tar, c->lr,
                                   c->lr_red, st));
        const bool want16 = o && (o->disp16 || o->lr16);
        if (want16) {
            hipLaunchKernelGGL(k_disp16, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, st, (long long)S,
                               p->ndisp, p->lr_mode, p->lr_check, c->d_ref, c->d_tar, c->code_ref, c->code_tar,
                               c->disp16, c->lr16);
            HIPCHK(hipGetLastError());
        }
    }
    // the sub-pixel maps and the speckle filter: never captured, launched on the stream after
    // the graph replay; the disp map is computed once for both
    const bool sub_work = c->sub_on || speckle_wants_disp(c), post_work = sub_work || c->spk_on;
    if (post_work) HIPCHK(hipEventRecord(ev[e_sub], st));
    if (sub_work) ASWCHK(subpixel_work(c));
    if (c->spk_on) ASWCHK(speckle_work(c));
    HIPCHK(hipEventRecord(ev[e_cons], st));
    // pre-refinement outputs leave before the loop updates its buffers in place
    if (c->spk_on) {
        const asw_speckle_outputs &so = c->spo;
        const size_t off = pair * S;
        if (so.filtered16) HIPCHK(hipMemcpyAsync(so.filtered16 + off, c->spk_f16, S * 2, hipMemcpyDeviceToHost, st));
        if (so.size) HIPCHK(hipMemcpyAsync(so.size + off, c->spk_size, S * 4, hipMemcpyDeviceToHost, st));
        if (so.keep) HIPCHK(hipMemcpyAsync(so.keep + off, c->spk_keep, S, hipMemcpyDeviceToHost, st));
        if (so.disp_lr) HIPCHK(hipMemcpyAsync(so.disp_lr + off, c->spk_lr, S * 4, hipMemcpyDeviceToHost, st));
        if (so.disp_filled)
            HIPCHK(hipMemcpyAsync(so.disp_filled + off, c->spk_fill, S * 4, hipMemcpyDeviceToHost, st));
    }
    if (c->sub_on) {
        const size_t off = pair * S;
        if (c->sub.disp) HIPCHK(hipMemcpyAsync(c->sub.disp + off, c->sp_disp, S * 4, hipMemcpyDeviceToHost, st));
        if (c->sub.disp_lr) HIPCHK(hipMemcpyAsync(c->sub.disp_lr + off, c->sp_lr, S * 4, hipMemcpyDeviceToHost, st));
        if (c->sub.disp_filled)
            HIPCHK(hipMemcpyAsync(c->sub.disp_filled + off, c->sp_fill, S * 4, hipMemcpyDeviceToHost, st));
    }
    if (o) {
        if (o->d_ref) HIPCHK(hipMemcpyAsync(o->d_ref, c->d_ref, S * 4, hipMemcpyDeviceToHost, st));
        if (o->d_tar) HIPCHK(hipMemcpyAsync(o->d_tar, c->d_tar, S * 4, hipMemcpyDeviceToHost, st));
        if (o->conf_ref) HIPCHK(hipMemcpyAsync(o->conf_ref, c->conf_ref, S * 4, hipMemcpyDeviceToHost, st));
        if (o->conf_tar) HIPCHK(hipMemcpyAsync(o->conf_tar, c->conf_tar, S * 4, hipMemcpyDeviceToHost, st));
        if (o->disp_rgba) HIPCHK(hipMemcpyAsync(o->disp_rgba, c->disp, S * 4, hipMemcpyDeviceToHost, st));
        if (o->lr_rgba && p->lr_check) HIPCHK(hipMemcpyAsync(o->lr_rgba, c->lr, S * 4, hipMemcpyDeviceToHost, st));
        if (o->lr_red_rgba && p->lr_check)
            HIPCHK(hipMemcpyAsync(o->lr_red_rgba, c->lr_red, S * 4, hipMemcpyDeviceToHost, st));
        if (o->disp16) HIPCHK(hipMemcpyAsync(o->disp16, c->disp16, S * 2, hipMemcpyDeviceToHost, st));
        if (o->lr16 && p->lr_check) HIPCHK(hipMemcpyAsync(o->lr16, c->lr16, S * 2, hipMemcpyDeviceToHost, st));
        if (o->cost) {
            // [H][W][Dp] of the whole range: shard i fills planes [d_begin_i, d_end_i)
            const size_t Dp = (size_t)asw_disp_pitch(p);
            for (int i = 0; i < c->n; ++i) {
                Shard &s = c->sh[i];
                const size_t dps = (size_t)asw_disp_pitch(&s.p), nloc = (size_t)(s.p.d_end - s.p.d_begin);
                HIPCHK(hipSetDevice(s.device));
                HIPCHK(hipMemcpy2DAsync(o->cost + s.p.d_begin, Dp * 4, s.c0, dps * 4, (c->nranks == 1 ? dps : nloc) * 4,
                                        S, hipMemcpyDeviceToHost, s.stream));
                HIPCHK(hipStreamSynchronize(s.stream));
            }
            HIPCHK(hipSetDevice(s0.device));
        }
    }
    HIPCHK(hipEventRecord(ev[e_pre], st));
    const bool nrefine = c->nrefine && p->lr_check;  // the native loop: never on together with the 8-bit one
    const bool refine = c->refine && p->lr_check;
    if (refine) {  // main.cpp:540-617 on a copy of consistency_error
        if (graphed) ASWCHK(graph_run(st, &c->g_ref, &c->gx_ref, [&] { return refine_work(c); }));
        else ASWCHK(refine_work(c));
    } else if (nrefine) {
        if (graphed) ASWCHK(graph_run(st, &c->g_ref, &c->gx_ref, [&] { return refine_native_work(c); }));
        else ASWCHK(refine_native_work(c));
    }
    HIPCHK(hipEventRecord(ev[e_ref], st));
    if (nrefine) {
        const asw_refine_native_outputs &no = c->nro;
        const size_t off = pair * S;
        if (no.final16) HIPCHK(hipMemcpyAsync(no.final16 + off, c->n_final16, S * 2, hipMemcpyDeviceToHost, st));
        if (no.post16) HIPCHK(hipMemcpyAsync(no.post16 + off, c->n_post16, S * 2, hipMemcpyDeviceToHost, st));
        if (no.d_ref) HIPCHK(hipMemcpyAsync(no.d_ref + off, c->n_dr, S * 4, hipMemcpyDeviceToHost, st));
        if (no.d_tar) HIPCHK(hipMemcpyAsync(no.d_tar + off, c->n_dt, S * 4, hipMemcpyDeviceToHost, st));
    }
    if (o && refine) {
        if (o->final_rgba) HIPCHK(hipMemcpyAsync(o->final_rgba, c->final_rgba, S * 4, hipMemcpyDeviceToHost, st));
        if (o->post_red_rgba && c->rp.iters > 0)
            HIPCHK(hipMemcpyAsync(o->post_red_rgba, c->post_red, S * 4, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipEventRecord(ev[e_d2h], st));
    HIPCHK(hipStreamSynchronize(st));
    for (int i = 1; i < c->n; ++i) {
        HIPCHK(hipSetDevice(c->sh[i].device));
        HIPCHK(hipStreamSynchronize(c->sh[i].stream));
    }
    HIPCHK(hipSetDevice(s0.device));
    if (t && graphed) {  // one graph: only the coarse spans are measured
        std::memset(t, 0, sizeof(*t));
        t->h2d = ms_between(ev[0], ev[1]);
        t->total = ms_between(ev[1], ev[e_cons]);
        t->refine = refine || nrefine ? ms_between(ev[e_pre], ev[e_ref]) : 0.0;
        t->d2h = ms_between(ev[e_cons], ev[e_pre]) + ms_between(ev[e_ref], ev[e_d2h]);
    } else if (t) {
        std::memset(t, 0, sizeof(*t));
        t->h2d = ms_between(ev[0], ev[1]);
        t->raw_cost = ms_between(ev[1], ev[2]);
        if (c->sgm_on) {  // no supports, no passes: the SGM launches, up to the WTA's start, are the aggregation
            t->aggregation_total = ms_between(ev[e_pass0], ev[e_x]);
        } else {
            t->support = ms_between(ev[2], ev[e_pass0]);
            double v = 0.0, h = 0.0;
            for (int it = 0; it < r; ++it) {
                v += ms_between(ev[e_pass0 + 2 * it], ev[e_pass0 + 2 * it + 1]);
                h += ms_between(ev[e_pass0 + 2 * it + 1], ev[e_pass0 + 2 * it + 2]);
            }
            t->v_pass_mean = r ? v / r : 0.0;
            t->h_pass_mean = r ? h / r : 0.0;
            t->aggregation_total = ms_between(ev[e_pass0], ev[e_pass0 + 2 * r]);
        }
        const bool sharded = c->comm != COMM_NONE;
        // (SGM on a one-rank asw_create_rank context records no pass marks: its WTA protocol,
        // an exchange with no peer, is inside aggregation_total and both columns are 0)
        t->exchange = sharded && !c->sgm_on ? ms_between(ev[e_pass0 + 2 * r], ev[e_x]) : 0.0;
        t->wta = sharded ? t->exchange : ms_between(ev[e_x], ev[e_wta]);
        // the sub-pixel maps and the speckle filter: in no column
        t->consistency = ms_between(ev[e_wta], ev[post_work ? e_sub : e_cons]);
        t->total = ms_between(ev[1], ev[e_cons]);
        t->refine = refine || nrefine ? ms_between(ev[e_pre], ev[e_ref]) : 0.0;
        t->d2h = ms_between(ev[e_cons], ev[e_pre]) + ms_between(ev[e_ref], ev[e_d2h]);
    }
    return ASW_OK;
}

}  // namespace

extern "C" {

int asw_destroy(asw_ctx *ctx) { return destroy_ctx(ctx); }

int asw_create(const asw_params *p, int hip_device, asw_ctx **out) {
    return create_ctx(p, &hip_device, 1, 0, 1, COMM_NONE, nullptr, out);
}

int asw_create_multi(const asw_params *p, const int *hip_device_ids, int n_devices, asw_ctx **out) {
    if (!out) return ASW_E_INVALID;
    *out = nullptr;
    if (!hip_device_ids || n_devices < 1 || n_devices > kMaxShards) return ASW_E_INVALID;
    CommMode comm = n_devices == 1 ? COMM_NONE : COMM_RCCL;
    for (int i = 0; i < n_devices; ++i)
        for (int j = 0; j < i; ++j)
            if (hip_device_ids[i] == hip_device_ids[j]) comm = COMM_LOCAL;  // RCCL needs one rank per device
    if (n_devices > 1 && p && (p->flags & ASW_FLAG_COMM_LOCAL)) comm = COMM_LOCAL;
    return create_ctx(p, hip_device_ids, n_devices, 0, n_devices, comm, nullptr, out);
}

int asw_comm_unique_id(uint8_t id[ASW_COMM_ID_BYTES]) {
    if (!id) return ASW_E_INVALID;
    ncclUniqueId u;
    if (ncclGetUniqueId(&u) != ncclSuccess) return ASW_E_COMM;
    static_assert(sizeof(u) == ASW_COMM_ID_BYTES, "ncclUniqueId size");
    std::memcpy(id, &u, sizeof u);
    return ASW_OK;
}

int asw_create_rank(const asw_params *p, int hip_device, int rank, int nranks, const uint8_t id[ASW_COMM_ID_BYTES],
                    asw_ctx **out) {
    if (!out) return ASW_E_INVALID;
    *out = nullptr;
    if (!id || nranks < 1 || rank < 0 || rank >= nranks) return ASW_E_INVALID;
    ncclUniqueId u;
    std::memcpy(&u, id, sizeof u);
    return create_ctx(p, &hip_device, 1, rank, nranks, COMM_RCCL, &u, out);
}

int asw_ctx_shard(const asw_ctx *ctx, int i, int *n_shards, int *d_begin, int *d_end) {
    if (!ctx) return ASW_E_INVALID;
    if (n_shards) *n_shards = ctx->n;
    if (i < 0 || i >= ctx->n) return ASW_E_INVALID;
    if (d_begin) *d_begin = ctx->sh[i].p.d_begin;
    if (d_end) *d_end = ctx->sh[i].p.d_end;
    return ASW_OK;
}

int asw_device_name(int hip_device, char *buf, int len) {
    if (!buf || len < 1) return ASW_E_INVALID;
    buf[0] = '\0';
    hipDeviceProp_t prop;
    const hipError_t e = hipGetDeviceProperties(&prop, hip_device);
    if (e != hipSuccess) return hip_fail(e);
    std::snprintf(buf, (size_t)len, "%s", prop.name[0] ? prop.name : prop.gcnArchName);
    return ASW_OK;
}

// sharded refinement (either loop): the estimates of both views on every shard but the first,
// and the event that orders their copies; leaves shard 0's device current
static int alloc_sharded_refine(asw_ctx *c) {
    const size_t S = frame_pixels(&c->p);
    for (int i = 1; i < c->n; ++i) {
        Shard &s = c->sh[i];
        HIPCHK(hipSetDevice(s.device));
        if (!s.ref_l) ASWCHK(dev_alloc(&s.ref_l, 2 * S * 4));
        if (!s.ref_r) ASWCHK(dev_alloc(&s.ref_r, 2 * S * 4));
    }
    HIPCHK(hipSetDevice(c->sh[0].device));
    if (c->n > 1 && !c->red_done) HIPCHK(hipEventCreateWithFlags(&c->red_done, hipEventDisableTiming));
    return ASW_OK;
}

static void drop_refine_graph(asw_ctx *c) {
    if (!c->gx_ref) return;
    (void)hipGraphExecDestroy(c->gx_ref);
    (void)hipGraphDestroy(c->g_ref);
    c->gx_ref = nullptr;
    c->g_ref = nullptr;
}

int asw_set_refine_native(asw_ctx *c, const asw_refine_params *rp, const asw_refine_native_outputs *o) {
    if (!c) return ASW_E_INVALID;
    if (!rp || rp->iters <= 0) {
        if (c->nrefine) drop_refine_graph(c);
        c->nrefine = false;
        c->nro = asw_refine_native_outputs{};
        return ASW_OK;
    }
    if (!o) return ASW_E_INVALID;
    ASWCHK(asw_refine_native_params_check(&c->p, rp));
    if (!c->p.lr_check) return ASW_E_INVALID;  // the loop starts from the LR-checked confidences
    if (c->refine) return ASW_E_INVALID;       // one loop per context (asw_set_refine)
    const size_t S = frame_pixels(&c->p);
    ASWCHK(alloc_sharded_refine(c));
    const bool same = c->nrefine && std::memcmp(&c->nrp, rp, sizeof *rp) == 0;
    if (!same) {  // a captured loop used the previous workspace / parameters
        drop_refine_graph(c);
        if (c->nrws) (void)hipFree(c->nrws);
        c->nrws = nullptr;
        ASWCHK(dev_alloc(&c->nrws, asw_refine_native_workspace_bytes(&c->p, rp)));
    }
    if (!c->n_est) ASWCHK(dev_alloc(&c->n_est, S * 4));
    if (!c->n_dt) ASWCHK(dev_alloc(&c->n_dt, S * 4));
    if (!c->n_dr) ASWCHK(dev_alloc(&c->n_dr, S * 4));
    if (!c->n_post16) ASWCHK(dev_alloc(&c->n_post16, S * 2));
    if (!c->n_final16) ASWCHK(dev_alloc(&c->n_final16, S * 2));
    c->nrp = *rp;
    c->nro = *o;
    c->nrefine = true;
    return ASW_OK;
}

int asw_set_refine(asw_ctx *c, const asw_refine_params *rp) {
    if (!c) return ASW_E_INVALID;
    if (!rp || rp->iters <= 0) {
        c->refine = false;
        return ASW_OK;
    }
    const int s = asw_refine_params_check(&c->p, rp);
    if (s != ASW_OK) return s;
    if (!c->p.lr_check) return ASW_E_INVALID;  // the loop starts from the consistency image
    if (c->nrefine) return ASW_E_INVALID;      // one loop per context (asw_set_refine_native)
    const size_t S = frame_pixels(&c->p);
    ASWCHK(alloc_sharded_refine(c));
    const size_t ws = asw_refine_workspace_bytes(&c->p, rp);
    if (c->rws) (void)hipFree(c->rws);
    c->rws = nullptr;
    ASWCHK(dev_alloc(&c->rws, ws));
    if (!c->est) ASWCHK(dev_alloc(&c->est, S * 4));
    if (!c->post_red) ASWCHK(dev_alloc(&c->post_red, S * 4));
    if (!c->final_rgba) ASWCHK(dev_alloc(&c->final_rgba, S * 4));
    c->rp = *rp;
    c->refine = true;
    if (c->gx_ref) {  // the captured loop used the previous workspace / parameters
        (void)hipGraphExecDestroy(c->gx_ref);
        (void)hipGraphDestroy(c->g_ref);
        c->gx_ref = nullptr;
        c->g_ref = nullptr;
    }
    return ASW_OK;
}

// the device disp map of subpixel_work (asw_set_subpixel, asw_set_speckle's float outputs) and,
// on a sharded frame, the operands of its one all-reduce; allocated once
static int alloc_subpixel_disp(asw_ctx *c) {
    const size_t S = frame_pixels(&c->p);
    if (c->comm != COMM_NONE) {
        for (int i = 0; i < c->n; ++i) {
            Shard &s = c->sh[i];
            HIPCHK(hipSetDevice(s.device));
            if (!s.nb) ASWCHK(dev_alloc(&s.nb, 3 * S * 4));
        }
    }
    HIPCHK(hipSetDevice(c->sh[0].device));
    if (c->red_tmp && !c->sp_disp) {  // peer operands of the device-local exchange: 12 bytes per pixel now
        (void)hipFree(c->red_tmp);
        c->red_tmp = nullptr;
        ASWCHK(dev_alloc(&c->red_tmp, (size_t)(c->n - 1) * S * 12));
    }
    if (!c->sp_disp) ASWCHK(dev_alloc(&c->sp_disp, S * 4));
    return ASW_OK;
}

int asw_set_subpixel(asw_ctx *c, const asw_subpixel_outputs *o) {
    if (!c) return ASW_E_INVALID;
    if (!o || (!o->disp && !o->disp_lr && !o->disp_filled)) {
        c->sub_on = false;
        c->sub = asw_subpixel_outputs{};
        return ASW_OK;
    }
    if ((o->disp_lr || o->disp_filled) && !c->p.lr_check) return ASW_E_INVALID;  // they are LR-masked maps
    const size_t S = frame_pixels(&c->p);
    ASWCHK(alloc_subpixel_disp(c));
    if ((o->disp_lr || o->disp_filled) && !c->sp_lr) ASWCHK(dev_alloc(&c->sp_lr, S * 4));
    if (o->disp_filled && !c->sp_fill) ASWCHK(dev_alloc(&c->sp_fill, S * 4));
    c->sub = *o;
    c->sub_on = true;
    return ASW_OK;
}

int asw_set_speckle(asw_ctx *c, const asw_speckle_params *sp, const asw_speckle_outputs *o) {
    if (!c) return ASW_E_INVALID;
    if (!sp) {
        c->spk_on = false;
        c->spo = asw_speckle_outputs{};
        return ASW_OK;
    }
    if (!o) return ASW_E_INVALID;
    ASWCHK(asw_speckle_params_check(&c->p, sp));
    if (o->filtered16 && c->p.ndisp > 65535) return ASW_E_INVALID;  // asw_speckle_mask16's rule
    const size_t S = frame_pixels(&c->p);
    const bool want_disp = o->disp_lr || o->disp_filled;
    if (want_disp) ASWCHK(alloc_subpixel_disp(c));
    HIPCHK(hipSetDevice(c->sh[0].device));
    if (c->p.lr_check && !c->spk_valid) ASWCHK(dev_alloc(&c->spk_valid, S));
    if (!c->spk_ws) ASWCHK(dev_alloc(&c->spk_ws, asw_speckle_workspace_bytes(&c->p)));
    if (!c->spk_size) ASWCHK(dev_alloc(&c->spk_size, S * 4));
    if (!c->spk_keep) ASWCHK(dev_alloc(&c->spk_keep, S));
    if (o->filtered16 && !c->spk_f16) ASWCHK(dev_alloc(&c->spk_f16, S * 2));
    if (want_disp && !c->spk_lr) ASWCHK(dev_alloc(&c->spk_lr, S * 4));
    if (o->disp_filled && !c->spk_fill) ASWCHK(dev_alloc(&c->spk_fill, S * 4));
    c->spk = *sp;
    c->spo = *o;
    c->spk_on = true;
    return ASW_OK;
}

int asw_set_cross(asw_ctx *c, const asw_cross_params *cp, const asw_cross_outputs *o) {
    if (!c) return ASW_E_INVALID;
    if (!cp) {
        c->cross_on = false;
        c->cro = asw_cross_outputs{};
        return ASW_OK;
    }
    if (!o) return ASW_E_INVALID;
    if (c->n > 1 || c->nranks > 1) return ASW_E_UNSUPPORTED;  // shard-sized volumes
    ASWCHK(asw_cross_params_check(&c->p, cp));
    const size_t S = frame_pixels(&c->p);
    HIPCHK(hipSetDevice(c->sh[0].device));
    if (!c->cr_med_l) ASWCHK(dev_alloc(&c->cr_med_l, S * 4));
    if (!c->cr_med_r) ASWCHK(dev_alloc(&c->cr_med_r, S * 4));
    if (!c->cr_arms_l) ASWCHK(dev_alloc(&c->cr_arms_l, asw_cross_arm_bytes(&c->p)));
    if (!c->cr_arms_r) ASWCHK(dev_alloc(&c->cr_arms_r, asw_cross_arm_bytes(&c->p)));
    if (!c->cr_d0) ASWCHK(dev_alloc(&c->cr_d0, S * 4));
    if (!c->cr_code0) ASWCHK(dev_alloc(&c->cr_code0, S));
    if (!c->cr_code1) ASWCHK(dev_alloc(&c->cr_code1, S));
    if (!c->cr_init) ASWCHK(dev_alloc(&c->cr_init, S * 4));
    if (!c->cr_final) ASWCHK(dev_alloc(&c->cr_final, S * 4));
    if (c->cr_ev.empty()) {
        c->cr_ev.assign(kCrossEvents, nullptr);
        for (hipEvent_t &e : c->cr_ev) HIPCHK(hipEventCreate(&e));
    }
    c->cp = *cp;
    c->cro = *o;
    c->cross_on = true;
    return ASW_OK;
}

int asw_set_census(asw_ctx *c, const asw_census_params *cp) {
    if (!c) return ASW_E_INVALID;
    if (!cp && c->sgm_on && !cost16_exists(&c->p, nullptr)) return ASW_E_UNSUPPORTED;  // SGM reads the uint16 volume
    if (cp) {
        for (int i = 0; i < c->n; ++i) ASWCHK(asw_census_params_check(&c->sh[i].p, cp));
        if (c->sgm_on && !cost16_exists(&c->p, cp)) return ASW_E_UNSUPPORTED;  // SGM reads the uint16 volume
        for (int i = 0; i < c->n; ++i) {
            Shard &s = c->sh[i];
            HIPCHK(hipSetDevice(s.device));
            if (!s.cen_l) ASWCHK(dev_alloc(&s.cen_l, asw_census_bytes(&s.p)));
            if (!s.cen_r) ASWCHK(dev_alloc(&s.cen_r, asw_census_bytes(&s.p)));
            s.census16 = !(s.p.flags & ASW_FLAG_RAW_F32) && asw_census16_supported(&s.p, cp);
        }
        HIPCHK(hipSetDevice(c->sh[0].device));
        c->cen = *cp;
    }
    c->census_on = cp != nullptr;
    if (c->gx_main) {  // the captured frame holds the previous cost's launches: capture again
        (void)hipGraphExecDestroy(c->gx_main);
        (void)hipGraphDestroy(c->g_main);
        c->gx_main = nullptr;
        c->g_main = nullptr;
    }
    return ASW_OK;
}

int asw_set_sgm(asw_ctx *c, const asw_sgm_params *sp) {
    if (!c) return ASW_E_INVALID;
    if (sp) {
        if (c->n > 1 || c->nranks > 1) return ASW_E_UNSUPPORTED;  // m is a minimum over every disparity
        ASWCHK(asw_sgm_params_check(&c->sh[0].p, sp));
        ASWCHK(asw::sgm_shape_check(&c->sh[0].p));
        if (!cost16_exists(&c->p, c->census_on ? &c->cen : nullptr)) return ASW_E_UNSUPPORTED;
        const size_t ws = asw_sgm_workspace_bytes(&c->sh[0].p, sp);
        if (ws > 0) {
            HIPCHK(hipSetDevice(c->sh[0].device));
            void *buf = nullptr;
            ASWCHK(dev_alloc(&buf, ws));
            if (c->sgm_ws) (void)hipFree(c->sgm_ws);
            c->sgm_ws = buf;
        }
        c->sgm = *sp;
    } else if (!c->sgm_on) {
        return ASW_OK;  // off already: nothing captured differs
    }
    c->sgm_on = sp != nullptr;
    if (c->gx_main) {  // the captured frame holds the previous aggregator's launches: capture again
        (void)hipGraphExecDestroy(c->gx_main);
        (void)hipGraphDestroy(c->g_main);
        c->gx_main = nullptr;
        c->g_main = nullptr;
    }
    return ASW_OK;
}

int asw_set_graph(asw_ctx *c, int on) {
    if (!c) return ASW_E_INVALID;
    if (on && c->comm != COMM_NONE) return ASW_E_UNSUPPORTED;  // one shard, one stream
    c->graph = on != 0;
    return ASW_OK;
}

int asw_match(asw_ctx *c, const uint8_t *left_rgba, const uint8_t *right_rgba, asw_outputs *o, asw_timings *t) {
    if (!c || !left_rgba || !right_rgba) return ASW_E_INVALID;
    return match_one(c, left_rgba, right_rgba, o, t);
}

int asw_match_batch(asw_ctx *c, const uint8_t *left_rgba, const uint8_t *right_rgba, int batch, asw_outputs *out,
                    asw_timings *t) {
    if (!c || !left_rgba || !right_rgba || batch < 0 || (batch > 0 && !out)) return ASW_E_INVALID;
    const size_t img = frame_pixels(&c->p) * 4;
    for (int b = 0; b < batch; ++b)
        ASWCHK(match_one(c, left_rgba + (size_t)b * img, right_rgba + (size_t)b * img, &out[b], t ? &t[b] : nullptr,
                         (size_t)b));
    return ASW_OK;
}

}  // extern "C"
