// asw_sgm.hip — semi-global matching (Hirschmueller 2008) on the uint16 raw-cost volume
// (include/asw.h §SGM).  No reference counterpart: the reference's only
// aggregator is the iterated ASW pass.  Every operation is an integer one; the sum S of the
// path costs is below 2^24, so its float32 form and every float add of it are exact.
//
//   L_k(p, d) = C(p, d) + min(L_k(q, d), L_k(q, d-1) + P1, L_k(q, d+1) + P1, m + P2) - m
//   q = p - step_k,  m = min_j L_k(q, j);  L_k(p, d) = C(p, d) where q lies outside the image
//
// One kernel, k_sgm_path, serves all eight paths.  A WALKER is one block that follows one
// path through the image: a row for the horizontal paths (H walkers of W steps), a start
// column for the vertical and diagonal ones (W walkers of H steps; the column of a diagonal
// walker is (x0 + dx * step) mod W and its path restarts, L = C, whenever it wraps, so every
// walker is busy for all H rows and the border rule needs no other case).  The threads of a
// walker are spread over d, PL consecutive planes each, and L_k(q, .) never leaves their
// registers: the d +- 1 neighbours of the inner planes are registers of the same thread, the
// two outer ones come from the neighbouring lanes (and, in a walker of several waves, from
// the neighbouring wave through LDS), m is a DPP row reduction + four v_readlane per wave
// (+ one LDS exchange per step between waves: one barrier, double-buffered by step parity).
// The cost (and, when accumulating, sum) loads of a path are known in advance: a ring of PF
// steps is in flight ahead of the serial min/add chain, the only true dependency.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "asw_common.h"

namespace asw {
namespace {

constexpr int kSgmBig = 0x3FFFFFFF;      // "no such plane": + P1 or + P2 (<= 2^20) cannot overflow
constexpr int kSgmMaxPenalty = 1 << 20;  // 1048576
constexpr int kSgmMaxWaves = 16;

// step (dx, dy) of path k: the predecessor of (x, y) is (x - dx, y - dy)
constexpr int kSgmDx[8] = {+1, -1, 0, 0, +1, -1, -1, +1};
constexpr int kSgmDy[8] = {0, 0, +1, -1, +1, -1, +1, -1};

// PL uint16 costs of one thread, packed as loaded
template <int PL>
struct CostRegs {
    unsigned w[(PL + 1) / 2];
};

template <int PL>
__device__ __forceinline__ void load_cost(const unsigned short *__restrict__ p, CostRegs<PL> &r) {
    if constexpr (PL == 1) {
        r.w[0] = p[0];
    } else if constexpr (PL == 2) {
        r.w[0] = *reinterpret_cast<const unsigned *>(p);
    } else if constexpr (PL == 4) {
        const uint2 v = *reinterpret_cast<const uint2 *>(p);
        r.w[0] = v.x;
        r.w[1] = v.y;
    } else {
#pragma unroll
        for (int i = 0; i < PL / 8; ++i) {
            const uint4 v = reinterpret_cast<const uint4 *>(p)[i];
            r.w[4 * i] = v.x;
            r.w[4 * i + 1] = v.y;
            r.w[4 * i + 2] = v.z;
            r.w[4 * i + 3] = v.w;
        }
    }
}

template <int PL>
__device__ __forceinline__ int cost_of(const CostRegs<PL> &r, int j) {
    return (int)((r.w[j >> 1] >> ((j & 1) * 16)) & 0xFFFFu);
}

template <int N>
__device__ __forceinline__ void load_sum(const float *__restrict__ p, float *f) {
    if constexpr (N == 1) {
        f[0] = p[0];
    } else if constexpr (N == 2) {
        const float2 v = *reinterpret_cast<const float2 *>(p);
        f[0] = v.x;
        f[1] = v.y;
    } else {
#pragma unroll
        for (int i = 0; i < N / 4; ++i) {
            const float4 v = reinterpret_cast<const float4 *>(p)[i];
            f[4 * i] = v.x;
            f[4 * i + 1] = v.y;
            f[4 * i + 2] = v.z;
            f[4 * i + 3] = v.w;
        }
    }
}

template <int N>
__device__ __forceinline__ void store_sum(float *__restrict__ p, const float *f) {
    if constexpr (N == 1) {
        p[0] = f[0];
    } else if constexpr (N == 2) {
        *reinterpret_cast<float2 *>(p) = make_float2(f[0], f[1]);
    } else {
#pragma unroll
        for (int i = 0; i < N / 4; ++i)
            reinterpret_cast<float4 *>(p)[i] = make_float4(f[4 * i], f[4 * i + 1], f[4 * i + 2], f[4 * i + 3]);
    }
}

// minimum over the 64 lanes, wave-uniform: four DPP steps leave every row of 16 lanes with
// its minimum (the partners of quad_perm / row_half_mirror / row_mirror are symmetric), one
// v_readlane per row and three scalar minima join the rows.  Every lane must be active.
__device__ __forceinline__ int wave_min(int v) {
    v = min(v, __builtin_amdgcn_update_dpp(v, v, 0xB1, 0xF, 0xF, false));   // quad_perm [1,0,3,2]
    v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x4E, 0xF, 0xF, false));   // quad_perm [2,3,0,1]
    v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x141, 0xF, 0xF, false));  // row_half_mirror
    v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x140, 0xF, 0xF, false));  // row_mirror
    const int a = min(__builtin_amdgcn_readlane(v, 0), __builtin_amdgcn_readlane(v, 16));
    const int b = min(__builtin_amdgcn_readlane(v, 32), __builtin_amdgcn_readlane(v, 48));
    return min(a, b);
}

// position of a walker on its path; advance() returns whether the path restarts at the new
// position (a diagonal walker's column wrapped: the predecessor lies outside the image)
struct Cursor {
    int x, y;
    __device__ __forceinline__ bool advance(int dx, int dy, int W) {
        y += dy;
        x += dx;
        if (dy == 0) return false;  // a row walker never leaves its row before its last step
        if (x == W) {
            x = 0;
            return true;
        }
        if (x < 0) {
            x = W - 1;
            return true;
        }
        return false;
    }
};

// PL planes per thread; ONE: the walker is one wave (no LDS, no barrier).  PF steps of loads
// in flight: 4 where a step's registers are few, 1 for the deep forms.
template <int PL, bool ONE>
__global__ __launch_bounds__(ONE ? 64 : 1024) void k_sgm_path(const unsigned short *__restrict__ C,
                                                               float *__restrict__ S, int W, int H, int Dp,
                                                               int ndisp, int dx, int dy, int P1, int P2,
                                                               int accumulate) {
    constexpr int PF = PL <= 4 ? 4 : 1;
    constexpr bool kPrefetchSum = PL <= 4;
    constexpr bool kDeep = PL > 16;        // no ring: the costs are loaded in chunks inside the chain
    constexpr int CHK = kDeep ? 8 : PL;    // planes per chunk
    __shared__ int x_min[2][kSgmMaxWaves], x_first[2][kSgmMaxWaves], x_last[2][kSgmMaxWaves];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int nwaves = (int)blockDim.x >> 6;
    const int d0 = t * PL;
    const bool active = d0 < Dp;  // whole threads: PL divides 64, Dp is a multiple of 64
    const int nsteps = dy == 0 ? W : H;
    Cursor cur, pre;  // the step being computed, the step being loaded
    if (dy == 0) {
        cur.x = dx > 0 ? 0 : W - 1;
        cur.y = (int)blockIdx.x;
    } else {
        cur.x = (int)blockIdx.x;
        cur.y = dy > 0 ? 0 : H - 1;
    }
    pre = cur;
    auto offset = [&](const Cursor &c) __attribute__((always_inline)) {
        return ((long long)c.y * W + c.x) * Dp + d0;
    };

    int L[PL];
#pragma unroll
    for (int j = 0; j < PL; ++j) L[j] = kSgmBig;
    int m = 0, edge_left = kSgmBig, edge_right = kSgmBig;  // of the previous step
    bool restart = true;

    CostRegs<PL> cb[PF];
    float sb[PF][kPrefetchSum ? PL : 1];
#pragma unroll
    for (int i = 0; i < PF; ++i) {
#pragma unroll
        for (int j = 0; j < (PL + 1) / 2; ++j) cb[i].w[j] = 0u;
#pragma unroll
        for (int j = 0; j < (kPrefetchSum ? PL : 1); ++j) sb[i][j] = 0.0f;
        if (i < nsteps) {
            if (active) {
                const long long o = offset(pre);
                if constexpr (!kDeep) load_cost<PL>(C + o, cb[i]);
                if constexpr (kPrefetchSum)
                    if (accumulate) load_sum<PL>(S + o, sb[i]);
            }
            pre.advance(dx, dy, W);
        }
    }

    for (int s0 = 0; s0 < nsteps; s0 += PF) {
#pragma unroll
        for (int i = 0; i < PF; ++i) {
            const int s = s0 + i;
            if (s >= nsteps) break;  // block-uniform
            // ---- the serial chain: L of this pixel from L of the predecessor
            const long long ocur = offset(cur);
            auto chunk = [&](int q) __attribute__((always_inline)) {
                CostRegs<CHK> cq;
                if constexpr (kDeep) {  // loaded where it is used: 64 planes of L leave no room for a ring
#pragma unroll
                    for (int j = 0; j < (CHK + 1) / 2; ++j) cq.w[j] = 0u;
                    if (active) load_cost<CHK>(C + ocur + q * CHK, cq);
                } else {
                    cq = cb[i];
                }
                return cq;
            };
            if (restart) {
#pragma unroll
                for (int q = 0; q < PL / CHK; ++q) {
                    const CostRegs<CHK> cq = chunk(q);
#pragma unroll
                    for (int jj = 0; jj < CHK; ++jj) {
                        const int j = q * CHK + jj;
                        L[j] = d0 + j < ndisp ? cost_of<CHK>(cq, jj) : kSgmBig;
                    }
                }
            } else {
                int left = __shfl_up(L[PL - 1], 1), right = __shfl_down(L[0], 1);
                if (lane == 0) left = edge_left;
                if (lane == 63) right = edge_right;
                const int mp2 = m + P2;
                int prev = left;
#pragma unroll
                for (int q = 0; q < PL / CHK; ++q) {
                    const CostRegs<CHK> cq = chunk(q);
#pragma unroll
                    for (int jj = 0; jj < CHK; ++jj) {
                        const int j = q * CHK + jj;
                        const int old = L[j];
                        const int next = j + 1 < PL ? L[j + 1] : right;
                        const int v = min(min(old, mp2), min(prev, next) + P1);
                        L[j] = d0 + j < ndisp ? cost_of<CHK>(cq, jj) + v - m : kSgmBig;
                        prev = old;
                    }
                }
            }
            // ---- m and the outer planes of the neighbouring waves for the next step
            int lm = L[0];
#pragma unroll
            for (int j = 1; j < PL; ++j) lm = min(lm, L[j]);
            const int wm = wave_min(lm);
            if constexpr (ONE) {
                m = wm;
            } else {
                const int b = s & 1;
                if (lane == 0) {
                    x_min[b][wave] = wm;
                    x_first[b][wave] = L[0];
                }
                if (lane == 63) x_last[b][wave] = L[PL - 1];
                __syncthreads();
                m = x_min[b][0];
                for (int w = 1; w < nwaves; ++w) m = min(m, x_min[b][w]);
                edge_left = wave > 0 ? x_last[b][wave - 1] : kSgmBig;
                edge_right = wave + 1 < nwaves ? x_first[b][wave + 1] : kSgmBig;
            }
            // ---- the output row of this pixel
            if (active) {
                const long long o = ocur;
                if constexpr (kPrefetchSum) {
                    float f[PL];
#pragma unroll
                    for (int j = 0; j < PL; ++j) {
                        const bool valid = d0 + j < ndisp;
                        if (accumulate) f[j] = valid ? sb[i][j] + (float)L[j] : sb[i][j];
                        else f[j] = valid ? (float)L[j] : 0.0f;
                    }
                    store_sum<PL>(S + o, f);
                } else {
#pragma unroll
                    for (int q = 0; q < PL / 4; ++q) {
                        float f[4];
                        if (accumulate) load_sum<4>(S + o + 4 * q, f);
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const bool valid = d0 + 4 * q + j < ndisp;
                            if (accumulate) f[j] = valid ? f[j] + (float)L[4 * q + j] : f[j];
                            else f[j] = valid ? (float)L[4 * q + j] : 0.0f;
                        }
                        store_sum<4>(S + o + 4 * q, f);
                    }
                }
            }
            // ---- the loads of step s + PF into the slot this step has freed
            if (s + PF < nsteps) {
                if (active) {
                    const long long o = offset(pre);
                    if constexpr (!kDeep) load_cost<PL>(C + o, cb[i]);
                    if constexpr (kPrefetchSum)
                        if (accumulate) load_sum<PL>(S + o, sb[i]);
                }
                pre.advance(dx, dy, W);
            }
            restart = cur.advance(dx, dy, W);
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

template <int PL, bool ONE>
int launch_form(const asw_params *p, const asw_sgm_params *sp, int k, const uint16_t *cost16, float *sum,
                int accumulate, hipStream_t st) {
    const int Dp = asw_disp_pitch(p);
    const int threads = ONE ? 64 : round_up((Dp + PL - 1) / PL, 64);
    const int walkers = kSgmDy[k] == 0 ? p->height : p->width;
    hipLaunchKernelGGL((k_sgm_path<PL, ONE>), dim3((unsigned)walkers), dim3((unsigned)threads), 0, st, cost16, sum,
                       p->width, p->height, Dp, p->ndisp, kSgmDx[k], kSgmDy[k], sp->p1, sp->p2, accumulate ? 1 : 0);
    return finish_launch();
}

// the form of a pitch: one wave up to 256 planes, then up to 16 waves of 4, 16, 32 or 64
// planes per thread (the last, for ndisp > 32768 only, is the one form with scratch: 64
// planes of L and their validity masks exceed the 128 registers of a 1024-thread block).
// Offsets are 64-bit, so no shape overflows them; a pitch above 65536 planes is not built
// (sgm_shape_check).
int launch_path(const asw_params *p, const asw_sgm_params *sp, int k, const uint16_t *cost16, float *sum,
                int accumulate, hipStream_t st) {
    const int Dp = asw_disp_pitch(p);
    if (Dp == 64) return launch_form<1, true>(p, sp, k, cost16, sum, accumulate, st);
    if (Dp == 128) return launch_form<2, true>(p, sp, k, cost16, sum, accumulate, st);
    if (Dp <= 256) return launch_form<4, true>(p, sp, k, cost16, sum, accumulate, st);
    if (Dp <= 4 * 64 * kSgmMaxWaves) return launch_form<4, false>(p, sp, k, cost16, sum, accumulate, st);
    if (Dp <= 16 * 64 * kSgmMaxWaves) return launch_form<16, false>(p, sp, k, cost16, sum, accumulate, st);
    if (Dp <= 32 * 64 * kSgmMaxWaves) return launch_form<32, false>(p, sp, k, cost16, sum, accumulate, st);
    if (Dp <= 64 * 64 * kSgmMaxWaves) return launch_form<64, false>(p, sp, k, cost16, sum, accumulate, st);
    return ASW_E_UNSUPPORTED;
}

}  // namespace

// threads of a walker at a pitch (launch_path's forms)
static int sgm_threads(int Dp) {
    if (Dp <= 256) return 64;
    const int PL = Dp <= 4 * 64 * kSgmMaxWaves ? 4 : Dp <= 16 * 64 * kSgmMaxWaves ? 16 : Dp <= 32 * 64 * kSgmMaxWaves ? 32 : 64;
    return round_up((Dp + PL - 1) / PL, 64);
}

// a pitch k_sgm_path is built for, and launches (one block per row or per column) of at
// most 2^32 - 1 work-items, what a dispatch holds
int sgm_shape_check(const asw_params *p) {
    const int Dp = asw_disp_pitch(p);
    if (Dp > 64 * 64 * kSgmMaxWaves) return ASW_E_UNSUPPORTED;
    const long long walkers = p->width > p->height ? p->width : p->height;
    return walkers * sgm_threads(Dp) > 0xffffffffLL ? ASW_E_UNSUPPORTED : ASW_OK;
}

}  // namespace asw

using namespace asw;

extern "C" {

void asw_sgm_params_default(asw_sgm_params *sp) {
    if (!sp) return;
    sp->paths = 8;
    sp->p1 = 16;
    sp->p2 = 128;
}

int asw_sgm_params_check(const asw_params *p, const asw_sgm_params *sp) {
    if (!p || !sp) return ASW_E_INVALID;
    if (const int s = asw_params_check(p)) return s;
    if (p->d_begin > 0 || d_end_of_p(p) < p->ndisp) return ASW_E_INVALID;  // m is a minimum over every plane
    if (sp->paths != 4 && sp->paths != 8) return ASW_E_INVALID;
    if (sp->p1 < 0 || sp->p1 > sp->p2 || sp->p2 > kSgmMaxPenalty) return ASW_E_INVALID;
    return ASW_OK;
}

size_t asw_sgm_workspace_bytes(const asw_params *p, const asw_sgm_params *sp) {
    (void)p;
    (void)sp;
    return 0;  // every path accumulates directly in the float volume
}

int asw_sgm_path(const asw_params *p, const asw_sgm_params *sp, int k, const uint16_t *cost16, float *sum,
                 int accumulate, void *stream) {
    if (const int s = asw_sgm_params_check(p, sp)) return s;
    if (k < 0 || k >= 8 || !cost16 || !sum) return ASW_E_INVALID;
    if (static_cast<const void *>(cost16) == static_cast<const void *>(sum)) return ASW_E_INVALID;
    if (const int s = sgm_shape_check(p)) return s;
    return launch_path(p, sp, k, cost16, sum, accumulate, (hipStream_t)stream);
}

int asw_sgm(const asw_params *p, const asw_sgm_params *sp, const uint16_t *cost16, float *sum, void *workspace,
            void *stream) {
    if (const int s = asw_sgm_params_check(p, sp)) return s;
    if (!cost16 || !sum) return ASW_E_INVALID;
    if (static_cast<const void *>(cost16) == static_cast<const void *>(sum)) return ASW_E_INVALID;
    if (!workspace && asw_sgm_workspace_bytes(p, sp) > 0) return ASW_E_INVALID;
    if (const int s = sgm_shape_check(p)) return s;
    // the first path writes the volume (padding planes +0), the others add to it: every
    // partial sum is an integer below 2^24, so the order is free and each add exact
    for (int k = 0; k < sp->paths; ++k)
        if (const int s = launch_path(p, sp, k, cost16, sum, k > 0, (hipStream_t)stream)) return s;
    return ASW_OK;
}

}  // extern "C"
