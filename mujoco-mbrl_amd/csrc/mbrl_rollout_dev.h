// Device helpers shared by the rollout kernels (rollout.hip: rollout_kernel, rollout_m8_kernel,
// rollout_m4_kernel; rollout_f16x3.hip: rollout_split_kernel): the prologue staging, the action waves'
// work, the cost write-out and the diagnostic stamps. The goal-state epilogue is not here: each fp32
// kernel keeps its own copy (through a shared function hipcc compiled m4's and rollout_kernel's step
// loops longer), and so does rollout_kernel's statistics / s0 staging (its pair instances' loops grew).
// The split kernel shares rowsum16 and stage_params only. Everything is force-inlined; the LDS row
// stride lda comes in by value so that the ring instances' compile-time strides still fold.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mbrl_internal.h"

// State slots per lane (ceil(s / 16)) up to which the 8/16-candidate epilogues keep their per-lane
// parameter copies in registers; wider states read them from LDS (the copies spilled on humanoid).
#ifndef MBRL_EPI_REG_SLOTS
#define MBRL_EPI_REG_SLOTS 2
#endif

namespace mbrl {

// Sum over the 16 lanes of a DPP row (row_ror 8, 4, 2, 1): every lane of the row gets the total.
__device__ __forceinline__ float rowsum16(float v) {
    v += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x128, 0xF, 0xF, false));
    v += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x124, 0xF, 0xF, false));
    v += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x122, 0xF, 0xF, false));
    v += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x121, 0xF, 0xF, false));
    return v;
}

// Epilogue mapping: lane l of wave w owns candidate row m = 16r + 4w + (l >> 4) and the feature
// slots d = (l & 15) + 16k of that row, so per-row reductions are one DPP row sum.
constexpr int MAX_A_PER_LANE = 3;  // action_dim <= 48

__device__ __forceinline__ int epi_row(int r, int wave, int lane) { return 16 * r + 4 * wave + (lane >> 4); }

// a_t for this lane's (row, slots), loaded early and unconditionally (clamped indices) so hipcc
// emits no branch-around-load with its vmcnt(0) (cdna_hip_programming.md §5, trap (c)). M is the
// tile height: 16 R, or 8 / 4 with R = 1.
template <int R, int M = 16 * R>
__device__ __forceinline__ void fetch_actions(const RolloutArgs& A, int tile, int t, int wave, int lane,
                                              float (&av)[R][MAX_A_PER_LANE]) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int n = min(tile * M + epi_row(r, wave, lane), A.N - 1);
        const float* src = A.actions + ((size_t)t * A.N + n) * A.a;
#pragma unroll
        for (int k = 0; k < MAX_A_PER_LANE; ++k) av[r][k] = src[min((lane & 15) + 16 * k, A.a - 1)];
    }
}

// Statistics (NULL: mean 0, std 1, goal 0, weight 0) and the member's bias block into LDS. No
// barrier: the caller places its own before the first read. Lds is LdsMap or the split kernel's map.
template <class Lds>
__device__ __forceinline__ void stage_params(const RolloutArgs& A, const Lds& L, const float* member, int tid, int nt) {
    for (int i = tid; i < A.s; i += nt) {
        L.obs_mean[i] = A.obs_mean ? A.obs_mean[i] : 0.f;
        L.obs_std[i] = A.obs_std ? A.obs_std[i] : 1.f;
        L.goal[i] = A.goal ? A.goal[i] : 0.f;
        L.cw[i] = A.cw ? A.cw[i] : 0.f;
    }
    for (int i = tid; i < A.a; i += nt) {
        L.act_mean[i] = A.act_mean ? A.act_mean[i] : 0.f;
        L.act_std[i] = A.act_std ? A.act_std[i] : 1.f;
    }
    const float* bias_src = member + A.stream_floats;
    for (int i = tid; i < A.L * A.Wpad + 16 * A.NOT; i += nt) L.hbias[i] = bias_src[i];
}

// s0 -> the M normalised layer-0 input rows x[m * lda + d], and zeros in their k0pad_extra columns.
template <int M>
__device__ __forceinline__ void stage_s0(const RolloutArgs& A, const LdsMap& L, float* x, int lda, int tile, int tid,
                                         int nt) {
    for (int i = tid; i < M * A.s; i += nt) {
        const int m = i / A.s, d = i - (i / A.s) * A.s;
        const int n = min(tile * M + m, A.N - 1);
        const float sv = A.s0_per_cand ? A.s0[(size_t)n * A.s + d] : A.s0[d];
        x[m * lda + d] = A.norm_s ? (sv - L.obs_mean[d]) / L.obs_std[d] : sv;
    }
    for (int i = tid; i < M * A.k0pad_extra; i += nt) {
        const int m = i / A.k0pad_extra, j = i - (i / A.k0pad_extra) * A.k0pad_extra;
        x[m * lda + A.s + A.a + j] = 0.f;
    }
}

// Per-lane copies of the step-invariant epilogue operands (this lane's feature slots d = (l&15) +
// 16k), loaded once so the per-step epilogue issues no LDS parameter reads.
template <int SS>
struct EpiParams {
    float om[SS], os[SS], goal[SS], cw[SS], bo[SS];   // state slots
    float am[MAX_A_PER_LANE], as[MAX_A_PER_LANE];    // action slots
};

template <int SS>
__device__ __forceinline__ void load_epi_params(const RolloutArgs& A, const LdsMap& L, int lane, EpiParams<SS>& P) {
    const float* bout = L.hbias + A.L * A.Wpad;
#pragma unroll
    for (int k = 0; k < SS; ++k) {
        const int d = min((lane & 15) + 16 * k, A.s - 1);
        P.om[k] = L.obs_mean[d]; P.os[k] = L.obs_std[d]; P.goal[k] = L.goal[d]; P.cw[k] = L.cw[d]; P.bo[k] = bout[d];
    }
#pragma unroll
    for (int k = 0; k < MAX_A_PER_LANE; ++k) {
        const int d = min((lane & 15) + 16 * k, A.a - 1);
        P.am[k] = L.act_mean[d]; P.as[k] = L.act_std[d];
    }
}

// a_t -> normalised MLP input columns [s, s+a); returns this lane's share of sum_d (cosh(a_d/alpha)-1).
template <int R, int SS, bool REG = (SS <= MBRL_EPI_REG_SLOTS)>
__device__ __forceinline__ void stage_actions(const RolloutArgs& A, const EpiParams<SS>& P, const LdsMap& L, float* act,
                                              int wave, int lane, const float (&av)[R][MAX_A_PER_LANE],
                                              float (&acp)[R], int lda) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int m = epi_row(r, wave, lane);
        float c = 0.f;
#pragma unroll
        for (int k = 0; k < MAX_A_PER_LANE; ++k) {
            const int d = (lane & 15) + 16 * k;
            if (d < A.a) {
                const float x = av[r][k];
                // wide states keep no per-lane copies (see MBRL_EPI_REG_SLOTS): same values from LDS
                const float am = REG ? P.am[k] : L.act_mean[d];
                const float as = REG ? P.as[k] : L.act_std[d];
                const float xn = A.norm_a ? (x - am) / as : x;
                act[m * lda + A.s + d] = xn;
                if (A.reward) L.aterm[m * A.a + d] = xn;   // the state pass re-reads a_t
                if (A.has_ac) c += coshf(x / A.alpha_a) - 1.0f;
            }
        }
        acp[r] = c;
    }
}

// The action waves' per-row CoshLoss sums of stage_actions into acs[parity][M] for the state waves
// (all 16 lanes of a row take part in the DPP sum; lane 0 of the row stores).
template <int R>
__device__ __forceinline__ void publish_action_cost(float* acs, int parity, int M, int awave, int lane,
                                                    const float (&acp)[R]) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const float v = rowsum16(acp[r]);
        if ((lane & 15) == 0) acs[parity * M + epi_row(r, awave, lane)] = v;
    }
}

// The returns of this wave's epilogue rows: lane 0 of each row holds its candidate's total.
template <int R, int M = 16 * R>
__device__ __forceinline__ void write_costs(const RolloutArgs& A, int tile, int e, int wave, int lane,
                                            const float (&total)[R]) {
    if ((lane & 15) == 0) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int n = tile * M + epi_row(r, wave, lane);
            if (n < A.N) A.costs[(size_t)e * A.N + n] = total[r];
        }
    }
}

// Diagnostic build only (make diag, -DMBRL_STAMPS): this wave's segment sums to row (unit, wave) of
// the stamp buffer [units][nwp][NSEG]; the last segment is the 100 MHz clock since rt0.
#ifdef MBRL_STAMPS
constexpr int NSEG = 8;
__device__ __forceinline__ void write_stamps(unsigned long long* buf, unsigned long long (&seg)[NSEG],
                                             unsigned long long rt0, size_t unit, int nwp, int wave, int lane) {
    seg[NSEG - 1] = __builtin_amdgcn_s_memrealtime() - rt0;
    if (lane == 0 && buf != nullptr) {
        unsigned long long* dst = buf + (unit * nwp + wave) * NSEG;
#pragma unroll
        for (int k = 0; k < NSEG; ++k) dst[k] = seg[k];
    }
}
#endif

}  // namespace mbrl
