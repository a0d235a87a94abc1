// What the receding-horizon kernels share (cem_rh.hip, cem_noise.hip). Row access: a Philox block's four
// dimensions of one step of a kept row or of an output row, with 16-byte accesses where a is a multiple of
// 4 and the buffers are 16-byte aligned (VEC; the launchers' rh_*_vec), and the per-problem input flags.
// The grid-stride loops around the proposals that do not depend on the noise: the first launch's prologue
// (rh_init_prologue), the carry's returns (rh_best_returns) and the plan outputs (rh_final_outputs); gid /
// gsz are the calling thread's global index and the grid's thread count.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <initializer_list>

#include "mbrl_internal.h"

namespace mbrl {

inline bool aligned16(std::initializer_list<const void*> ps) {
    for (const void* p : ps)
        if (reinterpret_cast<uintptr_t>(p) & 15) return false;
    return true;
}

// Whether a launch takes its kernel's 16-byte instantiation: every buffer it reads or writes four
// dimensions at a time.
inline bool rh_init_vec(const RhInitArgs& A) { return (A.a & 3) == 0 && aligned16({A.carry_in, A.actions}); }
inline bool rh_gather_vec(const RhGatherArgs& A) {
    return (A.a & 3) == 0 && aligned16({A.kept_cur, A.aelite, A.kept_next, A.kept_copy});
}
inline bool rh_draw_vec(const RhDrawArgs& A) { return (A.a & 3) == 0 && aligned16({A.kept, A.actions}); }

typedef float rh_f4 __attribute__((ext_vector_type(4)));

// clip of a kept entry: a NaN stays NaN (np.minimum(np.maximum(x, lo), hi)), so a poisoned row's return
// is NaN and the row sorts last; fminf / fmaxf alone would turn it into lo.
__device__ __forceinline__ float kept_clip(float x, float lo, float hi) {
    return x != x ? x : fminf(fmaxf(x, lo), hi);
}

// Dimensions 4g .. 4g+3 of a kept row's step (src = the step's [a] floats), clipped.
template <bool VEC>
__device__ __forceinline__ void kept_load4(const float* __restrict__ src, int g, int a, float lo, float hi, float v[4]) {
    if (VEC) {
        const rh_f4 x = *reinterpret_cast<const rh_f4*>(src + 4 * g);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = kept_clip(x[j], lo, hi);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = 4 * g + j < a ? kept_clip(src[4 * g + j], lo, hi) : 0.f;
    }
}

template <bool VEC>
__device__ __forceinline__ void store4(float* __restrict__ dst, int g, int a, const float v[4]) {
    if (VEC) {
        *reinterpret_cast<rh_f4*>(dst + 4 * g) = rh_f4{v[0], v[1], v[2], v[3]};
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (4 * g + j < a) dst[4 * g + j] = v[j];
    }
}

// Which of the optional inputs apply to problem b (bit 0: mu rows, 1: sigma rows, 2: carry_in); no flags:
// every given pointer applies to every problem.
__device__ __forceinline__ int rh_flags(const int32_t* __restrict__ flags, int b) { return flags ? flags[b] : 7; }

// The initial distribution at index i of [B][H][a] for a problem with flags f: what the first launch's draws
// use, whether or not the drawing thread also stores it.
__device__ __forceinline__ float rh_mu0(const RhInitArgs& A, size_t i, int f) {
    return A.mu_rows && (f & 1) ? fminf(fmaxf(A.mu_rows[i], A.lo), A.hi) : A.init_mu;
}
__device__ __forceinline__ float rh_sg0(const RhInitArgs& A, size_t i, int f) {
    return A.sigma_rows && (f & 2) ? A.sigma_rows[i] : A.init_sigma;
}

// The first launch before its proposals: the hand-off words zeroed, problem b's state to each of its s0_rep
// rows (a single plan: the one copy), the mu / sigma rows and kept_0.
__device__ __forceinline__ void rh_init_prologue(const RhInitArgs& A, size_t gid, size_t gsz) {
#pragma unroll
    for (int r = 0; r < 2; ++r)
        for (size_t i = gid; A.zero.ptr[r] && i < A.zero.words[r]; i += gsz) A.zero.ptr[r][i] = 0u;
    if (A.s0_src) {
        const size_t s = (size_t)A.s, rep = (size_t)A.s0_rep;
        for (size_t i = gid; i < (size_t)A.B * rep * s; i += gsz) {
            const size_t row = i / s;
            A.s0_dst[i] = A.s0_src[(row / rep) * s + (i - row * s)];
        }
    }
    const size_t Ha = (size_t)A.H * A.a;
    for (size_t i = gid; i < (size_t)A.B * Ha; i += gsz) {
        const int f = rh_flags(A.flags, (int)(i / Ha));
        A.mu[i] = rh_mu0(A, i, f);
        A.sigma[i] = rh_sg0(A, i, f);
    }
    if (A.kept0) {
        const size_t per = (size_t)A.Kc * Ha;
        for (size_t i = gid; i < (size_t)A.B * per; i += gsz)
            A.kept0[i] = A.carry_in && (rh_flags(A.flags, (int)(i / per)) & 4) ? A.carry_in[i] : 0.f;
    }
}

// The returns of the best rows (the carry's), where the gather is asked for them.
__device__ __forceinline__ void rh_best_returns(const RhGatherArgs& A, size_t gid, size_t gsz) {
    if (!A.best_returns) return;
    for (size_t i = gid; i < (size_t)A.B * A.Kc; i += gsz) {
        const int64_t n = A.best[i];   // (a candidate index; anything else reads nothing)
        A.best_returns[i] = (uint64_t)n < (uint64_t)A.N ? A.returns[(i / A.Kc) * A.N + n] : __uint_as_float(0x7FC00000u);
    }
}

// The plan outputs (mu / sigma copies, clip(mu)), where the draw is asked for them.
__device__ __forceinline__ void rh_final_outputs(const RhDrawArgs& A, size_t gid, size_t gsz) {
    if (!A.fin_actions) return;
    for (size_t i = gid; i < (size_t)A.B * A.H * A.a; i += gsz) {
        const float m = A.mu[i];
        if (A.fin_mu) A.fin_mu[i] = m;
        if (A.fin_sigma) A.fin_sigma[i] = A.sigma[i];
        A.fin_actions[i] = fminf(fmaxf(m, A.lo), A.hi);
    }
}

}  // namespace mbrl
