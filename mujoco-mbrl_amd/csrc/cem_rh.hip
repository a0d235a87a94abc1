// Receding-horizon CEM (include/mbrl_cem.h mbrl_cem_plan_rh; DESIGN.md "Receding-horizon CEM"): the kernels
// around the selection and refit_kernel when rows are kept from one iteration (or plan) to the next --
// the plan's first launch, the gather of the elites' and the best rows' actions, and the next proposals'
// scatter and draw -- with their launchers (mbrl_internal.h). The plan loop is in plan.hip.
//
// Layouts, for B problems planned at once (B = 1: mbrl_cem_plan_rh; B > 1: mbrl_cem_plan_rh_batch): proposals
// `actions` [H][B N][a] time-major (the rollout's; problem b's candidate n is candidate b N + n, its Philox
// index), kept rows [B][Kc][H][a] row-contiguous (what a caller carries from plan to plan), the elites'
// actions [B][H][K][a] (refit_kernel's), mu / sigma [B][H][a], elites [B][K], best [B][Kc], returns [B][N].
// `flags` ([B] or NULL) say which optional inputs apply to a problem (rh_flags). Every kernel
// is a grid-stride loop of one thread per (row, t, d >> 2) -- a Philox block's four dimensions -- ordered
// so that consecutive threads write consecutive addresses of the buffer they fill, with 16-byte loads and
// stores where a is a multiple of 4 and the buffers are 16-byte aligned (VEC). Plain loads and stores
// only: nothing here waits on another workgroup.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mbrl_host.h"
#include "mbrl_rh_rows.h"
#include "mbrl_rng.h"

namespace mbrl {

// The same four dimensions drawn from the counter RNG around (mu_t, sigma_t) (the step's [a] floats each),
// as sample_kernel and gather_elites_kernel draw them.
__device__ __forceinline__ void draw4(uint64_t seed, uint32_t n, uint32_t t, uint32_t it, int g, int a,
                                      const float* __restrict__ mu_t, const float* __restrict__ sigma_t, float lo,
                                      float hi, float v[4]) {
    float z[4];
    cem_normal4(seed, n, t, it, (uint32_t)g, z);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int d = 4 * g + j;
        v[j] = d < a ? cem_action(mu_t[d], sigma_t[d], z[j], lo, hi) : 0.f;
    }
}

template <bool VEC>
__global__ void __launch_bounds__(256) rh_init_kernel(const RhInitArgs A) {
    const size_t gid = blockIdx.x * (size_t)blockDim.x + threadIdx.x, gsz = (size_t)gridDim.x * blockDim.x;
    rh_init_prologue(A, gid, gsz);
    if (!A.actions) return;
    const int a = A.a, B = A.B, N = A.N, G = (a + 3) >> 2;
    const size_t Ha = (size_t)A.H * a;
    const size_t BN = (size_t)B * N, total = (size_t)A.H * BN * G;
    for (size_t i = gid; i < total; i += gsz) {
        const int g = (int)(i % G), t = (int)(i / G / BN);
        const size_t c = (i / G) % BN;   // the candidate's Philox index: problem b's candidate n is b N + n
        const int b = (int)(c / N), n = (int)(c - (size_t)b * N), f = rh_flags(A.flags, b);
        float v[4];
        if (A.carry_in && (f & 4) && n < A.Kc) {
            kept_load4<VEC>(A.carry_in + (((size_t)b * A.Kc + n) * A.H + t) * a, g, a, A.lo, A.hi, v);
        } else {
            float z[4];
            cem_normal4(A.seed, (uint32_t)c, (uint32_t)t, 0u, (uint32_t)g, z);
            const size_t row = (size_t)b * Ha + (size_t)t * a;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int d = 4 * g + j;
                v[j] = d < a ? cem_action(rh_mu0(A, row + d, f), rh_sg0(A, row + d, f), z[j], A.lo, A.hi) : 0.f;
            }
        }
        store4<VEC>(A.actions + ((size_t)t * BN + c) * a, g, a, v);
    }
}

template <bool VEC>
__global__ void __launch_bounds__(256) rh_gather_kernel(const RhGatherArgs A) {
    const size_t gid = blockIdx.x * (size_t)blockDim.x + threadIdx.x, gsz = (size_t)gridDim.x * blockDim.x;
    const int a = A.a, H = A.H, K = A.K, Kc = A.Kc, N = A.N, B = A.B, G = (a + 3) >> 2;
    rh_best_returns(A, gid, gsz);
    // threads [0, B H K G): problem b's elite e's step t in (b, t, e, g) order, aelite's; then [0, B Kc H G):
    // best row j's step t in (b, j, t, g) order, the kept rows'
    const size_t n_el = (size_t)B * H * K * G, total = n_el + (size_t)B * Kc * H * G;
    for (size_t i = gid; i < total; i += gsz) {
        int g, t, n, b;
        float *dst, *dst2 = nullptr;
        if (i < n_el) {
            g = (int)(i % G);
            const int e = (int)((i / G) % K);
            t = (int)((i / G / K) % H);
            b = (int)(i / G / K / H);
            n = (int)A.elites[(size_t)b * K + e];
            dst = A.aelite + (((size_t)b * H + t) * K + e) * a;
        } else {
            const size_t q = i - n_el;
            g = (int)(q % G);
            t = (int)((q / G) % H);
            const int j = (int)((q / G / H) % Kc);
            b = (int)(q / G / H / Kc);
            n = (int)A.best[(size_t)b * Kc + j];
            const size_t o = (((size_t)b * Kc + j) * H + t) * a;
            dst = A.kept_next + o;
            if (A.kept_copy) dst2 = A.kept_copy + o;
        }
        float v[4];
        if (A.from_kept && (rh_flags(A.flags, b) & 4) && (unsigned)n < (unsigned)Kc)
            kept_load4<VEC>(A.kept_cur + (((size_t)b * Kc + n) * H + t) * a, g, a, A.lo, A.hi, v);
        else
            draw4(A.seed, (uint32_t)b * (uint32_t)N + (uint32_t)n, (uint32_t)t, (uint32_t)A.iteration, g, a,
                  A.mu + ((size_t)b * H + t) * a, A.sigma + ((size_t)b * H + t) * a, A.lo, A.hi, v);
        store4<VEC>(dst, g, a, v);
        if (dst2) store4<VEC>(dst2, g, a, v);
    }
}

template <bool VEC>
__global__ void __launch_bounds__(256) rh_draw_kernel(const RhDrawArgs A) {
    const size_t gid = blockIdx.x * (size_t)blockDim.x + threadIdx.x, gsz = (size_t)gridDim.x * blockDim.x;
    const int a = A.a, H = A.H, N = A.N, B = A.B, G = (a + 3) >> 2;
    rh_final_outputs(A, gid, gsz);
    if (!A.actions) return;
    const size_t BN = (size_t)B * N, total = (size_t)H * BN * G;
    for (size_t i = gid; i < total; i += gsz) {
        const int g = (int)(i % G), t = (int)(i / G / BN);
        const size_t c = (i / G) % BN;
        const int b = (int)(c / N), n = (int)(c - (size_t)b * N);
        float v[4];
        if (n < A.Kc)
            kept_load4<VEC>(A.kept + (((size_t)b * A.Kc + n) * H + t) * a, g, a, A.lo, A.hi, v);
        else
            draw4(A.seed, (uint32_t)c, (uint32_t)t, (uint32_t)A.iteration, g, a, A.mu + ((size_t)b * H + t) * a,
                  A.sigma + ((size_t)b * H + t) * a, A.lo, A.hi, v);
        store4<VEC>(A.actions + ((size_t)t * BN + c) * a, g, a, v);
    }
}

// One thread per Philox block, at most 8192 workgroups of 256 (sample_impl's grid).
static dim3 rh_grid(size_t threads) {
    const size_t b = (threads + 255) / 256;
    return dim3((unsigned)(b < 1 ? 1 : (b < 8192 ? b : 8192)));
}

hipError_t launch_rh_init(const RhInitArgs& A, hipStream_t stream) {
    const size_t G = (size_t)(A.a + 3) / 4;
    const size_t threads = (size_t)A.B * (A.actions ? (size_t)A.H * A.N * G : (size_t)A.H * A.a);
    if (rh_init_vec(A)) hipLaunchKernelGGL(rh_init_kernel<true>, rh_grid(threads), dim3(256), 0, stream, A);
    else hipLaunchKernelGGL(rh_init_kernel<false>, rh_grid(threads), dim3(256), 0, stream, A);
    return hipGetLastError();
}

hipError_t launch_rh_gather(const RhGatherArgs& A, hipStream_t stream) {
    const size_t G = (size_t)(A.a + 3) / 4;
    const dim3 grid = rh_grid((size_t)A.B * A.H * ((size_t)A.K + A.Kc) * G);
    if (rh_gather_vec(A)) hipLaunchKernelGGL(rh_gather_kernel<true>, grid, dim3(256), 0, stream, A);
    else hipLaunchKernelGGL(rh_gather_kernel<false>, grid, dim3(256), 0, stream, A);
    return hipGetLastError();
}

hipError_t launch_rh_draw(const RhDrawArgs& A, hipStream_t stream) {
    const size_t G = (size_t)(A.a + 3) / 4;
    const size_t threads = (size_t)A.B * (A.actions ? (size_t)A.H * A.N * G : (size_t)A.H * A.a);
    if (rh_draw_vec(A)) hipLaunchKernelGGL(rh_draw_kernel<true>, rh_grid(threads), dim3(256), 0, stream, A);
    else hipLaunchKernelGGL(rh_draw_kernel<false>, rh_grid(threads), dim3(256), 0, stream, A);
    return hipGetLastError();
}

}  // namespace mbrl
