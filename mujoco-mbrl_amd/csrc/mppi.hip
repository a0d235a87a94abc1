// MPPI update (DESIGN.md "MPPI"): the information-theoretic, softmax-weighted refit of the proposal
// distribution. One launch per iteration after the rollout, in the shape of cem_update_kernel
// (cem.hip): workgroup (t * S + j) of 1024 threads owns row t and draw slice j.
//
//   1. returns r_n = member mean of costs[.][n] (as the selection forms it), beta = min over the finite
//      ones, w_n = expf(-((r_n - beta) / lambda)) for finite r_n, else 0. Every workgroup forms all N
//      weights itself (redundant across rows, off the critical path). Thread c keeps the 32 weights of
//      chunk c = candidates [32 c, 32 c + 32) in registers: N <= 32768 is at most one chunk a thread.
//   2. eta = sum_n w_n and, per action dimension d of row t, sum_n w_n a[t][n][d] (and, with
//      update_sigma, sum_n w_n (a[t][n][d] - m_d)^2 in a second pass over the row) in ONE fixed order,
//      the 32-chunk order applied until one value is left:
//        level 1: the 32 candidates of a chunk, sequentially (31 additions);
//        level 2: the partials of 32 consecutive chunks, sequentially;
//        level 3: the (at most 32) level-2 partials, sequentially.
//      A last, short group sums only its real entries (in the tiles its missing candidates are -0.0
//      rows with weight 0: x + (-0.0) == x). The order depends on N alone, never on the grid, the slice
//      count or the wave layout; the longest dependent chain is D <= 93 additions.
//   3. The row is streamed once per pass through LDS tiles of TCH chunks (coalesced, 16-byte loads where
//      the row allows), in the refit's layout: one spare row after every chunk, so lane (c, d) of the
//      chunk sums reads conflict-free. A tile's weights go from the owning threads' registers to LDS.
//   4. Slice 0 writes mu' = alpha mu + (1 - alpha) m and sigma' (exact_sqrt of the smoothed variance, or
//      sigma unchanged); every slice then draws its share of iteration + 1's proposals from mu', sigma'
//      with update_draw's arithmetic and indexing (bit-identical to mbrl_sample_actions).
// If no return is finite the distribution is left unchanged, bit for bit.
// All arithmetic fp32, correctly rounded, no contraction.
// The same kernel serves B problems in one launch (mbrl_mppi_update_batch, mbrl_mppi_plan_batch): grid
// (H * S, B), each workgroup on one problem's slices of the batch's buffers (mppi_update_kernel<true>).
//
// Elite-restricted form (mbrl_mppi_update_elite, DESIGN.md "MPPI over the K best"): the same kernel over
// MppiEliteArgs. The stable top-K of the returns comes from the selection launch before it (select_impl, one
// segment per problem); every workgroup turns the list into an N-bit membership map in LDS (in the tile
// weights' area, which phase 1 does not use), a candidate outside it counts as invalid -- it stays out of
// beta and its weight is 0, so it takes part in every sum as a zero and the summation order is unchanged --
// and sigma' is clamped to [sigma_min, sigma_max] where update_sigma writes it. MppiArgs instantiations
// compile to the code they had: every addition is under `if constexpr (ELITE)`.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "mbrl_host.h"
#include "mbrl_rng.h"
#include "mbrl_wave.h"

namespace mbrl {

constexpr int MPPI_THREADS = 1024;
constexpr int MPPI_LDS_MAX = 160 * 1024;

// Chunks per LDS tile: a whole level-2 group where [32][33][a] floats fit beside phase 1's area.
__host__ __device__ inline int mppi_tile_chunks(int a) { return a <= 24 ? 32 : (a <= 48 ? 16 : 8); }

// LDS floats: wave minima [16], tile weights [32][33], level-1 partials [32][a], level-2 partials
// [32][a], mean [a4], mu' / sigma' [2][a4], mu / sigma [2][a4]; then one area used in turn by the
// returns (n at n + n / 32), the eta partials ([1024] + [32]) and the action tile ([TCH][33][a]).
__host__ __device__ inline size_t mppi_fixed_floats(int a) {
    const size_t a4 = ((size_t)a + 3) & ~(size_t)3;
    return 16 + 32 * 33 + 64 * (size_t)a + 5 * a4;
}
__host__ __device__ inline size_t mppi_area_floats(int N, int a) {
    const size_t ret = (size_t)N + (size_t)(N + 31) / 32;
    const size_t eta = 1024 + 32;
    const size_t tile = (size_t)mppi_tile_chunks(a) * 33 * a;
    size_t m = ret > eta ? ret : eta;
    m = m > tile ? m : tile;
    return (m + 3) & ~(size_t)3;
}

size_t mppi_update_lds_bytes(int N, int a) { return (mppi_fixed_floats(a) + mppi_area_floats(N, a)) * sizeof(float); }

// Order key of a return: finite values in ascending order (-0.0 taken as +0.0), everything else last.
__device__ __forceinline__ uint32_t mppi_key(float v) {
    uint32_t b = __float_as_uint(v);
    if ((b & 0x7F800000u) == 0x7F800000u) return 0xFFFFFFFFu;
    if (v == 0.0f) b = 0u;
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float mppi_unkey(uint32_t k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

// BATCH: grid (H * S, B), workgroup (t * S + j, b) on problem b of B = gridDim.y. Problem b's costs are columns
// [b N, (b + 1) N) of costs [E][B N], its proposals columns b N + n of actions [H][B N][a] (and of next_actions,
// drawn with Philox index b N + n), its distribution mu / sigma [B][H][a]; weights / returns [B][N], stats
// [B][2]. Every offset below is uniform over the workgroup; the arithmetic is the single kernel's, over the
// problem's own N (chunks counted from its candidate 0). BATCH = false compiles to the single-problem kernel.
// ARGS: MppiArgs, or MppiEliteArgs for the elite-restricted update (elites [K], batched [B][K], local indices).
template <bool BATCH, class ARGS>
__global__ void __launch_bounds__(MPPI_THREADS) mppi_update_kernel(ARGS A) {
#pragma clang fp contract(off)
    constexpr bool ELITE = std::is_same<ARGS, MppiEliteArgs>::value;
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int S = gridDim.x / A.H;                      // draw slices per row
    const int t = blockIdx.x / S, j = blockIdx.x - (blockIdx.x / S) * S;
    const bool lead = blockIdx.x == 0;                  // writes the (problem's) weights, returns and stats
    const int N = A.N, a = A.a, a4 = (a + 3) & ~3, E = A.E;
    const size_t cs = BATCH ? (size_t)gridDim.y * N : (size_t)N;   // member stride of costs, candidates per row
    if (BATCH) {
        const size_t bN = (size_t)blockIdx.y * N, bHa = (size_t)blockIdx.y * A.H * a;
        A.costs += bN; A.actions += bN * a; A.mu += bHa; A.sigma += bHa; A.mu_out += bHa; A.sigma_out += bHa;
        if (A.fin_actions) {
            A.fin_actions += bHa;
            if (A.fin_mu) A.fin_mu += bHa;
            if (A.fin_sigma) A.fin_sigma += bHa;
        }
        if (A.weights_out) A.weights_out += bN;
        if (A.returns_out) A.returns_out += bN;
        if (A.stats_out) A.stats_out += 2 * blockIdx.y;
        if (A.next_actions) A.next_actions += bN * a;
        if constexpr (ELITE) A.elites += (size_t)blockIdx.y * A.K;
    }
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nch = (N + ELITE_CHUNK - 1) / ELITE_CHUNK;
    const int n2 = (nch + ELITE_CHUNK - 1) / ELITE_CHUNK;
    uint32_t* wmin = reinterpret_cast<uint32_t*>(sm);   // [16]
    float* wt = sm + 16;                                 // [32][33] the tile's weights
    float* part1 = wt + 32 * 33;                         // [32][a] level-1 partials of the open group
    float* part2 = part1 + 32 * a;                       // [32][a] level-2 partials
    float* mean = part2 + 32 * a;                        // [a4]
    float* next = mean + a4;                             // [2][a4] mu', sigma' of row t
    float* musg = next + 2 * a4;                         // [2][a4] mu, sigma of row t
    float* area = musg + 2 * a4;
    // ---- the elites' membership map, bit n & 31 of word n >> 5 (nch <= 1024 words, in wt until the tiles);
    // an index outside [0, N) sets nothing
    uint32_t* emap = reinterpret_cast<uint32_t*>(wt);
    if constexpr (ELITE) {
        if (tid < nch) emap[tid] = 0u;
        __syncthreads();
        for (int k = tid; k < A.K; k += MPPI_THREADS) {
            const int64_t n = A.elites[k];
            if ((uint64_t)n < (uint64_t)N) atomicOr(&emap[n >> 5], 1u << (n & 31));
        }
        __syncthreads();
    }

    for (int d = tid; d < a; d += MPPI_THREADS) {
        musg[d] = A.mu[t * a + d];
        musg[a4 + d] = A.sigma[t * a + d];
    }
    // ---- returns (coalesced), their minimum
    uint32_t kmin = 0xFFFFFFFFu;
    for (int n = tid; n < N; n += MPPI_THREADS) {
        float r = A.costs[n];
        if (E > 1) {
            for (int e = 1; e < E; ++e) r = __fadd_rn(r, A.costs[e * cs + n]);
            r = __fdiv_rn(r, (float)E);
        }
        if (lead && A.returns_out) A.returns_out[n] = r;
        area[n + (n >> 5)] = r;
        if (!ELITE || ((emap[n >> 5] >> (n & 31)) & 1u)) kmin = min(kmin, mppi_key(r));
    }
    kmin = wave_min_u32(kmin);
    if (lane == 0) wmin[wave] = kmin;
    __syncthreads();
    uint32_t km = wmin[0];
#pragma unroll
    for (int w = 1; w < MPPI_THREADS / 64; ++w) km = min(km, wmin[w]);
    const bool any = km != 0xFFFFFFFFu;                 // (uniform) some return is finite
    const float beta = mppi_unkey(km);
    // ---- weights: thread c holds chunk c's
    const int c = tid;
    const uint32_t member = ELITE ? (c < nch ? emap[c] : 0u) : 0xFFFFFFFFu;   // chunk c's elites
    float w[ELITE_CHUNK];
#pragma unroll
    for (int q = 0; q < ELITE_CHUNK; ++q) {
        const int n = ELITE_CHUNK * c + q;
        float wq = 0.0f;
        if (n < N && any && ((member >> q) & 1u)) {
            const float r = area[(ELITE_CHUNK + 1) * c + q];
            if ((__float_as_uint(r) & 0x7F800000u) != 0x7F800000u)
                wq = expf(-__fdiv_rn(__fadd_rn(r, -beta), A.temperature));
        }
        w[q] = wq;
    }
    __syncthreads();   // the returns are consumed: their area becomes the eta partials'
    // ---- eta in the canonical order
    float* e1 = area;           // [1024]
    float* e2 = area + 1024;    // [32]
    {
        float s = w[0];
#pragma unroll
        for (int q = 1; q < ELITE_CHUNK; ++q) s = __fadd_rn(s, w[q]);
        e1[c] = s;
    }
    __syncthreads();
    if (tid < n2) {
        const int ng = min(ELITE_CHUNK, nch - ELITE_CHUNK * tid);
        float s = e1[ELITE_CHUNK * tid];
        for (int i = 1; i < ng; ++i) s = __fadd_rn(s, e1[ELITE_CHUNK * tid + i]);
        e2[tid] = s;
    }
    __syncthreads();
    float eta = e2[0];
    for (int g = 1; g < n2; ++g) eta = __fadd_rn(eta, e2[g]);
    if (lead && tid == 0 && A.stats_out) {
        A.stats_out[0] = any ? beta : __uint_as_float(0x7FC00000u);
        A.stats_out[1] = eta;
    }
    __syncthreads();   // eta read: the area becomes the action tiles'

    // ---- the weighted moments of row t
    const bool wr = j == 0;   // slice 0 of the row writes its refit
    auto finish = [&](int d, float m, float v) {
        const float mu0 = musg[d], s0 = musg[a4 + d];
        float mn = mu0, sn = s0;
        if (any) {
            mn = __fadd_rn(__fmul_rn(A.alpha, mu0), __fmul_rn(A.oma, m));
            if (A.update_sigma) {
                sn = exact_sqrt(__fadd_rn(__fmul_rn(A.alpha, __fmul_rn(s0, s0)), __fmul_rn(A.oma, v)));
                if constexpr (ELITE) {   // the clamp (comparisons: [0, +inf] changes no bit, -0.0 included)
                    if (sn < A.sigma_min) sn = A.sigma_min;
                    if (sn > A.sigma_max) sn = A.sigma_max;
                }
            }
        }
        next[d] = mn;
        next[a4 + d] = sn;
        if (wr) {
            A.mu_out[t * a + d] = mn;
            A.sigma_out[t * a + d] = sn;
            if (A.fin_actions) {
                if (A.fin_mu) A.fin_mu[t * a + d] = mn;
                if (A.fin_sigma) A.fin_sigma[t * a + d] = sn;
                A.fin_actions[t * a + d] = fminf(fmaxf(mn, A.lo), A.hi);
            }
        }
    };
    if (!any) {
        if (tid < a) finish(tid, 0.0f, 0.0f);
        if (lead && A.weights_out)
            for (int n = tid; n < N; n += MPPI_THREADS) A.weights_out[n] = 0.0f;
    } else {
        const int TCH = mppi_tile_chunks(a);
        const int ca = ELITE_CHUNK * a;
        const float* row = A.actions + (size_t)t * cs * a;
        float* tile = area;
        const int npass = A.update_sigma ? 2 : 1;
        for (int pass = 0; pass < npass; ++pass) {
            for (int c0 = 0; c0 < nch; c0 += TCH) {
                const int ntc = min(TCH, nch - c0);
                const int nl0 = ELITE_CHUNK * c0, nreal = min(N - nl0, ELITE_CHUNK * ntc);
                const int cnt = nreal * a;
                const float* src = row + (size_t)nl0 * a;
                // flat index f = n a + d of the tile lands at f + (f / ca) a (a spare row per chunk)
                if ((cnt & 3) == 0 && (reinterpret_cast<uintptr_t>(src) & 15) == 0) {
                    typedef float f4 __attribute__((ext_vector_type(4)));
                    const f4* s4 = reinterpret_cast<const f4*>(src);
                    const int n4 = cnt >> 2;
                    for (int i0 = tid; i0 < n4; i0 += 4 * MPPI_THREADS) {
                        f4 v[4];
#pragma unroll
                        for (int u = 0; u < 4; ++u)
                            if (i0 + u * MPPI_THREADS < n4) v[u] = s4[i0 + u * MPPI_THREADS];
#pragma unroll
                        for (int u = 0; u < 4; ++u)
                            if (i0 + u * MPPI_THREADS < n4) {
                                const int f = 4 * (i0 + u * MPPI_THREADS);   // (ca % 4 == 0: one chunk per group)
                                float* dst = tile + f + (f / ca) * a;
#pragma unroll
                                for (int k = 0; k < 4; ++k) dst[k] = v[u][k];
                            }
                    }
                } else {
                    for (int f = tid; f < cnt; f += MPPI_THREADS) tile[f + (f / ca) * a] = src[f];
                }
                // the last chunk's missing candidates: rows of -0.0 (their weights are 0)
                for (int i = tid; i < (ELITE_CHUNK * ntc - nreal) * a; i += MPPI_THREADS) {
                    const int nl = nreal + i / a, d = i - (i / a) * a;
                    tile[(nl + nl / ELITE_CHUNK) * a + d] = -0.0f;
                }
                if (c >= c0 && c < c0 + ntc) {
                    float* dst = wt + (c - c0) * (ELITE_CHUNK + 1);
#pragma unroll
                    for (int q = 0; q < ELITE_CHUNK; ++q) dst[q] = w[q];
                }
                __syncthreads();
                if (lead && pass == 0 && A.weights_out)
                    for (int i = tid; i < nreal; i += MPPI_THREADS)
                        A.weights_out[nl0 + i] = wt[(i >> 5) * (ELITE_CHUNK + 1) + (i & 31)];
                // level 1: lane (cl, d) sums chunk c0 + cl, dimension d
                for (int idx = tid; idx < ntc * a; idx += MPPI_THREADS) {
                    const int cl = idx / a, d = idx - (idx / a) * a;
                    const float* av = tile + cl * (ELITE_CHUNK + 1) * a + d;
                    const float* wv = wt + cl * (ELITE_CHUNK + 1);
                    float v[ELITE_CHUNK];
#pragma unroll
                    for (int q = 0; q < ELITE_CHUNK; ++q) v[q] = av[q * a];
                    if (pass == 1) {
                        const float md = mean[d];
#pragma unroll
                        for (int q = 0; q < ELITE_CHUNK; ++q) {
                            const float df = __fadd_rn(v[q], -md);
                            v[q] = __fmul_rn(df, df);
                        }
                    }
#pragma unroll
                    for (int q = 0; q < ELITE_CHUNK; ++q) v[q] = __fmul_rn(wv[q], v[q]);
                    float acc = v[0];
#pragma unroll
                    for (int q = 1; q < ELITE_CHUNK; ++q) acc = __fadd_rn(acc, v[q]);
                    part1[((c0 + cl) & (ELITE_CHUNK - 1)) * a + d] = acc;
                }
                // level 2 once the group of 32 chunks (or the row) is complete
                const int cend = c0 + ntc;
                if ((cend & (ELITE_CHUNK - 1)) == 0 || cend == nch) {
                    __syncthreads();
                    if (tid < a) {
                        const int g = (cend - 1) / ELITE_CHUNK, ng = cend - ELITE_CHUNK * g;
                        float s = part1[tid];
                        for (int i = 1; i < ng; ++i) s = __fadd_rn(s, part1[i * a + tid]);
                        part2[g * a + tid] = s;
                    }
                }
                __syncthreads();   // the tile, its weights and part1 are free again
            }
            // level 3, the mean or the variance
            if (tid < a) {
                float s = part2[tid];
                for (int g = 1; g < n2; ++g) s = __fadd_rn(s, part2[g * a + tid]);
                const float m = __fdiv_rn(s, eta);
                if (pass == 0) mean[tid] = m;
                if (pass + 1 == npass) finish(tid, mean[tid], m);
            }
            __syncthreads();
        }
    }
    if (!A.next_actions) return;
    __syncthreads();   // next complete
    // ---- row t of the next iteration's proposals for candidate slice j (update_draw, cem.hip)
    const int G = (a + 3) >> 2;
    const int Dn = BATCH ? N : A.draw_n;
    const size_t Dr = BATCH ? cs : (size_t)Dn;          // candidates per row of next_actions
    const uint32_t cbase = BATCH ? blockIdx.y * (uint32_t)N : (uint32_t)A.draw_off;
    const int NS = (Dn + S - 1) / S, n0 = j * NS, n1 = min(Dn, n0 + NS);
    for (int idx = tid; idx < (n1 - n0) * G; idx += MPPI_THREADS) {
        const int n = n0 + idx / G, g = idx - (idx / G) * G;
        float z[4];
        cem_normal4(A.seed, cbase + (uint32_t)n, (uint32_t)t, (uint32_t)(A.iteration + 1), (uint32_t)g, z);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int d = 4 * g + q;
            if (d < a)
                A.next_actions[((size_t)t * Dr + n) * a + d] = cem_action(next[d], next[a4 + d], z[q], A.lo, A.hi);
        }
    }
}

hipError_t launch_mppi_update(const MppiArgs& A, int S, hipStream_t stream) {
    const size_t lds = mppi_update_lds_bytes(A.N, A.a);
    if (A.N < 1 || A.N > MPPI_MAX_N || A.a < 1 || A.a > MPPI_MAX_A || A.H < 1 || S < 1 || lds > (size_t)MPPI_LDS_MAX)
        return hipErrorInvalidValue;
    hipError_t err = ensure_dynamic_lds(reinterpret_cast<const void*>(&mppi_update_kernel<false, MppiArgs>), MPPI_LDS_MAX);
    if (err != hipSuccess) return err;
    hipLaunchKernelGGL((mppi_update_kernel<false, MppiArgs>), dim3(A.H * S), dim3(MPPI_THREADS), lds, stream, A);
    return hipGetLastError();
}

hipError_t launch_mppi_update_batch(const MppiArgs& A, int S, int B, hipStream_t stream) {
    const size_t lds = mppi_update_lds_bytes(A.N, A.a);   // per problem: one workgroup sees one problem
    if (A.N < 1 || A.N > MPPI_MAX_N || A.a < 1 || A.a > MPPI_MAX_A || A.H < 1 || S < 1 || B < 1 || B > MPPI_MAX_B ||
        lds > (size_t)MPPI_LDS_MAX)
        return hipErrorInvalidValue;
    hipError_t err = ensure_dynamic_lds(reinterpret_cast<const void*>(&mppi_update_kernel<true, MppiArgs>), MPPI_LDS_MAX);
    if (err != hipSuccess) return err;
    hipLaunchKernelGGL((mppi_update_kernel<true, MppiArgs>), dim3(A.H * S, B), dim3(MPPI_THREADS), lds, stream, A);
    return hipGetLastError();
}

// The elite-restricted update: B == 0 the single kernel (grid H * S), B >= 1 the batched one (grid (H * S, B)).
// The map needs no LDS of its own (it lives in the tile weights' [32][33] words: nch <= 1024).
hipError_t launch_mppi_update_elite(const MppiEliteArgs& A, int S, int B, hipStream_t stream) {
    const size_t lds = mppi_update_lds_bytes(A.N, A.a);
    if (A.N < 1 || A.N > MPPI_MAX_N || A.a < 1 || A.a > MPPI_MAX_A || A.H < 1 || S < 1 || B < 0 || B > MPPI_MAX_B ||
        lds > (size_t)MPPI_LDS_MAX || !A.elites || A.K < 1 || A.K > A.N)
        return hipErrorInvalidValue;
    if (B == 0) {
        hipError_t err = ensure_dynamic_lds(reinterpret_cast<const void*>(&mppi_update_kernel<false, MppiEliteArgs>),
                                            MPPI_LDS_MAX);
        if (err != hipSuccess) return err;
        hipLaunchKernelGGL((mppi_update_kernel<false, MppiEliteArgs>), dim3(A.H * S), dim3(MPPI_THREADS), lds, stream, A);
    } else {
        hipError_t err = ensure_dynamic_lds(reinterpret_cast<const void*>(&mppi_update_kernel<true, MppiEliteArgs>),
                                            MPPI_LDS_MAX);
        if (err != hipSuccess) return err;
        hipLaunchKernelGGL((mppi_update_kernel<true, MppiEliteArgs>), dim3(A.H * S, B), dim3(MPPI_THREADS), lds, stream, A);
    }
    return hipGetLastError();
}

MppiEliteArgs make_mppi_elite_args(const MppiArgs& U, const int64_t* elites, int K, float sigma_min, float sigma_max) {
    MppiEliteArgs X{};
    static_cast<MppiArgs&>(X) = U;
    X.elites = elites; X.K = K; X.sigma_min = sigma_min; X.sigma_max = sigma_max;
    return X;
}

int mppi_elite_check(int N, int K, float sigma_min, float sigma_max) {
    if (K < 1 || K > N) return fail(MBRL_EINVAL, "mppi: need 1 <= K (%d) <= N (%d)", K, N);
    if (!(sigma_min >= 0.0f) || !(sigma_max >= sigma_min))   // (a NaN fails either comparison)
        return fail(MBRL_EINVAL, "mppi: need 0 <= sigma_min (%g) <= sigma_max (%g)", (double)sigma_min, (double)sigma_max);
    return MBRL_OK;
}

MppiArgs make_mppi_args(const float* costs, int E, int N, int H, int a, const float* actions, const mbrl_sampler& sp,
                        float temperature, float alpha, int update_sigma, float* mu_out, float* sigma_out) {
    MppiArgs U{};
    U.costs = costs; U.E = E; U.N = N; U.H = H; U.a = a; U.actions = actions;
    U.seed = sp.seed; U.iteration = sp.iteration; U.mu = sp.mu; U.sigma = sp.sigma;
    U.lo = sp.lo; U.hi = sp.hi; U.alpha = alpha; U.oma = 1.0f - alpha; U.temperature = temperature;
    U.update_sigma = update_sigma != 0;
    U.mu_out = mu_out; U.sigma_out = sigma_out;
    U.draw_off = 0; U.draw_n = N;
    return U;
}

int mppi_temperature_check(float temperature) {
    if (!(temperature > 0.0f) || temperature > 3.402823466e+38f)
        return fail(MBRL_EINVAL, "mppi: temperature %g must be finite and > 0", (double)temperature);
    return MBRL_OK;
}

int mppi_range_check(int N, int a) {
    if (N > MPPI_MAX_N || a > MPPI_MAX_A)
        return fail(MBRL_EUNSUPPORTED, "mppi: N=%d a=%d exceeds the update kernel (N <= %d, a <= %d)", N, a, MPPI_MAX_N,
                    MPPI_MAX_A);
    return MBRL_OK;
}

int mppi_batch_check(int B, int N) {
    if (B < 1) return fail(MBRL_EINVAL, "mppi: B=%d must be >= 1", B);
    if (B > MPPI_MAX_B) return fail(MBRL_EUNSUPPORTED, "mppi: B=%d exceeds %d", B, MPPI_MAX_B);
    if ((int64_t)B * N > INT32_MAX / 2) return fail(MBRL_EUNSUPPORTED, "mppi: B*N too large");
    return MBRL_OK;
}

}  // namespace mbrl

using namespace mbrl;

extern "C" int mbrl_mppi_update(const float* costs, int32_t E, int32_t N, const float* actions,
                                const mbrl_sampler* sampler, int32_t H, int32_t a, float temperature, float alpha,
                                int32_t update_sigma, float* mu_out, float* sigma_out, float* weights_out,
                                float* returns_out, float* stats_out, float* next_actions, int32_t draw_offset,
                                int32_t draw_count, mbrl_stream_t stream) {
    if (!costs || !actions || !sampler || !sampler->mu || !sampler->sigma || !mu_out || !sigma_out)
        return fail(MBRL_EINVAL, "mppi_update: NULL argument");
    if (N < 1 || E < 1 || H < 1 || a < 1) return fail(MBRL_EINVAL, "mppi_update: need N (%d), E, H, a >= 1", N);
    if (int rc = mppi_temperature_check(temperature)) return rc;
    if (next_actions && (draw_count < 1 || draw_offset < 0 || (int64_t)draw_offset + draw_count > N))
        return fail(MBRL_EINVAL, "mppi_update: draw range [%d, %d + %d) outside [0, %d)", draw_offset, draw_offset,
                    draw_count, N);
    if (next_actions == actions)
        return fail(MBRL_EINVAL, "mppi_update: next_actions must not be the actions buffer (other workgroups still read it)");
    if (int rc = mppi_range_check(N, a)) return rc;
    MppiArgs U = make_mppi_args(costs, E, N, H, a, actions, *sampler, temperature, alpha, update_sigma, mu_out, sigma_out);
    U.weights_out = weights_out; U.returns_out = returns_out; U.stats_out = stats_out;
    if (next_actions) { U.next_actions = next_actions; U.draw_off = draw_offset; U.draw_n = draw_count; }
    const int S = next_actions ? draw_slices(H, 1, draw_count, a) : 1;
    return hip_check(launch_mppi_update(U, S, reinterpret_cast<hipStream_t>(stream)), "mppi update launch");
}

extern "C" int mbrl_mppi_update_batch(const float* costs, int32_t E, int32_t N, int32_t B, const float* actions,
                                      const mbrl_sampler* sampler, int32_t H, int32_t a, float temperature, float alpha,
                                      int32_t update_sigma, float* mu_out, float* sigma_out, float* weights_out,
                                      float* returns_out, float* stats_out, float* next_actions, mbrl_stream_t stream) {
    if (!costs || !actions || !sampler || !sampler->mu || !sampler->sigma || !mu_out || !sigma_out)
        return fail(MBRL_EINVAL, "mppi_update_batch: NULL argument");
    if (N < 1 || E < 1 || H < 1 || a < 1) return fail(MBRL_EINVAL, "mppi_update_batch: need N (%d), E, H, a >= 1", N);
    if (int rc = mppi_temperature_check(temperature)) return rc;
    if (next_actions == actions)
        return fail(MBRL_EINVAL,
                    "mppi_update_batch: next_actions must not be the actions buffer (other workgroups still read it)");
    if (int rc = mppi_range_check(N, a)) return rc;
    if (int rc = mppi_batch_check(B, N)) return rc;
    MppiArgs U = make_mppi_args(costs, E, N, H, a, actions, *sampler, temperature, alpha, update_sigma, mu_out, sigma_out);
    U.weights_out = weights_out; U.returns_out = returns_out; U.stats_out = stats_out;
    U.next_actions = next_actions;
    const int S = next_actions ? draw_slices(H, B, N, a) : 1;
    return hip_check(launch_mppi_update_batch(U, S, B, reinterpret_cast<hipStream_t>(stream)), "mppi batched update launch");
}

// ---- elite-restricted MPPI (include/mbrl_cem.h "MPPI over the K best"): the selection launch, then the update.
// The workspace: the selection's keys first, then the elite list where the caller takes none.
static int mppi_update_elite_run(const float* costs, int E, int N, int K, int B, const float* actions,
                                 const mbrl_sampler* sampler, int H, int a, float temperature, float alpha,
                                 int update_sigma, float sigma_min, float sigma_max, float* mu_out, float* sigma_out,
                                 int64_t* elite_idx_out, float* weights_out, float* returns_out, float* stats_out,
                                 float* next_actions, int draw_offset, int draw_count, void* workspace, size_t ws_bytes,
                                 hipStream_t stream, const char* who) {
    const int nb = B ? B : 1;
    if (!costs || !actions || !sampler || !sampler->mu || !sampler->sigma || !mu_out || !sigma_out || !workspace)
        return fail(MBRL_EINVAL, "%s: NULL argument", who);
    if (N < 1 || E < 1 || H < 1 || a < 1) return fail(MBRL_EINVAL, "%s: need N (%d), E, H, a >= 1", who, N);
    if (int rc = mppi_temperature_check(temperature)) return rc;
    if (int rc = mppi_elite_check(N, K, sigma_min, sigma_max)) return rc;
    if (!B && next_actions && (draw_count < 1 || draw_offset < 0 || (int64_t)draw_offset + draw_count > N))
        return fail(MBRL_EINVAL, "%s: draw range [%d, %d + %d) outside [0, %d)", who, draw_offset, draw_offset,
                    draw_count, N);
    if (next_actions == actions)
        return fail(MBRL_EINVAL, "%s: next_actions must not be the actions buffer (other workgroups still read it)", who);
    if (int rc = mppi_range_check(N, a)) return rc;
    if (B)
        if (int rc = mppi_batch_check(B, N)) return rc;
    const size_t keys = align256((size_t)N * nb * 4);
    const size_t need = keys + (elite_idx_out ? 0 : align256((size_t)nb * K * 8));
    if (ws_bytes < need) return fail(MBRL_EWORKSPACE, "%s: workspace %zu < %zu", who, ws_bytes, need);
    int64_t* elites = elite_idx_out ? elite_idx_out : reinterpret_cast<int64_t*>(static_cast<char*>(workspace) + keys);
    if (int rc = select_impl(costs, E, N, K, MBRL_NAN_LAST, elites, nullptr, workspace, keys, stream, nb)) return rc;
    MppiArgs U = make_mppi_args(costs, E, N, H, a, actions, *sampler, temperature, alpha, update_sigma, mu_out, sigma_out);
    U.weights_out = weights_out; U.returns_out = returns_out; U.stats_out = stats_out;
    U.next_actions = next_actions;
    if (!B && next_actions) { U.draw_off = draw_offset; U.draw_n = draw_count; }
    const int S = next_actions ? (B ? draw_slices(H, B, N, a) : draw_slices(H, 1, draw_count, a)) : 1;
    return hip_check(launch_mppi_update_elite(make_mppi_elite_args(U, elites, K, sigma_min, sigma_max), S, B, stream),
                     "mppi elite update launch");
}

extern "C" int mbrl_mppi_update_elite(const float* costs, int32_t E, int32_t N, int32_t K, const float* actions,
                                      const mbrl_sampler* sampler, int32_t H, int32_t a, float temperature, float alpha,
                                      int32_t update_sigma, float sigma_min, float sigma_max, float* mu_out,
                                      float* sigma_out, int64_t* elite_idx_out, float* weights_out, float* returns_out,
                                      float* stats_out, float* next_actions, int32_t draw_offset, int32_t draw_count,
                                      void* workspace, size_t ws_bytes, mbrl_stream_t stream) {
    return mppi_update_elite_run(costs, E, N, K, 0, actions, sampler, H, a, temperature, alpha, update_sigma, sigma_min,
                                 sigma_max, mu_out, sigma_out, elite_idx_out, weights_out, returns_out, stats_out,
                                 next_actions, draw_offset, draw_count, workspace, ws_bytes,
                                 reinterpret_cast<hipStream_t>(stream), "mppi_update_elite");
}

extern "C" int mbrl_mppi_update_elite_batch(const float* costs, int32_t E, int32_t N, int32_t K, int32_t B,
                                            const float* actions, const mbrl_sampler* sampler, int32_t H, int32_t a,
                                            float temperature, float alpha, int32_t update_sigma, float sigma_min,
                                            float sigma_max, float* mu_out, float* sigma_out, int64_t* elite_idx_out,
                                            float* weights_out, float* returns_out, float* stats_out, float* next_actions,
                                            void* workspace, size_t ws_bytes, mbrl_stream_t stream) {
    if (B < 1) return fail(MBRL_EINVAL, "mppi_update_elite_batch: B=%d must be >= 1", B);
    return mppi_update_elite_run(costs, E, N, K, B, actions, sampler, H, a, temperature, alpha, update_sigma, sigma_min,
                                 sigma_max, mu_out, sigma_out, elite_idx_out, weights_out, returns_out, stats_out,
                                 next_actions, 0, 0, workspace, ws_bytes, reinterpret_cast<hipStream_t>(stream),
                                 "mppi_update_elite_batch");
}
