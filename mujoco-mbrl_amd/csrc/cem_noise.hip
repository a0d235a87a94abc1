// Coloured-noise proposals (include/mbrl_cem.h mbrl_sample_actions_mixed, mbrl_cem_plan_rh_mixed,
// mbrl_cem_plan_rh_batch_mixed; DESIGN.md "Coloured-noise proposals"): the proposal noise of step t is a
// fixed linear mix of the plan's white normals along the horizon,
//     e[t][n][d] = (..((C[t][0] z[0]) + C[t][1] z[1]) + ..) + C[t][H-1] z[H-1],    z[u] = cem_normal4 at (n, u, i, d >> 2),
// every product rounded to fp32 before it is added, the additions sequential in u, round to nearest, no
// contraction. The counter space is the white plan's.
//
// One tile routine (noise_tiles) serves the four kernels -- the plain mixed draw, and the receding-horizon
// plan's first launch, gather and draw (cem_rh.hip's, with the mix) -- so a draw and every regeneration of
// it agree bit for bit. A pair is (one action row, one Philox dimension group g); a workgroup of 256 threads
// owns tiles of P pairs (P = 16, 32 or 64, the launcher's choice):
//   LDS: C [H][H], then z [H][P] as 16-byte entries: 4 H^2 + 16 H P bytes (80 KiB at H = 64, P = 64);
//   stage 1: thread (u, pair) computes cem_normal4 once and writes z[u][pair]: H Philox blocks per pair, as
//            the white draw -- not H per output;
//   stage 2: thread (t, pair) forms the four sums: C[t][u] is one LDS address per P lanes (a broadcast),
//            z[u][pair] consecutive 16-byte entries across lanes; then cem_action and the store.
// A pair whose row is kept skips stage 1 and loads the row in stage 2 (kept_load4). VALU only: the
// summation order is the contract. Plain loads and stores; nothing waits on another workgroup.
// Layouts, flags and the VEC rule are cem_rh.hip's.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mbrl_host.h"
#include "mbrl_rh_rows.h"
#include "mbrl_rng.h"

namespace mbrl {

extern __shared__ __attribute__((aligned(16))) float noise_lds[];

// One pair of a tile: where its row comes from and where its steps go. Step t's four dimensions go to
// dst + t dst_step (and dst2 + t dst_step where given).
struct NoisePair {
    const float* kept;   // the row [H][a] this pair reads instead of drawing, or NULL
    float *dst, *dst2;
    size_t dst_step;
    uint32_t c;          // the candidate's Philox index
    int g, b;            // dimension group, problem
};

// Ops: describe(q, pair) for pair index q < npairs; dist(pair, t, d, mu, sigma), the distribution the
// pair's step t, dimension d is drawn around.
template <bool VEC, class Ops>
__device__ __forceinline__ void noise_tiles(const Ops& ops, const float* __restrict__ mix, uint64_t seed, uint32_t it,
                                            int H, int a, float lo, float hi, size_t npairs, int P) {
    float* Cs = noise_lds;
    rh_f4* zs = reinterpret_cast<rh_f4*>(noise_lds + ((H * H + 3) & ~3));
    for (int i = threadIdx.x; i < H * H; i += 256) Cs[i] = mix[i];
    const int pl = threadIdx.x & (P - 1), r0 = threadIdx.x / P, R = 256 / P;
    const size_t ntiles = (npairs + P - 1) / P;
    for (size_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const size_t q = tile * P + pl;
        const bool on = q < npairs;
        NoisePair p{};
        if (on) ops.describe(q, p);
        if (on && !p.kept)
            for (int u = r0; u < H; u += R) {
                float z[4];
                cem_normal4(seed, p.c, (uint32_t)u, it, (uint32_t)p.g, z);
                zs[u * P + pl] = rh_f4{z[0], z[1], z[2], z[3]};
            }
        __syncthreads();   // (the first one also publishes C)
        if (on)
            for (int t = r0; t < H; t += R) {
                float v[4];
                if (p.kept) {
                    kept_load4<VEC>(p.kept + (size_t)t * a, p.g, a, lo, hi, v);
                } else {
                    const float* Ct = Cs + t * H;
                    float e[4];
                    {
                        const rh_f4 z = zs[pl];
                        const float c = Ct[0];
#pragma unroll
                        for (int j = 0; j < 4; ++j) e[j] = __fmul_rn(c, z[j]);
                    }
                    for (int u = 1; u < H; ++u) {
                        const rh_f4 z = zs[u * P + pl];
                        const float c = Ct[u];
#pragma unroll
                        for (int j = 0; j < 4; ++j) e[j] = __fadd_rn(e[j], __fmul_rn(c, z[j]));
                    }
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int d = 4 * p.g + j;
                        float m = 0.f, s = 0.f;
                        if (d < a) ops.dist(p, t, d, m, s);
                        v[j] = d < a ? cem_action(m, s, e[j], lo, hi) : 0.f;
                    }
                }
                store4<VEC>(p.dst + (size_t)t * p.dst_step, p.g, a, v);
                if (p.dst2) store4<VEC>(p.dst2 + (size_t)t * p.dst_step, p.g, a, v);
            }
        __syncthreads();   // z is free for the next tile
    }
}

// ---- mbrl_sample_actions with the mix: out [H][N][a], candidate n is Philox index n_offset + n.
struct SampleOps {
    const float *mu, *sigma;
    float* out;
    int a, N, G, n_offset;
    __device__ void describe(size_t q, NoisePair& p) const {
        const size_t n = q / G;
        p.g = (int)(q - n * G);
        p.c = (uint32_t)n_offset + (uint32_t)n;
        p.dst = out + n * a;
        p.dst_step = (size_t)N * a;
    }
    __device__ void dist(const NoisePair&, int t, int d, float& m, float& s) const {
        m = mu[(size_t)t * a + d];
        s = sigma[(size_t)t * a + d];
    }
};

template <bool VEC>
__global__ void __launch_bounds__(256) noise_sample_kernel(uint64_t seed, int iteration, const float* __restrict__ mu,
                                                           const float* __restrict__ sigma, float lo, float hi, int H,
                                                           int a, int N, int n_offset, float* __restrict__ out,
                                                           const float* __restrict__ mix, int P) {
    const int G = (a + 3) >> 2;
    const SampleOps ops{mu, sigma, out, a, N, G, n_offset};
    noise_tiles<VEC>(ops, mix, seed, (uint32_t)iteration, H, a, lo, hi, (size_t)N * G, P);
}

// ---- the plan's first launch: rh_init_kernel with iteration 0's proposals coloured.
struct InitOps {
    RhInitArgs A;
    int G;
    __device__ void describe(size_t q, NoisePair& p) const {
        const size_t c = q / G;   // the candidate's Philox index: problem b's candidate n is b N + n
        p.g = (int)(q - c * G);
        p.c = (uint32_t)c;
        p.b = (int)(c / A.N);
        const int n = (int)(c - (size_t)p.b * A.N);
        if (A.carry_in && (rh_flags(A.flags, p.b) & 4) && n < A.Kc)
            p.kept = A.carry_in + ((size_t)p.b * A.Kc + n) * A.H * A.a;
        p.dst = A.actions + c * A.a;
        p.dst_step = (size_t)A.B * A.N * A.a;
    }
    __device__ void dist(const NoisePair& p, int t, int d, float& m, float& s) const {
        const int f = rh_flags(A.flags, p.b);
        const size_t i = ((size_t)p.b * A.H + t) * A.a + d;
        m = rh_mu0(A, i, f);
        s = rh_sg0(A, i, f);
    }
};

template <bool VEC>
__global__ void __launch_bounds__(256) noise_init_kernel(const RhInitArgs A, const float* __restrict__ mix, int P) {
    const size_t gid = blockIdx.x * (size_t)blockDim.x + threadIdx.x, gsz = (size_t)gridDim.x * blockDim.x;
    rh_init_prologue(A, gid, gsz);
    if (!A.actions) return;
    const InitOps ops{A, (A.a + 3) >> 2};
    noise_tiles<VEC>(ops, mix, A.seed, 0u, A.H, A.a, A.lo, A.hi, (size_t)A.B * A.N * ops.G, P);
}

// ---- after the two selections: rh_gather_kernel with the regenerated rows coloured. Pairs [0, B K G): problem
// b's elite e in (b, e, g) order; then [0, B Kc G): its best row j in (b, j, g) order.
struct GatherOps {
    RhGatherArgs A;
    int G;
    __device__ void describe(size_t q, NoisePair& p) const {
        const size_t n_el = (size_t)A.B * A.K * G;
        int n;
        if (q < n_el) {
            const size_t r = q / G;
            p.g = (int)(q - r * G);
            p.b = (int)(r / A.K);
            const int e = (int)(r - (size_t)p.b * A.K);
            n = (int)A.elites[r];
            p.dst = A.aelite + ((size_t)p.b * A.H * A.K + e) * A.a;
            p.dst_step = (size_t)A.K * A.a;
        } else {
            const size_t r = (q - n_el) / G;
            p.g = (int)(q - n_el - r * G);
            p.b = (int)(r / A.Kc);
            n = (int)A.best[r];
            const size_t o = r * A.H * A.a;
            p.dst = A.kept_next + o;
            if (A.kept_copy) p.dst2 = A.kept_copy + o;
            p.dst_step = (size_t)A.a;
        }
        p.c = (uint32_t)p.b * (uint32_t)A.N + (uint32_t)n;
        if (A.from_kept && (rh_flags(A.flags, p.b) & 4) && (unsigned)n < (unsigned)A.Kc)
            p.kept = A.kept_cur + ((size_t)p.b * A.Kc + n) * A.H * A.a;
    }
    __device__ void dist(const NoisePair& p, int t, int d, float& m, float& s) const {
        const size_t i = ((size_t)p.b * A.H + t) * A.a + d;
        m = A.mu[i];
        s = A.sigma[i];
    }
};

template <bool VEC>
__global__ void __launch_bounds__(256) noise_gather_kernel(const RhGatherArgs A, const float* __restrict__ mix, int P) {
    const size_t gid = blockIdx.x * (size_t)blockDim.x + threadIdx.x, gsz = (size_t)gridDim.x * blockDim.x;
    rh_best_returns(A, gid, gsz);
    const GatherOps ops{A, (A.a + 3) >> 2};
    noise_tiles<VEC>(ops, mix, A.seed, (uint32_t)A.iteration, A.H, A.a, A.lo, A.hi,
                     (size_t)A.B * ((size_t)A.K + A.Kc) * ops.G, P);
}

// ---- after the refit: rh_draw_kernel with the drawn slots coloured.
struct DrawOps {
    RhDrawArgs A;
    int G;
    __device__ void describe(size_t q, NoisePair& p) const {
        const size_t c = q / G;
        p.g = (int)(q - c * G);
        p.c = (uint32_t)c;
        p.b = (int)(c / A.N);
        const int n = (int)(c - (size_t)p.b * A.N);
        if (n < A.Kc) p.kept = A.kept + ((size_t)p.b * A.Kc + n) * A.H * A.a;
        p.dst = A.actions + c * A.a;
        p.dst_step = (size_t)A.B * A.N * A.a;
    }
    __device__ void dist(const NoisePair& p, int t, int d, float& m, float& s) const {
        const size_t i = ((size_t)p.b * A.H + t) * A.a + d;
        m = A.mu[i];
        s = A.sigma[i];
    }
};

template <bool VEC>
__global__ void __launch_bounds__(256) noise_draw_kernel(const RhDrawArgs A, const float* __restrict__ mix, int P) {
    const size_t gid = blockIdx.x * (size_t)blockDim.x + threadIdx.x, gsz = (size_t)gridDim.x * blockDim.x;
    rh_final_outputs(A, gid, gsz);
    if (!A.actions) return;
    const DrawOps ops{A, (A.a + 3) >> 2};
    noise_tiles<VEC>(ops, mix, A.seed, (uint32_t)A.iteration, A.H, A.a, A.lo, A.hi, (size_t)A.B * A.N * ops.G, P);
}

// ---- launchers
int noise_check(int H) {
    if (H > NOISE_MAX_H) return fail(MBRL_EUNSUPPORTED, "noise mix: H=%d exceeds %d", H, NOISE_MAX_H);
    return MBRL_OK;
}

// Pairs per tile: the largest of 64, 32, 16 that still gives every CU two workgroups; the grid (one
// workgroup per tile, at most 8192; `floor_threads`: the launch's other grid-stride loops) and the LDS.
struct NoiseLaunch {
    int P;
    dim3 grid;
    size_t lds;
};

static NoiseLaunch noise_launch(size_t npairs, int H, size_t floor_threads) {
    NoiseLaunch L;
    const size_t want = 2 * (size_t)device_cu_count();
    L.P = npairs >= 64 * want ? 64 : (npairs >= 32 * want ? 32 : 16);
    size_t blocks = (npairs + L.P - 1) / L.P;
    const size_t fl = (floor_threads + 255) / 256;
    if (blocks == 0) blocks = fl < 64 ? fl : 64;   // (no pairs: the launch's other loops alone)
    blocks = blocks < 1 ? 1 : (blocks < 8192 ? blocks : 8192);
    L.grid = dim3((unsigned)blocks);
    L.lds = ((size_t)((H * H + 3) & ~3) + (size_t)4 * H * L.P) * sizeof(float);
    return L;
}

template <class T>
struct as_given {
    using type = T;
};

// Launches the 16-byte (vec) or the scalar instantiation of one of the kernels above. Above 64 KiB of dynamic
// LDS the kernel's limit is raised first (H = 64 with 64-pair tiles: 80 KiB).
template <class... KArgs>
static hipError_t launch_noise_kernel(void (*vec_fn)(KArgs...), void (*scalar_fn)(KArgs...), bool vec,
                                      const NoiseLaunch& L, hipStream_t stream, typename as_given<KArgs>::type... args) {
    void (*fn)(KArgs...) = vec ? vec_fn : scalar_fn;
    if (L.lds > 64 * 1024) {
        const hipError_t e = ensure_dynamic_lds(reinterpret_cast<const void*>(fn), 80 * 1024);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(fn, L.grid, dim3(256), L.lds, stream, args...);
    return hipGetLastError();
}

static hipError_t launch_noise_sample(const mbrl_sampler* sp, const float* mix, int H, int a, int N, int n_offset,
                                      float* out, hipStream_t stream) {
    const NoiseLaunch L = noise_launch((size_t)N * ((a + 3) / 4), H, 0);
    const bool vec = (a & 3) == 0 && aligned16({out});
    return launch_noise_kernel(noise_sample_kernel<true>, noise_sample_kernel<false>, vec, L, stream, sp->seed,
                               sp->iteration, sp->mu, sp->sigma, sp->lo, sp->hi, H, a, N, n_offset, out, mix, L.P);
}

int noise_sample_impl(const mbrl_sampler* sp, const float* mix, int H, int a, int N, int n_offset, float* out,
                      hipStream_t stream) {
    if (int rc = noise_check(H)) return rc;
    return hip_check(launch_noise_sample(sp, mix, H, a, N, n_offset, out, stream), "mixed sample launch");
}

hipError_t launch_noise_init(const RhInitArgs& A, const float* mix, hipStream_t stream) {
    const size_t G = (size_t)(A.a + 3) / 4;
    const size_t others = (size_t)A.B * ((size_t)A.H * A.a * (A.kept0 ? 1 + A.Kc : 1) + (A.s0_src ? (size_t)A.s0_rep * A.s : 0));
    const NoiseLaunch L = noise_launch((size_t)A.B * A.N * G, A.H, others);
    return launch_noise_kernel(noise_init_kernel<true>, noise_init_kernel<false>, rh_init_vec(A), L, stream, A, mix, L.P);
}

hipError_t launch_noise_gather(const RhGatherArgs& A, const float* mix, hipStream_t stream) {
    const size_t G = (size_t)(A.a + 3) / 4;
    const NoiseLaunch L = noise_launch((size_t)A.B * ((size_t)A.K + A.Kc) * G, A.H, (size_t)A.B * A.Kc);
    return launch_noise_kernel(noise_gather_kernel<true>, noise_gather_kernel<false>, rh_gather_vec(A), L, stream, A, mix, L.P);
}

hipError_t launch_noise_draw(const RhDrawArgs& A, const float* mix, hipStream_t stream) {
    const size_t G = (size_t)(A.a + 3) / 4;
    const NoiseLaunch L = noise_launch(A.actions ? (size_t)A.B * A.N * G : 0, A.H, (size_t)A.B * A.H * A.a);
    return launch_noise_kernel(noise_draw_kernel<true>, noise_draw_kernel<false>, rh_draw_vec(A), L, stream, A, mix, L.P);
}

}  // namespace mbrl

using namespace mbrl;

extern "C" int mbrl_sample_actions_mixed(const mbrl_sampler* sampler, const float* mix, int32_t H, int32_t a, int32_t N,
                                         int32_t n_offset, float* actions_out, mbrl_stream_t stream) {
    if (!mix) return mbrl_sample_actions(sampler, H, a, N, n_offset, actions_out, stream);
    if (!sampler || !sampler->mu || !sampler->sigma || !actions_out) return fail(MBRL_EINVAL, "sample: NULL argument");
    if (H < 1 || a < 1 || N < 1 || n_offset < 0) return fail(MBRL_EINVAL, "sample: bad sizes");
    return noise_sample_impl(sampler, mix, H, a, N, n_offset, actions_out, reinterpret_cast<hipStream_t>(stream));
}
