// The CEM step's kernels -- elite selection, refit, proposal sampling, the fused per-iteration update,
// the plan's first launch -- with their launchers (mbrl_internal.h) and ABI entries (include/mbrl_cem.h).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <type_traits>

#include "mbrl_host.h"
#include "mbrl_rng.h"
#include "mbrl_wave.h"

namespace mbrl {

// (The wave64 cross-lane helpers -- dpp_u32, wave_inclusive_scan, wave_min_u32 / wave_max_u32,
// wave_ballot, block_exclusive_scan -- and ELITE_CHUNK live in mbrl_wave.h, shared with mppi.hip.)

// ------------------------------------------------------------------------------------------------
// Elite selection: returns -> order keys -> radix select of the K-th key -> stable tie break by
// index -> compaction in ascending index order. One workgroup of 1024 threads (N is small:
// 1e3..3e4 candidates; the pass is a few microseconds).
// ------------------------------------------------------------------------------------------------
// Diagnostic build only (-DMBRL_STAMPS): thread 0's s_memrealtime at fixed points of the select
// kernel, written to a buffer set by mbrl_diag_set_cem_stamps() (tools/select_stamps.py).
#ifdef MBRL_STAMPS
__device__ unsigned long long* g_cem_stamps;
#define CSTAMP(k)                                                                      \
    do {                                                                               \
        if (threadIdx.x == 0 && blockIdx.x == 0 && blockIdx.y == 0 && g_cem_stamps)                \
            g_cem_stamps[k] = __builtin_amdgcn_s_memrealtime();                                       \
    } while (0)
// ... and per workgroup of the split update's two kernels (iteration i, kernel q, workgroup b, point k):
// start, after the selection / the sums, end (mbrl_diag_set_cem_wg_stamps, tools/split_stamps.py).
__device__ unsigned long long* g_cem_wg_stamps;   // [8][2][1024][4]
#define WGSTAMP(q, k)                                                                                     \
    do {                                                                                                  \
        if (threadIdx.x == 0 && blockIdx.x < 1024 && g_cem_wg_stamps)                                     \
            g_cem_wg_stamps[(((U.iteration & 7) * 2 + (q)) * 1024 + blockIdx.x) * 4 + (k)] =              \
                __builtin_amdgcn_s_memrealtime();                                                         \
    } while (0)
#else
#define CSTAMP(k) \
    do {          \
    } while (0)
#define WGSTAMP(q, k) \
    do {              \
    } while (0)
#endif

__device__ __forceinline__ uint32_t order_key(float v, int nan_policy) {
    if (v != v) return nan_policy == MBRL_NAN_LAST ? 0xFFFFFFFFu : 0u;
    if (v == 0.0f) v = 0.0f;  // -0.0 ties with +0.0, as in NumPy's comparisons
    const uint32_t b = __float_as_uint(v);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__global__ void __launch_bounds__(1024) select_kernel(const float* __restrict__ costs, int E, int N, int K,
                                                      int nan_policy, int64_t* __restrict__ elite_idx,
                                                      float* __restrict__ returns_out, uint32_t* __restrict__ keys,
                                                      int member_stride) {
    costs += (size_t)blockIdx.x * N;                   // segment b (see select_reg_kernel)
    elite_idx += (size_t)blockIdx.x * K;
    if (returns_out) returns_out += (size_t)blockIdx.x * N;
    keys += (size_t)blockIdx.x * N;
    __shared__ uint32_t hist[16][257];   // per-wave rows, padded (no cross-wave bank collisions)
    __shared__ uint32_t scan_ws[16];
    __shared__ uint32_t sel[3];  // prefix, bucket, remaining k
    const int tid = threadIdx.x, nt = blockDim.x, wave = tid >> 6;
    for (int n = tid; n < N; n += nt) {
        float r = costs[n];
        if (E > 1) {
            for (int e = 1; e < E; ++e) r = __fadd_rn(r, costs[(size_t)e * member_stride + n]);
            r = __fdiv_rn(r, (float)E);
        }
        if (returns_out) returns_out[n] = r;
        keys[n] = order_key(r, nan_policy);
    }
    uint32_t prefix = 0, mask = 0, kk = (uint32_t)K;
    __syncthreads();
    for (int shift = 24; shift >= 0; shift -= 8) {
        for (int i = tid; i < 16 * 257; i += nt) (&hist[0][0])[i] = 0;
        __syncthreads();
        for (int n0 = 0; n0 < N; n0 += nt) {        // wave-uniform trip count (ballots below)
            const int n = n0 + tid;
            const uint32_t k = n < N ? keys[n] : 0u;
            const bool pending = n < N && (k & mask) == prefix;
            const uint32_t dig = (k >> shift) & 255u;
            const uint64_t act = __ballot(pending);
            if (act != 0) {
                const int leader = __builtin_ctzll(act);
                const uint32_t d0 = __shfl(dig, leader, 64);
                if (__ballot(pending && dig == d0) == act) {   // clustered: one add per wave
                    if ((tid & 63) == leader) atomicAdd(&hist[wave][d0], (uint32_t)__popcll(act));
                } else if (pending) {
                    atomicAdd(&hist[wave][dig], 1u);
                }
            }
        }
        __syncthreads();
        uint32_t tot;
        uint32_t h = 0;
        if (tid < 256)
            for (int w = 0; w < nt / 64; ++w) h += hist[w][tid];
        const uint32_t before = block_exclusive_scan(h, scan_ws, &tot);
        if (tid < 256 && before < kk && before + h >= kk) { sel[0] = (uint32_t)tid; sel[1] = before; }
        __syncthreads();
        prefix |= sel[0] << shift;
        mask |= 0xFFu << shift;
        kk -= sel[1];
        __syncthreads();
    }
    // prefix = K-th smallest key; kk = how many of the keys equal to it are elites (lowest index first)
    const int seg = (N + nt - 1) / nt;
    const int n0 = tid * seg, n1 = min(N, n0 + seg);
    uint32_t eq = 0;
    for (int n = n0; n < n1; ++n) eq += keys[n] == prefix;
    uint32_t tot;
    uint32_t eq_before = block_exclusive_scan(eq, scan_ws, &tot);
    uint32_t cnt = 0;
    for (int n = n0; n < n1; ++n) {
        const uint32_t k = keys[n];
        if (k < prefix) ++cnt;
        else if (k == prefix) { if (eq_before < kk) ++cnt; ++eq_before; }
    }
    eq_before -= eq;
    uint32_t pos = block_exclusive_scan(cnt, scan_ws, &tot);
    for (int n = n0; n < n1; ++n) {
        const uint32_t k = keys[n];
        bool take = false;
        if (k < prefix) take = true;
        else if (k == prefix) { take = eq_before < kk; ++eq_before; }
        if (take && pos < (uint32_t)K) elite_idx[pos++] = n;
    }
}

// Register-resident selection for N <= 1024 * KPT. Wave w owns candidates [64 KPT w, 64 KPT (w + 1)) and
// every load is coalesced: with 16-byte aligned rows (N and member_stride multiples of 4) lane l holds
// groups of four, group g at 64 KPT w + 256 g + 4 l (one float4 per lane, a contiguous KB per wave load
// instruction), else single keys at 64 KPT w + 64 g + l. A thread's keys are therefore not contiguous;
// the elites' ascending-index positions come from ballots over the lanes (in order) and the waves'
// totals (one barrier), so no key moves between threads.
// Passes: one wide pass over the first SEL_WIDE_BITS bits in which the keys differ (one shared
// histogram), the K-th key's bucket listed in LDS, 8-bit passes over that list (or over every key when
// the bucket is too large to list), then the compaction.
constexpr int SEL_HIST_WORDS = 2 * 16 * 257;   // two buffers of per-wave 8-bit digit histograms
constexpr int SEL_WIDE_BITS = 11, SEL_WIDE_BINS = 1 << SEL_WIDE_BITS;   // the first (wide) pass
constexpr int SEL_LIST = 2048;                  // keys of the wide pass's bucket kept in LDS
// LDS words of the register-resident selection: the histograms, the wide histogram, the list, its count
__host__ __device__ constexpr int sel_words(int) { return SEL_HIST_WORDS + SEL_WIDE_BINS + SEL_LIST + 4; }

// Segmented over blockIdx.x (independent problems of N candidates each, batched planning): segment
// b reads costs[e * member_stride + b * N + n] and writes elite_idx[b * K ..] (local indices) and
// returns_out[b * N ..].
// The body is shared with cem_update_kernel; emit(pos, n) receives each elite with its place in
// ascending candidate order.
template <int KPT, typename Emit>
__device__ __forceinline__ void select_reg_body(const float* __restrict__ costs, int E, int N, int K, int nan_policy,
                                                float* __restrict__ returns_out, int member_stride,
                                                uint32_t* sel_smem, Emit emit) {
    typedef float f4 __attribute__((ext_vector_type(4)));
    uint32_t(*hist)[16][257] = reinterpret_cast<uint32_t(*)[16][257]>(sel_smem);  // [2][16][257]
    __shared__ uint32_t scan_ws[16];
    __shared__ uint32_t sel[3];   // bucket, keys before it, keys in it
    CSTAMP(0);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const bool vec = KPT >= 4 && (N & 3) == 0 && (member_stride & 3) == 0;
    const int lv = 64 * KPT * wave + 4 * lane, ls = 64 * KPT * wave + lane;
    // candidate of this lane's key j (ascending in (wave, j / VW, lane, j % VW): the global order)
    auto idx = [&](int j) { return vec ? lv + 256 * (j >> 2) + (j & 3) : ls + 64 * j; };
    // idx rises with j, so this lane's keys below N are its first nv (one register, not KPT predicates)
    const int nv = vec ? 4 * max(0, min(KPT / 4, (N - lv + 255) / 256)) : max(0, min(KPT, (N - ls + 63) / 64));
    uint32_t key[KPT];
    if (vec && E == 1) {
        // (the plans' usual case) branch-free: every lane loads from a valid address -- its own group,
        // or the row's first where it has none -- and the keys past N are set to all ones by a select
        constexpr int G4 = KPT >= 4 ? KPT / 4 : 1;
        f4 v[G4];
#pragma unroll
        for (int g = 0; g < G4; ++g) v[g] = *reinterpret_cast<const f4*>(costs + (lv + 256 * g < N ? lv + 256 * g : 0));
        if (returns_out) {
#pragma unroll
            for (int g = 0; g < G4; ++g)
                if (lv + 256 * g < N) *reinterpret_cast<f4*>(returns_out + lv + 256 * g) = v[g];
        }
#pragma unroll
        for (int g = 0; g < G4; ++g)
#pragma unroll
            for (int i = 0; i < 4; ++i) key[4 * g + i] = 4 * g < nv ? order_key(v[g][i], nan_policy) : 0xFFFFFFFFu;
    } else {
        float r[KPT];   // every load in flight before the first use; the member sum keeps its order
        if (vec) {
            constexpr int G4 = KPT >= 4 ? KPT / 4 : 1;
#pragma unroll
            for (int g = 0; g < G4; ++g) {
                const int n = lv + 256 * g;
                const f4 v = n < N ? *reinterpret_cast<const f4*>(costs + n) : f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int i = 0; i < 4; ++i) r[4 * g + i] = v[i];
            }
            for (int e = 1; e < E; ++e)
#pragma unroll
                for (int g = 0; g < G4; ++g) {
                    const int n = lv + 256 * g;
                    if (n < N) {
                        const f4 c = *reinterpret_cast<const f4*>(costs + (size_t)e * member_stride + n);
#pragma unroll
                        for (int i = 0; i < 4; ++i) r[4 * g + i] = __fadd_rn(r[4 * g + i], c[i]);
                    }
                }
#pragma unroll
            for (int g = 0; g < G4; ++g) {
                const int n = lv + 256 * g;
                f4 v;
#pragma unroll
                for (int i = 0; i < 4; ++i) v[i] = E > 1 ? __fdiv_rn(r[4 * g + i], (float)E) : r[4 * g + i];
                if (returns_out && n < N) *reinterpret_cast<f4*>(returns_out + n) = v;
#pragma unroll
                for (int i = 0; i < 4; ++i) key[4 * g + i] = n < N ? order_key(v[i], nan_policy) : 0xFFFFFFFFu;
            }
        } else {
#pragma unroll
            for (int j = 0; j < KPT; ++j) {
                const int n = ls + 64 * j;
                r[j] = n < N ? costs[n] : 0.f;
            }
            for (int e = 1; e < E; ++e)
#pragma unroll
                for (int j = 0; j < KPT; ++j) {
                    const int n = ls + 64 * j;
                    if (n < N) r[j] = __fadd_rn(r[j], costs[(size_t)e * member_stride + n]);
                }
#pragma unroll
            for (int j = 0; j < KPT; ++j) {
                const int n = ls + 64 * j;
                const float v = E > 1 ? __fdiv_rn(r[j], (float)E) : r[j];
                if (returns_out && n < N) returns_out[n] = v;
                key[j] = n < N ? order_key(v, nan_policy) : 0xFFFFFFFFu;
            }
        }
    }
    // leading bits every key shares (block min / max): returns of one plan usually share sign and
    // exponent, so the first digit starts at the first bit in which the keys differ
    // every key of the wave below N (idx rises with the lane): the passes below skip the per-key test
    const bool wfull = __builtin_amdgcn_readlane(nv, 63) == KPT;
    uint32_t kmin = 0xFFFFFFFFu, kmax = 0u;
    if (wfull) {
#pragma unroll
        for (int j = 0; j < KPT; ++j) { kmin = min(kmin, key[j]); kmax = max(kmax, key[j]); }
    } else {
#pragma unroll
        for (int j = 0; j < KPT; ++j)
            if (j < nv) { kmin = min(kmin, key[j]); kmax = max(kmax, key[j]); }
    }
    kmin = wave_min_u32(kmin);
    kmax = wave_max_u32(kmax);
    __shared__ uint32_t mm_ws[2][16];
    if (lane == 0) { mm_ws[0][wave] = kmin; mm_ws[1][wave] = kmax; }
    uint32_t* wide = sel_smem + SEL_HIST_WORDS;          // [SEL_WIDE_BINS] the first pass's histogram
    uint32_t* list = wide + SEL_WIDE_BINS;               // [SEL_LIST] its bucket's keys, then
    uint32_t* list_n = list + SEL_LIST;                  // their count
    for (int i = tid; i < SEL_WIDE_BINS; i += 1024) wide[i] = 0;
    for (int i = tid; i < 16 * 257; i += 1024) (&hist[0][0][0])[i] = 0;
    if (tid == 0) *list_n = 0;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < 16; ++w) { kmin = min(kmin, mm_ws[0][w]); kmax = max(kmax, mm_ws[1][w]); }
    // keys relative to the smallest (order kept: every key is >= kmin, no wrap): the passes then
    // resolve the bits of (key - kmin), so the wide pass's 2048 bins span [kmin, kmax] whatever bit
    // boundaries the range straddles (plan returns of one binade sit in a few % of its mantissa range:
    // with bins over the bits below the shared ones, walker's K-th bucket held 200-500 keys, now ~10)
#pragma unroll
    for (int j = 0; j < KPT; ++j) key[j] -= kmin;
    const uint32_t kpad = 0xFFFFFFFFu - kmin;            // keys past N (all ones before the shift)
    const uint32_t range = kmax - kmin;
    const int lead = range == 0 ? 32 : __clz(range);     // leading bits every shifted key shares (zero)
    uint32_t mask = lead == 0 ? 0u : (lead >= 32 ? 0xFFFFFFFFu : ~(0xFFFFFFFFu >> lead));
    uint32_t prefix = 0u, kk = (uint32_t)K;
    uint32_t eqn = (uint32_t)N;                          // keys equal to prefix once it is resolved
    int rem = 32 - lead;                                 // bits below the shared ones still to resolve
    CSTAMP(1);
    // (1) one wide pass over the first SEL_WIDE_BITS differing bits: 2048 bins, one shared histogram
    // (plan returns spread over most of them, so the K-th key's bucket holds a handful of keys)
    bool listed = false;
    if (rem > 0) {
        const int wb = min(SEL_WIDE_BITS, rem), wshift = rem - wb;
        const uint32_t wmask = (1u << wb) - 1u;
        auto wide_count = [&](auto check) {   // (keys past N into a dummy bin: no branch per key)
#pragma unroll
            for (int j = 0; j < KPT; ++j)
                atomicAdd(&wide[(!decltype(check)::value || j < nv) ? (key[j] >> wshift) & wmask
                                                                   : SEL_WIDE_BINS + SEL_LIST + 1], 1u);
        };
        if (wfull) wide_count(std::false_type{});
        else wide_count(std::true_type{});
        __syncthreads();
        const uint32_t h0 = wide[2 * tid], h1 = wide[2 * tid + 1];
        uint32_t tot;
        const uint32_t b0 = block_exclusive_scan(h0 + h1, scan_ws, &tot);
        if (b0 < kk && b0 + h0 >= kk) { sel[0] = 2u * tid; sel[1] = b0; sel[2] = h0; }
        else if (b0 + h0 < kk && b0 + h0 + h1 >= kk) { sel[0] = 2u * tid + 1u; sel[1] = b0 + h0; sel[2] = h1; }
        __syncthreads();
        prefix |= sel[0] << wshift;
        mask |= wmask << wshift;
        kk -= sel[1];
        const uint32_t bsz = sel[2];   // (a register: wave 0 rewrites sel below)
        eqn = bsz;
        rem = wshift;
        CSTAMP(2);
        // (2) the bucket's keys (sel[2] of them) into an LDS list: the later passes read it, not the
        // KPT keys of every thread
        if (rem > 0 && bsz <= (uint32_t)SEL_LIST) {
            auto list_keys = [&](auto check) {
#pragma unroll
                for (int j = 0; j < KPT; ++j) {
                    const bool pend = (!decltype(check)::value || j < nv) && (key[j] & mask) == prefix;
                    const uint64_t act = wave_ballot(pend);
                    if (act != 0) {
                        const int leader = __builtin_ctzll(act);
                        uint32_t base = 0;
                        if (lane == leader) base = atomicAdd(list_n, (uint32_t)__popcll(act));
                        base = (uint32_t)__builtin_amdgcn_readlane((int)base, leader);
                        const uint32_t below = __builtin_amdgcn_mbcnt_hi(
                            (uint32_t)(act >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)act, 0u));
                        if (pend) list[base + below] = key[j];
                    }
                }
            };
            if (wfull) list_keys(std::false_type{});
            else list_keys(std::true_type{});
            listed = true;
            __syncthreads();
            // a bucket of at most 64 keys (the usual case): wave 0 ranks them directly -- the kk-th
            // smallest is the key with (keys below it) < kk <= (keys not above it) -- in place of the
            // remaining 8-bit passes and their barriers
            if (bsz <= 64u) {
                const uint32_t nb = (uint32_t)__builtin_amdgcn_readfirstlane((int)bsz);
                if (wave == 0) {
                    const uint32_t x = (uint32_t)lane < nb ? list[lane] : 0xFFFFFFFFu;
                    uint32_t lt = 0, le = 0;
                    for (uint32_t j = 0; j < nb; ++j) {   // key j to every lane (readlane: no LDS trip)
                        const uint32_t y = (uint32_t)__builtin_amdgcn_readlane((int)x, (int)j);
                        lt += y < x;
                        le += y <= x;
                    }
                    if ((uint32_t)lane < nb && lt < kk && le >= kk) { sel[0] = x; sel[1] = kk - lt; sel[2] = le - lt; }
                }
                __syncthreads();
                prefix = sel[0];
                kk = sel[1];
                eqn = sel[2];
                mask = 0xFFFFFFFFu;
                rem = 0;
            }
        }
        CSTAMP(3);
    }
    // (3) 8-bit radix passes over the remaining bits: over the list (a few keys, at most SEL_LIST / 1024
    // per thread), or over every thread's KPT keys when the bucket was too large to list. Per-wave
    // histograms (rows padded to 257: no cross-wave bank collisions on a shared digit); the buffer of pass
    // p+1 is cleared during pass p; the bucket search is a 256-entry scan by waves 0-3.
    const uint32_t nl = listed ? *list_n : 0u;
    int buf = 0;
    while (rem > 0) {
        const int db = min(8, rem), shift = rem - db;
        const uint32_t dmask = (1u << db) - 1u;
        auto count = [&](uint32_t kv, bool valid) {
            const bool pending = valid && (kv & mask) == prefix;
            const uint32_t dig = (kv >> shift) & dmask;
            const uint64_t act = wave_ballot(pending);
            if (act != 0) {
                const int leader = __builtin_ctzll(act);
                const uint32_t d0 = __shfl(dig, leader, 64);
                if (wave_ballot(pending && dig == d0) == act) {   // clustered: one add per wave
                    if (lane == leader) atomicAdd(&hist[buf][wave][d0], (uint32_t)__popcll(act));
                } else if (pending) {
                    atomicAdd(&hist[buf][wave][dig], 1u);
                }
            }
        };
        if (listed) {
            for (uint32_t i0 = 0; i0 < nl; i0 += 1024)   // block-uniform trip count
                count(i0 + tid < nl ? list[i0 + tid] : 0u, i0 + tid < nl);
        } else {
#pragma unroll
            for (int j = 0; j < KPT; ++j) count(key[j], j < nv);
        }
        for (int i = tid; i < 16 * 257; i += 1024) (&hist[buf ^ 1][0][0])[i] = 0;
        __syncthreads();
        uint32_t h = 0, incl = 0;
        if (tid < 256) {
#pragma unroll
            for (int w = 0; w < 16; ++w) h += hist[buf][w][tid];
            incl = wave_inclusive_scan(h);
            if (lane == 63) scan_ws[wave] = incl;
        }
        __syncthreads();
        if (tid < 256) {
            uint32_t before = incl - h;
            for (int w = 0; w < wave; ++w) before += scan_ws[w];
            if (before < kk && before + h >= kk) { sel[0] = (uint32_t)tid; sel[1] = before; sel[2] = h; }
        }
        __syncthreads();
        prefix |= sel[0] << shift;
        mask |= dmask << shift;
        kk -= sel[1];
        eqn = sel[2];
        rem = shift;
        buf ^= 1;
    }
    CSTAMP(4);
    // prefix = the K-th smallest key; the elites are every key below it and the first kk keys equal to
    // it in candidate order.
    // (a) Every key equal to it is an elite (eqn == kk: the K-th key unique, or all its ties taken --
    // the usual case): the elites are the keys <= prefix. Their flags go to an LDS bitmap in candidate
    // order (a lane's four adjacent keys are a nibble, eight lanes' nibbles one word, OR-ed by DPP;
    // or one ballot per key, two words, in the single-key layout), and thread t emits the set bits of
    // word t after a block scan of the words' counts: ~3 VALU ops per key instead of ~20.
    // Keys past N are kpad, the largest shifted key; prefix is not (checked), so they are never flagged.
    // (From KPT = 8: at 4 keys per lane and fewer the scan and barrier of (a) cost more than (b)'s
    // per-key work -- 1.35 against 0.76 us at N = 4096.)
    if (KPT >= 8 && eqn == kk && prefix != kpad) {
        uint32_t* bits = &hist[0][0][0];   // [32 KPT] (the 8-bit passes are done with it)
        auto ballot_words = [&]() {
#pragma unroll
            for (int j = 0; j < KPT; ++j) {
                const uint64_t m = wave_ballot(key[j] <= prefix);
                if (lane < 2) bits[((ls - lane + 64 * j) >> 5) + lane] = (uint32_t)(m >> (32 * lane));
            }
        };
        if constexpr (KPT >= 4) {
            if (vec) {
#pragma unroll
                for (int g = 0; g < KPT / 4; ++g) {
                    uint32_t nib = 0;
#pragma unroll
                    for (int i = 0; i < 4; ++i) nib |= (uint32_t)(key[4 * g + i] <= prefix) << i;
                    nib <<= 4 * (lane & 7);
                    nib |= dpp_u32<0xB1>(nib);    // quad_perm [1,0,3,2]
                    nib |= dpp_u32<0x4E>(nib);    // quad_perm [2,3,0,1]
                    nib |= dpp_u32<0x141>(nib);   // row_half_mirror: the other quad of the eight
                    if ((lane & 7) == 0) bits[(lv + 256 * g) >> 5] = nib;
                }
            } else {
                ballot_words();
            }
        } else {
            ballot_words();
        }
        __syncthreads();
        uint32_t m = tid < (N + 31) >> 5 ? bits[tid] : 0u, tot;
        uint32_t pos = block_exclusive_scan((uint32_t)__popc(m), scan_ws, &tot);
        while (m != 0u) {
            emit(pos++, 32 * tid + __builtin_ctz(m));
            m &= m - 1u;
        }
        CSTAMP(5);
        return;
    }
    // (b) Otherwise an elite's place in that order is (keys below it before it) + min(equal
    // keys before it, kk) -- below K by construction. Keys past N are kpad and follow every real key
    // in the order, so they can only tie with a K-th key of kpad after the kk real ones: no validity
    // test is needed here. Counts are packed (below << 16 | equal; N <= 32768, so neither half carries)
    // and kept in VALU registers; one conditional store per key is the only branch (the scalar unit,
    // shared by the CU's 16 waves, was the bottleneck of a ballot-per-key compaction).
    auto below = [&](uint64_t b) {   // set bits of b in lanes before this one
        return __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
    };
    auto cnt2 = [&](uint32_t k) { return ((uint32_t)(k < prefix) << 16) | (uint32_t)(k == prefix); };
    constexpr int VW = KPT >= 4 ? 4 : 1;   // keys of one lane that are adjacent in the order
    const int vw = vec ? VW : 1;
    {
        uint32_t c = 0;
#pragma unroll
        for (int j = 0; j < KPT; ++j) c += cnt2(key[j]);
        c = wave_inclusive_scan(c);
        if (lane == 63) scan_ws[wave] = c;   // this wave's keys below / equal to the prefix, packed
    }
    __syncthreads();
    uint32_t run = 0;   // packed counts of the keys before this wave's current group (wave-uniform)
    for (int w = 0; w < wave; ++w) run += scan_ws[w];
#pragma unroll
    for (int g = 0; g < KPT / VW; ++g) {
        // the group's keys in candidate order: lanes ascending, and inside a lane its vw keys (one
        // group of VW keys per lane), or VW groups of single keys (vw = 1)
        if (vw == VW) {
            // counts of the group's keys in lanes before this one: ballots and mbcnt (VALU only)
            uint64_t bl[VW], be[VW], beany = 0;
            uint32_t before = 0, tot = 0;
#pragma unroll
            for (int i = 0; i < VW; ++i) {
                bl[i] = wave_ballot(key[VW * g + i] < prefix);
                be[i] = wave_ballot(key[VW * g + i] == prefix);
                beany |= be[i];
                before += below(bl[i]) << 16;
                tot += (uint32_t)__popcll(bl[i]) << 16;
            }
            if (beany != 0) {   // (rare: keys equal to the K-th in this group)
#pragma unroll
                for (int i = 0; i < VW; ++i) {
                    before += below(be[i]);
                    tot += (uint32_t)__popcll(be[i]);
                }
            }
            uint32_t at = run + before;
#pragma unroll
            for (int i = 0; i < VW; ++i) {
                const uint32_t k = key[VW * g + i];
                const uint32_t lb = at >> 16, eb = at & 0xFFFFu;
                const bool lt = k < prefix, eq = k == prefix;
                const bool take = lt || (eq && eb < kk);
                const uint32_t pos = lb + (lt ? min(eb, kk) : eb);
                if (take) emit(pos, idx(VW * g + i));
                at += cnt2(k);
            }
            run += tot;
        } else {
#pragma unroll
            for (int i = 0; i < VW; ++i) {
                const uint32_t k = key[VW * g + i];
                const bool lt = k < prefix, eq = k == prefix;
                const uint64_t bl = wave_ballot(lt), be = wave_ballot(eq);
                const uint32_t lb = (run >> 16) + below(bl), eb = (run & 0xFFFFu) + below(be);
                const bool take = lt || (eq && eb < kk);
                const uint32_t pos = lb + (lt ? min(eb, kk) : eb);
                if (take) emit(pos, idx(VW * g + i));
                run += ((uint32_t)__popcll(bl) << 16) + (uint32_t)__popcll(be);
            }
        }
    }
    CSTAMP(5);
}

template <int KPT>
__global__ void __launch_bounds__(1024) select_reg_kernel(const float* __restrict__ costs, int E, int N, int K,
                                                          int nan_policy, int64_t* __restrict__ elite_idx,
                                                          float* __restrict__ returns_out, int member_stride) {
    extern __shared__ __attribute__((aligned(16))) uint32_t sel_smem[];
    costs += (size_t)blockIdx.x * N;
    elite_idx += (size_t)blockIdx.x * K;
    if (returns_out) returns_out += (size_t)blockIdx.x * N;
    select_reg_body<KPT>(costs, E, N, K, nan_policy, returns_out, member_stride, sel_smem,
                         [&](uint32_t pos, int n) { elite_idx[pos] = n; });
}

static size_t select_reg_lds(int KPT) { return 4 * (size_t)sel_words(KPT); }

// ------------------------------------------------------------------------------------------------
// CEM refit. gather: regenerate every elite's a_t from the counter RNG into aelite[t][e][a].
// refit: canonical chunked sums (ELITE_CHUNK = 32, oracle/cem.py:chunked_sum) -> mean, population
// variance -> alpha-smoothed mu / sigma. All float ops correctly rounded, no contraction.
// ------------------------------------------------------------------------------------------------

__global__ void gather_elites_kernel(uint64_t seed, int iteration, const float* __restrict__ mu,
                                     const float* __restrict__ sigma, float lo, float hi, int a,
                                     const int64_t* __restrict__ elite_idx, int K, float* __restrict__ aelite) {
    const int t = blockIdx.y;
    const int G = (a + 3) >> 2;
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= K * G) return;
    const int e = idx / G, g = idx - (idx / G) * G;
    float z[4];
    cem_normal4(seed, (uint32_t)elite_idx[e], (uint32_t)t, (uint32_t)iteration, (uint32_t)g, z);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int d = 4 * g + j;
        if (d < a) aelite[((size_t)t * K + e) * a + d] = cem_action(mu[t * a + d], sigma[t * a + d], z[j], lo, hi);
    }
}

__global__ void refit_kernel(const float* __restrict__ aelite, int a, int K, float alpha, float oma,
                             const float* __restrict__ mu, const float* __restrict__ sigma,
                             float* __restrict__ mu_out, float* __restrict__ sigma_out) {
#pragma clang fp contract(off)
    extern __shared__ float part[];  // [nch][a]
    __shared__ float mean[64];
    const int t = blockIdx.y * gridDim.x + blockIdx.x;   // row t of problem blockIdx.y: [B][H] rows
    const int nch = (K + ELITE_CHUNK - 1) / ELITE_CHUNK;
    const float* A = aelite + (size_t)t * K * a;
    for (int pass = 0; pass < 2; ++pass) {
        for (int idx = threadIdx.x; idx < nch * a; idx += blockDim.x) {
            const int c = idx / a, d = idx - (idx / a) * a;
            const int e0 = c * ELITE_CHUNK, e1 = min(K, e0 + ELITE_CHUNK);
            float acc = 0.f;
            for (int e = e0; e < e1; ++e) {
                float v = A[(size_t)e * a + d];
                if (pass == 1) { const float df = __fadd_rn(v, -mean[d]); v = __fmul_rn(df, df); }
                acc = (e == e0) ? v : __fadd_rn(acc, v);
            }
            part[c * a + d] = acc;
        }
        __syncthreads();
        if ((int)threadIdx.x < a) {
            const int d = threadIdx.x;
            float tot = part[d];
            for (int c = 1; c < nch; ++c) tot = __fadd_rn(tot, part[c * a + d]);
            const float m = __fdiv_rn(tot, (float)K);
            if (pass == 0) {
                mean[d] = m;
            } else {
                const float mu0 = mu[t * a + d], s0 = sigma[t * a + d];
                mu_out[t * a + d] = __fadd_rn(__fmul_rn(alpha, mu0), __fmul_rn(oma, mean[d]));
                const float v = __fadd_rn(__fmul_rn(alpha, __fmul_rn(s0, s0)), __fmul_rn(oma, m));
                sigma_out[t * a + d] = exact_sqrt(v);
            }
        }
        __syncthreads();
    }
}

// Fused gather + refit for one timestep per workgroup: the K elites' a_t are regenerated from the
// counter RNG straight into LDS ([K][a], when it fits), then the canonical chunked sums run out of
// LDS. Same operation order as gather_elites_kernel + refit_kernel (bit-identical). With `final`
// set it also writes the plan outputs: mu / sigma copies and actions = clip(mu', lo, hi).
constexpr int REFIT_THREADS = 1024;
constexpr size_t REFIT_LDS_MAX = 96 * 1024;

// The elites' actions in LDS: [K][a] with one spare row after every chunk of ELITE_CHUNK elites, so a
// chunk starts 33 a floats after the previous one and the chunk sums' lanes -- lane (c, d) reads
// elite 32 c + q, dimension d -- fall on consecutive banks (at 32 a they all shared a bank, ~10-way).
// The last chunk is padded to 32 rows of -0.0 (ael_pad): x + (-0.0) == x for every x, so every chunk
// sums 32 values with no per-element predicate and the same bits as a sum over its real elites.
__host__ __device__ inline int ael_pos(int e, int d, int a) { return (e + e / ELITE_CHUNK) * a + d; }
__host__ __device__ inline size_t ael_floats(int a, int K) {
    const size_t nch = (size_t)(K + ELITE_CHUNK - 1) / ELITE_CHUNK;
    return (nch * (ELITE_CHUNK + 1) * a + 3) & ~(size_t)3;
}
__device__ __forceinline__ void ael_pad(float* ael, int a, int K) {
    const int nch = (K + ELITE_CHUNK - 1) / ELITE_CHUNK, np = nch * ELITE_CHUNK - K;
    for (int i = threadIdx.x; i < np * a; i += blockDim.x) ael[ael_pos(K + i / a, i % a, a)] = -0.0f;
}

// LDS floats refit_rows works in: the elite actions (ael_pos), [nch][a] chunk partials, mean, this
// row's mu, sigma.
__host__ __device__ inline size_t refit_rows_floats(int a, int K) {
    const size_t nch = (size_t)(K + ELITE_CHUNK - 1) / ELITE_CHUNK;
    const size_t a4 = ((size_t)a + 3) & ~(size_t)3;
    return ael_floats(a, K) + ((nch * a + 3) & ~(size_t)3) + 3 * a4;
}

// Row t of the refit (mu, sigma, outputs already offset to the problem; NULL outputs are skipped): eidx
// = the K elites' global candidate indices in LDS (visible after refit_rows' first barrier). With
// `next` (LDS [2][a4]) the new mu_t, sigma_t are also left there for the next proposal draw.
// The chunked sums of refit_rows over the elites' actions already in LDS (ael = smem [K][a]) and this
// row's mu, sigma staged in musg: mean, population variance, the alpha-smoothed mu', sigma' and the
// outputs. Ends on a barrier.
__device__ __forceinline__ void refit_sums(int t, float* smem, float lo, float hi, int a, int K, float alpha, float oma,
                                           float* __restrict__ mu_out, float* __restrict__ sigma_out,
                                           float* __restrict__ fin_mu, float* __restrict__ fin_sigma,
                                           float* __restrict__ fin_actions, float* next) {
#pragma clang fp contract(off)
    const int nch = (K + ELITE_CHUNK - 1) / ELITE_CHUNK;
    const int a4 = (a + 3) & ~3;
    float* ael = smem;                                   // ael_pos layout
    float* part = smem + ael_floats(a, K);               // [nch][a]
    float* mean = part + (((size_t)nch * a + 3) & ~(size_t)3);  // [a]
    const float* smu = mean + a4;                               // [2][a]: this step's mu, sigma
    const float* ssg = smu + a4;
    CSTAMP(8);
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {   // (unrolled: each pass's code has no pass test)
        for (int idx = threadIdx.x; idx < nch * a; idx += blockDim.x) {
            const int c = idx / a, d = idx - (idx / a) * a;
            const int e0 = c * ELITE_CHUNK, n = min(K - e0, ELITE_CHUNK);
            const float md = pass == 1 ? mean[d] : 0.f;
            float v[ELITE_CHUNK];
            const float* src = ael + (e0 + c) * a + d;   // ael_pos(e0, d); the chunk's rows a floats apart
#pragma unroll
            for (int q = 0; q < ELITE_CHUNK; ++q) v[q] = src[q * a];   // (padding rows: -0.0)
            if (pass == 1)   // the squared deviations first, off the dependent chain; padding stays -0.0
#pragma unroll
                for (int q = 0; q < ELITE_CHUNK; ++q) {
                    const float df = __fadd_rn(v[q], -md);
                    v[q] = q < n ? __fmul_rn(df, df) : -0.0f;
                }
            float acc = v[0];
#pragma unroll
            for (int q = 1; q < ELITE_CHUNK; ++q) acc = __fadd_rn(acc, v[q]);   // 31 dependent additions
            part[c * a + d] = acc;
        }
        __syncthreads();
        CSTAMP(9 + 2 * pass);
        if ((int)threadIdx.x < a) {
            const int d = threadIdx.x;
            // the chunk partials in sequence, eight LDS reads in flight at a time (the same additions
            // in the same order: a dependent read per partial cost ~2 us per pass at walker's 52 chunks)
            float tot = part[d];
            int c = 1;
            for (; c + 8 <= nch; c += 8) {
                float v[8];
#pragma unroll
                for (int q = 0; q < 8; ++q) v[q] = part[(c + q) * a + d];
#pragma unroll
                for (int q = 0; q < 8; ++q) tot = __fadd_rn(tot, v[q]);
            }
            for (; c < nch; ++c) tot = __fadd_rn(tot, part[c * a + d]);
            const float m = __fdiv_rn(tot, (float)K);
            if (pass == 0) {
                mean[d] = m;
            } else {
                const float mu0 = smu[d], s0 = ssg[d];
                const float mn = __fadd_rn(__fmul_rn(alpha, mu0), __fmul_rn(oma, mean[d]));
                const float v = __fadd_rn(__fmul_rn(alpha, __fmul_rn(s0, s0)), __fmul_rn(oma, m));
                const float sn = exact_sqrt(v);
                if (mu_out) mu_out[t * a + d] = mn;
                if (sigma_out) sigma_out[t * a + d] = sn;
                if (next) { next[d] = mn; next[a4 + d] = sn; }
                if (fin_actions) {
                    if (fin_mu) fin_mu[t * a + d] = mn;
                    if (fin_sigma) fin_sigma[t * a + d] = sn;
                    fin_actions[t * a + d] = fminf(fmaxf(mn, lo), hi);
                }
            }
        }
        __syncthreads();
        CSTAMP(10 + 2 * pass);
    }
}

// Row t's mu, sigma into LDS (musg, behind the mean) -- refit_rows' and the split update's first step.
__device__ __forceinline__ void refit_stage_row(int t, float* smem, const float* __restrict__ mu,
                                                const float* __restrict__ sigma, int a, int K) {
    const int nch = (K + ELITE_CHUNK - 1) / ELITE_CHUNK;
    const int a4 = (a + 3) & ~3;
    float* musg = smem + ael_floats(a, K) + (((size_t)nch * a + 3) & ~(size_t)3) + a4;
    for (int d = threadIdx.x; d < a; d += blockDim.x) {
        musg[d] = mu[t * a + d];
        musg[a4 + d] = sigma[t * a + d];
    }
}

// Elites [e0, e1)'s actions of row t regenerated from the counter RNG (bit-identical to the sampled
// ones): into dst, [e][a] (global: the split update's hand-off) or in the ael_pos layout (LDS, padded).
// smu / ssg: this row's mu, sigma.
__device__ __forceinline__ void regen_elites(int t, const uint32_t* eidx, int e0, int e1, uint64_t seed, int iteration,
                                             const float* smu, const float* ssg, float lo, float hi, int a,
                                             float* __restrict__ dst, bool padded) {
#pragma clang fp contract(off)
    const int G = (a + 3) >> 2;
    for (int idx = threadIdx.x; idx < (e1 - e0) * G; idx += blockDim.x) {
        const int e = e0 + idx / G, g = idx - (idx / G) * G;
        float z[4];
        cem_normal4(seed, eidx[e], (uint32_t)t, (uint32_t)iteration, (uint32_t)g, z);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int d = 4 * g + j;
            if (d < a) dst[padded ? (size_t)ael_pos(e, d, a) : (size_t)e * a + d] = cem_action(smu[d], ssg[d], z[j], lo, hi);
        }
    }
}

__device__ __forceinline__ void refit_rows(int t, const uint32_t* eidx, float* smem, uint64_t seed, int iteration,
                                           const float* __restrict__ mu, const float* __restrict__ sigma, float lo,
                                           float hi, int a, int K, float alpha, float oma, float* __restrict__ mu_out,
                                           float* __restrict__ sigma_out, float* __restrict__ fin_mu,
                                           float* __restrict__ fin_sigma, float* __restrict__ fin_actions,
                                           float* next) {
    const int nch = (K + ELITE_CHUNK - 1) / ELITE_CHUNK;
    const int a4 = (a + 3) & ~3;
    const float* musg = smem + ael_floats(a, K) + (((size_t)nch * a + 3) & ~(size_t)3) + a4;
    // stage every global operand first (all loads in flight together), then compute from LDS
    refit_stage_row(t, smem, mu, sigma, a, K);
    ael_pad(smem, a, K);
    __syncthreads();
    regen_elites(t, eidx, 0, K, seed, iteration, musg, musg + a4, lo, hi, a, smem, true);
    __syncthreads();
    refit_sums(t, smem, lo, hi, a, K, alpha, oma, mu_out, sigma_out, fin_mu, fin_sigma, fin_actions, next);
}

__global__ void __launch_bounds__(REFIT_THREADS) refit_fused_kernel(
    uint64_t seed, int iteration, const float* __restrict__ mu, const float* __restrict__ sigma, float lo, float hi,
    int a, const int64_t* __restrict__ elite_idx, int K, float alpha, float oma, float* __restrict__ mu_out,
    float* __restrict__ sigma_out, float* __restrict__ fin_mu, float* __restrict__ fin_sigma,
    float* __restrict__ fin_actions, int n_env) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    // batched planning: blockIdx.y = problem b, whose [H][a] distribution rows sit at b*H*a, whose
    // K elites (local indices) at b*K, and whose candidates are global n = b*n_env + local
    const int t = blockIdx.x, H = gridDim.x;
    const size_t eo = (size_t)blockIdx.y * H * a;
    const uint32_t nbase = (uint32_t)blockIdx.y * (uint32_t)n_env;
    uint32_t* eidx = reinterpret_cast<uint32_t*>(smem + refit_rows_floats(a, K));   // [K]
    elite_idx += (size_t)blockIdx.y * K;
    for (int e = threadIdx.x; e < K; e += REFIT_THREADS) eidx[e] = nbase + (uint32_t)elite_idx[e];
    refit_rows(t, eidx, smem, seed, iteration, mu + eo, sigma + eo, lo, hi, a, K, alpha, oma, mu_out + eo,
               sigma_out + eo, fin_mu ? fin_mu + eo : nullptr, fin_sigma ? fin_sigma + eo : nullptr,
               fin_actions ? fin_actions + eo : nullptr, nullptr);
}

static size_t refit_fused_lds(int a, int K) { return (refit_rows_floats(a, K) + (size_t)K) * sizeof(float); }

// ------------------------------------------------------------------------------------------------
// One launch per CEM iteration after the rollout (DESIGN.md §3 "update"): workgroup (t * S + j, b)
// selects the elites of problem b (every workgroup of the problem the same, deterministic), refits
// row t, and draws row t of the next iteration's proposals for candidate slice j of S from the new
// mu_t, sigma_t. Bit-identical to select_reg_kernel + refit_fused_kernel + sample_kernel: the same
// bodies in the same order. Three launches and their gaps become one; the selection and the row's
// refit are repeated by the workgroups side by side instead of run once (no longer critical path),
// and the draw -- ~400 VALU ops per Philox block -- is spread over S x H workgroups (~256 CUs).
// ------------------------------------------------------------------------------------------------
// (UpdateArgs: mbrl_internal.h)
__host__ __device__ inline size_t update_lds_words(int KPT, int a, int K) {
    const size_t sel = (size_t)sel_words(KPT);
    const size_t ref = refit_rows_floats(a, K);
    return (((size_t)K + 3) & ~(size_t)3) + 2 * (((size_t)a + 3) & ~(size_t)3) + (sel > ref ? sel : ref);
}

// Row t of the next iteration's proposals for candidate slice j of S, from mu', sigma' in LDS (next).
__device__ __forceinline__ void update_draw(const UpdateArgs& U, int t, int j, int S, int b, uint32_t nbase,
                                            const float* next) {
    const int a = U.a, a4 = (a + 3) & ~3;
    const int G = (a + 3) >> 2;
    const int Dn = U.draw_n;
    const size_t row = (size_t)gridDim.y * Dn;
    const uint32_t cbase = nbase + (uint32_t)U.draw_off;   // global candidate of local index 0
    const int NS = (Dn + S - 1) / S, n0 = j * NS, n1 = min(Dn, n0 + NS);
    for (int idx = threadIdx.x; idx < (n1 - n0) * G; idx += 1024) {
        const int n = n0 + idx / G, g = idx - (idx / G) * G;
        float z[4];
        cem_normal4(U.seed, cbase + (uint32_t)n, (uint32_t)t, (uint32_t)(U.iteration + 1), (uint32_t)g, z);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int d = 4 * g + q;
            if (d < a)
                U.next_actions[((size_t)t * row + (size_t)b * Dn + n) * a + d] =
                    cem_action(next[d], next[a4 + d], z[q], U.lo, U.hi);
        }
    }
}

template <int KPT>
__global__ void __launch_bounds__(1024) cem_update_kernel(const UpdateArgs U) {
    extern __shared__ __attribute__((aligned(16))) uint32_t usmem[];
    const int S = gridDim.x / U.H;                      // draw slices per row
    const int t = blockIdx.x / S, j = blockIdx.x - (blockIdx.x / S) * S, b = blockIdx.y;
    const bool lead = t == 0 && j == 0;                 // writes the elites and returns
    const int K = U.K, N = U.N, a = U.a, a4 = (a + 3) & ~3;
    uint32_t* eidx = usmem;                                                  // [K] global candidate index
    float* next = reinterpret_cast<float*>(usmem + ((K + 3) & ~3));          // [2][a4] mu', sigma' of row t
    uint32_t* work = usmem + ((K + 3) & ~3) + 2 * a4;                        // select, then refit
    const uint32_t nbase = (uint32_t)b * (uint32_t)N;
    int64_t* eo = (U.elite_out && lead) ? U.elite_out + (size_t)b * K : nullptr;
    float* ro = (U.returns_out && lead) ? U.returns_out + (size_t)b * N : nullptr;
    select_reg_body<KPT>(U.costs + (size_t)b * N, U.E, N, K, MBRL_NAN_LAST, ro, U.member_stride, work,
                         [&](uint32_t pos, int n) {
                             eidx[pos] = nbase + (uint32_t)n;
                             if (eo) eo[pos] = n;
                         });
    __syncthreads();   // eidx complete; the selection's LDS becomes the refit's
    CSTAMP(6);
    const size_t rb = (size_t)b * U.H * a;
    const bool w = j == 0;   // slice 0 of the row writes its refit
    refit_rows(t, eidx, reinterpret_cast<float*>(work), U.seed, U.iteration, U.mu + rb, U.sigma + rb, U.lo, U.hi, a,
               K, U.alpha, U.oma, w ? U.mu_out + rb : nullptr, w ? U.sigma_out + rb : nullptr,
               (w && U.fin_mu) ? U.fin_mu + rb : nullptr, (w && U.fin_sigma) ? U.fin_sigma + rb : nullptr,
               (w && U.fin_actions) ? U.fin_actions + rb : nullptr, U.next_actions ? next : nullptr);
    CSTAMP(7);
    if (U.next_actions) update_draw(U, t, j, S, b, nbase, next);   // refit_rows ended on a barrier
}

// The same update as two launches (the split update): the regeneration of the K elites'
// actions -- K ceil(a / 4) Philox blocks per row, repeated by each of the row's S workgroups in
// cem_update_kernel -- is shared out: launch 1 (select + regenerate) has workgroup (t, j) select, then
// regenerate elites [j K / S, (j + 1) K / S) of row t into U.ael; launch 2 (refit + draw) has every
// workgroup of row t read the row's K elites back, then run the same chunked sums and the draw. The
// kernel boundary is the only hand-off. Bit-identical to cem_update_kernel: the same values in the
// same order.
template <int KPT>
__global__ void __launch_bounds__(1024) cem_select_regen_kernel(const UpdateArgs U) {
    extern __shared__ __attribute__((aligned(16))) uint32_t usmem[];
    const int S = gridDim.x / U.H;
    const int t = blockIdx.x / S, j = blockIdx.x - (blockIdx.x / S) * S;
    const bool lead = t == 0 && j == 0;
    const int K = U.K, N = U.N, a = U.a, a4 = (a + 3) & ~3;
    uint32_t* eidx = usmem;                                                  // [K] global candidate index
    float* row = reinterpret_cast<float*>(usmem + ((K + 3) & ~3));          // [2][a4] mu_t, sigma_t
    uint32_t* work = usmem + ((K + 3) & ~3) + 2 * a4;
    int64_t* eo = (U.elite_out && lead) ? U.elite_out : nullptr;
    float* ro = (U.returns_out && lead) ? U.returns_out : nullptr;
    WGSTAMP(0, 0);
    for (int d = threadIdx.x; d < a; d += 1024) {
        row[d] = U.mu[t * a + d];
        row[a4 + d] = U.sigma[t * a + d];
    }
    select_reg_body<KPT>(U.costs, U.E, N, K, MBRL_NAN_LAST, ro, U.member_stride, work,
                         [&](uint32_t pos, int n) {
                             eidx[pos] = (uint32_t)n;
                             if (eo) eo[pos] = n;
                         });
    __syncthreads();   // eidx complete (and the row staged)
    WGSTAMP(0, 1);
    const int KS = (K + S - 1) / S, e0 = min(K, j * KS), e1 = min(K, e0 + KS);
    regen_elites(t, eidx, e0, e1, U.seed, U.iteration, row, row + a4, U.lo, U.hi, a, U.ael + (size_t)t * K * a, false);
#ifdef MBRL_STAMPS
    __syncthreads();
    WGSTAMP(0, 2);
#endif
}

__global__ void __launch_bounds__(1024) cem_refit_draw_kernel(const UpdateArgs U) {
    extern __shared__ __attribute__((aligned(16))) float fsmem[];
    const int S = gridDim.x / U.H;
    const int t = blockIdx.x / S, j = blockIdx.x - (blockIdx.x / S) * S;
    const int K = U.K, a = U.a, a4 = (a + 3) & ~3;
    float* next = fsmem;                  // [2][a4] mu', sigma' of row t
    float* work = fsmem + 2 * a4;         // refit_rows' layout: [K][a] elites, partials, mean, mu / sigma
    WGSTAMP(1, 0);
    const float* src = U.ael + (size_t)t * K * a;
    const int n = K * a, ca = ELITE_CHUNK * a;   // flat index f = e a + d lands at f + (f / ca) a (ael_pos)
    if ((n & 3) == 0) {
        // 16-byte loads, up to four per thread in flight before the first LDS store
        typedef float f4 __attribute__((ext_vector_type(4)));
        const f4* s4 = reinterpret_cast<const f4*>(src);
        const int n4 = n >> 2;
        for (int i0 = threadIdx.x; i0 < n4; i0 += 4 * 1024) {
            f4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (i0 + u * 1024 < n4) v[u] = s4[i0 + u * 1024];
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (i0 + u * 1024 < n4)
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const int f = 4 * (i0 + u * 1024) + k;
                        work[f + (f / ca) * a] = v[u][k];
                    }
        }
    } else {
        for (int f = threadIdx.x; f < n; f += 1024) work[f + (f / ca) * a] = src[f];
    }
    refit_stage_row(t, work, U.mu, U.sigma, a, K);
    ael_pad(work, a, K);
    __syncthreads();
    WGSTAMP(1, 3);
    const bool w = j == 0;   // slice 0 of the row writes its refit
    refit_sums(t, work, U.lo, U.hi, a, K, U.alpha, U.oma, w ? U.mu_out : nullptr, w ? U.sigma_out : nullptr,
               (w && U.fin_mu) ? U.fin_mu : nullptr, (w && U.fin_sigma) ? U.fin_sigma : nullptr,
               (w && U.fin_actions) ? U.fin_actions : nullptr, U.next_actions ? next : nullptr);
    WGSTAMP(1, 1);
    if (U.next_actions) update_draw(U, t, j, S, 0, 0u, next);
#ifdef MBRL_STAMPS
    __syncthreads();
    WGSTAMP(1, 2);
#endif
}

// The plan's first launch: workgroup (t * S + j, b) sets row t of problem b's distribution to
// (init_mu, init_sigma) and, with `actions`, draws row t of iteration 0's proposals for candidate
// slice j (fill2_kernel + sample_kernel, bit-identical: the same floats go into cem_action).
// s0_src (optional): the plan's start state, device or mapped host memory, copied once into the
// workspace (s0_dst) so that every later launch reads device memory. draw_off: the global candidate
// index of local candidate 0 (a sharded plan's rank offset; 0 otherwise). zero[2] / zero_words[2]:
// the plan's hand-off words (the column-split pairs' flags, the trajectory kernel's granules and
// status; InitZero, mbrl_internal.h), zeroed here once per plan instead of by a memset before each
// launch that polls them.
// ROWS (the MPPI plan's warm start, single problem): the initial mean of row t is mu_rows[t][.] clipped
// to [lo, hi] instead of init_mu. ROWS = false compiles to the kernel without the argument.
template <bool ROWS>
__global__ void __launch_bounds__(1024) cem_init_kernel(uint64_t seed, float init_mu, float init_sigma, float lo,
                                                        float hi, int H, int a, int N, float* __restrict__ mu,
                                                        float* __restrict__ sigma, float* __restrict__ actions,
                                                        const float* __restrict__ s0_src, int s,
                                                        float* __restrict__ s0_dst, int draw_off, InitZero zero,
                                                        const float* __restrict__ mu_rows) {
    const int S = gridDim.x / H;
    const int t = blockIdx.x / S, j = blockIdx.x - (blockIdx.x / S) * S, b = blockIdx.y;
    const size_t ro = ((size_t)b * H + t) * a;
    {
        const size_t gid = ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * blockDim.x + threadIdx.x;
        const size_t gsz = (size_t)gridDim.x * gridDim.y * blockDim.x;
#pragma unroll
        for (int r = 0; r < 2; ++r)
            for (size_t i = gid; zero.ptr[r] && i < zero.words[r]; i += gsz) zero.ptr[r][i] = 0u;
    }
    if (s0_src && blockIdx.x == 0 && b == 0)
        for (int d = threadIdx.x; d < s; d += blockDim.x) s0_dst[d] = s0_src[d];
    if (j == 0)
        for (int d = threadIdx.x; d < a; d += blockDim.x) {
            float m0 = init_mu;
            if (ROWS) m0 = fminf(fmaxf(mu_rows[ro + d], lo), hi);
            mu[ro + d] = m0;
            sigma[ro + d] = init_sigma;
        }
    if (!actions) return;
    const int G = (a + 3) >> 2;
    const size_t BN = (size_t)gridDim.y * N;
    const uint32_t nbase = (uint32_t)b * (uint32_t)N;
    const int NS = (N + S - 1) / S, n0 = j * NS, n1 = min(N, n0 + NS);
    for (int idx = threadIdx.x; idx < (n1 - n0) * G; idx += blockDim.x) {
        const int n = n0 + idx / G, g = idx - (idx / G) * G;
        float z[4];
        cem_normal4(seed, nbase + (uint32_t)draw_off + (uint32_t)n, (uint32_t)t, 0u, (uint32_t)g, z);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int d = 4 * g + j;
            if (d < a) {
                float m0 = init_mu;
                if (ROWS) m0 = fminf(fmaxf(mu_rows[ro + d], lo), hi);
                actions[((size_t)t * BN + nbase + n) * a + d] = cem_action(m0, init_sigma, z[j], lo, hi);
            }
        }
    }
}

void launch_cem_init(dim3 grid, hipStream_t stream, uint64_t seed, float init_mu, float init_sigma, float lo, float hi,
                     int H, int a, int N, float* mu, float* sigma, float* actions, const float* s0_src, int s,
                     float* s0_dst, int draw_off, const InitZero& zero, const float* mu_rows) {
    if (mu_rows)
        hipLaunchKernelGGL(cem_init_kernel<true>, grid, dim3(1024), 0, stream, seed, init_mu, init_sigma, lo, hi, H, a, N,
                           mu, sigma, actions, s0_src, s, s0_dst, draw_off, zero, mu_rows);
    else
        hipLaunchKernelGGL(cem_init_kernel<false>, grid, dim3(1024), 0, stream, seed, init_mu, init_sigma, lo, hi, H, a,
                           N, mu, sigma, actions, s0_src, s, s0_dst, draw_off, zero, nullptr);
}

// Batched planning: local candidate n belongs to problem n / n_env, whose distribution rows sit at
// mu + (n / n_env) * H * a (n_env = N for a single problem).
__global__ void sample_kernel(uint64_t seed, int iteration, const float* __restrict__ mu,
                              const float* __restrict__ sigma, float lo, float hi, int H, int a, int N,
                              int n_offset, float* __restrict__ out, int n_env) {
    const int G = (a + 3) >> 2;
    const size_t total = (size_t)H * N * G;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int g = (int)(i % G);
        const int n = (int)((i / G) % N);
        const int t = (int)(i / G / N);
        float z[4];
        cem_normal4(seed, (uint32_t)(n_offset + n), (uint32_t)t, (uint32_t)iteration, (uint32_t)g, z);
        const size_t mo = (size_t)(n / n_env) * H * a + (size_t)t * a;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int d = 4 * g + j;
            if (d < a) out[((size_t)t * N + n) * a + d] = cem_action(mu[mo + d], sigma[mo + d], z[j], lo, hi);
        }
    }
}

__global__ void finalize_kernel(const float* __restrict__ mu_src, const float* __restrict__ sg_src, float lo,
                                float hi, int n, float* __restrict__ mu, float* __restrict__ sigma,
                                float* __restrict__ actions) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        const float m = mu_src[i];
        if (mu) mu[i] = m;
        if (sigma) sigma[i] = sg_src[i];
        actions[i] = fminf(fmaxf(m, lo), hi);
    }
}

int sample_impl(const mbrl_sampler* sp, int H, int a, int N, int n_offset, float* out, hipStream_t stream, int n_env) {
    const size_t total = (size_t)H * N * ((a + 3) / 4);
    const int blocks = (int)((total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192);
    hipLaunchKernelGGL(sample_kernel, dim3(blocks), dim3(256), 0, stream, sp->seed, sp->iteration, sp->mu, sp->sigma,
                       sp->lo, sp->hi, H, a, N, n_offset, out, n_env > 0 ? n_env : N);
    return hip_check(hipGetLastError(), "sample launch");
}

int select_impl(const float* costs, int E, int N, int K, int nan_policy, int64_t* elite_idx, float* returns_out,
                void* ws, size_t ws_bytes, hipStream_t stream, int segments) {
    if (!costs || !elite_idx || !ws) return fail(MBRL_EINVAL, "costs, elite_idx and workspace must be non-NULL");
    if (N < 1 || K < 1 || K > N || E < 1 || segments < 1)
        return fail(MBRL_EINVAL, "need 1 <= K (%d) <= N (%d), E >= 1, segments >= 1", K, N);
    const size_t need = align256((size_t)N * segments * 4);
    if (ws_bytes < need) return fail(MBRL_EWORKSPACE, "select workspace %zu < %zu", ws_bytes, need);
    const int member_stride = N * segments;
#define MBRL_SEL(KPT)                                                                                       \
    if (N <= 1024 * (KPT)) {                                                                                \
        const size_t lds = select_reg_lds(KPT);                                                             \
        hipError_t err = ensure_dynamic_lds(reinterpret_cast<const void*>(&select_reg_kernel<KPT>), (int)lds); \
        if (err != hipSuccess) return hip_check(err, "select attribute");                                   \
        hipLaunchKernelGGL(select_reg_kernel<KPT>, dim3(segments), dim3(1024), lds, stream, costs, E, N, K,  \
                           nan_policy, elite_idx, returns_out, member_stride);                              \
        return hip_check(hipGetLastError(), "select launch");                                               \
    }
    MBRL_SEL(1) MBRL_SEL(2) MBRL_SEL(4) MBRL_SEL(8) MBRL_SEL(16) MBRL_SEL(32)
#undef MBRL_SEL
    hipLaunchKernelGGL(select_kernel, dim3(segments), dim3(1024), 0, stream, costs, E, N, K, nan_policy, elite_idx,
                       returns_out, static_cast<uint32_t*>(ws), member_stride);
    return hip_check(hipGetLastError(), "select launch");
}

int refit_impl(const mbrl_sampler* sp, int H, int a, const int64_t* elite_idx, int K, float alpha, float* aelite,
               float* mu_out, float* sigma_out, hipStream_t stream, float* fin_mu, float* fin_sigma,
               float* fin_actions, int B, int n_env) {
    if (!sp || !sp->mu || !sp->sigma || !elite_idx || !mu_out || !sigma_out)
        return fail(MBRL_EINVAL, "refit: NULL argument");
    if (H < 1 || a < 1 || a > 64 || K < 1) return fail(MBRL_EINVAL, "refit: H=%d a=%d K=%d", H, a, K);
    const float oma = 1.0f - alpha;
    const size_t lds = refit_fused_lds(a, K);
    if (lds <= REFIT_LDS_MAX) {
        hipError_t err = ensure_dynamic_lds(reinterpret_cast<const void*>(&refit_fused_kernel), (int)REFIT_LDS_MAX);
        if (err != hipSuccess) return hip_check(err, "refit attribute");
        hipLaunchKernelGGL(refit_fused_kernel, dim3(H, B), dim3(REFIT_THREADS), lds, stream, sp->seed,
                           sp->iteration, sp->mu, sp->sigma, sp->lo, sp->hi, a, elite_idx, K, alpha, oma, mu_out,
                           sigma_out, fin_mu, fin_sigma, fin_actions, n_env);
        return hip_check(hipGetLastError(), "refit launch");
    }
    // large K x a: elite actions staged through HBM
    if (B != 1) return fail(MBRL_EUNSUPPORTED, "batched refit: K=%d x a=%d exceeds the fused kernel's LDS", K, a);
    if (!aelite) return fail(MBRL_EINVAL, "refit: NULL workspace");
    if ((size_t)((K + ELITE_CHUNK - 1) / ELITE_CHUNK) * a * sizeof(float) > 64 * 1024)
        return fail(MBRL_EUNSUPPORTED, "refit: K=%d x a=%d exceeds the refit kernel's LDS", K, a);
    const int G = (a + 3) / 4;
    hipLaunchKernelGGL(gather_elites_kernel, dim3((K * G + 255) / 256, H), dim3(256), 0, stream, sp->seed,
                       sp->iteration, sp->mu, sp->sigma, sp->lo, sp->hi, a, elite_idx, K, aelite);
    const int nch = (K + ELITE_CHUNK - 1) / ELITE_CHUNK;
    hipLaunchKernelGGL(refit_kernel, dim3(H), dim3(256), (size_t)nch * a * sizeof(float), stream, aelite, a, K,
                       alpha, oma, sp->mu, sp->sigma, mu_out, sigma_out);
    if (fin_actions)
        hipLaunchKernelGGL(finalize_kernel, dim3((H * a + 255) / 256), dim3(256), 0, stream, mu_out, sigma_out,
                           sp->lo, sp->hi, H * a, fin_mu, fin_sigma, fin_actions);
    return hip_check(hipGetLastError(), "refit launch");
}

int refit_staged_check(int a, int K) {
    if (a < 1 || a > 64 || K < 1) return fail(MBRL_EINVAL, "refit: a=%d K=%d", a, K);
    if ((size_t)((K + ELITE_CHUNK - 1) / ELITE_CHUNK) * a * sizeof(float) > 64 * 1024)
        return fail(MBRL_EUNSUPPORTED, "refit: K=%d x a=%d exceeds the refit kernel's LDS", K, a);
    return MBRL_OK;
}

int refit_staged_impl(const float* aelite, int H, int a, int K, float alpha, const float* mu, const float* sigma,
                      float* mu_out, float* sigma_out, hipStream_t stream, int B) {
    if (int rc = refit_staged_check(a, K)) return rc;
    if (B < 1 || B > 65535) return fail(MBRL_EINVAL, "refit: B=%d", B);
    const int nch = (K + ELITE_CHUNK - 1) / ELITE_CHUNK;
    hipLaunchKernelGGL(refit_kernel, dim3(H, B), dim3(256), (size_t)nch * a * sizeof(float), stream, aelite, a, K, alpha,
                       1.0f - alpha, mu, sigma, mu_out, sigma_out);
    return hip_check(hipGetLastError(), "refit launch");
}

// The fused per-iteration update (cem_update_kernel) when its selection fits in registers (N <= 32768)
// and the selection or refit working set fits LDS; KPT of that selection, 0 if not fusable.
int update_kpt(int N, int K, int a) {
    if (a > 64 || K < 1 || K > N) return 0;
    for (int kpt = 1; kpt <= 32; kpt *= 2)
        if (N <= 1024 * kpt) return update_lds_words(kpt, a, K) * 4 + 1024 <= 160 * 1024 ? kpt : 0;   // + static LDS
    return 0;
}

// Whether the update also draws the next iteration's proposals: at most 64 Philox blocks per thread
// (the H blocks of the launch draw N x H x a values between them).
bool update_samples(int N, int a) { return (size_t)N * ((a + 3) / 4) <= 64 * 1024; }

// Candidate slices per row for the fused draw: about 256 workgroups in all (one per CU; each runs the
// selection too), and no slice under 256 Philox blocks.
int draw_slices(int H, int B, int N, int a) {
    const long hb = (long)H * B;
    long s = 256 / hb;
    const long cap = ((long)N * ((a + 3) / 4) + 255) / 256;
    if (s > cap) s = cap;
    return s < 1 ? 1 : (int)s;
}

// The split update (two launches, cem_select_regen_kernel + cem_refit_draw_kernel) where the elites'
// regeneration is worth sharing out: at least SPLIT_MIN_BLOCKS Philox blocks per row (walker's K =
// 1638: 3276 blocks, ~10 us of one workgroup's VALU; cheetah's 818 would save less than the launch
// boundary costs). MBRL_OPT_UPDATE_SPLIT: 0 auto, 1 never, 2 wherever scratch is given (tests, A/B).
constexpr long SPLIT_MIN_BLOCKS = 2048;

static bool update_split(const UpdateArgs& U, int B) {
    const int o = opt(MBRL_OPT_UPDATE_SPLIT);
    if (o == 1 || B != 1 || !U.ael) return false;
    return o == 2 || (long)U.K * ((U.a + 3) / 4) >= SPLIT_MIN_BLOCKS;
}

static int update_split_impl(const UpdateArgs& U, int kpt, hipStream_t stream) {
    // workgroups per row: the draw's slices, and at least ~256 workgroups in all for the regeneration
    const int Sd = U.next_actions ? draw_slices(U.H, 1, U.draw_n, U.a) : 1;
    const int S = std::max(Sd, std::max(1, 256 / U.H));
    const int a4 = (U.a + 3) & ~3;
    const size_t lds_a = ((((size_t)U.K + 3) & ~(size_t)3) + 2 * a4 + (size_t)sel_words(kpt)) * 4;
    const size_t lds_b = (2 * a4 + refit_rows_floats(U.a, U.K)) * 4;
    if (lds_b + 1024 > 160 * 1024) return fail(MBRL_EUNSUPPORTED, "split update: K=%d a=%d exceeds LDS", U.K, U.a);
#define MBRL_SPLIT_A(KPT)                                                                                       \
    if (kpt == KPT) {                                                                                           \
        hipError_t err = ensure_dynamic_lds(reinterpret_cast<const void*>(&cem_select_regen_kernel<KPT>), (int)lds_a); \
        if (err != hipSuccess) return hip_check(err, "split update attribute");                                 \
        hipLaunchKernelGGL(cem_select_regen_kernel<KPT>, dim3(U.H * S), dim3(1024), lds_a, stream, U);          \
    }
    MBRL_SPLIT_A(1) MBRL_SPLIT_A(2) MBRL_SPLIT_A(4) MBRL_SPLIT_A(8) MBRL_SPLIT_A(16) MBRL_SPLIT_A(32)
#undef MBRL_SPLIT_A
    if (int rc = hip_check(hipGetLastError(), "split update launch 1")) return rc;
    hipError_t err = ensure_dynamic_lds(reinterpret_cast<const void*>(&cem_refit_draw_kernel), (int)lds_b);
    if (err != hipSuccess) return hip_check(err, "split update attribute");
    hipLaunchKernelGGL(cem_refit_draw_kernel, dim3(U.H * S), dim3(1024), lds_b, stream, U);
    return hip_check(hipGetLastError(), "split update launch 2");
}

int update_impl(const UpdateArgs& U, int B, hipStream_t stream) {
    const int kpt = update_kpt(U.N, U.K, U.a);
    if (!kpt) return fail(MBRL_EUNSUPPORTED, "update: N=%d K=%d a=%d not fusable", U.N, U.K, U.a);
    if (update_split(U, B)) return update_split_impl(U, kpt, stream);
    const size_t lds = update_lds_words(kpt, U.a, U.K) * 4;
    const int S = U.next_actions ? draw_slices(U.H, B, U.draw_n, U.a) : 1;
#define MBRL_UPD(KPT)                                                                                            \
    if (kpt == KPT) {                                                                                           \
        hipError_t err = ensure_dynamic_lds(reinterpret_cast<const void*>(&cem_update_kernel<KPT>), (int)lds);   \
        if (err != hipSuccess) return hip_check(err, "update attribute");                                       \
        hipLaunchKernelGGL(cem_update_kernel<KPT>, dim3(U.H * S, B), dim3(1024), lds, stream, U);                \
        return hip_check(hipGetLastError(), "update launch");                                                   \
    }
    MBRL_UPD(1) MBRL_UPD(2) MBRL_UPD(4) MBRL_UPD(8) MBRL_UPD(16) MBRL_UPD(32)
#undef MBRL_UPD
    return fail(MBRL_EUNSUPPORTED, "update: KPT %d", kpt);
}

}  // namespace mbrl

using namespace mbrl;

// ================================================================================================
// extern "C" ABI
// ================================================================================================
extern "C" {

size_t mbrl_select_workspace_bytes(int32_t N) { return align256((size_t)(N > 0 ? N : 1) * 4); }

int mbrl_select_elites(const float* costs, int32_t E, int32_t N, int32_t K, int32_t nan_policy, int64_t* elite_idx,
                       float* returns_out, void* workspace, size_t ws_bytes, mbrl_stream_t stream) {
    return select_impl(costs, E, N, K, nan_policy, elite_idx, returns_out, workspace, ws_bytes,
                       reinterpret_cast<hipStream_t>(stream));
}

size_t mbrl_refit_workspace_bytes(int32_t H, int32_t a, int32_t K) {
    return align256((size_t)(H > 0 ? H : 1) * (K > 0 ? K : 1) * (a > 0 ? a : 1) * sizeof(float));
}

int mbrl_cem_refit(const mbrl_sampler* sampler, int32_t H, int32_t a, const int64_t* elite_idx, int32_t K, float alpha,
                   float* mu_out, float* sigma_out, void* workspace, size_t ws_bytes, mbrl_stream_t stream) {
    if (!workspace) return fail(MBRL_EINVAL, "refit: workspace is NULL");
    if (ws_bytes < mbrl_refit_workspace_bytes(H, a, K))
        return fail(MBRL_EWORKSPACE, "refit workspace %zu < %zu", ws_bytes, mbrl_refit_workspace_bytes(H, a, K));
    return refit_impl(sampler, H, a, elite_idx, K, alpha, static_cast<float*>(workspace), mu_out, sigma_out,
                      reinterpret_cast<hipStream_t>(stream));
}

int mbrl_sample_actions(const mbrl_sampler* sampler, int32_t H, int32_t a, int32_t N, int32_t n_offset,
                        float* actions_out, mbrl_stream_t stream) {
    if (!sampler || !sampler->mu || !sampler->sigma || !actions_out) return fail(MBRL_EINVAL, "sample: NULL argument");
    if (H < 1 || a < 1 || N < 1 || n_offset < 0) return fail(MBRL_EINVAL, "sample: bad sizes");
    return sample_impl(sampler, H, a, N, n_offset, actions_out, reinterpret_cast<hipStream_t>(stream));
}

int mbrl_cem_update(const float* costs, int32_t E, int32_t N, int32_t K, const mbrl_sampler* sampler, int32_t H,
                    int32_t a, float alpha, int64_t* elite_idx, float* returns_out, float* mu_out, float* sigma_out,
                    float* next_actions, int32_t draw_offset, int32_t draw_count, mbrl_stream_t stream) {
    if (!costs || !sampler || !sampler->mu || !sampler->sigma || !mu_out || !sigma_out)
        return fail(MBRL_EINVAL, "cem_update: NULL argument");
    if (N < 1 || K < 1 || K > N || E < 1 || H < 1 || a < 1)
        return fail(MBRL_EINVAL, "cem_update: need 1 <= K (%d) <= N (%d), E, H, a >= 1", K, N);
    if (next_actions && (draw_count < 1 || draw_offset < 0 || (int64_t)draw_offset + draw_count > N))
        return fail(MBRL_EINVAL, "cem_update: draw range [%d, %d + %d) outside [0, %d)", draw_offset, draw_offset,
                    draw_count, N);
    if (!update_kpt(N, K, a))
        return fail(MBRL_EUNSUPPORTED, "cem_update: N=%d K=%d a=%d exceeds the fused kernel (select + refit + draw)",
                    N, K, a);
    UpdateArgs U{};
    U.costs = costs; U.E = E; U.N = N; U.K = K; U.member_stride = N; U.H = H; U.a = a;
    U.elite_out = elite_idx; U.returns_out = returns_out;
    U.seed = sampler->seed; U.iteration = sampler->iteration; U.mu = sampler->mu; U.sigma = sampler->sigma;
    U.lo = sampler->lo; U.hi = sampler->hi; U.alpha = alpha; U.oma = 1.0f - alpha;
    U.mu_out = mu_out; U.sigma_out = sigma_out;
    U.next_actions = next_actions; U.draw_off = next_actions ? draw_offset : 0; U.draw_n = next_actions ? draw_count : N;
    return update_impl(U, 1, reinterpret_cast<hipStream_t>(stream));
}

// MBRL_OPT_SHARD_EMULATE 2 (timing): the all-gather's rank-major buffer in one launch -- this rank's
// slot from its own costs, every other slot from the costs a mode-1 plan kept for this iteration --
// and the gathered status words (this rank's own, the others clear). Launched by plan_sharded.hip
// (launch_emu_gather below); it lives here, next to the stamp buffer it writes in the diagnostic build.
__global__ void emu_gather_kernel(const float* __restrict__ local, const float* __restrict__ kept, int G, int rank,
                                  size_t slot, const unsigned* __restrict__ own_status,
                                  const unsigned* __restrict__ own_pair, float* __restrict__ gathered,
                                  unsigned* __restrict__ peer) {
    const size_t total = (size_t)G * slot, lo = (size_t)rank * slot;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x)
        gathered[i] = (i >= lo && i < lo + slot) ? local[i - lo] : kept[i];
#ifdef MBRL_STAMPS
    if (threadIdx.x == 0 && g_cem_wg_stamps)   // (diagnostic) a workgroup's end, last writer wins
        g_cem_wg_stamps[8 * 2 * 1024 * 4 - 1] = __builtin_amdgcn_s_memrealtime();
#endif
    if (blockIdx.x == 0)
        for (int r = threadIdx.x; r < G; r += blockDim.x) {
            peer[r] = r == rank ? *own_status : 0u;
            peer[G + r] = (r == rank && own_pair) ? *own_pair : 0u;
        }
}

#ifdef MBRL_STAMPS
int mbrl_diag_set_cem_stamps(void* buf) {
    return (int)hipMemcpyToSymbol(HIP_SYMBOL(mbrl::g_cem_stamps), &buf, sizeof(buf));
}
int mbrl_diag_set_cem_wg_stamps(void* buf) {
    return (int)hipMemcpyToSymbol(HIP_SYMBOL(mbrl::g_cem_wg_stamps), &buf, sizeof(buf));
}
#endif

}  // extern "C"

void mbrl::launch_emu_gather(const float* local, const float* kept, int G, int rank, size_t slot,
                             const unsigned* own_status, const unsigned* own_pair, float* gathered, unsigned* peer,
                             hipStream_t stream) {
    hipLaunchKernelGGL(emu_gather_kernel, dim3(256), dim3(256), 0, stream, local, kept, G, rank, slot, own_status,
                       own_pair, gathered, peer);
}
