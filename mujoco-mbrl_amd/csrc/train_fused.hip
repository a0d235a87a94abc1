// The fused step for two hidden layers (the reference's Model / ModelWithReward, models.py:97-132):
// three launches per batch instead of five. Every product is the same MFMA chains over the same K
// ranges as in the five-launch layout, and every sum of partials runs in the same order, so the
// gradients, losses and Adam steps are the same floats (tests/test_gpu_train_native.py pins it):
//   F  train_fused_fwd_kernel: per 32 x 32 tile of H_1, the tile's 32 rows of H_0 are recomputed into
//      LDS (K0 = s + a is small: the layer-0 launch's 4-wave K split, summed in its wave order), then
//      the H_1 tile is the layer-1 launch's tile with its A operand from LDS. Removes a launch and
//      the H_0 round trip through memory before the layer-1 products. The first column tiles also
//      gather the batch's targets for O; in mbrl_train_epoch the second column tiles gather the next
//      batch's rows and targets into the other gather slot.
//   O  train_fused_out_kernel: per 32 x 32 tile of dH_1, the tile's 32 rows of dY (the output-layer
//      launch's tile: loss partials and dY column sums from the first column tile), dH_1 =
//      (dY W_out) * (H_1 > 0), and the output layer's weight-gradient partial over the tile's 32 rows
//      -- exactly wave tm of the separate dW_out product -- summed in wave order by the column block's
//      last arriver (an sc1 hand-off), which also finishes db_out, db_1 and b_1's Adam step.
//      Removes a launch and the dY round trip.
//   B  launch_gemm: dH_0 with the folded dW_0 and its Adam step, dW_1 -- whose tiles step W_1 in place
//      once the dH_0 tiles of their column block have read it -- and the output layer's Adam step as
//      extra workgroups. No Adam step is deferred to the next batch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mbrl_adam_dev.h"
#include "mbrl_train.h"

namespace mbrl {

#ifdef MBRL_STAMPS
static __device__ unsigned long long* g_train_stamps;   // FSTAMP's buffer (mbrl_train.h)
hipError_t train_fused_set_stamps(void* buf) {
    return hipMemcpyToSymbol(HIP_SYMBOL(g_train_stamps), &buf, sizeof(buf));
}
#endif

constexpr int TRAIN_SC1 = 16;   // buffer-op aux bit: sc1 (write-through stores, L1-bypassing loads)
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// A wave's K range in a launch of nw waves (gemm_tile's split: contiguous 16-deep chunks).
__device__ __forceinline__ void wave_k_range(int K, int nw, int w, int& kb0, int& kb1) {
    const int chunks = (K + 15) >> 4, per = (chunks + nw - 1) / nw;
    kb0 = w * per * 16;
    kb1 = min(K, (w + 1) * per * 16);
}

// Four consecutive k of one row of a row-major matrix (row stride ld), zero past K or for an absent
// row: load_operand<OP_DIRECT>'s values (float4 when aligned, else element by element).
// (The guarded loads here measured faster than load_raw's branch-free form in F and O: 49.2-49.3
// against 50.0 us per step, late r05 -- unlike the backward launch's K loop, where the branch-free
// form saves 3.6 us.)
__device__ __forceinline__ f32x4 row4(const float* row, bool valid, int k0, int K, bool vec) {
    f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
    if (!valid) return v;
    if (vec && k0 + 3 < K) return *reinterpret_cast<const f32x4*>(row + k0);
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (k0 + e < K) v[e] = row[k0 + e];
    return v;
}

constexpr int FUSED_HLD = FUSED_WMAX + 4, FUSED_XLD = FUSED_K0MAX + 4;

// F's body. KCH: 16-deep chunks of K0 (2: K0 <= 32, 4: K0 <= 64), one per wave of the layer-0 launch
// (4 waves). FO (one launch with O): the batch's targets and the H_1 tile leave as write-through (sc1)
// stores, the tile also stays in LDS (hm: O's ReLU mask and dW_out operand), and the workgroup then
// adds to its band's counter.
template <int NW, int KCH, bool FO>
__device__ __forceinline__ void fused_fwd(const FusedArgs& F, float (*red)[TT][TT + 1], float (*h0)[FUSED_HLD],
                                          float (*xr)[FUSED_XLD], float (*hm)[TT + 1]) {
    constexpr int NT = 64 * NW, EPT = TT * TT / NT, MAXPER = NW == 16 ? 2 : 4, MAXY = NW == 16 ? 2 : 4;
    constexpr int NW0 = 4;   // the layer-0 launch's waves (K0 < 256)
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, q = lane >> 4, c = lane & 15;
    const int tm = blockIdx.x / F.tiles_n, tn = blockIdx.x - tm * F.tiles_n, m0 = tm * TT, n0 = tn * TT;
    const int W = F.W, K0 = F.K0, R = F.R;
    FSTAMP(0, 0);
    if (blockIdx.x == 0 && F.zero_words)
        for (int i = tid; i < F.zero_n; i += NT) F.zero_words[i] = 0u;
    if (blockIdx.x == 0 && F.serial && tid == 0) *F.serial = *F.serial + 1u;
    // the batch's 32 input rows are gathered through the row indices: the indices, the rows, then every
    // weight operand of the launch (in-order vmcnt: a wait for the rows then waits for nothing issued
    // after them, and the weights travel while the rows do)
    constexpr int GPT = TT * 16 * KCH / NT;      // gathered elements per thread (k0pad <= 16 KCH)
    const int k0pad = (K0 + 15) & ~15;
    const bool nx = F.idx_next != nullptr && tn == 1;   // the second column tiles gather the next batch
    int64_t gi[GPT], gn[GPT];
#pragma unroll
    for (int j = 0; j < GPT; ++j) {
        const int e = tid + j * NT, r = e / k0pad, k = e - r * k0pad, m = m0 + r;
        gi[j] = (r < TT && m < R && k < K0) ? (F.pre_rows ? 0 : F.idx[m / F.H]) : -1;
        gn[j] = (nx && r < TT && m < F.R_next && k < K0) ? F.idx_next[m / F.H] : -1;
    }
    // the first column tiles also gather the targets O's loss epilogue needs (J <= 32: 32 x 32 slots)
    constexpr int TPT = TT * TT / NT;
    float tv[TPT];
    int64_t tsrc[TPT];
#pragma unroll
    for (int j = 0; j < TPT; ++j) {
        const int e = tid + j * NT, r = e >> 5, o = e & 31, m = m0 + r;
        tsrc[j] = -1;
        if (!F.pre_rows && tn == 0 && o < F.J && m < R) tsrc[j] = F.idx[m / F.H] * F.H + m % F.H;
        if (nx && o < F.J && m < F.R_next) tsrc[j] = F.idx_next[m / F.H] * F.H + m % F.H;
    }
    // the rows (zero past K0 to the chunk end); the first column tile keeps them for the layer-0 weight
    // gradient, as the layer-0 launch did
    float gv[GPT];
#pragma unroll
    for (int j = 0; j < GPT; ++j) {
        const int e = tid + j * NT, r = e / k0pad, k = e - r * k0pad, m = m0 + r;
        gv[j] = 0.0f;
        if (gi[j] >= 0) {
            if (F.pre_rows) {
                gv[j] = F.xstore[(int64_t)m * K0 + k];
            } else {
                const int64_t src = gi[j] * F.H + m % F.H;
                gv[j] = k < F.s ? F.gs[src * F.s + k] : F.ga[src * F.a + (k - F.s)];
            }
        }
    }
    float gx[GPT];
#pragma unroll
    for (int j = 0; j < GPT; ++j) {
        const int e = tid + j * NT, r = e / k0pad, k = e - r * k0pad, m = m0 + r;
        const int64_t src = gn[j] * F.H + m % F.H;
        gx[j] = gn[j] < 0 ? 0.0f : k < F.s ? F.gs[src * F.s + k] : F.ga[src * F.a + (k - F.s)];
    }
#pragma unroll
    for (int j = 0; j < TPT; ++j) {
        const int o = (tid + j * NT) & 31;
        tv[j] = tsrc[j] < 0 ? 0.0f : o < F.s ? F.gns[tsrc[j] * F.s + o] : F.grw[tsrc[j]];
    }
    // the layer-1 operands (this wave's K range of W_1's rows n0..n0+31, and the bias), issued behind
    // the rows: their latency overlaps the rows' and the H_0 recompute
    int kb0, kb1;
    wave_k_range(W, NW, wave, kb0, kb1);
    const bool vec1 = (W % 4 == 0) && (reinterpret_cast<uintptr_t>(F.w1) & 15) == 0;
    f32x4 bw[MAXPER][2];
#pragma unroll
    for (int u = 0; u < MAXPER; ++u)
#pragma unroll
        for (int y = 0; y < 2; ++y) {
            const int n = n0 + 16 * y + c, kb = kb0 + 16 * u;
            bw[u][y] = row4(F.w1 + (int64_t)min(n, W - 1) * W, n < W && kb < kb1, kb + 4 * q, W, vec1);
        }
    float pre[FO ? 1 : EPT];
    f32x4 pre4 = {0.0f, 0.0f, 0.0f, 0.0f};   // FO: thread t < 256 finishes 4 consecutive columns
    if constexpr (FO) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int n = n0 + (tid & 7) * 4 + i;
            pre4[i] = (tid < TT * TT / 4 && n < W) ? F.b1[n] : 0.0f;
        }
    } else {
#pragma unroll
        for (int j = 0; j < EPT; ++j) {
            const int e = tid + j * NT, n = n0 + (e & 31);
            pre[j] = n < W ? F.b1[n] : 0.0f;
        }
    }
    // W_0's rows for this wave's 16-column blocks of H_0 (y = wave, wave + NW, ...), every chunk
    const int ny = (W + 15) >> 4, nch0 = (K0 + 15) >> 4;
    const bool vec0 = (K0 % 4 == 0) && (reinterpret_cast<uintptr_t>(F.w0) & 15) == 0;
    f32x4 w0r[MAXY][KCH];
    float b0r[MAXY];
#pragma unroll
    for (int yy = 0; yy < MAXY; ++yy) {
        const int n = 16 * (wave + yy * NW) + c;
        b0r[yy] = n < W ? F.b0[n] : 0.0f;
#pragma unroll
        for (int ch = 0; ch < KCH; ++ch)
            w0r[yy][ch] = row4(F.w0 + (int64_t)min(n, W - 1) * K0, n < W && ch < nch0, 16 * ch + 4 * q, K0, vec0);
    }
#pragma unroll
    for (int j = 0; j < GPT; ++j) {
        const int e = tid + j * NT, r = e / k0pad, k = e - r * k0pad, m = m0 + r;
        if (r < TT) xr[r][k] = gv[j];
        if (gi[j] >= 0 && tn == 0 && !F.pre_rows) F.xstore[(int64_t)m * K0 + k] = gv[j];
        if (gn[j] >= 0) F.xnext[(int64_t)m * K0 + k] = gx[j];
    }
#pragma unroll
    for (int j = 0; j < TPT; ++j) {
        const int e = tid + j * NT, r = e >> 5, o = e & 31;
        if (tsrc[j] < 0) continue;
        float* dst = (nx ? F.tnext : F.tgt) + (int64_t)(m0 + r) * F.J + o;
        if (FO && !nx) __hip_atomic_store(dst, tv[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // O reads it
        else *dst = tv[j];
    }
    __syncthreads();
    FSTAMP(0, 1);
    // H_0 rows m0..m0+31, all W columns: wave w takes the 16-column blocks y = w, w + NW, ...; each
    // 16 x 16 block is the sum, in wave order, of the layer-0 launch's per-wave chains (NW0 waves,
    // empty ones adding +0), then bias and ReLU -- that launch's epilogue
#pragma unroll
    for (int yy = 0; yy < MAXY; ++yy) {
        const int y = wave + yy * NW, n = 16 * y + c;
        if (y >= ny) break;
        f32x4 tot[2];
#pragma unroll
        for (int vw = 0; vw < NW0; ++vw) {      // wave vw of the layer-0 launch: chunk vw (or nothing)
            f32x4 p[2] = {{0.0f, 0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f, 0.0f}};
            if (vw < KCH && vw < nch0) {
                f32x4 a[2];
#pragma unroll
                for (int x = 0; x < 2; ++x) a[x] = *reinterpret_cast<const f32x4*>(&xr[16 * x + c][16 * vw + 4 * q]);
#pragma unroll
                for (int s = 0; s < 4; ++s)
#pragma unroll
                    for (int x = 0; x < 2; ++x)
                        p[x] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[x][s], w0r[yy][vw < KCH ? vw : 0][s], p[x], 0, 0, 0);
            }
#pragma unroll
            for (int x = 0; x < 2; ++x) tot[x] = vw == 0 ? p[x] : tot[x] + p[x];
        }
        const float bias = b0r[yy];
#pragma unroll
        for (int x = 0; x < 2; ++x)
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int row = 16 * x + 4 * q + v;
                float h = tot[x][v] + bias;
                h = h > 0.0f ? h : 0.0f;
                h0[row][n] = (n < W && m0 + row < R) ? h : 0.0f;
            }
    }
    __syncthreads();
    FSTAMP(0, 2);
    // this tile's columns of H_0 (every element stored by exactly one workgroup)
    for (int e = tid; e < TT * TT; e += NT) {
        const int r = e >> 5, col = e & 31, m = m0 + r, n = n0 + col;
        if (m < R && n < W) F.act0[(int64_t)m * W + n] = h0[r][n];
    }
    // the H_1 tile: the layer-1 launch's chains with the A operand from LDS
    f32x4 acc[2][2];
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y) acc[x][y] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int u = 0; u < MAXPER; ++u) {
        const int kb = kb0 + 16 * u;
        if (kb >= kb1) break;
        f32x4 a[2];
#pragma unroll
        for (int x = 0; x < 2; ++x) a[x] = *reinterpret_cast<const f32x4*>(&h0[16 * x + c][kb + 4 * q]);
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int x = 0; x < 2; ++x)
#pragma unroll
                for (int y = 0; y < 2; ++y)
                    acc[x][y] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[x][s], bw[u][y][s], acc[x][y], 0, 0, 0);
    }
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y)
#pragma unroll
            for (int v = 0; v < 4; ++v) red[wave][16 * x + 4 * q + v][16 * y + c] = acc[x][y][v];
    __syncthreads();
    if constexpr (!FO) {
#pragma unroll
        for (int j = 0; j < EPT; ++j) {
            const int e = tid + j * NT, row = e >> 5, col = e & 31, m = m0 + row, n = n0 + col;
            if (m >= R || n >= W) continue;
            float v = red[0][row][col];
#pragma unroll
            for (int w = 1; w < NW; ++w) v = v + red[w][row][col];
            v = v + pre[j];
            F.act1[(int64_t)m * W + n] = v > 0.0f ? v : 0.0f;
        }
    } else {
        // the same sums, 4 columns per thread: one 16-byte write-through store (4-byte ones at a ragged
        // or unaligned edge), and the tile into hm
        if (tid < TT * TT / 4) {
            const int row = tid >> 3, c4 = (tid & 7) * 4, m = m0 + row;
            f32x4 h;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float v = red[0][row][c4 + i];
#pragma unroll
                for (int w = 1; w < NW; ++w) v = v + red[w][row][c4 + i];
                v = v + pre4[i];
                h[i] = (m < R && n0 + c4 + i < W) ? (v > 0.0f ? v : 0.0f) : 0.0f;
                hm[row][c4 + i] = h[i];
            }
            if (m < R) {
                const __amdgpu_buffer_rsrc_t ar = __builtin_amdgcn_make_buffer_rsrc(
                    F.act1, 0, (int)((int64_t)R * W * sizeof(float)), 0x00020000);
                const unsigned off = (unsigned)(((int64_t)m * W + n0 + c4) * sizeof(float));
                if ((W & 3) == 0 && (reinterpret_cast<uintptr_t>(F.act1) & 15) == 0 && n0 + c4 + 3 < W) {
                    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, h), ar, off, 0, TRAIN_SC1);
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        if (n0 + c4 + i < W)
                            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, (float)h[i]), ar, off + 4 * i, 0,
                                                                  TRAIN_SC1);
                }
            }
        }
        // every storing wave drains its stores, then one lane signals for the workgroup
        // (MI355X_MICROARCH.md, the first row of the sc1 hand-off table)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (tid == 0) __hip_atomic_fetch_add(F.band + tm * 32, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    FSTAMP(0, 3);
}

// KCH: as fused_fwd
template <int NW, int KCH>
__global__ __launch_bounds__(64 * NW) void train_fused_fwd_kernel(const FusedArgs F) {
    __shared__ float red[NW][TT][TT + 1];
    __shared__ __attribute__((aligned(16))) float h0[TT][FUSED_HLD];
    __shared__ __attribute__((aligned(16))) float xr[TT][FUSED_XLD];
    fused_fwd<NW, KCH, false>(F, red, h0, xr, nullptr);
}

// Four consecutive k of an H_1 row handed over in this launch: sc1 buffer loads (the row's byte
// offset `row_off`; row4's zero fill and element fallback)
__device__ __forceinline__ f32x4 row4_sc1(__amdgpu_buffer_rsrc_t r, unsigned row_off, bool valid, int k0, int K,
                                          bool vec) {
    f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
    if (!valid) return v;
    if (vec && k0 + 3 < K)
        return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, row_off + 4u * k0, 0, TRAIN_SC1));
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (k0 + e < K)
            v[e] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, row_off + 4u * (k0 + e), 0, TRAIN_SC1));
    return v;
}

// FO: wait until every F tile of band tm has written its H_1 columns (one lane polls, sc1 loads; a
// 1 s bound sets bit 0 of *status instead of hanging), then count this tile as past the wait; the
// band's last such add resets the counter for the next launch. The band's tiles are consecutive
// workgroup ids, so with in-order dispatch the earliest unfinished band is always fully resident.
__device__ __forceinline__ void band_wait(const FusedArgs& F, int tm) {
    if (threadIdx.x == 0) {
        unsigned* c = F.band + tm * 32;
        const unsigned need = (unsigned)F.tiles_n;
        const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
        while (__hip_atomic_load(c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < need) {
            if (__builtin_amdgcn_s_memrealtime() - t0 > 100000000ull) {
                atomicOr(F.status, 1u);
                break;
            }
            __builtin_amdgcn_s_sleep(1);
        }
        if (__hip_atomic_fetch_add(c, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1 == 2 * need)
            __hip_atomic_store(c, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
}

// O's body. dy: the tile's 32 rows of dY (columns past J zero); hm: H_1 of the tile (the ReLU mask and
// the dW_out operand). FO (one launch with F): hm is already there, W_out's rows are loaded before
// the band wait and the band's H_1 rows and targets after it, with sc1 loads.
template <int NW, bool FO>
__device__ __forceinline__ void fused_out(const FusedArgs& F, float (*red)[TT][TT + 1], float (*dy)[TT + 1],
                                          float (*hm)[TT + 1], unsigned& last) {
    constexpr int NT = 64 * NW, EPT = TT * TT / NT, MAXPER = NW == 16 ? 2 : 4;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, q = lane >> 4, c = lane & 15;
    const int tm = blockIdx.x / F.tiles_n, tn = blockIdx.x - tm * F.tiles_n, m0 = tm * TT, n0 = tn * TT;
    const int W = F.W, J = F.J, R = F.R, S = F.s;
    FSTAMP(1, 0);
    // b_1's Adam operands for this column block (threads 64-95), for the last arriver's tail
    const bool b1t = tid >= 64 && tid < 64 + TT && n0 + tid - 64 < W;
    float b1p = 0.0f, b1m = 0.0f, b1v = 0.0f;
    if (F.adam && b1t) {
        b1p = F.ab1.param[n0 + tid - 64];
        b1m = F.ab1.exp_avg[n0 + tid - 64];
        b1v = F.ab1.exp_avg_sq[n0 + tid - 64];
    }
    // ---- the output-layer tile (tm, 0): Y = H_1 W_out^T + b_out over this wave's K range
    int kb0, kb1;
    wave_k_range(W, NW, wave, kb0, kb1);
    const bool veca = (W % 4 == 0) && (reinterpret_cast<uintptr_t>(F.act1) & 15) == 0;
    const bool vecb = (W % 4 == 0) && ((reinterpret_cast<uintptr_t>(F.wo) | reinterpret_cast<uintptr_t>(F.wo_r)) & 15) == 0;
    f32x4 av[MAXPER][2], bv[MAXPER][2];
#pragma unroll
    for (int u = 0; u < MAXPER; ++u) {
        const int kb = kb0 + 16 * u;
#pragma unroll
        for (int y = 0; y < 2; ++y) {
            const int o = 16 * y + c;
            const float* row = o < S ? F.wo + (int64_t)o * W : F.wo_r;
            bv[u][y] = row4(row, o < J && kb < kb1, kb + 4 * q, W, vecb);
        }
    }
    if constexpr (FO) {
        band_wait(F, tm);
        const __amdgpu_buffer_rsrc_t ar = __builtin_amdgcn_make_buffer_rsrc(
            F.act1, 0, (int)((int64_t)R * W * sizeof(float)), 0x00020000);
#pragma unroll
        for (int u = 0; u < MAXPER; ++u) {
            const int kb = kb0 + 16 * u;
#pragma unroll
            for (int x = 0; x < 2; ++x) {
                const int m = m0 + 16 * x + c;
                av[u][x] = row4_sc1(ar, (unsigned)((int64_t)min(m, R - 1) * W * sizeof(float)), m < R && kb < kb1,
                                    kb + 4 * q, W, veca);
            }
        }
    } else {
#pragma unroll
        for (int u = 0; u < MAXPER; ++u) {
            const int kb = kb0 + 16 * u;
#pragma unroll
            for (int x = 0; x < 2; ++x) {
                const int m = m0 + 16 * x + c;
                av[u][x] = row4(F.act1 + (int64_t)min(m, R - 1) * W, m < R && kb < kb1, kb + 4 * q, W, veca);
            }
        }
    }
    // the loss epilogue's y - t = acc - (t - bias), and the tile's H_1 block (mask, dW_out operand)
    float pre[EPT];
#pragma unroll
    for (int j = 0; j < EPT; ++j) {
        const int e = tid + j * NT, m = m0 + (e >> 5), o = e & 31;
        pre[j] = 0.0f;
        if (m >= R || o >= J) continue;
        const float* tg = F.tgt + (int64_t)m * J + o;
        pre[j] = (FO ? __hip_atomic_load(tg, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : *tg) -
                 (o < S ? F.bo[o] : F.bo_r[o - S]);
    }
    if constexpr (!FO)
        for (int e = tid; e < TT * TT; e += NT) {
            const int r = e >> 5, col = e & 31, m = m0 + r, n = n0 + col;
            hm[r][col] = (m < R && n < W) ? F.act1[(int64_t)m * W + n] : 0.0f;
        }
    f32x4 acc[2][2];
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y) acc[x][y] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int u = 0; u < MAXPER; ++u) {
        if (kb0 + 16 * u >= kb1) break;
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int x = 0; x < 2; ++x)
#pragma unroll
                for (int y = 0; y < 2; ++y)
                    acc[x][y] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u][x][s], bv[u][y][s], acc[x][y], 0, 0, 0);
    }
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y)
#pragma unroll
            for (int v = 0; v < 4; ++v) red[wave][16 * x + 4 * q + v][16 * y + c] = acc[x][y][v];
    __syncthreads();
    // the output-layer launch's EPI_LOSS epilogue: dY = (Y - T) * 2 / numel, the loss terms
    float loss_s = 0.0f, loss_r = 0.0f;
#pragma unroll
    for (int j = 0; j < EPT; ++j) {
        const int e = tid + j * NT, row = e >> 5, col = e & 31, m = m0 + row;
        float v = 0.0f;
        if (m < R && col < J) {
            v = red[0][row][col];
#pragma unroll
            for (int w = 1; w < NW; ++w) v = v + red[w][row][col];
            const float d = v - pre[j];
            if (col < S) loss_s = loss_s + d * d * F.inv_s;
            else loss_r = loss_r + d * d * F.inv_r;
            v = d * (col < S ? F.scale_s : F.scale_r);
        }
        dy[row][col] = v;
    }
    __syncthreads();
    FSTAMP(1, 1);
    if (tn == 0) {
        // dY's column sums over the tile's rows (db_out), read back by this launch's last arriver
        if (tid < TT && tid < J) {
            float t = dy[0][tid];
            for (int r = 1; r < TT; ++r) t = t + dy[r][tid];
            __hip_atomic_store(F.cs_dy + (int64_t)tm * J + tid, t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            loss_s += __shfl_xor(loss_s, o);
            loss_r += __shfl_xor(loss_r, o);
        }
        float* sl = &red[1][0][0];      // red[1] is free: every wave's partials were summed above
        if (lane == 0) {
            sl[2 * wave] = loss_s;
            sl[2 * wave + 1] = loss_r;
        }
        __syncthreads();
        if (tid < 2) {
            float t = sl[tid];
            for (int w = 1; w < NW; ++w) t = t + sl[2 * w + tid];
            F.loss_part[tm * 2 + tid] = t;
        }
    }
    // ---- tasks 0-3: the dH_1 tile, K = J (the [dH_1 + dW_out] launch's split over nwb waves: one
    // 16-deep chunk per wave, the rest adding +0), masked by H_1 > 0. Tasks 4-7: the dW_out partial
    // over rows m0..m0+31 (that launch's wave tm: its two 16-row chunks, M = J, N = this column block)
    for (int task = wave; task < 8; task += NW) {   // (4 waves: each takes one block of both)
      if (task < 4) {
        const int x = task >> 1, y = task & 1, n = n0 + 16 * y + c;
        f32x4 tot = {0.0f, 0.0f, 0.0f, 0.0f};
        const int nch = (J + 15) >> 4;
        for (int ch = 0; ch < nch; ++ch) {
            f32x4 a, b, p = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int k = 16 * ch + 4 * q + s;     // an output unit o
                a[s] = dy[16 * x + c][k];
                b[s] = (k < J && n < W) ? (k < S ? F.wo[(int64_t)k * W + n] : F.wo_r[(int64_t)(k - S) * W + n]) : 0.0f;
            }
#pragma unroll
            for (int s = 0; s < 4; ++s) p = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s], b[s], p, 0, 0, 0);
            tot = ch == 0 ? p : tot + p;
        }
        for (int w = nch; w < F.nwb; ++w) tot = tot + f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int row = 16 * x + 4 * q + v, m = m0 + row;
            const float g = hm[row][16 * y + c] > 0.0f ? tot[v] : 0.0f;
            const float keep = (m < R && n < W) ? g : 0.0f;
            if (m < R && n < W) F.dh1[(int64_t)m * W + n] = g;
            red[0][row][16 * y + c] = keep;
        }
      } else {
        const int x = (task - 4) >> 1, y = (task - 4) & 1;
        f32x4 p = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            f32x4 a, b;
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int r = 16 * u + 4 * q + s;      // a row of the batch tile (K of this product)
                a[s] = dy[r][16 * x + c];
                b[s] = hm[r][16 * y + c];
            }
#pragma unroll
            for (int s = 0; s < 4; ++s) p = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s], b[s], p, 0, 0, 0);
        }
        const int i = n0 + 16 * y + c;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int o = 16 * x + 4 * q + v;
            if (o < J && i < W)    // sc1 (write-through) stores, read back by the last arriver
                __hip_atomic_store(F.out_part + ((int64_t)tm * J + o) * W + i, p[v], __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
        }
      }
    }
    __syncthreads();
    // dH_1's column sums over the tile's 32 rows, in row order (db_1: this column block's last arriver)
    if (tid < TT && n0 + tid < W) {
        float t = red[0][0][tid];
        for (int r = 1; r < TT; ++r) t = t + red[0][r][tid];
        __hip_atomic_store(F.cs_dh1 + (int64_t)tm * W + n0 + tid, t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    FSTAMP(1, 2);
    // the column block's last arriver sums the dW_out partials in wave order (row tiles past the
    // batch: the empty waves' +0), and the first column block's also db_out from dY's column sums
    if (tid == 0) {
        const unsigned t = __hip_atomic_fetch_add(&F.out_ticket[tn], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        last = (t + 1 == (unsigned)F.tiles_r) ? 1u : 0u;
        // every arrival is in: reset the ticket for the next launch (in one launch with F, nothing
        // zeroes it at the start)
        if (last) __hip_atomic_store(&F.out_ticket[tn], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    FSTAMP(1, 3);
    if (!last) return;
    // every load of the tail first (db_out's and db_1's column sums, then the partials): one round trip
    const bool dyt = tn == 0 && tid < J, tfast = F.tiles_r <= 16;
    float cs[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const float* src = dyt ? F.cs_dy + (int64_t)i * J + tid : F.cs_dh1 + (int64_t)i * W + n0 + tid - 64;
        cs[i] = ((dyt || b1t) && tfast && i < F.tiles_r)
                    ? __hip_atomic_load(src, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0f;
    }
    for (int e = tid; e < J * TT; e += NT) {
        const int o = e / TT, i = n0 + (e - o * TT);
        if (i >= W) continue;
        float p[16];
#pragma unroll
        for (int w = 0; w < 16; ++w)
            p[w] = (w < F.tiles_r && w < F.nwb)
                       ? __hip_atomic_load(F.out_part + ((int64_t)w * J + o) * W + i, __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_AGENT)
                       : 0.0f;
        float v = p[0];
#pragma unroll
        for (int w = 1; w < 16; ++w)
            if (w < F.nwb) v = v + p[w];
        if (o < S) F.dwo[(int64_t)o * W + i] = v;
        else F.dwo_r[(int64_t)(o - S) * W + i] = v;
    }
    if (dyt || b1t) {
        float g = cs[0];
#pragma unroll
        for (int i = 1; i < 16; ++i)
            if (i < F.tiles_r) g = g + cs[i];
        if (dyt) {              // db_out
            if (!tfast) g = ordered_sum<true>(F.cs_dy + tid, J, F.tiles_r);
            if (tid < S) F.dbo[tid] = g;
            else F.dbo_r[tid - S] = g;
        } else {                // db_1 (the five-launch layout's dW_1 launch summed the same column sums in
            const int n = n0 + tid - 64;   // the same order) and b_1's Adam step: nothing reads b_1 before
            if (!tfast) g = ordered_sum<true>(F.cs_dh1 + n, W, F.tiles_r);   // the next batch's F
            F.db1[n] = g;
            if (F.adam) {
                adam_element(b1p, g, b1m, b1v, F.ab1.step_size, F.ab1.bc2_sqrt, F.hp, F.arith);
                F.ab1.param[n] = b1p;
                F.ab1.exp_avg[n] = b1m;
                F.ab1.exp_avg_sq[n] = b1v;
            }
        }
    }
}

template <int NW>
__global__ __launch_bounds__(64 * NW) void train_fused_out_kernel(const FusedArgs F) {
    __shared__ float red[NW][TT][TT + 1];
    __shared__ float dy[TT][TT + 1];
    __shared__ float hm[TT][TT + 1];
    __shared__ unsigned last;
    fused_out<NW, false>(F, red, dy, hm, last);
}

// F and O as one launch: the O tiles of a 32-row band wait (band_wait) for that band's F tiles only,
// instead of the whole grid at a kernel boundary, and W_out's rows load during the wait. The same
// bodies, so the same bits as the two launches (MBRL_OPT_TRAIN_FO = 1 keeps them apart).
template <int NW, int KCH>
__global__ __launch_bounds__(64 * NW) void train_fused_fo_kernel(const FusedArgs F) {
    __shared__ float red[NW][TT][TT + 1];
    __shared__ __attribute__((aligned(16))) float h0[TT][FUSED_HLD];
    __shared__ __attribute__((aligned(16))) float xr[TT][FUSED_XLD];
    __shared__ unsigned last;
    // hm and dy alias h0, which F no longer reads once its H_1 products are in red
    float(*hm)[TT + 1] = reinterpret_cast<float(*)[TT + 1]>(&h0[0][0]);
    float(*dy)[TT + 1] = hm + TT;
    fused_fwd<NW, KCH, true>(F, red, h0, xr, hm);
    fused_out<NW, true>(F, red, dy, hm, last);
}

template <int NW, int KCH>
static void launch_fused_at(const FusedArgs& F, bool fo_split, hipStream_t stream) {
    const dim3 grid(F.tiles_r * F.tiles_n), block(64 * NW);
    if (!fo_split) {
        hipLaunchKernelGGL((train_fused_fo_kernel<NW, KCH>), grid, block, 0, stream, F);
        return;
    }
    hipLaunchKernelGGL((train_fused_fwd_kernel<NW, KCH>), grid, block, 0, stream, F);
    hipLaunchKernelGGL(train_fused_out_kernel<NW>, grid, block, 0, stream, F);
}

hipError_t launch_train_fused(const FusedArgs& F, bool fo_split, hipStream_t stream) {
    const int nw = F.W >= 256 ? 16 : 4;   // the wave count of the separate launches whose K is W
    const int kch = F.K0 <= 32 ? 2 : 4;   // K0's 16-deep chunks
    if (nw == 16 && kch == 2) launch_fused_at<16, 2>(F, fo_split, stream);
    else if (nw == 16) launch_fused_at<16, 4>(F, fo_split, stream);
    else if (kch == 2) launch_fused_at<4, 2>(F, fo_split, stream);
    else launch_fused_at<4, 4>(F, fo_split, stream);
    return hipGetLastError();
}

}  // namespace mbrl
