// Model training forward + backward (mbrl_train_grads): the gradient of the reference's per-batch
// loss (models.py:65-85 / 188-207: MSELoss of the predicted next state, plus the reward head's for
// ModelWithReward, summed over the horizon steps) with respect to every Linear of the MLP, as
// n_hidden + 2 launches of one tiled fp32 MFMA kernel instead of autograd's chain of library GEMMs,
// elementwise kernels and reductions.
//
// Every launch computes one or two products C = A . B^T over 32 x 32 tiles of C, one tile per
// workgroup: 4 or 16 waves split K, each accumulating a 32 x 32 partial with v_mfma_f32_16x16x4f32
// (lane l feeds A(m0 + l%16, k) and B(n0 + l%16, k) for k = kb + 4(l/16) + s, s = 0..3, so a lane's
// four k are consecutive and one float4 load serves four MFMAs when the operand is k-contiguous).
// The partials meet in LDS, summed in wave order, and the epilogue fuses what follows the product:
//   forward        H_l = relu(A W_l^T + b_l)                                  (EPI_ACT)
//   output layer   Y = H W_out^T + b_out;  dY = (Y - target) * 2 / numel, loss partials (EPI_LOSS)
//   backward dX    dH_{l-1} = (dH_l W_l) * (H_{l-1} > 0)                        (EPI_MASK)
//   backward dW    dW_l = dH_l^T H_{l-1}, db_l from column sums the dH / dY launch left per
//                  row tile                                                     (EPI_GRAD)
// The batch is gathered on the fly from the stacked transitions through the batch's row indices
// (no materialised input), and the state and reward heads are one output layer of s + 1 rows.
// Arithmetic is fp32 with fp32 accumulation; the summation order differs from autograd's, so the
// gradients agree with torch's to rounding (tests/test_gpu_train_native.py), not bit for bit.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <type_traits>
#include <utility>

#include "mbrl_adam_dev.h"
#include "mbrl_host.h"
#include "mbrl_train.h"

namespace mbrl {

#ifdef MBRL_STAMPS
static __device__ unsigned long long* g_train_stamps;   // TSTAMP's buffer (mbrl_train.h)
hipError_t train_gemm_set_stamps(void* buf) {
    return hipMemcpyToSymbol(HIP_SYMBOL(g_train_stamps), &buf, sizeof(buf));
}
#endif

enum { OP_DIRECT = 0, OP_TRANS = 1, OP_GATHER = 2 };
enum { EPI_ACT = 0, EPI_LOSS = 1, EPI_MASK = 2, EPI_GRAD = 3 };
constexpr int ADAM_FUSED_MAX = 4;   // tensors per fused Adam role (a layer's weight and bias, or both heads')
constexpr int FOLD_K0MAX = 64;      // the dW_0 fold stages its tile's input rows in LDS up to this K0

// Logical operand X(i, k), i < rows, k < K, over a row-major storage matrix S whose rows below
// `split` live at p0 and the rest at p1 (the state and reward heads as one matrix).
struct Operand {
    const float* p0;
    const float* p1;
    int split, ld;
    int kind;          // OP_DIRECT: X(i,k) = S[i][k]   OP_TRANS: X(i,k) = S[k][i]   OP_GATHER: batch input
    int rows;          // extent of i (including the ones row)
    int ones_row;      // i == ones_row reads 1 (the bias-gradient column); -1: none
    int gather_trans;  // OP_GATHER: 0: X(i,k) = input[row i][col k]; 1: X(i,k) = input[row k][col i]
    int vec;           // OP_DIRECT: rows 16-byte aligned (float4 loads)
};

struct Output {
    int mode;
    float* c0;
    float* c1;
    int split, ldc;           // C[m][n]: m < split -> c0[m*ldc + n], else c1[(m - split)*ldc + n]
    const float* b0;          // EPI_ACT / EPI_LOSS bias by column: n < bsplit ? b0[n] : b1[n - bsplit]
    const float* b1;
    int bsplit;
    int relu;
    const float* mask;        // EPI_MASK: C *= (mask[m*ldm + n] > 0)
    int ldm;
    float* g0;                // EPI_GRAD: the bias gradient, g0[m] / g1[m - split], from colsum_in
    float* g1;
    const float* colsum_in;   // EPI_GRAD: [colsum_tiles][M] column sums of this layer's output gradient
                              // (NULL: the bias gradient is finished elsewhere -- the fused step's O)
    int colsum_tiles;
    float* colsum_out;        // EPI_MASK / EPI_LOSS: [row tile][N] column sums of the stored C
    int adam;                 // EPI_GRAD: also take this layer's Adam step in place (nothing reads it
                              // in this launch): weight at aw (= c0 layout), bias at ab
    mbrl_adam_tensor aw, ab;
    // EPI_GRAD with adam, fused step: this launch's dH tiles read the weight block being stepped; the
    // tile waits until wait_ticket[n0 / 32] (their arrivals per column block) reaches wait_count.
    // Those tiles have lower workgroup ids, so they were dispatched first and always finish; the
    // bounded spin only guards against a hang (bit 0 of wait_status on timeout).
    const unsigned* wait_ticket;
    unsigned wait_count;
    unsigned* wait_status;
    unsigned* arrive_ticket;  // EPI_MASK, fused step: one add per tile to [n0 / 32] once its K loop (every
                              // read of the weight block) is done -- what wait_ticket counts
    // EPI_MASK of dH_0 with fold (launch_train_grads): the tile also yields the layer-0 weight
    // gradient's partial over each of its 32-row blocks -- exactly what wave tr of the separate dW_0
    // launch summed -- as tagged granules (fold_gran below); the dW_1 tiles of row block 0 add them
    // in wave order into dW_0 / db_0 and take layer 0's Adam step (fold_sum)
    int fold, fold_k0, fold_nw;         // input columns K0, the separate launch's wave count
    const float* fold_x;                // the gathered input [R][K0] (xbuf, written by the forward)
    float *fold_dw, *fold_db;           // dW_0 [W][K0], db_0 [W]
    int fold_cs_tiles;                  // 32-row tiles of the column sums (colsum_out of this product)
    int fold_adam;
    mbrl_adam_tensor fold_aw, fold_ab;
    // the fold's hand-off as tagged granules {value, tag} (8-byte stores, read untorn): the partials
    // [tr][W][K0] and the column sums [tr][W] of dH_0, tag = the step's serial (*fold_serial, raised
    // by the step's first launch); the dW_1 tiles of row block 0 (fold_sum) poll them and finish
    // dW_0 / db_0 and layer 0's Adam step. No drain, ticket or last arriver on the producers' side.
    unsigned long long *fold_gran, *cs_gran;
    const unsigned* fold_serial;
    unsigned* fold_status;              // bit 0: a bounded wait timed out
    int fold_sum;                       // EPI_GRAD (dW_1): row block 0's tiles run fold_sum
    float scale_s, scale_r;   // EPI_LOSS: dY scale of the state / reward columns (2 / numel)
    float inv_s, inv_r;       // EPI_LOSS: loss weight of the state / reward columns (1 / numel)
    int s;                    // EPI_LOSS: state columns (n >= s: the reward column)
    float* loss_part;         // EPI_LOSS: [tile][2] partial losses (state, reward)
};

struct GemmDesc {
    Operand A, B;
    Output out;
    int M, N, K, tiles_n, tiles;
};

struct GemmLaunch {
    GemmDesc d[2];
    int nd;
    // the batch: row r of the logical input is transition idx[r / H], horizon step r % H
    const int64_t* idx;
    const float* gs;    // stacked states      [T][H][s]
    const float* ga;    // stacked actions     [T][H][a]
    const float* gns;   // stacked next states [T][H][s]
    const float* grw;   // stacked rewards     [T][H]
    int H, s, a;
    float* xstore;      // [rows][s + a]: the gathered input, written by the layer-0 forward launch
    int slot;           // launch index within the step (diagnostic stamps)
    // loss: one extra workgroup sums the partials (fixed order) into loss_out[0..2]
    const float* loss_part;
    int loss_parts;
    float* loss_out;
    // fused Adam (mbrl_train_epoch): the step of a layer whose gradient the previous launch finished,
    // as extra workgroups after the products' tiles (ADAM_FUSED_CHUNK elements each)
    int adam_count, adam_blocks, adam_chunk;   // adam_chunk: elements per Adam workgroup
    mbrl_adam_tensor adam_t[ADAM_FUSED_MAX];
    unsigned* zero_words;   // workgroup 0 zeroes zero_n words first (the fold's tickets; forward launch)
    int zero_n;
    unsigned* serial;       // workgroup 0 raises the step's serial (the fold's granule tag; forward launch)
    int adam_first[ADAM_FUSED_MAX + 1];
    mbrl_adam_hparams hp;
    int arith;
    // product 0's tiles in XCD order (MBRL_OPT_TRAIN_XCD): every 64-row band of the batch on XCD
    // (band % 8) in every launch, so a launch reads the rows the previous launch wrote on its own XCD
    int xcd;
};

__device__ __forceinline__ int64_t batch_row(const GemmLaunch& L, int r) {
    return L.idx[r / L.H] * L.H + r % L.H;
}

__device__ __forceinline__ float input_at(const GemmLaunch& L, int r, int c) {
    const int64_t src = batch_row(L, r);
    return c < L.s ? L.gs[src * L.s + c] : L.ga[src * L.a + (c - L.s)];
}

__device__ __forceinline__ const float* storage_row(const Operand& o, int row) {
    return row < o.split ? o.p0 + (int64_t)row * o.ld : o.p1 + (int64_t)(row - o.split) * o.ld;
}

template <int KIND>
__device__ __forceinline__ f32x4 load_operand(const GemmLaunch& L, const Operand& o, int i, int k0, int K) {
    f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
    if (i >= o.rows) return v;
    if (i == o.ones_row) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = k0 + e < K ? 1.0f : 0.0f;
        return v;
    }
    if constexpr (KIND == OP_DIRECT) {
        const float* row = storage_row(o, i);
        if (o.vec && k0 + 3 < K) return *reinterpret_cast<const f32x4*>(row + k0);
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (k0 + e < K) v[e] = row[k0 + e];
    } else if constexpr (KIND == OP_TRANS) {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (k0 + e < K) v[e] = storage_row(o, k0 + e)[i];
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (k0 + e < K) v[e] = o.gather_trans ? input_at(L, k0 + e, i) : input_at(L, i, k0 + e);
    }
    return v;
}

// Whether a lane's 4 columns of chunk kb lie inside K on a row-contiguous operand: one 16-byte load.
template <int KIND>
__device__ __forceinline__ bool staged_vec(const Operand& o, int kb, int K) {
    return KIND == OP_DIRECT && o.vec && kb + 16 <= K;
}

// Branch-free operand loads (OP_DIRECT / OP_TRANS): every lane loads from a valid address -- its own
// element, or the operand's first element where it has none -- and the value is masked once all of
// the chunk's loads are in flight (mask_raw). load_operand's guarded loads compile to divergent
// branches, and hipcc closes each join with vmcnt(0): one memory round trip per fragment.
template <int KIND>
__device__ __forceinline__ f32x4 load_raw(const Operand& o, int i, int kb, int k0, int K) {
    const bool row_ok = i < o.rows && i != o.ones_row;
    if (staged_vec<KIND>(o, kb, K)) {
        const float* g = row_ok ? storage_row(o, i) + k0 : o.p0;
        return *reinterpret_cast<const f32x4*>(g);
    }
    f32x4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float* g = o.p0;
        if (row_ok && k0 + e < K) {
            if constexpr (KIND == OP_DIRECT) g = storage_row(o, i) + k0 + e;
            else g = storage_row(o, k0 + e) + i;
        }
        v[e] = *g;
    }
    return v;
}

template <int KIND>
__device__ __forceinline__ f32x4 mask_raw(const Operand& o, int i, int kb, int k0, int K, f32x4 v) {
    if (i >= o.rows) return f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    if (i == o.ones_row) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = k0 + e < K ? 1.0f : 0.0f;
        return v;
    }
    if (!staged_vec<KIND>(o, kb, K))
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (!(k0 + e < K)) v[e] = 0.0f;
    return v;
}

// The gathered batch input, kept for the layer-0 weight gradient (fwd0 writes it as it loads it).
__device__ __forceinline__ void stash_input(const GemmLaunch& L, const GemmDesc& D, const f32x4& v, int m, int k0) {
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (m < D.M && k0 + e < D.K) L.xstore[(int64_t)m * D.K + k0 + e] = v[e];
}

template <int NW, int TMX, int DI>
__device__ __forceinline__ void fold_dw0(const GemmLaunch& L, int tm, int n0, float (*red)[TT * TMX][TT + 1],
                                         const float (*xs)[FOLD_K0MAX]);
template <int NW>
__device__ __forceinline__ void fold_sum(const GemmLaunch& L, int n0);

// A tagged granule {value, tag}: one 8-byte store, read untorn (MI355X_MICROARCH.md, granules)
__device__ __forceinline__ unsigned long long granule(float v, unsigned tag) {
    return ((unsigned long long)tag << 32) | __float_as_uint(v);
}


// One lane polls an arrival counter (sc1 loads) until it reaches `need`, then the workgroup goes on.
// Used only where the awaited workgroups have lower ids than the waiter (dispatched before it), so the
// wait always ends; the 1 s bound (s_memrealtime, 100 MHz) turns a broken assumption into bit 0 of
// *status instead of a hang.
__device__ __forceinline__ void wait_arrivals(const unsigned* counter, unsigned need, unsigned* status) {
    if (threadIdx.x == 0) {
        const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
        while (__hip_atomic_load(counter, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < need) {
            if (__builtin_amdgcn_s_memrealtime() - t0 > 100000000ull) {
                if (status) atomicOr(status, 1u);
                break;
            }
            __builtin_amdgcn_s_sleep(2);
        }
    }
    __syncthreads();
}

// TMX = 1: 32 x 32 C tiles; TMX = 2: 64 x 32 (the W x W backward products, so that a launch's tiles
// fit one round of the CUs). Each element's K order is the same for both (the K split over the waves
// depends on K and NW only), so the tile height never changes a bit of the result.
// DI: which of the launch's products, a constant index into the kernel arguments. Always inlined: a
// call that is not would take the argument block's address, and the compiler copies the whole block
// (1.5 KB) to scratch per lane for that (the 4-wave backward launch did until r04).
// PLAIN (the ensemble launches, train_gemm_ens_kernel): the tile of the multi-launch layout only -- no
// in-place Adam step, no dW_0 fold, no ticket, granule or wait of any kind is compiled in.
template <int NW, int AK, int BK, int TMX, int DI, bool PLAIN = false>
__device__ __forceinline__ void gemm_tile(const GemmLaunch& L, int tile, float (*red)[TT * TMX][TT + 1],
                                          float (*xs)[FOLD_K0MAX]) {
    const GemmDesc& D = L.d[DI];
    constexpr int NT = 64 * NW;
    constexpr int TM = TT * TMX;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, q = lane >> 4, c = lane & 15;
    const int tm = tile / D.tiles_n, m0 = tm * TM, n0 = (tile % D.tiles_n) * TT;
    const bool stash = AK == OP_GATHER && L.xstore != nullptr && n0 == 0;
    // wave w takes the w-th of NW contiguous K ranges (in 16-deep chunks): a few chunks per wave, so
    // the loads' latency is paid about once per wave instead of once per chunk
    const int chunks = (D.K + 15) >> 4, per = (chunks + NW - 1) / NW;
    const int kb0 = wave * per * 16, kb1 = min(D.K, (wave + 1) * per * 16);
    f32x4 acc[2 * TMX][2];
#pragma unroll
    for (int x = 0; x < 2 * TMX; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y) acc[x][y] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    // the epilogue's own operands (bias, ReLU mask, loss targets) are fetched before the K loop so
    // their latency overlaps the products'
    const Output& O = D.out;
    constexpr int EPT = TM * TT / NT;       // C elements per thread in the epilogue
    float pre[EPT], ap[EPT], am[EPT], av[EPT];
#pragma unroll
    for (int j = 0; j < EPT; ++j) {
        const int e = tid + j * NT, m = m0 + (e >> 5), n = n0 + (e & 31);
        pre[j] = ap[j] = am[j] = av[j] = 0.0f;
        if (m >= D.M || n >= D.N) continue;
        if (O.mode == EPI_ACT) pre[j] = n < O.bsplit ? O.b0[n] : O.b1[n - O.bsplit];
        else if (O.mode == EPI_MASK) pre[j] = O.mask[(int64_t)m * O.ldm + n];
        else if (!PLAIN && O.mode == EPI_GRAD && O.adam) {   // the in-place Adam step's operands (only this tile
            const int64_t i = (int64_t)m * O.ldc + n;   // writes them; the weight is only read by others)
            ap[j] = O.aw.param[i];
            am[j] = O.aw.exp_avg[i];
            av[j] = O.aw.exp_avg_sq[i];
        }
        else if (O.mode == EPI_LOSS) {
            const int64_t src = batch_row(L, m);
            const float t = n < O.s ? L.gns[src * O.s + n] : L.grw[src];
            pre[j] = t - (n < O.bsplit ? O.b0[n] : O.b1[n - O.bsplit]);   // y - t = acc - (t - bias)
        }
    }
    // the dW_0 fold's operand, the tile's rows of the gathered input: loaded now, into LDS after the
    // K loop (its latency then hides behind the products')
    constexpr int XPT = TM * FOLD_K0MAX / NT;
    float xv[XPT];
    const bool xstage = !PLAIN && O.mode == EPI_MASK && O.fold && O.fold_k0 <= FOLD_K0MAX;
    if (xstage) {
#pragma unroll
        for (int j = 0; j < XPT; ++j) {
            const int e = tid + j * NT, r = e / FOLD_K0MAX, k = e % FOLD_K0MAX;
            xv[j] = (k < O.fold_k0 && m0 + r < D.M) ? O.fold_x[(int64_t)(m0 + r) * O.fold_k0 + k] : 0.0f;
        }
    }
    // (stamp slots: 0 entry, 1 K loop done, 2 after the reduction barrier / arrival wait, 3 exit)
    // up to GROUP chunks' operands in flight at once, then their MFMAs: with the usual 1-4 chunks
    // per wave the loads' latency is paid once
    constexpr int GROUP = NW == 16 ? (TMX == 2 ? 1 : 2) : NW == 8 ? 2 : 4;   // TMX 2 at 16 waves: the 128-VGPR budget
    int g0 = kb0;
    constexpr bool RAW = AK != OP_GATHER && BK != OP_GATHER;   // branch-free loads (load_raw / mask_raw)
    for (; g0 < kb1; g0 += 16 * GROUP) {
        f32x4 a[GROUP][2 * TMX], b[GROUP][2];
#pragma unroll
        for (int u = 0; u < GROUP; ++u) {
            const int kb = g0 + 16 * u;
            if (kb >= kb1) break;
            if constexpr (RAW) {
#pragma unroll
                for (int x = 0; x < 2 * TMX; ++x) a[u][x] = load_raw<AK>(D.A, m0 + 16 * x + c, kb, kb + 4 * q, D.K);
#pragma unroll
                for (int y = 0; y < 2; ++y) b[u][y] = load_raw<BK>(D.B, n0 + 16 * y + c, kb, kb + 4 * q, D.K);
            } else {
#pragma unroll
                for (int x = 0; x < 2 * TMX; ++x) {
                    a[u][x] = load_operand<AK>(L, D.A, m0 + 16 * x + c, kb + 4 * q, D.K);
                    if (stash) stash_input(L, D, a[u][x], m0 + 16 * x + c, kb + 4 * q);
                }
#pragma unroll
                for (int y = 0; y < 2; ++y) b[u][y] = load_operand<BK>(L, D.B, n0 + 16 * y + c, kb + 4 * q, D.K);
            }
        }
        if constexpr (RAW) {
#pragma unroll
            for (int u = 0; u < GROUP; ++u) {   // the masks, once every load of the group is in flight
                const int kb = g0 + 16 * u;
                if (kb >= kb1) break;
#pragma unroll
                for (int x = 0; x < 2 * TMX; ++x) a[u][x] = mask_raw<AK>(D.A, m0 + 16 * x + c, kb, kb + 4 * q, D.K, a[u][x]);
#pragma unroll
                for (int y = 0; y < 2; ++y) b[u][y] = mask_raw<BK>(D.B, n0 + 16 * y + c, kb, kb + 4 * q, D.K, b[u][y]);
            }
        }
#pragma unroll
        for (int u = 0; u < GROUP; ++u) {
            if (g0 + 16 * u >= kb1) break;
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int x = 0; x < 2 * TMX; ++x)
#pragma unroll
                    for (int y = 0; y < 2; ++y)
                        acc[x][y] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u][x][s], b[u][y][s], acc[x][y], 0, 0, 0);
        }
    }
    TSTAMP(1);
    // lane l holds C rows 16x + 4q + v, column 16y + c
#pragma unroll
    for (int x = 0; x < 2 * TMX; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y)
#pragma unroll
            for (int v = 0; v < 4; ++v) red[wave][16 * x + 4 * q + v][16 * y + c] = acc[x][y][v];
    if (xstage) {
#pragma unroll
        for (int j = 0; j < XPT; ++j) {
            const int e = tid + j * NT;
            xs[e / FOLD_K0MAX][e % FOLD_K0MAX] = xv[j];
        }
    }
    __syncthreads();
    // every wave's K loop is done: this tile no longer reads the weight block (its loads were consumed)
    if constexpr (!PLAIN) {
        if (O.mode == EPI_MASK && O.arrive_ticket && tid == 0)
            __hip_atomic_fetch_add(O.arrive_ticket + n0 / TT, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);

        if (O.mode == EPI_GRAD && O.adam && O.wait_ticket)
            wait_arrivals(O.wait_ticket + n0 / TT, O.wait_count, O.wait_status);
    }
    TSTAMP(2);

    // the fused epilogue, EPT C elements per thread; each element sums the waves' partials in wave
    // order. Elements of this tile that feed the next layer's bias gradient (EPI_MASK, EPI_LOSS)
    // are kept for the column sums below.
    float loss_s = 0.0f, loss_r = 0.0f;
    float keep[EPT];
#pragma unroll
    for (int j = 0; j < EPT; ++j) {
        const int e = tid + j * NT, row = e >> 5, col = e & 31, m = m0 + row, n = n0 + col;
        keep[j] = 0.0f;
        if (m >= D.M || n >= D.N) continue;
        float v = red[0][row][col];
#pragma unroll
        for (int w = 1; w < NW; ++w) v = v + red[w][row][col];
        if (O.mode == EPI_ACT) v = v + pre[j];
        if (O.mode == EPI_ACT && O.relu) v = v > 0.0f ? v : 0.0f;
        if (O.mode == EPI_MASK && !(pre[j] > 0.0f)) v = 0.0f;
        if (O.mode == EPI_LOSS) {
            const float d = v - pre[j];
            if (n < O.s) loss_s = loss_s + d * d * O.inv_s;
            else loss_r = loss_r + d * d * O.inv_r;
            v = d * (n < O.s ? O.scale_s : O.scale_r);
        }
        keep[j] = v;
        // (with the dW_0 fold nothing reads dH_0 after this launch: its tiles keep it in LDS only)
        if (PLAIN || !(O.mode == EPI_MASK && O.fold)) {
            float* dst = m < O.split ? O.c0 + (int64_t)m * O.ldc : O.c1 + (int64_t)(m - O.split) * O.ldc;
            dst[n] = v;
        }
        if (!PLAIN && O.mode == EPI_GRAD && O.adam) {
            const int64_t i = (int64_t)m * O.ldc + n;
            adam_element(ap[j], v, am[j], av[j], O.aw.step_size, O.aw.bc2_sqrt, L.hp, L.arith);
            O.aw.param[i] = ap[j];
            O.aw.exp_avg[i] = am[j];
            O.aw.exp_avg_sq[i] = av[j];
        }
    }
    // EPI_GRAD: the first column tile also finishes the bias gradient of each row m from the column
    // sums the launch that produced this layer's output gradient left per row tile
    if (O.mode == EPI_GRAD && O.colsum_in && n0 == 0 && tid < TM && m0 + tid < D.M) {
        const int m = m0 + tid;
        const float g = ordered_sum<false>(O.colsum_in + m, D.M, O.colsum_tiles);
        (m < O.split ? O.g0[m] : O.g1[m - O.split]) = g;
        if (!PLAIN && O.adam)
            adam_element(O.ab.param[m], g, O.ab.exp_avg[m], O.ab.exp_avg_sq[m], O.ab.step_size, O.ab.bc2_sqrt, L.hp,
                         L.arith);
    }
    if (O.mode == EPI_MASK || O.mode == EPI_LOSS) {   // per-32-row-tile column sums (the next bias gradient)
        __syncthreads();
#pragma unroll
        for (int j = 0; j < EPT; ++j) {
            const int e = tid + j * NT;
            red[0][e >> 5][e & 31] = keep[j];
        }
        __syncthreads();
        const int sub = tid / TT, col = tid - (tid / TT) * TT;
        if (tid < TM && n0 + col < D.N && m0 + TT * sub < D.M) {
            float t = red[0][TT * sub][col];
            for (int r = 1; r < TT; ++r) t = t + red[0][TT * sub + r][col];
            const int64_t di = (int64_t)(tm * TMX + sub) * D.N + n0 + col;
            if constexpr (PLAIN) {
                O.colsum_out[di] = t;
            } else {
                if (O.fold)   // read by fold_sum (dW_1 tile (0, n0 / 32)) as a tagged granule
                    __hip_atomic_store(O.cs_gran + di, granule(t, *O.fold_serial), __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_AGENT);
                else
                    O.colsum_out[di] = t;
            }
        }
        if constexpr (!PLAIN)
            if (O.mode == EPI_MASK && O.fold) fold_dw0<NW, TMX, DI>(L, tm, n0, red, xs);
    }
    if constexpr (!PLAIN)
        if (O.mode == EPI_GRAD && O.fold_sum && tm == 0) fold_sum<NW>(L, n0);
    if (O.mode == EPI_LOSS) {   // the tile's loss: a butterfly per wave, then the waves in order
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            loss_s += __shfl_xor(loss_s, o);
            loss_r += __shfl_xor(loss_r, o);
        }
        __syncthreads();        // red is reused
        float* sl = &red[1][0][0];
        if (lane == 0) {
            sl[2 * wave] = loss_s;
            sl[2 * wave + 1] = loss_r;
        }
        __syncthreads();
        if (tid < 2) {
            float t = sl[tid];
            for (int w = 1; w < NW; ++w) t = t + sl[2 * w + tid];
            O.loss_part[tile * 2 + tid] = t;
        }
    }
    TSTAMP(3);
}

// The layer-0 weight gradient folded into the dH_0 launch (Output.fold). red[0] holds this tile's
// dH_0 rows [m0, m0 + TM) x columns [n0, n0 + 32) (the EPI_MASK column-sum staging). The separate
// dW_0 launch (M = W, N = K0, K = R, fold_nw waves of 32 rows each) computed, per wave tr, one 32 x 32
// block of dW_0 over rows [32 tr, 32 tr + 32) with acc[x][y] over 16-row chunks u, k = 4 q + s: the
// same loads and MFMAs in the same order run here per 32-row half of the tile, so every partial is
// the same float; they leave as tagged granules, and fold_sum (a dW_1 tile of the same launch) adds
// them in wave order with the empty waves' +0 -- the separate launch's result bit for bit.
template <int NW, int TMX, int DI>
__device__ __forceinline__ void fold_dw0(const GemmLaunch& L, int tm, int n0, float (*red)[TT * TMX][TT + 1],
                                         const float (*xs)[FOLD_K0MAX]) {
    const GemmDesc& D = L.d[DI];
    constexpr int TM = TT * TMX;
    (void)TM;
    const Output& O = D.out;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, q = lane >> 4, c = lane & 15;
    const int R = D.M, W = D.N, K0 = O.fold_k0, m0 = tm * TT * TMX;
    const int kt = (K0 + TT - 1) / TT;
    const unsigned tag = *O.fold_serial;
    for (int task = wave; task < TMX * kt; task += NW) {
        const int h = task / kt, kb = task - (task / kt) * kt;
        const int r0 = m0 + TT * h;
        if (r0 >= R) continue;
        const int r1 = min(R, r0 + TT);
        f32x4 acc[2][2];
#pragma unroll
        for (int x = 0; x < 2; ++x)
#pragma unroll
            for (int y = 0; y < 2; ++y) acc[x][y] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int k0 = r0 + 16 * u;
            if (k0 >= r1) break;
            f32x4 a[2], b[2];
#pragma unroll
            for (int x = 0; x < 2; ++x) {          // A(i = j, k = r) = dH_0[r][j]
                const int j = 16 * x + c;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int r = k0 + 4 * q + e;
                    a[x][e] = (n0 + j < W && r < R) ? red[0][r - m0][j] : 0.0f;
                }
            }
#pragma unroll
            for (int y = 0; y < 2; ++y) {          // B(i = k, k = r) = X[r][k]
                const int kk = TT * kb + 16 * y + c;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int r = k0 + 4 * q + e;
                    b[y][e] = (kk < K0 && r < R) ? (K0 <= FOLD_K0MAX ? xs[r - m0][kk] : O.fold_x[(int64_t)r * K0 + kk])
                                                 : 0.0f;
                }
            }
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int x = 0; x < 2; ++x)
#pragma unroll
                    for (int y = 0; y < 2; ++y)
                        acc[x][y] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[x][s], b[y][s], acc[x][y], 0, 0, 0);
        }
        const int tr = r0 / TT;
#pragma unroll
        for (int x = 0; x < 2; ++x)
#pragma unroll
            for (int y = 0; y < 2; ++y)
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const int j = n0 + 16 * x + 4 * q + v, kk = TT * kb + 16 * y + c;
                    if (j < W && kk < K0)    // read by fold_sum as a tagged granule: nothing to drain
                        __hip_atomic_store(O.fold_gran + ((int64_t)tr * W + j) * K0 + kk, granule(acc[x][y][v], tag),
                                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
    }
}

// The fold's sums, in the dW_1 tile (0, n0 / 32) of the same launch (higher workgroup ids than every
// dH_0 tile, so those were dispatched first and always finish): the column block's per-32-row partials
// added in wave order with the empty waves' +0 -- the separate dW_0 launch's sum, bit for bit -- and
// db_0 from the column sums over the 32-row tiles, then layer 0's Adam step. Each lane loads all of its
// granules at once and reloads the ones whose tag is not yet this step's (bounded: 1 s, then bit 0 of
// the status word).
template <int NW>
__device__ __forceinline__ bool poll_granules(const unsigned long long* const* p, int n, unsigned tag, float* out,
                                              unsigned* status) {
    unsigned long long g[16];
    unsigned need = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        out[i] = 0.0f;
        if (i < n) need |= 1u << i;
    }
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    while (need) {
#pragma unroll
        for (int i = 0; i < 16; ++i)
            g[i] = ((need >> i) & 1u) ? __hip_atomic_load(p[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0ull;
#pragma unroll
        for (int i = 0; i < 16; ++i)
            if (((need >> i) & 1u) && (unsigned)(g[i] >> 32) == tag) {
                out[i] = __uint_as_float((unsigned)g[i]);
                need &= ~(1u << i);
            }
        if (!need) break;
        if (__builtin_amdgcn_s_memrealtime() - t0 > 100000000ull) {
            if (status) atomicOr(status, 1u);
            return false;
        }
        __builtin_amdgcn_s_sleep(1);
    }
    return true;
}

template <int NW>
__device__ __forceinline__ void fold_sum(const GemmLaunch& L, int n0) {
    const GemmDesc& D = L.d[0];
    const Output& O = D.out;
    const int tid = threadIdx.x;
    const int R = D.M, W = D.N, K0 = O.fold_k0;
    const int ntr = (R + TT - 1) / TT;      // non-empty waves of the separate launch
    const unsigned tag = *O.fold_serial;
    constexpr int NT = 64 * NW;
    const bool dbt = tid < TT && n0 + tid < W;
    // the Adam operands of this column block first: their latency overlaps the polls
    float bp = 0.0f, bm = 0.0f, bv = 0.0f;
    if (O.fold_adam && dbt) {
        bp = O.fold_ab.param[n0 + tid];
        bm = O.fold_ab.exp_avg[n0 + tid];
        bv = O.fold_ab.exp_avg_sq[n0 + tid];
    }
    for (int e0 = 0; e0 < TT * K0; e0 += NT) {
        const int e = e0 + tid, j = n0 + e / K0, kk = e - (e / K0) * K0;
        const bool in = e < TT * K0 && j < W;
        const int64_t i = (int64_t)j * K0 + kk;
        float fp = 0.0f, fm = 0.0f, fv = 0.0f;
        if (in && O.fold_adam) {
            fp = O.fold_aw.param[i];
            fm = O.fold_aw.exp_avg[i];
            fv = O.fold_aw.exp_avg_sq[i];
        }
        const unsigned long long* ptr[16];
        const int np = in ? min(ntr, O.fold_nw) : 0;
#pragma unroll
        for (int w = 0; w < 16; ++w) ptr[w] = O.fold_gran + ((int64_t)min(w, max(np - 1, 0)) * W + j) * K0 + kk;
        float p[16];
        poll_granules<NW>(ptr, np, tag, p, O.fold_status);
        if (!in) continue;
        float v = p[0];
#pragma unroll
        for (int w = 1; w < 16; ++w)
            if (w < O.fold_nw) v = v + p[w];
        O.fold_dw[i] = v;
        if (O.fold_adam) {
            adam_element(fp, v, fm, fv, O.fold_aw.step_size, O.fold_aw.bc2_sqrt, L.hp, L.arith);
            O.fold_aw.param[i] = fp;
            O.fold_aw.exp_avg[i] = fm;
            O.fold_aw.exp_avg_sq[i] = fv;
        }
    }
    if (tid < 64) {                          // db_0: the column sums of dH_0 over the 32-row tiles
        const int j = n0 + tid;
        const unsigned long long* ptr[16];
        const int np = dbt ? min(O.fold_cs_tiles, 16) : 0;
#pragma unroll
        for (int i = 0; i < 16; ++i) ptr[i] = O.cs_gran + (int64_t)min(i, max(np - 1, 0)) * W + min(j, W - 1);
        float cs[16];
        poll_granules<NW>(ptr, np, tag, cs, O.fold_status);
        if (dbt) {
            float g = cs[0];
#pragma unroll
            for (int i = 1; i < 16; ++i)
                if (i < O.fold_cs_tiles) g = g + cs[i];
            O.fold_db[j] = g;
            if (O.fold_adam) {
                adam_element(bp, g, bm, bv, O.fold_ab.step_size, O.fold_ab.bc2_sqrt, L.hp, L.arith);
                O.fold_ab.param[j] = bp;
                O.fold_ab.exp_avg[j] = bm;
                O.fold_ab.exp_avg_sq[j] = bv;
            }
        }
    }
}

// The loss workgroup: partials of the output-layer launch, summed in tile order into loss_out[0..2].
__device__ __forceinline__ void loss_workgroup(const GemmLaunch& L) {
    if (threadIdx.x < 2 && L.loss_out) {   // (loads 16 at a time in flight, sums in the same order)
        float t = 0.0f, u = 0.0f;
        for (int i0 = 0; i0 < L.loss_parts; i0 += 16) {
            float ps[16], pr[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const bool in = i0 + k < L.loss_parts;
                ps[k] = in ? L.loss_part[(i0 + k) * 2] : 0.0f;
                pr[k] = in ? L.loss_part[(i0 + k) * 2 + 1] : 0.0f;
            }
#pragma unroll
            for (int k = 0; k < 16; ++k)
                if (i0 + k < L.loss_parts) {
                    t = t + (threadIdx.x == 0 ? ps[k] : pr[k]);
                    u = u + ps[k] + pr[k];
                }
        }
        L.loss_out[1 + threadIdx.x] = t;
        if (threadIdx.x == 0) L.loss_out[0] = u;
    }
}

// NW waves per workgroup; A0/B0 (A1/B1): operand kinds of the launch's first (second) product, fixed
// at compile time so each instantiation carries only its own load paths.
template <int NW, int A0, int B0, int A1, int B1, int TMX>
__global__ __launch_bounds__(64 * NW) void train_gemm_kernel(const GemmLaunch L) {
    __shared__ __attribute__((aligned(16))) float red[NW][TT * TMX][TT + 1];   // (16-B: the staged chunk's slots)
    __shared__ float xs[TT * TMX][FOLD_K0MAX];   // the dW_0 fold's input rows (dH_0 launches only)
    TSTAMP(0);
    // (constant indices only: a dynamic index into the kernel arguments would copy them to scratch)
    const int b = blockIdx.x;
    if (b == 0 && L.zero_words)
        for (int i = threadIdx.x; i < L.zero_n; i += 64 * NW) L.zero_words[i] = 0u;
    if (b == 0 && L.serial && threadIdx.x == 0) *L.serial = *L.serial + 1u;
    if (b < L.d[0].tiles) {
        int tile = b;
        if (L.xcd) {   // block b on XCD b % 8 (round-robin dispatch) takes a tile of a 64-row band of that XCD
            constexpr int G = 2 / TMX;                    // tile rows per 64-row band
            const int tn_all = L.d[0].tiles_n, per = G * tn_all, x = b & 7, j = b >> 3;
            const int u = j / per, r = j - u * per;
            tile = ((x + 8 * u) * G + r / tn_all) * tn_all + r % tn_all;
        }
        gemm_tile<NW, A0, B0, TMX, 0>(L, tile, red, xs);
        return;
    }
    int r = b - L.d[0].tiles;
    if constexpr (A1 >= 0) {
        if (L.nd > 1 && r < L.d[1].tiles) {
            gemm_tile<NW, A1, B1, TMX, 1>(L, r, red, xs);
            return;
        }
        if (L.nd > 1) r -= L.d[1].tiles;
    }
    if (r < L.adam_blocks) {    // fused Adam: ADAM_FUSED_CHUNK elements of one tensor per workgroup
        int ti = 0;
        while (ti + 1 < L.adam_count && r >= L.adam_first[ti + 1]) ++ti;
        const mbrl_adam_tensor& T = L.adam_t[ti];
        const int64_t base = (int64_t)(r - L.adam_first[ti]) * L.adam_chunk;
        for (int64_t i = base + threadIdx.x; i < T.numel && i < base + L.adam_chunk; i += 64 * NW)
            adam_element(T.param[i], T.grad[i], T.exp_avg[i], T.exp_avg_sq[i], T.step_size, T.bc2_sqrt, L.hp,
                         L.arith);
        return;
    }
    loss_workgroup(L);
}

// ================================================================================================
// Ensemble training (mbrl_train_grads_ensemble / mbrl_train_epoch_ensemble): E members of one shape in
// the launches of the multi-launch layout, the member on grid axis y. Workgroup (x, e) runs exactly
// the tile x of member e's own launch -- the same loads, MFMA chains and sums in the same order -- so
// member e's gradients and losses are a single-model call's bit for bit. The launch struct is member
// 0's; the kernel moves every workspace pointer by e workspaces and the batch's rows by e orders, and
// takes the member's parameter and gradient pointers (at most ENS_MODEL_PTRS per launch) from a table.
// Nothing in these launches waits on another workgroup (gemm_tile's PLAIN form): every hand-off is a
// kernel boundary on the stream, so any number of members' tiles may queue behind the CUs.
constexpr int ENS_MODEL_PTRS = 6;

struct EnsLaunch {
    GemmLaunch g;          // member 0's launch
    int64_t ws_stride;     // floats between two members' workspaces
    int64_t idx_stride;    // rows between two members' orders
    int loss_stride;       // floats between two members' loss_out
    // forward / output launches: B.p0, B.p1, out.b0, out.b1; backward: d[0].B.p0, d[0].B.p1 (layer >= 1),
    // then the weight-gradient product's out.c0, out.c1, out.g0, out.g1
    const float* mp[MBRL_TRAIN_MAX_MEMBERS][ENS_MODEL_PTRS];
};

template <class T>
__device__ __forceinline__ void ens_move(T*& p, int64_t by) {
    if (p) p += by;
}

// Member e's launch from member 0's. KIND: 0 forward / output layer, 1 backward of a layer >= 1 (dH and
// dW products), 2 backward of layer 0 (dW only).
template <int KIND>
__device__ __forceinline__ void ens_member(GemmLaunch& L, const EnsLaunch& P, int e) {
    const int64_t by = (int64_t)e * P.ws_stride;
    L.idx += (int64_t)e * P.idx_stride;
    ens_move(L.xstore, by);
    ens_move(L.loss_part, by);
    ens_move(L.loss_out, (int64_t)e * P.loss_stride);
    const float* m[ENS_MODEL_PTRS];
#pragma unroll
    for (int i = 0; i < ENS_MODEL_PTRS; ++i) {   // (constant indices into the kernel arguments only)
        m[i] = P.mp[0][i];
#pragma unroll
        for (int k = 1; k < MBRL_TRAIN_MAX_MEMBERS; ++k)
            if (e == k) m[i] = P.mp[k][i];
    }
    GemmDesc& D0 = L.d[0];
    if constexpr (KIND == 0) {
        ens_move(D0.A.p0, by);
        ens_move(D0.A.p1, by);
        D0.B.p0 = m[0]; D0.B.p1 = m[1];
        D0.out.b0 = m[2]; D0.out.b1 = m[3];
        ens_move(D0.out.c0, by);
        ens_move(D0.out.c1, by);
        ens_move(D0.out.colsum_out, by);
        ens_move(D0.out.loss_part, by);
    } else {
        constexpr int DG = KIND == 1 ? 1 : 0;     // the weight-gradient product
        if constexpr (KIND == 1) {
            ens_move(D0.A.p0, by);
            ens_move(D0.A.p1, by);
            D0.B.p0 = m[0]; D0.B.p1 = m[1];
            ens_move(D0.out.c0, by);
            ens_move(D0.out.c1, by);
            ens_move(D0.out.mask, by);
            ens_move(D0.out.colsum_out, by);
        }
        GemmDesc& G = L.d[DG];
        ens_move(G.A.p0, by);
        ens_move(G.A.p1, by);
        ens_move(G.B.p0, by);
        ens_move(G.B.p1, by);
        G.out.c0 = const_cast<float*>(m[2]); G.out.c1 = const_cast<float*>(m[3]);
        G.out.g0 = const_cast<float*>(m[4]); G.out.g1 = const_cast<float*>(m[5]);
        ens_move(G.out.colsum_in, by);
    }
}

template <int NW, int A0, int B0, int A1, int B1, int TMX>
__global__ __launch_bounds__(64 * NW) void train_gemm_ens_kernel(const EnsLaunch P) {
    __shared__ __attribute__((aligned(16))) float red[NW][TT * TMX][TT + 1];
    constexpr int KIND = B0 == OP_DIRECT ? 0 : A0 == OP_DIRECT ? 1 : 2;
    GemmLaunch L = P.g;
    int e = blockIdx.y, b = blockIdx.x;
#ifdef MBRL_ENS_XCD_MAJOR
    // Measurement build (profiles/train_ensemble): the members XCD-major instead of member-major. Workgroup
    // w = y * gridDim.x + x runs on XCD w % 8 (round-robin dispatch) as that XCD's (w / 8)-th; numbering the
    // workgroups XCD by XCD gives member e a contiguous run of them, so a member's tiles share one or two
    // XCDs' L2 and all members run side by side. A bijection when the grid is a multiple of 8; the same bits.
    {
        const unsigned gx = gridDim.x, total = gx * gridDim.y, w = blockIdx.y * gx + blockIdx.x;
        if ((total & 7u) == 0) {
            const unsigned v = (w & 7u) * (total >> 3) + (w >> 3);
            e = (int)(v / gx);
            b = (int)(v - (v / gx) * gx);
        }
    }
#endif
    ens_member<KIND>(L, P, e);
    TSTAMP(0);   // (member 0's workgroups only)
    if (b < L.d[0].tiles) {
        gemm_tile<NW, A0, B0, TMX, 0, true>(L, b, red, nullptr);
        return;
    }
    if constexpr (A1 >= 0) {
        if (L.nd > 1 && b - L.d[0].tiles < L.d[1].tiles) {
            gemm_tile<NW, A1, B1, TMX, 1, true>(L, b - L.d[0].tiles, red, nullptr);
            return;
        }
    }
    loss_workgroup(L);
}

static Operand direct(const float* p0, const float* p1, int split, int ld, int rows) {
    Operand o{};
    o.p0 = p0; o.p1 = p1 ? p1 : p0; o.split = p1 ? split : rows; o.ld = ld; o.kind = OP_DIRECT; o.rows = rows;
    o.ones_row = -1;
    o.vec = (ld % 4 == 0) && ((reinterpret_cast<uintptr_t>(p0) | reinterpret_cast<uintptr_t>(o.p1)) & 15) == 0;
    return o;
}

static Operand transposed(const float* p0, const float* p1, int split, int ld, int rows) {
    Operand o{};
    o.p0 = p0; o.p1 = p1 ? p1 : p0; o.split = p1 ? split : (1 << 30); o.ld = ld; o.kind = OP_TRANS; o.rows = rows;
    o.ones_row = -1;
    return o;
}

// The EPI_GRAD output of layer l: its weight gradient [n_out][n_in] and, from `colsum` [colsum_tiles][n_out]
// (NULL: finished elsewhere), its bias gradient. The output layer's rows are the state head's, then the reward
// head's where there is one.
static Output grad_output(const TrainShape& t, int l, float* const* weight_grad, float* const* bias_grad,
                          const float* colsum, int colsum_tiles) {
    const int l2 = (l == t.L && t.reward) ? t.L + 1 : l;
    Output O{};
    O.mode = EPI_GRAD; O.ldc = l == 0 ? t.s + t.a : t.W; O.colsum_in = colsum; O.colsum_tiles = colsum_tiles;
    O.c0 = weight_grad[l]; O.c1 = weight_grad[l2]; O.split = l == t.L ? t.s : t.W;
    O.g0 = bias_grad[l]; O.g1 = bias_grad[l2];
    return O;
}

static void finish(GemmDesc& D, int M, int N, int K, int tmx = 1) {
    D.M = M; D.N = N; D.K = K;
    D.tiles_n = (N + TT - 1) / TT;
    D.tiles = ((M + TT * tmx - 1) / (TT * tmx)) * D.tiles_n;
}

// 16 waves split a long K (the hidden layers, every weight gradient); 4 suffice for short ones; 8 where
// the longest K is a weight gradient's batch rows in (128, 256) -- each wave then sums 32 rows, the
// row tile of the fused step's folds (launch_waves; fold_waves follows the same rule).
// TMX: the C tile height of every product of the launch (finish() with the same tmx).
static int launch_waves(const GemmLaunch& L) {
    int kmax = 0;
    bool grad_rows = false;
    for (int i = 0; i < L.nd; ++i) kmax = max(kmax, L.d[i].K);
    for (int i = 0; i < L.nd; ++i) grad_rows = grad_rows || (L.d[i].out.mode == EPI_GRAD && L.d[i].K == kmax);
    return kmax >= 256 ? 16 : (kmax > 128 && grad_rows) ? 8 : 4;
}

// One launch at nw waves: launch(NW) gets the wave count as a std::integral_constant to instantiate its kernel
// with. 64-row tiles (TMX == 2) are chosen only for long K (launch_train_grads): 16 waves.
template <int TMX, class Launch>
static hipError_t launch_at_waves(int nw, Launch launch) {
    if (TMX == 2 && nw != 16) return hipErrorInvalidValue;
    if (nw == 16) launch(std::integral_constant<int, 16>{});
    if constexpr (TMX == 1) {
        if (nw == 8) launch(std::integral_constant<int, 8>{});
        else if (nw != 16) launch(std::integral_constant<int, 4>{});
    }
    return hipGetLastError();
}

template <int A0, int B0, int A1 = -1, int B1 = -1, int TMX = 1>
static hipError_t launch_gemm(GemmLaunch& L, bool loss_wg, hipStream_t stream) {
    int blocks = loss_wg ? 1 : 0;
    for (int i = 0; i < L.nd; ++i) blocks += L.d[i].tiles;
    const int nw = launch_waves(L);
    // fused Adam blocks: chunks of 4 elements per thread of the launch's workgroup size
    const int chunk = 64 * nw * 4;
    L.adam_chunk = chunk;
    L.adam_blocks = 0;
    for (int i = 0; i < L.adam_count; ++i) {
        L.adam_first[i] = L.adam_blocks;
        L.adam_blocks += (int)((L.adam_t[i].numel + chunk - 1) / chunk);
    }
    L.adam_first[L.adam_count] = L.adam_blocks;
    blocks += L.adam_blocks;
    if (!loss_wg) L.loss_out = nullptr;
    ++L.slot;
    // XCD order needs whole groups of 8 64-row bands (a bijection of the tiles)
    const int tiles_m0 = L.d[0].tiles / L.d[0].tiles_n;
    L.xcd = L.xcd && (tiles_m0 % (8 * (2 / TMX)) == 0);
    return launch_at_waves<TMX>(nw, [&](auto NW) {
        hipLaunchKernelGGL((train_gemm_kernel<NW.value, A0, B0, A1, B1, TMX>), dim3(blocks), dim3(64 * NW.value), 0,
                           stream, L);
    });
}

// The same launch for every member of an ensemble (train_gemm_ens_kernel), or launch_gemm without one.
// `layer`: the Linear whose parameters (forward) or gradients (backward) the launch touches.
template <int A0, int B0, int A1 = -1, int B1 = -1, int TMX = 1>
static hipError_t launch_gemm_any(GemmLaunch& G, bool loss_wg, hipStream_t stream, const TrainEnsemble* ens,
                                  const TrainShape& t, int layer) {
    if (!ens) return launch_gemm<A0, B0, A1, B1, TMX>(G, loss_wg, stream);
    if (ens->E < 1 || ens->E > MBRL_TRAIN_MAX_MEMBERS || G.adam_count != 0) return hipErrorInvalidValue;
    constexpr int KIND = B0 == OP_DIRECT ? 0 : A0 == OP_DIRECT ? 1 : 2;
    EnsLaunch P{};
    const bool heads = layer == t.L && t.reward;   // the output layer's second storage block: the reward head
    bool vec = true;
    for (int e = 0; e < ens->E; ++e) {
        const mbrl_train_model& m = ens->members[e];
        const int l2 = heads ? t.L + 1 : layer;
        if (KIND == 0) {
            P.mp[e][0] = m.weight[layer]; P.mp[e][1] = m.weight[l2];
            P.mp[e][2] = m.bias[layer]; P.mp[e][3] = m.bias[l2];
            vec = vec && ((reinterpret_cast<uintptr_t>(m.weight[layer]) | reinterpret_cast<uintptr_t>(m.weight[l2])) & 15) == 0;
        } else {
            P.mp[e][0] = m.weight[layer]; P.mp[e][1] = m.weight[l2];
            P.mp[e][2] = m.weight_grad[layer]; P.mp[e][3] = m.weight_grad[l2];
            P.mp[e][4] = m.bias_grad[layer]; P.mp[e][5] = m.bias_grad[l2];
        }
    }
    if (KIND == 0 && !vec) G.d[0].B.vec = 0;   // one load path for all members (the values are the same)
    if (!loss_wg) G.loss_out = nullptr;
    G.xcd = 0;
    ++G.slot;
    P.g = G;
    P.ws_stride = ens->ws_stride; P.idx_stride = ens->idx_stride; P.loss_stride = ens->loss_stride;
    int blocks = loss_wg ? 1 : 0;
    for (int i = 0; i < G.nd; ++i) blocks += G.d[i].tiles;
    const dim3 grid(blocks, ens->E);
    return launch_at_waves<TMX>(launch_waves(G), [&](auto NW) {
        hipLaunchKernelGGL((train_gemm_ens_kernel<NW.value, A0, B0, A1, B1, TMX>), grid, dim3(64 * NW.value), 0, stream,
                           P);
    });
}

// Workspace (floats, each piece 256-byte aligned): hidden activations H_0..H_{L-1} [R][W], two
// backward buffers dH [R][W], dY [R][J], loss partials, the gathered input [R][s + a], and the
// per-row-tile column sums of dY [tiles][J] and of the two dH [tiles][W].
struct TrainWs {
    float* act[MBRL_TRAIN_MAX_LAYERS];
    float *dh[2], *dy, *loss_part, *xbuf, *cs_dy, *cs_dh[2];
    float *xbuf2, *tgt2;  // the fused step's second gather slot (the next batch's rows and targets)
    float* out_part;      // fused step: the output layer's weight-gradient partials [row tile][J][W]
    float* tgt;           // fused step: the batch's targets [R][J] (F gathers, O reads)
    unsigned* tickets;    // [ceil(W / 32)] each: (unused: the dW_0 fold's before its granules), the fused
                          // dH_0 tiles' W_1-read arrivals, the fused dW_out fold's
    unsigned* status;     // fused step: bit 0 = a bounded wait timed out (never expected)
    unsigned* bands;      // fused step, F and O in one launch: [row tiles][32] band counters (one line each)
    unsigned* serial;     // the step's serial: the dW_0 fold's granule tag (raised by each step's first launch)
    unsigned long long *fold_gran, *cs_gran;   // the fold's tagged partials [tr][W][K0] and column sums [tr][W]
    size_t floats;
};

static TrainWs train_ws(const TrainShape& t, int batch, float* base) {
    const size_t R = (size_t)batch * t.H, J = t.s + (t.reward ? 1 : 0), W = t.W, tiles_r = (R + TT - 1) / TT;
    const size_t tiles_out = tiles_r * ((J + TT - 1) / TT);
    auto up = [](size_t x) { return (x + 63) & ~(size_t)63; };
    TrainWs w{};
    size_t off = 0;
    auto take = [&](size_t n) { float* p = base ? base + off : nullptr; off += up(n); return p; };
    // the control words first, at offsets that depend on the model only: every batch of an epoch
    // (the short last one lays out its data areas for its own size) finds the tickets, the sticky
    // status word and the band counters where the others left them, zero between launches; the band
    // counters sized for the fused step's largest batch (FUSED_MAX_BANDS)
    // (tickets and band counters first: every training call zeroes them in one memset on entry, see
    // train_status_offset; the status word and the serial behind them keep their values)
    w.tickets = reinterpret_cast<unsigned*>(take(3 * ((W + TT - 1) / TT)));
    w.bands = reinterpret_cast<unsigned*>(take(32 * FUSED_MAX_BANDS));
    w.status = reinterpret_cast<unsigned*>(take(1));
    w.serial = reinterpret_cast<unsigned*>(take(1));
    for (int l = 0; l < t.L; ++l) w.act[l] = take(R * W);
    w.dh[0] = take(R * W);
    w.dh[1] = take(R * W);
    w.dy = take(R * J);
    w.loss_part = take(tiles_out * 2);
    w.xbuf = take(R * (t.s + t.a));
    w.cs_dy = take(tiles_r * J);
    w.cs_dh[0] = take(tiles_r * W);
    w.cs_dh[1] = take(tiles_r * W);
    w.out_part = take(tiles_r * J * W);
    w.tgt = take(R * J);
    w.xbuf2 = take(R * (t.s + t.a));
    w.tgt2 = take(R * J);
    w.fold_gran = reinterpret_cast<unsigned long long*>(take(2 * tiles_r * W * (size_t)(t.s + t.a)));
    w.cs_gran = reinterpret_cast<unsigned long long*>(take(2 * tiles_r * W));
    w.floats = off;
    return w;
}

size_t train_ws_floats(const TrainShape& t, int batch) { return train_ws(t, batch, nullptr).floats; }

// The status word's byte offset, which is also the size of what lies before it: the fused step's arrival
// tickets and band counters. Their protocol leaves them zero between launches, but a workspace that was never
// zeroed, or a step whose bounded wait timed out, would leave counts behind: mbrl_train_grads /
// mbrl_train_epoch clear them once per call (one memset of this many bytes). The sticky status word and the
// fold's serial lie behind them and are kept.
size_t train_status_offset(const TrainShape& t, int batch) {
    float* base = reinterpret_cast<float*>(static_cast<uintptr_t>(64));   // any aligned base: offsets only
    return (size_t)(reinterpret_cast<char*>(train_ws(t, batch, base).status) - reinterpret_cast<char*>(base));
}

// Whether the layer-0 weight gradient folds into the dH_0 launch bit-identically: its separate launch
// (M = W, K = R) gives each of its waves one 32-row block of the batch (16 waves at R >= 256, 8 in
// (128, 256), else 4: launch_waves).
static int fold_waves(const TrainShape& t, int R) {
    if (t.fold == 0 || t.L < 1) return 0;
    const int nw = R >= 256 ? 16 : R > 128 ? 8 : 4, chunks = (R + 15) / 16, per = (chunks + nw - 1) / nw;
    return per == 2 ? nw : 0;
}

// Whether the fused three-launch step applies (train_fused_*_kernel): two hidden layers, the dW_0
// fold (its 32-row waves are also the dW_out partials' row tiles), dY within one 32-column tile, the
// layer-0 input within one chunk per wave of its launch, H_0's tile rows within LDS.
static bool fused_step(const TrainShape& t, int fold_nw) {
    const int J = t.s + (t.reward ? 1 : 0), K0 = t.s + t.a;
    return t.split == 0 && t.L == 2 && fold_nw > 0 && J <= TT && K0 <= FUSED_K0MAX && t.W <= FUSED_WMAX;
}
static bool fused_step(const TrainShape& t, int fold_nw, int R) {
    return fused_step(t, fold_nw) && (R + TT - 1) / TT <= FUSED_MAX_BANDS;   // (fold_nw > 0 implies it)
}

bool train_fused_applies(const TrainShape& t, int batch) {
    return fused_step(t, fold_waves(t, batch * t.H), batch * t.H);
}

hipError_t launch_train_grads(const TrainShape& t, const TrainTensors& w, const int64_t* idx, int batch,
                              float* loss_out, float* ws, hipStream_t stream, const TrainStep& step) {
    const mbrl_adam_tensor *adam = step.adam, *prior = step.prior;
    const mbrl_adam_hparams* hp = step.hp;
    const int arith = step.arith, prior_n = step.prior_n;
    mbrl_adam_tensor* pending = step.pending;
    int* pending_n = step.pending_n;
    const TrainGather* gather = step.gather;
    const TrainEnsemble* ens = step.ens;
    const int R = batch * t.H, W = t.W, K0 = t.s + t.a, J = t.s + (t.reward ? 1 : 0), L = t.L;
    const int tiles_r = (R + TT - 1) / TT;
    const int fold_nw = fold_waves(t, R);
    const bool fused = fused_step(t, fold_nw, R);
    if (pending_n) *pending_n = 0;
    if ((prior_n > 0 && !prior) || prior_n > ADAM_FUSED_MAX || (adam && fold_nw && (!pending || !pending_n)))
        return hipErrorInvalidValue;
    // an ensemble runs the multi-launch layout only: gradients, no fold, no Adam step in the launches
    if (ens && (fused || fold_nw || adam || prior_n > 0)) return hipErrorInvalidValue;
    TrainWs B = train_ws(t, batch, ws);
    // the fused step's gather slot: the caller alternates them when F gathers the next batch
    float *xnext = B.xbuf2, *tnext = B.tgt2;
    if (fused && gather && gather->slot) {
        std::swap(B.xbuf, B.xbuf2);
        std::swap(B.tgt, B.tgt2);
        xnext = B.xbuf2;
        tnext = B.tgt2;
    }
    const float* wo_r = t.reward ? w.weight[L + 1] : nullptr;
    const float* bo_r = t.reward ? w.bias[L + 1] : w.bias[L];

    GemmLaunch G{};
    G.idx = idx; G.gs = w.states; G.ga = w.actions; G.gns = w.next_states; G.grw = w.rewards;
    const int xcd_opt = t.xcd;
    G.H = t.H; G.s = t.s; G.a = t.a;
    G.xstore = B.xbuf;
    G.slot = fused ? 1 : -1;   // diagnostic stamps: the fused step's F and O are slots 0 and 1
    if (adam) {
        G.hp = *hp;
        G.arith = arith;
    }
    hipError_t e;
    const int tiles_n = (W + TT - 1) / TT;
    if (fused) {   // F and O (train_fused_*_kernel); the backward launch below is B
        // a step the five-launch layout deferred (a smaller batch before this one): F reads W_1
        if (prior_n > 0 && (e = launch_adam_step(prior, prior_n, *hp, arith, stream)) != hipSuccess) return e;
        FusedArgs F{};
        F.idx = idx; F.gs = w.states; F.ga = w.actions; F.gns = w.next_states; F.grw = w.rewards;
        F.H = t.H; F.s = t.s; F.a = t.a;
        F.R = R; F.W = W; F.K0 = K0; F.J = J; F.tiles_n = tiles_n; F.tiles_r = tiles_r;
        F.nwb = fold_nw;
        F.w0 = w.weight[0]; F.b0 = w.bias[0]; F.w1 = w.weight[1]; F.b1 = w.bias[1];
        F.wo = w.weight[L]; F.wo_r = wo_r; F.bo = w.bias[L]; F.bo_r = bo_r;
        F.act0 = B.act[0]; F.act1 = B.act[1]; F.xstore = B.xbuf; F.tgt = B.tgt;
        if (gather) {   // (the workspace layout depends on the batch size: only equal batches hand over)
            F.pre_rows = gather->pre_rows;
            if (gather->idx_next && gather->batch_next == batch && tiles_n > 1) {
                F.idx_next = gather->idx_next;
                F.R_next = gather->batch_next * t.H;
                F.xnext = xnext;
                F.tnext = tnext;
            }
        }
        F.dh1 = B.dh[1]; F.cs_dh1 = B.cs_dh[1]; F.cs_dy = B.cs_dy; F.loss_part = B.loss_part;
        F.out_part = B.out_part;
        F.dwo = w.weight_grad[L]; F.dwo_r = t.reward ? w.weight_grad[L + 1] : w.weight_grad[L];
        F.dbo = w.bias_grad[L]; F.dbo_r = t.reward ? w.bias_grad[L + 1] : w.bias_grad[L];
        F.out_ticket = B.tickets + 2 * tiles_n;
        F.band = B.bands; F.status = B.status;
        F.db1 = w.bias_grad[1];
        if (adam) {
            F.adam = 1; F.ab1 = adam[3]; F.hp = *hp; F.arith = arith;
        }
        // F zeroes the later launches' tickets (in one launch with O, not O's own: its last arrivers
        // reset them)
        const bool fo = t.fo_split == 0;
        F.zero_words = B.tickets; F.zero_n = (fo ? 2 : 3) * tiles_n;
        F.serial = B.serial;
        F.scale_s = 2.0f / (float)((int64_t)batch * t.s); F.scale_r = 2.0f / (float)batch;
        F.inv_s = 1.0f / (float)((int64_t)batch * t.s); F.inv_r = 1.0f / (float)batch;
        if ((e = launch_train_fused(F, !fo, stream)) != hipSuccess) return e;
    }
    // forward through the hidden layers
    for (int l = 0; l < (fused ? 0 : L); ++l) {
        GemmDesc& D = G.d[0];
        D = GemmDesc{};
        if (l == 0) {
            D.A = Operand{};
            D.A.kind = OP_GATHER; D.A.rows = R; D.A.ones_row = -1;
        } else {
            D.A = direct(B.act[l - 1], nullptr, 0, W, R);
        }
        D.B = direct(w.weight[l], nullptr, 0, l == 0 ? K0 : W, W);
        D.out.mode = EPI_ACT; D.out.c0 = D.out.c1 = B.act[l]; D.out.split = R; D.out.ldc = W;
        D.out.b0 = D.out.b1 = w.bias[l]; D.out.bsplit = W; D.out.relu = 1;
        finish(D, R, W, l == 0 ? K0 : W);
        G.nd = 1;
        if (l == 0) {
            // the forward launch raises the step's serial (the fold's granule tag) and takes the
            // previous step's deferred Adam step (a layer nothing before this step's second forward
            // launch reads)
            G.serial = fold_nw ? B.serial : nullptr;
            G.adam_count = 0;
            for (int i = 0; i < prior_n; ++i) G.adam_t[G.adam_count++] = prior[i];
        }
        G.xcd = xcd_opt;
        e = l == 0 ? launch_gemm_any<OP_GATHER, OP_DIRECT>(G, false, stream, ens, t, l)
                   : launch_gemm_any<OP_DIRECT, OP_DIRECT>(G, false, stream, ens, t, l);
        G.serial = nullptr;
        G.adam_count = 0;
        if (e != hipSuccess) return e;
    }
    // output layer (state head, reward head) + the loss gradient dY and its column sums
    if (!fused) {
        GemmDesc& D = G.d[0];
        D = GemmDesc{};
        D.A = direct(B.act[L - 1], nullptr, 0, W, R);
        D.B = direct(w.weight[L], wo_r, t.s, W, J);
        Output& O = D.out;
        O.mode = EPI_LOSS; O.c0 = O.c1 = B.dy; O.split = R; O.ldc = J;
        O.b0 = w.bias[L]; O.b1 = bo_r; O.bsplit = t.s;
        O.scale_s = 2.0f / (float)((int64_t)batch * t.s); O.scale_r = 2.0f / (float)batch;
        O.inv_s = 1.0f / (float)((int64_t)batch * t.s); O.inv_r = 1.0f / (float)batch;
        O.s = t.s; O.loss_part = B.loss_part; O.colsum_out = B.cs_dy;
        finish(D, R, J, W);
        G.nd = 1;
        G.xcd = xcd_opt;
        if ((e = launch_gemm_any<OP_DIRECT, OP_DIRECT>(G, false, stream, ens, t, L)) != hipSuccess) return e;
    }
    const int loss_parts = fused ? tiles_r : G.d[0].tiles;
    // backward: layer l = L (output) .. 0; launch l: dH_{l-1} (l >= 1) and dW_l, db_l. With the fold
    // (fold_waves) launch 1 also finishes dW_0 / db_0 and launch 0 does not exist.
    const int l_end = fold_nw ? 1 : 0;
    for (int l = fused ? L - 1 : L; l >= l_end; --l) {
        const bool out_layer = l == L;
        const float* g_in = out_layer ? B.dy : B.dh[l % 2];   // dL/d(pre-activation of layer l), [R][n_out]
        const float* cs_in = out_layer ? B.cs_dy : B.cs_dh[l % 2];
        const int n_out = out_layer ? J : W, n_in = l == 0 ? K0 : W;
        // 64-row tiles when the launch's 32 x 32 tiles would need a second round of the CUs
        // (2 x 512: dH_0 and dW_1 are 256 tiles each); the tile height changes no bit
        const int tiles32 = (l >= 1 ? tiles_r * ((W + TT - 1) / TT) : 0) +
                            ((n_out + TT - 1) / TT) * ((n_in + TT - 1) / TT);
        int tmx = (l >= 1 && tiles32 > device_cu_count() && (n_out >= 256 || R >= 256)) ? 2 : 1;
        if (t.tile == 32 || (t.tile == 64 && l >= 1 && (n_out >= 256 || R >= 256))) tmx = t.tile / 32;
        G.nd = 0;
        if (l >= 1) {           // dH_{l-1} = (g_in W_l) * (H_{l-1} > 0), and its column sums
            GemmDesc& D = G.d[G.nd++];
            D = GemmDesc{};
            D.A = direct(g_in, nullptr, 0, n_out, R);
            D.B = out_layer ? transposed(w.weight[L], wo_r, t.s, W, W) : transposed(w.weight[l], nullptr, 0, W, W);
            D.out.mode = EPI_MASK; D.out.c0 = D.out.c1 = B.dh[(l - 1) % 2]; D.out.split = R; D.out.ldc = W;
            D.out.mask = B.act[l - 1]; D.out.ldm = W; D.out.colsum_out = B.cs_dh[(l - 1) % 2];
            finish(D, R, W, n_out, tmx);
            if (l == 1 && fold_nw) {
                Output& O = D.out;
                O.fold = 1; O.fold_k0 = K0; O.fold_nw = fold_nw; O.fold_x = B.xbuf;
                O.fold_dw = w.weight_grad[0]; O.fold_db = w.bias_grad[0];
                O.fold_cs_tiles = tiles_r;   // <= 16: the fold's 32-row waves bound R by 512 (fold_waves)
                O.fold_gran = B.fold_gran; O.cs_gran = B.cs_gran; O.fold_serial = B.serial; O.fold_status = B.status;
                if (adam) {          // nothing in this launch reads layer 0's parameters
                    O.fold_adam = 1; O.fold_aw = adam[0]; O.fold_ab = adam[1];
                }
            }
        }
        {                       // dW_l = g_in^T X_l; db_l = the column sums of g_in over the row tiles
            GemmDesc& D = G.d[G.nd++];
            D = GemmDesc{};
            D.A = transposed(g_in, nullptr, 0, n_out, n_out);
            D.B = l == 0 ? transposed(B.xbuf, nullptr, 0, K0, n_in) : transposed(B.act[l - 1], nullptr, 0, W, n_in);
            // (fused: db_1 and b_1's Adam step came from O's last arrivers)
            D.out = grad_output(t, l, w.weight_grad, w.bias_grad, fused ? nullptr : cs_in, tiles_r);
            finish(D, n_out, n_in, R, tmx);
            if (l == 1 && fold_nw) D.out.fold_sum = 1;   // row block 0's tiles finish dW_0 / db_0 (fold_sum)
        }
        if (adam && l == 0) {   // nothing in this launch reads layer 0's parameters: step them in place
            G.d[G.nd - 1].out.adam = 1;
            G.d[G.nd - 1].out.aw = adam[0];
            G.d[G.nd - 1].out.ab = adam[1];
        }
        if (adam && fused && l == 1) {
            // the dH_0 tiles of a column block read that block of W_1: the dW_1 tiles step it in place
            // once those tiles' K loops are done (dH_0 tiles have the lower ids)
            Output& O = G.d[G.nd - 1].out;
            O.adam = 1; O.aw = adam[2];
            O.wait_ticket = B.tickets + tiles_n;
            O.wait_count = (unsigned)((R + TT * tmx - 1) / (TT * tmx));
            O.wait_status = B.status;
            G.d[0].out.arrive_ticket = B.tickets + tiles_n;
        }
        // layer l + 1's gradient is complete (previous launch) and this launch does not read its
        // parameters: its Adam step rides along (with the reward head when l + 1 is the output layer)
        G.adam_count = 0;
        if (adam && l + 1 <= L) {
            const int first = 2 * (l + 1), n = (l + 1 == L && t.reward) ? 4 : 2;
            for (int i = 0; i < n; ++i) G.adam_t[G.adam_count++] = adam[first + i];
        }
        G.loss_part = B.loss_part; G.loss_parts = loss_parts; G.loss_out = loss_out;
        const bool loss_wg = l == l_end && loss_out != nullptr;
        G.xcd = xcd_opt;
        e = l == 0    ? launch_gemm_any<OP_TRANS, OP_TRANS>(G, loss_wg, stream, ens, t, l)
            : tmx == 2 ? launch_gemm_any<OP_DIRECT, OP_TRANS, OP_TRANS, OP_TRANS, 2>(G, loss_wg, stream, ens, t, l)
                       : launch_gemm_any<OP_DIRECT, OP_TRANS, OP_TRANS, OP_TRANS>(G, loss_wg, stream, ens, t, l);
        if (e != hipSuccess) return e;
    }
    if (adam && fold_nw && !fused) {   // layer 1's step (launch 0's passenger before the fold): the next forward launch's
        const int n = (L == 1 && t.reward) ? 4 : 2;
        for (int i = 0; i < n; ++i) pending[i] = adam[2 + i];
        *pending_n = n;
    }
    return hipSuccess;
}

// One layer's weight and bias gradient for every member of an ensemble, from row-major deltas g [K][n_out] and
// layer inputs x [K][n_in] in the members' workspaces (member e's lie e * ens.ws_stride floats on): the EPI_GRAD
// product launch_train_grads runs for layer 0, dW = g^T x over K rows with the K split over the launch's waves
// (launch_waves: a function of K alone), db[m] = the ordered sum of colsum[0 .. colsum_tiles)[m]. The output
// layer (layer == t.L) with a reward head splits its rows between the two heads' gradient buffers.
hipError_t launch_train_wgrads(const TrainShape& t, int layer, const float* g, const float* x, const float* colsum,
                               int colsum_tiles, int K, const TrainEnsemble& ens, hipStream_t stream) {
    const int n_out = layer == t.L ? t.s + t.reward : t.W, n_in = layer == 0 ? t.s + t.a : t.W;
    const mbrl_train_model& m0 = ens.members[0];
    GemmLaunch G{};
    G.H = t.H; G.s = t.s; G.a = t.a;
    G.slot = -1;
    G.nd = 1;
    GemmDesc& D = G.d[0];
    D.A = transposed(g, nullptr, 0, n_out, n_out);
    D.B = transposed(x, nullptr, 0, n_in, n_in);
    D.out = grad_output(t, layer, m0.weight_grad, m0.bias_grad, colsum, colsum_tiles);
    finish(D, n_out, n_in, K);
    return launch_gemm_any<OP_TRANS, OP_TRANS>(G, false, stream, &ens, t, layer);
}

}  // namespace mbrl
