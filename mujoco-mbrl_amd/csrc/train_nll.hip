// Probabilistic members: training and evaluation on the Gaussian negative log-likelihood (include/mbrl_cem.h
// mbrl_train_grads_nll, mbrl_train_epoch_nll(_clipped), mbrl_eval_members_nll), E members in shared launches.
// The member's one head has 2 s rows: the mean, then the raw log-variance. Positions are numbered p = b * H + h
// (row-major, mbrl_eval_members' numbering) in every array, B = batch, P = B * H.
//
// Launch 1 (nll_fwd_kernel): eval_rows_kernel with a head of 2 s neurons. Grid (16-position tiles, members); the
// workgroup gathers its inputs through the rows, runs the MLP in two LDS buffers through eval_layer -- the head
// as one output layer, so the mean rows are mbrl_eval_members' fma chains -- and stores x0[p], every hidden
// activation act[l][p] and, from the head's outputs, the deltas dY[p] = (dm, dr). The per-element values
// (squared error, its weighted form plus lv, lv) are formed by all lanes in place, then one lane per position adds
// each of the three row values j ascending. With the store pointers NULL nothing but the row values leaves: that
// is mbrl_eval_members_nll's kernel, one body, so both entries return the same bytes.
//
// Launch 2 (nll_bwd_kernel): the same grid; train_ol_bwd_kernel at one step with no carry. The deltas go to
// LDS (zeros up to the next multiple of 16 and in the rows past P), then L transposed products, each masked by
// the stored activation and stored. The products are a second copy of train_bptt.h's bptt_layer on
// v_mfma_f64_16x16x4_f64 (nll_bptt_layer): the fp32 deltas and weights enter as doubles, the n-ordered chain is
// accumulated in fp64 and rounded to fp32 once. With exp(-lv) up to e^-min_lv on the deltas, a hidden unit's delta
// is often a sum whose terms cancel (58x in tests/train_nll_reference.py's case b1); an fp32 chain loses
// 3e-6 of such an element where the fp64 one loses 9e-7, and the products are a small part of the batch. Bias
// gradients: after each product one thread per column adds the tile's valid positions ascending; the sums leave
// as one partial per (layer, tile) and the weight-gradient launch adds the tiles in ascending order.
//
// Launches 3 .. L + 3: launch_train_wgrads (train.hip) over the P positions, the head as an output layer of 2 s
// rows. Launch L + 4 (with loss_out): nll_loss_kernel, eval_loss_kernel's rule on the three row arrays. The
// epoch entries add the ensemble's Adam launch (or the norm launches and the clipped one) per batch through
// train_epoch_members. Nothing waits on another workgroup and nothing is accumulated with atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "eval_mlp.h"
#include "mbrl_train.h"
#include "train_bptt.h"

namespace mbrl {

constexpr int NLL_LOSS_THREADS = 1024;   // eval.hip's EVAL_LOSS_THREADS: the same summation order

struct NllLaunch {
    EvalLaunch A;                         // A.rows: member 0's rows; A.P = B * H; A.reward = 0; row_err [E][P]
    const float *min_lv, *max_lv;         // [s]
    float *row_nll, *row_lv;              // [E][P]
    int64_t idx_stride;                   // rows between two members' rows (0: all members read the same rows)
    int64_t ws_stride;                    // floats between two members' workspace slices
    float* x0;                            // member 0's slice: [P][s + a]; NULL: no stores (mbrl_eval_members_nll)
    float* act[MBRL_TRAIN_MAX_LAYERS];    // [P][W], l < L
    float* dl[MBRL_TRAIN_MAX_LAYERS];     // delta_l [P][W], l < L
    float* gout;                          // dY [P][2 s]
    float* cs[MBRL_TRAIN_MAX_LAYERS];     // column sums [tiles][W] (l < L), [tiles][2 s] (l = L)
    float scale;                          // 1 / (B s)
};

// max(x, 0) + log1p(exp(-|x|)); a NaN stays a NaN through the second term
__device__ __forceinline__ float nll_softplus(float x) { return fmaxf(x, 0.0f) + log1pf(expf(-fabsf(x))); }
// 1 / (1 + exp(-x)) without an overflow on either side
__device__ __forceinline__ float nll_sigmoid(float x) {
    const float t = expf(-fabsf(x));
    return x >= 0.0f ? 1.0f / (1.0f + t) : t / (1.0f + t);
}

__global__ __launch_bounds__(OL_THREADS) void nll_fwd_kernel(const NllLaunch T) {
    extern __shared__ __attribute__((aligned(16))) float nll_lds[];
    const EvalLaunch& A = T.A;
    const int ld = A.ld, tid = threadIdx.x, e = blockIdx.y, s = A.s;
    float* buf[2] = {nll_lds, nll_lds + OL_TM * ld};
    const int64_t p0 = (int64_t)blockIdx.x * OL_TM;
    const int nvalid = (int)min((int64_t)OL_TM, A.P - p0);
    const EvalMember& M = A.m[e];
    const int64_t* rows = A.rows + (int64_t)e * T.idx_stride;
    const int64_t by = (int64_t)e * T.ws_stride;
    const bool store = T.x0 != nullptr;
    const int K0 = s + A.a, K0p = (K0 + 15) & ~15, J = 2 * s;
    // the tile's inputs (states, actions) through the rows; zeros past K0 and for positions past P
    for (int idx = tid; idx < OL_TM * K0p; idx += OL_THREADS) {
        const int row = idx / K0p, k = idx - row * K0p;
        float v = 0.0f;
        if (row < nvalid && k < K0) {
            const int64_t p = p0 + row, r = p / A.H, h = p - r * A.H;
            const int64_t at = rows[r] * A.H + h;
            v = k < s ? A.states[at * s + k] : A.actions[at * A.a + (k - s)];
        }
        buf[0][row * ld + k] = v;
    }
    __syncthreads();
    if (store) ol_store_rows(buf[0], ld, T.x0 + by + p0 * K0, K0, nvalid);
    int cur = 0;
    for (int l = 0; l < A.L; ++l) {
        eval_layer<true>(buf[cur], buf[cur ^ 1], ld, M.w[l], M.b[l], A.W, nullptr, nullptr, 0, l == 0 ? K0 : A.W);
        cur ^= 1;
        __syncthreads();
        if (store) ol_store_rows(buf[cur], ld, T.act[l] + by + p0 * A.W, A.W, nvalid);
    }
    eval_layer<false>(buf[cur], buf[cur ^ 1], ld, M.w[A.L], M.b[A.L], J, nullptr, nullptr, 0, A.W);
    cur ^= 1;
    __syncthreads();
    // per element, in place: column j <- (m - y)^2 exp(-lv) + lv, column s + j <- (m - y)^2, and lv to the other
    // buffer's column j (the head's input there has been read and stored); the deltas leave from here
    float* out = buf[cur];
    float* lvs = buf[cur ^ 1];
    for (int idx = tid; idx < nvalid * s; idx += OL_THREADS) {
        const int row = idx / s, j = idx - row * s;
        const int64_t p = p0 + row, r = p / A.H, h = p - r * A.H;
        const float y = A.next_states[(rows[r] * A.H + h) * s + j];
        const float lo = T.min_lv[j], hi = T.max_lv[j];
        const float m = out[row * ld + j], raw = out[row * ld + s + j];
        const float u = hi - nll_softplus(hi - raw);
        const float lv = lo + nll_softplus(u - lo);
        const float d = m - y, d2 = d * d, iv = expf(-lv), wd2 = d2 * iv;
        out[row * ld + j] = wd2 + lv;
        out[row * ld + s + j] = d2;
        lvs[row * ld + j] = lv;
        if (store) {
            float* g = T.gout + by + (p0 + row) * J;
            g[j] = 2.0f * d * iv * T.scale;
            g[s + j] = (1.0f - wd2) * T.scale * nll_sigmoid(u - lo) * nll_sigmoid(hi - raw);
        }
    }
    __syncthreads();
    if (tid < nvalid) {
        const float* v = out + tid * ld;
        const float* w = lvs + tid * ld;
        float nll = 0.0f, err = 0.0f, lv = 0.0f;
        for (int j = 0; j < s; ++j) {
            nll = nll + v[j];
            err = err + v[s + j];
            lv = lv + w[j];
        }
        const int64_t o = (int64_t)e * A.P + p0 + tid;
        T.row_nll[o] = nll;
        A.row_err[o] = err;
        T.row_lv[o] = lv;
    }
}

typedef double nll_f64x4 __attribute__((ext_vector_type(4)));

// bptt_layer (train_bptt.h) with the chain in fp64: out[p][m] = fp32(sum_n in[p][n] w[n][m]) (* (mask[p][m] > 0))
// for the tile's 16 positions and m < Kout, rows n < n0 of the weights with ldw floats per row; columns from Kout
// to the next multiple of 16 are written as zeros; rows past nvalid mask to zero and are not stored. Operands as
// in the f32 16x16x4 form, one double per lane (lane l: weight column 16 mb + l % 16 of row nb + 4 (l / 16) + i,
// position l % 16); the result's layout is the f64 instruction's own: lane l holds columns 16 mb + l / 16 + 4 v,
// v = 0 .. 3, of position l % 16.
__device__ __forceinline__ void nll_bptt_layer(const float* __restrict__ in, float* __restrict__ out, int ld,
                                               const float* __restrict__ w0, int n0, int ldw, int Kout,
                                               const float* __restrict__ mask, float* __restrict__ store, int ldo,
                                               int nvalid) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, q = lane >> 4;
    const int N16 = (n0 + 15) & ~15, MB = (Kout + 15) >> 4;
    for (int mb0 = wave * EVAL_JB; mb0 < MB; mb0 += EVAL_WAVES * EVAL_JB) {
        nll_f64x4 acc[EVAL_JB];
#pragma unroll
        for (int j = 0; j < EVAL_JB; ++j) acc[j] = nll_f64x4{0.0, 0.0, 0.0, 0.0};
        for (int nb = 0; nb < N16; nb += 16) {
            const int n = nb + 4 * q;
            const eval_f32x4 x = *reinterpret_cast<const eval_f32x4*>(&in[c * ld + n]);
            // every lane loads from a valid address (the last row where it has none, column 0 where it has no
            // column) and the value is masked afterwards: no divergent branch around the loads
            size_t roff[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) roff[i] = (size_t)min(n + i, n0 - 1) * ldw;
#pragma unroll
            for (int j = 0; j < EVAL_JB; ++j) {
                if (mb0 + j >= MB) continue;             // (wave-uniform)
                const int m = (mb0 + j) * 16 + c;
                const bool mok = m < Kout;
                eval_f32x4 wv;
#pragma unroll
                for (int i = 0; i < 4; ++i) wv[i] = w0[roff[i] + (mok ? m : 0)];
#pragma unroll
                for (int i = 0; i < 4; ++i) wv[i] = mok && n + i < n0 ? wv[i] : 0.0f;
                for (int i = 0; i < 4; ++i)
                    acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64((double)wv[i], (double)x[i], acc[j], 0, 0, 0);
            }
        }
#pragma unroll
        for (int j = 0; j < EVAL_JB; ++j) {
            if (mb0 + j >= MB) continue;
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int m = (mb0 + j) * 16 + q + 4 * v;
                float t = (float)acc[j][v];
                if (m >= Kout) {
                    t = 0.0f;                             // (0 x a non-finite delta is a NaN: the padding stays zero)
                } else if (mask) {
                    const float keep = c < nvalid ? mask[(int64_t)c * ldo + m] : 0.0f;
                    if (!(keep > 0.0f)) t = 0.0f;
                }
                out[c * ld + m] = t;
                if (store && c < nvalid && m < Kout) store[(int64_t)c * ldo + m] = t;
            }
        }
    }
}

__global__ __launch_bounds__(OL_THREADS) void nll_bwd_kernel(const NllLaunch T) {
    extern __shared__ __attribute__((aligned(16))) float nll_lds[];
    const EvalLaunch& A = T.A;
    const int ld = A.ld, tid = threadIdx.x, e = blockIdx.y, L = A.L, W = A.W;
    float* buf[2] = {nll_lds, nll_lds + OL_TM * ld};
    const int64_t p0 = (int64_t)blockIdx.x * OL_TM;
    const int nvalid = (int)min((int64_t)OL_TM, A.P - p0);
    const EvalMember& M = A.m[e];
    const int64_t by = (int64_t)e * T.ws_stride;
    const int J = 2 * A.s, J16 = (J + 15) & ~15;
    // the deltas of the head's outputs; zeros to J16 and in the rows past P
    const float* g = T.gout + by + p0 * J;
    for (int idx = tid; idx < OL_TM * J16; idx += OL_THREADS) {
        const int row = idx / J16, j = idx - row * J16;
        buf[0][row * ld + j] = row < nvalid && j < J ? g[(int64_t)row * J + j] : 0.0f;
    }
    __syncthreads();
    int cur = 0;
    ol_colsum(buf[cur], ld, J, nvalid, T.cs[L] + by + (int64_t)blockIdx.x * J, true);
    // delta_{L-1} through the head, then down the trunk
    nll_bptt_layer(buf[cur], buf[cur ^ 1], ld, M.w[L], J, W, W, T.act[L - 1] + by + p0 * W,
                   T.dl[L - 1] + by + p0 * W, W, nvalid);
    cur ^= 1;
    __syncthreads();
    ol_colsum(buf[cur], ld, W, nvalid, T.cs[L - 1] + by + (int64_t)blockIdx.x * W, true);
    for (int l = L - 1; l >= 1; --l) {
        nll_bptt_layer(buf[cur], buf[cur ^ 1], ld, M.w[l], W, W, W, T.act[l - 1] + by + p0 * W,
                       T.dl[l - 1] + by + p0 * W, W, nvalid);
        cur ^= 1;
        __syncthreads();
        ol_colsum(buf[cur], ld, W, nvalid, T.cs[l - 1] + by + (int64_t)blockIdx.x * W, true);
    }
}

// loss_out[e] = (nll, mse, mean_lv), each in eval_loss_kernel's order: per step h, lane t adds b = t, t + 1024, ..
// ascending, the partials meet pairwise (d = 512 .. 1), the sum is divided by B s and the steps are added h
// ascending.
__global__ __launch_bounds__(NLL_LOSS_THREADS) void nll_loss_kernel(const float* __restrict__ row_nll,
                                                                    const float* __restrict__ row_err,
                                                                    const float* __restrict__ row_lv,
                                                                    float* __restrict__ loss_out, int64_t R, int H, int s) {
    __shared__ float part[NLL_LOSS_THREADS];
    const int e = blockIdx.x, t = threadIdx.x;
    const float denom = (float)((double)R * (double)s);
    for (int which = 0; which < 3; ++which) {
        const float* src = (which == 0 ? row_nll : which == 1 ? row_err : row_lv) + (int64_t)e * R * H;
        float total = 0.0f;
        for (int h = 0; h < H; ++h) {
            float acc = 0.0f;
            for (int64_t r = t; r < R; r += NLL_LOSS_THREADS) acc += src[r * H + h];
            part[t] = acc;
            __syncthreads();
            for (int d = NLL_LOSS_THREADS / 2; d >= 1; d >>= 1) {
                if (t < d) part[t] += part[t + d];
                __syncthreads();
            }
            if (t == 0) total += part[0] / denom;
            __syncthreads();
        }
        if (t == 0) loss_out[3 * e + which] = total;
    }
}

// ---- host
static int nll_ld(const TrainShape& t) {
    const int widest = std::max(t.W, std::max(t.s + t.a, 2 * t.s));
    return ((widest + 15) & ~15) + EVAL_PAD;
}

struct NllPlan {
    int tiles;
    size_t row_nll, row_err, row_lv;      // float offsets of the members' common arrays
    size_t x0, act[MBRL_TRAIN_MAX_LAYERS], dl[MBRL_TRAIN_MAX_LAYERS], gout, cs[MBRL_TRAIN_MAX_LAYERS];
    size_t stride, first, floats;         // a member's slice, where member 0's starts, everything
};

static NllPlan nll_plan(const TrainShape& t, int E, int batch) {
    NllPlan p{};
    const size_t P = (size_t)batch * t.H, J = (size_t)2 * t.s, W = t.W;
    p.tiles = (int)((P + OL_TM - 1) / OL_TM);
    auto up = [](size_t x) { return (x + 63) & ~(size_t)63; };
    size_t off = 0;
    auto take = [&](size_t n) { const size_t at = off; off += up(n); return at; };
    p.row_nll = take((size_t)E * P);
    p.row_err = take((size_t)E * P);
    p.row_lv = take((size_t)E * P);
    p.first = off;
    off = 0;
    p.x0 = take(P * (t.s + t.a));
    for (int l = 0; l < t.L; ++l) p.act[l] = take(P * W);
    for (int l = 0; l < t.L; ++l) p.dl[l] = take(P * W);
    p.gout = take(P * J);
    for (int l = 0; l < t.L; ++l) p.cs[l] = take((size_t)p.tiles * W);
    p.cs[t.L] = take((size_t)p.tiles * J);
    p.stride = off;
    p.floats = p.first + (size_t)E * p.stride;
    return p;
}

size_t nll_ws_floats(const TrainShape& t, int E, int batch) { return nll_plan(t, E, batch).floats; }

bool nll_bounds_ok(const mbrl_nll_bounds* bounds) { return bounds && bounds->min_logvar && bounds->max_logvar; }

// The members' common shape inside the envelope: mbrl_eval_members', less what the two LDS buffers cannot hold.
int nll_envelope(const char* what, const TrainShape& t) {
    if (t.L + 2 > MBRL_TRAIN_MAX_LAYERS || t.W > MBRL_EVAL_MAX_DIM || t.s > MBRL_EVAL_MAX_DIM ||
        t.a > MBRL_EVAL_MAX_DIM || t.s + t.a > MBRL_EVAL_MAX_DIM)
        return fail(MBRL_EUNSUPPORTED, "%s: shape outside the envelope (state %d, action %d, hidden %d x %d; each of "
                    "state, state + action and hidden <= %d, n_hidden <= %d)", what, t.s, t.a, t.W, t.L,
                    MBRL_EVAL_MAX_DIM, MBRL_TRAIN_MAX_LAYERS - 2);
    const size_t lds = (size_t)2 * OL_TM * nll_ld(t) * sizeof(float);
    if (lds > (size_t)OL_LDS_BYTES)
        return fail(MBRL_EUNSUPPORTED, "%s: the kernels need %zu bytes of LDS for a head of 2 x %d outputs (32 rows of "
                    "%d floats): more than %d", what, lds, t.s, nll_ld(t), OL_LDS_BYTES);
    return MBRL_OK;
}

static void nll_fill(NllLaunch& T, const TrainShape& t, const mbrl_train_model* members, int E,
                     const mbrl_train_data* data, const int64_t* rows, int64_t idx_stride, int64_t R,
                     const mbrl_nll_bounds* bounds) {
    EvalLaunch& A = T.A;
    for (int e = 0; e < E; ++e)
        for (int l = 0; l <= t.L; ++l) {
            A.m[e].w[l] = members[e].weight[l];
            A.m[e].b[l] = members[e].bias[l];
        }
    A.states = data->states; A.actions = data->actions; A.next_states = data->next_states; A.rewards = nullptr;
    A.rows = rows;
    A.P = R * t.H;
    A.s = t.s; A.a = t.a; A.W = t.W; A.L = t.L; A.reward = 0; A.H = t.H;
    A.ld = nll_ld(t);
    T.min_lv = bounds->min_logvar;
    T.max_lv = bounds->max_logvar;
    T.idx_stride = idx_stride;
    T.scale = 1.0f / (float)((double)R * (double)t.s);
}

static hipError_t nll_loss(const NllLaunch& T, float* loss_out, int E, int64_t R, hipStream_t stream) {
    hipLaunchKernelGGL(nll_loss_kernel, dim3(E), dim3(NLL_LOSS_THREADS), 0, stream, T.row_nll, T.A.row_err, T.row_lv,
                       loss_out, R, T.A.H, T.A.s);
    return hipGetLastError();
}

// One batch's launches (checked arguments; EnsembleBatch, the workspace laid out for `batch` itself): forward,
// backward, L + 1 weight-gradient launches, loss.
static hipError_t nll_launch(const TrainShape& t, const mbrl_train_model* members, int E, const mbrl_train_data* data,
                             const int64_t* idx, int64_t idx_stride, int /*bs*/, int batch, float* loss_out, float* ws,
                             const mbrl_nll_bounds* bounds, hipStream_t stream) {
    const NllPlan p = nll_plan(t, E, batch);
    NllLaunch T{};
    nll_fill(T, t, members, E, data, idx, idx_stride, batch, bounds);
    T.row_nll = ws + p.row_nll;
    T.A.row_err = ws + p.row_err;
    T.row_lv = ws + p.row_lv;
    T.ws_stride = (int64_t)p.stride;
    float* m0 = ws + p.first;
    T.x0 = m0 + p.x0;
    for (int l = 0; l < t.L; ++l) {
        T.act[l] = m0 + p.act[l];
        T.dl[l] = m0 + p.dl[l];
    }
    T.gout = m0 + p.gout;
    for (int l = 0; l <= t.L; ++l) T.cs[l] = m0 + p.cs[l];
    hipError_t err;
    if ((err = ensure_dynamic_lds(reinterpret_cast<const void*>(nll_fwd_kernel), OL_LDS_BYTES)) != hipSuccess) return err;
    if ((err = ensure_dynamic_lds(reinterpret_cast<const void*>(nll_bwd_kernel), OL_LDS_BYTES)) != hipSuccess) return err;
    const dim3 grid(p.tiles, E);
    const size_t lds = (size_t)2 * OL_TM * T.A.ld * sizeof(float);
    hipLaunchKernelGGL(nll_fwd_kernel, grid, dim3(OL_THREADS), lds, stream, T);
    if ((err = hipGetLastError()) != hipSuccess) return err;
    hipLaunchKernelGGL(nll_bwd_kernel, grid, dim3(OL_THREADS), lds, stream, T);
    if ((err = hipGetLastError()) != hipSuccess) return err;
    const TrainEnsemble ens{members, E, (int64_t)p.stride, idx_stride, 3};
    // launch_train_wgrads takes the output layer's rows from the shape: one head of 2 s rows, no reward head
    TrainShape head = t;
    head.s = 2 * t.s;
    head.reward = 0;
    const int K = batch * t.H;
    for (int l = t.L; l >= 0; --l) {
        const float* g = l == t.L ? T.gout : T.dl[l];
        const float* x = l == 0 ? T.x0 : T.act[l - 1];
        if ((err = launch_train_wgrads(l == t.L ? head : t, l, g, x, T.cs[l], p.tiles, K, ens, stream)) != hipSuccess)
            return err;
    }
    if (!loss_out) return hipSuccess;
    return nll_loss(T, loss_out, E, batch, stream);
}

}  // namespace mbrl

using namespace mbrl;

extern "C" {

size_t mbrl_train_nll_workspace_bytes(const mbrl_train_model* members, int32_t E, int32_t batch) {
    TrainShape t;
    const char* what = "train_nll_workspace_bytes";
    if (batch < 1 || ensemble_shape(what, members, E, LOSS_NLL, &t) != MBRL_OK || ol_batch_ok(what, E, batch, t) != MBRL_OK)
        return 0;
    return nll_ws_floats(t, E, batch) * sizeof(float);
}

int mbrl_train_grads_nll(const mbrl_train_model* members, int32_t E, const mbrl_train_data* data,
                         const int64_t* batch_idx, int32_t batch, const mbrl_nll_bounds* bounds, float* loss_out,
                         void* workspace, size_t ws_bytes, mbrl_stream_t stream) {
    const char* what = "train_grads_nll";
    TrainShape t;
    if (int rc = ensemble_shape(what, members, E, LOSS_NLL, &t)) return rc;
    if (!train_data_ok(data, t) || !batch_idx || !workspace) return fail(MBRL_EINVAL, "%s: NULL argument", what);
    if (!nll_bounds_ok(bounds)) return fail(MBRL_EINVAL, "%s: NULL log-variance bounds", what);
    if (reinterpret_cast<uintptr_t>(workspace) & 15) return fail(MBRL_EINVAL, "%s: workspace not 16-byte aligned", what);
    if (batch < 1 || (int64_t)batch > data->transitions)
        return fail(MBRL_EINVAL, "%s: batch %d outside [1, %lld]", what, batch, (long long)data->transitions);
    if (int rc = ensemble_members(what, members, E, t)) return rc;
    if (int rc = ol_batch_ok(what, E, batch, t)) return rc;
    const size_t need = nll_ws_floats(t, E, batch) * sizeof(float);
    if (ws_bytes < need) return fail(MBRL_EWORKSPACE, "%s: workspace %zu < %zu bytes", what, ws_bytes, need);
    return hip_check(nll_launch(t, members, E, data, batch_idx, batch, batch, batch, loss_out,
                                static_cast<float*>(workspace), bounds, reinterpret_cast<hipStream_t>(stream)), what);
}

int mbrl_train_epoch_nll(const mbrl_train_model* members, int32_t E, const mbrl_train_data* data,
                         const int64_t* orders, int64_t rows, int32_t batch_size, const mbrl_adam_tensor* tensors,
                         int32_t count, const mbrl_adam_hparams* hparams, const float* step_sizes,
                         const float* bc2_sqrt, float* losses, void* workspace, size_t ws_bytes, mbrl_stream_t stream,
                         const mbrl_nll_bounds* bounds) {
    return train_epoch_members("train_epoch_nll", LOSS_NLL, false, nll_launch, members, E, data, orders, rows,
                               batch_size, tensors, count, hparams, step_sizes, bc2_sqrt, losses, workspace, ws_bytes,
                               nullptr, bounds, stream);
}

int mbrl_train_epoch_nll_clipped(const mbrl_train_model* members, int32_t E, const mbrl_train_data* data,
                                 const int64_t* orders, int64_t rows, int32_t batch_size,
                                 const mbrl_adam_tensor* tensors, int32_t count, const mbrl_adam_hparams* hparams,
                                 const float* step_sizes, const float* bc2_sqrt, float* losses, void* workspace,
                                 size_t ws_bytes, mbrl_stream_t stream, const mbrl_nll_bounds* bounds,
                                 const mbrl_grad_clip* clip) {
    return train_epoch_members("train_epoch_nll_clipped", LOSS_NLL, true, nll_launch, members, E, data, orders, rows,
                               batch_size, tensors, count, hparams, step_sizes, bc2_sqrt, losses, workspace, ws_bytes,
                               clip, bounds, stream);
}

int mbrl_eval_members_nll(const mbrl_train_model* members, int32_t E, const mbrl_train_data* data,
                          const int64_t* rows, int64_t R, const mbrl_nll_bounds* bounds, float* row_nll,
                          float* row_err, float* row_lv, float* loss_out, mbrl_stream_t stream) {
    const char* what = "eval_members_nll";
    TrainShape t;
    if (!members || !data || !rows || !row_nll || !row_err || !row_lv)
        return fail(MBRL_EINVAL, "%s: NULL members, data, rows, row_nll, row_err or row_lv", what);
    if (R < 1) return fail(MBRL_EINVAL, "%s: R = %lld rows", what, (long long)R);
    if (int rc = ensemble_shape(what, members, E, LOSS_NLL, &t)) return rc;
    if (!train_data_ok(data, t)) return fail(MBRL_EINVAL, "%s: NULL transitions", what);
    if (!nll_bounds_ok(bounds)) return fail(MBRL_EINVAL, "%s: NULL log-variance bounds", what);
    for (int e = 0; e < E; ++e)           // (forward only: the gradient pointers are ignored and may be NULL)
        for (int l = 0; l <= t.L; ++l)
            if (!members[e].weight[l] || !members[e].bias[l])
                return fail(MBRL_EINVAL, "%s: member %d, layer %d: NULL weight or bias", what, e, l);
    if (R >= ((int64_t)1 << 31)) return fail(MBRL_EUNSUPPORTED, "%s: R = %lld is not below 2^31", what, (long long)R);
    if (int rc = ol_batch_ok(what, E, R, t)) return rc;
    NllLaunch T{};
    nll_fill(T, t, members, E, data, rows, 0, R, bounds);
    T.row_nll = row_nll;
    T.A.row_err = row_err;
    T.row_lv = row_lv;
    const hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (int rc = hip_check(ensure_dynamic_lds(reinterpret_cast<const void*>(nll_fwd_kernel), OL_LDS_BYTES), what)) return rc;
    const unsigned tiles = (unsigned)((T.A.P + OL_TM - 1) / OL_TM);
    hipLaunchKernelGGL(nll_fwd_kernel, dim3(tiles, E), dim3(OL_THREADS), (size_t)2 * OL_TM * T.A.ld * sizeof(float), st, T);
    if (int rc = hip_check(hipGetLastError(), what)) return rc;
    if (!loss_out) return MBRL_OK;
    return hip_check(nll_loss(T, loss_out, E, R, st), what);
}

}  // extern "C"
