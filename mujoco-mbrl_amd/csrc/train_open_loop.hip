// Training on the open-loop loss (include/mbrl_cem.h mbrl_train_grads_open_loop, mbrl_train_epoch_open_loop):
// the gradient of mbrl_eval_members_open_loop's loss through the fed-back predictions (backpropagation
// through time), E members in shared launches. Positions are numbered p = h * B + b (step-major) in every
// workspace array, B = batch.
//
// Launch 1 (train_ol_fwd_kernel): eval_open_loop_kernel with stores. Grid (16-row tiles, members); the
// workgroup runs the horizon loop with the activations in two LDS buffers and the seam of eval.hip, through the
// same eval_layer calls, so the row errors -- and with eval_loss_kernel the losses -- are
// mbrl_eval_members_open_loop's bytes. Per (h, row) it stores the layer-0 input actually used x0[p] =
// (x_h, a_h), every hidden activation act[l][p] and the scaled residual dY[p] = (y - target) * 2 / numel.
//
// Launch 2 (train_ol_bwd_kernel): the same grid; the workgroup runs h = H - 1 .. 0 with the deltas in the two
// LDS buffers. Per step: g_out = dY[p] (+ the carry on the s state columns) is built in place where the carry
// sits, every column from s to the end of the last 16-deep chunk being rewritten (the reward column's dY, then
// zeros), so nothing stale to the right of the state columns reaches the next product; then L + 1 transposed
// products out[p][m] = sum_n in[p][n] w[n][m] on v_mfma_f32_16x16x4f32 -- the weights as the A operand read
// transposed (lane l: column 16 mb + l % 16 of rows nb + 4 (l / 16) + i), the deltas as B from LDS -- each
// masked by the stored activation (> 0, train.hip's EPI_MASK rule) and stored; the last one, through W_0, is
// taken for the s state columns only and is the carry of step h - 1. No wave splits a reduction: every element
// is one n-ordered fma chain over its own row's values, so the bytes of (member, row, step) depend on nothing
// else. Bias gradients: after each product one thread per column adds the tile's valid rows, row ascending,
// and adds that to the column's running sum over the steps (h descending) in LDS; the sums leave as one
// partial per (layer, tile), and the weight-gradient launch adds the tiles in ascending order.
//
// Launches 3 .. L + 3: launch_train_wgrads (train.hip), dW_l = delta_l^T x_l over the B * H positions with the
// member on a grid axis, the K split over the launch's waves a function of B * H alone.
// Launch L + 4 (with loss_out): eval_loss_kernel. The epoch entry adds the ensemble's Adam launch per batch.
// Nothing waits on another workgroup and nothing is accumulated with atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "eval_mlp.h"
#include "mbrl_train.h"
#include "train_bptt.h"

namespace mbrl {

struct OlLaunch {
    EvalLaunch A;                         // A.rows: member 0's batch rows; A.P = batch; row_err [E][B][H]
    int64_t idx_stride;                   // rows between two members' batch rows
    int64_t ws_stride;                    // floats between two members' workspace slices
    float* x0;                            // member 0's slice: [P][s + a]
    float* act[MBRL_TRAIN_MAX_LAYERS];    // [P][W], l < L
    float* dl[MBRL_TRAIN_MAX_LAYERS];     // delta_l [P][W], l < L
    float* gout;                          // dY after launch 1, g_out after launch 2: [P][J]
    float* cs[MBRL_TRAIN_MAX_LAYERS];     // column sums [tiles][W] (l < L), [tiles][J] (l = L)
    float scale_s, scale_r;
    int wacc;                             // floats per LDS column-sum row: max(W, J) rounded up to 16
};

__global__ __launch_bounds__(OL_THREADS) void train_ol_fwd_kernel(const OlLaunch T) {
    extern __shared__ __attribute__((aligned(16))) float ol_lds[];
    const EvalLaunch& A = T.A;
    const int ld = A.ld, tid = threadIdx.x, e = blockIdx.y;
    float* buf[2] = {ol_lds, ol_lds + OL_TM * ld};
    const int64_t r0 = (int64_t)blockIdx.x * OL_TM, R = A.P;
    const int nvalid = (int)min((int64_t)OL_TM, R - r0);
    const EvalMember& M = A.m[e];
    const int64_t* rows = A.rows + (int64_t)e * T.idx_stride;
    const int64_t by = (int64_t)e * T.ws_stride;
    const int K0 = A.s + A.a, K0p = (K0 + 15) & ~15, tail = K0p - A.s, J = A.s + A.reward;
    // x_0 = states[i][0]; rows past R run on zeros and store nothing
    for (int idx = tid; idx < OL_TM * A.s; idx += OL_THREADS) {
        const int row = idx / A.s, k = idx - row * A.s;
        buf[0][row * ld + k] = r0 + row < R ? A.states[rows[r0 + row] * A.H * A.s + k] : 0.0f;
    }
    int cur = 0;
    for (int h = 0; h < A.H; ++h) {
        const int64_t p0 = (int64_t)h * R + r0;
        // the seam of eval_open_loop_kernel: step h's actions, then zeros
        for (int idx = tid; idx < OL_TM * tail; idx += OL_THREADS) {
            const int row = idx / tail, k = idx - row * tail;
            float v = 0.0f;
            if (k < A.a && r0 + row < R) v = A.actions[(rows[r0 + row] * A.H + h) * A.a + k];
            buf[cur][row * ld + A.s + k] = v;
        }
        __syncthreads();
        ol_store_rows(buf[cur], ld, T.x0 + by + p0 * K0, K0, nvalid);
        for (int l = 0; l < A.L; ++l) {
            eval_layer<true>(buf[cur], buf[cur ^ 1], ld, M.w[l], M.b[l], A.W, nullptr, nullptr, 0, l == 0 ? K0 : A.W);
            cur ^= 1;
            __syncthreads();
            ol_store_rows(buf[cur], ld, T.act[l] + by + p0 * A.W, A.W, nvalid);
        }
        eval_layer<false>(buf[cur], buf[cur ^ 1], ld, M.w[A.L], M.b[A.L], A.s, A.reward ? M.w[A.L + 1] : nullptr,
                          A.reward ? M.b[A.L + 1] : nullptr, A.reward ? 1 : 0, A.W);
        cur ^= 1;
        __syncthreads();
        if (tid < OL_TM && r0 + tid < R) {
            const int64_t at = rows[r0 + tid] * A.H + h;
            const int64_t o = ((int64_t)e * R + r0 + tid) * A.H + h;
            const float* y = buf[cur] + tid * ld;
            const float* target = A.next_states + at * A.s;
            float sum = 0.0f;
            for (int j = 0; j < A.s; ++j) {
                const float d = y[j] - target[j];
                sum = sum + d * d;                        // (-ffp-contract=off: a product, then a sum)
            }
            A.row_err[o] = sum;
            if (A.reward) {
                const float d = y[A.s] - A.rewards[at];
                A.row_rew_err[o] = d * d;
            }
        }
        // dY = (y - target) * 2 / numel
        for (int idx = tid; idx < nvalid * J; idx += OL_THREADS) {
            const int row = idx / J, j = idx - row * J;
            const int64_t at = rows[r0 + row] * A.H + h;
            const float y = buf[cur][row * ld + j];
            const float v = j < A.s ? (y - A.next_states[at * A.s + j]) * T.scale_s : (y - A.rewards[at]) * T.scale_r;
            T.gout[by + (p0 + row) * J + j] = v;
        }
        __syncthreads();                                  // the outputs are read: the next step may overwrite column s
    }
}

__global__ __launch_bounds__(OL_THREADS) void train_ol_bwd_kernel(const OlLaunch T) {
    extern __shared__ __attribute__((aligned(16))) float ol_lds[];
    const EvalLaunch& A = T.A;
    const int ld = A.ld, tid = threadIdx.x, e = blockIdx.y, L = A.L;
    float* buf[2] = {ol_lds, ol_lds + OL_TM * ld};
    float* sums = ol_lds + 2 * OL_TM * ld;              // [L + 1][wacc]
    const int64_t r0 = (int64_t)blockIdx.x * OL_TM, R = A.P;
    const int nvalid = (int)min((int64_t)OL_TM, R - r0);
    const EvalMember& M = A.m[e];
    const int64_t by = (int64_t)e * T.ws_stride;
    const int K0 = A.s + A.a, J = A.s + A.reward, J16 = (J + 15) & ~15, W = A.W;
    int cur = 0;
    for (int h = A.H - 1; h >= 0; --h) {
        const bool first = h == A.H - 1;
        const int64_t p0 = (int64_t)h * R + r0;
        // g_out in place over the carry: dY (+ carry) on the state columns, the reward column's dY, zeros to J16
        float* g = T.gout + by + p0 * J;
        for (int idx = tid; idx < OL_TM * J16; idx += OL_THREADS) {
            const int row = idx / J16, j = idx - row * J16;
            float v = 0.0f;
            if (row < nvalid && j < J) {
                v = g[(int64_t)row * J + j];
                if (!first && j < A.s) v = v + buf[cur][row * ld + j];
                g[(int64_t)row * J + j] = v;
            }
            buf[cur][row * ld + j] = v;
        }
        __syncthreads();
        ol_colsum(buf[cur], ld, J, nvalid, sums + L * T.wacc, first);
        // delta_{L-1} through both heads, then down the trunk
        bptt_layer(buf[cur], buf[cur ^ 1], ld, M.w[L], A.s, A.reward ? M.w[L + 1] : nullptr, A.reward ? 1 : 0, W, W,
                   T.act[L - 1] + by + p0 * W, T.dl[L - 1] + by + p0 * W, W, nvalid);
        cur ^= 1;
        __syncthreads();
        ol_colsum(buf[cur], ld, W, nvalid, sums + (L - 1) * T.wacc, first);
        for (int l = L - 1; l >= 1; --l) {
            bptt_layer(buf[cur], buf[cur ^ 1], ld, M.w[l], W, nullptr, 0, W, W, T.act[l - 1] + by + p0 * W,
                       T.dl[l - 1] + by + p0 * W, W, nvalid);
            cur ^= 1;
            __syncthreads();
            ol_colsum(buf[cur], ld, W, nvalid, sums + (l - 1) * T.wacc, first);
        }
        if (h > 0) {   // the carry of step h - 1: delta_0 through W_0's state columns (the action columns dropped)
            bptt_layer(buf[cur], buf[cur ^ 1], ld, M.w[0], W, nullptr, 0, K0, A.s, nullptr, nullptr, 0, nvalid);
            cur ^= 1;
            __syncthreads();
        }
    }
    for (int l = 0; l <= L; ++l) {
        const int N = l == L ? J : W;
        float* dst = T.cs[l] + by + (int64_t)blockIdx.x * N;
        for (int n = tid; n < N; n += OL_THREADS) dst[n] = sums[l * T.wacc + n];
    }
}

// ---- host
struct OlPlan {
    TrainShape t;
    int tiles;
    size_t row_err, row_rew;              // float offsets of the members' common arrays
    size_t x0, act[MBRL_TRAIN_MAX_LAYERS], dl[MBRL_TRAIN_MAX_LAYERS], gout, cs[MBRL_TRAIN_MAX_LAYERS];
    size_t stride, first, floats;         // a member's slice, where member 0's starts, everything
    int ld, wacc;
    size_t lds_bwd;
};

static OlPlan ol_plan(const TrainShape& t, int E, int batch) {
    OlPlan p{};
    p.t = t;
    const size_t P = (size_t)batch * t.H, J = t.s + t.reward, W = t.W;
    p.tiles = (batch + OL_TM - 1) / OL_TM;
    auto up = [](size_t x) { return (x + 63) & ~(size_t)63; };
    size_t off = 0;
    auto take = [&](size_t n) { const size_t at = off; off += up(n); return at; };
    p.row_err = take((size_t)E * P);
    p.row_rew = take(t.reward ? (size_t)E * P : 0);
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
    p.ld = eval_ld(t.s, t.a, t.W, t.reward);
    p.wacc = (int)((std::max(W, J) + 15) & ~(size_t)15);
    p.lds_bwd = ((size_t)2 * OL_TM * p.ld + (size_t)(t.L + 1) * p.wacc) * sizeof(float);
    return p;
}

size_t ol_ws_floats(const TrainShape& t, int E, int batch) { return ol_plan(t, E, batch).floats; }

// The members' common shape (ensemble_shape) inside the envelope: mbrl_eval_members_open_loop's, less what the
// backward kernel's LDS cannot hold.
int ol_envelope(const char* what, const TrainShape& t) {
    if (t.L + 2 > MBRL_TRAIN_MAX_LAYERS || t.W > MBRL_EVAL_MAX_DIM || t.s > MBRL_EVAL_MAX_DIM ||
        t.a > MBRL_EVAL_MAX_DIM || t.s + t.a > MBRL_EVAL_MAX_DIM)
        return fail(MBRL_EUNSUPPORTED, "%s: shape outside the envelope (state %d, action %d, hidden %d x %d; each of "
                    "state, state + action and hidden <= %d, n_hidden <= %d)", what, t.s, t.a, t.W, t.L,
                    MBRL_EVAL_MAX_DIM, MBRL_TRAIN_MAX_LAYERS - 2);
    const OlPlan p = ol_plan(t, 1, 1);
    if (p.lds_bwd > (size_t)OL_LDS_BYTES)
        return fail(MBRL_EUNSUPPORTED, "%s: the backward kernel needs %zu bytes of LDS for hidden %d x %d (32 rows of "
                    "%d floats and %d column-sum rows of %d): more than %d", what, p.lds_bwd, t.W, t.L, p.ld, t.L + 1,
                    p.wacc, OL_LDS_BYTES);
    return MBRL_OK;
}

int ol_batch_ok(const char* what, int32_t E, int64_t batch, const TrainShape& t) {
    if ((int64_t)E * batch * t.H >= ((int64_t)1 << 31))
        return fail(MBRL_EUNSUPPORTED, "%s: E * batch * horizon = %d * %lld * %d is not below 2^31", what, E,
                    (long long)batch, t.H);
    return MBRL_OK;
}

// One batch's launches (checked arguments; EnsembleBatch, the workspace laid out for `batch` itself): forward,
// backward through time, L + 1 weight-gradient launches, loss.
static hipError_t ol_launch(const TrainShape& t, const mbrl_train_model* members, int E, const mbrl_train_data* data,
                            const int64_t* idx, int64_t idx_stride, int /*bs*/, int batch, float* loss_out, float* ws,
                            const mbrl_nll_bounds* /*bounds*/, hipStream_t stream) {
    const OlPlan p = ol_plan(t, E, batch);
    OlLaunch T{};
    EvalLaunch& A = T.A;
    const int layers = t.L + 1 + t.reward;
    for (int e = 0; e < E; ++e)
        for (int l = 0; l < layers; ++l) {
            A.m[e].w[l] = members[e].weight[l];
            A.m[e].b[l] = members[e].bias[l];
        }
    A.states = data->states; A.actions = data->actions; A.next_states = data->next_states; A.rewards = data->rewards;
    A.rows = idx;
    A.row_err = ws + p.row_err;
    A.row_rew_err = t.reward ? ws + p.row_rew : nullptr;
    A.P = batch;
    A.s = t.s; A.a = t.a; A.W = t.W; A.L = t.L; A.reward = t.reward; A.H = t.H;
    A.ld = p.ld;
    T.idx_stride = idx_stride;
    T.ws_stride = (int64_t)p.stride;
    float* m0 = ws + p.first;
    T.x0 = m0 + p.x0;
    for (int l = 0; l < t.L; ++l) {
        T.act[l] = m0 + p.act[l];
        T.dl[l] = m0 + p.dl[l];
    }
    T.gout = m0 + p.gout;
    for (int l = 0; l <= t.L; ++l) T.cs[l] = m0 + p.cs[l];
    T.scale_s = 2.0f / (float)((int64_t)batch * t.s);
    T.scale_r = 2.0f / (float)batch;
    T.wacc = p.wacc;
    hipError_t err;
    if ((err = ensure_dynamic_lds(reinterpret_cast<const void*>(train_ol_fwd_kernel), OL_LDS_BYTES)) != hipSuccess) return err;
    if ((err = ensure_dynamic_lds(reinterpret_cast<const void*>(train_ol_bwd_kernel), OL_LDS_BYTES)) != hipSuccess) return err;
    const dim3 grid(p.tiles, E);
    hipLaunchKernelGGL(train_ol_fwd_kernel, grid, dim3(OL_THREADS), (size_t)2 * OL_TM * p.ld * sizeof(float), stream, T);
    if ((err = hipGetLastError()) != hipSuccess) return err;
    hipLaunchKernelGGL(train_ol_bwd_kernel, grid, dim3(OL_THREADS), p.lds_bwd, stream, T);
    if ((err = hipGetLastError()) != hipSuccess) return err;
    const TrainEnsemble ens{members, E, (int64_t)p.stride, idx_stride, 3};
    const int K = batch * t.H;
    for (int l = t.L; l >= 0; --l) {
        const float* g = l == t.L ? T.gout : T.dl[l];
        const float* x = l == 0 ? T.x0 : T.act[l - 1];
        if ((err = launch_train_wgrads(t, l, g, x, T.cs[l], p.tiles, K, ens, stream)) != hipSuccess) return err;
    }
    if (!loss_out) return hipSuccess;
    return launch_eval_loss(A.row_err, A.row_rew_err, loss_out, E, batch, t.H, t.s, stream);
}

}  // namespace mbrl

using namespace mbrl;

extern "C" {

size_t mbrl_train_open_loop_workspace_bytes(const mbrl_train_model* members, int32_t E, int32_t batch) {
    TrainShape t;
    const char* what = "train_open_loop_workspace_bytes";
    if (batch < 1 || ensemble_shape(what, members, E, LOSS_OPEN_LOOP, &t) != MBRL_OK || ol_batch_ok(what, E, batch, t) != MBRL_OK)
        return 0;
    return ol_ws_floats(t, E, batch) * sizeof(float);
}

int mbrl_train_grads_open_loop(const mbrl_train_model* members, int32_t E, const mbrl_train_data* data,
                               const int64_t* batch_idx, int32_t batch, float* loss_out, void* workspace,
                               size_t ws_bytes, mbrl_stream_t stream) {
    const char* what = "train_grads_open_loop";
    TrainShape t;
    if (int rc = ensemble_shape(what, members, E, LOSS_OPEN_LOOP, &t)) return rc;
    if (!train_data_ok(data, t) || !batch_idx || !workspace) return fail(MBRL_EINVAL, "%s: NULL argument", what);
    if (reinterpret_cast<uintptr_t>(workspace) & 15) return fail(MBRL_EINVAL, "%s: workspace not 16-byte aligned", what);
    if (batch < 1 || (int64_t)batch > data->transitions)
        return fail(MBRL_EINVAL, "%s: batch %d outside [1, %lld]", what, batch, (long long)data->transitions);
    if (int rc = ensemble_members(what, members, E, t)) return rc;
    if (int rc = ol_batch_ok(what, E, batch, t)) return rc;
    const size_t need = ol_ws_floats(t, E, batch) * sizeof(float);
    if (ws_bytes < need) return fail(MBRL_EWORKSPACE, "%s: workspace %zu < %zu bytes", what, ws_bytes, need);
    return hip_check(ol_launch(t, members, E, data, batch_idx, batch, batch, batch, loss_out,
                               static_cast<float*>(workspace), nullptr, reinterpret_cast<hipStream_t>(stream)), what);
}

int mbrl_train_epoch_open_loop(const mbrl_train_model* members, int32_t E, const mbrl_train_data* data,
                               const int64_t* orders, int64_t rows, int32_t batch_size, const mbrl_adam_tensor* tensors,
                               int32_t count, const mbrl_adam_hparams* hparams, const float* step_sizes,
                               const float* bc2_sqrt, float* losses, void* workspace, size_t ws_bytes,
                               mbrl_stream_t stream) {
    return train_epoch_members("train_epoch_open_loop", LOSS_OPEN_LOOP, false, ol_launch, members, E, data, orders,
                               rows, batch_size, tensors, count, hparams, step_sizes, bc2_sqrt, losses, workspace,
                               ws_bytes, nullptr, nullptr, stream);
}

int mbrl_train_epoch_open_loop_clipped(const mbrl_train_model* members, int32_t E, const mbrl_train_data* data,
                                       const int64_t* orders, int64_t rows, int32_t batch_size,
                                       const mbrl_adam_tensor* tensors, int32_t count, const mbrl_adam_hparams* hparams,
                                       const float* step_sizes, const float* bc2_sqrt, float* losses, void* workspace,
                                       size_t ws_bytes, mbrl_stream_t stream, const mbrl_grad_clip* clip) {
    return train_epoch_members("train_epoch_open_loop_clipped", LOSS_OPEN_LOOP, true, ol_launch, members, E, data,
                               orders, rows, batch_size, tensors, count, hparams, step_sizes, bc2_sqrt, losses,
                               workspace, ws_bytes, clip, nullptr, stream);
}

}  // extern "C"
