// Held-out evaluation of ensemble members and keep-best snapshots (include/mbrl_cem.h
// mbrl_eval_members, mbrl_keep_best): what EnsembleModel.fit_members enqueues after every training
// epoch, with no host round trip and no scratch memory.
//
// mbrl_eval_members, launch 1 (eval_rows_kernel): grid (row tiles, members). A workgroup owns EVAL_TM = 16
// positions p = r * horizon + h of one member, gathers their inputs through `rows` into LDS and runs the
// whole MLP with the activations in two LDS buffers of 16 x ld floats that alternate from layer to layer;
// nothing of size R x W goes to memory. A layer is C^T = W . X^T on v_mfma_f32_16x16x4f32 with the weights
// as the A operand (lane l: neuron 16 nb + l % 16) and the activations as B (position l % 16), so that a
// lane ends with four consecutive neurons of one position: one 16-byte LDS store, and the next layer reads
// its k-contiguous 16 bytes back. Lane l takes k = kb + 4 (l / 16) + i in the i-th MFMA of a 16-deep chunk
// (train.hip's assignment: one 16-byte load feeds four MFMAs). The four waves split the layer's 16-neuron
// blocks; no wave splits K, so every output element is one k-ordered fma chain that depends on its own
// position's inputs alone: the result of a (member, row, step) is the same bits wherever it sits in
// whichever call. Weight rows are read from the live nn.Linear buffers, 16 bytes at a time where the
// pointer and K allow it and element by element otherwise (the same values in the same order). The state
// head and the reward head run as one output layer of s (+ 1) neurons; the squared error is then reduced
// per position, j ascending, by one lane, and only R x horizon floats per member are stored.
// Launch 2 (eval_loss_kernel, skipped without loss_out): one workgroup per member, the order documented
// in the header.
//
// mbrl_eval_members_open_loop, launch 1 (eval_open_loop_kernel): grid (row tiles, members). A workgroup owns
// EVAL_TM = 16 rows r of one member and runs the horizon loop itself: the same layer chain per step, in the
// same two LDS buffers, and between two steps the seam, built in place in the buffer that holds the outputs
// (it alternates with the parity of L): the predicted state stays where the output layer put it, columns
// 0 .. s - 1, and every column from s to the end of layer 0's last 16-deep chunk is rewritten -- the next
// step's actions, then zeros -- so that neither the reward head's output in column s nor an earlier layer's
// hidden activations further right reach layer 0. The error lanes and the pred_out stores read the outputs
// before a barrier, the rewrite follows it, and a second barrier stands before layer 0. The next actions are
// loaded from global memory at the seam, not ahead of it: their latency is covered by the other workgroups
// of the compute unit, not by this one's layers. Every output element is still one k-ordered fma chain over
// its own row's inputs, so the bytes of a (member, row, step) depend on nothing else.
// Launch 2: eval_loss_kernel on the open-loop row errors.
//
// mbrl_keep_best: copy launches that read loss and best_loss only, then the launch that updates
// best_loss, best_epoch and stale; the stream orders them, so no copy sees an updated best_loss.
#include "eval_mlp.h"

namespace mbrl {

constexpr int EVAL_TM = 16;        // (r, h) positions per workgroup: the MFMA's 16 columns
constexpr int EVAL_LOSS_THREADS = 1024;

__global__ __launch_bounds__(64 * EVAL_WAVES) void eval_rows_kernel(const EvalLaunch A) {
    extern __shared__ __attribute__((aligned(16))) float eval_lds[];
    const int ld = A.ld, tid = threadIdx.x, e = blockIdx.y;
    float* buf[2] = {eval_lds, eval_lds + EVAL_TM * ld};
    const int64_t p0 = (int64_t)blockIdx.x * EVAL_TM;
    const EvalMember& M = A.m[e];
    const int K0 = A.s + A.a, K0p = (K0 + 15) & ~15;
    // the tile's inputs (states, actions) through `rows`; zeros past K0 and for positions past P
    for (int idx = tid; idx < EVAL_TM * K0p; idx += 64 * EVAL_WAVES) {
        const int row = idx / K0p, k = idx - row * K0p;
        const int64_t p = p0 + row;
        float v = 0.0f;
        if (p < A.P && k < K0) {
            const int64_t r = p / A.H, h = p - r * A.H;
            const int64_t at = A.rows[r] * A.H + h;
            v = k < A.s ? A.states[at * A.s + k] : A.actions[at * A.a + (k - A.s)];
        }
        buf[0][row * ld + k] = v;
    }
    __syncthreads();
    int cur = 0;
    for (int l = 0; l < A.L; ++l) {
        eval_layer<true>(buf[cur], buf[cur ^ 1], ld, M.w[l], M.b[l], A.W, nullptr, nullptr, 0, l == 0 ? K0 : A.W);
        cur ^= 1;
        __syncthreads();
    }
    eval_layer<false>(buf[cur], buf[cur ^ 1], ld, M.w[A.L], M.b[A.L], A.s, A.reward ? M.w[A.L + 1] : nullptr,
                      A.reward ? M.b[A.L + 1] : nullptr, A.reward ? 1 : 0, A.W);
    cur ^= 1;
    __syncthreads();
    if (tid < EVAL_TM && p0 + tid < A.P) {
        const int64_t p = p0 + tid;
        const int64_t r = p / A.H, h = p - r * A.H;
        const int64_t at = A.rows[r] * A.H + h;
        const float* y = buf[cur] + tid * ld;
        const float* target = A.next_states + at * A.s;
        float sum = 0.0f;
        for (int j = 0; j < A.s; ++j) {
            const float d = y[j] - target[j];
            sum = sum + d * d;                            // (-ffp-contract=off: a product, then a sum)
        }
        A.row_err[(int64_t)e * A.P + p] = sum;
        if (A.reward) {
            const float d = y[A.s] - A.rewards[at];
            A.row_rew_err[(int64_t)e * A.P + p] = d * d;
        }
    }
}

// Open loop: the tile's 16 rows of one member through all H steps, x_{h+1} = s^_{h+1} (see the top of the file).
// A.P is R here, and row_err / row_rew_err / pred_out are [E][R][H](, [s]).
__global__ __launch_bounds__(64 * EVAL_WAVES) void eval_open_loop_kernel(const EvalLaunch A, float* __restrict__ pred_out) {
    extern __shared__ __attribute__((aligned(16))) float eval_lds[];
    const int ld = A.ld, tid = threadIdx.x, e = blockIdx.y;
    float* buf[2] = {eval_lds, eval_lds + EVAL_TM * ld};
    const int64_t r0 = (int64_t)blockIdx.x * EVAL_TM, R = A.P;
    const EvalMember& M = A.m[e];
    const int K0 = A.s + A.a, K0p = (K0 + 15) & ~15, tail = K0p - A.s;
    // x_0 = states[i][0]; rows past R run on zeros and store nothing
    for (int idx = tid; idx < EVAL_TM * A.s; idx += 64 * EVAL_WAVES) {
        const int row = idx / A.s, k = idx - row * A.s;
        buf[0][row * ld + k] = r0 + row < R ? A.states[A.rows[r0 + row] * A.H * A.s + k] : 0.0f;
    }
    int cur = 0;
    for (int h = 0; h < A.H; ++h) {
        // columns s .. K0p - 1 of the input: step h's actions, then zeros (over the reward head's output and
        // whatever an earlier layer left there)
        for (int idx = tid; idx < EVAL_TM * tail; idx += 64 * EVAL_WAVES) {
            const int row = idx / tail, k = idx - row * tail;
            float v = 0.0f;
            if (k < A.a && r0 + row < R) v = A.actions[(A.rows[r0 + row] * A.H + h) * A.a + k];
            buf[cur][row * ld + A.s + k] = v;
        }
        __syncthreads();
        cur = eval_forward(A, M, buf, cur);
        if (tid < EVAL_TM && r0 + tid < R) {
            const int64_t at = A.rows[r0 + tid] * A.H + h;
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
        if (pred_out) {
            for (int idx = tid; idx < EVAL_TM * A.s; idx += 64 * EVAL_WAVES) {
                const int row = idx / A.s, j = idx - row * A.s;
                if (r0 + row < R) pred_out[(((int64_t)e * R + r0 + row) * A.H + h) * A.s + j] = buf[cur][row * ld + j];
            }
        }
        __syncthreads();                                  // the outputs are read: the next step may overwrite column s
    }
}

// loss_out[e] = (state + reward, state, reward): per step h, lane t adds r = t, t + 1024, .. ascending,
// the partials meet pairwise (d = 512 .. 1), the mean is taken and the steps are added h ascending.
__global__ __launch_bounds__(EVAL_LOSS_THREADS) void eval_loss_kernel(const float* __restrict__ row_err,
                                                                      const float* __restrict__ row_rew_err,
                                                                      float* __restrict__ loss_out, int64_t R, int H,
                                                                      int s) {
    __shared__ float part[EVAL_LOSS_THREADS];
    const int e = blockIdx.x, t = threadIdx.x;
    float total[2] = {0.0f, 0.0f};
    for (int which = 0; which < (row_rew_err ? 2 : 1); ++which) {
        const float* src = (which ? row_rew_err : row_err) + (int64_t)e * R * H;
        const float denom = which ? (float)R : (float)((double)R * (double)s);
        for (int h = 0; h < H; ++h) {
            float acc = 0.0f;
            for (int64_t r = t; r < R; r += EVAL_LOSS_THREADS) acc += src[r * H + h];
            part[t] = acc;
            __syncthreads();
            for (int d = EVAL_LOSS_THREADS / 2; d >= 1; d >>= 1) {
                if (t < d) part[t] += part[t + d];
                __syncthreads();
            }
            if (t == 0) total[which] += part[0] / denom;
            __syncthreads();
        }
    }
    if (t == 0) {
        loss_out[3 * e + 0] = total[0] + total[1];
        loss_out[3 * e + 1] = total[0];
        loss_out[3 * e + 2] = total[1];
    }
}

// ---- keep-best snapshots
constexpr int COPY_TENSORS = 64;                 // tensors per launch (the table travels in the arguments)
constexpr int COPY_THREADS = 256;
constexpr int COPY_CHUNK = COPY_THREADS * 4;     // elements per workgroup (16 bytes per lane)

struct CopyLaunch {
    const float* src[COPY_TENSORS];
    float* dst[COPY_TENSORS];
    int64_t numel[COPY_TENSORS];
    int member[COPY_TENSORS];
    int first_block[COPY_TENSORS + 1];           // workgroup prefix over the tensors' chunks
    int count;
    int loss_stride;
    const float* loss;
    const float* best_loss;
};

__global__ __launch_bounds__(COPY_THREADS) void keep_best_copy_kernel(const CopyLaunch L) {
    const int blk = blockIdx.x;
    int ti = 0;
    while (ti + 1 < L.count && blk >= L.first_block[ti + 1]) ++ti;
    const int e = L.member[ti];
    if (!(L.loss[(int64_t)e * L.loss_stride] < L.best_loss[e])) return;    // (a NaN is never better)
    // bit for bit: the words move as integers
    const uint32_t* src = reinterpret_cast<const uint32_t*>(L.src[ti]);
    uint32_t* dst = reinterpret_cast<uint32_t*>(L.dst[ti]);
    const int64_t n = L.numel[ti];
    const int64_t i0 = (int64_t)(blk - L.first_block[ti]) * COPY_CHUNK + 4 * (int64_t)threadIdx.x;
    if (i0 >= n) return;
    if (i0 + 4 <= n && ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15) == 0) {
        *reinterpret_cast<uint4*>(dst + i0) = *reinterpret_cast<const uint4*>(src + i0);
        return;
    }
    for (int64_t i = i0; i < i0 + 4 && i < n; ++i) dst[i] = src[i];
}

__global__ void keep_best_decide_kernel(const float* __restrict__ loss, int loss_stride, int E, int epoch,
                                        float* __restrict__ best_loss, int* __restrict__ best_epoch,
                                        int* __restrict__ stale) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    const float v = loss[(int64_t)e * loss_stride];
    if (v < best_loss[e]) {
        best_loss[e] = v;
        best_epoch[e] = epoch;
        stale[e] = 0;
    } else {
        stale[e] += 1;
    }
}

static hipError_t launch_keep_best_copies(const float* loss, int loss_stride, const float* best_loss,
                                          const mbrl_copy_tensor* tensors, int E, int count, hipStream_t stream) {
    CopyLaunch L{};
    L.loss = loss;
    L.loss_stride = loss_stride;
    L.best_loss = best_loss;
    const int total = E * count;
    int blocks = 0;
    for (int i = 0; i <= total; ++i) {
        // launch when the table is full or the tensors are exhausted
        if (L.count == COPY_TENSORS || (i == total && L.count > 0)) {
            L.first_block[L.count] = blocks;
            hipLaunchKernelGGL(keep_best_copy_kernel, dim3(blocks), dim3(COPY_THREADS), 0, stream, L);
            const hipError_t err = hipGetLastError();
            if (err != hipSuccess) return err;
            L.count = 0;
            blocks = 0;
        }
        if (i == total || tensors[i].numel <= 0) continue;
        L.src[L.count] = tensors[i].src;
        L.dst[L.count] = tensors[i].dst;
        L.numel[L.count] = tensors[i].numel;
        L.member[L.count] = i / count;
        L.first_block[L.count] = blocks;
        blocks += (int)((tensors[i].numel + COPY_CHUNK - 1) / COPY_CHUNK);
        ++L.count;
    }
    return hipSuccess;
}

// The argument checks of mbrl_eval_members and mbrl_eval_members_open_loop (all before any launch) and the
// launch arguments both share; A.P is left to the caller.
static int eval_prepare(const char* what, const mbrl_train_model* members, int32_t E, const mbrl_train_data* data,
                        const int64_t* rows, int64_t R, float* row_err, float* row_rew_err, EvalLaunch& A) {
    if (!members || !data || !rows || !row_err) return fail(MBRL_EINVAL, "%s: NULL members, data, rows or row_err", what);
    if (E < 1 || R < 1) return fail(MBRL_EINVAL, "%s: E = %d members, R = %lld rows", what, E, (long long)R);
    if (E > MBRL_TRAIN_MAX_MEMBERS)
        return fail(MBRL_EUNSUPPORTED, "%s: E = %d members exceeds MBRL_TRAIN_MAX_MEMBERS = %d", what, E,
                    MBRL_TRAIN_MAX_MEMBERS);
    const mbrl_train_model& m0 = members[0];
    if (m0.state_dim < 1 || m0.action_dim < 0 || m0.hidden < 1 || m0.horizon < 1 || m0.n_hidden < 1 ||
        (m0.reward_head != 0 && m0.reward_head != 1))
        return fail(MBRL_EINVAL, "%s: bad shape (state %d, action %d, hidden %d x %d, horizon %d, reward %d)", what,
                    m0.state_dim, m0.action_dim, m0.hidden, m0.n_hidden, m0.horizon, m0.reward_head);
    for (int e = 1; e < E; ++e) {
        const mbrl_train_model& b = members[e];
        if (m0.state_dim != b.state_dim || m0.action_dim != b.action_dim || m0.hidden != b.hidden ||
            m0.n_hidden != b.n_hidden || m0.reward_head != b.reward_head || m0.horizon != b.horizon)
            return fail(MBRL_EINVAL, "%s: member %d's shape differs from member 0's", what, e);
    }
    if (m0.n_hidden + 2 > MBRL_TRAIN_MAX_LAYERS || m0.hidden > MBRL_EVAL_MAX_DIM || m0.state_dim > MBRL_EVAL_MAX_DIM ||
        m0.action_dim > MBRL_EVAL_MAX_DIM || m0.state_dim + m0.action_dim > MBRL_EVAL_MAX_DIM)
        return fail(MBRL_EUNSUPPORTED, "%s: shape outside the envelope (state %d, action %d, hidden %d x %d; each of "
                    "state, state + action and hidden <= %d, n_hidden <= %d)", what, m0.state_dim, m0.action_dim, m0.hidden,
                    m0.n_hidden, MBRL_EVAL_MAX_DIM, MBRL_TRAIN_MAX_LAYERS - 2);
    if (!data->states || !data->next_states || (m0.action_dim > 0 && !data->actions) ||
        (m0.reward_head && !data->rewards))
        return fail(MBRL_EINVAL, "%s: NULL transitions", what);
    if ((m0.reward_head != 0) != (row_rew_err != nullptr))
        return fail(MBRL_EINVAL, "%s: row_rew_err is required with a reward head and must be NULL without", what);
    const int layers = m0.n_hidden + 1 + m0.reward_head;
    for (int e = 0; e < E; ++e)
        for (int l = 0; l < layers; ++l)
            if (!members[e].weight[l] || !members[e].bias[l])
                return fail(MBRL_EINVAL, "%s: member %d, layer %d: NULL weight or bias", what, e, l);
    if (R >= ((int64_t)1 << 31) || (int64_t)E * R * m0.horizon >= ((int64_t)1 << 31))
        return fail(MBRL_EUNSUPPORTED, "%s: E * R * horizon = %d * %lld * %d is not below 2^31", what, E, (long long)R,
                    m0.horizon);

    for (int e = 0; e < E; ++e)
        for (int l = 0; l < layers; ++l) {
            A.m[e].w[l] = members[e].weight[l];
            A.m[e].b[l] = members[e].bias[l];
        }
    A.states = data->states;
    A.actions = data->actions;
    A.next_states = data->next_states;
    A.rewards = data->rewards;
    A.rows = rows;
    A.row_err = row_err;
    A.row_rew_err = row_rew_err;
    A.s = m0.state_dim; A.a = m0.action_dim; A.W = m0.hidden; A.L = m0.n_hidden; A.reward = m0.reward_head;
    A.H = m0.horizon;
    A.ld = eval_ld(A.s, A.a, A.W, A.reward);
    return MBRL_OK;
}

// the row errors' launch (grid: row tiles x members, the two activation buffers in dynamic LDS), then the losses
template <typename... Extra>
static int eval_launch(const char* what, void (*kernel)(EvalLaunch, Extra...), const EvalLaunch& A, int32_t E,
                       int64_t tile_items, int64_t R, float* loss_out, mbrl_stream_t stream, Extra... extra) {
    const size_t lds = (size_t)2 * EVAL_TM * A.ld * sizeof(float);
    const hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (int rc = hip_check(ensure_dynamic_lds(reinterpret_cast<const void*>(kernel), 160 * 1024), what)) return rc;
    const unsigned tiles = (unsigned)((tile_items + EVAL_TM - 1) / EVAL_TM);
    hipLaunchKernelGGL(kernel, dim3(tiles, E), dim3(64 * EVAL_WAVES), lds, st, A, extra...);
    if (int rc = hip_check(hipGetLastError(), what)) return rc;
    if (!loss_out) return MBRL_OK;
    return hip_check(launch_eval_loss(A.row_err, A.row_rew_err, loss_out, E, R, A.H, A.s, st), what);
}

hipError_t launch_eval_loss(const float* row_err, const float* row_rew_err, float* loss_out, int E, int64_t R, int H,
                            int s, hipStream_t stream) {
    hipLaunchKernelGGL(eval_loss_kernel, dim3(E), dim3(EVAL_LOSS_THREADS), 0, stream, row_err, row_rew_err, loss_out, R,
                       H, s);
    return hipGetLastError();
}

}  // namespace mbrl

using namespace mbrl;

// ---- ABI entries (include/mbrl_cem.h)
extern "C" {

int mbrl_eval_members(const mbrl_train_model* members, int32_t E, const mbrl_train_data* data,
                      const int64_t* rows, int64_t R, float* row_err, float* row_rew_err, float* loss_out,
                      mbrl_stream_t stream) {
    const char* what = "eval_members";
    EvalLaunch A{};
    if (int rc = eval_prepare(what, members, E, data, rows, R, row_err, row_rew_err, A)) return rc;
    A.P = R * A.H;
    return eval_launch(what, eval_rows_kernel, A, E, A.P, R, loss_out, stream);
}

int mbrl_eval_members_open_loop(const mbrl_train_model* members, int32_t E, const mbrl_train_data* data,
                                const int64_t* rows, int64_t R, float* row_err, float* row_rew_err,
                                float* pred_out, float* loss_out, mbrl_stream_t stream) {
    const char* what = "eval_members_open_loop";
    EvalLaunch A{};
    if (int rc = eval_prepare(what, members, E, data, rows, R, row_err, row_rew_err, A)) return rc;
    A.P = R;
    return eval_launch(what, eval_open_loop_kernel, A, E, R, R, loss_out, stream, pred_out);
}

int mbrl_keep_best(const float* loss, int32_t loss_stride, int32_t E, int32_t epoch, float* best_loss,
                   int32_t* best_epoch, int32_t* stale, const mbrl_copy_tensor* tensors, int32_t count,
                   mbrl_stream_t stream) {
    const char* what = "keep_best";
    if (!loss || !best_loss || !best_epoch || !stale) return fail(MBRL_EINVAL, "%s: NULL argument", what);
    if (E < 1 || loss_stride < 1 || epoch < 0 || count < 0 || (count > 0 && !tensors))
        return fail(MBRL_EINVAL, "%s: E = %d, loss_stride = %d, epoch = %d, count = %d%s", what, E, loss_stride, epoch,
                    count, count > 0 && !tensors ? " with a NULL table" : "");
    if ((int64_t)E * count >= ((int64_t)1 << 31)) return fail(MBRL_EUNSUPPORTED, "%s: E * count is not below 2^31", what);
    int64_t blocks = 0;
    for (int i = 0; i < E * count; ++i) {
        const mbrl_copy_tensor& t = tensors[i];
        if (t.numel < 0 || (t.numel > 0 && (!t.src || !t.dst)))
            return fail(MBRL_EINVAL, "%s: member %d, tensor %d: NULL pointer or negative numel", what, i / count, i % count);
        blocks = std::max(blocks, (t.numel + COPY_CHUNK - 1) / COPY_CHUNK);
    }
    if (blocks * COPY_TENSORS >= ((int64_t)1 << 31))
        return fail(MBRL_EUNSUPPORTED, "%s: a tensor is too large for one launch's grid", what);
    const hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (int rc = hip_check(launch_keep_best_copies(loss, loss_stride, best_loss, tensors, E, count, st), what)) return rc;
    hipLaunchKernelGGL(keep_best_decide_kernel, dim3((E + 63) / 64), dim3(64), 0, st, loss, loss_stride, E, epoch,
                       best_loss, best_epoch, stale);
    return hip_check(hipGetLastError(), what);
}

}  // extern "C"
