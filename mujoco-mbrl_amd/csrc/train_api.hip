// Training ABI entries (include/mbrl_cem.h): argument checks around the launchers of train.hip and adam.hip, for
// one model and for ensembles, and the ensemble epoch driver every loss kind shares (train_open_loop.hip's and
// train_nll.hip's entries call it too).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "mbrl_host.h"
#include "mbrl_train.h"

namespace mbrl {

// open_loop (the open-loop and NLL kinds): the kind bounds n_hidden with its envelope (ol_envelope, nll_envelope:
// MBRL_EUNSUPPORTED) and its launches read no option.
static int train_shape(const char* what, const mbrl_train_model* m, bool open_loop, TrainShape* t) {
    if (!m) return fail(MBRL_EINVAL, "%s: NULL model", what);
    if (m->state_dim < 1 || m->action_dim < 0 || m->hidden < 1 || m->horizon < 1 || m->n_hidden < 1 ||
        (!open_loop && m->n_hidden + 2 > MBRL_TRAIN_MAX_LAYERS) || (m->reward_head != 0 && m->reward_head != 1))
        return fail(MBRL_EINVAL, "%s: bad shape (state %d, action %d, hidden %d x %d, horizon %d, reward %d)", what,
                    m->state_dim, m->action_dim, m->hidden, m->n_hidden, m->horizon, m->reward_head);
    *t = TrainShape{};
    t->s = m->state_dim; t->a = m->action_dim; t->W = m->hidden; t->L = m->n_hidden; t->reward = m->reward_head;
    t->H = m->horizon;
    if (open_loop) return MBRL_OK;
    t->tile = opt(MBRL_OPT_TRAIN_TILE);
    t->fold = opt(MBRL_OPT_TRAIN_NO_FOLD) == 0 ? 1 : 0;
    t->xcd = opt(MBRL_OPT_TRAIN_XCD) == 1 ? 1 : 0;
    t->split = opt(MBRL_OPT_TRAIN_SPLIT) == 1 ? 1 : 0;
    t->fo_split = opt(MBRL_OPT_TRAIN_FO) == 1 ? 1 : 0;
    return MBRL_OK;
}

bool train_data_ok(const mbrl_train_data* data, const TrainShape& t) {
    return data && data->states && data->next_states && (t.a == 0 || data->actions) && (!t.reward || data->rewards);
}

// member < 0: one model, named without a member
static int layers_check(const char* what, const mbrl_train_model& m, const TrainShape& t, int member) {
    for (int l = 0; l < t.L + 1 + t.reward; ++l) {
        if (m.weight[l] && m.bias[l] && m.weight_grad[l] && m.bias_grad[l]) continue;
        if (member < 0) return fail(MBRL_EINVAL, "%s: layer %d: NULL weight, bias or gradient", what, l);
        return fail(MBRL_EINVAL, "%s: member %d, layer %d: NULL weight, bias or gradient", what, member, l);
    }
    return MBRL_OK;
}

static TrainTensors train_tensors(const mbrl_train_model& m, const mbrl_train_data& d) {
    return TrainTensors{m.weight, m.bias, m.weight_grad, m.bias_grad, d.states, d.actions, d.next_states, d.rewards};
}

// ---- ensembles: E members in shared launches (train_gemm_ens_kernel)

int ensemble_shape(const char* what, const mbrl_train_model* members, int32_t E, TrainLoss kind, TrainShape* t) {
    const bool open_loop = kind != LOSS_ONE_STEP;
    if (!members) return fail(MBRL_EINVAL, "%s: NULL members", what);
    if (E < 1) return fail(MBRL_EINVAL, "%s: E = %d members", what, E);
    if (E > MBRL_TRAIN_MAX_MEMBERS)
        return fail(MBRL_EUNSUPPORTED, "%s: E = %d members exceeds MBRL_TRAIN_MAX_MEMBERS = %d", what, E,
                    MBRL_TRAIN_MAX_MEMBERS);
    if (int rc = train_shape(open_loop ? what : "train", &members[0], open_loop, t)) return rc;
    for (int e = 1; e < E; ++e) {
        const mbrl_train_model &a = members[0], &b = members[e];
        if (a.state_dim != b.state_dim || a.action_dim != b.action_dim || a.hidden != b.hidden ||
            a.n_hidden != b.n_hidden || a.reward_head != b.reward_head || a.horizon != b.horizon)
            return fail(MBRL_EINVAL, "%s: member %d's shape differs from member 0's", what, e);
    }
    t->fold = 0;
    t->split = 1;
    t->xcd = 0;
    if (kind == LOSS_NLL && t->reward)
        return fail(MBRL_EINVAL, "%s: the NLL members have one head of 2 * state_dim rows: reward_head must be 0", what);
    return kind == LOSS_OPEN_LOOP ? ol_envelope(what, *t) : kind == LOSS_NLL ? nll_envelope(what, *t) : MBRL_OK;
}

int ensemble_members(const char* what, const mbrl_train_model* members, int32_t E, const TrainShape& t) {
    std::vector<const void*> seen;
    for (int e = 0; e < E; ++e) {
        const mbrl_train_model& m = members[e];
        if (int rc = layers_check(what, m, t, e)) return rc;
        for (int l = 0; l < t.L + 1 + t.reward; ++l)
            seen.insert(seen.end(), {m.weight[l], m.bias[l], m.weight_grad[l], m.bias_grad[l]});
    }
    std::sort(seen.begin(), seen.end());
    if (std::adjacent_find(seen.begin(), seen.end()) != seen.end())
        return fail(MBRL_EINVAL, "%s: a parameter or gradient pointer is bound twice", what);
    return MBRL_OK;
}

// The closed-loop kind's batch (EnsembleBatch): launch_train_grads with the members on a grid axis.
static hipError_t ensemble_batch(const TrainShape& t, const mbrl_train_model* members, int E,
                                 const mbrl_train_data* data, const int64_t* idx, int64_t idx_stride, int bs, int n,
                                 float* loss_out, float* ws, const mbrl_nll_bounds* /*bounds*/, hipStream_t stream) {
    const TrainEnsemble ens{members, E, (int64_t)train_ws_floats(t, bs), idx_stride, 3};
    TrainStep step{};
    step.ens = &ens;
    return launch_train_grads(t, train_tensors(members[0], *data), idx, n, loss_out, ws, stream, step);
}

int train_epoch_members(const char* what, TrainLoss kind, bool clipped, EnsembleBatch launch,
                        const mbrl_train_model* members, int32_t E, const mbrl_train_data* data, const int64_t* orders,
                        int64_t rows, int32_t batch_size, const mbrl_adam_tensor* tensors, int32_t count,
                        const mbrl_adam_hparams* hparams, const float* step_sizes, const float* bc2_sqrt, float* losses,
                        void* workspace, size_t ws_bytes, const mbrl_grad_clip* clip, const mbrl_nll_bounds* bounds,
                        mbrl_stream_t stream) {
    TrainShape t;
    const bool open_loop = kind != LOSS_ONE_STEP;   // (the kinds whose launches read 16 bytes at a time)
    if (int rc = ensemble_shape(what, members, E, kind, &t)) return rc;
    if (!train_data_ok(data, t) || !orders || !workspace || !tensors || count < 1 || !hparams || !step_sizes ||
        !bc2_sqrt)
        return fail(MBRL_EINVAL, "%s: NULL argument", what);
    if (kind == LOSS_NLL && !nll_bounds_ok(bounds)) return fail(MBRL_EINVAL, "%s: NULL log-variance bounds", what);
    if (open_loop && (reinterpret_cast<uintptr_t>(workspace) & 15))
        return fail(MBRL_EINVAL, "%s: workspace not 16-byte aligned", what);
    if (batch_size < 1 || rows < 1 || rows > data->transitions)
        return fail(MBRL_EINVAL, "%s: rows %lld / batch %d outside [1, %lld]", what, (long long)rows, batch_size,
                    (long long)data->transitions);
    if (int rc = ensemble_members(what, members, E, t)) return rc;
    if (int rc = adam_table_check(what, tensors, E, count)) return rc;
    const int bs = (int)std::min<int64_t>(batch_size, rows);
    if (open_loop)
        if (int rc = ol_batch_ok(what, E, bs, t)) return rc;
    const size_t need = (kind == LOSS_OPEN_LOOP ? ol_ws_floats(t, E, bs)
                         : kind == LOSS_NLL     ? nll_ws_floats(t, E, bs)
                                                : (size_t)E * train_ws_floats(t, bs)) * sizeof(float);
    if (ws_bytes < need) return fail(MBRL_EWORKSPACE, "%s: workspace %zu < %zu bytes", what, ws_bytes, need);
    if (clipped)
        if (int rc = grad_clip_check(what, clip, tensors, E, count)) return rc;
    const int total = E * count, ar = adam_arith();
    const hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    std::vector<mbrl_adam_tensor> table(tensors, tensors + total);
    const int64_t batches = (rows + batch_size - 1) / batch_size;
    for (int64_t b = 0; b < batches; ++b) {
        const int n = (int)std::min<int64_t>(batch_size, rows - b * batch_size);
        if (int rc = hip_check(launch(t, members, E, data, orders + b * batch_size, rows, bs, n,
                                      losses ? losses + 3 * (int64_t)E * b : nullptr, static_cast<float*>(workspace),
                                      bounds, st), what))
            return rc;
        for (int i = 0; i < total; ++i) {
            table[i].step_size = step_sizes[b * total + i];
            table[i].bc2_sqrt = bc2_sqrt[b * total + i];
        }
        // every member's step in one launch (64 tensors per launch: E x count beyond that takes more)
        if (int rc = hip_check(clipped ? launch_grad_clip_step(table.data(), E, count, *hparams, ar, *clip, b, st)
                                       : launch_adam_step_ensemble(table.data(), total, *hparams, ar, st), what))
            return rc;
    }
    return MBRL_OK;
}

}  // namespace mbrl

using namespace mbrl;

extern "C" {

#ifdef MBRL_STAMPS
int mbrl_diag_set_train_stamps(void* buf) {
    const hipError_t e = train_gemm_set_stamps(buf);
    return (int)(e != hipSuccess ? e : train_fused_set_stamps(buf));
}
#endif

size_t mbrl_train_workspace_bytes(const mbrl_train_model* model, int32_t batch) {
    TrainShape t;
    if (batch < 1 || train_shape("train", model, false, &t) != MBRL_OK) return 0;
    return train_ws_floats(t, batch) * sizeof(float);
}

size_t mbrl_train_status_offset(const mbrl_train_model* model, int32_t batch) {
    TrainShape t;
    if (batch < 1 || train_shape("train", model, false, &t) != MBRL_OK) return (size_t)-1;
    return train_status_offset(t, batch);
}

int mbrl_train_grads(const mbrl_train_model* model, const mbrl_train_data* data, const int64_t* batch_idx,
                     int32_t batch, float* loss_out, void* workspace, size_t ws_bytes, mbrl_stream_t stream) {
    const char* what = "train_grads";
    TrainShape t;
    if (int rc = train_shape("train", model, false, &t)) return rc;
    if (!train_data_ok(data, t) || !batch_idx || !workspace) return fail(MBRL_EINVAL, "%s: NULL argument", what);
    if (batch < 1 || (int64_t)batch > data->transitions)
        return fail(MBRL_EINVAL, "%s: batch %d outside [1, %lld]", what, batch, (long long)data->transitions);
    if (int rc = layers_check(what, *model, t, -1)) return rc;
    const size_t need = train_ws_floats(t, batch) * sizeof(float);
    if (ws_bytes < need) return fail(MBRL_EWORKSPACE, "%s: workspace %zu < %zu bytes", what, ws_bytes, need);
    const hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (int rc = hip_check(hipMemsetAsync(workspace, 0, train_status_offset(t, batch), st), "train_grads counters"))
        return rc;
    return hip_check(launch_train_grads(t, train_tensors(*model, *data), batch_idx, batch, loss_out,
                                        static_cast<float*>(workspace), st), what);
}

int mbrl_train_epoch(const mbrl_train_model* model, const mbrl_train_data* data, const int64_t* order, int64_t rows,
                     int32_t batch_size, const mbrl_adam_tensor* tensors, int32_t count,
                     const mbrl_adam_hparams* hparams, const float* step_sizes, const float* bc2_sqrt, float* losses,
                     void* workspace, size_t ws_bytes, mbrl_stream_t stream) {
    TrainShape t;
    if (int rc = train_shape("train", model, false, &t)) return rc;
    if (!train_data_ok(data, t) || !order || !workspace || !tensors || count < 1 || !hparams || !step_sizes ||
        !bc2_sqrt)
        return fail(MBRL_EINVAL, "train_epoch: NULL argument");
    if (batch_size < 1 || rows < 1 || rows > data->transitions)
        return fail(MBRL_EINVAL, "train_epoch: rows %lld / batch %d outside [1, %lld]", (long long)rows, batch_size,
                    (long long)data->transitions);
    if (int rc = layers_check("train_epoch", *model, t, -1)) return rc;
    if (int rc = adam_table_check("train_epoch: Adam tensor", tensors, 0, count)) return rc;
    const int layers = t.L + 1 + t.reward;
    const int bs = (int)std::min<int64_t>(batch_size, rows);
    const size_t need = train_ws_floats(t, bs) * sizeof(float);
    if (ws_bytes < need) return fail(MBRL_EWORKSPACE, "train_epoch: workspace %zu < %zu bytes", ws_bytes, need);
    const TrainTensors w = train_tensors(*model, *data);
    const hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    // the tickets and band counters start the epoch at zero whatever the workspace held
    if (int rc = hip_check(hipMemsetAsync(workspace, 0, train_status_offset(t, bs), st), "train_epoch counters"))
        return rc;
    std::vector<mbrl_adam_tensor> table(tensors, tensors + count);
    const int64_t batches = (rows + batch_size - 1) / batch_size;
    // the Adam step rides in the backward launches when the table is the model's layers in order
    // (weight, bias per Linear, gradients = the model's buffers); otherwise a separate launch
    bool fold = count == 2 * layers;
    for (int l = 0; fold && l < layers; ++l)
        fold = tensors[2 * l].param == model->weight[l] && tensors[2 * l].grad == model->weight_grad[l] &&
               tensors[2 * l + 1].param == model->bias[l] && tensors[2 * l + 1].grad == model->bias_grad[l];
    // a layer's step the layer-0 fold defers: carried by the next batch's first launch, or launched
    // after the last batch
    mbrl_adam_tensor carry[2][4];
    // the fused step's F gathers the next batch's rows while it runs when both batches are full-size
    // fused ones (alternating gather slots; the first batch gathers its own)
    TrainGather gather{};
    TrainStep step{};
    step.adam = fold ? table.data() : nullptr;
    step.hp = hparams;
    step.arith = adam_arith();
    step.gather = &gather;
    for (int64_t b = 0; b < batches; ++b) {
        const int n = (int)std::min<int64_t>(batch_size, rows - b * batch_size);
        const int n_next = b + 1 < batches ? (int)std::min<int64_t>(batch_size, rows - (b + 1) * batch_size) : 0;
        const bool hand = n_next == n && t.W > 32 && train_fused_applies(t, n);   // (F's second column tiles)
        gather.idx_next = hand ? order + (b + 1) * batch_size : nullptr;
        gather.batch_next = hand ? n_next : 0;
        for (int i = 0; i < count; ++i) {
            table[i].step_size = step_sizes[b * count + i];
            table[i].bc2_sqrt = bc2_sqrt[b * count + i];
        }
        int next_n = 0;
        step.prior = carry[b & 1];
        step.pending = carry[(b + 1) & 1];
        step.pending_n = &next_n;
        if (int rc = hip_check(launch_train_grads(t, w, order + b * batch_size, n, losses ? losses + 3 * b : nullptr,
                                                  static_cast<float*>(workspace), st, step),
                               "train_epoch grads"))
            return rc;
        gather.pre_rows = hand ? 1 : 0;
        if (hand) gather.slot ^= 1;
        step.prior_n = next_n;
        if (!fold)
            if (int rc = hip_check(launch_adam_step(table.data(), count, *hparams, step.arith, st), "train_epoch adam"))
                return rc;
    }
    if (step.prior_n > 0)
        if (int rc = hip_check(launch_adam_step(carry[batches & 1], step.prior_n, *hparams, step.arith, st),
                               "train_epoch adam tail"))
            return rc;
    return MBRL_OK;
}

size_t mbrl_train_ensemble_workspace_bytes(const mbrl_train_model* members, int32_t E, int32_t batch) {
    TrainShape t;
    if (batch < 1 || ensemble_shape("train_ensemble_workspace_bytes", members, E, LOSS_ONE_STEP, &t) != MBRL_OK) return 0;
    return (size_t)E * train_ws_floats(t, batch) * sizeof(float);
}

int mbrl_train_grads_ensemble(const mbrl_train_model* members, int32_t E, const mbrl_train_data* data,
                              const int64_t* batch_idx, int32_t batch, float* loss_out, void* workspace,
                              size_t ws_bytes, mbrl_stream_t stream) {
    const char* what = "train_grads_ensemble";
    TrainShape t;
    if (int rc = ensemble_shape(what, members, E, LOSS_ONE_STEP, &t)) return rc;
    if (!train_data_ok(data, t) || !batch_idx || !workspace) return fail(MBRL_EINVAL, "%s: NULL argument", what);
    if (batch < 1 || (int64_t)batch > data->transitions)
        return fail(MBRL_EINVAL, "%s: batch %d outside [1, %lld]", what, batch, (long long)data->transitions);
    if (int rc = ensemble_members(what, members, E, t)) return rc;
    const size_t need = (size_t)E * train_ws_floats(t, batch) * sizeof(float);
    if (ws_bytes < need) return fail(MBRL_EWORKSPACE, "%s: workspace %zu < %zu bytes", what, ws_bytes, need);
    return hip_check(ensemble_batch(t, members, E, data, batch_idx, batch, batch, batch, loss_out,
                                    static_cast<float*>(workspace), nullptr, reinterpret_cast<hipStream_t>(stream)), what);
}

int mbrl_train_epoch_ensemble(const mbrl_train_model* members, int32_t E, const mbrl_train_data* data,
                              const int64_t* orders, int64_t rows, int32_t batch_size, const mbrl_adam_tensor* tensors,
                              int32_t count, const mbrl_adam_hparams* hparams, const float* step_sizes,
                              const float* bc2_sqrt, float* losses, void* workspace, size_t ws_bytes,
                              mbrl_stream_t stream) {
    return train_epoch_members("train_epoch_ensemble", LOSS_ONE_STEP, false, ensemble_batch, members, E, data, orders,
                               rows, batch_size, tensors, count, hparams, step_sizes, bc2_sqrt, losses, workspace,
                               ws_bytes, nullptr, nullptr, stream);
}

int mbrl_train_epoch_ensemble_clipped(const mbrl_train_model* members, int32_t E, const mbrl_train_data* data,
                                      const int64_t* orders, int64_t rows, int32_t batch_size,
                                      const mbrl_adam_tensor* tensors, int32_t count, const mbrl_adam_hparams* hparams,
                                      const float* step_sizes, const float* bc2_sqrt, float* losses, void* workspace,
                                      size_t ws_bytes, mbrl_stream_t stream, const mbrl_grad_clip* clip) {
    return train_epoch_members("train_epoch_ensemble_clipped", LOSS_ONE_STEP, true, ensemble_batch, members, E, data,
                               orders, rows, batch_size, tensors, count, hparams, step_sizes, bc2_sqrt, losses,
                               workspace, ws_bytes, clip, nullptr, stream);
}

}  // extern "C"
