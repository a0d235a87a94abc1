// Trajectory-sampling rollouts of probabilistic ensemble members (include/mbrl_cem.h mbrl_rollout_cost_ts,
// mbrl_cem_plan_ts): PETS' TS-inf. Every candidate is rolled out as Q = E * P particles; particle row
// q = e * P + p stays on member e for the whole horizon and, at every step, takes its next state from the
// member's predicted Gaussian. The definition, operation by operation, is in the header.
//
// rollout_ts_kernel: grid (16-candidate tiles, Q), eval_open_loop_kernel's structure (eval.hip) with
// nll_fwd_kernel's head (train_nll.hip). A workgroup owns 16 candidates of one particle row and runs the horizon
// loop itself: the activations alternate between two LDS buffers of 16 x ld floats, every layer is eval_layer
// (eval_mlp.h) reading the member's live nn.Linear buffers, the head is one output layer of 2 s rows (mean, then
// raw log-variance), so every output element is one k-ordered fma chain over its own candidate's inputs. After
// the head, one thread per (candidate, group of four state dimensions) draws the group's four normals (one
// Philox4x32-10 call, two Box-Muller pairs), forms the sampled state and writes, in place, the next step's
// normalised input over the mean's columns 0 .. s - 1, the goal-state cost term of each dimension to the same
// columns of the other buffer (the head's input there has been read) and the state to states_out. Behind a
// barrier one lane per candidate adds the s cost terms j ascending, the action term d ascending from the raw
// actions, and the step's cost to its running total, t ascending. The seam then rewrites columns s to the end of
// layer 0's last 16-deep chunk -- the next step's normalised actions, then zeros -- over the raw log-variances.
// Candidates past N run on zero inputs and store nothing. No workgroup waits on another, nothing is accumulated
// with atomics, there is no workspace: the bytes of a (row, candidate) depend on its own inputs, its member's
// parameters and its counter words alone.
//
// Member modes (mbrl_rollout_cost_ts_rows): FIXED is the row layout above. RESAMPLED is PETS' TS-1: Q rows in all,
// independent of E, and row q runs, at step t, the member drawn from Philox counter (0, t, q, (iteration << 8) |
// 0xFF) -- a group byte no state-noise counter has. The draw has workgroup-uniform inputs: every wave computes it
// once per step and indexes the member table the launch already carries. No wait, atomic or workspace is added.
//
// mbrl_cem_plan_ts: mbrl_cem_plan's loop (plan.hip cem_plan_run) with the sampled rollout in place of
// rollout_impl and Q cost rows in place of E; the plan-loop helpers are mbrl_plan.h's.
//
// mbrl_cem_plan_ts_rh / mbrl_cem_plan_ts_rh_batch: the receding-horizon loop of plan.hip (rh_plan) with this
// rollout as its source (mbrl_plan.h TsSource): warm start, kept rows and batches on sampled rows.
#include <math.h>

#include "eval_mlp.h"
#include "mbrl_plan.h"
#include "mbrl_rng.h"
#include "mbrl_train.h"

namespace mbrl {

constexpr int TS_TM = 16;                      // candidates per workgroup: the MFMA's 16 columns
constexpr int TS_THREADS = 64 * EVAL_WAVES;
constexpr int TS_LDS_BYTES = 160 * 1024;       // the NLL entries' envelope: two buffers of 16 x ld floats

struct TsLaunch {
    EvalMember m[MBRL_TRAIN_MAX_MEMBERS];
    const float *min_lv, *max_lv;              // [s]
    const float *obs_mean, *obs_std, *act_mean, *act_std;
    const float *cw, *goal;                    // [s] (has_sc)
    const float* s0;                           // [s], or [N][s] with s0_per_cand
    const float* actions;                      // [H][N][a]
    float* costs;                              // [Q][N]
    float* states_out;                         // [Q][H][N][s] or NULL
    int32_t* members_out;                      // [Q][H] or NULL: the member each row ran at each step
    uint64_t noise_seed;
    float noise_scale, alpha_s, alpha_s2, alpha_a, alpha_a2;
    int norm_s, unnorm_s, norm_a, has_sc, has_ac, s0_per_cand;
    int s, a, W, L, ld, N, H, n_offset, P, iteration;
    int E, resampled;                          // resampled: MBRL_TS_MEMBER_RESAMPLED (P is then not read)
};

// max(x, 0) + log1p(exp(-|x|)): train_nll.hip's nll_softplus
__device__ __forceinline__ float ts_softplus(float x) { return fmaxf(x, 0.0f) + log1pf(expf(-fabsf(x))); }

__global__ __launch_bounds__(TS_THREADS) void rollout_ts_kernel(const TsLaunch T) {
    extern __shared__ __attribute__((aligned(16))) float ts_lds[];
    const int ld = T.ld, tid = threadIdx.x, row_q = blockIdx.y, s = T.s, a = T.a;
    float* buf[2] = {ts_lds, ts_lds + TS_TM * ld};
    const int64_t n0 = (int64_t)blockIdx.x * TS_TM;
    const int nvalid = (int)min((int64_t)TS_TM, (int64_t)T.N - n0);
    const int K0 = s + a, K0p = (K0 + 15) & ~15, tail = K0p - s, G = (s + 3) >> 2;
    // x_0: normalize_state(s0); candidates past N run on zeros and store nothing
    for (int idx = tid; idx < TS_TM * s; idx += TS_THREADS) {
        const int row = idx / s, k = idx - row * s;
        float v = 0.0f;
        if (row < nvalid) {
            const float sv = T.s0_per_cand ? T.s0[(n0 + row) * s + k] : T.s0[k];
            v = T.norm_s ? (sv - T.obs_mean[k]) / T.obs_std[k] : sv;
        }
        buf[0][row * ld + k] = v;
    }
    int cur = 0;
    float total = 0.0f;                                   // lanes tid < nvalid: their candidate's return
    for (int t = 0; t < T.H; ++t) {
        // this step's member: the row's own, or the step's draw (uniform over the workgroup, kept in a scalar)
        int e = T.resampled ? 0 : row_q / T.P;
        if (T.resampled) {
            const u32x4 w = philox4x32_10(u32x4{0u, (uint32_t)t, (uint32_t)row_q, ((uint32_t)T.iteration << 8) | 0xFFu},
                                          (uint32_t)T.noise_seed, (uint32_t)(T.noise_seed >> 32));
            e = __builtin_amdgcn_readfirstlane((int)__umulhi(w.x, (uint32_t)T.E));
        }
        const EvalMember& M = T.m[e];
        if (T.members_out && blockIdx.x == 0 && tid == 0) T.members_out[(int64_t)row_q * T.H + t] = e;
        // columns s .. K0p - 1 of the input: normalize_action(a_t), then zeros (over the raw log-variances and
        // whatever an earlier layer left there)
        for (int idx = tid; idx < TS_TM * tail; idx += TS_THREADS) {
            const int row = idx / tail, k = idx - row * tail;
            float v = 0.0f;
            if (k < a && row < nvalid) {
                const float x = T.actions[((int64_t)t * T.N + n0 + row) * a + k];
                v = T.norm_a ? (x - T.act_mean[k]) / T.act_std[k] : x;
            }
            buf[cur][row * ld + s + k] = v;
        }
        __syncthreads();
        for (int l = 0; l < T.L; ++l) {
            eval_layer<true>(buf[cur], buf[cur ^ 1], ld, M.w[l], M.b[l], T.W, nullptr, nullptr, 0, l == 0 ? K0 : T.W);
            cur ^= 1;
            __syncthreads();
        }
        eval_layer<false>(buf[cur], buf[cur ^ 1], ld, M.w[T.L], M.b[T.L], 2 * s, nullptr, nullptr, 0, T.W);
        cur ^= 1;
        __syncthreads();
        // per (candidate, four dimensions): the sampled state. Reads columns j and s + j of its own row, writes
        // column j of both buffers: no thread reads what another writes here.
        float* out = buf[cur];
        float* terms = buf[cur ^ 1];
        for (int idx = tid; idx < TS_TM * G; idx += TS_THREADS) {
            const int row = idx / G, g = idx - row * G;
            if (row >= nvalid) {
                for (int j = 4 * g; j < min(4 * g + 4, s); ++j) out[row * ld + j] = 0.0f;
                continue;
            }
            const int64_t n = n0 + row;
            const u32x4 w = philox4x32_10(u32x4{(uint32_t)(n + T.n_offset), (uint32_t)t, (uint32_t)row_q,
                                                ((uint32_t)T.iteration << 8) | (uint32_t)g},
                                          (uint32_t)T.noise_seed, (uint32_t)(T.noise_seed >> 32));
            float eps[4];
            box_muller(w.x, w.y, eps[0], eps[1]);
            box_muller(w.z, w.w, eps[2], eps[3]);
            for (int i = 0; i < 4; ++i) {
                const int j = 4 * g + i;
                if (j >= s) break;
                const float mean = out[row * ld + j], raw = out[row * ld + s + j];
                const float lo = T.min_lv[j], hi = T.max_lv[j];
                const float u = hi - ts_softplus(hi - raw);
                const float lv = lo + ts_softplus(u - lo);
                const float sd = expf(0.5f * lv) * T.noise_scale;
                const float z = mean + sd * eps[i];
                const float sn = T.unnorm_s ? z * T.obs_std[j] + T.obs_mean[j] : z;
                if (T.has_sc) {
                    const float x = (sn - T.goal[j]) * T.cw[j];
                    terms[row * ld + j] = sqrtf(x * x + T.alpha_s2) - T.alpha_s;
                }
                out[row * ld + j] = T.norm_s ? (sn - T.obs_mean[j]) / T.obs_std[j] : sn;
                if (T.states_out) T.states_out[(((int64_t)row_q * T.H + t) * T.N + n) * s + j] = sn;
            }
        }
        __syncthreads();
        // c_t = sum_j state terms (j ascending) + alpha_a^2 * (sum_d (cosh(a_d / alpha_a) - 1) (d ascending) / a)
        if (tid < nvalid) {
            float sc = 0.0f, ac = 0.0f;
            if (T.has_sc) {
                const float* v = terms + tid * ld;
                for (int j = 0; j < s; ++j) sc = sc + v[j];
            }
            if (T.has_ac) {
                const float* x = T.actions + ((int64_t)t * T.N + n0 + tid) * a;
                float acc = 0.0f;
                for (int d = 0; d < a; ++d) acc = acc + (coshf(x[d] / T.alpha_a) - 1.0f);
                ac = T.alpha_a2 * (acc / (float)a);
            }
            total = total + (sc + ac);
        }
        // (the next seam writes this buffer's columns from s on, which the threads above have read before the
        // barrier; the lanes' reads of `terms` end before the barrier that precedes layer 0's stores to it)
    }
    if (tid < nvalid) T.costs[(int64_t)row_q * T.N + n0 + tid] = total;
}

static int ts_ld(const TrainShape& t) {
    const int widest = std::max(t.W, std::max(t.s + t.a, 2 * t.s));
    return ((widest + 15) & ~15) + EVAL_PAD;
}

// Every argument check of mbrl_rollout_cost_ts (all before any launch) and the launch arguments. member_mode:
// mbrl_rollout_cost_ts_rows' (FIXED: the entry above). *Q: the launch's row count.
static int ts_prepare(const char* what, const mbrl_train_model* members, int32_t E, const mbrl_nll_bounds* bounds,
                      const mbrl_norm* norm, const mbrl_cost* cost, const float* s0, int s0_per_cand,
                      const float* actions, int N, int H, int n_offset, const mbrl_ts_params* ts, float* costs,
                      float* states_out, TsLaunch& T, int member_mode = MBRL_TS_MEMBER_FIXED,
                      int32_t* members_out = nullptr, int* Q = nullptr) {
    if (!members || !s0 || !actions || !ts || !costs)
        return fail(MBRL_EINVAL, "%s: NULL members, s0, actions, ts or costs", what);
    if (N < 1 || H < 1 || n_offset < 0) return fail(MBRL_EINVAL, "%s: N = %d, H = %d, n_offset = %d", what, N, H, n_offset);
    if (E < 1 || E > MBRL_TRAIN_MAX_MEMBERS)
        return fail(MBRL_EINVAL, "%s: E = %d members outside [1, MBRL_TRAIN_MAX_MEMBERS = %d]", what, E,
                    MBRL_TRAIN_MAX_MEMBERS);
    if (member_mode != MBRL_TS_MEMBER_FIXED && member_mode != MBRL_TS_MEMBER_RESAMPLED)
        return fail(MBRL_EINVAL, "%s: member_mode %d", what, member_mode);
    const bool resampled = member_mode == MBRL_TS_MEMBER_RESAMPLED;
    if (resampled && (ts->particles < 1 || ts->particles > MBRL_TS_MAX_ROWS))
        return fail(MBRL_EINVAL, "%s: %d resampled rows outside [1, MBRL_TS_MAX_ROWS = %d]", what, ts->particles,
                    MBRL_TS_MAX_ROWS);
    if (!resampled && (ts->particles < 1 || (int64_t)E * ts->particles > MBRL_TS_MAX_ROWS))
        return fail(MBRL_EINVAL, "%s: %d members x %d particles outside [1, MBRL_TS_MAX_ROWS = %d] rows", what, E,
                    ts->particles, MBRL_TS_MAX_ROWS);
    if (ts->iteration < 0 || ts->iteration >= (1 << 24))
        return fail(MBRL_EINVAL, "%s: iteration %d outside [0, 2^24)", what, ts->iteration);
    if (!(ts->noise_scale >= 0.0f) || isinf(ts->noise_scale))
        return fail(MBRL_EINVAL, "%s: noise_scale %g is negative or not finite", what, (double)ts->noise_scale);
    TrainShape t;
    if (int rc = ensemble_shape(what, members, E, LOSS_NLL, &t)) return rc;   // (with nll_envelope's LDS bound)
    if (t.a < 1) return fail(MBRL_EINVAL, "%s: action_dim %d < 1", what, t.a);
    if (!nll_bounds_ok(bounds)) return fail(MBRL_EINVAL, "%s: NULL log-variance bounds", what);
    for (int e = 0; e < E; ++e)           // (forward only: the gradient pointers are ignored and may be NULL)
        for (int l = 0; l <= t.L; ++l)
            if (!members[e].weight[l] || !members[e].bias[l])
                return fail(MBRL_EINVAL, "%s: member %d, layer %d: NULL weight or bias", what, e, l);
    if (norm) {
        if ((norm->normalize_state || norm->unnormalize_state) && (!norm->obs_mean || !norm->obs_std))
            return fail(MBRL_EINVAL, "%s: state normalisation requested without obs_mean/obs_std", what);
        if (norm->normalize_action && (!norm->act_mean || !norm->act_std))
            return fail(MBRL_EINVAL, "%s: action normalisation requested without act_mean/act_std", what);
    }
    if (cost) {
        if (cost->kind == MBRL_COST_MODEL_REWARD)
            return fail(MBRL_EINVAL, "%s: MODEL_REWARD cost: probabilistic members have no reward head", what);
        if (cost->kind != MBRL_COST_GOAL_STATE) return fail(MBRL_EUNSUPPORTED, "%s: cost kind %d", what, cost->kind);
        if (cost->has_state_cost && (!cost->weights || !cost->goal))
            return fail(MBRL_EINVAL, "%s: state cost without weights/goal", what);
    }

    for (int e = 0; e < E; ++e)
        for (int l = 0; l <= t.L; ++l) {
            T.m[e].w[l] = members[e].weight[l];
            T.m[e].b[l] = members[e].bias[l];
        }
    T.min_lv = bounds->min_logvar; T.max_lv = bounds->max_logvar;
    if (norm) {
        T.obs_mean = norm->obs_mean; T.obs_std = norm->obs_std; T.act_mean = norm->act_mean; T.act_std = norm->act_std;
        T.norm_s = norm->normalize_state != 0; T.unnorm_s = norm->unnormalize_state != 0;
        T.norm_a = norm->normalize_action != 0;
    }
    if (cost) {
        T.has_sc = cost->has_state_cost != 0; T.has_ac = cost->has_action_cost != 0;
        T.cw = cost->weights; T.goal = cost->goal;
        T.alpha_s = cost->alpha_state; T.alpha_s2 = cost->alpha_state * cost->alpha_state;
        T.alpha_a = cost->alpha_action; T.alpha_a2 = cost->alpha_action * cost->alpha_action;
    }
    T.s0 = s0; T.s0_per_cand = s0_per_cand != 0; T.actions = actions; T.costs = costs; T.states_out = states_out;
    T.noise_seed = ts->noise_seed; T.noise_scale = ts->noise_scale;
    T.s = t.s; T.a = t.a; T.W = t.W; T.L = t.L; T.ld = ts_ld(t);
    T.N = N; T.H = H; T.n_offset = n_offset; T.P = ts->particles; T.iteration = ts->iteration;
    T.E = E; T.resampled = resampled; T.members_out = members_out;
    if (Q) *Q = resampled ? ts->particles : E * ts->particles;
    return MBRL_OK;
}

static int ts_launch(const char* what, const TsLaunch& T, int Q, hipStream_t stream) {
    if (int rc = hip_check(ensure_dynamic_lds(reinterpret_cast<const void*>(rollout_ts_kernel), TS_LDS_BYTES), what))
        return rc;
    const unsigned tiles = (unsigned)(((int64_t)T.N + TS_TM - 1) / TS_TM);
    hipLaunchKernelGGL(rollout_ts_kernel, dim3(tiles, Q), dim3(TS_THREADS), (size_t)2 * TS_TM * T.ld * sizeof(float),
                       stream, T);
    return hip_check(hipGetLastError(), what);
}

// Workspace layout for mbrl_cem_plan_ts: mbrl_cem_plan's with Q cost rows and no pair area.
struct TsPlanWs {
    float *costs, *mu[2], *sigma[2], *aelite, *states, *actions, *s0;
    TrajScratch traj;
    int64_t* elites;
    uint32_t* keys;
    size_t bytes;
};

static TsPlanWs ts_plan_ws(const Geometry& g, const mbrl_cem_params* p, int Q, void* base) {
    TsPlanWs w{};
    WsCursor c(base);
    const size_t Ha = (size_t)p->H * g.a;
    w.costs = c.take<float>((size_t)Q * p->N * 4);
    w.actions = c.take<float>((size_t)p->H * p->N * g.a * 4);
    w.mu[0] = c.take<float>(Ha * 4); w.mu[1] = c.take<float>(Ha * 4);
    w.sigma[0] = c.take<float>(Ha * 4); w.sigma[1] = c.take<float>(Ha * 4);
    w.aelite = c.take<float>((size_t)p->H * p->K * g.a * 4);
    w.states = c.take<float>((size_t)g.E * p->H * g.s * 4);
    w.elites = c.take<int64_t>((size_t)p->K * 8);
    w.keys = c.take<uint32_t>((size_t)p->N * 4);
    w.traj = take_traj_scratch(c, g);
    w.s0 = c.take<float>((size_t)g.s * 4);
    w.bytes = c.off;
    return w;
}

// The checks of the plan's own arguments that need no buffer: shape against params and the particle rows.
static int ts_plan_sizes(const mbrl_mlp_shape* shape, const mbrl_cem_params* p, const mbrl_ts_params* ts, Geometry* g) {
    if (int rc = shape_geometry(shape, g)) return rc;
    if (!p || !ts) return fail(MBRL_EINVAL, "cem_plan_ts: NULL params or ts");
    if (int rc = cem_params_check(p)) return rc;
    if (shape->reward_head || shape->precision != MBRL_PRECISION_F32)
        return fail(MBRL_EUNSUPPORTED, "cem_plan_ts: fp32 members without a reward head only");
    if (g->E > MBRL_TRAIN_MAX_MEMBERS || ts->particles < 1 || (int64_t)g->E * ts->particles > MBRL_TS_MAX_ROWS)
        return fail(MBRL_EINVAL, "cem_plan_ts: %d members x %d particles outside [1, MBRL_TS_MAX_ROWS = %d] rows (E <= %d)",
                    g->E, ts->particles, MBRL_TS_MAX_ROWS, MBRL_TRAIN_MAX_MEMBERS);
    return MBRL_OK;
}

// The receding-horizon plans' checks that need no buffer: mbrl_cem_plan_ts's, with the row bound of the mode.
static int ts_rh_sizes(const mbrl_mlp_shape* shape, const mbrl_cem_rh_params* rp, const mbrl_ts_rows* rows, Geometry* g,
                       int* Q) {
    if (int rc = shape_geometry(shape, g)) return rc;
    if (!rp || !rows) return fail(MBRL_EINVAL, "cem_plan_ts_rh: NULL params or rows");
    if (int rc = cem_params_check(&rp->cem)) return rc;
    if (shape->reward_head || shape->precision != MBRL_PRECISION_F32)
        return fail(MBRL_EUNSUPPORTED, "cem_plan_ts_rh: fp32 members without a reward head only");
    if (rows->member_mode != MBRL_TS_MEMBER_FIXED && rows->member_mode != MBRL_TS_MEMBER_RESAMPLED)
        return fail(MBRL_EINVAL, "cem_plan_ts_rh: member_mode %d", rows->member_mode);
    const int P = rows->ts.particles;
    const int64_t q = rows->member_mode == MBRL_TS_MEMBER_RESAMPLED ? P : (int64_t)g->E * P;
    if (g->E > MBRL_TRAIN_MAX_MEMBERS || P < 1 || q > MBRL_TS_MAX_ROWS)
        return fail(MBRL_EINVAL, "cem_plan_ts_rh: %d members, %d particles: rows outside [1, MBRL_TS_MAX_ROWS = %d] (E <= %d)",
                    g->E, P, MBRL_TS_MAX_ROWS, MBRL_TRAIN_MAX_MEMBERS);
    *Q = (int)q;
    return MBRL_OK;
}

// mbrl_cem_plan_ts_rh and its batch: the sampled rollout's checks (on placeholder buffers: the loop sets the ones
// that move), then the receding-horizon entry's own, then its loop with the source.
static int ts_rh_plan(RhCall c, const mbrl_train_model* members, const mbrl_nll_bounds* bounds, const mbrl_ts_rows* rows) {
    Geometry g;
    int Q = 0, rc;
    if ((rc = ts_rh_sizes(c.shape, c.rp, rows, &g, &Q))) return rc;
    const mbrl_cem_params* p = &c.rp->cem;
    if (!c.packed || !members || !c.actions_out || !c.states_out || !c.workspace || !c.s0)
        return fail(MBRL_EINVAL, "%s: NULL packed, members, actions_out, states_out, workspace or s0", c.name);
    if (c.B < 1) return fail(MBRL_EINVAL, "%s: B=%d", c.name, c.B);
    if ((rc = rollout_validate(g, c.norm, c.cost))) return rc;   // (the final trajectories' checks)
    TsLaunch T{};
    mbrl_ts_params tp = rows->ts;
    tp.iteration = 0;
    float* const placeholder = static_cast<float*>(c.workspace);
    if ((rc = ts_prepare(c.name, members, g.E, bounds, c.norm, c.cost, placeholder, 1, placeholder, p->N, p->H, 0, &tp,
                         placeholder, nullptr, T, rows->member_mode)))
        return rc;
    if (T.s != g.s || T.a != g.a || T.W != g.W || T.L != g.L)
        return fail(MBRL_EINVAL, "%s: the members' shape differs from the packed shape", c.name);
    if (p->iterations > (1 << 24)) return fail(MBRL_EINVAL, "%s: iterations %d above 2^24", c.name, p->iterations);
    const TsSource src{&T, Q};
    c.ts = &src;
    return rh_plan(c);
}

int ts_source_rollout(const TsSource& ts, const float* s0, const float* actions, int BN, int it, float* costs,
                      hipStream_t stream) {
    TsLaunch T = *ts.launch;
    T.s0 = s0; T.s0_per_cand = 1; T.actions = actions; T.costs = costs; T.N = BN; T.iteration = it;
    return ts_launch("cem_plan_ts_rh", T, ts.Q, stream);
}

}  // namespace mbrl

using namespace mbrl;

extern "C" {

int mbrl_rollout_cost_ts(const mbrl_train_model* members, int32_t E, const mbrl_nll_bounds* bounds,
                         const mbrl_norm* norm, const mbrl_cost* cost, const float* s0, int32_t s0_per_candidate,
                         const float* actions, int32_t N, int32_t H, int32_t n_offset, const mbrl_ts_params* ts,
                         float* costs, float* states_out, mbrl_stream_t stream) {
    const char* what = "rollout_cost_ts";
    TsLaunch T{};
    if (int rc = ts_prepare(what, members, E, bounds, norm, cost, s0, s0_per_candidate, actions, N, H, n_offset, ts,
                            costs, states_out, T))
        return rc;
    return ts_launch(what, T, E * ts->particles, reinterpret_cast<hipStream_t>(stream));
}

int mbrl_rollout_cost_ts_rows(const mbrl_train_model* members, int32_t E, const mbrl_nll_bounds* bounds,
                              const mbrl_norm* norm, const mbrl_cost* cost, const float* s0, int32_t s0_per_candidate,
                              const float* actions, int32_t N, int32_t H, int32_t n_offset, const mbrl_ts_rows* rows,
                              float* costs, float* states_out, int32_t* members_out, mbrl_stream_t stream) {
    const char* what = "rollout_cost_ts_rows";
    if (!rows) return fail(MBRL_EINVAL, "%s: NULL rows", what);
    TsLaunch T{};
    int Q = 0;
    if (int rc = ts_prepare(what, members, E, bounds, norm, cost, s0, s0_per_candidate, actions, N, H, n_offset,
                            &rows->ts, costs, states_out, T, rows->member_mode, members_out, &Q))
        return rc;
    return ts_launch(what, T, Q, reinterpret_cast<hipStream_t>(stream));
}

size_t mbrl_cem_ts_rh_workspace_bytes(const mbrl_mlp_shape* shape, const mbrl_cem_rh_params* params,
                                      const mbrl_ts_rows* rows, int32_t B) {
    Geometry g;
    int Q = 0;
    if (ts_rh_sizes(shape, params, rows, &g, &Q) != MBRL_OK) return 0;
    return rh_ts_workspace_bytes(shape, params, Q, B);
}

int mbrl_cem_plan_ts_rh(const mbrl_mlp_shape* shape, const void* packed, const mbrl_train_model* members,
                        const mbrl_nll_bounds* bounds, const mbrl_norm* norm, const mbrl_cost* cost, const float* s0,
                        const mbrl_cem_rh_params* params, const mbrl_ts_rows* rows, const float* init_mu_rows,
                        const float* init_sigma_rows, const float* carry_in, float* mu, float* sigma,
                        float* actions_out, float* states_out, float* carry_out, float* carry_returns_out,
                        float* cost_hist, float* returns_hist, int64_t* elite_hist, float* kept_hist, void* ws,
                        size_t ws_bytes, mbrl_stream_t stream) {
    return ts_rh_plan({"cem_plan_ts_rh", false, shape, packed, norm, cost, s0, 1, params, init_mu_rows, init_sigma_rows,
                       carry_in, nullptr, nullptr, mu, sigma, actions_out, states_out, carry_out, carry_returns_out,
                       cost_hist, returns_hist, elite_hist, kept_hist, nullptr, ws, ws_bytes, stream},
                      members, bounds, rows);
}

int mbrl_cem_plan_ts_rh_batch(const mbrl_mlp_shape* shape, const void* packed, const mbrl_train_model* members,
                              const mbrl_nll_bounds* bounds, const mbrl_norm* norm, const mbrl_cost* cost,
                              const float* s0, int32_t B, const mbrl_cem_rh_params* params, const mbrl_ts_rows* rows,
                              const float* init_mu_rows, const float* init_sigma_rows, const float* carry_in,
                              const int32_t* input_flags, float* mu, float* sigma, float* actions_out,
                              float* states_out, float* carry_out, float* carry_returns_out, float* cost_hist,
                              float* returns_hist, int64_t* elite_hist, float* kept_hist, void* ws, size_t ws_bytes,
                              mbrl_stream_t stream) {
    return ts_rh_plan({"cem_plan_ts_rh_batch", true, shape, packed, norm, cost, s0, B, params, init_mu_rows,
                       init_sigma_rows, carry_in, input_flags, nullptr, mu, sigma, actions_out, states_out, carry_out,
                       carry_returns_out, cost_hist, returns_hist, elite_hist, kept_hist, nullptr, ws, ws_bytes, stream},
                      members, bounds, rows);
}

size_t mbrl_cem_ts_workspace_bytes(const mbrl_mlp_shape* shape, const mbrl_cem_params* params,
                                   const mbrl_ts_params* ts) {
    Geometry g;
    if (ts_plan_sizes(shape, params, ts, &g) != MBRL_OK) return 0;
    return ts_plan_ws(g, params, g.E * ts->particles, nullptr).bytes;
}

int mbrl_cem_plan_ts(const mbrl_mlp_shape* shape, const void* packed, const mbrl_train_model* members,
                     const mbrl_nll_bounds* bounds, const mbrl_norm* norm, const mbrl_cost* cost, const float* s0_in,
                     const mbrl_cem_params* p, const mbrl_ts_params* ts, float* mu, float* sigma, float* actions_out,
                     float* states_out, float* cost_hist, float* returns_hist, int64_t* elite_hist, void* workspace,
                     size_t ws_bytes, mbrl_stream_t stream_) {
    const char* what = "cem_plan_ts";
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    Geometry g;
    int rc;
    if ((rc = ts_plan_sizes(shape, p, ts, &g))) return rc;
    if (!packed || !members || !actions_out || !states_out || !workspace || !s0_in)
        return fail(MBRL_EINVAL, "%s: NULL packed, members, actions_out, states_out, workspace or s0", what);
    const int Q = g.E * ts->particles;
    const TsPlanWs w = ts_plan_ws(g, p, Q, workspace);
    if (ws_bytes < w.bytes) return fail(MBRL_EWORKSPACE, "%s: workspace %zu < %zu", what, ws_bytes, w.bytes);
    if ((rc = rollout_validate(g, norm, cost))) return rc;   // (the final trajectory's checks)
    // the sampled rollout's checks, all before the first launch; the buffers that move per iteration are set below
    TsLaunch T{};
    mbrl_ts_params tp = *ts;
    tp.iteration = 0;
    if ((rc = ts_prepare(what, members, g.E, bounds, norm, cost, w.s0, 0, w.actions, p->N, p->H, 0, &tp, w.costs, nullptr, T)))
        return rc;
    if (T.s != g.s || T.a != g.a || T.W != g.W || T.L != g.L)
        return fail(MBRL_EINVAL, "%s: the members' shape differs from the packed shape", what);
    if (p->iterations > (1 << 24)) return fail(MBRL_EINVAL, "%s: iterations %d above 2^24", what, p->iterations);

    const FusePlan f = fuse_plan(p->N, p->N, p->K, g.a);
    const InitZero z = plan_zero(g, p->N, nullptr, w.traj);
    launch_cem_init(dim3(p->H * (f.fuse_draw ? draw_slices(p->H, 1, p->N, g.a) : 1), 1), stream, p->seed, p->init_mu,
                    p->init_sigma, p->lo, p->hi, p->H, g.a, p->N, w.mu[0], w.sigma[0], f.fuse_draw ? w.actions : nullptr,
                    s0_in, g.s, w.s0, 0, z, nullptr);
    int cur = 0;
    for (int it = 0; it < p->iterations; ++it) {
        const mbrl_sampler sp = make_sampler(p, it, w.mu[cur], w.sigma[cur]);
        float* costs = cost_hist ? cost_hist + (size_t)it * Q * p->N : w.costs;
        int64_t* elites = elite_hist ? elite_hist + (size_t)it * p->K : w.elites;
        float* rets = returns_hist ? returns_hist + (size_t)it * p->N : nullptr;
        if (!f.fuse_draw && (rc = sample_impl(&sp, p->H, g.a, p->N, 0, w.actions, stream))) return rc;
        T.costs = costs;
        T.iteration = it;
        if ((rc = ts_launch(what, T, Q, stream))) return rc;
        // the update over Q rows: the selection and the fused update take the row count as their member count
        if (f.fuse) {
            UpdateArgs U = make_update_args(g, p, it, costs, w.mu[cur], w.sigma[cur], w.mu[cur ^ 1], w.sigma[cur ^ 1], mu,
                                            sigma, actions_out, f.fuse_draw ? w.actions : nullptr);
            U.E = Q;
            U.elite_out = elites; U.returns_out = rets;
            U.ael = w.aelite;
            rc = update_impl(U, 1, stream);
        } else {
            const bool last = it + 1 == p->iterations;
            rc = select_impl(costs, Q, p->N, p->K, MBRL_NAN_LAST, elites, rets, w.keys, align256((size_t)p->N * 4), stream);
            if (rc) return rc;
            rc = refit_impl(&sp, p->H, g.a, elites, p->K, p->alpha, w.aelite, w.mu[cur ^ 1], w.sigma[cur ^ 1], stream,
                            last ? mu : nullptr, last ? sigma : nullptr, last ? actions_out : nullptr);
        }
        if (rc) return rc;
        cur ^= 1;
    }
    // the final mean's predicted states: deterministic, the member mean of the mean rows (mbrl_cem_plan's)
    rc = final_trajectory(g, packed, norm, w.s0, actions_out, p->H, states_out, w.states, w.traj, stream,
                          z.ptr[1] != nullptr);
    if (rc) return rc;
    return hip_check(hipGetLastError(), "plan launch");
}

}  // extern "C"
