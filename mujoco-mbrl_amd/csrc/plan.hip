// The plans: host dispatch of the rollout and trajectory kernels (rollout_impl, traj_impl), the plan
// workspaces, the helpers the plan loops share (mbrl_plan.h) and the single-GPU plan entries
// (include/mbrl_cem.h): rollout cost, trajectory, CEM plan, receding-horizon CEM plan, MPPI plan, batched
// CEM plan, batched MPPI plan, batched receding-horizon CEM plan, and the two receding-horizon plans with a noise mix.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mbrl_plan.h"

namespace mbrl {

// MBRL_OPT_ROLLOUT_PAIR = 0 (auto) takes column-split pairs for small plans (2 = never, the A/B)
static constexpr bool kPairAuto = true;

__global__ void fill2_kernel(float* __restrict__ x, float vx, float* __restrict__ y, float vy, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { x[i] = vx; y[i] = vy; }
}

__global__ void member_mean_kernel(const float* __restrict__ src, int E, int n, float* __restrict__ dst) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        float acc = src[i];
        for (int e = 1; e < E; ++e) acc = __fadd_rn(acc, src[(size_t)e * n + i]);
        dst[i] = E > 1 ? __fdiv_rn(acc, (float)E) : acc;
    }
}

__global__ void expand_rows_kernel(const float* __restrict__ src, int B, int n_rep, int s, float* __restrict__ dst) {
    const size_t total = (size_t)B * n_rep * s;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t row = i / s;
        dst[i] = src[(row / n_rep) * s + (i - row * s)];
    }
}

// (0: Wpad != 512, or more than 256 workgroups, the co-resident count of the 256-CU MI355X)
size_t pair_area_bytes(const Geometry& g, int N) {
    const int ntiles = (N + 15) / 16;
    if (g.T != 8 || (size_t)2 * ntiles * g.E > 256) return 0;
    return pair_layout(g.Wpad, g.pw, ntiles, g.E).bytes;
}

int pair_forced_check(const Geometry& g, int N) {
    if (opt(MBRL_OPT_ROLLOUT_PAIR) == 1 && pair_area_bytes(g, N) == 0)
        return fail(MBRL_EUNSUPPORTED, "rollout_pair forced: no pair kernel for N=%d (Wpad %d, E %d)", N, g.Wpad, g.E);
    return MBRL_OK;
}

// The hand-off words a plan's first launch zeroes (cem_init_kernel): the pair flags of a shard of Nl
// candidates (when the workspace offers pairs) and the trajectory kernel's granules with the status
// word right behind them (the workspaces lay them out so; else the trajectory launch keeps its memset).
InitZero plan_zero(const Geometry& g, int Nl, void* pair, const TrajScratch& ts) {
    InitZero z{};
    if (pair && pair_area_bytes(g, Nl)) {
        z.ptr[0] = static_cast<unsigned*>(pair);
        z.words[0] = pair_layout(g.Wpad, g.pw, (Nl + 15) / 16, g.E).zero_bytes / 4;
    }
    if (ts.xchg && ts.status && reinterpret_cast<char*>(ts.status) == reinterpret_cast<char*>(ts.xchg) + ts.xchg_bytes) {
        z.ptr[1] = reinterpret_cast<unsigned*>(ts.xchg);
        z.words[1] = (ts.xchg_bytes + 16) / 4;
    }
    return z;
}

// The argument checks of rollout_impl that depend on the problem only (not on N or the buffers): the
// sharded plan runs them before its first collective.
// A state or action flag needs its statistics; a statistics pointer no flag uses may be NULL (the
// kernels then never read it, or read it as mean 0 / std 1). Shared by the rollout and the trajectory.
static int norm_stats_validate(const mbrl_norm* norm) {
    if (!norm) return MBRL_OK;
    if ((norm->normalize_state || norm->unnormalize_state) && (!norm->obs_mean || !norm->obs_std))
        return fail(MBRL_EINVAL, "state normalisation requested without obs_mean/obs_std");
    if (norm->normalize_action && (!norm->act_mean || !norm->act_std))
        return fail(MBRL_EINVAL, "action normalisation requested without act_mean/act_std");
    return MBRL_OK;
}

// Whether the output partials may live in the activation buffer the last hidden layer does not read
// (RolloutArgs.part_alias) with nw waves per workgroup.
static bool part_alias_ok(const Geometry& g, bool reward, int nw) {
    return !reward && g.L >= 3 && (g.L & 1) && (size_t)(nw > 4 ? nw : 4) * g.pw <= (size_t)g.lda;
}

// Dynamic LDS of the 16-candidate fp32 tile as rollout_impl launches it (8 waves from Wpad = 128, the
// partials aliased where they can be): the least any fp32 rollout of this shape needs.
static size_t min_tile_lds_bytes(const Geometry& g, bool reward) {
    RolloutArgs A{};
    A.s = g.s; A.a = g.a; A.L = g.L; A.Wpad = g.Wpad; A.NOT = g.NOT; A.lda = g.lda; A.pw = g.pw;
    A.nw = g.T >= 2 ? 8 : 4;
    A.part_alias = part_alias_ok(g, reward, A.nw) ? 1 : 0;
    return rollout_lds_bytes(A, 16);
}

int rollout_validate(const Geometry& g, const mbrl_norm* norm, const mbrl_cost* cost) {
    if (norm) {
        if (norm->unnormalize_reward && (!norm->rew_mean || !norm->rew_std))
            return fail(MBRL_EINVAL, "reward unnormalisation requested without rew_mean/rew_std");
        if (int rc = norm_stats_validate(norm)) return rc;
    }
    if (cost && cost->kind == MBRL_COST_MODEL_REWARD) {
        if (!g.reward) return fail(MBRL_EINVAL, "MODEL_REWARD cost needs a reward_head model");
    } else if (cost) {
        if (cost->kind != MBRL_COST_GOAL_STATE) return fail(MBRL_EUNSUPPORTED, "cost kind %d", cost->kind);
        if (cost->has_state_cost && (!cost->weights || !cost->goal))
            return fail(MBRL_EINVAL, "state cost without weights/goal");
    }
    if (16 * g.a > 768) return fail(MBRL_EUNSUPPORTED, "action_dim %d too large (max 48)", g.a);
    // the smallest fp32 tile (16 candidates) must fit LDS; refused here, before the proposal draw or any
    // other launch, so a refused call leaves every buffer as it was
    const bool reward = cost && cost->kind == MBRL_COST_MODEL_REWARD;
    if (const size_t need = min_tile_lds_bytes(g, reward); need > 160 * 1024)
        return fail(MBRL_EUNSUPPORTED, "LDS footprint %zu B exceeds 160 KiB", need);
    return MBRL_OK;
}

// pair_area: a pair_area_bytes(g, N) block of the caller's workspace, or NULL (no column-split pairs).
// pair_epoch: NULL (the pair flags are zeroed by a memset before a pair launch), or the plan's counter
// of pair launches, whose flags its first launch zeroed (cem_init_kernel): each pair launch takes the
// next epoch (RolloutArgs), and a memset only when the epochs would outgrow the 32-bit flags.
int rollout_impl(const Geometry& g, const void* packed, const mbrl_norm* norm, const mbrl_cost* cost, const float* s0,
                 int s0_per_cand, const float* actions, const mbrl_sampler* sampler, int N, int H, int n_offset,
                 float* costs, float* actions_out, float* states_out, hipStream_t stream, void* pair_area,
                 unsigned* pair_epoch, const unsigned** pair_status_out) {
    if (!packed || !s0 || !costs) return fail(MBRL_EINVAL, "packed, s0 and costs must be non-NULL");
    if (N < 1 || H < 1) return fail(MBRL_EINVAL, "N=%d H=%d must be >= 1", N, H);
    if (!actions && !sampler) return fail(MBRL_EINVAL, "need either actions or a sampler");
    if (n_offset < 0) return fail(MBRL_EINVAL, "n_offset=%d < 0", n_offset);
    if (int rc = rollout_validate(g, norm, cost)) return rc;
    RolloutArgs A{};
    A.packed = static_cast<const float*>(packed);
    A.member_stride = g.member_stride;
    A.stream_floats = g.stream_floats;
    A.s = g.s; A.a = g.a; A.L = g.L; A.Wpad = g.Wpad; A.K0C = g.K0C; A.NOT = g.NOT; A.E = g.E;
    A.chunks_per_step = g.C; A.lda = g.lda; A.pw = g.pw; A.k0pad_extra = 16 * g.K0C - g.s - g.a;
    A.N = N; A.H = H; A.n_offset = n_offset;
    if (norm) {
        A.obs_mean = norm->obs_mean; A.obs_std = norm->obs_std;
        A.act_mean = norm->act_mean; A.act_std = norm->act_std;
        A.norm_s = norm->normalize_state; A.unnorm_s = norm->unnormalize_state; A.norm_a = norm->normalize_action;
        A.unnorm_r = norm->unnormalize_reward; A.rew_mean = norm->rew_mean; A.rew_std = norm->rew_std;
    }
    if (cost && cost->kind == MBRL_COST_MODEL_REWARD) {
        A.reward = 1;
    } else if (cost) {
        A.has_sc = cost->has_state_cost; A.has_ac = cost->has_action_cost;
        A.cw = cost->weights; A.goal = cost->goal;
        A.alpha_s = cost->alpha_state; A.alpha_s2 = cost->alpha_state * cost->alpha_state;
        A.alpha_a = cost->alpha_action; A.alpha_a2 = cost->alpha_action * cost->alpha_action;
    }
    A.s0 = s0; A.s0_per_cand = s0_per_cand;
    if (!actions) {
        // CEM proposal: draw into actions_out first, then roll those actions out
        if (!actions_out) return fail(MBRL_EINVAL, "a sampled rollout needs actions_out to hold the draw");
        if (!sampler->mu || !sampler->sigma) return fail(MBRL_EINVAL, "sampler mu/sigma NULL");
        int rc = sample_impl(sampler, H, g.a, N, n_offset, actions_out, stream);
        if (rc) return rc;
        actions = actions_out;
    }
    A.actions = actions;
    A.costs = costs; A.states_out = states_out;
    {
        // half-group layer hand-offs of the 8-wave ring rollout (rollout.hip GS; same bits). Auto: on for
        // the instances it was measured on, W = 512 with two layer-0 and two output chunks -- cheetah's
        // 16- and walker's 32-candidate tiles; every other shape keeps the full barrier
        const int gs = opt(MBRL_OPT_ROLLOUT_GROUP_SEAM);
        const bool gs_auto = g.T == 8 && g.K0C == 2 && g.NOT == 2;
        A.group_seam = (gs == 1 || (gs == 0 && gs_auto)) ? 1 : 0;
    }
    // Tile height: two 16-row blocks per workgroup halve the weight stream per FLOP once there are
    // enough candidates to still give every CU a workgroup.
    int R = (N >= 2 * 16 * 256 && g.T <= 8) ? 2 : 1;
    const int G = (g.a + 3) / 4;
    (void)G;
    if (16 * R * g.a > 768) R = 1;
    // waves per workgroup as launch_rollout_t picks them: 8 for R = 1 (T >= 2), else 4
    A.nw = (R == 1 && g.T >= 2) ? 8 : 4;
    if ((g.precision == MBRL_PRECISION_F16X3 || g.precision == MBRL_PRECISION_F16X6) && g.split_ok && !A.reward) {
        const int P = g.precision == MBRL_PRECISION_F16X6 ? 3 : 2;
        RolloutArgs S = A;
        S.split_off = P == 3 ? g.split3_off : g.split_off;
        S.K0S = g.K0S;
        S.CS = g.CS;
        S.sr = P * (g.Wpad > 32 * g.K0S ? g.Wpad : 32 * g.K0S) + 8;
        S.nw = 8;
        // 32 candidates per workgroup once that still gives every CU a workgroup (N >= 8192): the
        // split kernel is bound by the L2 weight stream, which R = 2 halves per candidate. At
        // N = 4096 R = 2 would idle half the CUs: 0.607 vs 0.571 ms per F16X3 rollout (cheetah, r01).
        int RS = N >= 256 * 32 ? 2 : 1;
        if (const int o = opt(MBRL_OPT_SPLIT_TILE)) RS = o == 32 ? 2 : 1;
        RolloutArgs X = A;                 // the fp32 redo pass at the same tile height
        X.redo = 1;
        X.nw = RS == 1 && g.T >= 2 ? 8 : 4;
        if (RS == 2 && (!rollout_split_supported(S, g.T, 2, P) || rollout_lds_bytes(X, 32) > 160 * 1024)) {
            RS = 1;
            X.nw = g.T >= 2 ? 8 : 4;
        }
        if (rollout_split_supported(S, g.T, RS, P)) {
            hipError_t err = launch_rollout_split(S, g.T, RS, P, stream);
            if (err != hipSuccess) return hip_check(err, "split rollout launch");
            // fp32 redo of the workgroups that met an operand outside the split range (usually none:
            // every workgroup reads its candidates' costs and exits)
            return hip_check(launch_rollout(X, g.T, RS, stream), "split redo launch");
        }
    }
    // ensembles: member-major workgroup order per XCD (mbrl_internal.h xcd_unit), opt-in. The plain
    // (tile, member) grid already keeps each XCD on one member at a time (consecutive ids of one member
    // round-robin over the XCDs), so it measured the same (humanoid 75.5 ms either way)
    A.xcd_map = (g.E > 1 && opt(MBRL_OPT_XCD_MAP) == 1) ? 1 : 0;
    // 8-candidate tiles (rollout_m8_kernel, bit-identical sums) when 16-candidate tiles would leave
    // at least half the CUs idle: the shard of a strong-scaled plan, small plans.
    // MBRL_OPT_ROLLOUT_TILE = 8 / 16 forces a choice (tests, A/B).
    // column-split pairs: each 16-candidate tile on two workgroups of half the columns (16x16x4 MFMA at
    // full clock, half the weight stream per workgroup) where 16-candidate tiles would leave at least
    // half the CUs idle; opt-in until measured (MBRL_OPT_ROLLOUT_PAIR)
    if (pair_area && !A.reward && opt(MBRL_OPT_ROLLOUT_TILE) == 0) {
        const int po = opt(MBRL_OPT_ROLLOUT_PAIR);
        const int ntiles = (N + 15) / 16;
        // auto: where the pairs fill more than half the CUs and at most all of them (one workgroup per
        // CU, all co-resident): the 2048-candidate shard of walker over 8 GPUs, 0.691 vs 0.715-0.722 ms
        // per rollout on 8-candidate tiles with L2-resident hand-offs (profiles/r04/pair_l2_ab.json);
        // at 1024 (half the chip) the 8-candidate tiles stay ahead, 0.54 vs 0.69 ms
        const size_t pw = (size_t)ntiles * g.E * 2, cus = (size_t)device_cu_count();
        const bool want = po == 1 || (po == 0 && kPairAuto && 2 * pw > cus && pw <= cus);
        if (want && pair_area_bytes(g, N) != 0) {
            RolloutArgs P = A;
            P.pair_flags = static_cast<unsigned*>(pair_area);
            P.pair_data = reinterpret_cast<float*>(static_cast<char*>(pair_area) +
                                                   pair_layout(g.Wpad, g.pw, ntiles, g.E).flags_bytes);
            if (rollout_pair_supported(P, g.T)) {
                const int dpa = opt(MBRL_OPT_DEBUG_PAIR_ABORT);
                P.debug_abort = dpa == 1;
                P.pair_l2 = opt(MBRL_OPT_PAIR_L2) != 2;
                const unsigned qs = pair_handoffs(H, g.L);
                if (pair_epoch && (uint64_t)(*pair_epoch + 1) * qs + 16 < (1ull << 31)) {
                    P.pair_epoch = ++*pair_epoch;   // flags zeroed by the plan's first launch
                    P.pair_prezeroed = 1;
                } else {
                    P.pair_epoch = 1;               // a memset before the launch; the plan restarts its epochs
                    P.pair_prezeroed = 0;
                    if (pair_epoch) *pair_epoch = 1;
                }
                P.pair_base = (P.pair_epoch - 1) * qs;
                const hipError_t err = launch_rollout_pair(P, g.T, stream);
                if (err == hipSuccess && dpa == 2) return MBRL_OK;   // tests: the pair launch's own results
                if (err == hipSuccess && pair_status_out && P.pair_prezeroed) {
                    // the caller checks the plan's pair status word once, after the plan (a sharded plan
                    // with peers: it redoes the whole plan without pairs if any hand-off timed out), so
                    // no gated redo launch follows each pair launch
                    *pair_status_out = P.pair_flags + (size_t)2 * ntiles * g.E * 32;
                    return MBRL_OK;
                }
                if (err == hipSuccess) {
                    // A pair's halves wait on each other, and a plain launch does not promise that both
                    // are resident (another stream may hold CUs): a wait that timed out raised the status
                    // word after the flags to the launch's epoch and left its tile's costs invalid. The
                    // launch chosen below then recomputes every candidate if it did, else its workgroups
                    // exit at once (bit-identical sums on every tile height).
                    A.gate = P.pair_flags + (size_t)2 * ntiles * g.E * 32;
                    A.gate_epoch = P.pair_epoch;
                } else if (err != hipErrorCooperativeLaunchTooLarge || po == 1) {
                    return hip_check(err, "rollout pair launch");
                }
            } else if (po == 1) {
                return fail(MBRL_EUNSUPPORTED, "rollout_pair forced: shape not supported by the pair kernel");
            }
        } else if (po == 1) {
            return fail(MBRL_EUNSUPPORTED, "rollout_pair forced: no pair area for N=%d (Wpad %d, E %d)", N, g.Wpad, g.E);
        }
    }
    if (g.m8_ok) {
        A.m8_off = g.m8_off;
        A.C8 = g.C8;
        A.m4_off = g.m4_off;
        A.C4 = g.C4;
        const int o = opt(MBRL_OPT_ROLLOUT_TILE);
        // 4-candidate tiles (rollout_m4_kernel) once 8-candidate tiles would still leave at least half
        // the CUs idle (cartpole's N = 1024, shards of <= 1024 candidates); both bit-identical
        bool use4 = false;   // opt-in: slower than 8-candidate tiles at cartpole size
        bool use8 = (size_t)((N + 15) / 16) * g.E * 2 <= (size_t)device_cu_count();
        if (o) { use4 = o == 4; use8 = o == 8; }
        if (use4 && g.m4_ok && rollout_m4_supported(A, g.T, g.NG4))
            return hip_check(launch_rollout_m4(A, g.T, g.NG4, stream), "rollout m4 launch");
        if ((use8 || use4) && rollout_m8_supported(A, g.T))
            return hip_check(launch_rollout_m8(A, g.T, stream), "rollout m8 launch");
    }
    // partials in the activation buffer the last hidden layer does not read (rollout.hip): layer 0
    // writes act2, hidden layer l reads act2 for odd l, so with L odd the last one reads act and act2
    // is free from the barrier after layer L-2 until the next step's layer 0
    // 32-candidate tiles on 8 waves (two per SIMD) when the 8 partials fit the aliased activation
    // buffer: walker rollout 3.91 -> 3.83 ms, frac 0.883 -> 0.901 (profiles/r02_ab_r2_8waves.txt)
    if (R == 2 && g.T >= 2 && !A.reward && g.L >= 3 && (g.L & 1) && (size_t)8 * g.pw <= (size_t)g.lda) A.nw = 8;
    auto alias_ok = [&]() { return part_alias_ok(g, A.reward != 0, A.nw); };
    A.part_alias = alias_ok() ? 1 : 0;
    if (rollout_lds_bytes(A, 16 * R) > 160 * 1024) {
        // the 16-candidate tile of min_tile_lds_bytes, which rollout_validate found to fit
        R = 1;
        A.nw = g.T >= 2 ? 8 : 4;
        A.part_alias = alias_ok() ? 1 : 0;
        if (rollout_lds_bytes(A, 16) > 160 * 1024)
            return fail(MBRL_EUNSUPPORTED, "LDS footprint %zu B exceeds 160 KiB", rollout_lds_bytes(A, 16));
    }
    return hip_check(launch_rollout(A, g.T, R, stream), "rollout launch");
}

// prezeroed: the plan's first launch zeroed the granules and status (cem_init_kernel), so no memset here.
static int traj_impl(const Geometry& g, const void* packed, const mbrl_norm* norm, const float* s0,
                     const float* actions, int H, float* states_out, const TrajScratch& ts, hipStream_t stream,
                     int prezeroed) {
    if (int rc = norm_stats_validate(norm)) return rc;   // before any launch
    TrajArgs T{};
    T.prezeroed = prezeroed;
    T.packed = static_cast<const float*>(packed);
    T.member_stride = g.member_stride;
    T.bias_off = g.stream_floats;
    T.tw_base = g.stream_floats + g.bias_floats;
    for (int l = 0; l <= g.L; ++l) T.tw_off[l] = g.tw_off[l];
    T.s = g.s; T.a = g.a; T.W = g.W; T.Wpad = g.Wpad; T.L = g.L; T.H = H;
    if (norm) {
        T.obs_mean = norm->obs_mean; T.obs_std = norm->obs_std;
        T.act_mean = norm->act_mean; T.act_std = norm->act_std;
        T.norm_s = norm->normalize_state; T.unnorm_s = norm->unnormalize_state; T.norm_a = norm->normalize_action;
    }
    T.s0 = s0; T.actions = actions; T.states_out = states_out;
    if (traj_reg_supported(T) && opt(MBRL_OPT_DEBUG_TRAJ_ABORT) == 0)
        return hip_check(launch_traj_reg(T, g.E, stream), "trajectory launch");
    if (ts.xchg && ts.status && traj_coop_supported(T, g.E) && ts.xchg_bytes >= traj_coop_xchg_bytes(T, g.E)) {
        T.debug_abort = opt(MBRL_OPT_DEBUG_TRAJ_ABORT) != 0;
        const int hop = opt(MBRL_OPT_TRAJ_HOP);
        T.hop_mode = hop == 0 ? kTrajHopDefault : hop - 1;
        const hipError_t err = launch_traj_coop(T, g.E, ts.xchg, ts.status, stream);
        if (err != hipErrorCooperativeLaunchTooLarge) {   // too large: the grid cannot be co-resident
            int rc = hip_check(err, "trajectory launch");
            if (rc) return rc;
            // The cooperative kernel needs its P*E workgroups co-resident; if a hand-off ever timed
            // out (another process holding CUs, say) it set `status` and gave up. The single-workgroup
            // kernel then recomputes the states; otherwise its E workgroups read the status word and exit.
            // (Run inside the cooperative launch instead, the fallback's registers raised the kernel's
            // from 107 to 161 VGPRs: one workgroup per CU, and two plans' trajectories on one XCD then
            // waited on each other until the hand-off timeout.)
            T.gate = ts.status;
        }
        T.debug_abort = 0;
    }
    return hip_check(launch_traj(T, g.E, stream), "trajectory launch");
}

// ---- what the plan loops share (mbrl_plan.h)
TrajScratch take_traj_scratch(WsCursor& c, const Geometry& g) {
    TrajScratch ts{};
    ts.xchg_bytes = (size_t)g.E * 2 * g.Wpad * 8;   // a 16-byte multiple
    ts.xchg = c.take<unsigned long long>(ts.xchg_bytes);
    ts.status = c.take<unsigned>(16);
    return ts;
}

int cem_params_check(const mbrl_cem_params* p) {
    if (p->N < 1 || p->H < 1 || p->K < 1 || p->K > p->N || p->iterations < 1)
        return fail(MBRL_EINVAL, "bad CEM params N=%d H=%d K=%d I=%d", p->N, p->H, p->K, p->iterations);
    return MBRL_OK;
}

FusePlan fuse_plan(int N_select, int N_draw, int K, int a) {
    FusePlan f;
    f.fuse = update_kpt(N_select, K, a) != 0 && opt(MBRL_OPT_UNFUSED_UPDATE) == 0;
    f.fuse_draw = f.fuse && update_samples(N_draw, a);
    return f;
}

int record_rollout_event(mbrl_event_t* events, int idx, hipStream_t stream) {
    if (!events || !events[idx]) return MBRL_OK;
    return hip_check(hipEventRecord(reinterpret_cast<hipEvent_t>(events[idx]), stream), "event");
}

UpdateArgs make_update_args(const Geometry& g, const mbrl_cem_params* p, int it, const float* costs,
                            const float* mu_cur, const float* sigma_cur, float* mu_next, float* sigma_next,
                            float* fin_mu, float* fin_sigma, float* fin_actions, float* next_actions) {
    const bool last = it + 1 == p->iterations;   // the last refit also writes mu / sigma / clip(mu)
    UpdateArgs U{};
    U.costs = costs; U.E = g.E; U.N = p->N; U.K = p->K; U.member_stride = p->N; U.H = p->H; U.a = g.a;
    U.seed = p->seed; U.iteration = it; U.mu = mu_cur; U.sigma = sigma_cur;
    U.lo = p->lo; U.hi = p->hi; U.alpha = p->alpha; U.oma = 1.0f - p->alpha;
    U.mu_out = mu_next; U.sigma_out = sigma_next;
    U.fin_mu = last ? fin_mu : nullptr; U.fin_sigma = last ? fin_sigma : nullptr;
    U.fin_actions = last ? fin_actions : nullptr;
    U.next_actions = last ? nullptr : next_actions;
    U.draw_off = 0; U.draw_n = p->N;
    return U;
}

int final_trajectory(const Geometry& g, const void* packed, const mbrl_norm* norm, const float* s0,
                     const float* actions, int H, float* states_out, float* member_scratch, const TrajScratch& ts,
                     hipStream_t stream, int prezeroed, float* member_out) {
    float* per_member = member_out ? member_out : (g.E == 1 ? states_out : member_scratch);
    if (int rc = traj_impl(g, packed, norm, s0, actions, H, per_member, ts, stream, prezeroed)) return rc;
    if (per_member != states_out) {
        const int Hs = H * g.s;
        hipLaunchKernelGGL(member_mean_kernel, dim3((Hs + 255) / 256), dim3(256), 0, stream, per_member, g.E, Hs,
                           states_out);
    }
    return MBRL_OK;
}

}  // namespace mbrl

using namespace mbrl;

extern "C" {

int mbrl_rollout_cost(const mbrl_mlp_shape* shape, const void* packed, const mbrl_norm* norm, const mbrl_cost* cost,
                      const float* s0, int32_t s0_per_candidate, const float* actions, const mbrl_sampler* sampler,
                      int32_t N, int32_t H, int32_t n_offset, float* costs, float* actions_out, float* states_out,
                      mbrl_stream_t stream) {
    Geometry g;
    int rc = shape_geometry(shape, &g);
    if (rc) return rc;
    return rollout_impl(g, packed, norm, cost, s0, s0_per_candidate, actions, sampler, N, H, n_offset, costs,
                        actions_out, states_out, reinterpret_cast<hipStream_t>(stream));
}

// Workspace for mbrl_trajectory: the hand-off scratch first, then the per-member states.
struct TrajWs {
    TrajScratch traj;
    float* states;
    size_t bytes;
};

static TrajWs traj_ws(const Geometry& g, int H, void* base) {
    TrajWs w{};
    WsCursor c(base);
    w.traj = take_traj_scratch(c, g);
    w.states = c.take<float>((size_t)g.E * H * g.s * 4);
    w.bytes = c.off;
    return w;
}

size_t mbrl_trajectory_workspace_bytes(const mbrl_mlp_shape* shape, int32_t H) {
    Geometry g;
    if (shape_geometry(shape, &g) != MBRL_OK || H < 1) return 0;
    return traj_ws(g, H, nullptr).bytes;
}

int mbrl_trajectory(const mbrl_mlp_shape* shape, const void* packed, const mbrl_norm* norm, const float* s0,
                    const float* actions, int32_t H, float* states_out, float* member_states_out, void* workspace,
                    size_t ws_bytes, mbrl_stream_t stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    Geometry g;
    int rc = shape_geometry(shape, &g);
    if (rc) return rc;
    if (H < 1) return fail(MBRL_EINVAL, "trajectory: H=%d", H);
    if (!packed || !s0 || !actions || !states_out || !workspace) return fail(MBRL_EINVAL, "trajectory: NULL argument");
    TrajWs w = traj_ws(g, H, workspace);
    if (ws_bytes < w.bytes) return fail(MBRL_EWORKSPACE, "trajectory workspace %zu < %zu", ws_bytes, w.bytes);
    rc = final_trajectory(g, packed, norm, s0, actions, H, states_out, w.states, w.traj, stream, 0, member_states_out);
    if (rc) return rc;
    return hip_check(hipGetLastError(), "trajectory launch");
}

// Workspace layout for mbrl_cem_plan.
struct PlanWs {
    float *costs, *mu[2], *sigma[2], *aelite, *states, *tmp_cost, *actions, *s0;
    void* pair;   // column-split pair exchange area (NULL-sized when pairs are not offered)
    TrajScratch traj;
    int64_t* elites;
    uint32_t* keys;
    size_t bytes;
};

static PlanWs plan_ws(const Geometry& g, const mbrl_cem_params* p, void* base) {
    PlanWs w{};
    WsCursor c(base);
    const size_t Ha = (size_t)p->H * g.a;
    w.costs = c.take<float>((size_t)g.E * p->N * 4);
    w.actions = c.take<float>((size_t)p->H * p->N * g.a * 4);
    w.mu[0] = c.take<float>(Ha * 4); w.mu[1] = c.take<float>(Ha * 4);
    w.sigma[0] = c.take<float>(Ha * 4); w.sigma[1] = c.take<float>(Ha * 4);
    w.aelite = c.take<float>((size_t)p->H * p->K * g.a * 4);
    w.states = c.take<float>((size_t)g.E * p->H * g.s * 4);
    w.tmp_cost = c.take<float>((size_t)g.E * 4);
    w.elites = c.take<int64_t>((size_t)p->K * 8);
    w.keys = c.take<uint32_t>((size_t)p->N * 4);
    w.traj = take_traj_scratch(c, g);
    w.s0 = c.take<float>((size_t)g.s * 4);
    w.pair = c.take<char>(pair_area_bytes(g, p->N));
    w.bytes = c.off;
    return w;
}

size_t mbrl_cem_workspace_bytes(const mbrl_mlp_shape* shape, const mbrl_cem_params* params) {
    Geometry g;
    if (shape_geometry(shape, &g) != MBRL_OK || !params) return 0;
    return plan_ws(g, params, nullptr).bytes;
}

// mbrl_cem_plan's launches, the arguments checked and the workspace carved: shared with the receding-horizon
// plan that keeps no rows (mbrl_cem_plan_rh, keep == 0), which differs in the first launch alone -- the
// initial distribution's rows (mu_rows / sigma_rows, each or NULL).
static int cem_plan_run(const Geometry& g, const void* packed, const mbrl_norm* norm, const mbrl_cost* cost,
                        const float* s0_in, const mbrl_cem_params* p, const float* mu_rows, const float* sigma_rows,
                        float* mu, float* sigma, float* actions_out, float* states_out, float* cost_hist,
                        float* returns_hist, int64_t* elite_hist, mbrl_event_t* rollout_events, const PlanWs& w,
                        hipStream_t stream) {
    int rc;
    const FusePlan f = fuse_plan(p->N, p->N, p->K, g.a);
    // one first launch: distribution rows, the s0 copy, iteration 0's proposals (where the update
    // fuses the draw), and the plan's hand-off words zeroed (no memset before the pair / trajectory
    // launches)
    const InitZero z = plan_zero(g, p->N, w.pair, w.traj);
    if (sigma_rows) {   // (cem_init_kernel has no sigma rows: rh_init_kernel, the same values)
        RhInitArgs A{};
        A.seed = p->seed; A.init_mu = p->init_mu; A.init_sigma = p->init_sigma; A.lo = p->lo; A.hi = p->hi;
        A.H = p->H; A.a = g.a; A.N = p->N; A.s = g.s; A.B = 1; A.s0_rep = 1; A.mu_rows = mu_rows; A.sigma_rows = sigma_rows;
        A.mu = w.mu[0]; A.sigma = w.sigma[0]; A.actions = f.fuse_draw ? w.actions : nullptr;
        A.s0_src = s0_in; A.s0_dst = w.s0; A.zero = z;
        if ((rc = hip_check(launch_rh_init(A, stream), "init launch"))) return rc;
    } else {
        launch_cem_init(dim3(p->H * (f.fuse_draw ? draw_slices(p->H, 1, p->N, g.a) : 1), 1), stream, p->seed,
                        p->init_mu, p->init_sigma, p->lo, p->hi, p->H, g.a, p->N, w.mu[0], w.sigma[0],
                        f.fuse_draw ? w.actions : nullptr, s0_in, g.s, w.s0, 0, z, mu_rows);
    }
    unsigned pair_epoch = 0;
    const float* s0 = w.s0;   // the workspace copy (s0_in may be mapped host memory)
    int cur = 0;
    for (int it = 0; it < p->iterations; ++it) {
        const mbrl_sampler sp = make_sampler(p, it, w.mu[cur], w.sigma[cur]);
        float* costs = cost_hist ? cost_hist + (size_t)it * g.E * p->N : w.costs;
        int64_t* elites = elite_hist ? elite_hist + (size_t)it * p->K : w.elites;
        float* rets = returns_hist ? returns_hist + (size_t)it * p->N : nullptr;
        if ((rc = record_rollout_event(rollout_events, 2 * it, stream))) return rc;
        rc = rollout_impl(g, packed, norm, cost, s0, 0, f.fuse_draw ? w.actions : nullptr, f.fuse_draw ? nullptr : &sp,
                          p->N, p->H, 0, costs, w.actions, nullptr, stream, pair_area_bytes(g, p->N) ? w.pair : nullptr,
                          z.ptr[0] ? &pair_epoch : nullptr);
        if (rc) return rc;
        if ((rc = record_rollout_event(rollout_events, 2 * it + 1, stream))) return rc;
        if (f.fuse) {
            UpdateArgs U = make_update_args(g, p, it, costs, w.mu[cur], w.sigma[cur], w.mu[cur ^ 1], w.sigma[cur ^ 1], mu,
                                            sigma, actions_out, f.fuse_draw ? w.actions : nullptr);
            U.elite_out = elites; U.returns_out = rets;
            U.ael = w.aelite;   // (scratch of the split update)
            rc = update_impl(U, 1, stream);
        } else {
            const bool last = it + 1 == p->iterations;   // the last refit also writes mu / sigma / clip(mu)
            rc = select_impl(costs, g.E, p->N, p->K, MBRL_NAN_LAST, elites, rets, w.keys, align256((size_t)p->N * 4), stream);
            if (rc) return rc;
            rc = refit_impl(&sp, p->H, g.a, elites, p->K, p->alpha, w.aelite, w.mu[cur ^ 1], w.sigma[cur ^ 1], stream,
                            last ? mu : nullptr, last ? sigma : nullptr, last ? actions_out : nullptr);
        }
        if (rc) return rc;
        cur ^= 1;
    }
    // final mean's rollout -> predicted states [E][H][s] (E == 1: straight into states_out), member mean
    rc = final_trajectory(g, packed, norm, s0, actions_out, p->H, states_out, w.states, w.traj, stream,
                          z.ptr[1] != nullptr);
    if (rc) return rc;
    return hip_check(hipGetLastError(), "plan launch");
}

int mbrl_cem_plan(const mbrl_mlp_shape* shape, const void* packed, const mbrl_norm* norm, const mbrl_cost* cost,
                  const float* s0_in, const mbrl_cem_params* p, float* mu, float* sigma, float* actions_out,
                  float* states_out, float* cost_hist, float* returns_hist, int64_t* elite_hist,
                  mbrl_event_t* rollout_events, void* workspace, size_t ws_bytes, mbrl_stream_t stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    Geometry g;
    int rc = shape_geometry(shape, &g);
    if (rc) return rc;
    if (!p) return fail(MBRL_EINVAL, "params is NULL");
    if ((rc = cem_params_check(p))) return rc;
    if (!actions_out || !states_out || !workspace) return fail(MBRL_EINVAL, "actions_out/states_out/workspace NULL");
    if (!s0_in) return fail(MBRL_EINVAL, "s0 is NULL");
    PlanWs w = plan_ws(g, p, workspace);
    if (ws_bytes < w.bytes) return fail(MBRL_EWORKSPACE, "workspace %zu < %zu", ws_bytes, w.bytes);
    if ((rc = pair_forced_check(g, p->N))) return rc;
    return cem_plan_run(g, packed, norm, cost, s0_in, p, nullptr, nullptr, mu, sigma, actions_out, states_out,
                        cost_hist, returns_hist, elite_hist, rollout_events, w, stream);
}

// Workspace layout for mbrl_mppi_plan (PlanWs without the selection's and the elites' scratch).
struct MppiWs {
    float *costs, *mu[2], *sigma[2], *states, *actions[2], *s0;
    void* pair;
    TrajScratch traj;
    int64_t* elites;   // the elite-restricted plan's list [K] and the selection's keys (K == 0: neither)
    uint32_t* keys;
    size_t bytes;
};

// actions[2]: where the update draws the next proposals (update_samples) they go to the other buffer --
// the row's other workgroups are still streaming the proposals the rollout consumed.
static MppiWs mppi_ws(const Geometry& g, const mbrl_mppi_params* p, void* base, int K = 0) {
    MppiWs w{};
    WsCursor c(base);
    const size_t Ha = (size_t)p->H * g.a;
    w.costs = c.take<float>((size_t)g.E * p->N * 4);
    w.actions[0] = c.take<float>((size_t)p->H * p->N * g.a * 4);
    w.actions[1] = update_samples(p->N, g.a) ? c.take<float>((size_t)p->H * p->N * g.a * 4) : w.actions[0];
    w.mu[0] = c.take<float>(Ha * 4); w.mu[1] = c.take<float>(Ha * 4);
    w.sigma[0] = c.take<float>(Ha * 4); w.sigma[1] = c.take<float>(Ha * 4);
    w.states = c.take<float>((size_t)g.E * p->H * g.s * 4);
    w.traj = take_traj_scratch(c, g);
    w.s0 = c.take<float>((size_t)g.s * 4);
    w.pair = c.take<char>(pair_area_bytes(g, p->N));
    if (K > 0) {   // (behind mbrl_mppi_plan's layout, which does not move)
        w.elites = c.take<int64_t>((size_t)K * 8);
        w.keys = c.take<uint32_t>((size_t)p->N * 4);
    }
    w.bytes = c.off;
    return w;
}

static int mppi_params_check(const mbrl_mppi_params* p) {
    if (!p) return fail(MBRL_EINVAL, "mppi: params is NULL");
    if (p->N < 1 || p->H < 1 || p->iterations < 1)
        return fail(MBRL_EINVAL, "bad MPPI params N=%d H=%d I=%d", p->N, p->H, p->iterations);
    return mppi_temperature_check(p->temperature);
}

size_t mbrl_mppi_workspace_bytes(const mbrl_mlp_shape* shape, const mbrl_mppi_params* params) {
    Geometry g;
    if (shape_geometry(shape, &g) != MBRL_OK || mppi_params_check(params) != MBRL_OK) return 0;
    return mppi_ws(g, params, nullptr).bytes;
}

// The elite-restricted plans' extra settings: bad params first, then K and the clamp (MBRL_EINVAL).
static int mppi_elite_params_check(const mbrl_mppi_elite_params* ep) {
    if (!ep) return fail(MBRL_EINVAL, "mppi: params is NULL");
    if (int rc = mppi_params_check(&ep->mppi)) return rc;
    return mppi_elite_check(ep->mppi.N, ep->K, ep->sigma_min, ep->sigma_max);
}

// mbrl_mppi_plan and mbrl_mppi_plan_elite, the arguments checked and the workspace carved. ep == NULL: the classic
// plan (every finite candidate weighted), one update launch per iteration. With ep: a selection launch before each
// update (the K best into elite_hist's row or the workspace), the update restricted to them and sigma clamped;
// sigma_rows (rh_init_kernel as the first launch, as mbrl_cem_plan_rh's) only with ep.
static int mppi_plan_run(const Geometry& g, const void* packed, const mbrl_norm* norm, const mbrl_cost* cost,
                         const float* s0_in, const mbrl_mppi_params* p, const mbrl_mppi_elite_params* ep,
                         const float* init_mu_rows, const float* sigma_rows, float* mu, float* sigma, float* actions_out,
                         float* states_out, float* cost_hist, float* weight_hist, float* mu_hist, float* sigma_hist,
                         int64_t* elite_hist, mbrl_event_t* rollout_events, const MppiWs& w, hipStream_t stream) {
    int rc;
    // the update draws the next proposals itself where cem_update_kernel would (update_samples)
    const bool fuse_draw = update_samples(p->N, g.a);
    const int S = fuse_draw ? draw_slices(p->H, 1, p->N, g.a) : 1;
    const InitZero z = plan_zero(g, p->N, w.pair, w.traj);
    if (sigma_rows) {   // (cem_init_kernel has no sigma rows: rh_init_kernel, the same values)
        RhInitArgs A{};
        A.seed = p->seed; A.init_mu = p->init_mu; A.init_sigma = p->init_sigma; A.lo = p->lo; A.hi = p->hi;
        A.H = p->H; A.a = g.a; A.N = p->N; A.s = g.s; A.B = 1; A.s0_rep = 1; A.mu_rows = init_mu_rows;
        A.sigma_rows = sigma_rows; A.mu = w.mu[0]; A.sigma = w.sigma[0]; A.actions = fuse_draw ? w.actions[0] : nullptr;
        A.s0_src = s0_in; A.s0_dst = w.s0; A.zero = z;
        if ((rc = hip_check(launch_rh_init(A, stream), "init launch"))) return rc;
    } else {
        launch_cem_init(dim3(p->H * S, 1), stream, p->seed, p->init_mu, p->init_sigma, p->lo, p->hi, p->H, g.a, p->N,
                        w.mu[0], w.sigma[0], fuse_draw ? w.actions[0] : nullptr, s0_in, g.s, w.s0, 0, z, init_mu_rows);
        if ((rc = hip_check(hipGetLastError(), "init launch"))) return rc;
    }
    const size_t Ha = (size_t)p->H * g.a;
    auto record = [&](int row, int cur) {   // the distribution after `row` updates into the history
        hipError_t e = hipSuccess;
        if (mu_hist) e = hipMemcpyAsync(mu_hist + row * Ha, w.mu[cur], Ha * 4, hipMemcpyDeviceToDevice, stream);
        if (e == hipSuccess && sigma_hist)
            e = hipMemcpyAsync(sigma_hist + row * Ha, w.sigma[cur], Ha * 4, hipMemcpyDeviceToDevice, stream);
        return hip_check(e, "history copy");
    };
    if ((rc = record(0, 0))) return rc;
    unsigned pair_epoch = 0;
    const float* s0 = w.s0;   // the workspace copy (s0_in may be mapped host memory)
    int cur = 0;
    for (int it = 0; it < p->iterations; ++it) {
        const mbrl_sampler sp = make_sampler(p, it, w.mu[cur], w.sigma[cur]);
        float* costs = cost_hist ? cost_hist + (size_t)it * g.E * p->N : w.costs;
        if ((rc = record_rollout_event(rollout_events, 2 * it, stream))) return rc;
        float* acts = w.actions[fuse_draw ? (it & 1) : 0];   // this iteration's proposals
        rc = rollout_impl(g, packed, norm, cost, s0, 0, fuse_draw ? acts : nullptr, fuse_draw ? nullptr : &sp, p->N,
                          p->H, 0, costs, acts, nullptr, stream, pair_area_bytes(g, p->N) ? w.pair : nullptr,
                          z.ptr[0] ? &pair_epoch : nullptr);
        if (rc) return rc;
        if ((rc = record_rollout_event(rollout_events, 2 * it + 1, stream))) return rc;
        const bool last = it + 1 == p->iterations;   // the last update also writes mu / sigma / clip(mu)
        MppiArgs U = make_mppi_args(costs, g.E, p->N, p->H, g.a, acts, sp, p->temperature, p->alpha, p->update_sigma,
                                    w.mu[cur ^ 1], w.sigma[cur ^ 1]);
        U.fin_mu = last ? mu : nullptr; U.fin_sigma = last ? sigma : nullptr; U.fin_actions = last ? actions_out : nullptr;
        U.weights_out = weight_hist ? weight_hist + (size_t)it * p->N : nullptr;
        U.next_actions = (fuse_draw && !last) ? w.actions[(it + 1) & 1] : nullptr;
        if (ep) {
            int64_t* elites = elite_hist ? elite_hist + (size_t)it * ep->K : w.elites;
            rc = select_impl(costs, g.E, p->N, ep->K, MBRL_NAN_LAST, elites, nullptr, w.keys, align256((size_t)p->N * 4),
                             stream);
            if (rc) return rc;
            rc = hip_check(launch_mppi_update_elite(make_mppi_elite_args(U, elites, ep->K, ep->sigma_min, ep->sigma_max),
                                                    U.next_actions ? S : 1, 0, stream), "mppi elite update launch");
        } else {
            rc = hip_check(launch_mppi_update(U, U.next_actions ? S : 1, stream), "mppi update launch");
        }
        if (rc) return rc;
        cur ^= 1;
        if ((rc = record(it + 1, cur))) return rc;
    }
    // final mean's rollout -> predicted states [E][H][s] (E == 1: straight into states_out), member mean
    rc = final_trajectory(g, packed, norm, s0, actions_out, p->H, states_out, w.states, w.traj, stream,
                          z.ptr[1] != nullptr);
    if (rc) return rc;
    return hip_check(hipGetLastError(), "plan launch");
}

int mbrl_mppi_plan(const mbrl_mlp_shape* shape, const void* packed, const mbrl_norm* norm, const mbrl_cost* cost,
                   const float* s0_in, const mbrl_mppi_params* p, const float* init_mu_rows, float* mu, float* sigma,
                   float* actions_out, float* states_out, float* cost_hist, float* weight_hist, float* mu_hist,
                   float* sigma_hist, mbrl_event_t* rollout_events, void* workspace, size_t ws_bytes,
                   mbrl_stream_t stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    Geometry g;
    int rc = shape_geometry(shape, &g);
    if (rc) return rc;
    if ((rc = mppi_params_check(p))) return rc;
    if (!packed || !actions_out || !states_out || !workspace)
        return fail(MBRL_EINVAL, "mppi_plan: packed/actions_out/states_out/workspace NULL");
    if (!s0_in) return fail(MBRL_EINVAL, "mppi_plan: s0 is NULL");
    MppiWs w = mppi_ws(g, p, workspace);
    if (ws_bytes < w.bytes) return fail(MBRL_EINVAL, "mppi_plan: workspace %zu < %zu", ws_bytes, w.bytes);
    if ((rc = mppi_range_check(p->N, g.a))) return rc;
    if ((rc = pair_forced_check(g, p->N))) return rc;
    return mppi_plan_run(g, packed, norm, cost, s0_in, p, nullptr, init_mu_rows, nullptr, mu, sigma, actions_out,
                         states_out, cost_hist, weight_hist, mu_hist, sigma_hist, nullptr, rollout_events, w, stream);
}

int mbrl_mppi_plan_elite(const mbrl_mlp_shape* shape, const void* packed, const mbrl_norm* norm, const mbrl_cost* cost,
                         const float* s0_in, const mbrl_mppi_elite_params* ep, const float* init_mu_rows,
                         const float* init_sigma_rows, float* mu, float* sigma, float* actions_out, float* states_out,
                         float* cost_hist, float* weight_hist, float* mu_hist, float* sigma_hist, int64_t* elite_hist,
                         mbrl_event_t* rollout_events, void* workspace, size_t ws_bytes, mbrl_stream_t stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    Geometry g;
    int rc = shape_geometry(shape, &g);
    if (rc) return rc;
    if ((rc = mppi_elite_params_check(ep))) return rc;
    const mbrl_mppi_params* p = &ep->mppi;
    if (!packed || !actions_out || !states_out || !workspace)
        return fail(MBRL_EINVAL, "mppi_plan_elite: packed/actions_out/states_out/workspace NULL");
    if (!s0_in) return fail(MBRL_EINVAL, "mppi_plan_elite: s0 is NULL");
    MppiWs w = mppi_ws(g, p, workspace, ep->K);
    if (ws_bytes < w.bytes) return fail(MBRL_EINVAL, "mppi_plan_elite: workspace %zu < %zu", ws_bytes, w.bytes);
    if ((rc = mppi_range_check(p->N, g.a))) return rc;
    if ((rc = pair_forced_check(g, p->N))) return rc;
    return mppi_plan_run(g, packed, norm, cost, s0_in, p, ep, init_mu_rows, init_sigma_rows, mu, sigma, actions_out,
                         states_out, cost_hist, weight_hist, mu_hist, sigma_hist, elite_hist, rollout_events, w, stream);
}

// ---- batched planning: B independent CEM plans (one initial state each) in shared launches.
struct BatchWs {
    float *costs, *actions, *mu[2], *sigma[2], *s0x, *states;
    TrajScratch traj;
    int64_t* elites;
    uint32_t* keys;
    size_t bytes;
};

static BatchWs batch_ws(const Geometry& g, const mbrl_cem_params* p, int B, void* base) {
    BatchWs w{};
    WsCursor c(base);
    const size_t BN = (size_t)B * p->N, BHa = (size_t)B * p->H * g.a;
    w.traj = take_traj_scratch(c, g);   // memset block first, status right behind
    w.costs = c.take<float>((size_t)g.E * BN * 4);
    w.actions = c.take<float>((size_t)p->H * BN * g.a * 4);
    w.mu[0] = c.take<float>(BHa * 4); w.mu[1] = c.take<float>(BHa * 4);
    w.sigma[0] = c.take<float>(BHa * 4); w.sigma[1] = c.take<float>(BHa * 4);
    w.s0x = c.take<float>(BN * g.s * 4);
    w.states = c.take<float>((size_t)g.E * p->H * g.s * 4);
    w.elites = c.take<int64_t>((size_t)B * p->K * 8);
    w.keys = c.take<uint32_t>(BN * 4);
    w.bytes = c.off;
    return w;
}

size_t mbrl_cem_plan_batch_workspace_bytes(const mbrl_mlp_shape* shape, const mbrl_cem_params* params, int32_t B) {
    Geometry g;
    if (shape_geometry(shape, &g) != MBRL_OK || !params || B < 1) return 0;
    return batch_ws(g, params, B, nullptr).bytes;
}

// B * N, the candidates of one batched rollout, as mbrl_cem_plan_batch bounds it.
static int batch_size_check(int B, const mbrl_cem_params* p) {
    if ((int64_t)B * p->N > INT32_MAX / 2) return fail(MBRL_EUNSUPPORTED, "B*N too large");
    return MBRL_OK;
}

// Each problem's final mean rolled out: its states (the cooperative trajectory kernel), one launch each.
static int batch_final_trajectories(const Geometry& g, const void* packed, const mbrl_norm* norm, const float* s0, int B,
                                    int H, const float* actions_out, float* states_out, float* member_scratch,
                                    const TrajScratch& ts, hipStream_t stream) {
    const size_t Hs = (size_t)H * g.s;
    for (int b = 0; b < B; ++b) {
        int rc = final_trajectory(g, packed, norm, s0 + (size_t)b * g.s, actions_out + (size_t)b * H * g.a, H,
                                  states_out + b * Hs, member_scratch, ts, stream, 0);
        if (rc) return rc;
    }
    return hip_check(hipGetLastError(), "batched plan launch");
}

// mbrl_cem_plan_batch's launches, the arguments checked and the workspace carved: shared with the batched
// receding-horizon plan that keeps no rows (mbrl_cem_plan_rh_batch, keep == 0), which differs in the first
// launch alone where rows are given -- the initial distribution's rows (mu_rows / sigma_rows [B][H][a],
// each or NULL; flags: which apply to a problem) -- and may record (cost_hist [I][E][B N], returns_hist
// [I][B][N], elite_hist [I][B][K]).
static int cem_batch_run(const Geometry& g, const void* packed, const mbrl_norm* norm, const mbrl_cost* cost,
                         const float* s0, int B, const mbrl_cem_params* p, const float* mu_rows,
                         const float* sigma_rows, const int32_t* flags, float* mu, float* sigma, float* actions_out,
                         float* states_out, float* cost_hist, float* returns_hist, int64_t* elite_hist,
                         const BatchWs& w, hipStream_t stream) {
    int rc;
    const int BN = B * p->N, BHa = B * p->H * g.a;
    // as mbrl_cem_plan: one fused update launch per iteration where it fits (grid (H, B))
    const FusePlan f = fuse_plan(p->N, p->N, p->K, g.a);
    if (mu_rows || sigma_rows) {   // (cem_init_kernel has no per-problem rows: rh_init_kernel, the same values)
        RhInitArgs A{};
        A.seed = p->seed; A.init_mu = p->init_mu; A.init_sigma = p->init_sigma; A.lo = p->lo; A.hi = p->hi;
        A.H = p->H; A.a = g.a; A.N = p->N; A.s = g.s; A.B = B; A.mu_rows = mu_rows; A.sigma_rows = sigma_rows;
        A.flags = flags; A.mu = w.mu[0]; A.sigma = w.sigma[0]; A.actions = f.fuse_draw ? w.actions : nullptr;
        if ((rc = hip_check(launch_rh_init(A, stream), "init launch"))) return rc;
    } else if (f.fuse_draw) {
        launch_cem_init(dim3(p->H * draw_slices(p->H, B, p->N, g.a), B), stream, p->seed, p->init_mu, p->init_sigma, p->lo,
                        p->hi, p->H, g.a, p->N, w.mu[0], w.sigma[0], w.actions, nullptr, 0, nullptr, 0, InitZero{}, nullptr);
    } else {
        hipLaunchKernelGGL(fill2_kernel, dim3((BHa + 255) / 256), dim3(256), 0, stream, w.mu[0], p->init_mu,
                           w.sigma[0], p->init_sigma, BHa);
    }
    hipLaunchKernelGGL(expand_rows_kernel, dim3(256), dim3(256), 0, stream, s0, B, p->N, g.s, w.s0x);
    int cur = 0;
    for (int it = 0; it < p->iterations; ++it) {
        const mbrl_sampler sp = make_sampler(p, it, w.mu[cur], w.sigma[cur]);
        float* costs = cost_hist ? cost_hist + (size_t)it * g.E * BN : w.costs;
        int64_t* elites = elite_hist ? elite_hist + (size_t)it * B * p->K : w.elites;
        float* rets = returns_hist ? returns_hist + (size_t)it * BN : nullptr;
        // problem b's candidate n is global candidate b*N + n (its Philox counter)
        if (!f.fuse_draw) {
            rc = sample_impl(&sp, p->H, g.a, BN, 0, w.actions, stream, p->N);
            if (rc) return rc;
        }
        rc = rollout_impl(g, packed, norm, cost, w.s0x, 1, w.actions, nullptr, BN, p->H, 0, costs, nullptr, nullptr,
                          stream);
        if (rc) return rc;
        if (f.fuse) {
            UpdateArgs U = make_update_args(g, p, it, costs, w.mu[cur], w.sigma[cur], w.mu[cur ^ 1], w.sigma[cur ^ 1],
                                            mu, sigma, actions_out, f.fuse_draw ? w.actions : nullptr);
            U.member_stride = BN;
            if (elite_hist) U.elite_out = elites;
            U.returns_out = rets;
            rc = update_impl(U, B, stream);
        } else {
            const bool last = it + 1 == p->iterations;
            rc = select_impl(costs, g.E, p->N, p->K, MBRL_NAN_LAST, elites, rets, w.keys, align256((size_t)BN * 4),
                             stream, B);
            if (rc) return rc;
            rc = refit_impl(&sp, p->H, g.a, elites, p->K, p->alpha, nullptr, w.mu[cur ^ 1], w.sigma[cur ^ 1], stream,
                            last ? mu : nullptr, last ? sigma : nullptr, last ? actions_out : nullptr, B, p->N);
        }
        if (rc) return rc;
        cur ^= 1;
    }
    return batch_final_trajectories(g, packed, norm, s0, B, p->H, actions_out, states_out, w.states, w.traj, stream);
}

int mbrl_cem_plan_batch(const mbrl_mlp_shape* shape, const void* packed, const mbrl_norm* norm, const mbrl_cost* cost,
                        const float* s0, int32_t B, const mbrl_cem_params* p, float* mu, float* sigma,
                        float* actions_out, float* states_out, void* workspace, size_t ws_bytes,
                        mbrl_stream_t stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    Geometry g;
    int rc = shape_geometry(shape, &g);
    if (rc) return rc;
    if (!p || B < 1) return fail(MBRL_EINVAL, "params NULL or B=%d", B);
    if ((rc = cem_params_check(p))) return rc;
    if ((rc = batch_size_check(B, p))) return rc;
    if (!s0 || !actions_out || !states_out || !workspace) return fail(MBRL_EINVAL, "s0/actions_out/states_out/workspace NULL");
    BatchWs w = batch_ws(g, p, B, workspace);
    if (ws_bytes < w.bytes) return fail(MBRL_EWORKSPACE, "workspace %zu < %zu", ws_bytes, w.bytes);
    return cem_batch_run(g, packed, norm, cost, s0, B, p, nullptr, nullptr, nullptr, mu, sigma, actions_out, states_out,
                         nullptr, nullptr, nullptr, w, stream);
}

// ---- batched MPPI: B independent mbrl_mppi_plan plans in shared launches (BatchWs without the selection's
// scratch; actions[2] as MppiWs: where the update draws the next proposals they go to the other buffer).
struct MppiBatchWs {
    float *costs, *actions[2], *mu[2], *sigma[2], *s0x, *states;
    TrajScratch traj;
    int64_t* elites;   // the elite-restricted plan's lists [B][K] and the segmented selection's keys (K == 0: neither)
    uint32_t* keys;
    size_t bytes;
};

static MppiBatchWs mppi_batch_ws(const Geometry& g, const mbrl_mppi_params* p, int B, void* base, int K = 0) {
    MppiBatchWs w{};
    WsCursor c(base);
    const size_t BN = (size_t)B * p->N, BHa = (size_t)B * p->H * g.a;
    w.traj = take_traj_scratch(c, g);   // memset block first, status right behind
    w.costs = c.take<float>((size_t)g.E * BN * 4);
    w.actions[0] = c.take<float>((size_t)p->H * BN * g.a * 4);
    w.actions[1] = update_samples(p->N, g.a) ? c.take<float>((size_t)p->H * BN * g.a * 4) : w.actions[0];
    w.mu[0] = c.take<float>(BHa * 4); w.mu[1] = c.take<float>(BHa * 4);
    w.sigma[0] = c.take<float>(BHa * 4); w.sigma[1] = c.take<float>(BHa * 4);
    w.s0x = c.take<float>(BN * g.s * 4);
    w.states = c.take<float>((size_t)g.E * p->H * g.s * 4);
    if (K > 0) {   // (behind mbrl_mppi_plan_batch's layout, which does not move)
        w.elites = c.take<int64_t>((size_t)B * K * 8);
        w.keys = c.take<uint32_t>(BN * 4);
    }
    w.bytes = c.off;
    return w;
}

// What mbrl_mppi_batch_workspace_bytes answers and the plan demands: the larger of the batched layout and
// mbrl_mppi_plan's (which may hold a pair area the batch has no use for), so that the answer never shrinks
// as B grows and at B == 1 one query serves either entry.
static size_t mppi_batch_ws_bytes(const Geometry& g, const mbrl_mppi_params* p, int B, int K = 0) {
    const size_t batch = mppi_batch_ws(g, p, B, nullptr, K).bytes;
    const size_t single = mppi_ws(g, p, nullptr, K).bytes;
    return single > batch ? single : batch;
}

size_t mbrl_mppi_batch_workspace_bytes(const mbrl_mlp_shape* shape, const mbrl_mppi_params* params, int32_t B) {
    Geometry g;
    if (shape_geometry(shape, &g) != MBRL_OK || mppi_params_check(params) != MBRL_OK || B < 1) return 0;
    return mppi_batch_ws_bytes(g, params, B);
}

// The first launch (rh_init_kernel: each problem's initial mean from its rows or init_mu, sigma, the start
// states expanded to one per candidate and, where the update draws, iteration 0's proposals), then per
// iteration one rollout over the B N candidates and one update over the B problems (grid (H S, B)), then
// each problem's final mean rolled out, one trajectory launch each.
// With ep (mbrl_mppi_plan_elite_batch): one segmented selection launch before each update, whatever B is, the
// update restricted to each problem's K best and sigma clamped; sigma_rows [B][H][a] (flags bit 1) only with ep.
static int mppi_batch_run(const Geometry& g, const void* packed, const mbrl_norm* norm, const mbrl_cost* cost,
                          const float* s0, int B, const mbrl_mppi_params* p, const mbrl_mppi_elite_params* ep,
                          const float* init_mu_rows, const float* sigma_rows, const int32_t* input_flags, float* mu,
                          float* sigma, float* actions_out, float* states_out, float* cost_hist, float* weight_hist,
                          float* mu_hist, float* sigma_hist, int64_t* elite_hist, const MppiBatchWs& w,
                          hipStream_t stream) {
    int rc;
    const int N = p->N, BN = B * N;
    const size_t BHa = (size_t)B * p->H * g.a;
    // the update draws the next proposals itself where mbrl_mppi_plan's would (update_samples, per problem)
    const bool fuse_draw = update_samples(N, g.a);
    const int S = fuse_draw ? draw_slices(p->H, B, N, g.a) : 1;
    {
        RhInitArgs A{};
        A.seed = p->seed; A.init_mu = p->init_mu; A.init_sigma = p->init_sigma; A.lo = p->lo; A.hi = p->hi;
        A.H = p->H; A.a = g.a; A.N = N; A.s = g.s; A.B = B; A.s0_rep = N; A.mu_rows = init_mu_rows; A.flags = input_flags;
        A.sigma_rows = sigma_rows;
        A.mu = w.mu[0]; A.sigma = w.sigma[0]; A.actions = fuse_draw ? w.actions[0] : nullptr;
        A.s0_src = s0; A.s0_dst = w.s0x;
        if ((rc = hip_check(launch_rh_init(A, stream), "init launch"))) return rc;
    }
    auto record = [&](int row, int cur) {   // every problem's distribution after `row` updates into the history
        hipError_t e = hipSuccess;
        if (mu_hist) e = hipMemcpyAsync(mu_hist + row * BHa, w.mu[cur], BHa * 4, hipMemcpyDeviceToDevice, stream);
        if (e == hipSuccess && sigma_hist)
            e = hipMemcpyAsync(sigma_hist + row * BHa, w.sigma[cur], BHa * 4, hipMemcpyDeviceToDevice, stream);
        return hip_check(e, "history copy");
    };
    if ((rc = record(0, 0))) return rc;
    int cur = 0;
    for (int it = 0; it < p->iterations; ++it) {
        const mbrl_sampler sp = make_sampler(p, it, w.mu[cur], w.sigma[cur]);
        float* costs = cost_hist ? cost_hist + (size_t)it * g.E * BN : w.costs;
        float* acts = w.actions[fuse_draw ? (it & 1) : 0];   // this iteration's proposals
        // problem b's candidate n is global candidate b*N + n (its Philox counter)
        if (!fuse_draw && (rc = sample_impl(&sp, p->H, g.a, BN, 0, acts, stream, N))) return rc;
        rc = rollout_impl(g, packed, norm, cost, w.s0x, 1, acts, nullptr, BN, p->H, 0, costs, nullptr, nullptr, stream);
        if (rc) return rc;
        const bool last = it + 1 == p->iterations;   // the last update also writes mu / sigma / clip(mu)
        MppiArgs U = make_mppi_args(costs, g.E, N, p->H, g.a, acts, sp, p->temperature, p->alpha, p->update_sigma,
                                    w.mu[cur ^ 1], w.sigma[cur ^ 1]);
        U.fin_mu = last ? mu : nullptr; U.fin_sigma = last ? sigma : nullptr; U.fin_actions = last ? actions_out : nullptr;
        U.weights_out = weight_hist ? weight_hist + (size_t)it * BN : nullptr;
        U.next_actions = (fuse_draw && !last) ? w.actions[(it + 1) & 1] : nullptr;
        if (ep) {
            int64_t* elites = elite_hist ? elite_hist + (size_t)it * B * ep->K : w.elites;
            rc = select_impl(costs, g.E, N, ep->K, MBRL_NAN_LAST, elites, nullptr, w.keys, align256((size_t)BN * 4), stream,
                             B);
            if (rc) return rc;
            rc = hip_check(launch_mppi_update_elite(make_mppi_elite_args(U, elites, ep->K, ep->sigma_min, ep->sigma_max),
                                                    U.next_actions ? S : 1, B, stream), "mppi batched elite update launch");
        } else {
            rc = hip_check(launch_mppi_update_batch(U, U.next_actions ? S : 1, B, stream), "mppi batched update launch");
        }
        if (rc) return rc;
        cur ^= 1;
        if ((rc = record(it + 1, cur))) return rc;
    }
    return batch_final_trajectories(g, packed, norm, s0, B, p->H, actions_out, states_out, w.states, w.traj, stream);
}

int mbrl_mppi_plan_batch(const mbrl_mlp_shape* shape, const void* packed, const mbrl_norm* norm, const mbrl_cost* cost,
                         const float* s0, int32_t B, const mbrl_mppi_params* p, const float* init_mu_rows,
                         const int32_t* input_flags, float* mu, float* sigma, float* actions_out, float* states_out,
                         float* cost_hist, float* weight_hist, float* mu_hist, float* sigma_hist, void* workspace,
                         size_t ws_bytes, mbrl_stream_t stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    Geometry g;
    int rc = shape_geometry(shape, &g);
    if (rc) return rc;
    if ((rc = mppi_params_check(p))) return rc;
    if (B < 1) return fail(MBRL_EINVAL, "mppi_plan_batch: B=%d", B);
    if (!packed || !s0 || !actions_out || !states_out || !workspace)
        return fail(MBRL_EINVAL, "mppi_plan_batch: packed/s0/actions_out/states_out/workspace NULL");
    if ((rc = mppi_range_check(p->N, g.a))) return rc;
    if ((rc = mppi_batch_check(B, p->N))) return rc;
    const MppiBatchWs w = mppi_batch_ws(g, p, B, workspace);
    if (const size_t need = mppi_batch_ws_bytes(g, p, B); ws_bytes < need)
        return fail(MBRL_EWORKSPACE, "mppi_plan_batch: workspace %zu < %zu", ws_bytes, need);
    return mppi_batch_run(g, packed, norm, cost, s0, B, p, nullptr, init_mu_rows, nullptr, input_flags, mu, sigma,
                          actions_out, states_out, cost_hist, weight_hist, mu_hist, sigma_hist, nullptr, w, stream);
}

size_t mbrl_mppi_elite_workspace_bytes(const mbrl_mlp_shape* shape, const mbrl_mppi_elite_params* params, int32_t B) {
    Geometry g;
    if (shape_geometry(shape, &g) != MBRL_OK || mppi_elite_params_check(params) != MBRL_OK || B < 1) return 0;
    return mppi_batch_ws_bytes(g, &params->mppi, B, params->K);
}

int mbrl_mppi_plan_elite_batch(const mbrl_mlp_shape* shape, const void* packed, const mbrl_norm* norm,
                               const mbrl_cost* cost, const float* s0, int32_t B, const mbrl_mppi_elite_params* ep,
                               const float* init_mu_rows, const float* init_sigma_rows, const int32_t* input_flags,
                               float* mu, float* sigma, float* actions_out, float* states_out, float* cost_hist,
                               float* weight_hist, float* mu_hist, float* sigma_hist, int64_t* elite_hist,
                               void* workspace, size_t ws_bytes, mbrl_stream_t stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    Geometry g;
    int rc = shape_geometry(shape, &g);
    if (rc) return rc;
    if ((rc = mppi_elite_params_check(ep))) return rc;
    const mbrl_mppi_params* p = &ep->mppi;
    if (B < 1) return fail(MBRL_EINVAL, "mppi_plan_elite_batch: B=%d", B);
    if (!packed || !s0 || !actions_out || !states_out || !workspace)
        return fail(MBRL_EINVAL, "mppi_plan_elite_batch: packed/s0/actions_out/states_out/workspace NULL");
    if ((rc = mppi_range_check(p->N, g.a))) return rc;
    if ((rc = mppi_batch_check(B, p->N))) return rc;
    const MppiBatchWs w = mppi_batch_ws(g, p, B, workspace, ep->K);
    if (const size_t need = mppi_batch_ws_bytes(g, p, B, ep->K); ws_bytes < need)
        return fail(MBRL_EWORKSPACE, "mppi_plan_elite_batch: workspace %zu < %zu", ws_bytes, need);
    return mppi_batch_run(g, packed, norm, cost, s0, B, p, ep, init_mu_rows, init_sigma_rows, input_flags, mu, sigma,
                          actions_out, states_out, cost_hist, weight_hist, mu_hist, sigma_hist, elite_hist, w, stream);
}

// ---- receding-horizon CEM, single and batched, white and mixed (include/mbrl_cem.h mbrl_cem_plan_rh,
// mbrl_cem_plan_rh_batch and their _mixed forms; kernels in cem_rh.hip and cem_noise.hip). The workspaces:
// mbrl_cem_plan's (mbrl_cem_plan_batch's) first, then what kept rows need -- the two kept sets [B][Kc][H][a]
// (iteration i reads one and writes the other), the best indices [B][Kc], the returns [B][N] the carry's are
// read from and, batched, the staged elites' actions [B][H][K][a] (the single plan stages in PlanWs.aelite).
struct RhWs {
    PlanWs plan;
    float *kept[2], *rets;
    int64_t* best;
    size_t bytes;
};

// mixed: the returns also with keep == 0, where that plan selects unfused too.
static RhWs rh_ws(const Geometry& g, const mbrl_cem_rh_params* rp, void* base, bool mixed = false) {
    RhWs w{};
    w.plan = plan_ws(g, &rp->cem, base);
    WsCursor c(base);
    c.off = w.plan.bytes;
    const size_t kb = (size_t)rp->keep * rp->cem.H * g.a * 4;
    w.kept[0] = c.take<float>(kb); w.kept[1] = c.take<float>(kb);
    w.best = c.take<int64_t>((size_t)rp->keep * 8);
    w.rets = c.take<float>(rp->keep || mixed ? (size_t)rp->cem.N * 4 : 0);
    w.bytes = c.off;
    return w;
}

struct RhBatchWs {
    BatchWs plan;
    float *aelite, *kept[2], *rets;
    int64_t* best;
    size_t bytes;
};

// mixed: the staged elites and the returns also with keep == 0. ts_rows (a sampled-rollout source's Q, else 0):
// the layout of a mixed plan, then cost rows [Q][B N] of its own in place of the E rows.
static RhBatchWs rh_batch_ws(const Geometry& g, const mbrl_cem_rh_params* rp, int B, void* base, bool mixed = false,
                             int ts_rows = 0) {
    RhBatchWs w{};
    const mbrl_cem_params* p = &rp->cem;
    w.plan = batch_ws(g, p, B, base);
    WsCursor c(base);
    c.off = w.plan.bytes;
    const size_t kb = (size_t)B * rp->keep * p->H * g.a * 4;
    w.aelite = c.take<float>(rp->keep || mixed ? (size_t)B * p->H * p->K * g.a * 4 : 0);
    w.kept[0] = c.take<float>(kb); w.kept[1] = c.take<float>(kb);
    w.best = c.take<int64_t>((size_t)B * rp->keep * 8);
    w.rets = c.take<float>(rp->keep || mixed ? (size_t)B * p->N * 4 : 0);
    if (ts_rows) w.plan.costs = c.take<float>((size_t)ts_rows * B * p->N * 4);
    w.bytes = c.off;
    return w;
}

// What mbrl_cem_rh_mixed_workspace_bytes answers and both mixed entries demand: the batched layout, and for
// B == 1 the larger of it and the single plan's (one query serves either entry).
static size_t mixed_ws_bytes(const Geometry& g, const mbrl_cem_rh_params* rp, int B) {
    const size_t batch = rh_batch_ws(g, rp, B, nullptr, true).bytes;
    if (B > 1) return batch;
    const size_t single = rh_ws(g, rp, nullptr, true).bytes;
    return single > batch ? single : batch;
}

static int rh_params_check(const mbrl_cem_rh_params* rp) {
    if (!rp) return fail(MBRL_EINVAL, "cem_plan_rh: params is NULL");
    if (int rc = cem_params_check(&rp->cem)) return rc;
    if (rp->keep < 0 || rp->keep > rp->cem.K)
        return fail(MBRL_EINVAL, "cem_plan_rh: keep=%d outside [0, K=%d]", rp->keep, rp->cem.K);
    return MBRL_OK;
}

size_t mbrl_cem_rh_workspace_bytes(const mbrl_mlp_shape* shape, const mbrl_cem_rh_params* params) {
    Geometry g;
    if (shape_geometry(shape, &g) != MBRL_OK || rh_params_check(params) != MBRL_OK) return 0;
    return rh_ws(g, params, nullptr).bytes;
}

size_t mbrl_cem_rh_batch_workspace_bytes(const mbrl_mlp_shape* shape, const mbrl_cem_rh_params* params, int32_t B) {
    Geometry g;
    if (shape_geometry(shape, &g) != MBRL_OK || rh_params_check(params) != MBRL_OK || B < 1) return 0;
    return rh_batch_ws(g, params, B, nullptr).bytes;
}

size_t mbrl_cem_rh_mixed_workspace_bytes(const mbrl_mlp_shape* shape, const mbrl_cem_rh_params* params, int32_t B) {
    Geometry g;
    if (shape_geometry(shape, &g) != MBRL_OK || rh_params_check(params) != MBRL_OK || B < 1) return 0;
    if (params->cem.H > NOISE_MAX_H) return 0;
    return mixed_ws_bytes(g, params, B);
}

// Every refusal of the four entries, before any launch, in this order: the shape, B, the parameters, a carry
// without kept rows, NULL arguments, the mix's horizon, N, B N, then -- where the plan runs the kept-rows loop
// (keep > 0, a mix or a sampled-rollout source) -- B (the selections run one workgroup per problem, the staged refit a (H, B) grid) and
// the staged refit's K x a, the workspace (the single entries answer MBRL_EINVAL, the batched ones
// MBRL_EWORKSPACE) and, for the single plan, a forced pair kernel that does not apply. On MBRL_OK the entry's
// workspace is carved: *single or *batch. A call with a source carves the batched layout whichever entry it is
// (the single one keeps its codes) and has no pair kernel to force.
static int rh_entry_check(const RhCall& c, Geometry* g, RhWs* single, RhBatchWs* batch) {
    int rc = shape_geometry(c.shape, g);
    if (rc) return rc;
    if (c.B < 1) return fail(MBRL_EINVAL, "%s: B=%d", c.name, c.B);
    if ((rc = rh_params_check(c.rp))) return rc;
    const mbrl_cem_params* p = &c.rp->cem;
    const bool kept_loop = c.rp->keep > 0 || c.mix || c.ts;
    if (c.carry_in && c.rp->keep == 0) return fail(MBRL_EINVAL, "%s: carry_in given with keep == 0", c.name);
    if (!c.packed || (c.batched && !c.s0) || !c.actions_out || !c.states_out || !c.workspace)
        return fail(MBRL_EINVAL, "%s: packed/%sactions_out/states_out/workspace NULL", c.name, c.batched ? "s0/" : "");
    if (!c.s0) return fail(MBRL_EINVAL, "%s: s0 is NULL", c.name);
    if (c.mix && (rc = noise_check(p->H))) return rc;
    if (p->N > 32768) return fail(MBRL_EUNSUPPORTED, "%s: N=%d exceeds 32768", c.name, p->N);
    if ((rc = batch_size_check(c.B, p))) return rc;
    if (kept_loop && c.B > 65535) return fail(MBRL_EUNSUPPORTED, "%s: B=%d exceeds 65535", c.name, c.B);
    if (kept_loop && (rc = refit_staged_check(g->a, p->K))) return rc;
    // the entry's workspace carved (*single or *batch) and its size: a mixed plan demands what its query answers
    size_t need = c.ts        ? (*batch = rh_batch_ws(*g, c.rp, c.B, c.workspace, true, c.ts->Q)).bytes
                  : c.batched ? (*batch = rh_batch_ws(*g, c.rp, c.B, c.workspace, c.mix != nullptr)).bytes
                              : (*single = rh_ws(*g, c.rp, c.workspace, c.mix != nullptr)).bytes;
    if (c.mix) need = mixed_ws_bytes(*g, c.rp, c.B);
    if (c.ws_bytes < need)
        return fail(c.batched ? MBRL_EWORKSPACE : MBRL_EINVAL, "%s: workspace %zu < %zu", c.name, c.ws_bytes, need);
    return c.batched || c.ts ? MBRL_OK : pair_forced_check(*g, p->N);
}

// What the kept-rows loop of the single plan and of a batch differ in: where the buffers live and how the
// rollout and the trajectory are fed.
struct RhLoop {
    float *costs, *actions, *mu[2], *sigma[2], *aelite, *kept[2], *rets, *states;
    int64_t *elites, *best;
    uint32_t* keys;
    TrajScratch traj;
    float* s0_ws;           // the rollout's start states: s0_rep copies of each problem's
    int s0_rep, s0_per_cand;
    const float* s0_traj;   // [B][s] for the final trajectories
    void* pair;             // the pair area (the single plan, where its size offers pairs), or NULL
    InitZero zero;          // the hand-off words the first launch zeroes (the single plan's)
};

// The single plan: its own s0 copy (s0_in may be mapped host memory), the pair area and the prezeroed words.
static RhLoop rh_loop_single(const Geometry& g, int N, const RhWs& rw) {
    const PlanWs& w = rw.plan;
    return {w.costs, w.actions, {w.mu[0], w.mu[1]}, {w.sigma[0], w.sigma[1]}, w.aelite, {rw.kept[0], rw.kept[1]},
            rw.rets, w.states, w.elites, rw.best, w.keys, w.traj, w.s0, 1, 0, w.s0,
            pair_area_bytes(g, N) ? w.pair : nullptr, plan_zero(g, N, w.pair, w.traj)};
}

// A batch: per-candidate start states, no pairs, nothing prezeroed, the trajectories from the caller's s0.
static RhLoop rh_loop_batch(const RhBatchWs& rw, int N, const float* s0) {
    const BatchWs& w = rw.plan;
    return {w.costs, w.actions, {w.mu[0], w.mu[1]}, {w.sigma[0], w.sigma[1]}, rw.aelite, {rw.kept[0], rw.kept[1]},
            rw.rets, w.states, w.elites, rw.best, w.keys, w.traj, w.s0x, N, 1, s0, nullptr, InitZero{}};
}

static RhInitArgs rh_init_args(const Geometry& g, const RhCall& c, const RhLoop& L) {
    const mbrl_cem_params* p = &c.rp->cem;
    RhInitArgs A{};
    A.seed = p->seed; A.init_mu = p->init_mu; A.init_sigma = p->init_sigma; A.lo = p->lo; A.hi = p->hi;
    A.H = p->H; A.a = g.a; A.N = p->N; A.Kc = c.rp->keep; A.s = g.s; A.B = c.B; A.s0_rep = L.s0_rep;
    A.mu_rows = c.mu_rows; A.sigma_rows = c.sigma_rows; A.carry_in = c.carry_in; A.flags = c.flags;
    A.mu = L.mu[0]; A.sigma = L.sigma[0]; A.actions = L.actions; A.kept0 = c.kept_hist;
    A.s0_src = c.s0; A.s0_dst = L.s0_ws; A.zero = L.zero;
    return A;
}

// kept_cur / kept_next: kept_it and kept_{it+1}; iteration 0 reads carry_in where it is and honours the
// problems' input flags, from iteration 1 on every problem has a kept set.
static RhGatherArgs rh_gather_args(const Geometry& g, const RhCall& c, const RhLoop& L, int it, int cur,
                                   const float* rets, const int64_t* elites, const float* kept_cur, float* kept_next) {
    const mbrl_cem_params* p = &c.rp->cem;
    const bool last = it + 1 == p->iterations;
    RhGatherArgs G{};
    G.seed = p->seed; G.iteration = it; G.N = p->N; G.H = p->H; G.a = g.a; G.K = p->K; G.Kc = c.rp->keep; G.B = c.B;
    G.from_kept = it > 0 || c.carry_in; G.flags = it == 0 ? c.flags : nullptr; G.lo = p->lo; G.hi = p->hi;
    G.mu = L.mu[cur]; G.sigma = L.sigma[cur]; G.kept_cur = it == 0 ? c.carry_in : kept_cur; G.returns = rets;
    G.elites = elites; G.best = L.best; G.aelite = L.aelite; G.kept_next = kept_next;
    G.kept_copy = last ? c.carry_out : nullptr; G.best_returns = last ? c.carry_returns_out : nullptr;
    return G;
}

// After iteration `it`'s refit into mu / sigma [cur ^ 1]: the next proposals, or the plan outputs.
static RhDrawArgs rh_draw_args(const Geometry& g, const RhCall& c, const RhLoop& L, int it, int cur, const float* kept) {
    const mbrl_cem_params* p = &c.rp->cem;
    const bool last = it + 1 == p->iterations;
    RhDrawArgs D{};
    D.seed = p->seed; D.iteration = it + 1; D.H = p->H; D.a = g.a; D.N = p->N; D.Kc = c.rp->keep; D.B = c.B;
    D.lo = p->lo; D.hi = p->hi;
    D.mu = L.mu[cur ^ 1]; D.sigma = L.sigma[cur ^ 1]; D.kept = kept;
    D.actions = last ? nullptr : L.actions;
    D.fin_mu = last ? c.mu : nullptr; D.fin_sigma = last ? c.sigma : nullptr; D.fin_actions = last ? c.actions_out : nullptr;
    return D;
}

// keep > 0, B problems (the single plan: B = 1): every iteration is the one rollout of the B N proposals in
// L.actions, then five small launches, each over all B problems -- the K elites, the Kc best (the same returns
// selected twice, segmented by problem), the gather of both sets' action rows, the refit over the gathered
// elites (grid (H, B)), and the next proposals (kept rows scattered into slots [0, Kc), the rest drawn) or, on
// the last iteration, the plan outputs. kept_i lives in kept_hist's row i where the caller records, else in
// the workspace's two buffers. Then each problem's final mean rolled out, one trajectory launch each.
// mix (NULL: none): the same loop for any keep >= 0 with the first launch, the gather and the draw coloured
// (cem_noise.hip); the Kc selection runs only when Kc > 0.
// c.ts (NULL: none): the same white loop for any keep >= 0 with the sampled rollout of iteration `it` in place of
// the deterministic one; the cost rows, the selections and the returns then run over its Q rows.
static int cem_plan_rh_kept(const Geometry& g, const RhCall& c, const RhLoop& L, hipStream_t stream) {
    const mbrl_cem_params* p = &c.rp->cem;
    const float* mix = c.mix;
    const int B = c.B, Kc = c.rp->keep, BN = B * p->N, rows = c.ts ? c.ts->Q : g.E;
    const size_t kept_floats = (size_t)B * Kc * p->H * g.a;
    auto kept_at = [&](int i) { return c.kept_hist ? c.kept_hist + (size_t)i * kept_floats : L.kept[i & 1]; };
    int rc;
    const RhInitArgs A = rh_init_args(g, c, L);
    if ((rc = hip_check(mix ? launch_noise_init(A, mix, stream) : launch_rh_init(A, stream), "init launch"))) return rc;
    unsigned pair_epoch = 0;
    const size_t keys_bytes = align256((size_t)BN * 4);
    int cur = 0;
    for (int it = 0; it < p->iterations; ++it) {
        float* costs = c.cost_hist ? c.cost_hist + (size_t)it * rows * BN : L.costs;
        int64_t* elites = c.elite_hist ? c.elite_hist + (size_t)it * B * p->K : L.elites;
        float* rets = c.returns_hist ? c.returns_hist + (size_t)it * BN : L.rets;
        if ((rc = record_rollout_event(c.events, 2 * it, stream))) return rc;
        if (c.ts)
            rc = ts_source_rollout(*c.ts, L.s0_ws, L.actions, BN, it, costs, stream);
        else
            rc = rollout_impl(g, c.packed, c.norm, c.cost, L.s0_ws, L.s0_per_cand, L.actions, nullptr, BN, p->H, 0, costs,
                              nullptr, nullptr, stream, L.pair, L.zero.ptr[0] ? &pair_epoch : nullptr);
        if (rc) return rc;
        if ((rc = record_rollout_event(c.events, 2 * it + 1, stream))) return rc;
        if ((rc = select_impl(costs, rows, p->N, p->K, MBRL_NAN_LAST, elites, rets, L.keys, keys_bytes, stream, B)))
            return rc;
        if (Kc && (rc = select_impl(costs, rows, p->N, Kc, MBRL_NAN_LAST, L.best, nullptr, L.keys, keys_bytes, stream, B)))
            return rc;
        const RhGatherArgs G = rh_gather_args(g, c, L, it, cur, rets, elites, kept_at(it), kept_at(it + 1));
        if ((rc = hip_check(mix ? launch_noise_gather(G, mix, stream) : launch_rh_gather(G, stream), "gather launch")))
            return rc;
        rc = refit_staged_impl(L.aelite, p->H, g.a, p->K, p->alpha, L.mu[cur], L.sigma[cur], L.mu[cur ^ 1],
                               L.sigma[cur ^ 1], stream, B);
        if (rc) return rc;
        const RhDrawArgs D = rh_draw_args(g, c, L, it, cur, kept_at(it + 1));
        if ((rc = hip_check(mix ? launch_noise_draw(D, mix, stream) : launch_rh_draw(D, stream), "draw launch"))) return rc;
        cur ^= 1;
    }
    // each final mean's rollout -> predicted states [E][H][s] (E == 1: straight into states_out), member mean
    const size_t Hs = (size_t)p->H * g.s;
    for (int b = 0; b < B; ++b) {
        rc = final_trajectory(g, c.packed, c.norm, L.s0_traj + (size_t)b * g.s, c.actions_out + (size_t)b * p->H * g.a,
                              p->H, c.states_out + b * Hs, L.states, L.traj, stream, L.zero.ptr[1] != nullptr);
        if (rc) return rc;
    }
    return hip_check(hipGetLastError(), c.batched ? "batched plan launch" : "plan launch");
}

// The four entries: the checks, then the fused-update loops where no rows are kept and no mix is given
// (cem_plan_run / cem_batch_run with the initial distribution's rows), else the kept-rows loop. A call with a
// sampled-rollout source always takes the kept-rows loop, on the batched layout.
static int rh_plan_run(const RhCall& c) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(c.stream);
    Geometry g;
    RhWs w;
    RhBatchWs bw;
    if (int rc = rh_entry_check(c, &g, &w, &bw)) return rc;
    const mbrl_cem_params* p = &c.rp->cem;
    const bool kept_loop = c.rp->keep > 0 || c.mix || c.ts;
    if (kept_loop)
        return cem_plan_rh_kept(g, c, c.batched || c.ts ? rh_loop_batch(bw, p->N, c.s0) : rh_loop_single(g, p->N, w),
                                stream);
    if (c.batched)
        return cem_batch_run(g, c.packed, c.norm, c.cost, c.s0, c.B, p, c.mu_rows, c.sigma_rows, c.flags, c.mu, c.sigma,
                             c.actions_out, c.states_out, c.cost_hist, c.returns_hist, c.elite_hist, bw.plan, stream);
    return cem_plan_run(g, c.packed, c.norm, c.cost, c.s0, p, c.mu_rows, c.sigma_rows, c.mu, c.sigma, c.actions_out,
                        c.states_out, c.cost_hist, c.returns_hist, c.elite_hist, c.events, w.plan, stream);
}

int mbrl_cem_plan_rh_mixed(const mbrl_mlp_shape* shape, const void* packed, const mbrl_norm* norm,
                           const mbrl_cost* cost, const float* s0_in, const mbrl_cem_rh_params* rp,
                           const float* init_mu_rows, const float* init_sigma_rows, const float* carry_in,
                           const float* noise_mix, float* mu, float* sigma, float* actions_out, float* states_out,
                           float* carry_out, float* carry_returns_out, float* cost_hist, float* returns_hist,
                           int64_t* elite_hist, float* kept_hist, mbrl_event_t* rollout_events, void* workspace,
                           size_t ws_bytes, mbrl_stream_t stream) {
    return rh_plan_run({noise_mix ? "cem_plan_rh_mixed" : "cem_plan_rh", false, shape, packed, norm, cost, s0_in, 1, rp,
                    init_mu_rows, init_sigma_rows, carry_in, nullptr, noise_mix, mu, sigma, actions_out, states_out,
                    carry_out, carry_returns_out, cost_hist, returns_hist, elite_hist, kept_hist, rollout_events,
                    workspace, ws_bytes, stream});
}

int mbrl_cem_plan_rh(const mbrl_mlp_shape* shape, const void* packed, const mbrl_norm* norm, const mbrl_cost* cost,
                     const float* s0_in, const mbrl_cem_rh_params* rp, const float* init_mu_rows,
                     const float* init_sigma_rows, const float* carry_in, float* mu, float* sigma, float* actions_out,
                     float* states_out, float* carry_out, float* carry_returns_out, float* cost_hist,
                     float* returns_hist, int64_t* elite_hist, float* kept_hist, mbrl_event_t* rollout_events,
                     void* workspace, size_t ws_bytes, mbrl_stream_t stream) {
    return mbrl_cem_plan_rh_mixed(shape, packed, norm, cost, s0_in, rp, init_mu_rows, init_sigma_rows, carry_in, nullptr,
                                  mu, sigma, actions_out, states_out, carry_out, carry_returns_out, cost_hist,
                                  returns_hist, elite_hist, kept_hist, rollout_events, workspace, ws_bytes, stream);
}

int mbrl_cem_plan_rh_batch_mixed(const mbrl_mlp_shape* shape, const void* packed, const mbrl_norm* norm,
                                 const mbrl_cost* cost, const float* s0, int32_t B, const mbrl_cem_rh_params* rp,
                                 const float* init_mu_rows, const float* init_sigma_rows, const float* carry_in,
                                 const int32_t* input_flags, const float* noise_mix, float* mu, float* sigma,
                                 float* actions_out, float* states_out, float* carry_out, float* carry_returns_out,
                                 float* cost_hist, float* returns_hist, int64_t* elite_hist, float* kept_hist,
                                 void* workspace, size_t ws_bytes, mbrl_stream_t stream) {
    return rh_plan_run({noise_mix ? "cem_plan_rh_batch_mixed" : "cem_plan_rh_batch", true, shape, packed, norm, cost, s0, B,
                    rp, init_mu_rows, init_sigma_rows, carry_in, input_flags, noise_mix, mu, sigma, actions_out,
                    states_out, carry_out, carry_returns_out, cost_hist, returns_hist, elite_hist, kept_hist, nullptr,
                    workspace, ws_bytes, stream});
}

int mbrl_cem_plan_rh_batch(const mbrl_mlp_shape* shape, const void* packed, const mbrl_norm* norm,
                           const mbrl_cost* cost, const float* s0, int32_t B, const mbrl_cem_rh_params* rp,
                           const float* init_mu_rows, const float* init_sigma_rows, const float* carry_in,
                           const int32_t* input_flags, float* mu, float* sigma, float* actions_out, float* states_out,
                           float* carry_out, float* carry_returns_out, float* cost_hist, float* returns_hist,
                           int64_t* elite_hist, float* kept_hist, void* workspace, size_t ws_bytes,
                           mbrl_stream_t stream) {
    return mbrl_cem_plan_rh_batch_mixed(shape, packed, norm, cost, s0, B, rp, init_mu_rows, init_sigma_rows, carry_in,
                                        input_flags, nullptr, mu, sigma, actions_out, states_out, carry_out,
                                        carry_returns_out, cost_hist, returns_hist, elite_hist, kept_hist, workspace,
                                        ws_bytes, stream);
}

}  // extern "C"

namespace mbrl {

int rh_plan(const RhCall& c) { return rh_plan_run(c); }

size_t rh_ts_workspace_bytes(const mbrl_mlp_shape* shape, const mbrl_cem_rh_params* rp, int Q, int B) {
    Geometry g;
    if (shape_geometry(shape, &g) != MBRL_OK || rh_params_check(rp) != MBRL_OK || B < 1 || Q < 1) return 0;
    return rh_batch_ws(g, rp, B, nullptr, true, Q).bytes;
}

}  // namespace mbrl
