/*
 * mbrl_cem.h -- C ABI of the MI355X (gfx950) MPC/CEM planning hot path.
 *
 * This is the drop-in boundary under the reference's planner API. The reference is pure
 * Python/PyTorch-CPU and has no FFI of its own; each entry point below replaces
 * one piece of the reference's Python call chain, cited per function. The Python host layer
 * (mujoco-mbrl_amd/mbrl_amd) binds these with ctypes (INTEGRATION.md shows the binding).
 *
 * Conventions
 *   - All tensor pointers are DEVICE pointers (caller-owned HBM, e.g. torch tensors' data_ptr()),
 *     fp32 row-major unless stated; index buffers are int64 (torch.long).
 *   - Nothing here allocates or frees device memory, synchronises the device, or retains a pointer
 *     after it returns; scratch comes from the caller's workspace. Every call is stream-ordered on
 *     `stream` (a hipStream_t) and may be captured into a HIP graph.
 *   - A workspace may hold ANY bytes on entry: no call's result depends on what its workspace held
 *     before, and a call writes only its workspace's first *_workspace_bytes bytes and its outputs. One
 *     buffer may therefore be reused, without clearing, by calls of different entries, shapes and sizes
 *     that follow each other on one stream (every plan clears the flags, hand-off granules, gates and
 *     status words it polls in its own first launch or with a memset it enqueues itself). Calls that may
 *     be in flight at once -- on two streams, or from two threads -- need a workspace each. The one
 *     exception is the single-model training workspace (mbrl_train_grads / mbrl_train_epoch): the caller
 *     zeroes it once before its first use and then reuses it as it is (see mbrl_train_status_offset).
 *     tests/test_gpu_workspace_independence.py holds every entry to this.
 *   - Return value: MBRL_OK (0) or a negative MBRL_E* code; mbrl_last_error() then holds a
 *     thread-local message. The Python layer turns a nonzero code into RuntimeError, matching the
 *     reference's exceptions-only convention.
 *   - No HIP call happens at library load (fork safety: parallel.py:1-2,20-52 pickles planners
 *     into forkserver workers).
 */
#ifndef MBRL_CEM_H
#define MBRL_CEM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* v13 also carries the MPPI calls (mbrl_mppi_update, mbrl_mppi_workspace_bytes, mbrl_mppi_plan and
 * mbrl_mppi_params): they were added within v13, purely additively -- no existing entry point, struct
 * or option changed, so the version did not move. The receding-horizon CEM plan (mbrl_cem_rh_params,
 * mbrl_cem_rh_workspace_bytes, mbrl_cem_plan_rh) joined them the same way, and its batched form
 * (mbrl_cem_rh_batch_workspace_bytes, mbrl_cem_plan_rh_batch) after it, then batched MPPI
 * (mbrl_mppi_update_batch, mbrl_mppi_batch_workspace_bytes, mbrl_mppi_plan_batch), then MPPI over the K best
 * (mbrl_mppi_elite_params, mbrl_mppi_update_elite, mbrl_mppi_update_elite_batch,
 * mbrl_mppi_elite_workspace_bytes, mbrl_mppi_plan_elite, mbrl_mppi_plan_elite_batch), and training on the
 * open-loop loss (mbrl_train_open_loop_workspace_bytes, mbrl_train_grads_open_loop,
 * mbrl_train_epoch_open_loop), and global-norm gradient clipping for the ensemble epochs (mbrl_grad_clip,
 * mbrl_grad_clip_workspace_bytes, mbrl_grad_norm, mbrl_adam_step_clipped, mbrl_train_epoch_ensemble_clipped,
 * mbrl_train_epoch_open_loop_clipped), and the device-resident transitions (mbrl_stack_field, mbrl_dataset_stack,
 * mbrl_stats_field, mbrl_dataset_stats_workspace_bytes, mbrl_dataset_stats), and probabilistic members trained on
 * the Gaussian negative log-likelihood (mbrl_nll_bounds, mbrl_train_nll_workspace_bytes, mbrl_train_grads_nll,
 * mbrl_train_epoch_nll, mbrl_train_epoch_nll_clipped, mbrl_eval_members_nll), and trajectory-sampling rollouts on
 * them (mbrl_ts_params, mbrl_rollout_cost_ts, mbrl_cem_ts_workspace_bytes, mbrl_cem_plan_ts), then the per-step
 * member draw and the receding-horizon plans on sampled rows (mbrl_ts_rows, mbrl_rollout_cost_ts_rows,
 * mbrl_cem_ts_rh_workspace_bytes, mbrl_cem_plan_ts_rh, mbrl_cem_plan_ts_rh_batch). */
#define MBRL_ABI_VERSION 13

typedef struct ihipStream_t* mbrl_stream_t; /* == hipStream_t */
typedef struct ihipEvent_t* mbrl_event_t;   /* == hipEvent_t  */

enum {
    MBRL_OK = 0,
    MBRL_EINVAL = -1,        /* bad argument (null pointer, non-positive size, K > N, ...) */
    MBRL_EUNSUPPORTED = -2,  /* shape outside what the kernels are built for */
    MBRL_EHIP = -3,          /* a HIP runtime call failed */
    MBRL_EWORKSPACE = -4,    /* workspace too small */
    MBRL_EPEER = -5          /* mbrl_cem_plan_sharded: another rank failed during the plan (ABI v13); this
                                rank's outputs are void, its communicator stays usable */
};

/* Cost kinds.
 * GOAL_STATE   = state_action_cost(SmoothAbsLoss, CoshLoss) on (s_{t+1}, a_t), agents.py:182-183,231.
 * MODEL_REWARD = the reward head of the dynamics model itself, evaluated at (s_{t+1}, a_t) and
 *                unnormalised: RewardAgent's compose(partial(model, ...), itemgetter(1)) cost
 *                (agents.py:342-362, models.py:143-163). Needs mbrl_mlp_shape.reward_head = 1; every
 *                step then runs the MLP twice (the state pass, then the reward pass). */
enum { MBRL_COST_GOAL_STATE = 0, MBRL_COST_MODEL_REWARD = 1 };

/* Ordering of NaN returns in elite selection. */
enum {
    MBRL_NAN_LAST = 0,  /* np.argsort(kind="stable") order: NaN after every number (CEM elites)     */
    MBRL_NAN_FIRST = 1  /* np.argmin order: the first NaN wins (RandomShootingPlanner, planners.py:184) */
};

/* Matrix-product precision of the rollout's MLP layers (mbrl_mlp_shape.precision).
 * F32   = v_mfma_f32_16x16x4_f32: exact fp32 products, fp32 accumulation.
 * F16X3 / F16X6 = fp32 emulated on the f16 matrix cores (v_mfma_f32_16x16x32_f16, 16x the fp32
 *         matrix rate). Each operand is scaled by an exact power of two and split into P f16
 *         pieces x0 = f16(x), x1 = f16(x - x0) (, x2 = f16(x - x0 - x1)); the products x_i w_j with
 *         i + j < P accumulate in fp32.
 *         F16X3: P = 2, 3 products, operands to 22 significant bits (fp32: 24); the dropped
 *                term is 2^-22 relative.
 *         F16X6: P = 3, 6 products, operands to 33 significant bits, dropped terms <= 2^-33
 *                relative: at least fp32's operand precision with exact partial products.
 *         Operands past the split range (activations >= 2048, weights >= 128) cannot be split;
 *         a workgroup that meets one redoes its candidates in F32 (on the device, in the same
 *         call), so results never depend on the operand range. Used for goal-state costs with
 *         256 <= W <= 512; every other case runs F32. */
enum { MBRL_PRECISION_F32 = 0, MBRL_PRECISION_F16X3 = 1, MBRL_PRECISION_F16X6 = 2 };

/* Dynamics MLP shape: Linear(s+a -> W), ReLU, [Linear(W -> W), ReLU] x (L-1), Linear(W -> s).
 * models.py:96-110 (Model, L = 2) generalised to L hidden layers; E ensemble members.
 * reward_head = 1: ModelWithReward (models.py:125-141): the same trunk plus a reward head
 * Linear(W -> 1) beside the state head. */
typedef struct {
    int32_t state_dim;   /* s  (observation dim, env_wrappers.py:86 flat 'observations') */
    int32_t action_dim;  /* a  (rollouts and plans: <= 48, else MBRL_EUNSUPPORTED) */
    int32_t hidden;      /* W  (1 .. 1024, else MBRL_EUNSUPPORTED; zero-padded inside the packed stream) */
    int32_t n_hidden;    /* L  (1 .. 4, else MBRL_EUNSUPPORTED) */
    int32_t ensemble;    /* E >= 1 */
    int32_t reward_head; /* 0 or 1 */
    int32_t precision;   /* MBRL_PRECISION_* (rollout only; the packed buffer holds every weight
                            stream, so one pack serves each precision) */
} mbrl_mlp_shape;

/* Normalisation affine, TransitionsDataset.normalize_field / unnormalize_field (data.py:255-260),
 * bound as in agents.py:219-230. A zero flag = that keyword was None in the reference call.
 * A statistics pointer may be NULL exactly when no set flag uses it: obs_mean / obs_std when
 * normalize_state and unnormalize_state are both 0, act_mean / act_std when normalize_action is 0,
 * rew_mean / rew_std when unnormalize_reward is 0. A set flag whose statistics are NULL is
 * MBRL_EINVAL in every entry that takes an mbrl_norm, returned before any kernel that reads the
 * statistics is launched (mbrl_rollout_cost, mbrl_trajectory and mbrl_gd_plan launch nothing at
 * all; the whole-plan entries may already have launched their initialisation kernel, which reads
 * none). Passing norm == NULL means all four flags are 0. */
typedef struct {
    const float* obs_mean;  /* [s] */
    const float* obs_std;   /* [s] */
    const float* act_mean;  /* [a] */
    const float* act_std;   /* [a] */
    const float* rew_mean;  /* [1] "rewards" statistics (agents.py:340), reward_head models only */
    const float* rew_std;   /* [1] */
    int32_t normalize_state;
    int32_t unnormalize_state;
    int32_t normalize_action;
    int32_t unnormalize_reward;
} mbrl_norm;

/* Per-step cost on the (s_{t+1}, a_t) pair (planners.py:210). */
typedef struct {
    int32_t kind;             /* MBRL_COST_GOAL_STATE or MBRL_COST_MODEL_REWARD */
    int32_t has_state_cost;   /* SmoothAbsLoss term present (models.py:244-259) */
    int32_t has_action_cost;  /* CoshLoss term present (models.py:262-272) */
    int32_t _pad;
    const float* weights;     /* [s] SmoothAbsLoss.weights */
    const float* goal;        /* [s] SmoothAbsLoss.goal_state */
    float alpha_state;        /* SmoothAbsLoss.alpha (default 0.4) */
    float alpha_action;       /* CoshLoss.alpha (default 0.25) */
} mbrl_cost;

/* CEM proposal: a[t][n][d] = clip(mu[t][d] + sigma[t][d] * eps, lo, hi), eps from Philox4x32-10
 * keyed by `seed`, counter (n + n_offset, t, iteration, d >> 2). Bounds follow the reference's
 * dim-0 action bounds [max(min[0],-3), min(max[0],3)] (env_wrappers.py:52-55). */
typedef struct {
    uint64_t seed;
    int32_t iteration;
    int32_t _pad;
    const float* mu;     /* [H][a] */
    const float* sigma;  /* [H][a] */
    float lo;
    float hi;
} mbrl_sampler;

typedef struct {
    int32_t N;            /* candidates (global; == local when not sharded) */
    int32_t H;            /* horizon */
    int32_t K;            /* elites */
    int32_t iterations;   /* I */
    float alpha;          /* refit smoothing: mu <- alpha*mu + (1-alpha)*mu' */
    float lo, hi;         /* action bounds */
    float init_mu;        /* initial mean (0) */
    float init_sigma;     /* initial std ((hi-lo)/4) */
    int32_t _pad;
    uint64_t seed;
} mbrl_cem_params;

/* MPPI plan settings (added within ABI v13: the MPPI calls are purely additive). */
typedef struct {
    int32_t N, H, iterations, update_sigma; /* candidates, horizon, I, 1: refit sigma too (0: classic MPPI) */
    float temperature;     /* lambda > 0 */
    float alpha;           /* smoothing, as mbrl_cem_params.alpha */
    float lo, hi;          /* action bounds */
    float init_mu;         /* used when init_mu_rows == NULL */
    float init_sigma;
    uint64_t seed;
} mbrl_mppi_params;

int mbrl_abi_version(void);
/* "src=<16 hex digits> arch=gfx950": the sha256 prefix of the sources the library was built from
 * (mujoco-mbrl_amd/Makefile DIGEST_FILES), so a caller can check a prebuilt library against a tree. */
const char* mbrl_build_info(void);
const char* mbrl_last_error(void);

/* ---- process-wide switches for A/B runs and for tests that force a fallback. Every option starts
 * at 0 (automatic choice); the library never reads them from the environment, so a production launch
 * cannot be redirected by a stray variable. mbrl_set_option returns the previous value, or
 * MBRL_EINVAL for an unknown option or value. Not part of any reference interface. */
enum {
    MBRL_OPT_ROLLOUT_TILE = 0,      /* fp32 rollout candidates per workgroup: 0 auto, 4, 8, 16 (16 R) */
    MBRL_OPT_SPLIT_TILE = 1,        /* F16X3 / F16X6 rollout candidates per workgroup: 0 auto, 16, 32 */
    MBRL_OPT_DEBUG_TRAJ_ABORT = 2,  /* 1: the cooperative trajectory kernel gives up at once          */
    MBRL_OPT_GD_SINGLE = 3,         /* 1: mbrl_gd_plan runs its one-workgroup kernel                  */
    MBRL_OPT_DEBUG_GD_ABORT = 4,    /* 1: the cooperative gd kernel gives up at once                  */
    MBRL_OPT_UNFUSED_UPDATE = 5,    /* 1: plans run select / refit / proposal draw as separate launches */
    MBRL_OPT_ADAM_ARITH = 6,        /* mbrl_adam_step contraction pattern: 0 = torch's; 1 + bits (test) */
    MBRL_OPT_XCD_MAP = 7,           /* 1: ensemble rollouts map workgroups member-major per XCD (A/B) */
    MBRL_OPT_TRAIN_TILE = 8,        /* training backward C tile height: 0 auto, 32, 64 (bit-identical) */
    MBRL_OPT_TRAIN_NO_FOLD = 9,     /* 1: the layer-0 weight gradient in its own launch (bit-identical) */
    MBRL_OPT_ROLLOUT_PAIR = 10,     /* column-split pairs in plans: 0 auto, 1 forced (MBRL_EUNSUPPORTED where
                                       they cannot run), 2 never; standalone rollouts never use them  */
    MBRL_OPT_SHARD_EMULATE = 11,    /* 1 (tests): mbrl_cem_plan_sharded with comm == NULL computes every
                                       other rank's shard itself in place of the all-gather (G > 1 on one GPU)
                                       and keeps each iteration's gathered costs in the workspace; 2 (timing,
                                       ABI v13): the other ranks' slots are copied from those kept costs (one
                                       launch per iteration), so the call runs exactly one rank's work: its
                                       shard's rollout, the update over all N, its own draw, the trajectory.
                                       Mode 2 is bit-identical to mode 1 after a mode-1 plan of the same
                                       problem, seed and N (any rank id); set the option before the
                                       workspace query (the kept costs live in the workspace) */
    MBRL_OPT_DEBUG_PAIR_ABORT = 12, /* 1: the column-split pair kernel gives up at once (its redo runs);
                                       2: no redo launch behind it (tests of the pair kernel's own results) */
    MBRL_OPT_TRAJ_HOP = 13,         /* cooperative trajectory hand-offs: 0 auto, 1 (P, E) grid + sc1 granules,
                                       2 per-member XCD grid + sc1, 3 XCD grid + L2-resident granules when
                                       the roll call finds the member on one XCD (A/B; same results) */
    MBRL_OPT_GD_HOP = 14,           /* the cooperative gd kernel's hand-offs, as MBRL_OPT_TRAJ_HOP             */
    MBRL_OPT_PAIR_L2 = 15,          /* column-split pair hand-offs: 0 / 1 L2-resident when both halves share an
                                       XCD (roll call), 2 always written through (A/B; same results)     */
    MBRL_OPT_TRAIN_XCD = 16,        /* training launches: 1 row bands in XCD order (A/B; same bits)           */
    MBRL_OPT_TRAIN_SPLIT = 17,      /* 1: two-hidden-layer training in the five-launch layout instead of the
                                       fused three-launch step (A/B, tests; same bits)                    */
    MBRL_OPT_DEBUG_SHARD_FAIL = 18, /* i + 1 (tests): mbrl_cem_plan_sharded reports a failed launch at
                                       iteration i on the rank MBRL_OPT_DEBUG_SHARD_FAIL_RANK names (the rank
                                       then keeps joining the all-gathers); 0 off */
    MBRL_OPT_TRAIN_FO = 19,         /* 1: the fused training step's F and O as two launches (A/B; same bits) */
    MBRL_OPT_DEBUG_SHARD_FAIL_RANK = 20, /* (tests, ABI v13) r + 1: the injected failure is rank r's only (the
                                       other ranks see it as a peer failure; under MBRL_OPT_SHARD_EMULATE a
                                       call with another rank id fails that rank's emulated slot); 0: the
                                       calling rank's, whatever its id */
    MBRL_OPT_UPDATE_SPLIT = 21,     /* (ABI v13) plans' per-iteration update as two launches that share out the
                                       elites' regeneration (select + regenerate, then refit + draw): 0 auto
                                       (K ceil(a/4) >= 2048 Philox blocks per row), 1 never, 2 always (A/B,
                                       tests; same bits) */
    MBRL_OPT_COUNT = 22,            /* the options of v13's first table (tests/test_abi.py pins it) */
    /* added within v13, additively, as the MPPI calls were: ids go on from MBRL_OPT_COUNT */
    MBRL_OPT_ROLLOUT_GROUP_SEAM = 22, /* the 8-wave ring fp32 rollout's hidden-layer hand-offs per half group of
                                       four waves (two LDS counters) instead of a workgroup barrier: 0 auto
                                       (on where measured faster: W = 512 with s + a <= 32 and s <= 32,
                                       DESIGN.md §3.1), 1 on wherever the instance has it (8 waves, W <= 512),
                                       2 off (A/B, tests; same bits) */
    MBRL_OPT_END = 23               /* one past the last option id */
};
int mbrl_set_option(int32_t option, int32_t value);
int mbrl_get_option(int32_t option);

/* ---- multi-GPU (the reference has no distributed code): an RCCL communicator the
 * library owns. mbrl_comm_unique_id on one rank, the MBRL_COMM_ID_BYTES broadcast to the others by the
 * caller (torch.distributed), then mbrl_comm_init on every rank at once (collective), with the rank's
 * GPU current. RCCL (librccl.so.1) is opened on the first of these calls, not at load time: without it
 * they return MBRL_EUNSUPPORTED and everything else works. */
#define MBRL_COMM_ID_BYTES 128
typedef void* mbrl_comm_t;
int mbrl_comm_unique_id(void* id_out);
int mbrl_comm_init(const void* id, int32_t nranks, int32_t rank, mbrl_comm_t* comm_out);
int mbrl_comm_destroy(mbrl_comm_t comm);

/* ---- host staging: mapped, coherent pinned host memory (hipHostMalloc Mapped | Coherent) that the
 * kernels read and write directly. plan() (planners.py:14-25) takes its initial state from the host and
 * returns host tensors; passing mbrl_cem_plan a staged s0 and staged outputs replaces the two
 * host<->device copies around the plan with the plan's own first and last launches. *device_ptr is
 * the address kernels use (the same as *host_ptr under unified addressing). */
int mbrl_host_alloc(size_t bytes, void** host_ptr, void** device_ptr);
int mbrl_host_free(void* host_ptr);

/* ---- stream plumbing (no reference counterpart; ABI v12): events for ordering work between streams
 * and for the host to wait on, created without timing and without the system-scope fence a default
 * event's record ends in (which idles the GPU ~5.5 us per record). train_model's epoch loop orders its
 * row-order copies with them (mbrl_amd/models.py _OrderRing). A never-recorded event is complete. */
int mbrl_event_create(mbrl_event_t* event);
int mbrl_event_record(mbrl_event_t event, mbrl_stream_t stream);
int mbrl_stream_wait_event(mbrl_stream_t stream, mbrl_event_t event);
int mbrl_event_synchronize(mbrl_event_t event);
int mbrl_event_destroy(mbrl_event_t event);

/* ---- model upload: replaces the per-call nn.Linear weight reads of Model._forward (models.py:106-110) */
size_t mbrl_mlp_packed_bytes(const mbrl_mlp_shape* shape);
/* weights[e*NL+l] / biases[...], NL = L + 1 + reward_head: DEVICE pointers to nn.Linear weight
 * [out][in] and bias [out] (trunk layers, the state head, then the reward head), passed in a HOST
 * array. Writes the fragment-ordered weight stream the rollout kernel reads. */
int mbrl_mlp_pack(const mbrl_mlp_shape* shape, const float* const* weights, const float* const* biases,
                  void* packed, mbrl_stream_t stream);

/* ---- rollout + cost: replaces RandomShootingPlanner._generate_trajectories' model/cost loop
 * (planners.py:199-210) and DynamicsModel.forward (models.py:13-29) on its batch.
 * s0: [s] broadcast to every candidate (planners.py:204) or [N][s] when s0_per_candidate.
 * actions: [H][N][a] time-major (planners.py:200,207), or NULL to draw them from `sampler` into
 *          actions_out first (actions_out is then required).
 * costs: [E][N] per-member return sum_t cost(s_{t+1}, a_t), summed sequentially in t.
 * actions_out: [H][N][a] or NULL. states_out: [E][H][N][s] or NULL.
 * n_offset: global index of local candidate 0 (rank shard offset; keys the RNG).
 * W <= 1024, a <= 48 and L <= 4 are necessary, not sufficient: a 16-candidate workgroup must also fit
 * 160 KiB (163,840 B) of LDS, else MBRL_EUNSUPPORTED "LDS footprint ... B exceeds 160 KiB", returned
 * before the proposal draw or any other launch (the whole-plan entries may already have launched their
 * initialisation kernel). With Wp = W rounded up to 64, 128, 256, 512 or 1024, lda = max(Wp,
 * 32 ceil((s + a) / 32)) + 4 and po = 32 ceil((s + reward_head) / 32) the bytes are about
 *   4 (32 lda + 128 (po + 4) + 16 s + 32 a + L Wp + po + 4 s + 2 a + 16),
 * (64 (po + 4) in place of 128 (po + 4) for W <= 64), less the 128 (po + 4) term when L is 3, there is no reward head and 8 (po + 4) <= lda (the output
 * partials then share an activation buffer). So W = 1024 runs s = 17, a = 6 with L <= 3 (160,640 B at
 * L = 2) but not L = 4 (168,832 B), and s = 67, a = 21 only with L = 3. */
int mbrl_rollout_cost(const mbrl_mlp_shape* shape, const void* packed, const mbrl_norm* norm,
                      const mbrl_cost* cost, const float* s0, int32_t s0_per_candidate,
                      const float* actions, const mbrl_sampler* sampler, int32_t N, int32_t H,
                      int32_t n_offset, float* costs, float* actions_out, float* states_out,
                      mbrl_stream_t stream);

/* ---- selection: replaces np.argmin (planners.py:184) and adds CEM's stable top-K.
 * returns[n] = (sum_e costs[e][n]) / E (sequential in e; = costs[0][n] when E == 1).
 * elite_idx[0..K): the K smallest (return, index) pairs, written in ASCENDING candidate index.
 * returns_out: [N] or NULL. workspace: >= mbrl_select_workspace_bytes(N). */
size_t mbrl_select_workspace_bytes(int32_t N);
int mbrl_select_elites(const float* costs, int32_t E, int32_t N, int32_t K, int32_t nan_policy,
                       int64_t* elite_idx, float* returns_out, void* workspace, size_t ws_bytes,
                       mbrl_stream_t stream);

/* ---- CEM refit (not in the reference). Regenerates each elite's actions from
 * the counter RNG (so every rank can refit from the global elite list with no moment collective),
 * sums them in the canonical chunked order, writes mu' / sigma' ([H][a]).
 * Multi-GPU split step: SURVEY.md §8b proposed an mbrl_topk_moments (local elite moments, then an
 * all-gather of [G][2][H][a]). Here every rank runs mbrl_select_elites on the all-gathered
 * returns and mbrl_cem_refit on the global elite list: one collective per iteration instead of
 * two, and the result does not depend on the GPU count. */
size_t mbrl_refit_workspace_bytes(int32_t H, int32_t a, int32_t K);
int mbrl_cem_refit(const mbrl_sampler* sampler, int32_t H, int32_t a, const int64_t* elite_idx,
                   int32_t K, float alpha, float* mu_out, float* sigma_out, void* workspace,
                   size_t ws_bytes, mbrl_stream_t stream);

/* ---- proposal draw only (generic-callable path and RNG parity): actions_out [H][N][a]. */
int mbrl_sample_actions(const mbrl_sampler* sampler, int32_t H, int32_t a, int32_t N, int32_t n_offset,
                        float* actions_out, mbrl_stream_t stream);

/* ---- one trajectory per ensemble member: the states of a single action sequence (the final CEM
 * mean; replaces the N=1 use of planners.py:199-210). actions [H][a]; states_out [H][s] = member
 * mean; member_states_out [E][H][s] or NULL. workspace >= mbrl_trajectory_workspace_bytes. */
size_t mbrl_trajectory_workspace_bytes(const mbrl_mlp_shape* shape, int32_t H);
int mbrl_trajectory(const mbrl_mlp_shape* shape, const void* packed, const mbrl_norm* norm, const float* s0,
                    const float* actions, int32_t H, float* states_out, float* member_states_out,
                    void* workspace, size_t ws_bytes, mbrl_stream_t stream);

/* ---- whole single-GPU CEM plan: I x (rollout -> select -> refit), then the final mean's rollout.
 * mu / sigma: [H][a] final distribution. actions_out: [H][a] = clip(mu, lo, hi);
 * states_out: [H][s] rollout of actions_out (ensemble mean over members).
 * cost_hist [I][E][N], returns_hist [I][N], elite_hist [I][K]: optional per-iteration records (NULL = off).
 * rollout_events: NULL or 2*I events; pair i brackets iteration i's rollout launch on `stream`
 * (a NULL pair skips iteration i: each record leaves the GPU idle a few microseconds).
 * s0 [s] is read once, by the plan's first launch (into the workspace), and mu / sigma / actions_out /
 * states_out are written by its last launches only: all five may be device memory or mapped host
 * memory from mbrl_host_alloc (ABI v7; plan() on host tensors with no copy launch around it). */
size_t mbrl_cem_workspace_bytes(const mbrl_mlp_shape* shape, const mbrl_cem_params* params);
int mbrl_cem_plan(const mbrl_mlp_shape* shape, const void* packed, const mbrl_norm* norm,
                  const mbrl_cost* cost, const float* s0, const mbrl_cem_params* params,
                  float* mu, float* sigma, float* actions_out, float* states_out,
                  float* cost_hist, float* returns_hist, int64_t* elite_hist,
                  mbrl_event_t* rollout_events, void* workspace, size_t ws_bytes,
                  mbrl_stream_t stream);

/* ---- the same plan sharded over `nranks` GPUs, one call per rank: rank r rolls out global candidates
 * [r N / nranks, (r + 1) N / nranks) (proposals keyed by the global index), every iteration all-gathers
 * the [E][N / nranks] costs over `comm` as a step on `stream` (ncclAllGather), then every rank runs the
 * same selection over all N, the same refit and draws its own shard of the next proposals. Outputs are
 * bit-identical on every rank and to mbrl_cem_plan's for any nranks (records as mbrl_cem_plan's, over
 * all N). Replaces planners.cem_sharded_protocol's per-iteration Python loop. N % nranks == 0.
 * Every argument check runs before the first collective (the ranks pass the same shape, params and
 * nranks, so they agree on it). A launch that fails later does not end the call early: the rank skips
 * its remaining compute launches but still joins every remaining all-gather (its local costs poisoned
 * to NaN), so no peer waits on it and `comm` stays usable, and returns its own error at the end.
 * Failure is visible on every rank (ABI v13): the last iteration's all-gather also gathers one status
 * word per rank (grouped with the costs in one RCCL call), and a rank whose status word is set makes
 * every other rank return MBRL_EPEER instead of a plan over N - N / nranks candidates. With nranks > 1
 * the call therefore returns after the plan has completed on `stream` (one stream synchronisation, at
 * its end); with nranks == 1 it only enqueues, as mbrl_cem_plan.
 * comm == NULL is allowed only under MBRL_OPT_SHARD_EMULATE (tests, timing): each call then fills the
 * all-gather's rank-major buffer itself (mode 1: rolls out every rank's shard; mode 2: copies the other
 * ranks' costs kept by an earlier mode-1 plan), so one GPU runs any nranks. */
size_t mbrl_cem_plan_sharded_workspace_bytes(const mbrl_mlp_shape* shape, const mbrl_cem_params* params,
                                             int32_t nranks);
int mbrl_cem_plan_sharded(const mbrl_mlp_shape* shape, const void* packed, const mbrl_norm* norm,
                          const mbrl_cost* cost, const float* s0, const mbrl_cem_params* params, mbrl_comm_t comm,
                          int32_t nranks, int32_t rank, float* mu, float* sigma, float* actions_out,
                          float* states_out, float* cost_hist, float* returns_hist, int64_t* elite_hist,
                          mbrl_event_t* rollout_events, void* workspace, size_t ws_bytes, mbrl_stream_t stream);

/* ---- batched planning: B independent CEM plans, one per initial state s0[b] (parallel environments
 * feeding one GPU planner), in shared launches: one proposal draw, one rollout
 * of B*N candidates, one segmented selection, one batched refit per iteration. Problem b's candidate
 * n is global candidate b*N + n for the proposal RNG, so problem b's plan equals a single-problem
 * plan whose candidates are drawn with n_offset = b*N. params->N, ->K are PER problem.
 * s0: [B][s]; mu / sigma (optional): [B][H][a]; actions_out: [B][H][a] = clip(mu);
 * states_out: [B][H][s] (member mean). */
size_t mbrl_cem_plan_batch_workspace_bytes(const mbrl_mlp_shape* shape, const mbrl_cem_params* params, int32_t B);
int mbrl_cem_plan_batch(const mbrl_mlp_shape* shape, const void* packed, const mbrl_norm* norm,
                        const mbrl_cost* cost, const float* s0, int32_t B, const mbrl_cem_params* params,
                        float* mu, float* sigma, float* actions_out, float* states_out, void* workspace,
                        size_t ws_bytes, mbrl_stream_t stream);

/* ---- one CEM iteration's update after the rollout, as ONE launch (cem_update_kernel): the stable
 * top-K of the member-mean returns (as mbrl_select_elites, NAN_LAST), the refit of every row (as
 * mbrl_cem_refit) and, with next_actions, iteration sampler->iteration + 1's proposals for global
 * candidates [draw_offset, draw_offset + draw_count) drawn from the new mu / sigma (as
 * mbrl_sample_actions with n_offset = draw_offset). Bit-identical to those three calls; used by the
 * sharded (multi-GPU) plan, where every rank updates on the all-gathered costs and draws its shard.
 * costs: [E][N]; elite_idx: [K] or NULL; returns_out: [N] or NULL; mu_out / sigma_out: [H][a];
 * next_actions: [H][draw_count][a] or NULL. MBRL_EUNSUPPORTED when N > 32768 or the selection /
 * refit working set exceeds LDS: use the three calls. Not part of any reference interface. */
int mbrl_cem_update(const float* costs, int32_t E, int32_t N, int32_t K, const mbrl_sampler* sampler, int32_t H,
                    int32_t a, float alpha, int64_t* elite_idx, float* returns_out, float* mu_out, float* sigma_out,
                    float* next_actions, int32_t draw_offset, int32_t draw_count, mbrl_stream_t stream);

/* ---- MPPI (model-predictive path integral control, the information-theoretic update; not in the
 * reference; added within ABI v13). Where CEM refits on a hard top-K, MPPI weights EVERY candidate:
 *   r_n  = member-mean return (as mbrl_select_elites forms it); valid iff finite
 *   beta = min over valid r_n (a zero of either sign counts as +0.0)
 *   w_n  = expf(-((r_n - beta) / temperature)) for valid n, else 0;   eta = sum_n w_n  (>= 1)
 *   m[t][d] = sum_n (w_n a[t][n][d]) / eta;   with update_sigma: v[t][d] = sum_n w_n (a[t][n][d] - m[t][d])^2 / eta
 *   mu' = alpha mu + (1 - alpha) m;   sigma' = sqrt(alpha sigma^2 + (1 - alpha) v) (correctly rounded), or
 *   sigma' = sigma without update_sigma (classic MPPI). No valid candidate: mu' = mu, sigma' = sigma, bit for bit.
 * Every sum over n runs in one fixed order that depends on N alone (DESIGN.md "MPPI"): chunks of 32
 * consecutive candidates summed sequentially, the chunk partials again in groups of 32, then the
 * group partials; at most 93 dependent additions. fp32, round to nearest, no contraction.
 *
 * mbrl_mppi_update: one iteration's update as ONE launch (mppi_update_kernel), no workspace.
 * costs: [E][N]; actions: [H][N][a], the proposals the rollout consumed; sampler: this iteration's mu,
 * sigma, lo, hi, seed, iteration; mu_out / sigma_out: [H][a] (not the sampler's buffers).
 * Optional (NULL = off): weights_out [N]; returns_out [N]; stats_out [2] = (beta, eta), (NaN, 0) when no
 * candidate is valid; next_actions [H][draw_count][a]: iteration sampler->iteration + 1's proposals for
 * candidates [draw_offset, draw_offset + draw_count) drawn from mu_out / sigma_out, bit-identical to
 * mbrl_sample_actions with n_offset = draw_offset (a buffer other than `actions`, which the launch is
 * still reading). MBRL_EUNSUPPORTED when N > 32768 or a > 64; MBRL_EINVAL for NULL arguments, sizes
 * < 1, a temperature that is not finite and > 0, or a draw range outside [0, N) -- all before any launch. */
int mbrl_mppi_update(const float* costs, int32_t E, int32_t N, const float* actions, const mbrl_sampler* sampler,
                     int32_t H, int32_t a, float temperature, float alpha, int32_t update_sigma, float* mu_out,
                     float* sigma_out, float* weights_out, float* returns_out, float* stats_out, float* next_actions,
                     int32_t draw_offset, int32_t draw_count, mbrl_stream_t stream);

/* ---- whole single-GPU MPPI plan, the analogue of mbrl_cem_plan: I x (rollout -> mbrl_mppi_update), then
 * the final mean's trajectory (member mean). Proposals are drawn exactly as CEM's (the same counter
 * space: a plan is one or the other).
 * init_mu_rows: [H][a] device, or NULL. The warm start: row t of the initial mean is init_mu_rows[t]
 * clipped to [lo, hi] instead of params->init_mu (e.g. the previous plan shifted by one step).
 * mu / sigma (optional), actions_out = clip(mu, lo, hi), states_out: as mbrl_cem_plan; they and s0 may be
 * mapped host memory from mbrl_host_alloc.
 * Optional records (NULL = off): cost_hist [I][E][N]; weight_hist [I][N]; mu_hist / sigma_hist
 * [I + 1][H][a], row 0 the initial distribution and row i + 1 the result of iteration i; rollout_events
 * as mbrl_cem_plan's. mbrl_mppi_workspace_bytes returns 0 for a bad shape or bad params.
 * MBRL_EINVAL before any launch for NULL pointers, N / H / iterations < 1, a temperature that is not
 * finite and > 0, or a workspace that is too small; MBRL_EUNSUPPORTED for N > 32768. */
size_t mbrl_mppi_workspace_bytes(const mbrl_mlp_shape* shape, const mbrl_mppi_params* params);
int mbrl_mppi_plan(const mbrl_mlp_shape* shape, const void* packed, const mbrl_norm* norm, const mbrl_cost* cost,
                   const float* s0, const mbrl_mppi_params* params, const float* init_mu_rows, float* mu,
                   float* sigma, float* actions_out, float* states_out, float* cost_hist, float* weight_hist,
                   float* mu_hist, float* sigma_hist, mbrl_event_t* rollout_events, void* workspace,
                   size_t ws_bytes, mbrl_stream_t stream);

/* ---- batched MPPI (added within ABI v13, additively: no existing entry, struct or option changes).
 * mbrl_mppi_update_batch: mbrl_mppi_update for B problems as ONE launch (grid (H S, B)), no workspace.
 * Problem b's costs are columns [b N, (b + 1) N) of costs [E][B N], its proposals columns b N + n of actions
 * [H][B N][a]; the sampler's mu / sigma and mu_out / sigma_out are [B][H][a]. Each problem forms its own
 * returns, beta, weights and eta over its own N, in mbrl_mppi_update's summation order counted from its
 * candidate 0: every output of problem b equals mbrl_mppi_update on contiguous copies of its slices, bit for
 * bit (a problem without a finite return keeps its distribution while its neighbours update).
 * Optional (NULL = off): weights_out [B][N]; returns_out [B][N]; stats_out [B][2]; next_actions [H][B N][a]
 * (not `actions`): iteration sampler->iteration + 1's proposals of every problem, column b N + n drawn from
 * mu_out[b] / sigma_out[b] with Philox index b N + n, bit-identical to mbrl_sample_actions with n_offset = b N.
 * Before any launch: mbrl_mppi_update's checks; B < 1: MBRL_EINVAL; B > 65535 or B N beyond
 * mbrl_cem_plan_batch's bound: MBRL_EUNSUPPORTED. */
int mbrl_mppi_update_batch(const float* costs, int32_t E, int32_t N, int32_t B, const float* actions,
                           const mbrl_sampler* sampler, int32_t H, int32_t a, float temperature, float alpha,
                           int32_t update_sigma, float* mu_out, float* sigma_out, float* weights_out,
                           float* returns_out, float* stats_out, float* next_actions, mbrl_stream_t stream);

/* mbrl_mppi_plan_batch: B independent mbrl_mppi_plan plans (one initial state each, s0 [B][s] device) in
 * shared launches; params->N is per problem. One first launch (the distributions, the start states expanded
 * to one per candidate, iteration 0's proposals where the update draws them), then per iteration ONE rollout
 * over the B N candidates and ONE mbrl_mppi_update_batch launch, then each problem's final trajectory, one
 * launch each as in mbrl_cem_plan_batch.
 * Warm start: init_mu_rows [B][H][a] device or NULL; input_flags [B] int32 device or NULL. Bit 0 of
 * input_flags[b] set: problem b's initial mean is its rows clipped to [lo, hi]; clear: params->init_mu (its
 * first control step). NULL flags: every problem takes its rows; a set bit with NULL rows is ignored (as
 * mbrl_cem_plan_rh_batch, so one batch mixes first-step and mid-episode problems).
 * mu, sigma (optional), actions_out = clip(mu, lo, hi): [B][H][a]; states_out [B][H][s] (member mean); device.
 * Optional records (NULL = off): cost_hist [I][E][B N]; weight_hist [I][B][N]; mu_hist / sigma_hist
 * [I + 1][B][H][a], row 0 the initial distributions.
 * Problem 0 of any batch, and all of a B = 1 batch, is mbrl_mppi_plan bit for bit (outputs and records);
 * problem b is the same plan with Philox candidate index b N + n.
 * mbrl_mppi_batch_workspace_bytes returns 0 for a bad shape, bad params or B < 1; its answer never shrinks as B
 * grows and is never below mbrl_mppi_workspace_bytes (for B = 1 it also serves mbrl_mppi_plan). Before any launch: NULL packed / s0 / actions_out / states_out / workspace, B < 1
 * or bad params: MBRL_EINVAL; N > 32768, B > 65535 or B N beyond mbrl_cem_plan_batch's bound:
 * MBRL_EUNSUPPORTED; a workspace that is too small: MBRL_EWORKSPACE. */
size_t mbrl_mppi_batch_workspace_bytes(const mbrl_mlp_shape* shape, const mbrl_mppi_params* params, int32_t B);
int mbrl_mppi_plan_batch(const mbrl_mlp_shape* shape, const void* packed, const mbrl_norm* norm, const mbrl_cost* cost,
                         const float* s0, int32_t B, const mbrl_mppi_params* params, const float* init_mu_rows,
                         const int32_t* input_flags, float* mu, float* sigma, float* actions_out, float* states_out,
                         float* cost_hist, float* weight_hist, float* mu_hist, float* sigma_hist, void* workspace,
                         size_t ws_bytes, mbrl_stream_t stream);

/* ---- MPPI over the K best (the TD-MPC-style update: elite-restricted weights and a sigma clamp; not in the
 * reference; added within ABI v13, additively: no existing entry, struct or option changes, no new option id).
 * One iteration's update with K in [1, N] and 0 <= sigma_min <= sigma_max (+inf allowed):
 *   r_n   = member-mean return, exactly as mbrl_select_elites / mbrl_mppi_update form it;
 *   elite = the K smallest (r_n, n) pairs under MBRL_NAN_LAST -- what mbrl_select_elites returns: a stable
 *           order, so a tie at the boundary goes to the lower index;
 *   n is valid iff it is an elite AND r_n is finite (with fewer than K finite returns the selection holds NaN
 *           or inf rows; those stay invalid. -inf sorts first: it can fill the elite set with invalid rows);
 *   beta, x_n, w_n = expf(-x_n) as mbrl_mppi_update for valid n; w_n = 0 for every other n;
 *   eta, m, v are summed over ALL N candidates in mbrl_mppi_update's canonical 32-chunk order, the zero weights
 *           taking part as zeros: the order still depends on N alone;
 *   mu' as mbrl_mppi_update; with update_sigma
 *           sigma' = min(max(sqrt(alpha sigma^2 + (1 - alpha) v), sigma_min), sigma_max)
 *           (sigma_min = 0, sigma_max = +inf change no bit); without it sigma is copied unclamped (classic MPPI);
 *   no valid candidate: mu and sigma are copied bit for bit.
 * So K = N with the neutral clamp is mbrl_mppi_update byte for byte (every output), and K = 1 with alpha = 0
 * gives mu'[t][d] == the best candidate's proposal row. A large temperature with K < N is CEM's elite mean.
 *
 * mbrl_mppi_update_elite: TWO launches -- the selection (mbrl_select_elites' kernel), then the update kernel,
 * which builds an N-bit membership map from the list and zeroes every non-member's weight (csrc/mppi.hip).
 * Arguments as mbrl_mppi_update, plus K, the clamp, and
 *   elite_idx_out [K] int64 or NULL: the elite set in ascending candidate index (as mbrl_select_elites);
 *   weights_out [N]: 0 for non-elites; returns_out [N]: the true returns of all N; stats_out [2] = (beta, eta);
 *   workspace >= mbrl_select_workspace_bytes(N); with elite_idx_out == NULL the list lives behind it:
 *   8 K bytes rounded up to 256 more.
 * Before any launch: mbrl_mppi_update's checks; NULL workspace, K outside [1, N], sigma_min < 0,
 * sigma_max < sigma_min or a NaN clamp: MBRL_EINVAL; a workspace that is too small: MBRL_EWORKSPACE. */
int mbrl_mppi_update_elite(const float* costs, int32_t E, int32_t N, int32_t K, const float* actions,
                           const mbrl_sampler* sampler, int32_t H, int32_t a, float temperature, float alpha,
                           int32_t update_sigma, float sigma_min, float sigma_max, float* mu_out, float* sigma_out,
                           int64_t* elite_idx_out, float* weights_out, float* returns_out, float* stats_out,
                           float* next_actions, int32_t draw_offset, int32_t draw_count, void* workspace,
                           size_t ws_bytes, mbrl_stream_t stream);

/* mbrl_mppi_update_elite_batch: the same for B problems, laid out as mbrl_mppi_update_batch's; elite_idx_out
 * [B][K] (indices local to the problem) or NULL. Two launches whatever B is: the segmented selection, then the
 * update over grid (H S, B). Problem b equals mbrl_mppi_update_elite on contiguous copies of its slices, bit for
 * bit. workspace >= mbrl_select_workspace_bytes(B N), plus 8 B K bytes rounded up to 256 without elite_idx_out.
 * Checks: the two siblings'; a workspace that is too small: MBRL_EWORKSPACE. */
int mbrl_mppi_update_elite_batch(const float* costs, int32_t E, int32_t N, int32_t K, int32_t B, const float* actions,
                                 const mbrl_sampler* sampler, int32_t H, int32_t a, float temperature, float alpha,
                                 int32_t update_sigma, float sigma_min, float sigma_max, float* mu_out,
                                 float* sigma_out, int64_t* elite_idx_out, float* weights_out, float* returns_out,
                                 float* stats_out, float* next_actions, void* workspace, size_t ws_bytes,
                                 mbrl_stream_t stream);

/* The plans: mbrl_mppi_plan / mbrl_mppi_plan_batch with each iteration as rollout -> selection -> restricted
 * update (the next proposals' draw stays fused in the update launch wherever the classic plan fuses it; no
 * launch inside the loop is per problem), and two more inputs:
 *   init_sigma_rows [H][a] ([B][H][a]) device or NULL: row t of the initial std instead of params->mppi.init_sigma
 *     -- the previous plan's sigma carried to the next control step, which the clamp makes safe. Every entry
 *     finite and > 0: the CALLER'S check, as for mbrl_cem_plan_rh (Python makes it on the host). In the batch,
 *     bit 1 of input_flags[b] governs them as in mbrl_cem_plan_rh_batch (bit 0: init_mu_rows);
 *   elite_hist [I][K] ([I][B][K], local indices) int64 or NULL: each iteration's elite set.
 * Everything else -- outputs, records, mapped host memory for the single plan, the Philox counter space -- is the
 * sibling's. Problem 0 of a batch and a B = 1 batch are mbrl_mppi_plan_elite bit for bit.
 * mbrl_mppi_elite_workspace_bytes(shape, params, B) sizes both plans (B = 1: the single plan and a batch of one):
 * 0 for a bad shape, bad params (K and the clamp included) or B < 1; it never shrinks as B grows and is never
 * below mbrl_mppi_batch_workspace_bytes(shape, &params->mppi, B).
 * Before any launch: the siblings' checks and codes (a small workspace: MBRL_EINVAL from the single plan,
 * MBRL_EWORKSPACE from the batch), K outside [1, N], sigma_min < 0, sigma_max < sigma_min, a NaN clamp: MBRL_EINVAL. */
typedef struct {
    mbrl_mppi_params mppi;
    int32_t K;             /* elites, 1 .. N */
    int32_t _pad;
    float sigma_min, sigma_max; /* clamp on sigma' (update_sigma only): 0 <= sigma_min <= sigma_max, +inf allowed */
} mbrl_mppi_elite_params;
size_t mbrl_mppi_elite_workspace_bytes(const mbrl_mlp_shape* shape, const mbrl_mppi_elite_params* params, int32_t B);
int mbrl_mppi_plan_elite(const mbrl_mlp_shape* shape, const void* packed, const mbrl_norm* norm, const mbrl_cost* cost,
                         const float* s0, const mbrl_mppi_elite_params* params, const float* init_mu_rows,
                         const float* init_sigma_rows, float* mu, float* sigma, float* actions_out, float* states_out,
                         float* cost_hist, float* weight_hist, float* mu_hist, float* sigma_hist, int64_t* elite_hist,
                         mbrl_event_t* rollout_events, void* workspace, size_t ws_bytes, mbrl_stream_t stream);
int mbrl_mppi_plan_elite_batch(const mbrl_mlp_shape* shape, const void* packed, const mbrl_norm* norm,
                               const mbrl_cost* cost, const float* s0, int32_t B, const mbrl_mppi_elite_params* params,
                               const float* init_mu_rows, const float* init_sigma_rows, const int32_t* input_flags,
                               float* mu, float* sigma, float* actions_out, float* states_out, float* cost_hist,
                               float* weight_hist, float* mu_hist, float* sigma_hist, int64_t* elite_hist,
                               void* workspace, size_t ws_bytes, mbrl_stream_t stream);

/* ---- receding-horizon CEM plan (warm start and elite carry-over, the two iCEM ingredients of Pinneri
 * et al. 2020; not in the reference; added within ABI v13, additively, as the MPPI calls were).
 * mbrl_cem_plan with three more inputs and a `keep` count Kc (0 <= Kc <= K):
 *   init_mu_rows    [H][a] device or NULL: row t of the initial mean is init_mu_rows[t] clipped to [lo, hi]
 *                   instead of params->cem.init_mu (e.g. the previous plan shifted by one step);
 *   init_sigma_rows [H][a] device or NULL: row t of the initial std instead of params->cem.init_sigma. Every
 *                   entry must be finite and > 0; the C call cannot read device rows, so this is the CALLER'S
 *                   check (the Python layer makes it on the host and raises before the call);
 *   carry_in        [Kc][H][a] device or NULL: the rows kept from the previous plan (its carry_out, shifted).
 * Proposals of iteration i: candidate n < Kc takes kept_i[n] clipped to [lo, hi] (a NaN entry stays NaN:
 * the row's return is then NaN and it sorts last) when a kept set exists -- kept_0 = carry_in where given,
 * and always from iteration 1 on; every other candidate is drawn exactly as mbrl_cem_plan draws it, from
 * Philox counter (n, t, i, d >> 2). The counter space does not move: a slot taken by a kept row skips its
 * draw, so candidates n >= Kc are bit-identical to the plain plan's from the same mu / sigma.
 * After iteration i's rollout the member-mean returns give two selections (both mbrl_select_elites,
 * NAN_LAST, ascending candidate index): the K elites, refitted exactly as mbrl_cem_refit does over their
 * action rows, and the Kc best, whose action rows become kept_{i+1}. A row's actions are read back from
 * kept_i where the slot was filled from it, else regenerated from the counter RNG.
 * Outputs: mu, sigma, actions_out, states_out and the records cost_hist, returns_hist, elite_hist as
 * mbrl_cem_plan's. Optional (NULL = off): carry_out [Kc][H][a] = kept_I, the action rows of the last
 * iteration's Kc best; carry_returns_out [Kc] their returns; kept_hist [I + 1][Kc][H][a], row i = kept_i
 * (row 0: carry_in as given, or zeros without one).
 * keep == 0 enqueues exactly mbrl_cem_plan's launches (the fused or split update, the pair rollouts); only
 * the first launch differs where rows are given. keep > 0 runs each iteration's update as five small
 * launches (two selections, the gather, the refit, the next proposals' scatter and draw).
 * Before any launch: MBRL_EINVAL for bad mbrl_cem_params, keep outside [0, K], carry_in with keep == 0,
 * NULL packed / s0 / actions_out / states_out / workspace or a workspace below
 * mbrl_cem_rh_workspace_bytes (which returns 0 for a bad shape or bad params); MBRL_EUNSUPPORTED for
 * N > 32768. Sharded receding-horizon plans do not exist; B plans at once: mbrl_cem_plan_rh_batch below. */
typedef struct {
    mbrl_cem_params cem;
    int32_t keep;  /* Kc */
    int32_t _pad;
} mbrl_cem_rh_params;
size_t mbrl_cem_rh_workspace_bytes(const mbrl_mlp_shape* shape, const mbrl_cem_rh_params* params);
int mbrl_cem_plan_rh(const mbrl_mlp_shape* shape, const void* packed, const mbrl_norm* norm, const mbrl_cost* cost,
                     const float* s0, const mbrl_cem_rh_params* params, const float* init_mu_rows,
                     const float* init_sigma_rows, const float* carry_in, float* mu, float* sigma,
                     float* actions_out, float* states_out, float* carry_out, float* carry_returns_out,
                     float* cost_hist, float* returns_hist, int64_t* elite_hist, float* kept_hist,
                     mbrl_event_t* rollout_events, void* workspace, size_t ws_bytes, mbrl_stream_t stream);

/* ---- batched receding-horizon CEM plan (added within ABI v13, additively): B independent mbrl_cem_plan_rh
 * plans, one per initial state s0[b], in shared launches -- what mbrl_cem_plan_batch is to mbrl_cem_plan, for
 * parallel environments that each carry their own warm start and kept rows from control step to control step.
 * Problem b is mbrl_cem_plan_rh's plan on s0[b] with its own rows and carry; the one difference is the Philox
 * candidate index, b*N + n, as in mbrl_cem_plan_batch. params->cem.N, K and keep are PER problem. Problem 0
 * of any batch, and all of a B == 1 batch, is mbrl_cem_plan_rh bit for bit (outputs, carry and records).
 *   s0 [B][s]; init_mu_rows / init_sigma_rows [B][H][a] device or NULL; carry_in [B][Kc][H][a] device or NULL;
 *   input_flags [B] int32 device or NULL: which of the given inputs apply to problem b -- bit 0 init_mu_rows,
 *   bit 1 init_sigma_rows, bit 2 carry_in. A clear bit: problem b plans as if that pointer were NULL (it uses
 *   params->cem.init_mu / init_sigma, has no kept set at iteration 0 -- all N slots drawn -- and its
 *   kept_hist row 0 is zeros), so one batch mixes problems at their first control step with problems mid-
 *   episode. NULL flags: every given pointer applies to every problem. A set bit whose pointer is NULL is
 *   ignored. Positive finite sigma rows remain the caller's check.
 * Kept slots, the NaN-stays-NaN clip, the two selections, the refit over the elites' rows, the read-back-or-
 * regenerate rule and the unmoved counter space are mbrl_cem_plan_rh's, per problem.
 * Outputs: mu, sigma (optional), actions_out [B][H][a]; states_out [B][H][s]; optional carry_out
 * [B][Kc][H][a], carry_returns_out [B][Kc]; optional records cost_hist [I][E][B*N], returns_hist [I][B][N],
 * elite_hist [I][B][K] (indices local to the problem), kept_hist [I + 1][B][Kc][H][a].
 * keep == 0 without rows enqueues exactly mbrl_cem_plan_batch's launches (bit-identical); with rows only the
 * first launch differs. keep > 0: each iteration is the one rollout over B*N candidates plus the single
 * plan's five small launches, each over all B problems (no per-problem launch inside the iteration loop; the
 * first launch also expands s0 to the per-candidate start states); the B final trajectories are one launch
 * each, as in mbrl_cem_plan_batch.
 * Before any launch: MBRL_EINVAL for B < 1, bad params, keep outside [0, K], carry_in with keep == 0, NULL
 * packed / s0 / actions_out / states_out / workspace; MBRL_EUNSUPPORTED for N > 32768, B*N beyond
 * mbrl_cem_plan_batch's bound, and with keep > 0 a K x a the staged refit cannot hold or B > 65535;
 * MBRL_EWORKSPACE for a workspace below mbrl_cem_rh_batch_workspace_bytes (which returns 0 for a bad shape,
 * bad params or B < 1). */
size_t mbrl_cem_rh_batch_workspace_bytes(const mbrl_mlp_shape* shape, const mbrl_cem_rh_params* params, int32_t B);
int mbrl_cem_plan_rh_batch(const mbrl_mlp_shape* shape, const void* packed, const mbrl_norm* norm,
                           const mbrl_cost* cost, const float* s0, int32_t B, const mbrl_cem_rh_params* params,
                           const float* init_mu_rows, const float* init_sigma_rows, const float* carry_in,
                           const int32_t* input_flags, float* mu, float* sigma, float* actions_out,
                           float* states_out, float* carry_out, float* carry_returns_out, float* cost_hist,
                           float* returns_hist, int64_t* elite_hist, float* kept_hist, void* workspace,
                           size_t ws_bytes, mbrl_stream_t stream);

/* ---- coloured-noise proposals (the third iCEM ingredient: proposal noise correlated along the horizon; not in
 * the reference; added within ABI v13, additively). A plan may be given a noise mix: noise_mix [H][H], fp32,
 * row-major, device. With z[u][n][d], u = 0 .. H-1, the white normals every plan draws (Philox counter
 * (n, u, i, d >> 2): the counter space does not move), the noise of step t is
 *   e[t][n][d] = (..((C[t][0] z[0]) + C[t][1] z[1]) + ..) + C[t][H-1] z[H-1]
 * -- every product rounded to fp32 before it is added, the additions sequential in u, round to nearest, no
 * contraction -- and the action is clip(mu[t][d] + sigma[t][d] e[t][n][d]) as before. The matrix is the
 * caller's: a power-law spectrum (Python: planners.colored_noise_mix), AR(1), action repeat. Rows of unit
 * Euclidean norm keep e[t] marginally N(0, 1), so sigma keeps its meaning; the identity is the white draw.
 * Every entry must be finite: the CALLER'S check, as for the sigma rows (Python makes it on the host).
 * H > 64 with a mix is MBRL_EUNSUPPORTED before any launch (the kernels hold the matrix and one tile's normals
 * in LDS; csrc/cem_noise.hip). A NULL mix is the entry without one: the same launches, the same bits.
 *
 * mbrl_sample_actions_mixed: mbrl_sample_actions with the mix (RNG parity, step-by-step equivalents).
 *
 * mbrl_cem_plan_rh_mixed / mbrl_cem_plan_rh_batch_mixed: mbrl_cem_plan_rh / mbrl_cem_plan_rh_batch with
 * noise_mix after carry_in / input_flags (one matrix serves all B problems). Every drawn row and every
 * regenerated row uses the formula above; kept slots n < Kc, the NaN-stays-NaN clip, the two selections, the
 * refit over the elites' rows and the read-back-or-regenerate rule are unchanged, per problem. With a mix the
 * plan runs the unfused update whatever keep is: the first launch (rh's, coloured), then per iteration the
 * rollout, the K selection, the Kc selection (only when Kc > 0), the coloured gather, the refit over the
 * staged elites and the coloured draw -- 5 or 6 launches per iteration whatever B is -- then the final
 * trajectories. The argument checks are the existing entries', before any launch, plus H > 64 and, also with
 * keep == 0, a K x a the staged refit cannot hold (MBRL_EUNSUPPORTED).
 * workspace >= mbrl_cem_rh_mixed_workspace_bytes(shape, params, B) (B = 1: the single plan, and a batch of
 * one): a mixed plan with keep == 0 still stages the elites and keeps the returns, which the existing
 * queries size for keep > 0 only (their values are unchanged). 0 for a bad shape, bad params, B < 1 or H > 64. */
int mbrl_sample_actions_mixed(const mbrl_sampler* sampler, const float* mix, int32_t H, int32_t a, int32_t N,
                              int32_t n_offset, float* actions_out, mbrl_stream_t stream);
size_t mbrl_cem_rh_mixed_workspace_bytes(const mbrl_mlp_shape* shape, const mbrl_cem_rh_params* params, int32_t B);
int mbrl_cem_plan_rh_mixed(const mbrl_mlp_shape* shape, const void* packed, const mbrl_norm* norm,
                           const mbrl_cost* cost, const float* s0, const mbrl_cem_rh_params* params,
                           const float* init_mu_rows, const float* init_sigma_rows, const float* carry_in,
                           const float* noise_mix, float* mu, float* sigma, float* actions_out, float* states_out,
                           float* carry_out, float* carry_returns_out, float* cost_hist, float* returns_hist,
                           int64_t* elite_hist, float* kept_hist, mbrl_event_t* rollout_events, void* workspace,
                           size_t ws_bytes, mbrl_stream_t stream);
int mbrl_cem_plan_rh_batch_mixed(const mbrl_mlp_shape* shape, const void* packed, const mbrl_norm* norm,
                                 const mbrl_cost* cost, const float* s0, int32_t B, const mbrl_cem_rh_params* params,
                                 const float* init_mu_rows, const float* init_sigma_rows, const float* carry_in,
                                 const int32_t* input_flags, const float* noise_mix, float* mu, float* sigma,
                                 float* actions_out, float* states_out, float* carry_out, float* carry_returns_out,
                                 float* cost_hist, float* returns_hist, int64_t* elite_hist, float* kept_hist,
                                 void* workspace, size_t ws_bytes, mbrl_stream_t stream);

/* ---- gradient-descent planner: replaces GradientDescentPlanner's
 * _optimize_trajectory (planners.py:103-137) -- Adam(lr) on the action sequence through the dynamics
 * with the goal-state cost (or, for a reward_head model, the MODEL_REWARD cost of RewardAgent,
 * agents.py:336-362), stopping once mean |delta a| < stop_condition -- as one launch (forward,
 * backward and the Adam step on the device; no host round trip per iteration): Wpad/16 cooperating
 * workgroups that hand hidden vectors to each other, or one workgroup where those do not apply
 * (shapes outside the cooperative kernel's: L == 1, W not one of 64 / 128 / 256 / 512, s + a > 32;
 * reward-head models run either).
 * actions: [H][a] device, in: the initial sequence, out: the optimised one. states_out: [H+1][s]
 * = the last iteration's rollout (computed before its update, as the reference returns it).
 * iterations_out: device int32 (iterations run) or NULL. Needs ensemble == 1 and a GOAL_STATE cost
 * (reward_head == 0) or a MODEL_REWARD cost (reward_head == 1), else MBRL_EUNSUPPORTED.
 * workspace >= mbrl_gd_workspace_bytes(shape, H). */
size_t mbrl_gd_workspace_bytes(const mbrl_mlp_shape* shape, int32_t H);
size_t mbrl_gd_batch_workspace_bytes(const mbrl_mlp_shape* shape, int32_t H, int32_t B);
int mbrl_gd_plan(const mbrl_mlp_shape* shape, const void* packed, const mbrl_norm* norm, const mbrl_cost* cost,
                 const float* s0, float* actions, int32_t H, int32_t num_iterations, float stop_condition,
                 float lr, float* states_out, int32_t* iterations_out, void* workspace, size_t ws_bytes,
                 mbrl_stream_t stream);
/* B independent gradient-descent plans in shared launches (parallel environments: one start state
 * each, SURVEY.md §8f rank 3 "batching over restarts"): s0 [B][s], actions [B][H][a] (in: the initial
 * sequences, out: the optimised ones), states_out [B][H+1][s], iterations_out [B] or NULL. Each plan
 * is exactly mbrl_gd_plan's (same arithmetic, its own stop test); the cooperative grids of as many
 * plans as fit the device together run in one launch. workspace >= mbrl_gd_batch_workspace_bytes. */
int mbrl_gd_plan_batch(const mbrl_mlp_shape* shape, const void* packed, const mbrl_norm* norm, const mbrl_cost* cost,
                       const float* s0, float* actions, int32_t B, int32_t H, int32_t num_iterations,
                       float stop_condition, float lr, float* states_out, int32_t* iterations_out, void* workspace,
                       size_t ws_bytes, mbrl_stream_t stream);
/* The gradient one iteration of mbrl_gd_plan_batch consumes (added within ABI v13): the same kernels
 * through the same dispatch (cooperative or one workgroup, MBRL_OPT_GD_SINGLE / GD_HOP / DEBUG_GD_ABORT,
 * the groups of a batch) run the forward and backward pass of the given sequences and store
 * d loss / d actions, the values their Adam step reads, to grad_out [B][H][a] in place of that step.
 * actions [B][H][a] is only read; states_out [B][H+1][s] is the rollout of the given actions.
 * workspace >= mbrl_gd_batch_workspace_bytes(shape, H, B); checks and codes as mbrl_gd_plan_batch,
 * and MBRL_EINVAL for a NULL grad_out. */
int mbrl_gd_grad(const mbrl_mlp_shape* shape, const void* packed, const mbrl_norm* norm, const mbrl_cost* cost,
                 const float* s0, const float* actions, int32_t B, int32_t H, float* grad_out, float* states_out,
                 void* workspace, size_t ws_bytes, mbrl_stream_t stream);

/* ---- model training: torch.optim.Adam.step() for one fp32 parameter group
 * (torch/optim/adam.py _multi_tensor_adam, capturable = False, amsgrad = False, maximize = False),
 * the optimizer the reference's training loop steps once per batch (models.py:53-93 with the
 * optimizer of experiment.py:55-62), as one launch over all of the group's tensors. It leaves the
 * parameters, exp_avg and exp_avg_sq bit-identical to torch's own step; the caller keeps the step
 * counters (CPU tensors in torch) and computes the per-tensor scalars in double as adam.py does:
 *   step_size = float(-(lr / (1 - beta1 ** step))),  bc2_sqrt = float((1 - beta2 ** step) ** 0.5)
 * with `step` already incremented. grad is read only (weight decay does not write it back). */
typedef struct {
    float* param;
    const float* grad;
    float* exp_avg;
    float* exp_avg_sq;
    int64_t numel;
    float step_size;
    float bc2_sqrt;
} mbrl_adam_tensor;

typedef struct {
    float lerp_weight;      /* float(1 - beta1) */
    float beta2;            /* float(beta2)     */
    float one_minus_beta2;  /* float(1 - beta2) */
    float eps;              /* float(eps)       */
    float weight_decay;     /* float(weight_decay); 0 = none (L2 added to the gradient, Adam not AdamW) */
} mbrl_adam_hparams;

int mbrl_adam_step(const mbrl_adam_tensor* tensors, int32_t count, const mbrl_adam_hparams* hparams,
                   mbrl_stream_t stream);

/* ---- model training: the gradient of one batch's loss for the reference's
 * MLP dynamics models -- Model (models.py:96-110: n_hidden Linear-ReLU layers and a linear state
 * head) and ModelWithReward (models.py:125-163: the same trunk, a state head and a reward head) --
 * under the loss of their train_model (models.py:53-93, 165-217): MSELoss(predicted next state,
 * next state) (+ MSELoss(predicted reward, reward)) summed over the horizon steps, i.e. what
 * `loss.backward()` leaves in each Linear's .grad after optimizer.zero_grad(). The batch is
 * `batch` transitions of the stacked dataset, rows batch_idx[0..batch) (each < transitions, not
 * checked on the device), every horizon step of each. fp32 throughout; the summation order is not
 * autograd's, so gradients match torch's to rounding, not bit for bit.
 * weight / bias: linear1 .. linear{n_hidden} (the trunk, hidden x in), linear{n_hidden+1} (state
 * head, state_dim x hidden) and, with reward_head, linear{n_hidden+2} (1 x hidden); the *_grad
 * arrays are overwritten. loss_out: 3 device floats (total, state, reward) or NULL.
 * workspace >= mbrl_train_workspace_bytes(model, batch). */
#define MBRL_TRAIN_MAX_LAYERS 10   /* n_hidden + 2 */
typedef struct {
    int32_t state_dim, action_dim, hidden, n_hidden, reward_head, horizon;
    const float* weight[MBRL_TRAIN_MAX_LAYERS];
    const float* bias[MBRL_TRAIN_MAX_LAYERS];
    float* weight_grad[MBRL_TRAIN_MAX_LAYERS];
    float* bias_grad[MBRL_TRAIN_MAX_LAYERS];
} mbrl_train_model;

typedef struct {
    const float* states;       /* [transitions][horizon][state_dim]  (TransitionsDataset.stacked) */
    const float* actions;      /* [transitions][horizon][action_dim] */
    const float* next_states;  /* [transitions][horizon][state_dim]  */
    const float* rewards;      /* [transitions][horizon], read with reward_head only */
    int64_t transitions;
} mbrl_train_data;

size_t mbrl_train_workspace_bytes(const mbrl_train_model* model, int32_t batch);
/* Byte offset in the workspace of a 32-bit status word the fused training step (two hidden layers)
 * sets bit 0 of if one of its bounded in-launch waits timed out -- a workgroup-dispatch order the
 * kernels rely on was not kept and an Adam step may have raced a read of its weights. Never expected;
 * the word is sticky (the caller reads it after training and clears it). The caller zeroes the
 * workspace once before its first use: the fused step tags its layer-0 fold partials with a serial
 * kept in the workspace. Each mbrl_train_grads / mbrl_train_epoch call clears the step's arrival
 * tickets and band counters itself (one memset on entry, ABI v13), so a step that timed out does not
 * carry stale counts into the next call. (size_t)-1 for a bad shape. */
size_t mbrl_train_status_offset(const mbrl_train_model* model, int32_t batch);
int mbrl_train_grads(const mbrl_train_model* model, const mbrl_train_data* data, const int64_t* batch_idx,
                     int32_t batch, float* loss_out, void* workspace, size_t ws_bytes, mbrl_stream_t stream);

/* A whole training epoch with Adam (models.py:63-93 with experiment.py:55-62's optimizer): for each
 * batch b = 0 .. ceil(rows / batch_size) - 1 of the device row order `order` (the last one short),
 * mbrl_train_grads on rows order[b * batch_size ..] and then mbrl_adam_step over `tensors` (one
 * parameter group: every Linear's weight and bias, grad = the model's *_grad buffers) with that
 * step's scalars step_sizes[b * count + i], bc2_sqrt[b * count + i] (host arrays, computed as for
 * mbrl_adam_step). The host issues every launch of the epoch in one call. losses: [batches][3]
 * device floats (total, state, reward per batch) or NULL. workspace as for mbrl_train_grads with
 * batch = batch_size. Two hidden layers (the reference's models): two launches per batch (forward with
 * the output layer, then the backward with the layer-0 fold) with the Adam step inside them, each
 * batch's launches also gathering the next batch's rows; the result is the per-batch calls' bit for
 * bit (tests/test_gpu_train_native.py). */
int mbrl_train_epoch(const mbrl_train_model* model, const mbrl_train_data* data, const int64_t* order, int64_t rows,
                     int32_t batch_size, const mbrl_adam_tensor* tensors, int32_t count,
                     const mbrl_adam_hparams* hparams, const float* step_sizes, const float* bc2_sqrt, float* losses,
                     void* workspace, size_t ws_bytes, mbrl_stream_t stream);

/* ---- ensemble training (added within ABI v13): E members of one shape -- a PETS-style ensemble, each
 * member on its own bootstrap resample of one dataset -- trained in shared launches. `members` is a host
 * array of E mbrl_train_model with equal state_dim, action_dim, hidden, n_hidden, reward_head and
 * horizon and with their own weight, bias and gradient buffers. Member e's result -- gradients,
 * parameters, Adam state and losses -- is that of mbrl_train_grads / mbrl_train_epoch on that member
 * alone with its own rows, bit for bit.
 * Launches per batch: 2 (n_hidden + 1) of the tiled product kernel (the MBRL_OPT_TRAIN_SPLIT layout with
 * the layer-0 weight gradient in its own launch, the member on a grid axis) and, in the epoch call, one
 * Adam launch over all E * count tensors (up to 64 tensors per launch; more take further launches) --
 * whatever E is. None of these launches waits on another workgroup: every hand-off is a kernel boundary
 * on the stream. The training options (MBRL_OPT_TRAIN_*) other than MBRL_OPT_TRAIN_TILE do not apply.
 * batch_idx: [E][batch] device rows; orders: [E][rows] device rows (indices may repeat; each
 * < transitions, not checked on the device). tensors: [E][count] host; step_sizes, bc2_sqrt:
 * [batches][E * count] host; loss_out: [E][3], losses: [batches][E][3] device floats or NULL.
 * workspace >= mbrl_train_ensemble_workspace_bytes(members, E, batch) (0 for a bad shape); it needs no
 * zeroing and holds no status word.
 * Before any launch: MBRL_EINVAL for E < 1, members whose shapes differ, any NULL mbrl_train_epoch
 * rejects, or a weight, bias or gradient pointer bound twice among the members; MBRL_EUNSUPPORTED for
 * E > MBRL_TRAIN_MAX_MEMBERS (the members' pointer table travels in the launch arguments);
 * MBRL_EWORKSPACE for a workspace that is too small. */
#define MBRL_TRAIN_MAX_MEMBERS 8
size_t mbrl_train_ensemble_workspace_bytes(const mbrl_train_model* members, int32_t E, int32_t batch);
int mbrl_train_grads_ensemble(const mbrl_train_model* members, int32_t E, const mbrl_train_data* data,
                              const int64_t* batch_idx, int32_t batch, float* loss_out, void* workspace,
                              size_t ws_bytes, mbrl_stream_t stream);
int mbrl_train_epoch_ensemble(const mbrl_train_model* members, int32_t E, const mbrl_train_data* data,
                              const int64_t* orders, int64_t rows, int32_t batch_size, const mbrl_adam_tensor* tensors,
                              int32_t count, const mbrl_adam_hparams* hparams, const float* step_sizes,
                              const float* bc2_sqrt, float* losses, void* workspace, size_t ws_bytes,
                              mbrl_stream_t stream);

/* ---- held-out evaluation of ensemble members (added within ABI v13): E members of one shape, forward
 * only, on the dataset rows rows[0..R) (device int64; indices may repeat and need no order; each
 * < transitions, not checked on the device; R may exceed transitions). With i = rows[r],
 * x = (states[i][h], actions[i][h]) and (s^, r^) the member's forward pass as mbrl_train_grads defines it
 * (n_hidden Linear-ReLU layers, the state head and, with reward_head, the reward head; the weights are
 * read from the live buffers of the struct, whose weight_grad / bias_grad are ignored and may be NULL; a
 * member may be listed twice):
 *   row_err[e][r][h]     = sum_j (s^_j - next_states[i][h][j])^2      fp32, j ascending, no contraction
 *   row_rew_err[e][r][h] = (r^ - rewards[i][h])^2                     required iff reward_head, else NULL
 *   loss_out[e]          = (state + reward, state, reward) or NULL, with
 *                          state  = sum_h (sum_r row_err[e][r][h]) / (R s),
 *                          reward = sum_h (sum_r row_rew_err[e][r][h]) / R
 * -- mbrl_train_grads' loss of a batch made of these rows. The sum over r is taken in one order that
 * depends on R alone: lane t of 1024 adds r = t, t + 1024, ... ascending, and the 1024 partials meet in a
 * pairwise tree (partial[t] += partial[t + d], d = 512, 256, .. 1); the steps are added h ascending.
 * row_err[e][r][h] depends, byte for byte, on member e's parameters and dataset row rows[r] at step h
 * alone: not on E, the other members, R, r or the neighbouring rows. Every output element is written and
 * what the outputs held on entry never matters. No workspace, no allocation, no synchronisation: stream-
 * ordered and capturable. Two launches whatever E and R are (one with loss_out == NULL): the row errors
 * with the members on a grid axis, 16 (r, h) positions per workgroup, then one workgroup per member for
 * the losses; neither waits on another workgroup.
 * Envelope: state_dim, state_dim + action_dim and hidden <= MBRL_EVAL_MAX_DIM, n_hidden <=
 * MBRL_TRAIN_MAX_LAYERS - 2, action_dim = 0 with NULL actions, parameters at any 4-byte alignment;
 * beyond it MBRL_EUNSUPPORTED. Before any launch: MBRL_EINVAL for NULL members, data, rows or row_err, a
 * missing or superfluous row_rew_err, a NULL weight or bias, E < 1, R < 1, a bad shape or member shapes
 * that differ; MBRL_EUNSUPPORTED for E > MBRL_TRAIN_MAX_MEMBERS or E * R * horizon >= 2^31. */
#define MBRL_EVAL_MAX_DIM 1024
int mbrl_eval_members(const mbrl_train_model* members, int32_t E, const mbrl_train_data* data,
                      const int64_t* rows, int64_t R, float* row_err, float* row_rew_err, float* loss_out,
                      mbrl_stream_t stream);

/* ---- open-loop evaluation of ensemble members (added within ABI v13): the k-step error a planner's rollout
 * meets. Members, data, rows and R as for mbrl_eval_members; the member's own prediction is fed back as the
 * next state for horizon steps. With i = rows[r] and x_0 = states[i][0], for h = 0 .. horizon - 1:
 *   (s^_{h+1}, r^_h) = the member's forward pass on (x_h, actions[i][h])   as mbrl_eval_members defines it
 *   x_{h+1}          = s^_{h+1}       the state head's fp32 values, not renormalised and not clamped: the
 *                                     stacked dataset holds next_states[i][h] and states[i][h + 1] as one
 *                                     sample under one normalisation, so this is the identity in the space
 *                                     the member is trained in. NaN and inf propagate down the row's chain.
 *   row_err[e][r][h]     = sum_j (s^_{h+1,j} - next_states[i][h][j])^2     fp32, j ascending, no contraction
 *   row_rew_err[e][r][h] = (r^_h - rewards[i][h])^2                        required iff reward_head, else NULL
 *   pred_out[e][r][h][j] = s^_{h+1,j}                                      or NULL; every element is written
 *   loss_out[e]          = mbrl_eval_members' loss_out over these row_err / row_rew_err, in its summation
 *                          order, or NULL: open-loop and one-step losses share a scale, and mbrl_keep_best
 *                          takes either.
 * states[i][h] for h >= 1 is never read. At horizon 1 every output equals mbrl_eval_members', byte for byte,
 * and step h of a longer call equals mbrl_eval_members on a horizon-1 dataset whose states are
 * pred_out[e][r][h - 1]. The bytes of (e, r, h) depend on member e's parameters and dataset row rows[r]
 * alone: not on E, the other members, R, r, the neighbouring rows (a non-finite neighbour included) or what
 * the outputs held on entry. No workspace, no allocation, no synchronisation: stream-ordered and capturable.
 * Two launches whatever E, R and horizon are (one with loss_out == NULL): 16 rows of one member per
 * workgroup, which runs the horizon loop with the activations in LDS; no workgroup waits on another.
 * Envelope, argument checks and error codes are mbrl_eval_members', all before any launch. */
int mbrl_eval_members_open_loop(const mbrl_train_model* members, int32_t E, const mbrl_train_data* data,
                                const int64_t* rows, int64_t R, float* row_err, float* row_rew_err,
                                float* pred_out, float* loss_out, mbrl_stream_t stream);

/* ---- training on the open-loop loss (added within ABI v13, additively: no existing entry, struct or option
 * changes, no new option id): the training counterpart of mbrl_eval_members_open_loop, backpropagation through
 * the fed-back predictions. Per member e, over the rows i = batch_idx[e][b], b < B = batch, with
 * H = members[0].horizon and x_0 = states[i][0], for h = 0 .. H - 1:
 *   (s^_{h+1}, r^_h) = the member's forward pass on (x_h, actions[i][h])    exactly mbrl_eval_members_open_loop's
 *   x_{h+1}          = s^_{h+1}                                             not detached, clamped or renormalised
 *   loss = sum_h [ sum_b sum_j (s^_{h+1,j} - next_states[i][h][j])^2 / (B s) + sum_b (r^_h - rewards[i][h])^2 / B ]
 * -- the scale of mbrl_train_grads (2 / (B s) and 2 / B on the residuals) and of mbrl_eval_members' loss_out.
 * states[i][h] for h >= 1 is never read. The gradient is the full derivative: the residual of step h reaches
 * the parameters through every earlier step's prediction as well. At horizon 1 it is
 * mbrl_train_grads_ensemble's gradient to rounding. The *_grad arrays are overwritten.
 * Members, data, batch_idx [E][batch], orders [E][rows], tensors, step_sizes, bc2_sqrt, loss_out [E][3] and
 * losses [batches][E][3] as for mbrl_train_grads_ensemble / mbrl_train_epoch_ensemble; E = 1 is the single
 * model. loss_out[e] equals mbrl_eval_members_open_loop's loss_out[e] on rows = batch_idx[e], R = batch, byte
 * for byte. Member e's gradients and losses depend, byte for byte, on member e's parameters and rows alone --
 * not on E or the other members (a non-finite one included) -- and two calls on the same inputs return the same
 * bytes: no floating-point atomics, every output element one ordered chain. Summation orders: a weight
 * gradient sums the batch * H positions p = h * batch + b in the order of mbrl_train_grads' weight-gradient
 * product over K = batch * H rows (contiguous K ranges per wave, the waves' partials added in wave order: a
 * function of batch * H alone); a bias gradient adds, per 16-row tile of the batch, the steps h descending, each
 * step's valid rows ascending, and then the tiles ascending.
 * ws: the workspace, ws_bytes >= mbrl_train_open_loop_workspace_bytes(members, E, batch) (0 for a bad shape),
 * 16-byte aligned; it may hold any bytes on entry and needs no zeroing (tests/test_gpu_train_open_loop.py fills it
 * with NaN and with 0xFF bytes). Stream-ordered and capturable: no allocation, no
 * synchronisation, and no workgroup waits on another -- every hand-off is a kernel boundary.
 * Launches per batch, whatever E, batch and horizon are: n_hidden + 4 in mbrl_train_grads_open_loop (forward,
 * backward through time, n_hidden + 1 weight-gradient launches, the loss; one fewer with loss_out == NULL) and
 * n_hidden + 5 in mbrl_train_epoch_open_loop (the Adam launch over all E * count tensors, 64 tensors per launch;
 * more take further launches).
 * Envelope: mbrl_eval_members_open_loop's (state_dim, state_dim + action_dim and hidden <= MBRL_EVAL_MAX_DIM,
 * n_hidden <= MBRL_TRAIN_MAX_LAYERS - 2, action_dim = 0 with NULL actions, parameters and gradients at any
 * 4-byte alignment) less what the backward kernel's LDS (160 KiB) cannot hold: with up16(x) = x rounded up to a
 * multiple of 16, J = state_dim + reward_head,
 *   ld = up16(max(hidden, state_dim + action_dim, J)) + 4,   wacc = up16(max(hidden, J)),
 *   32 ld + (n_hidden + 1) wacc <= 40960 floats
 * (hidden = 1024 with state_dim + action_dim <= 1024: n_hidden <= 6; hidden <= 880: every n_hidden); beyond it
 * MBRL_EUNSUPPORTED. Before any launch: the argument checks and error codes of mbrl_train_grads_ensemble /
 * mbrl_train_epoch_ensemble (MBRL_EINVAL for E < 1, shapes that differ, NULL arguments, a pointer bound twice
 * or a misaligned workspace; MBRL_EUNSUPPORTED for E > MBRL_TRAIN_MAX_MEMBERS or E * batch * horizon >= 2^31;
 * MBRL_EWORKSPACE for a workspace that is too small). */
size_t mbrl_train_open_loop_workspace_bytes(const mbrl_train_model* members, int32_t E, int32_t batch);
int mbrl_train_grads_open_loop(const mbrl_train_model* members, int32_t E, const mbrl_train_data* data,
                               const int64_t* batch_idx, int32_t batch, float* loss_out, void* ws,
                               size_t ws_bytes, mbrl_stream_t stream);
int mbrl_train_epoch_open_loop(const mbrl_train_model* members, int32_t E, const mbrl_train_data* data,
                               const int64_t* orders, int64_t rows, int32_t batch_size, const mbrl_adam_tensor* tensors,
                               int32_t count, const mbrl_adam_hparams* hparams, const float* step_sizes,
                               const float* bc2_sqrt, float* losses, void* ws, size_t ws_bytes,
                               mbrl_stream_t stream);

/* ---- global-norm gradient clipping for the ensemble epochs (added within ABI v13, additively: no existing entry,
 * struct, option or version number changes): torch.nn.utils.clip_grad_norm_(member.parameters(), max_norm) (L2,
 * error_if_nonfinite = False) between backward() and Adam.step(), per member e and per batch, and a record of the
 * pre-clip norms. fp32, round to nearest, no contraction. tensors: [E][count] host, member e's `count` gradient
 * tensors (E <= MBRL_TRAIN_MAX_MEMBERS).
 * Sum of squares of member e, in one order that depends on its tensors' numels alone -- not on E, the member's
 * position, the other members or pointer alignment:
 *   - tensor i is cut into chunks of 1024 consecutive elements, the last one padded with zeros that take part as
 *     zeros; a tensor with numel == 0 has no chunk;
 *   - in a chunk, lane t of 256 forms ((g[4t]^2 + g[4t+1]^2) + g[4t+2]^2) + g[4t+3]^2, each square rounded before it
 *     is added, and the 256 lane values meet in the pairwise tree v[t] += v[t + d], d = 128, 64, .. 1;
 *   - the member's P chunk partials lie end to end, tensor ascending, chunk ascending, and are reduced by
 *     mbrl_eval_members' rule: lane t of 1024 adds partials t, t + 1024, .. ascending, then the pairwise tree
 *     d = 512, .. 1.
 *   norm = sqrtf(sum) correctly rounded,  q = max_norm / (norm + 1e-6f),  coef = q > 1 ? 1 : q  (a NaN q stays NaN,
 *   as under torch's clamp(max = 1)).
 * So a norm within max_norm gives coef == 1.0f exactly, max_norm = +inf never clips, and a zero gradient gives
 * coef = 1. A member with a NaN in its gradient gets norm = coef = NaN and NaN parameters from the clipped step; one
 * with an inf gets norm = inf and coef = max_norm / inf = 0 (NaN under max_norm = +inf), so its step consumes
 * inf * 0 = NaN where the inf was and 0 elsewhere -- both exactly as in torch -- while every other member's bytes
 * are what they are without it.
 * mbrl_grad_norm: norm_out[e] (device [E], or NULL) and coef_out[e] (device [E], required) for the E members; of
 * each tensor only grad and numel are read. Two launches whatever E, count and the shapes are: the chunk partials
 * of all E * count tensors (one workgroup per chunk; the table travels in the launch arguments, 64 tensors per
 * launch, more take further launches; 16-byte loads where the gradient pointer allows and 4-byte loads otherwise,
 * the same bytes either way), then one workgroup per member. No atomics; no workgroup waits on another.
 * mbrl_adam_step_clipped: mbrl_adam_step over all E * count tensors (one launch per 64 tensors) in which member e's
 * tensors consume g' = g * coef[e], one rounded fp32 product per element, in place of g; everything else, the
 * MBRL_OPT_ADAM_ARITH handling included, is mbrl_adam_step's, and coef[e] == 1.0f is mbrl_adam_step bit for bit.
 * The gradient buffers are only read: after the call they still hold the raw, unclipped gradient.
 * mbrl_train_epoch_ensemble_clipped / mbrl_train_epoch_open_loop_clipped: the sibling epoch with, per batch, the
 * two mbrl_grad_norm launches and the mbrl_adam_step_clipped launch in place of the Adam launch -- two launches
 * more per batch than the sibling. clip->norms[b][e] (or NULL) receives batch b's pre-clip norm of member e.
 * With max_norm = +inf the parameters, moments and losses are the sibling's byte for byte.
 * Workspace (mbrl_grad_norm's ws, clip->workspace): >= mbrl_grad_clip_workspace_bytes(tensors, E, count) bytes (0
 * for a bad table), 4-byte aligned; any bytes on entry, no zeroing (tests/test_gpu_grad_clip.py fills it, and the
 * epoch entries' own ws, with NaN and with 0xFF bytes). It holds coef[E] and the chunk partials. The epoch entries'
 * own ws is the siblings'.
 * Stream-ordered and capturable: no allocation, no synchronisation. Before any launch: MBRL_EINVAL for a NULL
 * clip, a max_norm that is NaN or <= 0, a NULL coef / coef_out / workspace, E < 1, count < 1, a NULL table or a
 * tensor with numel < 0 or with numel > 0 and a NULL grad (the epoch entries and mbrl_adam_step_clipped: a NULL
 * param or moment as well); MBRL_EUNSUPPORTED for E > MBRL_TRAIN_MAX_MEMBERS or a member of 2^28 chunks or more;
 * MBRL_EWORKSPACE for a clip workspace that is too small; and every check and code of the sibling entry. */
typedef struct {
    float max_norm;      /* > 0, +inf allowed (records norms, never clips); NaN or <= 0: MBRL_EINVAL */
    int32_t _pad;
    float* norms;        /* device [batches][E], or NULL */
    void* workspace;     /* >= mbrl_grad_clip_workspace_bytes; any bytes on entry, no zeroing */
    size_t ws_bytes;
} mbrl_grad_clip;
size_t mbrl_grad_clip_workspace_bytes(const mbrl_adam_tensor* tensors, int32_t E, int32_t count);
int mbrl_grad_norm(const mbrl_adam_tensor* tensors, int32_t E, int32_t count, float max_norm, float* norm_out,
                   float* coef_out, void* ws, size_t ws_bytes, mbrl_stream_t stream);
int mbrl_adam_step_clipped(const mbrl_adam_tensor* tensors, int32_t E, int32_t count,
                           const mbrl_adam_hparams* hparams, const float* coef, mbrl_stream_t stream);
int mbrl_train_epoch_ensemble_clipped(const mbrl_train_model* members, int32_t E, const mbrl_train_data* data,
                                      const int64_t* orders, int64_t rows, int32_t batch_size,
                                      const mbrl_adam_tensor* tensors, int32_t count, const mbrl_adam_hparams* hparams,
                                      const float* step_sizes, const float* bc2_sqrt, float* losses, void* ws,
                                      size_t ws_bytes, mbrl_stream_t stream, const mbrl_grad_clip* clip);
int mbrl_train_epoch_open_loop_clipped(const mbrl_train_model* members, int32_t E, const mbrl_train_data* data,
                                       const int64_t* orders, int64_t rows, int32_t batch_size,
                                       const mbrl_adam_tensor* tensors, int32_t count, const mbrl_adam_hparams* hparams,
                                       const float* step_sizes, const float* bc2_sqrt, float* losses, void* ws,
                                       size_t ws_bytes, mbrl_stream_t stream, const mbrl_grad_clip* clip);

/* ---- probabilistic members: training on the Gaussian negative log-likelihood (added within ABI v13, additively: no
 * existing entry, struct, option id or version number changes). A member is an mbrl_train_model with
 * reward_head == 0 whose output layer weight[n_hidden] / bias[n_hidden] (and their gradients) is ONE head of
 * 2 s rows, s = state_dim: [2 s][hidden] and [2 s]. Rows [0, s) are the predicted mean m, rows [s, 2 s) the raw
 * log-variance r. The mean rows are the head's first s rows, so the same struct is a deterministic member for
 * mbrl_eval_members, mbrl_mlp_pack and every planner: they read the mean and nothing else.
 * Per member e, over the positions p = (b, h), b < B = batch, h < H = horizon, teacher forced as in mbrl_train_grads:
 * with i = batch_idx[e][b] the input is (states[i][h], actions[i][h]) and the target y = next_states[i][h]. With
 * softplus(x) = max(x, 0) + log1p(exp(-|x|)), sigmoid(x) = 1 / (1 + exp(-x)), fp32 throughout:
 *   (m, r)  = the head's output on the trunk's last activation       mbrl_eval_members' fma chains, row by row
 *   u_j     = max_lv_j - softplus(max_lv_j - r_j)
 *   lv_j    = min_lv_j + softplus(u_j - min_lv_j)                    the bounded log-variance, in (min_lv, max_lv)
 *   row_nll[e][b][h] = sum_j [ (m_j - y_j)^2 * exp(-lv_j) + lv_j ]   j ascending, no contraction
 *   row_err[e][b][h] = sum_j (m_j - y_j)^2                           mbrl_eval_members' value, byte for byte
 *   row_lv [e][b][h] = sum_j lv_j
 *   loss_out[e] = (nll, mse, mean_lv), each sum_h (sum_b row_*[e][b][h]) / (B s) in mbrl_eval_members' summation
 *                 order: the project's scale, so the NLL and the MSE curves sit beside each other (the constant
 *                 s H log(2 pi) / 2 and the factor 1/2 of the textbook density are left out).
 * The gradient of nll with respect to the head's outputs:
 *   dm_j = 2 (m_j - y_j) exp(-lv_j) / (B s)
 *   dr_j = (1 - (m_j - y_j)^2 exp(-lv_j)) / (B s) * sigmoid(u_j - min_lv_j) * sigmoid(max_lv_j - r_j)
 * and the *_grad arrays receive d nll / d parameter (overwritten). The bounds are read only: they are not trained.
 * The deltas of the hidden layers (delta_l = (delta_{l+1} W_{l+1}) masked by the activation) are n-ordered chains
 * accumulated in fp64 from the fp32 deltas and weights and rounded to fp32 once: exp(-lv) makes their terms cancel.
 * bounds: min_logvar and max_logvar, device [s] each, shared by the E members.
 * mbrl_eval_members_nll: the same values forward only, on rows[0..R) for every member (mbrl_eval_members'
 * arguments); row_nll, row_err and row_lv are [E][R][H] device outputs, all three required (there is no workspace
 * for the third); loss_out [E][3] or NULL. It runs the gradient entry's forward kernel with its stores switched
 * off, so the gradient entry's loss_out[e] and row values equal this entry's on rows = batch_idx[e], R = batch, byte
 * for byte; row_err equals mbrl_eval_members' on the same struct.
 * Members, data, batch_idx [E][batch], orders [E][rows], tensors, step_sizes, bc2_sqrt, loss_out [E][3], losses
 * [batches][E][3] and clip as for mbrl_train_grads_open_loop / mbrl_train_epoch_open_loop(_clipped), and every
 * contract of those entries holds: member e's gradients, losses and row values depend, byte for byte, on member
 * e's parameters and rows alone -- not on E or the other members (a non-finite one included); two calls return
 * the same bytes; no floating-point atomics; no workgroup waits on another; stream-ordered and capturable, no
 * allocation. ws: >= mbrl_train_nll_workspace_bytes(members, E, batch) bytes (0 for a bad shape), 16-byte aligned,
 * any bytes on entry, no zeroing, no status word. After the call it begins with the row values: row_nll, row_err
 * and row_lv, each [E][batch][H] floats, each starting on a multiple of 64 floats (up64(E batch H) apart).
 * Summation orders: a weight gradient sums the B * H positions
 * p = b * H + h in the order of mbrl_train_grads' weight-gradient product over K = B * H rows; a bias gradient adds,
 * per 16-position tile, the valid positions ascending and then the tiles ascending.
 * Launches per batch, whatever E, batch and horizon are: n_hidden + 4 in mbrl_train_grads_nll (forward, backward,
 * n_hidden + 1 weight-gradient launches, the loss; one fewer with loss_out == NULL), n_hidden + 5 in
 * mbrl_train_epoch_nll (the Adam launch, 64 tensors per launch) and two more in mbrl_train_epoch_nll_clipped;
 * two in mbrl_eval_members_nll (one with loss_out == NULL).
 * Envelope: mbrl_eval_members' (state_dim, state_dim + action_dim and hidden <= MBRL_EVAL_MAX_DIM, n_hidden <=
 * MBRL_TRAIN_MAX_LAYERS - 2, action_dim = 0 with NULL actions, parameters and gradients at any 4-byte alignment)
 * less what the two 16-position activation buffers in LDS (160 KiB) cannot hold with a head of 2 s outputs: with
 * up16(x) = x rounded up to a multiple of 16,
 *   ld = up16(max(hidden, state_dim + action_dim, 2 state_dim)) + 4,   32 ld <= 40960 floats
 * (state_dim <= 632; hidden = 1024 with every n_hidden); beyond it MBRL_EUNSUPPORTED. Before any launch: the
 * argument checks and error codes of the open-loop entries (mbrl_eval_members' for mbrl_eval_members_nll), and
 * MBRL_EINVAL for NULL bounds, a NULL bound array, reward_head != 0 or a NULL row_nll / row_lv. */
typedef struct {
    const float* min_logvar;   /* device [state_dim] */
    const float* max_logvar;   /* device [state_dim] */
} mbrl_nll_bounds;
size_t mbrl_train_nll_workspace_bytes(const mbrl_train_model* members, int32_t E, int32_t batch);
int mbrl_train_grads_nll(const mbrl_train_model* members, int32_t E, const mbrl_train_data* data,
                         const int64_t* batch_idx, int32_t batch, const mbrl_nll_bounds* bounds, float* loss_out,
                         void* ws, size_t ws_bytes, mbrl_stream_t stream);
int mbrl_train_epoch_nll(const mbrl_train_model* members, int32_t E, const mbrl_train_data* data,
                         const int64_t* orders, int64_t rows, int32_t batch_size, const mbrl_adam_tensor* tensors,
                         int32_t count, const mbrl_adam_hparams* hparams, const float* step_sizes,
                         const float* bc2_sqrt, float* losses, void* ws, size_t ws_bytes, mbrl_stream_t stream,
                         const mbrl_nll_bounds* bounds);
int mbrl_train_epoch_nll_clipped(const mbrl_train_model* members, int32_t E, const mbrl_train_data* data,
                                 const int64_t* orders, int64_t rows, int32_t batch_size,
                                 const mbrl_adam_tensor* tensors, int32_t count, const mbrl_adam_hparams* hparams,
                                 const float* step_sizes, const float* bc2_sqrt, float* losses, void* ws,
                                 size_t ws_bytes, mbrl_stream_t stream, const mbrl_nll_bounds* bounds,
                                 const mbrl_grad_clip* clip);
int mbrl_eval_members_nll(const mbrl_train_model* members, int32_t E, const mbrl_train_data* data,
                          const int64_t* rows, int64_t R, const mbrl_nll_bounds* bounds, float* row_nll,
                          float* row_err, float* row_lv, float* loss_out, mbrl_stream_t stream);

/* ---- trajectory-sampling rollouts: CEM plans on sampled ensemble particles (PETS' TS-inf; added within ABI v13,
 * additively: no existing entry, struct, option id or version number changes). The members are the
 * probabilistic members above (mbrl_eval_members_nll's struct: live nn.Linear pointers, a head of 2 s rows,
 * reward_head == 0; the gradient pointers are not read and `horizon` only has to be >= 1). Every candidate is rolled
 * out as Q = E * particles rows; row q = e * particles + p is particle p of member e and stays on that member for
 * the whole horizon. Per row q, candidate n < N and step t < H, with s_0 = s0 (s0[n] with s0_per_candidate), fp32
 * throughout, round to nearest, no contraction, in this order:
 *   1. x       = (normalize_state(s_t), normalize_action(a_t)), state first, each if its flag is set:
 *                (v - mean) / std as written (oracle/cem.py model_input)
 *   2. (m, r)  = the head on the trunk: mbrl_eval_members' k-ordered fma chains, one chain per output element
 *   3. lv_j    = min_lv_j + softplus(u_j - min_lv_j), u_j = max_lv_j - softplus(max_lv_j - r_j): the bounded
 *                log-variance of mbrl_train_grads_nll, softplus(x) = max(x, 0) + log1p(exp(-|x|))
 *   4. sd_j    = expf(0.5f * lv_j) * noise_scale
 *   5. eps_j   = element j & 3 of the four normals (two Box-Muller pairs, as the proposal draw makes them) of
 *                Philox4x32-10 with counter (n + n_offset, t, q, (iteration << 8) | (j >> 2)) and the key
 *                (low, high) half of noise_seed
 *   6. z_j     = m_j + sd_j * eps_j: the noise is added in the space the members were trained in
 *   7. s_{t+1} = z * obs_std + obs_mean if unnormalize_state, else z; this state is fed back
 *   8. c_t     = sum_j (sqrt(((s_{t+1,j} - goal_j) * weights_j)^2 + alpha_state^2) - alpha_state), j ascending
 *                (0 without has_state_cost), plus alpha_action^2 * ((sum_d (cosh(a_{t,d} / alpha_action) - 1), d
 *                ascending) / a) on the raw action (0 without has_action_cost): MBRL_COST_GOAL_STATE
 *   9. costs[q][n] = sum_t c_t, t ascending from 0.
 * With noise_scale == 0 the states are the mean rollout's: states_out[e * particles + p][t][n] then equals
 * mbrl_eval_members_open_loop's pred_out[e][n][t] byte for byte where norm is NULL (the same chains).
 * mbrl_rollout_cost_ts: one launch, grid (ceil(N / 16), Q), no workspace, no atomics, no workgroup waits on another;
 * stream-ordered and capturable. The bytes of a (row, candidate) depend on that candidate's s0 and actions, its
 * member's parameters, the bounds and its counter words alone: not on N, its position in a tile, its neighbours (a
 * non-finite one included), the other members, particles (given q) or whether states_out is NULL.
 * actions [H][N][a] (required: the proposal draw stays mbrl_sample_actions); costs [Q][N] (required); states_out
 * [Q][H][N][s] or NULL; norm may be NULL (no flag set); cost NULL: every c_t is 0. iteration keys the noise only.
 * The group j >> 2 fits the eight bits beside it: the LDS envelope bounds s at 632 (2 * 16 * (2 * 632 + 4) * 4
 * bytes <= 160 KiB), hence at most 158 groups.
 * Before any launch (the outputs stay untouched): the argument checks and codes of mbrl_eval_members_nll, and
 * MBRL_EINVAL for a NULL s0, actions, ts or costs, N < 1, H < 1, n_offset < 0, E > MBRL_TRAIN_MAX_MEMBERS,
 * particles < 1, Q > MBRL_TS_MAX_ROWS, iteration outside [0, 2^24), a negative or non-finite noise_scale,
 * action_dim < 1, MBRL_COST_MODEL_REWARD, a state cost without weights or goal, or a set normaliser flag with NULL
 * statistics; MBRL_EUNSUPPORTED beyond the NLL entries' LDS envelope (above) or for an unknown cost kind.
 *
 * mbrl_cem_plan_ts: mbrl_cem_plan's loop with this rollout in place of the deterministic one. Per iteration `it`:
 * the proposals (mbrl_sample_actions' values), mbrl_rollout_cost_ts with iteration = it (ts->iteration is not
 * read, so every iteration's noise is fresh) into costs [Q][N], then the selection and refit of mbrl_cem_plan over
 * those Q rows (returns[n] = (sum_q costs[q][n]) / Q, sequential in q): bit for bit mbrl_sample_actions,
 * mbrl_rollout_cost_ts, mbrl_cem_update (or mbrl_select_elites + mbrl_cem_refit) with E = Q. states_out [H][s] is
 * mbrl_trajectory's member mean for the final actions: deterministic, on the packed mean rows -- hence both
 * shape / packed (mbrl_mlp_pack of the same members; ensemble = E, reward_head = 0, MBRL_PRECISION_F32) and
 * members [shape->ensemble] / bounds. Records (NULL = off): cost_hist [I][Q][N], returns_hist [I][N], elite_hist
 * [I][K]. ws: >= mbrl_cem_ts_workspace_bytes bytes (0 for bad arguments), any bytes on entry. Every argument check
 * runs before the first launch. The packed shape bounds this entry at four hidden layers (mbrl_rollout_cost_ts
 * alone runs eight). Out of scope for this entry: column-split pairs, sharding, batches, the
 * receding-horizon and coloured-noise inputs, MPPI and the f16 precisions.
 * Measured on the MI355X (s = 17, a = 6, E = 5, N = 4096, H = 30): 10.67 ms per launch at P = 1 and
 * 36.96 ms at P = 4 for 2 x 512 members (0.21 / 0.25 of the fp32 MFMA peak), 19.82 / 61.32 ms for 3 x 512 (0.22 /
 * 0.28); the deterministic mbrl_rollout_cost takes 2.69 / 4.91 ms for the 5 mean rows. The 16-candidate tile
 * streams the live weights from L2 and is 3.1-4.0x slower per row than the packed-stream rollout kernel. */
#define MBRL_TS_MAX_ROWS 256   /* Q = E * particles (PETS uses 20) */
typedef struct {
    int32_t particles;     /* P >= 1 per member */
    int32_t iteration;     /* < 2^24; keys the noise (mbrl_cem_plan_ts passes its own) */
    uint64_t noise_seed;
    float noise_scale;     /* >= 0, finite; 1: the members' own variance, 0: the mean rollout */
} mbrl_ts_params;
int mbrl_rollout_cost_ts(const mbrl_train_model* members, int32_t E, const mbrl_nll_bounds* bounds,
                         const mbrl_norm* norm, const mbrl_cost* cost, const float* s0, int32_t s0_per_candidate,
                         const float* actions, int32_t N, int32_t H, int32_t n_offset, const mbrl_ts_params* ts,
                         float* costs, float* states_out, mbrl_stream_t stream);
size_t mbrl_cem_ts_workspace_bytes(const mbrl_mlp_shape* shape, const mbrl_cem_params* params,
                                   const mbrl_ts_params* ts);
int mbrl_cem_plan_ts(const mbrl_mlp_shape* shape, const void* packed, const mbrl_train_model* members,
                     const mbrl_nll_bounds* bounds, const mbrl_norm* norm, const mbrl_cost* cost, const float* s0,
                     const mbrl_cem_params* params, const mbrl_ts_params* ts, float* mu, float* sigma,
                     float* actions_out, float* states_out, float* cost_hist, float* returns_hist,
                     int64_t* elite_hist, void* ws, size_t ws_bytes, mbrl_stream_t stream);

/* ---- sampled rows for the control loop: a per-step member draw (PETS' TS-1), and the receding-horizon plan on
 * sampled rows, single and batched (added within ABI v13, additively: no existing entry, struct, option id or
 * version number changes).
 * Member modes of the sampled rollout -- only step 2's member of the nine steps above changes:
 *   MBRL_TS_MEMBER_FIXED (0):     the rows above. Q = E * particles, row q stays on member q / particles.
 *   MBRL_TS_MEMBER_RESAMPLED (1): Q = particles rows in all, 1 <= Q <= MBRL_TS_MAX_ROWS, independent of E. Row q at
 *       step t runs member e(q, t) = (uint64(w.x) * E) >> 32, w = Philox4x32-10 of counter
 *       (0, t, q, (iteration << 8) | 0xFF) with the key (low, high) half of noise_seed. The state noise uses the
 *       groups j >> 2 < 158, so group byte 0xFF collides with no noise counter, whatever n + n_offset is. The draw
 *       is shared by all candidates, by design: every candidate's row q sees the same member sequence, so return
 *       differences between candidates carry no member-assignment noise. Every other step is unchanged, the noise
 *       counter (n + n_offset, t, q, (iteration << 8) | g) included.
 * mbrl_rollout_cost_ts_rows: mbrl_rollout_cost_ts with the mode and one more output; FIXED returns that entry's
 * bytes. members_out [Q][H] int32 or NULL: the member each row ran at each step (q / particles in FIXED mode, the
 * draw in RESAMPLED mode), written by the tile-0 workgroups only: a diagnostic. The launch, its independence
 * properties (a (row, candidate) also does not depend on whether members_out is NULL) and costs / states_out are
 * mbrl_rollout_cost_ts's with Q as above. Before any launch, the outputs untouched: that entry's checks and codes;
 * NULL rows or an unknown member_mode: MBRL_EINVAL; in RESAMPLED mode the Q bound applies to particles itself.
 *
 * mbrl_cem_plan_ts_rh / mbrl_cem_plan_ts_rh_batch: mbrl_cem_plan_rh / mbrl_cem_plan_rh_batch with the sampled
 * rollout (iteration = it, rows->ts.iteration is not read) in place of the deterministic one. Inputs, outputs,
 * flags and records are the siblings' with three differences: no events, no mix, and cost_hist has Q rows
 * ([I][Q][N], batched [I][Q][B N]). Every plan runs the kept-rows loop (the selections and the staged refit over
 * Q rows; returns[n] = (sum_q costs[q][n]) / Q), whatever keep is: with keep == 0, no rows and FIXED mode the
 * outputs and cost_hist are mbrl_cem_plan_ts's byte for byte. Problem b's candidate n has Philox index b N + n for
 * the proposals and the particle noise alike (the rollout is one launch over B N candidates with per-candidate
 * start states, n_offset 0); problem 0 of a batch and a B == 1 batch are the single plan byte for byte.
 * states_out is the deterministic member-mean trajectory on the packed mean rows, as in mbrl_cem_plan_ts.
 * ws: >= mbrl_cem_ts_rh_workspace_bytes(shape, params, rows, B) (B = 1 also serves the single plan; 0 for bad
 * arguments), any bytes on entry. Every check runs before the first launch: mbrl_cem_plan_ts's and the
 * receding-horizon siblings', each with its sibling's code (a small workspace: MBRL_EINVAL from the single plan,
 * MBRL_EWORKSPACE from the batch). Out of scope: coloured noise, sharding, column-split pairs, MPPI, the f16
 * precisions and a reward-head cost.
 * Measured on the MI355X: DESIGN.md §9f. */
#define MBRL_TS_MEMBER_FIXED 0
#define MBRL_TS_MEMBER_RESAMPLED 1
typedef struct {
    mbrl_ts_params ts;     /* RESAMPLED: ts.particles is Q */
    int32_t member_mode;   /* MBRL_TS_MEMBER_* */
    int32_t _pad;
} mbrl_ts_rows;
int mbrl_rollout_cost_ts_rows(const mbrl_train_model* members, int32_t E, const mbrl_nll_bounds* bounds,
                              const mbrl_norm* norm, const mbrl_cost* cost, const float* s0, int32_t s0_per_candidate,
                              const float* actions, int32_t N, int32_t H, int32_t n_offset, const mbrl_ts_rows* rows,
                              float* costs, float* states_out, int32_t* members_out, mbrl_stream_t stream);
size_t mbrl_cem_ts_rh_workspace_bytes(const mbrl_mlp_shape* shape, const mbrl_cem_rh_params* params,
                                      const mbrl_ts_rows* rows, int32_t B);
int mbrl_cem_plan_ts_rh(const mbrl_mlp_shape* shape, const void* packed, const mbrl_train_model* members,
                        const mbrl_nll_bounds* bounds, const mbrl_norm* norm, const mbrl_cost* cost, const float* s0,
                        const mbrl_cem_rh_params* params, const mbrl_ts_rows* rows, const float* init_mu_rows,
                        const float* init_sigma_rows, const float* carry_in, float* mu, float* sigma,
                        float* actions_out, float* states_out, float* carry_out, float* carry_returns_out,
                        float* cost_hist, float* returns_hist, int64_t* elite_hist, float* kept_hist, void* ws,
                        size_t ws_bytes, mbrl_stream_t stream);
int mbrl_cem_plan_ts_rh_batch(const mbrl_mlp_shape* shape, const void* packed, const mbrl_train_model* members,
                              const mbrl_nll_bounds* bounds, const mbrl_norm* norm, const mbrl_cost* cost,
                              const float* s0, int32_t B, const mbrl_cem_rh_params* params, const mbrl_ts_rows* rows,
                              const float* init_mu_rows, const float* init_sigma_rows, const float* carry_in,
                              const int32_t* input_flags, float* mu, float* sigma, float* actions_out,
                              float* states_out, float* carry_out, float* carry_returns_out, float* cost_hist,
                              float* returns_hist, int64_t* elite_hist, float* kept_hist, void* ws, size_t ws_bytes,
                              mbrl_stream_t stream);

/* Keep-best snapshots: per member e, v = loss[e * loss_stride] (device) against best_loss[e] AS IT WAS ON
 * ENTRY. If v < best_loss[e] (a NaN is never better): best_loss[e] = v, best_epoch[e] = epoch,
 * stale[e] = 0, and each of the member's `count` tensors tensors[e * count + i] (host table [E][count]) is
 * copied src -> dst bit for bit. Otherwise stale[e] += 1 and no byte of any dst is written. The caller
 * starts with best_loss = +inf, best_epoch = -1, stale = 0 (device arrays [E], in/out).
 * Ordering: the copy launches come first and only read loss and best_loss; the one launch that updates
 * best_loss, best_epoch and stale follows them on the stream, so no copy acts on an updated best_loss.
 * The table travels in the launch arguments (64 tensors per launch; more take further launches). A dst
 * must not overlap loss, best_loss or any src. No workspace, no allocation, no synchronisation.
 * Before any launch: MBRL_EINVAL for a NULL loss, best_loss, best_epoch or stale, E < 1, loss_stride < 1,
 * epoch < 0, count < 0, a NULL table with count > 0, or a tensor with numel < 0 or with numel > 0 and a
 * NULL src or dst. */
typedef struct {
    const float* src;
    float* dst;
    int64_t numel;
} mbrl_copy_tensor;
int mbrl_keep_best(const float* loss, int32_t loss_stride, int32_t E, int32_t epoch, float* best_loss,
                   int32_t* best_epoch, int32_t* stale, const mbrl_copy_tensor* tensors, int32_t count,
                   mbrl_stream_t stream);

/* ---- device-resident transitions (added within ABI v13, additively: no existing entry, struct, option or version
 * number changes): the stacked training tensors and the normalisation statistics of a dataset whose steps live in
 * device memory (mbrl_amd.device_data.DeviceTransitionsDataset), in place of the host's per-transition loops.
 * Step store (the caller's device memory, fp32): one row-major array [S][dim] per field -- states, observations,
 * actions, rewards. A rollout with K transitions occupies K + 1 consecutive rows; row k holds s_k, o_k, a_k, r_k. The
 * action in a rollout's last row and the reward in its first row are padding and are never read.
 *
 * mbrl_dataset_stack: the stacked windows of up to 8 fields in ONE launch (the table travels in the launch
 * arguments):
 *   dst[t][h][j] = (src[win_row[t] + h + shift][j] - mean[j]) / std[j]      t < T, h < horizon, j < dim
 * -- one fp32 subtraction and one correctly rounded fp32 division, the arithmetic of Rollout._norm -- or
 * src[win_row[t] + h + shift][j] itself with NULL statistics. win_row: device int64 [T], the store row of each
 * window's step 0 (not range-checked on the device: rows win_row[t] + shift .. win_row[t] + shift + horizon - 1 of
 * every field must exist). Every element of every dst is written. src, dst, mean and std may sit at any 4-byte
 * alignment: a workgroup walks 1024 consecutive dst elements, one dword per lane, so every load and store
 * instruction of a wave covers 256 consecutive bytes on every alignment (there is no separate vector path). No
 * workspace, no allocation, no synchronisation; stream-ordered and capturable.
 * Before any launch: MBRL_EINVAL for a NULL table, win_row, src or dst, a mean without a std or the reverse, count
 * outside 1 .. 8, T < 1, horizon < 1, dim < 1 or shift outside {0, 1}; MBRL_EUNSUPPORTED when T * horizon * dim >=
 * 2^31 for any field. */
typedef struct {
    const float* src;   /* [S][dim] */
    const float* mean;  /* [dim] or NULL */
    const float* std;   /* [dim] or NULL (both or neither) */
    float* dst;         /* [T][horizon][dim] */
    int32_t dim;
    int32_t shift;      /* 0: inputs (s, o, a); 1: outputs (r, s', o') */
} mbrl_stack_field;
int mbrl_dataset_stack(const mbrl_stack_field* fields, int32_t count, const int64_t* win_row, int64_t T,
                       int32_t horizon, mbrl_stream_t stream);

/* mbrl_dataset_stats: per field (up to 4 in a call) and per column j, over the store rows rows[0 .. R) of src (a
 * device int64 list per field; rows may repeat and need no order): mean[j], the unbiased std[j], min[j] and max[j],
 * four device arrays [dim]. x_i = src[rows[i]][j] is accumulated in float64 in one order that depends on R alone --
 * the same for every column, whatever dim, the other fields and the pointers' alignment are:
 *   - the list positions i are cut into chunks of 1024; absent positions of the last chunk contribute +0.0;
 *   - in a chunk, lane t of 256 forms ((x[4t] + x[4t+1]) + x[4t+2]) + x[4t+3] and the 256 lane values meet in the
 *     pairwise tree v[t] += v[t + d], d = 128, 64, .. 1;
 *   - the chunk partials are reduced by mbrl_eval_members' rule: lane t of 1024 adds partials t, t + 1024, ..
 *     ascending onto +0.0, then the pairwise tree d = 512, .. 1.
 *   mean64 = sum / R stays in float64; a second pass sums (double(x_i) - mean64)^2 (each square rounded before it is
 *   added) in the same order, absent positions again +0.0; std = sqrt(ss / (R - 1)). mean and std are rounded to fp32
 *   once, at the end. R = 1 gives std = NaN, as torch.std does. min and max are exact. A NaN anywhere in a column
 *   makes all four outputs NaN, as under torch; a column holding an inf has mean = +-inf (NaN with both signs) and
 *   std = NaN.
 * FOUR launches whatever count, R and dim are: the chunk sums with the chunk minima and maxima (one workgroup per
 * chunk and four columns), one workgroup per column for mean64, mean, min and max, the chunk sums of squares, and one
 * workgroup per column for std. No atomics; no workgroup waits on another. Stream-ordered and capturable: no
 * allocation, no synchronisation.
 * Workspace: >= mbrl_dataset_stats_workspace_bytes(fields, count) bytes (0 for a bad table; of each field it reads R
 * and dim only), 8-byte aligned; any bytes on entry, no zeroing. It holds the chunk partials and mean64.
 * Before any launch: MBRL_EINVAL for a NULL table, src, rows, output or workspace, a workspace that is not 8-byte
 * aligned, count outside 1 .. 4 or R < 1; MBRL_EUNSUPPORTED for dim outside 1 .. MBRL_EVAL_MAX_DIM (or 2^29 or more
 * chunks x column tiles in a field); MBRL_EWORKSPACE for a workspace that is too small. */
typedef struct {
    const float* src;     /* [S][dim] */
    const int64_t* rows;  /* device [R] */
    int64_t R;
    float* mean;          /* [dim] each */
    float* std;
    float* min;
    float* max;
    int32_t dim;
    int32_t _pad;
} mbrl_stats_field;
size_t mbrl_dataset_stats_workspace_bytes(const mbrl_stats_field* fields, int32_t count);
int mbrl_dataset_stats(const mbrl_stats_field* fields, int32_t count, void* ws, size_t ws_bytes,
                       mbrl_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MBRL_CEM_H */
