// What the plan loops share (plan.hip defines it; plan_sharded.hip is the other user): the host
// dispatch of the rollout and trajectory kernels, the workspace cursor, and the steps every plan
// repeats per iteration.
#pragma once
#include "mbrl_host.h"

namespace mbrl {

// Carves a workspace front to back, every block 256-byte aligned. base NULL: sizing only (off).
struct WsCursor {
    char* base;
    size_t off;
    explicit WsCursor(void* b) : base(static_cast<char*>(b)), off(0) {}
    template <typename T>
    T* take(size_t bytes) {
        T* r = base ? reinterpret_cast<T*>(base + off) : nullptr;
        off += align256(bytes);
        return r;
    }
};

// The trajectory kernel's hand-off granules with its status word right behind them (one zeroed
// block: plan_zero relies on the adjacency).
struct TrajScratch {
    unsigned long long* xchg;
    unsigned* status;
    size_t xchg_bytes;
};
TrajScratch take_traj_scratch(WsCursor& c, const Geometry& g);

// Column-split pair exchange area a plan workspace reserves for N candidates (0: pairs not offered).
size_t pair_area_bytes(const Geometry& g, int N);
// MBRL_OPT_ROLLOUT_PAIR = 1 on a plan whose shape or size has no pair area: an error, not a fallback.
int pair_forced_check(const Geometry& g, int N);
// The hand-off words a plan's first launch zeroes: ptr[0] the pair flags, ptr[1] the trajectory scratch.
InitZero plan_zero(const Geometry& g, int Nl, void* pair, const TrajScratch& ts);

int rollout_validate(const Geometry& g, const mbrl_norm* norm, const mbrl_cost* cost);
int rollout_impl(const Geometry& g, const void* packed, const mbrl_norm* norm, const mbrl_cost* cost, const float* s0,
                 int s0_per_cand, const float* actions, const mbrl_sampler* sampler, int N, int H, int n_offset,
                 float* costs, float* actions_out, float* states_out, hipStream_t stream, void* pair_area = nullptr,
                 unsigned* pair_epoch = nullptr, const unsigned** pair_status_out = nullptr);

// The same "bad CEM params" check and message for every CEM plan (p non-NULL).
int cem_params_check(const mbrl_cem_params* p);

// Launches per iteration: rollout + one fused update (select, refit, next proposals) where it fits
// (fuse; fuse_draw: the update also draws the next proposals); else the proposal draw, rollout, select
// and refit as separate launches. N_select candidates are selected from, N_draw drawn per launch (they
// differ in a sharded plan).
struct FusePlan {
    bool fuse, fuse_draw;
};
FusePlan fuse_plan(int N_select, int N_draw, int K, int a);

// Iteration `it`'s proposal distribution (P: mbrl_cem_params or mbrl_mppi_params).
template <typename P>
inline mbrl_sampler make_sampler(const P* p, int it, const float* mu, const float* sigma) {
    mbrl_sampler sp{};
    sp.seed = p->seed; sp.iteration = it; sp.mu = mu; sp.sigma = sigma; sp.lo = p->lo; sp.hi = p->hi;
    return sp;
}

// Records events[idx] on the stream where the caller gave one (events or the entry may be NULL).
int record_rollout_event(mbrl_event_t* events, int idx, hipStream_t stream);

// Iteration `it`'s fused update of one plan over p->N candidates: the refit of (mu_cur, sigma_cur) into
// (mu_next, sigma_next); the last iteration also writes the plan outputs fin_*; every other one draws
// the next proposals into next_actions (NULL: the draw is not fused). The caller sets what differs:
// member_stride, draw_off / draw_n, elite_out / returns_out, ael.
UpdateArgs make_update_args(const Geometry& g, const mbrl_cem_params* p, int it, const float* costs,
                            const float* mu_cur, const float* sigma_cur, float* mu_next, float* sigma_next,
                            float* fin_mu, float* fin_sigma, float* fin_actions, float* next_actions);

// The final mean's predicted states: traj_impl into states_out (E == 1) or member_scratch ([E][H][s],
// then their member mean into states_out). member_out (mbrl_trajectory): the caller wants the members'
// states; they go there whatever E. Leaves the last launch's error to the caller's hipGetLastError.
int final_trajectory(const Geometry& g, const void* packed, const mbrl_norm* norm, const float* s0,
                     const float* actions, int H, float* states_out, float* member_scratch, const TrajScratch& ts,
                     hipStream_t stream, int prezeroed, float* member_out = nullptr);

// A sampled-rollout source for the receding-horizon loop (rollout_ts.hip): the checked launch arguments of
// mbrl_rollout_cost_ts_rows and its row count Q. ts_source_rollout runs iteration `it`'s launch over BN candidates
// with per-candidate start states (candidate n has Philox index n: problem b's are b N + n) into costs [Q][BN].
struct TsLaunch;
struct TsSource {
    const TsLaunch* launch;
    int Q;
};
int ts_source_rollout(const TsSource& ts, const float* s0, const float* actions, int BN, int it, float* costs,
                      hipStream_t stream);

// One receding-horizon entry's arguments. The single entries: B = 1, no flags; the batched ones: no events;
// the white ones (and a mixed one called without a mix): mix NULL. ts (NULL: none): the sampled-rollout source of
// mbrl_cem_plan_ts_rh / mbrl_cem_plan_ts_rh_batch -- no events, no mix, Q cost rows.
struct RhCall {
    const char* name;   // the entry, for the messages
    bool batched;       // mbrl_cem_plan_rh_batch's layouts, and s0 checked with the other pointers
    const mbrl_mlp_shape* shape;
    const void* packed;
    const mbrl_norm* norm;
    const mbrl_cost* cost;
    const float* s0;
    int B;
    const mbrl_cem_rh_params* rp;
    const float *mu_rows, *sigma_rows, *carry_in;
    const int32_t* flags;
    const float* mix;
    float *mu, *sigma, *actions_out, *states_out, *carry_out, *carry_returns_out, *cost_hist, *returns_hist;
    int64_t* elite_hist;
    float* kept_hist;
    mbrl_event_t* events;
    void* workspace;
    size_t ws_bytes;
    mbrl_stream_t stream;
    const TsSource* ts = nullptr;
};

// The receding-horizon entries' one body (plan.hip): every check, then the loop. rh_ts_workspace_bytes: what a
// call with a source of Q rows demands (0 for a bad shape, bad params or B < 1).
int rh_plan(const RhCall& c);
size_t rh_ts_workspace_bytes(const mbrl_mlp_shape* shape, const mbrl_cem_rh_params* rp, int Q, int B);

}  // namespace mbrl
