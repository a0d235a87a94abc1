// The sharded CEM plan: one plan over the candidates of several GPUs, with an RCCL all-gather of the
// shards' costs as a stream-ordered step of every iteration (mbrl_comm_*, mbrl_cem_plan_sharded). The
// only file that knows RCCL.
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <stdint.h>
#include <string.h>

#include <mutex>
#include <string>

#include <rccl/rccl.h>

#include "mbrl_plan.h"

namespace mbrl {

// Sharded plans: the all-gathered costs arrive rank-major [G][E][Nl]; the selection reads [E][N] with
// candidate r * Nl + j of member e at e * N + r * Nl + j.
__global__ void shard_costs_kernel(const float* __restrict__ gathered, int G, int E, int Nl, float* __restrict__ costs) {
    const size_t total = (size_t)G * E * Nl;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t r = i / ((size_t)E * Nl), rem = i - r * E * Nl, e = rem / Nl, j = rem - e * Nl;
        costs[e * (size_t)G * Nl + r * Nl + j] = gathered[i];
    }
}

}  // namespace mbrl

using namespace mbrl;

extern "C" {

// ---- multi-GPU: an RCCL communicator owned by the library, and the sharded plan as
// one call with the all-gather as a stream-ordered step.
//
// RCCL is resolved at run time, on the first mbrl_comm_* / sharded call (dlopen of librccl.so.1, the
// soname torch.distributed loads, so both share one RCCL in the process): the single-GPU library has
// no link-time dependency on RCCL and loads on a host without it.
struct Rccl {
    const char* (*get_error_string)(ncclResult_t);
    ncclResult_t (*get_unique_id)(ncclUniqueId*);
    ncclResult_t (*comm_init_rank)(ncclComm_t*, int, ncclUniqueId, int);
    ncclResult_t (*comm_destroy)(ncclComm_t);
    ncclResult_t (*all_gather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t);
    ncclResult_t (*group_start)();
    ncclResult_t (*group_end)();
    std::string error;   // why the library could not be loaded ("" when it was)
};

static const Rccl& rccl() {
    static Rccl r{};
    static std::once_flag once;
    std::call_once(once, [] {
        void* h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
        if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
        if (!h) {
            const char* e = dlerror();
            r.error = e ? e : "dlopen(librccl.so.1) failed";
            return;
        }
        auto sym = [&](const char* name) {
            void* p = dlsym(h, name);
            if (!p && r.error.empty()) r.error = std::string("librccl: missing symbol ") + name;
            return p;
        };
        r.get_error_string = reinterpret_cast<decltype(r.get_error_string)>(sym("ncclGetErrorString"));
        r.get_unique_id = reinterpret_cast<decltype(r.get_unique_id)>(sym("ncclGetUniqueId"));
        r.comm_init_rank = reinterpret_cast<decltype(r.comm_init_rank)>(sym("ncclCommInitRank"));
        r.comm_destroy = reinterpret_cast<decltype(r.comm_destroy)>(sym("ncclCommDestroy"));
        r.all_gather = reinterpret_cast<decltype(r.all_gather)>(sym("ncclAllGather"));
        r.group_start = reinterpret_cast<decltype(r.group_start)>(sym("ncclGroupStart"));
        r.group_end = reinterpret_cast<decltype(r.group_end)>(sym("ncclGroupEnd"));
    });
    return r;
}

static int rccl_ready() {
    const Rccl& r = rccl();
    return r.error.empty() ? MBRL_OK : fail(MBRL_EUNSUPPORTED, "RCCL unavailable: %s", r.error.c_str());
}

static int nccl_check(ncclResult_t res, const char* what) {
    if (res == ncclSuccess) return MBRL_OK;
    return fail(MBRL_EHIP, "%s: %s", what, rccl().get_error_string(res));
}

int mbrl_comm_unique_id(void* id_out) {
    static_assert(sizeof(ncclUniqueId) == MBRL_COMM_ID_BYTES, "ncclUniqueId size");
    if (!id_out) return fail(MBRL_EINVAL, "comm_unique_id: NULL");
    if (int rc = rccl_ready()) return rc;
    ncclUniqueId id;
    if (int rc = nccl_check(rccl().get_unique_id(&id), "ncclGetUniqueId")) return rc;
    memcpy(id_out, &id, sizeof(id));
    return MBRL_OK;
}

int mbrl_comm_init(const void* id, int32_t nranks, int32_t rank, mbrl_comm_t* comm_out) {
    if (!id || !comm_out || nranks < 1 || rank < 0 || rank >= nranks)
        return fail(MBRL_EINVAL, "comm_init: bad arguments (nranks %d, rank %d)", nranks, rank);
    if (int rc = rccl_ready()) return rc;
    ncclUniqueId u;
    memcpy(&u, id, sizeof(u));
    ncclComm_t c = nullptr;
    if (int rc = nccl_check(rccl().comm_init_rank(&c, nranks, u, rank), "ncclCommInitRank")) return rc;
    *comm_out = reinterpret_cast<mbrl_comm_t>(c);
    return MBRL_OK;
}

int mbrl_comm_destroy(mbrl_comm_t comm) {
    if (!comm) return MBRL_OK;
    if (int rc = rccl_ready()) return rc;
    return nccl_check(rccl().comm_destroy(reinterpret_cast<ncclComm_t>(comm)), "ncclCommDestroy");
}

struct ShardWs {
    float *local, *gathered, *costs, *actions, *mu[2], *sigma[2], *aelite, *states, *s0;
    float* emu_actions;   // MBRL_OPT_SHARD_EMULATE 1: the other ranks' proposals, one shard at a time (taken
                          // in mode 2 as well, so both modes place emu_kept alike)
    float* emu_kept;      // MBRL_OPT_SHARD_EMULATE: [I][G][E][Nl] every iteration's gathered costs (mode 1
                          // writes them, mode 2 reads the other ranks' slots back)
    unsigned* peer;       // [2G] the ranks' status words, then their pair status words, gathered with the
                          // last iteration's costs
    void* pair;
    TrajScratch traj;     // the trajectory hand-off block; status words [1], [2] are this plan's own
    int64_t* elites;
    uint32_t* keys;
    size_t bytes;
};

static int shard_emulation() { return opt(MBRL_OPT_SHARD_EMULATE); }

static ShardWs shard_ws(const Geometry& g, const mbrl_cem_params* p, int G, void* base) {
    ShardWs w{};
    WsCursor c(base);
    const int Nl = p->N / G;
    const size_t Ha = (size_t)p->H * g.a;
    w.traj = take_traj_scratch(c, g);   // the trajectory hand-off block, status right behind
    w.local = c.take<float>((size_t)g.E * Nl * 4);
    w.gathered = c.take<float>((size_t)g.E * p->N * 4);
    w.costs = c.take<float>((size_t)g.E * p->N * 4);
    w.actions = c.take<float>((size_t)p->H * Nl * g.a * 4);
    w.mu[0] = c.take<float>(Ha * 4); w.mu[1] = c.take<float>(Ha * 4);
    w.sigma[0] = c.take<float>(Ha * 4); w.sigma[1] = c.take<float>(Ha * 4);
    w.aelite = c.take<float>((size_t)p->H * p->K * g.a * 4);
    w.states = c.take<float>((size_t)g.E * p->H * g.s * 4);
    w.elites = c.take<int64_t>((size_t)p->K * 8);
    w.keys = c.take<uint32_t>((size_t)p->N * 4);
    w.s0 = c.take<float>((size_t)g.s * 4);
    w.pair = c.take<char>(pair_area_bytes(g, Nl));
    w.peer = c.take<unsigned>((size_t)2 * G * 4);
    const int emu = shard_emulation();
    w.emu_actions = c.take<float>(emu != 0 && G > 1 ? (size_t)p->H * Nl * g.a * 4 : 0);
    w.emu_kept = c.take<float>(emu != 0 && G > 1 ? (size_t)p->iterations * g.E * p->N * 4 : 0);
    w.bytes = c.off;
    return w;
}

size_t mbrl_cem_plan_sharded_workspace_bytes(const mbrl_mlp_shape* shape, const mbrl_cem_params* params,
                                             int32_t nranks) {
    Geometry g;
    if (shape_geometry(shape, &g) != MBRL_OK || !params || nranks < 1 || params->N % nranks) return 0;
    return shard_ws(g, params, nranks, nullptr).bytes;
}

// The body of mbrl_cem_plan_sharded. Every check that can reject the call runs before the first
// collective, and each is a function of arguments every rank passes alike (shape, params, nranks,
// the workspace size the same query gives), so the ranks agree on it; what can still fail later is a
// HIP launch, and then the rank keeps its place in every remaining all-gather (below).
static int plan_sharded_body(const mbrl_mlp_shape* shape, const void* packed, const mbrl_norm* norm,
                             const mbrl_cost* cost, const float* s0_in, const mbrl_cem_params* p, mbrl_comm_t comm,
                             int32_t nranks, int32_t rank, float* mu, float* sigma, float* actions_out,
                             float* states_out, float* cost_hist, float* returns_hist, int64_t* elite_hist,
                             mbrl_event_t* rollout_events, void* workspace, size_t ws_bytes, hipStream_t stream,
                             bool allow_pairs = true) {
    Geometry g;
    int rc = shape_geometry(shape, &g);
    if (rc) return rc;
    // comm == NULL with MBRL_OPT_SHARD_EMULATE (tests, timing): this call fills the rank-major buffer the
    // all-gather would have delivered itself (mode 1: every other rank's shard rolled out here; mode 2:
    // the other ranks' costs a mode-1 plan kept)
    const int emu_mode = comm == nullptr ? shard_emulation() : 0;
    const bool emulate = emu_mode != 0;
    if (!p || (!comm && !emulate)) return fail(MBRL_EINVAL, "plan_sharded: NULL params or comm");
    if ((rc = cem_params_check(p))) return rc;
    if (nranks < 1 || rank < 0 || rank >= nranks || p->N % nranks)
        return fail(MBRL_EINVAL, "plan_sharded: N=%d over %d ranks (rank %d)", p->N, nranks, rank);
    if (!actions_out || !states_out || !workspace || !s0_in || !packed)
        return fail(MBRL_EINVAL, "plan_sharded: packed/s0/actions_out/states_out/workspace NULL");
    const ShardWs w = shard_ws(g, p, nranks, workspace);
    if (ws_bytes < w.bytes) return fail(MBRL_EWORKSPACE, "workspace %zu < %zu", ws_bytes, w.bytes);
    if (emulate && nranks > 1 && !w.emu_kept)
        return fail(MBRL_EINVAL, "plan_sharded: the workspace was sized without MBRL_OPT_SHARD_EMULATE");
    if ((rc = pair_forced_check(g, p->N / nranks))) return rc;
    if ((rc = rollout_validate(g, norm, cost))) return rc;
    if (!emulate && (rc = rccl_ready())) return rc;
    const int N = p->N, Nl = N / nranks, H = p->H, a = g.a, E = g.E;
    const int off = rank * Nl;   // this rank's global candidates [off, off + Nl)
    const size_t slot = (size_t)E * Nl;   // one rank's floats in the gathered buffer
    const FusePlan f = fuse_plan(N, Nl, p->K, a);   // selected from all N, drawn per shard
    const bool fuse = f.fuse, fuse_draw = f.fuse_draw;
    // injected failure (tests): iteration fail_it on rank fail_rank (the calling rank unless one is named)
    const int fail_it = opt(MBRL_OPT_DEBUG_SHARD_FAIL) - 1;
    const int fail_opt = opt(MBRL_OPT_DEBUG_SHARD_FAIL_RANK);
    const int fail_rank = fail_opt == 0 ? rank : fail_opt - 1;
    // From here on the ranks must issue the same collectives: a launch that fails on this rank does not
    // end the call. Its remaining compute launches are skipped, but it still joins every remaining
    // all-gather -- with its local costs poisoned to NaN (all bits set) and its status word set, which
    // the last iteration's all-gather hands to every peer -- and the first error is returned at the
    // end. (An abort of the communicator would not help: ncclCommAbort acts on the calling rank only,
    // and peers already inside an all-gather would wait on it.)
    int err = MBRL_OK;
    std::string err_msg;
    auto step = [&](int r) {
        if (r != MBRL_OK && err == MBRL_OK) {
            err = r;
            err_msg = mbrl_last_error();
        }
        return err == MBRL_OK;
    };
    unsigned* own_status = w.traj.status + 1;   // [0] is the trajectory kernel's; zeroed with it below
    unsigned* zero_word = w.traj.status + 2;    // stays 0: the pair status gathered when no pair launch ran
    // With peers the plan checks its column-split pair launches once, after the plan (the pair status
    // word, gathered with the last iteration's costs): any hand-off that timed out on any rank sends
    // every rank through the whole plan again without pairs. No gated redo launch per iteration.
    void* const pair_ws = allow_pairs ? w.pair : nullptr;
    const unsigned* pair_status = nullptr;
    const unsigned** const defer = nranks > 1 ? &pair_status : nullptr;
    // one first launch: distribution rows, the workspace copy of s0, iteration 0's proposals of this
    // shard (global candidates [off, off + Nl)), the hand-off words and this rank's status zeroed
    const InitZero z = plan_zero(g, Nl, w.pair, w.traj);
    if (!z.ptr[1]) step(hip_check(hipMemsetAsync(own_status, 0, 2 * sizeof(unsigned), stream), "status memset"));
    launch_cem_init(dim3(H * (fuse_draw ? draw_slices(H, 1, Nl, a) : 1), 1), stream, p->seed, p->init_mu, p->init_sigma,
                    p->lo, p->hi, H, a, Nl, w.mu[0], w.sigma[0], fuse_draw ? w.actions : nullptr, s0_in, g.s, w.s0, off, z,
                    nullptr);
    step(hip_check(hipGetLastError(), "init launch"));
    if (!fuse_draw && err == MBRL_OK) {
        const mbrl_sampler sp0 = make_sampler(p, 0, w.mu[0], w.sigma[0]);
        step(sample_impl(&sp0, H, a, Nl, off, w.actions, stream));
    }
    bool poisoned = false;   // this rank's local costs and status word carry its failure
    unsigned pair_epoch = 0;
    int cur = 0;
    for (int it = 0; it < p->iterations; ++it) {
        const bool last = it + 1 == p->iterations;
        const mbrl_sampler sp = make_sampler(p, it, w.mu[cur], w.sigma[cur]);
        if (err == MBRL_OK) step(record_rollout_event(rollout_events, 2 * it, stream));
        if (err == MBRL_OK)
            step(rollout_impl(g, packed, norm, cost, w.s0, 0, w.actions, nullptr, Nl, H, 0, w.local, nullptr, nullptr,
                              stream, pair_area_bytes(g, Nl) ? pair_ws : nullptr, z.ptr[0] ? &pair_epoch : nullptr,
                              defer));
        if (err == MBRL_OK && it == fail_it && fail_rank == rank)
            step(fail(MBRL_EHIP, "plan_sharded: injected launch failure at iteration %d (MBRL_OPT_DEBUG_SHARD_FAIL)", it));
        if (err == MBRL_OK) step(record_rollout_event(rollout_events, 2 * it + 1, stream));
        if (err != MBRL_OK && !poisoned) {
            // NaN costs sort last on every rank (MBRL_NAN_LAST); the status word tells the peers. If even
            // these fail the rank still joins the collectives (and returns its first error).
            poisoned = true;
            const int m1 = hip_check(hipMemsetAsync(w.local, 0xFF, slot * 4, stream), "poison memset");
            const int m2 = hip_check(hipMemsetAsync(own_status, 0x01, sizeof(unsigned), stream), "status memset");
            if (m1 || m2) err_msg += std::string("; then ") + mbrl_last_error();
        }
        // the one collective of an iteration: every rank's [E][Nl] costs, rank-major; the last one also
        // gathers the ranks' status words (grouped: one RCCL launch)
        if (!emulate) {
            const Rccl& R = rccl();
            ncclComm_t c = reinterpret_cast<ncclComm_t>(comm);
            if (last) step(nccl_check(R.group_start(), "ncclGroupStart"));
            step(nccl_check(R.all_gather(w.local, w.gathered, slot, ncclFloat, c, stream), "ncclAllGather"));
            if (last) {
                step(nccl_check(R.all_gather(own_status, w.peer, 1, ncclUint32, c, stream), "ncclAllGather status"));
                step(nccl_check(R.all_gather(pair_status ? pair_status : zero_word, w.peer + nranks, 1, ncclUint32, c,
                                             stream), "ncclAllGather pair status"));
                step(nccl_check(R.group_end(), "ncclGroupEnd"));
            }
        } else if (err == MBRL_OK && nranks == 1) {
            step(hip_check(hipMemcpyAsync(w.gathered, w.local, slot * 4, hipMemcpyDeviceToDevice, stream), "gather"));
            if (last) step(hip_check(hipMemcpyAsync(w.peer, own_status, 4, hipMemcpyDeviceToDevice, stream), "status"));
        } else if (err == MBRL_OK && emu_mode == 2) {
            float* kept = w.emu_kept + (size_t)it * nranks * slot;
            launch_emu_gather(w.local, kept, nranks, rank, slot, own_status, pair_status, w.gathered, w.peer, stream);
            step(hip_check(hipGetLastError(), "emulated gather"));
        } else if (err == MBRL_OK) {
            // rank r's slot: its proposals of this iteration (drawn at its global offset from this
            // iteration's mu / sigma, as its own previous update or initial draw made them) rolled out
            for (int r = 0; r < nranks && err == MBRL_OK; ++r) {
                float* sl = w.gathered + (size_t)r * slot;
                if (r == rank) {
                    step(hip_check(hipMemcpyAsync(sl, w.local, slot * 4, hipMemcpyDeviceToDevice, stream),
                                   "emulated gather"));
                } else if (fail_rank == r && fail_it >= 0 && it >= fail_it) {   // an emulated peer's failure
                    step(hip_check(hipMemsetAsync(sl, 0xFF, slot * 4, stream), "emulated peer poison"));
                } else if (step(sample_impl(&sp, H, a, Nl, r * Nl, w.emu_actions, stream))) {
                    step(rollout_impl(g, packed, norm, cost, w.s0, 0, w.emu_actions, nullptr, Nl, H, 0, sl, nullptr,
                                      nullptr, stream, pair_area_bytes(g, Nl) ? pair_ws : nullptr,
                                      z.ptr[0] ? &pair_epoch : nullptr));
                }
            }
            if (last && err == MBRL_OK) {
                step(hip_check(hipMemsetAsync(w.peer, 0, (size_t)2 * nranks * 4, stream), "emulated status"));
                if (fail_rank != rank && fail_rank < nranks && fail_it >= 0)
                    step(hip_check(hipMemsetAsync(w.peer + fail_rank, 0x01, 4, stream), "emulated peer status"));
                step(hip_check(hipMemcpyAsync(w.peer + rank, own_status, 4, hipMemcpyDeviceToDevice, stream),
                               "emulated status"));
                if (pair_status)
                    step(hip_check(hipMemcpyAsync(w.peer + nranks + rank, pair_status, 4, hipMemcpyDeviceToDevice,
                                                  stream), "emulated pair status"));
            }
            if (err == MBRL_OK)   // kept for mode 2
                step(hip_check(hipMemcpyAsync(w.emu_kept + (size_t)it * nranks * slot, w.gathered, nranks * slot * 4,
                                              hipMemcpyDeviceToDevice, stream), "emulated keep"));
        }
        if (err != MBRL_OK) continue;   // only the all-gathers remain for this rank
        float* costs = w.gathered;
        if (E > 1 && nranks > 1) {   // (one rank: the identity)
            hipLaunchKernelGGL(shard_costs_kernel, dim3(256), dim3(256), 0, stream, w.gathered, nranks, E, Nl, w.costs);
            costs = w.costs;
        }
        if (cost_hist)
            step(hip_check(hipMemcpyAsync(cost_hist + (size_t)it * E * N, costs, (size_t)E * N * 4,
                                          hipMemcpyDeviceToDevice, stream), "cost record"));
        int64_t* elites = elite_hist ? elite_hist + (size_t)it * p->K : w.elites;
        float* rets = returns_hist ? returns_hist + (size_t)it * N : nullptr;
        if (err != MBRL_OK) continue;
        if (fuse) {
            // (next proposals: this rank's shard of iteration it + 1)
            UpdateArgs U = make_update_args(g, p, it, costs, w.mu[cur], w.sigma[cur], w.mu[cur ^ 1], w.sigma[cur ^ 1], mu,
                                            sigma, actions_out, fuse_draw ? w.actions : nullptr);
            U.elite_out = elites; U.returns_out = rets;
            U.draw_off = off; U.draw_n = Nl;
            U.ael = w.aelite;   // (scratch of the split update)
            step(update_impl(U, 1, stream));
        } else if (step(select_impl(costs, E, N, p->K, MBRL_NAN_LAST, elites, rets, w.keys, align256((size_t)N * 4),
                                    stream))) {
            step(refit_impl(&sp, H, a, elites, p->K, p->alpha, w.aelite, w.mu[cur ^ 1], w.sigma[cur ^ 1], stream,
                            last ? mu : nullptr, last ? sigma : nullptr, last ? actions_out : nullptr));
        }
        cur ^= 1;
        if (!last && !fuse_draw && err == MBRL_OK) {
            mbrl_sampler sn = sp;
            sn.iteration = it + 1; sn.mu = w.mu[cur]; sn.sigma = w.sigma[cur];
            step(sample_impl(&sn, H, a, Nl, off, w.actions, stream));
        }
    }
    if (err != MBRL_OK) return fail(err, "%s (this rank still joined every all-gather of the plan)", err_msg.c_str());
    // the final mean's states, on every rank (the same on each)
    rc = final_trajectory(g, packed, norm, w.s0, actions_out, H, states_out, w.states, w.traj, stream,
                          z.ptr[1] != nullptr);
    if (rc) return rc;
    if ((rc = hip_check(hipGetLastError(), "sharded plan launch"))) return rc;
    if (nranks == 1) return MBRL_OK;   // no peers: enqueue only, as mbrl_cem_plan
    // the peers' status and pair status words (gathered with the last iteration's costs): one copy
    // behind the plan's last launch and one stream synchronisation
    static thread_local unsigned* peer_host = nullptr;
    static thread_local int peer_cap = 0;
    if (peer_cap < 2 * nranks) {
        if (peer_host) (void)hipHostFree(peer_host);
        peer_host = nullptr;
        peer_cap = 0;
        if ((rc = hip_check(hipHostMalloc(reinterpret_cast<void**>(&peer_host), (size_t)2 * nranks * 4),
                            "hipHostMalloc")))
            return rc;
        peer_cap = 2 * nranks;
    }
    if ((rc = hip_check(hipMemcpyAsync(peer_host, w.peer, (size_t)2 * nranks * 4, hipMemcpyDeviceToHost, stream),
                        "peer status copy")))
        return rc;
    if ((rc = hip_check(hipStreamSynchronize(stream), "plan synchronise"))) return rc;
    std::string failed;
    bool pair_timeout = false;
    for (int r = 0; r < nranks; ++r) {
        if (peer_host[r] && r != rank) failed += (failed.empty() ? "" : ", ") + std::to_string(r);
        if (peer_host[nranks + r]) pair_timeout = true;
    }
    if (!failed.empty())
        return fail(MBRL_EPEER, "plan_sharded: rank(s) %s failed during this plan (each returns its own error); "
                                "this rank's outputs are void", failed.c_str());
    // a column-split hand-off timed out on some rank (its tile's costs were invalid): every rank sees
    // the same gathered words, so every rank runs the plan again, without pairs (same bits)
    if (pair_timeout && allow_pairs)
        return plan_sharded_body(shape, packed, norm, cost, s0_in, p, comm, nranks, rank, mu, sigma, actions_out,
                                 states_out, cost_hist, returns_hist, elite_hist, rollout_events, workspace, ws_bytes,
                                 stream, false);
    return MBRL_OK;
}

int mbrl_cem_plan_sharded(const mbrl_mlp_shape* shape, const void* packed, const mbrl_norm* norm,
                          const mbrl_cost* cost, const float* s0_in, const mbrl_cem_params* p, mbrl_comm_t comm,
                          int32_t nranks, int32_t rank, float* mu, float* sigma, float* actions_out,
                          float* states_out, float* cost_hist, float* returns_hist, int64_t* elite_hist,
                          mbrl_event_t* rollout_events, void* workspace, size_t ws_bytes, mbrl_stream_t stream) {
    return plan_sharded_body(shape, packed, norm, cost, s0_in, p, comm, nranks, rank, mu, sigma, actions_out,
                             states_out, cost_hist, returns_hist, elite_hist, rollout_events, workspace, ws_bytes,
                             reinterpret_cast<hipStream_t>(stream));
}

}  // extern "C"
