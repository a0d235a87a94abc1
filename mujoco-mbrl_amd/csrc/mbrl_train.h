// What the training translation units (train.hip, train_fused.hip, train_api.hip) share and nobody else needs.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mbrl_internal.h"

namespace mbrl {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// Diagnostic build only (-DMBRL_STAMPS): s_memrealtime (100 MHz) at fixed points of the first and
// the last workgroup of each launch, 8 slots per launch, into the buffer set by
// mbrl_diag_set_train_stamps() (tools/train_stamps.py). Without relocatable device code a __device__
// global belongs to one translation unit: each file that stamps defines its own g_train_stamps and a
// setter, and mbrl_diag_set_train_stamps() (train_api.hip) calls both.
#ifdef MBRL_STAMPS
hipError_t train_gemm_set_stamps(void* buf);    // train.hip
hipError_t train_fused_set_stamps(void* buf);   // train_fused.hip
#define TSTAMP(k)                                                                                   \
    do {                                                                                             \
        const unsigned probe_ = L.nd > 1 ? (unsigned)L.d[0].tiles : gridDim.x - 1;                 \
        if (g_train_stamps && threadIdx.x == 0 && blockIdx.y == 0 && (blockIdx.x == 0 || blockIdx.x == probe_)) \
            g_train_stamps[L.slot * 8 + (blockIdx.x == 0 ? 0 : 4) + (k)] = __builtin_amdgcn_s_memrealtime(); \
    } while (0)
// the fused kernels: slot `slot_`, first workgroup and the last
#define FSTAMP(slot_, k)                                                                             \
    do {                                                                                             \
        if (g_train_stamps && threadIdx.x == 0 && (blockIdx.x == 0 || blockIdx.x == gridDim.x - 1)) \
            g_train_stamps[(slot_) * 8 + (blockIdx.x == 0 ? 0 : 4) + (k)] = __builtin_amdgcn_s_memrealtime(); \
    } while (0)
#else
#define TSTAMP(k) \
    do {          \
    } while (0)
#define FSTAMP(slot_, k) \
    do {                 \
    } while (0)
#endif

constexpr int TT = 32;              // C tile edge
constexpr int FUSED_WMAX = 512;    // H_0 rows of the tile in LDS: 32 x (W + 4) floats
constexpr int FUSED_K0MAX = 64;    // s + a: one 16-deep chunk per wave of the layer-0 launch's split
// The fused step needs the dW_0 fold, whose 32-row waves bound its rows: R <= 512, 16 bands of 32.
constexpr int FUSED_MAX_BANDS = 16;

// p[0] + p[stride] + ... + p[(n - 1) stride], summed in index order like a plain loop, with the loads
// of each 16 terms in flight together (a loop that loads one term per iteration pays the memory
// latency n times: ~10 us for the 16 row tiles of a bias gradient). SC1: agent-scope (sc1) loads.
template <bool SC1>
__device__ __forceinline__ float ordered_sum(const float* p, int64_t stride, int n) {
    float g = 0.0f;
    for (int i0 = 0; i0 < n; i0 += 16) {
        float t[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const float* a = p + (int64_t)(i0 + u) * stride;
            t[u] = i0 + u >= n ? 0.0f
                   : SC1       ? __hip_atomic_load(a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                               : *a;
        }
#pragma unroll
        for (int u = 0; u < 16; ++u)
            if (i0 + u < n) g = i0 + u == 0 ? t[u] : g + t[u];
    }
    return g;
}

struct FusedArgs {
    const int64_t* idx;
    const float *gs, *ga, *gns, *grw;   // stacked transitions (GemmLaunch's meaning)
    int H, s, a;
    int R, W, K0, J, tiles_n, tiles_r;
    int nwb;                            // waves of the separate backward launches (K = R): the dH_1 split
    const float *w0, *b0, *w1, *b1;
    const float *wo, *wo_r, *bo, *bo_r; // output layer: state rows from wo / bo, the reward row from *_r
    float *act0, *act1, *xstore;
    float* tgt;                         // [R][J] the batch's targets, gathered by F's first column tiles for O
    int pre_rows;                       // 1: xstore / tgt already hold this batch (the previous F gathered it)
    const int64_t* idx_next;            // non-NULL: F's second column tiles gather the next batch's rows
    int R_next;                         //   (R_next of them) into xnext / tnext
    float *xnext, *tnext;
    float *dh1, *cs_dh1, *cs_dy, *loss_part, *out_part;
    float *dwo, *dwo_r, *dbo, *dbo_r;
    unsigned* out_ticket;               // [tiles_n] arrivals per column block of dH_1 tiles (O)
    float* db1;                         // O's last arrivers: db_1 from dH_1's column sums (+ b_1's Adam step)
    int adam;
    mbrl_adam_tensor ab1;
    mbrl_adam_hparams hp;
    int arith;
    unsigned* zero_words;               // F's workgroup 0 zeroes zero_n words (the tickets of later launches)
    int zero_n;
    unsigned* serial;                   // F's workgroup 0 raises the step's serial (B's granule tag)
    float scale_s, scale_r, inv_s, inv_r;
    // F and O in one launch (train_fused_fo_kernel): per 32-row band of the batch a counter (own 128-B
    // line) that the band's F tiles add to once their H_1 columns are written through; each O tile
    // waits for all tiles_n, then adds again, and the last add of the band resets it (zero between
    // launches, as the caller's once-zeroed workspace starts). status: bit 0 = a bounded wait timed out.
    unsigned* band;
    unsigned* status;
};
// F and O for a filled FusedArgs (train_fused.hip): one launch, or two with fo_split (MBRL_OPT_TRAIN_FO = 1).
hipError_t launch_train_fused(const FusedArgs& F, bool fo_split, hipStream_t stream);

// ---- the entries' checks (train_api.hip), one copy for one model, for ensembles and for every loss kind
// The ensemble entries' loss: the teacher-forced MSE of mbrl_train_grads (the tiled launches of train.hip), the
// open-loop MSE (train_open_loop.hip) and the Gaussian negative log-likelihood (train_nll.hip).
enum TrainLoss { LOSS_ONE_STEP = 0, LOSS_OPEN_LOOP = 1, LOSS_NLL = 2 };
// The transitions' pointers a model of shape t reads.
bool train_data_ok(const mbrl_train_data* data, const TrainShape& t);
// The members' common shape in the layout the ensemble launches run: the multi-launch one, the layer-0
// weight gradient in its own launch (the only layout without a wait between workgroups). LOSS_OPEN_LOOP and
// LOSS_NLL: the kind's envelope (ol_envelope, nll_envelope) after the member comparison, and no launch option
// read; LOSS_NLL: a reward head is MBRL_EINVAL.
int ensemble_shape(const char* what, const mbrl_train_model* members, int32_t E, TrainLoss kind, TrainShape* t);
// NULL layers, and no parameter or gradient buffer bound twice (two members stepping one buffer would race)
int ensemble_members(const char* what, const mbrl_train_model* members, int32_t E, const TrainShape& t);
// One batch of an ensemble epoch: n transitions per member from rows idx (member e's idx_stride rows on), in a
// workspace laid out for batches of up to bs. bounds: LOSS_NLL's log-variance bounds, NULL for the other kinds.
typedef hipError_t (*EnsembleBatch)(const TrainShape& t, const mbrl_train_model* members, int E,
                                    const mbrl_train_data* data, const int64_t* idx, int64_t idx_stride, int bs, int n,
                                    float* loss_out, float* ws, const mbrl_nll_bounds* bounds, hipStream_t stream);
// The six ensemble epoch entries (mbrl_cem.h's arguments): the checks, then per batch `launch`, the Adam table's
// refresh and the members' Adam launch -- or, clipped, the norm launches and the clipped Adam launch.
int train_epoch_members(const char* what, TrainLoss kind, bool clipped, EnsembleBatch launch,
                        const mbrl_train_model* members, int32_t E, const mbrl_train_data* data, const int64_t* orders,
                        int64_t rows, int32_t batch_size, const mbrl_adam_tensor* tensors, int32_t count,
                        const mbrl_adam_hparams* hparams, const float* step_sizes, const float* bc2_sqrt, float* losses,
                        void* workspace, size_t ws_bytes, const mbrl_grad_clip* clip, const mbrl_nll_bounds* bounds,
                        mbrl_stream_t stream);
// The open-loop kind's own checks and workspace (train_open_loop.hip): the shape envelope, E * batch * horizon
// below 2^31, the floats for E members of `batch` transitions.
int ol_envelope(const char* what, const TrainShape& t);
int ol_batch_ok(const char* what, int32_t E, int64_t batch, const TrainShape& t);
size_t ol_ws_floats(const TrainShape& t, int E, int batch);
// The same for the Gaussian NLL (train_nll.hip); nll_bounds_ok: the bounds struct and both of its arrays.
int nll_envelope(const char* what, const TrainShape& t);
size_t nll_ws_floats(const TrainShape& t, int E, int batch);
bool nll_bounds_ok(const mbrl_nll_bounds* bounds);

}  // namespace mbrl
