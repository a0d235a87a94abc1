// The model-training optimizer step: torch.optim.Adam's step for fp32
// parameter groups as ONE launch over every tensor of the group (include/mbrl_cem.h
// mbrl_adam_step).
//
// torch.optim.Adam (foreach path, capturable = False: the default for CUDA/HIP parameters, and what
// the reference's experiment.py:55-62 builds) runs a chain of multi-tensor kernels per step, each a
// full pass over the group's state: lerp_ (exp_avg), mul_ + addcmul_ (exp_avg_sq), sqrt, div_,
// add_ (denominator), addcdiv_ (param) -- plus an add for weight decay. Every one of those rounds to
// fp32 once per element. This kernel applies the same element-wise chain with the same roundings in
// one pass (param, grad, exp_avg, exp_avg_sq read once, three arrays written once), so the
// parameters and optimizer state it leaves are bit-identical to torch's: the file is built with
// -ffp-contract=off and every fused multiply-add torch's own build forms is spelled out as fmaf()
// (AdamArith; pinned on the MI355X by tests/test_gpu_train_adam.py against torch.optim.Adam).
// Per-tensor scalars (bias corrections of that tensor's step count) come from the host, computed
// in double exactly as adam.py does and rounded to float as the multi-tensor kernels round them.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mbrl_adam_dev.h"
#include "mbrl_host.h"

namespace mbrl {

constexpr int ADAM_THREADS = 256;
constexpr int ADAM_CHUNK = ADAM_THREADS * 4;   // elements per workgroup (one float4 per lane)

// CAP tensors per launch: ADAM_MAX_TENSORS for one model's group; ADAM_ENS_TENSORS for an ensemble's
// members together (mbrl_train_epoch_ensemble), the most a launch's argument block holds.
template <int CAP>
struct AdamLaunchT {
    mbrl_adam_tensor t[CAP];
    int first_block[CAP + 1];                   // workgroup prefix over the tensors' chunks
    int count;
    mbrl_adam_hparams hp;
    int arith;                                  // AdamArith bits
};
using AdamLaunch = AdamLaunchT<ADAM_MAX_TENSORS>;
constexpr int ADAM_ENS_TENSORS = 64;

// One workgroup's chunk of one tensor. CLIP (mbrl_adam_step_clipped): the gradient is first scaled by its member's
// clipping coefficient coef[member[slot]], one rounded product per element; without it neither pointer is read.
template <int CAP, bool CLIP>
__device__ __forceinline__ void adam_step_body(const AdamLaunchT<CAP>& L, const float* coef, const uint8_t* member) {
    const int blk = blockIdx.x;
    int ti = 0;
    while (ti + 1 < L.count && blk >= L.first_block[ti + 1]) ++ti;
    const mbrl_adam_tensor& T = L.t[ti];
    const int64_t base = (int64_t)(blk - L.first_block[ti]) * ADAM_CHUNK;
    const int64_t i0 = base + 4 * (int64_t)threadIdx.x;
    if (i0 >= T.numel) return;
    const float ss = T.step_size, bc2 = T.bc2_sqrt;
    float c = 1.0f;
    if constexpr (CLIP) c = coef[member[ti]];
    const bool vec = i0 + 4 <= T.numel &&
                     ((reinterpret_cast<uintptr_t>(T.param) | reinterpret_cast<uintptr_t>(T.grad) |
                       reinterpret_cast<uintptr_t>(T.exp_avg) | reinterpret_cast<uintptr_t>(T.exp_avg_sq)) & 15) == 0;
    if (vec) {
        float4 p = *reinterpret_cast<const float4*>(T.param + i0);
        float4 g = *reinterpret_cast<const float4*>(T.grad + i0);
        float4 m = *reinterpret_cast<const float4*>(T.exp_avg + i0);
        float4 v = *reinterpret_cast<const float4*>(T.exp_avg_sq + i0);
        if constexpr (CLIP) { g.x = g.x * c; g.y = g.y * c; g.z = g.z * c; g.w = g.w * c; }
        adam_element(p.x, g.x, m.x, v.x, ss, bc2, L.hp, L.arith);
        adam_element(p.y, g.y, m.y, v.y, ss, bc2, L.hp, L.arith);
        adam_element(p.z, g.z, m.z, v.z, ss, bc2, L.hp, L.arith);
        adam_element(p.w, g.w, m.w, v.w, ss, bc2, L.hp, L.arith);
        *reinterpret_cast<float4*>(T.param + i0) = p;
        *reinterpret_cast<float4*>(T.exp_avg + i0) = m;
        *reinterpret_cast<float4*>(T.exp_avg_sq + i0) = v;
        return;
    }
    for (int64_t i = i0; i < i0 + 4 && i < T.numel; ++i) {
        float p = T.param[i], m = T.exp_avg[i], v = T.exp_avg_sq[i];
        float g = T.grad[i];
        if constexpr (CLIP) g = g * c;
        adam_element(p, g, m, v, ss, bc2, L.hp, L.arith);
        T.param[i] = p;
        T.exp_avg[i] = m;
        T.exp_avg_sq[i] = v;
    }
}

template <int CAP>
__global__ __launch_bounds__(ADAM_THREADS) void adam_step_kernel(const AdamLaunchT<CAP> L) {
    adam_step_body<CAP, false>(L, nullptr, nullptr);
}

// The ensemble launch with each tensor's member index and the members' device-side coefficients coef[E].
struct AdamClipLaunch {
    AdamLaunchT<ADAM_ENS_TENSORS> a;
    const float* coef;
    uint8_t member[ADAM_ENS_TENSORS];
};
__global__ __launch_bounds__(ADAM_THREADS) void adam_step_clipped_kernel(const AdamClipLaunch L) {
    adam_step_body<ADAM_ENS_TENSORS, true>(L.a, L.coef, L.member);
}

// Fills A with up to CAP non-empty tensors at a time (first_block: the workgroup prefix over their chunks) and calls
// fire(blocks) when the table is full or the tensors are exhausted; tag(slot, i) notes tensor i's slot in the table.
template <int CAP, class Tag, class Fire>
static hipError_t adam_table_walk(AdamLaunchT<CAP>& A, const mbrl_adam_tensor* tensors, int count, Tag tag, Fire fire) {
    int blocks = 0;
    for (int i = 0; i <= count; ++i) {
        if (A.count == CAP || (i == count && A.count > 0)) {
            A.first_block[A.count] = blocks;
            fire(blocks);
            const hipError_t e = hipGetLastError();
            if (e != hipSuccess) return e;
            A.count = 0;
            blocks = 0;
        }
        if (i == count || tensors[i].numel <= 0) continue;
        A.t[A.count] = tensors[i];
        tag(A.count, i);
        A.first_block[A.count] = blocks;
        blocks += (int)((tensors[i].numel + ADAM_CHUNK - 1) / ADAM_CHUNK);
        ++A.count;
    }
    return hipSuccess;
}

template <int CAP>
static hipError_t launch_adam_step_cap(const mbrl_adam_tensor* tensors, int count, const mbrl_adam_hparams& hp,
                                       int arith, hipStream_t stream) {
    AdamLaunchT<CAP> L{};
    L.hp = hp;
    L.arith = arith;
    return adam_table_walk<CAP>(L, tensors, count, [](int, int) {}, [&](int blocks) {
        hipLaunchKernelGGL(adam_step_kernel<CAP>, dim3(blocks), dim3(ADAM_THREADS), 0, stream, L);
    });
}

// tensors [E][count]: tensor i belongs to member i / count, whose coefficient scales its gradient.
hipError_t launch_adam_step_clipped(const mbrl_adam_tensor* tensors, int E, int count, const mbrl_adam_hparams& hp,
                                    int arith, const float* coef, hipStream_t stream) {
    AdamClipLaunch L{};
    L.a.hp = hp;
    L.a.arith = arith;
    L.coef = coef;
    return adam_table_walk<ADAM_ENS_TENSORS>(
        L.a, tensors, E * count, [&](int slot, int i) { L.member[slot] = (uint8_t)(i / count); },
        [&](int blocks) {
            hipLaunchKernelGGL(adam_step_clipped_kernel, dim3(blocks), dim3(ADAM_THREADS), 0, stream, L);
        });
}

hipError_t launch_adam_step(const mbrl_adam_tensor* tensors, int count, const mbrl_adam_hparams& hp, int arith,
                            hipStream_t stream) {
    return launch_adam_step_cap<ADAM_MAX_TENSORS>(tensors, count, hp, arith, stream);
}

hipError_t launch_adam_step_ensemble(const mbrl_adam_tensor* tensors, int count, const mbrl_adam_hparams& hp,
                                     int arith, hipStream_t stream) {
    return launch_adam_step_cap<ADAM_ENS_TENSORS>(tensors, count, hp, arith, stream);
}

int adam_arith() {
    const int o = opt(MBRL_OPT_ADAM_ARITH);
    return o ? o - 1 : ADAM_ARITH_TORCH;
}

int adam_table_check(const char* what, const mbrl_adam_tensor* tensors, int E, int count) {
    const int total = (E ? E : 1) * count;
    for (int i = 0; i < total; ++i) {
        const mbrl_adam_tensor& t = tensors[i];
        if (t.numel == 0 || (t.numel > 0 && t.param && t.grad && t.exp_avg && t.exp_avg_sq)) continue;
        if (E == 0) return fail(MBRL_EINVAL, "%s %d: NULL pointer or negative numel", what, i);
        return fail(MBRL_EINVAL, "%s: member %d, Adam tensor %d: NULL pointer or negative numel", what, i / count,
                    i % count);
    }
    return MBRL_OK;
}

}  // namespace mbrl

using namespace mbrl;

// ---- ABI entries (include/mbrl_cem.h): argument checks around the launchers above
extern "C" {

int mbrl_adam_step(const mbrl_adam_tensor* tensors, int32_t count, const mbrl_adam_hparams* hparams,
                   mbrl_stream_t stream) {
    if (count < 0 || (count > 0 && !tensors) || !hparams) return fail(MBRL_EINVAL, "adam_step: NULL argument");
    if (int rc = adam_table_check("adam_step: tensor", tensors, 0, count)) return rc;
    return hip_check(launch_adam_step(tensors, count, *hparams, adam_arith(), reinterpret_cast<hipStream_t>(stream)),
                     "adam_step");
}

int mbrl_adam_step_clipped(const mbrl_adam_tensor* tensors, int32_t E, int32_t count, const mbrl_adam_hparams* hparams,
                           const float* coef, mbrl_stream_t stream) {
    const char* what = "adam_step_clipped";
    if (!hparams || !coef) return fail(MBRL_EINVAL, "%s: NULL argument", what);
    if (int rc = grad_clip_table_check(what, tensors, E, count, true)) return rc;
    return hip_check(launch_adam_step_clipped(tensors, E, count, *hparams, adam_arith(), coef,
                                              reinterpret_cast<hipStream_t>(stream)), what);
}

}  // extern "C"
