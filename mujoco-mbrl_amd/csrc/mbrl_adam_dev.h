// One element of torch.optim.Adam's step: the only device function the Adam kernels (adam.hip), the tiled GEMM
// (train.hip) and the fused step (train_fused.hip) share. Always inlined: the project builds without
// relocatable device code, so shared device code lives in headers (as mbrl_rollout_dev.h).
#pragma once
#include <hip/hip_runtime.h>

#include "mbrl_internal.h"

namespace mbrl {

// One element of the chain. Bits of `arith` select which of torch's expressions were contracted to
// a fused multiply-add by the compiler that built torch (ForeachFunctors.cuh / Lerp.h):
//   ADAM_FMA_WD      grad + wd * param                        (_foreach_add(grads, params, alpha=wd))
//   ADAM_FMA_LERP    exp_avg + w * (grad - exp_avg)           (_foreach_lerp_, w < 0.5; else
//                    grad - (grad - exp_avg) * (1 - w))
//   ADAM_FMA_ADDCMUL exp_avg_sq + (1 - beta2) * (grad * grad) (_foreach_addcmul_)
//   ADAM_FMA_ADDCDIV param + step_size * (exp_avg / denom)    (_foreach_addcdiv_)
__device__ __forceinline__ void adam_element(float& p, float g, float& m, float& v, float step_size, float bc2,
                                             const mbrl_adam_hparams& hp, int arith) {
    if (hp.weight_decay != 0.0f)
        g = (arith & ADAM_FMA_WD) ? fmaf(hp.weight_decay, p, g) : g + hp.weight_decay * p;
    const float w = hp.lerp_weight;
    if (fabsf(w) < 0.5f) {
        const float d = g - m;
        m = (arith & ADAM_FMA_LERP) ? fmaf(w, d, m) : m + w * d;
    } else {
        const float d = g - m, omw = 1.0f - w;
        m = (arith & ADAM_FMA_LERP) ? fmaf(-d, omw, g) : g - d * omw;
    }
    v = v * hp.beta2;
    const float gg = g * g;
    v = (arith & ADAM_FMA_ADDCMUL) ? fmaf(hp.one_minus_beta2, gg, v) : v + hp.one_minus_beta2 * gg;
    float den = sqrtf(v);
    den = den / bc2;
    den = den + hp.eps;
    const float q = m / den;
    p = (arith & ADAM_FMA_ADDCDIV) ? fmaf(step_size, q, p) : p + step_size * q;
}

}  // namespace mbrl
