// Row access the receding-horizon kernels share (cem_rh.hip, cem_noise.hip): a Philox block's four
// dimensions of one step of a kept row or of an output row, with 16-byte accesses where a is a multiple of
// 4 and the buffers are 16-byte aligned (VEC), and the per-problem input flags.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mbrl {

typedef float rh_f4 __attribute__((ext_vector_type(4)));

// clip of a kept entry: a NaN stays NaN (np.minimum(np.maximum(x, lo), hi)), so a poisoned row's return
// is NaN and the row sorts last; fminf / fmaxf alone would turn it into lo.
__device__ __forceinline__ float kept_clip(float x, float lo, float hi) {
    return x != x ? x : fminf(fmaxf(x, lo), hi);
}

// Dimensions 4g .. 4g+3 of a kept row's step (src = the step's [a] floats), clipped.
template <bool VEC>
__device__ __forceinline__ void kept_load4(const float* __restrict__ src, int g, int a, float lo, float hi, float v[4]) {
    if (VEC) {
        const rh_f4 x = *reinterpret_cast<const rh_f4*>(src + 4 * g);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = kept_clip(x[j], lo, hi);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = 4 * g + j < a ? kept_clip(src[4 * g + j], lo, hi) : 0.f;
    }
}

template <bool VEC>
__device__ __forceinline__ void store4(float* __restrict__ dst, int g, int a, const float v[4]) {
    if (VEC) {
        *reinterpret_cast<rh_f4*>(dst + 4 * g) = rh_f4{v[0], v[1], v[2], v[3]};
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (4 * g + j < a) dst[4 * g + j] = v[j];
    }
}

// Which of the optional inputs apply to problem b (bit 0: mu rows, 1: sigma rows, 2: carry_in); no flags:
// every given pointer applies to every problem.
__device__ __forceinline__ int rh_flags(const int32_t* __restrict__ flags, int b) { return flags ? flags[b] : 7; }

}  // namespace mbrl
