// The 16-row MLP tile of eval.hip and train_open_loop.hip: one copy of the layer product, the forward pass
// and the launch arguments, so that mbrl_eval_members_open_loop and mbrl_train_grads_open_loop's forward
// kernel run the same fma chains and produce the same bytes (the layout is described at the top of eval.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "mbrl_host.h"

namespace mbrl {

typedef float eval_f32x4 __attribute__((ext_vector_type(4)));

constexpr int EVAL_WAVES = 4;      // waves per workgroup; each takes 16-neuron blocks of a layer
constexpr int EVAL_JB = 4;         // blocks a wave accumulates at once: one activation read feeds them all
constexpr int EVAL_PAD = 4;        // floats between LDS rows: 16-byte aligned rows on shifted banks

struct EvalMember {
    const float* w[MBRL_TRAIN_MAX_LAYERS];
    const float* b[MBRL_TRAIN_MAX_LAYERS];
};

struct EvalLaunch {
    EvalMember m[MBRL_TRAIN_MAX_MEMBERS];
    const float *states, *actions, *next_states, *rewards;
    const int64_t* rows;
    float *row_err, *row_rew_err;    // [E][P]
    int64_t P;                       // R * horizon
    int s, a, W, L, reward, H, ld;
};

// floats per LDS row: the widest layer rounded up to whole 16-deep chunks (the padding columns hold
// zeros, so that a chunk never reads what no layer wrote), plus EVAL_PAD
inline int eval_ld(int s, int a, int W, int reward) {
    const int widest = std::max(W, std::max(s + a, s + reward));
    return ((widest + 15) & ~15) + EVAL_PAD;
}

// out[p][n] = (relu)(sum_k in[p][k] w[n][k] + b[n]) for the tile's 16 positions, n < n0 from (w0, b0)
// and n0 <= n < n0 + n1 from (w1, b1); columns up to the next multiple of 16 are written as zeros.
template <bool RELU>
__device__ __forceinline__ void eval_layer(const float* __restrict__ in, float* __restrict__ out, int ld,
                                           const float* __restrict__ w0, const float* __restrict__ b0, int n0,
                                           const float* __restrict__ w1, const float* __restrict__ b1, int n1, int K) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, q = lane >> 4;
    const int N = n0 + n1, NB = (N + 15) >> 4, K16 = (K + 15) & ~15;
    const bool vec = (K & 3) == 0 &&
                     ((reinterpret_cast<uintptr_t>(w0) | (n1 ? reinterpret_cast<uintptr_t>(w1) : 0)) & 15) == 0;
    for (int nb0 = wave * EVAL_JB; nb0 < NB; nb0 += EVAL_WAVES * EVAL_JB) {
        eval_f32x4 acc[EVAL_JB];
        const float* wrow[EVAL_JB];
#pragma unroll
        for (int j = 0; j < EVAL_JB; ++j) {
            acc[j] = eval_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            const int n = (nb0 + j) * 16 + c;
            wrow[j] = n < n0 ? w0 + (size_t)n * K : n < N ? w1 + (size_t)(n - n0) * K : nullptr;
        }
        for (int kb = 0; kb < K16; kb += 16) {
            const int k = kb + 4 * q;
            const eval_f32x4 x = *reinterpret_cast<const eval_f32x4*>(&in[c * ld + k]);
#pragma unroll
            for (int j = 0; j < EVAL_JB; ++j) {
                if (nb0 + j >= NB) continue;             // (wave-uniform)
                eval_f32x4 wv = eval_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
                if (wrow[j]) {
                    if (vec) {
                        if (k < K) wv = *reinterpret_cast<const eval_f32x4*>(wrow[j] + k);
                    } else {
#pragma unroll
                        for (int i = 0; i < 4; ++i)
                            if (k + i < K) wv[i] = wrow[j][k + i];
                    }
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[i], x[i], acc[j], 0, 0, 0);
            }
        }
        // lane l holds neurons 16 nb + 4 q + v, v = 0 .. 3, of position c
#pragma unroll
        for (int j = 0; j < EVAL_JB; ++j) {
            if (nb0 + j >= NB) continue;
            const int nbase = (nb0 + j) * 16 + 4 * q;
            eval_f32x4 y;
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int n = nbase + v;
                const float bias = n < n0 ? b0[n] : n < N ? b1[n - n0] : 0.0f;
                float t = acc[j][v] + bias;
                if (RELU) t = t < 0.0f ? 0.0f : t;       // (a NaN stays a NaN, as torch's relu keeps it)
                y[v] = t;
            }
            *reinterpret_cast<eval_f32x4*>(&out[c * ld + nbase]) = y;
        }
    }
}

// The member's forward pass on the 16 inputs in buf[cur] (s + a columns, zeros up to the next multiple of
// 16): returns the buffer that holds (s^, r^) in columns 0 .. s (+ 1), zeros up to the next multiple of 16,
// behind a barrier.
__device__ __forceinline__ int eval_forward(const EvalLaunch& A, const EvalMember& M, float* const* buf, int cur) {
    for (int l = 0; l < A.L; ++l) {
        eval_layer<true>(buf[cur], buf[cur ^ 1], A.ld, M.w[l], M.b[l], A.W, nullptr, nullptr, 0,
                         l == 0 ? A.s + A.a : A.W);
        cur ^= 1;
        __syncthreads();
    }
    eval_layer<false>(buf[cur], buf[cur ^ 1], A.ld, M.w[A.L], M.b[A.L], A.s, A.reward ? M.w[A.L + 1] : nullptr,
                      A.reward ? M.b[A.L + 1] : nullptr, A.reward ? 1 : 0, A.W);
    __syncthreads();
    return cur ^ 1;
}

// eval_loss_kernel (eval.hip) over row_err / row_rew_err [E][R][H]: loss_out[e] in the order the header
// documents for mbrl_eval_members.
hipError_t launch_eval_loss(const float* row_err, const float* row_rew_err, float* loss_out, int E, int64_t R, int H,
                            int s, hipStream_t stream);

}  // namespace mbrl
