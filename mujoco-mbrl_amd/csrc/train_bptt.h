// The device routines of the 16-position backward kernels (train_open_loop.hip's backward through time and
// train_nll.hip's one-step backward): the store of a tile's rows and the ordered column sum, which both use, and
// the fp32 transposed layer product with the ReLU mask (train_nll.hip keeps a copy that accumulates in fp64).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "eval_mlp.h"

namespace mbrl {

constexpr int OL_TM = 16;            // rows of the batch per workgroup: the MFMA's 16 columns (eval.hip's EVAL_TM)
constexpr int OL_THREADS = 64 * EVAL_WAVES;
constexpr int OL_LDS_BYTES = 160 * 1024;

// rows [0, n) x columns [0, width) of an LDS buffer to dst[row * width + col]
__device__ __forceinline__ void ol_store_rows(const float* buf, int ld, float* dst, int width, int n) {
    if ((width & 3) == 0) {
        const int w4 = width >> 2;
        for (int idx = threadIdx.x; idx < n * w4; idx += OL_THREADS) {
            const int row = idx / w4, k = (idx - row * w4) * 4;
            *reinterpret_cast<eval_f32x4*>(dst + (int64_t)row * width + k) =
                *reinterpret_cast<const eval_f32x4*>(buf + row * ld + k);
        }
    } else {
        for (int idx = threadIdx.x; idx < n * width; idx += OL_THREADS) {
            const int row = idx / width, k = idx - row * width;
            dst[(int64_t)row * width + k] = buf[row * ld + k];
        }
    }
}

// out[p][m] = (sum_n in[p][n] w[n][m]) (* (mask[p][m] > 0)) for the tile's 16 positions and m < Kout, rows n < n0
// of the weights from w0 and n0 <= n < n0 + n1 from w1, both with ldw floats per row; columns from Kout to the
// next multiple of 16 are written as zeros. mask and store are the tile's rows of [.][ldo] arrays in global
// memory (NULL: none); rows past nvalid mask to zero and are not stored.
__device__ __forceinline__ void bptt_layer(const float* __restrict__ in, float* __restrict__ out, int ld,
                                           const float* __restrict__ w0, int n0, const float* __restrict__ w1, int n1,
                                           int ldw, int Kout, const float* __restrict__ mask, float* __restrict__ store,
                                           int ldo, int nvalid) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, q = lane >> 4;
    const int N = n0 + n1, N16 = (N + 15) & ~15, MB = (Kout + 15) >> 4;
    const bool vec = (ldo & 3) == 0;
    for (int mb0 = wave * EVAL_JB; mb0 < MB; mb0 += EVAL_WAVES * EVAL_JB) {
        eval_f32x4 acc[EVAL_JB], keep[EVAL_JB];
        float w1v[EVAL_JB];
#pragma unroll
        for (int j = 0; j < EVAL_JB; ++j) {
            acc[j] = eval_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            keep[j] = eval_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            w1v[j] = 0.0f;
            if (n1 && (mb0 + j) * 16 + c < Kout) w1v[j] = w1[(mb0 + j) * 16 + c];
            // the ReLU mask's activations, ahead of the products
            const int mbase = (mb0 + j) * 16 + 4 * q;
            if (mask && mb0 + j < MB && c < nvalid) {
                if (vec && mbase + 3 < Kout) {
                    keep[j] = *reinterpret_cast<const eval_f32x4*>(mask + (int64_t)c * ldo + mbase);
                } else {
#pragma unroll
                    for (int v = 0; v < 4; ++v)
                        if (mbase + v < Kout) keep[j][v] = mask[(int64_t)c * ldo + mbase + v];
                }
            }
        }
        for (int nb = 0; nb < N16; nb += 16) {
            const int n = nb + 4 * q;
            const eval_f32x4 x = *reinterpret_cast<const eval_f32x4*>(&in[c * ld + n]);
            // every lane loads from a valid address (the last row where it has none, column 0 where it has no
            // column) and the value is masked afterwards: no divergent branch around the loads. The second
            // block of rows is the reward head's one row: it was loaded ahead of the loop.
            size_t roff[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) roff[i] = (size_t)min(n + i, n0 - 1) * ldw;
#pragma unroll
            for (int j = 0; j < EVAL_JB; ++j) {
                if (mb0 + j >= MB) continue;             // (wave-uniform)
                const int m = (mb0 + j) * 16 + c;
                const bool mok = m < Kout;
                eval_f32x4 wv;
#pragma unroll
                for (int i = 0; i < 4; ++i) wv[i] = w0[roff[i] + (mok ? m : 0)];
#pragma unroll
                for (int i = 0; i < 4; ++i) wv[i] = !mok ? 0.0f : n + i < n0 ? wv[i] : n + i < N ? w1v[j] : 0.0f;
                for (int i = 0; i < 4; ++i) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[i], x[i], acc[j], 0, 0, 0);
            }
        }
        // lane l holds columns 16 mb + 4 q + v, v = 0 .. 3, of position c
#pragma unroll
        for (int j = 0; j < EVAL_JB; ++j) {
            if (mb0 + j >= MB) continue;
            const int mbase = (mb0 + j) * 16 + 4 * q;
            eval_f32x4 y;
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                float t = acc[j][v];
                if (mask && !(keep[j][v] > 0.0f)) t = 0.0f;
                if (mbase + v >= Kout) t = 0.0f;          // (0 x a non-finite delta is a NaN: the padding stays zero)
                y[v] = t;
            }
            *reinterpret_cast<eval_f32x4*>(&out[c * ld + mbase]) = y;
            if (store && c < nvalid) {
                if (vec && mbase + 3 < Kout) {
                    *reinterpret_cast<eval_f32x4*>(store + (int64_t)c * ldo + mbase) = y;
                } else {
#pragma unroll
                    for (int v = 0; v < 4; ++v)
                        if (mbase + v < Kout) store[(int64_t)c * ldo + mbase + v] = y[v];
                }
            }
        }
    }
}

// acc[n] (+)= buf[0][n] + buf[1][n] + .. + buf[nvalid - 1][n], rows ascending; thread n % OL_THREADS owns column n
__device__ __forceinline__ void ol_colsum(const float* buf, int ld, int N, int nvalid, float* acc, bool first) {
    for (int n = threadIdx.x; n < N; n += OL_THREADS) {
        float t = buf[n];
        for (int r = 1; r < nvalid; ++r) t = t + buf[r * ld + n];
        acc[n] = first ? t : acc[n] + t;
    }
}

}  // namespace mbrl
