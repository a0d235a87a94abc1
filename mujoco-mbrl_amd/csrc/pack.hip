// Weight packing: nn.Linear [out][in] -> the fragment streams the rollout kernels read (see the
// rollout.hip header) and the plain copies of traj.hip / gd.hip; mbrl_mlp_pack and its size query.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mbrl_host.h"

namespace mbrl {

// Canonical K order of a W->W layer (r05, DESIGN.md §3 "half-rotated K order"): an output column in
// the second half (n >= Wpad / 2) consumes its K chunks rotated by half, [nkc/2, nkc) then
// [0, nkc/2), so the column half a workgroup owns always starts on the inputs it produced itself
// (the column-split pairs' hand-off then lands behind half a layer of compute). Every fp32 tile
// height packs and reads the same order, so their sums stay bit-identical.
__device__ __forceinline__ int rot_chunk(int kc, int nkc, int n, int Wpad, int rot) {
    return (rot && 2 * n >= Wpad) ? (kc + nkc / 2) % nkc : kc;
}

// Hidden-type layer (layer 0 or W->W): chunk kc holds K rows 16kc..16kc+15 for this wave's T tiles
// (rot: a W->W layer, second-half columns in the rotated order above).
__global__ void pack_hidden_kernel(const float* __restrict__ w, int in_real, int out_real, int nkc, int T,
                                   int rot, float* __restrict__ dst /* chunk base */) {
    const size_t total = (size_t)nkc * 4 * T * 64 * 4;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int s = (int)(i & 3);
        const int lane = (int)((i >> 2) & 63);
        const size_t frag = i >> 8;           // (kc * 4 + wave) * T + j
        const int j = (int)(frag % T);
        const int wave = (int)((frag / T) & 3);
        const int kc = (int)(frag / T / 4);
        const int n = wave * 16 * T + 16 * j + (lane & 15);
        const int k = 16 * rot_chunk(kc, nkc, n, 64 * T, rot) + 4 * (lane >> 4) + s;
        dst[i] = (n < out_real && k < in_real) ? w[(size_t)n * in_real + k] : 0.0f;
    }
}

// Output layer: chunk j = output tile j; fragment kc covers this wave's K rows w*16T + 16kc + ...
// Rows [0, out_real) come from w; with a reward head, row out_real comes from w_r ([1][in]).
__global__ void pack_out_kernel(const float* __restrict__ w, const float* __restrict__ w_r, int in_real,
                                int out_real, int NOT, int T, float* __restrict__ dst) {
    const size_t total = (size_t)NOT * 4 * T * 64 * 4;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int s = (int)(i & 3);
        const int lane = (int)((i >> 2) & 63);
        const size_t frag = i >> 8;           // (j * 4 + wave) * T + kc
        const int kc = (int)(frag % T);
        const int wave = (int)((frag / T) & 3);
        const int j = (int)(frag / T / 4);
        const int n = 16 * j + (lane & 15);
        const int k = wave * 16 * T + 16 * kc + 4 * (lane >> 4) + s;
        float v = 0.0f;
        if (k < in_real) {
            if (n < out_real) v = w[(size_t)n * in_real + k];
            else if (w_r && n == out_real) v = w_r[k];
        }
        dst[i] = v;
    }
}

// 8-candidate stream (rollout.hip rollout_m8_kernel): per 16-deep chunk, per wave (T of them), per
// step s (4), lane l, element q: row 32 (2 pair + ((l >> 2) & 1)) + 4 (l >> 3) + (l & 3) -- the odd
// 4-lane blocks carry the pair's second 32-row tile (ABID 1) -- and k = 16 kc + 4 q + s.
// Hidden-type layers: chunk kc, pair = the wave's own tiles (rows 64 wave + ...).
// KP mode (Wpad 256, one 32-row output tile; rollout.hip m8_kp): 8 waves of one tile, per chunk
// per wave 2 loads x 64 lanes x float4; pair pi = 4 j + e, position p = 2 pi + ((l >> 2) & 1) of
// the chunk order p = 4 s + q, row 32 wave + 4 (l >> 3) + (l & 3).
__device__ __forceinline__ void m8kp_index(size_t i, int& lane, int& wave, size_t& chunk, int& s, int& q) {
    const int e = (int)(i & 3);
    lane = (int)((i >> 2) & 63);
    const int j = (int)((i >> 8) & 1);
    const size_t cw = i >> 9;                 // chunk * 8 + wave
    wave = (int)(cw & 7);
    chunk = cw >> 3;
    const int p = 2 * (4 * j + e) + ((lane >> 2) & 1);
    s = p >> 2;
    q = p & 3;
}

__global__ void pack_m8_hidden_kernel(const float* __restrict__ w, int in_real, int out_real, int nkc, int T,
                                      int kp, int rot, float* __restrict__ dst) {
    const size_t total = (size_t)nkc * T * 1024;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        int n, k;
        if (kp) {
            int lane, wave, s, q;
            size_t kc;
            m8kp_index(i, lane, wave, kc, s, q);
            n = 32 * wave + 4 * (lane >> 3) + (lane & 3);
            k = 16 * rot_chunk((int)kc, nkc, n, 64 * T, rot) + 4 * q + s;
        } else {
            const int q = (int)(i & 3);
            const int lane = (int)((i >> 2) & 63);
            const int s = (int)((i >> 8) & 3);
            const size_t cw = i >> 10;            // kc * T + wave
            const int wave = (int)(cw % T);
            const int kc = (int)(cw / T);
            n = 64 * wave + 32 * ((lane >> 2) & 1) + 4 * (lane >> 3) + (lane & 3);
            k = 16 * rot_chunk(kc, nkc, n, 64 * T, rot) + 4 * q + s;
        }
        dst[i] = (n < out_real && k < in_real) ? w[(size_t)n * in_real + k] : 0.0f;
    }
}

// Output layer over the wave's own K rows 64 wave + 16 kc + ...: with one 32-row tile (kpair) chunk o
// holds own K chunks 2o (even blocks) and 2o + 1 (odd blocks); else chunk o = kc * NOP + pair holds
// output tiles 2 pair (even blocks) and 2 pair + 1 (odd blocks).
__global__ void pack_m8_out_kernel(const float* __restrict__ w, int in_real, int out_real, int NOP, int kpair,
                                   int T, int kp, float* __restrict__ dst) {
    const size_t total = (size_t)(kpair ? 2 : 4 * NOP) * T * 1024;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        if (kp) {   // own K chunk o of the wave's 32 features, one 32-row output tile
            int lane, wave, s, q;
            size_t o;
            m8kp_index(i, lane, wave, o, s, q);
            const int n = 4 * (lane >> 3) + (lane & 3);
            const int k = 32 * wave + 16 * (int)o + 4 * q + s;
            dst[i] = (n < out_real && k < in_real) ? w[(size_t)n * in_real + k] : 0.0f;
            continue;
        }
        const int q = (int)(i & 3);
        const int lane = (int)((i >> 2) & 63);
        const int s = (int)((i >> 8) & 3);
        const size_t cw = i >> 10;            // o * T + wave
        const int wave = (int)(cw % T);
        const int o = (int)(cw / T);
        const int odd = (lane >> 2) & 1;
        const int kc = kpair ? 2 * o + odd : o / NOP;
        const int tile = kpair ? 0 : 2 * (o % NOP) + odd;
        const int n = 32 * tile + 4 * (lane >> 3) + (lane & 3);
        const int k = 64 * wave + 16 * kc + 4 * q + s;
        dst[i] = (n < out_real && k < in_real) ? w[(size_t)n * in_real + k] : 0.0f;
    }
}

// 4-candidate output chunks (rollout_m4_kernel): chunk kc of wave w's own 64 features; float4 s =
// output group g, element q: row n = 16 g + 4 (l >> 4) + (l & 3), k = 64 w + 16 kc + 4 q + chain,
// chain = (l >> 2) & 3 -- the canonical output chains of the 16-candidate kernel (mma_out).
__global__ void pack_m4_out_kernel(const float* __restrict__ w, int in_real, int out_real, int T,
                                   float* __restrict__ dst) {
    const size_t total = (size_t)4 * T * 1024;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int q = (int)(i & 3);
        const int lane = (int)((i >> 2) & 63);
        const int grp = (int)((i >> 8) & 3);
        const size_t cw = i >> 10;            // kc * T + wave
        const int wave = (int)(cw % T);
        const int kc = (int)(cw / T);
        const int n = 16 * grp + 4 * (lane >> 4) + (lane & 3);
        const int k = 64 * wave + 16 * kc + 4 * q + ((lane >> 2) & 3);
        dst[i] = (n < out_real && k < in_real) ? w[(size_t)n * in_real + k] : 0.0f;
    }
}

// Split streams (rollout_f16x3.hip): chunk = 32 K rows; per chunk 8 waves x (T/2 tiles x P pieces)
// fragments of 64 lanes x 8 halves. Fragment f of a hidden-type chunk = tile f / P, piece f % P.
// Lane l, element q: row n = 16 (wave T/2 + tile) + (l & 15), k = 32 kc + 8 (l >> 4) + q.
// Weights are scaled by MBRL_SPLIT_W_SCALE (exact) and split as w0 = f16(w), w1 = f16(w - w0),
// w2 = f16(w - w0 - w1). A scaled weight >= 32768 (|w| >= 128) cannot be split: *bad becomes
// nonzero and every workgroup of the rollout leaves its candidates to the fp32 redo pass.
__device__ __forceinline__ void split_weight(float v0, int P, _Float16* dst, unsigned* bad) {
    float v = v0 * MBRL_SPLIT_W_SCALE;
    if (!(fabsf(v) < 32768.0f)) atomicOr(bad, 1u);
    for (int q = 0; q < P; ++q) {
        const _Float16 h = (_Float16)v;
        dst[q * 512] = h;                 // piece q is fragment f + q: 64 lanes x 8 halves further
        v = v - (float)h;
    }
}

__global__ void pack_split_hidden_kernel(const float* __restrict__ w, int in_real, int out_real, int nkc, int T,
                                         int P, _Float16* __restrict__ dst, unsigned* __restrict__ bad) {
    const int TW = T / 2;
    const size_t total = (size_t)nkc * 8 * TW * 64 * 8;   // (kc, wave, tile, lane, q); all pieces per item
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int q = (int)(i & 7);
        const int lane = (int)((i >> 3) & 63);
        const size_t r = i >> 9;               // (kc * 8 + wave) * TW + tile
        const int tile = (int)(r % TW);
        const int wave = (int)((r / TW) & 7);
        const int kc = (int)(r / TW / 8);
        const int n = 16 * (wave * TW + tile) + (lane & 15);
        const int k = 32 * kc + 8 * (lane >> 4) + q;
        const float v = (n < out_real && k < in_real) ? w[(size_t)n * in_real + k] : 0.0f;
        const size_t frag = ((size_t)kc * 8 + wave) * TW * P + (size_t)tile * P;   // piece 0
        split_weight(v, P, dst + (frag * 64 + lane) * 8 + q, bad);
    }
}

// Output layer: chunk c pairs output tiles 2c, 2c + 1; wave w's K range is units [16 w TW, 16 (w+1) TW)
// taken as K-chunks kk of two tiles (2kk, 2kk+1) in the accumulator order: element q of lane group
// g is unit 16 (w TW + 2kk + (q >> 2)) + 4g + (q & 3). Fragment f = (u TW/2 + kk) P + piece.
__global__ void pack_split_out_kernel(const float* __restrict__ w, const float* __restrict__ w_r, int in_real,
                                      int out_real, int NOS, int T, int P, _Float16* __restrict__ dst,
                                      unsigned* __restrict__ bad) {
    const int TW = T / 2, KK = TW / 2;
    const size_t total = (size_t)NOS * 8 * 2 * KK * 64 * 8;   // (c, wave, u, kk, lane, q)
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int q = (int)(i & 7);
        const int lane = (int)((i >> 3) & 63);
        size_t r = i >> 9;
        const int kk = (int)(r % KK); r /= KK;
        const int u = (int)(r % 2); r /= 2;
        const int wave = (int)(r % 8);
        const int c = (int)(r / 8);
        const int n = 16 * (2 * c + u) + (lane & 15);
        const int k = 16 * (wave * TW + 2 * kk + (q >> 2)) + 4 * (lane >> 4) + (q & 3);
        float v = 0.0f;
        if (k < in_real) {
            if (n < out_real) v = w[(size_t)n * in_real + k];
            else if (w_r && n == out_real) v = w_r[k];
        }
        const size_t frag = ((size_t)c * 8 + wave) * TW * P + (size_t)(u * KK + kk) * P;
        split_weight(v, P, dst + (frag * 64 + lane) * 8 + q, bad);
    }
}

// Plain copies for traj.hip: transposed W^T [in][cols] (zero-padded columns) ...
__global__ void pack_transposed_kernel(const float* __restrict__ w, int in_real, int out_real, int cols,
                                       float* __restrict__ dst) {
    const size_t total = (size_t)in_real * cols;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int k = (int)(i / cols), n = (int)(i - (i / cols) * cols);
        dst[i] = n < out_real ? w[(size_t)n * in_real + k] : 0.0f;
    }
}

// ... and a straight copy (the output layer keeps nn.Linear's row-major [out][in]).
__global__ void copy_kernel(const float* __restrict__ src, size_t n, float* __restrict__ dst) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        dst[i] = src[i];
}

__global__ void pack_bias_kernel(const float* __restrict__ b, int n_real, int n_pad, float* __restrict__ dst) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n_pad; i += gridDim.x * blockDim.x)
        dst[i] = i < n_real ? b[i] : 0.0f;
}

}  // namespace mbrl

using namespace mbrl;

extern "C" {

size_t mbrl_mlp_packed_bytes(const mbrl_mlp_shape* shape) {
    Geometry g;
    if (shape_geometry(shape, &g) != MBRL_OK) return 0;
    return g.member_stride * (size_t)g.E * sizeof(float);
}

int mbrl_mlp_pack(const mbrl_mlp_shape* shape, const float* const* weights, const float* const* biases,
                  void* packed, mbrl_stream_t stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    Geometry g;
    int rc = shape_geometry(shape, &g);
    if (rc) return rc;
    if (!weights || !biases || !packed) return fail(MBRL_EINVAL, "pack: NULL argument");
    const int nl = g.L + 1 + g.reward;   // trunk, state head, [reward head]
    for (int e = 0; e < g.E; ++e) {
        float* base = static_cast<float*>(packed) + (size_t)e * g.member_stride;
        float* bias_base = base + g.stream_floats;
        size_t chunk = 0;
        // the 2-piece (F16X3) and 3-piece (F16X6) split streams, each followed by its flag word
        _Float16* split_base[2] = {reinterpret_cast<_Float16*>(base + g.split_off),
                                   reinterpret_cast<_Float16*>(base + g.split3_off)};
        unsigned* split_bad[2] = {reinterpret_cast<unsigned*>(base + g.split_off + (size_t)g.CS * 2048 * g.T),
                                  reinterpret_cast<unsigned*>(base + g.split3_off + (size_t)g.CS * 3072 * g.T)};
        size_t split_chunk = 0;
        float* m8_base = base + g.m8_off;
        size_t m8_chunk = 0;
        float* m4_base = base + g.m4_off;
        if (g.split_ok)
            for (int q = 0; q < 2; ++q) {
                hipError_t err = hipMemsetAsync(split_bad[q], 0, 4, stream);
                if (err != hipSuccess) return hip_check(err, "pack flag reset");
            }
        for (int l = 0; l <= g.L; ++l) {
            const float* w = weights[e * nl + l];
            const float* b = biases[e * nl + l];
            if (!w || !b) return fail(MBRL_EINVAL, "pack: NULL weight/bias for member %d layer %d", e, l);
            float* dst = base + chunk * 1024 * g.T;
            float* plain = base + g.stream_floats + g.bias_floats + g.tw_off[l];
            if (l < g.L) {
                const int in_real = l == 0 ? g.s + g.a : g.W;
                const int nkc = l == 0 ? g.K0C : 4 * g.T;
                const int rot = l > 0;   // W->W layers: the half-rotated K order of the second column half
                hipLaunchKernelGGL(pack_hidden_kernel, dim3(256), dim3(256), 0, stream, w, in_real, g.W, nkc, g.T, rot, dst);
                hipLaunchKernelGGL(pack_bias_kernel, dim3(4), dim3(256), 0, stream, b, g.W, g.Wpad, bias_base + (size_t)l * g.Wpad);
                hipLaunchKernelGGL(pack_transposed_kernel, dim3(256), dim3(256), 0, stream, w, in_real, g.W, g.Wpad, plain);
                if (g.split_ok) {
                    const int nks = l == 0 ? g.K0S : 2 * g.T;
                    for (int P = 2; P <= 3; ++P)
                        hipLaunchKernelGGL(pack_split_hidden_kernel, dim3(256), dim3(256), 0, stream, w, in_real, g.W,
                                           nks, g.T, P, split_base[P - 2] + split_chunk * 2048 * (size_t)g.T * P,
                                           split_bad[P - 2]);
                    split_chunk += nks;
                }
                if (g.m8_ok) {
                    hipLaunchKernelGGL(pack_m8_hidden_kernel, dim3(256), dim3(256), 0, stream, w, in_real, g.W, nkc,
                                       g.T, (int)(g.T == 4 && g.NOT == 2), rot, m8_base + m8_chunk * 1024 * (size_t)g.T);
                    if (g.m4_ok)   // the same chunks without KP pairing (the m8 chunk index = the m4 one here)
                        hipLaunchKernelGGL(pack_m8_hidden_kernel, dim3(256), dim3(256), 0, stream, w, in_real, g.W, nkc,
                                           g.T, 0, rot, m4_base + m8_chunk * 1024 * (size_t)g.T);
                    m8_chunk += nkc;
                }
                chunk += nkc;
            } else {
                const float* wr = g.reward ? weights[e * nl + g.L + 1] : nullptr;
                const float* br = g.reward ? biases[e * nl + g.L + 1] : nullptr;
                if (g.reward && (!wr || !br)) return fail(MBRL_EINVAL, "pack: NULL reward head for member %d", e);
                hipLaunchKernelGGL(pack_out_kernel, dim3(256), dim3(256), 0, stream, w, wr, g.W, g.s, g.NOT, g.T, dst);
                if (g.split_ok)
                    for (int P = 2; P <= 3; ++P)
                        hipLaunchKernelGGL(pack_split_out_kernel, dim3(256), dim3(256), 0, stream, w, wr, g.W, g.s,
                                           g.NOS, g.T, P, split_base[P - 2] + split_chunk * 2048 * (size_t)g.T * P,
                                           split_bad[P - 2]);
                if (g.m8_ok)
                    hipLaunchKernelGGL(pack_m8_out_kernel, dim3(256), dim3(256), 0, stream, w, g.W, g.s, g.NOP8, g.NOC8 == 2, g.T,
                                       (int)(g.T == 4 && g.NOT == 2),
                                       m8_base + m8_chunk * 1024 * (size_t)g.T);
                if (g.m4_ok)
                    hipLaunchKernelGGL(pack_m4_out_kernel, dim3(256), dim3(256), 0, stream, w, g.W, g.s, g.T,
                                       m4_base + m8_chunk * 1024 * (size_t)g.T);
                float* ob = bias_base + (size_t)g.L * g.Wpad;
                hipLaunchKernelGGL(pack_bias_kernel, dim3(1), dim3(256), 0, stream, b, g.s, 16 * g.NOT, ob);
                hipLaunchKernelGGL(copy_kernel, dim3(64), dim3(256), 0, stream, w, (size_t)g.s * g.W, plain);
                if (g.reward) {   // row s of the output block: the reward head (after the zero padding)
                    hipLaunchKernelGGL(copy_kernel, dim3(1), dim3(64), 0, stream, br, (size_t)1, ob + g.s);
                    hipLaunchKernelGGL(copy_kernel, dim3(4), dim3(256), 0, stream, wr, (size_t)g.W,
                                       plain + (size_t)g.s * g.W);
                }
                chunk += g.NOT;
            }
        }
    }
    return hip_check(hipGetLastError(), "pack launch");
}

}  // extern "C"
