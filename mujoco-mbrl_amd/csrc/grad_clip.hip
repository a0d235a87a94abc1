// Per-member global-norm gradient clipping for the ensemble training epochs (include/mbrl_cem.h mbrl_grad_norm,
// mbrl_grad_clip): torch.nn.utils.clip_grad_norm_(member.parameters(), max_norm) between backward() and
// Adam.step(), as two launches whatever E, count and the shapes are, ahead of the clipped Adam launch (adam.hip
// adam_step_clipped_kernel).
//
// The sum of squares of member e's gradient tensors is taken in ONE order that depends on the tensors' numels alone
// (tests/grad_clip_reference.py restates it in NumPy):
//   1. tensor i is cut into chunks of 1024 consecutive elements, the last one padded with zeros;
//   2. in a chunk, lane t of 256 forms ((g[4t]^2 + g[4t+1]^2) + g[4t+2]^2) + g[4t+3]^2, every square rounded
//      before it is added (the file is built with -ffp-contract=off), and the 256 lane values meet in the
//      pairwise tree v[t] += v[t + d], d = 128, 64, .. 1: the chunk's partial (grad_sumsq_kernel, one workgroup
//      per chunk, no atomics);
//   3. the member's P partials lie end to end, tensor ascending, chunk ascending, empty tensors contributing none;
//      lane t of 1024 adds partials t, t + 1024, .. ascending and the 1024 lane values meet in the pairwise tree
//      d = 512, .. 1 -- mbrl_eval_members' rule for its loss (grad_norm_finish_kernel, one workgroup per member).
// Then norm = sqrtf(sum), q = max_norm / (norm + 1e-6f), coef = q > 1 ? 1 : q (a NaN q stays NaN).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mbrl_host.h"

namespace mbrl {

constexpr int GC_THREADS = 256;
constexpr int GC_CHUNK = GC_THREADS * 4;    // elements per workgroup and partial
constexpr int GC_TENSORS = 64;              // tensors per launch (the table travels in the launch arguments)
constexpr int GC_FINISH_THREADS = 1024;
constexpr int GC_COEF_FLOATS = MBRL_TRAIN_MAX_MEMBERS;   // the workspace's head: coef[E]; the partials follow

struct GradSumsqLaunch {
    const float* grad[GC_TENSORS];
    float* partial[GC_TENSORS];             // where the tensor's chunk partials go
    int64_t numel[GC_TENSORS];
    int first_block[GC_TENSORS + 1];        // workgroup prefix over the tensors' chunks
    int count;
};

// v[t] += v[t + d] for d = N / 2 .. 1 over the workgroup's N lane values; the result in thread 0. The steps within
// one wave (d <= 32) are shuffles: the same additions of the same values, so the same bits as the LDS tree.
template <int N>
__device__ __forceinline__ float tree_sum(float v, float* lds) {
    const int t = threadIdx.x;
    lds[t] = v;
    __syncthreads();
    for (int d = N / 2; d >= 64; d >>= 1) {
        if (t < d) lds[t] += lds[t + d];
        __syncthreads();
    }
    v = lds[t];
    if (t < 64)
        for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d, 64);
    return v;
}

__global__ __launch_bounds__(GC_THREADS) void grad_sumsq_kernel(const GradSumsqLaunch L) {
    __shared__ float lds[GC_THREADS];
    const int blk = blockIdx.x;
    int ti = 0;
    while (ti + 1 < L.count && blk >= L.first_block[ti + 1]) ++ti;
    const float* g = L.grad[ti];
    const int64_t numel = L.numel[ti];
    const int chunk = blk - L.first_block[ti];
    const int64_t i0 = (int64_t)chunk * GC_CHUNK + 4 * (int64_t)threadIdx.x;
    float4 x = make_float4(0.0f, 0.0f, 0.0f, 0.0f);      // the padding takes part as zeros
    if (i0 + 4 <= numel && (reinterpret_cast<uintptr_t>(g) & 15) == 0) {
        x = *reinterpret_cast<const float4*>(g + i0);
    } else {
        if (i0 < numel) x.x = g[i0];
        if (i0 + 1 < numel) x.y = g[i0 + 1];
        if (i0 + 2 < numel) x.z = g[i0 + 2];
        if (i0 + 3 < numel) x.w = g[i0 + 3];
    }
    const float v = ((x.x * x.x + x.y * x.y) + x.z * x.z) + x.w * x.w;
    const float sum = tree_sum<GC_THREADS>(v, lds);
    if (threadIdx.x == 0) L.partial[ti][chunk] = sum;
}

struct GradNormFinish {
    const float* partial[MBRL_TRAIN_MAX_MEMBERS];
    int P[MBRL_TRAIN_MAX_MEMBERS];
    float max_norm;
    float* norm_out;    // [E] or NULL
    float* coef_out;    // [E]
};

__global__ __launch_bounds__(GC_FINISH_THREADS) void grad_norm_finish_kernel(const GradNormFinish F) {
    __shared__ float lds[GC_FINISH_THREADS];
    const int e = blockIdx.x;
    const float* p = F.partial[e];
    const int P = F.P[e];
    float acc = 0.0f;
    for (int i = threadIdx.x; i < P; i += GC_FINISH_THREADS) acc += p[i];
    const float sum = tree_sum<GC_FINISH_THREADS>(acc, lds);
    if (threadIdx.x != 0) return;
    const float norm = sqrtf(sum);
    const float q = F.max_norm / (norm + 1e-6f);
    if (F.norm_out) F.norm_out[e] = norm;
    F.coef_out[e] = q > 1.0f ? 1.0f : q;
}

static int64_t chunks_of(int64_t numel) { return (numel + GC_CHUNK - 1) / GC_CHUNK; }

// Member e's number of partials; the members' partials follow each other in the workspace.
static int64_t member_partials(const mbrl_adam_tensor* tensors, int e, int count) {
    int64_t P = 0;
    for (int i = 0; i < count; ++i) P += chunks_of(tensors[(int64_t)e * count + i].numel);
    return P;
}

int grad_clip_table_check(const char* what, const mbrl_adam_tensor* tensors, int E, int count, bool adam) {
    if (E < 1 || count < 1 || !tensors) return fail(MBRL_EINVAL, "%s: E = %d, count = %d or a NULL table", what, E, count);
    if (E > MBRL_TRAIN_MAX_MEMBERS)
        return fail(MBRL_EUNSUPPORTED, "%s: E = %d members exceeds MBRL_TRAIN_MAX_MEMBERS = %d", what, E,
                    MBRL_TRAIN_MAX_MEMBERS);
    for (int e = 0; e < E; ++e) {
        for (int i = 0; i < count; ++i) {
            const mbrl_adam_tensor& t = tensors[(int64_t)e * count + i];
            if (t.numel < 0 || (t.numel > 0 && (!t.grad || (adam && (!t.param || !t.exp_avg || !t.exp_avg_sq)))))
                return fail(MBRL_EINVAL, "%s: member %d, tensor %d: NULL pointer or negative numel", what, e, i);
        }
        if (member_partials(tensors, e, count) >= ((int64_t)1 << 31) / MBRL_TRAIN_MAX_MEMBERS)
            return fail(MBRL_EUNSUPPORTED, "%s: member %d's gradients exceed 2^28 chunks of %d", what, e, GC_CHUNK);
    }
    return MBRL_OK;
}

static size_t grad_clip_ws_bytes(const mbrl_adam_tensor* tensors, int E, int count) {
    int64_t floats = GC_COEF_FLOATS;
    for (int e = 0; e < E; ++e) floats += member_partials(tensors, e, count);
    return (size_t)floats * sizeof(float);
}

int grad_clip_check(const char* what, const mbrl_grad_clip* clip, const mbrl_adam_tensor* tensors, int E, int count) {
    if (!clip) return fail(MBRL_EINVAL, "%s: NULL clip", what);
    if (!(clip->max_norm > 0.0f)) return fail(MBRL_EINVAL, "%s: max_norm %g is not positive", what, clip->max_norm);
    if (!clip->workspace || (reinterpret_cast<uintptr_t>(clip->workspace) & 3))
        return fail(MBRL_EINVAL, "%s: clip workspace NULL or not 4-byte aligned", what);
    if (int rc = grad_clip_table_check(what, tensors, E, count, true)) return rc;
    const size_t need = grad_clip_ws_bytes(tensors, E, count);
    if (clip->ws_bytes < need)
        return fail(MBRL_EWORKSPACE, "%s: clip workspace %zu < %zu bytes", what, clip->ws_bytes, need);
    return MBRL_OK;
}

// The two norm launches (checked arguments): the chunk partials of all E * count tensors into `partials`
// (GC_TENSORS per launch; more take further launches), then one workgroup per member.
hipError_t launch_grad_norm(const mbrl_adam_tensor* tensors, int E, int count, float max_norm, float* norm_out,
                            float* coef_out, float* partials, hipStream_t stream) {
    GradSumsqLaunch L{};
    GradNormFinish F{};
    F.max_norm = max_norm;
    F.norm_out = norm_out;
    F.coef_out = coef_out;
    float* next = partials;
    int blocks = 0;
    const int total = E * count;
    for (int i = 0; i <= total; ++i) {
        if (L.count == GC_TENSORS || (i == total && L.count > 0)) {
            L.first_block[L.count] = blocks;
            hipLaunchKernelGGL(grad_sumsq_kernel, dim3(blocks), dim3(GC_THREADS), 0, stream, L);
            const hipError_t e = hipGetLastError();
            if (e != hipSuccess) return e;
            L.count = 0;
            blocks = 0;
        }
        if (i == total) break;
        if (i % count == 0) F.partial[i / count] = next;
        const int64_t n = chunks_of(tensors[i].numel);
        if (n == 0) continue;
        L.grad[L.count] = tensors[i].grad;
        L.partial[L.count] = next;
        L.numel[L.count] = tensors[i].numel;
        L.first_block[L.count] = blocks;
        ++L.count;
        blocks += (int)n;
        next += n;
        F.P[i / count] += (int)n;
    }
    hipLaunchKernelGGL(grad_norm_finish_kernel, dim3(E), dim3(GC_FINISH_THREADS), 0, stream, F);
    return hipGetLastError();
}

hipError_t launch_grad_clip_step(const mbrl_adam_tensor* tensors, int E, int count, const mbrl_adam_hparams& hp,
                                 int arith, const mbrl_grad_clip& clip, int64_t batch, hipStream_t stream) {
    float* ws = static_cast<float*>(clip.workspace);
    const hipError_t e = launch_grad_norm(tensors, E, count, clip.max_norm, clip.norms ? clip.norms + batch * E : nullptr,
                                          ws, ws + GC_COEF_FLOATS, stream);
    if (e != hipSuccess) return e;
    return launch_adam_step_clipped(tensors, E, count, hp, arith, ws, stream);
}

}  // namespace mbrl

using namespace mbrl;

extern "C" {

size_t mbrl_grad_clip_workspace_bytes(const mbrl_adam_tensor* tensors, int32_t E, int32_t count) {
    if (grad_clip_table_check("grad_clip_workspace_bytes", tensors, E, count, false) != MBRL_OK) return 0;
    return grad_clip_ws_bytes(tensors, E, count);
}

int mbrl_grad_norm(const mbrl_adam_tensor* tensors, int32_t E, int32_t count, float max_norm, float* norm_out,
                   float* coef_out, void* ws, size_t ws_bytes, mbrl_stream_t stream) {
    const char* what = "grad_norm";
    if (!(max_norm > 0.0f)) return fail(MBRL_EINVAL, "%s: max_norm %g is not positive", what, max_norm);
    if (!coef_out || !ws || (reinterpret_cast<uintptr_t>(ws) & 3))
        return fail(MBRL_EINVAL, "%s: NULL coef_out, or a workspace NULL or not 4-byte aligned", what);
    if (int rc = grad_clip_table_check(what, tensors, E, count, false)) return rc;
    const size_t need = grad_clip_ws_bytes(tensors, E, count);
    if (ws_bytes < need) return fail(MBRL_EWORKSPACE, "%s: workspace %zu < %zu bytes", what, ws_bytes, need);
    return hip_check(launch_grad_norm(tensors, E, count, max_norm, norm_out, coef_out,
                                      static_cast<float*>(ws) + GC_COEF_FLOATS, reinterpret_cast<hipStream_t>(stream)),
                     what);
}

}  // extern "C"
