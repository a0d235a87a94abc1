// Device-resident transitions (include/mbrl_cem.h mbrl_dataset_stack, mbrl_dataset_stats): what
// DeviceTransitionsDataset enqueues in place of the host's per-transition Python loops.
//
// Step store: one row-major fp32 array [S][dim] per field; a rollout with K transitions holds K + 1 consecutive
// rows, so the `horizon` steps of a window are horizon * dim CONSECUTIVE floats of the store, starting at row
// win_row[t] + shift. mbrl_dataset_stack (dataset_stack_kernel, one launch for up to 8 fields) therefore walks
// every destination linearly: a workgroup owns 1024 consecutive dst elements of one field, lane l of 256 takes the
// elements l, l + 256, l + 512, l + 768 of them, so every load and every store instruction of a wave covers 256
// consecutive bytes whatever the pointers' alignment is (no vector path: one dword per lane already streams at the
// rate of a copy, and there is then one path for every alignment). The element's (window, offset in the window,
// column) comes from two integer divisions for the lane's first element and from additions for the other three
// (the host passes 256 / (horizon * dim) and the two remainders). The value is (x - mean[j]) / std[j]: one fp32
// subtraction and one correctly rounded fp32 division (the file is built with -ffp-contract=off and without fast
// math), or x itself with NULL statistics.
//
// mbrl_dataset_stats: per field and column the mean, the unbiased std, the min and the max over the store rows
// rows[0 .. R), accumulated in float64 in ONE order that depends on R alone (DESIGN.md §7.6;
// tests/dataset_reference.py restates it in NumPy):
//   1. the list positions are cut into chunks of 1024, absent positions of the last chunk contributing +0.0;
//   2. in a chunk, lane t of 256 forms ((x[4t] + x[4t+1]) + x[4t+2]) + x[4t+3] and the 256 lane values meet in the
//      pairwise tree v[t] += v[t + d], d = 128 .. 1: the chunk's partial (stats_chunk_kernel);
//   3. the partials are reduced by mbrl_eval_members' rule: lane t of 1024 adds partials t, t + 1024, .. ascending
//      onto +0.0, then the pairwise tree d = 512 .. 1 (stats_finish_kernel, one workgroup per column).
// Four launches whatever the sizes are: chunk sums (with the chunk minima and maxima), finish (mean64 = sum / R kept
// in the workspace, mean, min, max out), chunk sums of (double(x) - mean64)^2, finish (std = sqrt(ss / (R - 1))).
// A chunk workgroup gathers its 1024 rows x up to 4 columns into LDS with adjacent lanes on adjacent columns of one
// row, then sums column by column; which physical lane adds what does not change the order above. The minima and
// maxima propagate a NaN, as torch.min / torch.max do. No atomics; no workgroup waits on another.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <limits>

#include "mbrl_host.h"

namespace mbrl {

// ---- mbrl_dataset_stack
constexpr int DS_STACK_FIELDS = 8;
constexpr int DS_THREADS = 256;
constexpr int DS_CHUNK = DS_THREADS * 4;     // dst elements per workgroup

struct StackLaunch {
    const float* src[DS_STACK_FIELDS];
    const float* mean[DS_STACK_FIELDS];
    const float* stdv[DS_STACK_FIELDS];
    float* dst[DS_STACK_FIELDS];
    uint32_t numel[DS_STACK_FIELDS];         // T * horizon * dim  (< 2^31)
    uint32_t hd[DS_STACK_FIELDS];            // horizon * dim: a window's floats
    uint32_t dim[DS_STACK_FIELDS];
    uint32_t shift_off[DS_STACK_FIELDS];     // shift * dim
    uint32_t q_hd[DS_STACK_FIELDS], r_hd[DS_STACK_FIELDS];   // 256 = q_hd * hd + r_hd
    uint32_t r_dim[DS_STACK_FIELDS];         // 256 % dim
    int first_block[DS_STACK_FIELDS + 1];    // workgroup prefix over the fields' chunks
    int count;
    const int64_t* win_row;
};

__global__ __launch_bounds__(DS_THREADS) void dataset_stack_kernel(const StackLaunch L) {
    const int blk = blockIdx.x;
    int f = 0;
    while (f + 1 < L.count && blk >= L.first_block[f + 1]) ++f;
    const uint32_t n = L.numel[f], hd = L.hd[f], dim = L.dim[f];
    const uint32_t q_hd = L.q_hd[f], r_hd = L.r_hd[f], r_dim = L.r_dim[f];
    const float* __restrict__ src = L.src[f] + L.shift_off[f];
    const float* __restrict__ mean = L.mean[f];
    const float* __restrict__ stdv = L.stdv[f];
    float* __restrict__ dst = L.dst[f];
    uint32_t e = (uint32_t)(blk - L.first_block[f]) * DS_CHUNK + threadIdx.x;
    uint32_t t = e / hd, rem = e - t * hd, j = rem % dim;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (e < n) {
            const float x = src[L.win_row[t] * (int64_t)dim + rem];
            dst[e] = mean ? (x - mean[j]) / stdv[j] : x;
        }
        e += DS_THREADS;
        t += q_hd;
        rem += r_hd;
        if (rem >= hd) { rem -= hd; ++t; }
        j += r_dim;                               // hd is a multiple of dim: the window seam leaves j alone
        if (j >= dim) j -= dim;
    }
}

// ---- mbrl_dataset_stats
constexpr int DS_STATS_FIELDS = 4;
constexpr int DS_COLS = 4;                     // columns per chunk workgroup (its LDS: 16 + 8 + 4 + 4 KiB)
constexpr int DS_LD = DS_CHUNK + 4;            // LDS row pitch (floats): the columns of one row in different banks
constexpr int DS_FINISH_THREADS = 1024;

// One field's slice of the workspace: sum[dim][chunks] doubles (the sums, then the sums of squares), mean64[dim]
// doubles, min[dim][chunks] and max[dim][chunks] floats.
struct StatsField {
    const float* src;
    const int64_t* rows;
    int64_t R;
    double* part;
    double* mean64;
    float* part_min;
    float* part_max;
    float* out_mean;
    float* out_std;
    float* out_min;
    float* out_max;
    int dim, chunks, tiles;
    int first_block;                           // chunk launches: workgroup prefix over the fields' chunks x tiles
    int first_col;                             // finish launches: prefix over the fields' columns
};

struct StatsLaunch {
    StatsField f[DS_STATS_FIELDS];
    int count;
};

// NaN-propagating, like torch.min / torch.max
__device__ __forceinline__ float nan_min(float a, float b) { return a != a ? a : (b != b ? b : (b < a ? b : a)); }
__device__ __forceinline__ float nan_max(float a, float b) { return a != a ? a : (b != b ? b : (b > a ? b : a)); }

// SECOND = false: the chunk's column sums, minima and maxima; true: its sums of (double(x) - mean64)^2.
template <bool SECOND>
__global__ __launch_bounds__(DS_THREADS) void stats_chunk_kernel(const StatsLaunch L) {
    __shared__ __attribute__((aligned(16))) float x_lds[DS_COLS * DS_LD];
    __shared__ double red[DS_COLS][DS_THREADS];
    __shared__ float red_min[SECOND ? 1 : DS_COLS][SECOND ? 1 : DS_THREADS];
    __shared__ float red_max[SECOND ? 1 : DS_COLS][SECOND ? 1 : DS_THREADS];
    const int blk = blockIdx.x, tid = threadIdx.x;
    int fi = 0;
    while (fi + 1 < L.count && blk >= L.f[fi + 1].first_block) ++fi;
    const StatsField& F = L.f[fi];
    const int local = blk - F.first_block;
    const int chunk = local / F.tiles, tile = local - chunk * F.tiles;
    const int j0 = tile * DS_COLS, ct = F.dim - j0 < DS_COLS ? F.dim - j0 : DS_COLS;
    const int64_t p0 = (int64_t)chunk * DS_CHUNK;
    const int valid = F.R - p0 < DS_CHUNK ? (int)(F.R - p0) : DS_CHUNK;   // positions of this chunk that exist (>= 1)
    // gather: adjacent lanes take adjacent columns of one row; absent positions hold +0.0
    for (int idx = tid; idx < DS_CHUNK * ct; idx += DS_THREADS) {
        const int p = idx / ct, jj = idx - p * ct;
        x_lds[jj * DS_LD + p] = p < valid ? F.src[F.rows[p0 + p] * (int64_t)F.dim + j0 + jj] : 0.0f;
    }
    __syncthreads();
    const int have = valid - 4 * tid;                             // this lane's positions 0 .. have - 1 exist
    for (int jj = 0; jj < ct; ++jj) {
        const float4 x = *reinterpret_cast<const float4*>(&x_lds[jj * DS_LD + 4 * tid]);
        double a = x.x, b = x.y, c = x.z, d = x.w;
        if (SECOND) {
            const double m = F.mean64[j0 + jj];
            a = have > 0 ? (a - m) * (a - m) : 0.0;
            b = have > 1 ? (b - m) * (b - m) : 0.0;
            c = have > 2 ? (c - m) * (c - m) : 0.0;
            d = have > 3 ? (d - m) * (d - m) : 0.0;
        } else {
            float lo = std::numeric_limits<float>::infinity(), hi = -std::numeric_limits<float>::infinity();
            if (have > 0) { lo = nan_min(lo, x.x); hi = nan_max(hi, x.x); }
            if (have > 1) { lo = nan_min(lo, x.y); hi = nan_max(hi, x.y); }
            if (have > 2) { lo = nan_min(lo, x.z); hi = nan_max(hi, x.z); }
            if (have > 3) { lo = nan_min(lo, x.w); hi = nan_max(hi, x.w); }
            red_min[jj][tid] = lo;
            red_max[jj][tid] = hi;
        }
        red[jj][tid] = ((a + b) + c) + d;
    }
    __syncthreads();
    for (int d = DS_THREADS / 2; d >= 1; d >>= 1) {
        if (tid < d) {
            for (int jj = 0; jj < ct; ++jj) {
                red[jj][tid] += red[jj][tid + d];
                if (!SECOND) {
                    red_min[jj][tid] = nan_min(red_min[jj][tid], red_min[jj][tid + d]);
                    red_max[jj][tid] = nan_max(red_max[jj][tid], red_max[jj][tid + d]);
                }
            }
        }
        __syncthreads();
    }
    if (tid < ct) {
        const int64_t at = (int64_t)(j0 + tid) * F.chunks + chunk;
        F.part[at] = red[tid][0];
        if (!SECOND) {
            F.part_min[at] = red_min[tid][0];
            F.part_max[at] = red_max[tid][0];
        }
    }
}

// One workgroup per column: mbrl_eval_members' rule over the column's chunk partials.
template <bool SECOND>
__global__ __launch_bounds__(DS_FINISH_THREADS) void stats_finish_kernel(const StatsLaunch L) {
    __shared__ double red[DS_FINISH_THREADS];
    __shared__ float red_min[SECOND ? 1 : DS_FINISH_THREADS];
    __shared__ float red_max[SECOND ? 1 : DS_FINISH_THREADS];
    const int blk = blockIdx.x, tid = threadIdx.x;
    int fi = 0;
    while (fi + 1 < L.count && blk >= L.f[fi + 1].first_col) ++fi;
    const StatsField& F = L.f[fi];
    const int j = blk - F.first_col;
    const double* p = F.part + (int64_t)j * F.chunks;
    double acc = 0.0;
    for (int i = tid; i < F.chunks; i += DS_FINISH_THREADS) acc += p[i];
    red[tid] = acc;
    if (!SECOND) {
        float lo = std::numeric_limits<float>::infinity(), hi = -std::numeric_limits<float>::infinity();
        for (int i = tid; i < F.chunks; i += DS_FINISH_THREADS) {
            lo = nan_min(lo, F.part_min[(int64_t)j * F.chunks + i]);
            hi = nan_max(hi, F.part_max[(int64_t)j * F.chunks + i]);
        }
        red_min[tid] = lo;
        red_max[tid] = hi;
    }
    __syncthreads();
    for (int d = DS_FINISH_THREADS / 2; d >= 1; d >>= 1) {
        if (tid < d) {
            red[tid] += red[tid + d];
            if (!SECOND) {
                red_min[tid] = nan_min(red_min[tid], red_min[tid + d]);
                red_max[tid] = nan_max(red_max[tid], red_max[tid + d]);
            }
        }
        __syncthreads();
    }
    if (tid != 0) return;
    if (SECOND) {
        F.out_std[j] = (float)sqrt(red[0] / (double)(F.R - 1));   // R = 1: 0 / 0 = NaN, as torch.std
    } else {
        const double mean64 = red[0] / (double)F.R;
        F.mean64[j] = mean64;
        F.out_mean[j] = (float)mean64;
        F.out_min[j] = red_min[0];
        F.out_max[j] = red_max[0];
    }
}

static int64_t stats_chunks(int64_t R) { return (R + DS_CHUNK - 1) / DS_CHUNK; }

// The argument checks both stats entries share (everything but the workspace), all before any launch.
static int stats_check(const char* what, const mbrl_stats_field* fields, int count, bool outputs) {
    if (!fields || count < 1 || count > DS_STATS_FIELDS)
        return fail(MBRL_EINVAL, "%s: count = %d fields (1 .. %d) or a NULL table", what, count, DS_STATS_FIELDS);
    for (int i = 0; i < count; ++i) {
        const mbrl_stats_field& f = fields[i];
        if (f.R < 1) return fail(MBRL_EINVAL, "%s: field %d: R = %lld rows", what, i, (long long)f.R);
        if (outputs && (!f.src || !f.rows || !f.mean || !f.std || !f.min || !f.max))
            return fail(MBRL_EINVAL, "%s: field %d: NULL src, rows or output", what, i);
        if (f.dim < 1 || f.dim > MBRL_EVAL_MAX_DIM)
            return fail(MBRL_EUNSUPPORTED, "%s: field %d: dim = %d is outside 1 .. %d", what, i, f.dim, MBRL_EVAL_MAX_DIM);
        // chunks x column tiles of all fields in one grid
        if (stats_chunks(f.R) * ((f.dim + DS_COLS - 1) / DS_COLS) >= ((int64_t)1 << 31) / DS_STATS_FIELDS)
            return fail(MBRL_EUNSUPPORTED, "%s: field %d: R = %lld rows x dim = %d is too large for one launch's grid",
                        what, i, (long long)f.R, f.dim);
    }
    return MBRL_OK;
}

// one field's workspace bytes: the doubles first, so that every slice stays 8-byte aligned
static size_t stats_field_bytes(const mbrl_stats_field& f) {
    const size_t cells = (size_t)f.dim * (size_t)stats_chunks(f.R);
    return cells * sizeof(double) + (size_t)f.dim * sizeof(double) + 2 * cells * sizeof(float);
}

static size_t stats_ws_bytes(const mbrl_stats_field* fields, int count) {
    size_t bytes = 0;
    for (int i = 0; i < count; ++i) bytes += stats_field_bytes(fields[i]);
    return bytes;
}

}  // namespace mbrl

using namespace mbrl;

// ---- ABI entries (include/mbrl_cem.h)
extern "C" {

int mbrl_dataset_stack(const mbrl_stack_field* fields, int32_t count, const int64_t* win_row, int64_t T,
                       int32_t horizon, mbrl_stream_t stream) {
    const char* what = "dataset_stack";
    if (!fields || !win_row) return fail(MBRL_EINVAL, "%s: NULL fields or win_row", what);
    if (count < 1 || count > DS_STACK_FIELDS || T < 1 || horizon < 1)
        return fail(MBRL_EINVAL, "%s: count = %d fields (1 .. %d), T = %lld, horizon = %d", what, count, DS_STACK_FIELDS,
                    (long long)T, horizon);
    for (int i = 0; i < count; ++i) {
        const mbrl_stack_field& f = fields[i];
        if (!f.src || !f.dst || (f.mean == nullptr) != (f.std == nullptr))
            return fail(MBRL_EINVAL, "%s: field %d: NULL src or dst, or mean without std", what, i);
        if (f.dim < 1 || (f.shift != 0 && f.shift != 1))
            return fail(MBRL_EINVAL, "%s: field %d: dim = %d, shift = %d", what, i, f.dim, f.shift);
    }
    StackLaunch L{};
    int64_t blocks = 0;
    for (int i = 0; i < count; ++i) {
        const mbrl_stack_field& f = fields[i];
        // T, horizon and dim are each below 2^31 here, so the first product cannot overflow
        const int64_t hd = (int64_t)horizon * f.dim;
        if (hd >= ((int64_t)1 << 31) || T >= ((int64_t)1 << 31) || T * hd >= ((int64_t)1 << 31))
            return fail(MBRL_EUNSUPPORTED, "%s: field %d: T * horizon * dim = %lld * %d * %d is not below 2^31", what, i,
                        (long long)T, horizon, f.dim);
        L.src[i] = f.src;
        L.mean[i] = f.mean;
        L.stdv[i] = f.std;
        L.dst[i] = f.dst;
        L.numel[i] = (uint32_t)(T * hd);
        L.hd[i] = (uint32_t)hd;
        L.dim[i] = (uint32_t)f.dim;
        L.shift_off[i] = (uint32_t)(f.shift * f.dim);
        L.q_hd[i] = (uint32_t)(DS_THREADS / hd);
        L.r_hd[i] = (uint32_t)(DS_THREADS % hd);
        L.r_dim[i] = (uint32_t)(DS_THREADS % f.dim);
        L.first_block[i] = (int)blocks;
        blocks += (T * hd + DS_CHUNK - 1) / DS_CHUNK;
    }
    L.first_block[count] = (int)blocks;          // <= 8 * 2^21
    L.count = count;
    L.win_row = win_row;
    hipLaunchKernelGGL(dataset_stack_kernel, dim3((unsigned)blocks), dim3(DS_THREADS), 0,
                       reinterpret_cast<hipStream_t>(stream), L);
    return hip_check(hipGetLastError(), what);
}

size_t mbrl_dataset_stats_workspace_bytes(const mbrl_stats_field* fields, int32_t count) {
    if (stats_check("dataset_stats_workspace_bytes", fields, count, false) != MBRL_OK) return 0;
    return stats_ws_bytes(fields, count);
}

int mbrl_dataset_stats(const mbrl_stats_field* fields, int32_t count, void* ws, size_t ws_bytes,
                       mbrl_stream_t stream) {
    const char* what = "dataset_stats";
    if (!ws || (reinterpret_cast<uintptr_t>(ws) & 7))
        return fail(MBRL_EINVAL, "%s: workspace NULL or not 8-byte aligned", what);
    if (int rc = stats_check(what, fields, count, true)) return rc;
    const size_t need = stats_ws_bytes(fields, count);
    if (ws_bytes < need) return fail(MBRL_EWORKSPACE, "%s: workspace %zu < %zu bytes", what, ws_bytes, need);
    StatsLaunch L{};
    L.count = count;
    char* at = static_cast<char*>(ws);
    int blocks = 0, cols = 0;
    for (int i = 0; i < count; ++i) {
        const mbrl_stats_field& f = fields[i];
        StatsField& F = L.f[i];
        F.src = f.src; F.rows = f.rows; F.R = f.R; F.dim = f.dim;
        F.out_mean = f.mean; F.out_std = f.std; F.out_min = f.min; F.out_max = f.max;
        F.chunks = (int)stats_chunks(f.R);
        F.tiles = (f.dim + DS_COLS - 1) / DS_COLS;
        const size_t cells = (size_t)f.dim * F.chunks;
        F.part = reinterpret_cast<double*>(at);
        F.mean64 = F.part + cells;
        F.part_min = reinterpret_cast<float*>(F.mean64 + f.dim);
        F.part_max = F.part_min + cells;
        at += stats_field_bytes(f);
        F.first_block = blocks;
        F.first_col = cols;
        blocks += F.chunks * F.tiles;
        cols += f.dim;
    }
    const hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(stats_chunk_kernel<false>, dim3(blocks), dim3(DS_THREADS), 0, st, L);
    if (int rc = hip_check(hipGetLastError(), what)) return rc;
    hipLaunchKernelGGL(stats_finish_kernel<false>, dim3(cols), dim3(DS_FINISH_THREADS), 0, st, L);
    if (int rc = hip_check(hipGetLastError(), what)) return rc;
    hipLaunchKernelGGL(stats_chunk_kernel<true>, dim3(blocks), dim3(DS_THREADS), 0, st, L);
    if (int rc = hip_check(hipGetLastError(), what)) return rc;
    hipLaunchKernelGGL(stats_finish_kernel<true>, dim3(cols), dim3(DS_FINISH_THREADS), 0, st, L);
    return hip_check(hipGetLastError(), what);
}

}  // extern "C"
