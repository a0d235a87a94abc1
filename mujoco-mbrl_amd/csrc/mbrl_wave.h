// Wave64 cross-lane helpers shared by the selection / refit kernels (cem.hip) and the MPPI update
// (mppi.hip): DPP moves, the wave scan, wave minimum / maximum, the ballot and the block scan.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mbrl {

// Canonical chunk length of the elite sums and of the MPPI weighted sums (oracle/cem.py ELITE_CHUNK).
constexpr int ELITE_CHUNK = 32;

// Cross-lane moves as DPP operand modifiers (VALU, no LDS round trip as __shfl's ds_bpermute takes).
// Lanes whose source is outside the row, or whose row is not in ROWS, read 0.
template <int CTRL, int ROWS = 0xF>
__device__ __forceinline__ uint32_t dpp_u32(uint32_t x) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, CTRL, ROWS, 0xF, false);
}

// Inclusive prefix sum over the wave: in-row shifts by 1, 2, 4, 8, then the row broadcasts.
__device__ __forceinline__ uint32_t wave_inclusive_scan(uint32_t x) {
    x += dpp_u32<0x111>(x);        // row_shr:1
    x += dpp_u32<0x112>(x);        // row_shr:2
    x += dpp_u32<0x114>(x);        // row_shr:4
    x += dpp_u32<0x118>(x);        // row_shr:8
    x += dpp_u32<0x142, 0xA>(x);   // row_bcast:15 (rows 1 and 3)
    x += dpp_u32<0x143, 0xC>(x);   // row_bcast:31 (rows 2 and 3)
    return x;
}

// Wave minimum / maximum: every lane of a row gets the row's (quad swaps, half mirror, mirror), then the
// four rows' through readlane.
__device__ __forceinline__ uint32_t wave_min_u32(uint32_t x) {
    x = min(x, dpp_u32<0xB1>(x));
    x = min(x, dpp_u32<0x4E>(x));
    x = min(x, dpp_u32<0x141>(x));
    x = min(x, dpp_u32<0x140>(x));
    return min(min((uint32_t)__builtin_amdgcn_readlane((int)x, 0), (uint32_t)__builtin_amdgcn_readlane((int)x, 16)),
               min((uint32_t)__builtin_amdgcn_readlane((int)x, 32), (uint32_t)__builtin_amdgcn_readlane((int)x, 48)));
}
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t x) {
    x = max(x, dpp_u32<0xB1>(x));
    x = max(x, dpp_u32<0x4E>(x));
    x = max(x, dpp_u32<0x141>(x));
    x = max(x, dpp_u32<0x140>(x));
    return max(max((uint32_t)__builtin_amdgcn_readlane((int)x, 0), (uint32_t)__builtin_amdgcn_readlane((int)x, 16)),
               max((uint32_t)__builtin_amdgcn_readlane((int)x, 32), (uint32_t)__builtin_amdgcn_readlane((int)x, 48)));
}

// The lanes' predicate as a 64-bit mask straight from the compare (HIP's __ballot goes through a
// select and a second compare).
__device__ __forceinline__ uint64_t wave_ballot(bool p) { return __builtin_amdgcn_ballot_w64(p); }

__device__ __forceinline__ uint32_t block_exclusive_scan(uint32_t v, uint32_t* lds_waves, uint32_t* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const uint32_t x = wave_inclusive_scan(v);
    if (lane == 63) lds_waves[wave] = x;
    __syncthreads();
    uint32_t before = 0, all = 0;   // every wave sums the wave totals itself (broadcast reads)
    for (int w = 0; w < nw; ++w) {
        const uint32_t t = lds_waves[w];
        before += w < wave ? t : 0u;
        all += t;
    }
    *total = all;
    __syncthreads();
    return before + x - v;
}

}  // namespace mbrl
