// Building blocks of the hand-written LSD radix sorts (fused_edges.hip: the edge lists; adjust.hip: the p-value keys).
// A chunk of keys belongs to ONE wave, which walks it slice by slice (64 keys): the lanes holding the same 8-bit digit
// find each other with eight ballots (same_digit), a lane's place is the chunk's running count of its digit plus the
// number of lower lanes in its group — stable by construction, no atomics, no cross-wave ranking.  The [256][chunks]
// digit table is turned into start offsets by exclusive_scan.
#pragma once

#include "common.hpp"

// internal linkage: every source that includes this gets its own kernels (each is registered with its own code object)
namespace {
namespace skr_radix {

constexpr int kDigits = 256;

// lanes of the wave that hold the same 8-bit digit as this one (all 64 lanes take part; `live` lanes only match live ones)
__device__ __forceinline__ unsigned long long same_digit(uint32_t d, bool live) {
    unsigned long long peers = __ballot(live);
#pragma unroll
    for (int b = 0; b < 8; b++) {
        const unsigned long long ones = __ballot(live && ((d >> b) & 1u));
        peers &= ((d >> b) & 1u) ? ones : ~ones;
    }
    return peers;
}

// ---- exclusive prefix sum of a uint32 / uint64 array in place (any length): block totals -> recursive scan of the
// totals -> local scan with the block's offset.  4 096 elements per 256-thread block.
constexpr int kScanBlock = 256, kScanPer = 16, kScanTile = kScanBlock * kScanPer;

template <typename U>
__device__ __forceinline__ U block_exclusive_scan(U v, U* lds, U* total) {
    // wave scan, then the four wave totals
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    U incl = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const U up = __shfl_up(incl, off, 64);
        if (lane >= off) incl += up;
    }
    if (lane == 63) lds[wave] = incl;
    __syncthreads();
    U before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < kScanBlock / 64; w++) {
        const U t = lds[w];
        if (w < wave) before += t;
        all += t;
    }
    __syncthreads();
    *total = all;
    return before + incl - v;
}

template <typename U>
__global__ __launch_bounds__(kScanBlock) void scan_totals_kernel(const U* __restrict__ x, int64_t n, U* __restrict__ totals) {
    __shared__ U lds[kScanBlock / 64];
    const int64_t base = (int64_t)blockIdx.x * kScanTile + (int64_t)threadIdx.x * kScanPer;
    U s = 0;
#pragma unroll
    for (int j = 0; j < kScanPer; j++)
        if (base + j < n) s += x[base + j];
    U total;
    (void)block_exclusive_scan(s, lds, &total);
    if (threadIdx.x == 0) totals[blockIdx.x] = total;
}

// offsets == nullptr: a single block scans the whole (short) array
template <typename U>
__global__ __launch_bounds__(kScanBlock) void scan_local_kernel(U* __restrict__ x, int64_t n, const U* __restrict__ offsets) {
    __shared__ U lds[kScanBlock / 64];
    const int64_t base = (int64_t)blockIdx.x * kScanTile + (int64_t)threadIdx.x * kScanPer;
    U v[kScanPer], s = 0;
#pragma unroll
    for (int j = 0; j < kScanPer; j++) {
        v[j] = base + j < n ? x[base + j] : (U)0;
        s += v[j];
    }
    U total;
    U run = block_exclusive_scan(s, lds, &total) + (offsets ? offsets[blockIdx.x] : (U)0);
#pragma unroll
    for (int j = 0; j < kScanPer; j++) {
        if (base + j < n) x[base + j] = run;
        run += v[j];
    }
}

// scratch: at least scan_scratch_words(n) elements behind the array's own storage
inline size_t scan_scratch_words(int64_t n) {
    size_t words = 0;
    while (n > kScanTile) {
        n = (n + kScanTile - 1) / kScanTile;
        words += (size_t)n;
    }
    return words;
}

template <typename U>
int exclusive_scan(skr_ctx* ctx, U* x, int64_t n, U* scratch) {
    if (n <= kScanTile) {
        hipLaunchKernelGGL(scan_local_kernel<U>, dim3(1), dim3(kScanBlock), 0, ctx->stream, x, n, (const U*)nullptr);
        SKR_HIP(hipGetLastError());
        return SKR_OK;
    }
    const int64_t blocks = (n + kScanTile - 1) / kScanTile;
    hipLaunchKernelGGL(scan_totals_kernel<U>, dim3((unsigned)blocks), dim3(kScanBlock), 0, ctx->stream, x, n, scratch);
    SKR_HIP(hipGetLastError());
    SKR_TRY(exclusive_scan<U>(ctx, scratch, blocks, scratch + blocks));
    hipLaunchKernelGGL(scan_local_kernel<U>, dim3((unsigned)blocks), dim3(kScanBlock), 0, ctx->stream, x, n, (const U*)scratch);
    SKR_HIP(hipGetLastError());
    return SKR_OK;
}

}  // namespace skr_radix
}  // namespace
