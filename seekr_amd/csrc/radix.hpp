// The hand-written LSD radix sort, 8 bits per pass, and the exclusive prefix sum it needs.  Users (fused_edges.hip: the
// edge lists; adjust.hip: the p-value keys) describe their keys in a policy struct and keep their own pass loop; the
// kernels, the chunk rule and the pass driver are here.
// A chunk of keys belongs to ONE wave, which walks it slice by slice (64 keys): the lanes holding the same 8-bit digit
// find each other with eight ballots (same_digit), a lane's place is the chunk's running count of its digit plus the
// number of lower lanes in its group — stable by construction, no atomics, no cross-wave ranking.  The [256][chunks]
// digit table is turned into start offsets by exclusive_scan (also used on its own: consumers.hip, the row offsets of
// skr_edges).
#pragma once

#include <algorithm>

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

// ---- the chunk rule.  Keys per wave: enough waves to fill the chip on short lists (16 per CU), at most kMaxChunk keys
// each on long ones (the [256][chunks] table stays at n / 32 words).  Both limits are multiples of 64.
constexpr int64_t kMinChunk = 512, kMaxChunk = 8192;
inline int64_t want_waves(const skr_ctx* ctx) { return (int64_t)ctx->num_cu * 16; }

struct Chunks {
    int64_t chunk = 0, n_chunks = 0;         // chunk: a multiple of 64
    size_t table_words = 0, scan_words = 0;  // the digit table, and exclusive_scan's scratch for it
};

inline Chunks plan_chunks(const skr_ctx* ctx, int64_t n) {
    Chunks p;
    const int64_t W = want_waves(ctx);
    const int64_t chunk = std::min(kMaxChunk, std::max(kMinChunk, (n + W - 1) / W));
    p.chunk = (chunk + 63) / 64 * 64;
    p.n_chunks = std::max<int64_t>(1, (n + p.chunk - 1) / p.chunk);
    p.table_words = (size_t)kDigits * (size_t)p.n_chunks;
    p.scan_words = scan_scratch_words((int64_t)p.table_words);
    return p;
}

// The largest table_words plan_chunks gives for any 1 <= n <= cap.  n_chunks is not monotone in n (the rounding of
// chunk to a multiple of 64 makes it step down), so plan_chunks(cap) alone is not the bound.  With W = want_waves,
// lo = kMinChunk, hi = kMaxChunk and chunk(n) = round64(clamp(ceil(n / W), lo, hi)), which stays within [lo, hi]:
//   n <= lo W:       chunk = lo, n_chunks = ceil(n / lo) <= min(ceil(cap / lo), W)
//   lo W < n <= hi W:  chunk >= ceil(n / W) gives n_chunks <= W, chunk >= lo gives n_chunks <= ceil(cap / lo)
//   n > hi W:        chunk = hi, n_chunks = ceil(n / hi) <= ceil(cap / hi)
// The first bound is reached at n = min(cap, lo W), the last at n = cap: the maximum of the two is tight.
// scan_scratch_words grows with its argument, so the scratch of this table covers every smaller one.
inline size_t max_table_words(const skr_ctx* ctx, int64_t cap) {
    const int64_t by_lo = (cap + kMinChunk - 1) / kMinChunk, by_hi = (cap + kMaxChunk - 1) / kMaxChunk;
    return (size_t)kDigits * (size_t)std::max(std::min(by_lo, want_waves(ctx)), by_hi);
}

// bits needed to hold v: a sort over a field whose largest value is v takes ceil(bit_length(v) / 8) passes
inline int bit_length(uint64_t v) {
    int b = 0;
    while (v) {
        b++;
        v >>= 1;
    }
    return b;
}

// ---- one pass of the sort: digit histogram per chunk -> exclusive scan of the table -> stable scatter.  The policy P
// (a plain struct, passed to the kernels by value) says what a key is:
//   using Count                  word of the digit table and of the running starts (uint32_t below 2^32 keys)
//   using Item                   what travels: the key, plus its payload if any
//   Item load(int64_t i)         (a first pass may convert raw input here)
//   uint32_t digit(const Item&)  the 8-bit digit of this pass
//   void store(Count pos, const Item&)   (a last pass may write a different layout here)
template <typename Count>
struct Pass {
    int64_t n, chunk, n_chunks;
    Count* table;  // [256][n_chunks] counts, then (scanned in place) start offsets
};

template <class P>
__global__ __launch_bounds__(64) void count_kernel(const P p, const Pass<typename P::Count> a) {
    __shared__ uint32_t cnt[kDigits];
    const int lane = threadIdx.x;
    const int64_t c = blockIdx.x;
    for (int d = lane; d < kDigits; d += 64) cnt[d] = 0;
    __syncthreads();
    const int64_t begin = c * a.chunk, end = std::min(a.n, begin + a.chunk);
    for (int64_t i = begin + lane; i - lane < end; i += 64) {
        const bool live = i < end;
        const uint32_t d = live ? p.digit(p.load(i)) : 0u;
        const unsigned long long peers = same_digit(d, live);
        // the highest lane of each group books the whole group: one LDS add per distinct digit and slice
        if (live && (peers >> lane) == 1ull) cnt[d] += (uint32_t)__popcll(peers);
        __syncthreads();
    }
    for (int d = lane; d < kDigits; d += 64) a.table[(size_t)d * a.n_chunks + c] = cnt[d];
}

template <class P>
__global__ __launch_bounds__(64) void scatter_kernel(const P p, const Pass<typename P::Count> a) {
    using Count = typename P::Count;
    __shared__ Count base[kDigits];
    const int lane = threadIdx.x;
    const int64_t c = blockIdx.x;
    for (int d = lane; d < kDigits; d += 64) base[d] = a.table[(size_t)d * a.n_chunks + c];
    __syncthreads();
    const unsigned long long below = lane ? (~0ull >> (64 - lane)) : 0ull;
    const int64_t begin = c * a.chunk, end = std::min(a.n, begin + a.chunk);
    for (int64_t i = begin + lane; i - lane < end; i += 64) {
        const bool live = i < end;
        typename P::Item it{};
        if (live) it = p.load(i);  // the whole item (key and payload) before the ballots
        const uint32_t d = live ? p.digit(it) : 0u;
        const unsigned long long peers = same_digit(d, live);
        Count pos = 0;
        if (live) pos = base[d] + (Count)__popcll(peers & below);
        __syncthreads();  // every lane has read its digit's running start before any group leader moves it
        if (live) {
            if ((peers >> lane) == 1ull) base[d] += (Count)__popcll(peers);
            p.store(pos, it);
        }
        __syncthreads();
    }
}

// scan_scratch: at least plan.scan_words words
template <class P>
int run_pass(skr_ctx* ctx, const P& p, int64_t n, const Chunks& plan, typename P::Count* table, typename P::Count* scan_scratch) {
    using Count = typename P::Count;
    const Pass<Count> a{n, plan.chunk, plan.n_chunks, table};
    hipLaunchKernelGGL(count_kernel<P>, dim3((unsigned)plan.n_chunks), dim3(64), 0, ctx->stream, p, a);
    SKR_HIP(hipGetLastError());
    SKR_TRY(exclusive_scan<Count>(ctx, table, (int64_t)plan.table_words, scan_scratch));
    hipLaunchKernelGGL(scatter_kernel<P>, dim3((unsigned)plan.n_chunks), dim3(64), 0, ctx->stream, p, a);
    SKR_HIP(hipGetLastError());
    return SKR_OK;
}

}  // namespace skr_radix
}  // namespace
