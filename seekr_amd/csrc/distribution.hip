// skr_hist_key_digits and skr_hist_edges: how the cells of a block of r are distributed, as 64-bit counts added into
// host arrays.  One kernel, two binning rules; nothing stays on the device between calls, and the counts are integers, so
// the same input gives the same numbers on every run.
//
// Cell rule: every cell of r[0:nrows, col_begin:col_end] is counted; with upper_only only the cells whose global column
// (col_global0 + j) is greater than their global row (row_global0 + i) — skr_edges' rule.  There is no zero rule.
// NaN rule: a NaN cell of either sign bit goes into a counter of its own and into no bin.
//
// Key digits: key(v) is float_key.hpp's uint32, whose order is the order of the float32 values, -0 just below +0
// (significant._key).
// A cell whose top prefix_bits key bits equal prefixes[q] adds one to hist[q][(key >> shift) & (2^bits - 1)]; with
// prefix_bits = 0 there is one histogram of every cell.  A radix descent over the key (distribution.py) is three such
// passes.  Edge table: bin b holds edges[b] <= v < edges[b + 1], the last bin is closed on the right, and the cells
// below edges[0] and above edges[n - 1] are counted apart.  The bin is found by bisection over the table in LDS.
//
// Tiling: cell_tile.hpp's, as skr_select_cells_ge — one row x one segment of 1 024 columns, 16-byte loads aligned in the
// row's memory, grid-stride over the tiles; a workgroup takes two tiles per step so that two loads are in flight per
// lane.  Each workgroup counts into an LDS histogram of uint32 (a workgroup never sees 2^32 cells: the grid is sized so)
// and at its end adds the non-zero bins into 64-bit counters in the ctx's workspace, which the host downloads and adds
// to the caller's arrays.  Static LDS: 32 KB (key digits: kDistKeyBins counters) and 33 KB (edge table: 4 096 counters
// and 4 097 edges).
//
// Lanes that hit one bin: plain LDS atomics, after `dist_match` rounds (SkrKnobs, default 0) in which the wave's first
// pending lane broadcasts its bin and the lanes that hold the same one are counted by a ballot and added once.
#include <algorithm>
#include <cmath>
#include <vector>

#include "cell_tile.hpp"
#include "common.hpp"
#include "float_key.hpp"

namespace {

constexpr int kDistKeyBins = 8192;    // n_prefixes << bits at most
constexpr int kDistMaxEdges = 4097;
constexpr int kDistMaxPrefixes = 8;
constexpr int kDistMatchRounds = 2;   // the rounds of the matching arm

struct DistArgs {
    int upper_only;
    int shift, bits, prefix_bits, n_prefixes;  // key digits
    uint32_t prefixes[kDistMaxPrefixes];
    int n_edges;                               // edge table
    int total_bins;                            // counters behind one another: the bins, then below, above (edge table), nan
};

// the counter of one cell: -1 for a cell that is not counted
template <bool kEdges>
__device__ __forceinline__ int dist_bin(const DistArgs& d, const float* edges, float v, bool counted) {
    if (!counted) return -1;
    if (v != v) return d.total_bins - 1;
    if (kEdges) {
        const int nb = d.n_edges - 1;
        if (v < edges[0]) return nb;
        if (v > edges[nb]) return nb + 1;
        int lo = 0, hi = nb;  // edges[lo] <= v, and v < edges[hi] or hi == nb: the bin is the last lo with edges[lo] <= v
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (edges[mid] <= v)
                lo = mid;
            else
                hi = mid;
        }
        return lo;
    } else {
        const uint32_t key = skr_float_key(v);
        const uint32_t top = d.prefix_bits ? key >> (32 - d.prefix_bits) : 0u;
        const int digit = (int)((key >> d.shift) & ((1u << d.bits) - 1u));
        int q = -1;
#pragma unroll
        for (int i = 0; i < kDistMaxPrefixes; i++)
            if (i < d.n_prefixes && top == d.prefixes[i]) q = i;
        return q < 0 ? -1 : (q << d.bits) + digit;
    }
}

template <int kMatch>
__device__ __forceinline__ void dist_add(unsigned* hist, int bin) {
    bool todo = bin >= 0;
#pragma unroll
    for (int round = 0; round < kMatch; round++) {
        if (todo) {  // the lanes still pending: the first one names a bin, every lane that holds it is counted at once
            const int named = __builtin_amdgcn_readfirstlane(bin);
            if (bin == named) {
                const unsigned long long same = __ballot(1);
                if ((int)(threadIdx.x & 63) == __ffsll((long long)same) - 1) atomicAdd(&hist[named], (unsigned)__popcll(same));
                todo = false;
            }
        }
    }
    if (todo) atomicAdd(&hist[bin], 1u);
}

template <bool kEdges, int kMatch>
__global__ __launch_bounds__(kCellBlock) void dist_hist_pass(CellArgs a, DistArgs d, const float* __restrict__ g_edges,
                                                               unsigned long long* __restrict__ g_counts) {
    __shared__ unsigned hist[kEdges ? kDistMaxEdges - 1 + 3 : kDistKeyBins + 1];
    __shared__ float edges[kEdges ? kDistMaxEdges : 1];
    for (int i = threadIdx.x; i < d.total_bins; i += kCellBlock) hist[i] = 0;
    if (kEdges)
        for (int i = threadIdx.x; i < d.n_edges; i += kCellBlock) edges[i] = g_edges[i];
    __syncthreads();
    const int64_t step = (int64_t)gridDim.x;
    for (int64_t t = blockIdx.x; t < a.tiles; t += 2 * step) {
        float v[2][kCellPer];
        bool live[2][kCellPer];
        int64_t row[2], c0[2];
        const bool second = t + step < a.tiles;  // the same for every lane of the workgroup
        load_group(a, t, v[0], live[0], row[0], c0[0]);
        if (second) load_group(a, t + step, v[1], live[1], row[1], c0[1]);
#pragma unroll
        for (int h = 0; h < 2; h++) {
            if (h == 1 && !second) break;
#pragma unroll
            for (int j = 0; j < kCellPer; j++) {
                const bool counted = live[h][j] && (!d.upper_only || a.b.col_global0 + c0[h] + j > a.b.row_global0 + row[h]);
                dist_add<kMatch>(hist, dist_bin<kEdges>(d, edges, v[h][j], counted));
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < d.total_bins; i += kCellBlock) {
        const unsigned n = hist[i];
        if (n) atomicAdd(&g_counts[i], (unsigned long long)n);
    }
}

// zero the counters, run the pass, download: out[0 : total_bins] receives this block's counts
int dist_run(skr_ctx* ctx, const CellArgs& a, const DistArgs& d, const float* h_edges, std::vector<unsigned long long>* out) {
    out->assign((size_t)d.total_bins, 0ull);
    if (a.tiles == 0) return SKR_OK;
    SKR_TRY(skr_activate(ctx));
    void* ws = nullptr;
    const size_t count_bytes = (size_t)d.total_bins * 8;
    SKR_TRY(skr_ctx_workspace(ctx, count_bytes + (size_t)kDistMaxEdges * 4, &ws));
    unsigned long long* g_counts = (unsigned long long*)ws;
    float* g_edges = (float*)((char*)ws + count_bytes);
    SKR_HIP(hipMemsetAsync(g_counts, 0, count_bytes, ctx->stream));
    if (h_edges) SKR_HIP(hipMemcpyAsync(g_edges, h_edges, (size_t)d.n_edges * 4, hipMemcpyHostToDevice, ctx->stream));
    // at least 2^20 tiles per workgroup would be needed for 2^32 cells in one: the grid never lets it come to that
    const int64_t want = std::max<int64_t>((int64_t)ctx->num_cu * 4, (a.tiles + (1 << 20) - 1) >> 20);
    const unsigned grid = (unsigned)std::min<int64_t>((a.tiles + 1) / 2, want);
    {
        SkrProfScope prof(ctx, h_edges ? "hist_edges" : "hist_key_digits");
        const bool match = ctx->knobs.dist_match != 0;
        if (h_edges) {
            if (match)
                hipLaunchKernelGGL((dist_hist_pass<true, kDistMatchRounds>), dim3(grid), dim3(kCellBlock), 0, ctx->stream, a, d, g_edges, g_counts);
            else
                hipLaunchKernelGGL((dist_hist_pass<true, 0>), dim3(grid), dim3(kCellBlock), 0, ctx->stream, a, d, g_edges, g_counts);
        } else {
            if (match)
                hipLaunchKernelGGL((dist_hist_pass<false, kDistMatchRounds>), dim3(grid), dim3(kCellBlock), 0, ctx->stream, a, d, g_edges, g_counts);
            else
                hipLaunchKernelGGL((dist_hist_pass<false, 0>), dim3(grid), dim3(kCellBlock), 0, ctx->stream, a, d, g_edges, g_counts);
        }
        SKR_HIP(hipGetLastError());
    }
    SKR_HIP(hipMemcpyAsync(out->data(), g_counts, count_bytes, hipMemcpyDeviceToHost, ctx->stream));
    SKR_HIP(hipStreamSynchronize(ctx->stream));
    return SKR_OK;
}

}  // namespace

extern "C" int skr_hist_key_digits(skr_ctx* ctx, const skr_mat* r, int64_t nrows, int64_t col_begin, int64_t col_end,
                                   int64_t row_global0, int64_t col_global0, int upper_only, int shift, int bits,
                                   int prefix_bits, const uint32_t* prefixes, int n_prefixes, uint64_t* hist, uint64_t* nan) {
    SkrBlock b;  // counts only: no global index is written
    SKR_TRY(skr_block(ctx, r, nrows, col_begin, col_end, row_global0, col_global0, SKR_FIT_NONE, &b));
    SKR_REQUIRE(hist && nan, "hist and nan must not be NULL");
    SKR_REQUIRE(bits >= 1 && bits <= 12 && shift >= 0 && shift + bits <= 32, "need 1 <= bits <= 12 and shift + bits <= 32");
    SKR_REQUIRE(prefix_bits >= 0 && prefix_bits <= 32, "prefix_bits out of range");
    SKR_REQUIRE(n_prefixes >= 1 && n_prefixes <= kDistMaxPrefixes && prefixes, "1 to %d prefixes", kDistMaxPrefixes);
    SKR_REQUIRE(((int64_t)n_prefixes << bits) <= kDistKeyBins, "n_prefixes * 2^bits must not exceed %d", kDistKeyBins);
    SKR_REQUIRE(prefix_bits > 0 || n_prefixes == 1, "prefix_bits = 0 is one histogram of every cell");
    DistArgs d{};
    d.upper_only = upper_only != 0;
    d.shift = shift, d.bits = bits, d.prefix_bits = prefix_bits, d.n_prefixes = n_prefixes;
    for (int i = 0; i < n_prefixes; i++) {
        SKR_REQUIRE(prefix_bits == 32 || (uint64_t)prefixes[i] < (1ull << prefix_bits), "prefix %d does not fit prefix_bits", i);
        for (int j = 0; j < i; j++) SKR_REQUIRE(prefixes[i] != prefixes[j], "the prefixes must be distinct");
        d.prefixes[i] = prefixes[i];
    }
    d.total_bins = (n_prefixes << bits) + 1;
    std::vector<unsigned long long> got;
    SKR_TRY(dist_run(ctx, cell_tiles(b, 0.f), d, nullptr, &got));
    for (int i = 0; i < d.total_bins - 1; i++) hist[i] += got[(size_t)i];
    *nan += got[(size_t)d.total_bins - 1];
    return SKR_OK;
}

extern "C" int skr_hist_edges(skr_ctx* ctx, const skr_mat* r, int64_t nrows, int64_t col_begin, int64_t col_end,
                              int64_t row_global0, int64_t col_global0, int upper_only, const float* edges, int n_edges,
                              uint64_t* hist, uint64_t* below, uint64_t* above, uint64_t* nan) {
    SkrBlock b;  // counts only: no global index is written
    SKR_TRY(skr_block(ctx, r, nrows, col_begin, col_end, row_global0, col_global0, SKR_FIT_NONE, &b));
    SKR_REQUIRE(hist && below && above && nan, "hist, below, above and nan must not be NULL");
    SKR_REQUIRE(edges && n_edges >= 2 && n_edges <= kDistMaxEdges, "2 to %d edges", kDistMaxEdges);
    for (int i = 0; i < n_edges; i++) {
        SKR_REQUIRE(std::isfinite(edges[i]), "edge %d is not finite", i);
        SKR_REQUIRE(i == 0 || edges[i - 1] < edges[i], "the edges must be strictly ascending (edge %d)", i);
    }
    DistArgs d{};
    d.upper_only = upper_only != 0;
    d.n_edges = n_edges;
    d.total_bins = n_edges - 1 + 3;
    std::vector<unsigned long long> got;
    SKR_TRY(dist_run(ctx, cell_tiles(b, 0.f), d, edges, &got));
    const int nb = n_edges - 1;
    for (int i = 0; i < nb; i++) hist[i] += got[(size_t)i];
    *below += got[(size_t)nb], *above += got[(size_t)nb + 1], *nan += got[(size_t)nb + 2];
    return SKR_OK;
}
