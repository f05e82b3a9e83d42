// skr_run_pieces_ge: the runs of hot cells (v >= cutoff, NaN never) inside the tiles of a query x window block of r, as a
// list of pieces (row, first, last, n_hot, peak, peak column) that stays on the device.  A piece is a maximal set of hot
// cells of ONE tile and one target sequence in which neighbouring hot cells are at most max_gap cold cells apart; nothing
// is carried from tile to tile, from chunk to chunk or from launch to launch — windows.merge_pieces joins the pieces
// across those edges on the host with the same rule.
//
// Tiling: cell_tile.hpp's, as skr_select_cells_ge — one row x one segment of 1 024 columns, four cells per lane, aligned
// 16-byte loads.  Position p = 4 * threadIdx.x + j of the tile is column seg0 + p.
//
// Inside a tile every lane needs, for each of its hot cells, the previous hot position of the tile and the last boundary
// position at or before the cell (a boundary: the tile's first live column, or a column whose sequence differs from the
// column before it; the four ids of a lane are one 16-byte load where the group is whole and aligned in the vector, the id
// before them comes from the lower lane).  Both are prefix maxima over positions: one packed inclusive max-scan over the wave (six shuffles
// carry both halves) and the totals of the lower waves through LDS.  A hot cell STARTS a piece iff there is no hot cell
// before it in the tile, or that cell lies before the last boundary, or more than max_gap positions lie between them.
//
// Pass 1 counts the starts per tile, radix.hpp's exclusive scan turns the counts into offsets, pass 2 writes.  A start's
// slot in its tile is the number of starts before it (four ballots and the wave totals, as in cells_fill_pass: lanes in
// order, cells in order within the lane), and every hot cell knows the slot of its own piece the same way.  The piece's
// n_hot is an LDS atomicAdd, its last position an LDS atomicMax, its peak ONE 64-bit LDS atomicMax of
// (key(v) << 32) | (0xFFFFFFFF - position): the largest value by the order of float_key.hpp's key (-0 below +0) and the
// earliest position that reaches it, whatever order the lanes arrive in.  Integers and maxima only: the same input gives
// the same bytes on every run.  No global atomic per cell.
#include <algorithm>

#include "cell_tile.hpp"
#include "common.hpp"
#include "count_scan.hpp"
#include "float_key.hpp"

namespace {

constexpr int kRunWaves = kCellBlock / 64;

struct RunArgs {
    const uint32_t* seq;  // sequence of every GLOBAL column, or nullptr: one sequence
    int max_gap;          // clamped to kCellSegment: no gap inside a tile is longer
};

// The lane's four cells of tile t: hot[j], and start[j] (the cell begins a piece).  One __syncthreads inside: every lane
// of the workgroup calls it.  scan_tot: kRunWaves words of LDS.  nan: set when a live cell is NaN.
__device__ __forceinline__ void find_starts(const CellArgs& a, const RunArgs& ra, int64_t t, unsigned* scan_tot,
                                            float (&v)[kCellPer], bool (&hot)[kCellPer], bool (&start)[kCellPer], int64_t& row,
                                            int64_t& c0, bool& nan) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned p0 = threadIdx.x * kCellPer;
    bool live[kCellPer], bnd[kCellPer];
    load_group(a, t, v, live, row, c0);
    const int64_t seg0 = c0 - (int64_t)p0, first_live = seg0 > a.b.col_begin ? seg0 : a.b.col_begin;  // (only the row's first segment starts below col_begin)
    if (ra.seq) {
        const uint32_t* sp = ra.seq + a.b.col_global0;  // by r's own column: the live ones lie in [col_begin, col_end)
        uint32_t s[kCellPer];
        if (live[0] && live[kCellPer - 1] && (((uintptr_t)(sp + c0)) & 15) == 0) {  // a whole group, aligned in the vector too
            const uint4 q = *reinterpret_cast<const uint4*>(sp + c0);
            s[0] = q.x, s[1] = q.y, s[2] = q.z, s[3] = q.w;
        } else {
#pragma unroll
            for (int j = 0; j < kCellPer; j++) s[j] = live[j] ? sp[c0 + j] : 0u;
        }
        // the column before the lane's first one is the lower lane's last; a wave's first lane reads it.  It is only looked
        // at when it is a live column of this tile (c0 > first_live).
        uint32_t prior = __shfl_up(s[kCellPer - 1], 1, 64);
        if (lane == 0 && live[0] && c0 > first_live) prior = sp[c0 - 1];
        bnd[0] = live[0] && (c0 == first_live || s[0] != prior);
#pragma unroll
        for (int j = 1; j < kCellPer; j++) bnd[j] = live[j] && (c0 + j == first_live || s[j] != s[j - 1]);
    } else {
#pragma unroll
        for (int j = 0; j < kCellPer; j++) bnd[j] = live[j] && c0 + j == first_live;
    }
    unsigned h = 0, b = 0;  // position + 1 of the last hot cell / the last boundary of the lanes up to this one; 0: none
#pragma unroll
    for (int j = 0; j < kCellPer; j++) {
        hot[j] = live[j] && v[j] >= a.cutoff;
        nan = nan || (live[j] && v[j] != v[j]);
        if (hot[j]) h = p0 + j + 1;
        if (bnd[j]) b = p0 + j + 1;
    }
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned up = __shfl_up((h << 16) | b, off, 64);
        if (lane >= off) h = max(h, up >> 16), b = max(b, up & 0xffffu);
    }
    if (lane == 63) scan_tot[wave] = (h << 16) | b;
    unsigned ex = __shfl_up((h << 16) | b, 1, 64);
    if (lane == 0) ex = 0;
    __syncthreads();
    unsigned ph = ex >> 16, pb = ex & 0xffffu;  // of the lanes BELOW this one
#pragma unroll
    for (int w = 0; w < kRunWaves; w++)
        if (w < wave) {
            const unsigned tot = scan_tot[w];
            ph = max(ph, tot >> 16), pb = max(pb, tot & 0xffffu);
        }
#pragma unroll
    for (int j = 0; j < kCellPer; j++) {
        const unsigned pos1 = p0 + j + 1;
        if (bnd[j]) pb = pos1;
        start[j] = hot[j] && (ph == 0 || ph < pb || (int)(pos1 - ph - 1) > ra.max_gap);
        if (hot[j]) ph = pos1;
    }
}

__global__ __launch_bounds__(kCellBlock) void runs_count_pass(CellArgs a, RunArgs ra, unsigned long long* __restrict__ counts,
                                                                unsigned* __restrict__ nan_flag) {
    __shared__ unsigned scan_tot[kRunWaves], red[kRunWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    bool nan = false;
    for (int64_t t = blockIdx.x; t < a.tiles; t += gridDim.x) {
        float v[kCellPer];
        bool hot[kCellPer], start[kCellPer];
        int64_t row, c0;
        find_starts(a, ra, t, scan_tot, v, hot, start, row, c0, nan);
        unsigned n = 0;
#pragma unroll
        for (int j = 0; j < kCellPer; j++) n += (unsigned)__popcll(__ballot(start[j]));
        if (lane == 0) red[wave] = n;
        __syncthreads();
        if (threadIdx.x == 0) counts[t] = (unsigned long long)red[0] + red[1] + red[2] + red[3];
    }
    if (nan) atomicOr(nan_flag, 1u);
}

struct RunOut {
    uint32_t *row, *first, *last, *n_hot, *peak_col;
    float* peak;
};

__global__ __launch_bounds__(kCellBlock) void runs_fill_pass(CellArgs a, RunArgs ra, const unsigned long long* __restrict__ offsets,
                                                               unsigned long long out_offset, RunOut out) {
    __shared__ unsigned scan_tot[kRunWaves], wave_n[kRunWaves];
    __shared__ unsigned p_nhot[kCellSegment], p_last[kCellSegment];  // a tile has at most one piece per column
    __shared__ unsigned long long p_peak[kCellSegment];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned p0 = threadIdx.x * kCellPer;
    const unsigned long long below = lane ? (~0ull >> (64 - lane)) : 0ull;
    bool nan = false;
    for (int64_t t = blockIdx.x; t < a.tiles; t += gridDim.x) {
        const unsigned long long base = offsets[t];
        if (offsets[t + 1] == base) continue;  // no piece in this tile (the same for every lane of the workgroup)
        float v[kCellPer];
        bool hot[kCellPer], start[kCellPer];
        int64_t row, c0;
        find_starts(a, ra, t, scan_tot, v, hot, start, row, c0, nan);
        unsigned lower = 0, all = 0;  // starts of the lower lanes of this wave; of the whole wave
#pragma unroll
        for (int j = 0; j < kCellPer; j++) {
            const unsigned long long mask = __ballot(start[j]);
            lower += (unsigned)__popcll(mask & below);
            all += (unsigned)__popcll(mask);
        }
        if (lane == 0) wave_n[wave] = all;
        __syncthreads();
        unsigned seen = lower;  // starts at or before the cell: its piece is seen - 1
#pragma unroll
        for (int w = 0; w < kRunWaves; w++)
            if (w < wave) seen += wave_n[w];
        unsigned id[kCellPer];
#pragma unroll
        for (int j = 0; j < kCellPer; j++) {
            if (start[j]) {
                p_nhot[seen] = 0u, p_last[seen] = 0u, p_peak[seen] = 0ull;
                seen++;
            }
            id[j] = seen - 1;  // (a hot cell always has a start at or before it)
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < kCellPer; j++)
            if (hot[j]) {
                const unsigned pos = p0 + j;
                atomicAdd(&p_nhot[id[j]], 1u);
                atomicMax(&p_last[id[j]], pos);
                atomicMax(&p_peak[id[j]], ((unsigned long long)skr_float_key(v[j]) << 32) | (0xFFFFFFFFu - pos));
            }
        __syncthreads();
        const int64_t g0 = a.b.col_global0 + c0 - (int64_t)p0;  // global column of position 0
#pragma unroll
        for (int j = 0; j < kCellPer; j++)
            if (start[j]) {
                const unsigned long long at = out_offset + base + id[j];
                const unsigned long long pk = p_peak[id[j]];
                out.row[at] = (uint32_t)(a.b.row_global0 + row);
                out.first[at] = (uint32_t)(g0 + p0 + j);
                out.last[at] = (uint32_t)(g0 + p_last[id[j]]);
                out.n_hot[at] = p_nhot[id[j]];
                out.peak[at] = skr_float_unkey((uint32_t)(pk >> 32));
                out.peak_col[at] = (uint32_t)(g0 + (0xFFFFFFFFu - (uint32_t)pk));
            }
        // (the next tile writes these LDS cells only after two more barriers)
    }
}

}  // namespace

extern "C" int skr_run_pieces_ge(skr_ctx* ctx, const skr_mat* r, int64_t nrows, int64_t col_begin, int64_t col_end,
                                 int64_t row_global0, int64_t col_global0, float cutoff, const skr_mat* seq_of_col,
                                 int64_t max_gap, skr_mat* out_rows, skr_mat* out_first, skr_mat* out_last, skr_mat* out_nhot,
                                 skr_mat* out_peak, skr_mat* out_peak_col, int64_t out_offset, int64_t* count, int* saw_nan) {
    SkrBlock b;
    SKR_TRY(skr_block(ctx, r, nrows, col_begin, col_end, row_global0, col_global0, SKR_FIT_BOTH, &b));
    SKR_REQUIRE(count, "count must not be NULL");
    SKR_REQUIRE(max_gap >= 0, "max_gap must not be negative");
    if (seq_of_col) {
        SKR_REQUIRE(seq_of_col->ctx == ctx && seq_of_col->dtype == SKR_U32, "seq_of_col is a U32 vector of this ctx");
        SKR_REQUIRE(seq_of_col->rows * seq_of_col->cols >= col_global0 + col_end, "seq_of_col must reach col_global0 + col_end");
    }
    skr_mat* const outs[6] = {out_rows, out_first, out_last, out_nhot, out_peak, out_peak_col};
    const int dtypes[6] = {SKR_U32, SKR_U32, SKR_U32, SKR_U32, SKR_F32, SKR_U32};
    bool fill = false;
    int64_t cap = 0;
    SKR_TRY(skr_list_outputs(ctx, outs, dtypes, 6, "outputs are U32 except the peak, which is F32", &fill, &cap));
    SKR_REQUIRE(!fill || out_offset >= 0, "out_offset must not be negative");
    SKR_TRY(skr_activate(ctx));
    *count = 0;
    if (saw_nan) *saw_nan = 0;
    if (nrows == 0 || col_begin == col_end) return SKR_OK;
    const CellArgs a = cell_tiles(b, cutoff);
    RunArgs ra{seq_of_col ? (const uint32_t*)seq_of_col->data : nullptr, (int)std::min<int64_t>(max_gap, kCellSegment)};
    SkrCountScan<unsigned long long> cs;  // one count per tile, and the NaN flag
    SKR_TRY(cs.begin(ctx, a.tiles, true));
    const unsigned grid = (unsigned)std::min<int64_t>(a.tiles, (int64_t)ctx->num_cu * 16);
    {
        SkrProfScope prof(ctx, "runs_count");
        hipLaunchKernelGGL(runs_count_pass, dim3(grid), dim3(kCellBlock), 0, ctx->stream, a, ra, cs.counts, cs.flag);
        SKR_HIP(hipGetLastError());
    }
    SKR_TRY(cs.finish(ctx, count, saw_nan));
    if (!fill || *count == 0) return SKR_OK;
    if (!skr_list_fits(cap, out_offset, *count)) return SKR_OK;  // the caller grows its buffers
    SkrProfScope prof(ctx, "runs_fill");
    RunOut out{(uint32_t*)out_rows->data, (uint32_t*)out_first->data, (uint32_t*)out_last->data, (uint32_t*)out_nhot->data,
               (uint32_t*)out_peak_col->data, (float*)out_peak->data};
    hipLaunchKernelGGL(runs_fill_pass, dim3(grid), dim3(kCellBlock), 0, ctx->stream, a, ra, cs.counts, (unsigned long long)out_offset, out);
    SKR_HIP(hipGetLastError());
    return SKR_OK;
}
