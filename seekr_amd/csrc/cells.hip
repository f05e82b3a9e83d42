// skr_select_cells_ge: the cells of a query x target block of r with !(v < cutoff) as a (row, column, value) list that
// stays on the device, skr_vec_copy, which such a list grows by, and skr_gather_cells, the opposite direction: the
// values of the cells a list names.  skr_edges (consumers.hip) is the graph's rule — it
// drops v == 0 and the global diagonal and gives a workgroup to each row; here every cell is an ordinary test and the
// work is tiled in both directions.
//
// A tile is one row x one segment of kCellSegment columns.  Segments are laid out in the row's MEMORY, not in its
// columns: the first one starts at the 16-byte boundary at or below the row's first selected cell, so that every group
// of four cells a lane reads is 16-byte aligned whatever the row start, col_begin and the leading dimension are.  A group
// that lies inside [col_begin, col_end) is one 16-byte load; a group that straddles either end (the head of a row's first
// segment, the tail of its last) is read cell by cell, the cells outside the range not at all.  Rows whose first cell is
// not aligned have up to 3 cells fewer in their first segment, which is why a row has ceil((width + 3) / kCellSegment)
// tiles, the last of which may be empty.
//
// Pass 1 counts per tile, radix.hpp's exclusive scan turns the counts into offsets, pass 2 writes.  A cell's place in
// its tile comes from four wave ballots (one per cell of the lane's group) and the four wave totals: lanes in order,
// cells in order within the lane — row-major, no atomic per cell, and the same bytes on every run.
#include <algorithm>

#include "cell_tile.hpp"
#include "common.hpp"
#include "count_scan.hpp"
#include "device_flag.hpp"

namespace {

__global__ __launch_bounds__(kCellBlock) void cells_count_pass(CellArgs a, unsigned long long* __restrict__ counts,
                                                                 unsigned* __restrict__ nan_flag) {
    __shared__ unsigned red[2][kCellBlock / 64];  // two sets: one barrier per tile
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    bool nan = false;
    int set = 0;
    for (int64_t t = blockIdx.x; t < a.tiles; t += gridDim.x, set ^= 1) {
        float v[kCellPer];
        bool live[kCellPer];
        int64_t row, c0;
        load_group(a, t, v, live, row, c0);
        unsigned n = 0;
#pragma unroll
        for (int j = 0; j < kCellPer; j++) {
            const bool keep = live[j] && !(v[j] < a.cutoff);
            nan = nan || (keep && v[j] != v[j]);
            n += (unsigned)__popcll(__ballot(keep));
        }
        if (lane == 0) red[set][wave] = n;
        __syncthreads();
        if (threadIdx.x == 0) counts[t] = (unsigned long long)red[set][0] + red[set][1] + red[set][2] + red[set][3];
    }
    if (nan) atomicOr(nan_flag, 1u);
}

__global__ __launch_bounds__(kCellBlock) void cells_fill_pass(CellArgs a, const unsigned long long* __restrict__ offsets,
                                                                unsigned long long out_offset, uint32_t* __restrict__ out_row,
                                                                uint32_t* __restrict__ out_col, float* __restrict__ out_val) {
    __shared__ unsigned wave_n[2][kCellBlock / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long below = lane ? (~0ull >> (64 - lane)) : 0ull;
    int set = 0;
    for (int64_t t = blockIdx.x; t < a.tiles; t += gridDim.x) {
        const unsigned long long base = offsets[t];
        if (offsets[t + 1] == base) continue;  // nothing kept in this tile (the same for every lane of the workgroup)
        float v[kCellPer];
        bool live[kCellPer], keep[kCellPer];
        int64_t row, c0;
        load_group(a, t, v, live, row, c0);
        unsigned lower = 0, all = 0;  // kept cells of the lower lanes of this wave; of the whole wave
#pragma unroll
        for (int j = 0; j < kCellPer; j++) {
            keep[j] = live[j] && !(v[j] < a.cutoff);
            const unsigned long long mask = __ballot(keep[j]);
            lower += (unsigned)__popcll(mask & below);
            all += (unsigned)__popcll(mask);
        }
        if (lane == 0) wave_n[set][wave] = all;
        __syncthreads();
        unsigned before = 0;
#pragma unroll
        for (int w = 0; w < kCellBlock / 64; w++)
            if (w < wave) before += wave_n[set][w];
        unsigned long long pos = out_offset + base + before + lower;
#pragma unroll
        for (int j = 0; j < kCellPer; j++)
            if (keep[j]) {
                out_row[pos] = (uint32_t)(a.b.row_global0 + row);
                out_col[pos] = (uint32_t)(a.b.col_global0 + c0 + j);
                out_val[pos] = v[j];
                pos++;
            }
        set ^= 1;
    }
}

// skr_gather_cells: one thread per listed slot.  The subtraction of the block's origin is made in 64 bits, so a global
// index far from the block can never alias into it; a slot whose cell lies in the block receives the cell's 32 bits as
// an integer (no float operation touches a NaN payload, -0 or a denormal), every other slot is left alone.  The loop
// bound is the same for every lane of a wave, so the ballot that counts the served slots sees whole waves.
__global__ __launch_bounds__(256) void gather_cells_pass(SkrBlock b, const uint32_t* __restrict__ rows,
                                                           const uint32_t* __restrict__ cols, int64_t first, int64_t count,
                                                           uint32_t* __restrict__ out, unsigned long long* __restrict__ gathered) {
    const uint32_t* __restrict__ r = reinterpret_cast<const uint32_t*>(b.r);  // the cells' bits
    const int lane = threadIdx.x & 63;
    unsigned long long served = 0;
    for (int64_t base = (int64_t)blockIdx.x * 256; base < count; base += (int64_t)gridDim.x * 256) {
        const int64_t t = base + threadIdx.x;
        bool hit = false;
        if (t < count) {
            const int64_t s = first + t;
            const int64_t i = (int64_t)rows[s] - b.row_global0, j = (int64_t)cols[s] - b.col_global0;
            hit = i >= 0 && i < b.rows && j >= b.col_begin && j < b.col_end;
            if (hit) out[s] = r[i * b.ld + j];
        }
        served += (unsigned long long)__popcll(__ballot(hit));
    }
    if (gathered && lane == 0 && served) atomicAdd(gathered, served);
}

}  // namespace

extern "C" int skr_select_cells_ge(skr_ctx* ctx, const skr_mat* r, int64_t nrows, int64_t col_begin, int64_t col_end,
                                   int64_t row_global0, int64_t col_global0, float cutoff, skr_mat* out_rows,
                                   skr_mat* out_cols, skr_mat* out_vals, int64_t out_offset, int64_t* count, int* saw_nan) {
    SkrBlock b;
    SKR_TRY(skr_block(ctx, r, nrows, col_begin, col_end, row_global0, col_global0, SKR_FIT_BOTH, &b));
    SKR_REQUIRE(count, "count must not be NULL");
    skr_mat* const outs[3] = {out_rows, out_cols, out_vals};
    const int dtypes[3] = {SKR_U32, SKR_U32, SKR_F32};
    bool fill = false;
    int64_t cap = 0;
    SKR_TRY(skr_list_outputs(ctx, outs, dtypes, 3, "outputs are U32, U32, F32", &fill, &cap));
    SKR_REQUIRE(!fill || out_offset >= 0, "out_offset must not be negative");
    SKR_TRY(skr_activate(ctx));
    *count = 0;
    if (saw_nan) *saw_nan = 0;
    if (nrows == 0 || col_begin == col_end) return SKR_OK;
    const CellArgs a = cell_tiles(b, cutoff);
    SkrCountScan<unsigned long long> cs;  // one count per tile, and the NaN flag
    SKR_TRY(cs.begin(ctx, a.tiles, true));
    const unsigned grid = (unsigned)std::min<int64_t>(a.tiles, (int64_t)ctx->num_cu * 16);
    {
        SkrProfScope prof(ctx, "cells_count");
        hipLaunchKernelGGL(cells_count_pass, dim3(grid), dim3(kCellBlock), 0, ctx->stream, a, cs.counts, cs.flag);
        SKR_HIP(hipGetLastError());
    }
    SKR_TRY(cs.finish(ctx, count, saw_nan));
    if (!fill || *count == 0) return SKR_OK;
    if (!skr_list_fits(cap, out_offset, *count)) return SKR_OK;  // the caller grows its buffers
    SkrProfScope prof(ctx, "cells_fill");
    hipLaunchKernelGGL(cells_fill_pass, dim3(grid), dim3(kCellBlock), 0, ctx->stream, a, cs.counts, (unsigned long long)out_offset,
                       (uint32_t*)out_rows->data, (uint32_t*)out_cols->data, (float*)out_vals->data);
    SKR_HIP(hipGetLastError());
    return SKR_OK;
}

extern "C" int skr_gather_cells(skr_ctx* ctx, const skr_mat* r, int64_t nrows, int64_t col_begin, int64_t col_end,
                                int64_t row_global0, int64_t col_global0, const skr_mat* rows, const skr_mat* cols,
                                int64_t first, int64_t count, skr_mat* out, int64_t* gathered) {
    SkrBlock b;  // the listed cells are uint32 pairs: a block past 32 bits could hold none of them
    SKR_TRY(skr_block(ctx, r, nrows, col_begin, col_end, row_global0, col_global0, SKR_FIT_BOTH, &b));
    SKR_REQUIRE(rows && cols && out, "NULL argument");
    SKR_REQUIRE(rows->ctx == ctx && cols->ctx == ctx && out->ctx == ctx, "foreign ctx");
    SKR_REQUIRE(rows->dtype == SKR_U32 && cols->dtype == SKR_U32 && out->dtype == SKR_F32, "out is F32, rows and cols are U32");
    const int64_t slots = rows->rows * rows->cols;
    SKR_REQUIRE(cols->rows * cols->cols == slots && out->rows * out->cols == slots, "rows, cols and out must have one length");
    SKR_REQUIRE(first >= 0 && count >= 0 && first <= slots && count <= slots - first, "first + count exceeds the list");
    SKR_TRY(skr_activate(ctx));
    if (gathered) *gathered = 0;
    if (count == 0) return SKR_OK;
    SkrDeviceFlag<unsigned long long> served;  // a counter: the kernel adds to it
    SKR_TRY(served.arm(ctx, gathered != nullptr));
    // at most one workgroup per CU: a sweep's block rarely holds more than a few thousand of the listed cells
    const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((count + 255) / 256, (int64_t)ctx->num_cu));
    {
        SkrProfScope prof(ctx, "gather_cells");
        hipLaunchKernelGGL(gather_cells_pass, dim3(grid), dim3(256), 0, ctx->stream, b, (const uint32_t*)rows->data,
                           (const uint32_t*)cols->data, first, count, (uint32_t*)out->data, served.d);
        SKR_HIP(hipGetLastError());
    }
    unsigned long long h_n = 0;
    SKR_TRY(served.read(ctx, &h_n));
    if (gathered) *gathered = (int64_t)h_n;
    return SKR_OK;
}

extern "C" int skr_vec_copy(skr_ctx* ctx, const skr_mat* src, int64_t src_off, skr_mat* dst, int64_t dst_off, int64_t count) {
    SKR_REQUIRE(ctx && src && dst, "NULL argument");
    SKR_REQUIRE(src->ctx == ctx && dst->ctx == ctx, "foreign ctx");
    SKR_REQUIRE(src->dtype == dst->dtype, "src and dst must have the same dtype");
    SKR_REQUIRE(src->dtype == SKR_U32 || src->dtype == SKR_F32 || src->dtype == SKR_F64, "U32, F32 or F64 cells");
    SKR_REQUIRE(count >= 0 && src_off >= 0 && dst_off >= 0, "offsets and count must not be negative");
    SKR_REQUIRE(src_off <= src->rows * src->cols && count <= src->rows * src->cols - src_off, "range outside src");
    SKR_REQUIRE(dst_off <= dst->rows * dst->cols && count <= dst->rows * dst->cols - dst_off, "range outside dst");
    SKR_TRY(skr_activate(ctx));
    if (count == 0) return SKR_OK;
    const size_t elem = src->elem();
    const char* s = (const char*)src->data + (size_t)src_off * elem;
    char* d = (char*)dst->data + (size_t)dst_off * elem;
    const size_t bytes = (size_t)count * elem;
    SKR_REQUIRE(s + bytes <= d || d + bytes <= s, "the ranges overlap");
    SKR_HIP(hipMemcpyAsync(d, s, bytes, hipMemcpyDeviceToDevice, ctx->stream));
    return SKR_OK;
}
