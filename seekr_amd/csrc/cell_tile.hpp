// The tiling skr_select_cells_ge (cells.hip) and the histogram kernels (distribution.hip) read a block of r by: one row x
// one segment of kCellSegment columns per tile, four cells per lane, every full group one aligned 16-byte load.  The
// layout is described at the top of cells.hip.
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

#include "block.hpp"

namespace {

constexpr int kCellBlock = 256, kCellPer = 4, kCellSegment = kCellBlock * kCellPer;  // 1 024: _lib.SELECT_CELLS_SEGMENT

struct CellArgs {
    SkrBlock b;
    int64_t nseg, tiles;  // segments per row, tiles in all
    float cutoff;
};

// the tiles of a block: a row whose first cell is not 16-byte aligned has up to kCellPer - 1 cells fewer in its first
// segment, hence the + (kCellPer - 1); the last tile of a row may be empty
inline CellArgs cell_tiles(const SkrBlock& b, float cutoff) {
    const int64_t nseg = (b.col_end - b.col_begin + (kCellPer - 1) + kCellSegment - 1) / kCellSegment;
    return CellArgs{b, nseg, b.rows * nseg, cutoff};
}

// the lane's four cells of tile t: v[j] and live[j] (inside the column range); c0 = column of v[0]
__device__ __forceinline__ void load_group(const CellArgs& a, int64_t t, float (&v)[kCellPer], bool (&live)[kCellPer], int64_t& row,
                                           int64_t& c0) {
    row = t / a.nseg;
    const int64_t seg = t - row * a.nseg;
    const float* rowp = a.b.r + (size_t)row * (size_t)a.b.ld;
    const int64_t mis = (int64_t)(((uintptr_t)(rowp + a.b.col_begin) >> 2) & 3);  // cells from the 16-byte boundary below to the first selected cell
    c0 = a.b.col_begin - mis + seg * kCellSegment + (int64_t)threadIdx.x * kCellPer;
    if (c0 >= a.b.col_begin && c0 + kCellPer <= a.b.col_end) {
        const float4 q = *reinterpret_cast<const float4*>(rowp + c0);  // 16-byte aligned by construction
        v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
#pragma unroll
        for (int j = 0; j < kCellPer; j++) live[j] = true;
    } else {
#pragma unroll
        for (int j = 0; j < kCellPer; j++) {
            live[j] = c0 + j >= a.b.col_begin && c0 + j < a.b.col_end;
            v[j] = live[j] ? rowp[c0 + j] : 0.f;
        }
    }
}

}  // namespace
