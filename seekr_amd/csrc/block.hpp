// A block of r, as every block consumer receives it: a float32 device matrix, how many of its rows and which of its
// columns are read, and the global position of its cell (0, 0).  skr_block is the only code that builds one, so the
// checks of the head exist once; what differs between the consumers is which global indices their kernels write as
// uint32, and they say so in `fit`.
#pragma once
#include "common.hpp"

struct SkrBlock {  // plain: passed to kernels by value
    const float* r;
    int64_t ld, rows, col_begin, col_end, row_global0, col_global0;
};

enum { SKR_FIT_NONE = 0, SKR_FIT_ROWS = 1, SKR_FIT_COLS = 2, SKR_FIT_BOTH = 3 };

// origin + extent <= 0xFFFFFFFF, compared without forming the sum: an origin near INT64_MAX is refused, not wrapped
inline bool skr_fits_u32(int64_t origin, int64_t extent) { return origin >= 0 && extent >= 0 && origin <= 0xffffffffLL - extent; }

inline int skr_block(const skr_ctx* ctx, const skr_mat* r, int64_t nrows, int64_t col_begin, int64_t col_end, int64_t row_global0,
                     int64_t col_global0, int fit, SkrBlock* b) {
    SKR_REQUIRE(ctx && r && r->ctx == ctx && r->dtype == SKR_F32, "need a float32 matrix of this ctx");
    SKR_REQUIRE(nrows >= 0 && nrows <= r->rows, "nrows out of range");
    SKR_REQUIRE(col_begin >= 0 && col_begin <= col_end && col_end <= r->cols, "column range out of the matrix");
    SKR_REQUIRE(row_global0 >= 0 && col_global0 >= 0, "global indices must not be negative");
    SKR_REQUIRE((!(fit & SKR_FIT_ROWS) || skr_fits_u32(row_global0, nrows)) &&
                    (!(fit & SKR_FIT_COLS) || skr_fits_u32(col_global0, col_end)), "global indices must fit 32 bits");
    *b = SkrBlock{(const float*)r->data, r->cols, nrows, col_begin, col_end, row_global0, col_global0};
    return SKR_OK;
}
