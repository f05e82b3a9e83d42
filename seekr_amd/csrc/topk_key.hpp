// The total order of the per-row top-k selections (consumers.hip: topk_rows_kernel, topk.hip: topk_merge_kernel).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "float_key.hpp"

// Keys order (value desc, column asc): a larger key is a better cell.  A key is never 0 for a column below 0xFFFFFFFF,
// so 0 stands for "no entry".
__device__ __forceinline__ unsigned long long topk_key(float v, uint32_t col) {
    // monotone map of the float to uint32 (larger float -> larger key), NaN to the smallest key;
    // the low word prefers the smaller column on equal values
    uint32_t b = skr_float_key(v == 0.f ? 0.f : v);  // -0 and +0 compare equal
    if (v != v) b = 0u;
    return ((unsigned long long)b << 32) | (0xFFFFFFFFu - col);
}
