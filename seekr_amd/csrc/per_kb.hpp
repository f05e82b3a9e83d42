// The per-kb value of a bin, shared by every counting kernel (count.hip, windows.hip).  Translation units that include
// this are compiled with -ffp-contract=off (seekr_amd/build.py): the arithmetic below must not be fused.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

constexpr int kTabSize = 16;  // counts below this are looked up per sequence instead of recomputed

// float32( n sequential float64 additions of `inc` ) — what kmer_counts.py:144-150 stores.
// n*inc (one rounding) equals the sequential sum unless the product sits within the
// accumulated rounding slack of a float32 rounding boundary; only then replay the additions.
__device__ __forceinline__ float per_kb_value(uint32_t n, double inc) {
    if (n == 0) return 0.0f;
    const double p = (double)n * inc;
    const float f = (float)p;
    if (n <= 3) return f;  // 1*inc, inc+inc and fl(2inc+inc) are single roundings of n*inc
    const double slack = p * ((double)(n + 4) * 0x1.0p-53);
    if ((float)(p - slack) == f && (float)(p + slack) == f) return f;
    double s = 0.0;
    for (uint32_t i = 0; i < n; i++) s += inc;
    return (float)s;
}

__device__ __forceinline__ double per_kb_value_f64(uint32_t n, double inc) {
    double s = 0.0;
    for (uint32_t i = 0; i < n; i++) s += inc;  // exact replay; f64 output is a small-input path
    return s;
}

// ds_add_u32 (no return) at a byte address of the LDS
__device__ __forceinline__ void lds_add_u32(uint32_t* lds_base, uint32_t byte_addr, uint32_t v) {
    (void)__hip_atomic_fetch_add(reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(lds_base) + byte_addr), v, __ATOMIC_RELAXED,
                                 __HIP_MEMORY_SCOPE_WORKGROUP);  // result unused: ds_add_u32
}
