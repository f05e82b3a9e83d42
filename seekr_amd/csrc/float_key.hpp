// The monotone map of float32 bits to uint32 and back: key(a) < key(b) exactly when a orders below b, with -0 just below
// +0 and the NaNs at the two ends (sign bit set: below every number; clear: above).  Callers that want another rule for
// -0 or NaN put it around the map (topk_key.hpp).  Device and host.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

__host__ __device__ __forceinline__ uint32_t skr_float_key(float v) {
    const uint32_t u = __builtin_bit_cast(uint32_t, v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__host__ __device__ __forceinline__ float skr_float_unkey(uint32_t k) {
    return __builtin_bit_cast(float, (k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}
