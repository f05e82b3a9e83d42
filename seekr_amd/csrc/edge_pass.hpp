// The policy (radix.hpp) of the sorts whose items are a 64-bit key row << 32 | column and ONE 32-bit word that travels with
// it: fused_edges.hip (the word is the edge's value) and knn_pairs.hip (the word is the bits of a slot number).
#pragma once

#include "common.hpp"
#include "radix.hpp"

// internal linkage, as radix.hpp's kernels: every source that includes this instantiates them for itself
namespace {

using skr_radix::kDigits;

// the sort's policy (radix.hpp): the value travels with the key, and the LAST pass splits the key into the caller's
// row and column arrays
template <bool LAST>
struct EdgePass {
    using Count = uint32_t;  // the list is below 2^31
    struct Item {
        unsigned long long key;
        float val;
    };
    const unsigned long long* keys_in;
    const float* vals_in;
    unsigned long long* keys_out;  // middle passes
    float* vals_out;               // every pass (the last one: the caller's value array)
    uint32_t* rows_out;            // last pass only
    uint32_t* cols_out;
    uint32_t row0;  // subtracted from the row field before a row digit is taken
    int shift;      // within the field
    int row_field;  // 0: digit from the column field, 1: from the row field
    __device__ __forceinline__ Item load(int64_t i) const { return Item{keys_in[i], vals_in[i]}; }
    __device__ __forceinline__ uint32_t digit(const Item& it) const {
        const uint32_t f = row_field ? (uint32_t)(it.key >> 32) - row0 : (uint32_t)it.key;
        return (f >> shift) & (kDigits - 1);
    }
    __device__ __forceinline__ void store(uint32_t pos, const Item& it) const {
        if (LAST) {
            rows_out[pos] = (uint32_t)(it.key >> 32);
            cols_out[pos] = (uint32_t)it.key;
        } else {
            keys_out[pos] = it.key;
        }
        vals_out[pos] = it.val;
    }
};

}  // namespace
