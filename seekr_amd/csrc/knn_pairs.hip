// skr_knn_pairs: top-k lists -> the mutual or union nearest-neighbour pairs, as (row, col, value, rank_row, rank_col) in
// ascending (row, col) order.  Two sets: idx_a [n1, k] names rows of B, idx_b [n2, k] names rows of A; one set (idx_b
// NULL): idx_a serves both sides and every pair is written once with row < col.
//
// Every slot of the lists (idx_a's first, then idx_b's, each row-major) becomes one item: the key row << 32 | col of the
// pair it is a candidate for, and its own slot number — which says everything else: the side and the rank are where the
// slot is, the value is read back through it.  A slot that is no candidate — a padded index, a NaN value, a node's own
// index in the self form — gets the key n1 << 32, which sorts behind every pair.  The items are sorted by key with
// radix.hpp's stable least-significant-digit sort over the bits that can be set, with the policy fused_edges.hip sorts its
// edges by (edge_pass.hpp; the slot number travels in the value's place).  Lists as the merge kernels leave them hold no
// index twice, so a key occurs at most twice, once per side.  One pass over neighbouring keys then marks the first item of
// every pair that is kept (mutual: the key occurs twice; union: always; positive_only: the pair's value is > 0),
// radix.hpp's scan turns the marks into places, and a last pass writes.  The lists' indices are never used as addresses,
// so an index out of range can only be reported; a slot number is below the number of slots by construction.
#include <algorithm>

#include "common.hpp"
#include "count_scan.hpp"
#include "edge_pass.hpp"

namespace {

constexpr uint32_t kNoIndex = 0xFFFFFFFFu;

struct PairLists {
    const uint32_t* idx_a;
    const float* val_a;
    const uint32_t* idx_b;  // NULL: the self form
    const float* val_b;
    int64_t n1, ka, n2, kb;
    __device__ __forceinline__ int64_t slots_a() const { return n1 * ka; }
    __device__ __forceinline__ int64_t slots() const { return n1 * ka + (idx_b ? n2 * kb : 0); }
    __device__ __forceinline__ unsigned long long none() const { return (unsigned long long)n1 << 32; }
};

struct PairSlot {  // what slot s of the lists says
    uint32_t u, rank, v, bits;  // the list's row, the place in it, the index found there, the value's bits
    bool side_b;
};

__device__ __forceinline__ PairSlot pair_slot(const PairLists& a, int64_t s) {
    PairSlot p;
    p.side_b = s >= a.slots_a();
    const int64_t t = p.side_b ? s - a.slots_a() : s, kk = p.side_b ? a.kb : a.ka;
    p.u = (uint32_t)(t / kk), p.rank = (uint32_t)(t % kk);
    p.v = p.side_b ? a.idx_b[t] : a.idx_a[t];
    p.bits = __float_as_uint(p.side_b ? a.val_b[t] : a.val_a[t]);
    return p;
}

__global__ __launch_bounds__(256) void pairs_emit_kernel(PairLists a, unsigned long long* __restrict__ keys,
                                                        float* __restrict__ slot_of, unsigned* __restrict__ bad) {
    const bool self = a.idx_b == nullptr;
    const int64_t slots = a.slots();
    bool out_of_range = false;
    for (int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x; s < slots; s += (int64_t)gridDim.x * 256) {
        const PairSlot p = pair_slot(a, s);
        unsigned long long key = a.none();
        if (p.v != kNoIndex) {
            const float x = __uint_as_float(p.bits);
            if ((int64_t)p.v >= (p.side_b || self ? a.n1 : a.n2)) {
                out_of_range = true;
            } else if (x == x) {
                if (self) {
                    if (p.v > p.u) key = (unsigned long long)p.u << 32 | p.v;
                    if (p.v < p.u) key = (unsigned long long)p.v << 32 | p.u;
                } else {
                    key = p.side_b ? (unsigned long long)p.v << 32 | p.u : (unsigned long long)p.u << 32 | p.v;
                }
            }
        }
        keys[s] = key, slot_of[s] = __uint_as_float((uint32_t)s);
    }
    if (out_of_range) atomicOr(bad, 1u);
}

struct PairOut {  // what the pair starting at sorted item i is, if it is kept
    bool keep;
    uint32_t val, rank_row, rank_col;
};

__device__ __forceinline__ PairOut pair_at(const PairLists& a, const unsigned long long* __restrict__ keys,
                                           const float* __restrict__ slot_of, int64_t i, int mode, int positive_only) {
    PairOut out{false, 0u, kNoIndex, kNoIndex};
    const int64_t slots = a.slots();
    const unsigned long long key = keys[i];
    if (key == a.none() || (i > 0 && keys[i - 1] == key)) return out;  // no candidate, or not the first of its key
    const bool twice = i + 1 < slots && keys[i + 1] == key;
    if (mode == 0 && !twice) return out;
    const bool self = a.idx_b == nullptr;
    bool have_row = false;
    for (int j = 0; j < (twice ? 2 : 1); j++) {
        const PairSlot p = pair_slot(a, (int64_t)__float_as_uint(slot_of[i + j]));
        // the entry read from the row side (two sets: idx_a; one set: the row that is the pair's smaller node) carries
        // rank_row and, when there is one, the pair's value
        const bool col_side = self ? p.u != (uint32_t)(key >> 32) : p.side_b;
        if (col_side) {
            out.rank_col = p.rank;
            if (!have_row) out.val = p.bits;
        } else {
            out.rank_row = p.rank, out.val = p.bits, have_row = true;
        }
    }
    out.keep = !positive_only || __uint_as_float(out.val) > 0.f;
    return out;
}

__global__ __launch_bounds__(256) void pairs_mark_kernel(PairLists a, const unsigned long long* __restrict__ keys,
                                                        const float* __restrict__ slot_of, int mode, int positive_only,
                                                        uint32_t* __restrict__ marks) {
    const int64_t slots = a.slots();
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < slots; i += (int64_t)gridDim.x * 256)
        marks[i] = pair_at(a, keys, slot_of, i, mode, positive_only).keep ? 1u : 0u;
}

__global__ __launch_bounds__(256) void pairs_write_kernel(PairLists a, const unsigned long long* __restrict__ keys,
                                                         const float* __restrict__ slot_of, int mode, int positive_only,
                                                         const uint32_t* __restrict__ places, unsigned long long out_offset,
                                                         uint32_t* __restrict__ out_row, uint32_t* __restrict__ out_col,
                                                         uint32_t* __restrict__ out_val, uint32_t* __restrict__ out_rank_row,
                                                         uint32_t* __restrict__ out_rank_col) {
    const int64_t slots = a.slots();
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < slots; i += (int64_t)gridDim.x * 256) {
        if (places[i + 1] == places[i]) continue;
        const PairOut p = pair_at(a, keys, slot_of, i, mode, positive_only);
        const unsigned long long at = out_offset + places[i], key = keys[i];
        out_row[at] = (uint32_t)(key >> 32), out_col[at] = (uint32_t)key, out_val[at] = p.val;
        out_rank_row[at] = p.rank_row, out_rank_col[at] = p.rank_col;
    }
}

}  // namespace

extern "C" int skr_knn_pairs(skr_ctx* ctx, const skr_mat* idx_a, const skr_mat* val_a, const skr_mat* idx_b,
                             const skr_mat* val_b, int mode, int positive_only, skr_mat* out_rows, skr_mat* out_cols,
                             skr_mat* out_vals, skr_mat* out_rank_row, skr_mat* out_rank_col, int64_t out_offset,
                             int64_t* count) {
    SKR_REQUIRE(ctx && idx_a && val_a && count, "NULL argument");
    SKR_REQUIRE((idx_b == nullptr) == (val_b == nullptr), "pass idx_b and val_b, or neither (the self form)");
    SKR_REQUIRE(mode == 0 || mode == 1, "mode: 0 = mutual, 1 = union");
    SKR_REQUIRE(idx_a->ctx == ctx && val_a->ctx == ctx && (!idx_b || (idx_b->ctx == ctx && val_b->ctx == ctx)), "foreign ctx");
    SKR_REQUIRE(idx_a->dtype == SKR_U32 && val_a->dtype == SKR_F32 && idx_a->rows == val_a->rows && idx_a->cols == val_a->cols,
                "idx_a U32 and val_a F32 of one shape");
    if (idx_b)
        SKR_REQUIRE(idx_b->dtype == SKR_U32 && val_b->dtype == SKR_F32 && idx_b->rows == val_b->rows && idx_b->cols == val_b->cols,
                    "idx_b U32 and val_b F32 of one shape");
    skr_mat* const outs[5] = {out_rows, out_cols, out_vals, out_rank_row, out_rank_col};
    const int dtypes[5] = {SKR_U32, SKR_U32, SKR_F32, SKR_U32, SKR_U32};
    bool given = false;
    int64_t cap = 0;
    SKR_TRY(skr_list_outputs(ctx, outs, dtypes, 5, "outputs are U32, U32, F32, U32, U32", &given, &cap));
    SKR_REQUIRE(!given || out_offset >= 0, "out_offset must not be negative");
    const int64_t n1 = idx_a->rows, ka = idx_a->cols;
    const int64_t n2 = idx_b ? idx_b->rows : n1, kb = idx_b ? idx_b->cols : 0;
    SKR_REQUIRE(n1 < 0xffffffffLL && n2 < 0xffffffffLL, "rows and columns must stay below 0xFFFFFFFF");
    SKR_REQUIRE(ka <= 0x7fffffff && kb <= 0x7fffffff && n1 * ka + n2 * kb <= 0x7fffffff, "at most 2^31 - 1 list slots per call");
    const int64_t slots = n1 * ka + n2 * kb;
    SKR_TRY(skr_activate(ctx));
    *count = 0;
    if (slots == 0) return SKR_OK;
    const PairLists lists{(const uint32_t*)idx_a->data, (const float*)val_a->data, idx_b ? (const uint32_t*)idx_b->data : nullptr,
                          idx_b ? (const float*)val_b->data : nullptr, n1, ka, n2, kb};

    // workspace: flags | keys A B | slot numbers A B | marks (+ one, + the scan's scratch) | digit table + its scan's scratch
    const size_t n = (size_t)slots;
    const size_t off_keys = 256, off_slots = off_keys + 2 * n * 8;
    const size_t off_marks = (off_slots + 2 * n * 4 + 255) & ~(size_t)255;
    const size_t mark_words = n + 1 + skr_radix::scan_scratch_words(slots + 1) + 16;
    const size_t off_table = (off_marks + mark_words * 4 + 255) & ~(size_t)255;
    const skr_radix::Chunks plan = skr_radix::plan_chunks(ctx, slots);
    void* ws = nullptr;
    SKR_TRY(skr_ctx_workspace(ctx, off_table + (plan.table_words + plan.scan_words + 16) * 4 + 256, &ws));
    char* base = (char*)ws;
    unsigned* bad = (unsigned*)base;
    unsigned long long* kbuf[2] = {(unsigned long long*)(base + off_keys), (unsigned long long*)(base + off_keys) + n};
    float* sbuf[2] = {(float*)(base + off_slots), (float*)(base + off_slots) + n};
    uint32_t* marks = (uint32_t*)(base + off_marks);
    uint32_t* table = (uint32_t*)(base + off_table);
    const unsigned grid = skr_grid(ctx, slots);
    SKR_HIP(hipMemsetAsync(bad, 0, 8, ctx->stream));
    {
        SkrProfScope prof(ctx, "knn_pairs_emit");
        hipLaunchKernelGGL(pairs_emit_kernel, dim3(grid), dim3(256), 0, ctx->stream, lists, kbuf[0], sbuf[0], bad);
        SKR_HIP(hipGetLastError());
    }
    int cur = 0;
    {
        SkrProfScope prof(ctx, "knn_pairs_sort");
        // columns are below max(n1, n2), rows at most n1 (the key of a slot that is no candidate): only those bits are sorted
        const int col_passes = (std::max(1, skr_radix::bit_length((uint64_t)(std::max(n1, n2) - 1))) + 7) / 8;
        const int row_passes = (skr_radix::bit_length((uint64_t)n1) + 7) / 8;
        for (int p = 0; p < col_passes + row_passes; p++) {
            const int row_field = p >= col_passes;
            const EdgePass<false> ep{kbuf[cur], sbuf[cur], kbuf[cur ^ 1], sbuf[cur ^ 1], nullptr, nullptr, 0u,
                                     8 * (row_field ? p - col_passes : p), row_field};
            SKR_TRY(skr_radix::run_pass(ctx, ep, slots, plan, table, table + plan.table_words));
            cur ^= 1;
        }
    }
    {
        SkrProfScope prof(ctx, "knn_pairs_mark");
        hipLaunchKernelGGL(pairs_mark_kernel, dim3(grid), dim3(256), 0, ctx->stream, lists, (const unsigned long long*)kbuf[cur],
                           (const float*)sbuf[cur], mode, positive_only != 0, marks);
        SKR_HIP(hipGetLastError());
        SKR_HIP(hipMemsetAsync(marks + n, 0, 4, ctx->stream));
        SKR_TRY(skr_radix::exclusive_scan<uint32_t>(ctx, marks, slots + 1, marks + n + 1));
    }
    uint32_t h_total = 0;
    unsigned h_bad = 0;
    SKR_HIP(hipMemcpyAsync(&h_total, marks + n, 4, hipMemcpyDeviceToHost, ctx->stream));
    SKR_HIP(hipMemcpyAsync(&h_bad, bad, 4, hipMemcpyDeviceToHost, ctx->stream));
    SKR_HIP(hipStreamSynchronize(ctx->stream));
    SKR_REQUIRE(!h_bad, "a list names an index outside the other set (idx_a: < %lld, idx_b: < %lld)", (long long)n2, (long long)n1);
    *count = (int64_t)h_total;
    if (!given || h_total == 0) return SKR_OK;
    if (!skr_list_fits(cap, out_offset, (int64_t)h_total)) return SKR_OK;  // the caller grows its buffers
    SkrProfScope prof(ctx, "knn_pairs_write");
    hipLaunchKernelGGL(pairs_write_kernel, dim3(grid), dim3(256), 0, ctx->stream, lists, (const unsigned long long*)kbuf[cur],
                       (const float*)sbuf[cur], mode, positive_only != 0, (const uint32_t*)marks, (unsigned long long)out_offset,
                       (uint32_t*)out_rows->data, (uint32_t*)out_cols->data, (uint32_t*)out_vals->data,
                       (uint32_t*)out_rank_row->data, (uint32_t*)out_rank_col->data);
    SKR_HIP(hipGetLastError());
    return SKR_OK;
}
