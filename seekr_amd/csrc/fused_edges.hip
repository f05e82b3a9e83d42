// Threshold fused into the contraction (kmer_leiden.py:91-96): the edge list of a block of r
// without ever writing the block.  The EDGES mode of the split contraction (pearson_bf16.hip) appends the surviving
// cells — unordered — to a list in the ctx workspace; here the list is put into (row, column) order, which is
// np.nonzero's order, by the hand-written least-significant-digit radix sort of radix.hpp (no library sort), whose last
// pass writes the three output arrays directly.  Against the two-step path (skr_pearson_gemm_op into a stripe buffer,
// then skr_edges) this saves the write of the stripe and the two reads of skr_edges' count and fill passes; the values
// are the same bits (same kernel arithmetic).
#include <algorithm>

#include "block.hpp"
#include "common.hpp"
#include "edge_pass.hpp"
#include "radix.hpp"

// ---------------------------------------------------------------------------------------------------------------
// LSD radix sort of (key = row << 32 | column, value) pairs, 8 bits per pass, only over the bits that can be set:
// ceil(bits(N) / 8) passes over the column field, then ceil(bits(M) / 8) over the row field (rows taken relative to
// the block's first row).  The kernels, the chunk rule and the pass itself are radix.hpp's; here are the policy (what a
// key is, what travels with it, where the last pass writes: edge_pass.hpp's EdgePass, shared with knn_pairs.hip), the
// workspace and the pass loop.
// ---------------------------------------------------------------------------------------------------------------

extern "C" int skr_pearson_gemm_edges_needs_scratch(skr_ctx* ctx, const skr_operand* a, const skr_operand* b, int* needs) {
    SKR_REQUIRE(ctx && a && b && needs, "NULL argument");
    *needs = a->kind != 0 && a->kt > skr_gemm_chunk_tiles(ctx, a->coherent || b->coherent);
    return SKR_OK;
}

extern "C" int skr_pearson_gemm_edges(skr_ctx* ctx, const skr_operand* a, const skr_operand* b, skr_mat* scratch,
                                      int64_t row_global0, int64_t col_global0, float cutoff, int upper_only,
                                      skr_mat* out_rows, skr_mat* out_cols, skr_mat* out_vals, int64_t* count) {
    SKR_REQUIRE(ctx && a && b && out_rows && out_cols && out_vals && count, "NULL argument");
    SKR_REQUIRE(a->ctx == ctx && b->ctx == ctx && out_rows->ctx == ctx && out_cols->ctx == ctx && out_vals->ctx == ctx,
                "handle belongs to a different ctx");
    SKR_REQUIRE(a->cols == b->cols && a->kind == b->kind && a->precision == b->precision,
                "operands were prepared for different shapes or precisions");
    SKR_TRY(skr_x8_pair_check(a, b));
    if (a->kind == 0)
        return skr_set_error(SKR_ERR_UNSUPPORTED, "float32-layout operands take the two-step path (skr_pearson_gemm_op + skr_edges)");
    SKR_REQUIRE(out_rows->dtype == SKR_U32 && out_cols->dtype == SKR_U32 && out_vals->dtype == SKR_F32, "outputs are U32, U32, F32");
    const int64_t M = a->rows, N = b->rows, K = a->cols;
    SKR_REQUIRE(skr_fits_u32(row_global0, M) && skr_fits_u32(col_global0, N), "global indices must fit 32 bits");
    const bool coherent = a->coherent || b->coherent;
    const int64_t chunk = skr_gemm_chunk_tiles(ctx, coherent);  // the rule the contraction itself applies (knob included)
    const bool multi_chunk = a->kt > chunk;
    if (multi_chunk)
        SKR_REQUIRE(scratch && scratch->ctx == ctx && scratch->dtype == SKR_F32 && scratch->rows >= M && scratch->cols >= N,
                    "rows of more than %lld columns need a float32 scratch block of at least [%lld, %lld]", (long long)(chunk * 32),
                    (long long)M, (long long)N);
    SKR_TRY(skr_activate(ctx));
    *count = 0;
    if (M == 0 || N == 0) return SKR_OK;
    const int64_t cap = std::min(out_rows->rows * out_rows->cols, std::min(out_cols->rows * out_cols->cols,
                                                                           out_vals->rows * out_vals->cols));
    SKR_REQUIRE(cap <= 0x7fffffff, "at most 2^31 - 1 edges per call");
    const size_t capu = (size_t)cap;
    // workspace: count | keys A | keys B | vals A | vals B | digit table + scan scratch (sized for any list of up to cap)
    const size_t off_keys_a = 256, off_keys_b = off_keys_a + capu * 8, off_vals_a = off_keys_b + capu * 8;
    const size_t off_vals_b = off_vals_a + capu * 4;
    const size_t off_table = (off_vals_b + capu * 4 + 255) & ~(size_t)255;
    const size_t table_words = skr_radix::max_table_words(ctx, std::max<int64_t>(cap, 1));
    const size_t scan_words = skr_radix::scan_scratch_words((int64_t)table_words) + 16;
    void* ws = nullptr;
    SKR_TRY(skr_ctx_workspace(ctx, off_table + (table_words + scan_words) * 4 + 256, &ws));
    char* base = (char*)ws;
    SkrEdgeSink sink;
    sink.count = (unsigned long long*)base;
    sink.keys = (unsigned long long*)(base + off_keys_a);
    sink.vals = (float*)(base + off_vals_a);
    sink.cap = (unsigned long long)cap;
    sink.row_global0 = row_global0;
    sink.col_global0 = col_global0;
    sink.cutoff = cutoff;
    sink.upper = upper_only != 0;
    SKR_HIP(hipMemsetAsync(sink.count, 0, 8, ctx->stream));
    float* C = multi_chunk ? (float*)scratch->data : nullptr;
    const int64_t ldc = multi_chunk ? scratch->cols : 0;
    SKR_TRY(skr_launch_gemm_edges(ctx, a->precision, a->data, b->data, C, M, N, a->kt, ldc, (float)K * a->scale * b->scale, coherent, sink));
    unsigned long long found = 0;
    SKR_HIP(hipMemcpyAsync(&found, sink.count, 8, hipMemcpyDeviceToHost, ctx->stream));
    SKR_HIP(hipStreamSynchronize(ctx->stream));
    *count = (int64_t)found;
    if (found == 0 || (int64_t)found > cap) return SKR_OK;  // too many for the outputs: the caller retries with larger ones

    SkrProfScope prof(ctx, "edges_sort");
    const skr_radix::Chunks plan = skr_radix::plan_chunks(ctx, (int64_t)found);
    SKR_REQUIRE(plan.table_words <= table_words, "internal: digit table larger than planned");
    // columns are below col_global0 + N, rows (relative to the block) below M: sort only the bits that can be set
    const int col_bits = std::max(1, skr_radix::bit_length((uint64_t)(col_global0 + N - 1)));
    const int row_bits = skr_radix::bit_length((uint64_t)(M - 1));
    const int col_passes = (col_bits + 7) / 8, row_passes = (row_bits + 7) / 8;
    uint32_t* table = (uint32_t*)(base + off_table);
    uint32_t* scan_scratch = table + table_words;
    unsigned long long* kbuf[2] = {(unsigned long long*)(base + off_keys_a), (unsigned long long*)(base + off_keys_b)};
    float* vbuf[2] = {(float*)(base + off_vals_a), (float*)(base + off_vals_b)};
    int cur = 0;
    for (int p = 0; p < col_passes + row_passes; p++) {
        const bool last = p + 1 == col_passes + row_passes;
        const int row_field = p >= col_passes;
        const int shift = 8 * (row_field ? p - col_passes : p);
        if (last) {
            const EdgePass<true> ep{kbuf[cur], vbuf[cur], nullptr, (float*)out_vals->data, (uint32_t*)out_rows->data,
                                    (uint32_t*)out_cols->data, (uint32_t)row_global0, shift, row_field};
            SKR_TRY(skr_radix::run_pass(ctx, ep, (int64_t)found, plan, table, scan_scratch));
        } else {
            const EdgePass<false> ep{kbuf[cur], vbuf[cur], kbuf[cur ^ 1], vbuf[cur ^ 1], nullptr, nullptr,
                                     (uint32_t)row_global0, shift, row_field};
            SKR_TRY(skr_radix::run_pass(ctx, ep, (int64_t)found, plan, table, scan_scratch));
        }
        cur ^= 1;
    }
    return SKR_OK;
}
