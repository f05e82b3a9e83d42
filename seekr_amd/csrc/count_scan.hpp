// The host side of every two-pass list: a count pass writes one count per tile, radix.hpp's exclusive scan turns the
// counts into offsets, the total comes to the host, and the caller's fill pass writes the list.  Here are the parts the
// lists share — the workspace, the scan with its one download and synchronise, and the check of the output vectors; the
// kernels, their grids and what happens when a list does not fit stay with the entry point.
//
//     SkrCountScan<unsigned long long> cs;
//     SKR_TRY(cs.begin(ctx, tiles, with_flag));         // counts | zero | scan scratch [| flag], zero and flag zeroed
//     <count pass>(..., cs.counts [, cs.flag]);
//     SKR_TRY(cs.finish(ctx, &total [, &flag]));        // scan, download, ONE synchronise: counts[t] is now tile t's offset
//     if (total fits) <fill pass>(..., cs.counts, ...);
//
// The counts start at the first byte of the ctx workspace, as an SkrDeviceFlag (device_flag.hpp) does: a call that
// counts and needs a flag asks for this driver's own (begin(ctx, n, true)), never for both.
#pragma once
#include <algorithm>
#include <cstdint>

#include "radix.hpp"

namespace {

template <typename U>  // the word of a count: radix.hpp scans uint32 and uint64
struct SkrCountScan {
    U* counts = nullptr;       // [n] counts, counts[n] = 0; after finish() the offsets, counts[n] the total
    unsigned* flag = nullptr;  // a zeroed word the count pass may raise (begin(..., true)), else NULL
    int64_t n = 0;

    int begin(skr_ctx* ctx, int64_t n_counts, bool with_flag = false) {
        n = n_counts;
        const size_t scan_words = skr_radix::scan_scratch_words(n + 1);
        void* ws = nullptr;
        SKR_TRY(skr_ctx_workspace(ctx, ((size_t)n + 1 + scan_words) * sizeof(U) + (with_flag ? 8 : 0), &ws));
        counts = (U*)ws;
        SKR_HIP(hipMemsetAsync(counts + n, 0, sizeof(U), ctx->stream));
        if (with_flag) {
            flag = (unsigned*)(counts + n + 1 + scan_words);
            SKR_HIP(hipMemsetAsync(flag, 0, 8, ctx->stream));
        }
        return SKR_OK;
    }

    int finish(skr_ctx* ctx, int64_t* total, int* raised = nullptr) {
        SKR_TRY(skr_radix::exclusive_scan<U>(ctx, counts, n + 1, counts + n + 1));
        U h_total = 0;
        unsigned h_flag = 0;
        SKR_HIP(hipMemcpyAsync(&h_total, counts + n, sizeof(U), hipMemcpyDeviceToHost, ctx->stream));
        if (flag) SKR_HIP(hipMemcpyAsync(&h_flag, flag, 4, hipMemcpyDeviceToHost, ctx->stream));
        SKR_HIP(hipStreamSynchronize(ctx->stream));
        *total = (int64_t)h_total;
        if (raised) *raised = h_flag ? 1 : 0;
        return SKR_OK;
    }
};

// The vectors a list is written to: all n of them or none (*fill), of this ctx, outs[i] of dtypes[i]; *cap = the
// shortest one's cells (0 when there are none).
inline int skr_list_outputs(const skr_ctx* ctx, skr_mat* const* outs, const int* dtypes, int n, const char* dtype_text, bool* fill,
                            int64_t* cap) {
    int given = 0;
    for (int i = 0; i < n; i++) given += outs[i] != nullptr;
    SKR_REQUIRE(given == 0 || given == n, "pass all %d outputs or none", n);
    *fill = given != 0;
    *cap = *fill ? INT64_MAX : 0;
    for (int i = 0; i < given; i++) {
        SKR_REQUIRE(outs[i]->ctx == ctx, "foreign ctx");
        SKR_REQUIRE(outs[i]->dtype == dtypes[i], "%s", dtype_text);
        *cap = std::min(*cap, outs[i]->rows * outs[i]->cols);
    }
    return SKR_OK;
}

// total more cells behind out_offset in vectors of cap cells
inline bool skr_list_fits(int64_t cap, int64_t out_offset, int64_t total) { return out_offset <= cap && total <= cap - out_offset; }

}  // namespace
