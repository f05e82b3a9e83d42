// A zeroed word of the ctx workspace that a kernel may raise (or add to), read back after the launch.  When the caller
// has no place to put the answer, arm(ctx, false) leaves `d` NULL and read() returns at once: no workspace request, no
// memset, no copy and no synchronise — a call without a flag never waits for the device.
// The word is the FIRST of the workspace, where SkrCountScan (count_scan.hpp) keeps its counts: a call uses one or the
// other, and a list consumer that needs a flag takes SkrCountScan's own (begin(ctx, n, true)).
#pragma once
#include "common.hpp"

template <typename W>
struct SkrDeviceFlag {
    W* d = nullptr;  // what the kernel receives: NULL when nobody asked

    int arm(skr_ctx* ctx, bool wanted = true) {
        if (!wanted) return SKR_OK;
        void* ws = nullptr;
        SKR_TRY(skr_ctx_workspace(ctx, 64, &ws));
        d = (W*)ws;
        SKR_HIP(hipMemsetAsync(d, 0, sizeof(W), ctx->stream));
        return SKR_OK;
    }

    // after the launch: the word into *out, which is valid when this returns
    int read(skr_ctx* ctx, W* out) {
        if (!d) return SKR_OK;
        SKR_HIP(hipMemcpyAsync(out, d, sizeof(W), hipMemcpyDeviceToHost, ctx->stream));
        SKR_HIP(hipStreamSynchronize(ctx->stream));
        return SKR_OK;
    }
};
