// Per-COLUMN top-k in one pass over a block, with a running result: topk.hip turned by 90 degrees.  Column j's new list
// is the k best entries of the union of the list it had on entry and the cells r[0:nrows, j], in topk_key's order with the
// GLOBAL ROW in the low word (value descending, -0 == +0, NaN after every number, ties to the smaller global row).  The
// order is total, so a column merged stripe by stripe gives the same list whatever the split — which is what lets one
// sweep of r = a b^T / K keep the k best rows of a for every row of b beside the k best rows of b for every row of a
// (consumers.py: pearson_topk_both).  The result equals skr_topk_merge_rows on the transposed block with row_global0 and
// col_global0 swapped; no transposed copy is ever written.
//
// A workgroup owns a strip of kColsStrip = 32 columns — one 128-byte line of every row — and walks the rows.  A sweep
// step is kColsStep = 16 rows: thread t reads column t & 31 of rows (t >> 5) and (t >> 5) + 8 of the step, so each half
// of a wave reads 128 contiguous bytes of one row (dword loads: a row may start at any offset from a 16-byte boundary)
// and every cell is read once, whatever k is.  A thread keeps its column for the whole strip, so the column's bound — the
// list's k-th key, 0 while the list is not full — sits in a register.  A cell that beats the bound is appended to ITS
// COLUMN's candidate segment in LDS (kColsCap = 64 slots per column, the slot taken by an LDS atomic: the order inside a
// segment does not matter, since the order of the keys is total).  When a segment might not hold the next step (more
// than kColsCap - kColsStep candidates wait in some column) every column that has candidates is merged by one wave:
// the segment is sorted in registers (bitonic over the 64 lanes, shuffles only), the lane-wise maximum of the sorted list
// and the reversed sorted segment is the bitonic sequence of the 64 best, one bitonic merge sorts it, the best k are the
// list and the bound tightens.  That is why kColsKmax = 64: one list slot per lane.  On columns in random order the cells
// that beat the bound after the first merge number about k ln(nrows / kColsCap) per column, so the merges are few.
//
// LDS: lists 32 x 65 x (8 + 4) bytes, segments the same (the pitch of 65 entries spreads the 32 columns of a half wave
// over the banks when they append at the same depth), 32 counters: 48.9 KiB, three workgroups per CU.
#include "block.hpp"
#include "common.hpp"
#include "device_flag.hpp"
#include "topk_key.hpp"

namespace {

constexpr int kColsKmax = 64;    // list slots per column: one per lane of the merging wave
constexpr int kColsStrip = 32;   // columns per workgroup
constexpr int kColsStep = 16;    // rows per sweep step: 256 threads x 2 rows / 32 columns
constexpr int kColsCap = 64;     // candidates per column segment; merged as one wave-wide sort
constexpr int kColsPitch = 65;   // entries between two columns' slots in LDS
static_assert(kColsCap == 64 && kColsKmax == 64, "a segment and a list are one register per lane of a wave");
static_assert(kColsStep <= kColsCap, "an empty segment must hold one step");
static_assert(kColsStrip * 8 == 256 && kColsStep == 16, "thread t: column t & 31, rows t >> 5 and (t >> 5) + 8");

struct ColsArgs {
    SkrBlock b;
    int exclude_diag, k, first;
    uint32_t* io_idx;
    float* io_val;
    int* saw_nan;  // device flag, or NULL
};

struct ColsEntry {
    unsigned long long key;  // 0 = no entry
    uint32_t val;            // the cell's own bits
};

__device__ __forceinline__ ColsEntry cols_shfl_xor(const ColsEntry& e, int mask) {
    return ColsEntry{__shfl_xor(e.key, mask, 64), __shfl_xor(e.val, mask, 64)};
}

// one entry per lane, any order -> lane l holds the l-th best.  Entries with equal keys (only "no entry") stay put.
__device__ __forceinline__ ColsEntry cols_wave_sort(ColsEntry e, int lane) {
#pragma unroll
    for (int size = 2; size <= 64; size <<= 1)
#pragma unroll
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            const ColsEntry o = cols_shfl_xor(e, stride);
            const bool want_max = ((lane & stride) == 0) == ((lane & size) == 0);  // descending over the whole wave
            if (want_max ? o.key > e.key : o.key < e.key) e = o;
        }
    return e;
}

// a bitonic sequence over the lanes -> descending
__device__ __forceinline__ ColsEntry cols_wave_merge(ColsEntry e, int lane) {
#pragma unroll
    for (int stride = 32; stride > 0; stride >>= 1) {
        const ColsEntry o = cols_shfl_xor(e, stride);
        if ((lane & stride) == 0 ? o.key > e.key : o.key < e.key) e = o;
    }
    return e;
}

__global__ __launch_bounds__(256) void topk_cols_kernel(ColsArgs a) {
    __shared__ unsigned long long lkey[kColsStrip][kColsPitch];  // the lists, best first; 0 = no entry
    __shared__ uint32_t lval[kColsStrip][kColsPitch];
    __shared__ unsigned long long ckey[kColsStrip][kColsPitch];  // the candidate segments
    __shared__ uint32_t cval[kColsStrip][kColsPitch];
    __shared__ unsigned ccount[kColsStrip];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, k = a.k;
    const int c = tid & (kColsStrip - 1), slot = tid >> 5;  // this thread's column of the strip, and its row of a step
    constexpr int kPerWave = kColsStrip / 4;                // columns a wave merges
    const int64_t strips = (a.b.col_end - a.b.col_begin + kColsStrip - 1) / kColsStrip;
    bool nan_seen = false;

    // every column's candidates into its list (every thread calls it; wave w serves columns w * 8 ... w * 8 + 7)
    auto flush = [&]() {
        for (int q = 0; q < kPerWave; q++) {
            const int cc = wave * kPerWave + q;
            const unsigned n = ccount[cc];  // <= kColsCap
            if (n == 0) continue;           // (the same for every lane of the wave)
            ColsEntry cand{0ull, 0u};
            if ((unsigned)lane < n) cand = ColsEntry{ckey[cc][lane], cval[cc][lane]};
            cand = cols_wave_sort(cand, lane);
            ColsEntry l{lkey[cc][lane], lval[cc][lane]};
            const ColsEntry o{__shfl(cand.key, 63 - lane, 64), __shfl(cand.val, 63 - lane, 64)};
            if (o.key > l.key) l = o;  // the 64 best of the 128, as a bitonic sequence
            l = cols_wave_merge(l, lane);
            if (lane >= k) l = ColsEntry{0ull, 0u};
            lkey[cc][lane] = l.key, lval[cc][lane] = l.val;
        }
        __syncthreads();
        if (tid < kColsStrip) ccount[tid] = 0u;
        __syncthreads();
    };

    for (int64_t s = blockIdx.x; s < strips; s += gridDim.x) {
        const int64_t j0 = a.b.col_begin + s * kColsStrip;  // the strip's first column in r
        const int ncols = (int)std::min<int64_t>(kColsStrip, a.b.col_end - j0);
        for (int q = 0; q < kPerWave; q++) {
            const int cc = wave * kPerWave + q;
            ColsEntry e{0ull, 0u};
            if (!a.first) {  // the running list in key order, whatever order it came in
                if (cc < ncols && lane < k) {
                    const size_t at = (size_t)(j0 - a.b.col_begin + cc) * k + lane;
                    const uint32_t idx = a.io_idx[at];
                    const float v = a.io_val[at];
                    e.val = __float_as_uint(v);
                    if (idx != 0xFFFFFFFFu) e.key = topk_key(v, idx);  // a padded slot is no entry, not a NaN candidate
                }
                e = cols_wave_sort(e, lane);
            }
            lkey[cc][lane] = e.key, lval[cc][lane] = e.val;
        }
        if (tid < kColsStrip) ccount[tid] = 0u;
        __syncthreads();
        unsigned long long bound = lkey[c][k - 1];

        const bool col_ok = c < ncols;
        const int64_t jc = j0 + c;
        const int64_t skip = a.exclude_diag ? a.b.col_global0 + jc - a.b.row_global0 : -1;  // local row of the diagonal
        const float* col = a.b.r + jc;
        float cur[2], nxt[2];
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const int64_t i = slot + 8 * h;
            cur[h] = col_ok && i < a.b.rows ? col[(size_t)i * a.b.ld] : 0.f;
        }
        for (int64_t i0 = 0; i0 < a.b.rows; i0 += kColsStep) {
            // the next step's cells are on their way while this step is ranked
#pragma unroll
            for (int h = 0; h < 2; h++) {
                const int64_t i = i0 + kColsStep + slot + 8 * h;
                nxt[h] = col_ok && i < a.b.rows ? col[(size_t)i * a.b.ld] : 0.f;
            }
            int crowded = 0;
#pragma unroll
            for (int h = 0; h < 2; h++) {
                const int64_t i = i0 + slot + 8 * h;
                const bool in = col_ok && i < a.b.rows && i != skip;
                const float v = cur[h];
                nan_seen = nan_seen || (in && v != v);
                const unsigned long long key = topk_key(v, (uint32_t)(a.b.row_global0 + i));
                if (in && key > bound) {
                    // before a step no segment holds more than kColsCap - kColsStep entries, and a step adds at most
                    // kColsStep to a column: pos < kColsCap
                    const unsigned pos = atomicAdd(&ccount[c], 1u);
                    ckey[c][pos] = key, cval[c][pos] = __float_as_uint(v);
                    crowded |= pos + 1 + kColsStep > kColsCap;
                }
            }
            if (__syncthreads_or(crowded)) {  // some segment might not hold the next step
                flush();
                bound = lkey[c][k - 1];
            }
            cur[0] = nxt[0], cur[1] = nxt[1];
        }
        flush();
        for (int q = 0; q < kPerWave; q++) {
            const int cc = wave * kPerWave + q;
            if (cc < ncols && lane < k) {
                const size_t at = (size_t)(j0 - a.b.col_begin + cc) * k + lane;
                const unsigned long long key = lkey[cc][lane];
                a.io_idx[at] = key ? 0xFFFFFFFFu - (uint32_t)key : 0xFFFFFFFFu;
                a.io_val[at] = __uint_as_float(key ? lval[cc][lane] : 0x7FC00000u);
            }
        }
        __syncthreads();
    }
    if (nan_seen && a.saw_nan) atomicOr(a.saw_nan, 1);
}

}  // namespace

extern "C" int skr_topk_merge_cols_limits(int* kmax, int* strip_cols, int* rows_step, int* candidate_cap) {
    if (kmax) *kmax = kColsKmax;
    if (strip_cols) *strip_cols = kColsStrip;
    if (rows_step) *rows_step = kColsStep;
    if (candidate_cap) *candidate_cap = kColsCap;
    return SKR_OK;
}

extern "C" int skr_topk_merge_cols(skr_ctx* ctx, const skr_mat* r, int64_t nrows, int64_t col_begin, int64_t col_end,
                                   int64_t row_global0, int64_t col_global0, int exclude_diag, int k, int first,
                                   skr_mat* io_idx, skr_mat* io_val, int* saw_nan) {
    SkrBlock b;  // rows are written, and 0xFFFFFFFF is the index of an unfilled slot; columns as in skr_topk_merge_rows
    SKR_TRY(skr_block(ctx, r, nrows, col_begin, col_end, row_global0, col_global0, SKR_FIT_BOTH, &b));
    SKR_REQUIRE(io_idx && io_val, "NULL argument");
    SKR_REQUIRE(io_idx->ctx == ctx && io_val->ctx == ctx, "foreign ctx");
    SKR_REQUIRE(io_idx->dtype == SKR_U32 && io_val->dtype == SKR_F32, "io_idx U32, io_val F32");
    SKR_REQUIRE(k >= 1 && k <= kColsKmax, "k must be in 1..%d (the column lists are one slot per lane of a wave)", kColsKmax);
    const int64_t width = col_end - col_begin;
    SKR_REQUIRE(io_idx->rows * io_idx->cols >= width * k && io_val->rows * io_val->cols >= width * k,
                "the lists must hold %lld cells", (long long)(width * k));
    SKR_TRY(skr_activate(ctx));
    if (saw_nan) *saw_nan = 0;
    if (width == 0) return SKR_OK;
    SkrDeviceFlag<int> nan_flag;
    SKR_TRY(nan_flag.arm(ctx, saw_nan != nullptr));
    {
        SkrProfScope prof(ctx, "topk_merge_cols");
        const ColsArgs a{b, exclude_diag != 0, k, first != 0, (uint32_t*)io_idx->data, (float*)io_val->data, nan_flag.d};
        const int64_t strips = (width + kColsStrip - 1) / kColsStrip;
        hipLaunchKernelGGL(topk_cols_kernel, dim3((unsigned)std::min<int64_t>(strips, (int64_t)ctx->num_cu * 4)), dim3(256), 0,
                           ctx->stream, a);
        SKR_HIP(hipGetLastError());
    }
    return nan_flag.read(ctx, saw_nan);  // no flag asked for: no wait for the device
}
