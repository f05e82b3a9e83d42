// Per-row top-k in ONE pass over the row, with a running result: row i's new list is the k best entries of the union
// of the list it had on entry and the cells of the block, in topk_key's order (value descending, -0 == +0, NaN after
// every number, ties to the smaller GLOBAL column).  The order is total, so a row merged panel by panel gives the same
// list whatever the split — which is what lets r be consumed one [stripe, panel] block at a time (consumers.py:
// pearson_topk) or one chunk of windows at a time (windows.py: domain_topk) without ever standing whole anywhere.
//
// One workgroup per row.  The row's list (k keys, best first, 0 = no entry) and a candidate buffer live in LDS.  A sweep
// step takes kTopkStep cells (one float4 per thread; a scalar head and tail where the row does not start or end on a
// 16-byte boundary); cells whose key beats the bound — the list's k-th key, 0 while the list is not full — are compacted
// into the buffer by wave ballots.  When the next step might not fit (more than kTopkCap - kTopkStep candidates wait)
// the buffer and the list are sorted together (bitonic, keys with their value bits as payload), the best k become the
// list and the bound tightens.  Every cell is read once, whatever k is; on rows in random order the number of cells
// that beat the bound after the first flush is about k ln(width / kTopkStep), so the sorts are few.
#include "block.hpp"
#include "common.hpp"
#include "device_flag.hpp"
#include "topk_key.hpp"

namespace {

constexpr int kTopkKmax = 256;                     // list slots in LDS
constexpr int kTopkStep = 1024;                    // cells per sweep step: 256 threads x 4
constexpr int kTopkCap = 1792;                     // candidate buffer; list + buffer = the 2 048 entries one sort takes
constexpr int kTopkSort = kTopkCap + kTopkKmax;    // 24 KiB of keys and values + 3 KiB of list: five workgroups per CU
static_assert((kTopkSort & (kTopkSort - 1)) == 0, "the sort takes a power of two");
static_assert(kTopkStep <= kTopkCap, "an empty buffer must hold one step");

struct TopkArgs {
    SkrBlock b;
    int exclude_diag, k, first;
    uint32_t* io_idx;
    float* io_val;
    int* saw_nan;  // device flag, or NULL
};

struct TopkCells {  // the four cells of one thread in one sweep step
    float v[4];
    bool ok[4];
};

// cells c0 .. c0 + 3 of the row (row + c0 is 16-byte aligned); only those inside [col_begin, col_end) are read
__device__ __forceinline__ TopkCells topk_load(const float* row, int64_t c0, int64_t col_begin, int64_t col_end) {
    TopkCells q;
    if (c0 >= col_begin && c0 + 4 <= col_end) {
        const float4 f = *reinterpret_cast<const float4*>(row + c0);
        q.v[0] = f.x, q.v[1] = f.y, q.v[2] = f.z, q.v[3] = f.w;
        q.ok[0] = q.ok[1] = q.ok[2] = q.ok[3] = true;
    } else {
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int64_t c = c0 + j;
            q.ok[j] = c >= col_begin && c < col_end;
            q.v[j] = q.ok[j] ? row[c] : 0.f;
        }
    }
    return q;
}

__global__ __launch_bounds__(256) void topk_merge_kernel(TopkArgs a) {
    __shared__ unsigned long long skey[kTopkSort];  // candidates from 0; the list joins them for a sort
    __shared__ uint32_t sval[kTopkSort];            // the cells' own bits
    __shared__ unsigned long long lkey[kTopkKmax];  // the list, best first; 0 = no entry
    __shared__ uint32_t lval[kTopkKmax];
    __shared__ unsigned wave_n[2][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, k = a.k;
    const unsigned long long below = (1ull << lane) - 1;
    bool nan_seen = false;

    // list + the first `ncand` candidates -> list (uniform arguments; every thread calls it)
    auto flush = [&](int ncand) {
        const int m = ncand + k;
        int n2 = 2;
        while (n2 < m) n2 <<= 1;  // <= kTopkSort: ncand <= kTopkCap, k <= kTopkKmax
        for (int t = tid; t < k; t += 256) skey[ncand + t] = lkey[t], sval[ncand + t] = lval[t];
        for (int t = m + tid; t < n2; t += 256) skey[t] = 0ull, sval[t] = 0u;
        __syncthreads();
        for (int size = 2; size <= n2; size <<= 1)
            for (int stride = size >> 1; stride > 0; stride >>= 1) {
                for (int t = tid; t < (n2 >> 1); t += 256) {
                    const int lo = 2 * t - (t & (stride - 1)), hi = lo + stride;
                    const unsigned long long x = skey[lo], y = skey[hi];
                    if ((x < y) == ((lo & size) == 0)) {  // descending over the whole array
                        skey[lo] = y, skey[hi] = x;
                        const uint32_t u = sval[lo];
                        sval[lo] = sval[hi], sval[hi] = u;
                    }
                }
                __syncthreads();
            }
        for (int t = tid; t < k; t += 256) lkey[t] = skey[t], lval[t] = sval[t];
        __syncthreads();
    };

    for (int64_t i = blockIdx.x; i < a.b.rows; i += gridDim.x) {
        const size_t out0 = (size_t)i * k;
        for (int t = tid; t < k; t += 256) {
            unsigned long long key = 0ull;
            uint32_t bits = 0u;
            if (!a.first) {
                const uint32_t idx = a.io_idx[out0 + t];
                const float v = a.io_val[out0 + t];
                bits = __float_as_uint(v);
                if (idx != 0xFFFFFFFFu) key = topk_key(v, idx);  // a padded slot is no entry, not a NaN candidate
            }
            lkey[t] = key, lval[t] = bits;
        }
        __syncthreads();
        if (!a.first) flush(0);  // the running list in key order, whatever order it came in
        unsigned long long bound = lkey[k - 1];

        const float* row = a.b.r + (size_t)i * a.b.ld;
        // the sweep starts at the 16-byte boundary at or below the first cell: never below the matrix, since the
        // matrix itself starts on one
        const int64_t start = a.b.col_begin - (int64_t)((reinterpret_cast<uintptr_t>(row + a.b.col_begin) >> 2) & 3);
        const int64_t ngroups = (a.b.col_end - start + 3) / 4;
        const int64_t skip = a.exclude_diag ? a.b.row_global0 + i - a.b.col_global0 : -1;  // local column of the diagonal
        int ncand = 0;
        unsigned it = 0;
        TopkCells cur = topk_load(row, start + 4 * (int64_t)tid, a.b.col_begin, tid < ngroups ? a.b.col_end : a.b.col_begin);
        for (int64_t g0 = 0; g0 < ngroups; g0 += 256, it++) {
            const int64_t c0 = start + 4 * (g0 + tid);
            // the next step's cells are on their way while this step is ranked
            const int64_t gn = g0 + 256 + tid;
            const TopkCells nxt = topk_load(row, start + 4 * gn, a.b.col_begin, gn < ngroups ? a.b.col_end : a.b.col_begin);
            if (ncand + kTopkStep > kTopkCap) {
                flush(ncand);
                ncand = 0;
                bound = lkey[k - 1];
            }
            unsigned long long key[4], mask[4];
            bool pass[4];
            unsigned cnt = 0;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int64_t c = c0 + j;
                const bool in = cur.ok[j] && c != skip;
                nan_seen = nan_seen || (in && cur.v[j] != cur.v[j]);
                key[j] = topk_key(cur.v[j], (uint32_t)(a.b.col_global0 + c));
                pass[j] = in && key[j] > bound;
                mask[j] = __ballot(pass[j]);
                cnt += (unsigned)__popcll(mask[j]);
            }
            if (lane == 0) wave_n[it & 1][wave] = cnt;  // two sets: a wave may write step t + 1 while another reads t
            __syncthreads();
            unsigned before = 0, all = 0;
#pragma unroll
            for (int w = 0; w < 4; w++) {
                const unsigned n = wave_n[it & 1][w];
                if (w < wave) before += n;
                all += n;
            }
            unsigned pos = (unsigned)ncand + before;  // ncand + all <= kTopkCap: checked above
#pragma unroll
            for (int j = 0; j < 4; j++) {
                if (pass[j]) {
                    const unsigned p = pos + (unsigned)__popcll(mask[j] & below);
                    skey[p] = key[j], sval[p] = __float_as_uint(cur.v[j]);
                }
                pos += (unsigned)__popcll(mask[j]);
            }
            ncand += (int)all;
            cur = nxt;
        }
        if (ncand) flush(ncand);
        for (int t = tid; t < k; t += 256) {
            const unsigned long long key = lkey[t];
            a.io_idx[out0 + t] = key ? 0xFFFFFFFFu - (uint32_t)key : 0xFFFFFFFFu;
            a.io_val[out0 + t] = __uint_as_float(key ? lval[t] : 0x7FC00000u);
        }
        __syncthreads();
    }
    if (nan_seen && a.saw_nan) atomicOr(a.saw_nan, 1);
}

}  // namespace

extern "C" int skr_topk_merge_limits(int* kmax, int* candidate_cap) {
    if (kmax) *kmax = kTopkKmax;
    if (candidate_cap) *candidate_cap = kTopkCap;
    return SKR_OK;
}

extern "C" int skr_topk_merge_rows(skr_ctx* ctx, const skr_mat* r, int64_t nrows, int64_t col_begin, int64_t col_end,
                                   int64_t row_global0, int64_t col_global0, int exclude_diag, int k, int first,
                                   skr_mat* io_idx, skr_mat* io_val, int* saw_nan) {
    SkrBlock b;  // only columns are written; 0xFFFFFFFF is the index of an unfilled slot
    SKR_TRY(skr_block(ctx, r, nrows, col_begin, col_end, row_global0, col_global0, SKR_FIT_COLS, &b));
    SKR_REQUIRE(io_idx && io_val, "NULL argument");
    SKR_REQUIRE(io_idx->ctx == ctx && io_val->ctx == ctx, "foreign ctx");
    SKR_REQUIRE(io_idx->dtype == SKR_U32 && io_val->dtype == SKR_F32, "io_idx U32, io_val F32");
    SKR_REQUIRE(k >= 1 && k <= kTopkKmax, "k must be in 1..%d (skr_topk_rows serves a block that stands whole up to 4096)",
                kTopkKmax);
    SKR_REQUIRE(io_idx->rows * io_idx->cols >= nrows * k && io_val->rows * io_val->cols >= nrows * k,
                "the lists must hold %lld cells", (long long)(nrows * k));
    SKR_TRY(skr_activate(ctx));
    if (saw_nan) *saw_nan = 0;
    if (nrows == 0) return SKR_OK;
    SkrDeviceFlag<int> nan_flag;
    SKR_TRY(nan_flag.arm(ctx, saw_nan != nullptr));
    {
        SkrProfScope prof(ctx, "topk_merge_rows");
        const TopkArgs a{b, exclude_diag != 0, k, first != 0, (uint32_t*)io_idx->data, (float*)io_val->data, nan_flag.d};
        hipLaunchKernelGGL(topk_merge_kernel, dim3((unsigned)std::min<int64_t>(nrows, (int64_t)ctx->num_cu * 8)), dim3(256), 0,
                           ctx->stream, a);
        SKR_HIP(hipGetLastError());
    }
    return nan_flag.read(ctx, saw_nan);  // no flag asked for: no wait for the device
}
