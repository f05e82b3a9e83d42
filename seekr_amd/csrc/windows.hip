// K2w — k-mer counting in sliding windows: one row of the output per WINDOW (sequence, start, length) of the packed
// sequences, bit for bit the row count.hip writes when the window's substring is packed as a sequence of its own
// (W = length - k + 1 windows of k letters counted in the per-kb increment, a k-mer over a non-alphabet base skipped but
// counted in W: kmer_counts.py:143-149; the same per_kb_value and the same log2-pre conversion).
//
// The window table is never materialised.  Sequence i gives ceil(max(L_i - window, 0) / slide) + 1 rows, row j of it
// starts at base j * slide and holds min(window, L_i - j * slide) letters (Python's seq[start : start + window]);
// row_begin[i] = first row of sequence i is built once per (window, slide) and kept with the skr_seqs; the workgroup of a
// row finds its sequence by binary search in it.
//
// count_windows_kernel: a row is owned by ONE WAVE at k <= 6 (64-thread workgroups, no barrier) or by a 4-wave workgroup
// at k = 7, as in count_rows_kernel.  A window starts at any base, so lane l of a sweep takes the 16 k-mers that start at
// bases start + 16 l ...: it loads the three packed words those 16 + k - 1 <= 22 bases can touch and funnel-shifts them
// (v_alignbit) by the start's offset inside its word into the (hi, lo) pair count_rows_kernel works on — from there the
// column of k-mer j is the top 2k bits of alignbit(hi, lo, 32 - 2j) as before.  The validity bits of the same 22 bases
// come from two mask words shifted by the base offset.  Bins live in the LDS: 16-bit counters packed two to a word
// (bin b and bin b + 4^k/2 share a word) while a window has at most 65 535 k-mers — 8 KiB a row at k = 6 — and 32-bit
// counters (WIDE) for longer windows.  ds_add_u32 without return; a sweep whose 64 lanes all hold the same (hi, lo)
// (homopolymers, short-period repeats: what the XIST-like queries of this analysis are made of) adds 64 from one lane.
// The flush reads four LDS words per lane step, converts through the 16-entry table of per-kb values of the row's W and
// streams 16-byte pieces of the dense row with nontemporal stores.  The row write — 4 * 4^k bytes per window against
// window / 4 bytes read, most of them L2 hits, consecutive windows overlap — bounds the kernel.  One workgroup per row,
// dispatched by the hardware in row order, as count_rows_kernel does it: the rows being written form a compact front.
// Bins, sweep, flush and launch LDS are the shared code of count_bins.hpp; the kernel below is what a window adds: the
// search in row_begin, the three-word funnel shift, the mask words at a base offset.
// (Runs of 2 / 4 / 8 / 16 consecutive rows per workgroup, with the next row's words in flight across the flush, were
// measured 3-7 % slower at 999 550 rows of k = 6 and removed: DESIGN section 4.)
//
// Counting each window afresh was kept: an incremental slide (drop `slide` k-mers, add `slide`) saves LDS atomics — 16
// per lane and row at window 1 000 — that are not what bounds the kernel, and needs 32-bit or signed bins.
#include <algorithm>
#include <vector>

#include "common.hpp"
#include "count_bins.hpp"  // OutKind, BinGeom, sweep_pair, flush_row, row_launch_lds (shared with count.hip)

namespace {

struct WinArgs {
    const uint32_t* packed;
    const int64_t* word_off;
    const int64_t* len;
    const uint32_t* mask;
    const int64_t* mask_off;
    const int64_t* row_begin;  // [n_seqs + 1]
    int64_t n_seqs;
    int64_t first_row, n_rows;  // rows [first_row, first_row + n_rows) of the table -> rows 0 .. n_rows-1 of out
    int64_t window, slide;
    void* out;
    int k;
};

template <int OUT, int WPS, bool WIDE>
__global__ __launch_bounds__(WPS * 64) void count_windows_kernel(const WinArgs a) {
    constexpr int T = WPS * 64;
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const int tid = threadIdx.x;
    const int k = a.k;
    const BinGeom<WIDE> g(lds, k, tid);
    const int64_t r = blockIdx.x;  // row of `out`
    const int64_t gr = a.first_row + r;  // row of the table
    g.template zero<T>(tid);

    // the row's sequence: the last i with row_begin[i] <= gr (every sequence has at least one row)
    int64_t seq = 0;
    for (int64_t hi = a.n_seqs - 1; seq < hi;) {
        const int64_t mid = (seq + hi + 1) >> 1;
        if (a.row_begin[mid] <= gr) seq = mid;
        else hi = mid - 1;
    }
    const int64_t L = a.len[seq], moff = a.mask_off[seq];
    const int64_t start = (gr - a.row_begin[seq]) * a.slide;
    const int64_t length = L - start < a.window ? L - start : a.window;  // seq[start : start + window]
    const int64_t Wtot = length - k + 1;  // k-mers, counting every character (kmer_counts.py:143-144)
    const int64_t Wn = Wtot > 0 ? Wtot : 0;
    const int64_t nww = (Wn + 15) >> 4;
    const double inc = Wtot > 0 ? 1000.0 / (double)Wtot : 0.0;
    build_value_table<OUT>(g.tab, tid, inc);
    const uint32_t bsh = (uint32_t)(start & 15) * 2;  // bit offset of the window's first base inside its packed word
    const uint32_t* words = a.packed + a.word_off[seq] + (start >> 4);
    if (WPS > 1) __syncthreads();  // bins zeroed
    else __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // one wave: the LDS executes its instructions in order

    for (int64_t base = 0; base < nww; base += T) {
        const int64_t w = base + tid;
        // The lane's word, clamped to the last one that holds the start of a k-mer: words wc + 1 and wc + 2 are then at
        // worst the sequence's pad word and the word after it (the next sequence's first, or the slack behind the last).
        const int64_t wc = w < nww ? w : nww - 1;
        const uint32_t wa = words[wc], wb = words[wc + 1], wc3 = words[wc + 2];
        // the 32 bases that start at base `start + 16 w`, first base in the top bits
        const uint32_t hi = bsh ? __builtin_amdgcn_alignbit(wa, wb, 32 - bsh) : wa;
        const uint32_t lo = bsh ? __builtin_amdgcn_alignbit(wb, wc3, 32 - bsh) : wb;
        sweep_pair(g, tid, hi, lo, moff < 0 && Wn - ((base + T - 1) << 4) >= 16, Wn - (w << 4), [&]() -> uint32_t {
            if (moff < 0) return 0;  // bit j: base start + 16 w + j is not in the alphabet
            const int64_t pbase = start + (wc << 4);
            const uint32_t* mwords = a.mask + moff + (pbase >> 5);
            return (uint32_t)(((unsigned long long)mwords[0] | ((unsigned long long)mwords[1] << 32)) >> (pbase & 31));
        });
    }
    if (WPS > 1) __syncthreads();
    else __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");

    // ---- flush: bins -> output values, dense row to HBM (one row per workgroup: nothing to zero, nothing read again)
    flush_row<OUT, WIDE, false, false, T>(g, tid, reinterpret_cast<uint32_t*>(a.out) + (size_t)r * g.nbins, inc);
}

template <int OUT, int WPS, bool WIDE>
int launch_windows(skr_ctx* ctx, const WinArgs& a, const char* name) {
    const int k = a.k;
    auto kern = count_windows_kernel<OUT, WPS, WIDE>;
    // as many workgroups per CU as count_rows_kernel writes rows of this width fastest with (count_bins.hpp: 17 at k = 6)
    const size_t lds_launch = row_launch_lds<WIDE>(ctx, WPS, k);
    SKR_TRY(skr_kernel_lds(ctx, reinterpret_cast<const void*>(kern), lds_launch));
    SKR_REQUIRE(a.n_rows <= 0x7fffffff, "%lld rows in one call: count them in runs", (long long)a.n_rows);
    SkrProfScope prof(ctx, name);
    hipLaunchKernelGGL(kern, dim3((unsigned)a.n_rows), dim3(WPS * 64), lds_launch, ctx->stream, a);
    SKR_HIP(hipGetLastError());
    return SKR_OK;
}

template <int OUT>
int launch_windows_any(skr_ctx* ctx, const WinArgs& a, const char* name) {
    // 16-bit bins hold a window of up to 65 535 k-mers; longer windows count into 32-bit bins
    const bool wide = a.window - a.k + 1 > 65535;
    if (a.k <= 6) return wide ? launch_windows<OUT, 1, true>(ctx, a, name) : launch_windows<OUT, 1, false>(ctx, a, name);
    return wide ? launch_windows<OUT, 4, true>(ctx, a, name) : launch_windows<OUT, 4, false>(ctx, a, name);
}

int64_t windows_of_length(int64_t L, int64_t window, int64_t slide) {
    return L > window ? (L - window + slide - 1) / slide + 1 : 1;
}

// row_begin of (window, slide), built and uploaded when the pair differs from the one the skr_seqs holds
int window_table(skr_ctx* ctx, const skr_seqs* s, int64_t window, int64_t slide) {
    if (s->win_window == window && s->win_slide == slide && s->d_row_begin) return SKR_OK;
    std::vector<int64_t> rb((size_t)s->n + 1, 0);
    for (int64_t i = 0; i < s->n; i++) rb[i + 1] = rb[i] + windows_of_length(s->h_len[i], window, slide);
    SKR_HIP(hipStreamSynchronize(ctx->stream));  // a launch still in flight may read the table of the previous pair
    if (!s->d_row_begin) SKR_HIP(hipMalloc((void**)&s->d_row_begin, rb.size() * sizeof(int64_t)));
    s->win_window = s->win_slide = 0;
    SKR_HIP(hipMemcpyAsync(s->d_row_begin, rb.data(), rb.size() * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
    SKR_HIP(hipStreamSynchronize(ctx->stream));  // `rb` is pageable host memory
    s->h_row_begin.swap(rb);
    s->win_window = window;
    s->win_slide = slide;
    return SKR_OK;
}

int prepare_windows(skr_ctx* ctx, const skr_seqs* s, int k, int64_t window, int64_t slide, int64_t first_row, int64_t n_rows,
                    const skr_mat* out, WinArgs* a) {
    SKR_REQUIRE(ctx && s && out, "NULL argument");
    SKR_REQUIRE(s->ctx == ctx && out->ctx == ctx, "handles belong to a different ctx");
    SKR_REQUIRE(k >= 1, "k must be >= 1 (got %d)", k);
    SKR_REQUIRE(window >= 1 && slide >= 1 && slide <= window, "window >= 1 and 1 <= slide <= window expected (got window %lld, slide %lld)",
                (long long)window, (long long)slide);
    if (k > 7) return skr_set_error(SKR_ERR_UNSUPPORTED, "k=%d: windows are counted for k <= 7 (count the substrings with skr_count_per_kb)", k);
    if (out->dtype == SKR_F64) return skr_set_error(SKR_ERR_UNSUPPORTED, "float64 rows are not implemented for windows");
    SKR_TRY(skr_activate(ctx));
    SKR_TRY(window_table(ctx, s, window, slide));
    const int64_t total = s->h_row_begin[s->n];
    SKR_REQUIRE(first_row >= 0 && n_rows >= 0 && first_row + n_rows <= total, "rows [%lld, %lld) are outside the table of %lld windows",
                (long long)first_row, (long long)(first_row + n_rows), (long long)total);
    SKR_REQUIRE(out->rows == n_rows && out->cols == ((int64_t)1 << (2 * k)), "output must be [%lld, %lld], got [%lld, %lld]",
                (long long)n_rows, (long long)1 << (2 * k), (long long)out->rows, (long long)out->cols);
    *a = WinArgs{s->d_packed, s->d_word_off, s->d_len, s->d_mask, s->d_mask_off, s->d_row_begin, s->n, first_row, n_rows,
                 window, slide, out->data, k};
    return SKR_OK;
}

// does a row of [first_row, first_row + n_rows) hold exactly k - 1 letters (1000 / 0 in the reference, kmer_counts.py:144)?
bool has_zero_window(const skr_seqs* s, int k, int64_t window, int64_t slide, int64_t first_row, int64_t n_rows) {
    if (n_rows < 1) return false;
    const std::vector<int64_t>& rb = s->h_row_begin;
    int64_t i = std::upper_bound(rb.begin(), rb.end(), first_row) - rb.begin() - 1;
    for (; i < s->n && rb[i] < first_row + n_rows; i++) {
        const int64_t last = rb[i + 1] - 1;  // the sequence's last row: the only one that may be shorter than `window`
        const int64_t last_len = std::min(window, s->h_len[i] - (last - rb[i]) * slide);
        if (last >= first_row && last < first_row + n_rows && last_len == k - 1) return true;
        // its other rows hold `window` letters
        if (window == k - 1 && std::max(rb[i], first_row) < std::min(last, first_row + n_rows)) return true;
    }
    return false;
}

}  // namespace

extern "C" int skr_count_windows_u32(skr_ctx* ctx, const skr_seqs* s, int k, int64_t window, int64_t slide, int64_t first_row,
                                     int64_t n_rows, skr_mat* out) {
    WinArgs a;
    SKR_TRY(prepare_windows(ctx, s, k, window, slide, first_row, n_rows, out, &a));
    SKR_REQUIRE(out->dtype == SKR_U32, "skr_count_windows_u32 needs a SKR_U32 matrix");
    if (n_rows == 0) return SKR_OK;
    return launch_windows_any<OUT_U32>(ctx, a, "count_windows_u32");
}

extern "C" int skr_count_windows_per_kb(skr_ctx* ctx, const skr_seqs* s, int k, int64_t window, int64_t slide, int64_t first_row,
                                        int64_t n_rows, int log2_pre, skr_mat* out) {
    WinArgs a;
    SKR_TRY(prepare_windows(ctx, s, k, window, slide, first_row, n_rows, out, &a));
    SKR_REQUIRE(out->dtype == SKR_F32, "skr_count_windows_per_kb needs a SKR_F32 matrix");
    if (has_zero_window(s, k, window, slide, first_row, n_rows))
        return skr_set_error(SKR_ERR_ZERODIV, "division by zero");  // the text Python gives `1000 / 0` (kmer_counts.py:144)
    if (n_rows == 0) return SKR_OK;
    if (log2_pre) return launch_windows_any<OUT_F32_LOG2>(ctx, a, "count_windows_f32_log2");
    return launch_windows_any<OUT_F32>(ctx, a, "count_windows_f32");
}
