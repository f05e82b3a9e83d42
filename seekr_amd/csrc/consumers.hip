// Consumers of the Pearson matrix that the reference runs right after `pearson`:
//   * kmer_leiden.py:94-96   ld_sim[ld_sim < cutoff] = 0; np.fill_diagonal(ld_sim, 0)
//   * find_dist.py:163       sim_counts[np.triu_indices(N, k=1)]   (+ :169 random subsample)
//   * find_pval.py:158-164   p[i,j] = np.sum(fitres > sim[i,j]) / len(fitres)   (O(M N |fitres|) Python loop)
// All three are streaming passes over r in HBM (HBM-bound); keeping them on the device avoids
// moving an N x N matrix over PCIe just to reduce it.
#include <algorithm>
#include <cstring>

#include "block.hpp"
#include "common.hpp"
#include "count_scan.hpp"
#include "device_flag.hpp"
#include "topk_key.hpp"

namespace {

__global__ __launch_bounds__(256) void threshold_zero_diag_kernel(float* __restrict__ r, int64_t rows, int64_t cols,
                                                                  float cutoff, int64_t diag_col0) {
    const int64_t total = rows * cols;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = i / cols, col = i % cols;
        float v = r[i];
        if (v < cutoff) v = 0.f;  // NaN < cutoff is false: NaN stays, as with numpy's boolean mask
        if (col == row + diag_col0) v = 0.f;
        r[i] = v;
    }
}

// out[start(i) + (j - i - k)] = r[i, j] for j >= i + k, start(i) = number of selected cells in rows < i:
// exactly the order of np.triu_indices(n, k).  One workgroup per row segment, coalesced copies.  float32 / float64.
template <typename T>
__global__ __launch_bounds__(256) void triu_flatten_kernel(const T* __restrict__ r, int64_t n, int64_t k,
                                                           T* __restrict__ out) {
    for (int64_t i = blockIdx.x; i < n; i += gridDim.x) {
        const int64_t first = i + k;
        if (first >= n) continue;
        // cells selected in rows 0..i-1: sum_{t<i} max(0, n - t - k)
        const int64_t full = std::min<int64_t>(i, std::max<int64_t>(0, n - k));
        const int64_t start = full * (n - k) - full * (full - 1) / 2;
        const T* src = r + (size_t)i * n + first;
        T* dst = out + start;
        for (int64_t c = threadIdx.x; c < n - first; c += blockDim.x) dst[c] = src[c];
    }
}

__global__ __launch_bounds__(256) void gather_kernel(const float* __restrict__ src, const int64_t* __restrict__ idx,
                                                     int64_t n, float* __restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        out[i] = src[idx[i]];
}

// p = float32( #(bg > v) / total ), bg ascending without NaN; #(bg > v) = n_bg - upper_bound(v).
// Two-level search: every `stride`-th background value sits in LDS (4096 entries), so 12 of the ~20
// steps of a 1 M-entry search are LDS reads and only the last ~8 walk one 256-entry bucket in the L2.
constexpr int kPvalTable = 4096;
__global__ __launch_bounds__(256) void empirical_p_kernel(const float* __restrict__ r, int64_t total_cells,
                                                          const float* __restrict__ bg, int64_t n_bg, double total_len,
                                                          float* __restrict__ p) {
    __shared__ float table[kPvalTable];
    const int64_t stride = (n_bg + kPvalTable - 1) / kPvalTable;          // table[t] = bg[min(n_bg-1, (t+1)*stride-1)]
    const int64_t n_table = (n_bg + stride - 1) / stride;                 // buckets actually used
    for (int64_t t = threadIdx.x; t < n_table; t += 256) table[t] = bg[std::min<int64_t>(n_bg - 1, (t + 1) * stride - 1)];
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total_cells; i += (int64_t)gridDim.x * blockDim.x) {
        const float v = r[i];
        int64_t lo;  // first index with bg[idx] > v
        if (v != v) {
            lo = n_bg;  // nothing compares greater than NaN
        } else {
            int64_t tl = 0, th = n_table;  // first bucket whose last value is > v
            while (tl < th) {
                const int64_t mid = (tl + th) >> 1;
                if (table[mid] > v) th = mid; else tl = mid + 1;
            }
            lo = tl * stride;
            int64_t hi = std::min<int64_t>(n_bg, lo + stride);
            if (tl == n_table) lo = hi = n_bg;
            while (lo < hi) {
                const int64_t mid = (lo + hi) >> 1;
                if (bg[mid] > v) hi = mid; else lo = mid + 1;
            }
        }
        p[i] = (float)((double)(n_bg - lo) / total_len);
    }
}

// ---- threshold -> edge list (kmer_leiden.py:94-96 without ever writing the zeros) -------------
// A cell survives `ld_sim[ld_sim < cutoff] = 0; np.fill_diagonal(ld_sim, 0)` as a non-zero iff
// !(v < cutoff) (NaN stays), v != 0 and it is off the diagonal.  upper: keep column > row only.
struct EdgeArgs {
    SkrBlock b;
    float cutoff;
    int upper;
};

__device__ __forceinline__ bool edge_kept(const EdgeArgs& a, int64_t grow, int64_t gcol, float v) {
    if (v < a.cutoff || v == 0.f) return false;
    return a.upper ? gcol > grow : gcol != grow;
}

__global__ __launch_bounds__(256) void edges_count_kernel(EdgeArgs a, unsigned long long* __restrict__ counts) {
    __shared__ unsigned red[4];
    for (int64_t i = blockIdx.x; i < a.b.rows; i += gridDim.x) {
        const float* row = a.b.r + (size_t)i * a.b.ld;
        const int64_t grow = a.b.row_global0 + i;
        unsigned n = 0;
        for (int64_t c = a.b.col_begin + threadIdx.x; c < a.b.col_end; c += 256) n += edge_kept(a, grow, a.b.col_global0 + c, row[c]);
        for (int off = 32; off; off >>= 1) n += __shfl_down(n, off, 64);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = n;
        __syncthreads();
        if (threadIdx.x == 0) counts[i] = (unsigned long long)red[0] + red[1] + red[2] + red[3];
        __syncthreads();
    }
}

// row-major order (== np.nonzero of the thresholded matrix): a workgroup walks its row 256 columns at
// a time; position inside the chunk from wave ballots + a 4-entry scan
__global__ __launch_bounds__(256) void edges_fill_kernel(EdgeArgs a, const unsigned long long* __restrict__ offsets,
                                                         uint32_t* __restrict__ out_row, uint32_t* __restrict__ out_col,
                                                         float* __restrict__ out_val) {
    __shared__ unsigned wave_n[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t i = blockIdx.x; i < a.b.rows; i += gridDim.x) {
        const float* row = a.b.r + (size_t)i * a.b.ld;
        const int64_t grow = a.b.row_global0 + i;
        unsigned long long base = offsets[i];
        for (int64_t c0 = a.b.col_begin; c0 < a.b.col_end; c0 += 256) {
            const int64_t c = c0 + threadIdx.x;
            const float v = c < a.b.col_end ? row[c] : 0.f;
            const bool keep = c < a.b.col_end && edge_kept(a, grow, a.b.col_global0 + c, v);
            const unsigned long long mask = __ballot(keep);
            if (lane == 0) wave_n[wave] = (unsigned)__popcll(mask);
            __syncthreads();
            unsigned before = 0, all = 0;
#pragma unroll
            for (int w = 0; w < 4; w++) {
                if (w < wave) before += wave_n[w];
                all += wave_n[w];
            }
            if (keep) {
                const unsigned long long pos = base + before + __popcll(mask & ((1ull << lane) - 1));
                out_row[pos] = (uint32_t)grow;
                out_col[pos] = (uint32_t)(a.b.col_global0 + c);
                out_val[pos] = v;
            }
            base += all;
            __syncthreads();
        }
    }
}

// ---- per-row top-k: the k largest cells of each row, descending, ties to the
// smaller column — np.argsort(-row, kind="stable")[:k] with NaN last and the row's own (global)
// diagonal cell excluded.  One workgroup per row; k selection passes over the row (it stays in the
// L2): pass t finds the largest key below the t-1-th winner.  Keys order (value desc, column asc).
// (The block arrives as its seven fields, not as an SkrBlock: the argument list is part of the kernel's symbol, and the
// committed counter summaries bench.py quotes belong to the library's present set of kernel symbols.)
__global__ __launch_bounds__(256) void topk_rows_kernel(const float* __restrict__ r, int64_t ld, int64_t rows,
                                                        int64_t col_begin, int64_t col_end, int64_t row_global0,
                                                        int64_t col_global0, int k, uint32_t* __restrict__ out_idx,
                                                        float* __restrict__ out_val) {
    __shared__ unsigned long long red[4];
    __shared__ unsigned long long s_best;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t i = blockIdx.x; i < rows; i += gridDim.x) {
        const float* row = r + (size_t)i * ld;
        const int64_t skip = row_global0 + i - col_global0;  // local column of the diagonal cell, if any
        unsigned long long bound = ~0ull;                     // keys must be strictly below this
        for (int t = 0; t < k; t++) {
            unsigned long long best = 0ull;
            for (int64_t c = col_begin + threadIdx.x; c < col_end; c += 256) {
                if (c == skip) continue;
                const unsigned long long key = topk_key(row[c], (uint32_t)(c - col_begin));
                if (key < bound && key > best) best = key;
            }
            for (int off = 32; off; off >>= 1) {
                const unsigned long long o = __shfl_down(best, off, 64);
                if (o > best) best = o;
            }
            if (lane == 0) red[wave] = best;
            __syncthreads();
            if (threadIdx.x == 0) {
                unsigned long long b = red[0];
                for (int w = 1; w < 4; w++) b = red[w] > b ? red[w] : b;
                s_best = b;
            }
            __syncthreads();
            best = s_best;
            if (threadIdx.x == 0) {
                if (best == 0ull) {  // fewer than k candidates in the row
                    out_idx[(size_t)i * k + t] = 0xFFFFFFFFu;
                    out_val[(size_t)i * k + t] = __uint_as_float(0x7FC00000u);
                } else {
                    const uint32_t c = 0xFFFFFFFFu - (uint32_t)best;
                    out_idx[(size_t)i * k + t] = (uint32_t)(col_global0 + col_begin + c);
                    out_val[(size_t)i * k + t] = row[col_begin + c];
                }
            }
            bound = best;
            if (best == 0ull) {  // nothing left: fill the remaining slots the same way
                for (int u = t + 1; u < k; u++)
                    if (threadIdx.x == 0) {
                        out_idx[(size_t)i * k + u] = 0xFFFFFFFFu;
                        out_val[(size_t)i * k + u] = __uint_as_float(0x7FC00000u);
                    }
                break;
            }
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------
// Parametric p-values (find_pval.py:118-133): p[i,j] = 1 - dist(*params).cdf(sim[i,j]) for the scipy.stats
// distribution find_dist fitted (find_dist.py:96-98, the `common10` list).  scipy evaluates the cdf of a float32
// argument in float64, `1 - cdf` in float64, and the assignment into np.zeros_like(sim) rounds to float32: the
// kernel does the same, one cell per thread.  params = shape parameters..., loc, scale as scipy orders them.
// ---------------------------------------------------------------------------------------
enum { DIST_CAUCHY = 0, DIST_CHI2, DIST_EXPON, DIST_EXPONPOW, DIST_GAMMA, DIST_LOGNORM, DIST_NORM, DIST_PARETO, DIST_RAYLEIGH,
       DIST_UNIFORM, DIST_COUNT, DIST_BAD_SHAPE };

// regularised lower incomplete gamma P(a, x), float64: series for x < a + 1, Lentz continued fraction for Q otherwise
// (Abramowitz & Stegun 6.5.29 / 6.5.31).  Near x = a the terms of both fall like exp(-n^2 / 2a): reaching 1e-17 takes
// about 8.2 sqrt(a) of them at every shape from 1e2 to 1e8, and at most 110 for shapes below 50 (the fraction just
// above x = a + 1 for a small shape) — counted in a float64 port of these loops.  A fit to Pearson similarities does
// return shapes of 1e5 and more (a gamma that imitates a normal), so the loops run up to
//     gamma_max_terms(a) = 200 + 12 sqrt(a)      (38 147 at kGammaMaxShape)
// terms, 1.4 times what was counted.  Shapes outside [kGammaMinShape, kGammaMaxShape] are refused on the host: above,
// the rounding of a log(x) - lgamma(a) in the prefactor grows with a (against scipy the port uses 0.06 of the tests'
// 2e-6 relative bar at a = 1e7 and 0.43 at 1e8) and nothing is tested; below, 1 - P loses its digits (past the bar at
// a = 1e-10).  A loop that ends without converging sets `failed`: the call then fails instead of returning a number
// that is not scipy's.
constexpr double kGammaMinShape = 1e-6, kGammaMaxShape = 1e7;
inline int gamma_max_terms(double a) { return 200 + (int)(12.0 * sqrt(a)); }

__device__ double gamma_p(double a, double x, int max_terms, bool& failed) {
    if (!(x > 0.0)) return 0.0;
    if (isinf(x)) return 1.0;
    const double lg = lgamma(a);
    bool converged = false;
    if (x < a + 1.0) {
        double ap = a, del = 1.0 / a, sum = del;
        for (int n = 0; n < max_terms; n++) {  // bounded: max_terms <= gamma_max_terms(kGammaMaxShape)
            ap += 1.0;
            del *= x / ap;
            sum += del;
            if (fabs(del) < fabs(sum) * 1e-17) {
                converged = true;
                break;
            }
        }
        if (!converged) failed = true;
        return sum * exp(-x + a * log(x) - lg);
    }
    const double tiny = 1e-300;
    double b = x + 1.0 - a, c = 1.0 / tiny, d = 1.0 / b, h = d;
    for (int i = 1; i <= max_terms; i++) {  // bounded likewise
        const double an = -(double)i * ((double)i - a);
        b += 2.0;
        d = an * d + b;
        if (fabs(d) < tiny) d = tiny;
        c = b + an / c;
        if (fabs(c) < tiny) c = tiny;
        d = 1.0 / d;
        const double del = d * c;
        h *= del;
        if (fabs(del - 1.0) < 1e-16) {
            converged = true;
            break;
        }
    }
    if (!converged) failed = true;
    return 1.0 - exp(-x + a * log(x) - lg) * h;
}

struct DistParams {
    int dist;
    double shape, loc, scale;
    int max_terms;        // of gamma_p's loops (gamma, chi2)
    int* not_converged;   // device flag a cell raises when such a loop ends unconverged (gamma, chi2; else NULL)
};

__device__ __forceinline__ double dist_cdf(const DistParams& d, double x, bool& failed) {
    const double z = (x - d.loc) / d.scale;
    switch (d.dist) {
        case DIST_CAUCHY: return 0.5 + atan(z) / 3.14159265358979323846;
        case DIST_CHI2: return z > 0.0 ? gamma_p(0.5 * d.shape, 0.5 * z, d.max_terms, failed) : 0.0;
        case DIST_EXPON: return z > 0.0 ? -expm1(-z) : 0.0;
        case DIST_EXPONPOW: return z > 0.0 ? -expm1(-expm1(pow(z, d.shape))) : 0.0;
        case DIST_GAMMA: return z > 0.0 ? gamma_p(d.shape, z, d.max_terms, failed) : 0.0;
        case DIST_LOGNORM: return z > 0.0 ? 0.5 * erfc(-(log(z) / d.shape) * 0.70710678118654752440) : 0.0;
        case DIST_NORM: return 0.5 * erfc(-z * 0.70710678118654752440);
        case DIST_PARETO: return z >= 1.0 ? 1.0 - pow(z, -d.shape) : 0.0;
        case DIST_RAYLEIGH: return z > 0.0 ? -expm1(-0.5 * z * z) : 0.0;
        default: return z <= 0.0 ? 0.0 : (z >= 1.0 ? 1.0 : z);  // uniform
    }
}

__global__ __launch_bounds__(256) void parametric_p_kernel(const float* __restrict__ r, int64_t cells, DistParams d,
                                                           float* __restrict__ p) {
    bool failed = false;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < cells; i += (int64_t)gridDim.x * blockDim.x) {
        const double x = (double)r[i];
        // cdf(nan) is nan in scipy; so is every cdf of a distribution whose shape parameter fails scipy's _argcheck
        p[i] = (x != x || d.dist == DIST_BAD_SHAPE) ? NAN : (float)(1.0 - dist_cdf(d, x, failed));
    }
    if (failed && d.not_converged) atomicOr(d.not_converged, 1);  // gamma / chi2 only: the others never set it
}

// ---- stable selection: the positions i with (double)values[i] <= bound, ascending (NaN never passes) ----------
// Tiles of 256 values, a workgroup walks tiles blockIdx.x, blockIdx.x + gridDim.x, ...: counts[tile] first, then (after
// the exclusive scan of the counts) the positions, a value's place inside its tile from wave ballots as in
// edges_fill_kernel.
constexpr int kSelectTile = 256;

template <typename T>
__global__ __launch_bounds__(kSelectTile) void select_count_kernel(const T* __restrict__ v, int64_t n, double bound,
                                                                   int64_t tiles, unsigned long long* __restrict__ counts) {
    __shared__ unsigned red[kSelectTile / 64];
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int64_t i = t * kSelectTile + threadIdx.x;
        const bool keep = i < n && (double)v[i] <= bound;
        const unsigned long long mask = __ballot(keep);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = (unsigned)__popcll(mask);
        __syncthreads();
        if (threadIdx.x == 0) counts[t] = (unsigned long long)red[0] + red[1] + red[2] + red[3];
        __syncthreads();
    }
}

template <typename T>
__global__ __launch_bounds__(kSelectTile) void select_fill_kernel(const T* __restrict__ v, int64_t n, double bound,
                                                                  int64_t tiles, const unsigned long long* __restrict__ offsets,
                                                                  uint32_t* __restrict__ out) {
    __shared__ unsigned wave_n[kSelectTile / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int64_t i = t * kSelectTile + threadIdx.x;
        const bool keep = i < n && (double)v[i] <= bound;
        const unsigned long long mask = __ballot(keep);
        if (lane == 0) wave_n[wave] = (unsigned)__popcll(mask);
        __syncthreads();
        unsigned before = 0;
#pragma unroll
        for (int w = 0; w < kSelectTile / 64; w++)
            if (w < wave) before += wave_n[w];
        if (keep) out[offsets[t] + before + __popcll(mask & ((1ull << lane) - 1))] = (uint32_t)i;
        __syncthreads();
    }
}

// out[i] = src[index[i]], 4- or 8-byte cells; an index outside src raises the flag and writes nothing
template <typename W>
__global__ __launch_bounds__(256) void gather_index_kernel(const W* __restrict__ src, int64_t n_src, const uint32_t* __restrict__ index,
                                                           int64_t count, W* __restrict__ out, int* __restrict__ bad) {
    bool any_bad = false;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (int64_t)gridDim.x * 256) {
        const int64_t j = index[i];
        if (j < n_src) out[i] = src[j];
        else any_bad = true;
    }
    if (any_bad) atomicOr(bad, 1);
}

}  // namespace

extern "C" int skr_threshold_zero_diag(skr_ctx* ctx, skr_mat* r, float cutoff, int64_t diag_col0) {
    SKR_REQUIRE(ctx && r && r->ctx == ctx && r->dtype == SKR_F32, "need a float32 matrix of this ctx");
    SKR_TRY(skr_activate(ctx));
    if (r->rows * r->cols == 0) return SKR_OK;
    SkrProfScope prof(ctx, "threshold_zero_diag");
    hipLaunchKernelGGL(threshold_zero_diag_kernel, dim3(skr_grid(ctx, r->rows * r->cols)), dim3(256), 0, ctx->stream,
                       (float*)r->data, r->rows, r->cols, cutoff, diag_col0);
    SKR_HIP(hipGetLastError());
    return SKR_OK;
}

extern "C" int skr_triu_flatten(skr_ctx* ctx, const skr_mat* r, int64_t k, skr_mat* out) {
    SKR_REQUIRE(ctx && r && out && r->ctx == ctx && out->ctx == ctx, "NULL argument or foreign ctx");
    SKR_REQUIRE((r->dtype == SKR_F32 || r->dtype == SKR_F64) && out->dtype == r->dtype,
                "float32 or float64, out of the same dtype as r");
    SKR_REQUIRE(r->rows == r->cols, "triu needs a square matrix");
    SKR_REQUIRE(k >= 0, "k must be >= 0");
    const int64_t n = r->rows, m = std::max<int64_t>(0, n - k);
    SKR_REQUIRE(out->rows * out->cols == m * (m + 1) / 2, "out must hold %lld values", (long long)(m * (m + 1) / 2));
    SKR_TRY(skr_activate(ctx));
    if (m == 0) return SKR_OK;
    SkrProfScope prof(ctx, "triu_flatten");
    const dim3 grid((unsigned)std::min<int64_t>(n, (int64_t)ctx->num_cu * 16));
    if (r->dtype == SKR_F64)
        hipLaunchKernelGGL(triu_flatten_kernel<double>, grid, dim3(256), 0, ctx->stream, (const double*)r->data, n, k,
                           (double*)out->data);
    else
        hipLaunchKernelGGL(triu_flatten_kernel<float>, grid, dim3(256), 0, ctx->stream, (const float*)r->data, n, k,
                           (float*)out->data);
    SKR_HIP(hipGetLastError());
    return SKR_OK;
}

extern "C" int skr_gather_f32(skr_ctx* ctx, const skr_mat* src, const int64_t* idx_host, int64_t n, float* out_host) {
    SKR_REQUIRE(ctx && src && src->ctx == ctx && src->dtype == SKR_F32, "need a float32 matrix of this ctx");
    SKR_REQUIRE(n >= 0 && (n == 0 || (idx_host && out_host)), "NULL argument");
    SKR_TRY(skr_activate(ctx));
    if (n == 0) return SKR_OK;
    const int64_t limit = src->rows * src->cols;
    for (int64_t i = 0; i < n; i++)
        SKR_REQUIRE(idx_host[i] >= 0 && idx_host[i] < limit, "index %lld out of range", (long long)idx_host[i]);
    void* ws = nullptr;
    SKR_TRY(skr_ctx_workspace(ctx, (size_t)n * 12 + 64, &ws));
    int64_t* d_idx = (int64_t*)ws;
    float* d_out = (float*)((char*)ws + (size_t)n * 8);
    SKR_HIP(hipMemcpyAsync(d_idx, idx_host, (size_t)n * 8, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(gather_kernel, dim3(skr_grid(ctx, n)), dim3(256), 0, ctx->stream, (const float*)src->data, d_idx, n,
                       d_out);
    SKR_HIP(hipGetLastError());
    SKR_HIP(hipMemcpyAsync(out_host, d_out, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
    SKR_HIP(hipStreamSynchronize(ctx->stream));
    return SKR_OK;
}

extern "C" int skr_empirical_pvalues(skr_ctx* ctx, const skr_mat* r, const skr_mat* sorted_bg, int64_t total_len,
                                     skr_mat* p) {
    SKR_REQUIRE(ctx && r && sorted_bg && p, "NULL argument");
    SKR_REQUIRE(r->ctx == ctx && sorted_bg->ctx == ctx && p->ctx == ctx, "foreign ctx");
    SKR_REQUIRE(r->dtype == SKR_F32 && sorted_bg->dtype == SKR_F32 && p->dtype == SKR_F32, "float32 only");
    SKR_REQUIRE(p->rows == r->rows && p->cols == r->cols, "p must have r's shape");
    SKR_REQUIRE(total_len > 0, "total_len must be positive");
    SKR_TRY(skr_activate(ctx));
    const int64_t cells = r->rows * r->cols;
    if (cells == 0) return SKR_OK;
    SkrProfScope prof(ctx, "empirical_pvalues");
    hipLaunchKernelGGL(empirical_p_kernel, dim3(skr_grid(ctx, cells)), dim3(256), 0, ctx->stream, (const float*)r->data,
                       cells, (const float*)sorted_bg->data, sorted_bg->rows * sorted_bg->cols, (double)total_len,
                       (float*)p->data);
    SKR_HIP(hipGetLastError());
    return SKR_OK;
}

extern "C" int skr_edges(skr_ctx* ctx, const skr_mat* r, int64_t nrows, int64_t col_begin, int64_t col_end,
                         int64_t row_global0, int64_t col_global0, float cutoff, int upper_only, skr_mat* out_rows,
                         skr_mat* out_cols, skr_mat* out_vals, int64_t* count) {
    EdgeArgs a{{}, cutoff, upper_only != 0};
    SKR_TRY(skr_block(ctx, r, nrows, col_begin, col_end, row_global0, col_global0, SKR_FIT_BOTH, &a.b));
    SKR_REQUIRE(count, "count must not be NULL");
    skr_mat* const outs[3] = {out_rows, out_cols, out_vals};
    const int dtypes[3] = {SKR_U32, SKR_U32, SKR_F32};
    bool fill = false;
    int64_t cap = 0;
    SKR_TRY(skr_list_outputs(ctx, outs, dtypes, 3, "outputs are U32, U32, F32", &fill, &cap));
    SKR_TRY(skr_activate(ctx));
    *count = 0;
    if (nrows == 0 || col_begin == col_end) return SKR_OK;
    SkrCountScan<unsigned long long> cs;  // one count per row
    SKR_TRY(cs.begin(ctx, nrows));
    const unsigned grid = (unsigned)std::min<int64_t>(nrows, (int64_t)ctx->num_cu * 16);
    {
        SkrProfScope prof(ctx, "edges_count");
        hipLaunchKernelGGL(edges_count_kernel, dim3(grid), dim3(256), 0, ctx->stream, a, cs.counts);
        SKR_HIP(hipGetLastError());
    }
    SKR_TRY(cs.finish(ctx, count));
    if (!fill || *count == 0) return SKR_OK;
    SKR_REQUIRE(*count <= cap, "%lld edges do not fit outputs of %lld cells", (long long)*count, (long long)cap);
    SkrProfScope prof(ctx, "edges_fill");
    hipLaunchKernelGGL(edges_fill_kernel, dim3(grid), dim3(256), 0, ctx->stream, a, cs.counts, (uint32_t*)out_rows->data,
                       (uint32_t*)out_cols->data, (float*)out_vals->data);
    SKR_HIP(hipGetLastError());
    return SKR_OK;
}

extern "C" int skr_select_le(skr_ctx* ctx, const skr_mat* values, double bound, skr_mat* out_index, int64_t* count) {
    SKR_REQUIRE(ctx && values && count && values->ctx == ctx, "need a vector of this ctx and a count");
    SKR_REQUIRE(values->dtype == SKR_F32 || values->dtype == SKR_F64, "float32 or float64 values");
    SKR_REQUIRE(!out_index || (out_index->ctx == ctx && out_index->dtype == SKR_U32), "out_index is a U32 vector of this ctx");
    const int64_t n = values->rows * values->cols;
    SKR_REQUIRE(n <= 0xffffffffLL, "positions must fit 32 bits");
    SKR_TRY(skr_activate(ctx));
    *count = 0;
    if (n == 0) return SKR_OK;
    const int64_t tiles = (n + kSelectTile - 1) / kSelectTile;
    SkrCountScan<unsigned long long> cs;  // one count per tile
    SKR_TRY(cs.begin(ctx, tiles));
    unsigned long long* counts = cs.counts;
    const dim3 grid((unsigned)std::min<int64_t>(tiles, (int64_t)ctx->num_cu * 16));
    const bool f64 = values->dtype == SKR_F64;
    {
        SkrProfScope prof(ctx, "select_count");
        if (f64)
            hipLaunchKernelGGL(select_count_kernel<double>, grid, dim3(kSelectTile), 0, ctx->stream, (const double*)values->data, n,
                               bound, tiles, counts);
        else
            hipLaunchKernelGGL(select_count_kernel<float>, grid, dim3(kSelectTile), 0, ctx->stream, (const float*)values->data, n,
                               bound, tiles, counts);
        SKR_HIP(hipGetLastError());
    }
    SKR_TRY(cs.finish(ctx, count));
    if (!out_index || *count == 0) return SKR_OK;
    const int64_t cap = out_index->rows * out_index->cols;
    SKR_REQUIRE(*count <= cap, "%lld positions do not fit an output of %lld cells", (long long)*count, (long long)cap);
    SkrProfScope prof(ctx, "select_fill");
    if (f64)
        hipLaunchKernelGGL(select_fill_kernel<double>, grid, dim3(kSelectTile), 0, ctx->stream, (const double*)values->data, n, bound,
                           tiles, counts, (uint32_t*)out_index->data);
    else
        hipLaunchKernelGGL(select_fill_kernel<float>, grid, dim3(kSelectTile), 0, ctx->stream, (const float*)values->data, n, bound,
                           tiles, counts, (uint32_t*)out_index->data);
    SKR_HIP(hipGetLastError());
    return SKR_OK;
}

extern "C" int skr_gather_index(skr_ctx* ctx, const skr_mat* src, const skr_mat* index, int64_t count, skr_mat* out) {
    SKR_REQUIRE(ctx && src && index && out, "NULL argument");
    SKR_REQUIRE(src->ctx == ctx && index->ctx == ctx && out->ctx == ctx, "foreign ctx");
    SKR_REQUIRE(index->dtype == SKR_U32 && out->dtype == src->dtype, "index is U32, out has src's dtype");
    SKR_REQUIRE(count >= 0 && count <= index->rows * index->cols && count <= out->rows * out->cols,
                "count exceeds the index list or the output");
    SKR_REQUIRE(out->data != src->data || count == 0, "out must not alias src");
    SKR_TRY(skr_activate(ctx));
    if (count == 0) return SKR_OK;
    SkrDeviceFlag<int> bad;
    SKR_TRY(bad.arm(ctx));
    const int64_t n_src = src->rows * src->cols;
    {
        SkrProfScope prof(ctx, "gather_index");
        if (src->elem() == 8)
            hipLaunchKernelGGL(gather_index_kernel<unsigned long long>, dim3(skr_grid(ctx, count)), dim3(256), 0, ctx->stream,
                               (const unsigned long long*)src->data, n_src, (const uint32_t*)index->data, count,
                               (unsigned long long*)out->data, bad.d);
        else
            hipLaunchKernelGGL(gather_index_kernel<uint32_t>, dim3(skr_grid(ctx, count)), dim3(256), 0, ctx->stream,
                               (const uint32_t*)src->data, n_src, (const uint32_t*)index->data, count, (uint32_t*)out->data, bad.d);
        SKR_HIP(hipGetLastError());
    }
    int h_bad = 0;
    SKR_TRY(bad.read(ctx, &h_bad));
    SKR_REQUIRE(!h_bad, "an index lies outside the %lld cells of src", (long long)n_src);
    return SKR_OK;
}

extern "C" int skr_topk_rows(skr_ctx* ctx, const skr_mat* r, int64_t nrows, int64_t col_begin, int64_t col_end,
                             int64_t row_global0, int64_t col_global0, int k, skr_mat* out_idx, skr_mat* out_val) {
    SkrBlock b;  // only columns are written; 0xFFFFFFFF is the index of an unfilled slot
    SKR_TRY(skr_block(ctx, r, nrows, col_begin, col_end, row_global0, col_global0, SKR_FIT_COLS, &b));
    SKR_REQUIRE(out_idx && out_val, "NULL argument");
    SKR_REQUIRE(out_idx->ctx == ctx && out_val->ctx == ctx, "foreign ctx");
    SKR_REQUIRE(out_idx->dtype == SKR_U32 && out_val->dtype == SKR_F32, "out_idx U32, out_val F32");
    SKR_REQUIRE(k >= 1 && k <= 4096, "k must be in 1..4096");
    SKR_REQUIRE(out_idx->rows * out_idx->cols >= nrows * k && out_val->rows * out_val->cols >= nrows * k,
                "outputs must hold %lld cells", (long long)(nrows * k));
    SKR_TRY(skr_activate(ctx));
    if (nrows == 0) return SKR_OK;
    SkrProfScope prof(ctx, "topk_rows");
    hipLaunchKernelGGL(topk_rows_kernel, dim3((unsigned)std::min<int64_t>(nrows, (int64_t)ctx->num_cu * 16)), dim3(256), 0,
                       ctx->stream, b.r, b.ld, b.rows, b.col_begin, b.col_end, b.row_global0, b.col_global0, k,
                       (uint32_t*)out_idx->data, (float*)out_val->data);
    SKR_HIP(hipGetLastError());
    return SKR_OK;
}

extern "C" int skr_parametric_pvalues(skr_ctx* ctx, const skr_mat* r, const char* dist_name, const double* params, int n_params,
                                      skr_mat* p) {
    SKR_REQUIRE(ctx && r && dist_name && p, "NULL argument");
    SKR_REQUIRE(r->ctx == ctx && p->ctx == ctx, "foreign ctx");
    SKR_REQUIRE(r->dtype == SKR_F32 && p->dtype == SKR_F32, "float32 only");
    SKR_REQUIRE(p->rows == r->rows && p->cols == r->cols, "p must have r's shape");
    static const struct { const char* name; int code; int shapes; } kDists[] = {
        {"cauchy", DIST_CAUCHY, 0}, {"chi2", DIST_CHI2, 1}, {"expon", DIST_EXPON, 0}, {"exponpow", DIST_EXPONPOW, 1},
        {"gamma", DIST_GAMMA, 1}, {"lognorm", DIST_LOGNORM, 1}, {"norm", DIST_NORM, 0}, {"pareto", DIST_PARETO, 1},
        {"rayleigh", DIST_RAYLEIGH, 0}, {"uniform", DIST_UNIFORM, 0}};
    DistParams d{-1, 0.0, 0.0, 1.0, 0, nullptr};
    for (const auto& k : kDists) {
        if (strcmp(k.name, dist_name) != 0) continue;
        // scipy: dist(*shapes, loc=0, scale=1); find_dist's fit returns all of them
        SKR_REQUIRE(n_params >= k.shapes && n_params <= k.shapes + 2 && (n_params == 0 || params),
                    "%s takes %d shape parameter(s) plus loc and scale, got %d values", dist_name, k.shapes, n_params);
        d.dist = k.code;
        if (k.shapes) d.shape = params[0];
        if (n_params > k.shapes) d.loc = params[k.shapes];
        if (n_params > k.shapes + 1) d.scale = params[k.shapes + 1];
    }
    if (d.dist < 0)
        return skr_set_error(SKR_ERR_UNSUPPORTED,
                             "distribution '%s' has no device cdf (available: cauchy, chi2, expon, exponpow, gamma, lognorm, "
                             "norm, pareto, rayleigh, uniform — find_dist's common10 list)", dist_name);
    SKR_REQUIRE(d.scale > 0.0, "scale must be positive");
    const bool has_shape = d.dist == DIST_CHI2 || d.dist == DIST_EXPONPOW || d.dist == DIST_GAMMA || d.dist == DIST_LOGNORM ||
                           d.dist == DIST_PARETO;
    const bool is_gamma = d.dist == DIST_CHI2 || d.dist == DIST_GAMMA;
    if (has_shape && !(d.shape > 0.0)) {
        d.dist = DIST_BAD_SHAPE;  // zero, negative or NaN: scipy's _argcheck fails and every cell is NaN
    } else if (is_gamma) {
        const double a = d.dist == DIST_CHI2 ? 0.5 * d.shape : d.shape;
        if (!(a >= kGammaMinShape && a <= kGammaMaxShape))
            return skr_set_error(SKR_ERR_UNSUPPORTED,
                                 "%s with shape %g: the device's incomplete gamma function covers gamma shapes (chi2: df / 2) "
                                 "from %g to %g", dist_name, d.shape, kGammaMinShape, kGammaMaxShape);
        d.max_terms = gamma_max_terms(a);
    }
    SKR_TRY(skr_activate(ctx));
    const int64_t cells = r->rows * r->cols;
    if (cells == 0) return SKR_OK;
    SkrDeviceFlag<int> not_converged;  // only gamma_p's loops can raise it
    SKR_TRY(not_converged.arm(ctx, d.dist == DIST_CHI2 || d.dist == DIST_GAMMA));  // (not a DIST_BAD_SHAPE)
    d.not_converged = not_converged.d;
    {
        SkrProfScope prof(ctx, "parametric_pvalues");
        hipLaunchKernelGGL(parametric_p_kernel, dim3(skr_grid(ctx, cells)), dim3(256), 0, ctx->stream, (const float*)r->data,
                           cells, d, (float*)p->data);
        SKR_HIP(hipGetLastError());
    }
    int h_flag = 0;
    SKR_TRY(not_converged.read(ctx, &h_flag));
    if (h_flag)
        return skr_set_error(SKR_ERR_UNSUPPORTED,
                             "%s with shape %g: the incomplete gamma function did not converge within %d terms for some "
                             "cell; p holds no valid result", dist_name, d.shape, d.max_terms);
    return SKR_OK;
}
