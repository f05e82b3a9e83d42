// Multiple-testing correction of a p-value matrix (adj_pval.py:53-138, statsmodels 0.12.2 multipletests): the symmetry
// test, the sort of the tests, the per-method pass and the write-back into the output layout, all on the device.
//
//   symmetric_kernel   is_symmetric's value test: each tile against its mirror tile (staged in LDS), diagonal skipped
//   key_bits_kernel    AND / OR of the tests' order-preserving keys: a radix pass whose digit is the same in every key
//                      (one bucket) is skipped
//   KeyPass            the key policy of radix.hpp's LSD radix sort: keys only, NaN last, -0.0 sorted as +0.0
//   scan_*             the method's values in sorted order fused into a running max (or a running min from the end):
//                      block aggregate -> scan of the block aggregates -> block fix-up; NaN wins as in numpy
//   mapback_kernel     each test cell finds its value's first sorted position (two-level lower-bound search) and writes
//                      the corrected value into the final layout
//   elementwise_kernel bonferroni / sidak: no sort, one pass
//   hommel_*           the O(n^2) definition in parallel (n <= 2^22)
// skr_adjust_pvalues_head runs the same passes over the E smallest of ntests tests: Raw::ntests is the number of tests in
// the formulas, Raw::n the entries that exist (seven methods: the values <= alpha need no more, DESIGN_PARITY.md)
//
// Every expression rounds as numpy evaluates the statsmodels source (this file is compiled with -ffp-contract=off); the
// one deliberate difference is sidak's float32 power, which is evaluated in float64 and rounded once (numpy's float32
// power is not correctly rounded).
#include <algorithm>
#include <cmath>

#include "common.hpp"
#include "radix.hpp"

namespace {

using skr_radix::kDigits;

constexpr int64_t kHommelLimit = (int64_t)1 << 22;

// ---- order-preserving keys: float32 -> uint32, float64 -> uint64.  NaN (any payload) -> all ones (last), -0 -> +0.
template <typename T> struct KeyOf;
template <> struct KeyOf<float> { using K = uint32_t; };
template <> struct KeyOf<double> { using K = unsigned long long; };

template <typename K>
__device__ __forceinline__ K key_of_bits(K u) {
    constexpr K sign = (K)1 << (8 * sizeof(K) - 1);
    constexpr K inf = sizeof(K) == 4 ? (K)0x7f800000u : (K)0x7ff0000000000000ull;
    const K mag = u & ~sign;
    if (mag > inf) return ~(K)0;
    if (mag == 0) return sign;
    return (u & sign) ? ~u : (u | sign);
}

template <typename T>
__device__ __forceinline__ T value_of_key(typename KeyOf<T>::K k) {
    using K = typename KeyOf<T>::K;
    constexpr K sign = (K)1 << (8 * sizeof(K) - 1);
    const K u = (k & sign) ? (k ^ sign) : ~k;
    return __builtin_bit_cast(T, u);
}

template <typename T>
__device__ __forceinline__ T round5(T x) {
    const T f = (T)1e5;
    return rint(x * f) / f;
}

// ---------------------------------------------------------------------------------------------- symmetry test --
// Tile (bi, bj) with bj >= bi against the transpose of tile (bj, bi): both read row-wise (coalesced), the mirror one
// through LDS.  flag starts at 1; any mismatch stores 0.
template <typename T>
__global__ __launch_bounds__(256) void symmetric_kernel(const T* __restrict__ p, int64_t n, int* __restrict__ flag) {
    __shared__ T tile[32][33];
    const int64_t bi = blockIdx.y, bj = blockIdx.x;
    if (bj < bi) return;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int r = ty; r < 32; r += 8) {  // tile[c][r] = p[bj*32 + r][bi*32 + c]
        const int64_t row = bj * 32 + r, col = bi * 32 + tx;
        if (row < n && col < n) tile[tx][r] = p[row * n + col];
    }
    __syncthreads();
    bool ok = true;
    for (int r = ty; r < 32; r += 8) {
        const int64_t row = bi * 32 + r, col = bj * 32 + tx;
        if (row < n && col < n && row != col) {
            const T a = round5(p[row * n + col]), b = round5(tile[r][tx]);  // tile[r][tx] = p[col][row]
            ok = ok && (a == b || (a != a && b != b));
        }
    }
    if (!ok) *flag = 0;
}

// ------------------------------------------------------------------------------------------------ radix sort --
// AND and OR of every key: the bits that are the same in all keys
template <typename K, bool RAW>
__global__ __launch_bounds__(256) void key_bits_kernel(const K* __restrict__ in, int64_t n, K* __restrict__ and_or) {
    K a = ~(K)0, o = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const K k = RAW ? key_of_bits<K>(in[i]) : in[i];
        a &= k;
        o |= k;
    }
    for (int off = 32; off; off >>= 1) {
        a &= __shfl_xor(a, off, 64);
        o |= __shfl_xor(o, off, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        atomicAnd(&and_or[0], a);
        atomicOr(&and_or[1], o);
    }
}

// the sort's policy (radix.hpp): keys only; the first pass (RAW) reads the float bits and turns them into keys
template <typename K, bool RAW>
struct KeyPass {
    using Count = unsigned long long;  // up to 2.5e9 tests
    using Item = K;
    const K* in;
    K* out;
    int shift;
    __device__ __forceinline__ K load(int64_t i) const { return RAW ? key_of_bits<K>(in[i]) : in[i]; }
    __device__ __forceinline__ uint32_t digit(K k) const { return (uint32_t)(k >> shift) & (kDigits - 1); }
    __device__ __forceinline__ void store(unsigned long long pos, K k) const { out[pos] = k; }
};

// ------------------------------------------------------------------------------------- per-method values + scan --
struct Raw {
    const void* keys;    // sorted keys (K of the dtype)
    const double* src;   // instead: a float64 array (the second scan of fdr_gbs, hommel's suffix max)
    int64_t n;           // entries of keys / src: the sorted positions that exist
    int64_t ntests;      // the number of tests the formulas speak of (n, or more: skr_adjust_pvalues_head)
    int method;
    double cm;           // fdr_by's sum of 1/k
};

// the method's value at sorted position i, before its running max / min (multitest.py, evaluated as numpy does)
template <typename T>
__device__ __forceinline__ double raw_at(const Raw& r, int64_t i) {
    if (r.src) return r.src[i];
    const T s = value_of_key<T>(((const typename KeyOf<T>::K*)r.keys)[i]);
    const double n = (double)r.ntests, ds = (double)s;
    switch (r.method) {
        case SKR_ADJ_HOLM_SIDAK: return 1.0 - pow((double)((T)1 - s), (double)(r.ntests - i));
        case SKR_ADJ_HOLM: return ds * (double)(r.ntests - i);
        case SKR_ADJ_SIMES_HOCHBERG: return (double)(r.ntests - i) * ds;
        case SKR_ADJ_FDR_BY: return ds / (((double)(i + 1) / n) / r.cm);
        case SKR_ADJ_FDR_GBS: return (n + 1.0 - (double)(i + 1)) / (double)(i + 1) * ds / (double)((T)1 - s);
        default: return ds / ((double)(i + 1) / n);  // fdr_bh and the two-stage methods
    }
}

// numpy's maximum / minimum: NaN wins
__device__ __forceinline__ double op_nan(double a, double b, bool is_max) {
    if (a != a || b != b) return NAN;
    return is_max ? (a > b ? a : b) : (a < b ? a : b);
}

constexpr int kAccBlock = 256, kAccPer = 16, kAccTile = kAccBlock * kAccPer;

struct Acc {
    Raw raw;
    double* out;
    double* totals;  // per block: aggregate, then (scanned) the carry from the blocks before it
    bool is_max;     // running max or running min
    bool backward;   // ... from the end
};

// logical position j (scan order) -> sorted position
__device__ __forceinline__ int64_t phys(const Acc& a, int64_t j) { return a.backward ? a.raw.n - 1 - j : j; }

__device__ __forceinline__ double block_reduce_op(double v, double* lds, bool is_max) {
    for (int off = 32; off; off >>= 1) v = op_nan(v, __shfl_xor(v, off, 64), is_max);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    double all = lds[0];
    for (int w = 1; w < kAccBlock / 64; w++) all = op_nan(all, lds[w], is_max);
    __syncthreads();
    return all;
}

template <typename T>
__global__ __launch_bounds__(kAccBlock) void scan_aggregate_kernel(const Acc a) {
    __shared__ double lds[kAccBlock / 64];
    const double ident = a.is_max ? -INFINITY : INFINITY;
    const int64_t j0 = (int64_t)blockIdx.x * kAccTile + (int64_t)threadIdx.x * kAccPer;
    double v = ident;
    for (int t = 0; t < kAccPer; t++)
        if (j0 + t < a.raw.n) v = op_nan(v, raw_at<T>(a.raw, phys(a, j0 + t)), a.is_max);
    v = block_reduce_op(v, lds, a.is_max);
    if (threadIdx.x == 0) a.totals[blockIdx.x] = v;
}

// one block: totals[b] <- op of totals[0..b-1] (identity for b = 0)
__global__ __launch_bounds__(1024) void scan_totals_kernel(double* __restrict__ totals, int64_t nb, bool is_max) {
    __shared__ double lds[1024];
    const double ident = is_max ? -INFINITY : INFINITY;
    const int64_t per = (nb + 1023) / 1024, b0 = (int64_t)threadIdx.x * per, b1 = std::min(nb, b0 + per);
    double v = ident;
    for (int64_t b = b0; b < b1; b++) v = op_nan(v, totals[b], is_max);
    lds[threadIdx.x] = v;
    __syncthreads();
    double run = ident;  // exclusive over the threads before this one
    for (int t = 0; t < (int)threadIdx.x; t++) run = op_nan(run, lds[t], is_max);
    for (int64_t b = b0; b < b1; b++) {
        const double x = totals[b];
        totals[b] = run;
        run = op_nan(run, x, is_max);
    }
}

template <typename T>
__global__ __launch_bounds__(kAccBlock) void scan_apply_kernel(const Acc a) {
    __shared__ double lds[kAccBlock];
    const double ident = a.is_max ? -INFINITY : INFINITY;
    const int64_t j0 = (int64_t)blockIdx.x * kAccTile + (int64_t)threadIdx.x * kAccPer;
    double v[kAccPer];
    double mine = ident;
    for (int t = 0; t < kAccPer; t++) {
        v[t] = j0 + t < a.raw.n ? raw_at<T>(a.raw, phys(a, j0 + t)) : ident;
        mine = op_nan(mine, v[t], a.is_max);
    }
    lds[threadIdx.x] = mine;
    __syncthreads();
    double run = a.totals[blockIdx.x];
    for (int t = 0; t < (int)threadIdx.x; t++) run = op_nan(run, lds[t], a.is_max);
    for (int t = 0; t < kAccPer; t++) {
        run = op_nan(run, v[t], a.is_max);
        if (j0 + t < a.raw.n) a.out[phys(a, j0 + t)] = run;
    }
}

// two-stage r1: 1 + the largest i with s_i <= ((i+1)/n) * alpha' (0 when none)
template <typename T>
__global__ __launch_bounds__(256) void rejections_kernel(const typename KeyOf<T>::K* __restrict__ keys, int64_t n,
                                                         double alpha_prime, unsigned long long* __restrict__ r1) {
    unsigned long long best = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const double s = (double)value_of_key<T>(keys[i]);
        if (s <= ((double)(i + 1) / (double)n) * alpha_prime) best = (unsigned long long)(i + 1);
    }
    for (int off = 32; off; off >>= 1) {
        const unsigned long long o = __shfl_xor(best, off, 64);
        best = o > best ? o : best;
    }
    if ((threadIdx.x & 63) == 0 && best) atomicMax(r1, best);
}

// fdr_by's cm = np.sum(1./np.arange(1, n+1)): numpy adds the array in buffers of 8 192 values, each by its pairwise
// summation (blocks of <= 128 summed with eight accumulators, longer ones split in halves rounded down to a multiple of
// 8), and the buffer sums one after the other.  One thread per buffer here; the host adds the buffer sums in order.
__device__ double harmonic_leaf(int64_t first, int64_t n) {  // values 1 / (first + i + 1)
    if (n < 8) {
        double res = 0.;
        for (int64_t i = 0; i < n; i++) res += 1.0 / (double)(first + i + 1);
        return res;
    }
    double r[8];
    for (int j = 0; j < 8; j++) r[j] = 1.0 / (double)(first + j + 1);
    int64_t i = 8;
    for (; i < n - (n % 8); i += 8)
        for (int j = 0; j < 8; j++) r[j] += 1.0 / (double)(first + i + j + 1);
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; i++) res += 1.0 / (double)(first + i + 1);
    return res;
}

__global__ __launch_bounds__(64) void harmonic_buffers_kernel(int64_t n, double* __restrict__ sums) {
    const int64_t b = (int64_t)blockIdx.x * 64 + threadIdx.x, nb = (n + 8191) / 8192;
    if (b >= nb) return;
    // the pairwise tree of one buffer, walked with an explicit stack (post-order)
    struct Node { int64_t first, n; double left; int state; };
    Node st[16];
    int sp = 0;
    st[0] = {b * 8192, std::min<int64_t>(8192, n - b * 8192), 0., 0};
    double ret = 0.;
    for (;;) {
        Node& f = st[sp];
        if (f.state == 0 && f.n > 128) {
            const int64_t n2 = f.n / 2 - (f.n / 2) % 8;
            f.state = 1;
            st[++sp] = {f.first, n2, 0., 0};
            continue;
        }
        if (f.state == 0) {
            ret = harmonic_leaf(f.first, f.n);
        } else if (f.state == 1) {
            const int64_t n2 = f.n / 2 - (f.n / 2) % 8;
            f.left = ret;
            f.state = 2;
            st[++sp] = {f.first + n2, f.n - n2, 0., 0};
            continue;
        } else {
            ret = f.left + ret;
        }
        if (sp == 0) break;
        --sp;
    }
    sums[b] = ret;
}

// ------------------------------------------------------------------------------------------------- write-back --
struct Fin {
    int two_stage;  // 0: clip; 1: clip(clip(c) * m1); 2: clip(clip(c) * m1 * m2)
    double m1, m2;
};

__device__ __forceinline__ double clip1(double v) { return v > 1.0 ? 1.0 : v; }

__device__ __forceinline__ double finish(double c, const Fin& f) {
    if (f.two_stage == 0) return clip1(c);
    double v = clip1(c) * f.m1;
    if (f.two_stage == 2) v = v * f.m2;
    return clip1(v);
}

constexpr int kSplit = 4096;

// first position of sorted (ascending, n entries) whose key is >= k; tab[u] = sorted[u * stride], u < n_tab
template <typename K>
__device__ __forceinline__ int64_t lower_bound2(const K* __restrict__ sorted, int64_t n, const K* tab, int64_t n_tab,
                                                int64_t stride, K k) {
    int64_t lo = 0, hi = n_tab;  // u* = number of table entries < k
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (tab[mid] < k) lo = mid + 1; else hi = mid;
    }
    if (lo == 0) return 0;
    int64_t a = (lo - 1) * stride + 1, b = std::min(n, lo * stride);
    while (a < b) {
        const int64_t mid = (a + b) >> 1;
        if (sorted[mid] < k) a = mid + 1; else b = mid;
    }
    return a;
}

// out = the corrected value of each test cell: upper -> [N, N] float64, NaN outside the strict upper triangle;
// otherwise [rows, cols] of OutT (float64, or the input dtype for hommel)
template <typename T, typename OutT, bool UPPER>
__global__ __launch_bounds__(256) void mapback_kernel(const T* __restrict__ p, int64_t cols, int64_t cells,
                                                      const typename KeyOf<T>::K* __restrict__ sorted, int64_t n,
                                                      const double* __restrict__ c, const Fin f, OutT* __restrict__ out) {
    using K = typename KeyOf<T>::K;
    __shared__ K tab[kSplit];
    const int64_t stride = (n + kSplit - 1) / kSplit, n_tab = (n + stride - 1) / stride;
    for (int64_t u = threadIdx.x; u < n_tab; u += 256) tab[u] = sorted[u * stride];
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < cells; i += (int64_t)gridDim.x * 256) {
        if (UPPER && i % cols <= i / cols) {
            out[i] = (OutT)NAN;
            continue;
        }
        const K k = key_of_bits<K>(__builtin_bit_cast(K, p[i]));
        const int64_t at = std::min<int64_t>(n - 1, lower_bound2<K>(sorted, n, tab, n_tab, stride, k));  // always found
        out[i] = (OutT)finish(c[at], f);
    }
}

// bonferroni: s * float(n) in the dtype; sidak: 1 - (1 - s) ** n in the dtype, the power evaluated in float64 and
// rounded once (numpy's float32 power is not correctly rounded).  Then c[c > 1] = 1.
template <typename T, typename OutT, bool UPPER>
__global__ __launch_bounds__(256) void elementwise_kernel(const T* __restrict__ p, int64_t cols, int64_t cells, int64_t n,
                                                          int sidak, OutT* __restrict__ out) {
    const T fn = (T)(double)n;  // float(ntests), then the dtype's rounding, as numpy casts the Python scalar
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < cells; i += (int64_t)gridDim.x * 256) {
        if (UPPER && i % cols <= i / cols) {
            out[i] = (OutT)NAN;
            continue;
        }
        const T s = p[i];
        T v;
        if (sidak) v = (T)1 - (T)pow((double)((T)1 - s), (double)fn);
        else v = s * fn;
        if (v > (T)1) v = (T)1;
        out[i] = (OutT)v;
    }
}

// ------------------------------------------------------------------------------------------------------ hommel --
// cim_m = min over k = 1..m of (m * s[n-m+k-1])_D / k in float64 (np.min: NaN wins), stored rounded to the dtype —
// every use of cim in the source is a maximum / minimum with dtype values, where rounding first gives the same result.
template <typename T>
__global__ __launch_bounds__(256) void hommel_cim_kernel(const typename KeyOf<T>::K* __restrict__ keys, int64_t n,
                                                         double* __restrict__ cim) {
    __shared__ double lds[4];
    for (int64_t m = (int64_t)blockIdx.x + 2; m <= n; m += gridDim.x) {
        const T fm = (T)m;
        double v = INFINITY;
        for (int64_t k = threadIdx.x + 1; k <= m; k += 256) {
            const T x = fm * value_of_key<T>(keys[n - m + k - 1]);
            v = op_nan(v, (double)x / (double)k, false);
        }
        v = block_reduce_op(v, lds, false);
        if (threadIdx.x == 0) cim[m] = (double)(T)v;
    }
}

// a_i = max(s_i, max over m >= n-i of cim_m, max over m < n-i of min((m * s_i)_D, cim_m)), m in [2, n];
// suf[m] = max over m' >= m of cim_m'.  256 cells per block share a staged tile of cim.
template <typename T>
__global__ __launch_bounds__(256) void hommel_cells_kernel(const typename KeyOf<T>::K* __restrict__ keys, int64_t n,
                                                           const double* __restrict__ cim, const double* __restrict__ suf,
                                                           double* __restrict__ a_out) {
    __shared__ T tile[256];
    const int64_t i0 = (int64_t)blockIdx.x * 256, i = i0 + threadIdx.x;
    const bool live = i < n;
    const T s = live ? value_of_key<T>(keys[i]) : (T)0;
    const bool any_nan = s != s;
    T a = s;
    if (live) {
        const int64_t m0 = std::max<int64_t>(2, n - i);
        if (m0 <= n) {
            const T x = (T)suf[m0];
            a = (a != a || x != x) ? (T)NAN : (a > x ? a : x);
        }
    }
    const int64_t m_end = n - i0 - 1;  // largest m any cell of this block uses in the second term
    const int64_t my_end = live ? n - i - 1 : 0;
    T best = -(T)INFINITY;
    bool nan_seen = any_nan;
    for (int64_t mb = 2; mb <= m_end; mb += 256) {
        __syncthreads();
        if (mb + threadIdx.x <= m_end) tile[threadIdx.x] = (T)cim[mb + threadIdx.x];
        __syncthreads();
        const int64_t top = std::min<int64_t>(255, my_end - mb);
        for (int t = 0; t <= top; t++) {
            const T cm = tile[t];
            const T x = (T)(mb + t) * s;
            nan_seen = nan_seen || cm != cm;
            const T lo = x < cm ? x : cm;
            best = lo > best ? lo : best;
        }
    }
    if (!live) return;
    if (nan_seen || a != a) a = (T)NAN;
    else if (best > a) a = best;
    a_out[i] = (double)a;
}

// ---------------------------------------------------------------------------------------------------- planning --
struct Plan {
    int64_t n = 0, acc_blocks = 0;
    skr_radix::Chunks sort;
    size_t off_keys_a = 0, off_keys_b = 0, off_c = 0, off_table = 0, off_scan = 0, off_acc = 0, off_hommel = 0,
           off_misc = 0, bytes = 0;
};

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// harmonic_n: the length fdr_by's harmonic sum runs over (the number of tests)
Plan plan_for(const skr_ctx* ctx, int64_t n, size_t key_bytes, bool hommel, int64_t harmonic_n) {
    Plan p;
    p.n = n;
    p.sort = skr_radix::plan_chunks(ctx, n);
    p.acc_blocks = std::max<int64_t>(1, (n + kAccTile - 1) / kAccTile);
    size_t off = 0;
    p.off_misc = off;
    off += 256;
    p.off_keys_a = off;
    off = align256(off + (size_t)n * key_bytes);
    p.off_keys_b = off;
    off = align256(off + (size_t)n * key_bytes);
    p.off_c = off;
    off = align256(off + (size_t)n * 8);
    p.off_table = off;
    off = align256(off + p.sort.table_words * 8);
    p.off_scan = off;
    off = align256(off + (p.sort.scan_words + 16) * 8);
    p.off_acc = off;  // scan aggregates, or fdr_by's buffer sums
    off = align256(off + (size_t)std::max<int64_t>(p.acc_blocks, (harmonic_n + 8191) / 8192 + 1) * 8);
    p.off_hommel = off;
    if (hommel) off = align256(off + (size_t)(n + 1) * 8 * 2);
    p.bytes = off;
    return p;
}

int workspace_for(skr_ctx* ctx, const Plan& plan, void** ws) {
    size_t free_b = 0, total_b = 0;
    SKR_HIP(hipMemGetInfo(&free_b, &total_b));
    const size_t have = free_b + (ctx->ws_bytes);
    if (plan.bytes > have)
        return skr_set_error(SKR_ERR_NOMEM,
                             "p-value correction of %lld tests needs %zu bytes of device workspace; %zu are free",
                             (long long)plan.n, plan.bytes, have);
    return skr_ctx_workspace(ctx, plan.bytes, ws);
}

// LSD sort of the n raw values at `raw` (float bits) into ascending keys; returns where the sorted keys are
template <typename T>
int sort_keys(skr_ctx* ctx, const Plan& plan, char* base, const void* raw, const typename KeyOf<T>::K** sorted) {
    using K = typename KeyOf<T>::K;
    const int64_t n = plan.n;
    K* and_or = (K*)(base + 64);
    const K init[2] = {~(K)0, (K)0};
    SKR_HIP(hipMemcpyAsync(and_or, init, sizeof(init), hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL((key_bits_kernel<K, true>), dim3(skr_grid(ctx, n)), dim3(256), 0, ctx->stream, (const K*)raw, n, and_or);
    SKR_HIP(hipGetLastError());
    K host[2];
    SKR_HIP(hipMemcpyAsync(host, and_or, sizeof(host), hipMemcpyDeviceToHost, ctx->stream));
    SKR_HIP(hipStreamSynchronize(ctx->stream));
    const K varying = host[0] ^ host[1];
    const int passes = (int)sizeof(K);
    int wanted[8], n_wanted = 0;
    for (int pss = 0; pss < passes; pss++)
        if ((varying >> (8 * pss)) & 0xff) wanted[n_wanted++] = pss;
    if (n_wanted == 0) wanted[n_wanted++] = passes - 1;  // one value throughout: one pass still turns it into keys
    K* buf[2] = {(K*)(base + plan.off_keys_a), (K*)(base + plan.off_keys_b)};
    unsigned long long* table = (unsigned long long*)(base + plan.off_table);
    unsigned long long* scan_scratch = (unsigned long long*)(base + plan.off_scan);
    const K* in = (const K*)raw;
    int cur = raw == (const void*)buf[0] ? 1 : 0;  // the output buffer of the first pass
    for (int w = 0; w < n_wanted; w++) {
        K* out = buf[cur];
        if (w == 0)
            SKR_TRY(skr_radix::run_pass(ctx, KeyPass<K, true>{in, out, 8 * wanted[w]}, n, plan.sort, table, scan_scratch));
        else
            SKR_TRY(skr_radix::run_pass(ctx, KeyPass<K, false>{in, out, 8 * wanted[w]}, n, plan.sort, table, scan_scratch));
        in = out;
        cur ^= 1;
    }
    *sorted = in;
    return SKR_OK;
}

// out[] <- the running max / min (from the start or from the end) of the method's values (or of raw.src) in sorted order
template <typename T>
int running(skr_ctx* ctx, const Plan& plan, char* base, const Raw& raw, bool is_max, bool backward, double* out) {
    Acc a;
    a.raw = raw;
    a.out = out;
    a.totals = (double*)(base + plan.off_acc);
    a.is_max = is_max;
    a.backward = backward;
    const int64_t blocks = (raw.n + kAccTile - 1) / kAccTile;
    hipLaunchKernelGGL(scan_aggregate_kernel<T>, dim3((unsigned)blocks), dim3(kAccBlock), 0, ctx->stream, a);
    SKR_HIP(hipGetLastError());
    hipLaunchKernelGGL(scan_totals_kernel, dim3(1), dim3(1024), 0, ctx->stream, a.totals, blocks, is_max);
    SKR_HIP(hipGetLastError());
    hipLaunchKernelGGL(scan_apply_kernel<T>, dim3((unsigned)blocks), dim3(kAccBlock), 0, ctx->stream, a);
    SKR_HIP(hipGetLastError());
    return SKR_OK;
}

// head_ntests > 0 (skr_adjust_pvalues_head): p holds the n smallest of head_ntests tests; every formula takes
// head_ntests as the number of tests, every array has n entries, and out is float64 as for `upper`
template <typename T>
int adjust_typed(skr_ctx* ctx, const skr_mat* p, int method, double alpha, bool upper, skr_mat* out, int64_t head_ntests = 0) {
    using K = typename KeyOf<T>::K;
    const int64_t rows = p->rows, cols = p->cols, cells = rows * cols;
    const int64_t n = upper ? rows * (rows - 1) / 2 : cells;
    const int64_t ntests = head_ntests > 0 ? head_ntests : n;
    if (ntests == 0) return skr_set_error(SKR_ERR_ZERODIV, "float division by zero");  // 1./ntests in multipletests
    if (n == 0) return SKR_OK;  // a head without tests: nothing to write
    const bool keep_dtype = method == SKR_ADJ_BONFERRONI || method == SKR_ADJ_SIDAK || method == SKR_ADJ_HOMMEL;
    const int out_dtype = upper || head_ntests > 0 || !keep_dtype ? SKR_F64 : p->dtype;
    SKR_REQUIRE(out->rows == rows && out->cols == cols && out->dtype == out_dtype,
                "out must be a [%lld, %lld] %s matrix", (long long)rows, (long long)cols,
                out_dtype == SKR_F64 ? "float64" : "float32");
    if (method == SKR_ADJ_HOMMEL && n > kHommelLimit)
        return skr_set_error(SKR_ERR_UNSUPPORTED, "hommel on the device is limited to %lld tests; this matrix has %lld",
                             (long long)kHommelLimit, (long long)n);
    const T* pd = (const T*)p->data;
    if (method == SKR_ADJ_BONFERRONI || method == SKR_ADJ_SIDAK) {
        SkrProfScope prof(ctx, "adjust_elementwise");
        const int sidak = method == SKR_ADJ_SIDAK;
        if (upper)
            hipLaunchKernelGGL((elementwise_kernel<T, double, true>), dim3(skr_grid(ctx, cells)), dim3(256), 0, ctx->stream, pd,
                               cols, cells, ntests, sidak, (double*)out->data);
        else if (out_dtype == SKR_F64)
            hipLaunchKernelGGL((elementwise_kernel<T, double, false>), dim3(skr_grid(ctx, cells)), dim3(256), 0, ctx->stream, pd,
                               cols, cells, ntests, sidak, (double*)out->data);
        else
            hipLaunchKernelGGL((elementwise_kernel<T, T, false>), dim3(skr_grid(ctx, cells)), dim3(256), 0, ctx->stream, pd,
                               cols, cells, ntests, sidak, (T*)out->data);
        SKR_HIP(hipGetLastError());
        return SKR_OK;
    }

    const Plan plan = plan_for(ctx, n, sizeof(K), method == SKR_ADJ_HOMMEL, method == SKR_ADJ_FDR_BY ? ntests : n);
    void* ws = nullptr;
    SKR_TRY(workspace_for(ctx, plan, &ws));
    char* base = (char*)ws;
    const void* raw = pd;
    if (upper) {  // the tests: the strict upper triangle in np.triu_indices order
        SkrProfScope prof(ctx, "adjust_gather");
        skr_mat tests;
        tests.ctx = ctx;
        tests.rows = 1;
        tests.cols = n;
        tests.dtype = p->dtype;
        tests.data = base + plan.off_keys_a;
        tests.owner = false;
        SKR_TRY(skr_triu_flatten(ctx, p, 1, &tests));
        raw = tests.data;
    }
    const K* sorted = nullptr;
    {
        SkrProfScope prof(ctx, "adjust_sort");
        SKR_TRY(sort_keys<T>(ctx, plan, base, raw, &sorted));
    }
    double* c = (double*)(base + plan.off_c);
    Fin fin{0, 1.0, 1.0};
    {
        SkrProfScope prof(ctx, "adjust_scan");
        Raw r{sorted, nullptr, n, ntests, method, 0.0};
        if (method == SKR_ADJ_HOMMEL) {
            double* cim = (double*)(base + plan.off_hommel);
            double* suf = cim + (n + 1);
            if (n >= 2) {
                hipLaunchKernelGGL(hommel_cim_kernel<T>, dim3((unsigned)std::min<int64_t>(n - 1, (int64_t)ctx->num_cu * 64)),
                                   dim3(256), 0, ctx->stream, sorted, n, cim);
                SKR_HIP(hipGetLastError());
                // suf[m] for m in [2, n]: the running max from the end of cim[2..n]
                const Raw rs{nullptr, cim + 2, n - 1, n - 1, method, 0.0};
                SKR_TRY(running<T>(ctx, plan, base, rs, true, true, suf + 2));
            }
            hipLaunchKernelGGL(hommel_cells_kernel<T>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, sorted, n,
                               cim, suf, c);
            SKR_HIP(hipGetLastError());
        } else {
            const bool fwd_max = method == SKR_ADJ_HOLM || method == SKR_ADJ_HOLM_SIDAK || method == SKR_ADJ_FDR_GBS;
            if (method == SKR_ADJ_FDR_BY) {
                double* sums = (double*)(base + plan.off_acc);
                const int64_t nb = (ntests + 8191) / 8192;
                hipLaunchKernelGGL(harmonic_buffers_kernel, dim3((unsigned)((nb + 63) / 64)), dim3(64), 0, ctx->stream, ntests, sums);
                SKR_HIP(hipGetLastError());
                double* host = (double*)malloc((size_t)nb * 8);
                if (!host) return skr_set_error(SKR_ERR_NOMEM, "host buffer of %lld doubles", (long long)nb);
                const hipError_t e1 = hipMemcpyAsync(host, sums, (size_t)nb * 8, hipMemcpyDeviceToHost, ctx->stream);
                const hipError_t e2 = e1 == hipSuccess ? hipStreamSynchronize(ctx->stream) : e1;
                double cm = 0.;
                for (int64_t b = 0; b < nb; b++) cm += host[b];
                free(host);
                SKR_HIP(e2);
                r.cm = cm;
            }
            if (method == SKR_ADJ_FDR_GBS) {  // running max, then a running min from the end of that
                SKR_TRY(running<T>(ctx, plan, base, r, true, false, c));
                const Raw r2{nullptr, c, n, n, method, 0.0};
                SKR_TRY(running<T>(ctx, plan, base, r2, false, true, c));
            } else {
                SKR_TRY(running<T>(ctx, plan, base, r, fwd_max, !fwd_max, c));
            }
            if (method == SKR_ADJ_FDR_TSBH || method == SKR_ADJ_FDR_TSBKY) {
                const bool bky = method == SKR_ADJ_FDR_TSBKY;
                const double fact = bky ? 1. + alpha : 1.;
                const double alpha_prime = bky ? alpha / fact : alpha;
                unsigned long long* r1d = (unsigned long long*)(base + 128);
                SKR_HIP(hipMemsetAsync(r1d, 0, 8, ctx->stream));
                hipLaunchKernelGGL(rejections_kernel<T>, dim3(skr_grid(ctx, n)), dim3(256), 0, ctx->stream, sorted, n, alpha_prime,
                                   r1d);
                SKR_HIP(hipGetLastError());
                unsigned long long r1 = 0;
                SKR_HIP(hipMemcpyAsync(&r1, r1d, 8, hipMemcpyDeviceToHost, ctx->stream));
                SKR_HIP(hipStreamSynchronize(ctx->stream));
                if (r1 == 0 || (int64_t)r1 == n) {
                    fin = Fin{1, fact, 1.0};
                } else {
                    const double ntests0 = 1.0 * (double)n - (double)r1;
                    fin = Fin{bky ? 2 : 1, ntests0 * 1.0 / (double)n, 1. + alpha};
                }
            }
        }
    }
    SkrProfScope prof(ctx, "adjust_mapback");
    const dim3 grid(skr_grid(ctx, cells));
    if (upper)
        hipLaunchKernelGGL((mapback_kernel<T, double, true>), grid, dim3(256), 0, ctx->stream, pd, cols, cells, sorted, n, c, fin,
                           (double*)out->data);
    else if (out_dtype == SKR_F64)
        hipLaunchKernelGGL((mapback_kernel<T, double, false>), grid, dim3(256), 0, ctx->stream, pd, cols, cells, sorted, n, c, fin,
                           (double*)out->data);
    else
        hipLaunchKernelGGL((mapback_kernel<T, T, false>), grid, dim3(256), 0, ctx->stream, pd, cols, cells, sorted, n, c, fin,
                           (T*)out->data);
    SKR_HIP(hipGetLastError());
    return SKR_OK;
}

}  // namespace

extern "C" int skr_pvals_symmetric(skr_ctx* ctx, const skr_mat* p, int* symmetric) {
    SKR_REQUIRE(ctx && p && symmetric && p->ctx == ctx, "NULL argument or foreign ctx");
    SKR_REQUIRE(p->dtype == SKR_F32 || p->dtype == SKR_F64, "float32 or float64 p-values");
    *symmetric = 0;
    if (p->rows != p->cols) return SKR_OK;
    SKR_TRY(skr_activate(ctx));
    const int64_t n = p->rows;
    if (n <= 1) {
        *symmetric = 1;
        return SKR_OK;
    }
    SkrProfScope prof(ctx, "pvals_symmetric");
    void* ws = nullptr;
    SKR_TRY(skr_ctx_workspace(ctx, 256, &ws));
    int* flag = (int*)ws;
    const int one = 1;
    SKR_HIP(hipMemcpyAsync(flag, &one, 4, hipMemcpyHostToDevice, ctx->stream));
    const int64_t tiles = (n + 31) / 32;
    SKR_REQUIRE(tiles <= 65535, "at most %lld rows", (long long)65535 * 32);
    if (p->dtype == SKR_F64)
        hipLaunchKernelGGL(symmetric_kernel<double>, dim3((unsigned)tiles, (unsigned)tiles), dim3(256), 0, ctx->stream,
                           (const double*)p->data, n, flag);
    else
        hipLaunchKernelGGL(symmetric_kernel<float>, dim3((unsigned)tiles, (unsigned)tiles), dim3(256), 0, ctx->stream,
                           (const float*)p->data, n, flag);
    SKR_HIP(hipGetLastError());
    int h = 0;
    SKR_HIP(hipMemcpyAsync(&h, flag, 4, hipMemcpyDeviceToHost, ctx->stream));
    SKR_HIP(hipStreamSynchronize(ctx->stream));
    *symmetric = h;
    return SKR_OK;
}

extern "C" int skr_adjust_pvalues(skr_ctx* ctx, const skr_mat* p, int method, double alpha, int upper_only, skr_mat* out) {
    SKR_REQUIRE(ctx && p && out && p->ctx == ctx && out->ctx == ctx, "NULL argument or foreign ctx");
    SKR_REQUIRE(p->dtype == SKR_F32 || p->dtype == SKR_F64, "float32 or float64 p-values");
    SKR_REQUIRE(method >= SKR_ADJ_BONFERRONI && method <= SKR_ADJ_FDR_GBS, "method not recognized");
    SKR_REQUIRE(!upper_only || p->rows == p->cols, "upper_only needs a square matrix");
    SKR_REQUIRE(out->data != p->data, "out must not alias p");
    SKR_TRY(skr_activate(ctx));
    if (p->dtype == SKR_F64) return adjust_typed<double>(ctx, p, method, alpha, upper_only != 0, out);
    return adjust_typed<float>(ctx, p, method, alpha, upper_only != 0, out);
}

extern "C" int skr_adjust_pvalues_head(skr_ctx* ctx, const skr_mat* p, int64_t ntests, int method, double alpha, skr_mat* out) {
    SKR_REQUIRE(ctx && p && out && p->ctx == ctx && out->ctx == ctx, "NULL argument or foreign ctx");
    SKR_REQUIRE(p->dtype == SKR_F32 || p->dtype == SKR_F64, "float32 or float64 p-values");
    SKR_REQUIRE(method >= SKR_ADJ_BONFERRONI && method <= SKR_ADJ_FDR_GBS, "method not recognized");
    static const char* const kNames[] = {"bonferroni", "sidak", "holm-sidak", "holm", "simes-hochberg", "hommel", "fdr_bh",
                                         "fdr_by", "fdr_tsbh", "fdr_tsbky", "fdr_gbs"};
    if (method == SKR_ADJ_HOMMEL || method == SKR_ADJ_FDR_TSBH || method == SKR_ADJ_FDR_TSBKY || method == SKR_ADJ_FDR_GBS)
        return skr_set_error(SKR_ERR_UNSUPPORTED,
                             "%s cannot be corrected from the smallest p-values alone: its values depend on the tests "
                             "that are left out", kNames[method]);
    const int64_t given = p->rows * p->cols;
    SKR_REQUIRE(ntests >= given, "ntests (%lld) is smaller than the %lld p-values given", (long long)ntests, (long long)given);
    SKR_REQUIRE(out->data != p->data || given == 0, "out must not alias p");
    SKR_TRY(skr_activate(ctx));
    if (ntests == 0) return skr_set_error(SKR_ERR_ZERODIV, "float division by zero");
    if (p->dtype == SKR_F64) return adjust_typed<double>(ctx, p, method, alpha, false, out, ntests);
    return adjust_typed<float>(ctx, p, method, alpha, false, out, ntests);
}
