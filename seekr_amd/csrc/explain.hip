// The k-mers behind a similarity.  r[i, j] is the mean over columns w of z_i[w] * z_j[w]: the terms of that sum say
// which k-mers make two rows similar (skr_pair_kmers), and the column means and standard deviations of the z-scores of
// a set of rows say which k-mers characterise a community (skr_group_colstat).
//
// skr_pair_kmers: one workgroup per pair.  The two rows are read once, multiplied cell by cell (one float32 rounding:
// this file is compiled with -ffp-contract=off) and the products go through topk.hip's selection — a candidate buffer
// filled by wave ballots, sorted together with the running list (bitonic) when the next step might not fit — in
// topk_key's order; there is no product matrix in memory.  The two rows of a pair start at unrelated 16-byte phases
// whenever the width is not a multiple of four, so both are read with 16-byte loads that only claim 4-byte alignment
// (normalize.hip: f4u) from column 0 on, and the last, ragged group cell by cell: no head, one tail.
// A short list (top <= 64) ranks the first 256 cells of a pair on their own, so that the first sort takes 512 entries
// and not 2 048: that sort's LDS traffic, not the rows' bytes, is what a pair costs.
//
// skr_group_colstat: colsum_seq_kernel's organisation (normalize.hip) with the rows taken through an index list: a
// workgroup owns a 16-column strip of ONE group; four staging waves bring tiles of the group's rows into LDS, wave 0
// walks them, one float32 chain per column, in the list's order.  Parity is defined by rounding: a tree would be more
// accurate and different from np.mean / np.std.
#include <cmath>

#include "common.hpp"
#include "topk_key.hpp"

#pragma clang fp contract(off)

namespace {

typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));  // 16 bytes of a row that is only 4-byte aligned

// ---------------------------------------------------------------------------------------------------------------------
// pairs
// ---------------------------------------------------------------------------------------------------------------------
constexpr int kPairKmax = 256;                     // list slots in LDS: skr_topk_merge_limits' kmax
constexpr int kPairStep = 1024;                    // cells per sweep step: 256 threads x 4
constexpr int kPairCap = 1792;                     // candidate buffer
constexpr int kPairSort = kPairCap + kPairKmax;    // what one sort takes
static_assert((kPairSort & (kPairSort - 1)) == 0, "the sort takes a power of two");
static_assert(kPairStep <= kPairCap, "an empty buffer must hold one step");
static_assert(kPairKmax <= 256, "one thread per list slot");
constexpr int kPairWarmK = 64;                     // lists up to this length rank wave 0's cells of the first step on their own

struct PairArgs {
    const float* z1;
    const float* z2;
    const uint32_t* rows;
    const uint32_t* cols;
    uint32_t n_pairs, n1, n2, width;  // n_pairs below 2^31, the others below 2^32: checked by the caller
    int top;
    uint32_t* out_idx;
    float* out_val;
    unsigned long long* first_bad;  // device word: the smallest pair index with a row outside its matrix
};

struct PairCells {  // the four columns of one thread in one sweep step
    float a[4], b[4];
    bool ok[4];
};

// columns c0 .. c0 + 3 of both rows; only those below `width` are read (width = 0: nothing is)
__device__ __forceinline__ PairCells pair_load(const float* ra, const float* rb, int64_t c0, int64_t width) {
    PairCells q;
    if (c0 + 4 <= width) {
        const f4u fa = *reinterpret_cast<const f4u*>(ra + c0);
        const f4u fb = *reinterpret_cast<const f4u*>(rb + c0);
#pragma unroll
        for (int j = 0; j < 4; j++) q.a[j] = fa[j], q.b[j] = fb[j], q.ok[j] = true;
    } else {
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int64_t c = c0 + j;
            q.ok[j] = c < width;
            q.a[j] = q.ok[j] ? ra[c] : 0.f;
            q.b[j] = q.ok[j] ? rb[c] : 0.f;
        }
    }
    return q;
}

template <bool LARGEST>
__global__ __launch_bounds__(256) void pair_kmers_kernel(PairArgs a) {
    __shared__ unsigned long long skey[kPairSort];  // candidates from 0; the list joins them for a sort
    __shared__ uint32_t sval[kPairSort];            // the products' own bits
    __shared__ unsigned long long lkey[kPairKmax];  // the list, best first; 0 = no entry
    __shared__ uint32_t lval[kPairKmax];
    __shared__ unsigned wave_n[2][4];
    const int tid = threadIdx.x, lane = tid & 63, k = a.top;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // a scalar: what depends on it needs no lane mask
    const unsigned long long below = (1ull << lane) - 1;

    // list + the first `ncand` candidates -> list (uniform arguments; every thread calls it)
    auto flush = [&](int ncand) {
        const int m = ncand + k;
        int n2 = 2;
        while (n2 < m) n2 <<= 1;  // <= kPairSort: ncand <= kPairCap, k <= kPairKmax
        if (tid < k) skey[ncand + tid] = lkey[tid], sval[ncand + tid] = lval[tid];  // k <= 256 threads: no loop
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
        if (tid < k) lkey[tid] = skey[tid], lval[tid] = sval[tid];
        __syncthreads();
    };

    for (uint32_t e = blockIdx.x; e < a.n_pairs; e += gridDim.x) {  // no wrap: n_pairs + gridDim.x < 2^32
        const size_t out0 = (size_t)e * k;
        // (the same for every lane: said so, the row pointers then live in scalar registers)
        const uint32_t ri = __builtin_amdgcn_readfirstlane(a.rows[e]), ci = __builtin_amdgcn_readfirstlane(a.cols[e]);
        if (ri >= a.n1 || ci >= a.n2) {  // uniform over the workgroup; nothing of either row is read
            if (tid < k) {
                a.out_idx[out0 + tid] = 0xFFFFFFFFu;
                a.out_val[out0 + tid] = __uint_as_float(0x7FC00000u);
            }
            if (tid == 0) atomicMin(a.first_bad, (unsigned long long)e);
            continue;
        }
        if (tid < k) lkey[tid] = 0ull, lval[tid] = 0u;
        __syncthreads();
        unsigned long long bound = 0ull;

        const float* ra = a.z1 + (size_t)ri * (size_t)a.width;
        const float* rb = a.z2 + (size_t)ci * (size_t)a.width;
        const uint32_t ngroups = (uint32_t)(((int64_t)a.width + 3) / 4);  // at most 2^30
        int ncand = 0;
        unsigned par = 0;  // which set of wave counts the next ranking uses
        // One load site and one ranking site: round g0 puts step g0's cells on their way, then ranks the cells of the step
        // before it, which the previous round loaded; the round past the last step only ranks.
        PairCells cur, nxt;
        for (uint32_t g0 = 0;; g0 += 256) {
            const uint32_t gn = g0 + tid;
            nxt = pair_load(ra, rb, 4 * (int64_t)gn, gn < ngroups ? a.width : 0);
            if (g0 == 0) {
                cur = nxt;
                continue;
            }
            const int64_t c0 = 4 * (int64_t)(g0 - 256 + tid);
            // A short list meets its first 1 024 cells in two parts: wave 0's 256 cells are ranked and sorted at once (512
            // entries), and the other 768 then meet the bound they leave — a few dozen candidates instead of a sort of
            // 2 048 entries per pair, which is what the kernel's time went into (LDS traffic).  The list is the same: the
            // bound is always the list's own last key.
            const int parts = (g0 == 256 && k <= kPairWarmK) ? 2 : 1;
            // (behind the last step one more turn that only sorts what waits: the sort then stands at ONE place in the code)
            const int turns = parts + (g0 >= ngroups ? 1 : 0);
            for (int part = 0; part < turns; part++) {
                const bool mine = parts == 1 || (part == 0) == (wave == 0);
                if (ncand + kPairStep > kPairCap || (parts == 2 && part == 1) || (part == parts && ncand > 0)) {
                    flush(ncand);
                    ncand = 0;
                    bound = lkey[k - 1];
                }
                if (part == parts) break;
                unsigned long long key[4];
                float prod[4];
                bool pass[4];
                unsigned off[4], cnt = 0;  // off: the cell's place among the wave's candidates of this step
                par ^= 1u;
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    prod[j] = __fmul_rn(cur.a[j], cur.b[j]);
                    key[j] = topk_key(LARGEST ? prod[j] : -prod[j], (uint32_t)(c0 + j));
                    pass[j] = mine && cur.ok[j] && key[j] > bound;
                    const unsigned long long mask = __ballot(pass[j]);
                    off[j] = cnt + (unsigned)__popcll(mask & below);
                    cnt += (unsigned)__popcll(mask);
                }
                if (lane == 0) wave_n[par][wave] = cnt;  // two sets: a wave may write the next part while another reads this one
                __syncthreads();
                unsigned before = 0, all = 0;
#pragma unroll
                for (int w = 0; w < 4; w++) {
                    const unsigned n = wave_n[par][w];
                    if (w < wave) before += n;
                    all += n;
                }
                const unsigned pos = (unsigned)ncand + before;  // ncand + all <= kPairCap: checked above
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    if (pass[j]) skey[pos + off[j]] = key[j], sval[pos + off[j]] = __float_as_uint(prod[j]);
                }
                ncand += (int)all;
            }
            cur = nxt;
            if (g0 >= ngroups) break;
        }
        if (tid < k) {
            const unsigned long long key = lkey[tid];
            a.out_idx[out0 + tid] = key ? 0xFFFFFFFFu - (uint32_t)key : 0xFFFFFFFFu;
            a.out_val[out0 + tid] = __uint_as_float(key ? lval[tid] : 0x7FC00000u);
        }
        __syncthreads();
    }
}

// The two factors of every chosen column: one thread per slot, a second look at lines the sweep has just read.  A padded
// slot (a column beyond the width, or a pair the sweep refused) reads nothing.
__global__ __launch_bounds__(256) void pair_factors_kernel(PairArgs a, float* out_z1, float* out_z2) {
    const int64_t slots = (int64_t)a.n_pairs * a.top;
    for (int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x; s < slots; s += (int64_t)gridDim.x * 256) {
        const uint32_t col = a.out_idx[s];
        float f1 = __uint_as_float(0x7FC00000u), f2 = f1;
        if (col != 0xFFFFFFFFu) {
            const int64_t e = s / a.top;
            f1 = a.z1[(size_t)a.rows[e] * (size_t)a.width + col];
            f2 = a.z2[(size_t)a.cols[e] * (size_t)a.width + col];
        }
        if (out_z1) out_z1[s] = f1;
        if (out_z2) out_z2[s] = f2;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// groups
// ---------------------------------------------------------------------------------------------------------------------
constexpr int kGrpCols = 16;      // 64-byte column strip per workgroup
constexpr int kGrpTileRows = 256; // rows staged in LDS per step (16 KiB per buffer)
constexpr int kGrpStagers = 256;  // waves 1..4 stage; wave 0 of the workgroup only walks
constexpr int kGrpThreads = kGrpStagers + 64;
constexpr int kGrpLanesPerRow = kGrpCols / 4;
constexpr int kGrpRowsPerPass = kGrpStagers / kGrpLanesPerRow;
constexpr int kGrpLoads = kGrpTileRows / kGrpRowsPerPass;

struct GroupArgs {
    const float* x;
    const uint32_t* order;
    const int64_t* starts;  // device copy, [n_groups + 1]
    int64_t n_rows, cols, n_groups, strips;
    float* mean;
    float* sd;  // or NULL
    unsigned long long* first_bad;
};

typedef float (*GrpTile)[kGrpCols][kGrpTileRows + 4];

// One pass over the rows of the group: SQUARE = false adds x, SQUARE = true adds fl32(fl32(x - mean)^2).  Tile t + 1 is
// loaded into registers while tile t is walked and stored to the other LDS buffer right after the barrier.  Returns (in
// the walker's lanes < 16) the chain's result; the chain starts at +0, as np.mean's and np.std's sums do (a column of -0 sums to +0).
template <bool SQUARE, bool VEC>
__device__ __forceinline__ float group_pass(GrpTile tile, const GroupArgs& a, int64_t begin, int64_t n, int64_t col0,
                                            const float* smean) {
    const int64_t n_tiles = (n + kGrpTileRows - 1) / kGrpTileRows;
    if (threadIdx.x < 64) {  // ---- the walker wave
        const int wl = threadIdx.x;
        float running = 0.f;
        for (int64_t t = 0; t < n_tiles; t++) {
            __syncthreads();  // tile t is in buffer t & 1; the stagers now fill the other one
            if (wl < kGrpCols) {
                const int64_t left = n - t * kGrpTileRows;
                const int nr = (int)(left < kGrpTileRows ? left : kGrpTileRows);
                const float* colp = &tile[t & 1][wl][0];
                int r = 0;
                for (; r + 4 <= nr; r += 4) {
                    const float4 q = *reinterpret_cast<const float4*>(colp + r);
                    running = __fadd_rn(running, q.x);
                    running = __fadd_rn(running, q.y);
                    running = __fadd_rn(running, q.z);
                    running = __fadd_rn(running, q.w);
                }
                for (; r < nr; r++) running = __fadd_rn(running, colp[r]);
            }
        }
        return running;
    }
    // ---- the staging waves
    const int tid = threadIdx.x - 64;
    const int lane_c4 = (tid % kGrpLanesPerRow) * 4;  // 4 consecutive columns handled by this thread
    const int lane_r = tid / kGrpLanesPerRow;         // row inside a kGrpRowsPerPass-row slab
    float m[4] = {0.f, 0.f, 0.f, 0.f};
    if (SQUARE) {
#pragma unroll
        for (int j = 0; j < 4; j++) m[j] = smean[lane_c4 + j];
    }
    float4 regs[kGrpLoads];
    auto load_tile = [&](int64_t t) {
#pragma unroll
        for (int s = 0; s < kGrpLoads; s++) {
            const int64_t r = t * kGrpTileRows + s * kGrpRowsPerPass + lane_r;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (r < n) {  // rows behind the group's end are neither read nor walked
                int64_t row = a.order[begin + r];
                if (row >= a.n_rows) {  // never dereferenced: the flag makes the call fail, row 0 stands in
                    if (lane_c4 == 0 && !SQUARE) atomicMin(a.first_bad, (unsigned long long)(begin + r));
                    row = 0;
                }
                const float* p = a.x + (size_t)row * (size_t)a.cols;
                const int64_t c = col0 + lane_c4;
                if (VEC) {
                    const f4u q = *reinterpret_cast<const f4u*>(p + c);
                    v = make_float4(q[0], q[1], q[2], q[3]);
                } else {  // the ragged last strip: columns past the end re-read the last one and are never written back
                    v.x = p[c + 0 < a.cols ? c + 0 : a.cols - 1];
                    v.y = p[c + 1 < a.cols ? c + 1 : a.cols - 1];
                    v.z = p[c + 2 < a.cols ? c + 2 : a.cols - 1];
                    v.w = p[c + 3 < a.cols ? c + 3 : a.cols - 1];
                }
            }
            regs[s] = v;
        }
    };
    auto store_tile = [&](int buf) {
#pragma unroll
        for (int s = 0; s < kGrpLoads; s++) {
            float4 v = regs[s];
            if (SQUARE) {
                float d;
                d = __fsub_rn(v.x, m[0]), v.x = __fmul_rn(d, d);
                d = __fsub_rn(v.y, m[1]), v.y = __fmul_rn(d, d);
                d = __fsub_rn(v.z, m[2]), v.z = __fmul_rn(d, d);
                d = __fsub_rn(v.w, m[3]), v.w = __fmul_rn(d, d);
            }
            const int r = s * kGrpRowsPerPass + lane_r;
            tile[buf][lane_c4 + 0][r] = v.x;
            tile[buf][lane_c4 + 1][r] = v.y;
            tile[buf][lane_c4 + 2][r] = v.z;
            tile[buf][lane_c4 + 3][r] = v.w;
        }
    };
    // round t ends with the barrier the walker passes to walk tile t + 1: tile t + 1 goes into buffer (t + 1) & 1, which
    // the walker left before the barrier that ended round t - 1 (it walks tile t in the other buffer meanwhile), and the
    // loads of tile t + 2 are issued.  Both roles pass n_tiles barriers.
    load_tile(0);
    for (int64_t t = -1; t + 1 < n_tiles; t++) {
        store_tile((int)((t + 1) & 1));
        if (t + 2 < n_tiles) load_tile(t + 2);
        __syncthreads();
    }
    return 0.f;
}

template <bool VEC>
__device__ __forceinline__ void group_body(GrpTile tile, float* smean, const GroupArgs& a, int64_t g, int64_t strip) {
    const int64_t begin = a.starts[g], n = a.starts[g + 1] - begin;
    const int64_t col0 = strip * kGrpCols;
    const int wl = threadIdx.x;
    const bool mine = wl < kGrpCols && col0 + wl < a.cols;
    const float nan = __uint_as_float(0x7FC00000u);
    if (n <= 0) {  // uniform over the workgroup
        if (mine) {
            a.mean[(size_t)g * a.cols + col0 + wl] = nan;
            if (a.sd) a.sd[(size_t)g * a.cols + col0 + wl] = nan;
        }
        return;
    }
    const float sum = group_pass<false, VEC>(tile, a, begin, n, col0, smean);
    const float mean = __fdiv_rn(sum, (float)n);
    // a NaN result is written as THE quiet NaN 0x7FC00000: which NaN an operation hands on (x - NaN flips its sign here
    // and not on every host) is no property of the data
    if (mine) a.mean[(size_t)g * a.cols + col0 + wl] = mean != mean ? nan : mean;
    if (!a.sd) return;  // uniform
    if (wl < kGrpCols) smean[wl] = mean;
    __syncthreads();  // also: every walk of the first pass is over before the buffers are filled again
    const float sq = group_pass<true, VEC>(tile, a, begin, n, col0, smean);
    if (mine) {
        const float q = __fdiv_rn(sq, (float)(n - 1));
        // correctly rounded float32 sqrt: float64 sqrt, then one rounding (53 >= 2 * 24 + 2 bits)
        a.sd[(size_t)g * a.cols + col0 + wl] = q != q ? nan : (float)sqrt((double)q);
    }
}

__global__ __launch_bounds__(kGrpThreads) void group_colstat_kernel(GroupArgs a) {
    // column-major tile: the walker takes 4 consecutive rows of its column with one 16-byte LDS read; 4 floats of padding
    // per column keep the 16 walker lanes on distinct banks
    __shared__ __attribute__((aligned(16))) float tile[2][kGrpCols][kGrpTileRows + 4];
    __shared__ float smean[kGrpCols];
    const int64_t items = a.n_groups * a.strips;
    for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
        // neighbouring strips of one group are neighbouring work items: their 64-byte pieces share cache lines
        const int64_t g = item / a.strips, strip = item % a.strips;
        if ((strip + 1) * kGrpCols <= a.cols)  // uniform over the workgroup
            group_body<true>(tile, smean, a, g, strip);
        else
            group_body<false>(tile, smean, a, g, strip);
        __syncthreads();  // the buffers and smean are free for the next item
    }
}

int check_mat(const skr_ctx* ctx, const skr_mat* m, int dtype, const char* what) {
    SKR_REQUIRE(m, "%s is NULL", what);
    SKR_REQUIRE(m->ctx == ctx, "%s belongs to a different ctx", what);
    SKR_REQUIRE(m->dtype == dtype, "%s must be %s", what, dtype == SKR_F32 ? "float32" : "uint32");
    return SKR_OK;
}

// the device word both kernels lower to the first bad position (all ones = none)
int bad_word(skr_ctx* ctx, size_t offset, unsigned long long** out) {
    void* ws = nullptr;
    SKR_TRY(skr_ctx_workspace(ctx, offset + 64, &ws));
    *out = (unsigned long long*)((char*)ws + offset);
    SKR_HIP(hipMemsetAsync(*out, 0xFF, 8, ctx->stream));
    return SKR_OK;
}

int read_bad_word(skr_ctx* ctx, const unsigned long long* d_bad, unsigned long long* bad) {
    SKR_HIP(hipMemcpyAsync(bad, d_bad, 8, hipMemcpyDeviceToHost, ctx->stream));
    SKR_HIP(hipStreamSynchronize(ctx->stream));
    return SKR_OK;
}

}  // namespace

extern "C" int skr_pair_kmers(skr_ctx* ctx, const skr_mat* z1, const skr_mat* z2, const skr_mat* rows, const skr_mat* cols,
                              int64_t n_pairs, int top, int largest, skr_mat* out_idx, skr_mat* out_val, skr_mat* out_z1,
                              skr_mat* out_z2, int64_t* first_bad) {
    SKR_REQUIRE(ctx, "ctx is NULL");
    SKR_TRY(check_mat(ctx, z1, SKR_F32, "z1"));
    SKR_TRY(check_mat(ctx, z2, SKR_F32, "z2"));
    SKR_TRY(check_mat(ctx, rows, SKR_U32, "rows"));
    SKR_TRY(check_mat(ctx, cols, SKR_U32, "cols"));
    SKR_TRY(check_mat(ctx, out_idx, SKR_U32, "out_idx"));
    SKR_TRY(check_mat(ctx, out_val, SKR_F32, "out_val"));
    if (out_z1) SKR_TRY(check_mat(ctx, out_z1, SKR_F32, "out_z1"));
    if (out_z2) SKR_TRY(check_mat(ctx, out_z2, SKR_F32, "out_z2"));
    SKR_REQUIRE(z1->cols == z2->cols, "z1 has %lld columns, z2 has %lld", (long long)z1->cols, (long long)z2->cols);
    SKR_REQUIRE(z1->cols >= 1 && z1->cols < 0xffffffffLL, "the rows must have between 1 and 2^32 - 2 columns");
    SKR_REQUIRE(z1->rows <= 0xffffffffLL && z2->rows <= 0xffffffffLL, "row indices are uint32");  // 2^32 - 1 rows at most
    SKR_REQUIRE(n_pairs <= 0x7fffffffLL, "at most 2^31 - 1 pairs per call");
    SKR_REQUIRE(n_pairs >= 0 && n_pairs <= rows->rows * rows->cols && n_pairs <= cols->rows * cols->cols,
                "n_pairs exceeds the index lists");
    int kmax = 0;
    SKR_TRY(skr_topk_merge_limits(&kmax, nullptr));
    SKR_REQUIRE(top >= 1 && top <= kmax && top <= kPairKmax, "top must be in 1..%d", std::min(kmax, kPairKmax));
    const int64_t cells = n_pairs * top;
    SKR_REQUIRE(out_idx->rows * out_idx->cols >= cells && out_val->rows * out_val->cols >= cells &&
                    (!out_z1 || out_z1->rows * out_z1->cols >= cells) && (!out_z2 || out_z2->rows * out_z2->cols >= cells),
                "the lists must hold %lld cells", (long long)cells);
    SKR_TRY(skr_activate(ctx));
    if (first_bad) *first_bad = -1;
    if (n_pairs == 0) return SKR_OK;
    unsigned long long* d_bad = nullptr;
    SKR_TRY(bad_word(ctx, 0, &d_bad));
    {
        SkrProfScope prof(ctx, "pair_kmers");
        const PairArgs a{(const float*)z1->data, (const float*)z2->data, (const uint32_t*)rows->data, (const uint32_t*)cols->data,
                         (uint32_t)n_pairs, (uint32_t)z1->rows, (uint32_t)z2->rows, (uint32_t)z1->cols, top, (uint32_t*)out_idx->data,
                         (float*)out_val->data, d_bad};
        const dim3 grid((unsigned)std::min<int64_t>(n_pairs, (int64_t)ctx->num_cu * 8));
        if (largest)
            hipLaunchKernelGGL(pair_kmers_kernel<true>, grid, dim3(256), 0, ctx->stream, a);
        else
            hipLaunchKernelGGL(pair_kmers_kernel<false>, grid, dim3(256), 0, ctx->stream, a);
        SKR_HIP(hipGetLastError());
        if (out_z1 || out_z2)
            hipLaunchKernelGGL(pair_factors_kernel, dim3(skr_grid(ctx, cells)), dim3(256), 0, ctx->stream, a,
                               out_z1 ? (float*)out_z1->data : nullptr, out_z2 ? (float*)out_z2->data : nullptr);
        SKR_HIP(hipGetLastError());
    }
    unsigned long long bad = 0;
    SKR_TRY(read_bad_word(ctx, d_bad, &bad));
    if (bad != ~0ull) {
        if (first_bad) *first_bad = (int64_t)bad;
        return skr_set_error(SKR_ERR_INVALID, "pair %lld names a row outside its matrix (%lld and %lld rows)", (long long)bad,
                             (long long)z1->rows, (long long)z2->rows);
    }
    return SKR_OK;
}

extern "C" int skr_group_colstat(skr_ctx* ctx, const skr_mat* x, const skr_mat* order, const int64_t* starts, int64_t n_groups,
                                 skr_mat* mean, skr_mat* sd) {
    SKR_REQUIRE(ctx, "ctx is NULL");
    SKR_TRY(check_mat(ctx, x, SKR_F32, "x"));
    SKR_TRY(check_mat(ctx, order, SKR_U32, "order"));
    SKR_TRY(check_mat(ctx, mean, SKR_F32, "mean"));
    if (sd) SKR_TRY(check_mat(ctx, sd, SKR_F32, "sd"));
    SKR_REQUIRE(starts && n_groups >= 0, "starts is NULL or n_groups negative");
    SKR_REQUIRE(starts[0] >= 0, "starts[0] is negative");
    for (int64_t g = 0; g < n_groups; g++)
        SKR_REQUIRE(starts[g + 1] >= starts[g], "starts must not decrease (group %lld)", (long long)g);
    SKR_REQUIRE(starts[n_groups] <= order->rows * order->cols, "the groups name %lld entries, order holds %lld",
                (long long)starts[n_groups], (long long)(order->rows * order->cols));
    SKR_REQUIRE(mean->rows * mean->cols >= n_groups * x->cols && (!sd || sd->rows * sd->cols >= n_groups * x->cols),
                "mean and sd must hold [%lld, %lld]", (long long)n_groups, (long long)x->cols);
    SKR_TRY(skr_activate(ctx));
    if (n_groups == 0 || x->cols == 0) return SKR_OK;
    if (x->rows == 0 && starts[n_groups] > starts[0])
        return skr_set_error(SKR_ERR_INVALID, "entry %lld of order names a row outside the matrix (0 rows)", (long long)starts[0]);
    const int64_t strips = (x->cols + kGrpCols - 1) / kGrpCols;
    SKR_REQUIRE(n_groups <= (int64_t)0x7fffffff / strips, "too many (group, strip) work items");
    const size_t starts_bytes = ((size_t)(n_groups + 1) * 8 + 63) & ~(size_t)63;
    unsigned long long* d_bad = nullptr;
    SKR_TRY(bad_word(ctx, starts_bytes, &d_bad));
    int64_t* d_starts = (int64_t*)((char*)d_bad - starts_bytes);
    SKR_HIP(hipMemcpyAsync(d_starts, starts, (size_t)(n_groups + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
    {
        SkrProfScope prof(ctx, "group_colstat");
        const GroupArgs a{(const float*)x->data, (const uint32_t*)order->data, d_starts, x->rows, x->cols, n_groups, strips,
                          (float*)mean->data, sd ? (float*)sd->data : nullptr, d_bad};
        const int64_t items = n_groups * strips;
        hipLaunchKernelGGL(group_colstat_kernel, dim3((unsigned)std::min<int64_t>(items, (int64_t)ctx->num_cu * 16)),
                           dim3(kGrpThreads), 0, ctx->stream, a);
        SKR_HIP(hipGetLastError());
    }
    unsigned long long bad = 0;
    SKR_TRY(read_bad_word(ctx, d_bad, &bad));
    if (bad != ~0ull)
        return skr_set_error(SKR_ERR_INVALID, "entry %lld of order names a row outside the matrix (%lld rows)", (long long)bad,
                             (long long)x->rows);
    return SKR_OK;
}
