// The device and host pieces count_rows_kernel (count.hip) and count_windows_kernel (windows.hip) share: the packed bins of
// a k in the LDS, the sweep that counts the 16 k-mers of a (hi, lo) pair of packed words into them, the flush of the bins
// into a dense output row, and the LDS a launch asks for.  One copy: a fix or a retune reaches both kernels.  Included
// by count.hip and windows.hip only, so everything here is compiled with -ffp-contract=off (per_kb.hpp).
#pragma once
#include <algorithm>

#include "common.hpp"
#include "per_kb.hpp"

enum OutKind { OUT_F32 = 0, OUT_F32_LOG2 = 1, OUT_U32 = 2, OUT_F64 = 3 };

// The output value of a count: the per-kb value, then `counts += 1; log2` if the mode asks (kmer_counts.py:189-192).
template <bool LOG2>
__device__ __forceinline__ float per_kb_out(uint32_t n, double inc) {
    float t = per_kb_value(n, inc);
    if (LOG2) t = skr_log2_cr(t + 1.0f);
    return t;
}

// The item's output value for every small count (almost all bins): 16 lanes do the float64 work once, the flush just looks
// it up (visible to the flush after the barrier or wave fence that ends the counting).
template <int OUT>
__device__ __forceinline__ void build_value_table(float* tab, int tid, double inc) {
    if ((OUT == OUT_F32 || OUT == OUT_F32_LOG2) && tid < kTabSize) tab[tid] = per_kb_out<OUT == OUT_F32_LOG2>((uint32_t)tid, inc);
}

template <int OUT>
__device__ __forceinline__ float table_value(const float* tab, uint32_t n, double inc) {
    if (n < (uint32_t)kTabSize) return tab[n];
    return per_kb_out<OUT == OUT_F32_LOG2>(n, inc);
}

// LDS words of the bins of a k (at least the four that a lane step of the flush reads).
template <bool WIDE>
__host__ __device__ constexpr uint32_t bin_words(int k) {
    return std::max<uint32_t>(4u, (1u << (2 * k)) >> (WIDE ? 0 : 1));
}

// Bins of a k in the LDS: hist [hist_words] | trash [64] | tab [16].  16-bit counters packed two to a word — bin b and
// bin b + nwords share word b mod nwords, the top bit of the column picks the half — or, WIDE, one 32-bit bin per word.
template <bool WIDE>
struct BinGeom {
    uint32_t nbins, nwords, hist_words;
    uint32_t* hist;
    uint32_t trash_addr;  // one word per lane: no two lanes of a wave collide on it
    float* tab;
    uint32_t sh, amask;   // (v >> sh) & amask = byte address of the word of the k-mer in the top 2k bits of v
    uint32_t win_mask;    // k consecutive validity bits

    __device__ __forceinline__ BinGeom(uint32_t* lds, int k, int tid)
        : nbins(1u << (2 * k)), nwords(WIDE ? nbins : nbins >> 1), hist_words(bin_words<WIDE>(k)), hist(lds),
          trash_addr((hist_words + (tid & 63)) * 4), tab(reinterpret_cast<float*>(lds + hist_words + 64)), sh(30 - 2 * k),
          amask((nwords - 1) << 2), win_mask((1u << k) - 1u) {}

    template <int T>
    __device__ __forceinline__ void zero(int tid) const {  // bins and trash words, by the T threads of the workgroup
        for (uint32_t w = tid * 4; w < hist_words + 64; w += T * 4) *reinterpret_cast<uint4*>(&hist[w]) = make_uint4(0, 0, 0, 0);
    }
    static size_t lds_bytes(int k) { return ((size_t)bin_words<WIDE>(k) + 64 + kTabSize) * 4; }
};

// One sweep's share of a lane: the 16 k-mers that start in the 16 bases at the top of `hi` (first base in the top bits;
// `lo` holds the next 16).  k-mer j is r_j = v_alignbit(hi, lo, 32 - 2j) and its column the top 2k bits of r_j: no branch,
// five vector instructions per k-mer, counted by ds_add_u32 (no return).  `whole`: every lane of the workgroup has 16 whole
// k-mers and the sequence has no mask; `left`: k-mers of the item from this lane's first on (may be <= 0); `load_invalid()`
// gives the lane's validity word (bit j: base j of `hi` is not in the alphabet) and is called in the slow arm only, before
// the `lim > 0` test: its loads are neither on the fast path nor behind a second branch.
template <bool WIDE, typename MaskLoad>
__device__ __forceinline__ void sweep_pair(const BinGeom<WIDE>& g, int tid, uint32_t hi, uint32_t lo, bool whole, int64_t left,
                                           MaskLoad load_invalid) {
    // (The geometry in locals, and the increment spelled `WIDE ? 1 : (sign ? hi : lo)`: with `g.sh` read inside the arms, or
    // with `WIDE || ...` in the condition, hipcc turns the trash select of the slow arm into 16 exec-mask branches.)
    uint32_t* const hist = g.hist;
    const uint32_t sh = g.sh, amask = g.amask, trash_addr = g.trash_addr, win_mask = g.win_mask;
    if (whole) {
        // Wave-level aggregation: if all 64 lanes hold the same two words (homopolymers and every repeat whose period
        // divides 16 bases), each of the 16 columns would get 64 adds on one address: one lane adds 64 instead
        const uint32_t h0 = __builtin_amdgcn_readfirstlane(hi), l0 = __builtin_amdgcn_readfirstlane(lo);
        const bool same = __builtin_amdgcn_ballot_w64(((hi ^ h0) | (lo ^ l0)) != 0) == 0;
        if (same) {
            if ((tid & 63) == 0) {
#pragma unroll
                for (int j = 0; j < 16; j++) {
                    const uint32_t v = j ? __builtin_amdgcn_alignbit(hi, lo, 32 - 2 * j) : hi;
                    lds_add_u32(hist, (v >> sh) & amask, WIDE ? 64u : ((int32_t)v < 0 ? 0x400000u : 64u));
                }
            }
        } else {
#pragma unroll
            for (int j = 0; j < 16; j++) {
                const uint32_t v = j ? __builtin_amdgcn_alignbit(hi, lo, 32 - 2 * j) : hi;
                lds_add_u32(hist, (v >> sh) & amask, WIDE ? 1u : ((int32_t)v < 0 ? 0x10000u : 1u));
            }
        }
    } else {
        // a sweep that holds the end of the item or non-alphabet bases: k-mers that do not count are sent to a trash word
        // instead of being branched around (they are still counted in W: kmer_counts.py:143-149)
        const int lim = left < 0 ? 0 : (left > 16 ? 16 : (int)left);
        const uint32_t invalid = load_invalid();
        if (lim > 0) {  // lanes past the end of the item do nothing
#pragma unroll
            for (int j = 0; j < 16; j++) {
                const uint32_t v = j ? __builtin_amdgcn_alignbit(hi, lo, 32 - 2 * j) : hi;
                const bool ok = j < lim && ((invalid >> j) & win_mask) == 0;
                lds_add_u32(hist, ok ? ((v >> sh) & amask) : trash_addr, WIDE ? 1u : ((int32_t)v < 0 ? 0x10000u : 1u));
            }
        }
    }
}

// A 16-byte piece of a row.  KEEP: the row is read again in a moment, leave it in the L2 (ordinary store); else it is
// written once and not read again by the kernel: keep it out of the L2 (nontemporal store).
template <bool KEEP, typename V>
__device__ __forceinline__ void store_piece(V v, void* dst) {
    if (KEEP) *reinterpret_cast<V*>(dst) = v;
    else __builtin_nontemporal_store(v, reinterpret_cast<V*>(dst));
}

// The flush: bins -> output values, the dense row `out` (nbins cells of OUT's type) to HBM, by the T threads of the
// workgroup.  A lane step reads four words (eight packed bins), zeroes them if ZERO (a persistent workgroup counts its next
// item into them), converts the counts through the item's table and stores the two 16-byte pieces they make — bins
// b .. b+3 and b+nwords .. b+nwords+3 — lo piece, then hi piece, back to back.  (Two other orders were measured — the row
// strictly in ascending address order, the hi pieces parked in registers, with nontemporal or ordinary stores: 2 % at
// best at k = 6, 12-23 % slower at k = 7; DESIGN §4 — and removed again.)
template <int OUT, bool WIDE, bool ZERO, bool KEEP, int T>
__device__ __forceinline__ void flush_row(const BinGeom<WIDE>& g, int tid, void* out, double inc) {
    typedef float f4 __attribute__((ext_vector_type(4)));
    typedef uint32_t u4 __attribute__((ext_vector_type(4)));
    uint32_t* const out_u = reinterpret_cast<uint32_t*>(out);
    float* const out_f = reinterpret_cast<float*>(out);
    uint32_t* const hist = g.hist;
    const float* const tab = g.tab;
    const uint32_t nwords = g.nwords;
    auto value_of = [&](uint32_t n) -> float { return table_value<OUT>(tab, n, inc); };
    for (uint32_t w4 = tid * 4; w4 < nwords; w4 += T * 4) {
        const uint4 c = *reinterpret_cast<const uint4*>(&hist[w4]);
        if (ZERO) *reinterpret_cast<uint4*>(&hist[w4]) = make_uint4(0, 0, 0, 0);
        if (WIDE) {  // four bins of four words: one 16-byte piece (k = 1: the whole row)
            if (OUT == OUT_U32) store_piece<KEEP>(u4{c.x, c.y, c.z, c.w}, out_u + w4);
            else store_piece<KEEP>(f4{value_of(c.x), value_of(c.y), value_of(c.z), value_of(c.w)}, out_f + w4);
        } else if (nwords < 4) {  // k = 1: two words, four bins
            const uint32_t cw[2] = {c.x, c.y};
            for (int i = 0; i < 2; i++) {
                if (OUT == OUT_U32) {
                    out_u[i] = cw[i] & 0xFFFFu;
                    out_u[2 + i] = cw[i] >> 16;
                } else {
                    out_f[i] = value_of(cw[i] & 0xFFFFu);
                    out_f[2 + i] = value_of(cw[i] >> 16);
                }
            }
        } else if (OUT == OUT_U32) {
            store_piece<KEEP>(u4{c.x & 0xFFFFu, c.y & 0xFFFFu, c.z & 0xFFFFu, c.w & 0xFFFFu}, out_u + w4);
            store_piece<KEEP>(u4{c.x >> 16, c.y >> 16, c.z >> 16, c.w >> 16}, out_u + w4 + nwords);
        } else {
            f4 lo4, hi4;
            if (((c.x | c.y | c.z | c.w) & 0xFFF0FFF0u) == 0) {  // all eight counts below 16: table
                lo4 = f4{tab[c.x & 15u], tab[c.y & 15u], tab[c.z & 15u], tab[c.w & 15u]};
                hi4 = f4{tab[c.x >> 16], tab[c.y >> 16], tab[c.z >> 16], tab[c.w >> 16]};
            } else {
                lo4 = f4{value_of(c.x & 0xFFFFu), value_of(c.y & 0xFFFFu), value_of(c.z & 0xFFFFu), value_of(c.w & 0xFFFFu)};
                hi4 = f4{value_of(c.x >> 16), value_of(c.y >> 16), value_of(c.z >> 16), value_of(c.w >> 16)};
            }
            store_piece<KEEP>(lo4, out_f + w4);
            store_piece<KEEP>(hi4, out_f + w4 + nwords);
        }
    }
}

// LDS a launch of one workgroup per row asks for, so that `occ` workgroups share a CU (0: no more than the bins need).
// At k = 6 the 8 KiB of 16-bit bins would let 19 one-wave workgroups share a CU; SEVENTEEN (9.25 KiB of LDS each) write the
// rows 7-8 % faster behind a contraction — 0.138-0.140 ms against 0.149-0.150 for 50 000 x 2 kb, 0.76 against 0.70 of
// 8 TB/s, two runs of tools/count_bench.py --pre gemm (profiles/r4_count_occupancy.log: 18 and 19 per CU 0.150, 17 and 16
// 0.139, 15 and 14 0.146, 12 0.160, 8 0.187) — fewer row streams, no SIMD with a fifth wave for long.  Inside the bench
// step 17 measured 0.141-0.142 ms against 0.144-0.145 for 16 (two runs each), so 17 it is.  Smaller k (2 KiB of bins and
// less) are fastest unrestricted.  SEEKR_COUNT_OCC overrides.
template <bool WIDE>
inline size_t row_launch_lds(const skr_ctx* ctx, int wps, int k) {
    const size_t lds = BinGeom<WIDE>::lds_bytes(k);
    const int occ = ctx->knobs.count_occ > 0 ? ctx->knobs.count_occ : (wps == 1 && k == 6 && !WIDE ? 17 : 0);
    return occ > 0 ? std::max(lds, ((size_t)160 * 1024 / (size_t)occ) & ~(size_t)255) : lds;
}
