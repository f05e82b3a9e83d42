// Leiden communities of an undirected weighted edge list (the step kmer_leiden.py:131-146 hands to leidenalg), on the
// device.  Four phases, each a few kernels, driven by the host (no kernel waits for another workgroup):
//   CSR build     mirror the upper-triangle list, sort by (source, target) with radix.hpp (policy LPass below), row
//                 offsets by skr_radix::exclusive_scan
//   local moving  every node sums the weight to each neighbouring community in a hash table and proposes its best move
//                 against the totals of the sweep's start; work unit by degree: one wave per node (table in the LDS) up
//                 to kWaveDeg, one workgroup per node (LDS table) up to kLdsDeg, one workgroup per node with a table in
//                 the ctx workspace above.  A sweep is kept only if the quality rose; otherwise the same proposals are
//                 applied to a hashed subset of the nodes (1/2 .. 1/16), and at last to the single best one.  A move
//                 needs a gain > 0; on an aggregate a node alone in its community also joins a neighbouring community
//                 at a gain of exactly 0 (refinement's >= 0, one level up), and such a sweep is kept at equal quality
//                 when it leaves fewer communities: of partitions that tie, the coarser one is returned
//   refinement    inside each community, from singletons: a still-single node joins the neighbouring part of its own
//                 community with the best gain >= 0 (greedy, not random); single -> single only toward the smaller id,
//                 and a single node that is somebody's target stays, so every part is connected
//   aggregation   parts become nodes (dense relabel by scan), edges are mapped to (part, part), sorted, equal keys added;
//                 an intra-part edge becomes the node's self-loop entry; the aggregate starts from the unrefined
//                 communities
// Reproducibility: every sum that decides a move is an INTEGER sum — edge weights and degrees are taken to int64 fixed
// point (2^-F, F <= 40 chosen from the total weight) when the CSR is built, so hash-table slots, community totals and
// aggregated weights are the same bits whatever order the atomics arrive in.  Gains are float64 expressions of those
// integers.  The quality that is reported is a float64 sum of the original float32 weights in a fixed tree order.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "common.hpp"
#include "radix.hpp"

namespace {

using u32 = uint32_t;
using u64 = unsigned long long;
using i64 = long long;

constexpr int kWaveDeg = 64;      // degree <= this: one wave per node
constexpr int kWaveSlots = 128;
constexpr int kLdsDeg = 2048;     // degree <= this: one workgroup per node, table in the LDS
constexpr int kLdsSlots = 4096;   // 48 KiB
constexpr u32 kNone = 0xFFFFFFFFu;
constexpr int kMaxFrac = 40;      // fixed point: at most 40 fractional bits
constexpr int kSubsetTries = 4;   // halvings of the node subset before the single best move is tried

// ---- the sort's policy (radix.hpp): 64-bit key, 64-bit payload, digit at any bit of the key
struct LPass {
    using Count = u32;
    struct Item {
        u64 key;
        i64 pay;
    };
    const u64* kin;
    const i64* pin;
    u64* kout;
    i64* pout;
    int shift;
    __device__ __forceinline__ Item load(int64_t i) const { return Item{kin[i], pin[i]}; }
    __device__ __forceinline__ u32 digit(const Item& it) const { return (u32)(it.key >> shift) & 255u; }
    __device__ __forceinline__ void store(u32 pos, const Item& it) const {
        kout[pos] = it.key;
        pout[pos] = it.pay;
    }
};

// ---- deterministic float64 sum of f(0) .. f(n-1): 4 096 terms per workgroup (16 consecutive per thread, then a
// fixed shuffle tree), the workgroup sums added by one workgroup in the same way
__device__ __forceinline__ double block_sum(double v, double* lds) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) lds[wave] = v;
    __syncthreads();
    return (lds[0] + lds[1]) + (lds[2] + lds[3]);
}

template <class F>
__global__ __launch_bounds__(256) void sum_kernel(const F f, int64_t n, double* __restrict__ partials) {
    __shared__ double lds[4];
    const int64_t base = (int64_t)blockIdx.x * 4096 + (int64_t)threadIdx.x * 16;
    double s = 0.0;
    for (int j = 0; j < 16; j++)
        if (base + j < n) s += f(base + j);
    s = block_sum(s, lds);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

__global__ __launch_bounds__(256) void sum_final_kernel(const double* __restrict__ partials, int64_t nb, double* __restrict__ out) {
    __shared__ double lds[4];
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < nb; i += 256) s += partials[i];
    s = block_sum(s, lds);
    if (threadIdx.x == 0) *out = s;
}

template <class F>
int det_sum(skr_ctx* ctx, const F& f, int64_t n, double* partials, double* out) {
    const int64_t nb = std::max<int64_t>(1, (n + 4095) / 4096);
    hipLaunchKernelGGL(sum_kernel<F>, dim3((unsigned)nb), dim3(256), 0, ctx->stream, f, n, partials);
    SKR_HIP(hipGetLastError());
    hipLaunchKernelGGL(sum_final_kernel, dim3(1), dim3(256), 0, ctx->stream, (const double*)partials, nb, out);
    SKR_HIP(hipGetLastError());
    return SKR_OK;
}

// ---- input check (with the degrees, for the size of the device-memory tables) and mirror
__global__ __launch_bounds__(256) void validate_degree_kernel(const u32* __restrict__ rows, const u32* __restrict__ cols,
                                                              const float* __restrict__ vals, int64_t ne, u32 n, u32* __restrict__ deg,
                                                              u32* __restrict__ bad) {
    u32 flags = 0;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < ne; e += (int64_t)gridDim.x * 256) {
        const u32 r = rows[e], c = cols[e];
        const float w = vals[e];
        if (r >= c) flags |= 1u;
        if (!(w > 0.0f) || !(w <= 3.0e38f)) flags |= 2u;  // zero, negative, NaN, infinite
        if (r >= n || c >= n) {
            flags |= 4u;
        } else {
            atomicAdd(&deg[r], 1u);
            atomicAdd(&deg[c], 1u);
        }
    }
    if (flags) atomicOr(bad, flags);
}
__global__ __launch_bounds__(256) void max_u32_kernel(const u32* __restrict__ x, int64_t n, u32* __restrict__ out) {
    u32 m = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) m = max(m, x[i]);
    if (m) atomicMax(out, m);
}
__global__ __launch_bounds__(256) void mirror_kernel(const u32* __restrict__ rows, const u32* __restrict__ cols, const float* __restrict__ vals,
                                                     int64_t ne, u64* __restrict__ keys, i64* __restrict__ pay) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < ne; e += (int64_t)gridDim.x * 256) {
        const u32 r = rows[e], c = cols[e];
        keys[2 * e] = ((u64)r << 32) | c;
        keys[2 * e + 1] = ((u64)c << 32) | r;
        pay[2 * e] = pay[2 * e + 1] = (i64)__float_as_uint(vals[e]);
    }
}

struct ValSum {
    const float* vals;
    __device__ double operator()(int64_t e) const { return (double)vals[e]; }
};

__global__ __launch_bounds__(256) void iota_kernel(u32* __restrict__ x, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) x[i] = (u32)i;
}

// counts of entries per source into cnt[src] (integer atomics), for the row offsets
__global__ __launch_bounds__(256) void src_count_kernel(const u64* __restrict__ keys, int64_t ne, u32* __restrict__ cnt) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < ne; e += (int64_t)gridDim.x * 256) atomicAdd(&cnt[(u32)(keys[e] >> 32)], 1u);
}

// level 0, after the sort: float64 degree in CSR order (fixed lane stride + shuffle tree), payload float bits -> fixed point
__global__ __launch_bounds__(256) void degree0_kernel(const u32* __restrict__ offs, i64* __restrict__ pay, int64_t n, double scale,
                                                      double* __restrict__ deg0, i64* __restrict__ degfx) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;
    const u32 b = offs[i], e = offs[i + 1];
    double s = 0.0;
    i64 sf = 0;
    for (u32 t = b + lane; t < e; t += 64) {
        const double w = (double)__uint_as_float((u32)pay[t]);
        const i64 wf = (i64)llrint(w * scale);
        s += w;
        sf += wf;
        pay[t] = wf;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        s += __shfl_xor(s, off, 64);
        sf += __shfl_xor(sf, off, 64);
    }
    if (lane == 0) {
        deg0[i] = s;
        degfx[i] = sf;
    }
}

__global__ __launch_bounds__(256) void fill_i64_kernel(i64* __restrict__ x, int64_t n, i64 v) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) x[i] = v;
}

// ---- one level's graph and state, as the kernels see it
struct Level {
    int64_t n;            // nodes
    const u32* offs;      // [n + 1]
    const u64* keys;      // source << 32 | target, sorted; a (v, v) entry is v's self-loop (twice its inner weight)
    const i64* w;         // fixed-point weights
    const i64* mass;      // [n] fixed-point degree (configuration model) or node count (ER, CPM)
    double wscale;        // 2^-F
    double mscale;        // 2^-F or 1
    double gp;            // resolution * penalty scale: gamma / 2m, gamma * p, gamma
};

struct Cand {
    double g;
    u32 l;
};
__device__ __forceinline__ bool better(const Cand& a, const Cand& b) { return a.g > b.g || (a.g == b.g && a.l < b.l); }

// ---- the hash table: open addressing, integer atomics only.  GLOBAL: the table is in device memory and one workgroup
// is its only user; every access is an agent-scope atomic so that no stale line of the CU's L1 is ever read.
template <bool GLOBAL>
__device__ __forceinline__ u32 tab_key(const u32* keys, u32 s) {
    return GLOBAL ? __hip_atomic_load(keys + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : keys[s];
}
template <bool GLOBAL>
__device__ __forceinline__ u64 tab_val(const u64* vals, u32 s) {
    return GLOBAL ? __hip_atomic_load(vals + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : vals[s];
}
template <bool GLOBAL>
__device__ __forceinline__ void tab_clear(u32* keys, u64* vals, u32 slots, int tid, int nthreads) {
    for (u32 s = tid; s < slots; s += nthreads) {
        if (GLOBAL) {
            __hip_atomic_store(keys + s, kNone, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(vals + s, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else {
            keys[s] = kNone;
            vals[s] = 0ull;
        }
    }
}
__device__ __forceinline__ u32 tab_hash(u32 key, u32 mask) { return ((key * 2654435761u) >> 7) & mask; }

template <bool GLOBAL>
__device__ __forceinline__ void tab_add(u32* keys, u64* vals, u32 mask, u32 key, u64 w) {
    u32 h = tab_hash(key, mask);
    for (u32 probe = 0; probe <= mask; probe++) {  // the table has at least twice as many slots as keys: always ends early
        u32 seen = kNone;
        const bool won = GLOBAL ? __hip_atomic_compare_exchange_strong(keys + h, &seen, key, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                                : __hip_atomic_compare_exchange_strong(keys + h, &seen, key, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (won || seen == key) {
            if (GLOBAL)
                __hip_atomic_fetch_add(vals + h, w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            else
                __hip_atomic_fetch_add(vals + h, w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            return;
        }
        h = (h + 1) & mask;
    }
}
template <bool GLOBAL>
__device__ __forceinline__ u64 tab_find(const u32* keys, const u64* vals, u32 mask, u32 key) {
    u32 h = tab_hash(key, mask);
    for (u32 probe = 0; probe <= mask; probe++) {
        const u32 k = tab_key<GLOBAL>(keys, h);
        if (k == key) return tab_val<GLOBAL>(vals, h);
        if (k == kNone) return 0ull;
        h = (h + 1) & mask;
    }
    return 0ull;
}

// what a proposal pass reads and writes.  refine == 0: labels are communities, `tot` / `cnt` have 2 n entries (label
// n + v is v's own empty community to escape to).  refine != 0: labels are parts, neighbours outside bound[v] are
// ignored, only nodes whose part is still single propose, and `target` marks single parts that were proposed to.
struct Propose {
    const u32* label;
    const i64* tot;
    const u32* cnt;
    const u32* bound;
    u32* target;
    u32* prop;
    double* pgain;
    int refine;
    int ties;  // local moving on an aggregate: a node alone in its community also joins a neighbour at a gain of exactly 0
};

// One node, by the `nthreads` threads that share the table (a wave, or the whole workgroup).  Every thread of the
// workgroup calls this (the barriers are the workgroup's); `active` is false for threads whose group has no node.
template <bool GLOBAL, int WAVES>
__device__ __forceinline__ void node_propose(const Level& L, const Propose& P, bool active, u32 v, u32* keys, u64* vals, u32 slots, int tid,
                                             double* red_g, u32* red_l) {
    const int nthreads = WAVES * 64;
    const u32 mask = slots - 1;
    tab_clear<GLOBAL>(keys, vals, slots, tid, nthreads);
    __syncthreads();
    u32 own = kNone, b = 0, e = 0, vb = 0;
    if (active) {
        own = P.label[v];
        b = L.offs[v];
        e = L.offs[v + 1];
        if (P.refine) {
            vb = P.bound[v];
            if (P.cnt[own] != 1) active = false;  // no longer single: stays where it is
        }
    }
    if (active) {
        if (!P.refine && tid == 0) tab_add<GLOBAL>(keys, vals, mask, own, 0ull);
        for (u32 t = b + tid; t < e; t += nthreads) {
            const u32 j = (u32)L.keys[t];
            if (j == v) continue;  // the self-loop entry
            if (P.refine && P.bound[j] != vb) continue;
            tab_add<GLOBAL>(keys, vals, mask, P.label[j], (u64)L.w[t]);
        }
    }
    __syncthreads();
    Cand best{-INFINITY, kNone};
    double g_stay = 0.0;
    if (active) {
        const i64 mv = L.mass[v];
        const double a = (double)mv * L.mscale;
        const u32 own_cnt = P.cnt[own];
        if (!P.refine) {
            const double w_own = (double)(i64)tab_find<GLOBAL>(keys, vals, mask, own) * L.wscale;
            g_stay = w_own - L.gp * a * ((double)(P.tot[own] - mv) * L.mscale);
            // the node's own empty community: worth 0
            if (tid == 0 && own_cnt > 1 && P.cnt[(u32)L.n + v] == 0) best = Cand{0.0, (u32)L.n + v};
        }
        for (u32 s = tid; s < slots; s += nthreads) {
            const u32 d = tab_key<GLOBAL>(keys, s);
            if (d == kNone || d == own) continue;
            if (own_cnt == 1 && P.cnt[d] == 1 && d > own) continue;  // single into single only toward the smaller id
            const double wd = (double)(i64)tab_val<GLOBAL>(vals, s) * L.wscale;
            const Cand c{wd - L.gp * a * ((double)P.tot[d] * L.mscale), d};
            if (better(c, best)) best = c;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const Cand o{__shfl_xor(best.g, off, 64), __shfl_xor(best.l, off, 64)};
        if (better(o, best)) best = o;
    }
    if (WAVES > 1) {
        const int lane = tid & 63, wave = tid >> 6;
        if (lane == 0) {
            red_g[wave] = best.g;
            red_l[wave] = best.l;
        }
        __syncthreads();
        best = Cand{red_g[0], red_l[0]};
        for (int w = 1; w < WAVES; w++) {
            const Cand o{red_g[w], red_l[w]};
            if (better(o, best)) best = o;
        }
    }
    if (active && tid == 0) {
        const bool tie = P.ties && P.cnt[own] == 1 && best.g == g_stay;
        const bool go = best.l != kNone && (P.refine ? best.g >= 0.0 : best.g > g_stay || tie);
        P.prop[v] = go ? best.l : kNone;
        if (!P.refine) P.pgain[v] = go ? best.g - g_stay : 0.0;
        if (go && P.refine && P.cnt[best.l] == 1) P.target[best.l] = 1u;
    }
    __syncthreads();  // the table is cleared again by the next node
}

__global__ __launch_bounds__(256) void propose_wave_kernel(const Level L, const Propose P) {
    __shared__ u32 keys[4][kWaveSlots];
    __shared__ u64 vals[4][kWaveSlots];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t v = (int64_t)blockIdx.x * 4 + wave;
    bool active = v < L.n;
    if (active) active = L.offs[v + 1] - L.offs[v] <= (u32)kWaveDeg;
    node_propose<false, 1>(L, P, active, (u32)(active ? v : 0), keys[wave], vals[wave], kWaveSlots, lane, nullptr, nullptr);
}

__global__ __launch_bounds__(256) void propose_block_kernel(const Level L, const Propose P, const u32* __restrict__ list) {
    __shared__ u32 keys[kLdsSlots];
    __shared__ u64 vals[kLdsSlots];
    __shared__ double red_g[4];
    __shared__ u32 red_l[4];
    node_propose<false, 4>(L, P, true, list[blockIdx.x], keys, vals, kLdsSlots, threadIdx.x, red_g, red_l);
}

__global__ __launch_bounds__(256) void propose_global_kernel(const Level L, const Propose P, const u32* __restrict__ list, u32 count,
                                                             u32* __restrict__ tkeys, u64* __restrict__ tvals, u32 slots) {
    __shared__ double red_g[4];
    __shared__ u32 red_l[4];
    u32* keys = tkeys + (size_t)blockIdx.x * slots;
    u64* vals = tvals + (size_t)blockIdx.x * slots;
    for (u32 t = blockIdx.x; t < count; t += gridDim.x)
        node_propose<true, 4>(L, P, true, list[t], keys, vals, slots, threadIdx.x, red_g, red_l);
}

// nodes by work unit: lists of the workgroup-per-node classes (their order does not matter: nodes are independent)
__global__ __launch_bounds__(256) void classify_kernel(const u32* __restrict__ offs, int64_t n, u32* __restrict__ list_blk,
                                                       u32* __restrict__ list_glb, u32* __restrict__ counters /* blk, glb, maxdeg */) {
    for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < n; v += (int64_t)gridDim.x * 256) {
        const u32 d = offs[v + 1] - offs[v];
        if (d > (u32)kLdsDeg) {
            list_glb[atomicAdd(&counters[1], 1u)] = (u32)v;
            atomicMax(&counters[2], d);
        } else if (d > (u32)kWaveDeg) {
            list_blk[atomicAdd(&counters[0], 1u)] = (u32)v;
        }
    }
}

// ---- totals of a labelling (integer atomics)
__global__ __launch_bounds__(256) void totals_kernel(const u32* __restrict__ label, const i64* __restrict__ mass, int64_t n,
                                                     i64* __restrict__ tot, u32* __restrict__ cnt) {
    for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < n; v += (int64_t)gridDim.x * 256) {
        const u32 c = label[v];
        atomicAdd((u64*)&tot[c], (u64)mass[v]);
        atomicAdd(&cnt[c], 1u);
    }
}

// which proposals a sweep applies: all (tries == 0), a hashed 1 / 2^tries of the nodes, or one node
__device__ __forceinline__ bool chosen(u32 v, int tries, u32 salt, u32 only) {
    if (tries > kSubsetTries) return v == only;
    const u32 h = ((v ^ salt) * 2246822519u) >> 11;
    return (h & ((1u << tries) - 1u)) == 0u;
}

__global__ __launch_bounds__(256) void apply_kernel(const u32* __restrict__ comm, const u32* __restrict__ prop, const i64* __restrict__ mass,
                                                    int64_t n, int tries, u32 salt, const u32* __restrict__ only, u32* __restrict__ comm_try,
                                                    i64* __restrict__ tot, u32* __restrict__ cnt, u64* __restrict__ moves) {
    u32 moved = 0;
    const u32 one = tries > kSubsetTries ? *only : kNone;
    for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < n; v += (int64_t)gridDim.x * 256) {
        u32 c = comm[v];
        const u32 p = prop[v];
        if (p != kNone && chosen((u32)v, tries, salt, one)) {
            c = p;
            moved++;
        }
        comm_try[v] = c;
        atomicAdd((u64*)&tot[c], (u64)mass[v]);
        atomicAdd(&cnt[c], 1u);
    }
    if (moved) atomicAdd(moves, (u64)moved);
}

// the node with the largest gain (ties: the smallest node), in two integer-atomic steps
__device__ __forceinline__ u64 gain_bits(double g) { return (u64)__double_as_longlong(g); }  // gains here are >= 0: ordered as integers
__global__ __launch_bounds__(256) void best_gain_kernel(const u32* __restrict__ prop, const double* __restrict__ pgain, int64_t n, u64* __restrict__ best) {
    for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < n; v += (int64_t)gridDim.x * 256)
        if (prop[v] != kNone) atomicMax(best, gain_bits(pgain[v]));
}
__global__ __launch_bounds__(256) void best_node_kernel(const u32* __restrict__ prop, const double* __restrict__ pgain, int64_t n, const u64* __restrict__ best,
                                                        u32* __restrict__ node) {
    const u64 want = *best;
    for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < n; v += (int64_t)gridDim.x * 256)
        if (prop[v] != kNone && gain_bits(pgain[v]) == want) atomicMin(node, (u32)v);
}

// twice the weight inside the communities of `label` (self-loop entries included), as an integer
__global__ __launch_bounds__(256) void inner_weight_kernel(const Level L, const u32* __restrict__ label, u64* __restrict__ inner2) {
    const int lane = threadIdx.x & 63;
    const int64_t waves = (int64_t)gridDim.x * 4;
    i64 s = 0;
    for (int64_t v = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); v < L.n; v += waves) {
        const u32 b = L.offs[v], e = L.offs[v + 1], c = label[v];
        for (u32 t = b + lane; t < e; t += 64)
            if (label[(u32)L.keys[t]] == c) s += L.w[t];
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    if (lane == 0 && s) atomicAdd(inner2, (u64)s);
}

// sum over labels of A^2 (degree mass) or A (A - 1) (node-count mass), A in the mass's unit; or, with `cnt`, the number
// of labels in use as a sum of ones, which float64 holds exactly (a mode of this sum and not a kernel of its own: the
// committed PMC summaries are tied to the set of kernel symbols)
struct PenaltySum {
    const i64* tot;
    double mscale;
    int by_count;
    const u32* cnt;
    __device__ double operator()(int64_t c) const {
        if (cnt) return cnt[c] != 0u ? 1.0 : 0.0;
        const double A = (double)tot[c] * mscale;
        return by_count ? A * (A - 1.0) : A * A;
    }
};

// ---- refinement
__global__ __launch_bounds__(256) void refine_init_kernel(const i64* __restrict__ mass, int64_t n, u32* __restrict__ part, i64* __restrict__ ptot,
                                                          u32* __restrict__ pcnt) {
    for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < n; v += (int64_t)gridDim.x * 256) {
        part[v] = (u32)v;
        ptot[v] = mass[v];
        pcnt[v] = 1u;
    }
}
__global__ __launch_bounds__(256) void fill_u32_kernel(u32* __restrict__ x, int64_t n, u32 v) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) x[i] = v;
}
__global__ __launch_bounds__(256) void refine_apply_kernel(const u32* __restrict__ rprop, const u32* __restrict__ target, const i64* __restrict__ mass,
                                                           int64_t n, u32* __restrict__ part, i64* __restrict__ ptot, u32* __restrict__ pcnt,
                                                           u64* __restrict__ moves) {
    u32 moved = 0;
    for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < n; v += (int64_t)gridDim.x * 256) {
        const u32 p = rprop[v];
        if (p == kNone || target[v]) continue;  // somebody's target stays, so that what joins it stays connected to it
        part[v] = p;
        atomicAdd((u64*)&ptot[p], (u64)mass[v]);
        atomicAdd(&pcnt[p], 1u);
        moved++;
    }
    if (moved) atomicAdd(moves, (u64)moved);
}

// ---- aggregation
__global__ __launch_bounds__(256) void mark_kernel(const u32* __restrict__ label, int64_t n, u32* __restrict__ used) {
    for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < n; v += (int64_t)gridDim.x * 256) used[label[v]] = 1u;
}
__global__ __launch_bounds__(256) void collapse_nodes_kernel(const u32* __restrict__ part, const u32* __restrict__ comm, const i64* __restrict__ mass,
                                                             const u32* __restrict__ newid, const u32* __restrict__ cid, int64_t n,
                                                             i64* __restrict__ mass_new, u32* __restrict__ comm_new) {
    for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < n; v += (int64_t)gridDim.x * 256) {
        const u32 p = newid[part[v]];
        atomicAdd((u64*)&mass_new[p], (u64)mass[v]);
        comm_new[p] = cid[comm[v]];  // every member of a part is in the same community: the same value from each
    }
}
__global__ __launch_bounds__(256) void remap_kernel(u32* __restrict__ map0, int64_t n0, const u32* __restrict__ part, const u32* __restrict__ newid) {
    for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < n0; v += (int64_t)gridDim.x * 256) map0[v] = newid[part[map0[v]]];
}
__global__ __launch_bounds__(256) void collapse_edges_kernel(const u64* __restrict__ keys, int64_t ne, const u32* __restrict__ part,
                                                             const u32* __restrict__ newid, u64* __restrict__ out) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < ne; e += (int64_t)gridDim.x * 256) {
        const u64 k = keys[e];
        out[e] = ((u64)newid[part[(u32)(k >> 32)]] << 32) | newid[part[(u32)k]];
    }
}
__global__ __launch_bounds__(256) void heads_kernel(const u64* __restrict__ keys, int64_t ne, u32* __restrict__ head /* [ne + 1] */) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e <= ne; e += (int64_t)gridDim.x * 256)
        head[e] = e < ne && (e == 0 || keys[e] != keys[e - 1]) ? 1u : 0u;
}
__global__ __launch_bounds__(256) void merge_equal_kernel(const u64* __restrict__ keys, const i64* __restrict__ w, const u32* __restrict__ pos,
                                                          int64_t ne, u64* __restrict__ keys_out, i64* __restrict__ w_out) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < ne; e += (int64_t)gridDim.x * 256) {
        const u32 p = pos[e + 1] - 1;  // pos: heads before e; the run of e is the number of heads up to and including e, less one
        if (pos[e + 1] != pos[e]) keys_out[p] = keys[e];  // the head of a run of equal keys
        atomicAdd((u64*)&w_out[p], (u64)w[e]);
    }
}

// ---- the answer: numbering by size and the float64 quality
__global__ __launch_bounds__(256) void final_label_kernel(const u32* __restrict__ label, const u32* __restrict__ map0, int64_t n0, u32* __restrict__ lab0,
                                                          u32* __restrict__ size, u32* __restrict__ minnode) {
    for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < n0; v += (int64_t)gridDim.x * 256) {
        const u32 c = label[map0[v]];
        lab0[v] = c;
        atomicAdd(&size[c], 1u);
        atomicMin(&minnode[c], (u32)v);
    }
}
__global__ __launch_bounds__(256) void community_keys_kernel(const u32* __restrict__ size, const u32* __restrict__ minnode, const u32* __restrict__ pos,
                                                             int64_t nlabels, u32 n0, u64* __restrict__ keys, i64* __restrict__ pay) {
    for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c < nlabels; c += (int64_t)gridDim.x * 256) {
        if (!size[c]) continue;
        keys[pos[c]] = ((u64)(n0 - size[c]) << 32) | minnode[c];  // larger first, then the smaller first node
        pay[pos[c]] = c;
    }
}
__global__ __launch_bounds__(256) void rank_kernel(const i64* __restrict__ pay, const u32* __restrict__ size, int64_t nc, u32* __restrict__ rank,
                                                   u32* __restrict__ csize /* [nc + 1] */) {
    for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r <= nc; r += (int64_t)gridDim.x * 256) {
        if (r == nc) {
            csize[r] = 0u;
            continue;
        }
        const u32 c = (u32)pay[r];
        rank[c] = (u32)r;
        csize[r] = size[c];
    }
}
__global__ __launch_bounds__(256) void membership_kernel(const u32* __restrict__ lab0, const u32* __restrict__ rank, int64_t n0, u32* __restrict__ mem,
                                                         u64* __restrict__ keys, i64* __restrict__ pay) {
    for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < n0; v += (int64_t)gridDim.x * 256) {
        const u32 r = rank[lab0[v]];
        mem[v] = r;
        keys[v] = r;
        pay[v] = v;
    }
}
// float64 degree sum of every community over its nodes in ascending order (fixed lane stride + shuffle tree)
__global__ __launch_bounds__(256) void community_degree_kernel(const i64* __restrict__ nodes, const u32* __restrict__ cstart, int64_t nc,
                                                               const double* __restrict__ deg0, double* __restrict__ kc) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= nc) return;
    double s = 0.0;
    for (u32 t = cstart[r] + lane; t < cstart[r + 1]; t += 64) s += deg0[nodes[t]];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    if (lane == 0) kc[r] = s;
}
struct InnerSum {
    const u32 *rows, *cols, *mem;
    const float* vals;
    __device__ double operator()(int64_t e) const { return mem[rows[e]] == mem[cols[e]] ? (double)vals[e] : 0.0; }
};
struct FinalPenalty {
    const double* kc;
    const u32* cstart;
    int quality;
    double m, p;
    __device__ double operator()(int64_t r) const {
        const double nc = (double)(cstart[r + 1] - cstart[r]);
        if (quality <= 1) return kc[r] * kc[r] / (4.0 * m);
        return (quality == 2 ? p : 1.0) * (nc * (nc - 1.0) / 2.0);
    }
};

// ---- host side
struct Carver {
    size_t off = 0;
    size_t take(size_t bytes) {
        const size_t at = off;
        off = (off + bytes + 255) & ~(size_t)255;
        return at;
    }
};

struct Sorter {
    skr_ctx* ctx;
    u64* kbuf[2];
    i64* pbuf[2];
    u32 *table, *scan_scratch;
    int cur = 0;
    // stable sort of the n items in buffer `cur` by the key bits [lo_bits) and [32, 32 + hi_bits); result in buffer `cur`
    int run(int64_t n, int lo_bits, int hi_bits) {
        if (n <= 1) return SKR_OK;
        const skr_radix::Chunks plan = skr_radix::plan_chunks(ctx, n);
        for (int field = 0; field < 2; field++) {
            const int bits = field ? hi_bits : lo_bits;
            for (int s = 0; s < bits; s += 8) {
                const LPass lp{kbuf[cur], pbuf[cur], kbuf[cur ^ 1], pbuf[cur ^ 1], 32 * field + s};
                SKR_TRY(skr_radix::run_pass(ctx, lp, n, plan, table, scan_scratch));
                cur ^= 1;
            }
        }
        return SKR_OK;
    }
};

thread_local int g_converged = 1;
thread_local int64_t g_sweeps = 0;

// ---- the trace (skr_leiden_trace): host code only.  While it is on, the driver appends one record of kTraceWords
// uint64 words after every proposal pass of local moving, every refinement round and every measured sweep; the
// arrays a proposal wrote are copied to the host and hashed there.  Off (the default) nothing below runs.
constexpr int kTraceWords = 8;
constexpr u64 kTracePropose = 1, kTraceRefine = 2, kTraceSweep = 3;
struct Trace {
    bool on = false;
    int64_t dump = -1;           // the record whose arrays are kept whole
    std::vector<uint64_t> words;
    std::vector<unsigned char> a, b;  // of record `dump`: prop, and pgain (local moving) or target (refinement)
};
thread_local Trace g_trace;

uint64_t fnv1a64(const unsigned char* p, size_t bytes) {
    uint64_t h = 0xcbf29ce484222325ull;
    for (size_t i = 0; i < bytes; i++) h = (h ^ p[i]) * 0x100000001b3ull;
    return h;
}

// one record that hashes two device arrays: copies them on the stream, waits, hashes.  head: the words before the hashes
int trace_arrays(hipStream_t st, const uint64_t* head, int n_head, const void* d_a, size_t bytes_a, const void* d_b, size_t bytes_b,
                 uint64_t tail) {
    Trace& T = g_trace;
    std::vector<unsigned char> a(bytes_a), b(bytes_b);
    if (bytes_a) SKR_HIP(hipMemcpyAsync(a.data(), d_a, bytes_a, hipMemcpyDeviceToHost, st));
    if (bytes_b) SKR_HIP(hipMemcpyAsync(b.data(), d_b, bytes_b, hipMemcpyDeviceToHost, st));
    SKR_HIP(hipStreamSynchronize(st));
    uint64_t rec[kTraceWords] = {0};
    for (int i = 0; i < n_head; i++) rec[i] = head[i];
    rec[n_head] = fnv1a64(a.data(), bytes_a);
    rec[n_head + 1] = fnv1a64(b.data(), bytes_b);
    rec[n_head + 2] = tail;
    if ((int64_t)(T.words.size() / kTraceWords) == T.dump) {
        T.a.swap(a);
        T.b.swap(b);
    }
    T.words.insert(T.words.end(), rec, rec + kTraceWords);
    return SKR_OK;
}

}  // namespace

extern "C" int skr_leiden_trace(int on, int64_t dump_record) {
    g_trace.on = on != 0;
    g_trace.dump = on ? dump_record : -1;
    g_trace.words.clear();
    g_trace.a.clear();
    g_trace.b.clear();
    return SKR_OK;
}

extern "C" int skr_leiden_trace_read(uint64_t* out, int64_t capacity, int64_t* words) {
    SKR_REQUIRE(words && capacity >= 0 && (out || capacity == 0), "NULL argument");
    *words = (int64_t)g_trace.words.size();
    if (capacity >= *words && *words) memcpy(out, g_trace.words.data(), (size_t)*words * 8);
    return SKR_OK;
}

extern "C" int skr_leiden_trace_dump(void* a, int64_t capacity_a, void* b, int64_t capacity_b, int64_t* bytes_a, int64_t* bytes_b) {
    SKR_REQUIRE(bytes_a && bytes_b && capacity_a >= 0 && capacity_b >= 0, "NULL argument");
    *bytes_a = (int64_t)g_trace.a.size();
    *bytes_b = (int64_t)g_trace.b.size();
    if (a && capacity_a >= *bytes_a && *bytes_a) memcpy(a, g_trace.a.data(), (size_t)*bytes_a);
    if (b && capacity_b >= *bytes_b && *bytes_b) memcpy(b, g_trace.b.data(), (size_t)*bytes_b);
    return SKR_OK;
}

extern "C" int skr_leiden_last(int* converged, int64_t* sweeps) {
    if (converged) *converged = g_converged;
    if (sweeps) *sweeps = g_sweeps;
    return SKR_OK;
}

extern "C" int skr_leiden_limits(int* wave_degree, int* lds_degree) {
    if (wave_degree) *wave_degree = kWaveDeg;
    if (lds_degree) *lds_degree = kLdsDeg;
    return SKR_OK;
}

extern "C" int skr_leiden_table_groups(skr_ctx* ctx, int* groups) {
    SKR_REQUIRE(ctx && groups, "NULL argument");
    *groups = ctx->num_cu * 2;
    return SKR_OK;
}

extern "C" int skr_leiden(skr_ctx* ctx, const skr_mat* rows, const skr_mat* cols, const skr_mat* vals, int64_t n_edges, int64_t n_nodes,
                          int quality, double resolution, int max_levels, int max_sweeps, skr_mat* membership, double* quality_out,
                          int64_t* n_communities, int64_t* levels_run) {
    SKR_REQUIRE(ctx && membership && quality_out && n_communities && levels_run, "NULL argument");
    SKR_REQUIRE(n_edges >= 0 && n_nodes >= 0, "negative size");
    SKR_REQUIRE(n_edges == 0 || (rows && cols && vals), "NULL edge list");
    SKR_REQUIRE(quality >= 0 && quality <= 3, "quality is 0 (RBConfiguration), 1 (Modularity), 2 (RBER) or 3 (CPM)");
    SKR_REQUIRE(resolution >= 0.0 && resolution <= 1e300, "resolution must be a finite number >= 0");
    SKR_REQUIRE(max_levels >= 1 && max_sweeps >= 1, "max_levels and max_sweeps are at least 1");
    SKR_REQUIRE(membership->ctx == ctx && membership->dtype == SKR_U32 && membership->rows * membership->cols >= n_nodes,
                "membership is a 32-bit integer matrix of at least n_nodes cells");
    if (n_edges) {
        SKR_REQUIRE(rows->ctx == ctx && cols->ctx == ctx && vals->ctx == ctx, "handle belongs to a different ctx");
        SKR_REQUIRE(rows->dtype == SKR_U32 && cols->dtype == SKR_U32 && vals->dtype == SKR_F32, "the edge list is U32, U32, F32");
        SKR_REQUIRE(rows->rows * rows->cols >= n_edges && cols->rows * cols->cols >= n_edges && vals->rows * vals->cols >= n_edges,
                    "the edge list holds fewer than n_edges entries");
    }
    SKR_REQUIRE(n_nodes <= (1LL << 30) && 2 * n_edges + 2 * n_nodes < (1LL << 31), "at most 2^30 nodes and 2^30 edges");
    SKR_TRY(skr_activate(ctx));
    const double gamma = quality == 1 ? 1.0 : resolution;
    *quality_out = 0.0;
    *n_communities = n_nodes;
    *levels_run = 0;
    g_converged = 1;
    g_sweeps = 0;
    if (n_nodes == 0) return SKR_OK;
    const int64_t n0 = n_nodes, E2 = 2 * n_edges, NL = 2 * n0;  // labels of a level: 2 n
    hipStream_t st = ctx->stream;
    if (n_edges == 0) {  // every node alone: sizes tie, so the numbering is the node order; every function gives 0
        hipLaunchKernelGGL(iota_kernel, dim3(skr_grid(ctx, n0)), dim3(256), 0, st, (u32*)membership->data, n0);
        SKR_HIP(hipGetLastError());
        SKR_HIP(hipStreamSynchronize(st));
        return SKR_OK;
    }

    const u32 *e_rows = (const u32*)rows->data, *e_cols = (const u32*)cols->data;
    const float* e_vals = (const float*)vals->data;
    u64 h_small[16];
#define LAUNCH(kern, items, ...)                                                                        \
    do {                                                                                                \
        hipLaunchKernelGGL(kern, dim3(skr_grid(ctx, (items))), dim3(256), 0, st, __VA_ARGS__);          \
        SKR_HIP(hipGetLastError());                                                                     \
    } while (0)
#define WAVE_GRID(items) dim3((unsigned)(((items) + 3) / 4))

    // ---- before anything is kept: the input check, the total weight and the largest degree (which sizes the tables
    // of the device-memory work unit), in a small workspace of their own
    double m_total = 0.0;
    u32 maxdeg0 = 0;
    {
        Carver pc;
        const size_t o_s = pc.take(256), o_deg = pc.take((size_t)n0 * 4), o_par = pc.take((size_t)(n_edges / 4096 + 2) * 8);
        void* pws = nullptr;
        SKR_TRY(skr_ctx_workspace(ctx, pc.off, &pws));
        u64* ps = (u64*)((char*)pws + o_s);  // [0] sum  u32 view from [1]: bad flags, largest degree
        u32* deg = (u32*)((char*)pws + o_deg);
        SKR_HIP(hipMemsetAsync(pws, 0, o_deg + (size_t)n0 * 4, st));
        LAUNCH(validate_degree_kernel, n_edges, e_rows, e_cols, e_vals, n_edges, (u32)n0, deg, (u32*)(ps + 1));
        LAUNCH(max_u32_kernel, n0, (const u32*)deg, n0, (u32*)(ps + 1) + 1);
        SKR_TRY(det_sum(ctx, ValSum{e_vals}, n_edges, (double*)((char*)pws + o_par), (double*)ps));
        SKR_HIP(hipMemcpyAsync(h_small, ps, 16, hipMemcpyDeviceToHost, st));
        SKR_HIP(hipStreamSynchronize(st));
        const u32 bad = (u32)h_small[1];
        maxdeg0 = (u32)(h_small[1] >> 32);
        if (bad & 4u) return skr_set_error(SKR_ERR_INVALID, "an edge names a node >= n_nodes (%lld)", (long long)n0);
        if (bad & 1u) return skr_set_error(SKR_ERR_INVALID, "the edge list must be the upper triangle: row < col for every edge");
        if (bad & 2u) return skr_set_error(SKR_ERR_INVALID, "edge weights must be positive finite numbers (found zero, negative, NaN or infinite)");
        memcpy(&m_total, &h_small[0], 8);
        SKR_REQUIRE(m_total > 0.0 && m_total < 1e300, "the total edge weight is not a positive finite number");
    }
    // fixed point: (2 m + 2) 2^F stays below 2^60
    const int frac = std::min(kMaxFrac, 60 - (int)std::ceil(std::log2(2.0 * m_total + 2.0)));
    SKR_REQUIRE(frac >= 8, "the total edge weight is too large for the fixed-point totals");
    // tables in device memory: a node of any level has at most min(n, entries) neighbours, so one table of that size is
    // always reserved when that exceeds the LDS table; level 0's largest degree says how many tables are worth having
    auto slots_for = [](uint64_t degree) { return (size_t)1 << skr_radix::bit_length(2 * (degree + 1)); };  // more than twice the keys
    size_t tab_bytes = 0;
    if (std::min(n0, E2) > kLdsDeg) tab_bytes = slots_for((uint64_t)std::min(n0, E2)) * 12;
    if (maxdeg0 > (u32)kLdsDeg)
        tab_bytes = std::max(tab_bytes, std::min<size_t>((size_t)ctx->num_cu * 2 * slots_for(maxdeg0) * 12, (size_t)1 << 30));

    // ---- workspace
    const int64_t cap = std::max(E2, NL) + 1;
    Carver cv;
    const size_t o_small = cv.take(256);
    const size_t o_k0 = cv.take((size_t)cap * 8), o_k1 = cv.take((size_t)cap * 8), o_p0 = cv.take((size_t)cap * 8), o_p1 = cv.take((size_t)cap * 8);
    const size_t table_words = skr_radix::max_table_words(ctx, cap);
    const size_t o_table = cv.take((table_words + skr_radix::scan_scratch_words((int64_t)table_words) + 16) * 4);
    const size_t o_pos = cv.take((size_t)(cap + 1) * 4);
    const size_t o_scan = cv.take((skr_radix::scan_scratch_words(cap + 1) + 16) * 4);
    const size_t o_partials = cv.take((size_t)(cap / 4096 + 2) * 8);
    const size_t o_offs = cv.take((size_t)(n0 + 2) * 4);
    size_t o_u32[12];
    for (size_t& o : o_u32) o = cv.take((size_t)(n0 + 2) * 4);
    const size_t o_cid = cv.take((size_t)(NL + 2) * 4), o_cnt0 = cv.take((size_t)(NL + 2) * 4), o_cnt1 = cv.take((size_t)(NL + 2) * 4);
    const size_t o_rank = cv.take((size_t)(NL + 2) * 4), o_minnode = cv.take((size_t)(NL + 2) * 4);
    const size_t o_tot0 = cv.take((size_t)(NL + 2) * 8), o_tot1 = cv.take((size_t)(NL + 2) * 8);
    const size_t o_mass0 = cv.take((size_t)n0 * 8), o_mass1 = cv.take((size_t)n0 * 8), o_ptot = cv.take((size_t)n0 * 8);
    const size_t o_pgain = cv.take((size_t)n0 * 8), o_deg0 = cv.take((size_t)n0 * 8), o_kc = cv.take((size_t)n0 * 8);
    const size_t o_tab = cv.take(tab_bytes);
    void* ws = nullptr;
    SKR_TRY(skr_ctx_workspace(ctx, cv.off, &ws));
    char* base = (char*)ws;
    char* tab_base = base + o_tab;
    u64* d_small = (u64*)(base + o_small);  // [0] moves  [1] inner2  [2] best gain  [3..4] doubles  [5] labels in use  u32 view from [8]
    u32* d_small32 = (u32*)(d_small + 8);   // [0] bad flags [1] best node [2..4] class counters
    double* d_dbl = (double*)(d_small + 3);
    Sorter so{ctx, {(u64*)(base + o_k0), (u64*)(base + o_k1)}, {(i64*)(base + o_p0), (i64*)(base + o_p1)}, (u32*)(base + o_table), nullptr};
    so.scan_scratch = so.table + table_words;
    u32* d_pos = (u32*)(base + o_pos);
    u32* d_scan = (u32*)(base + o_scan);
    double* d_partials = (double*)(base + o_partials);
    u32* d_offs = (u32*)(base + o_offs);
    u32* un[12];
    for (int i = 0; i < 12; i++) un[i] = (u32*)(base + o_u32[i]);
    u32 *d_comm = un[0], *d_comm_try = un[1], *d_prop = un[2], *d_part = un[3], *d_target = un[4], *d_list_blk = un[5], *d_list_glb = un[6];
    u32 *d_newid = un[7], *d_comm_new = un[8], *d_map0 = un[9], *d_pcnt = un[10], *d_lab0 = un[11];
    u32 *d_cid = (u32*)(base + o_cid), *d_cnt = (u32*)(base + o_cnt0), *d_cnt_try = (u32*)(base + o_cnt1);
    u32 *d_rank = (u32*)(base + o_rank), *d_minnode = (u32*)(base + o_minnode);
    i64 *d_tot = (i64*)(base + o_tot0), *d_tot_try = (i64*)(base + o_tot1);
    i64 *d_mass = (i64*)(base + o_mass0), *d_mass_new = (i64*)(base + o_mass1), *d_ptot = (i64*)(base + o_ptot);
    double *d_pgain = (double*)(base + o_pgain), *d_deg0 = (double*)(base + o_deg0), *d_kc = (double*)(base + o_kc);
    // ---- CSR of level 0
    {
        SkrProfScope prof(ctx, "leiden_sort");
        SKR_HIP(hipMemsetAsync(d_small, 0, 256, st));
        LAUNCH(mirror_kernel, n_edges, e_rows, e_cols, e_vals, n_edges, so.kbuf[0], so.pbuf[0]);
        so.cur = 0;
        const int nbits = std::max(1, skr_radix::bit_length((uint64_t)(n0 - 1)));
        SKR_TRY(so.run(E2, nbits, nbits));
        SKR_HIP(hipMemsetAsync(d_offs, 0, (size_t)(n0 + 2) * 4, st));
        LAUNCH(src_count_kernel, E2, so.kbuf[so.cur], E2, d_offs);
        SKR_TRY(skr_radix::exclusive_scan<u32>(ctx, d_offs, n0 + 1, d_scan));
        hipLaunchKernelGGL(degree0_kernel, WAVE_GRID(n0), dim3(256), 0, st, (const u32*)d_offs, so.pbuf[so.cur], n0, std::ldexp(1.0, frac), d_deg0, d_mass);
        SKR_HIP(hipGetLastError());
        if (quality >= 2) LAUNCH(fill_i64_kernel, n0, d_mass, n0, (i64)1);  // mass = node count
        LAUNCH(iota_kernel, n0, d_comm, n0);
        LAUNCH(iota_kernel, n0, d_map0, n0);
    }
    const double wscale = std::ldexp(1.0, -frac);
    const double p_er = m_total / ((double)n0 * (double)(n0 - 1) / 2.0);
    Level L;
    L.n = n0;
    L.offs = d_offs;
    L.wscale = wscale;
    L.mscale = quality >= 2 ? 1.0 : wscale;
    L.gp = quality <= 1 ? gamma / (2.0 * m_total) : (quality == 2 ? gamma * p_er : gamma);
    const double pen_half = 0.5 * L.gp;  // quality of a labelling = inner2 * wscale / 2 - pen_half * PenaltySum
    int64_t ne = E2;
    bool converged = true, all_single = false, have_parts = false;
    int levels = 0;
    int64_t sweeps_run = 0;
    u32 tab_slots = 0, tab_groups = 0;

    // the proposal pass over all three work units
    u32 n_blk = 0, n_glb = 0;
    auto propose = [&](const Propose& P) -> int {
        hipLaunchKernelGGL(propose_wave_kernel, WAVE_GRID(L.n), dim3(256), 0, st, L, P);
        SKR_HIP(hipGetLastError());
        if (n_blk) {
            hipLaunchKernelGGL(propose_block_kernel, dim3(n_blk), dim3(256), 0, st, L, P, (const u32*)d_list_blk);
            SKR_HIP(hipGetLastError());
        }
        if (n_glb) {
            hipLaunchKernelGGL(propose_global_kernel, dim3(std::min(n_glb, tab_groups)), dim3(256), 0, st, L, P, (const u32*)d_list_glb, n_glb,
                               (u32*)tab_base, (u64*)(tab_base + (size_t)tab_groups * tab_slots * 4), tab_slots);
            SKR_HIP(hipGetLastError());
        }
        return SKR_OK;
    };
    // quality pieces of (label, tot) -> host
    auto measure = [&](const u32* label, const i64* tot, const u32* cnt, u64* moves_out, double* q_out, u64* used_out) -> int {
        SKR_HIP(hipMemsetAsync(d_small + 1, 0, 8, st));
        hipLaunchKernelGGL(inner_weight_kernel, dim3(std::max<unsigned>(1, std::min<int64_t>((L.n + 3) / 4, (int64_t)ctx->num_cu * 8))), dim3(256), 0, st,
                           L, label, d_small + 1);
        SKR_HIP(hipGetLastError());
        SKR_TRY(det_sum(ctx, PenaltySum{tot, L.mscale, quality >= 2, nullptr}, 2 * L.n, d_partials, d_dbl));
        SKR_TRY(det_sum(ctx, PenaltySum{nullptr, 1.0, 0, cnt}, 2 * L.n, d_partials, d_dbl + 2));
        SKR_HIP(hipMemcpyAsync(h_small, d_small, 128, hipMemcpyDeviceToHost, st));  // the one small download of a sweep
        SKR_HIP(hipStreamSynchronize(st));
        double pen;
        memcpy(&pen, &h_small[3], 8);
        *moves_out = h_small[0];
        double used;
        memcpy(&used, &h_small[5], 8);
        *used_out = (u64)used;
        *q_out = (double)(i64)h_small[1] * wscale * 0.5 - pen_half * pen;
        return SKR_OK;
    };
    auto refine = [&]() -> int {
        SkrProfScope prof(ctx, "leiden_refine");
        LAUNCH(refine_init_kernel, L.n, L.mass, L.n, d_part, d_ptot, d_pcnt);
        const Propose P{d_part, d_ptot, d_pcnt, d_comm, d_target, d_prop, nullptr, 1, 0};
        for (int round = 0; round < max_sweeps; round++) {
            LAUNCH(fill_u32_kernel, L.n, d_target, L.n, 0u);
            LAUNCH(fill_u32_kernel, L.n, d_prop, L.n, kNone);
            SKR_HIP(hipMemsetAsync(d_small, 0, 8, st));
            SKR_TRY(propose(P));
            LAUNCH(refine_apply_kernel, L.n, (const u32*)d_prop, (const u32*)d_target, L.mass, L.n, d_part, d_ptot, d_pcnt, d_small);
            SKR_HIP(hipMemcpyAsync(h_small, d_small, 8, hipMemcpyDeviceToHost, st));
            SKR_HIP(hipStreamSynchronize(st));
            if (g_trace.on) {  // prop and target are what this round's proposals wrote: the apply kernel only reads them
                const uint64_t head[5] = {kTraceRefine, (uint64_t)(levels - 1), (uint64_t)L.n, n_blk, n_glb};
                SKR_TRY(trace_arrays(st, head, 5, d_prop, (size_t)L.n * 4, d_target, (size_t)L.n * 4, h_small[0]));
            }
            if (h_small[0] == 0) break;
        }
        have_parts = true;
        return SKR_OK;
    };

    for (;;) {
        L.keys = so.kbuf[so.cur];
        L.w = so.pbuf[so.cur];
        L.mass = d_mass;
        have_parts = false;
        // ---- local moving
        {
            SkrProfScope prof(ctx, "leiden_move");
            SKR_HIP(hipMemsetAsync(d_small32 + 2, 0, 12, st));
            LAUNCH(classify_kernel, L.n, L.offs, L.n, d_list_blk, d_list_glb, d_small32 + 2);
            SKR_HIP(hipMemsetAsync(d_tot, 0, (size_t)(2 * L.n) * 8, st));
            SKR_HIP(hipMemsetAsync(d_cnt, 0, (size_t)(2 * L.n) * 4, st));
            LAUNCH(totals_kernel, L.n, (const u32*)d_comm, L.mass, L.n, d_tot, d_cnt);
            SKR_HIP(hipMemsetAsync(d_small, 0, 8, st));
            u64 moves = 0, used_cur = 0, used_try = 0;
            double q_cur = 0.0;
            SKR_TRY(measure(d_comm, d_tot, d_cnt, &moves, &q_cur, &used_cur));
            n_blk = (u32)(h_small[9] & 0xffffffffu);  // d_small32[2]
            n_glb = (u32)(h_small[9] >> 32);          // d_small32[3]
            const u32 maxdeg = (u32)(h_small[10] & 0xffffffffu);
            if (n_glb) {
                const size_t per = slots_for(maxdeg) * 12;
                SKR_REQUIRE(per <= tab_bytes, "internal: a node has more neighbours than the reserved table holds");
                tab_slots = (u32)slots_for(maxdeg);
                tab_groups = (u32)std::min<size_t>({(size_t)n_glb, (size_t)ctx->num_cu * 2, tab_bytes / per});
            }
            levels++;
            int tries = 0;
            bool proposed = false, quiet = false;
            for (int sweep = 0; sweep < max_sweeps; sweep++) {
                if (!proposed) {
                    const Propose P{d_comm, d_tot, d_cnt, nullptr, nullptr, d_prop, d_pgain, 0, levels > 1};
                    SKR_TRY(propose(P));
                    proposed = true;
                    if (g_trace.on) {
                        const uint64_t head[5] = {kTracePropose, (uint64_t)(levels - 1), (uint64_t)L.n, n_blk, n_glb};
                        SKR_TRY(trace_arrays(st, head, 5, d_prop, (size_t)L.n * 4, d_pgain, (size_t)L.n * 8, 0));
                    }
                }
                if (tries > kSubsetTries) {
                    SKR_HIP(hipMemsetAsync(d_small + 2, 0, 8, st));
                    SKR_HIP(hipMemsetAsync(d_small32 + 1, 0xff, 4, st));
                    LAUNCH(best_gain_kernel, L.n, (const u32*)d_prop, (const double*)d_pgain, L.n, d_small + 2);
                    LAUNCH(best_node_kernel, L.n, (const u32*)d_prop, (const double*)d_pgain, L.n, (const u64*)(d_small + 2), d_small32 + 1);
                }
                SKR_HIP(hipMemsetAsync(d_small, 0, 8, st));
                SKR_HIP(hipMemsetAsync(d_tot_try, 0, (size_t)(2 * L.n) * 8, st));
                SKR_HIP(hipMemsetAsync(d_cnt_try, 0, (size_t)(2 * L.n) * 4, st));
                LAUNCH(apply_kernel, L.n, (const u32*)d_comm, (const u32*)d_prop, L.mass, L.n, tries, (u32)(sweep * 0x9E3779B9u), (const u32*)(d_small32 + 1),
                       d_comm_try, d_tot_try, d_cnt_try, d_small);
                double q_try = 0.0;
                sweeps_run++;
                SKR_TRY(measure(d_comm_try, d_tot_try, d_cnt_try, &moves, &q_try, &used_try));
                if (g_trace.on) {
                    const bool kept = moves > 0 && (q_try > q_cur || (q_try == q_cur && used_try < used_cur));
                    uint64_t rec[kTraceWords] = {kTraceSweep, (uint64_t)(levels - 1), (uint64_t)tries, moves, 0, used_try, kept ? 1u : 0u, 0};
                    memcpy(&rec[4], &q_try, 8);
                    g_trace.words.insert(g_trace.words.end(), rec, rec + kTraceWords);
                }
                if (moves == 0 && tries == 0) {  // nobody wants to move
                    quiet = true;
                    break;
                }
                // kept: the quality rose, or (a tie of an aggregate) it is the same with fewer communities; either way
                // (quality, -communities) rises strictly, so no state comes back
                if (moves > 0 && (q_try > q_cur || (q_try == q_cur && used_try < used_cur))) {
                    std::swap(d_comm, d_comm_try);
                    std::swap(d_tot, d_tot_try);
                    std::swap(d_cnt, d_cnt_try);
                    q_cur = q_try;
                    used_cur = used_try;
                    tries = std::max(0, std::min(tries, kSubsetTries) - 1);
                    proposed = false;
                } else if (tries > kSubsetTries) {  // not even the best single move raises the quality in float64: done
                    quiet = true;
                    break;
                } else {
                    tries++;  // the sweep is not kept: the same proposals over fewer nodes
                }
            }
            if (!quiet) converged = false;
            // communities of this level, densely numbered
            SKR_HIP(hipMemsetAsync(d_cid, 0, (size_t)(2 * L.n + 1) * 4, st));
            LAUNCH(mark_kernel, L.n, (const u32*)d_comm, L.n, d_cid);
            SKR_TRY(skr_radix::exclusive_scan<u32>(ctx, d_cid, 2 * L.n + 1, d_scan));
            u32 n_comm = 0;
            SKR_HIP(hipMemcpyAsync(&n_comm, d_cid + 2 * L.n, 4, hipMemcpyDeviceToHost, st));
            SKR_HIP(hipStreamSynchronize(st));
            all_single = (int64_t)n_comm == L.n;
        }
        if (all_single) break;  // every community is one node, and a node is a connected part of the input graph
        SKR_TRY(refine());
        if (levels >= max_levels) {
            converged = false;
            break;
        }
        // ---- aggregation
        {
            SkrProfScope prof(ctx, "leiden_aggregate");
            SKR_HIP(hipMemsetAsync(d_newid, 0, (size_t)(L.n + 1) * 4, st));
            LAUNCH(mark_kernel, L.n, (const u32*)d_part, L.n, d_newid);
            SKR_TRY(skr_radix::exclusive_scan<u32>(ctx, d_newid, L.n + 1, d_scan));
            u32 n_new = 0;
            SKR_HIP(hipMemcpyAsync(&n_new, d_newid + L.n, 4, hipMemcpyDeviceToHost, st));
            SKR_HIP(hipStreamSynchronize(st));
            if ((int64_t)n_new >= L.n) {  // nothing merged (cannot happen while a community holds two joined nodes): stop here
                converged = false;
                break;
            }
            SKR_HIP(hipMemsetAsync(d_mass_new, 0, (size_t)n_new * 8, st));
            LAUNCH(collapse_nodes_kernel, L.n, (const u32*)d_part, (const u32*)d_comm, L.mass, (const u32*)d_newid, (const u32*)d_cid, L.n, d_mass_new,
                   d_comm_new);
            LAUNCH(remap_kernel, n0, d_map0, n0, (const u32*)d_part, (const u32*)d_newid);
            // the payload stays where it is for the first pass: only the keys are rewritten, in place
            LAUNCH(collapse_edges_kernel, ne, (const u64*)so.kbuf[so.cur], ne, (const u32*)d_part, (const u32*)d_newid, so.kbuf[so.cur]);
            const int nbits = std::max(1, skr_radix::bit_length((uint64_t)(n_new - 1)));
            SKR_TRY(so.run(ne, nbits, nbits));
            LAUNCH(heads_kernel, ne + 1, (const u64*)so.kbuf[so.cur], ne, d_pos);
            SKR_TRY(skr_radix::exclusive_scan<u32>(ctx, d_pos, ne + 1, d_scan));
            u32 ne_new = 0;
            SKR_HIP(hipMemcpyAsync(&ne_new, d_pos + ne, 4, hipMemcpyDeviceToHost, st));
            SKR_HIP(hipMemsetAsync(so.pbuf[so.cur ^ 1], 0, (size_t)ne * 8, st));
            LAUNCH(merge_equal_kernel, ne, (const u64*)so.kbuf[so.cur], (const i64*)so.pbuf[so.cur], (const u32*)d_pos, ne, so.kbuf[so.cur ^ 1],
                   so.pbuf[so.cur ^ 1]);
            SKR_HIP(hipStreamSynchronize(st));
            so.cur ^= 1;
            ne = ne_new;
            SKR_HIP(hipMemsetAsync(d_offs, 0, (size_t)(n_new + 2) * 4, st));
            LAUNCH(src_count_kernel, ne, (const u64*)so.kbuf[so.cur], ne, d_offs);
            SKR_TRY(skr_radix::exclusive_scan<u32>(ctx, d_offs, (int64_t)n_new + 1, d_scan));
            std::swap(d_mass, d_mass_new);
            std::swap(d_comm, d_comm_new);
            L.n = n_new;
        }
    }

    // ---- the answer.  Not finished (a bound was reached): the refined parts, which are connected whatever the state.
    const u32* label = all_single ? d_comm : d_part;
    if (!all_single && !have_parts) SKR_TRY(refine());
    {
        SkrProfScope prof(ctx, "leiden_number");
        const int64_t nl = all_single ? 2 * L.n : L.n;
        SKR_HIP(hipMemsetAsync(d_cnt, 0, (size_t)nl * 4, st));
        SKR_HIP(hipMemsetAsync(d_minnode, 0xff, (size_t)nl * 4, st));
        LAUNCH(final_label_kernel, n0, label, (const u32*)d_map0, n0, d_lab0, d_cnt, d_minnode);
        SKR_HIP(hipMemsetAsync(d_cid, 0, (size_t)(nl + 1) * 4, st));
        LAUNCH(mark_kernel, n0, (const u32*)d_lab0, n0, d_cid);
        SKR_TRY(skr_radix::exclusive_scan<u32>(ctx, d_cid, nl + 1, d_scan));
        u32 nc = 0;
        SKR_HIP(hipMemcpyAsync(&nc, d_cid + nl, 4, hipMemcpyDeviceToHost, st));
        SKR_HIP(hipStreamSynchronize(st));
        so.cur = 0;
        LAUNCH(community_keys_kernel, nl, (const u32*)d_cnt, (const u32*)d_minnode, (const u32*)d_cid, nl, (u32)n0, so.kbuf[0], so.pbuf[0]);
        const int nbits = std::max(1, skr_radix::bit_length((uint64_t)n0));
        SKR_TRY(so.run(nc, nbits, nbits));
        u32* d_csize = d_pos;  // [nc + 1] sizes in rank order, then their starts
        LAUNCH(rank_kernel, (int64_t)nc + 1, (const i64*)so.pbuf[so.cur], (const u32*)d_cnt, (int64_t)nc, d_rank, d_csize);
        SKR_TRY(skr_radix::exclusive_scan<u32>(ctx, d_csize, (int64_t)nc + 1, d_scan));
        so.cur = 0;
        LAUNCH(membership_kernel, n0, (const u32*)d_lab0, (const u32*)d_rank, n0, (u32*)membership->data, so.kbuf[0], so.pbuf[0]);
        SKR_TRY(so.run(n0, std::max(1, skr_radix::bit_length((uint64_t)nc)), 0));
        hipLaunchKernelGGL(community_degree_kernel, WAVE_GRID((int64_t)nc), dim3(256), 0, st, (const i64*)so.pbuf[so.cur], (const u32*)d_csize, (int64_t)nc,
                           (const double*)d_deg0, d_kc);
        SKR_HIP(hipGetLastError());
        SKR_TRY(det_sum(ctx, InnerSum{e_rows, e_cols, (const u32*)membership->data, e_vals}, n_edges, d_partials, d_dbl));
        SKR_TRY(det_sum(ctx, FinalPenalty{d_kc, d_csize, quality, m_total, p_er}, (int64_t)nc, d_partials, d_dbl + 1));
        SKR_HIP(hipMemcpyAsync(h_small, d_dbl, 16, hipMemcpyDeviceToHost, st));
        SKR_HIP(hipStreamSynchronize(st));
        double inner, pen;
        memcpy(&inner, &h_small[0], 8);
        memcpy(&pen, &h_small[1], 8);
        double q = inner - gamma * pen;
        if (quality == 1) q /= m_total;
        *quality_out = q;
        *n_communities = nc;
    }
    *levels_run = levels;
    g_converged = converged ? 1 : 0;
    g_sweeps = sweeps_run;
    return SKR_OK;
#undef LAUNCH
#undef WAVE_GRID
}
