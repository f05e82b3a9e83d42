"""The kernels behind adj_pval (adjust.hip, radix.hpp) and the row-offset scan of skr_edges, at MANY sizes, key byte
patterns and both dtypes.  They choose their code path by the number of tests (the chunk rule of the radix sort, the
levels of the prefix scan, the tiles of the running max / min, the stride of the write-back search) and by the bit
pattern of the keys (a radix pass whose byte is the same in every key is skipped).  This walks those instead of listing
a few, as tools/width_sweep.py does for the widths:

  sizes       every n 1 .. 200, 64 j and 4 096 j with their neighbours, the ends of the chunk rule (512 W and 8 192 W keys,
              W = 16 waves per CU) and its stepped region in between, where n_chunks steps DOWN as n grows, last chunks
              of 1 / 63 / 64 / 65 keys, seeded random sizes; both dtypes, [r, c] / [1, n] / [n, 1], symmetric=False.  The
              two-stage methods three times: as given, scaled so that nothing is rejected (r1 = 0) and so that
              everything is (r1 = n)
  upper       symmetric [N, N] matrices (the device's own symmetry verdict, triu_flatten, the raw values already in the
              first key buffer, the [N, N] write-back) with N (N - 1) / 2 on or next to those boundaries where an N
              exists, and N in 2, 3, 33, 91, 92, 2 049, 6 001
  hommel      n around the 256-cell blocks and 16 384, one run near 10^5, with ties
  bytes       inputs whose order-preserving keys vary in exactly a chosen set of bytes (all 16 subsets for float32; each
              single byte, all, the alternating sets, the halves and none for float64): which passes run, how many (the
              ping-pong buffer the sorted keys end in), the forced single pass, tables made entirely of duplicates.
              Pass counts are not observable through the ABI: the check is that the result is right whatever was skipped
  specials    10^6 tests mixing -0.0 with +0.0, denormals, +inf, distinct negatives, distinct values above 1, and NaNs of
              several payloads with and without the sign bit (holm: exactly the NaN cells are NaN)
  symmetry    skr_pvals_symmetric at N 1 .. 70 and around 96 / 128 / 1 024 / 4 096 and 10 007: exact, garbage on the
              diagonal, and single-cell edits (large, vanishing under round(x, 5), surviving it, NaN on one or both
              sides) in every tile class
  edges scan  skr_edges' uint64 row-offset scan with nrows + 1 around 4 096 and 4 096^2 (its third level)
  large       23 171 x 23 171 float32, fdr_bh: more than 65 536 chunks of 8 192 keys, a three-level digit-table scan

The reference throughout is tests/adj_rule.py (pinned to the reference's golden bytes by tests/test_adj_pval_cpu.py),
compared by that file's assert_matches: bit-exact, sidak and holm-sidak within 4 eps.  Tied values lie only inside
[0, 1]: there the corrected value is a function of the p-value alone, so numpy's unstable argsort cannot make the
reference ambiguous (tests/test_adjust_sweep_cpu.py checks this for every generator here).  Several methods on one
vector share ONE argsort (reference_many: adj_rule.correct's own lines around adj_rule._sorted; the CPU test holds it
to adj_rule.correct bit for bit).

NOT walked: the three-level uint32 scan (an edge list above 5.4e8 entries), hommel above ~10^5 tests (the host
reference is O(n^2)), and how many passes the sort ran.

    python tools/adjust_sweep.py [--full] [--seed 1] [--cus 256] [--only sizes,bytes] [--sizes 4097,8192]
                                 [--methods holm,fdr_bh] [--no-large]

Exit code 1 and the failing cases on stderr if any check fails.  Needs a real MI355X.
"""
import argparse
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import adj_rule  # noqa: E402
from test_adj_pval_cpu import assert_matches  # noqa: E402

DTYPES = (np.float32, np.float64)
NON_HOMMEL = [m for m in adj_rule.METHODS if m != "hommel"]
LARGE_METHODS = ["holm", "fdr_bh", "fdr_gbs", "fdr_by", "fdr_tsbky"]  # forward max, backward min, both, harmonic sum, r1
TWO_STAGE = ("fdr_tsbh", "fdr_tsbky")
ALL_METHODS_UP_TO = 70000
ALPHA = 0.05
LARGE_N = 23171  # 23 171^2 = 536 895 241 tests > 65 536 chunks of 8 192

# ---- the chunk rule of radix.hpp (plan_chunks), restated: num_cu is not part of the ABI --------------------------------
K_MIN_CHUNK, K_MAX_CHUNK, WAVES_PER_CU = 512, 8192, 16
SCAN_TILE = 4096  # radix.hpp kScanTile; also adjust.hip's kAccTile and kSplit


def plan_chunks(n, cus=256):
    """(chunk, n_chunks) of radix.hpp's plan_chunks for n keys on a device of `cus` compute units."""
    w = cus * WAVES_PER_CU
    chunk = min(K_MAX_CHUNK, max(K_MIN_CHUNK, -(-n // w)))
    chunk = (chunk + 63) // 64 * 64
    return chunk, max(1, -(-n // chunk))


def scan_levels(words):
    """Levels of radix.hpp's exclusive_scan for an array of `words` elements."""
    levels = 1
    while words > SCAN_TILE:
        words = -(-words // SCAN_TILE)
        levels += 1
    return levels


def step_downs(cus=256):
    """Every n in the stepped region with n_chunks(n + 1) < n_chunks(n): the chunk grows by 64 at n = c W + 1."""
    w = cus * WAVES_PER_CU
    return [c * w for c in range(K_MIN_CHUNK, K_MAX_CHUNK, 64) if plan_chunks(c * w + 1, cus)[1] < plan_chunks(c * w, cus)[1]]


def boundary_sizes(cus=256):
    """name -> sizes: the boundaries the issue names, derived from the restated rule."""
    w = cus * WAVES_PER_CU
    downs = step_downs(cus)
    assert downs and downs[0] == K_MIN_CHUNK * w, downs[:3]
    named = {
        "scan_tile": [SCAN_TILE * j + d for j in (1, 2, 3, 16, 17, 1024, 1025) for d in (-1, 0, 1)],
        "min_chunk_end": [K_MIN_CHUNK * w + d for d in (-1, 0, 1)],
        "max_chunk_begin": [K_MAX_CHUNK * w + d for d in (-1, 0, 1)],
        # the first two steps (chunk 512 -> 576 -> 640), both sides of each: n_chunks falls from W to 3 641 / 3 687
        "step_down": [downs[0], downs[0] + 1, downs[1], downs[1] + 1],
    }
    # last chunks of 1 / 63 / 64 / 65 keys: chunk 512 (37 whole chunks before it) and chunk 576 in the stepped region
    stepped_base = 576 * (w * 549 // 576)  # a multiple of 576 whose ceil(n / W) lies in (512, 576]
    named["last_chunk"] = [512 * 37 + r for r in (1, 63, 64, 65)] + [stepped_base + r for r in (1, 63, 64, 65)]
    for n in named["last_chunk"][:4]:
        assert plan_chunks(n, cus)[0] == 512
    if cus == 256:
        for n in named["last_chunk"][4:]:
            assert plan_chunks(n, cus)[0] == 576 and (n - 1) % 576 + 1 in (1, 63, 64, 65), n
    return named


def in_stepped_region(n, cus=256):
    w = cus * WAVES_PER_CU
    return K_MIN_CHUNK * w < n < K_MAX_CHUNK * w


def sizes(quick, cus=256, seed=1):
    """The numbers of tests walked by sweep_sizes; `quick` keeps, above 70 000, the boundary neighbours only."""
    s = set(range(1, 201))
    for j in range(1, 17):
        s.update(64 * j + d for d in (-1, 0, 1))
    named = boundary_sizes(cus)
    for v in named.values():
        s.update(v)
    rng = np.random.default_rng(seed)
    s.update(int(v) for v in rng.integers(201, ALL_METHODS_UP_TO, 28 if quick else 300))
    if not quick:
        w = cus * WAVES_PER_CU
        s.update(int(v) for v in rng.integers(ALL_METHODS_UP_TO, 5_000_000, 8))
        s.update(int(v) for v in rng.integers(K_MIN_CHUNK * w, 12 * K_MIN_CHUNK * w, 3))  # more of the stepped region
    out = sorted(s)
    stepped = [n for n in out if in_stepped_region(n, cus)]
    assert len(stepped) >= 6, stepped
    assert any(n in s and n + 1 in s for n in step_downs(cus))  # n_chunks(n + 1) < n_chunks(n), both in the list
    return out


# ---- generators ---------------------------------------------------------------------------------------------------------
def mixture(rng, n, dtype):
    """Uniform values, a coarse grid (ties), exact zeros and exact ones: every tie inside [0, 1]."""
    kind = rng.random(n)
    v = rng.random(n)
    grid = rng.integers(0, 17, n) / 16.0
    v = np.where(kind < 0.30, grid, v)
    v = np.where(kind < 0.05, 0.0, v)
    v = np.where(kind > 0.95, 1.0, v)
    return v.astype(dtype)


def two_stage_variants(p):
    """name -> inputs: as given, nothing rejected (every p >= 0.5 > alpha), everything rejected (every p <= 0.04 < alpha')."""
    t = p.dtype.type
    return {"given": p, "r1=0": (t(0.5) + t(0.5) * p).astype(p.dtype), "r1=n": (p * t(0.04)).astype(p.dtype)}


def r1_of(p, method, alpha=ALPHA, order=None):
    """The first stage's number of rejections, as multipletests counts it (adj_rule._sorted)."""
    s = np.sort(p.reshape(-1)) if order is None else np.take(p.reshape(-1), order)
    n = len(s)
    alpha_prime = alpha / (1. + alpha) if method == "fdr_tsbky" else alpha
    reject = s <= (np.arange(1, n + 1) / float(n)) * alpha_prime
    return int(np.nonzero(reject)[0].max()) + 1 if reject.any() else 0


def hommel_values(rng, n, dtype):
    v = (rng.random(n) ** 4).astype(dtype)
    if n >= 8:
        v[rng.integers(0, n, max(2, n // 10))] = v[0]  # ties
        v[rng.integers(0, n, 2)] = 0
    return v


_BYTES = {  # per byte, low to high: the largest value a varying byte takes, and the value of a fixed one.  The sign bit
    # stays clear, the exponent below all-ones and the value below 1 by construction
    np.float32: (np.uint32, (0xff, 0xff, 0x7f, 0x3f), (0x5a, 0xa5, 0x2a, 0x3f)),
    np.float64: (np.uint64, (0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xef, 0x3f), (0x5a, 0xa5, 0x3c, 0xc3, 0x69, 0x96, 0xd2, 0x3f)),
}


def byte_patterns(dtype):
    """The sets of key bytes (0 = lowest) that vary."""
    if dtype == np.float32:
        return [tuple(b for b in range(4) if m >> b & 1) for m in range(16)]
    return [()] + [(b,) for b in range(8)] + [tuple(range(8)), (0, 2, 4, 6), (1, 3, 5, 7), (0, 1, 2, 3), (4, 5, 6, 7)]


def pattern_values(rng, n, dtype, varying):
    """n values of `dtype` whose bit patterns differ exactly in the bytes `varying`."""
    utype, top, fixed = _BYTES[dtype]
    bits = np.zeros(n, dtype=utype)
    for b in range(len(top)):
        if b in varying:
            col = rng.integers(0, top[b] + 1, n).astype(utype)
            col[:2] = (0, top[b])  # the byte does vary, over its whole range
        else:
            col = np.full(n, fixed[b], dtype=utype)
        bits |= col << utype(8 * b)
    return bits.view(dtype)


def keys_of(v):
    """adjust.hip's key_of_bits on the host: NaN -> all ones, +-0 -> the sign bit, negatives inverted, others | sign."""
    utype = np.uint32 if v.dtype == np.float32 else np.uint64
    u = np.ascontiguousarray(v).reshape(-1).view(utype)
    sign = utype(1) << utype(8 * u.itemsize - 1)
    inf = utype(0x7f800000) if u.itemsize == 4 else utype(0x7ff0000000000000)
    mag = u & ~sign
    k = np.where(u & sign != 0, ~u, u | sign)
    k = np.where(mag == 0, sign, k)
    return np.where(mag > inf, ~utype(0), k).astype(utype)


def varying_bytes(v):
    """The bytes in which AND and OR of the keys differ (key_bits_kernel and the wanted[] loop)."""
    k = keys_of(v)
    diff = int(np.bitwise_and.reduce(k)) ^ int(np.bitwise_or.reduce(k))
    return tuple(b for b in range(k.itemsize) if diff >> (8 * b) & 0xff)


NAN_BITS = {np.float32: (0x7fc00000, 0x7f800001, 0xffc00000, 0xff800001, 0x7fffffff, 0xffffffff, 0x7fc12345),
            np.float64: (0x7ff8000000000000, 0x7ff0000000000001, 0xfff8000000000000, 0xfff0000000000001,
                         0x7fffffffffffffff, 0xffffffffffffffff, 0x7ff8000012345678)}


def specials(rng, n, dtype, inf=False, nan=False):
    """mixture() plus -0.0 and +0.0, denormals, distinct negatives, distinct values above 1; on request ONE +inf (a
    second would be a tie above 1) and NaNs of every payload in NAN_BITS.  Returns (values, mask of the NaN cells)."""
    v = mixture(rng, n, dtype)
    assert n >= 1000
    k = min(500, n // 20)
    where = rng.permutation(n)
    seg = [where[s * k:(s + 1) * k] for s in range(5)]
    tiny = np.finfo(dtype).smallest_subnormal
    v[seg[0]] = -0.0
    v[seg[1]] = 0.0
    v[seg[2]] = tiny * rng.integers(1, 1000, k).astype(dtype)  # denormals, ties among them
    v[seg[3]] = -(np.arange(k) + 1).astype(dtype) / dtype(1024)  # distinct negatives
    v[seg[4]] = dtype(1) + (np.arange(k) + 1).astype(dtype) / dtype(128)  # distinct, above 1
    at = 5 * k
    if inf:
        v[where[at]] = np.inf
    nan_cells = np.zeros(n, dtype=bool)
    if nan:
        utype = _BYTES[dtype][0]
        cells = where[at + 1:at + 50]
        v.view(utype)[cells] = np.array(NAN_BITS[dtype], dtype=utype)[np.arange(len(cells)) % len(NAN_BITS[dtype])]
        nan_cells[cells] = True
    return v, nan_cells


# ---- the reference ------------------------------------------------------------------------------------------------------
def reference_many(p, jobs, order=None, threads=6):
    """[adj_rule.correct(p, method, alpha) for method, alpha in jobs] with ONE argsort of p: correct()'s own lines around
    adj_rule._sorted.  Long vectors: the methods side by side (numpy releases the interpreter lock).  `order`: an
    argsort the caller already has (of p, or of values p is a non-decreasing function of: with every tie inside
    [0, 1] any ascending order gives the same result)."""
    p = np.asarray(p)
    if order is None:
        order = np.argsort(p)
    s = np.take(p, order)

    def one(job):
        with np.errstate(all="ignore"):  # inf and NaN arithmetic is part of the contract (1 / (1 - 1), inf - inf)
            c = adj_rule._sorted(s, adj_rule.canonical(job[0]), float(job[1]))
        c[c > 1] = 1
        out = np.empty_like(c)
        out[order] = c
        return out

    if len(jobs) == 1 or p.size < 200000:
        return [one(j) for j in jobs]
    with ThreadPoolExecutor(max_workers=threads) as pool:
        return list(pool.map(one, jobs))


def mismatch(got, want, method, dtype):
    """None, or what assert_matches (tests/test_adj_pval_cpu.py) objects to."""
    try:
        with np.errstate(all="ignore"):
            assert_matches(got, want, method, dtype)
        return None
    except AssertionError:
        if got.dtype != want.dtype or got.shape != want.shape:
            return "%s: %s %s, want %s %s" % (method, got.dtype, got.shape, want.dtype, want.shape)
        with np.errstate(all="ignore"):
            diff = ~((got == want) | (np.isnan(got) & np.isnan(want)))
        at = np.flatnonzero(diff.reshape(-1))
        first = int(at[0]) if len(at) else -1
        return "%s: %d of %d cells differ, first at %d: %r want %r" % (
            method, len(at), got.size, first, got.reshape(-1)[first], want.reshape(-1)[first])


# ---- the device ---------------------------------------------------------------------------------------------------------
def device_adjust(v, method, alpha, symmetric):
    from seekr_amd import _lib, consumers
    d = _lib.default_context().from_numpy(v)
    try:
        out = consumers.adjust_pvalues(d, method, alpha, symmetric=symmetric)
        try:
            return np.array(out.to_numpy())
        finally:
            out.free()
    finally:
        d.free()


def shape_for(n, i):
    """[1, n], [n, 1] or the most square [r, c] with r c = n, in turn."""
    if i % 3 == 0:
        return 1, n
    if i % 3 == 1:
        return n, 1
    r = int(np.sqrt(n))
    while n % r:
        r -= 1
    return r, n // r


def check_flat(bad, key, v, jobs, alpha=ALPHA, order=None):
    """v: an [r, c] array, symmetric=False; jobs: method names.  Appends the mismatches to bad[key]."""
    wants = reference_many(v.reshape(-1), [(m, alpha) for m in jobs], order) if v.size > ALL_METHODS_UP_TO and jobs else None
    for i, m in enumerate(jobs):
        with np.errstate(all="ignore"):
            want = wants[i] if wants is not None else adj_rule.correct(v.reshape(-1), m, alpha)
        compare(bad, key, v, m, want, alpha)


def compare(bad, key, v, method, want, alpha=ALPHA):
    got = device_adjust(v, method, alpha, False)
    wrong = mismatch(got, want.reshape(v.shape), method, v.dtype)
    if wrong:
        bad.setdefault(key, []).append(wrong)
        print("%s  FAIL  %s" % (key, wrong), file=sys.stderr, flush=True)


def sweep_sizes(ns, seed=1, methods=None, verbose=True, cus=256):
    """Every n of `ns`, both dtypes, symmetric=False (see the module docstring).  Returns bad: case -> problems."""
    bad = {}
    r1_seen = {"0": set(), "n": set(), "between": set()}
    for i, n in enumerate(ns):
        want_methods = NON_HOMMEL if n <= ALL_METHODS_UP_TO else LARGE_METHODS
        if methods:
            want_methods = [m for m in want_methods if m in methods] or list(methods)
        for dtype in DTYPES:
            rng = np.random.default_rng([seed, n, np.dtype(dtype).itemsize])
            p = mixture(rng, n, dtype).reshape(shape_for(n, i))
            name = "n=%d %s %s" % (n, np.dtype(dtype).name, "x".join(map(str, p.shape)))
            # above 70 000 tests one argsort serves every method and, the variants being non-decreasing in p, all three
            order = np.argsort(p.reshape(-1)) if n > ALL_METHODS_UP_TO else None
            two = [m for m in want_methods if m in TWO_STAGE]
            tasks = [(name, p, m) for m in want_methods if m not in TWO_STAGE]
            for variant, q in two_stage_variants(p).items() if two else ():
                for m in two:
                    r1 = r1_of(q, m, order=order)
                    r1_seen["0" if r1 == 0 else "n" if r1 == n else "between"].add(n)
                    tasks.append((name + " " + variant, q, m))
            if order is None:
                for key, q, m in tasks:
                    check_flat(bad, key, q, [m])
            else:  # the host references side by side, then the device
                with ThreadPoolExecutor(max_workers=8) as pool:
                    wants = list(pool.map(lambda t: reference_many(t[1].reshape(-1), [(t[2], ALPHA)], order)[0], tasks))
                for (key, q, m), want in zip(tasks, wants):
                    compare(bad, key, q, m, want)
                del wants
        if verbose and (i % 50 == 0 or n > ALL_METHODS_UP_TO):
            print("n %9d  chunk %4d x %5d  (%d of %d)" % ((n,) + plan_chunks(n, cus) + (i + 1, len(ns))), flush=True)
    if len(ns) > 20 and not methods:  # the three outcomes of the first stage each occurred at more than one size
        for outcome, at in r1_seen.items():
            assert len(at) > 1, ("two-stage r1 %s at sizes %s only" % (outcome, sorted(at)))
    return bad


def upper_sizes(cus=256):
    """N of the upper-mode cases: N (N - 1) / 2 within one of a boundary where such an N exists, and the fixed ones."""
    ns = {2, 3, 33, 91, 92, 2049, 6001}
    targets = set()
    for v in boundary_sizes(cus).values():
        targets.update(v)
    targets.update(64 * j for j in range(1, 17))
    for t in targets:
        if t > 20_000_000:
            continue
        m = int((1 + np.sqrt(1 + 8 * t)) / 2)
        for cand in (m - 1, m, m + 1):
            if cand >= 2 and abs(cand * (cand - 1) // 2 - t) <= 1:
                ns.add(cand)
    return sorted(ns)


def symmetric_from(rng, m, dtype, gen=mixture):
    """[m, m], exactly symmetric off the diagonal (values of gen), anything on it."""
    a = np.zeros((m, m), dtype=dtype)
    iu = np.triu_indices(m, 1)
    a[iu] = gen(rng, len(iu[0]), dtype)
    a = a + a.T
    a[np.arange(m), np.arange(m)] = rng.random(m).astype(dtype) * dtype(3) - dtype(1)
    return a, iu


def check_upper(bad, key, a, iu, jobs, alpha=ALPHA):
    """a: exactly symmetric; the device decides that itself (symmetric=None) and corrects the strict upper triangle."""
    assert adj_rule.values_symmetric(a)
    m = a.shape[0]
    if m <= 100:
        wants = [adj_rule.adj_frame(a, True, j, alpha)[1] for j in jobs]
    else:  # adj_frame's symmetric branch with one argsort for all methods
        flat = reference_many(a[iu], [(j, alpha) for j in jobs])
        wants = []
        for w in flat:
            full = np.full(a.shape, np.nan)
            full[iu] = w
            wants.append(full)
    for j, want in zip(jobs, wants):
        got = device_adjust(a, j, alpha, None)
        wrong = mismatch(got, want, j, a.dtype)
        if wrong:
            bad.setdefault(key, []).append(wrong)
            print("%s  FAIL  %s" % (key, wrong), file=sys.stderr, flush=True)


def sweep_upper(seed=1, verbose=True, cus=256, methods=None):
    bad = {}
    ms = upper_sizes(cus)
    for m in ms:
        jobs = NON_HOMMEL if m * (m - 1) // 2 <= ALL_METHODS_UP_TO else ["holm", "fdr_bh", "fdr_gbs"]
        if methods:
            jobs = list(methods)
        for dtype in DTYPES:
            rng = np.random.default_rng([seed, m, np.dtype(dtype).itemsize, 7])
            a, iu = symmetric_from(rng, m, dtype)
            check_upper(bad, "upper N=%d (%d tests) %s" % (m, len(iu[0]), np.dtype(dtype).name), a, iu, jobs)
        if verbose:
            print("upper N %5d: %9d tests" % (m, m * (m - 1) // 2), flush=True)
    return bad


HOMMEL_SIZES = (1, 2, 3, 255, 256, 257, 511, 513, 16384, 16385, 16386, 100003)


def sweep_hommel(seed=1, verbose=True, ns=HOMMEL_SIZES):
    bad = {}
    for i, n in enumerate(ns):
        for dtype in DTYPES:
            rng = np.random.default_rng([seed, n, np.dtype(dtype).itemsize, 11])
            v = hommel_values(rng, n, dtype).reshape(shape_for(n, i))
            t0 = time.time()
            check_flat(bad, "hommel n=%d %s" % (n, np.dtype(dtype).name), v, ["hommel"])
            if verbose and n > 1000:
                print("hommel n %6d %s: %.1f s" % (n, np.dtype(dtype).name, time.time() - t0), flush=True)
    return bad


BYTE_SIZES = (100003, 2100001)
BYTE_UPPER_N = 449  # 100 576 tests


def sweep_bytes(seed=1, verbose=True, ns=BYTE_SIZES):
    """Every byte pattern at the sizes `ns` (holm and fdr_bh, symmetric=False) and as one upper-mode matrix."""
    bad = {}
    for dtype in DTYPES:
        for varying in byte_patterns(dtype):
            tag = "bytes %s %s" % (np.dtype(dtype).name, ",".join(map(str, varying)) or "none")
            for n in ns:
                rng = np.random.default_rng([seed, n, np.dtype(dtype).itemsize, 13] + list(varying))
                v = pattern_values(rng, n, dtype, varying)
                assert varying_bytes(v) == tuple(varying), (tag, varying_bytes(v))
                check_flat(bad, "%s n=%d" % (tag, n), v.reshape(1, n), ["holm", "fdr_bh"])
            rng = np.random.default_rng([seed, BYTE_UPPER_N, np.dtype(dtype).itemsize, 17] + list(varying))
            a, iu = symmetric_from(rng, BYTE_UPPER_N, dtype, gen=lambda r, n, t: pattern_values(r, n, t, varying))
            assert varying_bytes(a[iu]) == tuple(varying)
            check_upper(bad, "%s upper N=%d" % (tag, BYTE_UPPER_N), a, iu, ["holm", "fdr_bh"])
            if verbose:
                print(tag + "  done", flush=True)
    return bad


def sweep_specials(seed=1, verbose=True, n=1000003):
    bad = {}
    for dtype in DTYPES:
        name = np.dtype(dtype).name
        for inf in (False, True):
            rng = np.random.default_rng([seed, n, np.dtype(dtype).itemsize, 19])
            v, _ = specials(rng, n, dtype, inf=inf)
            assert not np.isnan(v).any() and np.isinf(v).sum() == int(inf) and (v < 0).any() and (v > 1).any()
            assert np.signbit(v[v == 0]).any() and not np.signbit(v[v == 0]).all()
            check_flat(bad, "specials %s%s" % (name, " +inf" if inf else ""), v.reshape(shape_for(n, 2)), NON_HOMMEL)
        rng = np.random.default_rng([seed, n, np.dtype(dtype).itemsize, 19])
        v, nan_cells = specials(rng, n, dtype, inf=True, nan=True)
        assert np.array_equal(np.isnan(v), nan_cells) and nan_cells.sum() >= len(NAN_BITS[dtype])
        check_flat(bad, "specials %s NaN" % name, v.reshape(1, n), ["holm", "holm-sidak"])
        got = device_adjust(v.reshape(1, n), "holm", ALPHA, False).reshape(-1)
        if not np.array_equal(np.isnan(got), nan_cells):
            bad.setdefault("specials %s NaN" % name, []).append("holm: %d NaN cells, %d in the input" % (np.isnan(got).sum(), nan_cells.sum()))
        if verbose:
            print("specials %s  done" % name, flush=True)
    return bad


# ---- symmetry -----------------------------------------------------------------------------------------------------------
SYMMETRY_NS = tuple(range(1, 71)) + (95, 96, 97, 127, 128, 129, 1023, 1024, 1025, 4095, 4096, 4097, 10007)
EDIT_KINDS = ("large", "vanishes", "survives", "nan")


def symmetry_positions(n, rng):
    """name -> (i, j): the tile classes of symmetric_kernel (32 x 32 tiles, the mirror tile through LDS)."""
    if n < 2:
        return {}
    t = n // 32 - 1  # the last full tile column (block row 0); with a single tile its corners include two diagonal cells
    c0 = 32 * max(t, 0)
    pos = {"(0,1)": (0, 1), "(0,N-1)": (0, n - 1), "(N-2,N-1)": (n - 2, n - 1), "(N-1,0)": (n - 1, 0)}
    if n >= 32:
        pos.update({"tile corner 0": (0, c0), "tile corner 1": (0, c0 + 31), "tile corner 2": (31, c0), "tile corner 3": (31, c0 + 31)})
    if n % 32:
        r = n // 32 * 32
        pos["partial tile"] = (r if r < n - 1 else max(r - 1, 0), n - 1) if n > 1 else (0, 0)
        pos["partial tile, mirror side"] = (n - 1, max(n // 32 * 32 - 1, 0))
    pos["random"] = (int(rng.integers(0, n)), int(rng.integers(0, n)))
    pos["diagonal"] = (n // 2, n // 2)
    return pos


def symmetry_edits(n, dtype, rng):
    """[(name, kind, i, j, value at (i, j), value at (j, i))]: single-pair edits of an exactly symmetric matrix.  The
    generator itself holds `vanishes` / `survives` to adj_rule.round5 in that dtype."""
    t = dtype
    pairs = [("large", "large", t(0.25), t(0.75)),
             ("sixth decimal, same 1e-5 cell", "vanishes", t(0.500001), t(0.500003)),
             ("seventh decimal, same 1e-5 cell", "vanishes", t(0.1234561), t(0.1234563)),
             ("fifth decimal", "survives", t(0.50001), t(0.50002)),
             ("sixth decimal across a rounding edge", "survives", t(0.500004), t(0.500006)),
             ("seventh decimal across a rounding edge", "survives", t(0.2500049), t(0.2500051)),
             ("NaN on one side", "nan", t(np.nan), t(0.5)),
             ("NaN on the other side", "nan", t(0.5), t(np.nan)),
             ("NaN on both sides", "nan", t(np.nan), np.array([NAN_BITS[dtype][3]], dtype=_BYTES[dtype][0]).view(dtype)[0])]
    for name, kind, a, b in pairs:
        with np.errstate(invalid="ignore"):
            ra, rb = adj_rule.round5(np.array([a, b], dtype=dtype))
        if kind == "vanishes":
            assert a != b and ra == rb, (name, dtype)
        if kind == "survives":
            assert ra != rb, (name, dtype)
    out = []
    for pname, (i, j) in symmetry_positions(n, rng).items():
        for name, kind, a, b in pairs:
            out.append(("%s at %s" % (name, pname), kind, i, j, a, b))
    return out


def edit_verdict(i, j, a, b):
    """values_symmetric of an exactly symmetric matrix after cells (i, j) <- a and (j, i) <- b: the verdict on that pair
    alone (adj_rule.values_symmetric of the 2 x 2 matrix that holds it off its diagonal)."""
    if i == j:
        return True
    with np.errstate(invalid="ignore"):  # signalling NaNs
        return adj_rule.values_symmetric(np.array([[0, a], [b, 0]], dtype=np.asarray(a).dtype))


def whole_matrix_verdict(a):
    with np.errstate(invalid="ignore"):
        return adj_rule.values_symmetric(a)


def device_symmetric(d):
    from seekr_amd import consumers
    return consumers.pvals_symmetric(d)


def sweep_symmetry(seed=1, verbose=True, ns=SYMMETRY_NS, upload=None, verdict=None):
    """skr_pvals_symmetric against adj_rule.values_symmetric.  The matrix is uploaded once per (N, dtype); an edit
    re-uploads its two rows.  `upload` / `verdict` replace the device (the CPU test runs the list on the host)."""
    if upload is None:
        from seekr_amd import _lib
        upload, verdict = _lib.default_context().from_numpy, device_symmetric
    bad = {}
    seen = {(np.dtype(t).name, k): set() for t in DTYPES for k in EDIT_KINDS}
    for n in ns:
        for dtype in DTYPES:
            name = np.dtype(dtype).name
            rng = np.random.default_rng([seed, n, np.dtype(dtype).itemsize, 23])
            a, _ = symmetric_from(rng, n, dtype)
            if n > 2:
                a[n // 3, n // 3] = np.nan  # garbage on the diagonal
            problems = []
            d = upload(a)
            full_reference = n <= 1025
            if verdict(d) is not True or not whole_matrix_verdict(a):
                problems.append("exactly symmetric, garbage on the diagonal: not True")
            for ename, kind, i, j, x, y in symmetry_edits(n, dtype, rng):
                keep = a[[i, j]].copy()
                a[i, j], a[j, i] = x, y
                want = edit_verdict(i, j, x, y)
                if full_reference or ename.startswith("large at (0,N-1)"):
                    assert whole_matrix_verdict(a) == want, (n, name, ename)
                for row in {i, j}:
                    d.upload(a[row:row + 1], row0=row)
                got = verdict(d)
                seen[(name, kind)].add(want)
                if got is not want:
                    problems.append("%s: %s, want %s" % (ename, got, want))
                a[[i, j]] = keep
                for row in {i, j}:
                    d.upload(a[row:row + 1], row0=row)
            if verdict(d) is not True:
                problems.append("not True after the edits were undone")
            d.free()
            if problems:
                bad["symmetry N=%d %s" % (n, name)] = problems
                print("symmetry N=%d %s  FAIL  %s" % (n, name, "; ".join(problems[:4])), file=sys.stderr, flush=True)
        if verbose and (n % 16 == 0 or n > 1000):
            print("symmetry N %5d  ok so far: %s" % (n, not bad), flush=True)
    if len(ns) > 20:
        assert_both_verdicts(seen)
    return bad


def assert_both_verdicts(seen):
    """A kernel that always answers True (or False) must not pass: both verdicts per dtype and edit kind.  A difference
    that vanishes under round(x, 5) is symmetric by definition, so `vanishes` can only be True; its False comes from
    `survives`, the same decimals across a rounding edge."""
    for t in DTYPES:
        name = np.dtype(t).name
        for kind in ("large", "survives", "nan"):
            assert seen[(name, kind)] == {True, False}, (name, kind, seen[(name, kind)])
        assert seen[(name, "vanishes")] == {True}, seen[(name, "vanishes")]


def symmetry_verdicts(seed=1, ns=SYMMETRY_NS):
    """(dtype name, edit kind) -> the set of verdicts adj_rule.values_symmetric gives over the list, without a matrix."""
    seen = {(np.dtype(t).name, k): set() for t in DTYPES for k in EDIT_KINDS}
    for n in ns:
        for dtype in DTYPES:
            rng = np.random.default_rng([seed, n, np.dtype(dtype).itemsize, 23])
            for _, kind, i, j, x, y in symmetry_edits(n, dtype, rng):
                seen[(np.dtype(dtype).name, kind)].add(edit_verdict(i, j, x, y))
    return seen


# ---- the row-offset scan of skr_edges -----------------------------------------------------------------------------------
EDGE_ROWS_PLUS_1 = (4095, 4096, 4097, 8193, 16777215, 16777216, 16777217, 16777300)


def sweep_edges_scan(seed=1, verbose=True, rows_plus_1=EDGE_ROWS_PLUS_1):
    """consumers.edges on [nrows, c] float32 blocks, c in 1 / 2 / 3, sparse survivors (most rows have no edge), against
    np.nonzero as tests/test_gpu_consumers.py::test_edges_of_a_block_match_numpy does."""
    from seekr_amd import _lib, consumers
    ctx = _lib.default_context()
    bad = {}
    for k, np1 in enumerate(rows_plus_1):
        nrows, c = np1 - 1, 1 + k % 3
        assert scan_levels(np1) == (1 if np1 <= SCAN_TILE else 2 if np1 <= SCAN_TILE ** 2 else 3)
        rng = np.random.default_rng([seed, np1, 29])
        r = np.zeros((nrows, c), dtype=np.float32)
        cells = rng.integers(0, nrows * c, max(8, nrows // 7))
        r.reshape(-1)[cells] = (0.5 + 0.5 * rng.random(len(cells))).astype(np.float32)
        r.reshape(-1)[cells[:3]] = (np.nan, 0.1, 0.0)  # NaN stays, below the cutoff goes
        r[nrows - 1, c - 1] = 0.75  # the last row has an edge: the last offset matters
        cutoff = 0.25
        want = r.copy()
        with np.errstate(invalid="ignore"):
            want[want < cutoff] = 0
        np.fill_diagonal(want, 0)
        wi, wj = np.nonzero(want)
        wv = want[wi, wj]
        empty_rows = nrows - len(np.unique(wi))
        assert empty_rows > nrows // 2, (nrows, empty_rows)
        d = ctx.from_numpy(r)
        i, j, v = consumers.edges(d, cutoff)
        d.free()
        problems = []
        if not (np.array_equal(i, wi.astype(np.uint32)) and np.array_equal(j, wj.astype(np.uint32))):
            problems.append("%d edges, want %d; cells differ" % (len(i), len(wi)))
        elif not (np.array_equal(np.isnan(v), np.isnan(wv)) and np.array_equal(np.nan_to_num(v), np.nan_to_num(wv))):
            problems.append("values differ")
        if problems:
            bad["edges nrows+1=%d c=%d" % (np1, c)] = problems
            print("edges nrows+1=%d c=%d  FAIL  %s" % (np1, c, "; ".join(problems)), file=sys.stderr, flush=True)
        elif verbose:
            print("edges nrows+1 %9d c %d: %d edges, %d scan levels  ok" % (np1, c, len(wi), scan_levels(np1)), flush=True)
    return bad


# ---- the large case -----------------------------------------------------------------------------------------------------
def sweep_large(seed=1, verbose=True, m=LARGE_N, cus=256):
    """m x m float32, fdr_bh, symmetric=False, bit-exact against adj_rule.correct.  At 23 171 the digit table of the
    sort (256 x 65 539 words) takes a third scan level.  Tens of GB of host memory: intermediates are dropped early."""
    n = m * m
    chunk, n_chunks = plan_chunks(n, cus)
    levels = scan_levels(256 * n_chunks)
    if m == LARGE_N:
        assert n > 536870912 and chunk == 8192 and n_chunks > 65536 and levels == 3, (n, chunk, n_chunks, levels)
    rng = np.random.default_rng([seed, m, 31])
    v = rng.random((m, m), dtype=np.float32)
    grid = rng.integers(0, 1 << 20, size=-(-n // 16), dtype=np.int64)
    v.reshape(-1)[::16] = (grid / float(1 << 20)).astype(np.float32)  # ties, zeros among them
    del grid
    v[0, :64] = 1.0
    t0 = time.time()
    got = device_adjust(v, "fdr_bh", ALPHA, False)
    t1 = time.time()
    if verbose:
        print("large: %d tests, %d chunks of %d, %d scan levels; device and copies %.1f s" % (n, n_chunks, chunk, levels, t1 - t0), flush=True)
    want = adj_rule.correct(v.reshape(-1), "fdr_bh", ALPHA)
    if verbose:
        print("large: host reference %.1f s" % (time.time() - t1), flush=True)
    del v
    wrong = mismatch(got, want.reshape(m, m), "fdr_bh", np.float32)
    return {"large %d x %d float32" % (m, m): [wrong]} if wrong else {}


SWEEPS = ("sizes", "upper", "hommel", "bytes", "specials", "symmetry", "edges", "large")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--full", action="store_true", help="the unthinned size list")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--cus", type=int, default=256, help="compute units of the device (the chunk rule's W = 16 per CU)")
    ap.add_argument("--only", default=None, help="comma-separated: " + ",".join(SWEEPS))
    ap.add_argument("--sizes", default=None, help="comma-separated numbers of tests for the sizes sweep")
    ap.add_argument("--methods", default=None, help="comma-separated methods for the sizes / upper sweeps")
    ap.add_argument("--no-large", action="store_true")
    args = ap.parse_args()
    only = set(args.only.split(",")) if args.only else set(SWEEPS)
    if args.sizes:
        only = {"sizes"}
    if args.no_large:
        only.discard("large")
    methods = [adj_rule.canonical(m) for m in args.methods.split(",")] if args.methods else None
    failing = 0
    for name in SWEEPS:
        if name not in only:
            continue
        t0 = time.time()
        if name == "sizes":
            ns = [int(s) for s in args.sizes.split(",")] if args.sizes else sizes(not args.full, args.cus, args.seed)
            bad = sweep_sizes(ns, args.seed, methods, cus=args.cus)
            what = "%d sizes (%d .. %d)" % (len(ns), ns[0], ns[-1])
        elif name == "upper":
            bad, what = sweep_upper(args.seed, cus=args.cus, methods=methods), "upper-mode N %s" % (upper_sizes(args.cus),)
        elif name == "hommel":
            bad, what = sweep_hommel(args.seed), "hommel n %s" % (HOMMEL_SIZES,)
        elif name == "bytes":
            bad, what = sweep_bytes(args.seed), "%d + %d byte patterns" % (len(byte_patterns(np.float32)), len(byte_patterns(np.float64)))
        elif name == "specials":
            bad, what = sweep_specials(args.seed), "special values"
        elif name == "symmetry":
            bad, what = sweep_symmetry(args.seed), "%d matrix sizes of the symmetry test" % len(SYMMETRY_NS)
        elif name == "edges":
            bad, what = sweep_edges_scan(args.seed), "edge-list row counts %s" % (EDGE_ROWS_PLUS_1,)
        else:
            bad, what = sweep_large(args.seed, cus=args.cus), "%d x %d float32 fdr_bh" % (LARGE_N, LARGE_N)
        failing += len(bad)
        print("%s: %s, %d failing, %.1f s%s" % (name, what, len(bad), time.time() - t0, ": " + "; ".join(sorted(bad)) if bad else ""), flush=True)
    sys.exit(1 if failing else 0)


if __name__ == "__main__":
    main()
