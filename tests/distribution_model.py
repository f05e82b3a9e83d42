"""The specification of seekr_amd.distribution in plain numpy: the float32 ordering, one histogram pass over key digits,
the radix descent that turns such passes into order statistics, and the edge-table rule.  Nothing here touches the device;
tests/test_distribution_cpu.py holds these models to np.sort and np.histogram, tests/test_gpu_distribution.py holds the
device to them, count for count."""
from fractions import Fraction

import numpy as np

DIGITS = (12, 10, 10)  # the descent's digit widths, most significant first (seekr_amd.distribution.DIGITS)
MAX_PREFIXES = 8


def key(x):
    """float32 array -> uint32 array whose order is the order of the values, -0.0 just below +0.0 (significant._key)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def unkey(k):
    k = np.ascontiguousarray(k, dtype=np.uint32)
    return np.where(k & np.uint32(0x80000000), k ^ np.uint32(0x80000000), ~k).astype(np.uint32).view(np.float32)


def hist_pass(values, shift, bits, prefixes, prefix_bits):
    """(hist uint64 [len(prefixes), 2^bits], nan): a cell whose top prefix_bits key bits equal prefixes[q] adds one to
    hist[q][(key >> shift) & (2^bits - 1)]; NaN cells are counted apart and never binned."""
    v = np.ascontiguousarray(values, dtype=np.float32).reshape(-1)
    isnan = np.isnan(v)
    k = key(v[~isnan]).astype(np.uint64)
    top = k >> np.uint64(32 - prefix_bits) if prefix_bits else np.zeros_like(k)
    digit = (k >> np.uint64(shift)) & np.uint64((1 << bits) - 1)
    hist = np.zeros((len(prefixes), 1 << bits), dtype=np.uint64)
    for q, p in enumerate(prefixes):
        sel = top == np.uint64(p) if prefix_bits else np.ones(len(k), dtype=bool)
        hist[q] = np.bincount(digit[sel].astype(np.int64), minlength=1 << bits).astype(np.uint64)
    return hist, int(isnan.sum())


def descend(ranks, pass_fn, digits=DIGITS, max_prefixes=MAX_PREFIXES):
    """(values float32 [len(ranks)], M): for each 0-based ascending rank among the non-NaN cells the float32 with that
    rank in key order, by a radix descent over the key.  pass_fn(shift, bits, prefixes, prefix_bits) -> (hist, nan) is one
    sweep of all cells (hist_pass's signature without the values).  All ranks share a pass; more than max_prefixes
    distinct prefixes go in batches.  M, the number of non-NaN cells, is the first histogram's total; a rank outside
    [0, M) raises ValueError after the first pass."""
    ranks = [int(r) for r in ranks]
    state = [(0, r) for r in ranks]  # (prefix so far, rank among the cells under that prefix)
    done, total = 0, None
    for bits in digits:
        shift = 32 - done - bits
        distinct = sorted({p for p, _ in state}) if done else [0]
        table = {}
        for at in range(0, len(distinct), max_prefixes):
            batch = distinct[at:at + max_prefixes]
            hist, _ = pass_fn(shift, bits, batch, done)
            for q, p in enumerate(batch):
                table[p] = [int(c) for c in hist[q]]
        if total is None:
            total = sum(table[0])
            for r in ranks:
                if not 0 <= r < total:
                    raise ValueError("rank {} is outside [0, {}): the non-NaN cells".format(r, total))
        nxt = []
        for p, r in state:
            acc = 0
            for digit, c in enumerate(table[p]):
                if r < acc + c:
                    break
                acc += c
            nxt.append(((p << bits) | digit, r - acc))
        state = nxt
        done += bits
    assert done == 32
    return unkey(np.array([p for p, _ in state], dtype=np.uint32)), total


def order_statistics(values, ranks, **kw):
    """descend() driven by hist_pass on a host array."""
    return descend(ranks, lambda shift, bits, prefixes, prefix_bits: hist_pass(values, shift, bits, prefixes, prefix_bits), **kw)


def quantile_rank(q, m):
    """floor(q (m - 1)) in exact arithmetic: np.quantile(method='lower')'s index without its float rounding."""
    q = Fraction(q)
    if not 0 <= q <= 1:
        raise ValueError("a quantile lies in [0, 1] (got {!r})".format(q))
    return int(q * (m - 1) // 1)


def density_rank(density, m):
    """The ascending rank of the m_th largest of m cells, m_th = max(1, floor(density m))."""
    d = Fraction(density)
    if not 0 < d <= 1:
        raise ValueError("a density lies in (0, 1] (got {!r})".format(d))
    return m - max(1, int(d * m // 1))


def edge_hist(values, edges):
    """(hist uint64 [len(edges) - 1], below, above, nan): bin b holds edges[b] <= v < edges[b + 1], the last bin is closed
    on the right — searchsorted(edges, v, 'right') - 1 with v == edges[-1] going into the last bin."""
    v = np.ascontiguousarray(values, dtype=np.float32).reshape(-1)
    edges = np.asarray(edges, dtype=np.float32)
    isnan = np.isnan(v)
    v = v[~isnan]
    b = np.searchsorted(edges, v, "right").astype(np.int64) - 1
    b[v == edges[-1]] = len(edges) - 2
    below, above = b < 0, b > len(edges) - 2
    hist = np.bincount(b[~below & ~above], minlength=len(edges) - 1).astype(np.uint64)
    return hist, int(below.sum()), int(above.sum()), int(isnan.sum())
