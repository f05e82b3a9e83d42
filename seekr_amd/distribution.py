"""How the values of r are distributed, on MI355X without the r matrix: a histogram over any edge table and exact order
statistics (quantiles, the cutoff that keeps a given density of cells) of the self-comparison's upper triangle or of one
set of rows against another.  The reference answers this from the whole matrix (find_dist.py:163-169 takes
sim[np.triu_indices]); the specification here is numpy on this package's own float32 r,

    np.histogram(values, bins=edges) with the cells below, above and NaN counted apart (np.histogram drops them silently)
    np.sort(values[~isnan(values)])[rank] in the float32 ordering with -0 below +0

count for count and bit for bit (tests/distribution_model.py).  r is produced one [stripe, panel] block at a time by
consumers.Sweep; a block is reduced by skr_hist_edges / skr_hist_key_digits to 64-bit counts that are added up on the
host.  A cell list or a piece of r is never kept: device memory is one [stripe_rows, panel] buffer.

An order statistic is a radix descent over the order-preserving key of a float32 (consumers.float32_key): DIGITS
passes, each one sweep of all blocks (r is recomputed), each a histogram of the next key digit among the cells that share
the prefix found so far.  The descent itself runs on the host in Python ints.
"""
import ctypes as C
from fractions import Fraction

import numpy as np

from seekr_amd import _lib
from seekr_amd.consumers import Sweep, block_args, float32_unkey

DIGITS = (12, 10, 10)   # key bits per pass, most significant first
MAX_PREFIXES = 8        # distinct prefixes one pass takes (skr_hist_key_digits)
MAX_EDGES = 4097        # edges of one table (skr_hist_edges)


# ---- one block ----------------------------------------------------------------------------------------------------------
def check_edges(edges):
    """The edge table as the device takes it: 2 ... MAX_EDGES float32, finite, strictly ascending (ValueError otherwise)."""
    e = np.ascontiguousarray(edges, dtype=np.float32).reshape(-1)
    if not 2 <= len(e) <= MAX_EDGES:
        raise ValueError("an edge table has 2 to {} edges (got {})".format(MAX_EDGES, len(e)))
    if not np.isfinite(e).all() or not (e[1:] > e[:-1]).all():
        raise ValueError("the edges must be finite and strictly ascending in float32")
    return e


def make_edges(edges=None, bins=None, range=None):
    """`edges`, or `bins` equal bins over range=(lo, hi): float32 np.linspace on the host — the device sees edges only."""
    if edges is not None:
        if bins is not None or range is not None:
            raise ValueError("give edges, or bins with range, not both")
        return check_edges(edges)
    if bins is None or range is None:
        raise ValueError("give edges, or an integer bins with range=(lo, hi)")
    bins = int(bins)
    if bins < 1:
        raise ValueError("bins must be at least 1 (got {})".format(bins))
    lo, hi = range
    return check_edges(np.linspace(np.float32(lo), np.float32(hi), bins + 1, dtype=np.float32))


def hist_edges_block(r, edges, hist, extra, nrows=None, col_begin=0, col_end=None, row_global0=0, col_global0=0,
                     upper_only=False):
    """Add the cells of the device block r[0:nrows, col_begin:col_end] to hist (uint64 [len(edges) - 1]) and to
    extra = uint64 [3]: below, above, nan (skr_hist_edges)."""
    _lib.check(_lib.lib().skr_hist_edges(*block_args(r, nrows, col_begin, col_end, row_global0, col_global0),
                                         1 if upper_only else 0, edges.ctypes.data_as(C.c_void_p), len(edges),
                                         hist.ctypes.data_as(C.c_void_p), extra[0:].ctypes.data_as(C.c_void_p),
                                         extra[1:].ctypes.data_as(C.c_void_p), extra[2:].ctypes.data_as(C.c_void_p)))


def hist_key_block(r, shift, bits, prefixes, prefix_bits, hist, nan, nrows=None, col_begin=0, col_end=None, row_global0=0,
                   col_global0=0, upper_only=False):
    """Add the cells of the device block to hist (uint64 [len(prefixes), 2^bits]) and nan (uint64 [1]): one pass over
    key digits (skr_hist_key_digits)."""
    p = np.ascontiguousarray(prefixes, dtype=np.uint32)
    assert hist.dtype == np.uint64 and hist.flags.c_contiguous and hist.size == len(p) << bits
    _lib.check(_lib.lib().skr_hist_key_digits(*block_args(r, nrows, col_begin, col_end, row_global0, col_global0),
                                              1 if upper_only else 0, int(shift), int(bits), int(prefix_bits),
                                              p.ctypes.data_as(C.c_void_p), len(p), hist.ctypes.data_as(C.c_void_p),
                                              nan.ctypes.data_as(C.c_void_p)))


# ---- the sweep ----------------------------------------------------------------------------------------------------------
def n_cells(a, b=None):
    """The cells a sweep visits: the upper triangle (k = 1) of the self-comparison, or all of a x b."""
    return a.rows * (a.rows - 1) // 2 if b is None else a.rows * b.rows


def r_histogram(a, b=None, edges=None, bins=None, range=None, stripe_rows=8192, panel_rows=None):
    """(hist uint64 [len(edges) - 1], below, above, nan) of the cells of r for the prepared operand(s) (_lib.Operand, as
    neighbors._prepare leaves them): bin i holds edges[i] <= r < edges[i + 1], the last bin is closed on the right;
    below / above / nan (ints) are the cells np.histogram would leave out.  b=None: the upper triangle of the
    self-comparison; else every cell of a x b.  edges, or bins with range=(lo, hi) — make_edges."""
    edges = make_edges(edges, bins, range)
    hist, extra = np.zeros(len(edges) - 1, dtype=np.uint64), np.zeros(3, dtype=np.uint64)
    with Sweep(a, b, stripe_rows, panel_rows) as sweep:
        sweep.run(lambda buf, **where: hist_edges_block(buf, edges, hist, extra, **where))
    return hist, int(extra[0]), int(extra[1]), int(extra[2])


# ---- the descent over the float32 ordering ------------------------------------------------------------------------------
def descend(ranks, pass_fn):
    """(values float32 [len(ranks)], M) by a radix descent over the key: for each 0-based ascending rank among the
    non-NaN cells, the float32 with exactly that rank.  pass_fn(shift, bits, prefixes, prefix_bits) -> (uint64
    [len(prefixes), 2^bits], nan) is one sweep of all cells.  M is the first histogram's total; `ranks` may be a function
    of M (quantiles and densities need M, and get it without a sweep of their own).  All ranks share a pass, with their
    distinct prefixes; more than MAX_PREFIXES of them go in batches.  The next digit comes from a cumulative sum in
    Python ints and the rank that remains is kept.  A rank outside [0, M) raises ValueError after the first pass."""
    state, done, total = None, 0, None  # state, per rank: (the key prefix found so far, the rank among the cells under it)
    for bits in DIGITS:
        shift = 32 - done - bits
        distinct = sorted({p for p, _ in state}) if done else [0]
        table = {}
        for at in range(0, len(distinct), MAX_PREFIXES):
            batch = distinct[at:at + MAX_PREFIXES]
            hist = np.asarray(pass_fn(shift, bits, batch, done)[0]).reshape(len(batch), 1 << bits)
            for q, p in enumerate(batch):
                table[p] = hist[q].tolist()
        if total is None:
            total = sum(table[0])
            state = [(0, r) for r in _check_ranks(ranks(total) if callable(ranks) else ranks)]
            for _, r in state:
                if not 0 <= r < total:
                    raise ValueError("rank {} is outside [0, {}), the non-NaN cells".format(r, total))
        following = []
        for p, r in state:
            below = 0
            for digit, c in enumerate(table[p]):
                if r < below + c:
                    break
                below += c
            following.append(((p << bits) | digit, r - below))
        state = following
        done += bits
    return float32_unkey([p for p, _ in state]), total


def _check_ranks(ranks):
    out = []
    for r in np.asarray(ranks).reshape(-1).tolist():
        if int(r) != r:
            raise ValueError("a rank is an integer (got {!r})".format(r))
        out.append(int(r))
    return out


def _order_statistics(sweep, ranks):
    """(values, M, nan): descend() over the sweep's blocks; nan is the first pass's count of NaN cells."""
    nans = []

    def one_pass(shift, bits, prefixes, prefix_bits):
        hist, nan = np.zeros((len(prefixes), 1 << bits), dtype=np.uint64), np.zeros(1, dtype=np.uint64)
        sweep.run(lambda buf, **where: hist_key_block(buf, shift, bits, prefixes, prefix_bits, hist, nan, **where))
        nans.append(int(nan[0]))
        return hist, nans[-1]

    values, m = descend(ranks, one_pass)
    return values, m, nans[0]


def r_order_statistics(a, b=None, ranks=(), stripe_rows=8192, panel_rows=None):
    """float32 [len(ranks)]: for each 0-based ascending rank among the non-NaN cells of r (upper triangle of the
    self-comparison, or a x b) the value with exactly that rank — np.sort(values[~isnan])[rank], -0 below +0.  At most
    len(DIGITS) sweeps of all blocks whatever the number of ranks up to MAX_PREFIXES distinct prefixes (more: batches).
    A rank outside [0, M) raises ValueError after the first sweep.  Nothing is allocated in proportion to M."""
    ranks = _check_ranks(ranks)
    with Sweep(a, b, stripe_rows, panel_rows) as sweep:
        return _order_statistics(sweep, ranks)[0]


def quantile_rank(q, m):
    """floor(Fraction(q) (m - 1)): the rank of np.quantile(method='lower'), in exact arithmetic."""
    q = Fraction(q)
    if not 0 <= q <= 1:
        raise ValueError("a quantile lies in [0, 1] (got {})".format(float(q)))
    if m < 1:
        raise ValueError("no cell that is not NaN: there is no quantile")
    return int(q * (m - 1) // 1)


def density_rank(density, m):
    """The ascending rank of the m_th largest of m cells, m_th = max(1, floor(Fraction(density) m))."""
    d = Fraction(density)
    if not 0 < d <= 1:
        raise ValueError("a density lies in (0, 1] (got {})".format(float(d)))
    if m < 1:
        raise ValueError("no cell that is not NaN: there is no cutoff")
    return m - max(1, int(d * m // 1))


def r_quantiles(a, b=None, q=(), stripe_rows=8192, panel_rows=None):
    """(values float32 [len(q)], M): the cell of rank floor(Fraction(q) (M - 1)) among the M non-NaN cells, for each q
    in [0, 1] (a float, a Fraction or a string Fraction accepts)."""
    q = list(np.atleast_1d(q).tolist()) if not isinstance(q, (list, tuple)) else list(q)
    for x in q:
        quantile_rank(x, 1)  # the range check, before any sweep
    with Sweep(a, b, stripe_rows, panel_rows) as sweep:
        values, m, _ = _order_statistics(sweep, lambda m: [quantile_rank(x, m) for x in q])
    return values, m


def density_cutoff(a, density, b=None, stripe_rows=8192, panel_rows=None):
    """The float32 c that keeps `density` of the cells: the m-th largest non-NaN cell of r, m = max(1,
    floor(Fraction(density) M)) — at least m cells are >= c and fewer than m are > c.  pearson_edges(a, c) then holds at
    least m edges (ties with c are kept; cells equal to 0 are dropped by the edge rule, so choose a density with c > 0)."""
    density_rank(density, 1)
    with Sweep(a, b, stripe_rows, panel_rows) as sweep:
        values, _, _ = _order_statistics(sweep, lambda m: [density_rank(density, m)])
    return values[0]


# ---- host arrays --------------------------------------------------------------------------------------------------------
class RDistribution:
    """edges (float32) and hist (uint64) — None without an edge table — with below / above / nan (ints; nan always),
    q and quantiles (float32), densities and cutoffs (float32), n_cells (all cells visited) and n_values (those that are
    not NaN)."""

    def __init__(self, n_cells, n_values, nan, edges=None, hist=None, below=None, above=None, q=(), quantiles=None,
                 densities=(), cutoffs=None):
        self.n_cells, self.n_values, self.nan = int(n_cells), int(n_values), int(nan)
        self.edges, self.hist, self.below, self.above = edges, hist, below, above
        self.q, self.densities = list(q), list(densities)
        self.quantiles = np.empty(0, np.float32) if quantiles is None else quantiles
        self.cutoffs = np.empty(0, np.float32) if cutoffs is None else cutoffs

    def __repr__(self):
        return "RDistribution({} cells, {} NaN, {} bins, {} quantiles, {} cutoffs)".format(
            self.n_cells, self.nan, 0 if self.hist is None else len(self.hist), len(self.quantiles), len(self.cutoffs))


def distribution(a, b=None, edges=None, bins=None, range=None, q=(), densities=(), stripe_rows=8192, panel_rows=None):
    """RDistribution of the prepared operand(s): the histogram when an edge table is given (one sweep), the quantiles
    and density cutoffs when asked for (one descent for all of them)."""
    q, densities = list(q), list(densities)
    for x in q:
        quantile_rank(x, 1)
    for d in densities:
        density_rank(d, 1)
    want_hist = edges is not None or bins is not None
    if want_hist:
        edges = make_edges(edges, bins, range)
    out = {}
    with Sweep(a, b, stripe_rows, panel_rows) as sweep:
        if want_hist:
            hist, extra = np.zeros(len(edges) - 1, dtype=np.uint64), np.zeros(3, dtype=np.uint64)
            sweep.run(lambda buf, **where: hist_edges_block(buf, edges, hist, extra, **where))
            out.update(edges=edges, hist=hist, below=int(extra[0]), above=int(extra[1]))
            nan = int(extra[2])
            m = n_cells(a, b) - nan
        if q or densities or not want_hist:
            values, m, nan = _order_statistics(
                sweep, lambda m: [quantile_rank(x, m) for x in q] + [density_rank(d, m) for d in densities])
            out.update(q=q, quantiles=values[:len(q)], densities=densities, cutoffs=values[len(q):])
    return RDistribution(n_cells(a, b), m, nan, **out)


@_lib.api_call
def pearson_distribution(counts, counts2=None, edges=None, bins=None, range=None, q=(), densities=(), **kw):
    """distribution() for a host count matrix (anything np.ascontiguousarray(.., float32) accepts): the rows are prepared
    as pearson() and nearest() prepare them.  counts2=None (or `counts` itself): the upper triangle of the
    self-comparison; else the rows of counts against the rows of counts2.  `kw`: stripe_rows, panel_rows."""
    from seekr_amd import neighbors
    same = counts2 is None or counts2 is counts
    c = neighbors._f32(counts)
    c2 = c if same else neighbors._f32(counts2)
    if c.ndim != 2 or c2.ndim != 2:
        raise ValueError("counts must be a 2-D matrix")
    if c.shape[1] != c2.shape[1]:
        raise ValueError("counts and counts2 must have the same number of columns ({} and {})".format(c.shape[1], c2.shape[1]))
    if (c.shape[0] * (c.shape[0] - 1) // 2 if same else c.shape[0] * c2.shape[0]) == 0:
        raise ValueError("there is no cell of r to look at")
    # the argument checks of distribution(), before anything is uploaded
    for x in q:
        quantile_rank(x, 1)
    for d in densities:
        density_rank(d, 1)
    if edges is not None or bins is not None:
        edges, bins, range = make_edges(edges, bins, range), None, None
    ctx = _lib.default_context()
    z, z2 = neighbors._prepare(ctx, c, c2, same)
    try:
        return distribution(z, z2, edges=edges, q=q, densities=densities, **kw)
    finally:
        z.free()
        if z2 is not None:
            z2.free()
