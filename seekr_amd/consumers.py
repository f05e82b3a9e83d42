"""Device-side versions of what the reference does with the Pearson matrix right after computing
it: keeping these reductions on the GPU avoids shipping an N x N matrix over PCIe.

    threshold_zero_diag   kmer_leiden.py:94-96   ld_sim[ld_sim < cutoff] = 0; fill_diagonal(0)
    triu_values           find_dist.py:163       sim[np.triu_indices(N, k=1)]
    subsample             find_dist.py:169       np.random.choice(values, size, replace=False)
    empirical_pvalues     find_pval.py:158-164   p[i,j] = np.sum(fitres > sim[i,j]) / len(fitres)
    edges / pearson_edges kmer_leiden.py:91-96   the thresholded matrix as an edge list, r produced and consumed
                                                 one row stripe at a time (N x N never exists)
    Sweep                 —                      r one [stripe, panel] block after another in one reusable buffer, each handed
                                                 to a visitor (N x N never exists): all of a x b, or the upper triangle of
                                                 a x a.  Its visitors: pearson_cells, pearson_topk, seekr_amd.distribution
    select_cells / pearson_cells  —              the cells with !(r < cutoff) as a device list; pearson_cells over a Sweep
    topk_rows / pearson_topk  —                  the k most correlated rows of every row; pearson_topk merges a Sweep's
                                                 blocks into running lists
    topk_merge_cols / pearson_topk_both  —       the k most correlated rows of every COLUMN, merged beside the row lists in
                                                 one Sweep: both directions of a two-set comparison from one r
    knn_pairs / PairList  —                      top-k lists as mutual or union nearest-neighbour pairs with their ranks, a
                                                 device list (seekr_amd.reciprocal: reciprocal_hits, knn_graph)
    adjust_pvalues        adj_pval.py:53-138     multipletests on the p-value matrix (symmetric: upper triangle)
    adjust_pvalues_head   —                      the same for the smallest p-values of a longer list (seekr_amd.significant)
    select_le / gather_index  —                  the positions of a vector with value <= bound, and a gather by them

Every function takes and returns device matrices (`seekr_amd._lib.Matrix`); `*_host` helpers
wrap host arrays for drop-in use.
"""
import contextlib
import ctypes as C
import os

import numpy as np

from seekr_amd import _lib
from seekr_amd._lib import block_args  # the head of every call on a block of r


def threshold_zero_diag(r, cutoff, diag_col0=0):
    """In place on the device matrix `r`; returns `r`."""
    _lib.check(_lib.lib().skr_threshold_zero_diag(r.ctx._h, r._h, C.c_float(cutoff), int(diag_col0)))
    return r


def triu_values(r, k=1):
    """1 x (n-k)(n-k+1)/2 device vector in np.triu_indices order (float32 or float64, r's dtype)."""
    n = r.rows
    m = max(0, n - k)
    out = r.ctx.empty(1, m * (m + 1) // 2, r.dtype)
    _lib.check(_lib.lib().skr_triu_flatten(r.ctx._h, r._h, int(k), out._h))
    return out


def subsample(values, size, rng=None):
    """np.random.choice(values, size, replace=False) with the draw made on the host by numpy's
    generator (legacy global state by default, as the reference uses) and the gather on device."""
    n = values.rows * values.cols
    perm = (np.random if rng is None else rng).permutation(n)[:size]
    idx = np.ascontiguousarray(perm, dtype=np.int64)
    out = np.empty(len(idx), dtype=np.float32)
    _lib.check(_lib.lib().skr_gather_f32(values.ctx._h, values._h, idx.ctypes.data_as(C.c_void_p), len(idx),
                                         out.ctypes.data_as(C.c_void_p)))
    return out


TRIU_MAX_N = (1 << 31) - 1  # n (n - 1) / 2 and the row starts then fit int64 with room to spare


def _triu_row_starts(n):
    """int64 [n]: the rank of the first cell of row i of np.triu_indices(n, 1), i (2n - i - 1) / 2 (row n - 1 is empty
    and starts at n_cells)."""
    i = np.arange(n, dtype=np.int64)
    return i * (2 * np.int64(n) - i - 1) // 2


def _check_triu_n(n):
    n = int(n)
    if not 0 <= n <= TRIU_MAX_N:
        raise ValueError("n must be in 0..{} (got {})".format(TRIU_MAX_N, n))
    return n


def triu_unrank(index, n):
    """(i, j), int64: the cells of an n x n matrix at the positions `index` of np.triu_indices(n, 1): the row is the
    last one that starts at or before the index, row i starting at i (2n - i - 1) / 2 — np.searchsorted on the table of
    row starts, or, above 2^22 rows (the table would be 16 GiB at n = 2^31 - 1), the same search by bisection on starts
    computed as they are needed.  All arithmetic is int64.  n <= 2^31 - 1 (ValueError), index in [0, n (n - 1) / 2)
    (IndexError)."""
    n = _check_triu_n(n)
    index = np.asarray(index, dtype=np.int64)
    cells = n * (n - 1) // 2
    if index.size and (index.min() < 0 or index.max() >= cells):
        raise IndexError("index out of range for the {} cells of the upper triangle of {} rows".format(cells, n))
    if n <= (1 << 22):  # the table itself: the rightmost row that starts at or before the index
        i = np.searchsorted(_triu_row_starts(n), index, side="right").astype(np.int64) - 1
    else:  # the same search without the table: bisection on the row starts, evaluated in int64 as they are needed
        lo, hi = np.zeros(index.shape, np.int64), np.full(index.shape, max(n - 2, 0), np.int64)  # the row lies in lo ... hi
        for _ in range(max(1, int(n - 1).bit_length())):
            mid = (lo + hi + 1) // 2
            right = mid * (2 * np.int64(n) - mid - 1) // 2 <= index
            lo, hi = np.where(right, mid, lo), np.where(right, hi, mid - 1)
        i = lo
    start = i * (2 * np.int64(n) - i - 1) // 2
    return i, index - start + i + 1


def triu_rank(i, j, n):
    """int64: the position of the cells (i, j), i < j < n, in np.triu_indices(n, 1)."""
    n = _check_triu_n(n)
    i, j = np.asarray(i, dtype=np.int64), np.asarray(j, dtype=np.int64)
    if i.size and not (np.all(0 <= i) and np.all(i < j) and np.all(j < n)):
        raise IndexError("cells of the upper triangle have 0 <= i < j < n")
    return i * (2 * np.int64(n) - i - 1) // 2 + (j - i - 1)


LEGACY_DRAW_MAX_CELLS = 1 << 29  # above this the permutation the reference draws from is more than 4 GiB
SAMPLE_MAX = 1 << 28             # samples of one pearson_sample: the lists cost 12 bytes each on the device


def draw_index(n_cells, size, rng=None):
    """int64 [size]: which of n_cells values np.random.choice(values, size, replace=False) picks, in its order.
    rng=None, n_cells <= LEGACY_DRAW_MAX_CELLS: np.random.permutation(n_cells)[:size] from numpy's legacy global state —
    exactly what that choice() consumes and yields, so np.random.seed governs the sample as it does in the reference
    (find_dist.py:169).  rng=None above the limit: Generator.choice(n_cells, size, replace=False) of a default_rng seeded
    from np.random.randint(0, 2**31 - 1, size=4) — np.random.seed still governs the result and memory is O(size), but
    the draw is NOT the reference's (which cannot run there at all: it needs the permutation and the whole triangle).
    rng: a np.random.Generator, used that way at any size."""
    n_cells, size = int(n_cells), int(size)
    if size < 0 or size > n_cells:
        raise ValueError("cannot take {} of {} cells without replacement".format(size, n_cells))
    if rng is None:
        if n_cells <= LEGACY_DRAW_MAX_CELLS:
            # a copy: a slice would keep the whole permutation (8 bytes per cell) alive as long as the index lives
            return np.array(np.random.permutation(n_cells)[:size], dtype=np.int64)
        rng = np.random.default_rng(np.random.randint(0, 2 ** 31 - 1, size=4))
    return np.asarray(rng.choice(n_cells, size, replace=False), dtype=np.int64)


def gather_cells(r, rows, cols, out, first=0, count=None, nrows=None, col_begin=0, col_end=None, row_global0=0,
                 col_global0=0):
    """out[s] = the bits of the cell (rows[s], cols[s]) — global indices, uint32 device vectors — for the slots s in
    [first, first + count) whose cell lies in the device block r[0:nrows, col_begin:col_end]; every other slot of the
    float32 device vector `out` is left alone (skr_gather_cells).  Returns the number of slots written."""
    slots = rows.rows * rows.cols
    gathered = C.c_int64(0)
    _lib.check(_lib.lib().skr_gather_cells(*block_args(r, nrows, col_begin, col_end, row_global0, col_global0), rows._h,
                                           cols._h, int(first), int(slots - first if count is None else count), out._h,
                                           C.byref(gathered)))
    return gathered.value


def pearson_sample(a, b=None, index=(), stripe_rows=8192, panel_rows=None):
    """float32 [len(index)]: the cells of r = a b^T / K at the linear indices `index`, in the order of `index`, gathered
    out of the blocks of Sweep(a, b, stripe_rows, panel_rows) — the bits of the r that sweep makes; r never stands whole.
    a, b: prepared operands (_lib.Operand).  b=None: the upper triangle of a against itself, indices in triu_unrank
    order (np.triu_indices(n, 1)); else row-major i * b.rows + j.  Duplicates are served.

    The indices are sorted by (row, column) — which is their own order — and unranked on the host, and the sorted rows,
    columns and an output vector go to the device once (12 bytes per sample).  A block's visitor finds the samples of its rows by searchsorted on the
    sorted rows and hands that slice to skr_gather_cells, which skips those of other panels; the numbers gathered must
    add up to len(index) (RuntimeError otherwise: every sample is gathered exactly once).  One download, and the sort is
    undone on the host.  An index outside the cells: numpy's IndexError before any device call; more than SAMPLE_MAX
    samples: ValueError."""
    index = np.asarray(index)
    if index.ndim != 1:
        raise ValueError("index must be one-dimensional")
    if index.size and not np.issubdtype(index.dtype, np.integer):
        raise IndexError("arrays used as indices must be of integer (or boolean) type")
    index = index.astype(np.int64, copy=False)
    if len(index) > SAMPLE_MAX:
        raise ValueError("at most {} samples in one call (got {})".format(SAMPLE_MAX, len(index)))
    n, m = a.rows, (a if b is None else b).rows
    cells = n * (n - 1) // 2 if b is None else n * m
    if len(index) == 0:
        return np.empty(0, np.float32)
    lo, hi = int(index.min()), int(index.max())
    if lo < 0 or hi >= cells:
        raise IndexError("index {} is out of bounds for axis 0 with size {}".format(lo if lo < 0 else hi, cells))
    if max(n, m) > 0xFFFFFFFF:
        raise ValueError("rows and columns are uint32 on the device")
    # both linear orders grow with (row, column), so sorting the indices IS the lexsort by (row, column) — and sorted
    # indices unrank several times faster (the search walks the row starts in order); equal indices are equal cells, so
    # the sort need not be stable
    order = np.argsort(index)
    ranked = index[order]
    rows_sorted, cols_sorted = triu_unrank(ranked, n) if b is None else np.divmod(ranked, np.int64(m))
    ctx = a.ctx
    total = 0
    with contextlib.ExitStack() as held:  # the sweep's buffer and the three lists: freed however this ends
        sweep = held.enter_context(Sweep(a, b, stripe_rows, panel_rows))
        d_rows = ctx.from_numpy(rows_sorted.astype(np.uint32))
        held.callback(d_rows.free)
        d_cols = ctx.from_numpy(cols_sorted.astype(np.uint32))
        held.callback(d_cols.free)
        d_out = ctx.empty(1, len(index), np.float32)
        held.callback(d_out.free)

        def gather(buf, nrows, upper_only, **where):
            nonlocal total
            first, last = np.searchsorted(rows_sorted, [where["row_global0"], where["row_global0"] + nrows])
            if last > first:
                total += gather_cells(buf, d_rows, d_cols, d_out, int(first), int(last - first), nrows=nrows, **where)

        sweep.run(gather)
        if total != len(index):
            raise RuntimeError("{} of {} samples were gathered: every sample is gathered exactly once".format(total, len(index)))
        got = np.array(d_out.to_numpy()).reshape(-1)
    out = np.empty(len(index), np.float32)
    out[order] = got
    return out


def ceil_float32(values):
    """The smallest float32 >= each value (NaN stays NaN).  The reference compares `fitres > sim[i, j]` in the
    background's own precision.  For a float32 v, b > v exactly when ceil32(b) > v: no float32 lies strictly between b and
    ceil32(b), so v < b implies v < ceil32(b) or v = ceil32(b) = b, and ceil32(b) >= b gives the converse.  Rounding to
    nearest instead moves a value that sits just above a cell onto or below it, and the count is one short."""
    wide = np.asarray(values, dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        near = wide.astype(np.float32)  # beyond float32's range: +-inf, and -inf steps up to -FLT_MAX below
        return np.where(near < wide, np.nextafter(near, np.float32(np.inf)), near).astype(np.float32)


def float32_key(v):
    """float32 array -> uint32 keys whose order is the order of the values, -0 just below +0 (NaN: above +inf with the
    sign bit clear, below -inf with it set)."""
    u = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def float32_unkey(key):
    """uint32 keys -> the float32 array they are the keys of, bit for bit."""
    key = np.asarray(key, dtype=np.uint32)
    return np.where(key & np.uint32(0x80000000), key ^ np.uint32(0x80000000), ~key).astype(np.uint32).view(np.float32)


def empirical_pvalues(r, fitres):
    """Device matrix of p-values for the device matrix `r` against the 1-D background `fitres`."""
    fitres = np.asarray(fitres).reshape(-1)
    if fitres.dtype != np.float32:
        fitres = ceil_float32(fitres)
    bg = np.sort(fitres[~np.isnan(fitres)])
    ctx = r.ctx
    if len(bg) == 0:  # nothing compares greater: every count is 0
        return ctx.zeros(r.rows, r.cols)
    p = ctx.empty(r.rows, r.cols)
    d_bg = ctx.from_numpy(bg)
    _lib.check(_lib.lib().skr_empirical_pvalues(ctx._h, r._h, d_bg._h, int(len(fitres)), p._h))
    return p


def parametric_pvalues(r, dist_name, params):
    """Device matrix p = float32(1 - scipy.stats.<dist_name>(*params).cdf(r)) — find_pval's branch for a fitted
    distribution (find_pval.py:118-133); `params` is the tuple find_dist returns (shapes..., loc, scale).
    NotImplementedError for distributions outside find_dist's common10 list."""
    ctx = r.ctx
    vals = [float(v) for v in params]
    arr = (C.c_double * max(1, len(vals)))(*vals)
    p = ctx.empty(r.rows, r.cols)
    _lib.check(_lib.lib().skr_parametric_pvalues(ctx._h, r._h, dist_name.encode(), arr, len(vals), p._h))
    return p


def pvalues_host(sim, fitres, bestfit=1):
    """find_pval's p-value step for a host float32 `sim`: `fitres` is find_dist's output — a list of
    (distribution name, deviance, parameters) (the `bestfit`-th entry is used, find_pval.py:116-121) or a 1-D array of
    background similarities (:158-164).  Returns a host float32 matrix."""
    sim = np.ascontiguousarray(sim, dtype=np.float32)
    if isinstance(fitres, np.ndarray):
        return empirical_pvalues_host(sim, fitres)
    name, _, params = fitres[bestfit - 1]
    ctx = _lib.default_context()
    return parametric_pvalues(ctx.from_numpy(sim), name, params).to_numpy()


def empirical_pvalues_host(sim, fitres):
    """find_pval's numpy-array branch for a host float32 `sim`; returns a host float32 matrix."""
    sim = np.ascontiguousarray(sim, dtype=np.float32)
    ctx = _lib.default_context()
    return empirical_pvalues(ctx.from_numpy(sim), fitres).to_numpy()


def edges(r, cutoff, nrows=None, col_begin=0, col_end=None, row_global0=0, col_global0=0, upper_only=False, into=None):
    """(rows, cols, vals) numpy arrays (uint32, uint32, float32): the cells of the device block
    r[0:nrows, col_begin:col_end] that kmer_leiden.py:94-96 leaves non-zero, in np.nonzero order.  into: a CellList the
    outputs are appended to on the device instead; the number of edges is returned."""
    ctx = r.ctx
    count = C.c_int64(0)
    args = (*block_args(r, nrows, col_begin, col_end, row_global0, col_global0), C.c_float(cutoff), 1 if upper_only else 0)
    _lib.check(_lib.lib().skr_edges(*args, None, None, None, C.byref(count)))
    n = count.value
    if n == 0:
        return 0 if into is not None else (np.empty(0, np.uint32), np.empty(0, np.uint32), np.empty(0, np.float32))
    out_r, out_c, out_v = ctx.empty(1, n, np.uint32), ctx.empty(1, n, np.uint32), ctx.empty(1, n, np.float32)
    _lib.check(_lib.lib().skr_edges(*args, out_r._h, out_c._h, out_v._h, C.byref(count)))
    if into is not None:
        into.append_from(out_r, out_c, out_v, n)
        res = n
    else:
        res = out_r.to_numpy().reshape(-1), out_c.to_numpy().reshape(-1), out_v.to_numpy().reshape(-1)
    for m in (out_r, out_c, out_v):
        m.free()
    return res


class FusedEdges:
    """Edge lists straight from the contraction (skr_pearson_gemm_edges): r is never written.  Keeps the output buffers
    and, for rows of more than 4 096 columns, the scratch block between calls; when a block holds more edges than the
    buffers the call is repeated with larger ones."""

    def __init__(self, ctx, capacity=1 << 20):
        self.ctx, self.cap = ctx, int(capacity)
        self._out = None
        self._scratch = None

    def _buffers(self):
        if self._out is None or self._out[0].rows < self.cap:
            if self._out is not None:
                for m in self._out:
                    m.free()
            # cap x 1: a prefix of the list is then a row range, which is what skr_mat_download copies
            self._out = (self.ctx.empty(self.cap, 1, np.uint32), self.ctx.empty(self.cap, 1, np.uint32),
                         self.ctx.empty(self.cap, 1, np.float32))
        return self._out

    def block(self, a, b, cutoff, row_global0=0, col_global0=0, upper_only=False, scratch=None, retry=True, into=None):
        """(rows, cols, vals) of the block a b^T / K, global indices, np.nonzero order.  `scratch`: a float32 matrix of at
        least [a.rows, b.rows] for rows of more than 4 096 columns (allocated and kept here when not given).  The list
        buffers start at 2e-3 entries per cell; a block with more edges is run again with room (retry=True) or reported
        as None (retry=False: the caller has a cheaper way for lists that dense).  into: a CellList the filled prefix
        of the buffers is appended to on the device; the number of edges is returned and nothing crosses PCIe."""
        ctx = self.ctx
        # more than one accumulator restart per row?  the library's own rule, knob included (not re-derived here)
        needs = C.c_int(0)
        _lib.check(_lib.lib().skr_pearson_gemm_edges_needs_scratch(ctx._h, a._h, b._h, C.byref(needs)))
        needs = bool(needs.value)
        if needs and scratch is None:
            if self._scratch is None or self._scratch.rows < a.rows or self._scratch.cols < b.rows:
                if self._scratch is not None:
                    self._scratch.free()
                self._scratch = ctx.empty(a.rows, b.rows)
            scratch = self._scratch
        self.cap = max(self.cap, min(int(2e-3 * a.rows * b.rows) + 1024, 1 << 30))
        while True:
            o_r, o_c, o_v = self._buffers()
            count = C.c_int64(0)
            _lib.check(_lib.lib().skr_pearson_gemm_edges(ctx._h, a._h, b._h, _lib._h(scratch) if needs else None,
                                                         int(row_global0), int(col_global0), C.c_float(cutoff),
                                                         1 if upper_only else 0, o_r._h, o_c._h, o_v._h, C.byref(count)))
            n = count.value
            if n <= self.cap:
                break
            if not retry:
                return None
            self.cap = int(n * 1.25) + 1024  # more edges than the buffers hold: once more with room
        if into is not None:
            into.append_from(o_r, o_c, o_v, n)
            return n
        if n == 0:
            return np.empty(0, np.uint32), np.empty(0, np.uint32), np.empty(0, np.float32)
        return tuple(m.to_numpy(0, n).reshape(-1) for m in (o_r, o_c, o_v))  # only the filled prefix crosses PCIe

    def free(self):
        for m in (self._out or ()):
            m.free()
        if self._scratch is not None:
            self._scratch.free()
        self._out = self._scratch = None


def vec_copy(src, src_off, dst, dst_off, count):
    """dst[dst_off + i] = src[src_off + i] for i < count: device vectors of one dtype, on the device (skr_vec_copy)."""
    _lib.check(_lib.lib().skr_vec_copy(src.ctx._h, src._h, int(src_off), dst._h, int(dst_off), int(count)))


class CellList:
    """A (row, column, value) list that stays on the device: three vectors of `capacity` x 1 cells (uint32, uint32,
    float32 — a prefix is then a row range, as in FusedEdges) of which the first len(self) are filled.  select_cells and
    append_from add behind them; a block that does not fit makes the list grow to at least twice its capacity, the
    filled part carried over on the device (skr_vec_copy)."""
    DTYPES = (np.uint32, np.uint32, np.float32)

    def __init__(self, ctx, capacity=1 << 16):
        self.ctx, self.capacity, self.n = ctx, max(1, int(capacity)), 0
        self.bufs = tuple(ctx.empty(self.capacity, 1, t) for t in self.DTYPES)

    def __len__(self):
        return self.n

    def reserve(self, total):
        """Room for `total` cells in all: nothing happens when they fit."""
        if total <= self.capacity:
            return
        capacity = max(int(total), 2 * self.capacity)
        grown = tuple(self.ctx.empty(capacity, 1, t) for t in self.DTYPES)
        for old, new in zip(self.bufs, grown):
            if self.n:
                vec_copy(old, 0, new, 0, self.n)
            old.free()  # (stream-ordered: the copy above is enqueued before the memory goes back)
        self.bufs, self.capacity = grown, capacity

    def append_from(self, rows, cols, vals, count, src_off=0):
        """Append cells src_off ... src_off + count - 1 of three device vectors (skr_edges' or FusedEdges' outputs)."""
        count = int(count)
        self.reserve(self.n + count)
        for src, dst in zip((rows, cols, vals), self.bufs):
            vec_copy(src, src_off, dst, self.n, count)
        self.n += count

    def prefix(self):
        """Views (rows, cols, vals) of the filled part, each len(self) x 1; None for an empty list."""
        return tuple(m.view(0, self.n) for m in self.bufs) if self.n else None

    def free(self):
        for m in self.bufs:
            m.free()
        self.bufs, self.n, self.capacity = (), 0, 0


def _count_then_write(into, width, call):
    """(count, saw_nan) of one block appended to the CellList `into` (None: counted only, `width` NULL outputs).
    call(*outputs, offset, count, nan) is the library call: it writes behind `offset` when the block fits into the
    outputs and only counts when it does not; the list then grows and the call is made once more."""
    count, nan = C.c_int64(0), C.c_int(0)
    while True:
        outs = (None,) * width if into is None else tuple(m._h for m in into.bufs)
        _lib.check(call(*outs, 0 if into is None else into.n, C.byref(count), C.byref(nan)))
        if into is None or into.n + count.value <= into.capacity:
            break
        into.reserve(into.n + count.value)  # nothing was written: once more with room
    if into is not None:
        into.n += count.value
    return count.value, bool(nan.value)


def select_cells(r, cutoff, into, nrows=None, col_begin=0, col_end=None, row_global0=0, col_global0=0):
    """Append the cells of the device block r[0:nrows, col_begin:col_end] with !(v < cutoff) to the CellList `into`, as
    (row_global0 + i, col_global0 + j, v) in np.nonzero order of the mask: NaN and cells equal to the cutoff are kept,
    zeros and the diagonal are cells like any other (skr_select_cells_ge).  Returns (count, saw_nan).  into=None: only
    the count and the flag are made."""
    head = (*block_args(r, nrows, col_begin, col_end, row_global0, col_global0), C.c_float(cutoff))
    return _count_then_write(into, 3, lambda *tail: _lib.lib().skr_select_cells_ge(*head, *tail))


class PieceList(CellList):
    """CellList's six-vector sibling: the pieces run_pieces leaves on the device — row, first, last, n_hot (uint32), peak
    (float32) and peak column (uint32).  It grows by the same count-then-write contract."""
    DTYPES = (np.uint32, np.uint32, np.uint32, np.uint32, np.float32, np.uint32)

    def to_host(self):
        """The filled part as six host arrays (copies); empty arrays for an empty list."""
        if not self.n:
            return tuple(np.empty(0, t) for t in self.DTYPES)
        return tuple(np.array(m.to_numpy(0, self.n)).reshape(-1) for m in self.bufs)


def run_pieces(r, cutoff, into, max_gap=0, seq_of_col=None, nrows=None, col_begin=0, col_end=None, row_global0=0,
               col_global0=0):
    """Append the pieces of the device block r[0:nrows, col_begin:col_end] to the PieceList `into`: per tile of one row x
    1 024 columns the maximal runs of cells with v >= float32(cutoff) (NaN never) of one sequence whose neighbouring hot
    cells are at most max_gap cold cells apart (skr_run_pieces_ge), in row-major order.  seq_of_col: a uint32 device vector
    indexed by global column, or None for one sequence.  Returns (count, saw_nan); saw_nan: any cell of the range is NaN.
    into=None: only the count and the flag are made."""
    head = (*block_args(r, nrows, col_begin, col_end, row_global0, col_global0), C.c_float(cutoff),
            None if seq_of_col is None else seq_of_col._h, int(max_gap))
    return _count_then_write(into, 6, lambda *tail: _lib.lib().skr_run_pieces_ge(*head, *tail))


class Sweep:
    """The blocks of r = a b^T / K for prepared operands (_lib.Operand), one after another in one reusable
    [stripe_rows, panel_rows] buffer: per stripe of `stripe_rows` rows of a (clamped to 1 ... a.rows), per panel of
    `panel_rows` rows of b (None: all of b), skr_pearson_gemm_op and then the visitor, before the next contraction
    overwrites the block.  b=None: the upper triangle of a against itself — a stripe's panels start at its first row
    and the visitor is told upper_only=True; else all of a x b.  This is the only producer of [stripe, panel] blocks;
    pearson_cells, pearson_topk and seekr_amd.distribution are visitors.

    The buffer is allocated by the first run() that has a block to make and kept for the next one (an order statistic
    sweeps several times) until free(); `with Sweep(...) as sweep:` frees it.  A block that is a whole operand is
    contracted from the operand itself; every other block from views that are freed when the block is done, also when
    the contraction or the visitor raises."""

    def __init__(self, a, b=None, stripe_rows=8192, panel_rows=None):
        self.a, self.b, self.upper_only = a, (a if b is None else b), b is None
        n, m = a.rows, self.b.rows
        self.stripe_rows = max(1, min(int(stripe_rows), max(n, 1)))
        self.panel_rows = max(m, 1) if panel_rows is None else max(1, min(int(panel_rows), max(m, 1)))
        self.buf = None

    def run(self, visit):
        """visit(buf, nrows=, col_begin=, col_end=, row_global0=, col_global0=, upper_only=) for every block, stripes
        outermost.  The first panel of a stripe has col_global0 == 0 in a sweep of all of a x b, and the last one ends at
        col_global0 + col_end - col_begin == b.rows.  Nothing is allocated or called when a or b has no rows."""
        a, b = self.a, self.b
        n, m = a.rows, b.rows
        if n == 0 or m == 0:
            return
        if self.buf is None:
            self.buf = a.ctx.empty(self.stripe_rows, self.panel_rows)
        for s0 in range(0, n, self.stripe_rows):
            rows = min(self.stripe_rows, n - s0)
            a_s = a if rows == n else a.view(s0, rows)
            try:
                for p0 in range(s0 if self.upper_only else 0, m, self.panel_rows):
                    cols = min(self.panel_rows, m - p0)
                    b_p = b if cols == m else b.view(p0, cols)
                    try:
                        _lib.pearson_gemm_op(a.ctx, a_s, b_p, self.buf)
                        visit(self.buf, nrows=rows, col_begin=0, col_end=cols, row_global0=s0, col_global0=p0,
                              upper_only=self.upper_only)
                    finally:
                        if b_p is not b:
                            b_p.free()
            finally:
                if a_s is not a:
                    a_s.free()

    def free(self):
        if self.buf is not None:
            self.buf.free()
            self.buf = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()


def pearson_cells(a, b, cutoff, stripe_rows=8192, panel_rows=None):
    """(cells, saw_nan, panelled): the cells of r = a b^T / K with !(r < cutoff) as a CellList (rows index a, columns
    index b), whether one of them is NaN, and whether b was cut into panels.  a, b: prepared operands (_lib.Operand) of
    one storage kind, as neighbors._prepare leaves them.  Every block of Sweep(a, b, stripe_rows, panel_rows) goes through
    select_cells.  Without panels the list is row-major; with them it is row-major within each (stripe, panel) block, the
    blocks in the sweep's order.  The caller frees the list."""
    n, m = a.rows, b.rows
    cells = CellList(a.ctx, max(1 << 16, min(int(2e-3 * n * m), 1 << 26)))
    if n == 0 or m == 0:
        return cells, False, False
    nans = []
    try:
        with Sweep(a, b, stripe_rows, panel_rows) as sweep:
            sweep.run(lambda buf, upper_only, **where: nans.append(select_cells(buf, cutoff, cells, **where)[1]))
    except BaseException:
        cells.free()
        raise
    return cells, any(nans), sweep.panel_rows < m


def topk_rows(r, k, nrows=None, col_begin=0, col_end=None, row_global0=0, col_global0=0):
    """(idx uint32 [nrows, k], val float32 [nrows, k]): the k largest cells of each row of the device
    block, descending, diagonal cell excluded — np.argsort(-row, kind="stable")[:k] per row."""
    head = block_args(r, nrows, col_begin, col_end, row_global0, col_global0)
    nrows = head[2]
    idx, val = r.ctx.empty(nrows, k, np.uint32), r.ctx.empty(nrows, k, np.float32)
    _lib.check(_lib.lib().skr_topk_rows(*head, int(k), idx._h, val._h))
    out = idx.to_numpy(), val.to_numpy()
    idx.free()
    val.free()
    return out


def pearson_topk(a, b=None, k=10, stripe_rows=8192, panel_rows=None):
    """(idx uint32 [a.rows, k], val float32 [a.rows, k]): for every row of the prepared operand `a` (seekr_amd._lib.Operand)
    the k rows of `b` it correlates with most, best first — np.argsort(-r[i], kind="stable")[:k] of r = a b^T / K with
    NaN last and ties to the smaller row of b; rows with fewer than k candidates are padded with 0xFFFFFFFF / NaN.
    b=None: `a` against itself, a row's own cell excluded.

    r never stands whole: every block of Sweep(a, b, stripe_rows, panel_rows) is merged into its stripe's running lists
    (skr_topk_merge_rows: one read of the buffer, whatever k is), which start anew at a stripe's first panel and are
    downloaded after its last; only the finished [stripe, k] lists cross PCIe.  Device memory is stripe_rows x panel_rows
    floats plus the lists.  The order is total, so the result does not depend on either split.  Operands of either kind
    (split halves or float32 layout) run the same two steps, as pearson_edges' two-step path does.  Not done here: the
    self-comparison sweeps all of a x a, not the triangle (r's symmetry is not used), and the selection is a pass of its
    own over the buffer, not part of the contraction's epilogue."""
    k = _lib.check_topk_k(k)
    ctx = a.ctx
    self_cmp = b is None
    b = a if self_cmp else b
    n, m = a.rows, b.rows
    out_idx = np.full((n, k), _lib.TOPK_PAD_IDX, dtype=np.uint32)
    out_val = np.full((n, k), np.uint32(_lib.TOPK_PAD_BITS), dtype=np.uint32).view(np.float32)
    if n == 0 or m == 0:
        return out_idx, out_val
    with contextlib.ExitStack() as held:  # the sweep's buffer, idx and val: freed however this ends
        sweep = held.enter_context(Sweep(a, b, stripe_rows, panel_rows))
        idx = ctx.empty(sweep.stripe_rows, k, np.uint32)
        held.callback(idx.free)
        val = ctx.empty(sweep.stripe_rows, k, np.float32)
        held.callback(val.free)

        def merge(buf, nrows, col_begin, col_end, row_global0, col_global0, upper_only):
            _lib.topk_merge_rows(ctx, buf, idx, val, k, first=col_global0 == 0, nrows=nrows, col_begin=col_begin,
                                 col_end=col_end, row_global0=row_global0, col_global0=col_global0, exclude_diag=self_cmp)
            if col_global0 + col_end - col_begin == m:  # the stripe's last panel
                idx.to_numpy(0, nrows, out=out_idx[row_global0:row_global0 + nrows])
                val.to_numpy(0, nrows, out=out_val[row_global0:row_global0 + nrows])

        sweep.run(merge)
    return out_idx, out_val


topk_merge_cols = _lib.topk_merge_cols  # skr_topk_merge_cols, next to _lib.topk_merge_rows


def pearson_topk_both(a, b, k=10, stripe_rows=8192, panel_rows=None, keep_device=False):
    """(idx_a uint32 [a.rows, k], val_a float32 [a.rows, k], idx_b uint32 [b.rows, k], val_b float32 [b.rows, k]) from ONE
    Sweep(a, b, stripe_rows, panel_rows): the row lists are pearson_topk(a, b, k)'s, byte for byte (every block goes
    through skr_topk_merge_rows exactly as there), and the column lists are, for every row j of `b`, the k rows of `a` it
    correlates with most in the same order, ties to the smaller row of a — every block also goes through
    skr_topk_merge_cols on a row view of resident [b.rows, k] lists, which start anew on the first stripe.  Both lists
    of a pair (i, j) hold the bits of the one r[i, j] the sweep made, which two sweeps (a x b, then b x a) do not promise.
    The order is total, so neither list depends on either split.  Device memory: pearson_topk's plus the [b.rows, k]
    column lists and, with keep_device, [a.rows, k] row lists.  keep_device=True: the four lists come back as device
    matrices (_lib.Matrix) the caller frees, and nothing is downloaded.  1 <= k <= _lib.TOPK_COLS_KMAX."""
    k = _lib.check_topk_cols_k(k)
    ctx = a.ctx
    n, m = a.rows, b.rows
    pad_val = np.uint32(_lib.TOPK_PAD_BITS)
    if n == 0 or m == 0:
        if keep_device:
            raise ValueError("keep_device needs rows on both sides (got {} and {})".format(n, m))
        return (np.full((n, k), _lib.TOPK_PAD_IDX, dtype=np.uint32), np.full((n, k), pad_val, dtype=np.uint32).view(np.float32),
                np.full((m, k), _lib.TOPK_PAD_IDX, dtype=np.uint32), np.full((m, k), pad_val, dtype=np.uint32).view(np.float32))
    out = []
    try:
        with contextlib.ExitStack() as held:  # the sweep's buffer and the stripe's row lists: freed however this ends
            sweep = held.enter_context(Sweep(a, b, stripe_rows, panel_rows))
            for rows, dtype in ((m, np.uint32), (m, np.float32)) + (((n, np.uint32), (n, np.float32)) if keep_device else ()):
                out.append(ctx.empty(rows, k, dtype))
            cidx, cval = out[0], out[1]
            if keep_device:
                all_idx, all_val = out[2], out[3]
                out_idx = out_val = None
            else:
                idx = ctx.empty(sweep.stripe_rows, k, np.uint32)
                held.callback(idx.free)
                val = ctx.empty(sweep.stripe_rows, k, np.float32)
                held.callback(val.free)
                out_idx = np.full((n, k), _lib.TOPK_PAD_IDX, dtype=np.uint32)
                out_val = np.full((n, k), pad_val, dtype=np.uint32).view(np.float32)

            def merge(buf, nrows, col_begin, col_end, row_global0, col_global0, upper_only):
                where = dict(nrows=nrows, col_begin=col_begin, col_end=col_end, row_global0=row_global0,
                             col_global0=col_global0, exclude_diag=False)
                cols = col_end - col_begin
                if keep_device:  # the stripe's rows of the resident row lists
                    ridx, rval = all_idx.view(row_global0, nrows), all_val.view(row_global0, nrows)
                else:
                    ridx, rval = idx, val
                pidx, pval = cidx.view(col_global0, cols), cval.view(col_global0, cols)
                try:
                    _lib.topk_merge_rows(ctx, buf, ridx, rval, k, first=col_global0 == 0, **where)
                    _lib.topk_merge_cols(ctx, buf, pidx, pval, k, first=row_global0 == 0, **where)
                finally:
                    for v in (pidx, pval) + ((ridx, rval) if keep_device else ()):
                        v.free()
                if not keep_device and col_global0 + cols == m:  # the stripe's last panel
                    idx.to_numpy(0, nrows, out=out_idx[row_global0:row_global0 + nrows])
                    val.to_numpy(0, nrows, out=out_val[row_global0:row_global0 + nrows])

            sweep.run(merge)
        if keep_device:
            return out[2], out[3], out[0], out[1]
        res = out_idx, out_val, np.array(cidx.to_numpy()), np.array(cval.to_numpy())
    except BaseException:
        for x in out:
            x.free()
        raise
    for x in out:
        x.free()
    return res


class PairList(CellList):
    """CellList's five-vector sibling: the pairs knn_pairs leaves on the device — row, col (uint32), value (float32),
    rank_row, rank_col (uint32; 0xFFFFFFFF = the pair is not in that side's list).  It grows by the same
    count-then-write contract; its first three vectors are an edge list as leiden.communities takes it."""
    DTYPES = (np.uint32, np.uint32, np.float32, np.uint32, np.uint32)

    def to_host(self):
        """The filled part as five host arrays (copies); empty arrays for an empty list."""
        if not self.n:
            return tuple(np.empty(0, t) for t in self.DTYPES)
        return tuple(np.array(m.to_numpy(0, self.n)).reshape(-1) for m in self.bufs)


KNN_MODES = {"mutual": 0, "union": 1}


def knn_mode(mode):
    """0 / 1 for "mutual" / "union"; ValueError otherwise (no device call)."""
    if mode not in KNN_MODES:
        raise ValueError("mode is 'mutual' or 'union' (got {!r})".format(mode))
    return KNN_MODES[mode]


def knn_pairs(idx_a, val_a, idx_b=None, val_b=None, mode="mutual", positive_only=False, into=None):
    """Append the nearest-neighbour pairs of top-k lists on the device (skr_knn_pairs) to the PairList `into`; returns
    their number.  idx_a / val_a [n1, k]: row lists whose entries index set B; idx_b / val_b [n2, k]: column lists
    whose entries index set A (pearson_topk_both's four lists, keep_device=True).  idx_b = val_b = None: the self form —
    one set, every pair once with row < col.  mode "mutual": pairs in both lists; "union": in either.  A pair's value is
    its row-list entry's bits when there is one, else its column-list entry's; padded slots and NaN values never pair;
    positive_only drops pairs whose value is not > 0.  Pairs come in ascending (row, col) order.  into=None: only the
    count is made."""
    code = knn_mode(mode)
    if (idx_b is None) != (val_b is None):
        raise ValueError("pass idx_b and val_b, or neither")
    head = (idx_a.ctx._h, idx_a._h, val_a._h, None if idx_b is None else idx_b._h, None if val_b is None else val_b._h, code,
            1 if positive_only else 0)
    return _count_then_write(into, 5, lambda *tail: _lib.lib().skr_knn_pairs(*head, *tail[:-1]))[0]


FUSE_MAX_DENSITY = 1e-3  # edges per cell above which the fused epilogue costs more than writing the stripe (measured: 100 000 rows, k = 6)


def pearson_edges(z, cutoff, stripe_rows=8192, upper_only=True, engine_gemm=None, fuse="auto", into=None):
    """Edge list of the self-comparison of the prepared operand `z` (seekr_amd._lib.Operand):
    r is produced one stripe of `stripe_rows` rows at a time into one reusable buffer (columns at or
    right of the stripe when `upper_only`) and reduced to edges before the next stripe overwrites
    it, so memory is stripe_rows x N floats instead of N x N (config 5: 32 GB instead of 4 TB).
    Returns (rows, cols, vals) in row-major order: what np.nonzero / indexing of the thresholded,
    zero-diagonal matrix (kmer_leiden.py:94-96) gives — its upper triangle when `upper_only`.
    `fuse`: True — the threshold runs inside the contraction's epilogue (FusedEdges) and no stripe of r is ever
    written; False — the two-step path (contraction into a stripe buffer, then skr_edges); "auto" (default) — fused as
    long as the stripes seen so far hold fewer than FUSE_MAX_DENSITY edges per cell (a sparse list: 15 % faster at
    1e-5 edges per cell; a dense one — the reference's default cutoff 0 keeps half the cells — is cheaper through the
    stripe buffer).  The result is the same, bit for bit, whichever path a stripe takes.
    into: a CellList every stripe's edges are appended to on the device (the fused buffers' filled prefix, or skr_edges'
    outputs, through skr_vec_copy) — the same list in the same order, never on the host; the return value is then the
    number of edges."""
    ctx = z.ctx
    n = z.rows
    stripe_rows = max(1, min(int(stripe_rows), n))
    fused = FusedEdges(ctx) if z.kind != 0 and fuse else None  # float32-layout operands: two-step path
    buf = None
    out = ([], [], [])
    seen_cells = seen_edges = 0
    for s0 in range(0, n, stripe_rows):
        rows = min(stripe_rows, n - s0)
        c0 = s0 if upper_only else 0
        a = z.view(s0, rows)
        b = z.view(c0, n - c0) if c0 else z
        use_fused = fused is not None and (fuse is True or seen_edges <= FUSE_MAX_DENSITY * max(seen_cells, 1))
        part = None
        if use_fused:
            if z.cols > 1024 and buf is None:
                buf = ctx.empty(stripe_rows, n)  # k = 7: the earlier k chunks need a block to leave their sums in
            part = fused.block(a, b, cutoff, row_global0=s0, col_global0=c0, upper_only=upper_only, scratch=buf,
                               retry=fuse is True, into=into)
            if part is None:  # denser than the list buffers: through the stripe buffer from here on
                fused.free()
                fused = None
        if part is None:
            if buf is None:
                buf = ctx.empty(stripe_rows, n)
            _lib.pearson_gemm_op(ctx, a, b, buf, symmetric=False, row0=0, col0=c0)
            part = edges(buf, cutoff, nrows=rows, col_begin=c0, col_end=n, row_global0=s0, col_global0=0,
                         upper_only=upper_only, into=into)
        seen_cells += rows * (n - c0)
        seen_edges += part if into is not None else len(part[2])
        if into is None:
            for acc, p in zip(out, part):
                acc.append(p)
    if fused:
        fused.free()
    if buf is not None:
        buf.free()
    if into is not None:
        return seen_edges
    return tuple(np.concatenate(p) if p else np.empty(0) for p in out)


ADJ_METHODS = {"bonferroni": 0, "sidak": 1, "holm-sidak": 2, "holm": 3, "simes-hochberg": 4, "hommel": 5, "fdr_bh": 6,
               "fdr_by": 7, "fdr_tsbh": 8, "fdr_tsbky": 9, "fdr_gbs": 10}
_ADJ_ALIASES = {"bonferroni": ["b", "bonf"], "sidak": ["s"], "holm-sidak": ["hs"], "holm": ["h"], "simes-hochberg": ["sh"],
                "hommel": ["ho"], "fdr_bh": ["fdr_i", "fdr_p", "fdri", "fdrp"], "fdr_by": ["fdr_n", "fdr_c", "fdrn", "fdrcorr"],
                "fdr_tsbh": ["fdr_2sbh"], "fdr_tsbky": ["fdr_2sbky", "fdr_twostage"], "fdr_gbs": []}
ADJ_ALIASES = {a: name for name, more in _ADJ_ALIASES.items() for a in [name] + more}
HOMMEL_LIMIT = 1 << 22


def adjust_method(method):
    """The canonical multipletests name of `method` (aliases, any letter case); ValueError('method not recognized')."""
    name = ADJ_ALIASES.get(str(method).lower())
    if name is None:
        raise ValueError("method not recognized")
    return name


def adjust_out_dtype(method, dtype, symmetric):
    """dtype of adj_pval's result: float64, or the input dtype for bonferroni, sidak and hommel on the whole matrix."""
    if not symmetric and adjust_method(method) in ("bonferroni", "sidak", "hommel"):
        return np.dtype(dtype)
    return np.dtype(np.float64)


def check_hommel(method, n_tests):
    if adjust_method(method) == "hommel" and n_tests > HOMMEL_LIMIT:
        raise NotImplementedError("hommel on the device is limited to {} tests; this matrix has {}".format(HOMMEL_LIMIT,
                                                                                                          n_tests))


def pvals_symmetric(p):
    """is_symmetric's value test of the device matrix p (square; off the diagonal round(x, 5) equals its mirror)."""
    flag = C.c_int(0)
    _lib.check(_lib.lib().skr_pvals_symmetric(p.ctx._h, p._h, C.byref(flag)))
    return bool(flag.value)


def adjust_pvalues(p, method, alpha=0.05, symmetric=None):
    """multipletests(tests, alpha, method)[1] of the device matrix p (float32 or float64), left on the device: the
    tests are the strict upper triangle when p is symmetric (an [N, N] float64 result, NaN elsewhere), else all of p
    (p's shape, the method's dtype).  symmetric=None tests the values (skr_pvals_symmetric); labels are the caller's.
    Bit-exact with statsmodels 0.12.2 except sidak's float32 power (evaluated in float64 and rounded once: numpy's
    float32 power is not correctly rounded) and holm-sidak's float64 power (device pow, within a few ulp); tied
    negative p-values are outside the contract (numpy's unstable argsort decides those)."""
    name = adjust_method(method)
    if symmetric is None:
        symmetric = pvals_symmetric(p)
    symmetric = bool(symmetric) and p.rows == p.cols
    n_tests = p.rows * (p.rows - 1) // 2 if symmetric else p.rows * p.cols
    check_hommel(name, n_tests)
    out = p.ctx.empty(p.rows, p.cols, adjust_out_dtype(name, p.dtype, symmetric))
    _lib.check(_lib.lib().skr_adjust_pvalues(p.ctx._h, p._h, ADJ_METHODS[name], C.c_double(float(alpha)),
                                             1 if symmetric else 0, out._h))
    return out


HEAD_METHODS = ("bonferroni", "sidak", "holm-sidak", "holm", "simes-hochberg", "fdr_bh", "fdr_by")
HEAD_REFUSED = ("hommel", "fdr_tsbh", "fdr_tsbky", "fdr_gbs")


def head_method(method):
    """adjust_method(method) if the method can be corrected from the smallest p-values alone (HEAD_METHODS);
    NotImplementedError naming the four that cannot (no device call)."""
    name = adjust_method(method)
    if name in HEAD_REFUSED:
        raise NotImplementedError(
            "{} cannot be corrected from the smallest p-values alone: {} depend on the tests above alpha or on a rejection "
            "count that rescales alpha; use adjust_pvalues on the whole matrix".format(name, ", ".join(HEAD_REFUSED)))
    return name


def adjust_pvalues_head(p, ntests, method, alpha=0.05):
    """The corrected values (1 x E float64 device vector) of the E smallest of `ntests` tests, given in any order in the
    device vector p (float32 or float64): what adjust_pvalues(symmetric=True) gives those tests among all `ntests`, the
    missing ones taken to be larger than every given one (skr_adjust_pvalues_head).  HEAD_METHODS only."""
    name = head_method(method)
    n = p.rows * p.cols
    if int(ntests) < n:
        raise ValueError("ntests ({}) is smaller than the {} p-values given".format(int(ntests), n))
    if int(ntests) == 0:
        raise ZeroDivisionError("float division by zero")
    out = p.ctx.empty(1, n, np.float64)
    if n:
        _lib.check(_lib.lib().skr_adjust_pvalues_head(p.ctx._h, p._h, int(ntests), ADJ_METHODS[name], C.c_double(float(alpha)),
                                                      out._h))
    return out


def select_le(values, bound):
    """(index, count): the positions i of the device vector `values` (float32 or float64) with float64(values[i]) <= bound,
    ascending, as the first `count` cells of a uint32 device vector (skr_select_le: count, then write); NaN never
    passes.  index is None when nothing passes."""
    ctx = values.ctx
    count = C.c_int64(0)
    if values.rows * values.cols == 0:
        return None, 0
    _lib.check(_lib.lib().skr_select_le(ctx._h, values._h, C.c_double(float(bound)), None, C.byref(count)))
    n = count.value
    if n == 0:
        return None, 0
    index = ctx.empty(1, n, np.uint32)
    _lib.check(_lib.lib().skr_select_le(ctx._h, values._h, C.c_double(float(bound)), index._h, C.byref(count)))
    return index, n


def gather_index(src, index, count):
    """1 x count device vector out[i] = src[index[i]] (src: uint32, float32 or float64 cells; index as select_le gives it)."""
    out = src.ctx.empty(1, int(count), src.dtype)
    if count:
        _lib.check(_lib.lib().skr_gather_index(src.ctx._h, src._h, index._h, int(count), out._h))
    return out
