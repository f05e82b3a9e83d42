"""The significantly similar pairs of a self-comparison, or of one set of rows against another, on MI355X without any
N x N matrix: which cells of the corrected p-value matrix are <= alpha, with their r, p and corrected p.  The reference
answers this with three matrices (pearson, find_pval, adj_pval); the specification here is this package's own
full-matrix path on the same operand,

    r = pearson_gemm_op(z, z);  p = parametric_pvalues(r, ...) or empirical_pvalues(r, ...)
    p_adj = adjust_pvalues(p, method, alpha, symmetric=True);  the cells p_adj <= alpha in np.nonzero order

bit for bit.  It rests on two facts (DESIGN_PARITY.md, "significant_pairs"): a p-value is a non-increasing function of
r, so the cells with p <= alpha are the cells with r >= r0 for a cutoff found before the contraction runs, which the
fused edge list delivers; and for the seven methods of consumers.HEAD_METHODS a corrected value <= alpha depends only on
the tests with p <= alpha and on the number of tests (consumers.adjust_pvalues_head).

Two sets (`other`, `counts2`): the reference's find_pval(seq1file, seq2file) followed by adj_pval on the whole
non-symmetric matrix.  The specification is the same path with symmetric=False and n1 x n2 tests; every cell is a test, the
cell (i, i) included, so the candidates come from consumers.pearson_cells (skr_select_cells_ge: no zero rule, no diagonal
rule) and never leave the device.  p_adj is float64 here whatever the method: for bonferroni and sidak, which the full
path returns in float32, it is the widening of that float32 (DESIGN_PARITY.md).
"""
import numpy as np

from seekr_amd import _lib, consumers

GUARD_STEPS = 64     # float32 steps the cutoff is lowered by below the crossing the search finds
SEARCH_LO, SEARCH_HI = np.float32(-2.0), np.float32(2.0)


class SignificantPairs:
    """rows, cols (uint32), r, p (float32), p_adj (float64): the significant pairs in np.nonzero order;
    r_cutoff = the cutoff the candidate list was taken at (None when the search found none), n_candidates = the length
    of that list.  Self-comparison: row < col, both index the one set, n_tests = N (N - 1) / 2.  Two sets: rows index
    the first set (`z`, `counts`), cols the second (`other`, `counts2`), n_tests = N1 N2."""

    def __init__(self, n_tests, r_cutoff=None, n_candidates=0, rows=None, cols=None, r=None, p=None, p_adj=None):
        self.n_tests, self.r_cutoff, self.n_candidates = int(n_tests), r_cutoff, int(n_candidates)
        self.rows = np.empty(0, np.uint32) if rows is None else rows
        self.cols = np.empty(0, np.uint32) if cols is None else cols
        self.r = np.empty(0, np.float32) if r is None else r
        self.p = np.empty(0, np.float32) if p is None else p
        self.p_adj = np.empty(0, np.float64) if p_adj is None else p_adj

    def __len__(self):
        return len(self.rows)

    def __repr__(self):
        return "SignificantPairs({} of {} tests, r_cutoff={!r}, n_candidates={})".format(len(self), self.n_tests, self.r_cutoff,
                                                                                      self.n_candidates)


# ---- the float32 ordering ---------------------------------------------------------------------------------------------
def _key(x):
    """float32 -> int whose order is the order of the values (-0.0 just below +0.0): consumers.float32_key of a scalar."""
    return int(consumers.float32_key(np.float32(x))[0])


def _unkey(k):
    return consumers.float32_unkey(k)[()]


def float32_steps(x, steps):
    """The float32 `steps` places above (below: negative) x in the ordering of the finite values."""
    return _unkey(_key(x) + int(steps))


def alpha_float32(alpha):
    """The smallest float32 >= alpha: p is float32, so p <= alpha32 is p <= alpha."""
    return consumers.ceil_float32(np.array([alpha]))[0]


def find_cutoff(p_of, alpha32, lo=SEARCH_LO, hi=SEARCH_HI):
    """The smallest float32 r* in [lo, hi] with p_of(r*) <= alpha32, by bisection on the float32 ordering (at most 32
    steps), for a non-increasing p_of: float32 array -> float32 array.  None when p_of(hi) is NaN or above alpha32 (a
    p-value that is NaN everywhere, or no crossing)."""
    one = lambda x: p_of(np.array([x], dtype=np.float32)).reshape(-1)[0]  # noqa: E731
    if not one(hi) <= alpha32:
        return None
    if one(lo) <= alpha32:
        return np.float32(lo)
    a, b = _key(lo), _key(hi)  # p(a) > alpha32 or NaN, p(b) <= alpha32
    for _ in range(32):
        if b - a <= 1:
            break
        mid = (a + b) // 2
        if one(_unkey(mid)) <= alpha32:
            b = mid
        else:
            a = mid
    assert b - a <= 1
    return _unkey(b)


def cutoff_with_guard(r_star):
    """r0: r* lowered by GUARD_STEPS float32 steps.  ValueError when r0 <= 0."""
    r0 = float32_steps(r_star, -GUARD_STEPS)
    if not r0 > 0:
        raise ValueError("the background's alpha quantile is not positive (r cutoff {!r}): the candidate list would hold half "
                         "the matrix and the edge extraction drops cells that are exactly 0; use the full-matrix path "
                         "(pearson, pvalues, adjust_pvalues)".format(float(r0)))
    return r0


# ---- the p-value of a device vector of r ------------------------------------------------------------------------------
class _PValues:
    """find_pval's p-value step (consumers.pvalues_host's two branches) prepared once: the sorted background stays on the
    device between calls.  __call__(r) -> device matrix of r's shape."""

    def __init__(self, ctx, fitres, bestfit):
        self.ctx, self.bg, self.params = ctx, None, None
        if isinstance(fitres, np.ndarray):
            fitres = fitres.reshape(-1)
            self.total = len(fitres)
            if fitres.dtype != np.float32:
                fitres = consumers.ceil_float32(fitres)
            self.sorted_bg = np.sort(fitres[~np.isnan(fitres)])
        else:
            self.name, _, params = fitres[bestfit - 1]  # IndexError as find_pval's
            self.params = tuple(params)

    def __call__(self, r):
        if self.params is not None:
            return consumers.parametric_pvalues(r, self.name, self.params)
        if len(self.sorted_bg) == 0:
            return self.ctx.zeros(r.rows, r.cols)
        if self.bg is None:
            self.bg = self.ctx.from_numpy(self.sorted_bg)
        p = self.ctx.empty(r.rows, r.cols)
        _lib.check(_lib.lib().skr_empirical_pvalues(self.ctx._h, r._h, self.bg._h, int(self.total), p._h))
        return p

    def host(self, values):
        """p of a host float32 array, through the device."""
        d = self.ctx.from_numpy(np.ascontiguousarray(values, dtype=np.float32))
        p = self(d)
        out = np.array(p.to_numpy()).reshape(-1)
        d.free()
        p.free()
        return out

    def free(self):
        if self.bg is not None:
            self.bg.free()
            self.bg = None


def row_major_order(rows, cols):
    """The permutation that puts a (row, col) list into np.nonzero order: by row, then by column."""
    return np.lexsort((np.asarray(cols), np.asarray(rows)))


NAN_MESSAGE = ("r is NaN for some pair (a constant row): every corrected p-value of the full-matrix path is NaN as well; "
               "remove such rows first")


def _check_arguments(fitres, bestfit, method, alpha, candidates="host"):
    name = consumers.head_method(method)
    if not 0 < float(alpha) < 1:
        raise ValueError("alpha must lie strictly between 0 and 1 (got {!r})".format(alpha))
    if candidates not in ("host", "device"):
        raise ValueError("candidates must be 'host' or 'device' (got {!r})".format(candidates))
    if not isinstance(fitres, np.ndarray):
        fitres[bestfit - 1]  # the IndexError find_pval gives (find_pval.py:118)
    return name


def correct_candidates(pv, d_rows, d_cols, d_r, n_tests, name, alpha, held, lap=lambda step: None):
    """From the candidate list on the device (three vectors: row, column, r; every cell with p <= alpha among them) to
    the significant cells on the host: [rows, cols, r, p, p_adj] in the list's order, or None when there are none.  The
    p-values of the candidates (pv: _PValues), the cells with p <= alpha, their correction among all n_tests tests
    (consumers.adjust_pvalues_head, method `name`), the cells with corrected p <= alpha; only those leave the device.
    Every device matrix made on the way is appended to `held` for the caller to free."""
    d_p = pv(d_r)
    held.append(d_p)
    lap("p_values")
    idx, kept = consumers.select_le(d_p, float(alpha_float32(alpha)))
    if kept == 0:
        return None
    held.append(idx)
    lists = [consumers.gather_index(m, idx, kept) for m in (d_rows, d_cols, d_r, d_p)]
    held += lists
    lap("selection")
    d_adj = consumers.adjust_pvalues_head(lists[3], n_tests, name, alpha)
    held.append(d_adj)
    lap("correction")
    idx2, sig = consumers.select_le(d_adj, float(alpha))
    if sig == 0:
        return None
    held.append(idx2)
    final = [consumers.gather_index(m, idx2, sig) for m in lists + [d_adj]]
    held += final
    return [np.array(m.to_numpy()).reshape(-1) for m in final]


def pearson_significant(z, fitres, bestfit=1, method="fdr_bh", alpha=0.05, stripe_rows=8192, fuse="auto", timings=None,
                        other=None, panel_rows=None, candidates="host"):
    """The significant pairs (SignificantPairs) of the self-comparison of the prepared operand `z` (seekr_amd._lib.Operand,
    as pearson_edges takes it): the cells of adjust_pvalues(p, method, alpha, symmetric=True) that are <= alpha, with
    p = find_pval's p-values of r against `fitres` — find_dist's list of (name, deviance, parameters) (entry `bestfit`,
    counted from 1) or a 1-D array of background similarities.  method: one of consumers.HEAD_METHODS.

    Steps: the r cutoff r0 (find_cutoff on the device's own p-value kernel, lowered by GUARD_STEPS float32 steps), the
    candidate list pearson_edges(z, r0) (stripe_rows, fuse: as there), its p-values, the cells with p <= alpha,
    their correction among all N (N - 1) / 2 tests, the cells with corrected p <= alpha.  The candidate list is uploaded
    once; after that only the final lists leave the device.  ValueError: r0 <= 0 (use the full-matrix path), a NaN
    among the candidates (a constant row).  `timings`: a dict that receives the seconds of each step.

    candidates="device": the candidate list never visits the host — the fused buffers' filled prefix (or skr_edges'
    outputs) is appended to a consumers.CellList with skr_vec_copy; the result is the same in every byte.

    other: a second prepared operand of z's storage kind (neighbors._prepare): the rows of z against the rows of `other`,
    n_tests = z.rows x other.rows, every cell a test.  The candidates are consumers.pearson_cells(z, other, r0,
    stripe_rows, panel_rows) and stay on the device (`fuse` and `candidates` do not apply); with panels the final lists
    are put into (row, col) order on the host.  rows index z, cols index `other`."""
    import time
    name = _check_arguments(fitres, bestfit, method, alpha, candidates)
    ctx = z.ctx
    n = z.rows
    n_tests = n * (n - 1) // 2 if other is None else n * other.rows
    if n_tests == 0:
        return SignificantPairs(n_tests)
    alpha32 = alpha_float32(alpha)
    clock = [time.perf_counter()]

    def lap(step):
        if timings is not None:
            ctx.sync()
            now = time.perf_counter()
            timings[step] = timings.get(step, 0.0) + now - clock[0]
            clock[0] = now

    pv = _PValues(ctx, fitres, bestfit)
    held = []
    try:
        r_star = find_cutoff(pv.host, alpha32)
        lap("cutoff_search")
        if r_star is None:
            return SignificantPairs(n_tests)
        r0 = cutoff_with_guard(r_star)
        panelled = False
        if other is not None or candidates == "device":
            if other is not None:
                cells, saw_nan, panelled = consumers.pearson_cells(z, other, float(r0), stripe_rows=stripe_rows,
                                                                   panel_rows=panel_rows)
                held.append(cells)
            else:
                cells = consumers.CellList(ctx)
                held.append(cells)
                consumers.pearson_edges(z, float(r0), stripe_rows=stripe_rows, upper_only=True, fuse=fuse, into=cells)
                saw_nan = False
                if len(cells):  # a NaN among the values: the cells of the value vector (one column) that are not below +inf
                    views = cells.prefix()
                    saw_nan = consumers.select_cells(views[2], np.inf, None)[1]
                    for v in views:
                        v.free()
            n_cand = len(cells)
            lap("edge_list")
            if n_cand == 0:
                return SignificantPairs(n_tests, r0, 0)
            if saw_nan:
                raise ValueError(NAN_MESSAGE)
            d_rows, d_cols, d_r = cells.prefix()
            held[:0] = [d_rows, d_cols, d_r]  # the views go before the list they look into
            if timings is not None:
                timings["bytes_to_device"] = 0
        else:
            rows, cols, vals = consumers.pearson_edges(z, float(r0), stripe_rows=stripe_rows, upper_only=True, fuse=fuse)
            n_cand = len(vals)
            lap("edge_list")
            if n_cand == 0:
                return SignificantPairs(n_tests, r0, 0)
            if np.isnan(vals).any():
                raise ValueError(NAN_MESSAGE)
            d_rows, d_cols, d_r = (ctx.from_numpy(np.ascontiguousarray(a)) for a in (rows.astype(np.uint32, copy=False),
                                                                                    cols.astype(np.uint32, copy=False), vals))
            held += [d_rows, d_cols, d_r]
            if timings is not None:
                timings["bytes_to_device"] = n_cand * 12
        out = correct_candidates(pv, d_rows, d_cols, d_r, n_tests, name, alpha, held, lap)
        if out is None:
            return SignificantPairs(n_tests, r0, n_cand)
        sig = len(out[0])
        if panelled:  # the list came block by block: np.nonzero order is restored on the few cells that are left
            order = row_major_order(out[0], out[1])
            out = [a[order] for a in out]
        lap("selection")
        if timings is not None:
            timings["bytes_to_host"] = sig * (4 + 4 + 4 + 4 + 8)
        return SignificantPairs(n_tests, r0, n_cand, *out)
    finally:
        pv.free()
        for m in held:
            m.free()


@_lib.api_call
def significant_pairs(counts, fitres, bestfit=1, method="fdr_bh", alpha=0.05, counts2=None, **kw):
    """pearson_significant for a host count matrix (anything np.ascontiguousarray(.., float32) accepts): the rows are
    prepared as pearson() and nearest() prepare a self-comparison.  counts2 (not None and not `counts` itself): the
    rows of counts against the rows of counts2, both prepared as pearson() and nearest() prepare two sets.
    `kw`: stripe_rows, fuse, timings, panel_rows, candidates."""
    from seekr_amd import neighbors
    _check_arguments(fitres, bestfit, method, alpha, kw.get("candidates", "host"))
    same = counts2 is None or counts2 is counts
    c = neighbors._f32(counts)
    c2 = c if same else neighbors._f32(counts2)
    if c.ndim != 2 or c2.ndim != 2:
        raise ValueError("counts must be a 2-D matrix")
    if c.shape[1] != c2.shape[1]:
        raise ValueError("counts and counts2 must have the same number of columns ({} and {})".format(c.shape[1], c2.shape[1]))
    if not same and (c.shape[0] == 0 or c2.shape[0] == 0):
        return SignificantPairs(0)
    ctx = _lib.default_context()
    z, z2 = neighbors._prepare(ctx, c, c2, same)
    try:
        return pearson_significant(z, fitres, bestfit=bestfit, method=method, alpha=alpha, other=z2, **kw)
    finally:
        z.free()
        if z2 is not None:
            z2.free()
