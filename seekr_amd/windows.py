"""k-mer profiles of sliding windows and `domain_pearson` on MI355X: which part of a long transcript or of a genomic region
resembles a query.  The reference has no such function; the specification is an equivalence:

    the row of a window equals, bit for bit, the row `BasicCounter` gives when the window's substring is handed to it as
    a sequence of its own — same k, alphabet, log2, mean and std, same exceptions.

No substring is made anywhere: the target is packed and uploaded once (2 bits per base) and every window is counted from
the packed text at its base offset (`skr_count_windows_*`, csrc/windows.hip).  `domain_pearson` runs count -> normalise ->
operand fill -> contraction one chunk of window rows at a time, so the window matrix (16 KiB a row at k = 6) never
exists whole either.  Four distinct letters and k <= 7; anything else raises NotImplementedError.
"""
import os
from collections import namedtuple

import numpy as np

from seekr_amd import _lib
from seekr_amd import pearson as pearson_mod
from seekr_amd.consumers import float32_key, float32_unkey
from seekr_amd.fasta_reader import Reader
from seekr_amd.kmer_counts import NAN_WARNING, BasicCounter, _as_device_vector

WindowCounts = namedtuple("WindowCounts", ["counts", "table", "mean", "std"])


def window_table(lengths, window, slide):
    """The windows of sequences of the given lengths: int64 arrays (seq_index, start, length), ordered by sequence, then by
    start.  A sequence of length L has the starts j * slide for j = 0 ... ceil(max(L - window, 0) / slide); the window is
    seq[start : start + window] as Python slices it, so the last one may be shorter and a sequence shorter than `window`
    is one window."""
    window, slide = int(window), int(slide)
    if window < 1:
        raise ValueError("window must be at least 1 (got {})".format(window))
    if slide < 1:
        raise ValueError("slide must be at least 1 (got {})".format(slide))
    if slide > window:
        raise ValueError("slide ({}) must not exceed window ({}): bases between two windows would be skipped".format(slide, window))
    lengths = np.asarray(lengths, dtype=np.int64).reshape(-1)
    per_seq = np.where(lengths > window, (lengths - window + slide - 1) // slide + 1, 1)
    first_row = np.zeros(len(lengths) + 1, dtype=np.int64)
    np.cumsum(per_seq, out=first_row[1:])
    seq_index = np.repeat(np.arange(len(lengths), dtype=np.int64), per_seq)
    start = (np.arange(first_row[-1], dtype=np.int64) - first_row[seq_index]) * slide
    length = np.minimum(window, lengths[seq_index] - start)
    return seq_index, start, length


def _holder(infasta_or_seqs, k, log2, alphabet):
    """A BasicCounter that only holds the input: its constructor reads a FASTA file the way the reference does (and raises
    what the reference raises), `seqs` assignment keeps the caller's strings as they are (lower case is then skipped)."""
    if isinstance(infasta_or_seqs, (str, bytes, os.PathLike)):
        holder = BasicCounter(os.fspath(infasta_or_seqs), k=k, mean=False, std=False, log2=log2, silent=True, alphabet=alphabet)
    else:
        holder = BasicCounter(k=k, mean=False, std=False, log2=log2, silent=True, alphabet=alphabet)
        holder.seqs = list(infasta_or_seqs)
    holder._check_k()
    if not holder._two_bit:
        raise NotImplementedError("windows are counted by the 2-bit kernels: an alphabet of four distinct letters is needed "
                                  "(got {!r})".format(alphabet))
    return holder


def _headers(holder):
    if holder.infasta is None:
        return None
    held = holder._packed if holder._packed is not None else holder._fasta
    return held.headers() if held is not None else Reader(holder.infasta).get_headers()


def _frame(columns):
    from pandas import DataFrame
    return DataFrame(columns)


def _chunks(n_rows, chunk_rows):
    chunk_rows = n_rows if not chunk_rows else max(1, int(chunk_rows))
    return [(r0, min(chunk_rows, n_rows - r0)) for r0 in range(0, n_rows, max(chunk_rows, 1))]


@_lib.api_call
def window_counts(infasta_or_seqs, k, window, slide, mean=True, std=True, log2="Log2.post", alphabet="AGTC", chunk_rows=None):
    """`BasicCounter(...).get_counts()` over the sliding windows of the input (a FASTA path, or a list of strings as assigned
    to `BasicCounter.seqs`): WindowCounts(counts, table, mean, std).

    counts: float32 [n_windows, 4^k], normalised as BasicCounter normalises the substrings — mean / std True: computed
    over the windows; a path or an array: used as given; False: the step is skipped.  table: DataFrame with `seq_index`,
    `start`, `length` (and `header` first for FASTA input).  mean, std: what BasicCounter leaves in `.mean` / `.std`.
    chunk_rows: rows per counting launch (None: all at once); the rows do not depend on it.  The whole matrix stands on
    the device here (the column statistics need it): `domain_pearson` is the form that does not."""
    holder = _holder(infasta_or_seqs, k, log2, alphabet)
    mean = np.load(mean) if isinstance(mean, str) else mean
    std = np.load(std) if isinstance(std, str) else std
    packed = holder._packed_seqs()
    seq_index, start, length = window_table(packed.lengths(), window, slide)
    n_rows = len(seq_index)
    if n_rows == 1 and std is True:  # kmer_counts.py:124-130 on the substrings
        raise ValueError("You cannot standardize a single sequence. Please pass the path to an std. dev. array, "
                         "or use raw counts by setting std=False.")
    ctx = holder._ctx()
    dev = ctx.empty(n_rows, 4 ** k)
    for r0, n in _chunks(n_rows, chunk_rows):
        _lib.count_windows(ctx, packed, k, window, slide, r0, n, log2_pre=(log2 == "Log2.pre"),
                           out=dev if n == n_rows else dev.view(r0, n))
    mean_mode, mean_vec = 0, None
    if mean is True:
        mean_mode = 1
    elif mean is not False:
        mean_mode, mean_vec = 2, _as_device_vector(ctx, mean, dev.cols, dev.rows)
    std_mode, std_vec = 0, None
    if std is True:
        std_mode = 1
    elif std is not False:
        std_mode, std_vec = 2, _as_device_vector(ctx, std, dev.cols, dev.rows)
    # Log2.pre was fused into the counting flush, so the normaliser sees 'none' for it
    mean_out, std_out, has_nan = _lib.normalize(ctx, dev, "Log2.post" if log2 == "Log2.post" else "Log2.none", mean_mode,
                                                mean_vec, std_mode, std_vec)
    if mean_out is not None:
        mean = mean_out.vector()
    if std_out is not None:
        std = std_out.vector()
    if has_nan:
        print(NAN_WARNING)
    columns = {"seq_index": seq_index, "start": start, "length": length}
    headers = _headers(holder)
    if headers is not None:
        columns = dict(header=np.asarray(headers, dtype=object)[seq_index], **columns)
    return WindowCounts(dev.to_numpy(), _frame(columns), mean, std)


def _fixed_vector(vec, name):
    if isinstance(vec, (str, os.PathLike)):
        vec = np.load(vec)
    if vec is None or isinstance(vec, (bool, np.bool_)):
        raise ValueError("domain_pearson needs `{}` as a vector (an array or the path of a .npy file): the windows are "
                         "normalised chunk by chunk, which is only defined with fixed vectors".format(name))
    return vec


class _Side:
    """One operand of the chunked contraction in the layout asked for, refilled in float32 layout when a fill routes rows
    there (skr_operand_kind: both operands of a contraction must have the same kind)."""

    def __init__(self, ctx, rows, cols, precision):
        self.ctx, self.rows, self.cols, self.precision = ctx, rows, cols, precision
        self.ops, self.kinds = {}, {}

    def fill(self, x, precision, **tail):
        op = self.ops.get(precision)
        if op is not None and op.kind != self.kinds[precision]:
            # a full-size fill routed the cached operand itself, and skr_operand_fill keeps that kind: without a new operand
            # every later chunk would be filled twice and contracted in float32 layout, whatever its rows are
            op = None
        if op is None:
            op = self.ops[precision] = _lib.Operand(self.ctx, self.rows, self.cols, precision)
            self.kinds[precision] = op.kind
        view = op if x.rows == self.rows else op.view(0, x.rows)
        _, has_nan = _lib.operand_fill(self.ctx, x, view, precision, want_nan=True, **tail)
        return view, has_nan


class _DomainRun:
    """The loop domain_pearson and domain_topk share: the target packed and its window table, the query operand filled
    once, and per chunk of window rows count -> normalise -> operand fill -> contraction into one reusable block."""

    def __init__(self, query, target, k, window, slide, mean, std, log2, chunk_rows, what):
        mean, std = _fixed_vector(mean, "mean"), _fixed_vector(std, "std")
        cols = 4 ** k
        qmat = None
        if not isinstance(query, (str, bytes, os.PathLike)):  # (checked first: reading the target already packs it on the device)
            qmat = np.asarray(query)
            if qmat.ndim != 2 or qmat.shape[1] != cols or qmat.dtype != np.float32:
                raise ValueError("a query given as counts must be a float32 matrix of {} columns".format(cols))
        holder = _holder(target, k, log2, "AGTC")
        if holder.infasta is None:
            raise TypeError("{} takes the target as a FASTA path".format(what))
        ctx = holder._ctx()
        if qmat is None:
            qc = BasicCounter(os.fspath(query), k=k, mean=mean, std=std, log2=log2, silent=True)
            qc.get_counts()
            qmat = qc.counts
        packed = holder._packed_seqs()
        self.seq_index, self.start, self.length = window_table(packed.lengths(), window, slide)
        self.n_rows, self.n_query = len(self.seq_index), qmat.shape[0]
        self.chunk_rows = max(1, min(int(chunk_rows), max(self.n_rows, 1)))
        self.holder, self.ctx, self.cols, self.qmat, self.packed = holder, ctx, cols, qmat, packed
        self.k, self.window, self.slide, self.log2 = k, window, slide, log2
        self.center, self.scale = _as_device_vector(ctx, mean, cols, None), _as_device_vector(ctx, std, cols, None)

    def blocks(self):
        """(r0, n, r_dev, has_nan) per chunk: r_dev[:, :n] holds r of every query against window rows r0 .. r0 + n - 1
        (a [n_query, chunk_rows] block, overwritten by the next chunk); has_nan: the chunk's fill reported NaN."""
        ctx, cols, k, log2, chunk_rows = self.ctx, self.cols, self.k, self.log2, self.chunk_rows
        chunks = _chunks(self.n_rows, chunk_rows)
        center, scale = self.center, self.scale
        cnt = ctx.empty(chunk_rows, cols)

        def counted(r0, n):
            out = cnt if n == chunk_rows else cnt.view(0, n)
            return _lib.count_windows(ctx, self.packed, k, self.window, self.slide, r0, n, log2_pre=(log2 == "Log2.pre"), out=out)

        post, shift = log2 == "Log2.post", np.float32(0.0)
        if post:  # np.min over the whole normalised matrix (NaN-propagating), chunk by chunk
            lowest = np.float32(np.inf)
            for r0, n in chunks:
                mn, _ = _lib.min_nan(ctx, counted(r0, n), center, scale)
                lowest = np.minimum(lowest, mn)
            shift = np.abs(lowest)
        precision = pearson_mod._precision_for(np.dtype(np.float32), True)
        qdev = ctx.from_numpy(self.qmat)
        qside, tside = _Side(ctx, self.n_query, cols, precision), _Side(ctx, chunk_rows, cols, precision)
        q_op, _ = qside.fill(qdev, precision)
        if q_op.kind == 0:
            precision = _lib.PREC_FP32
        r_dev = ctx.empty(self.n_query, chunk_rows)
        for r0, n in chunks:
            x = counted(r0, n)
            tail = dict(center=center, scale=scale, post=post, shift=float(shift))
            t_op, has_nan = tside.fill(x, precision, **tail)
            a_op = q_op
            if t_op.kind != q_op.kind:  # rows the split layouts do not carry: this chunk in float32 layout on both sides
                t_op, has_nan = tside.fill(x, _lib.PREC_FP32, **tail)
                a_op, _ = qside.fill(qdev, _lib.PREC_FP32)
            _lib.pearson_gemm_op(ctx, a_op, t_op, r_dev)
            yield r0, n, r_dev, has_nan

    def headers(self):
        return np.asarray(_headers(self.holder), dtype=object)


@_lib.api_call
def domain_pearson(query, target, k, window, slide, mean, std, log2="Log2.post", chunk_rows=65536, outfile=None):
    """Pearson r between every query and every sliding window of the target: (r float32 [n_query, n_windows], table).

    query: a FASTA path (counted and normalised with `mean`, `std`, `log2` as BasicCounter does) or a normalised float32
    count matrix [n_query, 4^k].  target: a FASTA path.  mean, std: vectors (arrays or .npy paths) — required.  Per chunk
    of `chunk_rows` window rows: count -> normalise -> operand fill -> contraction against the query operand (filled
    once) -> r[:, chunk]; one chunk of window counts is on the device at any time and no window text exists on the host.
    With Log2.post the shift of kmer_counts.py:208 is the minimum over ALL windows, so the chunks are counted twice: once
    for that minimum, once for r.  table: DataFrame with `header`, `start`, `end` of every window (the columns of r).
    NAN_WARNING is printed once when a chunk's normalised counts or its block of r hold NaN.  outfile: r is also saved there
    as .npy."""
    run = _DomainRun(query, target, k, window, slide, mean, std, log2, chunk_rows, "domain_pearson")
    n_rows, nan_seen = run.n_rows, False
    r = np.empty((run.n_query, n_rows), dtype=np.float32)
    for r0, n, r_dev, has_nan in run.blocks():
        r[:, r0:r0 + n] = r_dev.to_numpy()[:, :n]
        # a constant row (a window of fewer than k letters under mean 0 / std 1) has finite counts and no r
        nan_seen = nan_seen or has_nan or bool(np.isnan(r[:, r0:r0 + n]).any())
    if nan_seen:
        print(NAN_WARNING)
    headers = run.headers()
    table = _frame({"header": headers[run.seq_index] if n_rows else headers[:0], "start": run.start,
                    "end": run.start + run.length})
    if outfile:
        _lib.save_npy(outfile, r)
    return r, table


@_lib.api_call
def domain_topk(query, target, k, window, slide, mean, std, top=10, log2="Log2.post", chunk_rows=65536):
    """The `top` windows of the target each query correlates with most: a DataFrame with one row per (query, rank) and the
    columns `query` (its index), `rank` (0 = best), `header`, `start`, `end` (the window) and `r` — the first `top`
    entries of np.argsort(-r[q], kind="stable") of domain_pearson's r for the same arguments, NaN last, ties to the
    earlier window.  domain_pearson's loop with one change: each chunk's block of r is merged into the queries' running
    lists on the device (skr_topk_merge_rows) and r is never downloaded — top x n_query entries cross PCIe instead of
    n_query x n_windows floats.  Fewer than `top` windows: fewer rows.  NAN_WARNING as in domain_pearson."""
    top = _lib.check_topk_k(top, "top")
    run = _DomainRun(query, target, k, window, slide, mean, std, log2, chunk_rows, "domain_topk")
    ctx, nan_seen = run.ctx, False
    idx, val = ctx.empty(run.n_query, top, np.uint32), ctx.empty(run.n_query, top, np.float32)
    first = True
    for r0, n, r_dev, has_nan in run.blocks():
        saw = _lib.topk_merge_rows(ctx, r_dev, idx, val, top, first=first, col_begin=0, col_end=n, col_global0=r0,
                                   exclude_diag=False, want_nan=True)
        nan_seen, first = nan_seen or has_nan or saw, False
    if nan_seen:
        print(NAN_WARNING)
    if first or run.n_query == 0:  # no window or no query
        win, rv = np.empty(0, np.int64), np.empty(0, np.float32)
        qi = rank = win
    else:
        hi, hv = idx.to_numpy(), val.to_numpy()
        keep = hi != _lib.TOPK_PAD_IDX  # padded slots are dropped
        qi, rank = np.nonzero(keep)
        win, rv = hi[keep].astype(np.int64), hv[keep]
    headers = run.headers()
    return _frame({"query": qi, "rank": rank, "header": headers[run.seq_index[win]] if len(win) else headers[:0],
                   "start": run.start[win], "end": run.start[win] + run.length[win], "r": rv})


@_lib.api_call
def domain_significant(query, target, k, window, slide, mean, std, fitres, bestfit=1, method="fdr_bh", alpha=0.05,
                       log2="Log2.post", chunk_rows=65536):
    """The windows of the target each query is significantly similar to: a DataFrame with one row per significant (query,
    window) cell in that order and the columns `query` (its index), `header`, `start`, `end` (the window), `r`, `p` and
    `p_adj` — the cells with p_adj <= alpha of domain_pearson's r for the same arguments taken through the full-matrix
    path (p-values against `fitres`, entry `bestfit`, as seekr_amd.significant takes them; consumers.adjust_pvalues on
    all n_query x n_windows tests, `method` one of consumers.HEAD_METHODS).  frame.attrs: n_tests, r_cutoff (None when
    the background never reaches alpha), n_candidates.

    domain_pearson's loop with one change: the cells of each chunk's block with r at or above the cutoff
    (significant.find_cutoff, lowered by its guard) are appended to a list on the device (skr_select_cells_ge) and r is
    never downloaded; the list is corrected as significant.pearson_significant corrects its candidates and only the
    significant cells cross PCIe.  ValueError: the cutoff is not positive, or r is NaN for a candidate (the first such
    window is named; usually a window of fewer than k letters).  NAN_WARNING as in domain_topk."""
    from seekr_amd import significant as sg
    name = sg._check_arguments(fitres, bestfit, method, alpha)
    run = _DomainRun(query, target, k, window, slide, mean, std, log2, chunk_rows, "domain_significant")
    (q, win, r, p, p_adj), attrs = _significant_cells(run, fitres, bestfit, name, alpha)
    headers = run.headers()
    out = _frame({"query": q, "header": headers[run.seq_index[win]] if len(win) else headers[:0], "start": run.start[win],
                  "end": run.start[win] + run.length[win], "r": r, "p": p, "p_adj": p_adj})
    out.attrs.update(attrs)
    return out


def _significant_cells(run, fitres, bestfit, name, alpha):
    """domain_significant's cells: ((query, window, r, p, p_adj) in row-major order, attrs)."""
    from seekr_amd import consumers
    from seekr_amd import significant as sg
    ctx, n_tests = run.ctx, run.n_query * run.n_rows
    attrs = {"n_tests": n_tests, "r_cutoff": None, "n_candidates": 0}
    none = np.empty(0, np.int64)
    empty = (none, none, np.empty(0, np.float32), np.empty(0, np.float32), np.empty(0, np.float64))
    if n_tests == 0:
        return empty, attrs
    pv = sg._PValues(ctx, fitres, bestfit)
    held = []
    try:
        r_star = sg.find_cutoff(pv.host, sg.alpha_float32(alpha))
        if r_star is None:
            return empty, attrs
        cutoff = sg.cutoff_with_guard(r_star)
        attrs["r_cutoff"] = cutoff
        cells = consumers.CellList(ctx)
        held.append(cells)
        nan_seen, nan_window = False, None
        for r0, n, r_dev, has_nan in run.blocks():
            _, saw = consumers.select_cells(r_dev, float(cutoff), cells, nrows=run.n_query, col_begin=0, col_end=n,
                                            row_global0=0, col_global0=r0)
            nan_seen = nan_seen or has_nan or saw
            if saw:  # (rare: the block is fetched to name the window)
                nan_window = r0 + int(np.isnan(r_dev.to_numpy()[:, :n]).any(axis=0).argmax())
                break
        if nan_seen:
            print(NAN_WARNING)
        if nan_window is not None:
            w = nan_window
            raise ValueError("r is NaN for window {} ({}:{}-{}; a window of fewer than k letters has no r): every corrected "
                             "p-value of the full-matrix path is NaN as well; leave such windows out".format(
                                 w, run.headers()[run.seq_index[w]], run.start[w], run.start[w] + run.length[w]))
        attrs["n_candidates"] = len(cells)
        if len(cells) == 0:
            return empty, attrs
        views = list(cells.prefix())
        held[:0] = views
        out = sg.correct_candidates(pv, *views, n_tests, name, alpha, held)
        if out is None:
            return empty, attrs
        order = sg.row_major_order(out[0], out[1])  # the list came chunk by chunk
        q, win, r, p, p_adj = (a[order] for a in out)
        return (q.astype(np.int64), win.astype(np.int64), r, p, p_adj), attrs
    finally:
        pv.free()
        for m in held:
            m.free()


def merge_pieces(row, first, last, n_hot, peak, peak_col, seq_index, max_gap):
    """The hits of a list of pieces, in any order: (row, first, last, n_hot, peak, peak_col) arrays ordered by (row, first).
    Two pieces of one row and one sequence (seq_index[first]) are joined iff first_b - last_a - 1 <= max_gap, the pieces
    taken sorted by (row, first); n_hot adds up, the peak is the larger key (float32_key), the earlier window on equal keys.
    Applied to the pieces of ANY tiling of the cells this gives the hits of the cells, which is why tiles, chunks and
    launches need no carry.  Vectorised: one lexsort and three reduceat."""
    row, first, last = (np.asarray(a, dtype=np.int64).reshape(-1) for a in (row, first, last))
    n_hot, peak_col = (np.asarray(a, dtype=np.int64).reshape(-1) for a in (n_hot, peak_col))
    peak = np.asarray(peak, dtype=np.float32).reshape(-1)
    if len(row) == 0:
        return row, first, last, n_hot, peak, peak_col
    order = np.lexsort((first, row))
    row, first, last, n_hot, peak, peak_col = (a[order] for a in (row, first, last, n_hot, peak, peak_col))
    seq_index = np.asarray(seq_index)
    join = np.zeros(len(row), dtype=bool)
    join[1:] = ((row[1:] == row[:-1]) & (seq_index[first[1:]] == seq_index[last[:-1]])
                & (first[1:] - last[:-1] - 1 <= int(max_gap)))
    begin = np.flatnonzero(~join)
    end = np.append(begin[1:], len(row)) - 1
    # (key << 32) | (0xFFFFFFFF - window): the largest key, then the earliest window
    packed = (float32_key(peak).astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - peak_col.astype(np.uint64))
    best = np.maximum.reduceat(packed, begin)
    return (row[begin], first[begin], last[end], np.add.reduceat(n_hot, begin), float32_unkey((best >> np.uint64(32)).astype(np.uint32)),
            (np.uint64(0xFFFFFFFF) - (best & np.uint64(0xFFFFFFFF))).astype(np.int64))


@_lib.api_call
def domain_hits(query, target, k, window, slide, mean, std, cutoff=None, fitres=None, bestfit=1, alpha=0.05, method=None,
                max_gap=0, min_windows=1, log2="Log2.post", chunk_rows=65536):
    """The intervals of the target each query resembles: hot windows merged into hits.  With r = domain_pearson's matrix
    for the same arguments, window w is hot for query q iff r[q, w] >= cutoff in float32 (NaN is never hot), and a hit is
    a maximal set of hot windows of ONE target sequence in which neighbouring hot windows are separated by at most
    `max_gap` windows that are not hot (0: strictly consecutive).  A DataFrame ordered by (query, first_window) with the
    columns `query`, `header`, `start`, `end` (first base of the first window, end of the last), `first_window`,
    `last_window`, `n_windows` (last - first + 1), `n_hot`, `peak_r` (the largest r, -0 below +0), `peak_start`,
    `peak_end` (the earliest window that reaches it); hits of fewer than `min_windows` windows are dropped.  frame.attrs:
    r_cutoff, n_pieces, n_hits.  No mean or sum of r: a floating-point sum would depend on how the run is cut.

    Exactly one way of choosing the hot cells:
      cutoff            a float: hot iff r >= float32(cutoff);
      fitres, alpha     (method None) cutoff = significant.find_cutoff of the background's p-value at alpha, without a
                        guard — the smallest float32 r with p <= alpha; it is reported, and None means no hits;
      fitres, method    the hot cells are domain_significant's cells for the same arguments (its ValueError on NaN stays).

    domain_pearson's loop with one change: each chunk's block of r is cut into pieces on the device (skr_run_pieces_ge:
    the runs inside one tile of one row x 1 024 windows; nothing is carried between tiles, chunks or launches), r is never
    downloaded, and after the last chunk only the pieces cross PCIe; merge_pieces joins them across tile and chunk edges.
    NAN_WARNING as in domain_topk."""
    from seekr_amd import consumers
    from seekr_amd import significant as sg
    if (cutoff is None) == (fitres is None):
        raise ValueError("give exactly one of `cutoff` and `fitres`")
    if cutoff is not None and method is not None:
        raise ValueError("`method` corrects p-values: it needs `fitres`, not `cutoff`")
    if int(max_gap) != max_gap or max_gap < 0:
        raise ValueError("max_gap must be a whole number of windows, 0 or more (got {!r})".format(max_gap))
    if int(min_windows) != min_windows or min_windows < 1:
        raise ValueError("min_windows must be a whole number, 1 or more (got {!r})".format(min_windows))
    max_gap, min_windows = int(max_gap), int(min_windows)
    name = None
    if cutoff is not None:
        cutoff = np.float32(cutoff)
        if np.isnan(cutoff):
            raise ValueError("cutoff must not be NaN")
    else:
        name = sg._check_arguments(fitres, bestfit, "fdr_bh" if method is None else method, alpha)
    run = _DomainRun(query, target, k, window, slide, mean, std, log2, chunk_rows, "domain_hits")
    ctx = run.ctx
    attrs = {"r_cutoff": None if cutoff is None else float(cutoff), "n_pieces": 0, "n_hits": 0}
    none = np.empty(0, np.int64)
    pieces = (none, none, none, none, np.empty(0, np.float32), none)
    if run.n_query * run.n_rows == 0:
        pass
    elif method is not None:
        (q, win, r, _, _), cell_attrs = _significant_cells(run, fitres, bestfit, name, alpha)
        attrs["r_cutoff"] = None if cell_attrs["r_cutoff"] is None else float(cell_attrs["r_cutoff"])
        pieces = (q, win, win, np.ones(len(q), np.int64), r, win)
    else:
        if cutoff is None:
            pv = sg._PValues(ctx, fitres, bestfit)
            try:
                cutoff = sg.find_cutoff(pv.host, sg.alpha_float32(alpha))
            finally:
                pv.free()
            attrs["r_cutoff"] = None if cutoff is None else float(cutoff)
        if cutoff is not None:
            seq_of_col = ctx.from_numpy(run.seq_index.astype(np.uint32))  # once per call
            found = consumers.PieceList(ctx)
            try:
                nan_seen = False
                for r0, n, r_dev, has_nan in run.blocks():
                    _, saw = consumers.run_pieces(r_dev, float(cutoff), found, max_gap=max_gap, seq_of_col=seq_of_col,
                                                  nrows=run.n_query, col_begin=0, col_end=n, row_global0=0, col_global0=r0)
                    nan_seen = nan_seen or has_nan or saw
                if nan_seen:
                    print(NAN_WARNING)
                pieces = found.to_host()
            finally:
                found.free()
                seq_of_col.free()
    attrs["n_pieces"] = len(pieces[0])
    q, first, last, n_hot, peak, peak_win = merge_pieces(*pieces, run.seq_index, max_gap)
    keep = last - first + 1 >= min_windows
    q, first, last, n_hot, peak, peak_win = (a[keep] for a in (q, first, last, n_hot, peak, peak_win))
    attrs["n_hits"] = len(q)
    headers = run.headers()
    out = _frame({"query": q, "header": headers[run.seq_index[first]] if len(q) else headers[:0], "start": run.start[first],
                  "end": run.start[last] + run.length[last], "first_window": first, "last_window": last,
                  "n_windows": last - first + 1, "n_hot": n_hot, "peak_r": peak, "peak_start": run.start[peak_win],
                  "peak_end": run.start[peak_win] + run.length[peak_win]})
    out.attrs.update(attrs)
    return out


def window_labels(table):
    """`header:start-end` of every row of domain_pearson's table: the column labels of r in a labelled CSV."""
    return ["{}:{}-{}".format(h, s, e) for h, s, e in zip(table["header"], table["start"], table["end"])]
