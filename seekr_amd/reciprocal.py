"""Reciprocal nearest neighbours and k-nearest-neighbour graphs on MI355X, from one sweep of r and without the r matrix.
The reference has no such functions; the specification is the numpy model in tests/reciprocal_model.py:

    reciprocal_hits   the pairs (i, j) where j is among the k rows of counts2 most correlated with row i of counts1 AND
                      (mode "mutual") or OR ("union") i is among the k rows of counts1 most correlated with row j of
                      counts2 — nearest()'s order on both sides.  Both lists come from ONE consumers.Sweep
                      (consumers.pearson_topk_both), so a pair has one r, whichever list it is read from.
    knn_graph         the mutual or union k-NN graph of one set as the upper-triangle edge list leiden.communities
                      takes: at most N k edges, every degree bounded, where a global cutoff keeps half of all cells.

The lists become pairs on the device (consumers.knn_pairs: skr_knn_pairs); only the pairs cross PCIe.
"""
import numpy as np

from seekr_amd import _lib, consumers
from seekr_amd import pearson as pearson_mod
from seekr_amd.neighbors import _f32, _prepare

COLUMNS = ("row", "col", "r", "rank_row", "rank_col")


def check_k(k, two_sets):
    """ValueError unless 1 <= k <= the limit of the kernels behind the form (no device call): the column kernel's for two
    sets (_lib.TOPK_COLS_KMAX), the row kernel's for one (_lib.TOPK_MERGE_KMAX)."""
    return _lib.check_topk_cols_k(k) if two_sets else _lib.check_topk_k(k)


def _labels(counts):
    """The row labels of a labelled frame, else None."""
    index = getattr(counts, "index", None)
    return None if index is None or callable(index) else list(index)


def operand_pairs(z1, z2=None, k=10, mode="mutual", positive_only=False, **kw):
    """The five host vectors (row, col, r, rank_row, rank_col) for prepared operands (_lib.Operand): z2=None is the self
    form — pearson_topk(z1) and the self form of knn_pairs; else pearson_topk_both(z1, z2) and the two-set form.  `kw`:
    stripe_rows, panel_rows of the sweep."""
    consumers.knn_mode(mode)
    k = check_k(k, z2 is not None)
    ctx = z1.ctx
    if z1.rows == 0 or (z2 is not None and z2.rows == 0):
        return tuple(np.empty(0, t) for t in consumers.PairList.DTYPES)
    held = []
    try:
        if z2 is None:
            idx, val = consumers.pearson_topk(z1, None, k=k, **kw)
            lists = [ctx.from_numpy(idx), ctx.from_numpy(val)]
            held += lists
            lists += [None, None]
        else:
            lists = list(consumers.pearson_topk_both(z1, z2, k=k, keep_device=True, **kw))
            held += lists
        pairs = consumers.PairList(ctx, max(1, z1.rows * k))
        held.append(pairs)
        consumers.knn_pairs(*lists, mode=mode, positive_only=positive_only, into=pairs)
        return pairs.to_host()
    finally:
        for m in held:
            m.free()


@_lib.api_call
def reciprocal_hits(counts1, counts2=None, k=10, mode="mutual", **kw):
    """A DataFrame with the columns row, col, r, rank_row, rank_col (plus row_name, col_name when the inputs are labelled
    frames): the reciprocal ("mutual") or one-sided ("union") nearest-neighbour pairs of the rows of counts1 and counts2
    by Pearson correlation, ascending by (row, col).  rank_row: where col stands in row's list of k (0 = best), rank_col:
    where row stands in col's; 0xFFFFFFFF when the pair is not in that list (union only).  r is the one value the sweep
    made for the pair.  counts2=None (or counts1 itself): one set, a row is not its own neighbour, every pair once with
    row < col.  k: at most _lib.TOPK_COLS_KMAX for two sets, _lib.TOPK_MERGE_KMAX for one (ValueError before any device
    work).  `kw`: stripe_rows, panel_rows."""
    consumers.knn_mode(mode)
    if counts2 is None:
        counts2 = counts1
    c1, c2, _, _, same = pearson_mod._operands(counts1, counts2)
    k = check_k(k, not same)
    names1, names2 = _labels(counts1), _labels(counts2)
    ctx = _lib.default_context()
    c1 = _f32(c1)
    z1, z2 = _prepare(ctx, c1, c1 if same else _f32(c2), same)
    try:
        cols = operand_pairs(z1, z2, k=k, mode=mode, **kw)
    finally:
        z1.free()
        if z2 is not None:
            z2.free()
    from pandas import DataFrame
    frame = dict(zip(COLUMNS, cols))
    if names1 is not None and names2 is not None:
        frame["row_name"] = [names1[i] for i in cols[0].tolist()]
        frame["col_name"] = [names2[j] for j in cols[1].tolist()]
    return DataFrame(frame)


def knn_graph(z, k, mode="union", **kw):
    """(rows, cols, vals) uint32, uint32, float32: the k-NN graph of the prepared operand `z` (_lib.Operand) as the
    upper-triangle edge list leiden.communities takes — the pairs {u, v} where v is among u's k nearest OR ("union") / AND
    ("mutual") u is among v's, weight r > 0 (pairs whose r is not positive are no edges), row < col, ascending.  At most
    z.rows * k edges.  1 <= k <= _lib.TOPK_MERGE_KMAX.  `kw`: stripe_rows, panel_rows."""
    rows, cols, vals, _, _ = operand_pairs(z, None, k=k, mode=mode, positive_only=True, **kw)
    return rows, cols, vals
