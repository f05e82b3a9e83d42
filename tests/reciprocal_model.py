"""What the reciprocal-neighbour tests expect — test infrastructure, numpy only: the column-direction merge as the row
merge of tests/neighbors_cases.py on the transposed block, and skr_knn_pairs written as plain loops straight from its
contract (include/seekr_hip.h).  Nothing here calls the device."""
import numpy as np

import neighbors_cases as nc

NO_RANK = 0xFFFFFFFF
MUTUAL, UNION = 0, 1
MODES = {"mutual": MUTUAL, "union": UNION}


def merge_cols_block(r, k, c0=0, c1=None, row0=0, col0=0, exclude_diag=True, running=None):
    """(idx [c1 - c0, k], val [c1 - c0, k]) of skr_topk_merge_cols on r[:, c0:c1]: the row merge of the transposed block
    with the globals swapped — entries are global rows row0 + i, the diagonal is global row == global column col0 + j."""
    r = np.asarray(r, dtype=np.float32)
    c1 = r.shape[1] if c1 is None else c1
    t = np.ascontiguousarray(r[:, c0:c1].T)
    return nc.merge_block(t, k, 0, r.shape[0], col0 + c0, row0, exclude_diag, running)


def saw_nan_cols(r, c0, c1, row0, col0, exclude_diag=True):
    return nc.saw_nan(r, c0, c1, row0, col0, exclude_diag)


def _is_nan_bits(b):
    return (int(b) & 0x7FFFFFFF) > 0x7F800000


def knn_pairs_model(idx_a, val_a, idx_b=None, val_b=None, mode=MUTUAL, positive_only=False):
    """(rows, cols, vals, rank_row, rank_col): uint32, uint32, float32, uint32, uint32, ascending by (row, col).
    ValueError for an index out of range (the library's SKR_ERR_INVALID)."""
    mode = MODES.get(mode, mode)
    idx_a = np.asarray(idx_a, np.uint32)
    bits_a = nc.bits(val_a).reshape(idx_a.shape)
    self_form = idx_b is None
    n1 = idx_a.shape[0]
    if not self_form:
        idx_b = np.asarray(idx_b, np.uint32)
        bits_b = nc.bits(val_b).reshape(idx_b.shape)
        n2 = idx_b.shape[0]
    cand = {}  # (row, col) -> [rank_row, bits of that entry, rank_col, bits of that entry]

    def add(pair, side, rank, bits):
        slot = cand.setdefault(pair, [None, None, None, None])
        if slot[2 * side] is None:  # (lists as the merge kernels leave them hold no index twice)
            slot[2 * side], slot[2 * side + 1] = rank, bits
    for u in range(n1):
        for t in range(idx_a.shape[1]):
            v = int(idx_a[u, t])
            if v == nc.NO_CELL:
                continue
            if v >= (n1 if self_form else n2):
                raise ValueError("index out of range")
            if _is_nan_bits(bits_a[u, t]):
                continue
            if self_form:
                if v != u:
                    add((min(u, v), max(u, v)), 0 if u < v else 1, t, int(bits_a[u, t]))
            else:
                add((u, v), 0, t, int(bits_a[u, t]))
    if not self_form:
        for j in range(n2):
            for t in range(idx_b.shape[1]):
                i = int(idx_b[j, t])
                if i == nc.NO_CELL:
                    continue
                if i >= n1:
                    raise ValueError("index out of range")
                if _is_nan_bits(bits_b[j, t]):
                    continue
                add((i, j), 1, t, int(bits_b[j, t]))
    out = []
    for (i, j) in sorted(cand):
        rank_row, bits_row, rank_col, bits_col = cand[(i, j)]
        if mode == MUTUAL and (rank_row is None or rank_col is None):
            continue
        bits = bits_row if rank_row is not None else bits_col
        if positive_only and not np.array([bits], np.uint32).view(np.float32)[0] > 0:
            continue
        out.append((i, j, bits, NO_RANK if rank_row is None else rank_row, NO_RANK if rank_col is None else rank_col))
    a = np.array(out, dtype=np.uint32).reshape(-1, 5)
    return a[:, 0].copy(), a[:, 1].copy(), a[:, 2].copy().view(np.float32), a[:, 3].copy(), a[:, 4].copy()


def same_pairs(got, want):
    """Five vectors against five vectors, values by their bits."""
    return all(np.array_equal(nc.bits(g) if i == 2 else np.asarray(g, np.uint32), nc.bits(w) if i == 2 else np.asarray(w, np.uint32))
               for i, (g, w) in enumerate(zip(got, want))) and len(got) == len(want) == 5


def random_lists(rng, n_rows, n_targets, k, self_form=False, pads=0.2, nans=0.15, values=(-0.5, -0.0, 0.0, 0.25, 0.5, 1.0)):
    """(idx uint32 [n_rows, k], val float32 [n_rows, k]): per row a prefix of a random permutation of the targets (no
    index twice; a row's own index left out in the self form), some slots padded (anywhere: lists are sets), some values
    NaN, the others from a few distinct values."""
    idx = np.full((n_rows, k), nc.NO_CELL, np.uint32)
    val = np.full((n_rows, k), nc.PAD_BITS, np.uint32).view(np.float32)
    pool = np.array(values, np.float32)
    for u in range(n_rows):
        targets = [v for v in rng.permutation(n_targets).tolist() if not (self_form and v == u)][:k]
        for t, v in enumerate(targets):
            if rng.random() < pads:
                continue
            idx[u, t] = v
            val[u, t] = np.nan if rng.random() < nans else pool[rng.integers(0, len(pool))]
    return idx, val


def brute_force_pairs(r, k, mode, positive_only=False, self_form=False):
    """The pairs straight from a dense r (no lists): j is among i's k best of row i / i among j's k best of column j, by
    ranking every row and column with a full sort in the order of neighbors_cases (value descending, ties to the smaller
    index, NaN last; NaN never pairs).  Self form: r is square, the diagonal is left out, pairs are (min, max) and the
    value is r[min, max]."""
    r = np.asarray(r, np.float32)
    n1, n2 = r.shape

    def ranks(line, skip):
        order = [j for j in np.argsort(-line, kind="stable").tolist() if j != skip][:k]
        return {j: t for t, j in enumerate(order) if not np.isnan(line[j])}
    with np.errstate(all="ignore"):
        by_row = [ranks(r[i], i if self_form else -1) for i in range(n1)]
        by_col = by_row if self_form else [ranks(r[:, j], -1) for j in range(n2)]
    out = []
    for i in range(n1):
        for j in range(i + 1 if self_form else 0, n2):
            rank_row = by_row[i].get(j)
            rank_col = by_col[j].get(i)
            have = (rank_row is not None) + (rank_col is not None)
            if have == 0 or (MODES.get(mode, mode) == MUTUAL and have < 2):
                continue
            v = r[i, j] if rank_row is not None else (r[j, i] if self_form else r[i, j])
            if positive_only and not v > 0:
                continue
            out.append((i, j, int(nc.bits(np.array([v]))[0]), NO_RANK if rank_row is None else rank_row,
                        NO_RANK if rank_col is None else rank_col))
    a = np.array(out, dtype=np.uint32).reshape(-1, 5)
    return a[:, 0].copy(), a[:, 1].copy(), a[:, 2].copy().view(np.float32), a[:, 3].copy(), a[:, 4].copy()
