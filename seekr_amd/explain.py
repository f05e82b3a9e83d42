"""The k-mers behind a similarity, on MI355X.  The reference has no such function; its plots take the answer as input
(`words` of kmer_comp_textplot / kmer_indi_textplot, the per-k-mer mean and sd of kmer_msd_barplot).

pair_kmers: r[i, j] is the mean over the columns w of z_i[w] * z_j[w] (z: the row-standardised counts pearson()
multiplies); for each listed pair the `top` columns with the largest (or smallest) term, with the term and its two
factors.  The specification is, per pair,

    c = z1[row] * z2[col] in float32;  key = c (largest) or -c;  np.argsort(-key, kind="stable")[:top]

NaN last, -0 == +0, ties to the smaller column: the order of nearest().  Both rows are read once on the device
(skr_pair_kmers); no product matrix stands anywhere.

group_kmers: np.mean(counts[labels == g], axis=0) and np.std(..., axis=0, ddof=1) for every label g, bit for bit (numpy's
own float32 chains, skr_group_colstat), and the `top` columns of each group by mean in the same order rule.
"""
import numpy as np

from seekr_amd import _lib


class PairKmers:
    """idx (uint32), contribution, z_row, z_col (float32), each [E, top]: per pair the chosen columns, best first, the
    term z_row * z_col and its factors.  Slots beyond the number of columns hold 0xFFFFFFFF / NaN.  `kmers`: the column
    names given to pair_kmers, or None."""

    def __init__(self, idx, contribution, z_row, z_col, kmers=None):
        self.idx, self.contribution, self.z_row, self.z_col, self.kmers = idx, contribution, z_row, z_col, kmers

    def __len__(self):
        return len(self.idx)

    def words(self, kmers=None):
        """Per pair the list of k-mer strings of its columns, best first, pads dropped.  kmers: the names of the columns
        (default: those given to pair_kmers)."""
        return _words(self.idx, self.kmers if kmers is None else kmers)


class GroupKmers:
    """labels (the distinct labels, np.unique order), sizes (int64), mean, sd (float32 [G, W]), idx (uint32 [G, top]: the
    top columns of each group by mean, best first; pads as PairKmers) and value (float32 [G, top]: their means)."""

    def __init__(self, labels, sizes, mean, sd, idx, value, kmers=None):
        self.labels, self.sizes, self.mean, self.sd, self.idx, self.value, self.kmers = labels, sizes, mean, sd, idx, value, kmers

    def __len__(self):
        return len(self.labels)

    def words(self, kmers=None):
        return _words(self.idx, self.kmers if kmers is None else kmers)


def _words(idx, kmers):
    if kmers is None:
        raise ValueError("no k-mer names: pass kmers= (the column names of the count matrix)")
    kmers = list(kmers)
    idx = np.asarray(idx)
    real = idx[idx != _lib.TOPK_PAD_IDX]
    if len(real) and int(real.max()) >= len(kmers):
        raise ValueError("column {} has no name: {} k-mer names were given".format(int(real.max()), len(kmers)))
    return [[kmers[int(j)] for j in row if j != _lib.TOPK_PAD_IDX] for row in idx]


def _integers(values, what):
    a = np.asarray(values)
    if a.ndim != 1:
        raise ValueError("{} must be a 1-D array of row indices (got shape {})".format(what, a.shape))
    if a.dtype.kind not in "iu":
        if a.size == 0 or (a.dtype.kind == "f" and np.all(np.mod(a, 1) == 0)):
            return a.astype(np.int64)
        raise ValueError("{} must hold integers (got dtype {})".format(what, a.dtype))
    return a


def _outside(a, limit):
    return (a < 0) | (a >= limit) if a.dtype.kind == "i" else a >= limit


def check_pairs(rows, cols, n1, n2):
    """rows, cols as uint32 arrays of one length with every pair inside [0, n1) x [0, n2); ValueError naming the first
    pair that is not."""
    ra, ca = _integers(rows, "rows"), _integers(cols, "cols")
    if len(ra) != len(ca):
        raise ValueError("rows and cols must have one length (got {} and {})".format(len(ra), len(ca)))
    bad = np.flatnonzero(_outside(ra, n1) | _outside(ca, n2))
    if len(bad):
        e = int(bad[0])
        raise ValueError("pair {} = ({}, {}) is the first bad one: it names a row outside its matrix ({} and {} rows)".format(
            e, int(ra[e]), int(ca[e]), int(n1), int(n2)))
    return np.ascontiguousarray(ra, dtype=np.uint32), np.ascontiguousarray(ca, dtype=np.uint32)


def _device_rows(ctx, counts, what):
    """(matrix, owned): `counts` on the device as float32 — a Matrix as it is, a host array uploaded."""
    if isinstance(counts, _lib.Matrix):
        if counts.dtype != np.float32:
            raise TypeError("{} on the device must be float32 (got {})".format(what, counts.dtype))
        return counts, False
    c = np.ascontiguousarray(counts, dtype=np.float32)
    if c.ndim != 2:
        raise ValueError("{} must be a 2-D matrix".format(what))
    return ctx.from_numpy(c), True


def _shape(counts):
    return counts.shape if isinstance(counts, _lib.Matrix) else np.shape(counts)


@_lib.api_call
def pair_kmers(counts, rows, cols=None, counts2=None, top=10, largest=True, row_standardize=True, kmers=None):
    """PairKmers of the pairs (rows[e], cols[e]): rows index `counts`, cols index `counts2` (None: `counts` again).
    counts / counts2: host arrays (ranked in float32, as nearest() does) or float32 device matrices.  rows may be a
    SignificantPairs, which carries both lists.  row_standardize=True multiplies the rows pearson() multiplies
    (_lib.row_standardize); False takes the matrices as they are.  largest=False lists the most negative terms.
    ValueError before any launch: top outside 1.._lib.TOPK_MERGE_KMAX, an index outside its matrix (the message names
    the first bad pair)."""
    top = _lib.check_topk_k(top, "top")
    if cols is None:
        if not (hasattr(rows, "rows") and hasattr(rows, "cols")):
            raise ValueError("cols is missing: pass two index arrays, or one SignificantPairs")
        rows, cols = rows.rows, rows.cols
    same = counts2 is None or counts2 is counts
    s1, s2 = _shape(counts), _shape(counts if same else counts2)
    if len(s1) != 2 or len(s2) != 2:
        raise ValueError("counts must be a 2-D matrix")
    if s1[1] != s2[1]:
        raise ValueError("counts and counts2 must have the same number of columns ({} and {})".format(s1[1], s2[1]))
    rows, cols = check_pairs(rows, cols, s1[0], s2[0])
    n = len(rows)
    if kmers is not None and len(kmers) != s1[1]:
        raise ValueError("{} k-mer names for {} columns".format(len(kmers), s1[1]))
    if n == 0 or s1[1] == 0:
        pad = np.full((n, top), _lib.TOPK_PAD_BITS, np.uint32).view(np.float32)
        return PairKmers(np.full((n, top), _lib.TOPK_PAD_IDX, np.uint32), pad, pad.copy(), pad.copy(), kmers)
    ctx = _lib.default_context()
    held = []
    try:
        x1, own = _device_rows(ctx, counts, "counts")
        held += [x1] if own else []
        if same:
            x2 = x1
        else:
            x2, own = _device_rows(ctx, counts2, "counts2")
            held += [x2] if own else []
        if row_standardize:
            z1 = _lib.row_standardize(ctx, x1)
            held.append(z1)
            z2 = z1 if same else _lib.row_standardize(ctx, x2)
            held += [] if same else [z2]
        else:
            z1, z2 = x1, x2
        d_rows, d_cols = ctx.from_numpy(rows), ctx.from_numpy(cols)
        outs = [ctx.empty(n, top, np.uint32)] + [ctx.empty(n, top, np.float32) for _ in range(3)]
        held += [d_rows, d_cols] + outs
        _lib.pair_kmers(ctx, z1, z2, d_rows, d_cols, n, top, largest, *outs)
        idx, val, f1, f2 = (np.array(m.to_numpy()) for m in outs)
        return PairKmers(idx, val, f1, f2, kmers)
    finally:
        for m in held:
            m.free()


def group_order(labels):
    """(unique labels, sizes int64, order uint32, starts int64): the rows of each label, ascending, label after label in
    np.unique order."""
    labels = np.asarray(labels)
    if labels.ndim != 1 or (labels.size and labels.dtype.kind not in "iu"):
        raise ValueError("labels must be a 1-D integer array (got shape {}, dtype {})".format(labels.shape, labels.dtype))
    uniq, inverse = np.unique(labels, return_inverse=True)
    inverse = inverse.reshape(-1)
    order = np.argsort(inverse, kind="stable").astype(np.uint32)
    sizes = np.bincount(inverse, minlength=len(uniq)).astype(np.int64)
    starts = np.zeros(len(uniq) + 1, np.int64)
    np.cumsum(sizes, out=starts[1:])
    return uniq, sizes, order, starts


def top_columns(values, top, largest=True):
    """(idx uint32 [G, top], value float32 [G, top]): per row of `values` its top columns in pair_kmers' order rule, with
    numpy; pads 0xFFFFFFFF / NaN beyond the width."""
    values = np.asarray(values, dtype=np.float32)
    g, w = values.shape
    idx = np.full((g, top), _lib.TOPK_PAD_IDX, np.uint32)
    val = np.full((g, top), _lib.TOPK_PAD_BITS, np.uint32).view(np.float32)
    m = min(top, w)
    for i in range(g):
        key = values[i] if largest else -values[i]
        order = np.argsort(-key, kind="stable")[:m]
        idx[i, :m] = order
        val[i, :m] = values[i][order]
    return idx, val


def group_kmers_device(ctx, x, labels, top=10, largest=True, kmers=None):
    """group_kmers on a float32 device matrix."""
    top = _lib.check_topk_k(top, "top")
    uniq, sizes, order, starts = group_order(labels)
    if len(order) != x.rows:
        raise ValueError("{} labels for {} rows".format(len(order), x.rows))
    g, w = len(uniq), x.cols
    if g == 0 or w == 0:
        empty = np.empty((g, w), np.float32)
        return GroupKmers(uniq, sizes, empty, empty.copy(), *top_columns(empty, top, largest), kmers)
    held = [ctx.from_numpy(order), ctx.empty(g, w), ctx.empty(g, w)]
    try:
        _lib.group_colstat(ctx, x, held[0], starts, held[1], held[2])
        mean, sd = np.array(held[1].to_numpy()), np.array(held[2].to_numpy())
    finally:
        for m in held:
            m.free()
    return GroupKmers(uniq, sizes, mean, sd, *top_columns(mean, top, largest), kmers)


@_lib.api_call
def group_kmers(counts, labels, top=10, largest=True, kmers=None):
    """GroupKmers: for every distinct label (np.unique order) the column means and sample standard deviations of the rows
    of `counts` (a host array, taken in float32, or a float32 device matrix) that carry it — np.mean(counts[labels == g],
    axis=0) and np.std(counts[labels == g], axis=0, ddof=1) in float32, bit for bit — and the `top` columns by mean
    (largest=False: the smallest means).  labels: any 1-D integer array, one per row."""
    _lib.check_topk_k(top, "top")
    if len(_shape(counts)) != 2:
        raise ValueError("counts must be a 2-D matrix")
    labels = np.asarray(labels)
    if labels.ndim != 1 or len(labels) != _shape(counts)[0]:
        raise ValueError("labels of shape {} for {} rows".format(labels.shape, _shape(counts)[0]))
    group_order(labels[:1])  # the dtype check, before any upload
    ctx = _lib.default_context()
    x, own = _device_rows(ctx, counts, "counts")
    try:
        return group_kmers_device(ctx, x, labels, top, largest, kmers)
    finally:
        if own:
            x.free()


# ---- the pair lists the commands write ----------------------------------------------------------------------------------
def read_pairs_csv(path, names1=None, names2=None):
    """(rows, cols) int64 from what seekr_significant_pairs (`row,col,...`) or seekr_nearest (`row,rank,neighbor,...`)
    writes: the header decides which columns are the pair.  Entries are integers, or names looked up in names1 (rows) /
    names2 (cols); ValueError for anything else."""
    import csv
    with open(path, newline="") as f:
        lines = list(csv.reader(f))
    if not lines:
        raise ValueError("{}: empty file".format(path))
    header = [h.strip() for h in lines[0]]
    if header[:2] == ["row", "col"]:
        ci = 1
    elif header[:3] == ["row", "rank", "neighbor"]:
        ci = 2
    else:
        raise ValueError("{}: the header starts with {!r}; expected row,col or row,rank,neighbor".format(path, header[:3]))
    look1 = None if names1 is None else {str(n): i for i, n in enumerate(names1)}
    look2 = None if names2 is None else {str(n): i for i, n in enumerate(names2)}

    def one(text, look, line):
        if look is not None and text in look:
            return look[text]
        try:
            return int(text)
        except ValueError:
            raise ValueError("{}: line {}: {!r} is neither a row name nor an integer".format(path, line, text)) from None

    rows, cols = [], []
    for at, rec in enumerate(lines[1:], start=2):
        if not rec:
            continue
        if len(rec) <= ci:
            raise ValueError("{}: line {}: {} fields, expected at least {}".format(path, at, len(rec), ci + 1))
        rows.append(one(rec[0], look1, at))
        cols.append(one(rec[ci], look2, at))
    return np.array(rows, np.int64), np.array(cols, np.int64)
