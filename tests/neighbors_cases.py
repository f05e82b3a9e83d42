"""What the nearest-neighbour tests expect — test infrastructure: the numpy reference of the one-pass top-k and its
merge, and the list of cases the GPU file runs (tests/test_neighbors_cpu.py pins that list).  Nothing here calls the
device; the capacities are the package's mirrored constants (the GPU file compares them with the library's own).

The order: np.argsort(-row, kind="stable") over the candidates SORTED BY GLOBAL COLUMN — values descending, -0 == +0,
NaN after every number, ties to the smaller global column.  It is total, so the k best of a union are the k best of
(the k best of one part) and the other part: a row merged panel by panel gives one answer whatever the split."""
import numpy as np

from seekr_amd._lib import TOPK_MERGE_CAP as CAP
from seekr_amd._lib import TOPK_MERGE_KMAX as KMAX
from seekr_amd._lib import TOPK_MERGE_STEP as STEP

NO_CELL = 0xFFFFFFFF
PAD_BITS = 0x7FC00000
TOP_COLUMN = 0xFFFFFFFE  # the largest legal global column


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def padded(k):
    return np.full(k, NO_CELL, dtype=np.uint32), np.full(k, PAD_BITS, dtype=np.uint32).view(np.float32)


def best(cols, vals, k):
    """(idx uint32 [k], val float32 [k]) of the candidates (global columns, float32 values): stable argsort of -vals
    after ordering by column; padded to k."""
    cols = np.asarray(cols, dtype=np.int64).reshape(-1)
    vals = np.asarray(vals, dtype=np.float32).reshape(-1)
    by_col = np.argsort(cols, kind="stable")
    cols, vals = cols[by_col], vals[by_col]
    with np.errstate(all="ignore"):
        order = np.argsort(-vals, kind="stable")[:k]
    idx, val = padded(k)
    idx[:len(order)] = cols[order]
    val[:len(order)] = vals[order]
    return idx, val


def merge_row(row, k, c0, c1, grow, col0, exclude_diag=True, running=None):
    """One row of skr_topk_merge_rows: the k best of `running` (idx, val; padded slots are no entries; None = first) and
    the cells row[c0:c1] at global columns col0 + c, minus global column == grow when exclude_diag."""
    c = np.arange(c0, c1, dtype=np.int64)
    if exclude_diag:
        c = c[c + col0 != grow]
    cols, vals = c + col0, np.asarray(row, dtype=np.float32)[c]
    if running is not None:
        keep = running[0] != NO_CELL
        cols = np.concatenate([running[0][keep].astype(np.int64), cols])
        vals = np.concatenate([running[1][keep], vals])
    return best(cols, vals, k)


def merge_block(r, k, c0=0, c1=None, row0=0, col0=0, exclude_diag=True, running=None):
    """(idx [rows, k], val [rows, k]) of a block; running: (idx, val) of the same shape, or None."""
    r = np.asarray(r, dtype=np.float32)
    c1 = r.shape[1] if c1 is None else c1
    out = [merge_row(r[i], k, c0, c1, row0 + i, col0, exclude_diag,
                     None if running is None else (running[0][i], running[1][i])) for i in range(r.shape[0])]
    return np.stack([o[0] for o in out]).reshape(r.shape[0], k), np.stack([o[1] for o in out]).reshape(r.shape[0], k)


def saw_nan(r, c0, c1, row0, col0, exclude_diag=True):
    """Is a cell of r[:, c0:c1], the excluded diagonal cells aside, NaN?"""
    r = np.asarray(r, dtype=np.float32)
    nan = np.isnan(r[:, c0:c1])
    if exclude_diag:
        for i in range(r.shape[0]):
            d = row0 + i - col0
            if c0 <= d < c1:
                nan[i, d - c0] = False
    return bool(nan.any())


# ---- the cases of the kernel on synthetic blocks ------------------------------------------------------------------------
# 1, 3, 4, 5: below / at / above one 16-byte load; 63 .. 65: a wave; 255 .. 257: a workgroup's threads; STEP +- 1: one
# sweep step and the start of the next (the buffer is flushed before a step that might not fit, i.e. as soon as more than
# CAP - STEP candidates wait: after every step of a row in ascending order); 2 STEP + 1: a third step; CAP +- 1, 2 CAP + 1:
# the buffer's capacity
WIDTHS = (1, 3, 4, 5, 63, 64, 65, 255, 256, 257, STEP - 1, STEP, STEP + 1, CAP - 1, CAP, CAP + 1, 2 * STEP + 1, 2 * CAP + 1)
PATTERNS = ("ascending", "descending", "equal", "five_values", "all_nan", "specials")
KS = (1, 2, 31, 32, 33, 64, KMAX - 1, KMAX)
ALIGNMENTS = ((0, 0), (1, 0), (4, 0), (0, 1), (1, 2), (4, 3), (3, 1))  # (col_begin, columns right of the window): the second
#                                                                       makes ld no multiple of 4 for some widths, and every
#                                                                       row then starts at another offset from a 16-byte line
ALIGN_WIDTHS = (1, 3, 4, 5, 63, 64, 65, 257, STEP + 1)
DIAGONALS = ("inside", "outside", "first", "last", "off")
MERGE_SPLITS = (2, 3, 7)
ROWS = 4


def ks_for(width):
    """The k of a width: the fixed list, and one above the width (padding) where KMAX allows."""
    ks = list(KS)
    if width + 3 <= KMAX and width + 3 not in ks:
        ks.append(width + 3)
    return ks


def fill(pattern, rows, width, seed):
    """[rows, width] float32 of the pattern; rows differ from each other."""
    rng = np.random.default_rng([seed, width, PATTERNS.index(pattern)])
    j = np.arange(width, dtype=np.float32)[None, :]
    i = np.arange(rows, dtype=np.float32)[:, None]
    if pattern == "ascending":      # every cell beats the bound: the most flushes
        return (j - 0.5 * width + i).astype(np.float32)
    if pattern == "descending":     # nothing beats the bound after the first k
        return (0.25 * width - j - i).astype(np.float32)
    if pattern == "equal":          # the answer is the k smallest columns
        return np.broadcast_to(np.float32(0.375) * (i + 1), (rows, width)).astype(np.float32)
    if pattern == "five_values":
        return np.array([-1.5, -0.0, 0.0, 0.25, 3.0], np.float32)[rng.integers(0, 5, (rows, width))]
    if pattern == "all_nan":
        return np.full((rows, width), np.nan, dtype=np.float32)
    pool = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1.0, -1.0, 1e-45, -1e-45], np.float32)
    x = pool[rng.integers(0, len(pool), (rows, width))]
    x.view(np.uint32)[np.isnan(x) & (rng.random((rows, width)) < 0.5)] = 0xFFC00123  # a NaN with a sign and a payload
    return x


def embed(block, col_begin, right, poison=np.nan):
    """The block as columns [col_begin, col_begin + width) of a wider matrix whose other cells are poison."""
    rows, width = block.shape
    m = np.full((rows, col_begin + width + right), poison, dtype=np.float32)
    m[:, col_begin:col_begin + width] = block
    return m


def diagonal_offsets(kind, col_begin, width, col_global0=7):
    """(row_global0, col_global0, exclude_diag) putting row 0's diagonal cell where `kind` says."""
    at = {"inside": col_begin + width // 2, "outside": col_begin + width + 5, "first": col_begin,
          "last": col_begin + width - 1, "off": col_begin + width // 2}[kind]
    return col_global0 + at, col_global0, kind != "off"


def kernel_cases():
    """Every (pattern, width, k) of the main grid, as dicts."""
    return [dict(pattern=p, width=w, k=k) for p in PATTERNS for w in WIDTHS for k in ks_for(w)]


def split_points(width, parts, seed):
    """parts - 1 uneven cut points inside (0, width), sorted; fewer when the width has no room."""
    rng = np.random.default_rng([seed, width, parts])
    inner = np.arange(1, width)
    if len(inner) == 0:
        return []
    cuts = rng.choice(inner, size=min(parts - 1, len(inner)), replace=False)
    return sorted(int(c) for c in cuts)


def kmer_profiles(n_rows, k, seed, length=400):
    """Column-normalised float32 k-mer profiles of random sequences: [n_rows, 4^k]."""
    rng = np.random.default_rng(seed)
    x = np.zeros((n_rows, 4 ** k), dtype=np.float64)
    for i in range(n_rows):
        s = rng.integers(0, 4, length + int(rng.integers(0, 200)))
        word = np.zeros(len(s) - k + 1, dtype=np.int64)
        for t in range(k):
            word = word * 4 + s[t:len(s) - k + 1 + t]
        x[i] = np.bincount(word, minlength=4 ** k) * (1000.0 / len(s))
    x = np.log2(x + 1.0)
    return ((x - x.mean(axis=0)) / x.std(axis=0)).astype(np.float32)
