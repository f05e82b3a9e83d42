"""Exact-sum inputs for the Pearson contractions and the integer model of what every kernel and mode must then store.

When every product a kernel forms and every partial sum of those products, in ANY order, is exactly representable in the
accumulator's type, the result cannot depend on tiling, phase order, wave geometry, k chunking, mirror or swapped form:
it is integer arithmetic and one division per k chunk, bit for bit.  This module builds such rows for the split kernels
(fp16 and bf16 halves), the fp32 kernel and the float64 kernels, states the conditions that make them exact (checked on
the host for every case, before anything is launched) and restates the result in a few lines of numpy.  numpy only: the
CPU tests (tests/test_exact_sum_cpu.py) and the GPU tests (tests/test_gpu_exact_sum.py) share the case table below.

Split rows, in scaled units n = x * scale (what the matrix cores see; fp16: scale = 2^floor(log2(32768 / sqrt(K))), bf16: 1):
  coarse cells 8 c, c in -3 .. 3          one half holds them: lo = 0
  fine cells   +-(m + 0.5), m in 1024 .. 1099   one or two per row, at a column that moves with the row: hi = m or m + 1
                                          by the column's rounding direction (fp16) or the nearest multiple of 8 (bf16),
                                          lo = the rest, never 0
The first k tile and the last column are always populated (what a k element read twice or skipped would touch); above
16 384 columns three columns of four are empty elsewhere, and the fine cells sit on the populated ones.  bf16 rows are
the same pattern times 2^-8 (|x| < sqrt(K) / 4 at K = 1 024); exactness does not depend on a power of two."""
import functools

import numpy as np

U = 0.5                      # every half is a multiple of U (pattern units), every product a multiple of U
CAP = 0.9 * 2.0 ** 24 * U    # condition (c): no subset of a pair's products sums past this
KIND = {"f16x3": 2, "bf16x3": 1}
BF16_UNIT = 2.0 ** -8        # bf16 rows: pattern x this (a power of two: the halves are the pattern's, scaled)


# ------------------------------------------------------------------ the stored halves, restated
def f16_scale(cols):
    """The power of two fp16 halves are stored times (operand.hip: skr_operand_create)."""
    return np.float32(2.0 ** np.floor(np.log2(32768.0 / np.sqrt(cols))))


def split_up(cols):
    """Per column: is the hi half rounded UP (operand.hip: split_flip)?"""
    col = np.arange(cols, dtype=np.uint64)
    return (((col * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)) >> np.uint64(31)).astype(bool)[None, :]


def f16_halves(x, scale):
    """(hi, lo, up) of float32 rows x: hi = x * scale rounded DOWN or UP by the hash of the column (operand.hip:
    split_hi_f16 - one conversion and a step), lo = fp16(x * scale - hi), with numpy's float16 conversion and nextafter."""
    zs = x * scale
    up = split_up(x.shape[1])
    with np.errstate(all="ignore"):
        h = zs.astype(np.float16)
        back = h.astype(np.float32)
        h_up = np.where(back < zs, np.nextafter(h, np.float16(np.inf)), h)
        h_dn = np.where(back > zs, np.nextafter(h, np.float16(-np.inf)), h)
        hi = np.where(up, h_up, h_dn).astype(np.float16)
        lo = (zs - hi.astype(np.float32)).astype(np.float16)
    return hi, lo, up


def _bf16_rne(v):
    """float32 -> the nearest bf16 (ties to even), returned as float32."""
    b = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32).astype(np.uint64)
    b = (b + np.uint64(0x7FFF) + ((b >> np.uint64(16)) & np.uint64(1))) & np.uint64(0xFFFF0000)
    return b.astype(np.uint32).view(np.float32)


def bf16_halves(x):
    """(hi, lo) of float32 rows x as float32 arrays holding bf16 values: both halves to nearest (operand.hip: split_hi_flip)."""
    hi = _bf16_rne(x)
    lo = _bf16_rne(x - hi)
    return hi, lo


def stored_halves(hi, lo, precision):
    """uint16 patterns [rows, kt, 2, 32] as the operand stores them ([rows, kt, {hi, lo}, 32]; padding columns hold +0)."""
    rows, cols = hi.shape
    kt = (cols + 31) // 32
    out = np.zeros((rows, kt, 2, 32), np.uint16)
    for h, half in enumerate((hi, lo)):
        if precision == "f16x3":
            pat = half.astype(np.float16).view(np.uint16)
        else:
            pat = (np.ascontiguousarray(half, dtype=np.float32).view(np.uint32) >> 16).astype(np.uint16)
        out[:, :, h, :] = np.concatenate([pat, np.zeros((rows, kt * 32 - cols), np.uint16)], axis=1).reshape(rows, kt, 32)
    return out


# ------------------------------------------------------------------ the rows
def split_pattern(rows, cols, seed):
    """Rows in pattern units (multiples of 0.5), float64.  See the module docstring."""
    rng = np.random.default_rng([seed, rows, cols])
    stride = 4 if cols > 16384 else 1
    col = np.arange(cols)
    populated = (col % stride == 0) | (col < 32) | (col == cols - 1)
    n = 8.0 * rng.integers(-3, 4, size=(rows, cols)) * populated[None, :]
    edge = np.r_[col[:32], cols - 1]                    # first k tile, last column: never empty
    n[:, edge] = 8.0 * rng.choice([-3, -2, -1, 1, 2, 3], size=(rows, edge.size))
    i = np.arange(rows)
    slots = cols // stride
    f1 = ((37 * i + 5 + 3 * seed) % slots) * stride
    f2 = ((slots // 2 + 101 * i + 11 + 7 * seed) % slots) * stride
    m = rng.integers(1024, 1100, size=(rows, 2))
    sign = rng.choice([-1.0, 1.0], size=(rows, 2))
    n[i, f1] = sign[:, 0] * (m[:, 0] + 0.5)
    two = (i % 3 != 0) & (f2 != f1)
    n[i[two], f2[two]] = sign[two, 1] * (m[two, 1] + 0.5)
    return n


class SplitRows:
    """x: the float32 rows to upload; hi, lo: the halves the matrix cores multiply (float32 arrays holding them exactly,
    the operand's own units); scale: the operand's storage scale; unit: what one pattern unit is in hi / lo."""

    def __init__(self, precision, rows, cols, seed):
        self.precision, self.rows, self.cols = precision, rows, cols
        n = split_pattern(rows, cols, seed)
        if precision == "f16x3":
            self.scale, self.unit = float(f16_scale(cols)), 1.0
            self.x = (n / self.scale).astype(np.float32)
            hi, lo, _ = f16_halves(self.x, np.float32(self.scale))
        else:
            self.scale, self.unit = 1.0, BF16_UNIT
            self.x = (n * BF16_UNIT).astype(np.float32)
            hi, lo = bf16_halves(self.x)
        self.n = n.astype(np.float32)                      # pattern units (multiples of 0.5 below 2^11: exact)
        self.hi, self.lo = hi.astype(np.float32), lo.astype(np.float32)
        self.stored = stored_halves(hi, lo, precision)


PRODUCTS = (("hi", "hi"), ("hi", "lo"), ("lo", "hi"))       # the product set of the split kernels: lo x lo is not in it
_BLOCK = 4096                                               # columns per float64 matmul of the host (memory only)


def _blocks(c0, c1):
    return [(k0, min(c1, k0 + _BLOCK)) for k0 in range(c0, c1, _BLOCK)]


def _dot(a, b, c0, c1):
    """sum over columns c0 .. c1 of a b^T in float64 (exact: multiples of U^2 units far below 2^53)."""
    s = 0.0
    for k0, k1 in _blocks(c0, c1):
        s = s + a[:, k0:k1].astype(np.float64) @ b[:, k0:k1].astype(np.float64).T
    return s


def check_split_conditions(a, b):
    """Conditions (a) - (d) of DESIGN_PARITY.md, "Exact-sum inputs", on the rows of a against the rows of b: properties of
    the inputs, asserted before anything is launched.  Returns the bound on the worst subset sum, in units of 2^23 U."""
    K = a.cols
    for s in (a, b):
        n = s.n.astype(np.float64) * s.unit
        assert np.array_equal(s.x.astype(np.float64) * s.scale, n)                          # the upload is the pattern
        assert np.array_equal(s.hi.astype(np.float64) + s.lo, n)                            # (a) hi + lo == n
        hi_u, lo_u = s.hi / np.float32(s.unit), s.lo / np.float32(s.unit)                  # pattern units
        # (b) every product is a multiple of U: the hi halves are integers, the lo halves multiples of U
        assert np.array_equal(np.round(hi_u), hi_u) and np.array_equal(np.round(lo_u / U), lo_u / U)
        if K >= 1024:
            assert 16.0 * float(np.max(s.x.astype(np.float64) ** 2)) < K                    # (d) stays on the split kernel
        assert float(np.abs(s.x).max()) * s.scale <= 65504.0                                # ... and inside the fp16 range
    # (c) per pair of rows i, j: sum_k |hi_i hi_j| + |hi_i lo_j| + |lo_i hi_j| <= sum_k v_i v_j <= |v_i| |v_j| with
    # v = |hi| + |lo| (Cauchy-Schwarz).  That bounds the positive products' sum and the negative products' sum of the
    # pair, and with them every subset sum — in float64, exactly, without a matrix product
    norm = [np.sqrt(((np.abs(s.hi.astype(np.float64)) + np.abs(s.lo)) ** 2).sum(axis=1).max()) / s.unit for s in (a, b)]
    worst = norm[0] * norm[1]
    assert worst <= CAP, ("condition (c)", a.precision, a.rows, b.rows, K, worst / CAP)
    return worst / (2.0 ** 23 * U)


def worst_subset_sum(a, b):
    """The per-pair figure itself, for the shapes where six float64 matmuls are cheap: max over the pairs of
    max(sum of the positive products, |sum of the negative products|), in units of 2^23 U.  The bound above is never below it."""
    def parts(v):
        v = v.astype(np.float64)
        return np.maximum(v, 0), np.maximum(-v, 0)
    pos = neg = 0.0
    for p, q in PRODUCTS:
        (ap, an), (bp, bn) = parts(getattr(a, p)), parts(getattr(b, q))
        pos = pos + ap @ bp.T + an @ bn.T
        neg = neg + ap @ bn.T + an @ bp.T
    return float(np.maximum(pos, neg).max()) / (a.unit * b.unit) / (2.0 ** 23 * U)


def cross_share(a, b):
    """Share of the cells of a against b that carry a non-zero cross term (hi x lo or lo x hi)."""
    nz = lambda v: (v != 0).astype(np.float32)
    return float(((nz(a.hi) @ nz(b.lo).T + nz(a.lo) @ nz(b.hi).T) != 0).mean())


# ------------------------------------------------------------------ the model
def k_chunks(cols, chunk_tiles):
    """Column ranges of the accumulator restarts: chunk_tiles k tiles of 32 columns each."""
    step = 32 * chunk_tiles
    return [(c0, min(cols, c0 + step)) for c0 in range(0, cols, step)]


def split_kdiv(a, b):
    return np.float32(a.cols) * np.float32(a.scale) * np.float32(b.scale)


def chunk_products(a, b, chunk_tiles):
    """Per k chunk the three sums [hi_a hi_b, hi_a lo_b, lo_a hi_b] over the chunk's columns, float64, exact."""
    return [[_dot(getattr(a, p), getattr(b, q), c0, c1) for p, q in PRODUCTS] for c0, c1 in k_chunks(a.cols, chunk_tiles)]


def fold(sums, kdiv, exact=True):
    """r = fl32(fl32(S_0) / kdiv) (+) fl32(fl32(S_1) / kdiv) (+) ... in chunk order, float32 (pearson_bf16.hip: the
    epilogue's divide-or-multiply, then the accumulating store of the later chunks).  exact=False (the mutants of the CPU
    tests, whose sums may leave float32): fl32(S_c) is a plain rounding instead of an assertion."""
    r = None
    for s in sums:
        s32 = s.astype(np.float32)
        assert not exact or np.array_equal(s32.astype(np.float64), s), "a chunk sum is not a float32 number: condition (c) is broken"
        q = s32 / np.float32(kdiv)
        r = q if r is None else (r + q).astype(np.float32)
    return r


def split_model(a, b, chunk_tiles):
    """S_c = sum over the chunk's columns of hi_a hi_b + hi_a lo_b + lo_a hi_b, then the fold."""
    return fold([p[0] + p[1] + p[2] for p in chunk_products(a, b, chunk_tiles)], split_kdiv(a, b))


def split_diag_model(a):
    """The diagonal of a self-comparison is written from the fill's own sum of squares, lo^2 included (operand.hip:
    patch_diag_kernel, diag = sum x^2 / K).  Returns (value, exact): where sum n^2 — and with it every partial sum, the
    terms being non-negative — is a float32 number the value is fl32(sum x^2 / K) bit for bit, elsewhere it holds to a
    relative K 2^-24."""
    n2 = (a.n.astype(np.float64) ** 2).sum(axis=1)            # pattern units: multiples of 0.25, exact in float64
    exact = n2 < 2.0 ** 22                                     # multiples of 0.25 below 2^22: 24 bits
    sq = (n2 * (a.unit / a.scale) ** 2).astype(np.float32)    # sum x^2 (a power of two times n2)
    return sq / np.float32(a.cols), exact


def edges_model(r, cutoff, row_global0, col_global0, upper_only, zero_rule=True):
    """The fused edge list: r >= cutoff, r != 0, off the global diagonal (pearson_bf16.hip: cell), sorted by (row, column).
    zero_rule=False: the mutant that lists cells of exactly 0."""
    gi = row_global0 + np.arange(r.shape[0], dtype=np.int64)[:, None]
    gj = col_global0 + np.arange(r.shape[1], dtype=np.int64)[None, :]
    keep = (r >= np.float32(cutoff)) & ((gj > gi) if upper_only else (gj != gi))
    if zero_rule:
        keep &= r != 0
    i, j = np.nonzero(keep)
    return sort_edges((gi[i, 0]).astype(np.uint32), (gj[0, j]).astype(np.uint32), r[i, j])


def pick_cutoff(r, row_global0=7, col_global0=11):
    """A positive value that occurs in r above the global diagonal (so that it has to be listed, upper_only or not): the
    median of those."""
    gi = row_global0 + np.arange(r.shape[0], dtype=np.int64)[:, None]
    gj = col_global0 + np.arange(r.shape[1], dtype=np.int64)[None, :]
    v = np.sort(r[(gj > gi) & (r > 0)])
    assert v.size, "no positive cell above the diagonal"
    return np.float32(v[v.size // 2])


def low_cutoffs(r):
    """Cutoffs that only the `r != 0` rule keeps the exactly-zero cells out of: 0 and the smallest value of r (negative in
    every case: everything that is not 0 has to be listed)."""
    lowest = np.float32(r.min())
    assert lowest < 0
    return np.float32(0.0), lowest


def zero_cells(r, row_global0=7, col_global0=11):
    """How many cells of r are exactly 0 above the global diagonal (listable with and without upper_only, but for the rule).
    Sums of products of integers cancel exactly now and then: only these inputs can put a cell there."""
    gi = row_global0 + np.arange(r.shape[0], dtype=np.int64)[:, None]
    gj = col_global0 + np.arange(r.shape[1], dtype=np.int64)[None, :]
    return int(((r == 0) & (gj > gi)).sum())


ZERO_CELL_ROWS = 257   # cases with at least this many rows of a hold exactly-zero cells above the diagonal (asserted)


def sort_edges(rows, cols, vals):
    order = np.lexsort((cols, rows))
    return rows[order], cols[order], np.ascontiguousarray(vals[order], dtype=np.float32)


# ------------------------------------------------------------------ the case table
# (precision, columns, SEEKR_GEMM_CHUNK_TILES or 0 for "whatever the operand chooses": only where K is a power of two,
#  so that the chunking cannot show).  The widths whose division rounds per chunk pin it, and the model takes the same number.
DEFAULT_CHUNK = 128   # only used by the model for the pinned widths and as "one chunk or more, it must not matter" elsewhere
WIDTHS = [
    ("f16x3", 64, 0), ("f16x3", 96, 128), ("f16x3", 160, 128), ("f16x3", 256, 0),
    ("f16x3", 1000, 128), ("f16x3", 1000, 8),
    ("f16x3", 1024, 0), ("f16x3", 4096, 0),
    ("f16x3", 4128, 128),
    ("f16x3", 16384, 0), ("f16x3", 65536, 0),
    ("f16x3", 512, 1), ("f16x3", 512, 3), ("f16x3", 512, 5),
    ("bf16x3", 1024, 0), ("bf16x3", 4096, 0), ("bf16x3", 16384, 0),
]
SHAPES = [(3, 5), (257, 300), (1024, 768), (4100, 300)]


def shape_allowed(cols, m, n):
    """4 100 rows only up to 160 columns (the host model stays under a second), 65 536 columns on at most 64 rows."""
    if m > 4000:
        return cols <= 160
    if cols >= 65536:
        return max(m, n) <= 64
    return True


SPLIT_CASES = [(p, k, ct, m, n) for p, k, ct in WIDTHS for m, n in SHAPES + [(40, 64)] if shape_allowed(k, m, n)
               and ((m, n) != (40, 64) or k >= 65536)]


@functools.lru_cache(maxsize=2)
def split_case(precision, cols, m, n):
    """(a, b): rows of the left and of the right operand (self-comparisons use a)."""
    return SplitRows(precision, m, cols, 1), SplitRows(precision, n, cols, 2)


def model_chunk_tiles(chunk_tiles):
    return chunk_tiles or DEFAULT_CHUNK


# ------------------------------------------------------------------ fp32 and float64 kernels
F32_SHAPES = [(1, 1, 4), (130, 257, 64), (300, 200, 100), (257, 129, 4096)]


def f32_case(m, n, cols, seed=0):
    """Small integers: every subset of a pair's products sums below 2^24."""
    rng = np.random.default_rng([seed, m, n, cols])
    a = rng.integers(-7, 8, size=(m, cols)).astype(np.float32)
    b = rng.integers(-7, 8, size=(n, cols)).astype(np.float32)
    a[:, [0, cols - 1]] = rng.choice([-5.0, 3.0, 7.0], size=(m, 2))
    b[:, [0, cols - 1]] = rng.choice([-5.0, 3.0, 7.0], size=(n, 2))
    assert float((np.abs(a.astype(np.float64)) @ np.abs(b.astype(np.float64)).T).max()) < 2.0 ** 24
    return a, b


def f32_model(a, b, cols=None):
    """fl32(S) / fl32(K), one IEEE division (pearson.hip: __fdiv_rn)."""
    s = a.astype(np.int64) @ b.astype(np.int64).T
    assert np.abs(s).max() < 2 ** 24
    return s.astype(np.float32) / np.float32(a.shape[1] if cols is None else cols)


F64_WIDTHS = [4, 12, 16, 48, 1000, 1008, 4096]
F64_SHAPES = [(1, 1), (31, 33), (127, 129), (129, 127), (300, 33), (33, 300)]


def f64_case(m, n, cols, seed=0):
    """Signed integers up to 2^20: every subset of a pair's products sums below 2^53 (K <= 4 096: 2^52)."""
    rng = np.random.default_rng([seed, m, n, cols])
    a = rng.integers(-2 ** 20, 2 ** 20 + 1, size=(m, cols)).astype(np.int64)
    b = rng.integers(-2 ** 20, 2 ** 20 + 1, size=(n, cols)).astype(np.int64)
    a[:, [0, cols - 1]] = rng.choice([-2 ** 20, 2 ** 20, 2 ** 20 - 1], size=(m, 2))
    b[:, [0, cols - 1]] = rng.choice([-2 ** 20, 2 ** 20, 2 ** 20 - 1], size=(n, 2))
    assert cols * 2 ** 40 < 2 ** 53
    return a, b


def f64_model(a, b):
    """float64(S) / float64(K) from int64 (pearson.hip: acc / kdiv)."""
    return (a @ b.T).astype(np.float64) / np.float64(a.shape[1])
