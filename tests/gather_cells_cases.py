"""The numpy model of skr_gather_cells and the lists its tests use — test infrastructure; nothing here calls the device.

model(): for s in [first, first + count), out[s] = the bits of r[rows[s] - row_global0, cols[s] - col_global0] when that
cell lies in r[0:nrows, col_begin:col_end] (Python-integer arithmetic: nothing wraps), every other slot untouched."""
import numpy as np

PATTERN = 0x7FC12345  # a NaN with a payload no gather writes by accident


def pattern(n):
    return np.full(n, PATTERN, dtype=np.uint32)


def model(r, nrows, col_begin, col_end, row_global0, col_global0, rows, cols, first, count, out_bits):
    """(out bits after the call, gathered)."""
    bits = np.ascontiguousarray(r, dtype=np.float32).view(np.uint32)
    out = out_bits.copy()
    gathered = 0
    for s in range(first, first + count):
        i, j = int(rows[s]) - int(row_global0), int(cols[s]) - int(col_global0)
        if 0 <= i < nrows and col_begin <= j < col_end:
            out[s] = bits[i, j]
            gathered += 1
    return out, gathered


def model_fast(r, nrows, col_begin, col_end, row_global0, col_global0, rows, cols, first, count, out_bits):
    """model() vectorised in int64 (indices below 2^32 and origins below 2^32 cannot overflow it)."""
    bits = np.ascontiguousarray(r, dtype=np.float32).view(np.uint32)
    out = out_bits.copy()
    s = np.arange(first, first + count)
    i = rows[s].astype(np.int64) - np.int64(row_global0)
    j = cols[s].astype(np.int64) - np.int64(col_global0)
    hit = (i >= 0) & (i < nrows) & (j >= col_begin) & (j < col_end)
    out[s[hit]] = bits[i[hit], j[hit]]
    return out, int(hit.sum())


# the 5 x 7 block inside a 9 x 16 matrix whose origin lies just below 2^32
EDGE = dict(nrows=5, col_begin=3, col_end=10, row_global0=2 ** 32 - 9, col_global0=2 ** 32 - 16)


def edge_matrix():
    return (np.random.default_rng(916).standard_normal((9, 16)) * 3).astype(np.float32)


def edge_list():
    """(rows, cols) uint32, shuffled: every cell of the block once, the cells one step outside each of its four edges
    (those of the matrix's other rows and columns among them), global indices that a subtraction narrower than 64 bits
    would take for cells of the block, and five duplicates."""
    g = EDGE
    r0, c0 = g["row_global0"], g["col_global0"]
    cells = [(r0 + i, c0 + j) for i in range(g["nrows"]) for j in range(g["col_begin"], g["col_end"])]
    outside = [(r0 - 1, c0 + j) for j in range(g["col_begin"], g["col_end"])]            # above the first row
    outside += [(r0 + g["nrows"], c0 + j) for j in range(g["col_begin"], g["col_end"])]   # row 5 of the matrix: not in nrows
    outside += [(r0 + i, c0 + g["col_begin"] - 1) for i in range(g["nrows"])]            # column 2: left of col_begin
    outside += [(r0 + i, c0 + g["col_end"]) for i in range(g["nrows"])]                  # column 10: col_end itself
    outside += [(r0 + i, c0 + j) for i in (0, 4) for j in (0, 15)]                       # columns of r outside the range
    # what a subtraction narrower than 64 bits confuses with a cell of the block.  A uint32 index congruent to a cell
    # modulo 2^32 IS that cell, so the list holds the next things: indices congruent modulo 2^31 (a sign bit lost or
    # gained on the way), and the block-local indices themselves (an origin that wrapped to 0: origin + 9 = 2^32)
    alias = [(r0 + i - 2 ** 31, c0 + j) for i in (0, 2, 4) for j in (3, 9)]
    alias += [(r0 + i, c0 + j - 2 ** 31) for i in (1, 3) for j in (3, 6, 9)]
    alias += [(r0 + 2 - 2 ** 31, c0 + 5 - 2 ** 31)]
    alias += [(i, j) for i in (0, 4) for j in (3, 9)] + [(i + 9, j + 16) for i in (0, 4) for j in (3, 9)]
    assert all(0 <= a < 2 ** 32 and 0 <= b < 2 ** 32 for a, b in cells + outside + alias)
    dup = [cells[k] for k in (0, 6, 17, 34, 34)]
    both = np.array(cells + outside + alias + dup, dtype=np.uint64)
    both = both[np.random.default_rng(7).permutation(len(both))]
    return both[:, 0].astype(np.uint32), both[:, 1].astype(np.uint32), len(cells) + len(dup)


def special_matrix():
    """6 x 8 float32 bit patterns: NaNs of both signs with payloads, +-0, +-inf, denormals, the pattern itself."""
    words = [0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x7FFFFFFF, 0xFFFFFFFF, 0x7FA5A5A5, 0xFFDEAD00,
             0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF,
             0x00400000, 0x80400000, PATTERN, 0x3F800000, 0xBF800000, 0x7F7FFFFF, 0xFF7FFFFF, 0x00800000]
    return np.array(words * 2, dtype=np.uint32).reshape(6, 8).view(np.float32)
