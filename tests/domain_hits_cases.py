"""The synthetic blocks tests/test_gpu_domain_hits.py uploads, and what they must contain (pinned without a GPU by
tests/test_domain_hits_cpu.py).  Plain numpy.

Two families.  PLANTED cases are built around the kernel's own tile edges so that every place where tile-local runs can
go wrong is present: a hit across an edge, one that ends at column 1 023 of a tile, one that begins at column 0, gaps of
exactly max_gap and max_gap + 1 over an edge, a sequence boundary between two hot windows inside a tile and at an edge,
and a peak tie.  `features` counts them from the cells and from the model's hits, and the CPU file asserts each count.
PATTERN cases are the shapes and fills of the sweep (none hot, all hot, alternating, values around the cutoff, NaN)."""
import numpy as np

import domain_hits_model as model

CUTOFF = np.float32(0.25)


def _cold(rng, shape):
    return rng.uniform(-0.5, 0.2, size=shape).astype(np.float32)


def _hot(rng, n):
    return rng.uniform(0.3, 0.9, size=n).astype(np.float32)


# ---- planted cases ----------------------------------------------------------------------------------------------------
# (name, rows, width, col_begin, extra columns of the parent behind the range, max_gap)
PLANTED = [("w4100_b%d_g%d" % (b, g), 3, 4100, b, 5, g) for b, g in ((0, 0), (1, 1), (2, 2), (3, 0), (3, 2))] + \
          [("w65536_g%d" % g, 3, 65536, 0, 0, g) for g in (1023, 1024, 5000)]


def planted_case(name):
    """(r_parent [rows, ld], col_begin, col_end, seq_index [width], cutoff, max_gap): features at the row's own edges, each
    more than max_gap columns from the next so that they stay apart."""
    _, rows, width, col_begin, extra, g = next(c for c in PLANTED if c[0] == name)
    rng = np.random.default_rng(sum(map(ord, name)))
    ld = col_begin + width + extra
    parent = _cold(rng, (rows, ld))
    starts = model.kernel_tile_starts(rows, ld, col_begin, col_begin + width)
    stride = (2 * g + 8) // model.SEGMENT + 1  # edges between two features: more than 2 * max_gap + 8 columns
    seq_cuts = set()
    for i in range(rows):
        edges = starts[i][1:]
        assert len(edges) >= 3 * stride + 1, (name, len(edges))
        row = parent[i, col_begin:col_begin + width]  # a view

        def heat(cols):
            row[list(cols)] = _hot(rng, len(list(cols)))

        e = edges[0]            # a hit across the edge, with its peak twice: before and behind the edge
        heat(range(e - 3, e + 3))
        row[e - 2] = row[e + 1] = np.float32(0.95)
        e = edges[stride]       # a gap of exactly max_gap over the edge: one hit
        x = e - 1 - g // 2
        heat([x - 1, x, x + g + 1, x + g + 2])
        e = edges[2 * stride]   # a gap of max_gap + 1 over the edge: two hits
        x = e - 1 - g // 2
        heat([x - 1, x, x + g + 2, x + g + 3])
        e = edges[3 * stride]   # hot on both sides of an edge that is also a sequence boundary (row 0's edge for every row:
        heat(range(e - 2, e + 2))  # the sequences are the columns', not the rows')
    e0 = starts[0][1:][3 * stride]
    for i in range(rows):       # row 0's edge is a boundary at the edge; the same column lies inside a tile of a row with
        parent[i, col_begin + e0 - 2:col_begin + e0 + 2] = _hot(rng, 4)  # another first segment
    seq_cuts.add(e0)
    mid = starts[0][1] // 2     # a sequence boundary between two hot windows inside a tile, for every row
    parent[:, col_begin + mid - 2:col_begin + mid + 2] = _hot(rng, (rows, 4))
    seq_cuts.add(mid)
    seq_index = np.zeros(width, dtype=np.int64)
    for c in seq_cuts:
        seq_index[c:] += 1
    return parent, col_begin, col_begin + width, seq_index, CUTOFF, g


def features(block, seq_index, cutoff, max_gap, starts):
    """What a block holds, counted from its cells and from the model's hits: a dict of the seven kinds."""
    hits = model.hits_of_cells(block, seq_index, cutoff, max_gap)
    n = dict.fromkeys(("spans_edge", "ends_at_1023", "begins_at_0", "gap_equal_over_edge", "gap_plus_one_over_edge",
                       "boundary_inside_tile", "boundary_at_edge", "peak_tie"), 0)
    for q, first, last, _, pk, _ in hits:
        edges = starts[q][1:]
        n["spans_edge"] += any(first < e <= last for e in edges)
        n["ends_at_1023"] += any(last == e - 1 for e in edges)  # (the column before an edge is column 1 023 of its segment)
        n["begins_at_0"] += any(first == e for e in edges)
        vals = block[q, first:last + 1]
        n["peak_tie"] += int((vals.view(np.uint32) == np.uint32(pk)).sum() >= 2)
    for q in range(block.shape[0]):
        edges = set(starts[q][1:])
        hot = np.flatnonzero(block[q] >= cutoff)
        for x, y in zip(hot[:-1], hot[1:]):
            over = any(x < e <= y for e in edges)
            same = seq_index[x] == seq_index[y]
            n["gap_equal_over_edge"] += bool(over and same and y - x - 1 == max_gap)
            n["gap_plus_one_over_edge"] += bool(over and same and y - x - 1 == max_gap + 1)
            if y == x + 1 and not same:
                n["boundary_at_edge" if y in edges else "boundary_inside_tile"] += 1
    return n


# ---- pattern cases ----------------------------------------------------------------------------------------------------
WIDTHS = (1, 3, 4, 5, 1023, 1024, 1025, 1027, 2051, 4100)
MAX_GAPS = (0, 1, 2, 1023, 1024, 5000)
BOUNDARY_SETS = ("none", "at_1", "at_1023", "at_1024", "at_1025", "every")


def seq_of(width, which, col0=0):
    """seq_index of `width` columns that start at global column col0: boundaries at the named GLOBAL columns."""
    g = np.arange(col0, col0 + width)
    if which == "none":
        return np.zeros(width, dtype=np.int64)
    if which == "every":
        return g.astype(np.int64)
    return (g >= int(which[3:])).astype(np.int64)


def random_block(rng, rows, ld, density=0.3):
    """Cold cells with hot ones at `density`, a few equal peaks, +-0 and NaN."""
    r = _cold(rng, (rows, ld))
    mask = rng.random((rows, ld)) < density
    r[mask] = rng.choice(np.array([0.3, 0.5, 0.5, 0.7, 0.7, 0.9], np.float32), size=int(mask.sum()))
    r[rng.random((rows, ld)) < 0.01] = np.nan
    return r


def pattern_block(pattern, rows, ld, cutoff):
    c = np.float32(cutoff)
    below, above = np.nextafter(c, np.float32(-np.inf)), np.nextafter(c, np.float32(np.inf))
    if pattern == "none":
        return np.full((rows, ld), below, dtype=np.float32)
    if pattern == "all":
        return np.full((rows, ld), above, dtype=np.float32)
    if pattern == "alternating":
        r = np.full((rows, ld), below, dtype=np.float32)
        r[:, ::2] = c
        return r
    if pattern == "neighbours":  # the cutoff and the float32 on either side of it, in turn
        return np.resize(np.array([c, below, above, above, c, below, below], np.float32), rows * ld).reshape(rows, ld)
    if pattern == "zeros":  # -0.0 and +0.0 and small values of both signs
        return np.resize(np.array([0.0, -0.0, -0.0, 0.0, 1e-30, -1e-30, 0.0, 0.0, -0.0], np.float32), rows * ld).reshape(rows, ld)
    if pattern == "nan":
        r = np.full((rows, ld), above, dtype=np.float32)
        r[:, 2::5] = np.nan
        return r
    raise ValueError(pattern)
