"""The specification of seekr_amd.windows.domain_hits as plain Python over a block of r (no GPU, no library code).

A hit or a piece is a tuple (query, first, last, n_hot, peak_bits, peak_window): window indices are columns of the block,
peak_bits the uint32 bits of the float32 peak (so that -0.0 and +0.0 differ and equality is exact).  Lists are ordered by
(query, first)."""
import numpy as np

SEGMENT = 1024  # columns of one tile of the kernel (cell_tile.hpp)


def key(x):
    """float32 -> int whose order is the order of the values, -0.0 just below +0.0."""
    u = int(np.float32(x).view(np.uint32))
    return (~u & 0xffffffff) if u & 0x80000000 else (u | 0x80000000)


def bits(x):
    return int(np.float32(x).view(np.uint32))


def hits_of_cells(r, seq_index, cutoff, max_gap):
    """The hits of the cells of r [n_query, n_windows], written as the obvious loop."""
    r = np.asarray(r, dtype=np.float32)
    cutoff = np.float32(cutoff)
    hits = []
    for q in range(r.shape[0]):
        cur = None  # [first, last, n_hot, peak value, peak window]
        for w in range(r.shape[1]):
            v = r[q, w]
            if not v >= cutoff:  # NaN is never hot
                continue
            if cur is not None and seq_index[w] == seq_index[cur[1]] and w - cur[1] - 1 <= max_gap:
                cur[1] = w
                cur[2] += 1
                if key(v) > key(cur[3]):  # the earliest window that reaches the peak stays
                    cur[3], cur[4] = v, w
            else:
                if cur is not None:
                    hits.append((q, cur[0], cur[1], cur[2], bits(cur[3]), cur[4]))
                cur = [w, w, 1, v, w]
        if cur is not None:
            hits.append((q, cur[0], cur[1], cur[2], bits(cur[3]), cur[4]))
    return hits


def pieces_of_tiling(r, seq_index, cutoff, max_gap, tile_starts):
    """The tile-local runs: the hits of every tile taken alone.  tile_starts: the ascending first columns of the tiles
    (the first one is 0), one list for every row or a list of such lists, one per row."""
    r = np.asarray(r, dtype=np.float32)
    seq_index = np.asarray(seq_index)
    per_row = len(tile_starts) > 0 and isinstance(tile_starts[0], (list, tuple, np.ndarray))
    pieces = []
    for q in range(r.shape[0]):
        starts = list(tile_starts[q] if per_row else tile_starts)
        assert starts[0] == 0 and starts == sorted(set(starts))
        for a, b in zip(starts, starts[1:] + [r.shape[1]]):
            for (_, first, last, n_hot, pk, pw) in hits_of_cells(r[q:q + 1, a:b], seq_index[a:b], cutoff, max_gap):
                pieces.append((q, a + first, a + last, n_hot, pk, a + pw))
    return pieces


def merge_pieces(pieces, seq_index, max_gap):
    """The merge rule on a list of pieces in any order: sorted by (query, first), two pieces of one query and one sequence
    are joined iff first_b - last_a - 1 <= max_gap; n_hot adds up, the larger key is the peak, the earlier window on
    equal keys."""
    out = []
    for p in sorted(pieces, key=lambda p: (p[0], p[1])):
        q, first, last, n_hot, pk, pw = p
        if out:
            a = out[-1]
            if a[0] == q:
                assert a[2] < first
            if a[0] == q and seq_index[a[2]] == seq_index[first] and first - a[2] - 1 <= max_gap:
                ka, kb = key(np.uint32(a[4]).view(np.float32)), key(np.uint32(pk).view(np.float32))
                peak = (pk, pw) if (kb, -pw) > (ka, -a[5]) else (a[4], a[5])
                out[-1] = (q, a[1], last, a[3] + n_hot, peak[0], peak[1])
                continue
        out.append((q, first, last, n_hot, pk, pw))
    return out


def kernel_tile_starts(rows, ld, col_begin, col_end):
    """The kernel's tiling of r[0:rows, col_begin:col_end] of a matrix with `ld` columns whose storage begins at a 16-byte
    boundary, as first columns RELATIVE to col_begin, one list per row: segments start at the 16-byte boundary at or below
    the row's first selected cell, so the first tile has up to 3 columns fewer."""
    width = col_end - col_begin
    out = []
    for i in range(rows):
        mis = (i * ld + col_begin) % 4
        out.append([0] + list(range(SEGMENT - mis, width, SEGMENT)))
    return out
