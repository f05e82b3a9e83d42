"""The head of every library call that reads a block of r (csrc/block.hpp: skr_block): one 5 x 40 float32 matrix of seeded
normals, k = 2, through the nine entry points' Python wrappers.

Which global indices an entry point writes as uint32 decides which origins it must refuse:

    skr_edges, skr_select_cells_ge, skr_gather_cells, skr_run_pieces_ge, skr_topk_merge_cols    rows and columns
    skr_topk_merge_rows, skr_topk_rows                                                           columns only
    skr_hist_key_digits, skr_hist_edges                                                          neither

On a limited side the largest origin that fits, 0xFFFFFFFF - extent (extent: nrows, col_end), is accepted and what comes
back — indices included — is the numpy model's; one more is refused, and so is 2^63 - 1, which a check that adds to the
origin lets through by signed overflow.  On a side without the rule 2^40 is accepted and returns what origin 0 returns.
A refused call raises ValueError before anything is launched: with profiling on, no kernel scope is recorded.

skr_topk_rows always drops the row's own global diagonal cell, so its comparison of row origins reads columns 8 ... 39, where
no diagonal cell lies at either origin; the merges are called with exclude_diag=False throughout, the histograms with
upper_only=False, skr_run_pieces_ge without a sequence vector (it would have to reach the origin)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

R = np.random.default_rng(20261021).standard_normal((5, 40)).astype(np.float32)
K = 2
CUT = np.float32(0.5)
EDGES = np.linspace(-2.0, 2.0, 9, dtype=np.float32)
U32 = 0xFFFFFFFF
PATTERN = np.uint32(0x7FC12345)
FULL = dict(nrows=5, col_begin=0, col_end=40, row_global0=0, col_global0=0)
ROWS, COLS = "rows", "cols"
LIMITED = {  # entry point -> the sides whose global indices must fit 32 bits
    "edges": (ROWS, COLS), "select_cells_ge": (ROWS, COLS), "gather_cells": (ROWS, COLS), "run_pieces_ge": (ROWS, COLS),
    "topk_merge_cols": (ROWS, COLS), "topk_merge_rows": (COLS,), "topk_rows": (COLS,), "hist_key_digits": (), "hist_edges": (),
}
NAMES = sorted(LIMITED)
ORIGIN = {ROWS: "row_global0", COLS: "col_global0"}
EXTENT = {ROWS: FULL["nrows"], COLS: FULL["col_end"]}


def block(**change):
    return dict(FULL, **change)


# ---- the device side: name -> tuple of host arrays --------------------------------------------------------------------
def _list_to_host(lst):
    return tuple(np.array(m.to_numpy(0, lst.n)).reshape(-1) if lst.n else np.empty(0, t) for m, t in zip(lst.bufs, lst.DTYPES))


def _gather_slots(blk):
    """Every cell of the block in a scrambled order, and one slot just below the block: global (rows, cols) as uint32."""
    i, j = np.mgrid[0:blk["nrows"], blk["col_begin"]:blk["col_end"]]
    order = np.random.default_rng(7).permutation(i.size)
    i, j = np.append(i.ravel()[order], blk["nrows"]), np.append(j.ravel()[order], blk["col_begin"])
    return i, j, ((blk["row_global0"] + i) & U32).astype(np.uint32), ((blk["col_global0"] + j) & U32).astype(np.uint32)


def device(name, d_r, blk):
    from seekr_amd import _lib, consumers, distribution
    ctx = d_r.ctx
    if name == "edges":
        return consumers.edges(d_r, CUT, **blk)
    if name in ("select_cells_ge", "run_pieces_ge"):
        lst = (consumers.CellList if name == "select_cells_ge" else consumers.PieceList)(ctx, 256)
        try:
            if name == "select_cells_ge":
                consumers.select_cells(d_r, CUT, lst, **blk)
            else:
                consumers.run_pieces(d_r, CUT, lst, max_gap=0, seq_of_col=None, **blk)
            return _list_to_host(lst)
        finally:
            lst.free()
    if name == "gather_cells":
        _, _, rows, cols = _gather_slots(blk)
        vecs = [ctx.from_numpy(v.reshape(-1, 1)) for v in (rows, cols, np.full(len(rows), PATTERN).view(np.float32))]
        try:
            n = consumers.gather_cells(d_r, *vecs, **blk)
            return np.array(vecs[2].to_numpy()).reshape(-1).view(np.uint32), np.array([n])
        finally:
            for m in vecs:
                m.free()
    if name in ("topk_merge_rows", "topk_merge_cols"):
        lists = max(1, blk["nrows"] if name == "topk_merge_rows" else blk["col_end"] - blk["col_begin"])  # (1: a refused range)
        idx, val = ctx.empty(lists * K, 1, np.uint32), ctx.empty(lists * K, 1, np.float32)
        try:
            getattr(_lib, name)(ctx, d_r, idx, val, K, True, exclude_diag=False, **blk)
            return np.array(idx.to_numpy()).reshape(lists, K), np.array(val.to_numpy()).reshape(lists, K)
        finally:
            idx.free()
            val.free()
    if name == "topk_rows":
        idx, val = consumers.topk_rows(d_r, K, **blk)
        return np.array(idx), np.array(val)
    if name == "hist_key_digits":
        hist, nan = np.zeros((1, 256), np.uint64), np.zeros(1, np.uint64)
        distribution.hist_key_block(d_r, 24, 8, [0], 0, hist, nan, upper_only=False, **blk)
        return hist.reshape(-1), nan
    assert name == "hist_edges"
    hist, extra = np.zeros(len(EDGES) - 1, np.uint64), np.zeros(3, np.uint64)
    distribution.hist_edges_block(d_r, EDGES, hist, extra, upper_only=False, **blk)
    return hist, extra


# ---- the numpy side ------------------------------------------------------------------------------------------------------
def _top(values, index):
    """(global index, value) of the K best: value descending, ties to the smaller index."""
    order = np.lexsort((index, -values.astype(np.float64)))[:K]
    return index[order], values[order]


def model(name, blk):
    n, cb, ce, rg, cg = (blk[f] for f in ("nrows", "col_begin", "col_end", "row_global0", "col_global0"))
    sub = R[:n, cb:ce]
    i, j = (a.ravel() for a in np.mgrid[0:n, cb:ce])
    v, gr, gc = sub.ravel(), rg + i, cg + j
    u32 = lambda a: np.asarray(a, np.int64).astype(np.uint32)  # noqa: E731
    if name in ("edges", "select_cells_ge"):
        keep = ~(v < CUT)
        if name == "edges":
            keep &= (v != 0) & (gc != gr)
        return u32(gr[keep]), u32(gc[keep]), v[keep]
    if name == "gather_cells":
        si, sj, _, _ = _gather_slots(blk)
        out = np.full(len(si), PATTERN)
        out[:-1] = R[si[:-1], sj[:-1]].view(np.uint32)
        return out, np.array([len(si) - 1])
    if name == "run_pieces_ge":
        pieces = []
        for row in range(n):
            hot = np.flatnonzero(sub[row] >= CUT)
            for run in np.split(hot, np.flatnonzero(np.diff(hot) > 1) + 1) if len(hot) else []:
                peak = run[np.argmax(sub[row, run])]  # the first position that reaches the maximum
                pieces.append((rg + row, cg + cb + run[0], cg + cb + run[-1], len(run), sub[row, peak], cg + cb + peak))
        cols = list(zip(*pieces))
        return tuple(np.array(c, np.float32) if t == 4 else u32(c) for t, c in enumerate(cols))
    if name == "topk_merge_rows":
        got = [_top(sub[row], cg + np.arange(cb, ce)) for row in range(n)]
    elif name == "topk_rows":
        got = [_top(sub[row][np.arange(cb, ce) != rg + row - cg], (cg + np.arange(cb, ce))[np.arange(cb, ce) != rg + row - cg])
               for row in range(n)]
    elif name == "topk_merge_cols":
        got = [_top(sub[:, col], rg + np.arange(n)) for col in range(ce - cb)]
    elif name == "hist_key_digits":
        bits = v.view(np.uint32)
        key = np.where(bits >> 31, ~bits, bits | np.uint32(0x80000000))
        return np.bincount(key >> 24, minlength=256).astype(np.uint64), np.zeros(1, np.uint64)
    else:
        hist = np.histogram(v, EDGES)[0].astype(np.uint64)
        return hist, np.array([(v < EDGES[0]).sum(), (v > EDGES[-1]).sum(), 0], np.uint64)
    return u32([g[0] for g in got]), np.array([g[1] for g in got], np.float32)


def same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape, (g.dtype, w.dtype, g.shape, w.shape)
        assert np.array_equal(g.view(np.uint32) if g.dtype == np.float32 else g, w.view(np.uint32) if w.dtype == np.float32 else w)


@pytest.fixture(scope="module")
def d_r():
    from seekr_amd import _lib
    m = _lib.default_context().from_numpy(R)
    yield m
    m.free()


def refused(name, d_r, blk):
    """The call raises ValueError and no kernel scope is recorded."""
    ctx = d_r.ctx
    ctx.prof_enable(True)
    ctx.prof_reset()
    try:
        with pytest.raises(ValueError):
            device(name, d_r, blk)
        assert ctx.prof_names() == [], ctx.prof_names()
    finally:
        ctx.prof_enable(False)
        ctx.prof_reset()


@pytest.mark.parametrize("name", NAMES)
def test_origin_zero_is_the_model_and_is_seen_by_the_profiler(name, d_r):
    ctx = d_r.ctx
    ctx.prof_enable(True)
    ctx.prof_reset()
    try:
        same(device(name, d_r, block()), model(name, block()))
        assert ctx.prof_names() != []  # what `refused` looks at does record an accepted call
    finally:
        ctx.prof_enable(False)
        ctx.prof_reset()


@pytest.mark.parametrize("change", [dict(nrows=6), dict(col_end=41), dict(col_begin=3, col_end=2), dict(row_global0=-1),
                                    dict(col_global0=-1)], ids=lambda c: ",".join("{}={}".format(*kv) for kv in c.items()))
@pytest.mark.parametrize("name", NAMES)
def test_a_block_outside_the_matrix_or_a_negative_origin_is_refused(name, change, d_r):
    refused(name, d_r, block(**change))


@pytest.mark.parametrize("side", [ROWS, COLS])
@pytest.mark.parametrize("name", NAMES)
def test_the_32_bit_limit_of_each_side(name, side, d_r):
    if side in LIMITED[name]:
        fits = block(**{ORIGIN[side]: U32 - EXTENT[side]})
        same(device(name, d_r, fits), model(name, fits))
        refused(name, d_r, block(**{ORIGIN[side]: U32 - EXTENT[side] + 1}))
        refused(name, d_r, block(**{ORIGIN[side]: 2 ** 63 - 1}))
    else:
        # (skr_topk_rows: columns 8 ... 39, where its diagonal rule meets no cell at either origin)
        where = dict(col_begin=8) if name == "topk_rows" else {}
        far, near = block(**{ORIGIN[side]: 2 ** 40}, **where), block(**where)
        got = device(name, d_r, far)
        same(got, device(name, d_r, near))
        same(got, model(name, far))


@pytest.mark.parametrize("name", ["hist_key_digits", "hist_edges"])
def test_the_histograms_accept_any_origin(name, d_r):
    want = model(name, block())
    same(device(name, d_r, block(row_global0=2 ** 63 - 1)), want)
    same(device(name, d_r, block(col_global0=2 ** 63 - 1)), want)
    same(device(name, d_r, block(row_global0=2 ** 63 - 1, col_global0=2 ** 63 - 1)), want)


def test_both_sides_at_their_limit_at_once(d_r):
    fits = block(row_global0=U32 - EXTENT[ROWS], col_global0=U32 - EXTENT[COLS])
    for name in NAMES:
        same(device(name, d_r, fits), model(name, fits))
