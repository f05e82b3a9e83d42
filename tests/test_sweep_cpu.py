"""consumers.Sweep, the one producer of [stripe, panel] blocks of r, without a device: stand-in operands and buffers that
count what is live, the contraction replaced by a recorder.  Which cells the blocks cover in both modes and for every
split, what is contracted (the operand itself where a block is all of it), that nothing is made for empty input, and
that no view or buffer outlives a run, a failing visitor, or a failing reduction in pearson_topk and pearson_cells.
Last, the array form of the float32 key against significant._key."""
import numpy as np
import pytest

from seekr_amd import _lib, consumers


class Ctx:
    """Hands out stand-in buffers and counts those not yet freed."""
    _h = None

    def __init__(self):
        self.live = self.made = 0

    def empty(self, rows, cols, dtype=np.float32):
        self.live += 1
        self.made += 1
        return Buf(self, rows, cols)


class Buf:
    _h = None

    def __init__(self, ctx, rows, cols):
        self.ctx, self.rows, self.cols, self.freed, self.downloads = ctx, rows, cols, False, []

    def to_numpy(self, row0, nrows, out):
        self.downloads.append((row0, nrows, out.shape[0]))

    def free(self):
        assert not self.freed, "a buffer is freed twice"
        self.freed = True
        self.ctx.live -= 1


class Op:
    """A prepared operand of `rows` rows, or a view of one: rows [row0, row0 + rows) of `root`."""
    _h = None

    def __init__(self, ctx, rows, root=None, row0=0):
        self.ctx, self.rows, self.root, self.row0, self.freed = ctx, rows, root, row0, False
        self.live_views = 0

    def view(self, row0, nrows):
        assert self.root is None and 0 <= row0 and nrows >= 1 and row0 + nrows <= self.rows
        self.live_views += 1
        return Op(self.ctx, nrows, self, row0)

    def free(self):
        assert self.root is not None, "the sweep frees an operand that is not its own"
        assert not self.freed, "a view is freed twice"
        self.freed = True
        self.root.live_views -= 1


@pytest.fixture
def gemms(monkeypatch):
    """The contractions a test asks for, as (a, b, buf), in place of the device call."""
    calls = []
    monkeypatch.setattr(_lib, "pearson_gemm_op", lambda ctx, a, b, buf, **kw: calls.append((a, b, buf)))
    return calls


def splits(n, m):
    return [(s, p) for s in (1, 3, n, n + 5) for p in (None, 1, 2, m + 5)]


def cover(sweep, n, m, gemms):
    """The visited-count matrix of one run; every block is checked against the contraction made just before it."""
    count = np.zeros((n, m), dtype=np.int64)
    a, b = sweep.a, sweep.b

    def visit(buf, nrows, col_begin, col_end, row_global0, col_global0, upper_only):
        op_a, op_b, into = gemms[-1]
        cols = col_end - col_begin
        assert into is buf is sweep.buf and nrows <= buf.rows and cols <= buf.cols and col_begin == 0
        assert upper_only == sweep.upper_only
        # a block that is the whole operand is the operand itself, any other a live view of exactly its rows
        for op, whole, row0, rows in ((op_a, a, row_global0, nrows), (op_b, b, col_global0, cols)):
            if rows == whole.rows:
                assert op is whole
            else:
                assert op.root is whole and (op.row0, op.rows) == (row0, rows) and not op.freed
        gi = row_global0 + np.arange(nrows)[:, None]
        gj = col_global0 + np.arange(col_begin, col_end)[None, :]
        if upper_only:
            assert gj.max() >= gi.min(), "a block wholly below the diagonal"
        count[gi, gj] += (gj > gi) if upper_only else np.ones((nrows, cols), dtype=bool)

    before = len(gemms)
    sweep.run(visit)
    return count, len(gemms) - before


@pytest.mark.parametrize("n,m", [(7, 5), (1, 1), (8, 8)])
def test_every_cell_lies_in_exactly_one_block(n, m, gemms):
    for stripe, panel in splits(n, m):
        ctx = Ctx()
        a, b = Op(ctx, n), Op(ctx, m)
        with consumers.Sweep(a, b, stripe, panel) as sweep:
            assert not sweep.upper_only
            count, blocks = cover(sweep, n, m, gemms)
            assert (count == 1).all(), (stripe, panel)
            assert blocks == -(-n // min(stripe, n)) * -(-m // min(panel or m, m))
            assert (sweep.buf.rows, sweep.buf.cols) == (min(stripe, n), min(panel or m, m))
            assert a.live_views == b.live_views == 0 and ctx.live == 1
            kept = sweep.buf
            again, _ = cover(sweep, n, m, gemms)  # a second pass: the same cells in the same buffer
            assert (again == 1).all() and sweep.buf is kept and ctx.made == 1
        assert ctx.live == 0 and a.live_views == b.live_views == 0


@pytest.mark.parametrize("n", [7, 1, 8])
def test_triangle_mode_covers_the_cells_right_of_the_diagonal_once(n, gemms):
    want = np.triu(np.ones((n, n), dtype=np.int64), 1)
    for stripe, panel in splits(n, n):
        ctx = Ctx()
        a = Op(ctx, n)
        with consumers.Sweep(a, None, stripe, panel) as sweep:
            assert sweep.upper_only and sweep.b is a
            count, blocks = cover(sweep, n, n, gemms)
            assert np.array_equal(count, want), (stripe, panel)
            assert blocks >= 1 and a.live_views == 0
        assert ctx.live == 0


def test_empty_input_makes_nothing(gemms):
    for n, m in ((0, 5), (5, 0), (0, 0)):
        ctx = Ctx()
        for sweep in (consumers.Sweep(Op(ctx, n), Op(ctx, m), 3, 2), consumers.Sweep(Op(ctx, n), Op(ctx, m))):
            sweep.run(lambda *a, **kw: pytest.fail("a visit without a cell"))
            sweep.free()
    ctx = Ctx()
    consumers.Sweep(Op(ctx, 0)).run(lambda *a, **kw: pytest.fail("a visit without a cell"))
    assert ctx.made == 0 and not gemms


@pytest.mark.parametrize("self_cmp", [False, True])
def test_a_failing_visitor_leaves_no_view_and_free_releases_the_buffer(self_cmp, gemms):
    ctx = Ctx()
    a, b = Op(ctx, 7), Op(ctx, 5)
    sweep = consumers.Sweep(a, None if self_cmp else b, 3, 2)
    seen = []

    def visit(buf, **where):
        seen.append(where)
        if len(seen) == 3:
            raise KeyError("third block")

    with pytest.raises(KeyError, match="third block"):
        sweep.run(visit)
    assert len(seen) == 3 and a.live_views == b.live_views == 0
    assert ctx.live == 1  # the buffer is the caller's until free()
    sweep.free()
    assert ctx.live == 0
    sweep.free()  # nothing left to do
    assert ctx.live == 0 and ctx.made == 1
    with pytest.raises(KeyError):  # and as a context manager
        with consumers.Sweep(a, None if self_cmp else b, 3, 2) as again:
            seen.clear()
            again.run(visit)
    assert ctx.live == 0 and a.live_views == b.live_views == 0


def test_a_failing_contraction_leaves_no_view(monkeypatch):
    def fail(ctx, a, b, buf, **kw):
        raise RuntimeError("contraction")

    monkeypatch.setattr(_lib, "pearson_gemm_op", fail)
    ctx = Ctx()
    a, b = Op(ctx, 7), Op(ctx, 5)
    with pytest.raises(RuntimeError, match="contraction"):
        with consumers.Sweep(a, b, 3, 2) as sweep:
            sweep.run(lambda *args, **kw: None)
    assert ctx.live == 0 and a.live_views == b.live_views == 0


# ---- the two callers ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("self_cmp", [False, True])
def test_pearson_topk_starts_and_downloads_each_stripe_once(self_cmp, gemms, monkeypatch):
    merges, lists = [], []

    def merge(ctx, r, idx, val, k, first, nrows, col_begin, col_end, row_global0, col_global0, exclude_diag):
        assert exclude_diag == self_cmp and idx.downloads == val.downloads
        lists[:] = [idx, val]
        merges.append((row_global0, col_global0, first, len(idx.downloads)))

    monkeypatch.setattr(_lib, "topk_merge_rows", merge)
    ctx = Ctx()
    a, b = Op(ctx, 7), Op(ctx, 5)
    m = 7 if self_cmp else 5
    idx, val = consumers.pearson_topk(a, None if self_cmp else b, k=4, stripe_rows=3, panel_rows=2)
    assert idx.shape == val.shape == (7, 4)
    # all of a x a in the self-comparison too; a stripe's lists start at its first panel and come down after its last
    assert [t[:2] for t in merges] == [(s0, p0) for s0 in (0, 3, 6) for p0 in range(0, m, 2)]
    assert all(first == (p0 == 0) and downloads == s0 // 3 for s0, p0, first, downloads in merges)
    assert lists[0].downloads == lists[1].downloads == [(0, 3, 3), (0, 3, 3), (0, 1, 1)]
    assert ctx.live == 0 and ctx.made == 3 and a.live_views == b.live_views == 0


@pytest.mark.parametrize("self_cmp", [False, True])
def test_pearson_topk_frees_everything_when_the_merge_raises(self_cmp, gemms, monkeypatch):
    calls = []

    def merge(*args, **kw):
        calls.append(kw)
        if len(calls) == 4:  # in the second stripe, past its first panel
            raise RuntimeError("merge")

    monkeypatch.setattr(_lib, "topk_merge_rows", merge)
    ctx = Ctx()
    a, b = Op(ctx, 7), Op(ctx, 5)
    with pytest.raises(RuntimeError, match="merge"):
        consumers.pearson_topk(a, None if self_cmp else b, k=4, stripe_rows=3, panel_rows=2)
    assert len(calls) == 4 and ctx.made == 3
    assert ctx.live == 0 and a.live_views == b.live_views == 0


def test_pearson_cells_frees_everything_when_the_selection_raises(gemms, monkeypatch):
    calls, fail_at = [], []

    def select(buf, cutoff, into, **where):
        calls.append(where)
        if len(calls) in fail_at:
            raise RuntimeError("select")
        return 0, len(calls) == 2

    monkeypatch.setattr(consumers, "select_cells", select)
    ctx = Ctx()
    a, b = Op(ctx, 7), Op(ctx, 5)
    cells, saw_nan, panelled = consumers.pearson_cells(a, b, 0.5, stripe_rows=3, panel_rows=2)
    assert saw_nan and panelled and len(calls) == 9
    assert set(calls[0]) == {"nrows", "col_begin", "col_end", "row_global0", "col_global0"}
    assert ctx.live == 3 and a.live_views == b.live_views == 0  # the list's three vectors are the caller's
    cells.free()
    calls.clear()
    cells, saw_nan, panelled = consumers.pearson_cells(a, b, 0.5, stripe_rows=7)
    assert not saw_nan and not panelled and len(calls) == 1
    cells.free()
    assert ctx.live == 0
    calls.clear()
    fail_at.append(4)
    made = ctx.made
    with pytest.raises(RuntimeError, match="select"):
        consumers.pearson_cells(a, b, 0.5, stripe_rows=3, panel_rows=2)
    assert len(calls) == 4 and ctx.made == made + 4 and ctx.live == 0 and a.live_views == b.live_views == 0


# ---- the float32 key ------------------------------------------------------------------------------------------------------
def test_the_array_key_is_significant_key_and_round_trips_the_bits():
    from seekr_amd import significant
    tiny, top = np.float32(1e-45), np.finfo(np.float32).max
    x = np.array([0.0, -0.0, np.inf, -np.inf, tiny, -tiny, np.float32(1e-39), -np.float32(1e-39), 1, -1, top, -top,
                  np.finfo(np.float32).tiny, -np.finfo(np.float32).tiny], dtype=np.float32)
    keys = consumers.float32_key(x)
    assert keys.dtype == np.uint32 and keys.shape == x.shape
    assert [int(k) for k in keys] == [significant._key(v) for v in x]
    back = consumers.float32_unkey(keys)
    assert back.dtype == np.float32 and np.array_equal(back.view(np.uint32), x.view(np.uint32))
    for v, k in zip(x, keys):
        assert type(significant._key(v)) is int
        s = significant._unkey(int(k))
        assert type(s) is np.float32 and s.view(np.uint32) == v.view(np.uint32)
    order = np.argsort(keys, kind="stable")
    assert np.array_equal(x[order].view(np.uint32), np.array(
        [-np.inf, -top, -1, -np.finfo(np.float32).tiny, -np.float32(1e-39), -tiny, -0.0, 0.0, tiny, np.float32(1e-39),
         np.finfo(np.float32).tiny, 1, top, np.inf], dtype=np.float32).view(np.uint32))
