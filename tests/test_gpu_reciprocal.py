"""skr_topk_merge_cols (csrc/topk_cols.hip), skr_knn_pairs (csrc/knn_pairs.hip) and what stands on them —
consumers.pearson_topk_both, consumers.knn_pairs, seekr_amd.reciprocal, the knn graph of kmer_leiden and the two commands —
against the numpy models of tests/reciprocal_model.py: indices as uint32, values by their uint32 view, no tolerance."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import neighbors_cases as nc
import reciprocal_model as rm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ctx():
    from seekr_amd import _lib
    return _lib.default_context()


def limits():
    from seekr_amd import _lib
    return _lib.topk_merge_cols_limits()


def same(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(nc.bits(got[1]), nc.bits(want[1]))


GUARD = 3  # list rows before and behind the lists a call may write


def guarded_lists(ctx, width, k, running=None):
    """Device lists [GUARD + width + GUARD, k] and a view of the middle: the guard rows, and — under first = 1 — the
    middle too, hold entries that would win every comparison if they were read."""
    idx = np.full((width + 2 * GUARD, k), 5, np.uint32)
    val = np.full((width + 2 * GUARD, k), np.inf, np.float32)
    if running is not None:
        idx[GUARD:GUARD + width], val[GUARD:GUARD + width] = running
    d_idx, d_val = ctx.from_numpy(idx), ctx.from_numpy(val)
    return (d_idx, d_val), (d_idx.view(GUARD, width), d_val.view(GUARD, width))


def guards_untouched(whole, width):
    idx, val = whole[0].to_numpy(), whole[1].to_numpy()
    edge = np.r_[0:GUARD, GUARD + width:2 * GUARD + width]
    return bool((idx[edge] == 5).all() and np.isposinf(val[edge]).all())


def merge_cols(ctx, d, k, first, c0, c1, row0, col0, exclude, lists, nrows=None):
    from seekr_amd import consumers
    saw = consumers.topk_merge_cols(ctx, d, lists[0], lists[1], k, first=first, nrows=nrows, col_begin=c0, col_end=c1, row_global0=row0,
                                    col_global0=col0, exclude_diag=exclude, want_nan=True)
    return (lists[0].to_numpy(), lists[1].to_numpy()), saw


def check_block(ctx, block, k, col_begin=0, right=0, diag="inside", col_global0=7, tag=None):
    """One call on the block embedded in a NaN-poisoned wider matrix: lists, saw_nan and the guard rows."""
    rows, width = block.shape
    m = nc.embed(block, col_begin, right)
    d = ctx.from_numpy(m)
    row0, col0, exclude = nc.diagonal_offsets(diag, col_begin, width, col_global0)
    whole, lists = guarded_lists(ctx, width, k)
    got, saw = merge_cols(ctx, d, k, True, col_begin, col_begin + width, row0, col0, exclude, lists)
    want = rm.merge_cols_block(m, k, col_begin, col_begin + width, row0, col0, exclude)
    where = (tag, rows, width, k, col_begin, right, diag)
    assert same(got, want), where
    assert saw == rm.saw_nan_cols(m, col_begin, col_begin + width, row0, col0, exclude), where
    assert guards_untouched(whole, width), where
    for mat in lists + whole + (d,):
        mat.free()


def test_limits_are_the_mirrored_constants():
    from seekr_amd import _lib
    kmax, strip, step, cap = limits()
    assert (kmax, strip, step, cap) == (_lib.TOPK_COLS_KMAX, _lib.TOPK_COLS_STRIP, _lib.TOPK_COLS_STEP, _lib.TOPK_COLS_CAP)
    assert kmax >= 32 and step <= cap


def row_counts(k):
    _, _, R, cap = limits()
    return sorted({n for n in (1, k - 1, k, k + 1, R - 1, R, R + 1, cap + 1, 2 * cap + 1) if n >= 1})


def widths():
    S = limits()[1]
    return (1, 3, 4, 5, S - 1, S, S + 1, 2 * S + 1)


def ks():
    kmax = limits()[0]
    return (1, 2, 31, 32, kmax - 1, kmax)


@pytest.mark.parametrize("pattern", nc.PATTERNS)
def test_kernel_grid(pattern):
    """Every row count, width and k at the kernel's edges; poisoned lists under first = 1 in every call."""
    ctx = _ctx()
    for k in ks():
        for rows in row_counts(k):
            for width in widths():
                check_block(ctx, nc.fill(pattern, rows, width, 41), k, tag=pattern)


@pytest.mark.parametrize("pattern", ["five_values", "specials", "ascending"])
def test_alignment(pattern):
    """Every (col_begin, right) of the row kernel's list: rows that start anywhere relative to a 16-byte line."""
    ctx = _ctx()
    _, S, R, _ = limits()
    odd_ld = False
    for width in (1, 3, 4, 5, S, S + 1, 2 * S + 1):
        block = nc.fill(pattern, R + 3, width, 42)
        for col_begin, right in nc.ALIGNMENTS:
            odd_ld = odd_ld or (col_begin + width + right) % 2 == 1
            for k in (2, 33):
                check_block(ctx, block, k, col_begin=col_begin, right=right, tag=pattern)
    assert odd_ld  # no row after the first is 16-byte aligned in those


@pytest.mark.parametrize("diag", nc.DIAGONALS)
def test_diagonal(diag):
    ctx = _ctx()
    _, S, R, _ = limits()
    for rows, width in ((4, 1), (4, 5), (2 * R + 5, S + 7), (3, 2 * S + 1), (S + 9, S + 9)):
        for pattern in ("five_values", "equal", "specials"):
            block = nc.fill(pattern, rows, width, 43)
            for k in (1, 3, 64):
                check_block(ctx, block, k, col_begin=4, right=9, diag=diag, tag=pattern)


def test_nan_only_on_the_excluded_diagonal():
    ctx = _ctx()
    for rows in (6, 70):
        m = np.arange(rows * 4, dtype=np.float32).reshape(rows, 4)
        for j in range(4):
            m[j + 2, j] = np.nan  # global row j + 2 == global column j + 2
        d = ctx.from_numpy(m)
        for exclude, want_saw in ((True, False), (False, True)):
            whole, lists = guarded_lists(ctx, 4, 3)
            got, saw = merge_cols(ctx, d, 3, True, 0, 4, 0, 2, exclude, lists)
            assert same(got, rm.merge_cols_block(m, 3, 0, 4, 0, 2, exclude)) and saw == want_saw
        # one column further the NaN cells are ordinary cells
        whole, lists = guarded_lists(ctx, 4, 3)
        assert merge_cols(ctx, d, 3, True, 0, 4, 0, 3, True, lists)[1]


def test_highest_global_rows():
    from seekr_amd import consumers
    ctx = _ctx()
    for rows in (5, 130):
        block = nc.fill("five_values", rows, 6, 44)
        block[-1] = 9.0  # the last row is every column's best
        d = ctx.from_numpy(block)
        row0 = nc.TOP_COLUMN - rows + 1
        for col0 in (row0 - 3, 3, nc.TOP_COLUMN - 5):
            whole, lists = guarded_lists(ctx, 6, 4)
            got, _ = merge_cols(ctx, d, 4, True, 0, 6, row0, col0, True, lists)
            want = rm.merge_cols_block(block, 4, 0, 6, row0, col0, True)
            assert same(got, want) and int(want[0].max()) == nc.TOP_COLUMN
        for bad in (dict(row_global0=row0 + 1), dict(col_global0=nc.TOP_COLUMN - 4)):
            with pytest.raises(ValueError):
                consumers.topk_merge_cols(ctx, d, lists[0], lists[1], 4, first=True, **bad)
    for k in (0, limits()[0] + 1):
        with pytest.raises(ValueError):
            consumers.topk_merge_cols(ctx, d, lists[0], lists[1], k, first=True)


def test_running_list_in_any_order_and_with_holes():
    """The list on entry is read as a set of entries: padded slots anywhere are no entries."""
    ctx = _ctx()
    block = nc.fill("five_values", 90, 3, 45)
    d = ctx.from_numpy(block)
    k = 6
    run_idx = np.array([[200, nc.NO_CELL, 150, 151, nc.NO_CELL, 300]] * 3, np.uint32)
    run_val = np.array([[0.25, np.nan, 9.0, 9.0, 5.0, -np.inf]] * 3, np.float32)
    whole, lists = guarded_lists(ctx, 3, k, running=(run_idx, run_val))
    got, saw = merge_cols(ctx, d, k, False, 0, 3, 0, 1000, False, lists, nrows=80)
    assert same(got, rm.merge_cols_block(block[:80], k, 0, 3, 0, 1000, False, running=(run_idx, run_val))) and not saw
    assert guards_untouched(whole, 3)


def test_more_strips_than_workgroups():
    """4 rows of a block wider than a launch's workgroups x the strip (the launch is capped at a few workgroups per CU)."""
    ctx = _ctx()
    S = limits()[1]
    width = S * 1200 + 5
    rng = np.random.default_rng(46)
    block = np.array([-1.5, 0.0, 0.25, 3.0, 7.0], np.float32)[rng.integers(0, 5, (4, width))]
    d = ctx.from_numpy(block)
    whole, lists = guarded_lists(ctx, width, 3)
    got, _ = merge_cols(ctx, d, 3, True, 0, width, 20, 0, True, lists)
    # the model, vectorised for this one shape: 4 candidates a column, stable by row; a diagonal cell is put last of the
    # four, which is where k = 3 cuts
    with np.errstate(all="ignore"):
        cand = np.where(np.arange(4)[:, None] + 20 == np.arange(width)[None, :], -np.inf, block)
        order = np.argsort(-cand, axis=0, kind="stable")[:3].T
    want = (order + 20).astype(np.uint32), np.take_along_axis(np.ascontiguousarray(block.T), order, axis=1)
    assert same(got, want) and guards_untouched(whole, width)
    # ... and the loop model on both ends (the first columns hold the diagonal)
    for c0, c1 in ((0, 40), (width - 40, width)):
        assert same((got[0][c0:c1], got[1][c0:c1]), rm.merge_cols_block(block, 3, c0, c1, 20, 0, True))


@pytest.mark.parametrize("pattern", ["five_values", "specials", "ascending", "descending", "equal"])
def test_merge_over_stripes(pattern):
    """2, 3 and 7 stripes at uneven split points == the unsplit call == the model, every intermediate list included."""
    ctx = _ctx()
    _, S, _, cap = limits()
    for rows in (7, 2 * cap + 1):
        block = nc.fill(pattern, rows, S + 3, 47)
        d = ctx.from_numpy(block)
        width = block.shape[1]
        for k in (1, 33, limits()[0]):
            row0, col0 = 1000, 1000 + rows // 3
            want = rm.merge_cols_block(block, k, 0, width, row0, col0, True)
            whole, lists = guarded_lists(ctx, width, k)
            got_whole, saw_whole = merge_cols(ctx, d, k, True, 0, width, row0, col0, True, lists)
            assert same(got_whole, want), (pattern, rows, k)
            for parts in nc.MERGE_SPLITS:
                cuts = [0] + nc.split_points(rows, parts, 48) + [rows]
                whole, lists = guarded_lists(ctx, width, k)
                saw_any = False
                for p in range(len(cuts) - 1):
                    stripe = d.view(cuts[p], cuts[p + 1] - cuts[p])
                    got, saw = merge_cols(ctx, stripe, k, p == 0, 0, width, row0 + cuts[p], col0, True, lists)
                    stripe.free()
                    saw_any = saw_any or saw
                    assert saw == rm.saw_nan_cols(block[cuts[p]:cuts[p + 1]], 0, width, row0 + cuts[p], col0)
                    assert same(got, rm.merge_cols_block(block[:cuts[p + 1]], k, 0, width, row0, col0, True)), (pattern, rows, k, parts, p)
                assert same(got, want) and saw_any == saw_whole and guards_untouched(whole, width), (pattern, rows, k, parts)
        d.free()


# ---- skr_knn_pairs ----------------------------------------------------------------------------------------------------------
def device_pairs(ctx, idx_a, val_a, idx_b=None, val_b=None, mode="mutual", positive_only=False, capacity=1):
    from seekr_amd import consumers
    mats = [ctx.from_numpy(x) for x in (idx_a, val_a)] + ([None, None] if idx_b is None else [ctx.from_numpy(x) for x in (idx_b, val_b)])
    pairs = consumers.PairList(ctx, capacity)
    n = consumers.knn_pairs(*mats, mode=mode, positive_only=positive_only, into=pairs)
    counted = consumers.knn_pairs(*mats, mode=mode, positive_only=positive_only, into=None)
    out = pairs.to_host()
    assert n == counted == len(out[0]) == len(pairs)
    pairs.free()
    for m in mats:
        if m is not None:
            m.free()
    return out


@pytest.mark.parametrize("self_form", [False, True])
def test_knn_pairs_against_the_model(self_form):
    ctx = _ctx()
    rng = np.random.default_rng(51)
    kmax = limits()[0]
    for n1, n2 in ((1, 1), (2, 3), (7, 5), (40, 40), (13, 40), (40, 9), (33, 17)):
        n2 = n1 if self_form else n2
        for k in (1, 2, 8, kmax):
            idx_a, val_a = rm.random_lists(rng, n1, n2, k, self_form)
            rest = (None, None) if self_form else rm.random_lists(rng, n2, n1, k)
            for mode in ("mutual", "union"):
                for positive_only in (False, True):
                    got = device_pairs(ctx, idx_a, val_a, *rest, mode=mode, positive_only=positive_only)
                    want = rm.knn_pairs_model(idx_a, val_a, *rest, mode=mode, positive_only=positive_only)
                    assert rm.same_pairs(got, want), (n1, n2, k, mode, positive_only)


def test_knn_pairs_refuses_an_index_out_of_range():
    """The index is reported, never used as an address (the pairing sorts keys; it reads no list through an index)."""
    from seekr_amd import consumers
    ctx = _ctx()
    val = np.full((4, 2), 0.5, np.float32)
    for self_form, bad in ((True, 4), (True, 0xFFFFFFFE), (False, 3), (False, 0x80000000)):
        idx_a = np.array([[1, 2], [0, 2], [0, bad], [1, 0]], np.uint32)
        idx_b = np.array([[0, 1], [1, 2], [3, 0]], np.uint32)
        mats = [ctx.from_numpy(idx_a), ctx.from_numpy(val)] + ([None, None] if self_form else [ctx.from_numpy(idx_b), ctx.from_numpy(val[:3])])
        with pytest.raises(ValueError):
            rm.knn_pairs_model(idx_a, val, *((None, None) if self_form else (idx_b, val[:3])))
        pairs = consumers.PairList(ctx, 64)
        with pytest.raises(ValueError):
            consumers.knn_pairs(*mats, mode="union", into=pairs)
        assert len(pairs) == 0
    # ... in idx_b: entries index set A
    idx_a = np.array([[1, 2], [0, 2], [0, 1], [1, 0]], np.uint32)
    idx_b = np.array([[0, 1], [1, 4], [3, 0]], np.uint32)
    with pytest.raises(ValueError):
        consumers.knn_pairs(ctx.from_numpy(idx_a), ctx.from_numpy(val), ctx.from_numpy(idx_b), ctx.from_numpy(val[:3]), mode="union")
    # a padded slot is no index
    idx_b[1, 1] = nc.NO_CELL
    assert consumers.knn_pairs(ctx.from_numpy(idx_a), ctx.from_numpy(val), ctx.from_numpy(idx_b), ctx.from_numpy(val[:3]), mode="union") > 0


def test_knn_pairs_count_then_write():
    """Outputs too small: nothing is written and the count comes back; the second call fills behind out_offset; some but
    not all outputs NULL is refused."""
    from seekr_amd import _lib
    ctx = _ctx()
    rng = np.random.default_rng(52)
    idx_a, val_a = rm.random_lists(rng, 30, 25, 6)
    idx_b, val_b = rm.random_lists(rng, 25, 30, 6)
    want = rm.knn_pairs_model(idx_a, val_a, idx_b, val_b, mode="union")
    n = len(want[0])
    assert n > 40
    mats = [ctx.from_numpy(x) for x in (idx_a, val_a, idx_b, val_b)]
    head = (ctx._h, mats[0]._h, mats[1]._h, mats[2]._h, mats[3]._h, 1, 0)
    dtypes = (np.uint32, np.uint32, np.float32, np.uint32, np.uint32)
    count = C.c_int64(0)
    _lib.check(_lib.lib().skr_knn_pairs(*head, None, None, None, None, None, 0, C.byref(count)))
    assert count.value == n
    offset = 7
    for cap in (n - 1, offset + n - 1, offset + n):
        outs = [ctx.from_numpy(np.full((cap, 1), 0xABABABAB, np.uint32).view(t)) for t in dtypes]
        count = C.c_int64(0)
        _lib.check(_lib.lib().skr_knn_pairs(*head, *[m._h for m in outs], offset, C.byref(count)))
        assert count.value == n
        host = [m.to_numpy().reshape(-1) for m in outs]
        if cap < offset + n:
            assert all((nc.bits(h) if h.dtype == np.float32 else h).tolist() == [0xABABABAB] * cap for h in host)
        else:
            assert all((nc.bits(h) if h.dtype == np.float32 else h)[:offset].tolist() == [0xABABABAB] * offset for h in host)
            assert rm.same_pairs(tuple(h[offset:] for h in host), want)
        with pytest.raises(ValueError):
            _lib.check(_lib.lib().skr_knn_pairs(*head, outs[0]._h, outs[1]._h, None, outs[3]._h, outs[4]._h, 0, C.byref(count)))
        for m in outs:
            m.free()


def test_knn_pairs_long_lists():
    """5 000 x 10 lists on either side: the sort takes several chunks per pass and three digit passes."""
    ctx = _ctx()
    rng = np.random.default_rng(53)
    n, k = 5000, 10
    near = lambda: ((np.arange(n)[:, None] + rng.integers(1, 40, (n, 1)) * np.arange(1, k + 1)[None, :]) % n).astype(np.uint32)  # noqa: E731
    vals = lambda: np.array([-0.5, 0.0, 0.25, 0.5, np.nan], np.float32)[rng.integers(0, 5, (n, k))]  # noqa: E731
    idx_a, val_a, idx_b, val_b = near(), vals(), near(), vals()
    idx_a[rng.random((n, k)) < 0.1] = nc.NO_CELL
    for rest in ((idx_b, val_b), (None, None)):
        for mode in ("mutual", "union"):
            got = device_pairs(ctx, idx_a, val_a, *rest, mode=mode, positive_only=mode == "union", capacity=1 << 12)
            assert rm.same_pairs(got, rm.knn_pairs_model(idx_a, val_a, *rest, mode=mode, positive_only=mode == "union")), mode


# ---- pearson_topk_both ------------------------------------------------------------------------------------------------------
SPLITS = ((128, 96), (300, None), (37, 300))


def prepared(ctx, x):
    from seekr_amd import _lib
    from seekr_amd import pearson as pearson_mod
    return _lib.operand_fill(ctx, ctx.from_numpy(x), None, pearson_mod._precision_for(np.dtype(np.float32), True))[0]


@functools.lru_cache(maxsize=None)
def two_sets():
    """300 x 257 profiles with exact copies across the sets (ties across stripes and panels) and their operands — once."""
    ctx = _ctx()
    x = nc.kmer_profiles(300, 3, 61)
    y = nc.kmer_profiles(257, 3, 62)
    y[[3, 100, 256]] = x[7]
    x[[150, 299]] = x[7]
    return x, y, prepared(ctx, x), prepared(ctx, y)


def assembled_r(ctx, a, b, stripe_rows, panel_rows):
    """r put together from the very contractions the sweep makes (as in tests/test_gpu_neighbors.py)."""
    from seekr_amd import _lib
    n, m = a.rows, b.rows
    stripe_rows = max(1, min(int(stripe_rows), n))
    panel_rows = m if panel_rows is None else max(1, min(int(panel_rows), m))
    buf = ctx.empty(stripe_rows, panel_rows)
    r = np.empty((n, m), np.float32)
    for s0 in range(0, n, stripe_rows):
        rows = min(stripe_rows, n - s0)
        for p0 in range(0, m, panel_rows):
            cols = min(panel_rows, m - p0)
            _lib.pearson_gemm_op(ctx, a if rows == n else a.view(s0, rows), b if cols == m else b.view(p0, cols), buf)
            r[s0:s0 + rows, p0:p0 + cols] = buf.to_numpy()[:rows, :cols]
    buf.free()
    return r


@functools.lru_cache(maxsize=None)
def both_of(split, k):
    from seekr_amd import consumers
    _, _, za, zb = two_sets()
    return consumers.pearson_topk_both(za, zb, k=k, stripe_rows=split[0], panel_rows=split[1])


@pytest.mark.parametrize("split", SPLITS)
def test_pearson_topk_both(split):
    from seekr_amd import consumers
    ctx = _ctx()
    _, _, za, zb = two_sets()
    r = assembled_r(ctx, za, zb, *split)
    for k in (1, 10, limits()[0]):
        got = both_of(split, k)
        rows = consumers.pearson_topk(za, zb, k=k, stripe_rows=split[0], panel_rows=split[1])
        assert same(got[:2], rows), (split, k)  # byte-identical to pearson_topk
        assert same(got[:2], nc.merge_block(r, k, exclude_diag=False)), (split, k)
        assert same(got[2:], rm.merge_cols_block(r, k, exclude_diag=False)), (split, k)
        if k == 10:  # the copies of x[7] find each other from both sides
            assert set(got[0][7][:3]) == {3, 100, 256} and set(got[2][100][:3]) == {7, 150, 299}
    # the lists left on the device are the same lists
    dev = consumers.pearson_topk_both(za, zb, k=10, stripe_rows=split[0], panel_rows=split[1], keep_device=True)
    host = both_of(split, 10)
    assert same((dev[0].to_numpy(), dev[1].to_numpy()), host[:2]) and same((dev[2].to_numpy(), dev[3].to_numpy()), host[2:])
    for m in dev:
        m.free()


def test_pearson_topk_both_all_splits_give_the_same_bytes():
    """The order is total, so the lists are a function of r alone.  The number of cells of r whose bits differ between the
    splits' own contractions is printed first (a [stripe, panel] block need not carry the bits of another block shape:
    tests/test_gpu_neighbors.py, test_blocks_against_the_whole_matrix_call)."""
    ctx = _ctx()
    _, _, za, zb = two_sets()
    rs = [assembled_r(ctx, za, zb, *split) for split in SPLITS]
    for split, r in zip(SPLITS[1:], rs[1:]):
        print("cells of r whose bits differ between the blocks of %r and of %r: %d" % (SPLITS[0], split, int((nc.bits(r) != nc.bits(rs[0])).sum())))
    first = both_of(SPLITS[0], 10)
    for split in SPLITS[1:]:
        got = both_of(split, 10)
        assert same(got[:2], first[:2]) and same(got[2:], first[2:]), split


def test_pearson_topk_both_float32_layout(golden_dir):
    from seekr_amd import _lib, consumers
    ctx = _ctx()
    x = np.ascontiguousarray(np.load(os.path.join(golden_dir, "regress_r4_two_level_rows.npz"))["a"][:12]).copy()
    rng = np.random.default_rng(63)
    x = np.concatenate([x, rng.standard_normal((8, x.shape[1])).astype(np.float32)])
    lo, hi = float(x[0].min()), float(x[0].max())
    x[3] = lo  # one column carries the row's energy: the fill routes the operand to the float32 layout
    x[3, 1234] = hi
    x[7] = x[2]
    za = prepared(ctx, x)
    assert za.kind == 0  # the route under test
    zb = _lib.operand_fill(ctx, ctx.from_numpy(np.ascontiguousarray(x[::-1][:15] * np.float32(0.5) + x[:15])), None, _lib.PREC_FP32)[0]
    assert zb.kind == 0
    for split in ((8, None), (7, 4)):
        r = assembled_r(ctx, za, zb, *split)
        got = consumers.pearson_topk_both(za, zb, k=5, stripe_rows=split[0], panel_rows=split[1])
        assert same(got[:2], consumers.pearson_topk(za, zb, k=5, stripe_rows=split[0], panel_rows=split[1]))
        assert same(got[:2], nc.merge_block(r, 5, exclude_diag=False)) and same(got[2:], rm.merge_cols_block(r, 5, exclude_diag=False))


# ---- end to end -------------------------------------------------------------------------------------------------------------
def frame_pairs(frame):
    from seekr_amd import reciprocal
    assert list(frame.columns)[:5] == list(reciprocal.COLUMNS)
    return tuple(frame[c].to_numpy() for c in reciprocal.COLUMNS)


@pytest.mark.parametrize("mode", ["mutual", "union"])
def test_reciprocal_hits(mode):
    import pandas as pd
    from seekr_amd import consumers
    from seekr_amd.neighbors import nearest
    from seekr_amd.reciprocal import reciprocal_hits
    x, y, za, zb = two_sets()
    # two sets: the model on the lists of the same sweep
    lists = consumers.pearson_topk_both(za, zb, k=4)
    got = frame_pairs(reciprocal_hits(x, y, k=4, mode=mode))
    assert rm.same_pairs(got, rm.knn_pairs_model(*lists, mode=mode)) and len(got[0]) > 0
    if mode == "mutual":
        assert {(7, 3), (7, 100), (7, 256)} <= set(zip(got[0].tolist(), got[1].tolist()))
    # one set: the model on nearest's lists, self form
    idx, val = nearest(x, k=4)
    got = frame_pairs(reciprocal_hits(x, k=4, mode=mode))
    assert rm.same_pairs(got, rm.knn_pairs_model(idx, val, mode=mode)) and (got[0] < got[1]).all()
    # labelled frames: names beside the indices
    fx = pd.DataFrame(x[:40], index=["a%d" % i for i in range(40)])
    fy = pd.DataFrame(y[:30], index=["b%d" % i for i in range(30)])
    frame = reciprocal_hits(fx, fy, k=2, mode=mode)
    assert list(frame["row_name"]) == ["a%d" % i for i in frame["row"]] and list(frame["col_name"]) == ["b%d" % j for j in frame["col"]]


@pytest.mark.parametrize("mode", ["mutual", "union"])
def test_knn_graph_into_communities(mode):
    from seekr_amd.consumers import pearson_topk
    from seekr_amd.leiden import communities, pearson_communities
    from seekr_amd.reciprocal import knn_graph
    x, _, za, _ = two_sets()
    rows, cols, vals = knn_graph(za, 6, mode=mode)
    want = rm.knn_pairs_model(*pearson_topk(za, k=6), mode=mode, positive_only=True)
    assert np.array_equal(rows, want[0]) and np.array_equal(cols, want[1]) and np.array_equal(nc.bits(vals), nc.bits(want[2]))
    assert (rows < cols).all() and (vals > 0).all() and len(rows) <= 300 * 6
    mem, q, _ = communities(rows, cols, vals, 300)
    mem_model, q_model, _ = communities(want[0], want[1], want[2], 300)
    assert np.array_equal(mem, mem_model) and q == q_model
    mem2, q2, info = pearson_communities(za, knn=6, knn_mode=mode)
    assert np.array_equal(mem2, mem) and q2 == q and info["n_edges"] == len(rows)


E2E_K = 3


@pytest.fixture(scope="module")
def repeats_case(tmp_path_factory):
    """Three groups of ten sequences, each group the tandem repeats of its own motif with a few letters changed."""
    from seekr_amd.kmer_counts import BasicCounter
    d = tmp_path_factory.mktemp("reciprocal")
    rng = np.random.default_rng(71)
    motifs = ["ACGGTCA", "TTTGCAAGC", "GATCCGGAAT"]
    seqs, which = [], []
    for i in range(30):
        s = list((motifs[i % 3] * 60)[:360 + int(rng.integers(0, 40))])
        for at in rng.integers(0, len(s), 25):
            s[at] = "ACGT"[int(rng.integers(0, 4))]
        seqs.append("".join(s))
        which.append(i % 3)
    fa = d / "seqs.fa"
    fa.write_text("".join(">tx%d\n%s\n" % (i, s) for i, s in enumerate(seqs)))
    c = BasicCounter(str(fa), k=E2E_K, silent=True)
    c.get_counts()
    np.save(d / "mean.npy", c.mean)
    np.save(d / "std.npy", c.std)
    return d, fa, np.asarray(which)


def test_kmer_leiden_knn(repeats_case):
    from seekr_amd.kmer_leiden import kmer_leiden
    d, fa, which = repeats_case
    mem = kmer_leiden(str(fa), str(d / "mean.npy"), str(d / "std.npy"), E2E_K, knn=5)
    for g in range(3):
        assert len(set(mem[which == g].tolist())) == 1, (g, mem)
    assert len(set(mem.tolist())) == 3
    # mutual: a sequence nobody lists back is a community of its own (its node has no edge), so a group may come in
    # pieces — but no community holds sequences of two groups
    mem = kmer_leiden(str(fa), str(d / "mean.npy"), str(d / "std.npy"), E2E_K, knn=5, knn_mode="mutual")
    for c in set(mem.tolist()):
        assert len(set(which[mem == c].tolist())) == 1, (c, mem)
    with pytest.raises(ValueError):
        kmer_leiden(str(fa), str(d / "mean.npy"), str(d / "std.npy"), E2E_K, knn=5, density=0.1)


def run_command(name, argv):
    code = "import sys; sys.argv = %r; from seekr_amd.console_scripts import %s; %s()" % (["seekr_" + name[8:]] + argv, name, name)
    proc = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0, proc.stderr


def test_commands(repeats_case, tmp_path):
    import pandas as pd
    from seekr_amd import _lib
    from seekr_amd.kmer_leiden import kmer_leiden
    from seekr_amd.reciprocal import reciprocal_hits
    x = nc.kmer_profiles(20, 3, 72).astype(np.float64)
    y = nc.kmer_profiles(14, 3, 73).astype(np.float64)
    names_x, names_y = ["tx%d" % i for i in range(20)], ["mm%d, v2" % j if j == 4 else "mm%d" % j for j in range(14)]
    kmers = ["c%d" % j for j in range(64)]
    pd.DataFrame(x, index=names_x, columns=kmers).to_csv(tmp_path / "x.csv")
    pd.DataFrame(y, index=names_y, columns=kmers).to_csv(tmp_path / "y.csv")
    out = tmp_path / "hits.csv"
    run_command("console_reciprocal_hits", [str(tmp_path / "x.csv"), str(tmp_path / "y.csv"), "-n", "3", "-m", "union", "-o", str(out)])
    vx, vy = pd.read_csv(tmp_path / "x.csv", index_col=0).to_numpy(), pd.read_csv(tmp_path / "y.csv", index_col=0).to_numpy()
    want = frame_pairs(reciprocal_hits(vx, vy, k=3, mode="union"))
    frame = pd.read_csv(out)
    assert list(frame.columns) == ["row", "col", "r", "rank_row", "rank_col"] and len(frame) == len(want[0]) > 0
    assert list(frame["row"]) == [names_x[i] for i in want[0]] and list(frame["col"]) == [names_y[j] for j in want[1]]
    assert np.array_equal(nc.bits(frame["r"].to_numpy().astype(np.float32)), nc.bits(want[2]))
    for col, ranks in (("rank_row", want[3]), ("rank_col", want[4])):
        assert [_lib.TOPK_PAD_IDX if np.isnan(v) else int(v) for v in frame[col]] == ranks.tolist()
    # .npy input, one file, mutual: indices instead of labels
    np.save(tmp_path / "x.npy", vx.astype(np.float32))
    out2 = tmp_path / "self.csv"
    run_command("console_reciprocal_hits", [str(tmp_path / "x.npy"), "-n", "2", "-o", str(out2), "-bi"])
    want = frame_pairs(reciprocal_hits(vx.astype(np.float32), k=2))
    frame = pd.read_csv(out2)
    assert list(frame["row"]) == want[0].tolist() and list(frame["col"]) == want[1].tolist() and len(frame) > 0
    assert list(frame["rank_row"]) == want[3].tolist() and list(frame["rank_col"]) == want[4].tolist()
    assert np.array_equal(nc.bits(frame["r"].to_numpy().astype(np.float32)), nc.bits(want[2]))
    # seekr_kmer_leiden -nn
    d, fa, _ = repeats_case
    run_command("console_kmer_leiden", [str(fa), str(d / "mean.npy"), str(d / "std.npy"), str(E2E_K), "-nn", "5", "-nm", "mutual", "-cf",
                                        str(tmp_path / "cmd"), "--edges", "nonzero"])
    mem = kmer_leiden(str(fa), str(d / "mean.npy"), str(d / "std.npy"), E2E_K, knn=5, knn_mode="mutual", csvfile=str(tmp_path / "api"),
                      edges="nonzero")
    nodes = pd.read_csv(tmp_path / "cmd_nodes_leiden.csv")
    assert [mem[int(s[2:])] + 1 for s in nodes["Id"]] == list(nodes["Color"])
    for name in ("nodes", "edges"):
        assert (tmp_path / ("cmd_%s_leiden.csv" % name)).read_bytes() == (tmp_path / ("api_%s_leiden.csv" % name)).read_bytes()
    assert len(pd.read_csv(tmp_path / "cmd_edges_leiden.csv")) <= 30 * 5
