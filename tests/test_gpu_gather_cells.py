"""skr_gather_cells on the device against the numpy model of tests/gather_cells_cases.py.  Every comparison is on uint32
views; `out` starts as the pattern 0x7FC12345, so a slot that must not be written is seen to keep it.  Every call is made
twice on fresh outputs: the same bytes and the same count."""
import ctypes as C

import numpy as np
import pytest

import gather_cells_cases as gc

pytestmark = pytest.mark.gpu
INVALID = -1


def _ctx():
    from seekr_amd import _lib
    return _lib.default_context()


def run(r, rows, cols, first=None, count=None, want_count=True, **block):
    """(out bits, gathered) of one call on fresh device vectors; block: nrows, col_begin, col_end, row_global0, col_global0."""
    from seekr_amd import _lib
    ctx = _ctx()
    d_r = ctx.from_numpy(r)
    d_rows, d_cols = ctx.empty(len(rows), 1, np.uint32), ctx.empty(len(rows), 1, np.uint32)
    d_out = ctx.empty(len(rows), 1, np.float32)
    try:
        if len(rows):
            d_rows.upload(rows.reshape(-1, 1))
            d_cols.upload(cols.reshape(-1, 1))
            d_out.upload(gc.pattern(len(rows)).view(np.float32).reshape(-1, 1))
        gathered = C.c_int64(-7)
        first = 0 if first is None else first
        count = len(rows) - first if count is None else count
        rc = _lib.lib().skr_gather_cells(*_lib.block_args(d_r, **block), d_rows._h, d_cols._h, first, count, d_out._h,
                                         C.byref(gathered) if want_count else None)
        assert rc == 0, _lib.lib().skr_last_error()
        out = np.array(d_out.to_numpy()).reshape(-1).view(np.uint32) if len(rows) else np.empty(0, np.uint32)
        return out, gathered.value
    finally:
        for m in (d_r, d_rows, d_cols, d_out):
            m.free()


def check(r, rows, cols, first=None, count=None, fast=False, **block):
    rows, cols = np.ascontiguousarray(rows, np.uint32), np.ascontiguousarray(cols, np.uint32)
    f = 0 if first is None else first
    c = len(rows) - f if count is None else count
    geometry = dict(nrows=r.shape[0], col_begin=0, col_end=r.shape[1], row_global0=0, col_global0=0)
    geometry.update(block)
    want, n = (gc.model_fast if fast else gc.model)(r, rows=rows, cols=cols, first=f, count=c, out_bits=gc.pattern(len(rows)),
                                                    **geometry)
    got, gathered = run(r, rows, cols, first, count, **block)
    again, gathered_again = run(r, rows, cols, first, count, **block)
    assert gathered == n == gathered_again
    assert np.array_equal(got, want) and np.array_equal(again, got)
    return got, n


def test_block_edges_and_origin_near_two_to_the_32():
    rows, cols, inside = gc.edge_list()
    got, n = check(gc.edge_matrix(), rows, cols, **gc.EDGE)
    assert n == inside == 40 and int((got == gc.PATTERN).sum()) == len(rows) - inside


def test_bit_patterns_pass_unchanged():
    r = gc.special_matrix()
    i, j = np.divmod(np.random.default_rng(3).permutation(r.size), r.shape[1])
    got, n = check(r, i, j)
    assert n == r.size and np.array_equal(got, r.view(np.uint32)[i, j])
    check(r, i + 100, j + 7, row_global0=100, col_global0=7)


def test_sub_range_leaves_the_other_slots_alone():
    r = gc.edge_matrix()
    rng = np.random.default_rng(5)
    rows, cols = rng.integers(0, 9, 300), rng.integers(0, 16, 300)  # every slot lies in the block
    got, n = check(r, rows, cols, first=70, count=130)
    assert n == 130 and np.all(got[:70] == gc.PATTERN) and np.all(got[200:] == gc.PATTERN)
    assert not np.any(got[70:200] == gc.PATTERN)
    check(r, rows, cols, first=299, count=1)
    check(r, rows, cols, first=0, count=64)
    check(r, rows, cols, first=63, count=66)


def test_empty_and_single():
    r = gc.edge_matrix()
    none = np.empty(0, np.uint32)
    assert run(r, none, none)[1] == 0                      # S = 0
    got, n = run(r, np.array([3], np.uint32), np.array([4], np.uint32), first=0, count=0)
    assert n == 0 and got[0] == gc.PATTERN                 # count = 0: no launch, the count is reset all the same
    got, n = run(r, np.array([3], np.uint32), np.array([4], np.uint32), first=1, count=0)
    assert n == 0 and got[0] == gc.PATTERN
    got, n = check(r, [3], [4])
    assert n == 1 and got[0] == r.view(np.uint32)[3, 4]
    got, n = check(r, [9], [4])
    assert n == 0
    got, n = run(r, np.array([3], np.uint32), np.array([4], np.uint32), want_count=False)  # gathered may be NULL
    assert got[0] == r.view(np.uint32)[3, 4]


def test_more_slots_than_one_pass_of_the_grid():
    from seekr_amd import _lib
    assert 70_001 > 256 * _ctx().compute_units()  # the grid is at most one workgroup per compute unit
    rng = np.random.default_rng(70001)
    r = rng.standard_normal((300, 300)).astype(np.float32)
    rows, cols = rng.integers(0, 300, 70_001), rng.integers(0, 300, 70_001)  # with replacement: duplicates
    got, n = check(r, rows, cols, fast=True)
    assert n == 70_001 and np.array_equal(got, r.view(np.uint32)[rows, cols])
    # a third of the list lies outside the panel [50, 250)
    got, n = check(r, rows, cols, fast=True, col_begin=50, col_end=250, nrows=299)
    assert 0 < n < 70_001


@pytest.mark.parametrize("shape", [(70_000, 3), (3, 70_000)])
def test_long_blocks(shape):
    rng = np.random.default_rng(shape[0])
    r = rng.standard_normal(shape).astype(np.float32)
    rows, cols = rng.integers(0, shape[0] + 2, 5000), rng.integers(0, shape[1] + 2, 5000)
    ends = np.array([[0, 0], [shape[0] - 1, shape[1] - 1], [shape[0] - 1, 0], [0, shape[1] - 1], [shape[0], 0], [0, shape[1]]])
    rows, cols = np.concatenate([rows, ends[:, 0]]), np.concatenate([cols, ends[:, 1]])
    got, n = check(r, rows, cols, fast=True)
    assert 0 < n < len(rows)
    check(r, rows + 1000, cols + 5, fast=True, row_global0=1000, col_global0=5)


def test_refusals_write_nothing():
    from seekr_amd import _lib
    ctx = _ctx()
    lib = _lib.lib()
    r = ctx.from_numpy(np.ones((6, 40), np.float32))
    r64, ru = ctx.empty(6, 40, np.float64), ctx.empty(6, 40, np.uint32)
    start = gc.pattern(101).view(np.float32).reshape(-1, 1)

    def u32(n=100):
        m = ctx.empty(n, 1, np.uint32)
        m.upload(np.zeros((n, 1), np.uint32))  # every slot names cell (0, 0): in the block
        return m

    def f32(n=100):
        m = ctx.empty(n, 1, np.float32)
        m.upload(start[:n])
        return m

    rows, cols, out = u32(), u32(), f32()
    made = [r, r64, ru, rows, cols, out]

    def call(mat=r, nrows=6, col_begin=0, col_end=40, row_global0=0, col_global0=0, lists=(rows, cols), first=0, count=100,
             dst=out, c=ctx, null=None):
        n = C.c_int64(-7)
        handles = [mat._h, lists[0]._h, lists[1]._h, dst._h]
        if null is not None:
            handles[null] = None
        return lib.skr_gather_cells(c._h, handles[0], nrows, col_begin, col_end, row_global0, col_global0, handles[1],
                                    handles[2], first, count, handles[3], C.byref(n))

    def untouched(m=out):
        return np.all(np.array(m.to_numpy()).view(np.uint32) == gc.PATTERN)

    refused = [dict(mat=r64), dict(mat=ru)]                                   # r is float32
    wrong = [f32(), u32(), u32(99), u32(101), f32(99), f32(101)]
    made += wrong
    refused += [dict(lists=(wrong[0], cols)), dict(lists=(rows, wrong[0])), dict(dst=wrong[1])]   # dtypes of the lists
    refused += [dict(lists=(wrong[2], cols)), dict(lists=(rows, wrong[3])), dict(dst=wrong[4]), dict(dst=wrong[5])]  # lengths
    refused += [dict(first=1), dict(first=0, count=101), dict(first=101, count=0), dict(first=100, count=1)]  # first + count > S
    refused += [dict(first=-1), dict(count=-1), dict(nrows=-1), dict(col_begin=-1), dict(row_global0=-1), dict(col_global0=-1)]
    refused += [dict(nrows=7), dict(col_end=41), dict(col_begin=30, col_end=20)]                    # a range outside r
    refused += [dict(row_global0=0xffffffff - 5), dict(col_global0=0xffffffff - 39)]                # indices past 2^32 - 1
    refused += [dict(row_global0=2 ** 63 - 1), dict(col_global0=2 ** 63 - 1), dict(row_global0=2 ** 63 - 3, col_global0=2 ** 63 - 20)]  # no wrap
    refused += [dict(null=k) for k in range(4)]
    for kw in refused:
        assert call(**kw) == INVALID, kw
        assert untouched() and all(untouched(m) for m in (wrong[0], wrong[4], wrong[5])), kw
    foreign = _lib.Context(_lib.default_device())
    assert call(c=foreign) == INVALID and untouched()
    foreign.close()
    with pytest.raises(ValueError):
        _lib.check(call(nrows=7))
    assert call(row_global0=0xffffffff - 6, col_global0=0xffffffff - 40) == 0 and untouched()  # legal, and nothing is there
    assert call(first=100, count=0) == 0 and untouched()
    assert call() == 0 and np.all(np.array(out.to_numpy()) == 1.0)
    for m in made:
        m.free()
