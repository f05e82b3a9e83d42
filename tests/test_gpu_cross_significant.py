"""skr_select_cells_ge / skr_vec_copy, consumers.CellList, and the functions on top of them on the device: two-set
significant.significant_pairs, candidates="device", windows.domain_significant and the two commands.  The expected cells
come from the package's own full-matrix path — pearson_gemm_op (or domain_pearson) -> p-values ->
adjust_pvalues(symmetric=False) over every cell — and are compared bit for bit; p_adj against the float64 of the full
path's value (it is float32 there for bonferroni and sidak), the significant cells being those with float64(p_adj) <= alpha.

The condition every parity test asserts on the full path before it compares anything (cross_significant_cases.condition):
at least one cell is significant and fewer than half of the cells are."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import cross_significant_cases as cc
import significant_cases as sc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALPHA = 0.05
FIELDS = ("rows", "cols", "r", "p", "p_adj")


def _ctx():
    from seekr_amd import _lib
    return _lib.default_context()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def device_p(r, fitres):
    from seekr_amd import consumers
    if isinstance(fitres, np.ndarray):
        return consumers.empirical_pvalues(r, fitres)
    name, _, params = fitres[0]
    return consumers.parametric_pvalues(r, name, params)


class FullPath:
    """r and p of a whole (device) matrix r for one background — once, left unchanged — and the expected cells per method."""

    def __init__(self, r_dev, fitres):
        self.d_p = device_p(r_dev, fitres)
        self.r, self.p = np.array(r_dev.to_numpy()), np.array(self.d_p.to_numpy())
        self.cells = self.r.size

    def expected(self, method, alpha=ALPHA):
        from seekr_amd import consumers
        adj = consumers.adjust_pvalues(self.d_p, method, alpha, symmetric=False)
        a = np.array(adj.to_numpy())
        adj.free()
        assert a.dtype == consumers.adjust_out_dtype(method, np.float32, False)
        wide = a.astype(np.float64)
        with np.errstate(invalid="ignore"):
            rows, cols = np.nonzero(wide <= alpha)
        assert cc.condition(len(rows), self.cells), (method, len(rows), self.cells)
        return rows.astype(np.uint32), cols.astype(np.uint32), self.r[rows, cols], self.p[rows, cols], wide[rows, cols]


def full_of(z1, z2, fitres):
    from seekr_amd import _lib
    ctx = z1.ctx
    r = ctx.empty(z1.rows, z2.rows)
    _lib.pearson_gemm_op(ctx, z1, z2, r)
    full = FullPath(r, fitres)
    r.free()
    return full


def assert_same_pairs(got, want, tag):
    rows, cols, r, p, p_adj = want
    assert got.rows.dtype == np.uint32 and got.cols.dtype == np.uint32 and got.r.dtype == np.float32
    assert got.p.dtype == np.float32 and got.p_adj.dtype == np.float64
    assert len(got) == len(rows), (tag, len(got), len(rows))
    assert np.array_equal(got.rows, rows) and np.array_equal(got.cols, cols), tag  # np.nonzero order: row-major
    for name, a, b in (("r", got.r, r), ("p", got.p, p), ("p_adj", got.p_adj, p_adj)):
        assert np.array_equal(bits(a), bits(b)), (tag, name)


def assert_equal_results(a, b, tag):
    for name in FIELDS:
        x, y = getattr(a, name), getattr(b, name)
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), (tag, name)
    assert (a.n_tests, a.r_cutoff, a.n_candidates) == (b.n_tests, b.r_cutoff, b.n_candidates), tag


@functools.lru_cache(maxsize=None)
def two_set_operands():
    from seekr_amd import neighbors
    q, t = cc.two_sets()
    z1, z2 = neighbors._prepare(_ctx(), q, t, False)
    assert z1.kind == z2.kind != 0
    return z1, z2


@functools.lru_cache(maxsize=None)
def planted_operand():
    """significant_cases.planted_counts() prepared as significant_pairs prepares a self-comparison."""
    from seekr_amd import neighbors
    z, _ = neighbors._prepare(_ctx(), sc.planted_counts(), sc.planted_counts(), True)
    assert z.kind != 0
    return z


@functools.lru_cache(maxsize=None)
def two_set_full(background):
    return full_of(*two_set_operands(), sc.backgrounds()[background])


# ---- skr_select_cells_ge --------------------------------------------------------------------------------------------------
SEGMENT_WIDTHS = (1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4099)
CUTOFF = np.float32(0.995)  # keeps 0.25 % of the uniform cells, the special ones aside


def run_select(r, cutoff, nrows, col_begin, col_end, row_global0=0, col_global0=0):
    """select_cells into a fresh list: (rows, cols, vals, count, saw_nan)."""
    from seekr_amd import consumers
    cells = consumers.CellList(r.ctx, 64)
    count, nan = consumers.select_cells(r, cutoff, cells, nrows=nrows, col_begin=col_begin, col_end=col_end,
                                        row_global0=row_global0, col_global0=col_global0)
    assert count == len(cells)
    views = cells.prefix()
    out = tuple(np.array(v.to_numpy()).reshape(-1) for v in views) if views else (np.empty(0, np.uint32), np.empty(0, np.uint32),
                                                                                np.empty(0, np.float32))
    cells.free()
    return out + (count, nan)


def check_select(r, x, cutoff, nrows, col_begin, col_end, row_global0=0, col_global0=0):
    from seekr_amd import consumers
    want = cc.expected_cells(x, cutoff, nrows, col_begin, col_end, row_global0, col_global0)
    tag = (x.shape, float(cutoff), nrows, col_begin, col_end)
    got = run_select(r, cutoff, nrows, col_begin, col_end, row_global0, col_global0)
    assert got[3] == len(want[2]), (tag, got[3], len(want[2]))
    assert got[0].dtype == got[1].dtype == np.uint32 and got[2].dtype == np.float32
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), tag
    assert np.array_equal(bits(got[2]), bits(want[2])), tag  # -0.0 and the NaN payload included
    assert got[4] == bool(np.isnan(want[2]).any()), tag
    count_only = consumers.select_cells(r, cutoff, None, nrows=nrows, col_begin=col_begin, col_end=col_end,
                                        row_global0=row_global0, col_global0=col_global0)
    assert count_only == (got[3], got[4]), tag
    return got[3]


@pytest.mark.parametrize("rows", [1, 2, 3, 5, 257])
def test_select_cells_against_numpy(rows):
    from seekr_amd import _lib
    ctx = _ctx()
    seg = _lib.SELECT_CELLS_SEGMENT
    assert seg == 1024
    kept = total = 0
    for width in sorted(set(SEGMENT_WIDTHS + (seg - 1, seg, seg + 1, 2 * seg - 3, 2 * seg + 1))):
        ld = 4 + width + 3  # wider than col_end on both sides; ld mod 4 changes with the width: every row start alignment
        x = cc.select_block(rows, ld, 11, CUTOFF)
        clean = cc.select_block(rows, ld, 12, CUTOFF, special=0.0)
        r, r_clean = ctx.from_numpy(x), ctx.from_numpy(clean)
        for col_begin in (0, 1, 3, 4):
            col_end = col_begin + width
            offsets = (1000, 77) if col_begin in (1, 4) else (0, 0)
            kept += check_select(r, x, CUTOFF, rows, col_begin, col_end, *offsets)                  # a few cells
            assert check_select(r, x, -np.inf, rows, col_begin, col_end, *offsets) == rows * width  # everything
            assert check_select(r_clean, clean, 2.0, rows, col_begin, col_end, *offsets) == 0       # nothing
            total += rows * width
        if rows > 1:  # fewer rows than the matrix has
            check_select(r, x, CUTOFF, rows - 1, 1, 1 + width)
        r.free()
        r_clean.free()
    print("select_cells, %d rows: %d of %d cells kept at the cutoff" % (rows, kept, total))
    assert 0 < kept < total // 4


@pytest.mark.parametrize("shape", [(3, 70001), (5000, 3)])
def test_select_cells_long_and_tall_blocks(shape):
    ctx = _ctx()
    x = cc.select_block(shape[0], shape[1], 13, CUTOFF, special=0.002)
    r = ctx.from_numpy(x)
    assert check_select(r, x, CUTOFF, shape[0], 0, shape[1], 5, 4000000000 - shape[1]) > 0
    assert check_select(r, x, CUTOFF, shape[0], 1, shape[1] - 1) > 0
    r.free()


def raw_select(ctx, r, cutoff, nrows, col_begin, col_end, outs, out_offset, want_nan=True):
    from seekr_amd import _lib
    count, nan = C.c_int64(-1), C.c_int(-1)
    rc = _lib.lib().skr_select_cells_ge(ctx._h, r._h, nrows, col_begin, col_end, 0, 0, C.c_float(cutoff),
                                        *[None if m is None else m._h for m in outs], out_offset, C.byref(count),
                                        C.byref(nan) if want_nan else None)
    return rc, count.value, nan.value


SENTINEL_U, SENTINEL_F = np.uint32(0xDEADBEEF), np.float32(-12345.5)


def sentinel_outputs(ctx, cap):
    return (ctx.from_numpy(np.full((cap, 1), SENTINEL_U)), ctx.from_numpy(np.full((cap, 1), SENTINEL_U)),
            ctx.from_numpy(np.full((cap, 1), SENTINEL_F)))


def test_select_cells_appends_behind_an_earlier_list():
    ctx = _ctx()
    x = cc.select_block(9, 2100, 14, CUTOFF)
    r = ctx.from_numpy(x)
    first = cc.expected_cells(x, CUTOFF, 4, 0, 2100)
    second = cc.expected_cells(x, CUTOFF, 9, 3, 2051)
    n1, n2, lead = len(first[2]), len(second[2]), 5
    assert n1 > 0 and n2 > 0
    outs = sentinel_outputs(ctx, lead + n1 + n2 + 7)
    assert raw_select(ctx, r, CUTOFF, 4, 0, 2100, outs, lead) == (0, n1, 1)
    assert raw_select(ctx, r, CUTOFF, 9, 3, 2051, outs, lead + n1, want_nan=False) == (0, n2, -1)
    for k, (m, sentinel) in enumerate(zip(outs, (SENTINEL_U, SENTINEL_U, SENTINEL_F))):
        got = np.array(m.to_numpy()).reshape(-1)
        assert (got[:lead] == sentinel).all() and (got[lead + n1 + n2:] == sentinel).all()
        assert np.array_equal(bits(got[lead:lead + n1]), bits(first[k])) and np.array_equal(bits(got[lead + n1:lead + n1 + n2]), bits(second[k]))
    # capacity one too small: the count comes back, nothing is written; and the same run twice gives the same bytes
    small = sentinel_outputs(ctx, lead + n1 - 1)
    assert raw_select(ctx, r, CUTOFF, 4, 0, 2100, small, lead) == (0, n1, 1)
    assert raw_select(ctx, r, CUTOFF, 4, 0, 2100, small, lead + n1) == (0, n1, 1)  # an offset beyond the outputs
    for m, sentinel in zip(small, (SENTINEL_U, SENTINEL_U, SENTINEL_F)):
        assert (np.array(m.to_numpy()) == sentinel).all()
    exact = sentinel_outputs(ctx, lead + n1)
    assert raw_select(ctx, r, CUTOFF, 4, 0, 2100, exact, lead) == (0, n1, 1)
    assert np.array_equal(bits(np.array(exact[2].to_numpy()).reshape(-1)[lead:]), bits(first[2]))
    assert raw_select(ctx, r, CUTOFF, 4, 0, 2100, (None, None, None), 0) == (0, n1, 1)  # count only
    assert raw_select(ctx, r, CUTOFF, 0, 0, 2100, outs, 0) == (0, 0, 0) and raw_select(ctx, r, CUTOFF, 4, 7, 7, outs, 0) == (0, 0, 0)
    for m in outs + small + exact + (r,):
        m.free()


def test_cell_list_grows_and_keeps_its_cells():
    from seekr_amd import consumers
    ctx = _ctx()
    x = cc.select_block(40, 1500, 15, CUTOFF)
    r = ctx.from_numpy(x)
    cells = consumers.CellList(ctx, 8)
    want = [[], [], []]
    for row0 in range(0, 40, 8):  # five appends into a list that starts with room for 8 cells
        view = r.view(row0, 8)
        count, _ = consumers.select_cells(view, CUTOFF, cells, row_global0=row0)
        part = cc.expected_cells(x[row0:row0 + 8], CUTOFF, 8, 0, 1500, row0, 0)
        assert count == len(part[2])
        for acc, p in zip(want, part):
            acc.append(p)
    assert len(cells) == sum(len(p) for p in want[2]) > 64 and cells.capacity >= len(cells)
    for view, parts in zip(cells.prefix(), want):
        assert view.shape == (len(cells), 1)
        assert np.array_equal(bits(np.array(view.to_numpy()).reshape(-1)), bits(np.concatenate(parts)))
    cells.free()
    r.free()


def test_vec_copy_round_trip_and_refusals():
    from seekr_amd import _lib, consumers
    ctx = _ctx()
    rng = np.random.default_rng(16)
    for dtype in (np.uint32, np.float32, np.float64):
        src = (rng.random(1000) * 1e6).astype(dtype)
        d_src, d_dst = ctx.from_numpy(src), ctx.from_numpy(np.zeros((50, 30), dtype))
        consumers.vec_copy(d_src, 17, d_dst, 101, 883)
        consumers.vec_copy(d_src, 0, d_dst, 0, 0)
        back = np.array(d_dst.to_numpy()).reshape(-1)
        assert np.array_equal(bits(back[101:984]), bits(src[17:900])) and not back[:101].any() and not back[984:].any()
        consumers.vec_copy(d_dst, 101, d_src, 0, 883)  # and back
        assert np.array_equal(bits(np.array(d_src.to_numpy()).reshape(-1)[:883]), bits(src[17:900]))
        for args in ((0, 0, 1001), (1, 0, 1000), (-1, 0, 5), (0, -1, 5), (0, 0, -1), (0, 1400, 101), (0, 1501, 0), (1001, 0, 0)):
            with pytest.raises(ValueError):
                consumers.vec_copy(d_src, args[0], d_dst, args[1], args[2])
        with pytest.raises(ValueError, match="overlap"):
            consumers.vec_copy(d_src, 0, d_src, 10, 20)
        consumers.vec_copy(d_src, 0, d_src, 20, 20)  # one allocation, ranges apart
        other = ctx.from_numpy(np.zeros(10, np.float64 if dtype != np.float64 else np.float32))
        with pytest.raises(ValueError, match="dtype"):
            consumers.vec_copy(d_src, 0, other, 0, 5)
        foreign = _lib.Context(_lib.default_device())
        with pytest.raises(ValueError, match="foreign"):
            _lib.check(_lib.lib().skr_vec_copy(foreign._h, d_src._h, 0, d_dst._h, 0, 5))
        foreign.close()
        for m in (d_src, d_dst, other):
            m.free()


def test_select_cells_refusals():
    from seekr_amd import _lib
    ctx = _ctx()
    r = ctx.from_numpy(np.zeros((6, 40), np.float32))
    u32 = lambda: ctx.empty(100, 1, np.uint32)  # noqa: E731
    f32 = lambda: ctx.empty(100, 1, np.float32)  # noqa: E731
    good = (u32(), u32(), f32())
    lib = _lib.lib()

    def call(mat=r, nrows=6, col_begin=0, col_end=40, row_global0=0, col_global0=0, outs=good, out_offset=0, c=ctx):
        count = C.c_int64(0)
        return lib.skr_select_cells_ge(c._h, mat._h, nrows, col_begin, col_end, row_global0, col_global0, C.c_float(0.5),
                                       *[None if m is None else m._h for m in outs], out_offset, C.byref(count), None)

    assert call() == 0
    invalid = -1
    r64, ru = ctx.empty(6, 40, np.float64), ctx.empty(6, 40, np.uint32)
    assert call(mat=r64) == invalid and call(mat=ru) == invalid
    assert call(outs=(f32(), good[1], good[2])) == invalid and call(outs=(good[0], f32(), good[2])) == invalid
    assert call(outs=(good[0], good[1], u32())) == invalid
    for outs in ((good[0], None, None), (None, good[1], good[2]), (good[0], good[1], None)):
        assert call(outs=outs) == invalid
    assert call(nrows=7) == invalid and call(nrows=-1) == invalid
    assert call(col_end=41) == invalid and call(col_begin=-1) == invalid and call(col_begin=30, col_end=20) == invalid
    assert call(row_global0=0xffffffff - 5) == invalid and call(col_global0=0xffffffff - 39) == invalid
    assert call(row_global0=0xffffffff - 6) == 0 and call(col_global0=0xffffffff - 40) == 0
    assert call(row_global0=-1) == invalid and call(col_global0=-1) == invalid and call(out_offset=-1) == invalid
    foreign = _lib.Context(_lib.default_device())
    assert call(c=foreign) == invalid
    other = foreign.empty(100, 1, np.uint32)
    assert call(outs=(other, good[1], good[2])) == invalid
    other.free()
    foreign.close()
    with pytest.raises(ValueError):
        _lib.check(call(nrows=7))


# ---- two sets against the full-matrix path ----------------------------------------------------------------------------------
SPLITS = [(s, p) for s in (8192, 16, 7) for p in (None, 100, 64)]


@pytest.mark.parametrize("background", ["norm", "gamma", "empirical_f32", "empirical_f64"])
def test_two_sets_against_the_full_matrix_path(background):
    from seekr_amd import significant as sg
    (z1, z2), full, fitres = two_set_operands(), two_set_full(background), sc.backgrounds()[background]
    n_tests = 37 * 263
    found = {}
    for m, method in enumerate(sc.HEAD_METHODS):
        want = full.expected(method)
        found[method] = len(want[0])
        # every split for fdr_bh and for one more method per background; the others at the default and at one odd split
        every = method == "fdr_bh" or m == list(sc.backgrounds()).index(background)
        first = None
        for stripe_rows, panel_rows in (SPLITS if every else (SPLITS[0], SPLITS[8])):
            got = sg.pearson_significant(z1, fitres, method=method, alpha=ALPHA, other=z2, stripe_rows=stripe_rows,
                                         panel_rows=panel_rows)
            assert_same_pairs(got, want, (background, method, stripe_rows, panel_rows))
            assert got.n_tests == n_tests and len(got) <= got.n_candidates < n_tests // 2 and got.r_cutoff > 0
            assert got.n_candidates >= int((full.p <= sc.alpha32(ALPHA)).sum())  # every cell with p <= alpha32 is a candidate
            first = first or got
            assert_equal_results(got, first, (background, method, stripe_rows, panel_rows))
    print("significant cells of %d, %s: %s" % (n_tests, background, found))
    assert found["fdr_bh"] > found["bonferroni"]


def test_two_sets_from_host_counts_and_alpha():
    from seekr_amd import significant as sg
    q, t = cc.two_sets()
    fitres = sc.backgrounds()["norm"]
    timings = {}
    got = sg.significant_pairs(q, fitres, counts2=t, timings=timings)
    assert_same_pairs(got, two_set_full("norm").expected("fdr_bh"), "host counts")
    assert timings["bytes_to_device"] == 0 and timings["bytes_to_host"] == len(got) * 24
    assert {"cutoff_search", "edge_list", "p_values", "selection", "correction"} <= set(timings)
    got = sg.significant_pairs(q.astype(np.float64), fitres, method="holm", alpha=0.01, counts2=[list(row) for row in t])
    assert_same_pairs(got, two_set_full("norm").expected("holm", 0.01), "float64 counts, alpha 0.01")


def test_one_set_calls_are_todays_call():
    from seekr_amd import significant as sg
    x = sc.planted_counts()
    fitres = sc.backgrounds()["empirical_f32"]
    today = sg.significant_pairs(x, fitres)
    assert len(today) >= 100 and today.n_tests == 300 * 299 // 2 and (today.rows < today.cols).all()
    assert_equal_results(sg.significant_pairs(x, fitres, counts2=None), today, "counts2=None")
    assert_equal_results(sg.significant_pairs(x, fitres, counts2=x), today, "counts2 is counts")
    two = sg.significant_pairs(x, fitres, counts2=x.copy())  # another object: 90 000 tests, the diagonal among them
    assert two.n_tests == 300 * 300 and (two.rows == two.cols).sum() == 300


def test_square_two_sets_keep_their_diagonal():
    from seekr_amd import neighbors
    from seekr_amd import significant as sg
    q2, t2 = cc.square_sets()
    fitres = sc.backgrounds()["norm"]
    z1, z2 = neighbors._prepare(_ctx(), q2, t2, False)
    for method in ("bonferroni", "fdr_bh"):
        want = full_of(z1, z2, fitres).expected(method)
        got = sg.pearson_significant(z1, fitres, method=method, other=z2)
        assert_same_pairs(got, want, ("square", method))
        assert got.n_tests == 37 * 37
        cells = set(zip(got.rows.tolist(), got.cols.tolist()))
        assert all((i, i) in cells for i in range(37)) and len(cells) < 37 * 37 // 2
    host = sg.significant_pairs(q2, fitres, counts2=t2)
    assert_same_pairs(host, want, "square, host counts")
    z1.free()
    z2.free()


def test_a_side_in_float32_layout():
    from seekr_amd import neighbors
    from seekr_amd import significant as sg
    rng = np.random.default_rng(33)
    t = rng.standard_normal((64, 1024))
    for g in range(3):
        t[g * 12:(g + 1) * 12] += 0.6 * rng.standard_normal(1024)
    t = t.astype(np.float32)
    q = (t[:20] + 0.5 * rng.standard_normal((20, 1024))).astype(np.float32)
    t[3] *= np.float32(0.01)
    t[3, 17] = 50.0  # one column carries the row: the fill routes this side, and with it the other, to the float32 layout
    z1, z2 = neighbors._prepare(_ctx(), q, t, False)
    assert z1.kind == 0 and z2.kind == 0
    fitres = [("norm", 0.0, (0.0, 1.0 / 32.0))]
    full = full_of(z1, z2, fitres)
    for method in ("simes-hochberg", "sidak"):
        want = full.expected(method)
        for stripe_rows, panel_rows in ((8192, None), (7, 30)):
            got = sg.pearson_significant(z1, fitres, method=method, other=z2, stripe_rows=stripe_rows, panel_rows=panel_rows)
            assert_same_pairs(got, want, ("float32 layout", method, stripe_rows, panel_rows))
    assert_same_pairs(sg.significant_pairs(q, fitres, method="sidak", counts2=t), want, "float32 layout, host counts")
    z1.free()
    z2.free()


def assert_empty(res, n_tests, r_cutoff_is_none=False):
    assert len(res) == 0 and res.n_tests == n_tests
    assert [getattr(res, f).dtype for f in FIELDS] == [np.uint32, np.uint32, np.float32, np.float32, np.float64]
    if r_cutoff_is_none:
        assert res.r_cutoff is None and res.n_candidates == 0


def test_two_set_errors_and_empty_results():
    from seekr_amd import significant as sg
    q, t = cc.two_sets()
    fitres = sc.backgrounds()["norm"]
    flat = np.array(t)
    flat[5] = 3.0
    with pytest.raises(ValueError, match="NaN"):
        sg.significant_pairs(q, fitres, counts2=flat)
    assert_empty(sg.significant_pairs(q, [("uniform", 0.0, (0.0, 5.0))], counts2=t), 37 * 263, True)  # p(2) = 0.6: no crossing
    noise = np.random.default_rng(34).standard_normal((50, 256)).astype(np.float32)  # no r near bonferroni's bar at 1e-9
    assert_empty(sg.significant_pairs(q, fitres, method="bonferroni", alpha=1e-9, counts2=noise), 37 * 50)
    assert_empty(sg.significant_pairs(q[:0], fitres, counts2=t), 0, True)
    assert_empty(sg.significant_pairs(q, fitres, counts2=t[:0]), 0, True)
    with pytest.raises(ValueError, match="not positive"):
        sg.significant_pairs(q, [("norm", 0.0, (-1.0, sc.SD))], counts2=t)
    with pytest.raises(ValueError, match="columns"):
        sg.significant_pairs(q, fitres, counts2=t[:, :100])


# ---- the candidate list of the self-comparison, kept on the device -----------------------------------------------------------
@pytest.mark.parametrize("background", ["empirical_f32", "gamma"])
def test_device_candidates_equal_host_candidates(background):
    from seekr_amd import significant as sg
    z, fitres = planted_operand(), sc.backgrounds()[background]
    for method in ("fdr_bh", "holm"):
        for stripe_rows, fuse in ((8192, "auto"), (64, True), (64, False)):  # the fused buffers and skr_edges' outputs
            t_host, t_dev = {}, {}
            host = sg.pearson_significant(z, fitres, method=method, stripe_rows=stripe_rows, fuse=fuse, timings=t_host)
            dev = sg.pearson_significant(z, fitres, method=method, stripe_rows=stripe_rows, fuse=fuse, timings=t_dev,
                                         candidates="device")
            assert len(host) >= 1
            assert_equal_results(dev, host, (background, method, stripe_rows, fuse))
            assert t_host["bytes_to_device"] == 12 * host.n_candidates and t_dev["bytes_to_device"] == 0
    x = sc.planted_counts()
    assert_equal_results(sg.significant_pairs(x, fitres, candidates="device"), sg.significant_pairs(x, fitres), background)
    flat = np.array(x)
    flat[7] = 1.0
    with pytest.raises(ValueError, match="NaN"):
        sg.significant_pairs(flat, fitres, candidates="device")


# ---- domain_significant ------------------------------------------------------------------------------------------------------
K, WINDOW, SLIDE = 4, 500, 50


@pytest.fixture(scope="module")
def domain_files(tmp_path_factory):
    """The FASTA files and norm vectors of the domain case in a directory of their own, and the two backgrounds."""
    from seekr_amd.kmer_counts import BasicCounter
    from seekr_amd.windows import domain_pearson
    d = str(tmp_path_factory.mktemp("cross_significant"))
    seqs = cc.domain_sequences()
    paths = {}
    for name in ("query", "target", "unrelated", "background"):
        paths[name] = os.path.join(d, name + ".fa")
        with open(paths[name], "w") as f:
            f.write(seqs[name])
    with open(os.path.join(d, "short.fa"), "w") as f:
        f.write(seqs["target"] + ">short\nAC\n")
    paths["short"] = os.path.join(d, "short.fa")
    counter = BasicCounter(paths["background"], k=K, silent=True)
    counter.get_counts()
    paths["mean"], paths["std"] = os.path.join(d, "mean.npy"), os.path.join(d, "std.npy")
    np.save(paths["mean"], counter.mean)
    np.save(paths["std"], counter.std)
    backgrounds = {}
    for log2 in ("Log2.post", "Log2.none"):
        bg, _ = domain_pearson(paths["query"], paths["unrelated"], K, WINDOW, SLIDE, paths["mean"], paths["std"], log2=log2)
        assert bg.dtype == np.float32 and bg.shape == (3, 171 + 91)
        flat = np.array(bg).reshape(-1)
        backgrounds[log2] = {"empirical": flat, "norm": [("norm", 0.0, (float(flat.mean(dtype=np.float64)),
                                                                       float(flat.std(dtype=np.float64))))]}
    return paths, backgrounds


@pytest.mark.parametrize("kind", ["empirical", "norm"])
@pytest.mark.parametrize("log2", ["Log2.post", "Log2.none"])
def test_domain_significant_against_the_full_path(domain_files, log2, kind):
    from seekr_amd.windows import domain_pearson, domain_significant
    paths, backgrounds = domain_files
    fitres = backgrounds[log2][kind]
    args = (paths["query"], paths["target"], K, WINDOW, SLIDE, paths["mean"], paths["std"])
    r, table = domain_pearson(*args, log2=log2)
    assert r.shape == (3, 111 + 73)
    r_dev = _ctx().from_numpy(r)
    full = FullPath(r_dev, fitres)
    r_dev.free()
    for method in ("fdr_bh", "holm") if kind == "norm" else ("fdr_bh",):
        rows, cols, want_r, want_p, want_adj = full.expected(method)
        print("domain_significant %s %s %s: %d of %d cells" % (log2, kind, method, len(rows), r.size))
        first = None
        for chunk_rows in (64, 50, 100000):
            got = domain_significant(*args, fitres, method=method, log2=log2, chunk_rows=chunk_rows)
            assert list(got.columns) == ["query", "header", "start", "end", "r", "p", "p_adj"]
            assert np.array_equal(got["query"].to_numpy(), rows) and got["query"].dtype == np.int64
            for column in ("header", "start", "end"):
                assert list(got[column]) == list(table[column].to_numpy()[cols]), (chunk_rows, column)
            assert got["r"].dtype == np.float32 and got["p"].dtype == np.float32 and got["p_adj"].dtype == np.float64
            assert np.array_equal(bits(got["r"].to_numpy()), bits(want_r)) and np.array_equal(bits(got["p"].to_numpy()), bits(want_p))
            assert np.array_equal(bits(got["p_adj"].to_numpy()), bits(want_adj))
            assert got.attrs["n_tests"] == r.size and got.attrs["r_cutoff"] > 0
            assert len(got) <= got.attrs["n_candidates"] < r.size // 2
            first = got if first is None else first
            assert got.attrs == first.attrs
        # every query is found where it was embedded: the windows that lie inside its copy
        for qi, ti, off in cc.domain_sequences()["embedded"]:
            hit = first[(first["query"] == qi) & first["header"].map(lambda h: str(h).endswith("target%d" % ti))]
            assert ((hit["start"] >= off) & (hit["end"] <= off + 600)).any(), (qi, ti, off)


def test_domain_significant_nan_window_and_empty_inputs(domain_files, capsys):
    from seekr_amd.kmer_counts import NAN_WARNING
    from seekr_amd.windows import domain_pearson, domain_significant
    paths, _ = domain_files
    mean, std = np.zeros(4 ** K, np.float32), np.ones(4 ** K, np.float32)
    fitres = [("norm", 0.0, (0.0, 0.07))]
    capsys.readouterr()
    r, table = domain_pearson(paths["query"], paths["short"], K, WINDOW, SLIDE, mean, std, log2="Log2.none")
    assert capsys.readouterr().out.count(NAN_WARNING) == 1 and np.isnan(r[:, 184]).all() and not np.isnan(r[:, :184]).any()
    for chunk_rows in (64, 100000):
        with pytest.raises(ValueError, match=r"window 184 \(>?short:0-2"):
            domain_significant(paths["query"], paths["short"], K, WINDOW, SLIDE, mean, std, fitres, log2="Log2.none",
                               chunk_rows=chunk_rows)
        assert capsys.readouterr().out.count(NAN_WARNING) == 1
    # no query: an empty frame with the columns; a background that never reaches alpha: no cutoff
    none = domain_significant(np.empty((0, 4 ** K), np.float32), paths["target"], K, WINDOW, SLIDE, mean, std, fitres)
    assert list(none.columns) == ["query", "header", "start", "end", "r", "p", "p_adj"] and len(none) == 0
    assert none.attrs == {"n_tests": 0, "r_cutoff": None, "n_candidates": 0}
    flat = domain_significant(paths["query"], paths["target"], K, WINDOW, SLIDE, paths["mean"], paths["std"],
                              [("uniform", 0.0, (0.0, 5.0))])
    assert len(flat) == 0 and flat.attrs == {"n_tests": 3 * 184, "r_cutoff": None, "n_candidates": 0}


# ---- the commands ---------------------------------------------------------------------------------------------------------
def run_command(function, argv):
    code = "import sys; sys.argv = %r; from seekr_amd.console_scripts import %s; %s()" % (argv, function, function)
    proc = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0, proc.stderr
    return proc


def test_commands_file_to_file(domain_files, tmp_path):
    from seekr_amd import _lib
    from seekr_amd import significant as sg
    from seekr_amd.windows import domain_significant
    q, t = cc.two_sets()
    names1, names2 = ["query|%d" % i for i in range(len(q))], ["target|%d" % i for i in range(len(t))]
    kmers = ["k%d" % j for j in range(q.shape[1])]
    _lib.save_csv_labelled(str(tmp_path / "q.csv"), q, names1, kmers)
    _lib.save_csv_labelled(str(tmp_path / "t.csv"), t, names2, kmers)
    np.save(tmp_path / "bg.npy", sc.backgrounds()["empirical_f64"])
    out = tmp_path / "pairs.csv"
    run_command("console_significant_pairs", ["seekr_significant_pairs", str(tmp_path / "q.csv"), str(tmp_path / "t.csv"), "-bg",
                                              str(tmp_path / "bg.npy"), "-o", str(out)])
    from seekr_amd.console_scripts import _read_labelled_csv
    want = sg.significant_pairs(_read_labelled_csv(str(tmp_path / "q.csv"))[0], sc.backgrounds()["empirical_f64"],
                                counts2=_read_labelled_csv(str(tmp_path / "t.csv"))[0])
    lines = out.read_text().split("\n")
    assert lines[0] == "row,col,r,p,p_adj" and lines[-1] == "" and len(lines) == len(want) + 2 and len(want) >= 48
    for line, i, j, r, p, a in zip(lines[1:], want.rows, want.cols, want.r, want.p, want.p_adj):
        assert line == "%s,%s,%s,%s,%r" % (names1[i], names2[j], str(r), str(p), float(a))
    np.save(tmp_path / "q.npy", q)
    np.save(tmp_path / "t.npy", t)
    run_command("console_significant_pairs", ["seekr_significant_pairs", str(tmp_path / "q.npy"), str(tmp_path / "t.npy"), "-bi", "-d",
                                              "norm", "-p", "0.0", "0.0625", "-m", "holm", "-a", "0.01", "-o", str(out)])
    want = sg.significant_pairs(q, [("norm", 0.0, (0.0, 0.0625))], method="holm", alpha=0.01, counts2=t)
    lines = out.read_text().split("\n")
    assert len(lines) == len(want) + 2 and len(want) >= 48
    for line, i, j, r, p, a in zip(lines[1:], want.rows, want.cols, want.r, want.p, want.p_adj):
        assert line == "%d,%d,%s,%s,%r" % (i, j, str(r), str(p), float(a))
    # seekr_domain_significant
    paths, backgrounds = domain_files
    np.save(tmp_path / "dbg.npy", backgrounds["Log2.post"]["empirical"])
    dout = tmp_path / "domains.csv"
    run_command("console_domain_significant", ["seekr_domain_significant", paths["query"], paths["target"], paths["mean"], paths["std"],
                                               "-k", str(K), "-w", str(WINDOW), "-s", str(SLIDE), "-bg", str(tmp_path / "dbg.npy"),
                                               "-o", str(dout)])
    frame = domain_significant(paths["query"], paths["target"], K, WINDOW, SLIDE, paths["mean"], paths["std"],
                               backgrounds["Log2.post"]["empirical"])
    lines = dout.read_text().split("\n")
    assert lines[0] == "query,header,start,end,r,p,p_adj" and len(lines) == len(frame) + 2 and len(frame) >= 1
    for line, (_, row) in zip(lines[1:], frame.iterrows()):
        assert line == "%d,%s,%d,%d,%s,%s,%r" % (row["query"], row["header"], row["start"], row["end"], str(np.float32(row["r"])),
                                                 str(np.float32(row["p"])), float(row["p_adj"]))
