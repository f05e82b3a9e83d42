"""significant.pearson_significant / significant_pairs, consumers.adjust_pvalues_head, consumers.select_le and the
seekr_significant_pairs command on the device.  The expected pairs come from the package's own full-matrix path on the
same operand — pearson_gemm_op -> parametric_pvalues / empirical_pvalues -> adjust_pvalues(symmetric=True), each step
pinned against scipy and statsmodels goldens elsewhere — and are compared bit for bit."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import significant_cases as sc
from test_adj_pval_cpu import assert_matches

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALPHA = 0.05


def _ctx():
    from seekr_amd import _lib
    return _lib.default_context()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def prepared(ctx, x):
    from seekr_amd import _lib
    from seekr_amd import pearson as pearson_mod
    return _lib.operand_fill(ctx, ctx.from_numpy(x), None, pearson_mod._precision_for(np.dtype(np.float32), True))[0]


def device_p(ctx, r, fitres):
    from seekr_amd import consumers
    if isinstance(fitres, np.ndarray):
        return consumers.empirical_pvalues(r, fitres)
    name, _, params = fitres[0]
    return consumers.parametric_pvalues(r, name, params)


class FullPath:
    """r and p of the whole matrix for one operand and one background — once, left unchanged — and the corrected matrix
    per method."""

    def __init__(self, ctx, z, fitres):
        from seekr_amd import _lib
        self.ctx, self.n = ctx, z.rows
        r = ctx.empty(z.rows, z.rows)
        _lib.pearson_gemm_op(ctx, z, z, r)
        self.d_p = device_p(ctx, r, fitres)
        self.r, self.p = np.array(r.to_numpy()), np.array(self.d_p.to_numpy())
        r.free()

    def expected(self, method, alpha=ALPHA):
        from seekr_amd import consumers
        adj = consumers.adjust_pvalues(self.d_p, method, alpha, symmetric=True)
        a = np.array(adj.to_numpy())
        adj.free()
        assert a.dtype == np.float64
        with np.errstate(invalid="ignore"):
            rows, cols = np.nonzero(a <= alpha)
        return rows.astype(np.uint32), cols.astype(np.uint32), self.r[rows, cols], self.p[rows, cols], a[rows, cols]


def assert_same_pairs(got, want, tag):
    rows, cols, r, p, p_adj = want
    assert got.rows.dtype == np.uint32 and got.cols.dtype == np.uint32 and got.r.dtype == np.float32
    assert got.p.dtype == np.float32 and got.p_adj.dtype == np.float64
    assert len(got) == len(rows), (tag, len(got), len(rows))
    assert np.array_equal(got.rows, rows) and np.array_equal(got.cols, cols), tag  # np.nonzero order: row-major
    assert (got.rows < got.cols).all()
    for name, a, b in (("r", got.r, r), ("p", got.p, p), ("p_adj", got.p_adj, p_adj)):
        assert np.array_equal(bits(a), bits(b)), (tag, name)


@functools.lru_cache(maxsize=None)
def planted():
    ctx = _ctx()
    z = prepared(ctx, sc.planted_counts())
    assert z.kind != 0
    return z


@functools.lru_cache(maxsize=None)
def planted_full(background):
    return FullPath(_ctx(), planted(), sc.backgrounds()[background])


# ---- parity with the full path --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("background", ["norm", "gamma", "empirical_f32", "empirical_f64"])
def test_parity_with_the_full_matrix_path(background):
    from seekr_amd import significant as sg
    z, full, fitres = planted(), planted_full(background), sc.backgrounds()[background]
    n_tests = 300 * 299 // 2
    found = {}
    for method in sc.HEAD_METHODS:
        want = full.expected(method)
        found[method] = len(want[0])
        for stripe_rows in (64, 300):
            for fuse in (True, False):
                got = sg.pearson_significant(z, fitres, method=method, alpha=ALPHA, stripe_rows=stripe_rows, fuse=fuse)
                assert_same_pairs(got, want, (background, method, stripe_rows, fuse))
                assert got.n_tests == n_tests and len(got) <= got.n_candidates < n_tests // 2 and got.r_cutoff > 0
                # every cell of the matrix with p <= alpha32 is a candidate
                assert got.n_candidates >= int((full.p[np.triu_indices(300, 1)] <= sc.alpha32(ALPHA)).sum())
    print("significant pairs of %d, %s: %s" % (n_tests, background, found))
    assert found["fdr_bh"] >= 100 and found["bonferroni"] >= 1 and found["fdr_bh"] > found["bonferroni"]


def test_default_arguments_and_a_second_call():
    from seekr_amd import significant as sg
    z, fitres = planted(), sc.backgrounds()["norm"]
    want = planted_full("norm").expected("fdr_bh")
    one = sg.pearson_significant(z, fitres)
    two = sg.pearson_significant(z, fitres)
    assert_same_pairs(one, want, "defaults")
    for name in ("rows", "cols", "r", "p", "p_adj"):
        assert getattr(one, name).tobytes() == getattr(two, name).tobytes(), name
    assert (one.n_tests, one.r_cutoff, one.n_candidates) == (two.n_tests, two.r_cutoff, two.n_candidates)
    host = sg.significant_pairs(sc.planted_counts(), fitres)  # the host level prepares the same operand
    assert_same_pairs(host, want, "significant_pairs")
    assert_same_pairs(sg.significant_pairs(sc.planted_counts().astype(np.float64), fitres, alpha=0.01, method="holm"),
                      planted_full("norm").expected("holm", 0.01), "float64 counts, alpha 0.01")


# ---- further layouts ----------------------------------------------------------------------------------------------------
def grouped_rows(n_rows, n_cols, seed, group=12, strength=0.5):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n_rows, n_cols))
    for g in range(3):
        x[g * group:(g + 1) * group] += strength * rng.standard_normal(n_cols)
    return x.astype(np.float32)


def test_rows_of_8192_columns_take_the_scratch_block():
    import ctypes as C
    from seekr_amd import _lib
    from seekr_amd import significant as sg
    ctx = _ctx()
    z = prepared(ctx, grouped_rows(130, 8192, 31))
    needs = C.c_int(0)
    _lib.check(_lib.lib().skr_pearson_gemm_edges_needs_scratch(ctx._h, z._h, z._h, C.byref(needs)))
    assert z.kind != 0 and needs.value == 1  # the path under test
    fitres = [("norm", 0.0, (0.0, 1.0 / np.sqrt(8192.0)))]
    want = FullPath(ctx, z, fitres).expected("fdr_by")
    assert len(want[0]) >= 100
    for stripe_rows in (50, 130):
        got = sg.pearson_significant(z, fitres, method="fdr_by", stripe_rows=stripe_rows, fuse=True)
        assert_same_pairs(got, want, ("8192 columns", stripe_rows))
    z.free()


def test_float32_layout_takes_the_two_step_path():
    from seekr_amd import significant as sg
    ctx = _ctx()
    x = grouped_rows(64, 1024, 32, strength=0.6)
    x[3] *= np.float32(0.01)
    x[3, 17] = 50.0  # one column carries the row: the fill routes the operand to the float32 layout
    z = prepared(ctx, x)
    assert z.kind == 0
    fitres = [("norm", 0.0, (0.0, 1.0 / 32.0))]
    want = FullPath(ctx, z, fitres).expected("simes-hochberg")
    assert len(want[0]) >= 50
    for stripe_rows in (20, 64):
        got = sg.pearson_significant(z, fitres, method="simes-hochberg", stripe_rows=stripe_rows)
        assert_same_pairs(got, want, ("float32 layout", stripe_rows))
    z.free()


# ---- adjust_pvalues_head alone --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("given", [1, 255, 4096, 4097, 70000])
def test_adjust_pvalues_head_against_the_prefix_formulas(given):
    from seekr_amd import consumers
    ctx = _ctx()
    for dtype in (np.float32, np.float64):
        rng = np.random.default_rng([41, given, np.dtype(dtype).itemsize])
        p = sc.tied_pvalues(rng, given, dtype)
        d = ctx.from_numpy(p)
        for ntests in (given, given + 1, 10 * given, 1249975000):
            for method in sc.HEAD_METHODS:
                if method == "fdr_by" and ntests > 5_000_000:  # numpy's harmonic sum is the expected value: kept small
                    continue
                out = consumers.adjust_pvalues_head(d, ntests, method, ALPHA)
                got = np.array(out.to_numpy()).reshape(-1)
                out.free()
                with np.errstate(all="ignore"):
                    want = sc.head_correct(p, ntests, method).astype(np.float64)
                try:
                    assert_matches(got, want, method, dtype)
                except AssertionError:
                    differ = np.flatnonzero(bits(got) != bits(want))
                    raise AssertionError("%s E=%d ntests=%d %s: %d cells differ, first %d: %r want %r" % (
                        method, given, ntests, np.dtype(dtype).name, len(differ), differ[0], got[differ[0]], want[differ[0]]))
        d.free()


def test_adjust_pvalues_head_whole_list_is_adjust_pvalues():
    """ntests = E: the bytes skr_adjust_pvalues gives the same tests as the upper triangle of a symmetric matrix."""
    from seekr_amd import consumers
    ctx = _ctx()
    rng = np.random.default_rng(42)
    n = 91
    iu = np.triu_indices(n, 1)
    for dtype in (np.float32, np.float64):
        a = np.zeros((n, n), dtype)
        a[iu] = sc.tied_pvalues(rng, len(iu[0]), dtype)
        a = a + a.T
        d_full, d_vec = ctx.from_numpy(a), ctx.from_numpy(a[iu])
        for method in sc.HEAD_METHODS:
            whole = consumers.adjust_pvalues(d_full, method, ALPHA, symmetric=True)
            head = consumers.adjust_pvalues_head(d_vec, len(iu[0]), method, ALPHA)
            assert np.array_equal(bits(np.array(whole.to_numpy())[iu]), bits(np.array(head.to_numpy()).reshape(-1))), method
            whole.free()
            head.free()
        d_full.free()
        d_vec.free()


def test_adjust_pvalues_head_refusals():
    import ctypes as C
    from seekr_amd import _lib, consumers
    ctx = _ctx()
    d = ctx.from_numpy(np.array([0.01, 0.02, 0.03], np.float32))
    for method in sc.REFUSED:
        with pytest.raises(NotImplementedError, match=method):
            consumers.adjust_pvalues_head(d, 10, method)
        out = ctx.empty(1, 3, np.float64)
        rc = _lib.lib().skr_adjust_pvalues_head(ctx._h, d._h, 10, consumers.ADJ_METHODS[method], C.c_double(ALPHA), out._h)
        assert rc == -4 and method in _lib.lib().skr_last_error().decode()  # SKR_ERR_UNSUPPORTED names the method
        out.free()
    with pytest.raises(ValueError, match="smaller"):
        consumers.adjust_pvalues_head(d, 2, "holm")
    empty = ctx.empty(1, 0, np.float32)
    with pytest.raises(ZeroDivisionError):
        consumers.adjust_pvalues_head(empty, 0, "holm")
    none = consumers.adjust_pvalues_head(empty, 5, "holm")
    assert (none.rows, none.cols, none.dtype) == (1, 0, np.float64)


# ---- select_le ------------------------------------------------------------------------------------------------------------
def selected(ctx, values, bound):
    from seekr_amd import consumers
    d = ctx.from_numpy(values)
    index, count = consumers.select_le(d, bound)
    got = np.empty(0, np.uint32) if index is None else np.array(index.to_numpy()).reshape(-1)
    assert len(got) == count and got.dtype == np.uint32
    picked = None
    if index is not None:
        g = consumers.gather_index(d, index, count)
        picked = np.array(g.to_numpy()).reshape(-1)
        g.free()
        index.free()
    d.free()
    return got, picked


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_select_le(dtype):
    ctx = _ctx()
    rng = np.random.default_rng(43)
    for n in (1, 63, 256, 257, 5000, 1_500_000):  # 1 500 000: more tiles than workgroups, a two-level scan of the counts
        v = rng.random(n).astype(dtype)
        v[rng.integers(0, n, max(1, n // 50))] = dtype(0.05)  # the bound is a present value, many times
        if n >= 63:
            v[[1, 7, 60]] = (np.nan, np.inf, -np.inf)
            v[[2, 11]] = (np.nextafter(np.float32(0.05), np.float32(1)), np.nextafter(np.float32(0.05), np.float32(0)))
        for bound in (0.05, float(np.float32(0.05)), float(np.nextafter(np.float32(0.05), np.float32(1))),
                      float(np.nextafter(np.float32(0.05), np.float32(0))), -np.inf, np.inf, 2.0, -1.0):
            with np.errstate(invalid="ignore"):
                want = np.flatnonzero(v.astype(np.float64) <= bound).astype(np.uint32)
            got, picked = selected(ctx, v, bound)
            assert np.array_equal(got, want), (n, bound, len(got), len(want))
            if picked is not None:
                assert np.array_equal(bits(picked), bits(v[want])), (n, bound)
    from seekr_amd import consumers
    assert consumers.select_le(ctx.empty(1, 0, dtype), 1.0) == (None, 0)  # E = 0


def test_gather_index_of_uint32_and_a_bad_index():
    from seekr_amd import consumers
    ctx = _ctx()
    src = ctx.from_numpy(np.arange(100, 110, dtype=np.uint32))
    index = ctx.from_numpy(np.array([9, 0, 3, 3], np.uint32))
    out = consumers.gather_index(src, index, 4)
    assert list(out.to_numpy().reshape(-1)) == [109, 100, 103, 103]
    with pytest.raises(ValueError, match="outside"):
        consumers.gather_index(src, ctx.from_numpy(np.array([1, 10], np.uint32)), 2)


# ---- the guard --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("background", ["norm", "gamma"])
def test_guard_has_room(background):
    """p on every float32 from 4 096 steps below r* to 64 above: nothing below r0 = r* - 64 steps has p <= alpha32, and
    the largest distance below r* at which p <= alpha32 still occurs (0 for a monotone p) stays under a quarter of the
    guard.  Measured on an MI355X: 0 for both fixtures."""
    from seekr_amd import significant as sg
    ctx = _ctx()
    fitres = sc.backgrounds()[background]
    a32 = sc.alpha32(ALPHA)
    pv = sg._PValues(ctx, fitres, 1)
    r_star = sg.find_cutoff(pv.host, a32)
    assert r_star is not None and r_star > 0
    steps = np.arange(-4096, 65)
    values = np.array([sg.float32_steps(r_star, int(s)) for s in steps], dtype=np.float32)
    assert (np.diff(values.astype(np.float64)) > 0).all()
    p = pv.host(values)
    passing = p <= a32
    assert passing[steps == 0][0] and passing[steps >= 0].all()
    below = steps[passing & (steps < 0)]
    distance = int(-below.min()) if len(below) else 0
    print("guard, %s background: r* = %r, p <= alpha32 reaches %d float32 steps below r* (guard: %d)"
          % (background, float(r_star), distance, sg.GUARD_STEPS))
    assert not passing[steps < -sg.GUARD_STEPS].any()
    assert distance < sg.GUARD_STEPS // 4


# ---- edges ----------------------------------------------------------------------------------------------------------------
def assert_empty(res, n_tests):
    assert res.n_tests == n_tests and len(res) == 0
    assert [a.dtype for a in (res.rows, res.cols, res.r, res.p, res.p_adj)] == [np.uint32, np.uint32, np.float32, np.float32,
                                                                               np.float64]
    assert all(a.shape == (0,) for a in (res.rows, res.cols, res.r, res.p, res.p_adj))


def test_two_and_three_rows():
    from seekr_amd import significant as sg
    ctx = _ctx()
    rng = np.random.default_rng(44)
    base = rng.standard_normal(256)
    for n in (2, 3):
        x = (base + 0.3 * rng.standard_normal((n, 256))).astype(np.float32)  # every pair far in the tail
        z = prepared(ctx, x)
        fitres = sc.backgrounds()["norm"]
        for method in ("bonferroni", "fdr_bh"):
            got = sg.pearson_significant(z, fitres, method=method)
            want = FullPath(ctx, z, fitres).expected(method)
            assert len(want[0]) == n * (n - 1) // 2 == got.n_tests
            assert_same_pairs(got, want, (n, method))
        z.free()
    assert_empty(sg.significant_pairs(x[:1], fitres), 0)


def test_nothing_significant():
    from seekr_amd import significant as sg
    x = np.random.default_rng(45).standard_normal((40, 256)).astype(np.float32)
    res = sg.significant_pairs(x, sc.backgrounds()["norm"], method="bonferroni", alpha=1e-9)
    assert_empty(res, 780)
    assert res.r_cutoff is not None and res.r_cutoff > 0  # the search found a cutoff; no pair reached it, or none survived
    # p is NaN everywhere (a shape scipy rejects), and a background nothing exceeds
    assert_empty(sg.significant_pairs(x, [("gamma", 0.0, (-1.0, 0.0, 1.0))]), 780)
    assert_empty(sg.significant_pairs(x, [("uniform", 0.0, (0.0, 5.0))]), 780)


def test_refusals_on_the_device():
    from seekr_amd import significant as sg
    x = sc.planted_counts()[:50].copy()
    with pytest.raises(ValueError, match="not positive"):  # a background far to the left: r0 <= 0
        sg.significant_pairs(x, [("norm", 0.0, (-1.0, 0.0625))])
    with pytest.raises(ValueError, match="not positive"):
        sg.significant_pairs(x, np.full(100, -0.5))
    x[7] = 2.5  # a constant row: r is NaN in its row and column
    with pytest.raises(ValueError, match="constant row"):
        sg.significant_pairs(x, sc.backgrounds()["norm"])
    for method in sc.REFUSED:  # refused before the operand is looked at: no kernel is launched
        with pytest.raises(NotImplementedError):
            sg.pearson_significant(object(), sc.backgrounds()["norm"], method=method)


# ---- the command ------------------------------------------------------------------------------------------------------------
def run_command(argv):
    code = ("import sys; sys.argv = %r; from seekr_amd.console_scripts import console_significant_pairs; "
            "console_significant_pairs()" % (argv,))
    proc = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0, proc.stderr


def test_command(tmp_path):
    import pandas as pd
    from seekr_amd import significant as sg
    x = sc.planted_counts()[:120].astype(np.float64)
    names = ["tx%d, v1" % i if i == 4 else "tx%d" % i for i in range(len(x))]
    csv = tmp_path / "counts.csv"
    pd.DataFrame(x, index=names, columns=["c%d" % j for j in range(x.shape[1])]).to_csv(csv)
    bg = sc.backgrounds()["empirical_f64"]
    np.savetxt(tmp_path / "bg.csv", bg, delimiter=",")  # what find_dist(fit_model=False, outputname=...) writes
    out = tmp_path / "pairs.csv"
    run_command(["seekr_significant_pairs", str(csv), "-bg", str(tmp_path / "bg.csv"), "-o", str(out)])
    values = pd.read_csv(csv, index_col=0).to_numpy()
    want = sg.significant_pairs(values, np.loadtxt(tmp_path / "bg.csv", delimiter=","))
    frame = pd.read_csv(out, float_precision="round_trip")  # the default parser is off by an ulp now and then
    assert list(frame.columns) == ["row", "col", "r", "p", "p_adj"] and len(frame) == len(want) >= 20
    assert list(frame["row"]) == [names[i] for i in want.rows] and list(frame["col"]) == [names[j] for j in want.cols]
    assert np.array_equal(bits(frame["r"].to_numpy().astype(np.float32)), bits(want.r))
    assert np.array_equal(bits(frame["p"].to_numpy().astype(np.float32)), bits(want.p))
    assert np.array_equal(bits(frame["p_adj"].to_numpy()), bits(want.p_adj))
    # .npy input and a fitted distribution: indices instead of labels
    np.save(tmp_path / "counts.npy", values.astype(np.float32))
    out2 = tmp_path / "pairs2.csv"
    run_command(["seekr_significant_pairs", str(tmp_path / "counts.npy"), "-bi", "-d", "norm", "-p", "0.0", "0.0625", "-m", "holm",
                 "-a", "0.01", "-o", str(out2)])
    want2 = sg.significant_pairs(values.astype(np.float32), [("norm", 0.0, (0.0, 0.0625))], method="holm", alpha=0.01)
    frame2 = pd.read_csv(out2, float_precision="round_trip")
    assert len(frame2) == len(want2) >= 10
    assert list(frame2["row"]) == list(want2.rows) and list(frame2["col"]) == list(want2.cols)
    assert np.array_equal(bits(frame2["p_adj"].to_numpy()), bits(want2.p_adj))
    assert np.array_equal(bits(frame2["r"].to_numpy().astype(np.float32)), bits(want2.r))
