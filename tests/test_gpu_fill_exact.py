"""The four operand fill kernels against one numpy model (tests/fill_exact_cases.py): rows whose sum, centred sum and sum of
squared deviations are exact in float32 in any order, so that mean, sd, z = fl32(d / q), the stored halves, the diagonal
and every flag count are the same whatever order a kernel sums in and whatever form its division takes.  Every comparison
is an equality of bit patterns; the one exception is the diagonal of a class-B row (z rounded), which holds to the derived
K 2^-24 relative.  Needs a real MI355X: run with `-m gpu`."""
import numpy as np
import pytest

import fill_exact_cases as fc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    from seekr_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def ctx(L):
    return L.default_context()


@pytest.fixture(scope="module")
def cus(ctx):
    """Compute units of the device the context runs on: read, not assumed."""
    n = ctx.compute_units()
    assert n > 0
    return n


class Tally:
    """Collects every arm of a case before failing, so that one run shows which of them disagree with the model."""

    def __init__(self):
        self.bad = []

    def same(self, label, got, want):
        got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
        if got.shape != want.shape or got.dtype != want.dtype:
            self.bad.append((label, "shape / dtype", got.shape, got.dtype, want.shape, want.dtype))
            return
        diff = got != want
        if diff.any():
            at = tuple(int(v) for v in np.argwhere(diff)[0])
            self.bad.append((label, "%d of %d cells differ, first at %s: %#x vs the model's %#x"
                             % (int(diff.sum()), diff.size, at, int(got[at]), int(want[at]))))

    def check(self, label, ok, *what):
        if not ok:
            self.bad.append((label,) + what)

    def done(self):
        assert not self.bad, self.bad


def run_fill(L, ctx, precision, mode, x=None, tail=None, standardize=True):
    """One L.operand_fill.  mode "m0": rows x as they are; "m1" / "m1y" / "m1a": tail = (raw, centre, scale) through the
    normalisation tail, without y, with y, with y aliasing the input; "c": a centre vector alone.  Returns (op, has_nan, y)."""
    prec = L.PRECISIONS[precision]
    if mode == "m0":
        op, nan = L.operand_fill(ctx, ctx.from_numpy(x), precision=prec, row_standardize=standardize, want_nan=True)
        return op, nan, None
    raw, centre, scale = tail
    dx, dc = ctx.from_numpy(raw), ctx.from_numpy(centre)
    ds = ctx.from_numpy(scale) if scale is not None else None
    y = ctx.zeros(*raw.shape) if mode == "m1y" else dx if mode == "m1a" else None
    op, nan = L.operand_fill(ctx, dx, precision=prec, center=dc, scale=ds, y=y, want_nan=True)
    return op, nan, (y.to_numpy() if y is not None else None)


def stored_of(op):
    return fc.read_back(op.as_matrix().to_numpy(), op.rows, op.cols, op.kind)


def diagonal(L, ctx, op, row0=0, n=None):
    v = op if n is None else op.view(row0, n)
    r = ctx.zeros(v.rows, v.rows)
    L.pearson_gemm_op(ctx, v, v, r, symmetric=True)
    return r.to_numpy().diagonal().copy()


def check_diag(t, label, got, rows, idx=None):
    want, exact = fc.diag_model(rows)
    if idx is not None:
        want, exact = want[idx], exact[idx]
    t.same(label + " diag (class A rows)", got[exact].view(np.uint32), want[exact].view(np.uint32))
    loose = ~exact
    ok = np.abs(got[loose].astype(np.float64) - want[loose]) <= rows.cols * 2.0 ** -24 * want[loose]
    t.check(label + " diag outside K 2^-24", ok.all(), got[loose].tolist(), want[loose].tolist())


# ------------------------------------------------------------------ a. stored operand, diag, y
@pytest.mark.parametrize("cls", ["A", "B"])
@pytest.mark.parametrize("family,cols,modes", fc.STORE_CASES)
def test_stored_operand_is_the_model(L, ctx, family, cols, modes, cls):
    """5 rows of distinct permutations, every mode of the width's kernel, float32 layout, fp16 halves and bf16 halves:
    as_matrix() by its bits, the kind, no flag, the diagonal of a self-comparison, and y == x bit for bit."""
    rows = fc.assert_unflagged(fc.class_rows(cols, cls))
    t = Tally()
    want = {p: fc.stored(rows.z, p) for p in fc.PRECISIONS}
    for mode in modes:
        tail = fc.tail_inputs(rows, 3, with_scale=mode != "c") if mode != "m0" else None
        for precision in fc.PRECISIONS:
            label = "%s %s %s" % (family, mode, precision)
            op, nan, y = run_fill(L, ctx, precision, mode, x=rows.x, tail=tail)
            t.check(label + " kind", op.kind == fc.kind_of(precision, cols), op.kind)
            t.check(label + " flags", not op.coherent and not nan, op.coherent, nan)
            if op.kind == fc.kind_of(precision, cols):
                t.same(label, stored_of(op), want[precision])
            check_diag(t, label, diagonal(L, ctx, op), rows)
            if y is not None:
                t.same(label + " y", y.view(np.uint32), rows.x.view(np.uint32))
            op.free()
    t.done()


@pytest.mark.parametrize("family,cols,per_cu", fc.ROW_LOOP_CASES)
def test_row_loop_stores_every_row(L, ctx, cus, family, cols, per_cu):
    """More rows than the launch has workgroups, + 3 (a ragged last pass; the rowreg prefetch then re-reads its own row):
    every row's halves against the model.  The register kernel has no loop: 5 rows, four to a workgroup."""
    base = fc.class_rows(cols, "B")
    n = cus * per_cu + 3 if per_cu else 5
    idx = np.arange(n) % base.rows
    op, nan, _ = run_fill(L, ctx, "f16x3", "m0", x=base.x[idx])
    t = Tally()
    t.check("kind / flags", op.kind == 2 and not op.coherent and not nan, op.kind, op.coherent, nan)
    t.same("halves", stored_of(op), fc.stored(base.z, "f16x3")[idx])
    last = min(n, 9)
    check_diag(t, "last rows", diagonal(L, ctx, op, n - last, last), base, idx[n - last:])
    t.done()


# ------------------------------------------------------------------ b. thresholds: one flagged row among unflagged ones
def among(base, row, where, n):
    """n rows: `row` (a Rows of one row) at index `where`, the rows of base around it.  Returns (x, z)."""
    idx = np.arange(n) % base.rows
    x, z = base.x[idx].copy(), base.z[idx].copy()
    x[where], z[where] = row.x[0], row.z[0]
    return x, z


def flag_case(L, ctx, t, label, base, row, where, n, coherent, precision="f16x3"):
    x, z = among(base, row, where, n)
    op, nan, _ = run_fill(L, ctx, precision, "m0", x=x)
    t.check(label + " kind", op.kind == fc.kind_of(precision, base.cols), op.kind)
    t.check(label + " coherent (row %d of %d)" % (where, n), op.coherent == coherent, op.coherent, coherent)
    if n <= 16 and op.kind == fc.kind_of(precision, base.cols):
        t.same(label + " halves", stored_of(op), fc.stored(z, precision))
    op.free()


def second_pass_rows(cus, family, cols):
    """(rows, index of a row of the second grid pass) for the width's kernel; the register kernel: a later workgroup."""
    per_cu = {"wave": 32, "rowreg": 1, "wide": 2}.get(family)
    if family == "block":
        per_cu = max(1, (150 * 1024) // (4 * ((cols + 3) & ~3)))
    if family == "reg":
        return 9, 6
    return cus * per_cu + 3, cus * per_cu + 1


@pytest.mark.parametrize("family,cols", fc.FLAG_WIDTHS)
def test_same_threshold_from_both_sides(L, ctx, cus, family, cols):
    """`same` at the smallest count that satisfies the float32 comparison, and at one less, with the flagged row first,
    last, and in the second pass of the row loop."""
    base = fc.assert_unflagged(fc.class_rows(cols, "A"), family)
    n2, w2 = second_pass_rows(cus, family, cols)
    t = Tally()
    for label, row, flagged in fc.same_cases(family, cols):
        for where, n in ((0, 6), (5, 6), (w2, n2)):
            flag_case(L, ctx, t, label, base, row, where, n, flagged)
    t.done()


def test_same_threshold_with_bf16_halves(L, ctx):
    base = fc.assert_unflagged(fc.class_rows(4096, "A"), "reg")
    t = Tally()
    for label, row, flagged in fc.same_cases("reg", 4096):
        flag_case(L, ctx, t, label, base, row, 5, 6, flagged, precision="bf16x3")
    t.done()


@pytest.mark.parametrize("family,cols", fc.FLAG_WIDTHS)
def test_equal_neighbours_on_every_seam(L, ctx, family, cols):
    """Equal neighbours at the threshold with the pair that tips it on each seam of the kernel in turn, every other equal
    pair off all seams, and each one's twin with that pair broken (register kernel: moved across the quad boundary)."""
    base = fc.assert_unflagged(fc.class_rows(cols, "A"), family)
    t = Tally()
    for i, (label, row, flagged) in enumerate(fc.pair_cases(family, cols)):
        flag_case(L, ctx, t, label, base, row, (0, 5)[(i // 2) % 2], 6, flagged)
    t.done()


@pytest.mark.parametrize("family,cols", fc.LEVEL_WIDTHS)
def test_two_level_rule(L, ctx, family, cols):
    """A +-1 row (statistic 0) is coherent by the two-level rule alone; a three-level class-A row is not."""
    base = fc.assert_unflagged(fc.class_rows(cols, "A"), family)
    two = fc.Rows(fc.two_level_row(cols), 1).check()
    three = fc.Rows(fc.three_level_row(cols), 1).check()
    f2, f3 = fc.row_flags(two, family), fc.row_flags(three, family)
    assert f2["levels"][0] and not f2["same"][0] and not f2["pairs"][0] and not f2["outlier"][0]
    assert not f3["coherent"][0] and not f3["outlier"][0]
    t = Tally()
    flag_case(L, ctx, t, "two levels", base, two, 5, 6, True)
    flag_case(L, ctx, t, "three levels", base, three, 5, 6, False)
    t.done()


@pytest.mark.parametrize("family,cols", fc.OUTLIER_WIDTHS + [("wave", 1000)])
def test_outlier_reroute_from_both_sides(L, ctx, family, cols):
    """One cell at the smallest multiple of 1/2 with 16 z^2 >= K: the operand is refilled in the float32 layout (kind 0) and
    that layout is the model's z, also through the normalisation tail with y (the refill reads y); 1/2 less: fp16 halves.
    Below 1 024 columns there is never a reroute."""
    base = fc.assert_unflagged(fc.class_rows(cols, "A"), family)
    top = fc.smallest_outlier(cols)
    t = Tally()
    for two_z, rerouted in ((top, cols >= 1024), (top - 1, False)):
        row = fc.Rows(fc.outlier_row(cols, two_z), 2).check()
        f = fc.row_flags(row, family)
        assert bool(f["outlier"][0]) == rerouted and not f["coherent"][0]
        both = fc.Rows(np.vstack([base.d, row.d]), np.r_[base.q, row.q]).check()   # the outlier row last
        x, z = both.x, both.z
        for mode in ("m0", "m1y"):
            label = "z = %g %s" % (two_z / 2, mode)
            tail = fc.tail_inputs(both, 5) if mode != "m0" else None
            op, nan, y = run_fill(L, ctx, "f16x3", mode, x=x, tail=tail)
            kind = 0 if rerouted else 2
            t.check(label + " kind", op.kind == kind and not op.coherent and not nan, op.kind, op.coherent, nan)
            if op.kind == kind:
                t.same(label, stored_of(op), fc.stored(z, "fp32" if rerouted else "f16x3"))
            if y is not None:
                t.same(label + " y", y.view(np.uint32), x.view(np.uint32))
            check_diag(t, label, diagonal(L, ctx, op), both)
            op.free()
    t.done()


@pytest.mark.parametrize("cols", [256, 1000])
def test_fp16_range_from_both_sides(L, ctx, cols):
    """row_standardize=False: a cell of exactly 65 504 / scale is accepted (and stored), the next float32 raises the range
    error; the cell sits at column 0 or at the last column of the last row."""
    base = fc.class_rows(cols, "A")
    edge = np.float32(65504.0) / fc.ec.f16_scale(cols)
    assert float(edge) * float(fc.ec.f16_scale(cols)) == 65504.0
    t = Tally()
    for col in (0, cols - 1):
        for sign in (1.0, -1.0):
            x = base.x.copy()
            x[-1, col] = sign * edge
            op, _, _ = run_fill(L, ctx, "f16x3", "m0", x=x, standardize=False)
            t.check("kind", op.kind == 2, op.kind)
            t.same("halves, %g at column %d" % (sign * edge, col), stored_of(op), fc.stored(x, "f16x3"))
            x[-1, col] = sign * np.nextafter(edge, np.float32(np.inf))
            with pytest.raises(ValueError, match="exceeds the split-fp16 operand range"):
                run_fill(L, ctx, "f16x3", "m0", x=x, standardize=False)
    t.done()


def nan_cells(cus, family, cols):
    """[(rows, row, column)]: (0, 0); the last row's last column; rowreg at 9 999 columns: a whole piece of the unmasked body
    and the ragged piece; a row of the second pass of the row loop."""
    cells = [(6, 0, 0), (6, 5, cols - 1)]
    if (family, cols) == ("rowreg", 9999):
        cells += [(6, 2, 5000), (6, 2, 9997)]
    n2, w2 = second_pass_rows(cus, family, cols)
    return cells + [(n2, w2, cols // 2 + 1)]


@pytest.mark.parametrize("family,cols", fc.NAN_WIDTHS)
def test_one_nan_cell(L, ctx, cus, family, cols):
    """One NaN cell going through the normalisation tail (centre and scale vectors, y written): has_nan, y is NaN exactly
    there, that row of the operand is NaN (its padding +0), every other row's halves are the model's."""
    base = fc.assert_unflagged(fc.class_rows(cols, "A"), family)
    want5 = fc.stored(base.z, "f16x3")
    raw5, centre, scale = fc.tail_inputs(base, 9)
    kt = (cols + 31) // 32
    real = (np.arange(kt * 32) < cols).reshape(kt, 1, 32) & np.ones((1, 2, 1), bool)
    t = Tally()
    for n, row, col in nan_cells(cus, family, cols):
        idx = np.arange(n) % base.rows
        raw = raw5[idx].copy()
        raw[row, col] = np.nan
        op, nan, y = run_fill(L, ctx, "f16x3", "m1y", tail=(raw, centre, scale))
        label = "NaN at (%d, %d) of %d rows" % (row, col, n)
        t.check(label + " has_nan / kind", nan and op.kind == 2, nan, op.kind)
        want_y = base.x[idx].copy()
        want_y[row, col] = np.nan
        t.check(label + " y NaN there", np.isnan(y[row, col]))
        y[row, col] = want_y[row, col]
        t.same(label + " y", y.view(np.uint32), want_y.view(np.uint32))
        if op.kind == 2:
            got = stored_of(op)
            others = np.arange(n) != row
            t.same(label + " other rows", got[others], want5[idx][others])
            cells = got[row].view(np.float16)
            t.check(label + " the row is NaN", np.isnan(cells[real]).all(), int(np.isnan(cells[real]).sum()))
            t.check(label + " its padding is +0", not got[row][~real].any())
        op.free()
    t.done()
