"""What tests/test_gpu_fill_exact.py relies on, shown without a GPU: the builder's conditions hold for every GPU case, the
row sums are order-free in float32, the threshold rows sit on the intended side, and each mutant of the model changes
what the GPU test compares."""
import numpy as np
import pytest

import fill_exact_cases as fc

F32 = np.float32
FAMILY_WIDTHS = {"wave": 300, "reg": 1024, "rowreg": 9999, "block": 16807, "wide": 40004}


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


# ------------------------------------------------------------------ the conditions, for every GPU case
@pytest.mark.parametrize("cls", ["A", "B"])
@pytest.mark.parametrize("family,cols,modes", fc.STORE_CASES)
def test_store_cases_meet_the_conditions(family, cols, modes, cls):
    rows = fc.assert_unflagged(fc.class_rows(cols, cls))       # check(): the two sums, the bound, the round trip
    assert len({r.tobytes() for r in rows.d}) == rows.rows       # distinct permutations
    assert np.array_equal(bits(fc.fill_arith(rows.x)), bits(rows.z))   # the plain restatement gives the model's z
    for mode in modes:
        if mode != "m0":
            fc.tail_inputs(rows, 3, with_scale=mode != "c")      # asserts (raw - centre) / scale == x by its bits
    _, exact = fc.diag_model(rows)
    assert exact.all() == (cls == "A")
    if cls == "B":   # lo != 0 at the operand's scale: the directed rounding of hi is exercised
        hi, lo, _ = fc.ec.f16_halves(rows.z, fc.ec.f16_scale(cols))
        assert (lo != 0).mean() >= 0.5
        near, _ = fc.f16_halves_nearest(rows.z, fc.ec.f16_scale(cols))
        assert (hi.view(np.uint16) != near.view(np.uint16)).mean() >= 0.2


@pytest.mark.parametrize("family,cols", fc.FLAG_WIDTHS)
def test_threshold_rows_sit_on_the_intended_side(family, cols):
    """same_cases and pair_cases assert, in float32: the flag that is meant and no other, the counts themselves, every
    other listed seam broken.  Here also: one row each side, and the arithmetic restatement gives their z."""
    same = fc.same_cases(family, cols)
    assert [f for _, _, f in same] == [True, False]
    pairs = fc.pair_cases(family, cols)
    assert [f for _, _, f in pairs] == [True, False] * (len(pairs) // 2) and len(pairs) >= 6
    for _, r, _ in same + pairs:
        assert np.array_equal(bits(fc.fill_arith(r.x)), bits(r.z))
    if cols == 4096 or family == "reg":
        fc.same_cases("reg", 4096)


def test_where_a_threshold_is_met_with_equality():
    """float32(share) * float32(K) is an integer at few widths: only there can `>` for `>=` show.  Of the widths tested
    these are: `same` at 300 columns, equal neighbours at 8 191, 9 991 and 40 001 (one width per kernel that has the
    rule; the register kernel's three widths meet none), the outlier rule at 1 024, 16 384 and 65 536, and the
    fp16 range (65 504 itself)."""
    met = {(name, K) for family, K in fc.FLAG_WIDTHS + [("reg", 4096)]
           for name, thr in (("same", fc.same_threshold(K)),
                             ("quads", fc.quad_threshold(K)) if family == "reg" else ("pairs", fc.pair_threshold(K)))
           if float(thr) == int(thr)}
    assert met == {("same", 300), ("pairs", 8191), ("pairs", 9991), ("pairs", 40001)}
    assert [K for _, K in fc.OUTLIER_WIDTHS if 4 * fc.smallest_outlier(K) ** 2 == K] == [1024, 16384, 65536]


@pytest.mark.parametrize("family,cols", fc.LEVEL_WIDTHS + fc.OUTLIER_WIDTHS)
def test_level_and_outlier_rows(family, cols):
    base = fc.class_rows(cols, "A")
    if (family, cols) in fc.LEVEL_WIDTHS:
        two, three = fc.Rows(fc.two_level_row(cols), 1).check(), fc.Rows(fc.three_level_row(cols), 1).check()
        f2, f3 = fc.row_flags(two, family), fc.row_flags(three, family)
        assert f2["levels"][0] and not (f2["same"][0] or f2["pairs"][0] or f2["outlier"][0])
        assert not f3["coherent"][0] and not f3["outlier"][0]
    if (family, cols) in fc.OUTLIER_WIDTHS:
        top = fc.smallest_outlier(cols)
        for two_z, flagged in ((top, True), (top - 1, False)):
            r = fc.Rows(fc.outlier_row(cols, two_z), 2).check()
            f = fc.row_flags(r, family)
            assert bool(f["outlier"][0]) == flagged and not f["coherent"][0]
            both = fc.Rows(np.vstack([base.d, r.d]), np.r_[base.q, r.q]).check()
            fc.tail_inputs(both, 5)
    r = fc.Rows(fc.outlier_row(1000, fc.smallest_outlier(1000)), 2).check()
    assert not fc.row_flags(r, "wave")["outlier"][0]            # never below 1 024 columns


# ------------------------------------------------------------------ the sums are order-free
def sums_in_four_orders(v):
    """float32 sums of the rows of v: sequential, reversed, numpy's pairwise order, 16 strided accumulators."""
    v = np.ascontiguousarray(v, dtype=F32)
    seq = np.cumsum(v, axis=1, dtype=F32)[:, -1]
    rev = np.cumsum(v[:, ::-1], axis=1, dtype=F32)[:, -1]
    pair = np.add.reduce(v, axis=1, dtype=F32)
    pad = np.zeros((v.shape[0], -v.shape[1] % 16), F32)
    acc = np.cumsum(np.concatenate([v, pad], axis=1).reshape(v.shape[0], -1, 16), axis=1, dtype=F32)[:, -1, :]
    strided = np.cumsum(acc, axis=1, dtype=F32)[:, -1]
    return seq, rev, pair, strided


@pytest.mark.parametrize("cols", [64, 100, 300, 1000, 1024, 4096, 4100, 8191, 8192, 8200, 9999, 15625, 16384, 16807, 40004, 65536])
def test_row_sums_are_order_free(cols):
    for cls in "AB":
        rows = fc.class_rows(cols, cls)
        rng = np.random.default_rng(cols)
        for shuffle in (False, True):
            x = rows.x[:, rng.permutation(cols)] if shuffle else rows.x
            mean = F32(3) * rows.s.astype(F32)
            c = x - mean[:, None]
            sd = (rows.q * rows.s).astype(F32)
            for what, v, want in (("sum x", x, mean * F32(cols)), ("centred sum", c, np.zeros(rows.rows, F32)),
                                  ("squared deviations", c * c, sd * sd * F32(cols))):
                for got in sums_in_four_orders(v):
                    assert np.array_equal(bits(got), bits(want)), (what, cols, cls, shuffle)
            if cls == "A":   # sum z^2 = K: diag == 1.0f
                z = c / sd[:, None]
                for got in sums_in_four_orders(z * z):
                    assert np.array_equal(bits(got / F32(cols)), bits(np.ones(rows.rows, F32)))


# ------------------------------------------------------------------ the mutants
@pytest.mark.parametrize("family,cols", sorted(FAMILY_WIDTHS.items()))
@pytest.mark.parametrize("mutant", ["last", "pad", "km1", "recip", "hi_nearest"])
def test_arithmetic_mutants_change_the_stored_operand(family, cols, mutant):
    """On the rows of the family's store case every mutant changes the fp16 halves the GPU test compares (class B for the
    two that only rounded quotients can show; both classes for the others), and the first three the float32 layout too."""
    for cls in ("B",) if mutant in ("recip", "hi_nearest") else ("A", "B"):
        rows = fc.class_rows(cols, cls)
        want = fc.stored(rows.z, "f16x3")
        if mutant == "hi_nearest":
            got = fc.stored(rows.z, "f16x3", mutant=mutant)
        else:
            z = fc.fill_arith(rows.x, mutant).astype(F32)
            got = fc.stored(z, "f16x3")
            if mutant != "recip":
                assert (bits(z) != bits(rows.z)).any(axis=1).all()
        assert (got != want).any(axis=(1, 2, 3)).all(), (family, cols, cls, mutant)   # every row


@pytest.mark.parametrize("family,cols", [c for c in fc.FLAG_WIDTHS if c[0] != "reg"])
def test_a_pair_not_counted_at_a_seam_clears_the_flag(family, cols):
    """The row that is tipped by the pair on a seam loses its flag when that one pair is not counted, on every seam (the
    register kernel counts inside quads: its twin rows move a pair across the boundary instead, below)."""
    tipped = [(r, r.seam) for note, r, flagged in fc.pair_cases(family, cols) if flagged]
    assert len(tipped) == len(fc.seams(family, cols))
    for r, seam in tipped:
        assert fc.row_flags(r, family)["coherent"][0]
        assert not fc.row_flags(r, family, skip_pair=seam[0])["coherent"][0], seam


def test_quad_twins_count_across_the_boundary_in_a_whole_row_count():
    """The register kernel's twin rows: the pair moved across the quad boundary is still an equal pair of the row — a
    kernel that counted across lanes would keep the flag."""
    for cols in (1024, 16384):
        cases = fc.pair_cases("reg", cols)
        for (_, a, _), (_, b, _) in zip(cases[0::2], cases[1::2]):
            (_, pa, qa), (_, pb, qb) = fc.counts(a.x), fc.counts(b.x)
            assert pa[0] == pb[0] and qa[0] == qb[0] + 1


def test_strict_comparison_shows_where_equality_is_met():
    """`>` for `>=`: changes the verdict of the threshold row exactly where the threshold is an integer."""
    for family, cols, rule in (("wave", 300, "same"), ("block", 8191, "pairs"), ("rowreg", 9991, "pairs"), ("wide", 40001, "pairs")):
        cases = fc.same_cases(family, cols) if rule == "same" else fc.pair_cases(family, cols)
        note, r, flagged = cases[0]
        assert flagged and not fc.row_flags(r, family, strict=rule)["coherent"][0]
    for family, cols in (("reg", 1024), ("reg", 16384), ("rowreg", 65536)):
        r = fc.Rows(fc.outlier_row(cols, fc.smallest_outlier(cols)), 2)
        assert fc.row_flags(r, family)["outlier"][0] and not fc.row_flags(r, family, strict="outlier")["outlier"][0]
    for family, cols in (("reg", 1024), ("rowreg", 9999), ("wide", 40004)):      # ... and nowhere else
        for note, r, flagged in fc.same_cases(family, cols) + fc.pair_cases(family, cols)[:2]:
            assert fc.row_flags(r, family, strict="same")["coherent"][0] == flagged
            assert fc.row_flags(r, family, strict="pairs")["coherent"][0] == flagged
