"""tools/consumer_sweep.py without a device: its references against the reference's own lines by brute force, the sizes,
cells, windows and offsets its generators must contain, and the case list of tests/golden/pvals_sweep.npz."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import consumer_sweep as sweep  # noqa: E402

SMALL_SIZES = tuple(n for n in sweep.BG_SIZES if n <= 5000) + (5000,)


def brute_force(cells, fitres):
    """find_pval.py:158-164: np.sum(fitres > sim[i, j]) / len(fitres) stored into a float32 matrix."""
    out = np.zeros(len(cells), dtype=np.float32)
    with np.errstate(invalid="ignore"):
        for lo in range(0, len(cells), 4096):
            out[lo:lo + 4096] = (fitres[None, :] > cells[lo:lo + 4096, None]).sum(axis=1) / len(fitres)
    return out


@pytest.mark.parametrize("kind", sweep.BG_KINDS)
def test_searchsorted_rule_is_the_reference_loop(kind):
    for n in SMALL_SIZES:
        fitres = sweep.background(kind, n, seed=1)
        assert fitres.dtype == (np.float64 if kind == "float64 near cells" else np.float32) and len(fitres) == n
        cells = sweep.pvalue_cells(fitres, seed=1)
        if n >= 4095:  # every fourth cell, and all of the special and random ones
            cells = np.concatenate([cells[::4], cells[:sweep.N_RANDOM_CELLS + 5]])
        want = brute_force(cells, fitres)
        got = sweep.pvalue_rule(cells, fitres)
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), (kind, n)
        one = np.float32(cells[7])  # and the scalar form, as the reference writes it
        with np.errstate(invalid="ignore"):
            assert np.float32(np.sum(fitres > one) / len(fitres)) == sweep.pvalue_rule(cells[7:8], fitres)[0]


def test_background_kinds_hold_what_they_are_named_for():
    for n in (257, 8193, 1000003):
        stride, _ = sweep.table_geometry(n)
        ties = sweep.background("two decimals", n)
        _, counts = np.unique(ties, return_counts=True)
        assert counts.max() > 2 * stride, (n, counts.max())  # a tie run longer than a bucket
        assert len(np.unique(sweep.background("constant", n))) == 1
        inf = sweep.background("inf", n)
        assert np.isneginf(inf).any() and np.isposinf(inf).any()
        assert np.isnan(sweep.background("nan", n)).any()
    assert np.isnan(sweep.background("nan", 1)).all()  # no valid value at all
    near = sweep.background("float64 near cells", 5000)
    cells = sweep.random_cells(1).astype(np.float64)
    gap = np.abs(near[:, None] - cells[None, :80]).min(axis=1)
    assert near.dtype == np.float64 and ((gap > 0) & (gap < 2e-10)).sum() >= 80
    # rounding such a background to the nearest float32 changes counts (what the sweep must catch); rounding up does not
    from seekr_amd.consumers import ceil_float32
    all_cells = sweep.pvalue_cells(near)
    want = sweep.pvalue_rule(all_cells, near)
    assert not np.array_equal(sweep.pvalue_rule(all_cells, near.astype(np.float32)), want)
    assert np.array_equal(sweep.pvalue_rule(all_cells, ceil_float32(near)), want)


def test_ceil_float32():
    from seekr_amd.consumers import ceil_float32
    rng = np.random.default_rng(3)
    v = np.concatenate([rng.normal(0, 0.3, 5000), rng.normal(0, 0.3, 500).astype(np.float32), [0.0, -0.0, 1e-50, -1e-50, 1e39, -1e39,
                        3.4028235677973366e38, np.inf, -np.inf, np.nan]])
    c = ceil_float32(v)
    ok = ~np.isnan(v)
    assert c.dtype == np.float32 and np.array_equal(np.isnan(c), ~ok)
    wide = c[ok].astype(np.float64)
    assert (wide >= v[ok]).all()
    with np.errstate(over="ignore"):
        below = np.nextafter(c[ok], np.float32(-np.inf)).astype(np.float64)
    assert ((below < v[ok]) | np.isneginf(v[ok])).all()  # the smallest such float32
    assert c[ok][-3] == np.inf and c[ok][-4] == -np.finfo(np.float32).max  # 1e39 and -1e39
    assert np.array_equal(ceil_float32(np.arange(-5, 5)), np.arange(-5, 5, dtype=np.float32))


def test_background_sizes_reach_every_stride_and_table_length():
    assert {1, 2, 3, 255, 256, 257, 4095, 4096, 4097, 8191, 8192, 8193, 12288, 12289, 1000003, 1 << 20, (1 << 20) + 1,
            (1 << 22) + 1} == set(sweep.BG_SIZES)
    geometry = [sweep.table_geometry(n) for n in sweep.BG_SIZES]
    assert {g[0] for g in geometry} == {1, 2, 3, 4, 245, 256, 257, 1025}
    assert {g[1] for g in geometry} >= {1, 2, 3, 255, 2049, 2731, 4082, 4093, 4096}
    assert sweep.table_geometry(4096) == (1, 4096) and sweep.table_geometry(4097) == (2, 2049)
    ragged = [n for n, (stride, n_table) in zip(sweep.BG_SIZES, geometry) if n % stride]  # a last bucket that is not full
    assert len(ragged) >= 5, ragged


def test_cells_hold_every_table_entry_and_its_neighbours():
    for n in (3, 4097, 12289):
        fitres = sweep.background("normal", n)
        bg = np.sort(fitres)
        stride, n_table = sweep.table_geometry(n)
        cells = sweep.pvalue_cells(fitres)
        have = set(cells[~np.isnan(cells)].view(np.uint32).tolist())

        def held(v):
            return set(np.asarray(v, dtype=np.float32).view(np.uint32).tolist()) <= have

        entries = bg[np.minimum(n - 1, (np.arange(n_table) + 1) * stride - 1)]
        firsts = bg[np.arange(n_table) * stride]
        for v in (entries, firsts, bg[:1], bg[-1:]):
            assert held(v) and held(np.nextafter(v, np.float32(np.inf))) and held(np.nextafter(v, np.float32(-np.inf)))
        assert held([0.0, -0.0, np.inf, -np.inf]) and np.isnan(cells).any()
        assert len(cells) >= sweep.N_RANDOM_CELLS + 6 * n_table


def test_topk_lists_windows_and_reference():
    assert set(sweep.TOPK_KS) == {1, 2, 63, 64, 65, 255, 256, 257, 1000, 4096}
    assert set(sweep.TOPK_WIDTHS) == {1, 2, 255, 256, 257, 513, 5000}
    assert any(m - 1 < k for m in sweep.TOPK_WIDTHS for k in sweep.TOPK_KS)
    assert sweep.TOPK_LOOP_SHAPE == (4200, 40, 3) and sweep.TOPK_LOOP_SHAPE[0] > 16 * 256
    rows = sweep.TOPK_ROWS
    for m in (257, 5000):
        seen = set()
        for name, c0, c1, row0, col0 in sweep.topk_windows(m, rows):
            assert 0 <= c0 <= c1 <= m and row0 >= 0 and col0 >= 0
            diag = row0 + np.arange(rows) - col0  # local column of each row's diagonal cell
            inside = (diag >= c0) & (diag < c1)
            if c0 < c1 and col0 != 0:
                seen.add("inside" if inside.all() else "outside" if not inside.any() else
                         "first edge" if diag.min() < c0 else "last edge")
                if not inside.all() and inside.any():
                    assert (c0 in diag and c0 - 1 in diag) or (c1 - 1 in diag and c1 in diag), name
        assert seen == {"inside", "outside", "first edge", "last edge"}, seen
    r = sweep.topk_block(np.random.default_rng(1), rows, 40)
    assert np.isnan(r[1]).all() and len(np.unique(r[2])) == 1 and np.isinf(r[4]).any()
    assert (r[3] == 0).all() and np.signbit(r[3]).any() and not np.signbit(r[3]).all()
    idx, val = sweep.topk_reference(r, 5, 10, 30, 1012, 1000)
    for i in range(rows):  # by selection: the largest remaining value, the smaller column on ties, NaN last
        left = [c for c in range(10, 30) if c != 12 + i]
        for t in range(5):
            finite = [c for c in left if not np.isnan(r[i, c])]
            best = max(finite, key=lambda c: (r[i, c], -c)) if finite else left[0]
            assert idx[i, t] == best + 1000 and (val[i, t] == r[i, best] or np.isnan(r[i, best]))
            left.remove(best)
    idx, val = sweep.topk_reference(r, 4, 7, 9, 0, 0)  # two candidates (one on the diagonal rows): the rest is empty
    assert (idx[:, 2:] == sweep.NO_CELL).all() and np.isnan(val[:, 2:]).all() and idx[7, 1] == sweep.NO_CELL


def test_threshold_edges_and_triu_references():
    rng = np.random.default_rng(2)
    r = sweep.block_with_specials(rng, 60, 60)
    assert np.isnan(r).any() and np.isinf(r).any() and np.signbit(r[r == 0]).any()
    names = sweep.cutoffs(sweep.present_value(r))
    p = sweep.present_value(r)
    assert (r == p).any() and names["just below it"] < p < names["just above it"]
    assert np.isnan(names["NaN"]) and names["+inf"] == np.inf and names["-inf"] == -np.inf
    for cutoff in names.values():
        want = r.copy()
        with np.errstate(invalid="ignore"):
            want[want < cutoff] = 0
        np.fill_diagonal(want, 0)
        assert sweep.same_bits_or_nan(sweep.threshold_reference(r, cutoff, 0), want)
        blk = sweep.threshold_reference(r[20:45], cutoff, 20)  # a row block: the diagonal starts at column 20
        assert sweep.same_bits_or_nan(blk, want[20:45])
        for upper in (False, True):
            kept = np.triu(want, 1) if upper else want
            i, j = np.nonzero(kept)
            gi, gj, gv = sweep.edges_reference(r, cutoff, 60, 0, 60, 0, 0, upper)
            assert np.array_equal(gi, i) and np.array_equal(gj, j) and sweep.same_bits_or_nan(gv, kept[i, j])
            gi, gj, gv = sweep.edges_reference(r[20:45], cutoff, 25, 10, 50, 20, 0, upper)  # rows 20 .. 44, columns 10 .. 49
            sub = np.zeros_like(kept)
            sub[20:45, 10:50] = kept[20:45, 10:50]
            i, j = np.nonzero(sub)
            assert np.array_equal(gi, i) and np.array_equal(gj, j) and sweep.same_bits_or_nan(gv, sub[i, j])
    rows, cols = sweep.THRESHOLD_SHAPE
    offsets = sweep.diag_offsets(rows, cols)
    assert any(d < -rows for d in offsets) and any(-rows < d < 0 for d in offsets) and any(d >= cols for d in offsets)
    assert sweep.THRESHOLD_LARGE[0] * sweep.THRESHOLD_LARGE[1] > 256 * 8 * 256 * 4
    assert np.array_equal(sweep.threshold_reference(r, np.float32(-np.inf), 1 << 40), r, equal_nan=True)
    assert set(sweep.TRIU_NS) == {255, 256, 257, 4099} and max(sweep.TRIU_NS) > 16 * 256
    for n in (1, 7, 64):
        a = rng.standard_normal((n, n))
        assert sweep.triu_ks(n) == (0, 1, n - 1, n, n + 3)
        for k in sweep.triu_ks(n):
            assert np.array_equal(sweep.triu_reference(a, k), a[np.triu_indices(n, k=k)])


def test_fixture_covers_the_ten_distributions_and_the_large_shapes(golden_dir):
    cases = sweep.fixture_cases()
    names = {c[0] for c in cases}
    assert names == {"cauchy", "chi2", "expon", "exponpow", "gamma", "lognorm", "norm", "pareto", "rayleigh", "uniform"}
    fits = [c for c in cases if c[2].startswith("fit to ")]
    assert len(fits) == 40 and {c[0] for c in fits} == names and len({c[2] for c in fits}) == 4
    hand = {(c[0], c[1][0]) for c in cases if c[2] == "hand-set"}
    for a in (0.05, 1.0, 3e3, 2e4, 1e5, 187114.0, 3e5, 1e6, 1e7):
        assert ("gamma", a) in hand and ("chi2", 2 * a) in hand
    assert {("exponpow", 0.2), ("exponpow", 40.0), ("lognorm", 0.005), ("lognorm", 3.0), ("pareto", 0.5)} <= hand
    assert sum(1 for c in cases if c[0] in ("gamma", "chi2") and c[1][0] >= 1e5) >= 10
    assert 55 <= len(cases) <= 75
    bad = [c for c in cases if c[2] == "bad shape"]
    assert {c[0] for c in bad} >= {"gamma", "chi2"} and all(np.isnan(c[4]).all() for c in bad)  # what scipy returns
    assert any(np.isnan(c[1][0]) for c in bad) and any(c[1][0] == 0 for c in bad) and any(c[1][0] < 0 for c in bad)
    for name, params, origin, cells, p in cases:
        assert cells.dtype == np.float32 and p.dtype == np.float32 and len(cells) == len(p) == 568
        assert np.isnan(cells).sum() == 1 and (origin == "bad shape" or np.isnan(p).sum() == 1)
        loc32 = np.float32(params[-2])
        assert {np.nextafter(loc32, np.float32(-np.inf)), loc32, np.nextafter(loc32, np.float32(np.inf))} <= set(cells[-6:-3])
    # exponpow b = 40 with z up to 1e8: z ** 40 is inf, the cdf is 1 and p is 0
    over = [c for c in cases if c[0] == "exponpow" and c[1][0] == 40.0 and c[1][2] < 1e-6]
    assert over and ((over[0][3].astype(np.float64) - over[0][1][1]) / over[0][1][2] > 1e8 - 1).any() and (over[0][4][:-7] == 0).sum() > 400
    g = np.load(os.path.join(golden_dir, "pvals_sweep.npz"))
    assert str(g["scipy_version"])[0].isdigit()
    assert os.path.getsize(os.path.join(golden_dir, "pvals_sweep.npz")) <= os.path.getsize(os.path.join(golden_dir, "pvals_common10.npz"))


def test_gamma_port_meets_the_bar_within_the_term_bound():
    """The kernel's incomplete gamma loops, restated in host float64 (sweep.gamma_p_port), on the fixture's gamma and chi2
    cases up to shape 2e4 (every third cell; the larger shapes take minutes in Python and are the device test's): they
    converge within gamma_max_terms and meet the bar, and with the 2 000 terms the kernel used to stop at the count at
    shape 1e7 is far from done."""
    worst_use = 0.0
    for name, params, origin, cells, want in sweep.fixture_cases():
        a = params[0] / 2 if name == "chi2" else params[0]
        if name not in ("gamma", "chi2") or origin == "bad shape" or a > 2e4:
            continue
        bound = sweep.gamma_max_terms(a)
        for x, w in list(zip(cells.astype(np.float64), want.astype(np.float64)))[::3]:
            if np.isnan(x):
                continue
            z = (x - params[1]) / params[2]
            p, used, converged = sweep.gamma_p_port(a, z / 2 if name == "chi2" else z, bound)
            assert converged, (name, params, x)
            worst_use = max(worst_use, used / bound)
            assert abs(float(np.float32(1.0 - p)) - w) <= sweep.RTOL * abs(w) + sweep.ATOL, (name, params, x, 1.0 - p, w)
    assert 0.3 < worst_use < 0.75, worst_use  # the bound is neither tight nor idle
    assert sweep.gamma_max_terms(1e7) == 38147
    _, used, converged = sweep.gamma_p_port(1e7, 1e7, 2000)
    assert not converged and used == 2000
