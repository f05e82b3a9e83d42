"""The host side of significant_pairs, without a GPU: the truncation argument behind consumers.adjust_pvalues_head in numpy
(tests/adj_rule.py against tests/significant_cases.head_correct), the cutoff search against numpy p-functions, the
conditions the GPU fixture must meet so that tests/test_gpu_significant.py cannot pass on an empty list, the argument
checks that run before any device call, and the command's help and setup.py entry."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import adj_rule
import significant_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALPHAS = (0.01, 0.05, 0.2)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def bound_for(alpha, dtype):
    """The selection bound in p's precision: alpha32 for float32 p-values, alpha for float64 ones."""
    return float(sc.alpha32(alpha)) if np.dtype(dtype) == np.float32 else alpha


def vectors(count, seed):
    rng = np.random.default_rng(seed)
    for v in range(count):
        n = int(rng.integers(3, 4001)) if v % 4 else int(rng.integers(3, 40))
        dtype = (np.float32, np.float64)[v % 2]
        yield sc.tied_pvalues(rng, n, dtype, small=(0.05, 0.3, 0.9)[v % 3])


# ---- the truncation argument ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", sc.HEAD_METHODS)
def test_values_at_or_below_alpha_come_from_the_prefix_alone(method):
    """correct(p) on all tests against the same formulas on the p <= alpha prefix with the full test count: the cells
    <= alpha are equal bit for bit, the same cells, and no cell with p above the bound is corrected to <= alpha."""
    compared = 0
    for p in vectors(300, 5):
        for alpha in ALPHAS:
            with np.errstate(all="ignore"):
                full = adj_rule.correct(p, method, alpha).astype(np.float64)
            head = p <= bound_for(alpha, p.dtype)
            assert not (full[~head] <= alpha).any(), (method, alpha, len(p))
            if not head.any():
                continue
            with np.errstate(all="ignore"):
                got = sc.head_correct(p[head], len(p), method).astype(np.float64)
            sig = full[head] <= alpha
            assert np.array_equal(got <= alpha, sig), (method, alpha, len(p))
            assert np.array_equal(bits(got[sig]), bits(full[head][sig])), (method, alpha, len(p))
            compared += int(sig.sum())
    assert compared > 1000, compared  # not vacuous: bonferroni, the strictest, still compares thousands of cells


def test_head_of_everything_is_the_whole_correction():
    rng = np.random.default_rng(6)
    for dtype in (np.float32, np.float64):
        p = sc.tied_pvalues(rng, 777, dtype)
        for method in sc.HEAD_METHODS:
            want = adj_rule.correct(p, method).astype(np.float64)
            assert np.array_equal(bits(sc.head_correct(p, len(p), method).astype(np.float64)), bits(want)), method


def _naive_head(p, ntests, method, alpha):
    """What "the same formulas on the prefix with the full test count" gives a refused method: n replaced where it is
    written as the number of tests; hommel's formula has no such n (every m from the array length down is one)."""
    s = np.sort(p)
    n, e = int(ntests), len(s)
    ii = np.arange(1, e + 1)
    if method == "hommel":
        return adj_rule._sorted(s, "hommel", alpha)
    if method == "fdr_gbs":
        q = (n + 1. - ii) / ii * s / (1. - s)
        return np.minimum.accumulate(np.maximum.accumulate(q)[::-1])[::-1]
    c = sc._head_sorted(s, n, "fdr_bh")
    bky = method == "fdr_tsbky"
    fact = (1. + alpha) if bky else 1.
    reject = s <= (ii / float(n)) * (alpha / fact)
    r1 = int(np.nonzero(reject)[0].max()) + 1 if reject.any() else 0
    if r1 == 0 or r1 == n:
        return c * fact
    c = c * ((1.0 * n - r1) / n)
    return c * (1. + alpha) if bky else c


REFUSED_VECTORS = {
    # the first stage's rejections shrink every value: tests above alpha come out below it
    "fdr_tsbh": [0.001, 0.002, 0.03, 0.04] + [0.051] * 6,
    "fdr_tsbky": [0.001, 0.002, 0.03, 0.04] + [0.051] * 6,
    # (n + 1 - i) / i falls to 1 / n at the last test: a p-value of 0.06 is corrected to 0.0064
    "fdr_gbs": [1e-6] * 9 + [0.06],
    # the definition walks m = n .. 2 over ALL tests; on the prefix it is the correction of four tests, not of ten
    "hommel": [0.001, 0.002, 0.03, 0.04] + [0.99] * 6,
}


@pytest.mark.parametrize("method", sc.REFUSED)
def test_refused_methods_break_the_equality(method):
    alpha = 0.05
    p = np.array(REFUSED_VECTORS[method])
    full = adj_rule.correct(p, method, alpha)
    head = p <= alpha
    above_comes_out_below = bool((full[~head] <= alpha).any())
    naive = np.minimum(_naive_head(p[head], len(p), method, alpha), 1.0)
    in_order = full[head][np.argsort(p[head], kind="stable")]  # naive is in sorted order
    sig = in_order <= alpha
    values_differ = not np.array_equal(naive[sig], in_order[sig])
    assert above_comes_out_below or values_differ, method
    if method in ("fdr_tsbh", "fdr_tsbky", "fdr_gbs"):
        assert above_comes_out_below
    else:
        assert values_differ
    # the same vector does not break a supported method
    for ok in sc.HEAD_METHODS:
        whole = adj_rule.correct(p, ok, alpha)
        assert not (whole[~head] <= alpha).any()
        keep = whole[head] <= alpha
        assert np.array_equal(sc.head_correct(p[head], len(p), ok)[keep], whole[head][keep]), (method, ok)


# ---- the cutoff search --------------------------------------------------------------------------------------------------
def test_cutoff_of_a_step_function():
    from seekr_amd import significant as sg
    a32 = sc.alpha32(0.05)
    for edge in (0.125, 0.3, 1e-3, 1.9999, 2.0, np.float32(0.1), 0.7071067811865476):
        calls = []

        def p_of(r, edge=edge, calls=calls):
            calls.append(len(r))
            return np.where(r.astype(np.float64) >= edge, np.float32(0.01), np.float32(0.5)).astype(np.float32)

        r_star = sg.find_cutoff(p_of, a32)
        assert r_star.dtype == np.float32 and r_star == sc.ceil_float32(np.array([edge]))[0], edge
        assert len(calls) <= 34 and set(calls) == {1}  # 32 bisection steps and the two ends, one value each
        assert sg.float32_steps(r_star, -sg.GUARD_STEPS) == sg.cutoff_with_guard(r_star) < r_star
    # p equal to the bound passes; one float32 above it does not
    at = lambda r: np.where(r >= 0.5, a32, np.nextafter(a32, np.float32(1))).astype(np.float32)  # noqa: E731
    assert sg.find_cutoff(at, a32) == np.float32(0.5)


def test_cutoff_of_a_normal_tail():
    from seekr_amd import significant as sg
    a32 = sc.alpha32(0.05)
    sf = lambda r: np.array([0.5 * math.erfc(float(x) / sc.SD / math.sqrt(2.0)) for x in r], dtype=np.float32)  # noqa: E731
    r_star = sg.find_cutoff(sf, a32)
    below = sg.float32_steps(r_star, -1)
    assert sf([r_star])[0] <= a32 < sf([below])[0]
    assert abs(float(r_star) - 1.6448536 * sc.SD) < 1e-6


def test_cutoff_without_an_answer():
    from seekr_amd import significant as sg
    a32 = sc.alpha32(0.05)
    assert sg.find_cutoff(lambda r: np.full(len(r), np.nan, np.float32), a32) is None       # NaN everywhere
    assert sg.find_cutoff(lambda r: np.full(len(r), 0.5, np.float32), a32) is None          # no crossing
    r_star = sg.find_cutoff(lambda r: np.where(r >= -0.25, 0.01, 0.5).astype(np.float32), a32)  # a crossing below 0
    assert r_star == np.float32(-0.25)
    with pytest.raises(ValueError, match="not positive"):
        sg.cutoff_with_guard(r_star)
    with pytest.raises(ValueError, match="not positive"):  # 64 steps above zero is still zero or less after the guard
        sg.cutoff_with_guard(sg.float32_steps(np.float32(0), 64))
    assert sg.cutoff_with_guard(sg.float32_steps(np.float32(0), 66)) > 0
    assert sg.find_cutoff(lambda r: np.zeros(len(r), np.float32), a32) == np.float32(-2)    # significant everywhere


def test_float32_ordering():
    from seekr_amd import significant as sg
    xs = np.array([-2, -1, -1e-30, -0.0, 0.0, 1e-45, 1e-30, 0.05, 1, 2], dtype=np.float32)
    keys = [sg._key(x) for x in xs]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    for x in xs:
        assert bits(np.array([sg._unkey(sg._key(x))]))[0] == bits(np.array([x]))[0]
    assert sg.float32_steps(np.float32(1), 1) == np.nextafter(np.float32(1), np.float32(2))
    assert sg.float32_steps(np.float32(1), -64) == np.float32(1) - np.float32(64 * 2.0 ** -24)
    assert sg.alpha_float32(0.05) >= 0.05 > np.nextafter(sg.alpha_float32(0.05), np.float32(0))
    assert sg.alpha_float32(0.25) == 0.25


# ---- the data fixture of the GPU file -------------------------------------------------------------------------------------
def test_fixture_cannot_pass_on_an_empty_list():
    from oracle import seekr_oracle as orc
    x = sc.planted_counts()
    assert x.shape == (300, 256) and x.dtype == np.float32
    r = orc.pearson(x.astype(np.float64), x.astype(np.float64)).astype(np.float32)
    iu = np.triu_indices(300, 1)
    tests = r[iu]
    for name in ("empirical_f32", "empirical_f64"):
        bg = sc.backgrounds()[name]
        assert bg.shape == (10000,) and bg.dtype == (np.float32 if name == "empirical_f32" else np.float64)
        p = sc.empirical_p(tests, bg)
        for alpha in (0.05,):
            candidates = int((p <= sc.alpha32(alpha)).sum())
            assert candidates < len(tests) // 2, (name, candidates)
            bh = adj_rule.correct(p, "fdr_bh", alpha)
            assert int((bh <= alpha).sum()) >= 100, (name, int((bh <= alpha).sum()))
            assert int((bh <= alpha).sum()) < candidates  # the correction does remove pairs
            assert int((adj_rule.correct(p, "bonferroni", alpha) <= alpha).sum()) >= 1, name
    two = sc.backgrounds()["empirical_f32"]
    assert len(np.unique(two)) < 100 and np.array_equal(two, np.round(two, 2).astype(np.float32))  # long tie runs
    assert np.quantile(two, 0.95) > 64 * 2.0 ** -24  # the alpha quantile is positive: r0 > 0


# ---- arguments refused before any device call ---------------------------------------------------------------------------
def test_arguments_are_checked_first():
    from seekr_amd import consumers
    from seekr_amd import significant as sg
    x = sc.planted_counts()[:5]
    fit = sc.backgrounds()["norm"]
    for method in sc.REFUSED + ["ho", "fdr_twostage"]:
        with pytest.raises(NotImplementedError) as err:
            sg.significant_pairs(x, fit, method=method)
        assert all(name in str(err.value) for name in sc.REFUSED)
    with pytest.raises(ValueError, match="method not recognized"):
        sg.significant_pairs(x, fit, method="nonsense")
    for alpha in (0, 1, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="alpha"):
            sg.significant_pairs(x, fit, alpha=alpha)
    with pytest.raises(IndexError):
        sg.significant_pairs(x, fit, bestfit=2)
    assert consumers.HEAD_METHODS == tuple(sc.HEAD_METHODS) and consumers.HEAD_REFUSED == tuple(sc.REFUSED)
    assert sorted(consumers.HEAD_METHODS + consumers.HEAD_REFUSED) == sorted(adj_rule.METHODS)


# ---- the command ----------------------------------------------------------------------------------------------------------
def test_command_help_and_entry_point():
    code = ("import sys; sys.argv = ['seekr_significant_pairs', '-h']; "
            "from seekr_amd.console_scripts import console_significant_pairs; console_significant_pairs()")
    proc = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert proc.returncode == 0, proc.stderr
    for word in ("row,col,r,p,p_adj", "-bg", "-bi", "--method", "--alpha", "--params", "fdr_bh"):
        assert word in proc.stdout, word
    with open(os.path.join(ROOT, "setup.py")) as f:
        setup = f.read()
    assert "seekr_significant_pairs = seekr_amd.console_scripts:console_significant_pairs" in setup
