"""seekr_amd.distribution on the host: the numpy models (tests/distribution_model.py) against np.sort and np.histogram,
the package's descent driven by the model's histogram pass, the rank rules in exact arithmetic, argument errors and the
command's entry point.  No device call is made here."""
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

import distribution_model as dm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def random_sets():
    """20 sets with ties, NaN of both signs, +-inf, +-0 and subnormals."""
    rng = np.random.default_rng(20260)
    special = np.array([0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x7fc00000, 0xffc00000, 0x00000001, 0x80000001,
                        0x7f7fffff, 0xff7fffff, 0x7f800001], dtype=np.uint32).view(np.float32)
    sets = []
    for i in range(20):
        n = int(rng.integers(1, 4000))
        x = rng.normal(0, 0.05 * (1 + i), n).astype(np.float32)
        x = np.round(x, 2) if i % 3 == 0 else x                        # ties
        x[rng.integers(0, n, n // 7)] = rng.choice(special, n // 7)    # the special values
        if np.isnan(x).all():
            x[0] = 1.0
        sets.append(x)
    return sets


SETS = random_sets()


def sorted_by_key(x):
    """The non-NaN values in key order: np.sort, with -0 put below +0 (np.sort leaves equal values in any order)."""
    x = np.asarray(x, np.float32).reshape(-1)
    return dm.unkey(np.sort(dm.key(x[~np.isnan(x)])))


def test_key_is_the_order_of_the_values_and_of_significant_key():
    from seekr_amd import significant
    for x in SETS[:5]:
        v = x[~np.isnan(x)]
        k = dm.key(v)
        assert [int(t) for t in k[:50]] == [significant._key(t) for t in v[:50]]
        assert (bits(dm.unkey(k)) == bits(v)).all()
        order = np.argsort(k, kind="stable")
        assert (v[order][1:] >= v[order][:-1]).all()
    assert dm.key(np.float32(-0.0)) + 1 == dm.key(np.float32(0.0))


def test_descent_of_the_model_is_the_sort():
    rng = np.random.default_rng(3)
    for x in SETS:
        want = sorted_by_key(x)
        m = len(want)
        ranks = sorted({0, m - 1, m // 2, *rng.integers(0, m, 5).tolist()})
        got, total = dm.order_statistics(x, ranks)
        assert total == m
        assert (bits(got) == bits(want[ranks])).all()
        assert (got == np.sort(x[~np.isnan(x)])[ranks]).all()  # as values, np.sort's own answer


def test_edge_rule_is_np_histogram():
    for i, x in enumerate(SETS):
        v = x[np.isfinite(x)]
        for edges in (np.linspace(-0.3, 0.3, 17, dtype=np.float32), np.array([v.min(), v.max() + 1], np.float32),
                      np.sort(np.unique(v))[:min(len(np.unique(v)), 4097)] if len(np.unique(v)) > 1 else np.float32([0, 1])):
            hist, below, above, nan = dm.edge_hist(x, edges)
            assert (hist == np.histogram(v.astype(np.float32), bins=edges)[0].astype(np.uint64)).all(), i
            assert below == int((x < edges[0]).sum()) and above == int((x > edges[-1]).sum()) and nan == int(np.isnan(x).sum())
            assert int(hist.sum()) + below + above + nan == len(x)
    hist, below, above, nan = dm.edge_hist(np.float32([1, 2, 2, 3, 3, 3, np.nan]), np.float32([1, 2, 3]))
    assert hist.tolist() == [1, 5] and (below, above, nan) == (0, 0, 1)  # the last bin is closed on the right


@pytest.mark.parametrize("n_ranks", [1, 8, 9])
def test_package_descent_driven_by_the_model_pass(n_ranks):
    from seekr_amd import distribution
    assert distribution.DIGITS == dm.DIGITS and distribution.MAX_PREFIXES == dm.MAX_PREFIXES
    rng = np.random.default_rng(n_ranks)
    for x in SETS[:8]:
        want = sorted_by_key(x)
        m = len(want)
        ranks = rng.integers(0, m, n_ranks).tolist()
        if n_ranks > 1:
            ranks[1] = ranks[0]                       # a duplicate rank
            ranks[-1] = min(ranks[0] + 1, m - 1)      # a neighbour: shares its prefix unless it crosses a bin
        calls = []

        def one_pass(shift, nbits, prefixes, prefix_bits):
            calls.append((shift, nbits, len(prefixes), prefix_bits))
            assert len(prefixes) <= dm.MAX_PREFIXES and len(set(prefixes)) == len(prefixes)
            return dm.hist_pass(x, shift, nbits, prefixes, prefix_bits)

        got, total = distribution.descend(ranks, one_pass)
        assert total == m and got.dtype == np.float32
        assert (bits(got) == bits(want[ranks])).all()
        assert calls[0] == (20, 12, 1, 0)
        assert {c[:2] + c[3:] for c in calls} == {(20, 12, 0), (10, 10, 12), (0, 10, 22)}
        assert len(calls) <= 3 if n_ranks <= 8 else len(calls) <= 5
    # ranks as a function of M: asked once, after the first pass
    got, total = distribution.descend(lambda m: [m - 1, 0], lambda *a: dm.hist_pass(SETS[0], *a))
    assert (bits(got) == bits(sorted_by_key(SETS[0])[[-1, 0]])).all()


def test_nine_distinct_prefixes_go_in_two_batches():
    from seekr_amd import distribution
    x = np.linspace(-1, 1, 5001, dtype=np.float32)
    ranks = list(range(0, 5001, 556))[:9]
    sizes = []

    def one_pass(shift, nbits, prefixes, prefix_bits):
        sizes.append(len(prefixes))
        return dm.hist_pass(x, shift, nbits, prefixes, prefix_bits)

    got, _ = distribution.descend(ranks, one_pass)
    assert (got == x[ranks]).all()
    assert sizes[0] == 1 and 9 in (sizes[1] + sizes[2], ) and sizes[1] == 8 and sizes[2] == 1


@pytest.mark.parametrize("m", [1, 2, 3, 7, 1000, 10 ** 12 + 1])
def test_rank_rules(m):
    from seekr_amd import distribution as d
    assert d.quantile_rank(0, m) == 0 and d.quantile_rank(1, m) == m - 1
    assert d.quantile_rank(0.5, m) == dm.quantile_rank(0.5, m) == (m - 1) // 2
    assert d.quantile_rank(Fraction(1, 3), m) == (m - 1) // 3 and d.quantile_rank("1/3", m) == (m - 1) // 3
    assert d.density_rank(1, m) == 0 and d.density_rank(Fraction(1, 10 ** 15), m) == m - 1
    assert d.density_rank(Fraction(1, 2), m) == m - max(1, m // 2) == dm.density_rank(Fraction(1, 2), m)
    if m <= 1000:  # np.quantile's own arithmetic, where it is exact: q in {0, 1}, and 0.5 at odd M
        x = np.arange(m, dtype=np.float32)
        for q in (0, 1) + ((0.5,) if m % 2 else ()):
            assert x[d.quantile_rank(q, m)] == np.quantile(x, q, method="lower")


def test_order_statistics_at_one_and_two_cells():
    from seekr_amd import distribution
    for x in (np.float32([0.25]), np.float32([0.5, -0.0]), np.float32([np.nan, 3, 3])):
        m = int((~np.isnan(x)).sum())
        got, total = distribution.descend([0, m - 1], lambda *a: dm.hist_pass(x, *a))
        assert total == m and (bits(got) == bits(sorted_by_key(x)[[0, m - 1]])).all()


def test_argument_errors():
    from seekr_amd import distribution as d
    x = np.float32([1, 2, 3, np.nan])
    one_pass = lambda *a: dm.hist_pass(x, *a)  # noqa: E731
    for bad in ([3], [-1], [0, 5]):
        with pytest.raises(ValueError, match="outside"):
            d.descend(bad, one_pass)
    with pytest.raises(ValueError, match="integer"):
        d.descend([0.5], one_pass)
    for q in (-0.1, 1.5):
        with pytest.raises(ValueError, match="quantile"):
            d.quantile_rank(q, 10)
    for dens in (0, -1, 1.01):
        with pytest.raises(ValueError, match="density"):
            d.density_rank(dens, 10)
    with pytest.raises(ValueError):
        d.quantile_rank(0.5, 0)
    for edges in ([1.0], [1, 1], [2, 1], [0, np.inf], [0, np.nan, 1], np.arange(4098), [1, 1 + 1e-9]):
        with pytest.raises(ValueError, match="edge"):
            d.check_edges(edges)
    assert d.check_edges(np.arange(4097)).dtype == np.float32
    with pytest.raises(ValueError):
        d.make_edges(None, None, None)
    with pytest.raises(ValueError):
        d.make_edges([0, 1], 3, (0, 1))
    with pytest.raises(ValueError):
        d.make_edges(None, 0, (0, 1))
    e = d.make_edges(None, 200, (-1, 1))
    assert e.dtype == np.float32 and (bits(e) == bits(np.linspace(np.float32(-1), np.float32(1), 201, dtype=np.float32))).all()
    with pytest.raises(ValueError, match="2-D"):
        d.pearson_distribution(np.zeros(5), q=[0.5])
    with pytest.raises(ValueError, match="same number of columns"):
        d.pearson_distribution(np.zeros((3, 4)), np.zeros((3, 5)), q=[0.5])
    with pytest.raises(ValueError, match="no cell"):
        d.pearson_distribution(np.zeros((1, 4)), q=[0.5])


def test_kmer_leiden_density_arguments():
    from seekr_amd.kmer_leiden import kmer_leiden
    with pytest.raises(ValueError, match="not both"):
        kmer_leiden("x.fa", "m.npy", "s.npy", 4, pearsoncutoff=0.1, density=0.01)
    for bad in (0, 1.5):
        with pytest.raises(ValueError, match="density"):
            kmer_leiden("x.fa", "m.npy", "s.npy", 4, density=bad)


def test_command_help_and_entry_point():
    code = ("import sys; sys.argv = ['seekr_r_distribution', '-h']; "
            "from seekr_amd.console_scripts import console_r_distribution; console_r_distribution()")
    proc = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert proc.returncode == 0, proc.stderr
    for flag in ("--bins", "--range", "--quantiles", "--density", "--outfile", "--binary_input"):
        assert flag in proc.stdout
    code = "import sys; sys.argv = ['seekr_kmer_leiden', '-h']; from seekr_amd.console_scripts import console_kmer_leiden; console_kmer_leiden()"
    proc = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert proc.returncode == 0 and "--density" in proc.stdout, proc.stderr
    with open(os.path.join(ROOT, "setup.py")) as f:
        assert "seekr_r_distribution = seekr_amd.console_scripts:console_r_distribution" in f.read()
