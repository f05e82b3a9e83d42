"""The host side of find_dist and find_pval, without a GPU: the triangle's rank arithmetic, the draw, the model list, the
fitting loop against the reference's loop around the same scipy calls, the two CSV forms, and find_pval's length check
(which comes before any device call) against the table recorded from the reference."""
import os

import numpy as np
import pytest

import find_dist_cases as fc
from seekr_amd import consumers, find_dist, find_pval

GOLD = fc.text()


@pytest.mark.parametrize("n", [2, 3, 5, 17, 300])
def test_unrank_and_rank_against_triu_indices(n):
    i, j = np.triu_indices(n, 1)
    got_i, got_j = consumers.triu_unrank(np.arange(len(i)), n)
    assert got_i.dtype == np.int64 and got_j.dtype == np.int64
    assert np.array_equal(got_i, i) and np.array_equal(got_j, j)
    assert np.array_equal(consumers.triu_rank(i, j, n), np.arange(len(i)))


@pytest.mark.parametrize("n", [200_000, 2 ** 31 - 1])
def test_unrank_and_rank_at_large_n(n):
    cells = n * (n - 1) // 2
    edge = []
    for row in (0, 1, n - 3, n - 2):
        start = fc.exact_rank(row, row + 1, n)
        edge += [start, fc.exact_rank(row, n - 1, n)]
    assert edge[0] == 0 and edge[-1] == cells - 1
    index = np.array(edge + [int(v) for v in np.random.default_rng(n % 1000).integers(0, cells, 1000)], dtype=np.int64)
    got_i, got_j = consumers.triu_unrank(index, n)
    want = [fc.exact_unrank(v, n) for v in index.tolist()]
    assert got_i.tolist() == [w[0] for w in want] and got_j.tolist() == [w[1] for w in want]
    assert consumers.triu_rank(got_i, got_j, n).tolist() == index.tolist()
    with pytest.raises(IndexError):
        consumers.triu_unrank([cells], n)


def test_unrank_refuses_more_than_int31_rows():
    with pytest.raises(ValueError):
        consumers.triu_unrank([0], 2 ** 31)
    with pytest.raises(ValueError):
        consumers.triu_rank([0], [1], 2 ** 31)


@pytest.mark.parametrize("seed,n,size", [(0, 10, 3), (3, 780, 200), (7, 5000, 5000), (11, 100_000, 1)])
def test_draw_is_the_legacy_choice(seed, n, size):
    np.random.seed(seed)
    want = np.random.choice(np.arange(n), size, replace=False)
    np.random.seed(seed)
    got = consumers.draw_index(n, size)
    assert got.dtype == np.int64 and np.array_equal(got, want)
    values = np.random.default_rng(seed).standard_normal(n).astype(np.float32)
    np.random.seed(seed)
    assert np.array_equal(values[got], np.random.choice(values, size, replace=False))


def test_draw_above_the_legacy_limit(monkeypatch):
    monkeypatch.setattr(consumers, "LEGACY_DRAW_MAX_CELLS", 1000)
    n = 10 ** 6
    np.random.seed(5)
    first = consumers.draw_index(n, 5000)
    assert first.dtype == np.int64 and len(first) == 5000 and len(np.unique(first)) == 5000
    assert first.min() >= 0 and first.max() < n
    np.random.seed(5)
    assert np.array_equal(consumers.draw_index(n, 5000), first)
    np.random.seed(6)
    assert not np.array_equal(consumers.draw_index(n, 5000), first)
    a = consumers.draw_index(500, 20, rng=np.random.default_rng(1))  # a Generator is used as such at any size
    assert np.array_equal(a, np.random.default_rng(1).choice(500, 20, replace=False))


def test_resolve_models_against_the_reference():
    assert find_dist.resolve_models("common10") == find_dist.COMMON10
    tail = find_dist.SUBSET_TOO_LARGE + "\n"  # the golden text goes on to the sampling step
    names, out = fc.captured(find_dist.resolve_models, GOLD["models_invalid"])
    assert names == ["norm", "expon"] and out + tail == GOLD["models_invalid_stdout"]
    names, out = fc.captured(find_dist.resolve_models, GOLD["models_discrete"])
    assert names == ["norm", "gamma"] and out + tail == GOLD["models_discrete_stdout"]
    names, out = fc.captured(find_dist.resolve_models, "all")
    assert out == "" and "norm" in names and "levy_stable" not in names and "poisson" not in names and len(names) > 80


@pytest.mark.parametrize("statsmethod", ["ks", "mse", "aic", "bic"])
def test_fit_distributions_is_the_reference_loop(statsmethod):
    sample, names = fc.fit_sample(), ["norm", "expon", "uniform", "gamma"]
    np.random.seed(17)
    want = fc.reference_loop(sample, names, statsmethod)
    np.random.seed(17)
    got = find_dist.fit_distributions(sample, names, statsmethod, False)
    assert [g[0] for g in got] == [w[0] for w in want] and sorted(g[0] for g in got) == sorted(names)
    for g, w in zip(got, want):
        assert g[1] == w[1] and g[2] == w[2], (g, w)
    assert [g[1] for g in got] == sorted(g[1] for g in got)


def test_unknown_statsmethod_falls_back_to_ks():
    sample, names = fc.fit_sample(), ["norm", "uniform"]
    got, out = fc.captured(find_dist.fit_distributions, sample, names, "nope", False)
    assert out == (find_dist.BAD_STATSMETHOD + "\n") * len(names)
    assert got == find_dist.fit_distributions(sample, names, "ks", False)


def test_a_distribution_that_cannot_be_fitted_is_excluded():
    sample = np.full(50, np.nan, np.float32)
    got, out = fc.captured(find_dist.fit_distributions, sample, ["norm", "gamma"], "ks", False)
    assert len(got) + out.count("excluding it from the results") == 2 and "Could not fit gamma because" in out


def test_fitted_csv_reads_back(tmp_path):
    results = [("gamma", np.float64(0.012345678901234567), (np.float64(2.5), np.float32(-0.1), 3e-310)),
               ("norm", 0.5, (np.float64(-1.25e-7), 1.0)), ("expon", np.float32(0.75), (0.1 + 0.2, np.float64(1e300)))]
    plain = [(n, float(d), tuple(float(p) for p in ps)) for n, d, ps in results]
    path = str(tmp_path / "fits.csv")
    find_dist.write_fit_csv(path, results)
    text = open(path).read()
    assert "np.float" not in text and text.splitlines()[0] == "distribution_name,D_statistics,params"
    assert find_dist.read_fit_csv(path) == plain
    wrapped = str(tmp_path / "wrapped.csv")  # what numpy 2 makes of the reference's own file
    with open(wrapped, "w") as fh:
        fh.write("distribution_name,D_statistics,params\n")
        for n, d, ps in results:
            cells = ", ".join("np.{}({!r})".format(type(p).__name__ if isinstance(p, np.floating) else "float64", float(p))
                              for p in ps)
            fh.write('{},{!r},"({})"\n'.format(n, float(d), cells))
    assert "np.float32(" in open(wrapped).read() and "np.float64(" in open(wrapped).read()
    assert find_dist.read_fit_csv(wrapped) == plain
    one = str(tmp_path / "one.csv")  # a one-parameter tuple has a trailing comma
    find_dist.write_fit_csv(one, [("x", 1.0, (2.0,))])
    assert find_dist.read_fit_csv(one) == [("x", 1.0, (2.0,))]


def test_sample_csv_is_savetxt(tmp_path):
    from seekr_amd import _lib
    sample = np.concatenate([fc.arrays()["sample200"], np.array([0.0, -0.0, 1.0, -1.0, 1e-30, np.nan], np.float32)])
    np.savetxt(str(tmp_path / "want.csv"), sample, delimiter=",")
    _lib.save_csv(str(tmp_path / "got.csv"), sample.reshape(-1, 1), fmt=_lib.FMT_SCI18)
    assert open(str(tmp_path / "got.csv"), "rb").read() == open(str(tmp_path / "want.csv"), "rb").read()
    assert np.array_equal(np.loadtxt(str(tmp_path / "got.csv"), delimiter=",").astype(np.float32)[:200], sample[:200])


@pytest.mark.parametrize("row", GOLD["length_check"], ids=lambda r: "{}-{}".format(r["mean_len"], r["std_len"]))
def test_length_check_is_the_reference_line(row, tmp_path, monkeypatch):
    assert find_pval.lengths_refused(row["mean_len"], row["std_len"], fc.K) == row["refused"]
    if not row["refused"]:
        return
    gold = fc.arrays()
    mean, std = str(tmp_path / "m.npy"), str(tmp_path / "s.npy")
    np.save(mean, np.resize(gold["bkg_mean"], row["mean_len"]))
    np.save(std, np.resize(gold["bkg_std"], row["std_len"]))

    def no_device(*a, **k):
        raise AssertionError("the length check comes before anything is counted")
    monkeypatch.setattr(find_pval, "BasicCounter", no_device)
    res, out = fc.captured(find_pval.find_pval, "a.fa", "b.fa", mean, std, fc.K, "other type", progress_bar=False)
    assert res is None and out == row["stdout"]


def test_refusal_sentences_are_the_reference_text():
    lines = {k: v["stdout"].splitlines() for k, v in GOLD["refused"].items()}
    dup = [find_pval.NOT_UNIQUE.format(1), find_pval.NOT_UNIQUE_2]
    assert lines["list_wrong_format"] == dup + list(find_pval.BAD_LIST) == lines["list_not_tuples"]
    assert lines["array_2d"] == dup + list(find_pval.BAD_ARRAY)
    assert lines["other_type"] == dup + list(find_pval.BAD_TYPE)
    assert not find_pval.fitres_list_ok(fc.BAD_FITRES["list_wrong_format"])
    assert not find_pval.fitres_list_ok(fc.BAD_FITRES["list_not_tuples"])
    assert find_pval.fitres_list_ok([("norm", np.float64(0.1), (np.float32(0.0), 1.0))])


def test_commands_are_registered():
    from seekr_amd import console_scripts
    setup = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "setup.py")).read()
    for name in ("find_dist", "find_pval"):
        assert callable(getattr(console_scripts, "console_" + name))
        assert "seekr_{0} = seekr_amd.console_scripts:console_{0}".format(name) in setup


def test_default_background_is_refused():
    with pytest.raises(FileNotFoundError) as err:
        fc.captured(find_dist.find_dist, "default", fit_model=False)
    assert os.path.join("seekr_amd", "data", find_dist.DEFAULT_FASTA) in str(err.value)
