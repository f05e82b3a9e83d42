"""consumers.pearson_sample, find_dist, find_pval and their commands on the device.

pearson_sample's specification is the r that Sweep(a, b, stripe_rows, panel_rows) itself makes — every block downloaded
into a host matrix by a visitor, with the same split as the call (a block need not carry the bits of the whole-matrix
call: tests/test_gpu_neighbors.py::test_blocks_against_the_whole_matrix_call) — and the comparison is bit for bit, in the
order of the index.  find_dist is compared with the reference's recorded sample (tests/golden/find_dist.npz) under the
parity rule of the fuzzers, and bit for bit with this package's own full-matrix composition."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import find_dist_cases as fc
import neighbors_cases as nc
import parity_rule

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ctx():
    from seekr_amd import _lib
    return _lib.default_context()


def prepared(ctx, x):
    from seekr_amd import _lib
    from seekr_amd import pearson as pearson_mod
    return _lib.operand_fill(ctx, ctx.from_numpy(x), None, pearson_mod._precision_for(np.dtype(np.float32), True))[0]


def swept_r(a, b, stripe_rows, panel_rows):
    """The cells Sweep(a, b, stripe_rows, panel_rows) makes, as a host matrix of bits (cells it never makes: 0xFFFFFFFF)."""
    from seekr_amd import consumers
    r = np.full((a.rows, (a if b is None else b).rows), 0xFFFFFFFF, dtype=np.uint32)

    def visit(buf, nrows, col_begin, col_end, row_global0, col_global0, upper_only):
        block = np.array(buf.to_numpy(0, nrows))[:, col_begin:col_end]
        r[row_global0:row_global0 + nrows, col_global0:col_global0 + col_end - col_begin] = block.view(np.uint32)

    with consumers.Sweep(a, b, stripe_rows, panel_rows) as sweep:
        sweep.run(visit)
    return r


@functools.lru_cache(maxsize=None)
def self_case():
    ctx = _ctx()
    x = nc.kmer_profiles(300, 3, 23)
    return x, prepared(ctx, x)


@pytest.mark.parametrize("split", [(128, 96), (300, None), (77, 101)])
def test_pearson_sample_self(split):
    from seekr_amd import consumers
    _, z = self_case()
    n = z.rows
    cells = n * (n - 1) // 2
    assert cells == 44_850
    spec = swept_r(z, None, *split)
    rng = np.random.default_rng(split[0])
    every = rng.permutation(cells)
    for index in (every, every[:500], np.concatenate([every[:7], every[:7]])):  # the last one: duplicates are served
        i, j = consumers.triu_unrank(index, n)
        got = consumers.pearson_sample(z, None, index, stripe_rows=split[0], panel_rows=split[1])
        assert got.dtype == np.float32 and got.shape == (len(index),)
        assert np.array_equal(fc.bits(got), spec[i, j])
    assert not np.any(spec[np.triu_indices(n, 1)] == 0xFFFFFFFF)


@pytest.mark.parametrize("split", [(20, 96), (37, None)])
def test_pearson_sample_two_sets(split):
    from seekr_amd import consumers
    x, z = self_case()
    a = prepared(_ctx(), np.ascontiguousarray(x[100:137] + np.float32(0.25) * x[5:42]))
    try:
        spec = swept_r(a, z, *split)
        index = np.random.default_rng(37).permutation(37 * 300)
        for idx in (index, index[:500]):
            got = consumers.pearson_sample(a, z, idx, stripe_rows=split[0], panel_rows=split[1])
            assert np.array_equal(fc.bits(got), spec[idx // 300, idx % 300])
    finally:
        a.free()


def test_pearson_sample_float32_layout(golden_dir):
    from seekr_amd import consumers
    ctx = _ctx()
    x = np.ascontiguousarray(np.load(os.path.join(golden_dir, "regress_r4_two_level_rows.npz"))["a"][:12]).copy()
    x = np.concatenate([x, np.random.default_rng(21).standard_normal((8, x.shape[1])).astype(np.float32)])
    lo, hi = float(x[0].min()), float(x[0].max())
    x[3] = lo
    x[3, 1234] = hi
    x[7] = x[2]
    z = prepared(ctx, x)
    try:
        assert z.kind == 0  # the route under test
        index = np.random.default_rng(1).permutation(190)
        for split in ((8, 7), (20, None)):
            spec = swept_r(z, None, *split)
            i, j = consumers.triu_unrank(index, 20)
            got = consumers.pearson_sample(z, None, index, stripe_rows=split[0], panel_rows=split[1])
            assert np.array_equal(fc.bits(got), spec[i, j])
    finally:
        z.free()


def test_pearson_sample_refuses_before_any_device_call(monkeypatch):
    from seekr_amd import consumers
    _, z = self_case()

    def no_sweep(*a, **k):
        raise AssertionError("no sweep for an index out of range or an empty one")
    monkeypatch.setattr(consumers, "Sweep", no_sweep)
    for bad in ([44_850], [-1], [0, 5, 44_850]):
        with pytest.raises(IndexError):
            consumers.pearson_sample(z, None, bad)
    with pytest.raises(IndexError):
        consumers.pearson_sample(z, z, [300 * 300])
    for empty in ((), [], np.empty(0, np.int64)):
        got = consumers.pearson_sample(z, None, empty)
        assert got.dtype == np.float32 and got.shape == (0,)


# ---- find_dist against the reference's recorded run ---------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def gold():
    g = fc.arrays()
    with np.errstate(all="ignore"):
        za = parity_rule.f32_rows(g["counts"]).astype(np.float64)
        g["truth"] = za @ za.T / za.shape[1]
        ref_rows = parity_rule.f32_rows(g["counts"])
        g["ref_r"] = (np.inner(ref_rows, ref_rows) / ref_rows.shape[1]).astype(np.float32)
    for v in g.values():
        v.setflags(write=False)
    return g


def judged(values, ref_values, index, what):
    """The parity rule on the cells a sample holds: values[s] and ref_values[s] are the cell triu_unrank(index[s])."""
    from seekr_amd import consumers
    g = gold()
    i, j = consumers.triu_unrank(index, fc.N_SEQS)
    assert np.array_equal(fc.bits(ref_values), fc.bits(g["ref_r"][i, j])) or np.allclose(ref_values, g["ref_r"][i, j], atol=1e-6)
    got, ref, ok = (np.zeros((fc.N_SEQS, fc.N_SEQS)) for _ in range(3))
    got[i, j], ref[i, j], ok[i, j] = values, ref_values, 1
    res = parity_rule.judge(got, ref, g["truth"], ok.astype(bool), g["counts"], g["counts"])
    print("{}: worst |got - ref| / bar = {:.4f} over {} cells, {} beyond the bar".format(
        what, res["strict_ratio"], res["n_cells"], res["n_strict_fail"]))
    assert not res["failures"], res["failures"]
    return res


@pytest.fixture()
def background(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    return fc.write_background(str(tmp_path / "bkg.fa"))


def test_find_dist_sample_against_the_reference(background):
    from seekr_amd import consumers, find_dist
    g = gold()
    np.random.seed(fc.SEED)
    sample, out = fc.captured(find_dist.find_dist, background, fc.K, subset_size=200, fit_model=False)
    assert out == fc.text()["sample200_stdout"] == ""
    for name in ("mean", "std"):
        mine = np.load("bkg_{}_{}mers.npy".format(name, fc.K))
        assert mine.dtype == g["bkg_" + name].dtype and np.array_equal(fc.bits(mine), fc.bits(g["bkg_" + name])), name
    assert sample.dtype == g["sample200"].dtype == np.float32 and sample.shape == g["sample200"].shape == (200,)
    np.random.seed(fc.SEED)
    index = consumers.draw_index(fc.N_CELLS, 200)
    judged(sample, g["sample200"], index, "200 sampled cells")


def test_find_dist_whole_triangle_against_the_reference(background):
    from seekr_amd import find_dist
    g = gold()
    np.random.seed(fc.SEED)
    sample, out = fc.captured(find_dist.find_dist, background, fc.K, subset_size=10 ** 6, fit_model=False)
    assert out == fc.text()["triangle_stdout"] == find_dist.SUBSET_TOO_LARGE + "\n"
    assert sample.dtype == np.float32 and sample.shape == g["triangle"].shape == (fc.N_CELLS,)
    judged(sample, g["triangle"], np.arange(fc.N_CELLS), "the whole triangle")
    quiet, out = fc.captured(find_dist.find_dist, background, fc.K, subsetting=False, fit_model=False)
    assert out == "" and np.array_equal(fc.bits(quiet), fc.bits(sample))


def test_find_dist_equals_the_full_matrix_composition(background):
    from seekr_amd import _lib, find_dist
    from seekr_amd.kmer_counts import BasicCounter
    from seekr_amd.pearson import pearson
    ctx = _ctx()
    np.random.seed(fc.SEED)
    sample = find_dist.find_dist(background, fc.K, subset_size=200, fit_model=False)
    z, n = find_dist.background_operand(background, fc.K)
    r = ctx.empty(n, n)
    try:
        _lib.pearson_gemm_op(ctx, z, z, r)
        triangle = np.array(r.to_numpy())[np.triu_indices(n, 1)]
    finally:
        r.free()
        z.free()
    np.random.seed(fc.SEED)
    want = np.random.choice(triangle, size=200, replace=False)
    assert np.array_equal(fc.bits(sample), fc.bits(want))
    whole = find_dist.find_dist(background, fc.K, subsetting=False, fit_model=False)
    assert np.array_equal(fc.bits(whole), fc.bits(triangle))
    # the public API's r of the same counts: the same values within the bar; the bits may differ (another call shape)
    counter = BasicCounter(background, mean="bkg_mean_3mers.npy", std="bkg_std_3mers.npy", k=fc.K, silent=True)
    counter.make_count_file()
    public = np.asarray(pearson(counter.counts, counter.counts), dtype=np.float32)[np.triu_indices(n, 1)]
    print("cells whose bits differ from pearson(counts, counts): {} of {}".format(
        int((fc.bits(public) != fc.bits(whole)).sum()), len(whole)))
    assert np.all(np.abs(whole.astype(np.float64) - public) <= parity_rule.bar_of(public.astype(np.float64)))


def test_find_dist_with_fits(background):
    from seekr_amd import find_dist
    names = ["norm", "expon", "uniform"]
    np.random.seed(11)
    sample = find_dist.find_dist(background, fc.K, subset_size=200, fit_model=False)
    np.random.seed(11)
    got, out = fc.captured(find_dist.find_dist, background, fc.K, "Log2.post", names, True, 200, True, "ks", False, "x", "fits")
    assert got == find_dist.fit_distributions(sample, names, "ks", False) and len(got) == 3
    assert out == find_dist.NO_PLOT.format("x") + "\n" and not os.path.exists("x.pdf") and not os.path.exists("x")
    plain = [(n, float(d), tuple(float(p) for p in ps)) for n, d, ps in got]
    assert find_dist.read_fit_csv("fits.csv") == plain and "np.float" not in open("fits.csv").read()
    np.random.seed(11)
    _, out = fc.captured(find_dist.find_dist, background, fc.K, subset_size=200, fit_model=False, plotfit="x", outputname="s")
    assert out == find_dist.NO_PLOT_WITHOUT_FIT + "\n" and not os.path.exists("x.pdf")
    np.savetxt("want.csv", sample, delimiter=",")
    assert open("s.csv", "rb").read() == open("want.csv", "rb").read()


# ---- find_pval ----------------------------------------------------------------------------------------------------------------
def small_fasta(path):
    with open(path, "w") as fh:
        fh.write(fc.text()["small_fasta"])
    return path


def vectors():
    g = gold()
    np.save("m.npy", g["bkg_mean"])
    np.save("s.npy", g["bkg_std"])
    return "m.npy", "s.npy"


FITRES = {
    "norm": [("gamma", 0.2, (2.0, -0.5, 0.3)), ("norm", np.float64(0.1), (np.float64(0.01), np.float32(0.12)))],
    "gamma": [("gamma", 0.2, (2.0, -0.5, 0.3))],
    "empirical": None,  # the golden sample
}


@pytest.mark.parametrize("which", sorted(FITRES))
def test_find_pval_is_the_device_step_with_labels(background, which):
    from seekr_amd import consumers, find_pval
    from seekr_amd.kmer_counts import BasicCounter
    from seekr_amd.pearson import pearson
    small = small_fasta("small.fa")
    mean, std = vectors()
    fitres = gold()["sample200"].copy() if FITRES[which] is None else FITRES[which]
    bestfit = 2 if which == "norm" else 1
    frame, out = fc.captured(find_pval.find_pval, small, background, mean, std, fc.K, fitres, bestfit=bestfit, outputname="p")
    assert out.splitlines() == [find_pval.NOT_UNIQUE.format(1), find_pval.NOT_UNIQUE_2]
    counters = [BasicCounter(f, mean=mean, std=std, k=fc.K, log2="Log2.post", silent=True) for f in (small, background)]
    for c in counters:
        c.make_count_file()
    want = consumers.pvalues_host(pearson(counters[0].counts, counters[1].counts), fitres, bestfit)
    assert frame.values.dtype == np.float32 and frame.shape == (3, fc.N_SEQS)
    assert np.array_equal(fc.bits(frame.values), fc.bits(want))
    assert list(frame.index) == ["a", "b", "a"] and list(frame.columns) == ["s{}".format(i) for i in range(fc.N_SEQS)]
    assert open("p.csv", "rb").read() == frame.to_csv().encode()
    _, out = fc.captured(find_pval.find_pval, background, small, mean, std, fc.K, fitres, bestfit=bestfit, progress_bar=False)
    assert out.splitlines() == [find_pval.NOT_UNIQUE.format(2), find_pval.NOT_UNIQUE_2]


def test_find_pval_refusals(background):
    from seekr_amd import find_pval
    small = small_fasta("small.fa")
    mean, std = vectors()
    for key, case in fc.text()["refused"].items():
        res, out = fc.captured(find_pval.find_pval, small, background, mean, std, fc.K, fc.BAD_FITRES[key], progress_bar=False)
        assert res is None and case["is_none"] and out == case["stdout"], key
    with pytest.raises(NotImplementedError, match="cauchy, chi2, expon, exponpow, gamma, lognorm, norm, pareto, rayleigh, uniform"):
        fc.captured(find_pval.find_pval, small, background, mean, std, fc.K, [("laplace", 0.1, (0.0, 1.0))])


# ---- the commands ---------------------------------------------------------------------------------------------------------------
def command(name, argv, cwd):
    code = "import sys; sys.argv = %r; from seekr_amd.console_scripts import console_%s; console_%s()" % (
        ["seekr_" + name] + [str(a) for a in argv], name, name)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    proc = subprocess.run([sys.executable, "-c", code], cwd=cwd, env=env, capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0, proc.stdout + proc.stderr
    return proc.stdout


@pytest.mark.parametrize("form", ["distribution", "npy"])
def test_commands_file_to_file(background, tmp_path, form):
    from seekr_amd import find_dist, find_pval
    small = small_fasta("small.fa")
    os.makedirs("api")
    if form == "distribution":
        command("find_dist", [background, "-k", fc.K, "-mdl", "norm,expon,uniform", "-fm", "-sbs", "1000000", "-o", "cli"], str(tmp_path))
        fitres = find_dist.find_dist(background, fc.K, models=["norm", "expon", "uniform"], subsetting=False, subset_size=10 ** 6,
                                     outputname="api/fit")
        assert find_dist.read_fit_csv("cli.csv") == find_dist.read_fit_csv("api/fit.csv") == [
            (n, float(d), tuple(float(p) for p in ps)) for n, d, ps in fitres]
        assert open("cli.csv", "rb").read() == open("api/fit.csv", "rb").read()
        fitres, extra = find_dist.read_fit_csv("cli.csv"), ["-bf", "2"]
    else:
        out = command("find_dist", [background, "-k", fc.K, "-sbt", "-sbs", "1000000", "-o", "cli"], str(tmp_path))
        assert out == find_dist.SUBSET_TOO_LARGE + "\n"
        find_dist.find_dist(background, fc.K, subsetting=False, fit_model=False, outputname="api/sample")
        assert open("cli.csv", "rb").read() == open("api/sample.csv", "rb").read()
        fitres, extra = np.loadtxt("cli.csv", delimiter=","), ["-ft", "npy"]
    mean, std = "bkg_mean_{}mers.npy".format(fc.K), "bkg_std_{}mers.npy".format(fc.K)  # the ones the command wrote
    command("find_pval", [small, background, mean, std, fc.K, "cli.csv", "-o", "cli_p"] + extra, str(tmp_path))
    fc.captured(find_pval.find_pval, small, background, mean, std, fc.K, fitres, bestfit=2 if extra[0] == "-bf" else 1,
                outputname="api/p")
    assert open("cli_p.csv", "rb").read() == open("api/p.csv", "rb").read()
    assert len(open("cli_p.csv").read().splitlines()) == 4
