"""find_dist of the reference (find_dist.py:82-294) on MI355X: the background sample is drawn before r exists.

The reference counts the background, builds the whole N x N Pearson matrix, flattens its upper triangle and draws
`subset_size` values from it.  Here the indices are drawn first (consumers.draw_index: the same draw from numpy's legacy
state) and those cells are gathered out of the [stripe, panel] blocks of one sweep of r (consumers.pearson_sample), so a
background of 200 000 transcripts needs the operands and one block buffer.  The sampled values are the bits of the r that
sweep makes.  The fits are scipy's own calls on the host, on at most `subset_size` float32 values: `distribution.fit` and
`kstest` give exactly the result the reference gives for the same sample; no device code evaluates a pdf, a likelihood
or a KS statistic.

Kept as the reference has them: `bkg_mean_{k}mers.npy` / `bkg_std_{k}mers.npy` are written to the working directory
(find_pval takes them), and the second counter is built WITHOUT the `log2` argument (find_dist.py:156), so the background
is always counted with BasicCounter's default whatever `log2` says.  Different, all in DESIGN_PARITY.md: no plot is drawn
(`plotfit` prints a notice; the returned sample is what a plot needs); `inputseq='default'` raises FileNotFoundError (the
13 000-transcript FASTA is not shipped); the fitted CSV holds plain floats.  find_dist can fit any scipy model, find_pval
has a device cdf for the ten of COMMON10 only.
"""
import os
import warnings

import numpy as np

from seekr_amd import _lib, consumers, neighbors
from seekr_amd.kmer_counts import BasicCounter

COMMON10 = ["cauchy", "chi2", "expon", "exponpow", "gamma", "lognorm", "norm", "pareto", "rayleigh", "uniform"]
DEFAULT_FASTA = "gencode.vM25.lncRNA_transcripts.unique.genesequence_withfullairn.fa"
DEFAULT_LINES = ("Using default background sequences: mouse vM25 Long non-coding RNA transcript sequences from Gencode.",
                 "https://www.gencodegenes.org/mouse/release_M25.html",
                 "Only including unique sequences and have the full length Airn(chr17:12741398-12830151) appended.")
INVALID_NAMES = ("Please enter valid distribution names available in scipy.stats. refer to "
                 "https://docs.scipy.org/doc/scipy/reference/stats.html#continuous-distributions")
SUBSET_TOO_LARGE = "subset_size is larger than the actual data size, use the actual data size instead"
MANY_AND_LARGE = ("The input sequence count and distribution number for fitting are both large, subsetting is recommended "
                  "to save time")
BAD_STATSMETHOD = "Please enter a valid statsmethod: 'ks', 'mse', 'aic', or 'bic'. Use default 'ks' now."
NO_PLOT_WITHOUT_FIT = ("No plot will be produced as fit_model is set to False, please set fit_model=True to plot the fitted "
                       "distributions vs the actual data")
NO_PLOT = "plotfit={!r}: no plot is drawn here; the returned sample and fits are what a plot needs."


def _scipy_stats():
    try:
        from scipy import stats
    except ImportError as e:
        raise ImportError("fitting distributions needs scipy ({}); find_dist(fit_model=False) returns the background "
                          "sample and needs no scipy".format(e)) from e
    return stats


def resolve_models(models):
    """The names of the distributions find_dist fits for `models` — 'common10', 'all' or a list of names — with the
    reference's filtering and printed sentences (find_dist.py:96-144): names scipy.stats does not have as a continuous
    or discrete distribution are dropped (as are private names, levy_stable and studentized_range), then names whose
    object has no `fit` method.  The second sentence lists EVERY name that passed the first filter, not only the ones
    without `fit`: the reference looks the names up in a list of distribution objects, where no string is ever found
    (find_dist.py:143); kept, since the sentence is part of what a user sees."""
    if models == "common10":
        names = list(COMMON10)
    else:
        stats = _scipy_stats()
        known = [d for d in dir(stats) if isinstance(getattr(stats, d), stats.rv_continuous)]
        known += [d for d in dir(stats) if isinstance(getattr(stats, d), stats.rv_discrete)]
        names = [d for d in known if d[0] != "_" and d not in ("levy_stable", "studentized_range")]
        if models != "all":
            asked = len(models)
            names = [d for d in models if d in names]
            if len(names) < asked:
                print(INVALID_NAMES)
                print(f"Excluding invalid distributions for fitting: {[d for d in models if d not in names]}")
    if models == "common10":
        return names  # all ten have a fit method; nothing is printed for this choice either way
    fitting = [d for d in names if "fit" in dir(getattr(stats, d))]
    if len(fitting) < len(names) and models != "all":
        print(f"Excluding distributions do not have a 'fit' method: {names}")
    return fitting


def background_operand(inputseq, k_mer=4, log2="Log2.post"):
    """(z, n): the prepared operand (_lib.Operand, the caller frees it) of the background's standardised counts and its
    number of rows — find_dist.py:148-157 on this package.  The first counter computes mean and std, which are written to
    bkg_mean_{k}mers.npy / bkg_std_{k}mers.npy in the working directory; the second one is built with those files and,
    exactly as the reference calls it, without `log2`."""
    norm_counter = BasicCounter(inputseq, log2=log2, k=k_mer, silent=True)
    norm_counter.get_counts()
    mean_path, std_path = f"bkg_mean_{k_mer}mers.npy", f"bkg_std_{k_mer}mers.npy"
    np.save(mean_path, norm_counter.mean)
    np.save(std_path, norm_counter.std)
    counter = BasicCounter(inputseq, mean=mean_path, std=std_path, k=k_mer, silent=True)
    counter.make_count_file()
    counts = np.ascontiguousarray(counter.counts, dtype=np.float32)
    z, _ = neighbors._prepare(_lib.default_context(), counts, counts, True)
    return z, counts.shape[0]


def sample_operand(z, subsetting=True, subset_size=100000, rng=None, stripe_rows=8192, panel_rows=None):
    """float32 sample of the upper triangle of r of the prepared operand z (find_dist.py:163-171): subset_size cells at
    consumers.draw_index's positions when subsetting and the triangle is longer, else the whole triangle in
    np.triu_indices order (with the reference's sentence when subsetting was asked for).  r is never made.  The whole
    triangle goes through the same gather, so it is limited to consumers.SAMPLE_MAX = 2^28 cells (23 170 rows):
    ValueError above that, before the sweep starts — a background that large is what subsetting is for."""
    n = z.rows
    n_cells = n * (n - 1) // 2
    if subsetting and n_cells > subset_size:
        index = consumers.draw_index(n_cells, subset_size, rng)
    else:
        if subsetting:
            print(SUBSET_TOO_LARGE)
        index = np.arange(n_cells, dtype=np.int64)
    return consumers.pearson_sample(z, None, index, stripe_rows=stripe_rows, panel_rows=panel_rows)


@_lib.api_call
def background_sample(inputseq, k_mer=4, log2="Log2.post", subsetting=True, subset_size=100000, rng=None, stripe_rows=8192,
                      panel_rows=None):
    """background_operand, then sample_operand: the values find_dist fits or returns."""
    z, _ = background_operand(inputseq, k_mer, log2)
    try:
        return sample_operand(z, subsetting, subset_size, rng, stripe_rows, panel_rows)
    finally:
        z.free()


def fit_distributions(sample, names, statsmethod="ks", progress_bar=False):
    """[(name, statistic, params)] sorted by statistic: the loop of find_dist.py:181-242 around scipy's own fit, kstest,
    rvs, logpdf and logpmf — same messages, same exclusion of a distribution that raises, same fallback to ks for an
    unknown statsmethod.  'mse' draws its rvs from numpy's legacy global state, after the subsample's draw."""
    stats = _scipy_stats()
    from scipy.stats import kstest
    results = []
    distributions = [getattr(stats, d) for d in names]
    if progress_bar:
        from seekr_amd.my_tqdm import my_tqdm
        distributions = my_tqdm()(distributions)
    n = len(sample)
    for distribution in distributions:
        continuous = isinstance(distribution, stats.rv_continuous)
        with warnings.catch_warnings():
            warnings.filterwarnings("ignore")
            try:
                params = distribution.fit(sample)
                if statsmethod == "mse":
                    if continuous:
                        drawn = distribution.rvs(*params, size=n)
                    else:
                        drawn = distribution.rvs(*params[:-2], loc=params[-2], scale=params[-1], size=n)
                    D = np.mean((sample - drawn) ** 2)
                elif statsmethod in ("aic", "bic"):
                    if continuous:
                        loglik = np.sum(distribution.logpdf(sample, *params))
                    else:
                        loglik = np.sum(distribution.logpmf(sample, *params[:-2], loc=params[-2], scale=params[-1]))
                    weight = 2 if statsmethod == "aic" else np.log(n)
                    D = weight * len(params) - 2 * loglik
                else:
                    if statsmethod != "ks":
                        print(BAD_STATSMETHOD)
                    D, _ = kstest(sample, distribution.name, args=params)
            except Exception as e:  # noqa: BLE001 - the reference excludes whatever cannot be fitted
                print(f"Could not fit {distribution.name} because {e}, excluding it from the results")
                continue
            results.append((distribution.name, D, params))
    results.sort(key=lambda x: x[1])
    return results


def write_fit_csv(path, results):
    """The reference's three-column CSV (distribution_name, D_statistics, params) with every number converted by float()
    first: a plain float's repr reads back exactly under numpy 1 and 2, where numpy 2 would print np.float64(...)."""
    import pandas as pd
    plain = [(name, float(D), tuple(float(p) for p in params)) for name, D, params in results]
    pd.DataFrame(plain, columns=["distribution_name", "D_statistics", "params"]).to_csv(path, index=False)


def _number(text):
    text = text.strip()
    for wrap in ("np.float64(", "np.float32("):
        if text.startswith(wrap) and text.endswith(")"):
            return float(text[len(wrap):-1])
    return float(text)


def read_fit_csv(path):
    """[(name, statistic, params)] of a fitted-distribution CSV: the plain-float form write_fit_csv writes, or
    parameters wrapped as np.float64(...) / np.float32(...) as the reference writes them under numpy 2."""
    import pandas as pd
    frame = pd.read_csv(path, float_precision="round_trip")  # the default parser is an ulp off on some statistics
    return [(row[0], row[1], tuple(_number(t) for t in row[2].strip()[1:-1].split(",") if t.strip()))
            for row in frame.values]


def find_dist(inputseq="default", k_mer=4, log2="Log2.post", models="common10", subsetting=True, subset_size=100000,
              fit_model=True, statsmethod="ks", progress_bar=False, plotfit=None, outputname=None, *, rng=None,
              stripe_rows=8192, panel_rows=None):
    """The reference's find_dist: with fit_model the list [(distribution name, statistic, params)] of the fitted
    `models`, best first; without it the float32 background sample itself.  `outputname`: <outputname>.csv receives the
    fits (write_fit_csv) or the sample (np.savetxt's bytes).  rng: a np.random.Generator for the draw instead of numpy's
    legacy global state; stripe_rows, panel_rows: the sweep's blocks (consumers.Sweep).  See the module docstring for
    what is kept and what differs.  Without subsetting (or with a subset_size no shorter than the triangle) the whole
    triangle is returned, which is limited to 2^28 cells — about 23 170 sequences (ValueError above)."""
    if inputseq == "default":
        for line in DEFAULT_LINES:
            print(line)
        inputseq = os.path.join(os.path.dirname(os.path.realpath(__file__)), "data", DEFAULT_FASTA)
        if not os.path.exists(inputseq):
            raise FileNotFoundError("the default background is not shipped with this package: {} does not exist; pass the "
                                    "path of a FASTA file".format(inputseq))
    try:
        names = resolve_models(models)  # before anything is counted, as in the reference: its sentences come first
    except ImportError:
        if fit_model:
            raise
        names = []  # fit_model=False needs no scipy: the list would not be used
    sample = background_sample(inputseq, k_mer, log2, subsetting, subset_size, rng, stripe_rows, panel_rows)
    if fit_model:
        if len(names) > 50 and len(sample) > 5000000 and subsetting == False:  # noqa: E712 - the reference's comparison
            print(MANY_AND_LARGE)
        results = fit_distributions(sample, names, statsmethod, progress_bar)
        if plotfit:
            print(NO_PLOT.format(plotfit))
        if outputname:
            write_fit_csv(f"{outputname}.csv", results)
        return results
    if plotfit:
        print(NO_PLOT_WITHOUT_FIT)
    if outputname:
        _lib.save_csv(f"{outputname}.csv", sample.reshape(-1, 1), fmt=_lib.FMT_SCI18)
    return sample
