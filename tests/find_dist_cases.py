"""What the find_dist / find_pval tests share — test infrastructure: the golden fixtures (tests/golden/find_dist.npz and
.json, made by make_golden_find_dist.py from the reference), the background FASTA they were made from, the fitting loop
of find_dist.py:181-242 written out around the same scipy calls (the yardstick of fit_distributions), and exact
Python-integer arithmetic for the triangle's ranks.  Nothing here calls the device."""
import contextlib
import io
import json
import os
import warnings

import numpy as np

import inputs

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
K = 3
SEED = 3
N_SEQS = 40
N_CELLS = N_SEQS * (N_SEQS - 1) // 2


def arrays():
    with np.load(os.path.join(GOLDEN, "find_dist.npz")) as z:
        return {k: z[k] for k in z.files}


def text():
    with open(os.path.join(GOLDEN, "find_dist.json")) as fh:
        return json.load(fh)


def write_background(path):
    inputs.write_fasta(path, inputs.skewed_set(11, N_SEQS))
    return path


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def captured(fn, *args, **kw):
    """(result, what it printed)."""
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        res = fn(*args, **kw)
    return res, out.getvalue()


# the refused fitres of the golden file, rebuilt (a JSON file cannot hold them)
BAD_FITRES = {
    "list_wrong_format": [("norm", 0.1, [0.0, 1.0])],
    "list_not_tuples": [("norm", 0.1)],
    "array_2d": np.zeros((3, 2), np.float32),
    "other_type": "norm",
}


def exact_unrank(index, n):
    """(i, j) of one position of np.triu_indices(n, 1) in Python integers (no overflow, no rounding)."""
    index, n = int(index), int(n)
    lo, hi = 0, n - 2
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if mid * (2 * n - mid - 1) // 2 <= index:
            lo = mid
        else:
            hi = mid - 1
    return lo, index - lo * (2 * n - lo - 1) // 2 + lo + 1


def exact_rank(i, j, n):
    i, j, n = int(i), int(j), int(n)
    return i * (2 * n - i - 1) // 2 + j - i - 1


def reference_loop(sample, names, statsmethod):
    """find_dist.py:181-242 for distribution names that are known to fit: the statistic of each by `statsmethod` around
    scipy's own calls, sorted by statistic.  An unknown statsmethod falls back to ks, as there."""
    from scipy import stats
    from scipy.stats import kstest
    results = []
    for distribution in [getattr(stats, d) for d in names]:
        with warnings.catch_warnings():
            warnings.filterwarnings("ignore")
            params = distribution.fit(sample)
            if statsmethod == "mse":
                D = np.mean((sample - distribution.rvs(*params, size=len(sample))) ** 2)
            elif statsmethod == "aic":
                D = 2 * len(params) - 2 * np.sum(distribution.logpdf(sample, *params))
            elif statsmethod == "bic":
                D = np.log(len(sample)) * len(params) - 2 * np.sum(distribution.logpdf(sample, *params))
            else:
                D, _ = kstest(sample, distribution.name, args=params)
        results.append((distribution.name, D, params))
    results.sort(key=lambda x: x[1])
    return results


def fit_sample():
    """2 000 float32 values shaped like a background of correlations: a skewed bell around 0."""
    rng = np.random.default_rng(2000)
    return (0.08 * rng.standard_normal(2000) + 0.05 * rng.gamma(2.0, 1.0, 2000) - 0.1).astype(np.float32)
