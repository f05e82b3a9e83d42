"""Inputs of the significant-pairs tests, from fixed seeds (plain numpy, no GPU), and the numpy side of their checks.

  planted_counts()   300 rows x 256 columns: six planted groups of 20 rows of graded strength (r inside a group from about
                     one to eight standard deviations of the background) plus 180 noise rows
  backgrounds()      name -> fitres as pearson_significant takes it: a norm tuple, a shifted gamma tuple, a float32
                     empirical background of 10 000 two-decimal values (long tie runs), a float64 empirical background
  empirical_p        find_pval.py:158-164 in numpy
  head_correct       adj_rule's formulas run on the smallest p-values of a longer list: adj_rule._sorted evaluated with the
                     full number of tests at the sorted positions that exist — the "prefix formulas"
"""
import functools

import numpy as np

import adj_rule

N_ROWS, N_COLS, GROUPS, GROUP_ROWS = 300, 256, 6, 20
SD = 1.0 / 16.0  # the standard deviation of r between two noise rows of 256 columns
HEAD_METHODS = ["bonferroni", "sidak", "holm-sidak", "holm", "simes-hochberg", "fdr_bh", "fdr_by"]
REFUSED = ["hommel", "fdr_tsbh", "fdr_tsbky", "fdr_gbs"]


@functools.lru_cache(maxsize=None)
def planted_counts():
    rng = np.random.default_rng(20261019)
    x = rng.standard_normal((N_ROWS, N_COLS))
    strength = (0.25, 0.35, 0.45, 0.55, 0.7, 0.9)
    for g in range(GROUPS):
        centre = rng.standard_normal(N_COLS)
        rows = slice(g * GROUP_ROWS, (g + 1) * GROUP_ROWS)
        x[rows] += strength[g] * centre
    x = x[rng.permutation(N_ROWS)]  # the groups are not blocks of the matrix
    x.setflags(write=False)
    out = x.astype(np.float32)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def backgrounds():
    rng = np.random.default_rng(20261020)
    shape = 16.0
    scale = SD / np.sqrt(shape)
    two_decimals = np.round(rng.standard_normal(10000) * SD, 2).astype(np.float32)
    wide = rng.standard_normal(10000) * SD
    for a in (two_decimals, wide):
        a.setflags(write=False)
    return {"norm": [("norm", 0.0, (0.0, SD))],
            "gamma": [("gamma", 0.0, (shape, -shape * scale, scale))],
            "empirical_f32": two_decimals,
            "empirical_f64": wide}


def ceil_float32(values):
    wide = np.asarray(values, dtype=np.float64)
    near = wide.astype(np.float32)
    return np.where(near < wide, np.nextafter(near, np.float32(np.inf)), near).astype(np.float32)


def empirical_p(r, fitres):
    """p[i] = float32(count(fitres > r[i]) / len(fitres)), the comparison in the background's own precision."""
    fitres = np.asarray(fitres).reshape(-1)
    bg = np.sort(fitres if fitres.dtype == np.float32 else ceil_float32(fitres))
    r = np.asarray(r, dtype=np.float32)
    return ((len(bg) - np.searchsorted(bg, r, side="right")) / float(len(fitres))).astype(np.float32)


def alpha32(alpha):
    return ceil_float32(np.array([alpha]))[0]


def _head_sorted(s, ntests, method):
    """adj_rule._sorted with `ntests` in place of n wherever n is the number of tests; s: the len(s) smallest, ascending."""
    e = len(s)
    n = int(ntests)
    if method == "bonferroni":
        return s * float(n)
    if method == "sidak":
        return 1 - np.power((1. - s), n)
    down = np.arange(n, n - e, -1)
    if method == "holm-sidak":
        return np.maximum.accumulate(1 - np.power((1. - s), down))
    if method == "holm":
        return np.maximum.accumulate(s * down)
    if method == "simes-hochberg":
        return np.minimum.accumulate((down * s)[::-1])[::-1]
    ecdf = np.arange(1, e + 1) / float(n)
    if method == "fdr_by":
        ecdf = ecdf / np.sum(1. / np.arange(1, n + 1))
    elif method != "fdr_bh":
        raise ValueError(method)
    c = np.minimum.accumulate((s / ecdf)[::-1])[::-1]
    c[c > 1] = 1
    return c


def head_correct(p, ntests, method):
    """The corrected values of the tests p (any order), taken as the len(p) smallest of `ntests` tests."""
    p = np.asarray(p)
    order = np.argsort(p, kind="stable")
    c = _head_sorted(np.take(p, order), ntests, adj_rule.canonical(method))
    c[c > 1] = 1
    out = np.empty_like(c)
    out[order] = c
    return out


def tied_pvalues(rng, n, dtype, small=0.3):
    """p-values with ties: a share `small` of them below 0.25 on a coarse grid or uniform, the rest uniform in [0, 1]."""
    v = rng.random(n)
    kind = rng.random(n)
    v = np.where(kind < small, v * 0.25, v)
    grid = rng.integers(0, 65, n) / 256.0
    v = np.where(kind < small * 0.5, grid, v)
    return v.astype(dtype)
