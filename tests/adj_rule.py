"""numpy restatement of the reference's multiple-testing correction (seekr/adj_pval.py, statsmodels 0.12.2
`multipletests`): the contract seekr_amd.adj_pval reproduces on the device, written without statsmodels so that the GPU
tests and tools/adj_pval_bench.py can check sizes the golden fixtures cannot hold.

`correct(p, method, alpha)` takes the tests in any order and returns the corrected values in that order, in the dtype
the reference returns.  `adj_frame(values, labels_equal, method, alpha)` is adj_pval's two branches on a 2-D array.
"""
import numpy as np

_ALIAS_LISTS = {"bonferroni": ["b", "bonf"], "sidak": ["s"], "holm-sidak": ["hs"], "holm": ["h"],
                "simes-hochberg": ["sh"], "hommel": ["ho"], "fdr_bh": ["fdr_i", "fdr_p", "fdri", "fdrp"],
                "fdr_by": ["fdr_n", "fdr_c", "fdrn", "fdrcorr"], "fdr_tsbh": ["fdr_2sbh"],
                "fdr_tsbky": ["fdr_2sbky", "fdr_twostage"], "fdr_gbs": []}
ALIASES = {a: name for name, more in _ALIAS_LISTS.items() for a in [name] + more}
METHODS = ["bonferroni", "sidak", "holm-sidak", "holm", "simes-hochberg", "hommel", "fdr_bh", "fdr_by", "fdr_tsbh",
           "fdr_tsbky", "fdr_gbs"]


def canonical(method):
    """The method's canonical name; ValueError('method not recognized') like multipletests."""
    name = ALIASES.get(str(method).lower())
    if name is None:
        raise ValueError("method not recognized")
    return name


def _fdr_bh_sorted(s):
    n = len(s)
    ecdf = np.arange(1, n + 1) / float(n)
    c = np.minimum.accumulate((s / ecdf)[::-1])[::-1]
    c[c > 1] = 1
    return c


def _sorted(s, method, alpha):
    n = len(s)
    if method == "bonferroni":
        return s * float(n)
    if method == "sidak":
        return 1 - np.power((1. - s), n)
    if method == "holm-sidak":
        return np.maximum.accumulate(1 - np.power((1. - s), np.arange(n, 0, -1)))
    if method == "holm":
        return np.maximum.accumulate(s * np.arange(n, 0, -1))
    if method == "simes-hochberg":
        return np.minimum.accumulate((np.arange(n, 0, -1) * s)[::-1])[::-1]
    if method == "hommel":
        a = s.copy()
        for m in range(n, 1, -1):
            cim = np.min(m * s[-m:] / np.arange(1, m + 1.))
            a[-m:] = np.maximum(a[-m:], cim)
            a[:-m] = np.maximum(a[:-m], np.minimum(m * s[:-m], cim))
        return a
    if method == "fdr_bh":
        return _fdr_bh_sorted(s)
    if method == "fdr_by":
        cm = np.sum(1. / np.arange(1, n + 1))
        ecdf = np.arange(1, n + 1) / float(n) / cm
        c = np.minimum.accumulate((s / ecdf)[::-1])[::-1]
        c[c > 1] = 1
        return c
    if method in ("fdr_tsbh", "fdr_tsbky"):
        bky = method == "fdr_tsbky"
        fact = (1. + alpha) if bky else 1.
        alpha_prime = alpha / fact if bky else alpha
        c = _fdr_bh_sorted(s)
        reject = s <= (np.arange(1, n + 1) / float(n)) * alpha_prime
        r1 = int(np.nonzero(reject)[0].max()) + 1 if reject.any() else 0
        if r1 == 0 or r1 == n:
            return c * fact
        c *= (1.0 * n - r1) * 1.0 / n
        if bky:
            c *= (1. + alpha)
        return c
    if method == "fdr_gbs":
        ii = np.arange(1, n + 1)
        q = (n + 1. - ii) / ii * s / (1. - s)
        return np.minimum.accumulate(np.maximum.accumulate(q)[::-1])[::-1]
    raise ValueError("method not recognized")


def correct(p, method, alpha=0.05):
    """multipletests(p, alpha, method)[1] for a 1-D float32 / float64 array."""
    method = canonical(method)
    p = np.asarray(p)
    order = np.argsort(p)
    c = _sorted(np.take(p, order), method, float(alpha))
    c[c > 1] = 1
    out = np.empty_like(c)
    out[order] = c
    return out


def round5(x):
    """np.round(x, 5) in x's dtype: rint(x * 1e5) / 1e5 with the scale cast to that dtype."""
    f = x.dtype.type(1e5)
    return np.rint(x * f) / f


def values_symmetric(v):
    """is_symmetric's value test on a square array: off the diagonal round(x, 5) equals its mirror, NaN equal to NaN."""
    n = v.shape[0]
    if v.ndim != 2 or v.shape[1] != n:
        return False
    r = round5(v)
    t = r.T
    off = ~np.eye(n, dtype=bool)
    same = (r == t) | (np.isnan(r) & np.isnan(t))
    return bool(same[off].all())


def adj_frame(v, labels_equal, method, alpha=0.05):
    """(symmetric, values) of adj_pval for the 2-D array v (labels_equal: the row labels equal the column labels)."""
    method = canonical(method)
    if v.shape[0] == v.shape[1] and labels_equal and values_symmetric(v):
        iu = np.triu_indices(v.shape[0], 1)
        out = np.full(v.shape, np.nan)
        out[iu] = correct(v[iu], method, alpha)
        return True, out
    return False, correct(v.reshape(-1), method, alpha).reshape(v.shape)
