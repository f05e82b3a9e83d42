"""The consumers of r (seekr_amd/csrc/consumers.hip) at the sizes, widths, parameters and byte patterns at which their
kernels change path, as tools/adjust_sweep.py does for the p-value correction:

  empirical   empirical_p_kernel searches a table of every `stride`-th background value in LDS (stride = ceil(n / 4096))
              and then one bucket of `stride` values.  Background sizes 1 .. 2^22 + 1 around every change of stride and
              table length (strides 1, 2, 3, 4, 245, 256, 257, 1 025; tables of 1 .. 4 096 entries, ragged last buckets),
              as normals, values rounded to two decimals (tie runs longer than a bucket), one constant, with -inf / +inf,
              with NaN (which counts in len(fitres)) and as float64 with values 1e-10 above and below cells of r.  Cells:
              every table entry, every bucket's first value, their float32 neighbours, min / max +- 1 ulp, +-0, +-inf,
              NaN and 2 000 random ones.  Expected: the searchsorted form of find_pval.py:158-164 (pvalue_rule; the CPU
              test holds it to np.sum(fitres > v) / len(fitres)), bit-exact
  parametric  tests/golden/pvals_sweep.npz (tests/golden/make_golden_pvals.py --sweep, scipy): what dist.fit returns on
              four samples for each of find_dist's ten distributions, gamma shapes 0.05 .. 1e7 and chi2 of twice those
              at mean 0 / sd 0.12, exponpow whose power overflows, lognorm s = 0.005 and 3, pareto b = 0.5, invalid
              shapes (scipy: all NaN).  |dp| <= 2e-6 |p| + 4e-16 and the same NaN cells, the bar of
              tests/test_gpu_consumers.py; the worst err / tol per distribution is printed.  Shapes outside the
              supported range must be refused (NotImplementedError), never answered
  topk        k 1 .. 4 096 by widths 1 .. 5 000 (m - 1 < k included), column windows with global offsets and the diagonal
              inside, on both edges of and outside the window, an empty window, rows of all NaN / all equal / +-0 / +-inf,
              and 4 200 rows (more than the grid: the row loop).  Expected: the stable argsort
  threshold   cutoff NaN / +inf / -inf / +-0 / around a value that is present; diag_col0 negative, inside and >= cols; one
              matrix larger than the grid.  Expected: numpy on the host copy, bit for bit
  edges       the same cutoffs, column windows and global offsets that put the diagonal inside / outside, upper and full
  triu        n 255 .. 4 099 (more rows than the grid) by k 0, 1, n - 1, n, n + 3, float32 and float64

Every sweep_* returns the list of failing cases.

    python tools/consumer_sweep.py [--only empirical,topk] [--seed 1] [--lib path/to/libseekr_hip.so]

Exit code 1 and the failing cases on stderr if any check fails.  Needs a real MI355X.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")


def fail(bad, case, what):
    bad.append("%s: %s" % (case, what))
    print("%s  FAIL  %s" % (case, what), file=sys.stderr, flush=True)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def same_bits_or_nan(got, want):
    """Equal bit for bit where `want` is not NaN (the sign of a zero included), NaN exactly where `want` is."""
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(bits(got)[~nan], bits(want)[~nan]))


def context():
    from seekr_amd import _lib
    return _lib.default_context()


# ---- empirical p-values -------------------------------------------------------------------------------------------------
PVAL_TABLE = 4096  # consumers.hip kPvalTable
BG_SIZES = (1, 2, 3, 255, 256, 257, 4095, 4096, 4097, 8191, 8192, 8193, 12288, 12289, 1000003, 1 << 20, (1 << 20) + 1,
            (1 << 22) + 1)
BG_KINDS = ("normal", "two decimals", "constant", "inf", "nan", "float64 near cells")
N_RANDOM_CELLS = 2000
NEAR = 1e-10  # far below the float32 spacing of a value of r's size (6e-8 relative)


def table_geometry(n_bg):
    """(stride, n_table) of empirical_p_kernel for a background of n_bg values."""
    stride = -(-n_bg // PVAL_TABLE)
    return stride, -(-n_bg // stride)


def random_cells(seed):
    """The random cells of r: the same for every background, so that a float64 background can sit next to them."""
    rng = np.random.default_rng([seed, 41])
    return np.clip(rng.normal(0.0, 0.12, N_RANDOM_CELLS), -1, 1).astype(np.float32)


def background(kind, n, seed=1):
    """The 1-D background `fitres` of `kind` with n values (float32; float64 for the last kind), NaNs included."""
    rng = np.random.default_rng([seed, n, 43])
    v = np.clip(rng.normal(0.0, 0.12, n), -1, 1).astype(np.float32)
    if kind == "normal":
        return v
    if kind == "two decimals":
        return np.round(v, 2)
    if kind == "constant":
        return np.full(n, np.float32(0.0625))
    if kind == "inf":
        v[rng.integers(0, n, max(1, n // 50))] = -np.inf
        v[rng.integers(0, n, max(1, n // 70))] = np.inf
        return v
    if kind == "nan":
        v[rng.integers(0, n, max(1, n // 20))] = np.nan
        return v
    assert kind == "float64 near cells"
    w = v.astype(np.float64)
    cells = random_cells(seed).astype(np.float64)
    m = min(n, 80)
    at = rng.permutation(n)[:m]
    w[at] = cells[:m] + np.where(np.arange(m) % 2 == 0, NEAR, -NEAR)
    return w


def pvalue_cells(fitres, seed=1):
    """The cells of r for a background: every table entry and every bucket's first value of the sorted background
    rounded to float32 (to nearest: with the neighbours below, rounding up is covered too), each with its float32
    neighbours, min / max +- 1 ulp, +-0, +-inf, NaN, and the random cells."""
    valid = np.sort(fitres[~np.isnan(fitres)])
    with np.errstate(over="ignore"):
        bg = valid.astype(np.float32)
    parts = [random_cells(seed), np.array([0.0, -0.0, np.inf, -np.inf, np.nan], dtype=np.float32)]
    if len(bg):
        stride, n_table = table_geometry(len(bg))
        t = np.arange(n_table)
        entries = bg[np.minimum(len(bg) - 1, (t + 1) * stride - 1)]
        firsts = bg[t * stride]
        ends = np.array([bg[0], bg[-1]], dtype=np.float32)
        for v in (entries, firsts, ends):
            parts += [v, np.nextafter(v, np.float32(-np.inf)), np.nextafter(v, np.float32(np.inf))]
    return np.concatenate(parts).astype(np.float32)


def pvalue_rule(cells, fitres):
    """find_pval.py:158-164 for float32 cells: float32(np.sum(fitres > v) / len(fitres)), by one sort and a search in
    the background's own precision instead of the reference's loop.  A NaN cell, like a NaN in fitres, compares False."""
    fitres = np.asarray(fitres).reshape(-1)
    valid = np.sort(fitres[~np.isnan(fitres)]).astype(np.float64)  # exact for a float32 background
    v = cells.astype(np.float64)
    greater = len(valid) - np.searchsorted(valid, v, side="right")
    greater = np.where(np.isnan(v), 0, greater)
    return (greater / float(len(fitres))).astype(np.float32)


def sweep_empirical(seed=1, sizes=BG_SIZES, kinds=BG_KINDS, verbose=False):
    from seekr_amd import consumers
    ctx = context()
    bad = []
    for n in sizes:
        for kind in kinds:
            fitres = background(kind, n, seed)
            cells = pvalue_cells(fitres, seed)
            want = pvalue_rule(cells, fitres)
            d = ctx.from_numpy(cells)
            p = consumers.empirical_pvalues(d, fitres)
            got = p.to_numpy().reshape(-1)
            p.free()
            d.free()
            n_valid = int((~np.isnan(fitres)).sum())
            case = "empirical n=%d %s (stride %d, table %d)" % ((n, kind) + table_geometry(max(1, n_valid)))
            if got.dtype != np.float32 or not np.array_equal(bits(got), bits(want)):
                wrong = np.flatnonzero(bits(got) != bits(want))
                fail(bad, case, "%d of %d cells differ, first: cell %r got %r want %r" % (
                    len(wrong), len(cells), cells[wrong[0]], got[wrong[0]], want[wrong[0]]))
            elif verbose:
                print(case + "  ok, %d cells" % len(cells), flush=True)
    return bad


# ---- parametric p-values ------------------------------------------------------------------------------------------------
RTOL, ATOL = 2e-6, 4e-16  # the bar of tests/test_gpu_consumers.py::test_parametric_pvalues_against_scipy_fixtures
# (distribution, params) that must be refused: gamma shapes (chi2: df / 2) outside [1e-6, 1e7]
REFUSED = (("gamma", (1.0000001e7, -379.5, 3.8e-5)), ("gamma", (1e9, -3794.7, 3.8e-6)), ("gamma", (float("inf"), -1.0, 1.0)),
           ("chi2", (2.1e7, -379.5, 1.9e-5)), ("gamma", (1e-9, -0.3, 0.2)), ("chi2", (1e-7, -0.3, 0.2)))


def gamma_max_terms(a):
    """consumers.hip gamma_max_terms: the bound of gamma_p's loops for the gamma shape a."""
    return 200 + int(12.0 * np.sqrt(a))


def gamma_p_port(a, x, max_terms):
    """consumers.hip gamma_p in host float64, line by line: (P(a, x), terms used, converged)."""
    import math
    if not x > 0.0:
        return 0.0, 0, True
    if math.isinf(x):
        return 1.0, 0, True
    lg = math.lgamma(a)
    if x < a + 1.0:
        ap, delta = a, 1.0 / a
        total = delta
        for n in range(max_terms):
            ap += 1.0
            delta *= x / ap
            total += delta
            if abs(delta) < abs(total) * 1e-17:
                return total * math.exp(-x + a * math.log(x) - lg), n + 1, True
        return total * math.exp(-x + a * math.log(x) - lg), max_terms, False
    tiny = 1e-300
    b, c = x + 1.0 - a, 1.0 / tiny
    d = 1.0 / b
    h = d
    for i in range(1, max_terms + 1):
        an = -float(i) * (float(i) - a)
        b += 2.0
        d = an * d + b
        if abs(d) < tiny:
            d = tiny
        c = b + an / c
        if abs(c) < tiny:
            c = tiny
        d = 1.0 / d
        delta = d * c
        h *= delta
        if abs(delta - 1.0) < 1e-16:
            return 1.0 - math.exp(-x + a * math.log(x) - lg) * h, i, True
    return 1.0 - math.exp(-x + a * math.log(x) - lg) * h, max_terms, False


def fixture_cases(path=None):
    """[(distribution, params, origin, cells, p)] of tests/golden/pvals_sweep.npz."""
    g = np.load(path or os.path.join(GOLDEN, "pvals_sweep.npz"))
    out = []
    for i, (name, params, origin) in enumerate(zip(g["names"], g["params"], g["origins"])):
        cells = np.concatenate([g["sim"], g["own%d" % i]])
        out.append((str(name), tuple(float(v) for v in str(params).split(",")), str(origin), cells, g["p%d" % i]))
    return out


def sweep_parametric(verbose=True, worst=None):
    """`worst`: a dict that receives distribution -> (largest err / tol, params)."""
    from seekr_amd import consumers
    ctx = context()
    bad = []
    worst = {} if worst is None else worst
    for name, params, origin, cells, want in fixture_cases():
        case = "parametric %s(%s) [%s]" % (name, ", ".join("%.9g" % v for v in params), origin)
        d = ctx.from_numpy(cells)
        try:
            p = consumers.parametric_pvalues(d, name, params)
            got = p.to_numpy().reshape(-1)
            p.free()
        except (NotImplementedError, ValueError) as e:
            fail(bad, case, "refused: %s" % e)
            continue
        finally:
            d.free()
        if not np.array_equal(np.isnan(got), np.isnan(want)):
            fail(bad, case, "%d NaN cells, want %d" % (np.isnan(got).sum(), np.isnan(want).sum()))
            continue
        ok = ~np.isnan(want)
        if not ok.any():
            continue
        err = np.abs(got[ok].astype(np.float64) - want[ok])
        tol = RTOL * np.abs(want[ok].astype(np.float64)) + ATOL
        ratio = float((err / tol).max())
        if ratio > worst.get(name, (-1.0, None))[0]:
            worst[name] = (ratio, params)
        if ratio > 1.0:
            at = int(np.argmax(err / tol))
            fail(bad, case, "%d of %d cells past the bar, worst err / tol %.3g at cell %r: %r want %r" % (
                (err > tol).sum(), ok.sum(), ratio, cells[ok][at], got[ok][at], want[ok][at]))
    d = ctx.from_numpy(np.linspace(-1, 1, 33).astype(np.float32))
    for name, params in REFUSED:
        try:
            consumers.parametric_pvalues(d, name, params).free()
            fail(bad, "parametric %s%r" % (name, params), "answered; a shape outside the supported range must be refused")
        except NotImplementedError:
            pass
    d.free()
    if verbose:
        for name in sorted(worst):
            print("parametric %-9s worst err / tol %.3g at %s" % (name, worst[name][0], worst[name][1]), flush=True)
    return bad


# ---- per-row top-k ------------------------------------------------------------------------------------------------------
TOPK_KS = (1, 2, 63, 64, 65, 255, 256, 257, 1000, 4096)
TOPK_WIDTHS = (1, 2, 255, 256, 257, 513, 5000)
TOPK_ROWS = 12
TOPK_LOOP_SHAPE = (4200, 40, 3)  # rows, columns, k: more rows than 16 workgroups per compute unit of a 256-CU device
NO_CELL = 0xFFFFFFFF


def topk_block(rng, rows, m):
    """rows x m float32: normals, with rows of all NaN, one value, +-0 mixed, +-inf, coarse ties and scattered NaN."""
    r = np.clip(rng.normal(0.0, 0.12, (rows, m)), -1, 1).astype(np.float32)
    if rows >= 8:
        r[1] = np.nan
        r[2] = 0.25
        r[3] = np.where(rng.integers(0, 2, m) == 0, np.float32(0.0), np.float32(-0.0))
        r[4, rng.integers(0, m, max(1, m // 5))] = np.inf
        r[4, rng.integers(0, m, max(1, m // 5))] = -np.inf
        r[5] = np.round(r[5], 1)
        r[6, rng.integers(0, m, max(1, m // 4))] = np.nan
        r[7] = np.where(rng.integers(0, 3, m) == 0, np.float32(-0.0), r[7])
    return r


def topk_windows(m, rows):
    """[(name, col_begin, col_end, row_global0, col_global0)]: the diagonal cell of local row i sits at local column
    row_global0 + i - col_global0."""
    c0, c1 = m // 3, m - m // 4
    g = 1000
    half = rows // 2
    return [("whole, diagonal from column 0", 0, m, 0, 0),
            ("whole, diagonal past the last column", 0, m, m + 50, 0),
            ("window, diagonal inside", c0, c1, g + c0 + 1, g),
            ("window, diagonal across its first column", c0, c1, g + c0 - half, g),
            ("window, diagonal across its last column", c0, c1, g + c1 - 1 - half, g),
            ("window, diagonal left of it", c0, c1, max(0, g + c0 - rows - 3), g),
            ("window, diagonal outside the matrix", c0, c1, g + m + 7, g),
            ("window at the global origin", c0, c1, 0, 0),
            ("empty window", c0, c0, 0, g)]


def topk_reference(r, k, c0, c1, row0, col0):
    """np.argsort(-row, kind="stable")[:k] over the window's candidates, the diagonal cell excluded, global columns."""
    rows = r.shape[0]
    idx = np.full((rows, k), NO_CELL, dtype=np.uint32)
    val = np.full((rows, k), np.nan, dtype=np.float32)
    for i in range(rows):
        cand = np.arange(c0, c1)
        cand = cand[cand != row0 + i - col0]
        order = cand[np.argsort(-r[i][cand], kind="stable")][:k]
        idx[i, :len(order)] = order + col0
        val[i, :len(order)] = r[i][order]
    return idx, val


def topk_check(bad, case, d, r, k, c0, c1, row0, col0):
    from seekr_amd import consumers
    idx, val = consumers.topk_rows(d, k, col_begin=c0, col_end=c1, row_global0=row0, col_global0=col0)
    want_idx, want_val = topk_reference(r, k, c0, c1, row0, col0)
    if not np.array_equal(idx, want_idx):
        rows = np.flatnonzero((idx != want_idx).any(axis=1))
        i = int(rows[0])
        fail(bad, case, "columns differ in %d rows, first row %d: %s want %s" % (len(rows), i, idx[i][:6], want_idx[i][:6]))
    elif not same_bits_or_nan(np.asarray(val), want_val):
        fail(bad, case, "values differ")


def sweep_topk(seed=1, ks=TOPK_KS, widths=TOPK_WIDTHS, verbose=False):
    ctx = context()
    bad = []
    for m in widths:
        rng = np.random.default_rng([seed, m, 47])
        r = topk_block(rng, TOPK_ROWS, m)
        d = ctx.from_numpy(r)
        for k in ks:
            for name, c0, c1, row0, col0 in topk_windows(m, TOPK_ROWS):
                topk_check(bad, "topk m=%d k=%d %s [%d, %d) row0 %d col0 %d" % (m, k, name, c0, c1, row0, col0), d, r, k, c0, c1,
                           row0, col0)
        d.free()
        if verbose:
            print("topk m %4d  ok so far: %s" % (m, not bad), flush=True)
    rows, m, k = TOPK_LOOP_SHAPE
    rng = np.random.default_rng([seed, rows, 53])
    r = topk_block(rng, rows, m)
    d = ctx.from_numpy(r)
    topk_check(bad, "topk %d x %d k=%d" % (rows, m, k), d, r, k, 0, m, 0, 0)
    topk_check(bad, "topk %d x %d k=%d window" % (rows, m, k), d, r, k, 5, 33, 4100, 17)
    d.free()
    return bad


# ---- threshold / edges / triu -------------------------------------------------------------------------------------------
def block_with_specials(rng, rows, cols):
    r = np.clip(rng.normal(0.0, 0.12, (rows, cols)), -1, 1).astype(np.float32)
    flat = r.reshape(-1)
    at = rng.permutation(flat.size)[:30]
    flat[at] = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1.0], dtype=np.float32)[np.arange(len(at)) % 6]
    return r


def cutoffs(present):
    """name -> cutoff: the extremes and the float32 neighbourhood of a value that is in the matrix."""
    p = np.float32(present)
    return {"NaN": np.float32(np.nan), "+inf": np.float32(np.inf), "-inf": np.float32(-np.inf), "+0": np.float32(0.0),
            "-0": np.float32(-0.0), "a present value": p, "just below it": np.nextafter(p, np.float32(-np.inf)),
            "just above it": np.nextafter(p, np.float32(np.inf))}


def present_value(r):
    """A positive finite value of r that is not special."""
    flat = r.reshape(-1)
    ok = np.isfinite(flat) & (flat > 0.05) & (flat < 0.9)
    return flat[np.flatnonzero(ok)[7]]


def threshold_reference(r, cutoff, diag_col0):
    want = r.copy()
    with np.errstate(invalid="ignore"):
        want[want < cutoff] = 0       # kmer_leiden.py:94
    i = np.arange(r.shape[0])
    c = i + diag_col0
    inside = (c >= 0) & (c < r.shape[1])
    want[i[inside], c[inside]] = 0    # :96 for a row block whose diagonal starts at column diag_col0
    return want


THRESHOLD_SHAPE = (80, 301)
THRESHOLD_LARGE = (1500, 1400)  # 2.1 M cells: more than 256 x 8 workgroups per compute unit of a 256-CU device


def diag_offsets(rows, cols):
    return (0, 1, -1, -5, -(rows - 1), -rows, -rows - 1, cols - rows, cols - 1, cols, cols + 7, 1 << 40, -(1 << 40))


def sweep_threshold(seed=1, verbose=False):
    from seekr_amd import consumers
    ctx = context()
    bad = []
    for shape, offsets in ((THRESHOLD_SHAPE, diag_offsets(*THRESHOLD_SHAPE)), (THRESHOLD_LARGE, (0, -3, 1399))):
        rng = np.random.default_rng([seed, shape[0], 59])
        r = block_with_specials(rng, *shape)
        for cname, cutoff in cutoffs(present_value(r)).items():
            for dc in offsets:
                d = ctx.from_numpy(r)
                consumers.threshold_zero_diag(d, float(cutoff), diag_col0=dc)
                got = d.to_numpy()
                d.free()
                if not same_bits_or_nan(np.asarray(got), threshold_reference(r, cutoff, dc)):
                    fail(bad, "threshold %dx%d cutoff %s diag_col0 %d" % (shape + (cname, dc)), "differs from numpy")
    return bad


def edges_reference(r, cutoff, nrows, c0, c1, row0, col0, upper):
    """kmer_leiden.py:94-96 on a host copy of the block placed at global (row0, col0 + c0), then np.nonzero."""
    blk = r[:nrows, c0:c1].copy()
    with np.errstate(invalid="ignore"):
        blk[blk < cutoff] = 0
    gi = (row0 + np.arange(nrows, dtype=np.int64))[:, None]
    gj = (col0 + np.arange(c0, c1, dtype=np.int64))[None, :]
    blk[np.broadcast_to(gi == gj, blk.shape)] = 0
    if upper:
        blk[np.broadcast_to(gj <= gi, blk.shape)] = 0
    i, j = np.nonzero(blk)  # NaN counts as non-zero
    return (i + row0).astype(np.uint32), (j + c0 + col0).astype(np.uint32), blk[i, j]


EDGES_SHAPE = (130, 517)


def edge_windows(rows, cols):
    """[(name, nrows, col_begin, col_end, row_global0, col_global0)]"""
    c0, c1 = cols // 3, cols - cols // 4
    return [("whole", rows, 0, cols, 0, 0),
            ("window, diagonal inside", rows, c0, c1, 5000 + c0 + 2, 5000),
            ("window, diagonal across its first column", rows, c0, c1, 5000 + c0 - rows // 2, 5000),
            ("window, diagonal across its last column", rows, c0, c1, 5000 + c1 - rows // 2, 5000),
            ("window above the diagonal", rows - 7, c0, c1, 0, 70000),
            ("window below the diagonal", rows, c0, c1, 70000, 0),
            ("one column", rows, c0, c0 + 1, c0 + 3, 0),
            ("empty window", rows, c0, c0, 0, 0)]


def sweep_edges(seed=1, verbose=False):
    from seekr_amd import consumers
    ctx = context()
    bad = []
    rng = np.random.default_rng([seed, EDGES_SHAPE[0], 61])
    r = block_with_specials(rng, *EDGES_SHAPE)
    d = ctx.from_numpy(r)
    for cname, cutoff in cutoffs(present_value(r)).items():
        for wname, nrows, c0, c1, row0, col0 in edge_windows(*EDGES_SHAPE):
            for upper in (False, True):
                i, j, v = consumers.edges(d, float(cutoff), nrows=nrows, col_begin=c0, col_end=c1, row_global0=row0,
                                          col_global0=col0, upper_only=upper)
                wi, wj, wv = edges_reference(r, cutoff, nrows, c0, c1, row0, col0, upper)
                case = "edges cutoff %s %s%s" % (cname, wname, " upper" if upper else "")
                if not (np.array_equal(i, wi) and np.array_equal(j, wj)):
                    fail(bad, case, "%d edges, want %d; cells differ" % (len(i), len(wi)))
                elif not same_bits_or_nan(v, wv):
                    fail(bad, case, "values differ")
    d.free()
    return bad


TRIU_NS = (255, 256, 257, 4099)  # 4 099 rows: more than 16 workgroups per compute unit of a 256-CU device


def triu_ks(n):
    return (0, 1, n - 1, n, n + 3)


def triu_reference(r, k):
    """r[np.triu_indices(n, k)] (find_dist.py:163) without the index arrays: np.triu_indices is nonzero(~tri(n, n, k - 1)),
    and a boolean mask selects in the same row-major order."""
    n = r.shape[0]
    return r[~np.tri(n, n, k - 1, dtype=bool)]


def sweep_triu(seed=1, ns=TRIU_NS, verbose=False):
    from seekr_amd import consumers
    ctx = context()
    bad = []
    for n in ns:
        for dtype in (np.float32, np.float64):
            rng = np.random.default_rng([seed, n, np.dtype(dtype).itemsize, 67])
            r = rng.standard_normal((n, n), dtype=dtype)
            r[rng.integers(0, n, 5), rng.integers(0, n, 5)] = np.nan
            r[0, n - 1] = -0.0
            d = ctx.from_numpy(r)
            for k in triu_ks(n):
                want = triu_reference(r, k)
                flat = consumers.triu_values(d, k=k)
                case = "triu n=%d k=%d %s" % (n, k, np.dtype(dtype).name)
                if flat.cols != len(want) or flat.dtype != np.dtype(dtype):
                    fail(bad, case, "%d values of %s, want %d" % (flat.cols, flat.dtype, len(want)))
                elif len(want) and not np.array_equal(bits(flat.to_numpy().reshape(-1)), bits(want)):
                    fail(bad, case, "values differ")
                flat.free()
            d.free()
    return bad


SWEEPS = ("empirical", "parametric", "topk", "threshold", "edges", "triu")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--only", default=None, help="comma-separated: " + ",".join(SWEEPS))
    ap.add_argument("--lib", default=None, help="another build of libseekr_hip.so to run the sweep against")
    args = ap.parse_args()
    if args.lib:
        from seekr_amd import _lib
        _lib.LIB_PATH = os.path.abspath(args.lib)
    only = set(args.only.split(",")) if args.only else set(SWEEPS)
    failing = 0
    for name in SWEEPS:
        if name not in only:
            continue
        t0 = time.time()
        if name == "empirical":
            bad, what = sweep_empirical(args.seed), "%d background sizes x %d kinds" % (len(BG_SIZES), len(BG_KINDS))
        elif name == "parametric":
            bad, what = sweep_parametric(), "%d fixture cases, %d refused shapes" % (len(fixture_cases()), len(REFUSED))
        elif name == "topk":
            bad, what = sweep_topk(args.seed), "k %s by widths %s, %d x %d" % ((TOPK_KS, TOPK_WIDTHS) + TOPK_LOOP_SHAPE[:2])
        elif name == "threshold":
            bad, what = sweep_threshold(args.seed), "%d cutoffs x %d diagonal offsets" % (len(cutoffs(0.5)), len(diag_offsets(2, 3)))
        elif name == "edges":
            bad, what = sweep_edges(args.seed), "%d cutoffs x %d windows" % (len(cutoffs(0.5)), len(edge_windows(9, 9)))
        else:
            bad, what = sweep_triu(args.seed), "n %s, k 0 / 1 / n - 1 / n / n + 3, both dtypes" % (TRIU_NS,)
        failing += len(bad)
        print("%s: %s, %d failing, %.1f s" % (name, what, len(bad), time.time() - t0), flush=True)
    sys.exit(1 if failing else 0)


if __name__ == "__main__":
    main()
