"""Consumers of the Pearson matrix against their numpy definitions in the
reference: kmer_leiden.py:94-96, find_dist.py:163,169, find_pval.py:158-164.  Bit-exact: they
are copies, comparisons and one correctly rounded division."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from seekr_amd import _lib
    return _lib.default_context()


def rand_r(n, m=None, seed=0):
    rng = np.random.default_rng(seed)
    r = np.clip(rng.normal(0.0, 0.12, size=(n, m or n)), -1, 1).astype(np.float32)
    return r


def test_threshold_zero_diag(ctx):
    from seekr_amd import consumers
    r = rand_r(301, seed=1)
    r[5, 7] = np.nan
    want = r.copy()
    with np.errstate(invalid="ignore"):
        want[want < 0.1] = 0       # kmer_leiden.py:94
    np.fill_diagonal(want, 0)      # :96
    d = ctx.from_numpy(r)
    consumers.threshold_zero_diag(d, 0.1)
    got = d.to_numpy()
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.nan_to_num(got), np.nan_to_num(want))
    # a row block [100:180, :] of the same matrix: the diagonal sits at column row + 100
    blk = ctx.from_numpy(r[100:180])
    consumers.threshold_zero_diag(blk, 0.1, diag_col0=100)
    assert np.array_equal(np.nan_to_num(blk.to_numpy()), np.nan_to_num(want[100:180]))


@pytest.mark.parametrize("n,k", [(1, 1), (2, 1), (7, 1), (300, 1), (1025, 1), (64, 0), (64, 3)])
def test_triu_values_and_subsample(n, k, ctx):
    from seekr_amd import consumers
    r = rand_r(n, seed=n)
    want = r[np.triu_indices(n, k=k)]  # find_dist.py:163
    d = ctx.from_numpy(r)
    flat = consumers.triu_values(d, k=k)
    assert flat.cols == len(want)
    if len(want):
        assert np.array_equal(flat.to_numpy().reshape(-1), want)
    if len(want) > 10:
        np.random.seed(42)
        ref = np.random.choice(want, size=10, replace=False)  # find_dist.py:169
        np.random.seed(42)
        got = consumers.subsample(flat, 10)
        assert np.array_equal(got, ref)


def test_empirical_pvalues(ctx):
    from seekr_amd import consumers
    sim = rand_r(40, 55, seed=3)
    sim[0, 0] = np.nan
    fitres = rand_r(1, 5000, seed=4).reshape(-1)
    fitres[:55] = sim[1]  # ties with sim values
    fitres[13] = np.nan
    want = np.zeros_like(sim)  # find_pval.py:154-164
    with np.errstate(invalid="ignore"):
        for i in range(sim.shape[0]):
            for j in range(sim.shape[1]):
                want[i, j] = np.sum(fitres > sim[i, j]) / len(fitres)
    got = consumers.empirical_pvalues_host(sim, fitres)
    assert got.dtype == np.float32 and np.array_equal(got, want)
    assert np.array_equal(consumers.empirical_pvalues_host(sim, np.array([np.nan, np.nan])), np.zeros_like(sim))


def nonzero_edges(r, cutoff, upper):
    """kmer_leiden.py:94-96 on a host copy, then the non-zero cells in np.nonzero order."""
    want = r.copy()
    with np.errstate(invalid="ignore"):
        want[want < cutoff] = 0
    np.fill_diagonal(want, 0)
    if upper:
        want = np.triu(want, 1)
    i, j = np.nonzero(want)  # NaN counts as non-zero
    return i.astype(np.uint32), j.astype(np.uint32), want[i, j]


@pytest.mark.parametrize("n,m,cutoff", [(301, 301, 0.1), (64, 1000, 0.25), (513, 513, -5.0), (100, 100, 2.0), (257, 255, 0.0),
                                        (4500, 130, 0.1)])
def test_edges_of_a_block_match_numpy(n, m, cutoff, ctx):
    from seekr_amd import consumers
    r = rand_r(n, m, seed=n)
    r[3, 5] = np.nan
    r[7, 9] = 0.0
    d = ctx.from_numpy(r)
    for upper in (False, True):
        i, j, v = consumers.edges(d, cutoff, upper_only=upper)
        wi, wj, wv = nonzero_edges(r, cutoff, upper)
        assert np.array_equal(i, wi) and np.array_equal(j, wj)
        assert np.array_equal(np.isnan(v), np.isnan(wv)) and np.array_equal(np.nan_to_num(v), np.nan_to_num(wv))
    # a sub-block with global offsets: rows 10.. of the matrix, columns 20..m, diagonal where global ids meet
    sub = ctx.from_numpy(r[10:50])
    i, j, v = consumers.edges(sub, cutoff, col_begin=20, row_global0=10)
    full = np.full_like(r, 0)
    full[10:50, 20:] = r[10:50, 20:]
    wi, wj, wv = nonzero_edges(full, cutoff, False)
    assert np.array_equal(i, wi) and np.array_equal(j, wj) and np.array_equal(np.nan_to_num(v), np.nan_to_num(wv))


def test_pearson_edges_striped_equals_full_matrix(ctx):
    """r produced and thresholded one row stripe at a time (never N x N) gives the edge list of the
    full matrix: same cells, same order, same float32 values."""
    from seekr_amd import _lib as L, consumers
    rng = np.random.default_rng(5)
    n, k = 3001, 4096
    base = rng.binomial(40, 0.05, size=(60, k)).astype(np.float32)
    x = (base[rng.integers(0, 60, n)] + rng.binomial(6, 0.3, size=(n, k))).astype(np.float32)  # clustered rows
    z, _ = L.operand_fill(ctx, ctx.from_numpy(x))
    full = ctx.empty(n, n)
    L.pearson_gemm_op(ctx, z, z, full, symmetric=False)
    r = full.to_numpy()
    cutoff = float(np.quantile(r, 0.97))
    for upper, stripe in ((True, 700), (False, 1024), (True, 5000)):
        i, j, v = consumers.pearson_edges(z, cutoff, stripe_rows=stripe, upper_only=upper)
        wi, wj, wv = nonzero_edges(r, cutoff, upper)
        assert len(wi) > 1000
        assert np.array_equal(i, wi) and np.array_equal(j, wj) and np.array_equal(v, wv)


@pytest.mark.parametrize("n,m,k", [(50, 50, 5), (301, 1000, 17), (64, 64, 80), (20, 3000, 1)])
def test_topk_rows_matches_stable_argsort(n, m, k, ctx):
    from seekr_amd import consumers
    r = rand_r(n, m, seed=n + k)
    r[:, 5] = r[:, 7]          # ties: the smaller column wins
    r[3, 11] = np.nan          # NaN sorts last
    r[4, :] = 0.25             # a constant row
    idx, val = consumers.topk_rows(ctx.from_numpy(r), k)
    for i in range(n):
        row = r[i].copy()
        cand = np.array([c for c in range(m) if c != i])          # the diagonal cell is excluded
        order = cand[np.argsort(-row[cand], kind="stable")][:k]
        want_idx = np.full(k, 0xFFFFFFFF, np.uint32)
        want_idx[:len(order)] = order
        assert np.array_equal(idx[i], want_idx), (i, idx[i][:8], want_idx[:8])
        got = val[i][:len(order)]
        assert np.array_equal(np.isnan(got), np.isnan(row[order])) and np.array_equal(np.nan_to_num(got), np.nan_to_num(row[order]))
        assert np.isnan(val[i][len(order):]).all()
    # a row block with global offsets: rows 10.., the diagonal sits at local column 10 + i
    blk = ctx.from_numpy(r[10:20])
    idx2, _ = consumers.topk_rows(blk, 3, row_global0=10)
    for i in range(10):
        cand = np.array([c for c in range(m) if c != 10 + i])
        assert np.array_equal(idx2[i], cand[np.argsort(-r[10 + i][cand], kind="stable")][:3])


def test_parametric_pvalues_against_scipy_fixtures(ctx, golden_dir):
    """find_pval.py:118-133: p = 1 - dist.cdf(sim) for find_dist's common10 distributions, fixtures from scipy
    (tests/golden/make_golden_pvals.py).  scipy works in float64 and the store rounds to float32; the device does
    the same with its own float64 atan / erfc / expm1 / pow / incomplete gamma, so the results agree to float32
    rounding of values that differ by a few float64 ulps: |dp| <= 2e-6 p + 4e-16 (the absolute term is the float64
    granularity of 1 - cdf where the cdf has reached 1)."""
    from seekr_amd import consumers
    g = np.load(os.path.join(golden_dir, "pvals_common10.npz"))
    sim = g["sim"]
    d = ctx.from_numpy(sim)
    for i, (name, params) in enumerate(zip(g["names"], g["params"])):
        want = g["p%d" % i]
        got = consumers.parametric_pvalues(d, str(name), [float(v) for v in str(params).split(",")]).to_numpy()
        assert np.array_equal(np.isnan(got), np.isnan(want)), name
        ok = np.abs(got - want) <= 2e-6 * np.abs(want) + 4e-16
        assert (ok | np.isnan(want)).all(), (str(name), str(params), float(np.nanmax(np.abs(got - want) / (np.abs(want) + 1e-300))))
    # the host helper takes find_dist's result list as it is
    host = consumers.pvalues_host(sim, [("norm", 0.01, (0.01, 0.08))])
    assert np.allclose(host, g["p0"], rtol=2e-6, atol=4e-16, equal_nan=True)
    with pytest.raises(NotImplementedError):
        consumers.parametric_pvalues(d, "weibull_min", (1.5, 0.0, 1.0))


@pytest.mark.parametrize("shape", [(700, 4096, 0.05, True), (1300, 4096, -0.01, False), (530, 16384, 0.04, True),
                                   (300, 1024, 0.0, False)])
def test_threshold_fused_into_the_contraction_equals_the_two_step_path(shape, ctx):
    """skr_pearson_gemm_edges (EDGES mode of the split contraction: the epilogue thresholds, nothing is stored, the
    list is sorted on the device) against skr_pearson_gemm_op + skr_edges: identical rows, columns and values, bit for
    bit — stripes, offsets, upper / full, k = 7 rows (four k chunks: the first three leave partial sums in the scratch
    block), a constant row (NaN cells are edges, as in numpy) and a buffer that is too small at first."""
    from seekr_amd import _lib, consumers
    n, cols, cutoff, upper = shape
    rng = np.random.default_rng(n)
    x = (rng.binomial(40, 0.06, size=(n, cols)) * np.float32(0.5)).astype(np.float32)
    x[5] = x[3]            # r = 1 exactly off the diagonal
    x[7] = 2.5             # constant row: NaN row and column
    z, _ = _lib.operand_fill(ctx, ctx.from_numpy(x), precision=_lib.PREC_F16X3)
    assert z.kind == 2
    for stripe in (n, 257):
        two = consumers.pearson_edges(z, cutoff, stripe_rows=stripe, upper_only=upper, fuse=False)
        one = consumers.pearson_edges(z, cutoff, stripe_rows=stripe, upper_only=upper, fuse=True)
        assert len(two[2]) > 50
        for a, b in zip(one, two):
            assert a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    fe = consumers.FusedEdges(ctx, capacity=16)  # far too small: the call repeats itself with room
    got = fe.block(z, z, cutoff, upper_only=upper)
    want = consumers.pearson_edges(z, cutoff, stripe_rows=n, upper_only=upper, fuse=False)
    for a, b in zip(got, want):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    fe.free()


def test_device_radix_sort_of_a_dense_edge_list(ctx):
    """The hand-written LSD radix sort behind skr_pearson_gemm_edges (fused_edges.hip; VERDICT r2 #6: no library sort) on
    lists far longer than a chunk: every cell of a 3 000 x 2 900 block kept (8.7 M entries: 8 192-key chunks, a
    two-level scan of the digit table), global offsets that put set bits into the third byte of both fields, full and
    upper-triangle variants — rows, columns and values equal to np.nonzero order of the block computed the two-step way."""
    from seekr_amd import _lib, consumers
    rng = np.random.default_rng(5)
    xa = (rng.binomial(40, 0.06, size=(3000, 1024)) * np.float32(0.5)).astype(np.float32)
    xb = (rng.binomial(40, 0.06, size=(2900, 1024)) * np.float32(0.5)).astype(np.float32)
    za, _ = _lib.operand_fill(ctx, ctx.from_numpy(xa), precision=_lib.PREC_F16X3)
    zb, _ = _lib.operand_fill(ctx, ctx.from_numpy(xb), precision=_lib.PREC_F16X3)
    r = ctx.empty(3000, 2900)
    _lib.pearson_gemm_op(ctx, za, zb, r)
    full = r.to_numpy()
    fe = consumers.FusedEdges(ctx, capacity=1 << 24)
    for row0, col0, upper in ((0, 0, False), (70000, 131000, False), (65000, 66000, True)):
        got = fe.block(za, zb, -2.0, row_global0=row0, col_global0=col0, upper_only=upper)
        gi, gj = np.meshgrid(np.arange(row0, row0 + 3000, dtype=np.int64), np.arange(col0, col0 + 2900, dtype=np.int64), indexing="ij")
        keep = (full != 0) & ((gj > gi) if upper else (gj != gi))
        ii, jj = np.nonzero(keep)
        assert len(got[0]) == len(ii) > (3_000_000 if upper else 8_000_000)
        assert np.array_equal(got[0], (ii + row0).astype(np.uint32)) and np.array_equal(got[1], (jj + col0).astype(np.uint32))
        assert np.array_equal(got[2].view(np.uint32), full[ii, jj].view(np.uint32))
    fe.free()
