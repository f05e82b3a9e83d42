"""skr_hist_key_digits / skr_hist_edges (csrc/distribution.hip) and what stands on them — distribution.r_histogram,
r_order_statistics, r_quantiles, density_cutoff, pearson_distribution, kmer_leiden(density=), the seekr_r_distribution
command — against the numpy models of tests/distribution_model.py.  Every expectation is an exact uint64 count or a
float32 bit pattern: there is no tolerance anywhere in this file."""
import ctypes as C
import functools
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

import distribution_model as dm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = 5  # what the caller's arrays hold before a call: the calls ADD

NEG_ZERO, POS_NAN, NEG_NAN = (np.array([b], np.uint32).view(np.float32)[0] for b in (0x80000000, 0x7fc00000, 0xffc00001))
SPECIAL = np.array([0.0, NEG_ZERO, np.inf, -np.inf, POS_NAN, NEG_NAN, 1e-45, -1e-45, 1.1754942e-38, -1.1754942e-38,
                    3.4028235e38, -3.4028235e38], dtype=np.float32)


def _ctx():
    from seekr_amd import _lib
    return _lib.default_context()


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def steps(x, n):
    return dm.unkey(np.array([int(dm.key(np.float32(x)).reshape(-1)[0]) + n], np.uint32))[0]


def mixed(rng, shape, special=0.1):
    """r-like values around 0 with the special ones strewn in."""
    x = rng.normal(0, 0.05, shape).astype(np.float32)
    hit = rng.random(shape) < special
    x[hit] = rng.choice(SPECIAL, int(hit.sum()))
    return x


def embed(block, col_begin, right):
    """The block inside a matrix whose other cells are NaN: a cell read outside the range shows up in the nan count."""
    m = np.full((block.shape[0], col_begin + block.shape[1] + right), POS_NAN, np.float32)
    m[:, col_begin:col_begin + block.shape[1]] = block
    return m


def counted(m, nrows, col_begin, col_end, row0, col0, upper):
    """The cells the device counts, by the rule of the header: r's own column index is the global one's offset."""
    block = m[:nrows, col_begin:col_end]
    if not upper:
        return block.reshape(-1)
    i = np.arange(nrows)[:, None] + row0
    j = np.arange(col_begin, col_end)[None, :] + col0
    return block[j > i]


def check_key(ctx, m, d, where, shift, nbits, prefixes, prefix_bits, tag=None):
    from seekr_amd import distribution
    hist, nan = np.full((len(prefixes), 1 << nbits), BASE, np.uint64), np.full(1, BASE, np.uint64)
    distribution.hist_key_block(d, shift, nbits, prefixes, prefix_bits, hist, nan, **where)
    want, want_nan = dm.hist_pass(counted(m, where.get("nrows", m.shape[0]), where.get("col_begin", 0), where.get("col_end", m.shape[1]),
                                          where.get("row_global0", 0), where.get("col_global0", 0), where.get("upper_only", False)),
                                  shift, nbits, prefixes, prefix_bits)
    assert np.array_equal(hist - np.uint64(BASE), want), (tag, where, shift, nbits, prefixes)
    assert int(nan[0]) - BASE == want_nan, (tag, where)


def check_edges(ctx, m, d, where, edges, tag=None):
    from seekr_amd import distribution
    edges = np.ascontiguousarray(edges, np.float32)
    hist, extra = np.full(len(edges) - 1, BASE, np.uint64), np.full(3, BASE, np.uint64)
    distribution.hist_edges_block(d, edges, hist, extra, **where)
    want = dm.edge_hist(counted(m, where.get("nrows", m.shape[0]), where.get("col_begin", 0), where.get("col_end", m.shape[1]),
                                where.get("row_global0", 0), where.get("col_global0", 0), where.get("upper_only", False)), edges)
    assert np.array_equal(hist - np.uint64(BASE), want[0]), (tag, where, len(edges))
    assert tuple(int(v) - BASE for v in extra) == want[1:], (tag, where, len(edges))


def data_prefixes(values, prefix_bits, n):
    """n distinct prefixes: those of the data first, then values no cell has."""
    v = np.asarray(values, np.float32).reshape(-1)
    have = sorted(set((dm.key(v[~np.isnan(v)]) >> np.uint32(32 - prefix_bits)).tolist()))
    out, p = have[:n - 1], 0
    while len(out) < n:
        if p not in have:
            out.append(p)
        p += 1
    return out


EDGES17 = np.linspace(-0.2, 0.2, 17, dtype=np.float32)


# ---- (a) the kernel on uploaded blocks ----------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [1, 3, 4, 5, 1021, 1024, 1025, 2051])
def test_shapes_and_alignments(width):
    """Every width x rows 1, 2, 7 x col_begin 0, 1, 2, 3, 5 x a leading dimension that equals / exceeds the range's end."""
    ctx = _ctx()
    rng = np.random.default_rng(width)
    for rows in (1, 2, 7):
        block = mixed(rng, (rows, width))
        for col_begin in (0, 1, 2, 3, 5):
            for right in (0, 3):
                m = embed(block, col_begin, right)
                d = ctx.from_numpy(m)
                where = dict(col_begin=col_begin, col_end=col_begin + width)
                check_key(ctx, m, d, where, 20, 12, [0], 0)
                check_key(ctx, m, d, where, 10, 10, data_prefixes(block, 12, 8), 12)
                check_edges(ctx, m, d, where, EDGES17)
                d.free()


def test_short_nrows_and_empty_ranges():
    ctx = _ctx()
    m = mixed(np.random.default_rng(1), (7, 40))
    d = ctx.from_numpy(m)
    for where in (dict(nrows=3), dict(nrows=0), dict(col_begin=9, col_end=9), dict(nrows=5, col_begin=2, col_end=33)):
        check_key(ctx, m, d, where, 20, 12, [0], 0)
        check_edges(ctx, m, d, where, EDGES17)
    d.free()


def test_grid_stride_70000_rows():
    ctx = _ctx()
    m = mixed(np.random.default_rng(2), (70000, 3))
    d = ctx.from_numpy(m)
    check_key(ctx, m, d, {}, 20, 12, [0], 0)
    check_key(ctx, m, d, dict(upper_only=True, row_global0=0, col_global0=69990), 20, 12, [0], 0)
    check_edges(ctx, m, d, {}, EDGES17)
    d.free()


@pytest.mark.parametrize("row0,col0,what", [(0, 100, "above"), (0, 3, "first column"), (5, 0, "last column"), (2, 0, "inside"),
                                            (100, 0, "below")])
def test_upper_only_offsets(row0, col0, what):
    """The global diagonal above the block (every cell counts), across its first column, across its last column, inside,
    below it (no cell counts)."""
    ctx = _ctx()
    rng = np.random.default_rng(row0 * 7 + col0)
    for shape, col_begin in (((7, 9), 0), ((7, 9), 3), ((3, 1030), 1)):
        m = embed(mixed(rng, shape), col_begin, 2)
        d = ctx.from_numpy(m)
        where = dict(col_begin=col_begin, col_end=col_begin + shape[1], row_global0=row0, col_global0=col0, upper_only=True)
        n = len(counted(m, shape[0], col_begin, col_begin + shape[1], row0, col0, True))
        if shape == (7, 9) and col_begin == 0:
            assert {"above": n == 63, "below": n == 0}.get(what, 0 < n < 63), (what, n)
        check_key(ctx, m, d, where, 20, 12, [0], 0, what)
        check_edges(ctx, m, d, where, EDGES17, what)
        d.free()


def value_sets():
    rng = np.random.default_rng(9)
    near = np.float32(0.0123)
    low = (np.uint32(dm.key(np.float32(0.031))) & np.uint32(0xfffffc00)) | rng.integers(0, 1024, (40, 333)).astype(np.uint32)
    return {
        "one value": np.full((300, 1500), 0.37, np.float32),  # every lane hits one bin
        "two neighbours": np.where(rng.random((60, 700)) < 0.5, near, steps(near, 1)).astype(np.float32),
        "equal in 22 key bits": dm.unkey(low).reshape(40, 333),  # only the last pass tells them apart
        "special": rng.choice(SPECIAL, (33, 1030)).astype(np.float32),
        "two decimals": np.round(rng.normal(0, 0.2, (50, 1027)), 2).astype(np.float32),
    }


@pytest.mark.parametrize("name", ["one value", "two neighbours", "equal in 22 key bits", "special", "two decimals"])
def test_value_sets_all_three_passes(name):
    """Every pass of the descent with prefix sets of 1 and 8 (one of which matches no cell), the edge rule, and the descent
    itself on the device's passes."""
    from seekr_amd import distribution
    ctx = _ctx()
    m = value_sets()[name]
    d = ctx.from_numpy(m)
    check_key(ctx, m, d, {}, 20, 12, [0], 0, name)
    for shift, nbits, prefix_bits in ((10, 10, 12), (0, 10, 22)):
        for n in (1, 8):
            prefixes = data_prefixes(m, prefix_bits, n)
            check_key(ctx, m, d, {}, shift, nbits, prefixes, prefix_bits, name)
        check_key(ctx, m, d, {}, shift, nbits, data_prefixes(np.float32([np.nan]), prefix_bits, 1), prefix_bits, name)  # matches no cell
    check_edges(ctx, m, d, {}, EDGES17, name)
    check_edges(ctx, m, d, {}, np.float32([-3.4028235e38, 0, 3.4028235e38]), name)

    def one_pass(shift, nbits, prefixes, prefix_bits):
        hist, nan = np.zeros((len(prefixes), 1 << nbits), np.uint64), np.zeros(1, np.uint64)
        distribution.hist_key_block(d, shift, nbits, prefixes, prefix_bits, hist, nan)
        return hist, int(nan[0])

    flat = m.reshape(-1)
    want = dm.unkey(np.sort(dm.key(flat[~np.isnan(flat)])))
    ranks = sorted({0, len(want) - 1, len(want) // 2, len(want) // 3, 1, len(want) - 2})
    got, total = distribution.descend(ranks, one_pass)
    assert total == len(want) and np.array_equal(bits(got), bits(want[ranks])), name
    d.free()


@pytest.mark.parametrize("n_edges", [2, 3, 257, 4097])
def test_edge_tables(n_edges):
    """Cells on every edge, one float32 step to either side of the first and the last edge, the special values, and
    values between the edges."""
    ctx = _ctx()
    rng = np.random.default_rng(n_edges)
    edges = np.sort(rng.normal(0, 0.1, 3 * n_edges).astype(np.float32))
    edges = np.unique(edges)[:n_edges]
    assert len(edges) == n_edges
    cells = np.concatenate([edges, edges, [steps(edges[0], -1), steps(edges[0], 1), steps(edges[-1], -1), steps(edges[-1], 1)],
                            SPECIAL, rng.normal(0, 0.12, 5000).astype(np.float32)]).astype(np.float32)
    rng.shuffle(cells)
    width = 1027
    rows = -(-len(cells) // width)
    m = np.concatenate([cells, rng.choice(edges, rows * width - len(cells))]).astype(np.float32).reshape(rows, width)
    d = ctx.from_numpy(m)
    check_edges(ctx, m, d, {}, edges)
    check_edges(ctx, m, d, dict(col_begin=1, col_end=1000, upper_only=True, row_global0=0, col_global0=2), edges)
    d.free()


def test_c_abi_refuses_bad_tables():
    from seekr_amd import _lib
    ctx = _ctx()
    d = ctx.from_numpy(np.zeros((2, 8), np.float32))
    out = np.zeros(8192 + 8, np.uint64)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    head = (ctx._h, d._h, 2, 0, 8, 0, 0, 0)

    def edges_rc(e):
        e = np.ascontiguousarray(e, np.float32)
        return _lib.lib().skr_hist_edges(*head, ptr(e), len(e), ptr(out), ptr(out[4100:]), ptr(out[4101:]), ptr(out[4102:]))

    def key_rc(shift, nbits, prefix_bits, prefixes):
        p = np.ascontiguousarray(prefixes, np.uint32)
        return _lib.lib().skr_hist_key_digits(*head, shift, nbits, prefix_bits, ptr(p), len(p), ptr(out), ptr(out[8192:]))

    for e in ([1.0], [1, 1], [2, 1], [0, np.inf], [0, np.nan], np.arange(4098)):
        assert edges_rc(e) == -1, e
    assert edges_rc([0, 1]) == 0 and edges_rc(np.arange(4097)) == 0
    for bad in ((20, 13, 0, [0]), (20, 0, 0, [0]), (25, 10, 0, [0]), (10, 10, 12, [1, 1]), (10, 10, 12, [4096]), (10, 10, 12, list(range(9))),
                (10, 11, 12, list(range(8))), (20, 12, 0, [0, 1]), (10, 10, 33, [0]), (10, 10, 12, [])):
        assert key_rc(*bad) == -1, bad
    assert key_rc(20, 12, 0, [0]) == 0 and key_rc(10, 10, 12, list(range(8))) == 0 and key_rc(20, 12, 1, [0, 1]) == 0
    d.free()


def test_the_same_numbers_on_every_run():
    from seekr_amd import distribution
    ctx = _ctx()
    m = mixed(np.random.default_rng(4), (64, 3001))
    d = ctx.from_numpy(m)
    runs = []
    for _ in range(3):
        hist, nan = np.zeros((1, 4096), np.uint64), np.zeros(1, np.uint64)
        distribution.hist_key_block(d, 20, 12, [0], 0, hist, nan)
        runs.append((hist.tobytes(), int(nan[0])))
    assert runs[0] == runs[1] == runs[2]
    d.free()


# ---- (b) end to end -----------------------------------------------------------------------------------------------------
def counts_case(name):
    """Host count matrices: (counts, counts2 or None).  Each holds a constant row (a NaN row of r) and a duplicated row
    (runs of tied cells)."""
    rng = np.random.default_rng(len(name))
    cols = 256 if "256" in name else 4096
    n1, n2 = (300, 130) if cols == 256 else (200, 130)
    c1 = rng.gamma(2.0, 1.0, (n1, cols)).astype(np.float32)
    c1[7] = 3.0
    c1[11] = c1[5]
    c1[n1 - 1] = c1[5]
    if "self" in name:
        return c1, None
    c2 = rng.gamma(2.0, 1.0, (n2, cols)).astype(np.float32)
    c2[3] = c2[9]
    c2[n2 - 2] = 1.5
    return c1, c2


CASES = ["self 256", "two sets 256", "self 4096", "two sets 4096"]


@functools.lru_cache(maxsize=None)
def prepared(name):
    from seekr_amd import neighbors
    c1, c2 = counts_case(name)
    return neighbors._prepare(_ctx(), c1, c1 if c2 is None else c2, c2 is None)


@functools.lru_cache(maxsize=None)
def reference_values(name):
    """The counted cells of r, downloaded block by block through the sweep's own pearson_gemm_op calls (unsplit)."""
    from seekr_amd import consumers
    z, z2 = prepared(name)
    parts = []

    def visit(buf, nrows, col_begin, col_end, row_global0, col_global0, upper_only):
        m = np.array(buf.to_numpy(0, nrows))
        parts.append(counted(m, nrows, col_begin, col_end, row_global0, col_global0, upper_only).copy())

    sweep = consumers.Sweep(z, z2)
    sweep.run(visit)
    sweep.free()
    values = np.concatenate(parts)
    values.setflags(write=False)
    return values


def tie_ranks(want):
    """Ranks 0, M - 1, the middle, and a whole run of tied cells with the ranks just outside it."""
    same = np.flatnonzero(bits(want[1:]) == bits(want[:-1]))
    assert len(same)
    first = int(same[len(same) // 2])
    while first > 0 and bits(want[first - 1]) == bits(want[first]):
        first -= 1
    last = first
    while last + 1 < len(want) and bits(want[last + 1]) == bits(want[first]):
        last += 1
    run = list(range(first, min(last, first + 3) + 1)) + [last]
    spread = list(range(0, len(want), len(want) // 10))  # more distinct values than one pass takes prefixes
    return [0, len(want) - 1, len(want) // 2] + [r for r in (first - 1, *run, last + 1) if 0 <= r < len(want)] + spread


@pytest.mark.parametrize("name", CASES)
def test_end_to_end_against_the_models_for_every_split(name):
    from seekr_amd import distribution
    z, z2 = prepared(name)
    values = reference_values(name)
    n_cells = distribution.n_cells(z, z2)
    assert len(values) == n_cells
    nan = int(np.isnan(values).sum())
    assert nan == (z.rows - 1 if z2 is None else z2.rows + z.rows - 1)  # the constant row(s) of the case
    want_sorted = dm.unkey(np.sort(dm.key(values[~np.isnan(values)])))
    m = len(want_sorted)
    assert m == n_cells - nan
    edges = distribution.make_edges(None, 200, (-1, 1))
    want_hist = dm.edge_hist(values, edges)
    tight = np.float32([-0.01, 0.0, 0.01, 0.02])
    want_tight = dm.edge_hist(values, tight)
    ranks = tie_ranks(want_sorted)
    assert len(set(bits(want_sorted[ranks]).tolist())) > 8  # more distinct prefixes than one pass takes, by the last pass
    qs = [0, 1, 0.5, Fraction(1, 3), "0.999"]
    want_q = want_sorted[[dm.quantile_rank(q, m) for q in qs]]
    for stripe in (64, 100, None):
        for panel in (50, None):
            kw = dict(stripe_rows=z.rows if stripe is None else stripe, panel_rows=panel)
            hist, below, above, got_nan = distribution.r_histogram(z, z2, edges=edges, **kw)
            assert hist.dtype == np.uint64 and np.array_equal(hist, want_hist[0]) and (below, above, got_nan) == want_hist[1:], kw
            hist, below, above, got_nan = distribution.r_histogram(z, z2, edges=tight, **kw)
            assert np.array_equal(hist, want_tight[0]) and (below, above, got_nan) == want_tight[1:], kw
            got = distribution.r_order_statistics(z, z2, ranks=ranks, **kw)
            assert got.dtype == np.float32 and np.array_equal(bits(got), bits(want_sorted[ranks])), kw
            got_q, got_m = distribution.r_quantiles(z, z2, q=qs, **kw)
            assert got_m == m and np.array_equal(bits(got_q), bits(want_q)), kw
    hist, below, above, got_nan = distribution.r_histogram(z, z2, bins=200, range=(-1, 1))
    assert np.array_equal(hist, want_hist[0])
    for bad in ([m], [-1]):
        with pytest.raises(ValueError, match="outside"):
            distribution.r_order_statistics(z, z2, ranks=bad)


@pytest.mark.parametrize("name", ["self 256", "two sets 4096"])
def test_pearson_distribution_front_end(name):
    from seekr_amd import distribution
    c1, c2 = counts_case(name)
    values = reference_values(name)
    want_sorted = dm.unkey(np.sort(dm.key(values[~np.isnan(values)])))
    m = len(want_sorted)
    res = distribution.pearson_distribution(c1, c2, bins=64, range=(-0.5, 0.5), q=[0.25, 0.75], densities=[0.01, Fraction(1, 7)],
                                            stripe_rows=128)
    edges = np.linspace(np.float32(-0.5), np.float32(0.5), 65, dtype=np.float32)
    want = dm.edge_hist(values, edges)
    assert np.array_equal(bits(res.edges), bits(edges)) and np.array_equal(res.hist, want[0])
    assert (res.below, res.above, res.nan) == want[1:] and res.n_cells == len(values) and res.n_values == m
    assert np.array_equal(bits(res.quantiles), bits(want_sorted[[dm.quantile_rank(q, m) for q in (0.25, 0.75)]]))
    assert np.array_equal(bits(res.cutoffs), bits(want_sorted[[dm.density_rank(d, m) for d in (0.01, Fraction(1, 7))]]))
    only_q = distribution.pearson_distribution(c1, c2, q=[0.5])
    assert only_q.hist is None and only_q.nan == want[3] and bits(only_q.quantiles)[0] == bits(want_sorted[(m - 1) // 2])


def test_density_cutoff_is_the_edge_count():
    """NaN-free rows: pearson_edges at the cutoff holds exactly the cells >= c, at least m of them; one float32 step
    higher it holds fewer than m."""
    from seekr_amd import consumers, distribution, neighbors, significant
    ctx = _ctx()
    c = np.random.default_rng(12).gamma(2.0, 1.0, (300, 256)).astype(np.float32)
    c[40] = c[41]
    z, _ = neighbors._prepare(ctx, c, c, True)
    parts = []
    sweep = consumers.Sweep(z)
    sweep.run(lambda buf, nrows, col_begin, col_end, row_global0, col_global0, upper_only: parts.append(
        counted(np.array(buf.to_numpy(0, nrows)), nrows, col_begin, col_end, row_global0, col_global0, upper_only).copy()))
    sweep.free()
    values = np.concatenate(parts)
    assert not np.isnan(values).any()
    total = len(values)
    for density in (0.01, Fraction(1, 1000), 1e-9):
        m = max(1, int(Fraction(density) * total // 1))
        cut = distribution.density_cutoff(z, density, stripe_rows=128)
        assert cut > 0 and bits(cut) == bits(np.sort(values)[total - m])
        at = len(consumers.pearson_edges(z, float(cut))[2])
        assert at == int((values >= cut).sum()) and at >= m
        assert len(consumers.pearson_edges(z, float(significant.float32_steps(cut, 1)))[2]) < m
    z.free()


def test_kmer_leiden_density_is_the_cutoff_it_finds(tmp_path):
    from seekr_amd import _lib, distribution
    from seekr_amd import pearson as pearson_mod
    from seekr_amd.kmer_counts import BasicCounter
    from seekr_amd.kmer_leiden import kmer_leiden
    from seekr_amd.synthetic import profile_seqs
    seqs, _ = profile_seqs(6, 120, 400)
    fa = tmp_path / "seqs.fa"
    with open(fa, "w") as f:
        for i, s in enumerate(seqs):
            f.write(">tx%d\n%s\n" % (i, s))
    c = BasicCounter(str(fa), k=3, silent=True)
    c.get_counts()
    np.save(tmp_path / "mean.npy", c.mean)
    np.save(tmp_path / "std.npy", c.std)
    args = (str(fa), str(tmp_path / "mean.npy"), str(tmp_path / "std.npy"), 3)
    again = BasicCounter(str(fa), mean=np.load(tmp_path / "mean.npy"), std=np.load(tmp_path / "std.npy"), k=3, silent=True)
    again.get_counts()
    ctx = _ctx()
    x = ctx.from_numpy(np.ascontiguousarray(again.counts, dtype=np.float32))
    z, _ = _lib.operand_fill(ctx, x, None, pearson_mod._precision_for(np.dtype(np.float32), True))
    cut = distribution.density_cutoff(z, 0.05)
    z.free()
    x.free()
    assert cut > 0
    by_cutoff = kmer_leiden(*args, pearsoncutoff=float(cut), csvfile=str(tmp_path / "cut"), edges="nonzero")
    by_density = kmer_leiden(*args, density=0.05, csvfile=str(tmp_path / "den"), edges="nonzero")
    assert by_density.tobytes() == by_cutoff.tobytes()
    for name in ("nodes", "edges"):
        assert (tmp_path / ("den_%s_leiden.csv" % name)).read_bytes() == (tmp_path / ("cut_%s_leiden.csv" % name)).read_bytes()
    n_edges = len((tmp_path / "den_edges_leiden.csv").read_text().splitlines()) - 1
    assert n_edges >= int(0.05 * (120 * 119 // 2))


def test_command_gives_the_numbers_of_the_api(tmp_path):
    from seekr_amd import distribution
    c1, c2 = counts_case("two sets 256")
    np.save(tmp_path / "a.npy", c1)
    np.save(tmp_path / "b.npy", c2)
    res = distribution.pearson_distribution(c1, c2, bins=20, range=(-1, 1), q=["0.5", "9/10"], densities=["0.01"])
    code = ("import sys; sys.argv = ['seekr_r_distribution', %r, %r, '-bi', '--bins', '20', '--range', '-1', '1', '-q', '0.5', '9/10', "
            "'--density', '0.01', '-o', %r]; from seekr_amd.console_scripts import console_r_distribution; console_r_distribution()"
            % (str(tmp_path / "a.npy"), str(tmp_path / "b.npy"), str(tmp_path / "hist.csv")))
    proc = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0, proc.stderr
    want_out = ["%s,%s" % (q, v) for q, v in zip(["0.5", "9/10"], res.quantiles)] + ["density 0.01,%s" % res.cutoffs[0]]
    assert proc.stdout.splitlines() == want_out
    lines = (tmp_path / "hist.csv").read_text().splitlines()
    assert lines[0] == "left,right,count" and len(lines) == 1 + 20 + 3
    assert [int(line.split(",")[2]) for line in lines[1:21]] == res.hist.tolist()
    assert [line.split(",")[0] for line in lines[1:21]] == [str(e) for e in res.edges[:-1]]
    assert [int(line.split(",")[2]) for line in lines[21:]] == [res.below, res.above, res.nan]
