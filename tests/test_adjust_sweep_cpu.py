"""tools/adjust_sweep.py without a device: the restated chunk rule, the size list, the byte patterns, the symmetry list,
and the condition under which comparing the device with tests/adj_rule.py means anything — with the generators' ties
the reference's result is a function of the p-value alone (numpy's unstable argsort cannot change it)."""
import os
import sys

import numpy as np
import pytest

import adj_rule

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import adjust_sweep as sweep  # noqa: E402

W = 4096  # 256 CUs x 16 waves


def test_chunk_rule_at_its_boundaries():
    assert sweep.plan_chunks(1) == (512, 1)
    assert sweep.plan_chunks(513) == (512, 2)
    assert sweep.plan_chunks(512 * W - 1) == (512, W)
    assert sweep.plan_chunks(512 * W) == (512, W)
    assert sweep.plan_chunks(512 * W + 1) == (576, 3641)  # ceil(2 097 153 / 576): a step down
    assert sweep.plan_chunks(576 * W) == (576, W)
    assert sweep.plan_chunks(576 * W + 1) == (640, 3687)
    assert sweep.plan_chunks(8128 * W) == (8128, W)
    assert sweep.plan_chunks(8128 * W + 1) == (8192, 4065)
    assert sweep.plan_chunks(8192 * W - 1) == (8192, W)
    assert sweep.plan_chunks(8192 * W) == (8192, W)
    assert sweep.plan_chunks(8192 * W + 1) == (8192, W + 1)
    assert sweep.plan_chunks(sweep.LARGE_N ** 2) == (8192, 65539)
    assert sweep.plan_chunks(512 * 1664 + 1, cus=104) == (576, 1480)  # another device: W = 1 664
    for n in (1, 4096, 8 * W + 5, 700 * W + 3, 9000 * W):
        chunk, n_chunks = sweep.plan_chunks(n)
        assert chunk % 64 == 0 and 512 <= chunk <= 8192 and (n_chunks - 1) * chunk < n <= n_chunks * chunk
    # table_words = 256 n_chunks crosses the scan tile at n = 8 192 (17 chunks of 512), and its third level at 65 537 chunks
    assert sweep.scan_levels(256 * sweep.plan_chunks(8192)[1]) == 1 and sweep.scan_levels(256 * sweep.plan_chunks(8193)[1]) == 2
    assert sweep.scan_levels(256 * 65536) == 2 and sweep.scan_levels(256 * 65537) == 3
    assert sweep.scan_levels(256 * sweep.plan_chunks(sweep.LARGE_N ** 2)[1]) == 3
    assert sweep.scan_levels(4096 ** 2) == 2 and sweep.scan_levels(4096 ** 2 + 1) == 3


@pytest.mark.parametrize("quick", [True, False])
def test_size_list_holds_every_named_boundary(quick):
    ns = sweep.sizes(quick, 256, 1)
    have = set(ns)
    assert len(ns) > 300 and set(range(1, 201)) <= have
    for j in range(1, 17):
        assert {64 * j - 1, 64 * j, 64 * j + 1} <= have
    for j in (1, 2, 3, 16, 17, 1024, 1025):
        assert {4096 * j - 1, 4096 * j, 4096 * j + 1} <= have
    assert {512 * W - 1, 512 * W + 1, 8192 * W - 1, 8192 * W + 1} <= have
    stepped = [n for n in ns if 512 * W < n < 8192 * W]
    assert len(stepped) >= 6
    downs = [n for n in stepped + [512 * W] if n + 1 in have and sweep.plan_chunks(n + 1)[1] < sweep.plan_chunks(n)[1]]
    assert downs, "no size where n_chunks steps down as n grows"
    last = {(n - 1) % sweep.plan_chunks(n)[0] + 1 for n in ns if sweep.plan_chunks(n)[1] > 1}
    assert {1, 63, 64, 65} <= last
    assert {(n - 1) % 576 + 1 for n in stepped if sweep.plan_chunks(n)[0] == 576} >= {1, 63, 64, 65}
    if quick:  # above 70 000 only the boundary neighbours remain
        named = set()
        for v in sweep.boundary_sizes(256).values():
            named.update(v)
        assert {n for n in ns if n > sweep.ALL_METHODS_UP_TO} <= named
    assert set(sweep.sizes(True, 256, 1)) <= set(sweep.sizes(False, 256, 1))  # quick only thins


def test_upper_mode_sizes_sit_on_the_boundaries():
    ns = sweep.upper_sizes(256)
    assert {2, 3, 33, 91, 92, 2049, 6001} <= set(ns)
    assert 91 * 90 // 2 == 4095 and 512 * W < 2049 * 2048 // 2 < 576 * W
    targets = set()
    for v in sweep.boundary_sizes(256).values():
        targets.update(v)
    for m in range(2, 6400):  # every N whose number of tests is within one of a named boundary is in the list
        t = m * (m - 1) // 2
        if {t - 1, t, t + 1} & targets:
            assert m in ns, m


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_byte_patterns_vary_exactly_in_their_bytes(dtype):
    patterns = sweep.byte_patterns(dtype)
    width = np.dtype(dtype).itemsize
    assert len(set(patterns)) == len(patterns) and () in patterns and tuple(range(width)) in patterns
    if dtype == np.float32:
        assert len(patterns) == 16
    else:
        assert {(b,) for b in range(8)} | {(0, 2, 4, 6), (1, 3, 5, 7), (0, 1, 2, 3), (4, 5, 6, 7)} <= set(patterns)
    assert {len(p) % 2 for p in patterns} == {0, 1}  # odd and even pass counts: both ping-pong buffers
    for varying in patterns:
        for n in (449 * 448 // 2, 100003):
            v = sweep.pattern_values(np.random.default_rng([n, width] + list(varying)), n, dtype, varying)
            assert v.dtype == dtype and sweep.varying_bytes(v) == tuple(varying)
            assert not np.signbit(v).any() and np.isfinite(v).all() and (v < 1).all()
            if not varying:
                assert len(np.unique(v)) == 1


def test_keys_restate_the_device_conversion():
    for dtype, utype in ((np.float32, np.uint32), (np.float64, np.uint64)):
        nan = np.array(sweep.NAN_BITS[dtype], dtype=utype).view(dtype)
        assert np.isnan(nan).all()
        v = np.concatenate([nan, np.array([-np.inf, -2.5, -1e-300 if dtype == np.float64 else -1e-40, -0.0, 0.0,
                                           np.finfo(dtype).smallest_subnormal, 0.5, 1.0, 7.25, np.inf], dtype=dtype)])
        k = sweep.keys_of(v)
        assert (k[:len(nan)] == ~utype(0)).all()
        rest = k[len(nan):]
        assert rest[3] == rest[4] and (np.diff(rest.astype(object)) >= 0).all() and len(set(rest.tolist())) == len(rest) - 1


def _assert_function_of_p(p, methods):
    """correct(p[perm]) == correct(p)[perm], and equal inputs get equal outputs: the reference is unambiguous on p."""
    rng = np.random.default_rng(len(p))
    perm = rng.permutation(len(p))
    _, first, inverse = np.unique(p, return_index=True, return_inverse=True)
    with np.errstate(all="ignore"):
        for m in methods:
            c = adj_rule.correct(p, m, sweep.ALPHA)
            assert np.array_equal(adj_rule.correct(p[perm], m, sweep.ALPHA), c[perm], equal_nan=True), m
            assert np.array_equal(c, c[first][inverse.reshape(-1)], equal_nan=True), m
            again = sweep.reference_many(p, [(m, sweep.ALPHA)])[0]  # the shared-argsort reference is adj_rule.correct
            assert again.dtype == c.dtype and np.array_equal(again, c, equal_nan=True), m


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n", [1, 2, 17, 1000, 70000])
def test_mixture_ties_leave_the_reference_unambiguous(dtype, n):
    p = sweep.mixture(np.random.default_rng([3, n]), n, dtype)
    if n >= 1000:
        assert (p == 0).any() and (p == 1).any() and len(np.unique(p)) < n
    for name, q in sweep.two_stage_variants(p).items():
        assert q.dtype == dtype
        _assert_function_of_p(q, sweep.NON_HOMMEL if name == "given" else sweep.TWO_STAGE)
        order = np.argsort(p)  # the variants are non-decreasing in p: p's order sorts them too
        assert (np.diff(q[order]) >= 0).all()
        with np.errstate(all="ignore"):
            for m in sweep.TWO_STAGE:
                shared = sweep.reference_many(q, [(m, sweep.ALPHA)], order)[0]
                assert np.array_equal(shared, adj_rule.correct(q, m, sweep.ALPHA))
                assert sweep.r1_of(q, m, order=order) == sweep.r1_of(q, m)
    if n >= 1000:
        variants = sweep.two_stage_variants(p)
        for m in sweep.TWO_STAGE:
            assert sweep.r1_of(variants["r1=0"], m) == 0 and sweep.r1_of(variants["r1=n"], m) == n
            assert 0 < sweep.r1_of(p, m) < n


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_hommel_ties_leave_the_reference_unambiguous(dtype):
    for n in (3, 257, 3001):
        p = sweep.hommel_values(np.random.default_rng([5, n]), n, dtype)
        _assert_function_of_p(p, ["hommel"])
    assert len(np.unique(p)) < len(p)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_byte_pattern_ties_leave_the_reference_unambiguous(dtype):
    for varying in sweep.byte_patterns(dtype):
        p = sweep.pattern_values(np.random.default_rng([7] + list(varying)), 20011, dtype, varying)
        _assert_function_of_p(p, ["holm", "fdr_bh"])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n", [1000, 70000])
def test_special_values_leave_the_reference_unambiguous(dtype, n):
    for inf in (False, True):
        p, nan_cells = sweep.specials(np.random.default_rng([9, n]), n, dtype, inf=inf)
        assert not nan_cells.any() and not np.isnan(p).any()
        outside = p[(p < 0) | (p > 1)]
        assert len(np.unique(outside)) == len(outside) and np.isinf(p).sum() == int(inf)  # ties only inside [0, 1]
        assert np.signbit(p[p == 0]).any() and not np.signbit(p[p == 0]).all()
        assert ((p > 0) & (p < np.finfo(dtype).tiny)).any()
        _assert_function_of_p(p, sweep.NON_HOMMEL)
    p, nan_cells = sweep.specials(np.random.default_rng([9, n]), n, dtype, inf=True, nan=True)
    assert np.array_equal(np.isnan(p), nan_cells) and nan_cells.sum() == 49
    bits = p.view(np.uint32 if dtype == np.float32 else np.uint64)[nan_cells]
    assert set(bits.tolist()) == set(sweep.NAN_BITS[dtype])
    with np.errstate(all="ignore"):
        assert np.array_equal(np.isnan(adj_rule.correct(p, "holm")), nan_cells)
    _assert_function_of_p(p, ["holm", "holm-sidak"])


def test_symmetry_list_gives_both_verdicts_for_every_edit_kind():
    seen = sweep.symmetry_verdicts(seed=1)
    sweep.assert_both_verdicts(seen)
    for n in (2, 31, 32, 33, 70, 97, 1025):
        names = {e[0].split(" at ", 1)[1] for e in sweep.symmetry_edits(n, np.float32, np.random.default_rng(n))}
        assert {"(0,1)", "(0,N-1)", "(N-2,N-1)", "random", "diagonal"} <= names
        assert (n < 32) or {"tile corner %d" % c for c in range(4)} <= names
        assert (n % 32 == 0) or "partial tile" in names


def test_symmetry_sweep_agrees_with_the_rule_on_whole_matrices():
    """The sweep's own logic with the host in the device's place: the verdict on the edited pair alone equals
    values_symmetric of the whole matrix (asserted inside the sweep), and nothing is reported."""
    class Host:
        def __init__(self, a):
            self.a = a  # the sweep edits `a` in place and re-uploads the rows it touched

        def upload(self, rows, row0=0):
            assert np.array_equal(self.a[row0:row0 + 1], rows, equal_nan=True)

        def free(self):
            pass

    ns = tuple(range(1, 71)) + (95, 96, 97, 127, 128, 129)
    with np.errstate(all="ignore"):
        bad = sweep.sweep_symmetry(seed=1, verbose=False, ns=ns, upload=Host, verdict=lambda d: adj_rule.values_symmetric(d.a))
    assert not bad, bad
