"""skr_pair_kmers / skr_group_colstat and seekr_amd.explain on the device, bit for bit (uint32 views) against the numpy
models of tests/explain_cases.py.  The low-level tests hand the kernels float32 matrices as they are, and the API tests
download z from the device, so row standardisation's own rounding is never in play."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import explain_cases as ec

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POISON = 0xDEADBEEF


def _ctx():
    from seekr_amd import _lib
    return _lib.default_context()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def device_pairs(z1, z2, rows, cols, top, largest=True, factors=True, guard_rows=2):
    """skr_pair_kmers on device matrices z1 / z2 (z2 None: z1 twice) into outputs `guard_rows` rows longer than the list
    and poisoned; returns [idx, val, f1, f2] of the list's rows as uint32 after checking that the guard rows survived."""
    from seekr_amd import _lib
    ctx = _ctx()
    n = len(rows)
    d_rows = ctx.from_numpy(np.asarray(rows, np.uint32) if n else np.zeros(1, np.uint32))
    d_cols = ctx.from_numpy(np.asarray(cols, np.uint32) if n else np.zeros(1, np.uint32))
    poison = np.full((n + guard_rows, top), POISON, np.uint32)
    outs = [ctx.from_numpy(poison)] + [ctx.from_numpy(poison.view(np.float32)) for _ in range(3 if factors else 1)]
    try:
        _lib.pair_kmers(ctx, z1, z1 if z2 is None else z2, d_rows, d_cols, n, top, largest, *outs)
    finally:
        host = [bits(np.array(m.to_numpy())) for m in outs]
        for m in [d_rows, d_cols] + outs:
            m.free()
    for h in host:
        assert (h[n:] == POISON).all(), "cells behind the list were written"
    return [h[:n] for h in host]


def assert_pairs(got, want, what=""):
    for name, g, w in zip(("idx", "contribution", "z_row", "z_col"), got, want):
        w = bits(w)
        if not np.array_equal(g, w):
            e, t = np.argwhere(g != w)[0]
            raise AssertionError("{} {}: pair {} slot {}: device {:#x}, model {:#x}".format(what, name, e, t, int(g[e, t]), int(w[e, t])))


# ---- pairs: widths and alignment ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", ec.PAIR_WIDTHS)
def test_pairs_every_width_and_phase(w):
    """9 rows and all 81 ordered pairs, (i, i) included: with a width that is no multiple of four the two rows of a pair
    start at every combination of 16-byte phases.  top beyond the width pads."""
    ctx = _ctx()
    z = ec.pair_rows(9, w, 1000 + w)
    rows, cols = ec.all_pairs(9)
    d = ctx.from_numpy(z)
    try:
        for top in ec.PAIR_TOPS:
            for largest in (True, False):
                want = ec.pair_model(z, z, rows, cols, top, largest)
                assert_pairs(device_pairs(d, None, rows, cols, top, largest), want, "w=%d top=%d largest=%s" % (w, top, largest))
    finally:
        d.free()


def test_pairs_selection_stress():
    """W = 4 099: products ascending with the column (every cell of every step beats the bound, so the buffer is flushed
    at every step), descending, all equal (the list is columns 0 .. top - 1) and of two values."""
    ctx = _ctx()
    z = ec.stress_rows()
    rows = np.array([0, 1, 4, 2, 3, 2], np.uint32)
    cols = np.array([4, 4, 4, 4, 4, 3], np.uint32)
    d = ctx.from_numpy(z)
    try:
        for top in (1, 10, 256):
            for largest in (True, False):
                want = ec.pair_model(z, z, rows, cols, top, largest)
                got = device_pairs(d, None, rows, cols, top, largest)
                assert_pairs(got, want, "top=%d largest=%s" % (top, largest))
                assert list(got[0][2]) == list(range(top))  # all equal
    finally:
        d.free()


def test_pairs_special_values():
    """NaN columns, products that are -0 and +0, inf, inf * 0, overflow to inf, subnormal products and subnormal factors:
    the model is IEEE float32 and so is the kernel."""
    ctx = _ctx()
    z1, z2 = ec.special_rows()
    with np.errstate(all="ignore"):
        prod = z1[:, None, :] * z2[None, :, :]
    tiny = np.finfo(np.float32).tiny
    assert np.isnan(prod).any() and np.isinf(prod).any() and ((prod != 0) & (np.abs(prod) < tiny)).any()
    assert (bits(prod) == 0x80000000).any() and (bits(prod) == 0).any() and ((z1 != 0) & (np.abs(z1) < tiny)).any()
    rows, cols = ec.all_pairs(6, 6)
    d1, d2 = ctx.from_numpy(z1), ctx.from_numpy(z2)
    try:
        for top in (10, 256):
            for largest in (True, False):
                want = ec.pair_model(z1, z2, rows, cols, top, largest)
                assert_pairs(device_pairs(d1, d2, rows, cols, top, largest), want, "top=%d largest=%s" % (top, largest))
    finally:
        d1.free()
        d2.free()


# ---- pairs: list shapes ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_pairs", [0, 1, 255, 256, 257])
def test_pairs_list_lengths(n_pairs):
    """Duplicate and unsorted pairs among them; no pairs launches nothing and writes nothing."""
    ctx = _ctx()
    rng = np.random.default_rng(n_pairs)
    z = ec.pair_rows(20, 65, 77)
    rows, cols = rng.integers(0, 20, n_pairs).astype(np.uint32), rng.integers(0, 20, n_pairs).astype(np.uint32)
    if n_pairs >= 255:
        rows[10:14], cols[10:14] = rows[3], cols[3]  # duplicates
    d = ctx.from_numpy(z)
    try:
        assert_pairs(device_pairs(d, None, rows, cols, 10), ec.pair_model(z, z, rows, cols, 10))
    finally:
        d.free()


def test_pairs_more_than_65535():
    """E = 70 000 at W = 64: above what a 16-bit grid dimension holds."""
    ctx = _ctx()
    rng = np.random.default_rng(70000)
    z = ec.pair_rows(300, 64, 78)
    rows, cols = rng.integers(0, 300, 70000).astype(np.uint32), rng.integers(0, 300, 70000).astype(np.uint32)
    d = ctx.from_numpy(z)
    try:
        got = device_pairs(d, None, rows, cols, 3, factors=False)
    finally:
        d.free()
    assert_pairs(got, ec.pair_model(z, z, rows, cols, 3)[:2])


def test_pairs_without_factor_outputs():
    ctx = _ctx()
    z = ec.pair_rows(9, 257, 79)
    rows, cols = ec.all_pairs(9)
    d = ctx.from_numpy(z)
    try:
        got = device_pairs(d, None, rows, cols, 10, factors=False)
    finally:
        d.free()
    assert len(got) == 2
    assert_pairs(got, ec.pair_model(z, z, rows, cols, 10)[:2])


# ---- pairs: sets and views ---------------------------------------------------------------------------------------------------
def test_pairs_two_sets_and_row_views():
    """N1 != N2, and operands that are row views at a non-zero offset of one parent (width 1 027: a view's first row
    starts at another 16-byte phase than the parent)."""
    ctx = _ctx()
    parent = ec.pair_rows(12, 1027, 80)
    d = ctx.from_numpy(parent)
    v1, v2 = d.view(3, 5), d.view(6, 6)
    other = ec.pair_rows(4, 1027, 81)
    d_other = ctx.from_numpy(other)
    try:
        rows, cols = ec.all_pairs(5, 6)
        assert_pairs(device_pairs(v1, v2, rows, cols, 10), ec.pair_model(parent[3:8], parent[6:12], rows, cols, 10), "views")
        rows, cols = ec.all_pairs(12, 4)
        assert_pairs(device_pairs(d, d_other, rows, cols, 64, False), ec.pair_model(parent, other, rows, cols, 64, False), "two sets")
    finally:
        for m in (v1, v2, d_other, d):
            m.free()


# ---- the index guards, made safe ---------------------------------------------------------------------------------------------
def test_pairs_index_guard():
    """z1 is a view of rows 0..4 of a 9-row parent and a pair names row 7: a missing guard would read valid memory and
    the call would wrongly succeed.  Expected: the error with the first bad pair, its slots padded, every other pair as
    the model has it."""
    from seekr_amd import _lib
    ctx = _ctx()
    parent = ec.pair_rows(9, 65, 82)
    d = ctx.from_numpy(parent)
    v = d.view(0, 5)
    rows = np.array([0, 1, 2, 7, 3, 4, 6], np.uint32)
    cols = np.array([1, 2, 3, 0, 4, 0, 1], np.uint32)
    poison = np.full((7, 4), POISON, np.uint32)
    try:
        for z1, z2, r, c in ((v, d, rows, cols), (d, v, cols, rows)):
            d_rows, d_cols = ctx.from_numpy(r), ctx.from_numpy(c)
            outs = [ctx.from_numpy(poison)] + [ctx.from_numpy(poison.view(np.float32)) for _ in range(3)]
            with pytest.raises(_lib.BadIndex, match="pair 3") as info:
                _lib.pair_kmers(ctx, z1, z2, d_rows, d_cols, 7, 4, True, *outs)
            assert info.value.first_bad == 3 and isinstance(info.value, ValueError)
            host = [bits(np.array(m.to_numpy())) for m in outs]
            for m in [d_rows, d_cols] + outs:
                m.free()
            good = np.array([0, 1, 2, 4, 5])
            want = ec.pair_model(parent, parent, r[good], c[good], 4)
            assert_pairs([h[good] for h in host], want)
            assert (host[0][[3, 6]] == ec.PAD_IDX).all() and all((h[[3, 6]] == ec.PAD_BITS).all() for h in host[1:])
    finally:
        v.free()
        d.free()


def test_groups_index_guard():
    from seekr_amd import _lib
    ctx = _ctx()
    x = ec.group_matrix(9, 33, 83)
    d = ctx.from_numpy(x)
    v = d.view(0, 5)
    order = ctx.from_numpy(np.array([0, 2, 4, 1, 7, 3], np.uint32))
    mean, sd = ctx.empty(2, 33), ctx.empty(2, 33)
    try:
        with pytest.raises(ValueError, match="entry 4 of order"):
            _lib.group_colstat(ctx, v, order, [0, 3, 6], mean, sd)
        _lib.group_colstat(ctx, d, order, [0, 3, 6], mean, sd)  # the same list is fine on the parent
        want = ec.group_model(x, [0, 2, 4, 1, 7, 3], [0, 3, 6])
        assert np.array_equal(bits(mean.to_numpy()), bits(want[0])) and np.array_equal(bits(sd.to_numpy()), bits(want[1]))
    finally:
        for m in (mean, sd, order, v, d):
            m.free()


def test_refusals():
    from seekr_amd import _lib
    ctx = _ctx()
    z = ctx.from_numpy(ec.pair_rows(4, 16, 84))
    narrow = ctx.from_numpy(ec.pair_rows(4, 15, 85))
    idx = ctx.from_numpy(np.zeros(2, np.uint32))
    out_i, out_v = ctx.empty(2, 4, np.uint32), ctx.empty(2, 4)
    try:
        with pytest.raises(ValueError, match="columns"):
            _lib.pair_kmers(ctx, z, narrow, idx, idx, 2, 4, True, out_i, out_v)
        with pytest.raises(ValueError, match="cells"):
            _lib.pair_kmers(ctx, z, z, idx, idx, 2, 5, True, out_i, out_v)
        with pytest.raises(ValueError, match="n_pairs"):
            _lib.pair_kmers(ctx, z, z, idx, idx, 3, 1, True, out_i, out_v)
        with pytest.raises(ValueError):
            _lib.pair_kmers(ctx, z, z, out_v, idx, 2, 4, True, out_i, out_v)  # rows must be uint32
        with pytest.raises(ValueError, match="decrease"):
            _lib.group_colstat(ctx, z, idx, [0, 2, 1], out_v)
        with pytest.raises(ValueError, match="order holds"):
            _lib.group_colstat(ctx, z, idx, [0, 3], out_v)
        kmax, _ = _lib.topk_merge_limits()
        assert kmax == _lib.TOPK_MERGE_KMAX
    finally:
        for m in (z, narrow, idx, out_i, out_v):
            m.free()


# ---- groups ------------------------------------------------------------------------------------------------------------------
def device_groups(x_dev, labels, want_sd=True):
    from seekr_amd import _lib
    ctx = _ctx()
    uniq, order, starts = ec.order_of(labels)
    g, w = len(uniq), x_dev.cols
    d_order = ctx.from_numpy(order)
    poison = np.full((g + 1, w), POISON, np.uint32).view(np.float32)
    mean, sd = ctx.from_numpy(poison), (ctx.from_numpy(poison) if want_sd else None)
    try:
        _lib.group_colstat(ctx, x_dev, d_order, starts, mean, sd)
        out = [bits(np.array(m.to_numpy())) for m in (mean, sd) if m is not None]
    finally:
        for m in (d_order, mean, sd):
            if m is not None:
                m.free()
    for h in out:
        assert (h[g:] == POISON).all(), "cells behind the last group were written"
    return [h[:g] for h in out], order, starts


@pytest.mark.parametrize("w", ec.GROUP_WIDTHS)
def test_groups_widths_and_sizes(w):
    """Group sizes 1, 2, 3, around the 256-row tile and its multiples, and 1 025, interleaved in row order, under int64
    labels that are negative, far apart and beyond 32 bits."""
    ctx = _ctx()
    labels = ec.interleaved_labels()
    x = ec.group_matrix(len(labels), w, 2000 + w)
    d = ctx.from_numpy(x)
    try:
        (mean, sd), order, starts = device_groups(d, labels)
    finally:
        d.free()
    want_mean, want_sd = ec.group_model(x, order, starts)
    assert np.array_equal(mean, bits(want_mean)), "mean, w=%d" % w
    assert np.array_equal(sd, bits(want_sd)), "sd, w=%d" % w
    assert np.isnan(want_sd[np.diff(starts) == 1]).all()


def test_groups_discriminating_case_and_one_group():
    """One group holding all 1 025 rows of the case whose sequential mean is not the correctly rounded one
    (test_explain_cpu.test_discriminating_case), with and without sd."""
    ctx = _ctx()
    x = ec.discriminating_group()
    labels = np.zeros(len(x), np.int32)
    d = ctx.from_numpy(x)
    try:
        (mean, sd), order, starts = device_groups(d, labels)
        (mean_only,), _, _ = device_groups(d, labels, want_sd=False)
    finally:
        d.free()
    want_mean, want_sd = ec.group_model(x, order, starts)
    assert np.array_equal(mean, bits(want_mean)) and np.array_equal(sd, bits(want_sd)) and np.array_equal(mean_only, mean)
    assert (mean[0] != bits(x.astype(np.float64).mean(axis=0).astype(np.float32))).any()


def test_groups_every_row_its_own_and_special_cells():
    """G = N = 300 (sd all NaN), then NaN, inf and -0 cells in groups of several rows."""
    ctx = _ctx()
    x = ec.group_matrix(300, 17, 90)
    d = ctx.from_numpy(x)
    try:
        (mean, sd), order, starts = device_groups(d, np.arange(300)[::-1].copy())
    finally:
        d.free()
    want_mean, _ = ec.group_model(x, order, starts, want_sd=False)
    assert np.array_equal(mean, bits(want_mean)) and np.array_equal(mean, bits(x[::-1])) and np.isnan(sd.view(np.float32)).all()
    y = ec.group_matrix(40, 19, 91)
    y[3, 0], y[5, 1], y[6, 1], y[7, 2], y[8, 2] = np.nan, np.inf, -np.inf, np.inf, 1.0
    y[:, 3] = -0.0
    labels = np.arange(40) % 3
    d = ctx.from_numpy(y)
    try:
        (mean, sd), order, starts = device_groups(d, labels)
    finally:
        d.free()
    want_mean, want_sd = ec.group_model(y, order, starts)
    assert np.array_equal(mean, bits(want_mean)) and np.array_equal(sd, bits(want_sd))
    assert (mean[:, 3] == 0).all()  # a sum of -0 is +0, as numpy's


# ---- through the API ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def planted():
    import significant_cases as sc
    return sc.planted_counts()[:120].astype(np.float32), sc.backgrounds()["empirical_f32"]


def device_z(counts):
    from seekr_amd import _lib
    ctx = _ctx()
    x = ctx.from_numpy(np.ascontiguousarray(counts, dtype=np.float32))
    z = _lib.row_standardize(ctx, x)
    out = np.array(z.to_numpy())
    x.free()
    z.free()
    return out


def test_pair_kmers_on_significant_pairs():
    from seekr_amd import explain
    from seekr_amd.significant import significant_pairs
    counts, bg = planted()
    sig = significant_pairs(counts, bg)
    assert len(sig) >= 20
    kmers = ["w%d" % j for j in range(counts.shape[1])]
    res = explain.pair_kmers(counts, sig, top=7, kmers=kmers)
    z = device_z(counts)
    want = ec.pair_model(z, z, sig.rows, sig.cols, 7)
    assert_pairs([bits(a) for a in (res.idx, res.contribution, res.z_row, res.z_col)], want)
    assert res.words() == [[kmers[j] for j in row] for row in want[0]]
    # the terms are those of r: their mean over ALL columns is the pair's r to float32 accuracy
    full = explain.pair_kmers(counts, sig.rows[:5], sig.cols[:5], top=256)
    assert np.allclose(full.contribution.astype(np.float64).sum(axis=1) / counts.shape[1], sig.r[:5], atol=2e-6)
    # a device matrix, the smallest terms, no standardisation, a second set
    ctx = _ctx()
    d = ctx.from_numpy(counts)
    second = counts[:50] * np.float32(2)
    low = explain.pair_kmers(d, sig.rows, sig.cols % 50, counts2=second, top=3, largest=False, row_standardize=False)
    d.free()
    assert_pairs([bits(a) for a in (low.idx, low.contribution, low.z_row, low.z_col)],
                 ec.pair_model(counts, second, sig.rows, sig.cols % 50, 3, False))
    with pytest.raises(ValueError, match="first bad one"):
        explain.pair_kmers(counts, sig.rows, sig.cols, counts2=counts[:2])


def test_pair_kmers_constant_row():
    """A constant row standardises to NaN: every term is NaN, NaN ties go to the smaller column."""
    from seekr_amd import explain
    counts = planted()[0][:4].copy()
    counts[2] = 3.0
    res = explain.pair_kmers(counts, [2, 0], [1, 2], top=5)
    assert (res.idx == np.arange(5, dtype=np.uint32)).all() and np.isnan(res.contribution).all() and np.isnan(res.z_row[0]).all()
    assert not np.isnan(res.z_row[1]).any() and np.isnan(res.z_col[1]).all()


def run_command(function, argv):
    code = "import sys; sys.argv = %r; from seekr_amd.console_scripts import %s; %s()" % (argv, function, function)
    proc = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0, proc.stderr


def test_pair_kmers_command(tmp_path):
    """seekr_pair_kmers on what seekr_significant_pairs (labelled CSV, names) and seekr_nearest (.npy, two files, indices)
    wrote."""
    import pandas as pd
    from itertools import product
    from seekr_amd import explain
    counts, bg = planted()
    x = counts.astype(np.float64)
    names = ["tx%d, v1" % i if i == 4 else "tx%d" % i for i in range(len(x))]
    kmers = ["".join(t) for t in product("AGTC", repeat=4)]
    assert len(kmers) == x.shape[1]
    csv = tmp_path / "counts.csv"
    pd.DataFrame(x, index=names, columns=kmers).to_csv(csv)
    np.save(tmp_path / "bg.npy", bg)
    run_command("console_significant_pairs", ["seekr_significant_pairs", str(csv), "-bg", str(tmp_path / "bg.npy"), "-o", str(tmp_path / "pairs.csv")])
    run_command("console_pair_kmers", ["seekr_pair_kmers", str(csv), str(tmp_path / "pairs.csv"), "-t", "4", "-o", str(tmp_path / "pk.csv")])
    pairs = pd.read_csv(tmp_path / "pairs.csv")
    look = {n: i for i, n in enumerate(names)}
    rows, cols = np.array([look[n] for n in pairs["row"]]), np.array([look[n] for n in pairs["col"]])
    values = pd.read_csv(csv, index_col=0).to_numpy()
    want = explain.pair_kmers(values, rows, cols, top=4, kmers=kmers)
    frame = pd.read_csv(tmp_path / "pk.csv", float_precision="round_trip")
    assert list(frame.columns) == ["row", "col", "rank", "kmer", "contribution", "z_row", "z_col"] and len(frame) == 4 * len(rows) >= 80
    assert list(frame["row"]) == [names[i] for i in rows for _ in range(4)] and list(frame["col"]) == [names[j] for j in cols for _ in range(4)]
    assert list(frame["rank"]) == list(range(4)) * len(rows) and list(frame["kmer"]) == [w for ws in want.words() for w in ws]
    for name, a in (("contribution", want.contribution), ("z_row", want.z_row), ("z_col", want.z_col)):
        assert np.array_equal(bits(frame[name].to_numpy().astype(np.float32)), bits(a.reshape(-1)))
    # .npy input, two files, the list seekr_nearest writes, the smallest terms
    np.save(tmp_path / "a.npy", counts[:6])
    np.save(tmp_path / "b.npy", counts)
    run_command("console_nearest", ["seekr_nearest", str(tmp_path / "a.npy"), str(tmp_path / "b.npy"), "-n", "3", "-o", str(tmp_path / "near.csv"), "-bi"])
    run_command("console_pair_kmers", ["seekr_pair_kmers", str(tmp_path / "a.npy"), str(tmp_path / "b.npy"), str(tmp_path / "near.csv"), "-bi", "-k", "4",
                                       "-t", "2", "--smallest", "-o", str(tmp_path / "pk2.csv")])
    near = pd.read_csv(tmp_path / "near.csv")
    want2 = explain.pair_kmers(counts[:6], near["row"].to_numpy(), near["neighbor"].to_numpy(), counts2=counts, top=2, largest=False, kmers=kmers)
    frame2 = pd.read_csv(tmp_path / "pk2.csv", float_precision="round_trip")
    assert len(frame2) == 2 * 18 and list(frame2["row"]) == [i for i in near["row"] for _ in range(2)]
    assert list(frame2["col"]) == [j for j in near["neighbor"] for _ in range(2)] and list(frame2["kmer"]) == [w for ws in want2.words() for w in ws]
    assert np.array_equal(bits(frame2["contribution"].to_numpy().astype(np.float32)), bits(want2.contribution.reshape(-1)))


def test_group_kmers_api():
    from seekr_amd import explain
    labels = ec.interleaved_labels()[:500]
    x = ec.group_matrix(500, 33, 92)
    res = explain.group_kmers(x, labels, top=40)
    uniq, order, starts = ec.order_of(labels)
    want_mean, want_sd = ec.group_model(x, order, starts)
    assert np.array_equal(res.labels, uniq) and np.array_equal(res.sizes, np.diff(starts)) and res.labels.dtype == np.int64
    assert np.array_equal(bits(res.mean), bits(want_mean)) and np.array_equal(bits(res.sd), bits(want_sd))
    for g in range(len(uniq)):
        assert np.array_equal(res.idx[g, :33], ec.model_order(want_mean[g])) and (res.idx[g, 33:] == ec.PAD_IDX).all()
        assert np.array_equal(bits(res.value[g, :33]), bits(want_mean[g][res.idx[g, :33]]))
    ctx = _ctx()
    d = ctx.from_numpy(x)
    low = explain.group_kmers(d, labels, top=2, largest=False)
    d.free()
    assert np.array_equal(bits(low.mean), bits(want_mean)) and np.array_equal(low.idx[0], ec.model_order(-want_mean[0])[:2])


def test_kmer_leiden_writes_the_kmers_file(tmp_path):
    """kmer_leiden(kmers_top=5, csvfile=...) on a small FASTA against group_kmers of the same counts; without kmers_top
    no such file appears."""
    import pandas as pd
    from seekr_amd import explain
    from seekr_amd.kmer_counts import BasicCounter
    from seekr_amd.kmer_leiden import kmer_leiden
    from seekr_amd.synthetic import profile_seqs
    seqs, _ = profile_seqs(5, 300, 400)
    fa = tmp_path / "seqs.fa"
    with open(fa, "w") as f:
        for i, s in enumerate(seqs):
            f.write(">tx%d\n%s\n" % (i, s))
    c = BasicCounter(str(fa), k=3, silent=True)
    c.get_counts()
    np.save(tmp_path / "mean.npy", c.mean)
    np.save(tmp_path / "std.npy", c.std)
    args = (str(fa), str(tmp_path / "mean.npy"), str(tmp_path / "std.npy"), 3)
    plain = kmer_leiden(*args, pearsoncutoff=0.2, csvfile=str(tmp_path / "plain"), edges="nonzero")
    assert not os.path.exists(tmp_path / "plain_kmers_leiden.csv")
    mem = kmer_leiden(*args, pearsoncutoff=0.2, csvfile=str(tmp_path / "out"), edges="nonzero", kmers_top=5)
    assert np.array_equal(mem, plain)
    for name in ("nodes", "edges"):
        assert (tmp_path / ("out_%s_leiden.csv" % name)).read_bytes() == (tmp_path / ("plain_%s_leiden.csv" % name)).read_bytes()
    again = BasicCounter(str(fa), mean=np.load(tmp_path / "mean.npy"), std=np.load(tmp_path / "std.npy"), k=3, silent=True)
    again.get_counts()
    want = explain.group_kmers(np.asarray(again.counts, dtype=np.float32), mem, top=5, kmers=again.kmers)
    frame = pd.read_csv(tmp_path / "out_kmers_leiden.csv", float_precision="round_trip")
    assert list(frame.columns) == ["Community", "Size", "Rank", "Kmer", "Mean", "Sd"] and len(frame) == 5 * len(want) == 15
    assert list(frame["Community"]) == [g for g in range(3) for _ in range(5)] and list(frame["Rank"]) == list(range(5)) * 3
    assert list(frame["Size"]) == [int(want.sizes[g]) for g in range(3) for _ in range(5)]
    assert list(frame["Kmer"]) == [w for ws in want.words() for w in ws]
    assert np.array_equal(bits(frame["Mean"].to_numpy().astype(np.float32)), bits(want.value.reshape(-1)))
    sd = np.array([want.sd[g, j] for g in range(3) for j in want.idx[g]], np.float32)
    assert np.array_equal(bits(frame["Sd"].to_numpy().astype(np.float32)), bits(sd))
    # the command
    argv = ["seekr_kmer_leiden", *args[:3], "3", "-pco", "0.2", "-cf", str(tmp_path / "cmd"), "--edges", "nonzero", "-kt", "5"]
    run_command("console_kmer_leiden", argv)
    assert (tmp_path / "cmd_kmers_leiden.csv").read_bytes() == (tmp_path / "out_kmers_leiden.csv").read_bytes()
