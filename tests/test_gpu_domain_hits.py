"""skr_run_pieces_ge (csrc/domain_hits.hip) through the C ABI on uploaded synthetic blocks, and seekr_amd.windows.domain_hits
end to end on a small FASTA target.

The kernel's pieces are compared with tests/domain_hits_model.py's pieces_of_tiling under the kernel's own tiling as exact
integers and float32 bits; after the host merge (windows.merge_pieces) they are compared with hits_of_cells.  Cases:
tests/domain_hits_cases.py, pinned without a GPU by tests/test_domain_hits_cpu.py.  domain_hits is compared with the model on
domain_pearson's r for the same arguments and the same chunk_rows.  Needs a real MI355X: run with `-m gpu`."""
import bisect
import ctypes as C
import os
from collections import Counter

import numpy as np
import pytest

import domain_hits_cases as dc
import domain_hits_model as model
import window_sweep_cases as sc
import windows_cases as wc

pytestmark = pytest.mark.gpu
SENTINEL_U, SENTINEL_F = np.uint32(0xDEADBEEF), np.float32(-12345.5)
FRAME_COLUMNS = ["query", "header", "start", "end", "first_window", "last_window", "n_windows", "n_hot", "peak_r", "peak_start",
                 "peak_end"]


def _ctx():
    from seekr_amd import _lib
    return _lib.default_context()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def sentinel_outputs(ctx, cap):
    return tuple(ctx.from_numpy(np.full((cap, 1), SENTINEL_F if k == 4 else SENTINEL_U)) for k in range(6))


def raw_pieces(ctx, r, nrows, col_begin, col_end, cutoff, seq, max_gap, outs, out_offset=0, row_global0=0, col_global0=0,
               want_nan=True):
    from seekr_amd import _lib
    count, nan = C.c_int64(-1), C.c_int(-1)
    rc = _lib.lib().skr_run_pieces_ge(ctx._h, r._h, nrows, col_begin, col_end, row_global0, col_global0, C.c_float(cutoff),
                                      None if seq is None else seq._h, max_gap, *[None if m is None else m._h for m in outs],
                                      out_offset, C.byref(count), C.byref(nan) if want_nan else None)
    return rc, count.value, nan.value


def global_seq(seq_index, col_begin, col_global0):
    """seq_of_col as the kernel takes it: indexed by global column, the range's own entries at col_global0 + col_begin."""
    out = np.full(col_global0 + col_begin + len(seq_index), 0xFFFFFFF0, dtype=np.uint32)
    out[col_global0 + col_begin:] = seq_index
    return out


def download(outs, lo, n):
    cols = [np.array(m.to_numpy()).reshape(-1)[lo:lo + n] for m in outs]
    return [tuple(int(v) for v in p) for p in zip(cols[0], cols[1], cols[2], cols[3], bits(cols[4]), cols[5])]


def check(parent, nrows, col_begin, col_end, cutoff, seq_index, max_gap, row_global0=0, col_global0=0, r_dev=None):
    """Kernel against model on one range of one parent: the pieces exactly, the merged pieces against the hits of the cells,
    the NaN flag.  Returns (pieces, hits)."""
    from seekr_amd.windows import merge_pieces
    ctx = _ctx()
    r = ctx.from_numpy(parent) if r_dev is None else r_dev
    seq = None if seq_index is None else ctx.from_numpy(global_seq(seq_index, col_begin, col_global0))
    where = dict(row_global0=row_global0, col_global0=col_global0)
    rc, count, nan = raw_pieces(ctx, r, nrows, col_begin, col_end, cutoff, seq, max_gap, (None,) * 6, **where)
    assert rc == 0
    outs = sentinel_outputs(ctx, count + 2)
    assert raw_pieces(ctx, r, nrows, col_begin, col_end, cutoff, seq, max_gap, outs, 1, **where) == (0, count, nan)
    got = download(outs, 1, count)
    for k, m in enumerate(outs):
        ends = np.array(m.to_numpy()).reshape(-1)[[0, -1]]
        assert (ends == (SENTINEL_F if k == 4 else SENTINEL_U)).all()
        m.free()
    if seq is not None:
        seq.free()
    if r_dev is None:
        r.free()
    block = parent[:nrows, col_begin:col_end]
    ids = np.zeros(col_end - col_begin, dtype=np.int64) if seq_index is None else np.asarray(seq_index)
    starts = model.kernel_tile_starts(nrows, parent.shape[1], col_begin, col_end)
    shift = col_global0 + col_begin
    want = [(row_global0 + q, shift + a, shift + b, n, pk, shift + pw)
            for q, a, b, n, pk, pw in model.pieces_of_tiling(block, ids, cutoff, max_gap, starts)]
    assert len(got) == len(want), (len(got), len(want))
    assert got == want, next((g, w) for g, w in zip(got, want) if g != w)
    assert nan == int(np.isnan(block).any())
    hits = [(row_global0 + q, shift + a, shift + b, n, pk, shift + pw)
            for q, a, b, n, pk, pw in model.hits_of_cells(block, ids, cutoff, max_gap)]
    cols = [np.array(c, dtype=np.int64) for c in zip(*got)] if got else [np.empty(0, np.int64)] * 6
    merged = merge_pieces(cols[0], cols[1] - shift, cols[2] - shift, cols[3], cols[4].astype(np.uint32).view(np.float32),
                          cols[5] - shift, ids, max_gap)  # (columns of the range: a table of 4 * 10^9 windows is not made here)
    merged = [(int(q), int(a) + shift, int(b) + shift, int(n), int(pk), int(pw) + shift)
              for q, a, b, n, pk, pw in zip(merged[0], merged[1], merged[2], merged[3], bits(merged[4]), merged[5])]
    assert merged == hits
    return got, hits


def ragged_seq(rng, width, cuts=5):
    seq = np.zeros(width, dtype=np.int64)
    for c in rng.integers(1, max(width, 2), size=min(cuts, width - 1)):
        seq[c:] += 1
    return seq


# ---- the kernel ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c[0] for c in dc.PLANTED])
def test_planted_cases(name):
    parent, col_begin, col_end, seq_index, cutoff, max_gap = dc.planted_case(name)
    pieces, hits = check(parent, parent.shape[0], col_begin, col_end, cutoff, seq_index, max_gap, col_global0=11)
    print("%s: %d pieces, %d hits" % (name, len(pieces), len(hits)))
    assert len(pieces) > len(hits) > 0


@pytest.mark.parametrize("width", dc.WIDTHS)
def test_widths_and_misaligned_first_segments(width):
    """Every width at col_begin 0 ... 3 in a parent wider than the range (ld > cols, and ld odd: the rows start at every
    phase of a 16-byte line), with and without sequences."""
    rng = np.random.default_rng(width)
    found = 0
    for col_begin in range(4):
        ld = col_begin + width + 5 + (col_begin + width) % 2
        parent = dc.random_block(rng, 3, ld, density=rng.choice([0.1, 0.5]))
        for max_gap, seq_index in ((0, None), (2, ragged_seq(rng, width)), (1, dc.seq_of(width, "every"))):
            found += len(check(parent, 3, col_begin, col_begin + width, 0.25, seq_index, max_gap, row_global0=7, col_global0=3)[0])
    assert found > 0


def test_many_rows_and_far_global_offsets():
    rng = np.random.default_rng(300)
    parent = dc.random_block(rng, 300, 1027, density=0.2)
    pieces, _ = check(parent, 300, 0, 1027, 0.25, ragged_seq(rng, 1027), 1, row_global0=5, col_global0=9)
    assert len({p[0] for p in pieces}) == 300
    pieces, _ = check(parent, 1, 2, 1027, 0.25, None, 0, row_global0=4000000000, col_global0=4000000000 - 1027)
    assert len(pieces) > 10 and all(p[0] == 4000000000 and 4000000000 - 1025 <= p[1] <= p[5] <= p[2] < 4000000000 for p in pieces)


@pytest.mark.parametrize("pattern", ["none", "all", "alternating", "neighbours", "nan"])
def test_patterns(pattern):
    n = 0
    for width, col_begin in ((5, 1), (1025, 0), (2051, 3)):
        parent = dc.pattern_block(pattern, 3, col_begin + width + 3, dc.CUTOFF)
        starts = model.kernel_tile_starts(3, parent.shape[1], col_begin, col_begin + width)
        for which, max_gap in (("none", 0), ("none", 1), ("every", 2), ("at_1024", 1)):
            seq_index = dc.seq_of(width, which, col_begin)
            pieces, hits = check(parent, 3, col_begin, col_begin + width, dc.CUTOFF, seq_index, max_gap)
            n += len(pieces)
            if pattern == "none":
                assert pieces == []
            if pattern == "all" and which == "none":
                assert len(hits) == 3 and len(pieces) == sum(len(s) for s in starts)  # one piece per tile, one hit per sequence
            if pattern == "all" and which == "every":
                assert len(hits) == len(pieces) == 3 * width  # 1 024 pieces in a tile
            if pattern == "alternating" and max_gap == 0 and width == 2051:
                per_tile = Counter((p[0], bisect.bisect_right(starts[p[0]], p[1] - col_begin)) for p in pieces)
                assert max(per_tile.values()) == 512  # every other column of a whole tile
    assert (n == 0) == (pattern == "none")


@pytest.mark.parametrize("cutoff", [0.0, -0.0, -1e-30, -0.25])
def test_zero_and_negative_cutoffs(cutoff):
    parent = dc.pattern_block("zeros", 3, 2060, 0.0)
    parent[1] = -parent[1]
    pieces, hits = check(parent, 3, 1, 2052, cutoff, dc.seq_of(2051, "at_1023", 1), 1)
    assert len(hits) > 0 and {h[4] for h in hits} <= {int(bits(np.float32(1e-30))[0]), 0}  # the peak is 1e-30 or +0.0, never -0.0


@pytest.mark.parametrize("max_gap", dc.MAX_GAPS)
def test_max_gaps_and_boundaries(max_gap):
    """Sparse hot cells (gaps of hundreds of columns) over four tiles, every max_gap against every boundary set."""
    rng = np.random.default_rng(50 + max_gap)
    ctx = _ctx()
    parent = dc.random_block(rng, 3, 4107, density=0.002)
    parent[:, [1021, 1022, 1023, 1024, 1025, 1026, 2046, 2047, 2048, 2049]] = np.float32(0.5)  # hot around the boundaries
    r = ctx.from_numpy(parent)
    joined = 0
    for which in dc.BOUNDARY_SETS:
        for col_begin in (0, 2):
            pieces, hits = check(parent, 3, col_begin, col_begin + 4100, 0.25, dc.seq_of(4100, which, col_begin), max_gap, r_dev=r)
            joined += len(pieces) - len(hits)
            if which == "none":  # seq_of_col NULL is one sequence
                assert check(parent, 3, col_begin, col_begin + 4100, 0.25, None, max_gap, r_dev=r) == (pieces, hits)
    r.free()
    assert joined > 0


def test_three_long_rows():
    rng = np.random.default_rng(65536)
    parent = dc.random_block(rng, 3, 65536, density=0.01)
    pieces, hits = check(parent, 3, 0, 65536, 0.25, ragged_seq(rng, 65536, cuts=40), 50)
    assert len(pieces) > len(hits) > 100


def test_contract_of_the_c_entry_point():
    ctx = _ctx()
    rng = np.random.default_rng(8)
    parent = dc.random_block(rng, 4, 2100, density=0.3)
    seq_index = ragged_seq(rng, 2048)
    want, _ = check(parent, 4, 3, 2051, 0.25, seq_index, 1)
    n = len(want)
    assert n > 50
    r, seq = ctx.from_numpy(parent), ctx.from_numpy(global_seq(seq_index, 3, 0))
    call = lambda outs, off, **kw: raw_pieces(ctx, r, 4, 3, 2051, 0.25, seq, 1, outs, off, **kw)  # noqa: E731
    nan = int(np.isnan(parent[:, 3:2051]).any())
    assert call((None,) * 6, 0) == (0, n, nan)                                     # count only
    assert call((None,) * 6, 0, want_nan=False) == (0, n, -1)                      # saw_nan may be NULL
    small = sentinel_outputs(ctx, 5 + n - 1)
    assert call(small, 5) == (0, n, nan) and call(small, 5 + n) == (0, n, nan)     # one cell short; an offset beyond the outputs
    for k, m in enumerate(small):
        assert (np.array(m.to_numpy()) == (SENTINEL_F if k == 4 else SENTINEL_U)).all()
    exact, again = sentinel_outputs(ctx, 5 + n), sentinel_outputs(ctx, 5 + n)
    assert call(exact, 5) == (0, n, nan) and call(again, 5) == (0, n, nan)         # out_offset > 0, and the same bytes twice
    assert download(exact, 5, n) == want
    for a, b in zip(exact, again):
        assert np.array(a.to_numpy()).tobytes() == np.array(b.to_numpy()).tobytes()
    short = ctx.from_numpy(global_seq(seq_index, 3, 0)[:2050])
    assert raw_pieces(ctx, r, 4, 3, 2051, 0.25, short, 1, (None,) * 6)[0] == -1   # SKR_ERR_INVALID: seq_of_col too short
    assert raw_pieces(ctx, r, 4, 3, 2051, 0.25, seq, 1, (None,) * 6, col_global0=1)[0] == -1
    assert raw_pieces(ctx, r, 4, 3, 2051, 0.25, seq, -1, (None,) * 6)[0] == -1
    assert raw_pieces(ctx, r, 4, 3, 2051, 0.25, seq, 1, exact[:5] + (None,))[0] == -1
    assert raw_pieces(ctx, r, 4, 3, 2051, 0.25, seq, 1, (exact[4],) + exact[1:])[0] == -1  # a float vector where rows go
    assert raw_pieces(ctx, r, 0, 3, 2051, 0.25, seq, 1, exact) == (0, 0, 0) and raw_pieces(ctx, r, 4, 7, 7, 0.25, seq, 1, exact) == (0, 0, 0)
    assert raw_pieces(ctx, r, 4, 3, 2051, 0.25, seq, 1 << 40, (None,) * 6)[:2] == (0, len(check(parent, 4, 3, 2051, 0.25, seq_index, 5000)[0]))
    for m in small + exact + again + (r, seq, short):
        m.free()


def test_piece_list_grows_and_keeps_its_pieces():
    from seekr_amd import consumers
    ctx = _ctx()
    rng = np.random.default_rng(9)
    parent = dc.random_block(rng, 5, 3000, density=0.3)
    want, _ = check(parent, 5, 0, 3000, 0.25, None, 0)
    r = ctx.from_numpy(parent)
    found = consumers.PieceList(ctx, capacity=4)
    n1, _ = consumers.run_pieces(r, 0.25, found, nrows=2)
    n2, _ = consumers.run_pieces(r.view(2, 3), 0.25, found, row_global0=2)
    assert n1 + n2 == len(found) == len(want) and found.capacity >= len(want)
    host = found.to_host()
    assert [tuple(int(v) for v in p) for p in zip(host[0], host[1], host[2], host[3], bits(host[4]), host[5])] == want
    assert consumers.run_pieces(r, 0.25, None) == (len(want), bool(np.isnan(parent).any()))
    found.free()
    r.free()


# ---- domain_hits end to end -----------------------------------------------------------------------------------------------------
WINDOW, SLIDE = 64, 9
CHUNKS = (16, 50, 100000)


def expected_frame(hits, table, seq_index, min_windows=1):
    start, end, header = table["start"].to_numpy(), table["end"].to_numpy(), table["header"].to_numpy()
    rows = [(q, header[a], start[a], end[b], a, b, b - a + 1, n, np.uint32(pk).view(np.float32), start[pw], end[pw])
            for q, a, b, n, pk, pw in hits if b - a + 1 >= min_windows]
    return rows


def frame_rows(frame):
    assert list(frame.columns) == FRAME_COLUMNS
    assert frame["peak_r"].dtype == np.float32 or len(frame) == 0
    return [tuple(row) for row in zip(*(frame[c].to_numpy() for c in FRAME_COLUMNS))]


def same_rows(got, want):
    assert len(got) == len(want), (len(got), len(want))
    for g, w in zip(got, want):
        assert g[:8] == w[:8] and g[9:] == w[9:] and bits(g[8]) == bits(w[8]), (g, w)


@pytest.fixture(scope="module", params=[3, 4])
def domain(request, tmp_path_factory):
    """A target of several records (a long one with repeats, one of a few windows, one shorter than the window, one of k - 2
    letters), queries cut from it and random ones, the background vectors, and domain_pearson's r per chunk size."""
    from seekr_amd.windows import domain_pearson, window_table
    k = request.param
    d = tmp_path_factory.mktemp("domain_hits_k%d" % k)
    rng = np.random.default_rng(70 + k)
    long = sc.long_record(rng, (("random", 900), ("A", 150), ("random", 800), ("GT", 200), ("random", 700)))
    records = [long, wc.random_seq(rng, 300), wc.random_seq(rng, 40), wc.random_seq(rng, k - 2), wc.random_seq(rng, 500)]
    names = ["long", "some", "short", "tiny", "last"]
    queries = [long[300:520], long[1900:2200], records[4][100:400], wc.random_seq(rng, 250), records[1][:200] + long[1000:1100]]
    paths = {"target": str(d / "target.fa"), "query": str(d / "query.fa"), "unrelated": str(d / "unrelated.fa")}
    for key, (nm, seqs) in (("target", (names, records)), ("query", (["q%d" % i for i in range(5)], queries)),
                            ("unrelated", (["u0", "u1"], [wc.random_seq(rng, 1500), wc.random_seq(rng, 900)]))):
        with open(paths[key], "w") as f:
            f.write("".join(">%s\n%s\n" % (n, s) for n, s in zip(nm, seqs)))
    mean, std = sc.background(k, "Log2.post")
    seq_index = window_table([len(s) for s in records], WINDOW, SLIDE)[0]
    args = (paths["query"], paths["target"], k, WINDOW, SLIDE, mean, std)
    r = {}
    for chunk_rows in CHUNKS:
        r[chunk_rows], table = domain_pearson(*args, chunk_rows=chunk_rows)
    assert r[16].shape == (5, len(seq_index)) and len(set(seq_index.tolist())) == 5
    return dict(k=k, paths=paths, args=args, mean=mean, std=std, seq_index=seq_index, r=r, table=table)


@pytest.mark.parametrize("max_gap,min_windows", [(0, 1), (1, 1), (3, 19)])
def test_domain_hits_equals_the_model_on_domain_pearsons_r(domain, max_gap, min_windows):
    from seekr_amd.windows import domain_hits
    cutoff = 0.3
    frames = {}
    for chunk_rows in CHUNKS:
        r = domain["r"][chunk_rows]
        hits = model.hits_of_cells(r, domain["seq_index"], cutoff, max_gap)
        want = expected_frame(hits, domain["table"], domain["seq_index"], min_windows)
        got = domain_hits(*domain["args"], cutoff=cutoff, max_gap=max_gap, min_windows=min_windows, chunk_rows=chunk_rows)
        same_rows(frame_rows(got), want)
        assert got["query"].dtype == np.int64 and got.attrs["r_cutoff"] == float(np.float32(cutoff))
        assert got.attrs["n_hits"] == len(want) and got.attrs["n_pieces"] >= len(hits)
        assert (got["n_windows"] >= min_windows).all() and len(want) > (3 if min_windows == 1 else 0)
        if min_windows > 1:  # (the copies of the queries span 18 windows and more, the chance hits fewer)
            assert len(want) < len(hits)
        frames[chunk_rows] = got
        print("k=%d max_gap=%d chunk_rows=%d: %d hot, %d pieces, %d hits, %d kept" % (
            domain["k"], max_gap, chunk_rows, int((r >= np.float32(cutoff)).sum()), got.attrs["n_pieces"], len(hits), len(want)))
    # chunk_rows 16 cuts every run of more than 16 windows: more pieces, the same hits wherever r is the same
    assert frames[16].attrs["n_pieces"] > frames[100000].attrs["n_pieces"]
    for chunk_rows in CHUNKS[:2]:
        if np.array_equal(bits(domain["r"][chunk_rows]), bits(domain["r"][100000])):
            same_rows(frame_rows(frames[chunk_rows]), frame_rows(frames[100000]))
        else:
            print("r differs between chunk_rows %d and one chunk (another operand layout): frames not compared" % chunk_rows)


def test_raw_p_mode_is_the_cutoff_mode_at_the_reported_cutoff(domain):
    from seekr_amd.windows import domain_hits, domain_pearson
    a = domain["args"]
    bg, _ = domain_pearson(a[0], domain["paths"]["unrelated"], *a[2:])
    bg = np.array(bg).reshape(-1)
    by_p = domain_hits(*a, fitres=bg, alpha=0.05, max_gap=1)
    cutoff = by_p.attrs["r_cutoff"]
    assert cutoff is not None and float(np.float32(cutoff)) == cutoff and len(by_p) > 0
    by_cutoff = domain_hits(*a, cutoff=cutoff, max_gap=1)
    same_rows(frame_rows(by_p), frame_rows(by_cutoff))
    assert by_p.attrs == by_cutoff.attrs
    hits = model.hits_of_cells(domain["r"][100000], domain["seq_index"], cutoff, 1)
    same_rows(frame_rows(by_p), expected_frame(hits, domain["table"], domain["seq_index"]))
    never = domain_hits(*a, fitres=[("uniform", 0.0, (0.0, 5.0))], alpha=0.05)
    assert len(never) == 0 and never.attrs == {"r_cutoff": None, "n_pieces": 0, "n_hits": 0} and list(never.columns) == FRAME_COLUMNS


def test_method_mode_merges_domain_significants_cells(domain):
    from seekr_amd.windows import domain_hits, domain_significant
    a = domain["args"]
    r = domain["r"][100000]
    fitres = [("norm", 0.0, (0.0, 0.12))]
    cells = domain_significant(*a, fitres, method="fdr_bh", alpha=0.05)
    assert len(cells) > 5
    table = domain["table"]
    row_of = {(h, s): i for i, (h, s) in enumerate(zip(table["header"], table["start"]))}
    hot = np.full(r.shape, np.nan, dtype=np.float32)
    for q, h, s, v in zip(cells["query"], cells["header"], cells["start"], cells["r"]):
        hot[q, row_of[(h, s)]] = v
    for max_gap in (0, 2):
        want = expected_frame(model.hits_of_cells(hot, domain["seq_index"], -np.inf, max_gap), table, domain["seq_index"])
        for chunk_rows in (50, 100000):
            got = domain_hits(*a, fitres=fitres, method="fdr_bh", alpha=0.05, max_gap=max_gap, chunk_rows=chunk_rows)
            same_rows(frame_rows(got), want)
            assert got.attrs["n_pieces"] == len(cells) and got.attrs["r_cutoff"] == cells.attrs["r_cutoff"]
        assert int(got["n_hot"].sum()) == len(cells)


def test_nan_windows_warn_once_and_are_never_hot(domain, capsys):
    from seekr_amd.kmer_counts import NAN_WARNING
    from seekr_amd.windows import domain_hits, domain_pearson
    k = domain["k"]
    mean, std = np.zeros(4 ** k, np.float32), np.ones(4 ** k, np.float32)
    a = domain["args"][:5] + (mean, std)
    capsys.readouterr()
    r, table = domain_pearson(*a, log2="Log2.none")
    tiny = int(np.flatnonzero(domain["seq_index"] == 3)[0])
    assert capsys.readouterr().out.count(NAN_WARNING) == 1 and np.isnan(r[:, tiny]).all() and np.isnan(r).sum() == r.shape[0]
    for chunk_rows in (16, 100000):
        got = domain_hits(*a, cutoff=-2.0, max_gap=5, log2="Log2.none", chunk_rows=chunk_rows)  # everything but NaN is hot
        assert capsys.readouterr().out.count(NAN_WARNING) == 1
        same_rows(frame_rows(got), expected_frame(model.hits_of_cells(r, domain["seq_index"], -2.0, 5), table, domain["seq_index"]))
        assert len(got) == 4 * r.shape[0] and not (got["first_window"] == tiny).any()  # one hit per other record and query
    with pytest.raises(ValueError, match="NaN"):
        domain_hits(*a, fitres=[("norm", 0.0, (0.0, 0.12))], method="fdr_bh", log2="Log2.none")
    assert capsys.readouterr().out.count(NAN_WARNING) == 1


def test_empty_inputs_and_no_hit(domain, tmp_path):
    from seekr_amd.windows import domain_hits
    a = domain["args"]
    empty_attrs = {"r_cutoff": 0.5, "n_pieces": 0, "n_hits": 0}
    none = domain_hits(np.empty((0, 4 ** domain["k"]), np.float32), *a[1:], cutoff=0.5)
    assert list(none.columns) == FRAME_COLUMNS and len(none) == 0 and none.attrs == empty_attrs
    empty = tmp_path / "empty.fa"
    empty.write_text("")
    none = domain_hits(a[0], str(empty), *a[2:], cutoff=0.5)
    assert list(none.columns) == FRAME_COLUMNS and len(none) == 0 and none.attrs == empty_attrs
    high = domain_hits(*a, cutoff=1.5)
    assert list(high.columns) == FRAME_COLUMNS and len(high) == 0 and high.attrs == {"r_cutoff": 1.5, "n_pieces": 0, "n_hits": 0}
    with pytest.raises(ValueError, match="exactly one"):
        domain_hits(*a)
    with pytest.raises(TypeError):
        domain_hits(a[0], ["ACGT" * 40], *a[2:], cutoff=0.5)


def test_command_writes_the_frame(domain, tmp_path):
    import subprocess
    import sys
    from seekr_amd.windows import domain_hits
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    mean, std, out = str(tmp_path / "mean.npy"), str(tmp_path / "std.npy"), str(tmp_path / "hits.csv")
    np.save(mean, domain["mean"])
    np.save(std, domain["std"])
    argv = ["seekr_domain_hits", domain["paths"]["query"], domain["paths"]["target"], mean, std, "-k", str(domain["k"]), "-w", str(WINDOW),
            "-s", str(SLIDE), "-c", "0.3", "-g", "1", "-mw", "2", "-o", out]
    code = "import sys; sys.argv = %r; from seekr_amd.console_scripts import console_domain_hits as f; f()" % (argv,)
    proc = subprocess.run([sys.executable, "-c", code], cwd=root, capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0, proc.stderr
    frame = domain_hits(*domain["args"], cutoff=0.3, max_gap=1, min_windows=2)
    with open(out) as f:
        lines = f.read().splitlines()
    assert lines[0] == ",".join(FRAME_COLUMNS) and len(lines) == 1 + len(frame) > 1
    for line, row in zip(lines[1:], frame_rows(frame)):
        assert line.split(",") == [str(v) for v in row]
