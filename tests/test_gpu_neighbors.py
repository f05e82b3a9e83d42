"""skr_topk_merge_rows (csrc/topk.hip) and what stands on it — consumers.pearson_topk, neighbors.nearest,
windows.domain_topk, the seekr_nearest command — against the numpy reference of tests/neighbors_cases.py, bit for bit on
the indices and on the uint32 view of the values.  The reference's order is total, so one expectation serves every split
of a row into panels, stripes or chunks."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import neighbors_cases as nc
import windows_cases as wc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ctx():
    from seekr_amd import _lib
    return _lib.default_context()


def same(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(nc.bits(got[1]), nc.bits(want[1]))


def lists(ctx, rows, k, poison=False):
    """Device lists [rows, k]; poison: entries that would win every comparison if they were read."""
    idx = ctx.from_numpy(np.full((rows, k), 5 if poison else 0, np.uint32))
    val = ctx.from_numpy(np.full((rows, k), np.inf if poison else 0, np.float32))
    return idx, val


def merge(ctx, d, k, first, c0, c1, row0, col0, exclude, idx, val):
    from seekr_amd import _lib
    saw = _lib.topk_merge_rows(ctx, d, idx, val, k, first=first, col_begin=c0, col_end=c1, row_global0=row0, col_global0=col0,
                               exclude_diag=exclude, want_nan=True)
    return (idx.to_numpy(), val.to_numpy()), saw


def check_block(ctx, block, k, col_begin=0, right=0, diag="inside", col_global0=7, tag=None):
    """One call on the block embedded in a NaN-poisoned matrix: lists and saw_nan against the reference."""
    width = block.shape[1]
    m = nc.embed(block, col_begin, right)
    d = ctx.from_numpy(m)
    row0, col0, exclude = nc.diagonal_offsets(diag, col_begin, width, col_global0)
    idx, val = lists(ctx, m.shape[0], k, poison=True)
    got, saw = merge(ctx, d, k, True, col_begin, col_begin + width, row0, col0, exclude, idx, val)
    want = nc.merge_block(m, k, col_begin, col_begin + width, row0, col0, exclude)
    assert same(got, want), (tag, width, k, col_begin, right, diag)
    assert saw == nc.saw_nan(m, col_begin, col_begin + width, row0, col0, exclude), (tag, width, k, col_begin, right, diag)
    for mat in (d, idx, val):
        mat.free()


def test_limits_are_the_mirrored_constants():
    from seekr_amd import _lib
    assert _lib.topk_merge_limits() == (_lib.TOPK_MERGE_KMAX, _lib.TOPK_MERGE_CAP)


@pytest.mark.parametrize("pattern", nc.PATTERNS)
def test_kernel_grid(pattern):
    """Every width and k of the case list; a poisoned running list under first = 1 in every call."""
    ctx = _ctx()
    for case in nc.kernel_cases():
        if case["pattern"] != pattern:
            continue
        block = nc.fill(pattern, nc.ROWS, case["width"], 11)
        check_block(ctx, block, case["k"], tag=pattern)


@pytest.mark.parametrize("pattern", ["five_values", "specials", "ascending"])
def test_alignment(pattern):
    """col_begin 0, 1, 4 and rows that start off a 16-byte line: the scalar head and tail."""
    ctx = _ctx()
    for width in nc.ALIGN_WIDTHS:
        block = nc.fill(pattern, 5, width, 12)
        for col_begin, right in nc.ALIGNMENTS:
            for k in (2, 33):
                check_block(ctx, block, k, col_begin=col_begin, right=right, tag=pattern)


@pytest.mark.parametrize("diag", nc.DIAGONALS)
def test_diagonal(diag):
    ctx = _ctx()
    for width in (1, 5, 64, 257, nc.STEP + 1):
        for pattern in ("five_values", "equal", "specials"):
            block = nc.fill(pattern, nc.ROWS, width, 13)
            for k in (1, 3, 64):
                check_block(ctx, block, k, col_begin=4, right=9, diag=diag, tag=pattern)


def test_nan_only_on_the_excluded_diagonal():
    ctx = _ctx()
    for width in (6, 300):
        m = np.arange(4 * width, dtype=np.float32).reshape(4, width)
        for i in range(4):
            m[i, i + 2] = np.nan
        d = ctx.from_numpy(m)
        for exclude, want_saw in ((True, False), (False, True)):
            idx, val = lists(ctx, 4, 3)
            got, saw = merge(ctx, d, 3, True, 0, width, 2, 0, exclude, idx, val)
            assert same(got, nc.merge_block(m, 3, 0, width, 2, 0, exclude)) and saw == want_saw
        # one row further the NaN cells are ordinary cells
        idx, val = lists(ctx, 4, 3)
        assert merge(ctx, d, 3, True, 0, width, 3, 0, True, idx, val)[1]


def test_highest_global_columns():
    from seekr_amd import _lib
    ctx = _ctx()
    for width in (5, 257):
        block = nc.fill("five_values", nc.ROWS, width, 14)
        d = ctx.from_numpy(block)
        col0 = nc.TOP_COLUMN - width + 1
        for row0 in (col0 + 2, 3):
            idx, val = lists(ctx, nc.ROWS, 4)
            got, _ = merge(ctx, d, 4, True, 0, width, row0, col0, True, idx, val)
            want = nc.merge_block(block, 4, 0, width, row0, col0, True)
            assert same(got, want) and int(want[0].max()) <= nc.TOP_COLUMN
        with pytest.raises(ValueError):
            _lib.topk_merge_rows(ctx, d, idx, val, 4, first=True, col_global0=col0 + 1)
    for k in (0, nc.KMAX + 1):
        with pytest.raises(ValueError):
            _lib.topk_merge_rows(ctx, d, idx, val, k, first=True)


@pytest.mark.parametrize("pattern", ["five_values", "specials", "ascending", "descending", "equal"])
def test_merge_over_panels(pattern):
    """2, 3 and 7 panels at uneven split points == the unsplit call == the reference."""
    ctx = _ctx()
    for width in (7, 257, 2 * nc.CAP + 1):
        block = nc.fill(pattern, 3, width, 15)
        d = ctx.from_numpy(block)
        for k in (1, 33, nc.KMAX):
            row0, col0 = 1000 + width // 3, 1000
            want = nc.merge_block(block, k, 0, width, row0, col0, True)
            idx, val = lists(ctx, 3, k, poison=True)
            whole, saw_whole = merge(ctx, d, k, True, 0, width, row0, col0, True, idx, val)
            assert same(whole, want), (pattern, width, k)
            for parts in nc.MERGE_SPLITS:
                cuts = [0] + nc.split_points(width, parts, 16) + [width]
                idx, val = lists(ctx, 3, k, poison=True)
                saw_any = False
                for p in range(len(cuts) - 1):
                    got, saw = merge(ctx, d, k, p == 0, cuts[p], cuts[p + 1], row0, col0, True, idx, val)
                    saw_any = saw_any or saw
                    assert saw == nc.saw_nan(block, cuts[p], cuts[p + 1], row0, col0)
                    # every intermediate list is the reference of the columns seen so far
                    assert same(got, nc.merge_block(block, k, 0, cuts[p + 1], row0, col0, True)), (pattern, width, k, parts, p)
                assert same(got, want) and saw_any == saw_whole, (pattern, width, k, parts)
        d.free()


def test_running_list_in_any_order_and_with_holes():
    """The list on entry is read as a set of entries: padded slots anywhere are no entries."""
    ctx = _ctx()
    block = nc.fill("five_values", 3, 90, 17)
    d = ctx.from_numpy(block)
    k = 6
    run_idx = np.array([[200, nc.NO_CELL, 150, 151, nc.NO_CELL, 300]] * 3, np.uint32)
    run_val = np.array([[0.25, np.nan, 9.0, 9.0, 5.0, -np.inf]] * 3, np.float32)
    idx, val = ctx.from_numpy(run_idx), ctx.from_numpy(run_val)
    got, saw = merge(ctx, d, k, False, 10, 80, 0, 0, False, idx, val)
    assert same(got, nc.merge_block(block, k, 10, 80, 0, 0, False, running=(run_idx, run_val))) and not saw


def test_more_rows_than_workgroups():
    ctx = _ctx()
    rng = np.random.default_rng(18)
    block = np.array([-1.5, 0.0, 0.25, 3.0, 7.0], np.float32)[rng.integers(0, 5, (5000, 70))]
    d = ctx.from_numpy(block)
    idx, val = lists(ctx, 5000, 3, poison=True)
    got, _ = merge(ctx, d, 3, True, 0, 70, 20, 0, True, idx, val)
    assert same(got, nc.merge_block(block, 3, 0, 70, 20, 0, True))


def test_old_kernel_and_new_agree_where_their_orders_coincide():
    """skr_topk_rows breaks ties by the local column: the same order when col_begin = 0 or all values are distinct."""
    from seekr_amd import consumers
    ctx = _ctx()
    rng = np.random.default_rng(19)
    for width in (5, 257, nc.CAP + 1):
        tied = nc.fill("five_values", 3, width, 19)
        distinct = rng.permutation(3 * width).astype(np.float32).reshape(3, width)
        for block, c0 in ((tied, 0), (distinct, 0), (distinct, 3 if width > 3 else 0)):
            d = ctx.from_numpy(block)
            for k in (1, 33):
                old = consumers.topk_rows(d, k, col_begin=c0, row_global0=9, col_global0=7)
                idx, val = lists(ctx, 3, k)
                new, _ = merge(ctx, d, k, True, c0, width, 9, 7, True, idx, val)
                assert same(new, old), (width, c0, k)
            d.free()


# ---- pearson_topk -----------------------------------------------------------------------------------------------------------
def prepared(ctx, x):
    from seekr_amd import _lib
    from seekr_amd import pearson as pearson_mod
    return _lib.operand_fill(ctx, ctx.from_numpy(x), None, pearson_mod._precision_for(np.dtype(np.float32), True))[0]


@functools.lru_cache(maxsize=None)
def profile_case(k):
    """Profiles with exact copies of row 0 (ties across panels), their operand and the whole r — once, left unchanged."""
    from seekr_amd import _lib
    ctx = _ctx()
    x = nc.kmer_profiles(300, k, 20 + k)
    x[[10, 150, 299]] = x[0]
    z = prepared(ctx, x)
    r_full = ctx.empty(300, 300)
    _lib.pearson_gemm_op(ctx, z, z, r_full)
    r = r_full.to_numpy().copy()
    r_full.free()
    return x, z, r


def assembled_r(ctx, a, b, stripe_rows, panel_rows):
    """r put together from the very contractions pearson_topk makes: the same operand views into a buffer of the same
    shape.  The split contraction chooses its tiles from the block's shape, and a [stripe, panel] block need not carry the
    bits of the same cells in a whole-matrix call (test_blocks_against_the_whole_matrix_call counts the cells)."""
    from seekr_amd import _lib
    n, m = a.rows, b.rows
    stripe_rows = max(1, min(int(stripe_rows), n))
    panel_rows = m if panel_rows is None else max(1, min(int(panel_rows), m))
    buf = ctx.empty(stripe_rows, panel_rows)
    r = np.empty((n, m), np.float32)
    for s0 in range(0, n, stripe_rows):
        rows = min(stripe_rows, n - s0)
        for p0 in range(0, m, panel_rows):
            cols = min(panel_rows, m - p0)
            _lib.pearson_gemm_op(ctx, a if rows == n else a.view(s0, rows), b if cols == m else b.view(p0, cols), buf)
            r[s0:s0 + rows, p0:p0 + cols] = buf.to_numpy()[:rows, :cols]
    buf.free()
    return r


def test_blocks_against_the_whole_matrix_call():
    """A [stripe, panel] block against the same cells of the whole-matrix call: the same values within the bar of
    tests/test_gpu_parity.py; the number of cells whose bits differ is printed (300 rows of 64 columns, stripes of 128,
    panels of 96: measured on an MI355X, see the pull request that added this file)."""
    ctx = _ctx()
    _, z, r = profile_case(3)
    blocks = assembled_r(ctx, z, z, 128, 96)
    differ = int((nc.bits(blocks) != nc.bits(r)).sum())
    print("cells of 300 x 300 whose bits differ between [128, 96] blocks and the whole-matrix call: %d, largest |difference| %.3g"
          % (differ, float(np.abs(blocks - r).max())))
    assert (np.abs(blocks.astype(np.float64) - r) <= 2e-6 + 1e-5 * np.abs(r)).all()
    assert np.array_equal(nc.bits(assembled_r(ctx, z, z, 300, None)), nc.bits(r))  # the same call gives the same bits


@pytest.mark.parametrize("stripe_rows", [128, 300])
@pytest.mark.parametrize("panel_rows", [96, 300, None])
def test_pearson_topk(stripe_rows, panel_rows):
    from seekr_amd import consumers
    ctx = _ctx()
    _, z, _ = profile_case(3)
    r = assembled_r(ctx, z, z, stripe_rows, panel_rows)
    for k in (1, 10, 64):
        got = consumers.pearson_topk(z, k=k, stripe_rows=stripe_rows, panel_rows=panel_rows)
        want = nc.merge_block(r, k)
        assert same(got, want), (stripe_rows, panel_rows, k)
        if k == 10:  # the copies of row 0 find each other
            assert set(got[0][0][:3]) == {10, 150, 299} and set(got[0][150][:3]) == {0, 10, 299}


def test_pearson_topk_256_columns():
    from seekr_amd import consumers
    ctx = _ctx()
    _, z, _ = profile_case(4)
    assert same(consumers.pearson_topk(z, k=4, stripe_rows=77, panel_rows=101), nc.merge_block(assembled_r(ctx, z, z, 77, 101), 4))


def test_pearson_topk_two_operands():
    from seekr_amd import consumers
    ctx = _ctx()
    x, z, _ = profile_case(3)
    a = prepared(ctx, np.ascontiguousarray(x[100:137] + np.float32(0.25) * x[5:42]))
    for panel_rows in (None, 96):
        got = consumers.pearson_topk(a, z, k=10, stripe_rows=20, panel_rows=panel_rows)
        assert same(got, nc.merge_block(assembled_r(ctx, a, z, 20, panel_rows), 10, exclude_diag=False)), panel_rows


def float32_layout_input(golden_dir):
    """Rows whose fill routes the operand to the float32 layout: two-level rows of the round-4 fixture, one of them with a
    single column on its upper level (one column carries the row's energy)."""
    x = np.ascontiguousarray(np.load(os.path.join(golden_dir, "regress_r4_two_level_rows.npz"))["a"][:12]).copy()
    rng = np.random.default_rng(21)
    x = np.concatenate([x, rng.standard_normal((8, x.shape[1])).astype(np.float32)])
    lo, hi = float(x[0].min()), float(x[0].max())
    x[3] = lo
    x[3, 1234] = hi
    x[7] = x[2]
    return x


def test_pearson_topk_float32_layout(golden_dir):
    from seekr_amd import _lib, consumers
    ctx = _ctx()
    x = float32_layout_input(golden_dir)
    z = prepared(ctx, x)
    assert z.kind == 0  # the route under test
    for panel_rows in (None, 7):
        r = assembled_r(ctx, z, z, 8, panel_rows)
        assert same(consumers.pearson_topk(z, k=5, stripe_rows=8, panel_rows=panel_rows), nc.merge_block(r, 5))


# ---- nearest ----------------------------------------------------------------------------------------------------------------
def test_nearest_is_pearson_topk_of_the_same_input(golden_dir):
    from seekr_amd import consumers
    from seekr_amd.neighbors import nearest
    ctx = _ctx()
    x, z, r = profile_case(3)
    assert same(nearest(x, k=7), consumers.pearson_topk(z, k=7))
    assert same(nearest(x, x, k=7, stripe_rows=64, panel_rows=50), nc.merge_block(assembled_r(ctx, z, z, 64, 50), 7))
    assert same(nearest(x.astype(np.float64), k=3), nc.merge_block(r, 3))  # ranked in float32
    a = np.ascontiguousarray(x[100:137] + np.float32(0.25) * x[5:42])
    assert same(nearest(a, x, k=10), consumers.pearson_topk(prepared(ctx, a), z, k=10))
    # one side routed to the float32 layout takes the other with it
    wide = float32_layout_input(golden_dir)
    other = np.random.default_rng(22).standard_normal((9, wide.shape[1])).astype(np.float32)
    zw, zo = prepared(ctx, wide), ctx.from_numpy(other)
    from seekr_amd import _lib
    zo = _lib.operand_fill(ctx, zo, None, _lib.PREC_FP32)[0]
    assert zw.kind == 0 and zo.kind == 0
    assert same(nearest(other, wide, k=4), consumers.pearson_topk(zo, zw, k=4))


# ---- domain_topk ------------------------------------------------------------------------------------------------------------
DT_K, DT_WINDOW, DT_SLIDE = 4, 200, 25


@functools.lru_cache(maxsize=None)
def dt_case():
    rng = np.random.default_rng(23)
    targets = [wc.random_seq(rng, 5130), wc.random_seq(rng, 2417)]  # 199 + 90 windows
    queries = [wc.random_seq(rng, L) for L in (300, 450, 800)]
    queries.append(targets[0][1000:1200])  # a window itself
    mean = rng.standard_normal(4 ** DT_K).astype(np.float32) * 0.1 + 1.0
    std = rng.uniform(0.5, 1.5, 4 ** DT_K).astype(np.float32)
    return targets, queries, mean, std


def write_fasta(path, names, seqs):
    path.write_text("".join(">%s\n%s\n" % (n, s) for n, s in zip(names, seqs)))
    return str(path)


def expected_frame(r, table, top):
    idx, val = nc.merge_block(r, top, exclude_diag=False)
    rows = []
    for q in range(r.shape[0]):
        for t in range(top):
            if idx[q, t] != nc.NO_CELL:
                w = int(idx[q, t])
                rows.append((q, t, table["header"][w], int(table["start"][w]), int(table["end"][w]), val[q, t]))
    return rows


def assert_frame(frame, want):
    assert list(frame.columns) == ["query", "rank", "header", "start", "end", "r"] and len(frame) == len(want)
    got = list(zip(frame["query"], frame["rank"], frame["header"], frame["start"], frame["end"]))
    assert got == [w[:5] for w in want]
    assert np.array_equal(nc.bits(frame["r"].to_numpy()), nc.bits(np.array([w[5] for w in want], np.float32)))


@pytest.mark.parametrize("chunk_rows", [7, 64, 65536])
def test_domain_topk(tmp_path, capsys, chunk_rows):
    from seekr_amd.windows import domain_pearson, domain_topk
    targets, queries, mean, std = dt_case()
    qfa = write_fasta(tmp_path / "q.fa", ["q%d" % i for i in range(len(queries))], queries)
    tfa = write_fasta(tmp_path / "t.fa", ["chrT", "chrU"], targets)
    r, table = domain_pearson(qfa, tfa, DT_K, DT_WINDOW, DT_SLIDE, mean, std, chunk_rows=chunk_rows)
    n = r.shape[1]
    assert 200 < n < 400 and np.isfinite(r).all()
    for top in (1, 5, nc.KMAX):
        frame = domain_topk(qfa, tfa, DT_K, DT_WINDOW, DT_SLIDE, mean, std, top=top, chunk_rows=chunk_rows)
        assert_frame(frame, expected_frame(r, table, top))
    # more than there are windows: the padded slots are dropped
    few = write_fasta(tmp_path / "few.fa", ["chrS"], [targets[0][:300]])
    r2, table2 = domain_pearson(qfa, few, DT_K, DT_WINDOW, DT_SLIDE, mean, std, chunk_rows=chunk_rows)
    frame = domain_topk(qfa, few, DT_K, DT_WINDOW, DT_SLIDE, mean, std, top=9, chunk_rows=chunk_rows)
    assert r2.shape[1] == 5 and len(frame) == 5 * len(queries)
    assert_frame(frame, expected_frame(r2, table2, 9))
    from seekr_amd.kmer_counts import NAN_WARNING
    assert NAN_WARNING not in capsys.readouterr().out


def test_domain_topk_window_shorter_than_k(tmp_path, capsys):
    """A sequence of fewer than k - 1 letters is one window without a k-mer: a constant row under mean 0 / std 1, no r."""
    from seekr_amd.kmer_counts import NAN_WARNING
    from seekr_amd.windows import domain_pearson, domain_topk
    targets, queries, _, _ = dt_case()
    mean, std = np.zeros(4 ** DT_K, np.float32), np.ones(4 ** DT_K, np.float32)
    qfa = write_fasta(tmp_path / "q.fa", ["q0", "q1"], queries[:2])
    tfa = write_fasta(tmp_path / "t.fa", ["a", "short", "b"], [targets[0][:300], "AC", targets[1][:250]])
    for chunk_rows in (3, 65536):
        capsys.readouterr()
        r, table = domain_pearson(qfa, tfa, DT_K, DT_WINDOW, DT_SLIDE, mean, std, log2="Log2.none", chunk_rows=chunk_rows)
        assert capsys.readouterr().out.count(NAN_WARNING) == 1
        assert r.shape[1] == 9 and np.isnan(r[:, 5]).all() and np.isfinite(np.delete(r, 5, axis=1)).all()
        frame = domain_topk(qfa, tfa, DT_K, DT_WINDOW, DT_SLIDE, mean, std, top=9, log2="Log2.none", chunk_rows=chunk_rows)
        assert capsys.readouterr().out.count(NAN_WARNING) == 1
        assert_frame(frame, expected_frame(r, table, 9))
        last = frame[frame["rank"] == 8]
        assert np.isnan(last["r"].to_numpy()).all() and set(last["header"]) == {">short"}
        # with top within the finite windows the NaN window is not ranked, and the warning is still printed once
        frame = domain_topk(qfa, tfa, DT_K, DT_WINDOW, DT_SLIDE, mean, std, top=8, log2="Log2.none", chunk_rows=chunk_rows)
        assert capsys.readouterr().out.count(NAN_WARNING) == 1 and np.isfinite(frame["r"].to_numpy()).all()


# ---- the command ------------------------------------------------------------------------------------------------------------
def test_command(tmp_path):
    import pandas as pd
    from seekr_amd import _lib
    from seekr_amd.neighbors import nearest
    x = nc.kmer_profiles(20, 3, 24).astype(np.float64)
    names = ["tx%d, v1" % i if i == 4 else "tx%d" % i for i in range(20)]
    kmers = ["c%d" % j for j in range(64)]
    csv = tmp_path / "counts.csv"
    pd.DataFrame(x, index=names, columns=kmers).to_csv(csv)
    out = tmp_path / "nearest.csv"
    argv = ["seekr_nearest", str(csv), "-n", "25", "-o", str(out)]
    code = "import sys; sys.argv = %r; from seekr_amd.console_scripts import console_nearest; console_nearest()" % (argv,)
    proc = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0, proc.stderr
    values = pd.read_csv(csv, index_col=0).to_numpy()
    idx, val = nearest(values, k=25)
    frame = pd.read_csv(out)
    assert list(frame.columns) == ["row", "rank", "neighbor", "r"] and len(frame) == 20 * 19  # 19 candidates a row
    keep = idx != _lib.TOPK_PAD_IDX
    assert keep.sum() == 20 * 19
    qi, rank = np.nonzero(keep)
    assert list(frame["row"]) == [names[i] for i in qi] and list(frame["rank"]) == list(rank)
    assert list(frame["neighbor"]) == [names[j] for j in idx[keep]]
    assert np.array_equal(nc.bits(frame["r"].to_numpy().astype(np.float32)), nc.bits(val[keep]))
    # .npy input, two files: indices instead of labels
    np.save(tmp_path / "a.npy", values[:6].astype(np.float32))
    np.save(tmp_path / "b.npy", values.astype(np.float32))
    out2 = tmp_path / "n2.csv"
    argv = ["seekr_nearest", str(tmp_path / "a.npy"), str(tmp_path / "b.npy"), "-n", "3", "-o", str(out2), "-bi"]
    code = "import sys; sys.argv = %r; from seekr_amd.console_scripts import console_nearest; console_nearest()" % (argv,)
    proc = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0, proc.stderr
    idx2, val2 = nearest(values[:6].astype(np.float32), values.astype(np.float32), k=3)
    frame = pd.read_csv(out2)
    assert list(frame["row"]) == [i for i in range(6) for _ in range(3)] and list(frame["neighbor"]) == list(idx2.reshape(-1))
    assert np.array_equal(nc.bits(frame["r"].to_numpy().astype(np.float32)), nc.bits(val2.reshape(-1)))
