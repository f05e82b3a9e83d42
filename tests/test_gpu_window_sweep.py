"""The sweep of count_windows_kernel and domain_pearson on the MI355X: the inputs the kernel was written for (windows of whole
sweeps, homopolymers and short-period repeats, bins that end at 65 535), one N at every phase, runs of rows over a ragged
table, and FASTA targets whose windows send domain_pearson's chunks down different operand layouts.

Cases and expectations: tests/window_sweep_cases.py (pinned without a GPU by tests/test_window_sweep_cpu.py).  Rows are
compared as tests/test_gpu_windows.py compares them (check_all_forms: uint32 and float32 rows bit for bit against the oracle
on explicit substrings and against the device's own BasicCounter, Log2.pre rows bit for bit against the device path and
within its bar against the oracle); r is judged by tests/parity_rule.py against the oracle, as assert_parity does.
Needs a real MI355X: run with `-m gpu`."""
import numpy as np
import pytest

import parity_rule
from oracle import seekr_oracle as orc
import window_sweep_cases as sc
import windows_cases as wc
from test_gpu_windows import _ctx, assert_parity, bits, check_all_forms, new_rows, write_fasta

pytestmark = pytest.mark.gpu

FORMS = ((np.uint32, False), (np.float32, False), (np.float32, True))  # uint32, per-kb float32, Log2.pre


# ---------------------------------------------------------------------------------------------------------------------
# counting
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,wi", [(k, wi) for k in sc.SWEEP_KS for wi in range(6)])
def test_full_sweeps_on_random_text(k, wi):
    """S - 1 bases: the slow branch alone; S, S + 1: one fast sweep; 2S - 1, 2S, 2S + 17: two and a partial one — with window
    starts at every base offset inside a packed word."""
    window = sc.sweep_windows(k)[wi]
    offsets_seen = set()
    for slide in sc.SWEEP_SLIDES:
        seqs, _, _, _ = sc.sweep_case(k, window, slide)
        assert check_all_forms(seqs, k, window, slide) == -(-40 // slide) + 1
        offsets_seen |= set((wc.substrings(seqs, window, slide)[1][:, 1] % 16).tolist())
    assert offsets_seen == set(range(16))


@pytest.mark.parametrize("k,slide", [(k, slide) for k in sc.SWEEP_KS for slide in sc.REPEAT_SLIDES])
def test_repeats_and_their_controls(k, slide):
    """Homopolymers of every letter, periods 2, 4, 8 and 16 in the lower half, the upper half and both halves of the bin
    words (the aggregated arm), periods 3 and 5 (the plain arm), a row that takes both arms and the partial sweep, and a
    repeat with one N (the masked branch)."""
    names, (seqs, _, window, _) = sc.repeat_case(k, slide)
    check_all_forms(seqs, k, window, slide)
    got = new_rows(seqs, k, window, slide, np.uint32)
    table = wc.substrings(seqs, window, slide)[1]
    for letter in "AGTC":
        rows = np.nonzero(table[:, 0] == names.index(letter))[0]
        assert len(rows) >= 2
        for r in rows:
            W = table[r, 2] - k + 1
            want = np.zeros(4 ** k, dtype=np.uint32)
            want[sc.homopolymer_column(letter, k)] = W
            assert np.array_equal(got[r], want), (letter, k, int(table[r, 1]))


@pytest.mark.parametrize("k,n_kmers,letter", sc.EDGE_CASES)
def test_bins_that_end_at_65535_and_65536(k, n_kmers, letter):
    """65 535 k-mers of one homopolymer fill a 16-bit half to its last value (T: the upper half, A: the lower); 65 536 is the
    first window counted into 32-bit bins."""
    seqs, _, window, slide = sc.edge_case(k, n_kmers, letter)
    assert check_all_forms(seqs, k, window, slide) == 3
    subs, _ = wc.substrings(seqs, window, slide)
    got, want = new_rows(seqs, k, window, slide, np.uint32), wc.expected_u32(subs, k)
    col, half = sc.homopolymer_column(letter, k), 4 ** k // 2
    other = col - half if col >= half else col + half  # the bin in the same word
    assert got[0, col] == n_kmers and got[0].sum() == n_kmers
    assert np.array_equal(got[:, other], want[:, other]) and got[0, other] == 0
    assert np.array_equal(got[:, col], want[:, col]) and got[1, col] < 65535 <= got[0, col]


@pytest.mark.parametrize("k", sc.N_KS)
def test_one_n_at_every_phase(k):
    for seqs, _, window, slide in (sc.n_phase_case(k), sc.n_sweep_case(k)):
        n_rows = check_all_forms(seqs, k, window, slide)
        got = new_rows(seqs, k, window, slide, np.uint32)
        table = wc.substrings(seqs, window, slide)[1]
        assert n_rows == len(table) and (window > 44 or n_rows == 77)
        sums = [sc.kmers_in_row(seqs[i], s, L, k) for i, s, L in table]  # W minus the k-mers that cover the N
        assert got.sum(axis=1).tolist() == sums, (k, window)


def count_in_runs(ctx, packed, case, runs, dtype, log2_pre):
    """The rows of (first_row, n_rows) runs counted into views of one matrix."""
    from seekr_amd import _lib
    _, k, window, slide = case
    dev = ctx.zeros(sum(n for _, n in runs), 4 ** k, dtype)
    for r0, n in runs:
        _lib.count_windows(ctx, packed, k, window, slide, r0, n, log2_pre=log2_pre, out=dev.view(r0, n))
    return dev.to_numpy()


def test_runs_over_a_table_of_many_sequences():
    """Runs of 1, 2, 5 and 37 rows, and runs that begin and end exactly on a sequence's first row, give the bits of the whole
    call; with a sequence of k - 1 letters in the table exactly the runs that hold its row raise ZeroDivisionError."""
    from seekr_amd import _lib
    case = seqs, k, window, slide = sc.table_case()
    check_all_forms(seqs, k, window, slide)
    ctx = _ctx()
    packed = ctx.pack(seqs)
    rb = sc.row_begin(seqs, window, slide)
    total = int(rb[-1])
    for dtype, pre in FORMS:
        whole = bits(_lib.count_windows(ctx, packed, k, window, slide, 0, total, dtype=dtype, log2_pre=pre).to_numpy())
        for run in sc.TABLE_RUNS:
            runs = [(r0, min(run, total - r0)) for r0 in range(0, total, run)]
            assert np.array_equal(bits(count_in_runs(ctx, packed, case, runs, dtype, pre)), whole), (dtype, pre, run)
        for r0, n in sc.boundary_runs(rb):
            got = _lib.count_windows(ctx, packed, k, window, slide, r0, n, dtype=dtype, log2_pre=pre).to_numpy()
            assert np.array_equal(bits(got), whole[r0:r0 + n]), (dtype, pre, r0, n)
    # one sequence of k - 1 letters: its row raises in the per-kb and the Log2.pre form, and only there
    (seqs, _, _, _), bad = sc.table_case_with_zero_division()
    packed = ctx.pack(seqs)
    subs, _ = wc.substrings(seqs, window, slide)
    rb = sc.row_begin(seqs, window, slide)
    total = int(rb[-1])
    assert len(subs[bad]) == k - 1 and bad in rb
    want_u32 = wc.expected_u32(subs, k)
    assert np.array_equal(_lib.count_windows(ctx, packed, k, window, slide, 0, total, dtype=np.uint32).to_numpy(), want_u32)
    good = [r for r in range(total) if r != bad]
    all_runs = [(r0, min(run, total - r0)) for run in sc.TABLE_RUNS for r0 in range(0, total, run)] + sc.boundary_runs(rb)
    n_raised = 0
    for pre in (False, True):
        want = np.zeros((total, 4 ** k), dtype=np.float32)
        want[good] = wc.expected_per_kb([subs[r] for r in good], k, log2_pre=pre)
        if pre:  # bit-equal to the device's own rows (two runs around the failing row), which are within the bar of the oracle's
            dev = np.zeros_like(want)
            dev[:bad] = _lib.count_windows(ctx, packed, k, window, slide, 0, bad, log2_pre=True).to_numpy()
            dev[bad + 1:] = _lib.count_windows(ctx, packed, k, window, slide, bad + 1, total - bad - 1, log2_pre=True).to_numpy()
            assert np.allclose(dev, want, rtol=wc.RTOL, atol=wc.ATOL_LOG)
            want = dev
        want = bits(want)
        for r0, n in all_runs:
            if r0 <= bad < r0 + n:
                with pytest.raises(ZeroDivisionError):
                    _lib.count_windows(ctx, packed, k, window, slide, r0, n, log2_pre=pre)
                n_raised += 1
            else:
                got = bits(_lib.count_windows(ctx, packed, k, window, slide, r0, n, log2_pre=pre).to_numpy())
                assert np.array_equal(got, want[r0:r0 + n]), (pre, r0, n)
            got = _lib.count_windows(ctx, packed, k, window, slide, r0, n, dtype=np.uint32).to_numpy()  # never raises
            assert np.array_equal(got, want_u32[r0:r0 + n]), (r0, n)
    assert n_raised >= 2 * (len(sc.TABLE_RUNS) + 3)


# ---------------------------------------------------------------------------------------------------------------------
# domain_pearson on structured targets
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def routes(monkeypatch):
    """What the chunk loop of domain_pearson did: every operand fill (precision asked for, rows, resulting kind and coherent
    flag) and every contraction (the kinds of its two operands, the rows of the target's)."""
    from seekr_amd import _lib
    log = []
    fill, gemm = _lib.operand_fill, _lib.pearson_gemm_op

    def logged_fill(ctx, x, op=None, precision=_lib.PREC_F16X3, **kwargs):
        res = fill(ctx, x, op, precision, **kwargs)
        log.append(("fill", int(precision), x.rows, res[0].kind, res[0].coherent))
        return res

    def logged_gemm(ctx, a, b, r, *args, **kwargs):
        log.append(("gemm", a.kind, b.kind, b.rows, a.coherent or b.coherent))
        return gemm(ctx, a, b, r, *args, **kwargs)

    monkeypatch.setattr(_lib, "operand_fill", logged_fill)
    monkeypatch.setattr(_lib, "pearson_gemm_op", logged_gemm)
    return log


def fasta_of(tmp_path, case):
    qfa = write_fasta(tmp_path / "q.fa", ["q%d" % i for i in range(len(case["queries"]))], case["queries"])
    tfa = write_fasta(tmp_path / "t.fa", case["names"], case["records"])
    return qfa, tfa


def assert_routes(log, case, which, chunk_rows):
    from seekr_amd import _lib
    n = len(case["table"])
    chunks = sc.chunks_of(n, chunk_rows)
    gemms = [e for e in log if e[0] == "gemm"]
    assert [g[3] for g in gemms] == [c[1] for c in chunks], log
    float32 = [g[1] == 0 and g[2] == 0 for g in gemms]
    split = [g[1] == g[2] != 0 for g in gemms]
    assert all(f or s for f, s in zip(float32, split)), log  # never two operands of different kinds
    if which == "b":  # the query operand itself routed: the whole call in float32 layout
        assert all(float32), log
        assert log[0][:4] == ("fill", log[0][1], len(case["queries"]), 0) and log[0][1] != _lib.PREC_FP32, log
        return
    predicted = sc.predicted_routes(case["share"], chunk_rows)
    for i, want in enumerate(predicted):
        if want == "fp32":
            assert float32[i], (i, chunks[i], log)
        elif want == "split":
            assert split[i], (i, chunks[i], log)
    if chunk_rows < n:
        assert predicted.count("fp32") >= 2 and predicted.count("split") >= 2
        assert any(float32) and any(split)  # both layouts in one call
        # the cached parent operand after a full-size chunk routed it: a later chunk of ordinary rows is split again
        first = min(i for i, c in enumerate(chunks) if predicted[i] == "fp32" and c[1] == chunk_rows)
        later = [i for i in range(first + 1, len(chunks)) if predicted[i] == "split"]
        assert later and all(split[i] for i in later), log
        # ... and is filled once, in the layout asked for
        at = [j for j, e in enumerate(log) if e[0] == "gemm"][later[0]]
        assert log[at - 1][0] == "fill" and log[at - 1][3] != 0 and log[at - 2][0] == "gemm", log[at - 3:at + 1]


@pytest.mark.parametrize("which", ["a", "b"])
@pytest.mark.parametrize("k,log2", sc.DP_MODES)
def test_domain_pearson_routes_chunks_of_a_structured_target(tmp_path, routes, k, log2, which):
    """A target with an A run, a GT run and an N run, a record shorter than the window and one of k - 2 letters.  Set (a),
    five random queries: the chunks that hold windows of the runs go to float32 layout on both sides, the others stay split,
    in one call.  Set (b), two repeat queries more: the query operand routes and with it the whole call.  r is within the
    project's bar of the oracle for every chunking, and the chunkings agree with each other under the same rule."""
    from seekr_amd.windows import domain_pearson
    case = sc.query_set(sc.domain_case(k, log2), which)
    qfa, tfa = fasta_of(tmp_path, case)
    n = len(case["table"])
    results = {}
    for chunk_rows in sc.DP_CHUNKS + (n + 7,):
        del routes[:]
        r, table = domain_pearson(qfa, tfa, k, sc.DP_WINDOW, sc.DP_SLIDE, case["mean"], case["std"], log2=log2, chunk_rows=chunk_rows)
        assert r.dtype == np.float32 and r.shape == (len(case["queries"]), n)
        assert_parity(r, case["ref"], case)
        assert_routes(routes, case, which, chunk_rows)
        assert list(table["header"]) == [">" + case["names"][i] for i in case["table"][:, 0]]
        assert np.array_equal(table["start"].to_numpy(), case["table"][:, 1])
        assert np.array_equal(table["end"].to_numpy(), case["table"][:, 1] + case["table"][:, 2])
        results[chunk_rows] = r
    assert_parity(results[50], results[16], case)
    assert_parity(results[n + 7], results[16], case)
    if which == "b":  # the repeat queries meet the target's own runs
        assert results[16][5:].max(axis=1).min() > 0.6


def nan_run(tmp_path, log2):
    from seekr_amd.windows import domain_pearson
    k = 6
    case = sc.query_set(sc.nan_case(k, log2), "a")
    qfa, tfa = fasta_of(tmp_path, case)
    r, _ = domain_pearson(qfa, tfa, k, sc.DP_WINDOW, sc.DP_SLIDE, case["mean"], case["std"], log2=log2, chunk_rows=16)
    return case, r


@pytest.mark.parametrize("log2", ["Log2.post", "Log2.pre", "Log2.none"])
def test_domain_pearson_nan_in_one_column(tmp_path, log2):
    """mean = 0 and std = 1: the window of the record of k - 2 letters is a constant row, the last row of the tail chunk.  r is
    NaN in that column and nowhere else, and the rest is within the bar."""
    case, r = nan_run(tmp_path, log2)
    n = len(case["table"])
    ok = ~np.isnan(case["ref"])
    assert np.count_nonzero(~ok) == 5 and not ok[:, n - 1].any()  # that one column and nothing more
    assert np.array_equal(np.isnan(r), ~ok)
    res = parity_rule.judge(r, case["ref"], case["truth"], ok, case["qn"], case["tn"])
    assert res["n_cells"] == 5 * (n - 1) and res["failures"] == [], res["failures"][:5]


@pytest.mark.parametrize("log2", ["Log2.post", "Log2.pre", "Log2.none"])
def test_domain_pearson_nan_in_one_column_prints_the_warning_once(tmp_path, capsys, log2):
    """The same call prints NAN_WARNING once: the counts of the constant row are finite (the fill's has_nan stays clear in
    every chunk), its column of r is not, and domain_pearson warns for either."""
    from seekr_amd.kmer_counts import NAN_WARNING
    capsys.readouterr()
    nan_run(tmp_path, log2)
    printed = capsys.readouterr().out.count(NAN_WARNING)
    print("NAN_WARNING printed", printed, "times")
    assert printed == 1


def test_domain_pearson_nan_counts_print_the_warning_once(tmp_path, capsys):
    """A std of 0 in one column: every window row holds NaN or inf there, every chunk reports has_nan, the warning is printed
    once for the call and r is NaN where the oracle's is — everywhere."""
    from seekr_amd.kmer_counts import NAN_WARNING
    from seekr_amd.windows import domain_pearson
    k, log2 = 6, "Log2.none"
    case = sc.query_set(sc.nan_case(k, log2), "a")
    _, tfa = fasta_of(tmp_path, case)
    std = case["std"].copy()
    std[0] = 0
    with np.errstate(all="ignore"):
        tn = orc.get_counts(case["subs"], k=k, mean=case["mean"], std=std, log2=log2)[0]
        ref = orc.pearson(case["qn"], tn)
    assert np.isnan(tn[:, 0]).any() and np.isnan(ref).all() and len(tn) > 7 * 16
    capsys.readouterr()
    r, _ = domain_pearson(case["qn"], tfa, k, sc.DP_WINDOW, sc.DP_SLIDE, case["mean"], std, log2=log2, chunk_rows=16)
    assert capsys.readouterr().out.count(NAN_WARNING) == 1
    assert np.array_equal(np.isnan(r), np.isnan(ref))


@pytest.mark.parametrize("log2", ["Log2.post", "Log2.pre", "Log2.none"])
def test_domain_pearson_zero_division_in_the_last_chunk(tmp_path, log2):
    from seekr_amd.windows import domain_pearson
    k = 6
    mean, std = sc.background(k, log2)
    records = sc.zero_division_records(k)
    assert (len(wc.substrings(records, sc.DP_WINDOW, sc.DP_SLIDE)[0]) - 1) // 16 >= 5  # the failing row is in a late chunk
    case = dict(queries=sc.domain_case(k, log2)["queries"][:5], names=["long", "short", "tiny"], records=records)
    qfa, tfa = fasta_of(tmp_path, case)
    with pytest.raises(ZeroDivisionError):
        domain_pearson(qfa, tfa, k, sc.DP_WINDOW, sc.DP_SLIDE, mean, std, log2=log2, chunk_rows=16)
