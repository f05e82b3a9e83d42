"""Sliding-window counting and domain_pearson on the MI355X (seekr_amd.windows, csrc/windows.hip).

Every row is checked against two references: the oracle on explicit substrings (tests/windows_cases.py) and the device's
own BasicCounter / skr_count_u32 with the same substrings assigned as `seqs`.  uint32 and float32 (Log2.none) rows are
bit-equal to both; Log2.pre rows are bit-equal to the device path and within the bar of test_gpu_parity.py against the
oracle.  Needs a real MI355X: run with `-m gpu`."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import parity_rule
import windows_cases as wc
from oracle import seekr_oracle as orc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ctx():
    from seekr_amd import _lib
    return _lib.default_context()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def new_rows(seqs, k, window, slide, dtype=np.float32, log2_pre=False, first_row=0, n_rows=None):
    from seekr_amd import _lib
    from seekr_amd.windows import window_table
    ctx = _ctx()
    packed = ctx.pack(seqs)
    if n_rows is None:
        n_rows = len(window_table([len(s) for s in seqs], window, slide)[0]) - first_row
    return _lib.count_windows(ctx, packed, k, window, slide, first_row, n_rows, dtype=dtype, log2_pre=log2_pre).to_numpy()


def device_u32(subs, k):
    from seekr_amd import _lib
    ctx = _ctx()
    return _lib.count_u32(ctx, ctx.pack(subs), k).to_numpy()


def device_counter(subs, k, log2="Log2.none", mean=False, std=False):
    from seekr_amd.kmer_counts import BasicCounter
    c = BasicCounter(k=k, mean=mean, std=std, log2=log2, silent=True)
    c.seqs = subs
    c.get_counts()
    return c


def check_all_forms(seqs, k, window, slide):
    """uint32, float32 and Log2.pre rows of the windows of `seqs` against both references."""
    from oracle import c_oracle
    subs, table = wc.substrings(seqs, window, slide)
    want_u32 = wc.expected_u32(subs, k)
    got = new_rows(seqs, k, window, slide, np.uint32)
    assert got.shape == (len(subs), 4 ** k)
    assert np.array_equal(got, want_u32), ("u32 vs oracle", k, window, slide)
    assert np.array_equal(got, device_u32(subs, k)), ("u32 vs device", k, window, slide)
    if wc.has_zero_division(subs, k):
        with pytest.raises(ZeroDivisionError):
            new_rows(seqs, k, window, slide)
        with pytest.raises(ZeroDivisionError):
            device_counter(subs, k)
        return len(subs)
    want = c_oracle.per_kb_f32(want_u32, [len(s) for s in subs], k)  # = wc.expected_per_kb(subs, k), counted once
    got = new_rows(seqs, k, window, slide)
    assert np.array_equal(bits(got), bits(want)), ("f32 vs oracle", k, window, slide)
    assert np.array_equal(bits(got), bits(device_counter(subs, k).counts)), ("f32 vs device", k, window, slide)
    got = new_rows(seqs, k, window, slide, log2_pre=True)
    assert np.array_equal(bits(got), bits(device_counter(subs, k, "Log2.pre").counts)), ("Log2.pre vs device", k, window, slide)
    assert np.allclose(got, orc.log2_plus_one(want), rtol=wc.RTOL, atol=wc.ATOL_LOG), ("Log2.pre vs oracle", k, window, slide)
    return len(subs)


GRID_KS = (1, 3, 6, 7)


def grid_windows(k):
    return (k, k + 1, 15, 16, 17, 33, 1000)


def grid_slides(window):
    return sorted({s for s in (1, 7, 16, window - 1, window) if 1 <= s <= window})


def grid_lengths(k, window, slide):
    return (k, window - 1, window, window + 1, window + slide, 5 * window + 3)


@pytest.mark.parametrize("k,wi", [(k, wi) for k in GRID_KS for wi in range(7)])
def test_grid_of_window_sizes_and_offsets(k, wi):
    """Window starts at every base offset inside a packed word (slides 1 and 7), windows that end on and next to word and
    sequence ends.  The six lengths of the grid are six sequences of one call; the ones whose windows include one of
    k - 1 letters (ZeroDivisionError for the whole call, as for BasicCounter) are a call of their own."""
    window = grid_windows(k)[wi]
    rng = np.random.default_rng(1000 * k + window)
    offsets_seen = set()
    for slide in grid_slides(window):
        seqs = [wc.random_seq(rng, L) for L in grid_lengths(k, window, slide)]
        if window <= 33:  # the longest once more with letters outside the alphabet
            seqs.append(wc.random_seq(rng, 5 * window + 3, "ACGTACGTACGTN"))
        bad = [s for s in seqs if wc.has_zero_division(wc.substrings([s], window, slide)[0], k)]
        good = [s for s in seqs if s not in bad]
        assert len(good) >= 3
        check_all_forms(good, k, window, slide)
        if bad:
            check_all_forms(bad, k, window, slide)
        offsets_seen |= set((wc.substrings(seqs, window, slide)[1][:, 1] % 16).tolist())
    if 4 * window + 3 >= 15:  # the longest sequence has a start at every offset inside a packed word
        assert offsets_seen == set(range(16))


def test_many_ragged_sequences_in_one_call():
    k, window, slide = 4, 64, 9
    rng = np.random.default_rng(7)
    seqs = []
    while len(seqs) < 300:
        s = wc.random_seq(rng, int(rng.integers(1, 400)), "ACGT" if len(seqs) % 5 else "ACGTACGTN")
        if not wc.has_zero_division(wc.substrings([s], window, slide)[0], k):
            seqs.append(s)
    assert sum(len(s) < window for s in seqs) >= 20 and sum(len(s) < k for s in seqs) >= 1
    assert check_all_forms(seqs, k, window, slide) > 3000


def test_long_sequence_whole_and_in_runs():
    """200 kb, window 1 000, slide 100: 1 991 rows, whole and in runs of 1, 7 and 1 000 rows — the same rows however cut."""
    from seekr_amd import _lib
    k, window, slide = 6, 1000, 100
    seq = wc.random_seq(np.random.default_rng(11), 200_000)
    subs, _ = wc.substrings([seq], window, slide)
    assert len(subs) == 1991
    check_all_forms([seq], k, window, slide)
    ctx = _ctx()
    packed = ctx.pack([seq])
    want = bits(wc.expected_per_kb(subs, k))
    for run in (1, 7, 1000):
        dev = ctx.zeros(1991, 4 ** k)
        for r0 in range(0, 1991, run):
            n = min(run, 1991 - r0)
            _lib.count_windows(ctx, packed, k, window, slide, r0, n, out=dev.view(r0, n))
        assert np.array_equal(bits(dev.to_numpy()), want), run
    # a run from the middle into a matrix of its own, uint32
    got = _lib.count_windows(ctx, packed, k, window, slide, 1234, 7, dtype=np.uint32).to_numpy()
    assert np.array_equal(got, wc.expected_u32(subs[1234:1241], k))


def test_letters_outside_the_alphabet():
    k, window, slide = 3, 20, 5
    rng = np.random.default_rng(3)
    seq = list(wc.random_seq(rng, 140))
    seq[5] = "N"             # first base of the window at 5
    seq[10 + 19] = "N"       # last base of the window at 10
    seq[39:42] = "NNN"       # over the boundary between the windows ending at 40 and starting at 40
    seq[60:80] = "N" * 20    # the whole window at 60
    seq[100:104] = "acgt"    # lower case through `seqs`: skipped, as the reference skips it
    seq = "".join(seq)
    check_all_forms([seq, wc.random_seq(rng, 50), "N" * 30], k, window, slide)
    subs, _ = wc.substrings([seq], window, slide)
    got = new_rows([seq], k, window, slide, np.uint32)
    assert got[12].sum() == 0 and subs[12] == "N" * 20
    assert got[1].sum() == window - k + 1 - 1 and got[2].sum() == window - k + 1 - 1  # N is the first base; N is the last base


def test_value_where_product_and_running_sum_round_differently():
    """(n, W) = (35 604, 35 747) of tests/golden/count_value_pairs.json: float32(n * inc) is not the float32 of the
    reference's n additions.  A window of W + k - 1 letters with a run of A giving n times AAA; the next window is a control."""
    k, n, W = 3, 35604, 35747
    pairs = json.load(open(os.path.join(ROOT, "tests", "golden", "count_value_pairs.json")))["mismatch"]
    want_bits = [b for (pn, pw, b) in pairs if (pn, pw) == (n, W)]
    assert len(want_bits) == 1
    window, slide = W + k - 1, 20000
    filler = "C" + "GTC" * 20000
    seq = "A" * (n + k - 1) + filler[:window - (n + k - 1) + slide]
    assert len(seq) == window + slide
    subs, _ = wc.substrings([seq], window, slide)
    assert len(subs) == 2 and len(subs[0]) == window == len(subs[1])
    u = new_rows([seq], k, window, slide, np.uint32)
    assert u[0, 0] == n and u[0].sum() == W and u[1, 0] == n - slide
    got = new_rows([seq], k, window, slide)
    assert int(bits(got)[0, 0]) == want_bits[0]
    assert np.float32(n * (1000.0 / W)).view(np.uint32) != want_bits[0]  # the product alone would have missed it
    check_all_forms([seq], k, window, slide)


def test_window_of_more_than_65535_kmers():
    """32-bit bins: one bin alone passes 65 535."""
    k, window, slide = 2, 70_000, 25
    seq = "A" * 69_990 + wc.random_seq(np.random.default_rng(5), 60)
    check_all_forms([seq], k, window, slide)
    assert new_rows([seq], k, window, slide, np.uint32)[0, 0] > 65535


def test_refusals():
    from seekr_amd.windows import window_counts
    seqs = ["ACGTACGTACGT", "ACGTAC"]
    with pytest.raises(ZeroDivisionError):
        new_rows(["ACGTACG"], 4, 3, 1)  # every window has k - 1 letters
    with pytest.raises(ZeroDivisionError):
        window_counts(["ACGTACGTAC", "ACGTAC"], 4, 7, 7, mean=False, std=False)  # the tail ACG of the first sequence
    with pytest.raises(NotImplementedError):
        new_rows(seqs, 8, 10, 2)
    with pytest.raises(NotImplementedError):
        window_counts(seqs, 2, 5, 2, alphabet="ACGTN")
    with pytest.raises(NotImplementedError):
        new_rows(seqs, 2, 5, 2, dtype=np.float64)
    with pytest.raises(ValueError):
        new_rows(seqs, 2, 5, 6)
    with pytest.raises(ValueError):
        window_counts(["ACGT"], 2, 10, 1)  # one window, std=True: "You cannot standardize a single sequence"


@pytest.mark.parametrize("chunk_rows", [None, 10])
def test_window_counts_with_computed_statistics(tmp_path, chunk_rows):
    from seekr_amd.windows import window_counts
    k, window, slide = 3, 50, 10
    rng = np.random.default_rng(21)
    seqs = [wc.random_seq(rng, L) for L in (300, 47, 411)]
    subs, table = wc.substrings(seqs, window, slide)
    res = window_counts(seqs, k, window, slide, log2="Log2.none", chunk_rows=chunk_rows)
    ref = device_counter(subs, k, "Log2.none", mean=True, std=True)
    want, want_mean, want_std = orc.get_counts(subs, k=k, log2="Log2.none")
    for got, dev, oracle in ((res.mean, ref.mean, want_mean), (res.std, ref.std, want_std), (res.counts, ref.counts, want)):
        assert np.array_equal(bits(got), bits(dev)) and np.array_equal(bits(got), bits(oracle))
    assert np.array_equal(res.table[["seq_index", "start", "length"]].to_numpy(), table)
    post = window_counts(seqs, k, window, slide, chunk_rows=chunk_rows)
    assert np.array_equal(bits(post.counts), bits(device_counter(subs, k, "Log2.post", mean=True, std=True).counts))
    assert np.allclose(post.counts, orc.get_counts(subs, k=k)[0], rtol=wc.RTOL, atol=wc.ATOL_POST)
    # stored vectors, and a FASTA file: headers in the table, the reader's upper-casing
    fa = tmp_path / "t.fa"
    fa.write_text("".join(">s%d\n%s\n" % (i, s.lower() if i == 1 else s) for i, s in enumerate(seqs)))
    vec = window_counts(str(fa), k, window, slide, mean=want_mean, std=want_std, log2="Log2.none", chunk_rows=chunk_rows)
    assert np.array_equal(bits(vec.counts), bits(want))
    assert list(vec.table["header"]) == [">s%d" % i for i in table[:, 0]]


# ---------------------------------------------------------------------------------------------------------------------
# domain_pearson
# ---------------------------------------------------------------------------------------------------------------------
DP_WINDOW, DP_SLIDE, DP_TARGET_LEN = 500, 10, 30_400  # 2 991 windows


@functools.lru_cache(maxsize=None)
def dp_case(k):
    """Queries, target, background vectors and the oracle's r — computed once per k and left unchanged."""
    rng = np.random.default_rng(100 + k)
    background = [wc.random_seq(rng, 2000) for _ in range(150)]
    _, mean, std = orc.get_counts(background, k=k)
    queries = [wc.random_seq(rng, L) for L in (400, 650, 1000, 1500, 2100)]
    target = wc.random_seq(rng, DP_TARGET_LEN - 3000) + queries[2] + wc.random_seq(rng, 2000)  # one query sits in the target
    subs, table = wc.substrings([target], DP_WINDOW, DP_SLIDE)
    qn = orc.get_counts(queries, k=k, mean=mean, std=std)[0]
    tn = orc.get_counts(subs, k=k, mean=mean, std=std)[0]
    return dict(k=k, mean=mean, std=std, queries=queries, target=target, table=table, qn=qn, tn=tn, ref=orc.pearson(qn, tn),
                truth=orc.pearson_f64_truth(qn, tn))


def write_fasta(path, names, seqs):
    path.write_text("".join(">%s\n%s\n" % (n, s) for n, s in zip(names, seqs)))
    return str(path)


def assert_parity(got, ref, case):
    ok = np.isfinite(ref)
    assert ok.all()
    res = parity_rule.judge(got, ref, case["truth"], ok, case["qn"], case["tn"])
    assert res["failures"] == [], res["failures"][:5]


@pytest.mark.parametrize("k", [4, 6])
def test_domain_pearson(tmp_path, k):
    from seekr_amd.kmer_counts import BasicCounter
    from seekr_amd.windows import domain_pearson
    case = dp_case(k)
    qfa = write_fasta(tmp_path / "q.fa", ["q%d" % i for i in range(5)], case["queries"])
    tfa = write_fasta(tmp_path / "t.fa", ["chrT"], [case["target"]])
    n = len(case["table"])
    assert 2900 < n < 3100
    results = {}
    for chunk_rows in (64, 1000, n + 500):
        r, table = domain_pearson(qfa, tfa, k, DP_WINDOW, DP_SLIDE, case["mean"], case["std"], chunk_rows=chunk_rows)
        assert r.dtype == np.float32 and r.shape == (5, n)
        assert_parity(r, case["ref"], case)
        assert list(table.columns) == ["header", "start", "end"] and set(table["header"]) == {">chrT"}
        assert np.array_equal(table["start"].to_numpy(), case["table"][:, 1])
        assert np.array_equal(table["end"].to_numpy(), case["table"][:, 1] + case["table"][:, 2])
        results[chunk_rows] = r
    assert_parity(results[1000], results[64], case)
    assert_parity(results[n + 500], results[64], case)
    # the query that sits in the target finds itself: the two windows inside it are its best columns
    best = int(np.argmax(results[64][2]))
    assert DP_TARGET_LEN - 3000 <= case["table"][best, 1] <= DP_TARGET_LEN - 3000 + 500
    # a query given as a normalised count matrix, vectors given as files
    np.save(tmp_path / "mean.npy", case["mean"])
    np.save(tmp_path / "std.npy", case["std"])
    qc = BasicCounter(qfa, k=k, mean=case["mean"], std=case["std"], silent=True)
    qc.get_counts()
    out = tmp_path / "r.npy"
    r2, _ = domain_pearson(qc.counts, tfa, k, DP_WINDOW, DP_SLIDE, str(tmp_path / "mean.npy"), str(tmp_path / "std.npy"),
                           chunk_rows=1000, outfile=str(out))
    assert np.array_equal(bits(r2), bits(results[1000]))
    assert np.array_equal(bits(np.load(out)), bits(r2))
    with pytest.raises(ValueError):
        domain_pearson(qfa, tfa, k, DP_WINDOW, DP_SLIDE, True, case["std"])


@pytest.mark.parametrize("log2", ["Log2.pre", "Log2.none"])
def test_domain_pearson_other_log2_modes(tmp_path, log2):
    from seekr_amd.windows import domain_pearson
    k = 4
    case = dp_case(k)
    background_mean_std = orc.get_counts([case["target"][i:i + 2000] for i in range(0, 24000, 2000)], k=k, log2=log2)[1:]
    mean, std = background_mean_std
    subs, _ = wc.substrings([case["target"]], DP_WINDOW, 100)
    qn = orc.get_counts(case["queries"], k=k, mean=mean, std=std, log2=log2)[0]
    tn = orc.get_counts(subs, k=k, mean=mean, std=std, log2=log2)[0]
    qfa = write_fasta(tmp_path / "q.fa", ["q%d" % i for i in range(5)], case["queries"])
    tfa = write_fasta(tmp_path / "t.fa", ["chrT"], [case["target"]])
    r, _ = domain_pearson(qfa, tfa, k, DP_WINDOW, 100, mean, std, log2=log2, chunk_rows=128)
    ref = orc.pearson(qn, tn)
    res = parity_rule.judge(r, ref, orc.pearson_f64_truth(qn, tn), np.isfinite(ref), qn, tn)
    assert np.isfinite(ref).all() and res["failures"] == [], res["failures"][:5]


@pytest.mark.parametrize("binary", [True, False])
def test_command(tmp_path, binary):
    from seekr_amd.windows import domain_pearson
    k, window, slide = 4, 300, 50
    case = dp_case(k)
    names = ["q%d some text" % i for i in range(5)]
    qfa = write_fasta(tmp_path / "q.fa", names, case["queries"])
    tfa = write_fasta(tmp_path / "t.fa", ["chrT", "chrU"], [case["target"][:5020], case["target"][6000:6500]])
    np.save(tmp_path / "mean.npy", case["mean"])
    np.save(tmp_path / "std.npy", case["std"])
    out = tmp_path / ("r.npy" if binary else "r.csv")
    argv = ["seekr_domain_pearson", qfa, tfa, str(tmp_path / "mean.npy"), str(tmp_path / "std.npy"), "-k", str(k), "-w", str(window),
            "-s", str(slide), "-o", str(out)] + (["-bo"] if binary else [])
    code = ("import sys; sys.argv = %r; from seekr_amd.console_scripts import console_domain_pearson; "
            "console_domain_pearson()") % (argv,)
    proc = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0, proc.stderr
    r, table = domain_pearson(qfa, tfa, k, window, slide, case["mean"], case["std"])
    assert r.shape == (5, 96 + 5)
    if binary:
        assert np.array_equal(bits(np.load(out)), bits(r))
        return
    import pandas as pd
    frame = pd.read_csv(out, index_col=0)
    assert list(frame.index) == [">" + n for n in names]
    labels = ["%s:%d-%d" % (h, s, e) for h, s, e in zip(table["header"], table["start"], table["end"])]
    assert list(frame.columns) == labels and labels[0] == ">chrT:0-300" and labels[-1] == ">chrU:200-500"
    assert np.array_equal(bits(frame.to_numpy().astype(np.float32)), bits(r))  # the writer prints the shortest digits that read back
