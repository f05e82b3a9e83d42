"""The specifications of seekr_amd.explain on the host: the group model is numpy's own arithmetic, the pair model's order
is numpy's stable argsort, and the host-side checks (indices, top, pair files, words) behave."""
import os
import subprocess
import sys

import numpy as np
import pytest

import explain_cases as ec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def numpy_group_stats(x, labels):
    import warnings
    uniq = np.unique(labels)
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")  # "Degrees of freedom <= 0" at n = 1
        mean = np.stack([np.mean(x[labels == g], axis=0) for g in uniq])
        sd = np.stack([np.std(x[labels == g], axis=0, ddof=1) for g in uniq])
    return mean, sd


@pytest.mark.parametrize("w", [2, 3, 16, 17, 64, 625])
def test_group_model_is_numpy(w):
    """Widths >= 2 and group sizes from 2 to 5 000 (numpy 2.2.6 here): np.mean and np.std(ddof=1) of x[labels == g] bit for
    bit.  Two exceptions: at one column numpy adds pairwise and the model is the specification (not compared), and at
    n = 1 both give NaN for sd, compared with isnan."""
    rng = np.random.default_rng(w)
    sizes = [1, 2, 3, 8, 9, 127, 128, 129, 1025, 5000]
    labels = np.repeat(np.arange(len(sizes)) * 3 - 4, sizes)
    rng.shuffle(labels)
    x = ec.group_matrix(len(labels), w, 100 + w)
    uniq, order, starts = ec.order_of(labels)
    mean, sd = ec.group_model(x, order, starts)
    want_mean, want_sd = numpy_group_stats(x, labels)
    assert mean.dtype == want_mean.dtype == np.float32 and sd.dtype == want_sd.dtype == np.float32
    assert np.array_equal(ec.bits(mean), ec.bits(want_mean))
    single = np.diff(starts) == 1
    assert single.sum() == 1 and np.isnan(sd[single]).all() and np.isnan(want_sd[single]).all()
    assert np.array_equal(ec.bits(sd[~single]), ec.bits(want_sd[~single]))


def test_group_model_sums_negative_zeros_as_numpy():
    x = np.full((3, 4), -0.0, np.float32)
    mean, _ = ec.group_model(x, np.arange(3), np.array([0, 3]))
    assert np.array_equal(ec.bits(mean[0]), ec.bits(np.mean(x, axis=0))) and not np.signbit(mean).any()


def test_discriminating_case():
    """The sequential float32 mean of the 1 025-row case is not float32(mean in float64): a tree-reducing kernel, which
    would land on the latter far more often, cannot pass the GPU test by being more accurate."""
    x = ec.discriminating_group()
    mean, sd = ec.group_model(x, np.arange(len(x)), np.array([0, len(x)]))
    exact = x.astype(np.float64).mean(axis=0).astype(np.float32)
    assert np.array_equal(ec.bits(mean[0]), ec.bits(np.mean(x, axis=0)))
    assert (ec.bits(mean[0]) != ec.bits(exact)).any()
    exact_sd = x.astype(np.float64).std(axis=0, ddof=1).astype(np.float32)
    assert (ec.bits(sd[0]) != ec.bits(exact_sd)).any()


def order_vectors():
    rng = np.random.default_rng(11)
    a = rng.standard_normal(500).astype(np.float32)
    ties = (rng.integers(-2, 3, 500) / 2.0).astype(np.float32)
    ties[::5] = -0.0
    special = ties.copy()
    special[3::17] = np.nan
    special[5::19] = np.inf
    special[7::23] = -np.inf
    return {"random": a, "ties and zeros": ties, "nan and inf": special, "all nan": np.full(40, np.nan, np.float32),
            "all equal": np.ones(70, np.float32), "one": np.array([2.5], np.float32),
            "signed zeros": np.array([0.0, -0.0, -0.0, 0.0], np.float32)}


@pytest.mark.parametrize("name", list(order_vectors()))
def test_pair_model_order_is_the_stable_argsort(name):
    c = order_vectors()[name]
    for key in (c, -c):
        assert np.array_equal(ec.model_order(key), np.argsort(-key, kind="stable"))


def test_pair_model_values_and_pads():
    z1, z2 = ec.special_rows(50)
    rows, cols = ec.all_pairs(6, 6)
    idx, val, f1, f2 = ec.pair_model(z1, z2, rows, cols, 64, largest=False)
    assert (idx[:, 50:] == ec.PAD_IDX).all() and (ec.bits(val[:, 50:]) == ec.PAD_BITS).all()
    with np.errstate(all="ignore"):
        for e in (0, 7, 35):
            c = z1[rows[e]] * z2[cols[e]]
            assert np.array_equal(idx[e, :50], np.argsort(c, kind="stable"))  # the order of -c
            assert np.array_equal(ec.bits(val[e, :50]), ec.bits(c[idx[e, :50]]))  # c's own bits, not the negated ones
            assert np.array_equal(ec.bits(f1[e, :50]), ec.bits(z1[rows[e]][idx[e, :50]]))


# ---- host-side checks -------------------------------------------------------------------------------------------------------
def test_index_validation_names_the_first_bad_pair():
    from seekr_amd import explain
    rows, cols = explain.check_pairs([0, 4, 2], np.array([1, 1, 8], np.int64), 5, 9)
    assert rows.dtype == cols.dtype == np.uint32 and list(rows) == [0, 4, 2] and list(cols) == [1, 1, 8]
    with pytest.raises(ValueError, match=r"pair 2 = \(5, 0\) is the first bad one"):
        explain.check_pairs([0, 1, 5, 9], [0, 0, 0, 0], 5, 9)
    with pytest.raises(ValueError, match=r"pair 1 = \(1, 9\) is the first bad one"):
        explain.check_pairs([0, 1, 5], [0, 9, 0], 5, 9)
    with pytest.raises(ValueError, match=r"pair 0 = \(-1, 0\)"):
        explain.check_pairs(np.array([-1]), np.array([0]), 5, 9)
    with pytest.raises(ValueError, match="one length"):
        explain.check_pairs([0, 1], [0], 5, 9)
    with pytest.raises(ValueError, match="integers"):
        explain.check_pairs([0.5], [0], 5, 9)
    with pytest.raises(ValueError, match="1-D"):
        explain.check_pairs([[0]], [[0]], 5, 9)
    r0, c0 = explain.check_pairs([], [], 5, 9)
    assert len(r0) == len(c0) == 0 and r0.dtype == np.uint32


def test_arguments_are_refused_before_any_launch():
    """No GPU here: each of these must raise its ValueError before the library is asked for a context."""
    from seekr_amd import _lib, explain
    x = np.zeros((4, 8), np.float32)
    for top in (0, _lib.TOPK_MERGE_KMAX + 1, 2.5):
        with pytest.raises(ValueError, match="top"):
            explain.pair_kmers(x, [0], [1], top=top)
        with pytest.raises(ValueError, match="top"):
            explain.group_kmers(x, [0, 0, 1, 1], top=top)
    with pytest.raises(ValueError, match="pair 1"):
        explain.pair_kmers(x, [0, 4], [1, 1])
    with pytest.raises(ValueError, match="pair 0"):
        explain.pair_kmers(x, [0], [3], counts2=np.zeros((3, 8), np.float32))
    with pytest.raises(ValueError, match="same number of columns"):
        explain.pair_kmers(x, [0], [0], counts2=np.zeros((3, 9), np.float32))
    with pytest.raises(ValueError, match="cols is missing"):
        explain.pair_kmers(x, [0])
    with pytest.raises(ValueError, match="k-mer names"):
        explain.pair_kmers(x, [0], [1], kmers=["A", "C"])
    with pytest.raises(ValueError, match="labels"):
        explain.group_kmers(x, [0, 1, 2])
    with pytest.raises(ValueError, match="integer"):
        explain.group_kmers(x, np.array([0.0, 1.0, 1.0, 0.0]))
    empty = explain.pair_kmers(x, [], [], top=3)  # no pairs: nothing is launched
    assert empty.idx.shape == empty.contribution.shape == empty.z_row.shape == empty.z_col.shape == (0, 3)


def test_topk_limit_is_mirrored():
    from seekr_amd import _lib
    with open(os.path.join(ROOT, "seekr_amd", "csrc", "explain.hip")) as f:
        src = f.read()
    assert "constexpr int kPairKmax = %d;" % _lib.TOPK_MERGE_KMAX in src and "skr_topk_merge_limits(&kmax" in src
    with open(os.path.join(ROOT, "seekr_amd", "build.py")) as f:
        assert '"explain.hip": ["-ffp-contract=off"]' in f.read()


def test_words_drop_pads():
    from seekr_amd import _lib, explain
    idx = np.array([[2, 0, _lib.TOPK_PAD_IDX], [1, _lib.TOPK_PAD_IDX, _lib.TOPK_PAD_IDX]], np.uint32)
    nan = np.full((2, 3), np.nan, np.float32)
    res = explain.PairKmers(idx, nan, nan, nan, kmers=["AA", "AG", "AT"])
    assert res.words() == [["AT", "AA"], ["AG"]] and len(res) == 2
    assert res.words(["x", "y", "z"]) == [["z", "x"], ["y"]]
    with pytest.raises(ValueError, match="no name"):
        res.words(["x", "y"])
    with pytest.raises(ValueError, match="no k-mer names"):
        explain.PairKmers(idx, nan, nan, nan).words()


def test_top_columns_is_the_same_order_rule():
    from seekr_amd import explain
    v = np.array([[1.0, np.nan, 3.0, 3.0, -0.0, 0.0], [np.nan] * 6], np.float32)
    idx, val = explain.top_columns(v, 8)
    assert list(idx[0]) == [2, 3, 0, 4, 5, 1, ec.PAD_IDX, ec.PAD_IDX] and list(idx[1][:6]) == [0, 1, 2, 3, 4, 5]
    assert np.array_equal(ec.bits(val[0, :6]), ec.bits(v[0][[2, 3, 0, 4, 5, 1]])) and (ec.bits(val[:, 6:]) == ec.PAD_BITS).all()
    idx, _ = explain.top_columns(v, 3, largest=False)
    assert list(idx[0]) == [4, 5, 0]
    for i in range(2):
        assert np.array_equal(explain.top_columns(v, 6)[0][i], ec.model_order(v[i]))


def test_group_order():
    from seekr_amd import explain
    labels = ec.interleaved_labels()
    uniq, sizes, order, starts = explain.group_order(labels)
    want_uniq, want_order, want_starts = ec.order_of(labels)
    assert np.array_equal(uniq, want_uniq) and np.array_equal(order, want_order) and np.array_equal(starts, want_starts)
    assert order.dtype == np.uint32 and starts.dtype == np.int64 and sizes.sum() == len(labels)
    for g, label in enumerate(uniq):
        assert np.array_equal(order[starts[g]:starts[g + 1]], np.flatnonzero(labels == label))


def test_pair_files_of_both_commands(tmp_path):
    from seekr_amd import explain
    a = tmp_path / "sig.csv"
    a.write_text('row,col,r,p,p_adj\ntx1,"tx4, v1",0.5,0.001,0.01\n3,0,0.4,0.002,0.02\n')
    names = ["tx0", "tx1", "tx2", "tx3", "tx4, v1"]
    rows, cols = explain.read_pairs_csv(a, names, names)
    assert list(rows) == [1, 3] and list(cols) == [4, 0] and rows.dtype == np.int64
    b = tmp_path / "near.csv"
    b.write_text("row,rank,neighbor,r\n0,0,7,0.9\n0,1,2,0.8\n5,0,1,0.7\n")
    rows, cols = explain.read_pairs_csv(b)
    assert list(rows) == [0, 0, 5] and list(cols) == [7, 2, 1]
    c = tmp_path / "bad.csv"
    c.write_text("a,b\n0,1\n")
    with pytest.raises(ValueError, match="header"):
        explain.read_pairs_csv(c)
    d = tmp_path / "bad2.csv"
    d.write_text("row,col,r\n0,nobody,0.5\n")
    with pytest.raises(ValueError, match="line 2"):
        explain.read_pairs_csv(d, names, names)
    e = tmp_path / "empty.csv"
    e.write_text("row,col,r,p,p_adj\n")
    rows, cols = explain.read_pairs_csv(e)
    assert len(rows) == len(cols) == 0


def test_commands_help_and_entry_points():
    code = "import sys; sys.argv = ['seekr_pair_kmers', '-h']; from seekr_amd.console_scripts import console_pair_kmers; console_pair_kmers()"
    proc = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert proc.returncode == 0, proc.stderr
    for flag in ("--top", "--outfile", "--binary_input", "--kmer", "--alphabet", "--smallest"):
        assert flag in proc.stdout
    code = "import sys; sys.argv = ['seekr_kmer_leiden', '-h']; from seekr_amd.console_scripts import console_kmer_leiden; console_kmer_leiden()"
    proc = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert proc.returncode == 0 and "--kmers_top" in proc.stdout, proc.stderr
    with open(os.path.join(ROOT, "setup.py")) as f:
        assert "seekr_pair_kmers = seekr_amd.console_scripts:console_pair_kmers" in f.read()


def test_kmer_leiden_takes_kmers_top_and_nothing_else():
    from seekr_amd.kmer_leiden import kmer_leiden
    with pytest.raises(ValueError, match="kmers_top"):
        kmer_leiden("x.fa", "m.npy", "s.npy", 4, kmers_top=0)
    with pytest.raises(TypeError, match="unexpected keyword argument 'kmers'"):
        kmer_leiden("x.fa", "m.npy", "s.npy", 4, kmers=3)


def test_write_kmers_csv(tmp_path):
    from seekr_amd import explain
    from seekr_amd.kmer_leiden import write_kmers_csv
    mean = np.array([[0.5, 2.0, 1.0], [3.0, np.nan, 4.0]], np.float32)
    sd = np.array([[0.1, 0.2, 0.3], [np.nan] * 3], np.float32)
    groups = explain.GroupKmers(np.array([0, 1]), np.array([5, 1]), mean, sd, *explain.top_columns(mean, 2), ["AA", "AG", "AT"])
    write_kmers_csv(tmp_path / "k.csv", groups)
    assert (tmp_path / "k.csv").read_text().splitlines() == [
        "Community,Size,Rank,Kmer,Mean,Sd", "0,5,0,AG,2.0,0.2", "0,5,1,AT,1.0,0.3", "1,1,0,AT,4.0,nan", "1,1,1,AA,3.0,nan"]
