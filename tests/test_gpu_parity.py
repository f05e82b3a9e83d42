"""Parity of the HIP path (through the C-ABI / the seekr_amd API) with the oracle and with the
golden vectors captured from the reference.  Needs a real MI355X: run with `-m gpu`.

Bars (BASELINE.json north_star): integer counts and everything that is pure IEEE arithmetic
(per-kb float32 counts, column mean/std, centred / standardised values) BIT-EXACT;
log2 outputs and Pearson r within |a-b| <= atol + 1e-5 |b| with atol stated per test.
"""
import hashlib
import io
import json
import os
import contextlib

import numpy as np
import pytest

from oracle import seekr_oracle as orc
from exact_sum_cases import f16_halves
from inputs import EXAMPLE_FA, big_count_matrix, skewed_set, synth_2000, write_fasta

pytestmark = pytest.mark.gpu

RTOL = 1e-5
ATOL_R = 2e-6      # Pearson r (the reference's own error vs fp64 is 4.8e-7)
ATOL_LOG = 1e-6    # log2 outputs (values in [0, ~5]; device log2f vs numpy log2: <= 1 ulp)


def sha16(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_bits(a, b, what=""):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    bad = bits(a) != bits(b)
    both_nan = np.isnan(a) & np.isnan(b)
    bad &= ~both_nan
    assert not bad.any(), "{}: {} of {} cells differ, first at {}: {} vs {}".format(
        what, int(bad.sum()), bad.size, np.argwhere(bad)[0], a[bad][0], b[bad][0])


@pytest.fixture(scope="module")
def L():
    from seekr_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def ctx(L):
    return L.default_context()


@pytest.fixture(scope="module")
def gold(golden_dir):
    out = {name: np.load(os.path.join(golden_dir, name + ".npz")) for name in
           ("reference_fixtures", "g1_example", "g3_skewed", "g4_synth2000", "g5_bigN", "g6_edges")}
    with open(os.path.join(golden_dir, "meta.json")) as fh:
        out["meta"] = json.load(fh)
    return out


@pytest.fixture(scope="module")
def example_fa(tmp_path_factory):
    p = tmp_path_factory.mktemp("fa") / "example.fa"
    p.write_text(EXAMPLE_FA)
    return str(p)


def counter(seqs=None, **kw):
    from seekr_amd.kmer_counts import BasicCounter
    c = BasicCounter(silent=True, **kw)
    if seqs is not None:
        c.seqs = list(seqs)
    return c


def run(seqs, **kw):
    c = counter(seqs, **kw)
    with contextlib.redirect_stdout(io.StringIO()):
        c.get_counts()
    return c


# ------------------------------------------------------------------ config 1 + reference KATs
def test_cfg1_example_raw_counts_bitexact(example_fa, gold, L, ctx):
    from seekr_amd.kmer_counts import BasicCounter
    g1 = gold["g1_example"]
    for k in (1, 2, 3):
        c = BasicCounter(example_fa, k=k, mean=False, std=False, log2="Log2.none", silent=True)
        c.get_counts()
        assert c.counts.dtype == np.float32
        assert_bits(c.counts, g1["raw_k%d" % k], "example raw k=%d" % k)
        assert sha16(c.counts) == gold["meta"]["example_raw_k%d_sha" % k]
    n = L.count_u32(ctx, ctx.pack_fasta(example_fa), 2).to_numpy()
    assert n.dtype == np.uint32 and n.sum(axis=1).tolist() == [5, 11, 15, 74, 75]
    assert np.array_equal(n, orc.count_kmers_u32(orc.read_fasta(example_fa)[1], 2))


def test_reference_known_answers_through_api(example_fa, gold):
    """seekr/tests/test_kmer_counts.py:13-117 and test_pearson.py:7-24 replayed on the HIP path."""
    from seekr_amd.kmer_counts import BasicCounter
    from seekr_amd.pearson import pearson
    c = BasicCounter(example_fa, k=1, silent=True)
    assert len(c.seqs) == 5 and c.seqs[0] == "AAAAAA"
    assert np.allclose(c.occurrences(np.zeros(4), c.seqs[0]), [1000, 0, 0, 0])
    assert np.allclose(c.occurrences(np.zeros(4), c.seqs[1]), [0, 500, 500, 0])
    c2 = BasicCounter(example_fa, k=2, silent=True)
    exp = np.zeros(16)
    exp[5], exp[9], exp[10] = 454.545, 90.909, 454.545
    row = c2.occurrences(np.zeros(16), c2.seqs[1])
    assert np.allclose(row, exp)
    assert np.array_equal(row, gold["g6_edges"]["kat_occ_k2_seq1"])  # float64 row: exact replay
    # center / standardize / log2_norm on hand-assigned matrices
    c.counts = np.array([[1, 2, 3, 4], [1, -2, 5, 10]], dtype=np.float32)
    c.center()
    assert np.allclose(c.counts, [[0, 2, -1, -3], [0, -2, 1, 3]])
    c = BasicCounter(example_fa, k=1, silent=True)
    c.counts = np.array([[1, 2, 3, 4], [1, -2, 5, 10]], dtype=np.float32)
    c.mean = np.array([1, 1, 1, -1.0])
    c.center()
    assert np.allclose(c.counts, [[0, 1, 2, 5], [0, -3, 4, 11]])
    c = BasicCounter(example_fa, k=1, silent=True)
    c.counts = np.array([[1, 2, 3, 4], [0, -2, 5, 10]], dtype=np.float32)
    c.standardize()
    assert np.allclose(c.counts, [[2, 1, 3, 4 / 3], [0, -1, 5, 10 / 3]])
    c = BasicCounter(example_fa, k=1, silent=True)
    c.counts = np.array([[1, 2, 3, 4], [0, -2, 5, 10]], dtype=np.float32)
    c.std = np.arange(1, 5)
    c.standardize()
    assert np.allclose(c.counts, [[1, 1, 1, 1], [0, -1, 5 / 3, 2.5]])
    c.counts = np.array([[3, 4, 5, 6], [2, 0, 7, 12]], dtype=np.float32)
    c.log2_norm()
    assert np.allclose(c.counts, np.log2(np.array([[4, 5, 6, 7], [3, 1, 8, 13]], dtype=np.float32)))
    c = BasicCounter(example_fa, k=1, silent=True)
    c.get_counts()
    expected = np.array([[2.1798673, 0.27807194, 0.0, 0.5133058],
                         [0.6370419, 2.1100981, 2.048016, 0.5133058],
                         [1.2010899, 1.4672222, 1.3604679, 1.8107259],
                         [1.2073011, 1.3895708, 1.3721647, 1.8666755],
                         [1.318994, 1.1856667, 1.5349197, 1.6688585]], dtype=np.float32)
    assert np.allclose(c.counts, expected, rtol=1e-4, atol=1e-5)
    # pearson literals (integer inputs -> float64 path)
    c1 = np.array([[8, 5, 6, 9, 2], [8, 3, 6, 6, 7], [7, 7, 3, 3, 7]])
    c2_ = np.array([[2, 8, -9, -1, -8], [-4, 1, 2, -1, 2], [5, -3, -7, 2, -9]])
    r = pearson(c1, c2_)
    assert r.dtype == np.float64
    assert np.allclose(r, [[0.3217847, -0.71611487, 0.85110363], [-0.52756992, -0.47172818, 0.22652512],
                           [0.43762719, -0.17902872, 0.01547461]])
    assert np.allclose(r, gold["g6_edges"]["kat_pearson_int"], rtol=1e-12, atol=1e-14)
    one = np.array([[1, 2, 3, 4], [2, 4, 6, 8]])
    assert np.allclose(pearson(one, one), np.ones((2, 2)))


def test_reference_data_fixtures_through_cli(example_fa, gold, tmp_path):
    """seekr/tests/test_console_scripts.py:34-124 against the reference's own data files."""
    from seekr_amd import console_scripts as cs
    fx = gold["reference_fixtures"]
    out = str(tmp_path / "2mers.npy")
    cs._run_kmer_counts(example_fa, out, 2, True, True, True, "Log2.post", True, None, None, "AGTC")
    assert np.allclose(np.load(out), fx["example_2mers_counts"])
    out = str(tmp_path / "3mers.csv")
    cs._run_kmer_counts(example_fa, out, 3, False, False, False, "Log2.none", True, None, None, "AGTC")
    assert np.array_equal(np.loadtxt(out, delimiter=","), fx["example_3mers_raw_csv"])
    mv, sv = str(tmp_path / "mean.npy"), str(tmp_path / "std.npy")
    cs._run_norm_vectors(example_fa, mv, sv, "Log2.none", 2)
    assert_bits(np.load(mv), fx["example_mean"], "norm vector mean")
    assert_bits(np.load(sv), fx["example_std"], "norm vector std")
    out = str(tmp_path / "2mers_vectors.npy")
    cs._run_kmer_counts(example_fa, out, 2, True, False, False, "Log2.post", True, mv, sv, "AGTC")
    assert np.allclose(np.load(out), fx["example_2mers_count"])
    # seekr_pearson: .npy in/out and labelled csv in/out
    cs._run_kmer_counts(example_fa, str(tmp_path / "lab.csv"), 2, False, True, True, "Log2.post", False, None, None,
                        "AGTC")
    cs._run_pearson(str(tmp_path / "lab.csv"), str(tmp_path / "lab.csv"), str(tmp_path / "r.csv"), False, False)
    import pandas as pd
    rdf = pd.read_csv(str(tmp_path / "r.csv"), index_col=0)
    assert list(rdf.index) == [">SEQ1", ">SEQ2", ">SEQ3", ">SEQ4", ">SEQ5"] == list(rdf.columns)
    cs._run_pearson(str(tmp_path / "2mers.npy"), str(tmp_path / "2mers.npy"), str(tmp_path / "r.npy"), True, True)
    rb = np.load(str(tmp_path / "r.npy"))
    assert rb.dtype == np.float32
    assert np.allclose(rb, orc.pearson(fx["example_2mers_counts"], fx["example_2mers_counts"]), rtol=RTOL, atol=ATOL_R)
    assert np.allclose(rdf.values, rb, rtol=1e-5, atol=1e-5)  # csv text round trip of the counts


# ------------------------------------------------------------------ golden vectors
def test_g1_example_pipelines(example_fa, gold):
    g1 = gold["g1_example"]
    seqs = orc.read_fasta(example_fa)[1]
    for k in (1, 2):
        for tag in ("post", "pre", "none"):
            mode = "Log2." + tag
            with np.errstate(all="ignore"):
                c = run(seqs, k=k, log2=mode)
                if tag == "pre":  # statistics of log2 values: device log2f may differ in the last ulp
                    assert np.allclose(c.mean, g1["full_pre_k%d_mean" % k], rtol=RTOL, atol=ATOL_LOG)
                    assert np.allclose(c.std, g1["full_pre_k%d_std" % k], rtol=RTOL, atol=ATOL_LOG)
                else:
                    assert_bits(c.mean, g1["full_%s_k%d_mean" % (tag, k)], "mean %s k%d" % (tag, k))
                    assert_bits(c.std, g1["full_%s_k%d_std" % (tag, k)], "std %s k%d" % (tag, k))
                if tag == "none":
                    assert_bits(c.counts, g1["full_none_k%d" % k], "z k%d" % k)
                else:
                    assert np.allclose(c.counts, g1["full_%s_k%d" % (tag, k)], rtol=RTOL, atol=2e-6, equal_nan=True)
                v = run(seqs, k=k, log2=mode, mean=g1["mean_none_k%d" % k], std=g1["std_none_k%d" % k])
                assert np.allclose(v.counts, g1["vec_%s_k%d" % (tag, k)], rtol=RTOL, atol=2e-6, equal_nan=True)
                mo = run(seqs, k=k, log2=mode, mean=True, std=False)
                assert np.allclose(mo.counts, g1["meanonly_%s_k%d" % (tag, k)], rtol=RTOL, atol=2e-6, equal_nan=True)


def test_g3_skewed_sets_counts_and_pearson(gold):
    from seekr_amd.pearson import pearson
    g3 = gold["g3_skewed"]
    s1, s2 = skewed_set(101, 111), skewed_set(202, 151)
    assert_bits(run(s1, k=4, mean=False, std=False, log2="Log2.none").counts, g3["s1_raw_k4"], "raw k4")
    for k in (4, 5):
        nv = run(s1, k=k)
        assert_bits(nv.mean, g3["mean_k%d" % k], "mean k%d" % k)
        assert_bits(nv.std, g3["std_k%d" % k], "std k%d" % k)
        c1 = run(s1, k=k, mean=nv.mean, std=nv.std)
        c2 = run(s2, k=k, mean=nv.mean, std=nv.std)
        if k == 4:
            assert np.allclose(c1.counts, g3["s1_counts_k4"], rtol=RTOL, atol=ATOL_LOG)
            assert np.allclose(nv.counts, g3["s1_self_default_k4"], rtol=RTOL, atol=ATOL_LOG)
        r = pearson(c1.counts, c2.counts)
        assert r.dtype == np.float32 and r.shape == (111, 151)
        assert np.allclose(r, g3["pearson_k%d" % k], rtol=RTOL, atol=ATOL_R)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        x6 = counter(s1, k=6)
        x6.get_counts()
    assert "WARNING: You have `np.nan` values" in buf.getvalue()
    assert np.isnan(x6.counts).all()  # NaN propagates through np.min (kmer_counts.py:208)
    assert np.isnan(pearson(x6.counts, x6.counts)).all()
    a, b = g3["s1_counts_k4"][:7], g3["s1_counts_k4"][7:12]
    assert np.allclose(pearson(a, b, row_standardize=False), g3["pearson_nostd"], rtol=RTOL, atol=ATOL_R)
    r64 = pearson(a.astype(np.float64), b.astype(np.float64))
    assert r64.dtype == np.float64 and np.allclose(r64, g3["pearson_f64"], rtol=1e-12, atol=1e-14)
    rm = pearson(a, b.astype(np.float64))
    # the float32 operand is standardised in float32 (its own dtype) before the promotion
    assert rm.dtype == np.float64 and np.allclose(rm, g3["pearson_mixed"], rtol=RTOL, atol=ATOL_R)


def test_pearson_returns_the_references_dtype_for_every_operand_pair(tmp_path):
    """pearson.py:35-41 lets numpy promote: a float dtype survives np.mean / np.std, integers become float64, np.inner takes
    the wider of the two.  The dtype of r for every pair — float16 included, where the value is the float64 result rounded to
    the reference's dtype (the reference's own half-precision arithmetic is 1e-3 away from the truth; held to that)."""
    from seekr_amd.pearson import pearson, pearson_to_file
    rng = np.random.default_rng(3)
    a, b = rng.poisson(2.0, size=(9, 64)), rng.poisson(2.0, size=(7, 64))
    for d1, d2 in (("float16", "float16"), ("float16", "float32"), ("float32", "float16"), ("float16", "float64"), ("int32", "float32"),
                   ("float16", "int32"), ("uint8", "uint8"), ("float32", "float32"), ("float64", "float32"), ("bool", "float16")):
        x, y = (a > 1 if d1 == "bool" else a).astype(d1), b.astype(d2)
        with np.errstate(all="ignore"):
            want = orc.pearson(x, y)
        got = pearson(x, y)
        assert got.dtype == want.dtype and got.shape == want.shape, (d1, d2, got.dtype, want.dtype)
        tol = 2e-2 if "float16" in (d1, d2) else 1e-5
        assert np.allclose(got.astype(np.float64), want.astype(np.float64), rtol=tol, atol=tol), (d1, d2)
    out = str(tmp_path / "r16.npy")
    pearson_to_file(a.astype("float16"), b.astype("float16"), out)
    assert np.load(out).dtype == np.float16 and np.array_equal(np.load(out), pearson(a.astype("float16"), b.astype("float16")))


def test_g4_synthetic_2000x2kb(gold, L, ctx):
    from seekr_amd.pearson import pearson
    g4, meta = gold["g4_synth2000"], gold["meta"]
    seqs = synth_2000()
    packed = ctx.pack(seqs, "AGTC")
    n = L.count_u32(ctx, packed, 6).to_numpy()
    assert sha16(n) == meta["g4_u32_sha"] and int(n.sum()) == 2000 * 1995
    raw = L.count_per_kb(ctx, packed, 6).to_numpy()
    assert sha16(raw) == meta["g4_raw_sha"]
    for tag in ("post", "none", "pre"):
        c = run(seqs, k=6, log2="Log2." + tag)
        if tag == "pre":
            assert np.allclose(c.mean, g4["mean_pre"], rtol=RTOL, atol=ATOL_LOG)
            assert np.allclose(c.std, g4["std_pre"], rtol=RTOL, atol=ATOL_LOG)
        else:
            assert_bits(c.mean, g4["mean_" + tag], "mean " + tag)
            assert_bits(c.std, g4["std_" + tag], "std " + tag)
        if tag == "none":
            assert sha16(c.counts) == meta["g4_counts_none_sha"]
        assert np.allclose(c.counts[:8], g4["counts_%s_head" % tag], rtol=RTOL, atol=2e-6)
        r = pearson(c.counts[:256], c.counts[:256])
        assert np.allclose(r, g4["pearson256_" + tag], rtol=RTOL, atol=ATOL_R)


def test_g5_large_n_column_stats_bitexact(gold, L, ctx):
    """50 000 rows: float32 row-sequential drift must be reproduced, not improved upon."""
    g5 = gold["g5_bigN"]
    big = big_count_matrix()
    c = counter(["ACGT"] * 2, k=6)
    c.counts = big
    c.center()
    assert_bits(c.mean, g5["mean"], "mean 50k")
    c.standardize()
    assert_bits(c.std, g5["std"], "std 50k")
    assert_bits(c.counts[0], g5["z_row0"], "z row 0")
    assert_bits(c.counts[-1], g5["z_rowlast"], "z last row")
    dev = ctx.from_numpy(c.counts)
    mn, has_nan = L.min_nan(ctx, dev)
    assert not has_nan and np.float32(mn) == g5["z_min"]


def test_g6_edges(example_fa, gold, tmp_path):
    from seekr_amd.kmer_counts import BasicCounter
    from seekr_amd.fasta_reader import Reader
    from seekr_amd.pearson import pearson
    g6, edge = gold["g6_edges"], gold["meta"]["edge"]
    assert_bits(run(edge["edge_seqs"], k=3, mean=False, std=False, log2="Log2.none").counts, g6["edge_raw_k3"], "edges")
    with pytest.raises(ZeroDivisionError):
        run(["ACGTAC", "AC"], k=3, mean=False, std=False, log2="Log2.none")
    seqs = orc.read_fasta(example_fa)[1]
    assert_bits(run(seqs, k=2, mean=False, std=False, log2="Log2.none", alphabet="ACGT").counts, g6["raw_k2_ACGT"], "ACGT")
    # reader: python mirror and native packer agree with the reference on a CRLF / multi-line / lower-case file
    rs = skewed_set(303, 6, 50, 200)
    p = str(tmp_path / "ml.fa")
    write_fasta(p, rs, width=60, crlf=True, lower=True)
    assert Reader(p).get_seqs() == rs and Reader(p).get_headers() == edge["reader_headers"]
    native = BasicCounter(p, k=3, mean=False, std=False, log2="Log2.none", silent=True)
    native.get_counts()
    assert_bits(native.counts, orc.raw_counts(rs, 3), "native fasta")
    assert native._packed.headers() == edge["reader_headers"]
    for name, text, exc in (("blank_line", ">a\nACGT\n\n>b\nACGT\n", IndexError),
                            ("double_header", ">a\nACGT\n>b\n>c\nACGT\n", AssertionError)):
        q = tmp_path / (name + ".fa")
        q.write_text(text)
        for make in (lambda: Reader(str(q)).get_seqs(), lambda: BasicCounter(str(q), k=2)):
            with pytest.raises(exc) as info:
                make()
            assert edge["reader_" + name] == type(info.value).__name__ + ": " + str(info.value)
    one = tmp_path / "one.fa"
    one.write_text(">a\nACGTACGT\n")
    with pytest.raises(ValueError) as info:
        BasicCounter(str(one), k=2)
    assert edge["single_seq_infasta"] == "ValueError: " + str(info.value)
    with pytest.raises(ValueError) as info:
        BasicCounter(example_fa, k=2, log2="log2")
    assert edge["bad_log2"] == "ValueError: " + str(info.value)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf), np.errstate(all="ignore"):
        c = counter(seqs, k=3, log2="Log2.none")
        c.get_counts()
    assert buf.getvalue() == edge["nan_warning_text"]
    assert_bits(c.counts, g6["example_k3_none_with_nan"], "k3 none NaN pattern")
    with contextlib.redirect_stdout(io.StringIO()):
        c = counter(seqs, k=3, log2="Log2.post")
        c.get_counts()
    assert np.isnan(c.counts).all()
    c = run(seqs, k=1, log2="Log2.none", mean=np.array([100.0, 200.5, 300.25, 50.125]), std=np.array([3, 7, 11, 13]))
    assert_bits(c.counts, g6["user_vec_f64_int_k1"], "f64/int user vectors")
    m = np.array([[1, 2, 3, 4], [5, 5, 5, 5], [4, 1, 3, 2]], dtype=np.float32)
    r = pearson(m, m)
    assert np.array_equal(np.isnan(r), np.isnan(g6["pearson_const_row"]))
    assert np.allclose(r, g6["pearson_const_row"], equal_nan=True, rtol=RTOL, atol=ATOL_R)
    with pytest.raises(ValueError):
        pearson(np.zeros((2, 4), np.float32), np.zeros((2, 5), np.float32), row_standardize=False)
    # save modes
    out = str(tmp_path / "counts.seekr")
    c = BasicCounter(example_fa, outfile=out, k=2, binary=True, label=False, silent=True)
    c.make_count_file()
    assert sorted(f for f in os.listdir(tmp_path) if f.startswith("counts.seekr")) == edge["npy_suffix_written"]
    out = str(tmp_path / "plain.csv")
    BasicCounter(example_fa, outfile=out, k=2, binary=False, label=False, silent=True, mean=False, std=False,
                 log2="Log2.none").make_count_file()
    assert open(out).readline().strip() == edge["plain_csv_first_line"]
    out = str(tmp_path / "label.csv")
    BasicCounter(example_fa, outfile=out, k=1, binary=False, label=True, silent=True, mean=False, std=False,
                 log2="Log2.none").make_count_file()
    assert open(out).read() == edge["label_csv_text"]
    with pytest.raises(AssertionError):
        BasicCounter(example_fa, outfile=out, k=1, binary=True, label=True, silent=True).save()


# ------------------------------------------------------------------ seeded sweeps vs the oracle
def ragged_set(seed, n, lo, hi, n_rate=0.002):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        length = int(rng.integers(lo, hi + 1))
        s = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=length)
        bad = rng.random(length) < (n_rate if i % 3 == 0 else 0.0)
        s = np.where(bad, ord("N"), s).astype(np.uint8)
        out.append(s.tobytes().decode())
    # adversarial rows: homopolymer, dinucleotide repeat, all-N, shorter than k, exactly k
    out += ["A" * 5000, "AC" * 3000, "N" * 300, "ACG", "ACGTACG", "T" * 70000, "ACGT" * 16 + "N" + "ACGT" * 16]
    return out


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 6, 7])
def test_counts_bitexact_vs_oracle_ragged(k, L, ctx):
    seqs = [s for s in ragged_set(11 + k, 300, 1, 3000) if len(s) != k - 1]
    packed = ctx.pack(seqs, "AGTC")
    n_gpu = L.count_u32(ctx, packed, k).to_numpy()
    n_ref = orc.count_kmers_u32(seqs, k)
    assert np.array_equal(n_gpu, n_ref)
    raw_gpu = L.count_per_kb(ctx, packed, k).to_numpy()
    assert_bits(raw_gpu, orc.per_kb_from_counts(n_ref, [len(s) for s in seqs], k), "per-kb k=%d" % k)
    f64 = L.count_per_kb(ctx, packed, k, dtype=np.float64).to_numpy()
    assert np.array_equal(f64, orc.per_kb_from_counts(n_ref, [len(s) for s in seqs], k, dtype=np.float64))


@pytest.mark.parametrize("k", [3, 6, 7])
def test_long_sequences_are_cut_into_tiles(k, L, ctx):
    """Sequences of more than 8 192 windows are counted as tiles of 8 192 windows spread over the chip and
    summed (count.hip: reduce_tiles_kernel) — the reference handles any length (kmer_counts.py:140-151;
    its shipped background holds the ~90 kb Airn).  Lengths on both sides of every tile boundary, N runs
    across a boundary, homopolymers (one bin holds every window: far past a 16-bit counter), a 5 Mbase
    sequence; raw counts bit-exact against the C oracle, per-kb float32 bit-exact."""
    from oracle import c_oracle as co
    rng = np.random.default_rng(100 + k)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)

    def rnd(n):
        return letters[rng.integers(0, 4, size=n)].copy()

    arrs = [rnd(n) for n in (8191 + k - 1, 8192 + k - 1, 8193 + k - 1, 16384 + k - 1, 16385 + k, 30011, 90_000, 5_000_000)]
    with_n = rnd(40_000)
    with_n[8180:8215] = ord("N")        # a run of N across the first tile boundary
    with_n[16384 + 3] = ord("N")
    with_n[-1] = ord("N")
    arrs += [with_n, np.full(70_000, ord("T"), np.uint8), np.frombuffer(b"AC" * 20_000, np.uint8),
             np.frombuffer(b"ACG" * 11_000, np.uint8), rnd(700), rnd(2000), np.full(9000, ord("A"), np.uint8)]
    seqs = [a.tobytes().decode() for a in arrs]
    blob, offsets = co.seqs_to_blob(seqs)
    n_ref = co.count_u32(blob, offsets, k)
    packed = ctx.pack(seqs, "AGTC")
    assert np.array_equal(L.count_u32(ctx, packed, k).to_numpy(), n_ref)
    lens = [len(s) for s in seqs]
    assert_bits(L.count_per_kb(ctx, packed, k).to_numpy(), co.per_kb_f32(n_ref, lens, k), "per-kb of long sequences, k=%d" % k)
    want_pre = orc.log2_plus_one(co.per_kb_f32(n_ref, lens, k))
    got_pre = L.count_per_kb(ctx, packed, k, log2_pre=True).to_numpy()
    assert np.allclose(got_pre, want_pre, rtol=RTOL, atol=ATOL_LOG)


@pytest.mark.parametrize("k", [1, 2])
def test_tiles_and_rows_of_the_smallest_k(k, L, ctx):
    """The row flush (count_bins.hpp: flush_row) at k = 1 — two packed words, fewer than the four a lane step reads — and
    k = 2, in its zero-on-the-way-out arm (sequences) and its tile arm (ordinary stores), which only a sequence of more
    than 8 192 windows reaches at these k: one window, 40 bases, exactly one tile, two tiles of which the second holds one
    window (once with an N next to the boundary), a homopolymer of two tiles.  Raw counts and per-kb float32 bit for bit
    against the C oracle, Log2.pre within the bar of this file."""
    from oracle import c_oracle as co
    rng = np.random.default_rng(200 + k)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    arrs = [letters[rng.integers(0, 4, size=n)].copy() for n in (k, 40, 8192 + k - 1, 8193 + k - 1, 8193 + k - 1)]
    arrs[-1][8190] = ord("N")
    arrs.append(np.full(9000, ord("G"), np.uint8))
    seqs = [a.tobytes().decode() for a in arrs]
    lens = [len(s) for s in seqs]
    blob, offsets = co.seqs_to_blob(seqs)
    n_ref = co.count_u32(blob, offsets, k)
    assert [int(r.sum()) for r in n_ref] == [1, 41 - k, 8192, 8193, 8193 - k, 9001 - k]  # the N voids the k k-mers over it
    packed = ctx.pack(seqs, "AGTC")
    assert np.array_equal(L.count_u32(ctx, packed, k).to_numpy(), n_ref)
    want = co.per_kb_f32(n_ref, lens, k)
    assert_bits(L.count_per_kb(ctx, packed, k).to_numpy(), want, "per-kb of one and two tiles, k=%d" % k)
    got_pre = L.count_per_kb(ctx, packed, k, log2_pre=True).to_numpy()
    assert np.allclose(got_pre, orc.log2_plus_one(want), rtol=RTOL, atol=ATOL_LOG)


def test_normalize_bitexact_vs_oracle_odd_shapes(L, ctx):
    rng = np.random.default_rng(3)
    for rows, cols in ((7, 4), (300, 16), (1025, 64), (513, 100), (2500, 1024)):
        x = (rng.binomial(40, 0.05, size=(rows, cols)) * np.float32(1000 / 397)).astype(np.float32)
        x[:, 0] += 1.0  # no zero-variance columns -> no NaN
        z_ref, mean_ref, std_ref = orc.normalize(x, log2="Log2.none")
        dev = ctx.from_numpy(x)
        mean_out, std_out, has_nan = L.normalize(ctx, dev, "Log2.none", 1, None, 1, None)
        assert not has_nan
        assert_bits(mean_out.vector(), mean_ref, "mean %dx%d" % (rows, cols))
        assert_bits(std_out.vector(), std_ref, "std %dx%d" % (rows, cols))
        assert_bits(dev.to_numpy(), z_ref, "z %dx%d" % (rows, cols))
        post_ref, _, _ = orc.normalize(x, log2="Log2.post")
        dev = ctx.from_numpy(x)
        L.normalize(ctx, dev, "Log2.post", 1, None, 1, None)
        assert np.allclose(dev.to_numpy(), post_ref, rtol=RTOL, atol=2e-6)


def test_colsum_chain_carry_equals_single_pass(L, ctx):
    """Splitting the rows over shards and passing the accumulator on (the multi-GPU chain)
    gives the same bits as one pass."""
    x = big_count_matrix(seed=9, n=6000, k_cols=256)
    whole = ctx.zeros(1, 256)
    L.colsum_seq(ctx, ctx.from_numpy(x), whole)
    acc = ctx.zeros(1, 256)
    for lo, hi in ((0, 1), (1, 2049), (2049, 2050), (2050, 6000)):
        L.colsum_seq(ctx, ctx.from_numpy(x[lo:hi]), acc)
    assert_bits(acc.vector(), whole.vector(), "chained colsum")
    assert_bits(whole.vector(), orc.seqsum_f32(x), "colsum vs oracle")


@pytest.mark.parametrize("shape", [(1, 1, 4), (5, 7, 16), (130, 257, 64), (300, 200, 100), (640, 515, 4096)])
def test_pearson_fp32_vs_oracle(shape, L, ctx, monkeypatch):
    monkeypatch.setenv("SEEKR_PRECISION", "fp32")
    m, n, k = shape
    rng = np.random.default_rng(m * 1000 + n)
    a = rng.gamma(2.0, 1.0, size=(m, k)).astype(np.float32)
    b = rng.gamma(2.0, 1.0, size=(n, k)).astype(np.float32)
    if k > 16:
        b[: min(n, m)] = 0.9 * a[: min(n, m)] + 0.1 * b[: min(n, m)]  # some strongly correlated pairs
    from seekr_amd.pearson import pearson
    with np.errstate(all="ignore"):
        got = pearson(a, b)
        ref = orc.pearson(a, b)
        truth = orc.pearson_f64_truth(a, b)
    assert got.dtype == np.float32 and got.shape == (m, n)
    assert np.allclose(got, ref, rtol=RTOL, atol=ATOL_R, equal_nan=True)
    if k > 4:
        assert np.nanmax(np.abs(got - truth)) < 2e-6
    got_raw = pearson(a, b, row_standardize=False)
    assert np.allclose(got_raw, orc.pearson(a, b, row_standardize=False), rtol=RTOL, atol=1e-5)
    a64 = pearson(a.astype(np.float64), b.astype(np.float64))
    assert np.allclose(a64, truth, rtol=1e-11, atol=1e-13, equal_nan=True)


# ------------------------------------------------------------------ full-size properties (config 2)
def test_cfg2_full_size_properties(L, ctx):
    """50 000 x 2 kb, k=6: size-independent properties at BASELINE size + oracle on a prefix."""
    n_seqs, length, k = 50_000, 2000, 6
    codes = orc.synthetic_codes(2, n_seqs, length)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    blob = letters[codes].reshape(-1)
    offsets = np.arange(n_seqs + 1, dtype=np.int64) * length
    packed = L.PackedSeqs.from_buffer(ctx, blob, offsets, "AGTC")
    assert packed.n == n_seqs and packed.total_bases == n_seqs * length
    n = L.count_u32(ctx, packed, k)
    n_host = n.to_numpy()
    assert (n_host.sum(axis=1) == length - k + 1).all()          # every window lands in exactly one bin
    prefix = orc.codes_to_seqs(codes[:300])
    assert np.array_equal(n_host[:300], orc.count_kmers_u32(prefix, k))
    from oracle import c_oracle as co  # C restatement: 12 000 rows spread over the set, bit-exact
    for first in (0, 23_456, 46_000):
        sl = slice(first, first + 4000)
        ref_n = co.count_u32(blob[first * length:(first + 4000) * length], offsets[:4001], k)
        assert np.array_equal(n_host[sl], ref_n)
    x = L.count_per_kb(ctx, packed, k)
    raw_head = x.to_numpy(0, 300)
    assert_bits(raw_head, orc.per_kb_from_counts(n_host[:300], [length] * 300, k), "per-kb prefix")
    # linearity of the integer surface: counts of a concatenated set = stacked counts
    sub = L.PackedSeqs.from_buffer(ctx, blob[1000 * length:1300 * length], offsets[:301], "AGTC")
    assert np.array_equal(L.count_u32(ctx, sub, k).to_numpy(), n_host[1000:1300])
    del n, n_host
    mean_out, std_out, has_nan = L.normalize(ctx, x, "Log2.post", 1, None, 1, None)
    assert not has_nan
    raw = np.empty((n_seqs, 4 ** k), dtype=np.float32)
    L.count_per_kb(ctx, packed, k).to_numpy(out=raw)
    assert_bits(mean_out.vector(), orc.column_mean_f32(raw), "mean 50k x 4096")
    raw -= mean_out.vector()
    assert_bits(std_out.vector(), orc.column_std_f32(raw), "std 50k x 4096")
    del raw
    # Pearson on a 4096-row slab against float64 truth, plus structural properties
    slab = ctx.from_numpy(x.to_numpy(0, 4096))
    r = L.pearson(ctx, slab, slab).to_numpy()
    # NOTE: the diagonal of a SELF-comparison is not the contraction's value — patch_diag_kernel
    # (operand.hip) overwrites r[i, i] with the float32 tree sum of z^2 taken while the operand was filled (inside the bar,
    # closer to 1 than the reference's own chain).  So this assertion is met by the patch; what the contraction itself does
    # on r ~ 1 cells is asserted where no patch reaches: the cross comparison of a matrix with a COPY of itself below, and
    # the near-copy pairs of the regression fixtures (tests/test_gpu_fuzz.py: regress_r4_two_level_rows.npz,
    # regress_sparse_rows.json, test_constructed_worst_case_*).
    assert np.allclose(np.diag(r), 1.0, atol=2e-6)
    twin = ctx.from_numpy(x.to_numpy(0, 4096))  # the same rows as another matrix: PLAIN mode, nothing patched
    r_twin = L.pearson(ctx, slab, twin).to_numpy()
    assert np.abs(np.diag(r_twin) - 1.0).max() <= 2e-6 + 1e-5  # the unpatched r = 1 cells: within the bar
    assert np.abs(np.diag(r_twin) - 1.0).max() > 0              # ... and really the contraction's own sums, not the patch
    assert np.array_equal(r, r.T)  # same products, same k order: exactly symmetric
    xs = slab.to_numpy()
    truth = orc.pearson_f64_truth(xs[:512], xs[:700])
    assert np.max(np.abs(r[:512, :700] - truth)) < 2e-6
    assert np.allclose(r[:512, :700], orc.pearson(xs[:512], xs[:700]), rtol=RTOL, atol=ATOL_R)


# ------------------------------------------------------------------ fused operand preparation
@pytest.mark.parametrize("cols", [16, 100, 1024, 4096, 16384])
def test_operand_fill_equals_separate_kernels(cols, L, ctx):
    """skr_operand_fill (normalisation tail + row standardisation + operand layout in one pass)
    must give the normalised counts of skr_apply bit for bit and the r of the unfused path."""
    rng = np.random.default_rng(cols)
    x = (rng.binomial(30, 0.1, size=(257, cols)) * np.float32(1000 / 1995)).astype(np.float32)
    x[:, 0] += 0.25
    _, mean, std = orc.normalize(x, log2="Log2.none")
    dmean, dstd = ctx.from_numpy(mean), ctx.from_numpy(std)
    for post in (False, True):
        shift = 0.0
        if post:
            shift = float(np.abs(L.min_nan(ctx, ctx.from_numpy(x), dmean, dstd)[0]))
        ref_y = ctx.from_numpy(x)
        L.apply(ctx, ref_y, center=dmean, scale=dstd, post=post, shift=shift)
        for prec in ("fp32", "bf16x3", "f16x3"):
            y = ctx.from_numpy(x)
            op, has_nan = L.operand_fill(ctx, y, precision=L.PRECISIONS[prec], center=dmean, scale=dstd, post=post,
                                         shift=shift, y=y, row_standardize=True, want_nan=True)
            assert not has_nan
            assert_bits(y.to_numpy(), ref_y.to_numpy(), "fused counts cols=%d post=%s" % (cols, post))
            r = ctx.empty(257, 257)
            L.pearson_gemm_op(ctx, op, op, r, symmetric=True)
            want = L.pearson(ctx, ref_y, ref_y, precision=L.PRECISIONS[prec]).to_numpy()
            assert np.array_equal(r.to_numpy(), want)
            # the same operand when the caller does not ask for the normalised counts (y = NULL: own kernel instances)
            op2, _ = L.operand_fill(ctx, ctx.from_numpy(x), precision=L.PRECISIONS[prec], center=dmean, scale=dstd,
                                    post=post, shift=shift, y=None, row_standardize=True)
            r2 = ctx.empty(257, 257)
            L.pearson_gemm_op(ctx, op2, op2, r2, symmetric=True)
            assert np.array_equal(r2.to_numpy(), want)
            assert np.allclose(want, orc.pearson(ref_y.to_numpy(), ref_y.to_numpy()), rtol=RTOL, atol=ATOL_R)
    # NaN reporting: a zero-variance column divides 0 by 0
    x[:, 3] = 1.0
    _, mean, std = orc.normalize(x, log2="Log2.none")
    y = ctx.from_numpy(x)
    _, has_nan = L.operand_fill(ctx, y, center=ctx.from_numpy(mean), scale=ctx.from_numpy(std), y=y, want_nan=True)
    assert has_nan and np.isnan(y.to_numpy()[:, 3]).all()


@pytest.mark.parametrize("cols", [1024, 4096])
def test_fill_quotients_are_the_ieee_quotients(cols, L, ctx):
    """The register fill kernels divide by multiplying with a float64 reciprocal (operand.hip: div_by_recip) — claimed to
    be THE correctly rounded float32 quotient for every pair of float32 numbers.  Held against numpy's float32 division
    over the whole exponent range: subnormal, huge, zero, infinite and NaN numerators and divisors, exact quotients,
    quotients next to a rounding boundary (x = q d rounded, q a float plus half an ulp), signed zeros."""
    rng = np.random.default_rng(cols)
    rows = 600

    def wild(shape):
        v = (rng.choice([-1.0, 1.0], shape) * np.exp2(rng.uniform(-149, 127, shape)) * rng.uniform(1, 2, shape))
        v = v.astype(np.float32)
        special = rng.random(shape)
        v[special < 0.01] = 0.0
        v[(special >= 0.01) & (special < 0.015)] = -0.0
        v[(special >= 0.015) & (special < 0.02)] = np.inf
        v[(special >= 0.02) & (special < 0.025)] = -np.inf
        v[(special >= 0.025) & (special < 0.03)] = np.nan
        return v

    s = wild((cols,))
    x = wild((rows, cols))
    with np.errstate(all="ignore"):
        # a third of the rows: moderate magnitudes (the pipeline's range), half of those built next to rounding boundaries
        d = np.where(np.isfinite(s) & (s != 0), s, np.float32(3.0)).astype(np.float64)
        q = rng.uniform(-64, 64, (rows // 3, cols)).astype(np.float32).astype(np.float64)
        q[::2] += np.spacing(q[::2].astype(np.float32)).astype(np.float64) * 0.5   # midpoints between two floats
        x[: rows // 3] = (q * d).astype(np.float32)
        want = x / s                                                              # numpy float32 division: IEEE
    zero = np.zeros((1, cols), np.float32)
    y = ctx.empty(rows, cols)
    L.operand_fill(ctx, ctx.from_numpy(x), precision=L.PREC_FP32, center=ctx.from_numpy(zero),
                   scale=ctx.from_numpy(s.reshape(1, -1)), y=y, row_standardize=False)
    got = y.to_numpy()
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])
    assert nan.mean() > 0.005 and (np.abs(want[~nan]) < 1.2e-38).mean() > 0.05   # NaNs and subnormal / zero quotients occurred


@pytest.mark.parametrize("cols", [256, 4096, 16384, 8200, 9999, 16807, 40004, 65536])
def test_split_halves_against_a_numpy_restatement(cols, L, ctx):
    """The stored fp16 halves, bit for bit: hi = z x scale rounded DOWN or UP by the hash of the column (operand.hip:
    split_hi_f16 — one conversion and a step, not the device library's directed conversions), lo = fp16(z x scale - hi).
    Restated with numpy's float16 conversion and nextafter; the widths take every place the fill kernels split a row:
    wave-private LDS rows (256), one row per wave in registers (4 096), four waves per row
    (16 384), the row in the registers of sixteen waves with 4 pieces a thread (8 200; 9 999: ragged last piece) and with
    16 (65 536), a workgroup per row with the row in the LDS (16 807, ragged) and re-read from global memory by 1 024
    threads (40 004).  The register-resident kernels split through split_cells, the wave-per-row and the workgroup-per-row
    kernel write their pass 3 out.  The columns that pad the last 32-column tile hold +0 in both halves."""
    rng = np.random.default_rng(cols)
    rows = 64
    scale = np.float32(2.0 ** np.floor(np.log2(32768.0 / np.sqrt(cols))))
    x = (rng.standard_normal((rows, cols)) * rng.choice([1e-9, 1e-6, 1e-3, 0.3, 3.0], (rows, 1))).astype(np.float32)
    x[:, ::7] = np.float32(0.75)                      # a repeated value: both directions must occur for it
    x[3, :5] = [0.0, -0.0, 6e-8 / scale, -6e-8 / scale, 1.0 / 3.0]   # zeros, half the smallest fp16 subnormal, a repeating fraction
    op, _ = L.operand_fill(ctx, ctx.from_numpy(x), precision=L.PREC_F16X3, row_standardize=False)
    assert op.kind == 2
    kt = (cols + 31) // 32
    got = op.as_matrix().to_numpy().view(np.uint16).reshape(rows, kt, 2, 32)
    hi, lo, up = f16_halves(x, scale)  # the numpy restatement (tests/exact_sum_cases.py, shared with the exact-sum tests)
    pad = np.zeros((rows, kt * 32 - cols), np.uint16)  # +0
    want_hi = np.concatenate([hi.view(np.uint16), pad], axis=1).reshape(rows, kt, 32)
    want_lo = np.concatenate([lo.view(np.uint16), pad], axis=1).reshape(rows, kt, 32)
    # signed zeros: RD(+0) = +0, RU(-0) = -0 and an exact value keeps its sign — numpy's nextafter path never runs there
    assert np.array_equal(got[:, :, 0, :], want_hi), np.argwhere(got[:, :, 0, :] != want_hi)[:5]
    assert np.array_equal(got[:, :, 1, :], want_lo), np.argwhere(got[:, :, 1, :] != want_lo)[:5]
    assert up.mean() > 0.4 and (~up).mean() > 0.4


# ------------------------------------------------------------------ k = 7 (config 5 geometry)
def test_k7_pipeline_16384_columns(L, ctx):
    """k=7: 64 KiB LDS histogram per sequence, 16 384 columns through normalisation, the operand
    fill (one wave per workgroup at this width) and every contraction mode."""
    from seekr_amd.pearson import pearson
    seqs = orc.codes_to_seqs(orc.synthetic_codes(5, 300, 5000)) + ["ACGTN" * 900, "G" * 4000]
    c = run(seqs, k=7, log2="Log2.none", mean=True, std=False)
    raw = orc.raw_counts(seqs, 7)
    ref, mean, _ = orc.normalize(raw, mean=True, std=False, log2="Log2.none")
    assert c.counts.shape == (302, 16384)
    assert_bits(c.mean, mean, "k=7 mean")
    assert_bits(c.counts, ref, "k=7 centred counts")
    want = orc.pearson(ref, ref)
    for prec in ("fp32", "bf16x3", "f16x3"):
        d = ctx.from_numpy(ref)
        got = L.pearson(ctx, d, d, precision=L.PRECISIONS[prec]).to_numpy()
        assert np.allclose(got, want, rtol=RTOL, atol=ATOL_R), (prec, np.abs(got - want).max())
    assert np.allclose(pearson(ref, ref[:100]), want[:, :100], rtol=RTOL, atol=ATOL_R)
    with pytest.raises(NotImplementedError):
        run(seqs[:3], k=13, mean=False, std=False, log2="Log2.none")
    # 5 letters: no 2-bit packing, the general counting kernel serves it (test_g7_alphabets_other_than_four_letters)
    assert run(seqs[:3], k=3, mean=False, std=False, log2="Log2.none", alphabet="ACGTN").counts.shape == (3, 125)


@pytest.mark.parametrize("k", [8, 9])
def test_k8_and_up_global_histogram(k, L, ctx):
    """k >= 8: 4^k bins no longer fit the LDS, the histogram lives in the output row (L2 atomics) and is
    converted in place; rows of 65 536+ columns take the wide operand fill.  Same bars as every other k."""
    from seekr_amd.pearson import pearson
    seqs = orc.codes_to_seqs(orc.synthetic_codes(k, 60, 3000)) + ["ACGTN" * 700, "G" * 2500, "ACGT" * 3, "AC"]
    n = L.count_u32(ctx, ctx.pack(seqs), k).to_numpy()
    assert np.array_equal(n, orc.count_kmers_u32(seqs, k))
    raw = orc.raw_counts(seqs, k)
    assert_bits(run(seqs, k=k, mean=False, std=False, log2="Log2.none").counts, raw, "k=%d raw" % k)
    c = run(seqs, k=k, log2="Log2.post", mean=True, std=True)
    with np.errstate(all="ignore"):
        ref, mean, std = orc.normalize(raw, log2="Log2.post")
    assert_bits(c.mean, mean, "mean")
    assert_bits(c.std, std, "std")
    assert np.allclose(c.counts, ref, rtol=RTOL, atol=2e-6, equal_nan=True)
    # Pearson on a NaN-free version (Log2.none, centred only): wide rows through every contraction
    ref2, _, _ = orc.normalize(raw, mean=True, std=False, log2="Log2.none")
    want = orc.pearson(ref2, ref2)
    for prec in ("fp32", "f16x3", "bf16x3"):
        d = ctx.from_numpy(ref2)
        got = L.pearson(ctx, d, d, precision=L.PRECISIONS[prec]).to_numpy()
        assert np.allclose(got, want, rtol=RTOL, atol=ATOL_R, equal_nan=True), (prec, np.nanmax(np.abs(got - want)))
    assert np.allclose(pearson(ref2, ref2[:20]), want[:, :20], rtol=RTOL, atol=ATOL_R, equal_nan=True)


# ------------------------------------------------------------------ RCCL plumbing on one rank
def test_rccl_single_rank_plumbing(L):
    """A 1-rank communicator exercises librccl loading, init, the ticketed send/recv to self on
    the communication stream, the compute-stream wait and the host all-reduce (the N>1 schedule
    itself is covered by the gloo tests; 8-GPU runs are the driver's)."""
    ctx = L.Context(0)
    L.comm_init(ctx, 1, 0, L.comm_unique_id())
    try:
        assert L.comm_allreduce(ctx, [3.5, -1.0], "max") == [3.5, -1.0]
        assert L.comm_allreduce(ctx, [2.0], "sum") == [2.0]
        L.comm_barrier(ctx)
        src = ctx.from_numpy(np.arange(6 * 64, dtype=np.float32).reshape(6, 64))
        dst = ctx.zeros(8, 64)
        t = L.comm_sendrecv(ctx, src, 1, 4, 0, dst, 2, 4, 0)  # rows 1..4 -> rows 2..5 of dst
        L.comm_wait(ctx, t)
        got = dst.to_numpy()
        assert np.array_equal(got[2:6], src.to_numpy()[1:5]) and not got[:2].any() and not got[6:].any()
        from seekr_amd.distributed import (HipEngine, RcclComm, shard_bounds, sharded_normalize_prepare,
                                           sharded_pearson_rowblock)
        x = (np.random.default_rng(0).binomial(50, 0.05, size=(300, 1024)) * np.float32(2.5)).astype(np.float32)
        ref, mref, sref = orc.normalize(x, log2="Log2.post")
        for prec in (L.PREC_FP32, L.PREC_F16X3, L.PREC_BF16X3):
            dev = ctx.from_numpy(x)
            eng, comm = HipEngine(ctx, prec), RcclComm(ctx, 0, 1)
            mean, std, has_nan, z = sharded_normalize_prepare(eng, comm, dev, 300, "Log2.post", True, True)
            assert_bits(mean.vector(), mref, "mean via RcclComm")
            assert_bits(std.vector(), sref, "std via RcclComm")
            assert not has_nan and np.allclose(dev.to_numpy(), ref, rtol=RTOL, atol=2e-6)
            # operand storage round trip through the send/recv path (what a peer GPU would receive)
            buf = eng.empty_operand(320, 1024)
            t = comm.shift(z, 0, buf, 300, 0)
            comm.wait(t)
            r = ctx.empty(300, 300)
            eng.gemm(z, eng.view(buf, 0, 300), r, 0)
            assert np.allclose(r.to_numpy(), orc.pearson(ref, ref), rtol=RTOL, atol=ATOL_R)
            r2 = ctx.empty(300, 300)
            sharded_pearson_rowblock(eng, comm, z, shard_bounds(300, 1), r2, [None, None])
            got2, got1 = r2.to_numpy(), r.to_numpy()   # r2: self block (diagonal from the z^2 tree sum), r: z x received copy
            off_diag = ~np.eye(300, dtype=bool)
            assert np.allclose(got2[off_diag], got1[off_diag], rtol=1e-6, atol=2e-7)
            assert np.allclose(np.diag(got2), 1.0, rtol=0, atol=5e-7) and np.allclose(np.diag(got1), 1.0, rtol=0, atol=1e-5)
            # grouped all-gather (1 rank: only the own-shard copy) and the striped edge list on top of it
            full = eng.empty_operand(300, 1024)
            comm.wait(comm.allgather_rows(z, full, [0, 300]))
            r3 = ctx.empty(300, 300)
            eng.gemm(full, full, r3, 0)
            assert_bits(r3.to_numpy(), r.to_numpy(), "all-gathered operand")
            from seekr_amd import consumers
            from seekr_amd.distributed import sharded_pearson_edges
            e1 = sharded_pearson_edges(eng, comm, z, [0, 300], 0.02, stripe_rows=64)
            e2 = consumers.pearson_edges(z, 0.02, stripe_rows=128)
            assert len(e1[0]) > 100 and all(np.array_equal(a, b) for a, b in zip(e1, e2))
    finally:
        ctx.close()


@pytest.mark.parametrize("prec", ["bf16x3", "f16x3", "fp32"])
@pytest.mark.parametrize("shape", [(700, 800, 4096, 0, 0), (513, 259, 1024, 3, 5), (260, 1030, 4096, 1, 2)])
def test_gemm_mirror_block_and_transpose(prec, shape, L, ctx):
    """skr_pearson_gemm_op_mirror: the direct block equals the plain contraction bit for bit and
    the second matrix receives exactly its transpose (aligned and unaligned placements)."""
    m, n, k, roff, coff = shape
    precision = {"bf16x3": L.PREC_BF16X3, "f16x3": L.PREC_F16X3, "fp32": L.PREC_FP32}[prec]
    rng = np.random.default_rng(m + n)
    xa = rng.standard_normal((m, k)).astype(np.float32)
    xb = rng.standard_normal((n, k)).astype(np.float32)
    a, _ = L.operand_fill(ctx, ctx.from_numpy(xa), precision=precision)
    b, _ = L.operand_fill(ctx, ctx.from_numpy(xb), precision=precision)
    plain = ctx.empty(m, n)
    L.pearson_gemm_op(ctx, a, b, plain)
    r = ctx.from_numpy(np.full((m + roff + 2, n + coff + 3), -7.0, np.float32))
    rt = ctx.from_numpy(np.full((n + coff + 1, m + roff + 6), -7.0, np.float32))
    L.pearson_gemm_op_mirror(ctx, a, b, r, roff, coff, rt, coff, roff)
    want = plain.to_numpy()
    got, got_t = r.to_numpy(), rt.to_numpy()
    assert_bits(got[roff:roff + m, coff:coff + n], want, "direct block")
    assert_bits(got_t[coff:coff + n, roff:roff + m], want.T.copy(), "mirrored block")
    for buf, r0, r1, c0, c1 in ((got, roff, roff + m, coff, coff + n), (got_t, coff, coff + n, roff, roff + m)):
        mask = np.ones(buf.shape, bool)
        mask[r0:r1, c0:c1] = False
        assert (buf[mask] == -7.0).all()  # nothing outside the two blocks is touched
    assert np.allclose(want, orc.pearson(xa, xb), rtol=RTOL, atol=ATOL_R)
    with pytest.raises(ValueError):  # overlapping block and mirror inside one matrix
        sq = ctx.empty(max(m, n) + 8, max(m, n) + 8)
        L.pearson_gemm_op_mirror(ctx, a, b, sq, 0, 0, sq, 0, 0)


@pytest.mark.parametrize("size", [2, 3, 4, 8])
def test_half_ring_on_one_gpu(size, L):
    """The symmetric multi-GPU schedule with all `size` ranks played by one GPU, one after the
    other, over a 1-rank RCCL communicator (send/recv to self stands in for the xGMI shift):
    the assembled blocks equal the single-GPU symmetric r."""
    from seekr_amd.distributed import HipEngine, shard_bounds, sharded_pearson_symmetric
    ctx = L.Context(0)
    L.comm_init(ctx, 1, 0, L.comm_unique_id())
    try:
        n_rows, k = 1801, 4096
        x = (np.random.default_rng(size).binomial(50, 0.05, size=(n_rows, k)) * np.float32(2.5)).astype(np.float32)
        bounds = shard_bounds(n_rows, size)
        eng = HipEngine(ctx, L.PREC_F16X3)
        dev = ctx.from_numpy(x)
        z_all, _ = L.operand_fill(ctx, dev, precision=L.PREC_F16X3)
        single = ctx.empty(n_rows, n_rows)
        L.pearson_gemm_op(ctx, z_all, z_all, single, symmetric=True)
        want = single.to_numpy()
        shards = [z_all.view(bounds[g], bounds[g + 1] - bounds[g]) for g in range(size)]

        class LoopbackComm:
            def __init__(self, rank):
                self.rank, self.size = rank, size

            def shift(self, send, dst, recv, recv_rows, src):
                peer = shards[src]  # what rank `src` would have sent us
                return L.comm_sendrecv(ctx, peer.as_matrix(), 0, peer.rows, 0, recv.as_matrix(), 0, recv_rows, 0)

            def wait(self, ticket):
                L.comm_wait(ctx, ticket)

        full = np.zeros((n_rows, n_rows), np.float32)
        hits = np.zeros((n_rows, n_rows), np.int32)
        max_shard = max(bounds[g + 1] - bounds[g] for g in range(size))
        recv = [eng.empty_operand(max_shard, k) for _ in range(2)]
        for rank in range(size):
            n_g = bounds[rank + 1] - bounds[rank]
            r_row, r_col = ctx.zeros(n_g, n_rows), ctx.zeros(n_rows, n_g)
            blocks = sharded_pearson_symmetric(eng, LoopbackComm(rank), shards[rank], bounds, r_row, r_col, recv)
            hrow, hcol = r_row.to_numpy(), r_col.to_numpy()
            for which, br, bc, nr, nc, gr, gc in blocks:
                buf = hrow if which == "row" else hcol
                full[gr:gr + nr, gc:gc + nc] = buf[br:br + nr, bc:bc + nc]
                hits[gr:gr + nr, gc:gc + nc] += 1
            r_row.free(); r_col.free()
        assert (hits == 1).all()
        assert_bits(full, full.T.copy(), "assembled matrix is exactly symmetric")
        assert np.allclose(full, want, rtol=1e-6, atol=1e-6)  # tile boundaries differ: not bit-equal
        truth = orc.pearson(x, x)
        assert np.allclose(full, truth, rtol=RTOL, atol=ATOL_R)
    finally:
        ctx.close()


def test_default_precision_on_few_valued_rows(L, ctx):
    """Rows with very few distinct values (raw counts of short sequences, 0/1 rows): the operand
    residual of a value repeats in thousands of columns and adds up instead of averaging out.
    The default split-fp16 operands (22 significand bits) stay as close to float64 as numpy's
    own float32 result does; split-bf16 (16 bits) does not, which is why it is not the default."""
    rng = np.random.default_rng(0)
    n, k = 1024, 4096
    sparse = np.zeros((n, k), np.float32)
    for i in range(n):
        nnz = rng.integers(3, 200)
        sparse[i, rng.choice(k, nnz, replace=False)] = rng.integers(1, 4, nnz) * np.float32(1000.0 / rng.integers(50, 900))
    binom = (rng.binomial(50, 0.05, size=(n, k)) * np.float32(2.5)).astype(np.float32)
    two = (rng.random((n, k)) < 0.5).astype(np.float32)
    off = ~np.eye(n, dtype=bool)
    for name, x in (("sparse", sparse), ("binomial", binom), ("two-valued", two)):
        truth = orc.pearson_f64_truth(x, x)
        ref = orc.pearson(x, x)
        ref_err = np.abs(ref.astype(np.float64) - truth)    # the reference's arithmetic
        dev = ctx.from_numpy(x)
        got = {p: L.pearson(ctx, dev, dev, True, L.PRECISIONS[p]).to_numpy() for p in ("f16x3", "bf16x3")}
        err = {p: np.abs(got[p].astype(np.float64) - truth) for p in got}
        # STRICT: the default precision against the reference's own float32 result, cell by cell, no allowance for
        # the reference's error (tools/strict_parity.py prints the whole grid: worst 0.86 of the bar, on sparse rows,
        # where the reference itself is 0.9 of the bar from float64 and the device 0.15-0.3)
        strict = np.abs(got["f16x3"].astype(np.float64) - ref) / (ATOL_R + RTOL * np.abs(ref))
        assert strict.max() <= 1.0, (name, float(strict.max()))
        # off the diagonal: float32-grade, and far inside the absolute part of the bar
        assert err["f16x3"][off].max() < max(1.0e-6, 4 * ref_err[off].max()), (name, err["f16x3"][off].max())
        # on it (r = 1): 4096 near-equal squares added into one float32 accumulator in k order round
        # the same way again and again — numpy's own diagonal is 4-6e-6 from float64 here and a
        # contraction's up to 2e-5 — so the diagonal of a self-comparison is written from the float32
        # tree sum of z^2 taken while the operand is filled (operand.hip: patch_diag_kernel)
        assert err["f16x3"][~off].max() < 2e-6, (name, err["f16x3"][~off].max())
        assert err["bf16x3"][~off].max() < 2e-6, (name, err["bf16x3"][~off].max())
        assert err["f16x3"][off].max() <= err["bf16x3"][off].max(), name


# ------------------------------------------------------------------ split-bf16 MFMA path
@pytest.mark.parametrize("prec", ["bf16x3", "f16x3"])
@pytest.mark.parametrize("shape", [(5, 7, 16), (130, 257, 64), (300, 200, 100), (640, 515, 4096), (1000, 1000, 1024)])
def test_pearson_split_bf16_vs_oracle(prec, shape, L, ctx):
    m, n, k = shape
    rng = np.random.default_rng(m * 7 + n)
    a = rng.gamma(2.0, 1.0, size=(m, k)).astype(np.float32)
    b = rng.gamma(2.0, 1.0, size=(n, k)).astype(np.float32)
    if k > 16:
        b[: min(n, m)] = 0.9 * a[: min(n, m)] + 0.1 * b[: min(n, m)]
    da, db = ctx.from_numpy(a), ctx.from_numpy(b)
    got = L.pearson(ctx, da, db, precision=L.PRECISIONS[prec]).to_numpy()
    ref = orc.pearson(a, b)
    truth = orc.pearson_f64_truth(a, b)
    assert np.allclose(got, ref, rtol=RTOL, atol=ATOL_R), np.abs(got - ref).max()
    err = np.abs(got - truth)
    if k >= 1024:  # the split path proper (bf16 halves below 1 024 columns, fp16 halves below 64: fp32 MFMA kernel)
        assert err.max() < (6e-6 if prec == "bf16x3" else 2.5e-6), err.max()  # error vs float64 truth, on r ~ 1 pairs
    else:
        assert err.max() < 1.5e-6, err.max()
    # self comparison: the mirrored triangle equals the computed one bit for bit
    rs = L.pearson(ctx, da, da, precision=L.PRECISIONS[prec]).to_numpy()
    assert np.array_equal(rs, rs.T)
    assert np.allclose(rs, orc.pearson(a, a), rtol=RTOL, atol=ATOL_R)
    op, _ = L.operand_fill(ctx, da, precision=L.PRECISIONS[prec], row_standardize=True)
    full = ctx.empty(m, m)
    L.pearson_gemm_op(ctx, op, op, full, symmetric=False)
    full = full.to_numpy()
    # computing both triangles gives the upper one bit for bit; the lower differs only in the
    # order the hi*lo and lo*hi cross terms enter the float32 accumulator
    assert np.array_equal(np.triu(full), np.triu(rs))
    assert np.allclose(full, rs, rtol=1e-6, atol=2e-7)


@pytest.mark.parametrize("K", [64, 256])
def test_split_fp16_from_64_columns_up(K, L, ctx):
    """k = 3 and k = 4 profiles (64 / 256 columns) run on the split-fp16 kernel too: its operands carry 22 bits, so the
    error is bounded by ~2^-21 sum|z_i z_j| / K whatever K is — no averaging over columns is needed, unlike bf16 halves,
    which keep the fp32 kernel below 1 024 columns.  Worst case for a split: few-valued rows and near copies (r ~ 1)."""
    rng = np.random.default_rng(K)
    n = 700
    few = rng.choice([0.0, 1.0, 2.0, 7.0], (n, K), p=[0.6, 0.25, 0.1, 0.05]).astype(np.float32)
    few[1::2] = few[0::2]
    for i in range(1, n, 2):
        few[i, rng.integers(0, K, 2)] = rng.integers(0, 8, 2)
    smooth = rng.gamma(2.0, 1.0, size=(n, K)).astype(np.float32)
    onehot = np.zeros((n, K), np.float32)   # homopolymers: the whole row in one column (|z| = sqrt(K - 1) there)
    onehot[np.arange(n), rng.integers(0, 4, n)] = rng.integers(1, 50, n)
    onehot[n // 2:] += (rng.random((n - n // 2, K)) < 0.1) * np.float32(0.25)
    for x in (few, smooth, onehot):
        dev = ctx.from_numpy(x)
        op, _ = L.operand_fill(ctx, dev, precision=L.PREC_F16X3)
        assert op.kind == 2
        op_b, _ = L.operand_fill(ctx, dev, precision=L.PREC_BF16X3)
        assert op_b.kind == 0
        truth = orc.pearson_f64_truth(x, x)
        got = L.pearson(ctx, dev, dev, True, L.PREC_F16X3).to_numpy().astype(np.float64)
        err, bar = np.abs(got - truth), ATOL_R + RTOL * np.abs(truth)
        assert (err / bar).max() < 0.5, (err / bar).max()
        assert np.array_equal(got, got.T)
    tiny, _ = L.operand_fill(ctx, ctx.from_numpy(smooth[:, :16].copy()), precision=L.PREC_F16X3)
    assert tiny.kind == 0   # k <= 2: one padded k tile, nothing to gain


def test_split_fp16_small_values_and_range(L, ctx):
    """fp16 halves are stored times a power of two (a function of K), so tiny values keep float32-grade
    relative precision instead of falling into fp16 subnormals; rows that are not row-standardised and
    too large for the halves end in the float32 layout instead of turning into inf."""
    K = 1024
    ones = ctx.from_numpy(np.ones((16, K), np.float32))
    for val in (1e-6, 3e-5, 1e-4, 0.01):
        a = ctx.from_numpy(np.full((16, K), val, np.float32))
        r = ctx.empty(16, 16)
        L.pearson_gemm(ctx, a, ones, r, precision=L.PREC_F16X3)
        got = float(r.to_numpy()[0, 0])
        # what a dot product needs is absolute precision: < 1e-11 here (3e-8 without the scale) ...
        assert abs(got - val) < 1e-11 + 2e-6 * val, (val, got)
    # values beyond what the scaled fp16 halves can hold (rows that were not standardised): such rows
    # are "dominated" in the sense of row_needs_fp32 long before they overflow, so the operand takes the
    # float32 layout and the result is simply right (the range check behind it is a safety net)
    big = ctx.from_numpy(np.full((16, K), 1000.0, np.float32))
    for prec in (L.PREC_F16X3, L.PREC_BF16X3):
        r = ctx.empty(16, 16)
        L.pearson_gemm(ctx, big, ones, r, precision=prec)
        assert abs(float(r.to_numpy()[0, 0]) / 1000.0 - 1.0) < 1e-6


def test_rows_dominated_by_one_column_take_the_fp32_kernel(L, ctx):
    """Raw counts of homopolymers are one-hot rows: z = sqrt(K-1) in one column, -1/sqrt(K-1) elsewhere.
    With one float32 accumulator per cell the MFMA drops every product below ~2^-24 of the huge one —
    all the other columns, 1/K of r.  The fill detects such rows and the operand falls back to the
    float32 layout (blocked accumulation); ordinary rows keep the split layout."""
    from seekr_amd.pearson import pearson
    rng = np.random.default_rng(0)
    K = 4096
    x = (rng.binomial(30, 0.1, size=(600, K)) * np.float32(0.5)).astype(np.float32)
    op, _ = L.operand_fill(ctx, ctx.from_numpy(x))
    assert op.kind == 2                                    # ordinary rows: split-fp16
    x[10, :] = 0; x[10, 77] = 1000.0                       # two identical one-hot rows and a third elsewhere
    x[20, :] = 0; x[20, 77] = 1000.0
    x[30, :] = 0; x[30, 4000] = 500.0
    op, _ = L.operand_fill(ctx, ctx.from_numpy(x))
    assert op.kind == 0                                    # fell back
    got = pearson(x, x)
    want = orc.pearson_f64_truth(x, x)
    assert abs(got[10, 20] - 1.0) < 1e-6 and abs(got[10, 30] - want[10, 30]) < 2e-6
    assert np.allclose(got, want, rtol=RTOL, atol=ATOL_R)
    assert np.allclose(got, orc.pearson(x, x), rtol=RTOL, atol=ATOL_R)   # strict: against the float32 reference path itself
    # one flagged operand against an ordinary one: both end in the same layout
    y = (rng.binomial(30, 0.1, size=(300, K)) * np.float32(0.5)).astype(np.float32)
    assert np.allclose(pearson(x, y), orc.pearson_f64_truth(x, y), rtol=RTOL, atol=ATOL_R)
    assert np.allclose(pearson(y, x), orc.pearson_f64_truth(y, x), rtol=RTOL, atol=ATOL_R)
    assert np.allclose(pearson(x, y), orc.pearson(x, y), rtol=RTOL, atol=ATOL_R)


def test_pearson_split_bf16_nan_rows(L, ctx):
    m = np.array([[1, 2, 3, 4], [5, 5, 5, 5], [4, 1, 3, 2]], dtype=np.float32)
    ref = orc.pearson(m, m)
    for prec in ("bf16x3", "f16x3"):
        d = ctx.from_numpy(m)
        got = L.pearson(ctx, d, d, precision=L.PRECISIONS[prec]).to_numpy()
        assert np.array_equal(np.isnan(got), np.isnan(ref))
        assert np.allclose(got, ref, rtol=RTOL, atol=ATOL_R, equal_nan=True)


def test_cfg2_slab_split_bf16(L, ctx):
    """8192 normalised 2 kb transcripts (config-2 data): bf16x3 / f16x3 / fp32 against float64 truth."""
    n_seqs, length, k = 8192, 2000, 6
    blob, offsets = __import__("seekr_amd.synthetic", fromlist=["x"]).synthetic_ascii(2, n_seqs, length)
    packed = L.PackedSeqs.from_buffer(ctx, blob, offsets, "AGTC")
    x = L.count_per_kb(ctx, packed, k)
    L.normalize(ctx, x, "Log2.post", 1, None, 1, None)
    xs = x.to_numpy()
    truth = orc.pearson_f64_truth(xs[:1024], xs[:2048])
    ref = orc.pearson(xs[:1024], xs[:2048])
    # bound = worst |r - truth|, reached on the r = 1 diagonal (4096 positive terms chained in one
    # float32 accumulator); off-diagonal errors are ~1e-7
    for prec, bound in (("bf16x3", 6e-6), ("f16x3", 6e-6), ("fp32", 1.2e-6)):
        r = L.pearson(ctx, x, x, precision=L.PRECISIONS[prec]).to_numpy()
        assert np.array_equal(r, r.T)
        blk = r[:1024, :2048]
        assert np.abs(blk - truth).max() < bound, (prec, np.abs(blk - truth).max())
        off = ~np.eye(1024, 2048, dtype=bool)
        assert np.abs(blk - truth)[off].max() < 1.2e-6, (prec, np.abs(blk - truth)[off].max())
        assert np.allclose(blk, ref, rtol=RTOL, atol=ATOL_R), prec
        assert np.allclose(np.diag(r), 1.0, atol=4e-6)  # met by patch_diag_kernel, not by the kernel under test (see the
        # note in test_cfg2_full_size_properties: the unpatched r = 1 cells are asserted there and in the regression fixtures)


def test_cfg3_like_pipeline():
    """SURVEY config 3 stand-in at its FULL size (18 000 length-skewed transcripts, 30.8 Mbases; the real GENCODE file
    cannot be fetched offline): norm vectors -> counts with those vectors -> Pearson through the public API; raw counts
    and vectors bit-exact, normalised counts within 1e-5, Pearson STRICT against the float32 reference path
    (|got - oracle.pearson| <= 2e-6 + 1e-5 |ref|, no slack) — all checked inside the tool."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "tools", "cfg3_pipeline.py"), "--rows", "18000",
                          "--check-prefix", "600"], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and "cfg3 pipeline ok rows=18000" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]


def test_c_program_through_one_call_host_forms(tmp_path):
    """tests/c_abi/host_example.c — plain C, linked against libseekr_hip.so — runs counts + Pearson through
    skr_host_get_counts / skr_host_pearson; results checked against the oracle."""
    import subprocess
    from test_host_cpu import _build_c_example
    exe = _build_c_example(tmp_path)
    seqs = skewed_set(77, 300, 150, 900)
    fa = str(tmp_path / "in.fa")
    write_fasta(fa, seqs, width=70)
    c_path, r_path = str(tmp_path / "c.npy"), str(tmp_path / "r.npy")
    out = subprocess.run([exe, fa, "4", c_path, r_path], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    want, want_mean, want_std = orc.get_counts(seqs, 4, True, True, "Log2.post")
    got = np.load(c_path)
    np.testing.assert_allclose(got, want, rtol=1e-5, atol=2e-6)
    assert "mean[0]=%.9g std[0]=%.9g" % (want_mean[0], want_std[0]) in out.stdout
    r = np.load(r_path)
    truth = orc.pearson_f64_truth(got, got)
    assert np.abs(r - truth).max() < 2e-6 + 1e-5
    assert r.dtype == np.float32 and r.shape == (300, 300)
    # the reference's error surface: a sequence of length k-1 -> SKR_ERR_ZERODIV (-5) -> exit code 6
    write_fasta(fa, ["ACG", "ACGTACGT"])
    out = subprocess.run([exe, fa, "4", c_path, r_path], capture_output=True, text=True, timeout=120)
    assert out.returncode == 6, out.stdout + out.stderr


def test_matrices_beyond_4gib():
    """Byte offsets past 2^32 in every kernel of the path (config 5 shards are 8 GB): tools/big_offsets.py
    counts 72 000 sequences at k = 7 (4.7 GB matrix) and checks counting, statistics, the fused fill and a
    contraction of the last rows against the first against the oracle."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "tools", "big_offsets.py")], capture_output=True, text=True,
                         timeout=600)
    assert out.returncode == 0 and "big offsets ok" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]


def test_g8_file_whose_first_line_is_not_a_header(golden_dir, tmp_path):
    """The native reader refuses such a file; BasicCounter then packs the strings of the Python Reader, which slices
    the entry list exactly as the reference does: same `seqs`, same raw counts, bit for bit."""
    g = json.load(open(os.path.join(golden_dir, "g8_headerless.json")))
    path = str(tmp_path / "h.fa")
    with open(path, "w") as fh:
        fh.write(g["text"])
    c = counter(k=2, mean=False, std=False, log2="Log2.none", infasta=path)
    assert list(c.seqs) == g["counter_seqs"]
    c.get_counts()
    assert np.array_equal(bits(c.counts), np.array(g["raw_k2_bits"], dtype=np.uint32))


@pytest.mark.parametrize("k", [8, 9])
def test_occurrences_float64_row_at_k8_and_up(k):
    """BasicCounter.occurrences on a float64 row for k >= 8 (the float64 flush exists for k <= 7 only):
    the values are rebuilt on the host from the integer counts — n sequential float64 additions of 1000/W."""
    from seekr_amd.kmer_counts import BasicCounter
    rng = np.random.default_rng(k)
    seq = "".join(rng.choice(list("ACGT"), size=3000)) + "A" * 40
    c = BasicCounter(k=k, silent=True)
    row = np.zeros(4 ** k, dtype=np.float64)
    c.occurrences(row, seq)
    n = orc.count_kmers_u32([seq], k)[0]
    want = orc.per_kb_from_counts(n[None, :], [len(seq)], k, dtype=np.float64)[0]
    assert np.array_equal(row, want)
    row32 = np.zeros(4 ** k, dtype=np.float32)
    c.occurrences(row32, seq)
    assert np.array_equal(row32, want.astype(np.float32))


def test_g7_alphabets_other_than_four_letters(golden_dir, tmp_path):
    """Alphabets of 1, 2, 5 and 20 letters and with a repeated letter (the general counting kernel) against the
    reference's output: raw counts and `occurrences` bit-exact, normalised matrices within the bar."""
    from make_golden_g7 import CASES, sequences
    from seekr_amd.kmer_counts import BasicCounter
    g7 = np.load(os.path.join(golden_dir, "g7_alphabets.npz"))
    for name, alphabet, k, letters in CASES:
        seqs = sequences(name, letters)
        for tag, kw in (("raw", dict(mean=False, std=False, log2="Log2.none")),
                        ("pre", dict(mean=True, std=False, log2="Log2.pre")),
                        ("post", dict(mean=True, std=True, log2="Log2.post"))):
            c = BasicCounter(k=k, alphabet=alphabet, silent=True, **kw)
            c.seqs = list(seqs)
            with contextlib.redirect_stdout(io.StringIO()):
                c.get_counts()
            want = g7["%s_%s" % (name, tag)]
            assert c.counts.shape == want.shape and c.counts.dtype == np.float32
            if tag == "raw":
                assert np.array_equal(c.counts.view(np.uint32), want.view(np.uint32)), name
            else:
                assert np.array_equal(np.isnan(c.counts), np.isnan(want)), (name, tag)
                ok = ~np.isnan(want)
                np.testing.assert_allclose(c.counts[ok], want[ok], rtol=1e-5, atol=2e-6, err_msg=name + tag)
        c = BasicCounter(k=k, alphabet=alphabet, silent=True)
        row = c.occurrences(np.full(len(alphabet) ** k, -1.0), seqs[0])
        assert np.array_equal(row, g7[name + "_occ"]), name
    # from a FASTA file (the reader upper-cases) and through save(): labelled CSV with the 25 2-mers of ACGTN
    fa = str(tmp_path / "n.fa")
    write_fasta(fa, sequences("acgtn", "ACGTN"), lower=True)
    out = str(tmp_path / "n.csv")
    c = BasicCounter(fa, out, k=2, alphabet="ACGTN", binary=False, label=True, mean=False, std=False, log2="Log2.none",
                     silent=True)
    c.make_count_file()
    assert np.array_equal(c.counts.view(np.uint32), g7["acgtn_raw"].view(np.uint32))
    header = open(out).readline().strip().split(",")
    assert header[0] == "" and header[1:4] == ["AA", "AC", "AG"] and len(header) == 26
    # len == k-1 raises as in the reference, also on this path
    c = BasicCounter(k=3, alphabet="ACGTN", silent=True, mean=False, std=False)
    c.seqs = ["ACGTA", "AC"]
    with pytest.raises(ZeroDivisionError):
        c.get_counts()



@pytest.mark.parametrize("alphabet,k", [("ACDEFGHIKL", 4), ("ACDEFGHIKLMNPQRSTVWYBZ", 3), ("ACGTNRYKMSWBDH", 4)])
def test_alphabets_whose_width_is_a_multiple_of_8_but_not_of_32(alphabet, k):
    """10^4 = 10 000, 22^3 = 10 648 and 14^4 = 38 416 columns: rows that the operand fill's one-workgroup-per-row kernel
    reads sixteen bytes at a time and that end inside a 32-column tile.  Until round 5 the vector path also read the tile's
    padding — the next row's first cells — into the row's mean and standard deviation (r about 5 bars off, and the
    normalised counts of the next row overwritten when they were kept in place); no test had such a width.  Counts
    bit-exact (raw) / within the bar (normalised) against the oracle (kmer_counts.py:120-151, 217-246), r within the bar of
    the reference AND of float64 (pearson.py:35-41)."""
    from seekr_amd.kmer_counts import BasicCounter
    from seekr_amd.pearson import pearson
    rng = np.random.default_rng(len(alphabet))
    letters = np.array(list(alphabet))
    seqs = ["".join(rng.choice(letters, size=int(n))) for n in rng.integers(4000, 12000, 90)]
    seqs[7] = seqs[6][3:] + seqs[6][:3]  # a near-copy: r close to 1
    want_raw = orc.raw_counts(seqs, k, alphabet)
    for kw in (dict(mean=False, std=False, log2="Log2.none"), dict(mean=True, std=True, log2="Log2.post")):
        c = BasicCounter(k=k, alphabet=alphabet, silent=True, **kw)
        c.seqs = list(seqs)
        with contextlib.redirect_stdout(io.StringIO()):
            c.get_counts()
        with np.errstate(all="ignore"):
            want = orc.normalize(want_raw, mean=kw["mean"], std=kw["std"], log2=kw["log2"])[0]
        if not kw["mean"]:
            assert_bits(c.counts, want, "raw")
        else:
            assert not np.isnan(want).any() and not np.isnan(c.counts).any()
            np.testing.assert_allclose(c.counts, want, rtol=1e-5, atol=2e-6)
        x = c.counts
        got = pearson(x, x).astype(np.float64)
        with np.errstate(all="ignore"):
            ref, truth = orc.pearson(x, x).astype(np.float64), orc.pearson_f64_truth(x, x)
        assert (np.abs(got - ref) <= 2e-6 + 1e-5 * np.abs(ref)).all(), float((np.abs(got - ref) / (2e-6 + 1e-5 * np.abs(ref))).max())
        assert (np.abs(got - truth) <= 2e-6 + 1e-5 * np.abs(truth)).all()
        assert np.array_equal(got, got.T)



def test_g9_wide_rows_of_other_alphabets_against_the_reference(golden_dir):
    """G9 (tests/golden/make_golden_g9.py): the REFERENCE's output for 10 letters at k = 4 (10 000 columns: the width class
    whose fill was wrong until round 5), ACGTN at k = 6 (15 625) and 7 letters at k = 5 (16 807: the LDS histogram above
    16 384 bins, the block fill) — raw counts bit-exact, the mean-centred Log2.post matrix on 64 seeded cells and in its
    sum, r of both matrices within the north_star's bar of the reference's own `pearson` (kmer_counts.py:140-151,201-209;
    pearson.py:32-44)."""
    import sys
    sys.path.insert(0, golden_dir)
    import make_golden_g9 as mk
    from seekr_amd.kmer_counts import BasicCounter
    from seekr_amd.pearson import pearson
    g9 = np.load(os.path.join(golden_dir, "g9_wide_alphabets.npz"))
    for name, alphabet, k in mk.CASES:
        seqs = mk.sequences(name, alphabet)
        for tag, kw in (("raw", dict(mean=False, std=False, log2="Log2.none")), ("post", dict(mean=True, std=False, log2="Log2.post"))):
            c = BasicCounter(k=k, alphabet=alphabet, silent=True, **kw)
            c.seqs = list(seqs)
            with contextlib.redirect_stdout(io.StringIO()):
                c.get_counts()
            if tag == "raw":
                assert np.array_equal(c.counts.view(np.uint32), g9[name + "_raw"].view(np.uint32)), name
            else:
                rows, cols = mk.sampled_cells(name, c.counts.shape)
                np.testing.assert_allclose(c.counts[rows, cols], g9[name + "_post_cells"], rtol=1e-5, atol=2e-6)
                want_sum = float(g9[name + "_post_sum"])
                assert abs(c.counts.astype(np.float64).sum() - want_sum) <= 1e-5 * abs(want_sum)
            want = g9["%s_r_%s" % (name, tag)].astype(np.float64)
            got = pearson(c.counts, c.counts).astype(np.float64)
            assert got.shape == want.shape
            assert (np.abs(got - want) <= 2e-6 + 1e-5 * np.abs(want)).all(), (name, tag, float(np.abs(got - want).max()))

def test_four_wave_geometry_gives_the_same_bits():
    """The 4-wave / 128 x 128 wave-tile arm of the split contraction (libseekr_hip_diag.so only: measured
    13 % slower and not shipped) adds the same products to every accumulator in the same order as the 8-wave kernel: r
    the same bits in SELF, PLAIN, CROSS and thresholding mode, several k chunks, ragged edges (tools/w4_check.py)."""
    import subprocess
    import sys
    from seekr_amd import _lib
    if not os.path.exists(_lib.DIAG_LIB_PATH):
        pytest.skip("libseekr_hip_diag.so is not built (python -m seekr_amd.build --diag)")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "tools", "w4_check.py")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "w4 check ok" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]


def test_lean_epilogue_gives_the_general_loops_bits():
    """Round 6: whole off-diagonal tiles of the split contraction leave through a branch-free epilogue whose store
    instructions cover 4 rows x 256 bytes (v_permlane32_swap / v_permlane16_swap / DPP row moves gather four accumulator
    tiles; later k chunks add the old cells first).  Against the general loop (SEEKR_GEMM_EPILOGUE=0) and for all three
    run lengths: the same bits in SELF, PLAIN, CROSS, row-stripe and thresholding mode, three split precisions, ragged
    edges, targets whose rows are not 16-byte aligned (must decline), 1 / 2 / 4 k chunks (tools/epilogue_check.py)."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "tools", "epilogue_check.py")], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and "epilogue check ok" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]


@pytest.mark.parametrize("cols,shards", [(4096, [700, 0, 513, 1200]), (16384, [300, 301]), (1000, [64, 1, 0, 0, 90, 7, 300, 5]), (48, [3, 9])])
def test_peer_mailbox_chain_links_in_one_process(cols, shards, L, ctx):
    """skr_colsum_seq_chain (the column-sum chain across GPUs through peer mailboxes) with the ranks' mailboxes connected
    inside ONE process (skr_chain_connect_local) and the links issued rank after rank on one stream: plain, centred and
    squared-deviation passes and the first pass's column minima must equal ONE kernel over all rows bit for bit — ragged
    shards, empty shards (chain_forward_kernel), a column count that is not a multiple of 16, k = 7 (1 024 strips)."""
    rng = np.random.default_rng(cols)
    n = sum(shards)
    x = (rng.binomial(1995, 1.0 / 4096, size=(n, cols)) * np.float32(0.5)).astype(np.float32)
    whole = ctx.from_numpy(x)
    bounds = np.concatenate([[0], np.cumsum(shards)])
    parts = [ctx.from_numpy(x[bounds[g]:bounds[g + 1]]) if shards[g] else ctx.empty(0, cols) for g in range(len(shards))]
    P = len(shards)
    chains = [L.Chain(ctx, cols) for _ in range(P)]
    for g, c in enumerate(chains):
        c.connect_local(g, chains)

    def chained(center=None, center2=None, square=False, want_min=False):
        accs = [ctx.zeros(1, cols) for _ in range(P)]
        mins = [ctx.zeros(4, cols) if (want_min and shards[g]) else None for g in range(P)]
        for g in range(P):
            chains[g].colsum(parts[g], accs[g], center, center2, square, colmin=mins[g], defer_result=True)
        for g in range(P - 1):
            chains[g].result(accs[g])
        ctx.sync()
        assert not any(c.timed_out() for c in chains)
        vecs = [a.vector() for a in accs]
        for v in vecs[1:]:
            assert_bits(v, vecs[0], "every rank ends with the same sums")
        return vecs[0], mins

    # pass 1 (+ minima), pass 2 (centred), pass 3 (squared deviations)
    acc = ctx.zeros(1, cols)
    can_min = cols % 16 == 0
    if can_min:
        cm = ctx.zeros(4, cols)
        L.colsum_seq_colmin(ctx, whole, acc, cm)
    else:
        L.colsum_seq(ctx, whole, acc)
    got, mins = chained(want_min=can_min)
    assert_bits(got, acc.vector(), "chained plain sums")
    if can_min:
        want_min = np.fmin.reduce(cm.to_numpy(), axis=0)
        got_min = np.fmin.reduce(np.concatenate([m.to_numpy() for m in mins if m is not None]), axis=0)
        assert_bits(got_min, want_min, "column minima gathered over the links")
    mean = ctx.from_numpy(acc.vector().reshape(1, -1))
    L.vec_finish(ctx, mean, n)
    acc2 = ctx.zeros(1, cols)
    L.colsum_seq(ctx, whole, acc2, mean)
    got2, _ = chained(center=mean)
    assert_bits(got2, acc2.vector(), "chained centred sums")
    mp = ctx.from_numpy(acc2.vector().reshape(1, -1))
    L.vec_finish(ctx, mp, n)
    acc3 = ctx.zeros(1, cols)
    L.colsum_seq(ctx, whole, acc3, mean, mp, True)
    got3, _ = chained(center=mean, center2=mp, square=True)
    assert_bits(got3, acc3.vector(), "chained squared deviations")
    for c in chains:
        c.free()


def test_rows_are_standardised_in_numpys_summation_order(L, ctx):
    """pearson.py:35-38 on rows whose standardisation is ill-conditioned — 4 or 16 near-equal values (k = 1, 2), short
    rows of large nearly constant counts — depends on every rounding of np.mean / np.std, i.e. on numpy's pairwise
    summation order.  The generic fill kernel adds in exactly that order (operand.hip: np_pairwise_sum), so the device
    meets the STRICT bar |got - oracle.pearson| <= 2e-6 + 1e-5 |ref| there too, where a tree sum of the same accuracy
    lands bars away (the reference itself is up to 8 bars from float64 on such rows: tests/strict_tally.py)."""
    from seekr_amd.pearson import pearson
    rng = np.random.default_rng(11)
    worst = 0.0
    for K in (4, 5, 16, 31, 64, 100, 129, 255, 257, 729, 2000, 4100):
        for scale in (1e-3, 3e-2):
            base = rng.uniform(50, 900, size=(1, K)).astype(np.float32)
            x = (base * (1 + scale * rng.standard_normal((40, K)))).astype(np.float32)
            x[7] = x[3]                                # duplicates: r = 1 up to the row sums' rounding
            x[9] = x[3] * np.float32(2.0)
            with np.errstate(all="ignore"):
                want = orc.pearson(x, x)
                truth = orc.pearson_f64_truth(x, x)
            got = pearson(x, x)
            ok = np.isfinite(want)
            assert np.array_equal(np.isfinite(got), ok), K
            ratio = float(np.max(np.abs(got[ok].astype(np.float64) - want[ok]) / (ATOL_R + RTOL * np.abs(want[ok]))))
            ref_off = float(np.max(np.abs(want[ok].astype(np.float64) - truth[ok]) / (ATOL_R + RTOL * np.abs(truth[ok]))))
            worst = max(worst, ratio)
            assert ratio <= 1.0, (K, scale, ratio, ref_off)
    assert worst <= 1.0


# ------------------------------------------------------------------ round 4: new counting paths
def _with_knobs(ctx, env, fn):
    """Run fn() with A/B knobs set (the ctx reads them once: reload before and after)."""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    ctx.reload_knobs()
    try:
        return fn()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        ctx.reload_knobs()


@pytest.mark.parametrize("alphabet,k", [("ACGTN", 6), ("ACGTN", 2), ("ARNDCQEGHILKMFPSTWYV", 3), ("AT", 7), ("AGTA", 5), ("T", 4),
                                        ("ACGTRYN", 4), ("ACDEFGH", 5), ("ACGTRYNK", 5), ("ACGTN", 7), ("ACDEFG", 6)])
def test_any_alphabet_counts_in_the_lds(alphabet, k, L, ctx):
    """Round 4: up to 16 384 columns (round 5: 36 864, and wider rows one range of 36 864 bins per launch) the any-alphabet counter keeps its histogram in the LDS (count_generic_lds_kernel) and
    counts from sequences RESIDENT on the device (skr_aseqs).  Integer counts, float32 / float64 per-kb values and the
    Log2.pre form bit-exact against the oracle (kmer_counts.py:120-122,140-151) — sequences longer than one LDS chunk
    (4 096 characters), shorter than k, empty, with letters outside the alphabet, lower case — and identical to the
    round-1 path (histogram in HBM, SEEKR_COUNT_GENERIC_GLOBAL=1)."""
    rng = np.random.default_rng(len(alphabet) * 100 + k)
    pool = np.array(sorted(set(alphabet + "Nxa")))
    seqs = ["".join(rng.choice(pool, size=int(n))) for n in (0, 1, k - 2 if k > 2 else 3, k, k + 1, 77, 1999, 4095, 4096, 4097,
                                                            4096 + k - 1, 9000, 20011)]
    seqs = [s for s in seqs if len(s) != k - 1] + [alphabet[0] * 5000, (alphabet * 900)[:8200]]
    want_n = orc.count_kmers_u32(seqs, k, alphabet)
    assert np.array_equal(L.count_generic(ctx, seqs, alphabet, k, np.uint32).to_numpy(), want_n)
    want = orc.raw_counts(seqs, k, alphabet)
    assert_bits(L.count_generic(ctx, seqs, alphabet, k, np.float32).to_numpy(), want, "float32")
    got64 = L.count_generic(ctx, seqs, alphabet, k, np.float64).to_numpy()
    assert np.array_equal(got64, orc.per_kb_from_counts(want_n, [len(s) for s in seqs], k, dtype=np.float64))
    # resident handle: several calls on one upload, into a matrix the caller owns
    lengths = np.array([len(s) for s in seqs], dtype=np.int64)
    offsets = np.concatenate([[0], np.cumsum(lengths)])
    a = L.AsciiSeqs(ctx, "".join(seqs).encode("latin-1"), offsets)
    out = ctx.empty(len(seqs), len(alphabet) ** k)
    for _ in range(2):
        L.count_generic_dev(ctx, a, alphabet, k, out=out)
        assert_bits(out.to_numpy(), want, "resident")
    pre = L.count_generic_dev(ctx, a, alphabet, k, log2_pre=True).to_numpy()
    old = _with_knobs(ctx, {"SEEKR_COUNT_GENERIC_GLOBAL": "1"},
                      lambda: (L.count_generic_dev(ctx, a, alphabet, k).to_numpy(), L.count_generic_dev(ctx, a, alphabet, k, log2_pre=True).to_numpy()))
    assert_bits(old[0], want, "round-1 path")
    assert_bits(pre, old[1], "Log2.pre: LDS path == round-1 path")
    a.free()


def test_any_alphabet_rows_without_a_window_after_other_work(L, ctx):
    """Regression (round 4, found by the differential fuzzer 165 cases into a soak): a sequence shorter than k - 1 has no
    window, hence no chunk and — before the fix — no barrier between the 16 lanes that build the per-sequence value
    table and the waves that flush the row; as the FIRST sequence of its workgroup it read the table from whatever the
    LDS held.  Every workgroup here gets exactly one such sequence, right after a launch that leaves the LDS dirty."""
    alphabet, k = "ACGTRYN", 4
    dirty = L.count_generic(ctx, ["ACGTRYN" * 600] * 600, alphabet, k, np.float32, log2_pre=True)
    dirty.free()
    seqs = ["AC", "", "A", "GT", "NN", "ac"] * 40
    for log2_pre in (False, True):
        got = L.count_generic(ctx, seqs, alphabet, k, np.float32, log2_pre=log2_pre).to_numpy()
        assert not got.any(), (log2_pre, float(np.abs(got).max()))
    assert not L.count_generic(ctx, seqs, alphabet, k, np.uint32).to_numpy().any()


def test_split_fp16_contraction_at_65536_columns(L, ctx):
    """Round 4: k = 8 rows (65 536 columns) take the split-fp16 contraction in sixteen 4 096-column chunks instead of the
    fp32 kernel (3.4 x faster); strict against the reference on normalised-count-like and gaussian rows, and within a
    tenth of the bar of what the fp32 kernel gives."""
    rng = np.random.default_rng(8)
    K, rows = 65536, 192
    for name, x in (("gaussian", rng.standard_normal((rows, K)).astype(np.float32)),
                    ("Log2.post of binomial counts", None)):
        if x is None:
            raw = (rng.binomial(7993, 1.0 / K, size=(rows, K)) * (1000.0 / 7993)).astype(np.float32)
            with np.errstate(all="ignore"):
                x = np.ascontiguousarray(orc.normalize(raw, True, True, "Log2.post")[0], dtype=np.float32)
            if not np.isfinite(x).all():
                continue
        with np.errstate(all="ignore"):
            ref = orc.pearson(x, x).astype(np.float64)
        dev = ctx.from_numpy(x)
        op, _ = L.operand_fill(ctx, dev, precision=L.PREC_F16X3, row_standardize=True)
        assert op.kind == 2, name
        r = ctx.empty(rows, rows)
        L.pearson_gemm_op(ctx, op, op, r, symmetric=True)
        got = r.to_numpy().astype(np.float64)
        got32 = L.pearson(ctx, dev, dev, True, L.PREC_FP32).to_numpy().astype(np.float64)
        bar = 2e-6 + 1e-5 * np.abs(ref)
        assert (np.abs(got - ref) / bar).max() <= 0.5, (name, float((np.abs(got - ref) / bar).max()))
        assert (np.abs(got - got32) / bar).max() <= 0.2, name


def test_k8_counts_in_the_lds_like_the_round_1_path(L, ctx):
    """Round 4: k = 8 on the tuned kernel (65 536 sixteen-bit bins = 128 KiB of LDS, one 4-wave workgroup per CU); the
    same bits as the histogram-in-HBM path it replaces, incl. N runs, a homopolymer and a sequence cut into 8 192-window
    tiles."""
    k = 8
    seqs = orc.codes_to_seqs(orc.synthetic_codes(8, 40, 3000)) + ["ACGTN" * 900, "G" * 6000, "ACGT" * 3, "AC", "ACGTAC",
                                                                 "".join(orc.codes_to_seqs(orc.synthetic_codes(9, 1, 30000)))]
    packed = ctx.pack(seqs)
    n_new = L.count_u32(ctx, packed, k).to_numpy()
    x_new = L.count_per_kb(ctx, packed, k).to_numpy()
    n_old, x_old = _with_knobs(ctx, {"SEEKR_COUNT_K8_GLOBAL": "1"},
                               lambda: (L.count_u32(ctx, packed, k).to_numpy(), L.count_per_kb(ctx, packed, k).to_numpy()))
    assert np.array_equal(n_new, n_old) and np.array_equal(n_new, orc.count_kmers_u32(seqs, k))
    assert_bits(x_new, x_old, "k = 8 per-kb")


@pytest.mark.parametrize("k,length", [(6, 2000), (5, 900), (7, 5000), (3, 300)])
def test_counting_kernel_ab_knobs_give_the_same_bits(k, length, L, ctx):
    """The A/B knobs of the counting launch (tools/count_bench.py: SEEKR_COUNT_OCC = fewer one-wave workgroups per CU,
    SEEKR_COUNT_PERSIST = persistent grid or one workgroup per sequence) only move work around."""
    seqs = orc.codes_to_seqs(orc.synthetic_codes(k, 300, length)) + ["A" * (length + 7), "ACGTN" * 50, "AC" * 40]
    packed = ctx.pack(seqs)
    base = L.count_per_kb(ctx, packed, k).to_numpy()
    assert_bits(base, orc.raw_counts(seqs, k), "base")
    for env in ({"SEEKR_COUNT_OCC": "10"}, {"SEEKR_COUNT_OCC": "19"}, {"SEEKR_COUNT_PERSIST": "1"}, {"SEEKR_COUNT_PERSIST": "2"}):
        got = _with_knobs(ctx, env, lambda: L.count_per_kb(ctx, packed, k).to_numpy())
        assert_bits(got, base, str(env))
        pre = _with_knobs(ctx, env, lambda: L.count_per_kb(ctx, packed, k, log2_pre=True).to_numpy())
        assert_bits(pre, L.count_per_kb(ctx, packed, k, log2_pre=True).to_numpy(), "log2 " + str(env))


@pytest.mark.parametrize("K,rows,W", [(4096, 1500, 1995), (16384, 500, 4993)])
def test_two_product_unit_precision_f16f8(K, rows, W, L, ctx):
    """Round 4, opt-in SKR_PREC_F16F8: hi x hi on the fp16 MFMA and both cross terms as ONE block-scaled fp8 MFMA (two
    product-units per k instead of three).  On Log2.post-normalised counts (the pipeline's data) the operand keeps the
    H / X line layout (kind 3) and r is inside the bar against the reference's float32 result AND against float64; raw
    counts (few-valued rows: the fp8 roundings of a repeated value add up) are detected in the fill and served by the
    three-product split, bit for bit what f16x3 gives; every other width degrades the same way."""
    rng = np.random.default_rng(K)
    raw = (rng.binomial(W, 1.0 / K, size=(rows, K)) * (1000.0 / W)).astype(np.float32)
    with np.errstate(all="ignore"):
        x = np.ascontiguousarray(orc.normalize(raw.copy(), True, True, "Log2.post")[0], dtype=np.float32)
    assert np.isfinite(x).all()
    with np.errstate(all="ignore"):
        ref, truth = orc.pearson(x, x).astype(np.float64), orc.pearson_f64_truth(x, x)
    dev = ctx.from_numpy(x)
    op, _ = L.operand_fill(ctx, dev, precision=L.PREC_F16F8, row_standardize=True)
    assert op.kind == 3
    r = ctx.empty(rows, rows)
    L.pearson_gemm_op(ctx, op, op, r, symmetric=True)
    got = r.to_numpy().astype(np.float64)
    strict = np.abs(got - ref) / (2e-6 + 1e-5 * np.abs(ref))
    vs64 = np.abs(got - truth) / (2e-6 + 1e-5 * np.abs(truth))
    assert strict.max() <= 1.0 and vs64.max() <= 1.0, (float(strict.max()), float(vs64.max()))
    assert np.array_equal(got, got.T)                       # the mirrored triangle
    # a plain (non-symmetric) block of the same operands: same values as the self block off the diagonal tiles
    r2 = ctx.empty(rows, rows)
    L.pearson_gemm_op(ctx, op, op.view(0, rows), r2, symmetric=False)
    g2 = r2.to_numpy().astype(np.float64)
    assert (np.abs(g2 - truth) / (2e-6 + 1e-5 * np.abs(truth))).max() <= 1.0
    # the thresholding epilogue (EDGES mode, K = 16 384: through the scratch block of the earlier k chunks) keeps exactly
    # the cells of this very r
    from seekr_amd import consumers
    cutoff = 0.03 if K == 4096 else 0.015
    fe = consumers.FusedEdges(ctx)
    ei, ej, ev = fe.block(op, op.view(0, rows), cutoff, upper_only=True)
    want = np.triu(np.where(r2.to_numpy() < cutoff, np.float32(0), r2.to_numpy()), 1)
    wi, wj = np.nonzero(want)
    assert len(ei) > 50 and np.array_equal(ei, wi.astype(np.uint32)) and np.array_equal(ej, wj.astype(np.uint32))
    assert np.array_equal(ev.view(np.uint32), want[wi, wj].view(np.uint32))
    fe.free()
    # few-valued rows: degraded to the three-product split by the fill's own flag
    draw = ctx.from_numpy(raw)
    op_raw, _ = L.operand_fill(ctx, draw, precision=L.PREC_F16F8, row_standardize=True)
    op_x3, _ = L.operand_fill(ctx, draw, precision=L.PREC_F16X3, row_standardize=True)
    assert op_raw.kind in (2, 0) and op_raw.kind == op_x3.kind
    ra, rb = ctx.empty(rows, rows), ctx.empty(rows, rows)
    L.pearson_gemm_op(ctx, op_raw, op_raw, ra, symmetric=True)
    L.pearson_gemm_op(ctx, op_x3, op_x3, rb, symmetric=True)
    assert np.array_equal(ra.to_numpy().view(np.uint32), rb.to_numpy().view(np.uint32))
    for m in (dev, draw, r, r2, ra, rb, op, op_raw, op_x3):
        m.free()


@pytest.mark.parametrize("K,period", [(4096, 3), (4096, 64), (4096, 513), (4096, 1500), (16384, 64), (16384, 1025)])
def test_f16f8_routes_rows_that_repeat_values_without_equal_neighbours(K, period, L, ctx):
    """Rows of a short period, each a shifted copy of the same sequence of distinct values: no cell equals its neighbour
    (the adjacent-pair flag sees nothing), but the same PAIR of values meets once per period, the fp8 roundings of the
    cross terms add up instead of averaging out (tools/f8_cross_study.py: 2.4 / 1.1 / 0.8 bars at periods 3 / 64 / 513).
    The fill counts the row's distinct values through a hashed bitmap in the LDS and sends such rows back to the
    three-product split: the operand reports kind 2 and r has f16x3's bits."""
    rng = np.random.default_rng(period)
    vals = rng.standard_normal(period).astype(np.float32)
    rows = 260
    idx = (np.arange(K)[None, :] + rng.integers(0, period, (rows, 1))) % period
    x = np.ascontiguousarray(vals[idx])
    assert not (x[:, 1:] == x[:, :-1]).any()
    dev = ctx.from_numpy(x)
    op8, _ = L.operand_fill(ctx, dev, precision=L.PREC_F16F8, row_standardize=True)
    op3, _ = L.operand_fill(ctx, dev, precision=L.PREC_F16X3, row_standardize=True)
    assert op8.kind == 2 and op3.kind == 2
    ra, rb = ctx.empty(rows, rows), ctx.empty(rows, rows)
    L.pearson_gemm_op(ctx, op8, op8, ra, symmetric=True)
    L.pearson_gemm_op(ctx, op3, op3, rb, symmetric=True)
    got = ra.to_numpy()
    assert np.array_equal(got.view(np.uint32), rb.to_numpy().view(np.uint32))
    truth = orc.pearson_f64_truth(x, x)
    assert (np.abs(got - truth) / (2e-6 + 1e-5 * np.abs(truth))).max() <= 1.0
    # mixed: ONE such row among distinct-valued ones is enough (the flag is per operand)
    y = rng.standard_normal((rows, K)).astype(np.float32)
    opy, _ = L.operand_fill(ctx, ctx.from_numpy(y), precision=L.PREC_F16F8, row_standardize=True)
    assert opy.kind == 3
    y[17] = x[0]
    opm, _ = L.operand_fill(ctx, ctx.from_numpy(y), precision=L.PREC_F16F8, row_standardize=True)
    assert opm.kind == 2
    for m in (dev, ra, rb, op8, op3, opy, opm):
        m.free()


@pytest.mark.parametrize("K,levels,jitter,kept", [(4096, 2, 1e-4, False), (4096, 4, 1e-5, False), (4096, 16, 1e-5, False),
                                                  (16384, 2, 1e-4, False), (4096, 4, 1e-2, True), (16384, 16, 1e-3, True)])
def test_f16f8_routes_tightly_clustered_rows(K, levels, jitter, kept, L, ctx):
    """Values on a few levels with a jitter below the fp16 spacing: every value is distinct, no neighbour equals another
    (neither repeat flag fires), yet all cells of a level share hi, its fp8 copy AND the sign of lo — the rounding
    residues have non-zero row means and the cross term of two rows is off by K x mean x mean (tools/f8_cross_study.py:
    up to 7 bars).  The fill keeps the largest row means of the residues and routes the operand back when their products
    bound the error above 0.6 of the bar; levels whose jitter spans many fp16 steps (the pipeline's own data: count levels
    jittered by the column statistics) keep the layout and stay inside the bar."""
    rng = np.random.default_rng(levels)
    centres = (rng.standard_normal(levels) * 2).astype(np.float32)
    rows = 260
    x = np.ascontiguousarray((centres[rng.integers(0, levels, (rows, K))] * (1.0 + jitter * rng.standard_normal((rows, K)))).astype(np.float32))
    dev = ctx.from_numpy(x)
    op8, _ = L.operand_fill(ctx, dev, precision=L.PREC_F16F8, row_standardize=True)
    op3, _ = L.operand_fill(ctx, dev, precision=L.PREC_F16X3, row_standardize=True)
    assert op8.kind == (3 if kept else 2)
    ra, rb = ctx.empty(rows, rows), ctx.empty(rows, rows)
    L.pearson_gemm_op(ctx, op8, op8, ra, symmetric=True)
    L.pearson_gemm_op(ctx, op3, op3, rb, symmetric=True)
    got = ra.to_numpy()
    if not kept:
        assert np.array_equal(got.view(np.uint32), rb.to_numpy().view(np.uint32))
    truth = orc.pearson_f64_truth(x, x)
    assert (np.abs(got - truth) / (2e-6 + 1e-5 * np.abs(truth))).max() <= (0.6 if kept else 1.0)
    for m in (dev, ra, rb, op8, op3):
        m.free()


def test_f16f8_routes_rows_whose_levels_are_aligned(L, ctx, golden_dir):
    """Found by the structured-row class of tests/fuzz_pearson.py under SEEKR_PRECISION=f16f8 (soak, round 4): the same level
    in a column for EVERY row (rows scaled and jittered by 3e-5) — near-copies of each other that meet in the same pairs of
    values in every column: r = 1.0000176, 1.5 bars.  The row means of the residues cancel between the levels; what does not
    is the row's own cross-term error, the fourth statistic of the fill.  12 of the 33 rows of the failing case."""
    x = np.ascontiguousarray(np.load(os.path.join(golden_dir, "regress_r4_f16f8_aligned_levels.npz"))["a"])
    rows = len(x)
    dev = ctx.from_numpy(x)
    op8, _ = L.operand_fill(ctx, dev, precision=L.PREC_F16F8, row_standardize=True)
    assert op8.kind == 2
    r = ctx.empty(rows, rows)
    L.pearson_gemm_op(ctx, op8, op8, r, symmetric=True)
    got = r.to_numpy().astype(np.float64)
    truth = orc.pearson_f64_truth(x, x)
    assert (np.abs(got - truth) / (2e-6 + 1e-5 * np.abs(truth))).max() <= 0.5
    for m in (dev, r, op8):
        m.free()


def test_f16f8_operands_filled_separately_are_checked_as_a_pair(L, ctx, golden_dir, monkeypatch):
    """Found by tests/fuzz_pearson.py under SEEKR_PRECISION=f16f8 (round 4): pearson(a, b) of two DIFFERENT matrices, each on a
    few aligned levels.  Each passes the rule on the row means on its own (bound 0.29 of the bar: a loses little in the fp8
    copy of hi but its lo does not average out, b the other way round); together mean(hi - 128 h8) of b meets mean(lo) of a:
    r = 0.00342 came out 1.4 bars off.  The fill keeps the three maxima with the operand (skr_operand_x8_stats), the
    contraction refuses the pair, and skr_pearson refills both as f16x3."""
    d = np.load(os.path.join(golden_dir, "regress_r4_f16f8_two_operands.npz"))
    a, b = np.ascontiguousarray(d["a"]), np.ascontiguousarray(d["b"])
    oa, _ = L.operand_fill(ctx, ctx.from_numpy(a), precision=L.PREC_F16F8, row_standardize=True)
    ob, _ = L.operand_fill(ctx, ctx.from_numpy(b), precision=L.PREC_F16F8, row_standardize=True)
    assert oa.kind == 3 and ob.kind == 3
    sa, sb = oa.x8_stats, ob.x8_stats
    assert oa.x8_pair_bound()[1] and ob.x8_pair_bound()[1]    # each passes the rule on its own
    assert not oa.x8_pair_bound(ob)[1]                         # the cross product of their means does not
    assert max(sa[0] * sb[1], sb[0] * sa[1]) / 256.0 ** 2 > 0.6 * 2e-6
    r = ctx.empty(len(a), len(b))
    with pytest.raises(NotImplementedError, match="do not go together"):
        L.pearson_gemm_op(ctx, oa, ob, r)
    L.pearson_gemm_op(ctx, oa, oa.view(0, 3), ctx.empty(len(a), 3))   # views of one operand always go together
    from seekr_amd.pearson import pearson
    monkeypatch.setenv("SEEKR_PRECISION", "f16f8")
    got = pearson(a, b).astype(np.float64)
    with np.errstate(all="ignore"):
        ref, truth = orc.pearson(a, b).astype(np.float64), orc.pearson_f64_truth(a, b)
    assert (np.abs(got - ref) <= 2e-6 + 1e-5 * np.abs(ref)).all()
    assert (np.abs(got - truth) <= 0.5 * (2e-6 + 1e-5 * np.abs(truth))).all()
    # a receive buffer that adopted its shard's layout takes the shard's (all-reduced) maxima over
    buf = L.Operand(ctx, len(a), a.shape[1], L.PREC_F16F8).adopt_layout(oa)
    assert buf.x8_stats == sa
    for m in (oa, ob, r, buf):
        m.free()


def test_f16f8_degrades_on_other_widths_and_through_the_api(L, ctx, monkeypatch):
    rng = np.random.default_rng(3)
    for cols in (729, 1024):
        x = rng.standard_normal((300, cols)).astype(np.float32)
        op, _ = L.operand_fill(ctx, ctx.from_numpy(x), precision=L.PREC_F16F8, row_standardize=True)
        assert op.kind == 2                                  # no H / X layout below 4 096 columns: split-fp16
    from seekr_amd.pearson import pearson
    y = rng.standard_normal((400, 4096)).astype(np.float32)
    want = orc.pearson(y, y)
    monkeypatch.setenv("SEEKR_PRECISION", "f16f8")
    got = pearson(y, y)
    assert np.allclose(got, want, rtol=RTOL, atol=ATOL_R)
    got2 = pearson(y, y[:100] * np.float32(3.0) + np.float32(1.0))
    assert np.allclose(got2, want[:, :100], rtol=RTOL, atol=ATOL_R)


# ------------------------------------------------------------------ G11: normalisation methods on any host dtype
def test_g11_normalisation_methods_on_matrices_that_are_not_float32(golden_dir):
    """VERDICT r5 missing #3: center() / standardize() / log2_norm() on a hand-assigned count matrix that is not float32
    (kmer_counts.py:165-192 act on whatever dtype it has).  Golden set G11, made by the reference on float64 / float16 /
    integer / bool matrices of 7 x 5 and 3 000 x 256 with computed and user-supplied vectors of six types: the device
    path (skr_host_colstat / skr_host_apply) leaves the reference's BYTES for mean, std and the centred / scaled matrices
    of every dtype — float64 bit-exact is the bar, float16 and the integer cases come out exact too — log2 outputs
    within |a - b| <= 1e-6 + 1e-5 |b| (one unit of half for float16), and numpy's own exception, worded as numpy words
    it, where the reference gets one (with `mean` / `std` already replaced by the computed vector)."""
    import g11_cases
    from seekr_amd.kmer_counts import BasicCounter
    assert g11_cases.check_all(golden_dir, g11_cases.run_counter(BasicCounter)) == 9 * 2 * 16


def test_get_counts_takes_a_user_vector_by_numpys_broadcasting_rules():
    """kmer_counts.py:169,175 inside get_counts(): a (1, K) mean / std (np.load of a row saved as a matrix) is what numpy
    spreads over the rows — the same counts as the (K,) vector; a vector of the wrong length is refused in numpy's sentence
    with the matrix's real shape, after counting, as in the reference."""
    from seekr_amd.kmer_counts import BasicCounter
    example_seqs = skewed_set(9, 6, 40, 120)
    rng = np.random.default_rng(4)
    mean, std = rng.uniform(1, 50, 16).astype(np.float32), rng.uniform(5, 60, 16)

    def run(m, s):
        c = BasicCounter(k=2, mean=m, std=s, silent=True, log2="Log2.none")
        c.seqs = example_seqs
        c.get_counts()
        return c.counts
    flat = run(mean, std)
    assert np.array_equal(bits(flat), bits(orc.get_counts(example_seqs, 2, mean, std, "Log2.none")[0]))
    assert np.array_equal(bits(run(mean.reshape(1, 16), std.reshape(1, 16))), bits(flat))
    n = len(example_seqs)
    with pytest.raises(ValueError) as err:
        run(mean[:5], False)
    assert str(err.value) == "operands could not be broadcast together with shapes (%d,16) (5,) (%d,16) " % (n, n)
    with pytest.raises(ValueError) as err:
        run(False, std.reshape(1, 1, 16))
    assert str(err.value) == "non-broadcastable output operand with shape (%d,16) doesn't match the broadcast shape (1,%d,16)" % (n, n)


def test_g12_column_major_matrices_through_the_device(golden_dir):
    """Golden set G12 through seekr_amd.BasicCounter: column-major, strided column-major and single-column matrices of
    float32 / float64 / float16 / int32 / uint8 — mean, std, the centred-then-standardised matrix, dtypes, in-place-ness and
    numpy's exception, byte for byte what the reference left (skr_host_colstat_colmajor + the tuned float32 path)."""
    import g12_cases
    from seekr_amd.kmer_counts import BasicCounter
    assert g12_cases.check_all(golden_dir, BasicCounter) == 5 * 2 * 3


@pytest.mark.parametrize("dtype", ["float64", "float16", "int32"])
def test_normalisation_on_other_dtypes_is_in_place_like_the_reference(dtype):
    """`counts -= mean` / `counts /= std` are in-place operations in the reference (kmer_counts.py:169,175): the caller's
    own array holds the result afterwards, also when it is a non-contiguous view; log2_norm adds 1 in place and binds a
    NEW array (:191-192).  Random matrices against the oracle's restatement (which follows numpy's summation order for the
    view's layout: oracle.colsum_any), bit for bit."""
    from seekr_amd.kmer_counts import BasicCounter
    rng = np.random.default_rng(5)
    base = (rng.poisson(1.3, size=(40, 24)) * (0.5 if dtype != "int32" else 1)).astype(dtype)
    for view in (lambda a: a, lambda a: a[:, ::2], lambda a: a.T):
        mine = base.copy()
        target = view(mine)
        c = BasicCounter(k=1, silent=True)
        c.counts = target
        want = view(base.copy())  # the same LAYOUT: numpy adds a column-major float64 matrix column by column, pairwise
        if dtype == "int32":
            vec = np.arange(target.shape[1], dtype=np.int64)
            c.mean = vec
            c.center()
            orc.host_center(want, vec)[1]()
            assert c.counts is target and np.array_equal(target, want)
        else:
            c.center()
            m, op = orc.host_center(want)
            op()
            assert c.counts is target and target.tobytes() == want.tobytes() and c.mean.tobytes() == m.tobytes()
            with contextlib.redirect_stdout(io.StringIO()):
                c.standardize()
            s, op = orc.host_standardize(want)
            with np.errstate(all="ignore"):
                op()
            assert c.counts is target and np.array_equal(target, want, equal_nan=True) and c.std.tobytes() == s.tobytes()
        before = view(base.copy()).copy()
        c2 = BasicCounter(k=1, silent=True)
        held = view(base.copy())
        c2.counts = held
        c2.log2_norm()
        assert c2.counts is not held and np.array_equal(held, before + 1)  # the `+= 1` landed in the caller's array
        with np.errstate(all="ignore"):
            assert np.allclose(c2.counts, np.log2(before + 1), rtol=2e-3 if dtype == "float16" else 1e-12, equal_nan=True)


@pytest.mark.parametrize("total", [4096, 2 << 20])
def test_any_alphabet_counter_with_trailing_empty_sequences_on_an_allocation_boundary(total, L, ctx):
    """the any-alphabet counter's unconditional prefetch of the next sequence's first bytes read bases[total] —
    one past the buffer — for trailing EMPTY sequences (off == total); with `total` a multiple of the allocation granule
    that is a fault.  The address is clamped now (and the buffer has slack): counts of such a set, bit for bit, including
    the reference's rows for the empty sequences (all zero: len < k - 1)."""
    rng = np.random.default_rng(total)
    lens = [total // 4, total // 4, total // 2 - 37, 37, 0, 0, 0]
    assert sum(lens) == total
    seqs = ["".join(rng.choice(list("ACGTN"), size=n, p=[.24, .24, .24, .24, .04])) for n in lens]
    for dtype, want in ((np.uint32, orc.count_kmers_u32(seqs, 3, "ACGTN")), (np.float32, orc.raw_counts(seqs, 3, "ACGTN"))):
        got = L.count_generic(ctx, seqs, "ACGTN", 3, dtype).to_numpy()
        assert got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))
        assert not got[-3:].any()
    resident = L.AsciiSeqs(ctx, "".join(seqs).encode(), np.cumsum([0] + lens))  # the resident form: exactly `total` bytes
    got = L.count_generic_dev(ctx, resident, "ACGTN", 3, np.uint32).to_numpy()
    assert np.array_equal(got, orc.count_kmers_u32(seqs, 3, "ACGTN"))
