"""The host side of the two-set significance functions, without a GPU: the planted two-set case meets the condition its
GPU parity tests assert, the head argument in its non-symmetric form (every cell of an N1 x N2 matrix a test), the
ordering helper for panelled lists, the argument checks that run before any device call, and the commands' help."""
import os
import subprocess
import sys

import numpy as np
import pytest

import adj_rule
import cross_significant_cases as cc
import significant_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


@pytest.fixture(scope="module")
def two_set_p():
    q, t = cc.two_sets()
    assert q.shape == (37, 256) and t.shape == (263, 256) and q.dtype == t.dtype == np.float32
    r = cc.pearson64(q, t).astype(np.float32)
    return r, {name: cc.tail_p(r, fit) for name, fit in sc.backgrounds().items()}


# ---- the data fixture of the GPU file -------------------------------------------------------------------------------------
def test_planted_two_set_case_meets_the_condition(two_set_p):
    r, ps = two_set_p
    cells = r.size
    assert cells == 9731
    for name, p in ps.items():
        for alpha in cc.ALPHAS:
            head = p <= sc.alpha32(alpha)
            # the cutoff stays above 0 after the guard: every candidate has a clearly positive r
            assert 0.08 < r[head].min() < 0.2, (name, alpha, r[head].min())
            for method in ("bonferroni", "holm", "fdr_by", "fdr_bh"):
                found = len(cc.full_path(p, method, alpha)[0])
                assert cc.condition(found, cells) and 48 <= found <= 160, (name, method, alpha, found)


def test_square_case_has_a_significant_diagonal():
    q2, t2 = cc.square_sets()
    r = cc.pearson64(q2, t2).astype(np.float32)
    assert r.shape == (37, 37) and np.diag(r).min() > 0.99
    p = cc.tail_p(r, sc.backgrounds()["norm"])
    rows, cols, _ = cc.full_path(p, "bonferroni", 0.05)
    assert cc.condition(len(rows), r.size)
    assert set(zip(range(37), range(37))) <= set(zip(rows.tolist(), cols.tolist()))


# ---- the head argument, every cell a test -----------------------------------------------------------------------------------
@pytest.mark.parametrize("method", sc.HEAD_METHODS)
def test_head_of_a_non_symmetric_matrix(method, two_set_p):
    """head_correct on the cells with p <= alpha32, with N1 N2 as the number of tests, against the correction of the
    whole flattened matrix: the same cells come out <= alpha, with the same bits."""
    _, ps = two_set_p
    compared = 0
    for name, p in ps.items():
        flat = p.reshape(-1)
        for alpha in cc.ALPHAS:
            with np.errstate(all="ignore"):
                full = adj_rule.correct(flat, method, alpha).astype(np.float64)
            head = flat <= sc.alpha32(alpha)
            assert not (full[~head] <= alpha).any(), (name, alpha)
            with np.errstate(all="ignore"):
                got = sc.head_correct(flat[head], flat.size, method).astype(np.float64)
            sig = full[head] <= alpha
            assert sig.any() and np.array_equal(got <= alpha, sig), (name, alpha)
            assert np.array_equal(bits(got[sig]), bits(full[head][sig])), (name, alpha)
            compared += int(sig.sum())
    assert compared >= 8 * 48


def test_row_major_order():
    from seekr_amd import significant as sg
    rng = np.random.default_rng(7)
    mask = rng.random((23, 41)) < 0.2
    rows, cols = np.nonzero(mask)
    # the list as panels of 16 columns deliver it: panel after panel, row-major inside each
    panel = np.concatenate([np.nonzero((cols >= c0) & (cols < c0 + 16))[0] for c0 in range(0, 41, 16)])
    assert not np.array_equal(panel, np.arange(len(rows)))
    order = sg.row_major_order(rows[panel].astype(np.uint32), cols[panel].astype(np.uint32))
    assert np.array_equal(rows[panel][order], rows) and np.array_equal(cols[panel][order], cols)
    assert len(sg.row_major_order(np.empty(0, np.uint32), np.empty(0, np.uint32))) == 0


# ---- arguments refused before any device call ---------------------------------------------------------------------------
def test_arguments_are_checked_first():
    from seekr_amd import significant as sg
    from seekr_amd import windows
    q, t = cc.two_sets()
    fit = sc.backgrounds()["norm"]
    calls = [lambda **kw: sg.significant_pairs(q[:4], fit, counts2=t[:5], **kw),
             lambda **kw: sg.pearson_significant(object(), fit, other=object(), **kw),
             lambda **kw: windows.domain_significant("no_query.fa", "no_target.fa", 4, 500, 50, None, None, fit, **kw)]
    for call in calls:
        for method in sc.REFUSED:
            with pytest.raises(NotImplementedError) as err:
                call(method=method)
            assert all(name in str(err.value) for name in sc.REFUSED)
        with pytest.raises(ValueError, match="method not recognized"):
            call(method="nonsense")
        for alpha in (0, 1, -0.1, 1.5, float("nan")):
            with pytest.raises(ValueError, match="alpha"):
                call(alpha=alpha)
        with pytest.raises(IndexError):
            call(bestfit=2)
    for call in calls[:2]:
        for candidates in ("gpu", None, "Host"):
            with pytest.raises(ValueError, match="candidates"):
                call(candidates=candidates)
    with pytest.raises(ValueError, match="candidates"):
        sg.significant_pairs(q[:4], fit, candidates="both")


# ---- the commands ---------------------------------------------------------------------------------------------------------
def help_of(function, name):
    code = ("import sys; sys.argv = [%r, '-h']; from seekr_amd.console_scripts import %s; %s()" % (name, function, function))
    proc = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert proc.returncode == 0, proc.stderr
    return proc.stdout


def test_command_help_and_entry_points():
    text = help_of("console_significant_pairs", "seekr_significant_pairs")
    for word in ("counts2", "row,col,r,p,p_adj", "-bg", "-bi", "--method", "--alpha", "--params"):
        assert word in text, word
    text = help_of("console_domain_significant", "seekr_domain_significant")
    for word in ("query,header,start,end,r,p,p_adj", "query", "target", "mean", "std", "--kmer", "--window", "--slide", "--log2",
                 "-bg", "--distribution", "--params", "--method", "--alpha", "--outfile"):
        assert word in text, word
    with open(os.path.join(ROOT, "setup.py")) as f:
        setup = f.read()
    assert "seekr_domain_significant = seekr_amd.console_scripts:console_domain_significant" in setup


def test_second_count_file_is_optional(monkeypatch):
    from seekr_amd import console_scripts as cs
    seen = []
    monkeypatch.setattr(cs, "_run_significant_pairs", lambda *a: seen.append(a))
    monkeypatch.setattr(cs, "_run_domain_significant", lambda *a: seen.append(a))
    monkeypatch.setattr(sys, "argv", ["seekr_significant_pairs", "a.csv", "-bg", "bg.npy"])
    cs.console_significant_pairs()
    monkeypatch.setattr(sys, "argv", ["seekr_significant_pairs", "a.npy", "b.npy", "-bi", "-d", "norm", "-p", "0", "0.1", "-m", "holm",
                                      "-a", "0.01", "-o", "out.csv"])
    cs.console_significant_pairs()
    assert seen[0] == ("a.csv", "significant_pairs.csv", False, "bg.npy", None, None, "fdr_bh", 0.05, None)
    assert seen[1] == ("a.npy", "out.csv", True, None, "norm", ["0", "0.1"], "holm", 0.01, "b.npy")
    monkeypatch.setattr(sys, "argv", ["seekr_domain_significant", "q.fa", "t.fa", "m.npy", "s.npy", "-k", "4", "-w", "500", "-s", "50",
                                      "-l", "Log2.none", "-bg", "bg.npy", "-a", "0.01"])
    cs.console_domain_significant()
    assert seen[2] == ("q.fa", "t.fa", "m.npy", "s.npy", 4, 500, 50, "Log2.none", "domain_significant.csv", "bg.npy", None, None,
                       "fdr_bh", 0.01)
