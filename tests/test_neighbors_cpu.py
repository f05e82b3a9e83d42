"""The host side of the nearest-neighbour functions, without a GPU: the numpy reference of the top-k merge is independent
of how a row is split, the case list of tests/test_gpu_neighbors.py is what it is meant to be, and bad arguments are
refused before any device call."""
import os
import subprocess
import sys

import numpy as np
import pytest

import neighbors_cases as nc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(nc.bits(a[1]), nc.bits(b[1]))


def rows_of_40():
    rng = np.random.default_rng(40)
    rows = [nc.fill(p, 1, 40, 3)[0] for p in nc.PATTERNS]
    rows.append(np.array([1.0, 1.0, 0.5, np.nan, -0.0, 0.0, np.inf, -np.inf, np.inf, 1.0] * 4, np.float32))
    rows.append(rng.standard_normal(40).astype(np.float32))
    return rows


@pytest.mark.parametrize("k", [1, 3, 10, 39, 40, 41, 64])
def test_reference_is_independent_of_the_split(k):
    """Panel by panel at every split point of a 40-column row == the unsplit row; ties, +-0, +-inf, NaN, k > candidates."""
    for ri, row in enumerate(rows_of_40()):
        for grow, exclude in ((17, True), (0, True), (39, True), (500, True), (17, False)):
            whole = nc.merge_row(row, k, 0, 40, grow, 0, exclude)
            n_cand = 40 - (1 if exclude and grow < 40 else 0)
            assert int((whole[0] != nc.NO_CELL).sum()) == min(k, n_cand)
            for cut in range(0, 41):
                left = nc.merge_row(row, k, 0, cut, grow, 0, exclude)
                both = nc.merge_row(row, k, cut, 40, grow, 0, exclude, running=left)
                assert same(both, whole), (ri, grow, exclude, cut)
                # and right to left: the order of the panels does not matter either
                right = nc.merge_row(row, k, cut, 40, grow, 0, exclude)
                assert same(nc.merge_row(row, k, 0, cut, grow, 0, exclude, running=right), whole), (ri, grow, exclude, cut)


def test_reference_order():
    row = np.array([0.5, np.nan, 2.0, -0.0, 2.0, 0.0, -np.inf, np.inf], np.float32)
    idx, val = nc.merge_row(row, 9, 0, 8, 100, 10, True)
    assert list(idx) == [17, 12, 14, 10, 13, 15, 16, 11, nc.NO_CELL]
    assert list(nc.bits(val)[[3, 4, 5]]) == [0x3F000000, 0x80000000, 0x00000000]  # -0 keeps its bits and ties with +0
    assert nc.bits(val)[8] == nc.PAD_BITS and np.isnan(val[7])
    # the diagonal cell is left out by GLOBAL column
    idx, _ = nc.merge_row(row, 2, 0, 8, 17, 10, True)
    assert list(idx) == [12, 14]
    # a padded slot of a running list is no entry, not a NaN candidate
    run = nc.padded(3)
    assert list(nc.merge_row(row, 3, 0, 2, 100, 10, True, running=run)[0]) == [10, 11, nc.NO_CELL]


def test_saw_nan_reference():
    r = np.zeros((3, 6), np.float32)
    assert not nc.saw_nan(r, 0, 6, 0, 0)
    r[1, 1] = np.nan
    assert not nc.saw_nan(r, 0, 6, 0, 0) and nc.saw_nan(r, 0, 6, 0, 0, exclude_diag=False) and nc.saw_nan(r, 0, 6, 1, 0)
    assert not nc.saw_nan(r, 2, 6, 1, 0)


def test_case_list():
    """Pins what the GPU file runs."""
    from seekr_amd import _lib
    assert (nc.KMAX, nc.CAP, nc.STEP) == (_lib.TOPK_MERGE_KMAX, _lib.TOPK_MERGE_CAP, _lib.TOPK_MERGE_STEP)
    assert nc.KMAX >= 128 and nc.STEP <= nc.CAP
    for w in (1, 3, 4, 5, 63, 64, 65, 255, 256, 257, nc.CAP - 1, nc.CAP, nc.CAP + 1, 2 * nc.CAP + 1, nc.STEP - 1, nc.STEP,
              nc.STEP + 1):
        assert w in nc.WIDTHS
    assert set(nc.PATTERNS) == {"ascending", "descending", "equal", "five_values", "all_nan", "specials"}
    for k in (1, 2, 31, 32, 33, 64, nc.KMAX - 1, nc.KMAX):
        assert k in nc.KS
    cases = nc.kernel_cases()
    assert len(cases) == sum(len(nc.ks_for(w)) for w in nc.WIDTHS) * len(nc.PATTERNS)
    assert any(c["k"] > c["width"] for c in cases) and all(1 <= c["k"] <= nc.KMAX for c in cases)
    assert {a[0] for a in nc.ALIGNMENTS} >= {0, 1, 4}
    assert any((cb + w + right) % 4 for cb, right in nc.ALIGNMENTS for w in nc.ALIGN_WIDTHS)
    assert set(nc.DIAGONALS) == {"inside", "outside", "first", "last", "off"} and nc.MERGE_SPLITS == (2, 3, 7)
    # the patterns are what their names say
    a = nc.fill("ascending", 3, 50, 1)
    assert (np.diff(a, axis=1) > 0).all() and (np.diff(nc.fill("descending", 3, 50, 1), axis=1) < 0).all()
    assert len(np.unique(nc.fill("equal", 1, 50, 1))) == 1 and np.isnan(nc.fill("all_nan", 2, 9, 1)).all()
    five = nc.fill("five_values", 4, 300, 1)
    assert len(np.unique(nc.bits(five))) == 5
    sp = nc.fill("specials", 4, 400, 1)
    assert np.isnan(sp).any() and np.isposinf(sp).any() and np.isneginf(sp).any() and (nc.bits(sp) == 0x80000000).any()
    # diagonal placements, as local columns of row 0
    for kind, want in (("inside", 4 + 5), ("first", 4), ("last", 4 + 9), ("outside", 4 + 15)):
        row0, col0, ex = nc.diagonal_offsets(kind, 4, 10)
        assert ex and row0 - col0 == want
    assert nc.diagonal_offsets("off", 4, 10)[2] is False
    assert nc.split_points(3585, 7, 1) == sorted(set(nc.split_points(3585, 7, 1))) and len(nc.split_points(3585, 7, 1)) == 6
    p = nc.kmer_profiles(12, 3, 5)
    assert p.shape == (12, 64) and p.dtype == np.float32 and np.isfinite(p).all()


def test_k_is_refused_before_any_device_call(monkeypatch):
    from seekr_amd import _lib, neighbors
    monkeypatch.setattr(_lib, "default_context", lambda: pytest.fail("a device call was made"))
    monkeypatch.setattr(_lib, "lib", lambda: pytest.fail("the library was loaded"))
    x = np.zeros((5, 16), np.float32)
    for k in (0, -1, _lib.TOPK_MERGE_KMAX + 1, 2.5):
        with pytest.raises(ValueError):
            neighbors.nearest(x, k=k)
        with pytest.raises(ValueError):
            neighbors.nearest(x, x, k=k)


def test_domain_topk_refuses_before_any_device_call(tmp_path, monkeypatch):
    from seekr_amd import _lib, windows
    monkeypatch.setattr(_lib, "default_context", lambda: pytest.fail("a device call was made"))
    fa = tmp_path / "t.fa"
    fa.write_text(">t\n" + "ACGT" * 50 + "\n")
    vec = np.ones(16, np.float32)
    q = np.zeros((2, 16), np.float32)
    for top in (0, -3, _lib.TOPK_MERGE_KMAX + 1):
        with pytest.raises(ValueError):
            windows.domain_topk(q, str(fa), 2, 20, 5, vec, vec, top=top)
    for bad in (np.zeros((2, 15), np.float32), np.zeros((2, 16), np.float64), np.zeros(16, np.float32)):
        with pytest.raises(ValueError):
            windows.domain_topk(bad, str(fa), 2, 20, 5, vec, vec, top=3)
        with pytest.raises(ValueError):
            windows.domain_pearson(bad, str(fa), 2, 20, 5, vec, vec)


def test_command_help():
    code = "import sys; sys.argv = ['seekr_nearest', '-h']; from seekr_amd.console_scripts import console_nearest; console_nearest()"
    proc = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert proc.returncode == 0, proc.stderr
    assert "--neighbors" in proc.stdout and "counts1" in proc.stdout
    setup = open(os.path.join(ROOT, "setup.py")).read()
    assert "seekr_nearest = seekr_amd.console_scripts:console_nearest" in setup
