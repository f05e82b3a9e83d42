"""domain_hits without a GPU: the property that makes tiles, chunks and launches independent (the merge rule applied to the
pieces of ANY tiling gives the hits of the cells) proved on the model of tests/domain_hits_model.py and on the library's
vectorised windows.merge_pieces; what the GPU cases of tests/test_gpu_domain_hits.py must contain; the argument checks, the
command and the header."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import domain_hits_cases as dc
import domain_hits_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_GAPS = (0, 1, 2, 5, 2000)


def random_case(rng, rows, width):
    """r with equal peaks, +-0 and NaN among the hot values, and ragged sequence boundaries."""
    r = rng.uniform(-1, 0.2, size=(rows, width)).astype(np.float32)
    mask = rng.random((rows, width)) < rng.choice([0.05, 0.3, 0.8])
    r[mask] = rng.choice(np.array([0.0, -0.0, 0.25, 0.5, 0.5, 0.75, 0.75, 1.0], np.float32), size=int(mask.sum()))
    r[rng.random((rows, width)) < 0.03] = np.nan
    cuts = np.sort(rng.choice(np.arange(1, max(width, 2)), size=min(width - 1, int(rng.integers(0, 6))), replace=False)) if width > 1 else []
    seq_index = np.zeros(width, dtype=np.int64)
    for c in cuts:
        seq_index[c:] += 1
    return r, seq_index


def random_tiling(rng, width, single=False):
    if single:
        return list(range(width))
    inner = np.flatnonzero(rng.random(width - 1) < rng.choice([0.02, 0.2, 0.6])) + 1 if width > 1 else []
    return [0] + [int(c) for c in inner]


def library_merge(pieces, seq_index, max_gap):
    from seekr_amd.windows import merge_pieces
    cols = list(zip(*pieces)) if pieces else [[]] * 6
    peak = np.array(cols[4], dtype=np.uint32).view(np.float32)
    out = merge_pieces(cols[0], cols[1], cols[2], cols[3], peak, cols[5], seq_index, max_gap)
    return [tuple(int(v) for v in row) for row in zip(out[0], out[1], out[2], out[3], out[4].view(np.uint32), out[5])]


@pytest.mark.parametrize("max_gap", MAX_GAPS)
def test_merging_the_pieces_of_any_tiling_gives_the_hits_of_the_cells(max_gap):
    rng = np.random.default_rng(1000 + max_gap)
    seen_joins = seen_zero_peaks = 0
    for trial in range(60):
        rows, width = int(rng.integers(1, 4)), int(rng.choice([1, 2, 7, 40, 130]))
        r, seq_index = random_case(rng, rows, width)
        cutoff = np.float32(rng.choice([0.0, -0.0, 0.25, 0.5, -0.5]))
        want = model.hits_of_cells(r, seq_index, cutoff, max_gap)
        tilings = [random_tiling(rng, width), random_tiling(rng, width, single=True),
                   [random_tiling(rng, width) for _ in range(rows)]]  # the same for every row, one column a tile, per row
        for tiling in tilings:
            pieces = model.pieces_of_tiling(r, seq_index, cutoff, max_gap, tiling)
            assert model.merge_pieces(pieces, seq_index, max_gap) == want, (trial, tiling)
            shuffled = [pieces[i] for i in rng.permutation(len(pieces))]
            assert model.merge_pieces(shuffled, seq_index, max_gap) == want
            assert library_merge(shuffled, seq_index, max_gap) == want
            seen_joins += len(pieces) - len(want)
        assert sum(h[3] for h in want) == int((r >= cutoff).sum())  # every hot cell lies in exactly one hit
        seen_zero_peaks += sum(1 for h in want if h[4] in (0, 0x80000000))
    assert seen_joins > 100 and seen_zero_peaks > 0


def test_the_definition_on_a_case_worked_by_hand():
    z, n = np.float32(-0.0), np.float32(np.nan)
    r = np.array([[.5, .1, .5, .7, n, .7, .1, .1, .6, .6],
                  [z, 0., 0., z, -1, -1, 0., -1, -1, -1]], dtype=np.float32)
    seq = np.array([0, 0, 0, 0, 0, 0, 0, 0, 0, 1])
    b = model.bits
    assert model.hits_of_cells(r, seq, 0.5, 0) == [(0, 0, 0, 1, b(.5), 0), (0, 2, 3, 2, b(.7), 3), (0, 5, 5, 1, b(.7), 5),
                                                  (0, 8, 8, 1, b(.6), 8), (0, 9, 9, 1, b(.6), 9)]
    assert model.hits_of_cells(r, seq, 0.5, 1) == [(0, 0, 5, 4, b(.7), 3), (0, 8, 8, 1, b(.6), 8), (0, 9, 9, 1, b(.6), 9)]
    assert model.hits_of_cells(r, seq, 0.5, 2)[0] == (0, 0, 8, 5, b(.7), 3)
    # -0.0 >= +0.0 is hot, and +0.0 is the peak wherever it stands: the earliest +0.0, not the earliest zero
    assert model.hits_of_cells(r[1:], seq, 0.0, 0) == [(0, 0, 3, 4, b(0.), 1), (0, 6, 6, 1, b(0.), 6)]
    assert model.hits_of_cells(r[1:], seq, -0.0, 2) == [(0, 0, 6, 5, b(0.), 1)]
    assert model.hits_of_cells(np.full((1, 4), n, np.float32), seq[:4], -np.inf, 0) == []


def test_kernel_tiling_of_the_model():
    assert model.kernel_tile_starts(1, 5000, 0, 4100) == [[0, 1024, 2048, 3072, 4096]]
    assert model.kernel_tile_starts(3, 4101, 3, 2054) == [[0, 1021, 2045], [0, 1024, 2048], [0, 1023, 2047]]
    assert model.kernel_tile_starts(2, 8, 1, 4) == [[0], [0]]


@pytest.mark.parametrize("name", [c[0] for c in dc.PLANTED])
def test_planted_gpu_cases_contain_every_feature(name):
    """A GPU test that finds no hit across an edge proves nothing about edges: each planted case must show every kind."""
    parent, col_begin, col_end, seq_index, cutoff, max_gap = dc.planted_case(name)
    block = parent[:, col_begin:col_end]
    starts = model.kernel_tile_starts(parent.shape[0], parent.shape[1], col_begin, col_end)
    found = dc.features(block, seq_index, cutoff, max_gap, starts)
    assert all(n >= 1 for n in found.values()), found
    hits = model.hits_of_cells(block, seq_index, cutoff, max_gap)
    pieces = model.pieces_of_tiling(block, seq_index, cutoff, max_gap, starts)
    assert len(pieces) > len(hits) >= 7 * parent.shape[0] - 2
    assert model.merge_pieces(pieces, seq_index, max_gap) == hits
    assert library_merge(pieces, seq_index, max_gap) == hits


def test_pattern_cases_are_what_they_say():
    c = dc.CUTOFF
    none, every = dc.seq_of(2051, "none"), dc.seq_of(2051, "every")
    starts = model.kernel_tile_starts(1, 2051, 0, 2051)
    assert model.hits_of_cells(dc.pattern_block("none", 1, 2051, c), none, c, 5000) == []
    full = dc.pattern_block("all", 1, 2051, c)
    assert len(model.pieces_of_tiling(full, none, c, 0, starts)) == 3 and len(model.hits_of_cells(full, none, c, 0)) == 1
    assert len(model.hits_of_cells(full, every, c, 5)) == 2051  # one hit per sequence
    assert len(model.hits_of_cells(full, dc.seq_of(2051, "at_1024"), c, 5)) == 2
    alt = dc.pattern_block("alternating", 1, 2051, c)
    assert [p[1] // 1024 for p in model.pieces_of_tiling(alt, none, c, 0, starts)].count(0) == 512
    assert len(model.hits_of_cells(alt, none, c, 1)) == 1
    near = dc.pattern_block("neighbours", 1, 70, c)
    assert int((near >= c).sum()) == 40 and int((near == c).sum()) == 20
    zeros = dc.pattern_block("zeros", 1, 90, 0.0)
    assert len(model.hits_of_cells(zeros, none[:90], 0.0, 0)) == 11 and len(model.hits_of_cells(zeros, none[:90], -1e-30, 0)) == 1
    assert np.isnan(dc.pattern_block("nan", 2, 100, c)).sum() == 40
    assert dc.seq_of(5, "at_1025", 1023).tolist() == [0, 0, 1, 1, 1]


# ---- arguments refused before any device call ---------------------------------------------------------------------------
def test_arguments_are_checked_first():
    from seekr_amd.windows import domain_hits
    fit = [("norm", 0.0, (0.0, 0.07))]
    call = lambda **kw: domain_hits("no_query.fa", "no_target.fa", 4, 64, 9, None, None, **kw)  # noqa: E731
    with pytest.raises(ValueError, match="exactly one"):
        call()
    with pytest.raises(ValueError, match="exactly one"):
        call(cutoff=0.2, fitres=fit)
    with pytest.raises(ValueError, match="method"):
        call(cutoff=0.2, method="fdr_bh")
    with pytest.raises(ValueError, match="NaN"):
        call(cutoff=float("nan"))
    for gap in (-1, 0.5):
        with pytest.raises(ValueError, match="max_gap"):
            call(cutoff=0.2, max_gap=gap)
    for least in (0, -3, 1.5):
        with pytest.raises(ValueError, match="min_windows"):
            call(cutoff=0.2, min_windows=least)
    for alpha in (0, 1, float("nan")):
        with pytest.raises(ValueError, match="alpha"):
            call(fitres=fit, alpha=alpha)
    with pytest.raises(ValueError, match="method not recognized"):
        call(fitres=fit, method="nonsense")
    with pytest.raises(NotImplementedError):
        call(fitres=fit, method="hommel")
    with pytest.raises(IndexError):
        call(fitres=fit, bestfit=2)


# ---- the command and the header -------------------------------------------------------------------------------------------
def test_command_help_and_entry_point():
    code = "import sys; sys.argv = ['seekr_domain_hits', '-h']; from seekr_amd.console_scripts import console_domain_hits as f; f()"
    proc = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert proc.returncode == 0, proc.stderr
    for word in ("query,header,start,end,first_window,last_window,n_windows,n_hot,peak_r,peak_start,peak_end", "query", "target",
                 "mean", "std", "--kmer", "--window", "--slide", "--log2", "-bg", "--distribution", "--params", "--method", "--alpha",
                 "--outfile", "-c", "--cutoff", "-g", "--max_gap", "-mw", "--min_windows"):
        assert word in proc.stdout, word
    with open(os.path.join(ROOT, "setup.py")) as f:
        assert "seekr_domain_hits = seekr_amd.console_scripts:console_domain_hits" in f.read()


def test_command_passes_its_arguments_on(monkeypatch):
    from seekr_amd import console_scripts as cs
    seen = []
    monkeypatch.setattr(cs, "_run_domain_hits", lambda *a: seen.append(a))
    monkeypatch.setattr(sys, "argv", ["seekr_domain_hits", "q.fa", "t.fa", "m.npy", "s.npy", "-k", "4", "-w", "64", "-s", "9", "-c", "0.2",
                                      "-g", "2", "-mw", "3"])
    cs.console_domain_hits()
    monkeypatch.setattr(sys, "argv", ["seekr_domain_hits", "q.fa", "t.fa", "m.npy", "s.npy", "-bg", "bg.npy", "-a", "0.01", "-m", "holm",
                                      "-l", "Log2.none", "-o", "out.csv"])
    cs.console_domain_hits()
    assert seen[0] == ("q.fa", "t.fa", "m.npy", "s.npy", 4, 64, 9, "Log2.post", "domain_hits.csv", 0.2, None, None, None, None, 0.05,
                       2, 3)
    assert seen[1] == ("q.fa", "t.fa", "m.npy", "s.npy", 6, 1000, 100, "Log2.none", "out.csv", None, "bg.npy", None, None, "holm",
                       0.01, 0, 1)
    monkeypatch.setattr(sys, "argv", ["seekr_domain_hits", "q.fa", "t.fa", "m.npy", "s.npy", "-c", "0.2", "-m", "holm"])
    with pytest.raises(SystemExit):
        cs.console_domain_hits()


def test_header_binding_and_source_list():
    from seekr_amd import _lib, build
    with open(os.path.join(ROOT, "include", "seekr_hip.h")) as f:
        header = f.read()
    decl = re.search(r"int skr_run_pieces_ge\(([^;]*)\);", header)
    assert decl is not None
    args = [a.strip() for a in decl.group(1).replace("\n", " ").split(",")]
    assert len(args) == 19 == len(_lib.SIGNATURES["skr_run_pieces_ge"][1])
    assert "const skr_mat* seq_of_col" in args and "int64_t max_gap" in args and args[-1] == "int* saw_nan"
    assert "domain_hits.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "domain_hits.hip"))
