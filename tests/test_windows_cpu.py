"""Window enumeration (seekr_amd.windows.window_table) against a brute-force loop, and the expectation the GPU window tests
use (tests/windows_cases.py): the oracle's counts of explicit substrings.  No GPU needed."""
import math
import os

import numpy as np
import pytest

import windows_cases as wc
from oracle import seekr_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def brute_table(lengths, window, slide):
    rows = []
    for i, L in enumerate(lengths):
        for j in range(math.ceil(max(L - window, 0) / slide) + 1):
            start = j * slide
            rows.append((i, start, len(range(L)[start:start + window])))
    return np.asarray(rows, dtype=np.int64).reshape(-1, 3)


def assert_table(lengths, window, slide):
    from seekr_amd.windows import window_table
    got = window_table(lengths, window, slide)
    want = brute_table(lengths, window, slide)
    assert all(g.dtype == np.int64 for g in got)
    assert np.array_equal(np.stack(got, axis=1), want), (window, slide)


def test_window_table_small_grid():
    lengths = list(range(41))
    for window in range(1, 13):
        for slide in range(1, window + 1):
            assert_table(lengths, window, slide)
            assert_table(lengths[::-1], window, slide)


@pytest.mark.parametrize("slide", [100, 999])
def test_window_table_around_a_million(slide):
    lengths = [10 ** 6 + d for d in (-1001, -1000, -999, -100, -1, 0, 1, 98, 99, 100, 101, 997, 998, 999, 1000)]
    assert_table(lengths, 1000, slide)
    from seekr_amd.windows import window_table
    seq_index, start, length = window_table([10 ** 6], 1000, slide)
    assert len(start) == math.ceil((10 ** 6 - 1000) / slide) + 1 and start[-1] + length[-1] == 10 ** 6


def test_window_table_no_sequences():
    from seekr_amd.windows import window_table
    assert [len(a) for a in window_table([], 5, 2)] == [0, 0, 0]


@pytest.mark.parametrize("window,slide", [(0, 1), (5, 0), (5, 6)])
def test_window_table_refuses(window, slide):
    from seekr_amd.windows import window_table
    with pytest.raises(ValueError):
        window_table([10, 20], window, slide)


def test_expected_rows_are_the_oracles_counts_of_explicit_substrings():
    """tests/windows_cases.py cuts substrings by slicing and counts them with the oracle: written out by hand here."""
    seq = "ACGTNACGTTAGC"  # 13 letters
    subs, table = wc.substrings([seq, "AC"], 5, 4)
    assert subs == ["ACGTN", "NACGT", "TTAGC", "AC"]  # starts 0, 4, 8 (8 + 5 >= 13 ends the sequence); a short sequence is one window
    assert table.tolist() == [[0, 0, 5], [0, 4, 5], [0, 8, 5], [1, 0, 2]]
    assert np.array_equal(table, brute_table([13, 2], 5, 4))
    k = 2
    want = orc.raw_counts_py(subs, k)  # the structure-faithful loop of the reference
    assert np.array_equal(wc.expected_per_kb(subs, k).view(np.uint32), want.view(np.uint32))
    assert np.array_equal(wc.expected_u32(subs, k), orc.count_kmers_u32(subs, k))
    assert wc.expected_u32(subs, k)[0].sum() == 3 and wc.expected_u32(subs, k)[3].sum() == 1  # the k-mer over N is skipped
    assert np.array_equal(wc.expected_per_kb(subs, k, log2_pre=True), np.log2(want + np.float32(1)))
    assert wc.has_zero_division(["ACG", "A"], 2) and not wc.has_zero_division(["ACG", ""], 2)
    with pytest.raises(ZeroDivisionError):
        wc.expected_per_kb(["ACG", "A"], 2)


def test_expectation_does_not_come_from_the_package():
    src = open(os.path.join(ROOT, "tests", "windows_cases.py")).read()
    assert "seekr_amd" not in src.replace("seekr_amd.windows", "").split('"""', 2)[2]
    assert "from oracle import seekr_oracle" in src and "from oracle import c_oracle" in src
