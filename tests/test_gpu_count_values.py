"""The float32 per-kb value of every counting kernel (per_kb.hpp: per_kb_value, which six kernels reach through per_kb_out
of count_bins.hpp) at the pairs (count, windows) of tests/golden/count_value_pairs.json — where float32(n * inc) is not the float32 of the reference's
running sum, where only the slack test fires, inside the 16-entry tables — and the launch boundaries of the same file
(tile batches, gridDim.y, the any-alphabet HBM path in several batches), as tools/count_value_sweep.py walks them.  Bit-exact
against the C oracle, Log2.pre within the bar of test_gpu_parity.py.  Needs a real MI355X: run with `-m gpu`."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))


def _run(fn, *args, **kwargs):
    """A case the machine cannot allocate is skipped with the allocation error as the reason, not tried again."""
    import count_value_sweep as s
    try:
        return fn(*args, **kwargs)
    except s.CannotAllocate as e:
        pytest.skip(str(e))


def test_rows_flush_of_one_wave_at_the_control_pairs():
    import count_value_sweep as s
    assert s.ROWS1_KS == (1, 3, 6) and len(s.pairs("control")) == 60
    assert (s.RTOL, s.ATOL_LOG) == (1e-5, 1e-6)
    bad = s.sweep_rows1(seed=1)
    assert bad == [], bad


def test_rows_flush_of_four_waves_at_the_control_pairs():
    import count_value_sweep as s
    assert s.ROWS4_KS == (7, 8)
    bad = s.sweep_rows4(seed=1)
    assert bad == [], bad


@pytest.mark.parametrize("k", [1, 3, 6, 7, 8])
def test_long_sequences_where_the_replay_decides_the_bits(k):
    """convert_long_kernel.  k = 3 carries the pair of 5 000 000 windows, whose replay is 3.8 10^6 dependent float64 additions
    in one lane (its time is in profiles/count_value_sweep_gpu.log)."""
    import count_value_sweep as s
    assert k in s.LONG_KS and len(s.LONG_KS) == 5 and s.BIG_PAIR_K == 3
    ps = s.long_pairs(k)
    assert len(ps) >= 48 + 12 + 48 + 2 + (k == 3) and ((3826931, s.W_BIG) in [p[:2] for p in ps]) == (k == 3)
    assert {(35604, 35747), (25486, 63551), (16617, 16681), (10, 26214399), (10, 26214401)} <= {p[:2] for p in ps}
    bad = s.sweep_long(seed=1, ks=(k,))
    assert bad == [], bad


def test_rows_in_hbm_at_k9_where_the_replay_decides_the_bits():
    import count_value_sweep as s
    assert s.GLOBAL_K == 9 and 20 <= len(s.global_pairs()) <= 24
    bad = s.sweep_global(seed=1)
    assert bad == [], bad


def test_float64_rows_are_the_running_sum():
    import count_value_sweep as s
    assert s.F64_KS == (3, 7) and len(s.upto(s.pairs("mismatch"), 300_000)) >= 60
    bad = s.sweep_f64(seed=1)
    assert bad == [], bad


@pytest.mark.parametrize("case", [0, 1])
def test_any_alphabet_lds_rows_with_the_wave_wide_table(case):
    import count_value_sweep as s
    assert s.GEN_FAST == (("ACGTN", 2), ("ARNDCQEGHILKMFPSTWYV", 2)) and s.GEN_ONE_LETTER == ("T", 3)
    alphabet, k = s.GEN_FAST[case]
    assert s.generic_geometry(alphabet, k, 50_000) == (1, 1)
    bad = s.sweep_gen_fast(seed=1, cases=(s.GEN_FAST[case],))
    assert bad == [], bad


def test_any_alphabet_lds_rows_without_the_wave_wide_table():
    import count_value_sweep as s
    assert s.GEN_SLOW == ("ACG", 9) and s.generic_geometry(*s.GEN_SLOW, 50_000) == (1, 0)
    bad = s.sweep_gen_slow(seed=1)
    assert bad == [], bad


def test_any_alphabet_lds_rows_in_three_bin_ranges():
    import count_value_sweep as s
    assert s.GEN_RANGES == ("ACGTN", 7) and s.generic_geometry(*s.GEN_RANGES, 50_000) == (3, 0)
    bad = s.sweep_gen_ranges(seed=1)
    assert bad == [], bad


def test_any_alphabet_hbm_conversion_where_the_replay_decides_the_bits():
    import count_value_sweep as s
    assert s.GEN_HBM == ("ACGTN", 2)
    bad = s.sweep_gen_hbm(seed=1)
    assert bad == [], bad


def test_tile_batches_split_and_a_sequence_larger_than_a_batch():
    import count_value_sweep as s
    assert s.SPLIT_K == 8 and s.batch_tiles(8) == 8192 and s.SPLIT_TILES == (4900, 0, 2, 4900, 8300)
    assert s.batches_of(s.split_lengths(), 8) == [[0, 2], [3], [4]]
    bad = _run(s.sweep_split, seed=1)
    assert bad == [], bad


def test_more_long_sequences_than_grid_rows():
    import count_value_sweep as s
    assert s.GRIDY_K == 1 and s.GRIDY_LONG == 65540 and s.GRIDY_SHORT_AT == (0, 65534, 65535, 65536)
    assert [len(b) for b in s.batches_of(s.gridy_lengths(), 1)] == [65535, 5]
    bad = _run(s.sweep_gridy, seed=1)
    assert bad == [], bad


@pytest.mark.parametrize("which", ["knob", "wide"])
def test_any_alphabet_hbm_path_in_several_batches(which):
    import count_value_sweep as s
    assert s.HBM_KNOB == ("ARNDCQEGHILKMFPSTWYV", 4, 430) and s.hbm_batch(*s.HBM_KNOB) == 419
    assert s.HBM_WIDE == ("ACGTN", 11, 3) and s.hbm_batch(*s.HBM_WIDE) == 1
    bad = _run(s.sweep_hbm_batches, seed=1, which=(which,))
    assert bad == [], bad
