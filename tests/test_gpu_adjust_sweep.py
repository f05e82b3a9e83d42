"""adj_pval's kernels (adjust.hip, radix.hpp) and skr_edges' row-offset scan at several hundred sizes, every key byte
pattern and both dtypes (tools/adjust_sweep.py, the thinned size list): the chunk rule's ends and its stepped region, the
scan / accumulation / write-back tiles of 4 096 and their neighbours, last chunks of 1 / 63 / 64 / 65 keys, upper mode,
hommel, radix passes skipped by byte pattern, -0.0 / denormals / inf / NaN payloads at 10^6 tests, the symmetry test in
every tile class, and one 23 171 x 23 171 case whose digit table needs a three-level scan.  Against tests/adj_rule.py by
test_adj_pval_cpu.assert_matches: bit-exact, sidak and holm-sidak within 4 eps.  Needs a real MI355X: run with `-m gpu`."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))


def test_sizes_around_every_boundary_of_the_sort_and_the_scans():
    import adjust_sweep as s
    ns = s.sizes(quick=True, cus=256, seed=1)
    named = s.boundary_sizes(256)
    assert len(ns) > 300 and set(range(1, 201)) <= set(ns)
    for sizes in named.values():
        assert set(sizes) <= set(ns), sizes
    assert {4095, 4096, 4097, 8191, 8192, 8193, 65536, 69632, 4194303, 4194305, 4198401, 2097151, 2097153, 33554431,
            33554433} <= set(ns)
    print("%d sizes, %d of them above %d tests" % (len(ns), sum(n > s.ALL_METHODS_UP_TO for n in ns), s.ALL_METHODS_UP_TO))
    bad = s.sweep_sizes(ns, seed=1, verbose=False)
    assert not bad, bad


def test_upper_mode_sizes():
    import adjust_sweep as s
    assert {2, 3, 33, 91, 92, 2049, 6001} <= set(s.upper_sizes(256))
    bad = s.sweep_upper(seed=1, verbose=False)
    assert not bad, bad


def test_hommel_sizes():
    import adjust_sweep as s
    assert {1, 2, 3, 255, 256, 257, 511, 513, 16384, 16385, 16386} <= set(s.HOMMEL_SIZES) and max(s.HOMMEL_SIZES) >= 100000
    bad = s.sweep_hommel(seed=1, verbose=False)
    assert not bad, bad


def test_key_byte_patterns():
    import numpy as np
    import adjust_sweep as s
    assert len(s.byte_patterns(np.float32)) == 16 and len(s.byte_patterns(np.float64)) == 14
    assert s.BYTE_SIZES == (100003, 2100001)
    bad = s.sweep_bytes(seed=1, verbose=False)
    assert not bad, bad


def test_special_values_at_a_million_tests():
    import adjust_sweep as s
    bad = s.sweep_specials(seed=1, verbose=False)
    assert not bad, bad


def test_symmetry_in_every_tile_class():
    import adjust_sweep as s
    assert set(range(1, 71)) | {95, 96, 97, 127, 128, 129, 1023, 1024, 1025, 4095, 4096, 4097, 10007} == set(s.SYMMETRY_NS)
    bad = s.sweep_symmetry(seed=1, verbose=False)
    assert not bad, bad


def test_edges_row_offset_scan():
    import adjust_sweep as s
    assert s.EDGE_ROWS_PLUS_1 == (4095, 4096, 4097, 8193, 16777215, 16777216, 16777217, 16777300)
    bad = s.sweep_edges_scan(seed=1, verbose=False)
    assert not bad, bad


def test_three_level_digit_table_scan():
    """23 171 x 23 171 float32, fdr_bh: 536 895 241 tests, 65 539 chunks of 8 192 keys, bit-exact against adj_rule."""
    import adjust_sweep as s
    assert s.LARGE_N ** 2 >= 536870913
    bad = s.sweep_large(seed=1, verbose=True)
    assert not bad, bad
