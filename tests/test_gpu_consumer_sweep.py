"""The consumers of r (consumers.hip) at the background sizes, distribution parameters, k / width pairs, column windows,
cutoffs and diagonal offsets of tools/consumer_sweep.py: every stride and table length of the empirical search, scipy's
own fits and gamma shapes up to 1e7 for the parametric cdfs, k up to 4 096 with windows and global offsets, more rows
than the grid.  Bit-exact against numpy, the parametric p-values within 2e-6 |p| + 4e-16 of scipy's.  Needs a real
MI355X: run with `-m gpu`."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))


@pytest.mark.parametrize("kind", ["normal", "two decimals", "constant", "inf", "nan", "float64 near cells"])
def test_empirical_pvalues_at_every_stride_and_table_length(kind):
    import consumer_sweep as s
    assert s.BG_SIZES == (1, 2, 3, 255, 256, 257, 4095, 4096, 4097, 8191, 8192, 8193, 12288, 12289, 1000003, 1 << 20,
                          (1 << 20) + 1, (1 << 22) + 1)
    assert kind in s.BG_KINDS and len(s.BG_KINDS) == 6
    bad = s.sweep_empirical(seed=1, kinds=(kind,))
    assert bad == [], bad


def test_parametric_pvalues_at_fitted_and_extreme_parameters():
    import consumer_sweep as s
    cases = s.fixture_cases()
    shapes = {(name, params[0]) for name, params, origin, _, _ in cases if origin == "hand-set" and name in ("gamma", "chi2")}
    for a in (0.05, 1.0, 3e3, 2e4, 1e5, 187114.0, 3e5, 1e6, 1e7):
        assert ("gamma", a) in shapes and ("chi2", 2 * a) in shapes, a
    worst = {}
    bad = s.sweep_parametric(verbose=True, worst=worst)
    assert bad == [], bad
    assert len(worst) == 10


def test_topk_rows_at_every_k_width_and_window():
    import consumer_sweep as s
    assert s.TOPK_KS == (1, 2, 63, 64, 65, 255, 256, 257, 1000, 4096)
    assert s.TOPK_WIDTHS == (1, 2, 255, 256, 257, 513, 5000)
    assert s.TOPK_LOOP_SHAPE == (4200, 40, 3)
    bad = s.sweep_topk(seed=1)
    assert bad == [], bad


def test_threshold_at_extreme_cutoffs_and_diagonal_offsets():
    import consumer_sweep as s
    assert {"NaN", "+inf", "-inf", "just below it", "just above it"} <= set(s.cutoffs(0.5))
    rows, cols = s.THRESHOLD_SHAPE
    offsets = s.diag_offsets(rows, cols)
    assert min(offsets) < -rows and {-1, cols, cols + 7} <= set(offsets)
    bad = s.sweep_threshold(seed=1)
    assert bad == [], bad


def test_edges_at_extreme_cutoffs_and_windows():
    import consumer_sweep as s
    bad = s.sweep_edges(seed=1)
    assert bad == [], bad


def test_triu_values_at_every_offset_and_more_rows_than_the_grid():
    import consumer_sweep as s
    assert s.TRIU_NS == (255, 256, 257, 4099)
    assert all(s.triu_ks(n) == (0, 1, n - 1, n, n + 3) for n in s.TRIU_NS)
    bad = s.sweep_triu(seed=1)
    assert bad == [], bad
