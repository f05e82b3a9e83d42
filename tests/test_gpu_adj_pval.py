"""adj_pval on the MI355X: the device against the reference's golden outputs (tests/golden/adj_pval.*), against the
numpy restatement (tests/adj_rule.py) at sizes the fixtures cannot hold, and the device-only chain
pearson-style matrix -> parametric_pvalues -> adjust_pvalues."""
import contextlib
import io
import os
import subprocess
import sys

import numpy as np
import pytest

import adj_rule
from test_adj_pval_cpu import CASES, CSVS, assert_matches

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _frame(case, v):
    import pandas as pd
    return pd.DataFrame(v, index=case["rows"], columns=case["cols"])


@pytest.mark.parametrize("idx", range(len(CASES)), ids=["%d-%s-%s" % (i, c[0]["name"], c[0]["method"]) for i, c in enumerate(CASES)])
def test_device_matches_reference(idx):
    from seekr_amd.adj_pval import adj_pval
    case, v, want = CASES[idx]
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        res = adj_pval(_frame(case, v), case["method"], case["alpha"])
    assert buf.getvalue().strip() == case["message"]
    assert list(res.index) == case["rows"] and list(res.columns) == case["cols"]
    assert_matches(res.to_numpy(), want, case["method"], v.dtype)


@pytest.mark.parametrize("which", range(3))
def test_cli_writes_reference_bytes(tmp_path, which):
    c = CSVS[which]
    src = tmp_path / "p.csv"
    src.write_text(c["input"])
    out = tmp_path / "out"
    code = ("import sys; sys.argv = ['seekr_adj_pval', %r, %r, '-a', %r, '-o', %r]; "
            "from seekr_amd.console_scripts import console_adj_pval; console_adj_pval()") % (
        str(src), c["method"], str(c["alpha"]), str(out))
    proc = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0, proc.stderr
    assert proc.stdout.strip() == c["message"]
    assert (tmp_path / "out.csv").read_text() == c["output"]


def _device(a):
    from seekr_amd import _lib
    return _lib.default_context().from_numpy(np.ascontiguousarray(a))


@pytest.fixture(scope="module")
def big_tests():
    """2 500 x 4 000 float32 p-values (10^7 tests): ties on a 1e-4 grid, zeros, ones and a few exact duplicates."""
    rng = np.random.default_rng(5)
    v = (rng.integers(0, 10001, size=(2500, 4000)) / 1e4).astype(np.float32)
    v[rng.random(v.shape) < 0.01] = np.float32(0.123456)
    v.reshape(-1)[rng.choice(v.size, 1000, replace=False)] = 0
    return v


@pytest.mark.parametrize("method", [m for m in adj_rule.METHODS if m != "hommel"])  # hommel: 20 000 tests, below
def test_ten_million_tests_against_rule(big_tests, method):
    from seekr_amd import consumers
    d = _device(big_tests)
    got = consumers.adjust_pvalues(d, method, 0.05, symmetric=False).to_numpy()
    want = adj_rule.correct(big_tests.reshape(-1), method, 0.05).reshape(big_tests.shape)
    assert_matches(got, want, method, np.float32)


@pytest.mark.parametrize("method", ["holm", "fdr_bh", "fdr_tsbh"])
def test_nan_behaviour(big_tests, method):
    """One NaN: confined to its cell for holm, everywhere for the running-min methods (np.minimum propagates it)."""
    from seekr_amd import consumers
    v = big_tests[:500].copy()
    v[7, 11] = np.nan
    got = consumers.adjust_pvalues(_device(v), method, 0.05, symmetric=False).to_numpy()
    want = adj_rule.correct(v.reshape(-1), method, 0.05).reshape(v.shape)
    assert np.array_equal(got, want, equal_nan=True)
    assert np.isnan(got).sum() == (1 if method == "holm" else v.size)


@pytest.fixture(scope="module")
def sym20k():
    n = 20000
    rng = np.random.default_rng(11)
    a = rng.random((n, n), dtype=np.float32)
    a = np.triu(a, 1)
    a += a.T
    iu = np.triu_indices(n, 1)
    return a, iu


@pytest.mark.parametrize("method", ["fdr_bh", "holm"])
def test_symmetric_20k(sym20k, method):
    from seekr_amd import consumers
    a, iu = sym20k
    d = _device(a)
    assert consumers.pvals_symmetric(d)
    out = consumers.adjust_pvalues(d, method, 0.05)
    got = out.to_numpy()
    out.free()
    d.free()
    assert np.isnan(got[np.tril_indices(a.shape[0])]).all()
    want = adj_rule.correct(a[iu], method, 0.05)
    assert np.array_equal(got[iu], want)


def test_sidak_symmetric_20k_power_rounded_once(sym20k):
    from seekr_amd import consumers
    a, iu = sym20k
    d = _device(a)
    out = consumers.adjust_pvalues(d, "sidak", 0.05, symmetric=True)
    got = out.to_numpy()[iu]
    out.free()
    d.free()
    s = a[iu]
    n = s.size
    pw = np.power((np.float32(1) - s).astype(np.float64), float(np.float32(n))).astype(np.float32)
    want = (np.float32(1) - pw).astype(np.float32)
    want[want > 1] = 1
    ulps = np.abs(got.astype(np.float32).view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
    assert ulps.max() <= 1


def test_chain_after_parametric_pvalues_equals_dataframe_path():
    import pandas as pd
    from seekr_amd import consumers
    from seekr_amd.adj_pval import adj_pval
    rng = np.random.default_rng(3)
    z = rng.standard_normal((300, 64)).astype(np.float32)
    r = np.corrcoef(z).astype(np.float32)
    r = np.triu(r, 1) + np.triu(r, 1).T + np.eye(300, dtype=np.float32)
    p = consumers.parametric_pvalues(_device(r), "norm", (0.0, 0.1))
    dev = consumers.adjust_pvalues(p, "fdr_by").to_numpy()
    names = ["t%d" % i for i in range(300)]
    with contextlib.redirect_stdout(io.StringIO()):
        df = adj_pval(pd.DataFrame(p.to_numpy(), index=names, columns=names), "fdr_by")
    assert np.array_equal(dev, df.to_numpy(), equal_nan=True)
    assert np.isnan(dev[np.tril_indices(300)]).all()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_hommel_20000_tests(dtype):
    from seekr_amd import consumers
    rng = np.random.default_rng(17)
    v = (rng.random((100, 200)) ** 4).astype(dtype)
    v[3, :5] = v[0, 0]  # ties
    got = consumers.adjust_pvalues(_device(v), "hommel", 0.05, symmetric=False).to_numpy()
    want = adj_rule.correct(v.reshape(-1), "hommel").reshape(v.shape)
    assert got.dtype == np.dtype(dtype)
    assert np.array_equal(got, want)


def test_triu_flatten_float64():
    from seekr_amd import consumers
    rng = np.random.default_rng(2)
    a = rng.random((257, 257))
    got = consumers.triu_values(_device(a)).to_numpy().reshape(-1)
    assert got.dtype == np.float64
    assert np.array_equal(got, a[np.triu_indices(257, 1)])
