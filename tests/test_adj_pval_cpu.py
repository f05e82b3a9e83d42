"""adj_pval without a device: the numpy restatement (tests/adj_rule.py) against the reference's golden outputs, and the
package's argument handling that runs before any device work."""
import json
import os

import numpy as np
import pytest

import adj_rule

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
POWER_METHODS = ("sidak", "holm-sidak")  # numpy's power vs the device's: held to 4 eps of the dtype (see assert_matches)


def load_cases():
    with open(os.path.join(GOLDEN, "adj_pval.json")) as f:
        meta = json.load(f)
    data = np.load(os.path.join(GOLDEN, "adj_pval.npz"))
    return [(c, data["in%d" % i], data["out%d" % i]) for i, c in enumerate(meta["cases"])], meta["csv"]


CASES, CSVS = load_cases()


def assert_matches(got, want, method, in_dtype):
    assert got.dtype == want.dtype, (got.dtype, want.dtype)
    assert got.shape == want.shape
    if method in POWER_METHODS:
        assert np.array_equal(np.isnan(got), np.isnan(want))
        g, w = got[~np.isnan(want)].astype(np.float64), want[~np.isnan(want)].astype(np.float64)
        same = g == w  # infinities included
        # 4 eps absolute for p-values; relative for the huge values inputs above 1 produce (1 - (1 - 7.25) ** n)
        bar = 4 * np.finfo(in_dtype).eps * np.maximum(1.0, np.abs(np.where(same, 1.0, w)))
        assert np.all(same | (np.abs(np.where(same, 0, g - w)) <= bar))
    else:
        assert np.array_equal(got, want, equal_nan=True)


@pytest.mark.parametrize("idx", range(len(CASES)), ids=["%d-%s-%s" % (i, c[0]["name"], c[0]["method"]) for i, c in enumerate(CASES)])
def test_rule_matches_reference(idx):
    case, v, want = CASES[idx]
    symmetric, got = adj_rule.adj_frame(v, case["rows"] == case["cols"], case["method"], case["alpha"])
    assert symmetric == case["message"].startswith("The input pvals is a symmetric")
    assert str(want.dtype) == case["out_dtype"]
    assert_matches(got, want, case["method"], v.dtype)


def test_fixture_covers_the_contract():
    methods = {c["method"] for c, _, _ in CASES}
    assert methods == set(adj_rule.METHODS)
    assert {v.dtype for _, v, _ in CASES} == {np.dtype(np.float32), np.dtype(np.float64)}
    assert any(c["message"].startswith("The input pvals is a symmetric") for c, _, _ in CASES)
    assert max(v.size for c, v, _ in CASES if c["method"] == "hommel") >= 2000
    assert [c["name"] for c in CSVS] == ["text_labels_sym", "numeric_headers", "repeated_headers"]


def test_aliases_match_the_rule():
    from seekr_amd import consumers
    assert consumers.ADJ_ALIASES == adj_rule.ALIASES
    for alias, name in adj_rule.ALIASES.items():
        assert consumers.adjust_method(alias.upper()) == name
    with pytest.raises(ValueError, match="method not recognized"):
        consumers.adjust_method("bh")


def test_not_a_frame(capsys):
    from seekr_amd.adj_pval import adj_pval
    assert adj_pval(np.zeros((3, 3), np.float32), "fdr_bh") is None
    assert capsys.readouterr().out == "The input pvals is not a dataframe. Please check the input.\n"


def test_unknown_method_after_the_message(capsys):
    import pandas as pd
    from seekr_amd.adj_pval import adj_pval
    df = pd.DataFrame(np.full((2, 3), 0.5, np.float32))
    with pytest.raises(ValueError, match="method not recognized"):
        adj_pval(df, "no-such-method")
    assert capsys.readouterr().out.startswith("The input pvals is not a symmetric matrix.")


def test_other_dtypes_refused():
    import pandas as pd
    from seekr_amd.adj_pval import adj_pval
    with pytest.raises(NotImplementedError, match="int64"):
        adj_pval(pd.DataFrame(np.ones((2, 3), np.int64)), "holm")


def test_hommel_limit(capsys):
    import pandas as pd
    from seekr_amd.adj_pval import adj_pval
    df = pd.DataFrame(np.full((2048, 2049), 0.5, np.float32))
    with pytest.raises(NotImplementedError, match="4194304.*4196352"):
        adj_pval(df, "hommel")
    assert capsys.readouterr().out.startswith("The input pvals is not a symmetric matrix.")


def test_csv_writer_gives_the_reference_bytes(tmp_path):
    """The native labelled writer (no device) writes what DataFrame.to_csv wrote for the reference's results."""
    import pandas as pd
    from seekr_amd import _lib
    for c in CSVS:
        src = tmp_path / (c["name"] + ".csv")
        src.write_text(c["output"])
        df = pd.read_csv(src, header=0, index_col=0, float_precision="round_trip")
        out = tmp_path / (c["name"] + "_again.csv")
        _lib.save_csv_labelled(out, np.ascontiguousarray(df.to_numpy()), df.index, df.columns)
        assert out.read_text() == c["output"], c["name"]
