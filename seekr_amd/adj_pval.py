"""adj_pval (adj_pval.py:53-138): multiple-testing correction of a p-value DataFrame, computed on an MI355X.

The frame is symmetric when it is square, its row labels equal its column labels and, off the diagonal, round(x, 5)
in the frame's dtype equals the mirror cell (NaN equal to NaN).  Then the tests are the strict upper triangle and the
result is a float64 frame that is NaN elsewhere; otherwise the tests are the whole matrix and the result has the
method's dtype (the input dtype for bonferroni, sidak and hommel, float64 for every other method).  The corrected
values are statsmodels 0.12.2 multipletests' bits, with two exceptions: sidak's float32 power is evaluated in float64
and rounded once (numpy's float32 power is not correctly rounded, so the device is the closer of the two), and
holm-sidak's float64 power comes from the device's pow (within a few ulp).  Tied negative p-values are outside the
contract: the reference's result then depends on numpy's unstable argsort.

float32 and float64 frames only (NotImplementedError for any other dtype); hommel is limited to 2^22 tests.
"""
import numpy as np

from seekr_amd import _lib
from seekr_amd import consumers

NOT_A_FRAME = "The input pvals is not a dataframe. Please check the input."
SYMMETRIC = ("The input pvals is a symmetric matrix. Only the upper triangle of the matrix (excluding diagonal) is used "
             "for multiple comparison correction.")
NOT_SYMMETRIC = "The input pvals is not a symmetric matrix. The total matrix is used for multiple comparison correction."


def _values(df):
    dtypes = set(df.dtypes)
    if len(dtypes) != 1 or next(iter(dtypes)) not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise NotImplementedError("adj_pval takes float32 or float64 frames; this one holds {}".format(
            ", ".join(sorted(str(d) for d in dtypes)) or "no columns"))
    return np.ascontiguousarray(df.to_numpy())


def _labels_equal(df):
    return df.index.equals(df.columns) and df.columns.equals(df.index)


def _symmetric_on_device(df, values):
    """(symmetric, device matrix or None): the value test runs only for square frames whose labels match."""
    if df.shape[0] != df.shape[1] or not _labels_equal(df):
        return False, None
    d = _lib.default_context().from_numpy(values)
    return consumers.pvals_symmetric(d), d


def is_symmetric(df):
    """is_symmetric (adj_pval.py:57-63) of a float32 / float64 DataFrame."""
    return _symmetric_on_device(df, _values(df))[0]


def adj_pval(pvals, method, alpha=0.05, outputname=None):
    """The reference's adj_pval: a DataFrame of corrected p-values with pvals' labels (see the module docstring);
    writes f"{outputname}.csv" as DataFrame.to_csv does when outputname is given."""
    import pandas as pd
    if not isinstance(pvals, pd.DataFrame):
        print(NOT_A_FRAME)
        return None
    values = _values(pvals)
    symmetric, d = _symmetric_on_device(pvals, values)
    print(SYMMETRIC if symmetric else NOT_SYMMETRIC)
    name = consumers.adjust_method(method)
    rows, cols = values.shape
    n_tests = rows * (rows - 1) // 2 if symmetric else rows * cols
    if n_tests == 0:
        raise ZeroDivisionError("float division by zero")  # multipletests' 1./ntests
    consumers.check_hommel(name, n_tests)
    if d is None:
        d = _lib.default_context().from_numpy(values)
    out = consumers.adjust_pvalues(d, name, alpha, symmetric=symmetric)
    result = np.array(out.to_numpy())
    out.free()
    d.free()
    adj_df = pd.DataFrame(result, index=pvals.index, columns=pvals.columns)
    if outputname:
        path = f"{outputname}.csv"
        if pvals.index.name is None and pvals.columns.name is None:
            _lib.save_csv_labelled(path, result, pvals.index, pvals.columns)
        else:
            adj_df.to_csv(path)
    return adj_df
