"""find_pval of the reference (find_pval.py:70-183) on MI355X: p-values of the Pearson correlations of two FASTA files
against find_dist's result, as a DataFrame labelled with the headers.

The reference's two Python loops over the cells are replaced by one device call: consumers.parametric_pvalues for a list
of fitted distributions (the `bestfit`-th is used), consumers.empirical_pvalues for a 1-D array of background
similarities.  The frame is float32, as the reference's np.zeros_like(sim).  `progress_bar` is accepted and nothing is
shown: there is no loop.  The refusals keep the reference's sentences, order and None; the length check of the mean and
std vectors is evaluated as Python evaluates the reference's line — a chained comparison around a bitwise or — and is
not repaired (DESIGN_PARITY.md).  A distribution outside find_dist.COMMON10 has no device cdf: NotImplementedError
naming the ten.
"""
import numpy as np

from seekr_amd import _lib, consumers
from seekr_amd.fasta_reader import Reader
from seekr_amd.find_dist import COMMON10
from seekr_amd.kmer_counts import BasicCounter
from seekr_amd.pearson import pearson

NO_OUTPUT = "No p value is calculated. The output is None."
BAD_LENGTH = ("k_mer size is not compatible with the normalization mean and/or std files.",
              "Please make sure the normalization mean and std files are generated using the same kmer size as specified "
              "here in k_mer.", NO_OUTPUT)
BAD_LIST = ("The format of fitres is wrong.",
            "fitres should be a list consisting of tuples (string, number, tuple of numbers) corresponds to (distribution "
            "name, deviance, parameters)", "fitres should be the output of find_dist.", NO_OUTPUT)
BAD_ARRAY = ("The dimension of fitres as a numpy array is wrong. fitres should be a 1D numpy array.",
             "fitres should be the output of find_dist.", NO_OUTPUT)
BAD_TYPE = ("fitres should be the output of find_dist. It should be either a list of distributions or a numpy array.",
            NO_OUTPUT)
NOT_UNIQUE = "The headers of seq{}file is not unique."
NOT_UNIQUE_2 = "Be carefule during further analysis as there are potential indexing problems."


def lengths_refused(mean_len, std_len, k_mer):
    """The reference's length check (find_pval.py:76) for vectors of these lengths, as Python evaluates it: `|` binds
    tighter than `!=`, so the line is the chain  mean_len != (4**k | std_len) != 4**k.  A std vector of the wrong length
    is therefore only noticed when its bits change 4**k, and a wrong mean vector passes beside a right std vector."""
    return mean_len != 4 ** (k_mer) | std_len != 4 ** (k_mer)


def _is_number(x):
    return isinstance(x, float) or np.isscalar(x)


def fitres_list_ok(fitres):
    """Every entry is (str, number, tuple of numbers), by the reference's test (find_pval.py:55-67)."""
    return all(len(t) == 3 and isinstance(t[0], str) and _is_number(t[1]) and isinstance(t[2], tuple)
               and all(_is_number(x) for x in t[2]) for t in fitres)


def _say(lines):
    for line in lines:
        print(line)


@_lib.api_call
def find_pval(seq1file, seq2file, mean_path, std_path, k_mer, fitres, log2="Log2.post", bestfit=1, outputname=None,
              progress_bar=True):
    """DataFrame of p-values (float32; rows: the headers of seq1file, columns: those of seq2file, without '>'), or None
    after the reference's sentences when the vectors do not fit k_mer or fitres is not find_dist's output.
    <outputname>.csv receives DataFrame.to_csv's bytes."""
    import pandas as pd
    meanfile, stdfile = np.load(mean_path), np.load(std_path)
    if lengths_refused(len(meanfile), len(stdfile), k_mer):
        _say(BAD_LENGTH)
        return None
    t1 = BasicCounter(seq1file, mean=mean_path, std=std_path, k=k_mer, log2=log2, silent=True)
    t2 = BasicCounter(seq2file, mean=mean_path, std=std_path, k=k_mer, log2=log2, silent=True)
    t1.make_count_file()
    t2.make_count_file()
    sim = pearson(t1.counts, t2.counts)
    header1 = [h[1:] for h in Reader(seq1file).get_headers()]
    header2 = [h[1:] for h in Reader(seq2file).get_headers()]
    for which, header in ((1, header1), (2, header2)):
        if len(header) != len(set(header)):
            print(NOT_UNIQUE.format(which))
            print(NOT_UNIQUE_2)
    if isinstance(fitres, list):
        if not fitres_list_ok(fitres):
            _say(BAD_LIST)
            return None
        name, _, params = fitres[bestfit - 1]
        if name not in COMMON10:
            raise NotImplementedError("no device cdf for {!r}: find_dist fits any scipy distribution, find_pval knows {}"
                                      .format(name, ", ".join(COMMON10)))
    elif isinstance(fitres, np.ndarray):
        if len(fitres.shape) != 1:
            _say(BAD_ARRAY)
            return None
    else:
        _say(BAD_TYPE)
        return None
    p_values = np.array(consumers.pvalues_host(sim, fitres, bestfit))
    pval_df = pd.DataFrame(p_values, index=header1, columns=header2)
    if outputname:
        _lib.save_csv_labelled(f"{outputname}.csv", p_values, header1, header2)
    return pval_df
