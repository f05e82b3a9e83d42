"""`seekr_kmer_counts`, `seekr_pearson`, `seekr_norm_vectors` and `seekr_adj_pval` with the reference's flags
(console_scripts.py:564-681, 887-918), and `seekr_domain_pearson` (sliding windows of a target against queries: no
counterpart in the reference), `seekr_nearest` (the k most correlated rows of every row: likewise) and
`seekr_significant_pairs` (the pairs whose corrected p-value is at most alpha, without any N x N matrix: likewise), and
`seekr_kmer_leiden` with the reference's flags (console_scripts.py:1033-1101) plus --edges, --kmers_top and --density, and
`seekr_pair_kmers` (the k-mers behind the similarity of listed pairs: no counterpart) and `seekr_r_distribution` (the
histogram, quantiles and density cutoffs of r without the matrix: likewise), and `seekr_domain_significant` and
`seekr_domain_hits` (the significant windows of a target, and hot windows merged into intervals: likewise), and
`seekr_find_dist` and `seekr_find_pval` with the reference's flags (console_scripts.py:741-885).  Only the commands on
the hot path are provided."""
import argparse
import sys

import numpy as np

from seekr_amd import _lib
from seekr_amd import pearson as pearson_mod
from seekr_amd.kmer_counts import BasicCounter

KMER_COUNTS_DOC = """
Description
-----------
Counts the k-mers of every sequence of a FASTA file on an MI355X and writes the per-kb,
normalised count matrix: one row per sequence, 4^k columns.  Flags and output files are
those of the reference command of the same name.

Examples
--------
    labelled CSV, 6-mers:            seekr_kmer_counts transcripts.fa -o counts.csv
    binary, unlabelled, 5-mers:      seekr_kmer_counts transcripts.fa -o counts.npy -k 5 -b -rl
    normalise with stored vectors:   seekr_kmer_counts transcripts.fa -o counts.csv -mv mean.npy -sv std.npy
"""

PEARSON_DOC = """
Description
-----------
All-pairs Pearson correlation between the rows of two k-mer count files, computed on an
MI355X.  Flags and output files are those of the reference command of the same name.

Examples
--------
    labelled CSV in and out:   seekr_pearson counts.csv counts.csv -o r.csv
    .npy in and out:           seekr_pearson counts.npy counts.npy -o r.npy -bi -bo
"""

ADJ_PVAL_DOC = """
Description
-----------
Multiple-testing correction of a labelled p-value CSV (the output of find_pval) on an MI355X,
with statsmodels' multipletests methods.  A symmetric matrix (same row and column names, the
same values on both sides of the diagonal to 5 decimals) is corrected over its upper triangle
only and the rest of the output is empty; any other matrix is corrected as a whole.  Flags and
output file are those of the reference command of the same name.

Examples
--------
    Bonferroni at 0.05, written to adj.csv:   seekr_adj_pval pvals.csv bonferroni -a 0.05 -o adj
    Benjamini-Hochberg, not saved:            seekr_adj_pval pvals.csv fdr_bh
"""

NORM_VECTORS_DOC = """
Description
-----------
Column mean and standard deviation of the k-mer counts of a (large) FASTA file, saved as two .npy
vectors that later runs can normalise against (-mv / -sv of seekr_kmer_counts).

Examples
--------
    defaults (6-mers, mean.npy, std.npy):   seekr_norm_vectors gencode.fa
    5-mers, named outputs:                  seekr_norm_vectors gencode.fa -k 5 -mv mean5.npy -sv std5.npy
"""

DOMAIN_PEARSON_DOC = """
Description
-----------
Pearson correlation between the k-mer profile of every query sequence and the profile of every sliding window of the
target sequences, computed on an MI355X: which part of a long transcript or region resembles a query.  The windows are
counted from the packed target on the device; both sides are normalised with the stored mean and std vectors
(seekr_norm_vectors).  Rows of the output are the queries, columns the windows, labelled header:start-end.

Examples
--------
    labelled CSV:   seekr_domain_pearson repeats.fa chrX_region.fa mean.npy std.npy -k 6 -w 1000 -s 100 -o r.csv
    .npy:           seekr_domain_pearson repeats.fa chrX_region.fa mean.npy std.npy -w 500 -s 50 -o r.npy -bo
"""

NEAREST_DOC = """
Description
-----------
For every row of a k-mer count file, the rows of a second count file (or of the same one) it correlates with most,
computed on an MI355X without the all-pairs matrix ever standing anywhere.  The output is a CSV with the columns
row,rank,neighbor,r: rank 0 is the best neighbour; rows and neighbours are named by the labels of the count files, or
by their indices for .npy input.  With one count file a row is not its own neighbour.

Examples
--------
    ten neighbours within one file:    seekr_nearest counts.csv -o nearest.csv
    three of b.npy for each of a.npy:  seekr_nearest a.npy b.npy -n 3 -o nearest.csv -bi
"""

RECIPROCAL_HITS_DOC = """
Description
-----------
The reciprocal nearest neighbours of the rows of two k-mer count files (or of one), computed on an MI355X from ONE sweep of
the correlations and without the all-pairs matrix: the pairs (row, col) where col is among the K rows of the second file
row correlates with most and (mutual) or or (union) row is among the K rows of the first file col correlates with most.
The output is a CSV with the columns row,col,r,rank_row,rank_col, ascending by row and col: rank 0 is the best
neighbour, an empty rank means the pair is not in that side's list (union only); rows and columns are named by the
labels of the count files, or by their indices for .npy input.  With one count file a row is not its own neighbour and
every pair comes once, the smaller row first.

Examples
--------
    mutual best hits of two files:        seekr_reciprocal_hits a.csv b.csv -n 1 -o hits.csv
    union 15-neighbour pairs of one file:  seekr_reciprocal_hits counts.npy -n 15 -m union -o pairs.csv -bi
"""

SIGNIFICANT_PAIRS_DOC = """
Description
-----------
The significantly similar pairs of rows of a k-mer count file, computed on an MI355X without the all-pairs matrix, the
p-value matrix or the corrected matrix ever standing anywhere: r of every pair against a background (the similarities
find_dist saved, or a fitted distribution with its parameters), the p-values corrected over all N (N - 1) / 2 pairs, and
the pairs whose corrected p-value is at most alpha.  The output is a CSV with the columns row,col,r,p,p_adj, one line
per pair (row before col), named by the labels of the count file or by indices for .npy input.  Methods: bonferroni,
sidak, holm-sidak, holm, simes-hochberg, fdr_bh, fdr_by.  With a second count file the rows of the first are tested
against the rows of the second (find_pval's two-file form): N1 x N2 tests, every cell one of them, `row` named from
the first file and `col` from the second.

Examples
--------
    against saved background similarities:   seekr_significant_pairs counts.csv -bg background.npy -o pairs.csv
    against a fitted normal, Bonferroni:     seekr_significant_pairs counts.npy -bi -d norm -p 0.01 0.12 -m bonferroni -a 0.01 -o pairs.csv
    queries against a transcriptome:         seekr_significant_pairs queries.csv transcripts.csv -bg background.npy -o pairs.csv
"""

DOMAIN_SIGNIFICANT_DOC = """
Description
-----------
The sliding windows of the target sequences that each query is significantly similar to, computed on an MI355X without
the query x window matrix ever leaving the device: r of every query against every window (as seekr_domain_pearson
computes it), its p-value against a background (saved similarities, or a fitted distribution with its parameters),
the p-values corrected over all queries x windows tests, and the cells whose corrected p-value is at most alpha.  The
output is a CSV with the columns query,header,start,end,r,p,p_adj, one line per significant (query, window) cell in
that order.  Methods: bonferroni, sidak, holm-sidak, holm, simes-hochberg, fdr_bh, fdr_by.

Examples
--------
    seekr_domain_significant query.fa target.fa mean.npy std.npy -k 4 -w 500 -s 50 -bg background.npy -o domains.csv
    seekr_domain_significant query.fa target.fa mean.npy std.npy -d norm -p 0.0 0.07 -m bonferroni -a 0.01 -o domains.csv
"""

DOMAIN_HITS_DOC = """
Description
-----------
The intervals of the target sequences that each query resembles, computed on an MI355X without the query x window
matrix ever leaving the device: r of every query against every sliding window (as seekr_domain_pearson computes it),
the windows with r at or above a cutoff, and consecutive such windows of one target sequence merged into hits (at most
--max_gap windows below the cutoff between two of them).  The cutoff is given (-c), or taken from a background at
alpha (-bg, or -d with -p: the smallest r whose p-value is at most alpha), or — with -m — the windows are those
seekr_domain_significant lists.  The output is a CSV with the columns
query,header,start,end,first_window,last_window,n_windows,n_hot,peak_r,peak_start,peak_end, one line per hit, ordered
by query and position.

Examples
--------
    seekr_domain_hits query.fa target.fa mean.npy std.npy -k 4 -w 500 -s 50 -c 0.2 -g 1 -o hits.csv
    seekr_domain_hits query.fa target.fa mean.npy std.npy -bg background.npy -a 0.01 -mw 3 -o hits.csv
    seekr_domain_hits query.fa target.fa mean.npy std.npy -d norm -p 0.0 0.07 -m fdr_bh -o hits.csv
"""

_LOG2 = ["Log2.post", "Log2.pre", "Log2.none"]


def _parse_args_or_exit(parser):
    if len(sys.argv) == 1:  # console_scripts.py:520-525
        parser.print_help()
        sys.exit(0)
    return parser.parse_args()


def _run_kmer_counts(fasta, outfile, kmer, binary, centered, standardized, log2, remove_labels, mean_vector,
                     std_vector, alphabet):
    mean = mean_vector or centered  # console_scripts.py:568-569
    std = std_vector or standardized
    counter = BasicCounter(fasta, outfile, kmer, binary, mean, std, log2, label=not remove_labels, alphabet=alphabet)
    counter.make_count_file()


def console_kmer_counts():
    parser = argparse.ArgumentParser(usage=KMER_COUNTS_DOC, formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    parser.add_argument("fasta", help="FASTA file with the sequences to count.")
    parser.add_argument("-o", "--outfile", default="counts.seekr", help="Where the count matrix goes.")
    parser.add_argument("-k", "--kmer", default=6, help="k, the word length (4^k columns).")
    parser.add_argument("-b", "--binary", action="store_true", help="Write .npy instead of CSV.")
    parser.add_argument("-uc", "--uncentered", action="store_false",
                        help="Leave the column means in (no centring).")
    parser.add_argument("-us", "--unstandardized", action="store_false",
                        help="Do not divide by the column standard deviations.")
    parser.add_argument("-l", "--log2", default="Log2.post", choices=_LOG2,
                        help="log2 before the column statistics (pre), after them (post), or not at all (none).")
    parser.add_argument("-rl", "--remove_labels", action="store_true",
                        help="Plain CSV without the header row and the name column (required with -b).")
    parser.add_argument("-mv", "--mean_vector", default=None, help="Centre with this stored mean vector (.npy) instead of the set's own.")
    parser.add_argument("-sv", "--std_vector", default=None, help="Scale with this stored std vector (.npy) instead of the set's own.")
    parser.add_argument("-a", "--alphabet", default="AGTC", help="The four letters, in column-index order.")
    args = _parse_args_or_exit(parser)
    _run_kmer_counts(args.fasta, args.outfile, int(args.kmer), args.binary, args.uncentered, args.unstandardized,
                     args.log2, args.remove_labels, args.mean_vector, args.std_vector, args.alphabet)


def _read_labelled_csv(path):
    """pd.read_csv(path, index_col=0) -> (float64 values, index labels): natively for the files the
    count command writes, through pandas for anything the native reader declines (csv_read.hip)."""
    native = _lib.load_csv_labelled(path)
    if native is not None:
        return native[0], np.array(native[1], dtype=object)
    import pandas as pd
    frame = pd.read_csv(path, index_col=0)
    return frame, frame.index.values


def _run_pearson(counts1, counts2, outfile, binary_input, binary_output):
    names1 = names2 = None
    same_file = counts1 == counts2  # one file twice: read once, and the contraction computes one triangle
    if binary_input:
        counts1 = np.load(counts1)
        counts2 = counts1 if same_file else np.load(counts2)
    else:  # labelled CSVs; float64 path (console_scripts.py:628-631)
        counts1, names1 = _read_labelled_csv(counts1)
        counts2, names2 = (counts1, names1) if same_file else _read_labelled_csv(counts2)
    if binary_output:
        # np.save(outfile, dist) without dist ever standing in host memory: stripes of r go from the GPU(s) to the file
        pearson_mod.pearson_to_file(counts1, counts2, outfile)
    else:
        dist = pearson_mod.pearson(counts1, counts2)
        # pd.DataFrame(dist, names1, names2).to_csv(outfile); names None -> RangeIndex labels 0..n-1
        _lib.save_csv_labelled(outfile, dist, range(dist.shape[0]) if names1 is None else names1,
                               range(dist.shape[1]) if names2 is None else names2)


def console_pearson():
    parser = argparse.ArgumentParser(usage=PEARSON_DOC, formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    parser.add_argument("counts1", help="First count file (rows of the result).")
    parser.add_argument("counts2", help="Second count file (columns of the result); may be the first one again.")
    parser.add_argument("-o", "--outfile", default="pearson.seekr", help="Where the correlation matrix goes.")
    parser.add_argument("-bi", "--binary_input", action="store_true", help="The count files are .npy, not labelled CSV.")
    parser.add_argument("-bo", "--binary_output", action="store_true", help="Write .npy instead of CSV.")
    args = _parse_args_or_exit(parser)
    _run_pearson(args.counts1, args.counts2, args.outfile, args.binary_input, args.binary_output)


def _run_norm_vectors(fasta, mean_vector, std_vector, log2, kmer):
    counter = BasicCounter(fasta, k=int(kmer), log2=log2)
    counter.get_counts()
    _lib.save_npy(mean_vector, counter.mean)
    _lib.save_npy(std_vector, counter.std)


def console_norm_vectors():
    parser = argparse.ArgumentParser(usage=NORM_VECTORS_DOC, formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    parser.add_argument("fasta", help="FASTA file to take the statistics of.")
    parser.add_argument("-mv", "--mean_vector", default="mean.npy", help="Output: column means (.npy).")
    parser.add_argument("-sv", "--std_vector", default="std.npy", help="Output: column standard deviations (.npy).")
    parser.add_argument("-l", "--log2", default="Log2.post", choices=_LOG2,
                        help="log2 before the column statistics (pre), after them (post), or not at all (none).")
    parser.add_argument("-k", "--kmer", default=6, help="k, the word length.")
    args = _parse_args_or_exit(parser)
    _run_norm_vectors(args.fasta, args.mean_vector, args.std_vector, args.log2, int(args.kmer))


def _read_pval_csv(path):
    """pd.read_csv(path, header=0, index_col=0) (console_scripts.py:913): natively when the file is in the subset the
    native reader reproduces (an empty corner cell, text row labels, distinct column labels), else through pandas."""
    import pandas as pd
    with open(path, "rb") as f:
        corner_empty = f.read(1) == b","
    native = _lib.load_csv_labelled(path) if corner_empty else None
    if native is None:
        return pd.read_csv(path, header=0, index_col=0)
    values, rows, cols = native
    return pd.DataFrame(values, index=pd.Index(rows, dtype=object), columns=pd.Index(cols, dtype=object))


def console_adj_pval():
    from seekr_amd import adj_pval
    parser = argparse.ArgumentParser(usage=ADJ_PVAL_DOC, formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    parser.add_argument("pval_path", help="Labelled CSV of the p-values to correct (find_pval's output).")
    parser.add_argument("method", help=("Correction method: bonferroni, sidak, holm-sidak, holm, simes-hochberg, hommel, "
                                        "fdr_bh, fdr_by, fdr_tsbh, fdr_tsbky (statsmodels' multipletests names)."))
    parser.add_argument("-a", "--alpha", default=0.05, help="Family-wise error rate (only the two-stage FDR methods use it).")
    parser.add_argument("-o", "--outputname", default=None,
                        help="Where the corrected matrix goes ('.csv' is appended); not saved when omitted.")
    args = _parse_args_or_exit(parser)
    pvals = _read_pval_csv(args.pval_path)
    adj_pval.adj_pval(pvals, args.method, float(args.alpha), args.outputname)


def _run_domain_pearson(query, target, mean, std, kmer, window, slide, log2, outfile, binary_output):
    from seekr_amd import windows
    from seekr_amd.fasta_reader import Reader
    r, table = windows.domain_pearson(query, target, kmer, window, slide, mean, std, log2=log2)
    if binary_output:
        _lib.save_npy(outfile, r)
    else:
        _lib.save_csv_labelled(outfile, r, Reader(query).get_headers(), windows.window_labels(table))


def console_domain_pearson():
    parser = argparse.ArgumentParser(usage=DOMAIN_PEARSON_DOC, formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    parser.add_argument("query", help="FASTA file with the query sequences (rows of the result).")
    parser.add_argument("target", help="FASTA file with the target sequences; their sliding windows are the columns.")
    parser.add_argument("mean", help="Stored mean vector (.npy) both sides are centred with.")
    parser.add_argument("std", help="Stored std vector (.npy) both sides are scaled with.")
    parser.add_argument("-k", "--kmer", default=6, help="k, the word length (4^k columns; up to 7).")
    parser.add_argument("-w", "--window", default=1000, help="Letters per window.")
    parser.add_argument("-s", "--slide", default=100, help="Letters between the starts of two windows (at most the window).")
    parser.add_argument("-l", "--log2", default="Log2.post", choices=_LOG2,
                        help="log2 before the column statistics (pre), after them (post), or not at all (none).")
    parser.add_argument("-o", "--outfile", default="domain_pearson.seekr", help="Where the correlation matrix goes.")
    parser.add_argument("-bo", "--binary_output", action="store_true", help="Write .npy instead of a labelled CSV.")
    args = _parse_args_or_exit(parser)
    _run_domain_pearson(args.query, args.target, args.mean, args.std, int(args.kmer), int(args.window), int(args.slide),
                        args.log2, args.outfile, args.binary_output)


def _run_nearest(counts1, counts2, neighbors, outfile, binary_input):
    import csv
    from seekr_amd import neighbors as neighbors_mod
    names1 = names2 = None
    same_file = counts2 is None or counts1 == counts2
    if binary_input:  # read as _run_pearson reads them
        counts1 = np.load(counts1)
        counts2 = None if same_file else np.load(counts2)
    else:
        counts1, names1 = _read_labelled_csv(counts1)
        counts2, names2 = (None, names1) if same_file else _read_labelled_csv(counts2)
    idx, val = neighbors_mod.nearest(counts1, counts2, k=neighbors)
    with open(outfile, "w", newline="") as f:
        out = csv.writer(f, lineterminator="\n")
        out.writerow(["row", "rank", "neighbor", "r"])
        for i in range(idx.shape[0]):
            for t in range(idx.shape[1]):
                j = int(idx[i, t])
                if j == _lib.TOPK_PAD_IDX:  # fewer candidates than neighbours asked for
                    break
                out.writerow([i if names1 is None else names1[i], t, j if names2 is None else names2[j], str(val[i, t])])


def console_nearest():
    parser = argparse.ArgumentParser(usage=NEAREST_DOC, formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    parser.add_argument("counts1", help="Count file whose rows are asked about.")
    parser.add_argument("counts2", nargs="?", default=None,
                        help="Count file the neighbours come from (default: counts1 itself, a row's own cell left out).")
    parser.add_argument("-n", "--neighbors", default=10, help="Neighbours per row (at most %d)." % _lib.TOPK_MERGE_KMAX)
    parser.add_argument("-o", "--outfile", default="nearest.csv", help="Where the list goes (CSV: row,rank,neighbor,r).")
    parser.add_argument("-bi", "--binary_input", action="store_true", help="The count files are .npy, not labelled CSV.")
    args = _parse_args_or_exit(parser)
    _run_nearest(args.counts1, args.counts2, int(args.neighbors), args.outfile, args.binary_input)


def _run_reciprocal_hits(counts1, counts2, neighbors, mode, outfile, binary_input):
    import csv
    from seekr_amd import reciprocal
    names1 = names2 = None
    same_file = counts2 is None or counts1 == counts2
    if binary_input:  # read as _run_nearest reads them
        counts1 = np.load(counts1)
        counts2 = None if same_file else np.load(counts2)
    else:
        counts1, names1 = _read_labelled_csv(counts1)
        counts2, names2 = (None, names1) if same_file else _read_labelled_csv(counts2)
    hits = reciprocal.reciprocal_hits(counts1, counts2, k=neighbors, mode=mode)
    with open(outfile, "w", newline="") as f:
        out = csv.writer(f, lineterminator="\n")
        out.writerow(list(reciprocal.COLUMNS))
        for i, j, r, rank_row, rank_col in zip(*(hits[c].to_numpy() for c in reciprocal.COLUMNS)):
            out.writerow([int(i) if names1 is None else names1[int(i)], int(j) if names2 is None else names2[int(j)], str(r),
                          "" if rank_row == _lib.TOPK_PAD_IDX else int(rank_row),
                          "" if rank_col == _lib.TOPK_PAD_IDX else int(rank_col)])


def console_reciprocal_hits():
    parser = argparse.ArgumentParser(usage=RECIPROCAL_HITS_DOC, formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    parser.add_argument("counts1", help="Count file whose rows are the `row` side.")
    parser.add_argument("counts2", nargs="?", default=None,
                        help="Count file whose rows are the `col` side (default: counts1 itself, every pair once).")
    parser.add_argument("-n", "--neighbors", default=10,
                        help="Neighbours per row (at most %d with two files, %d with one)." % (_lib.TOPK_COLS_KMAX, _lib.TOPK_MERGE_KMAX))
    parser.add_argument("-m", "--mode", default="mutual", choices=["mutual", "union"],
                        help="Keep a pair when both sides list each other (mutual) or when either does (union).")
    parser.add_argument("-o", "--outfile", default="reciprocal_hits.csv", help="Where the pairs go (CSV: row,col,r,rank_row,rank_col).")
    parser.add_argument("-bi", "--binary_input", action="store_true", help="The count files are .npy, not labelled CSV.")
    args = _parse_args_or_exit(parser)
    _run_reciprocal_hits(args.counts1, args.counts2, int(args.neighbors), args.mode, args.outfile, args.binary_input)


def _read_background(path):
    """A 1-D array of background similarities: a .npy file or a one-column CSV (what find_dist writes with
    fit_model=False and an outputname)."""
    if str(path).endswith(".npy"):
        return np.asarray(np.load(path)).reshape(-1)
    return np.loadtxt(path, delimiter=",", ndmin=1).reshape(-1)


def _fitres(background, dist, params):
    return _read_background(background) if background is not None else [(dist, 0.0, tuple(float(v) for v in params))]


def _add_significance_arguments(parser, what):
    """-bg | -d -p, -m and -a: the background, the correction method and alpha of the significance commands."""
    source = parser.add_mutually_exclusive_group(required=True)
    source.add_argument("-bg", "--background", default=None,
                        help="Background similarities: a .npy file or a one-column CSV (find_dist's output without a fit).")
    source.add_argument("-d", "--distribution", default=None, help="Name of the fitted distribution (with -p).")
    parser.add_argument("-p", "--params", nargs="+", default=None, help="Its parameters as find_dist lists them (shape, loc, scale).")
    parser.add_argument("-m", "--method", default="fdr_bh", help="Correction method (statsmodels' multipletests names).")
    parser.add_argument("-a", "--alpha", default=0.05, help="%s with a corrected p-value of at most this are listed." % what)


def _run_significant_pairs(counts, outfile, binary_input, background, dist, params, method, alpha, counts2=None):
    import csv
    from seekr_amd import significant
    names = names2 = None
    if binary_input:
        counts = np.load(counts)
        counts2 = None if counts2 is None else np.load(counts2)
    else:
        counts, names = _read_labelled_csv(counts)
        counts2, names2 = (None, names) if counts2 is None else _read_labelled_csv(counts2)
    res = significant.significant_pairs(counts, _fitres(background, dist, params), method=method, alpha=alpha, counts2=counts2)
    with open(outfile, "w", newline="") as f:
        out = csv.writer(f, lineterminator="\n")
        out.writerow(["row", "col", "r", "p", "p_adj"])
        for i, j, r, p, q in zip(res.rows, res.cols, res.r, res.p, res.p_adj):
            out.writerow([int(i) if names is None else names[int(i)], int(j) if names2 is None else names2[int(j)], str(r), str(p),
                          repr(float(q))])


def console_significant_pairs():
    parser = argparse.ArgumentParser(usage=SIGNIFICANT_PAIRS_DOC, formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    parser.add_argument("counts", help="Count file whose pairs of rows are tested.")
    parser.add_argument("counts2", nargs="?", default=None,
                        help="Count file whose rows those of `counts` are tested against (default: counts against itself).")
    parser.add_argument("-bi", "--binary_input", action="store_true", help="The count files are .npy, not labelled CSV.")
    parser.add_argument("-o", "--outfile", default="significant_pairs.csv", help="Where the list goes (CSV: row,col,r,p,p_adj).")
    _add_significance_arguments(parser, "Pairs")
    args = _parse_args_or_exit(parser)
    if args.distribution is not None and not args.params:
        parser.error("-d needs the parameters of the distribution: -p P [P ...]")
    _run_significant_pairs(args.counts, args.outfile, args.binary_input, args.background, args.distribution, args.params,
                           args.method, float(args.alpha), args.counts2)


def _run_domain_significant(query, target, mean, std, kmer, window, slide, log2, outfile, background, dist, params, method,
                            alpha):
    import csv
    from seekr_amd import windows
    frame = windows.domain_significant(query, target, kmer, window, slide, mean, std, _fitres(background, dist, params),
                                       method=method, alpha=alpha, log2=log2)
    with open(outfile, "w", newline="") as f:
        out = csv.writer(f, lineterminator="\n")
        out.writerow(["query", "header", "start", "end", "r", "p", "p_adj"])
        for q, h, s, e, r, p, a in zip(frame["query"], frame["header"], frame["start"], frame["end"], frame["r"], frame["p"],
                                       frame["p_adj"]):
            out.writerow([int(q), h, int(s), int(e), str(np.float32(r)), str(np.float32(p)), repr(float(a))])


def console_domain_significant():
    parser = argparse.ArgumentParser(usage=DOMAIN_SIGNIFICANT_DOC, formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    parser.add_argument("query", help="FASTA file with the query sequences.")
    parser.add_argument("target", help="FASTA file with the target sequences; their sliding windows are tested.")
    parser.add_argument("mean", help="Stored mean vector (.npy) both sides are centred with.")
    parser.add_argument("std", help="Stored std vector (.npy) both sides are scaled with.")
    parser.add_argument("-k", "--kmer", default=6, help="k, the word length (4^k columns; up to 7).")
    parser.add_argument("-w", "--window", default=1000, help="Letters per window.")
    parser.add_argument("-s", "--slide", default=100, help="Letters between the starts of two windows (at most the window).")
    parser.add_argument("-l", "--log2", default="Log2.post", choices=_LOG2,
                        help="log2 before the column statistics (pre), after them (post), or not at all (none).")
    parser.add_argument("-o", "--outfile", default="domain_significant.csv",
                        help="Where the list goes (CSV: query,header,start,end,r,p,p_adj).")
    _add_significance_arguments(parser, "Windows")
    args = _parse_args_or_exit(parser)
    if args.distribution is not None and not args.params:
        parser.error("-d needs the parameters of the distribution: -p P [P ...]")
    _run_domain_significant(args.query, args.target, args.mean, args.std, int(args.kmer), int(args.window), int(args.slide),
                            args.log2, args.outfile, args.background, args.distribution, args.params, args.method,
                            float(args.alpha))


HITS_COLUMNS = ["query", "header", "start", "end", "first_window", "last_window", "n_windows", "n_hot", "peak_r", "peak_start",
                "peak_end"]


def _run_domain_hits(query, target, mean, std, kmer, window, slide, log2, outfile, cutoff, background, dist, params, method,
                     alpha, max_gap, min_windows):
    import csv
    from seekr_amd import windows
    fitres = None if cutoff is not None else _fitres(background, dist, params)
    frame = windows.domain_hits(query, target, kmer, window, slide, mean, std, cutoff=cutoff, fitres=fitres, alpha=alpha,
                                method=method, max_gap=max_gap, min_windows=min_windows, log2=log2)
    with open(outfile, "w", newline="") as f:
        out = csv.writer(f, lineterminator="\n")
        out.writerow(HITS_COLUMNS)
        for row in zip(*(frame[c] for c in HITS_COLUMNS)):
            out.writerow([str(np.float32(v)) if c == "peak_r" else v if c == "header" else int(v) for c, v in zip(HITS_COLUMNS, row)])


def console_domain_hits():
    parser = argparse.ArgumentParser(usage=DOMAIN_HITS_DOC, formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    parser.add_argument("query", help="FASTA file with the query sequences.")
    parser.add_argument("target", help="FASTA file with the target sequences; their sliding windows are merged into hits.")
    parser.add_argument("mean", help="Stored mean vector (.npy) both sides are centred with.")
    parser.add_argument("std", help="Stored std vector (.npy) both sides are scaled with.")
    parser.add_argument("-k", "--kmer", default=6, help="k, the word length (4^k columns; up to 7).")
    parser.add_argument("-w", "--window", default=1000, help="Letters per window.")
    parser.add_argument("-s", "--slide", default=100, help="Letters between the starts of two windows (at most the window).")
    parser.add_argument("-l", "--log2", default="Log2.post", choices=_LOG2,
                        help="log2 before the column statistics (pre), after them (post), or not at all (none).")
    parser.add_argument("-o", "--outfile", default="domain_hits.csv", help="Where the hits go (CSV: %s)." % ",".join(HITS_COLUMNS))
    source = parser.add_mutually_exclusive_group(required=True)
    source.add_argument("-c", "--cutoff", default=None, help="A window is hot when its r is at least this.")
    source.add_argument("-bg", "--background", default=None,
                        help="Background similarities: a .npy file or a one-column CSV (find_dist's output without a fit).")
    source.add_argument("-d", "--distribution", default=None, help="Name of the fitted distribution (with -p).")
    parser.add_argument("-p", "--params", nargs="+", default=None, help="Its parameters as find_dist lists them (shape, loc, scale).")
    parser.add_argument("-m", "--method", default=None,
                        help="Correct the p-values over all queries x windows tests with this method and take the significant "
                             "windows (default: no correction, the r whose p-value is alpha is the cutoff).")
    parser.add_argument("-a", "--alpha", default=0.05, help="The p-value (corrected with -m) a window may have at most.")
    parser.add_argument("-g", "--max_gap", default=0, help="Windows below the cutoff that two windows of one hit may have between them.")
    parser.add_argument("-mw", "--min_windows", default=1, help="Hits that span fewer windows are dropped.")
    args = _parse_args_or_exit(parser)
    if args.distribution is not None and not args.params:
        parser.error("-d needs the parameters of the distribution: -p P [P ...]")
    if args.cutoff is not None and args.method is not None:
        parser.error("-m corrects p-values: it goes with -bg or -d, not with -c")
    _run_domain_hits(args.query, args.target, args.mean, args.std, int(args.kmer), int(args.window), int(args.slide), args.log2,
                     args.outfile, None if args.cutoff is None else float(args.cutoff), args.background, args.distribution,
                     args.params, args.method, float(args.alpha), int(args.max_gap), int(args.min_windows))


PAIR_KMERS_DOC = """
Description
-----------
The k-mers behind a similarity: for every pair of a pair list (what seekr_significant_pairs or seekr_nearest writes) the
k-mers whose z-score product contributes most to the pair's Pearson correlation, computed on an MI355X from the count
file(s) the list was made from.  r of a pair is the mean of these products over all k-mers.  The output is a CSV with
the columns row,col,rank,kmer,contribution,z_row,z_col: rank 0 is the largest contribution (--smallest: the most
negative one).  K-mer names come from the header of the labelled count file; with -bi they are the words over the
alphabet (-a) of length -k in counting order.

Examples
--------
    ten k-mers per significant pair:   seekr_pair_kmers counts.csv pairs.csv -t 10 -o pair_kmers.csv
    neighbours across two .npy files:  seekr_pair_kmers a.npy b.npy nearest.csv -bi -k 6 -o pair_kmers.csv
"""


def _run_pair_kmers(counts, counts2, pairs, top, outfile, binary_input, kmer, alphabet, smallest):
    import csv
    from itertools import product
    from seekr_amd import explain
    names = names2 = None
    if binary_input:
        counts = np.load(counts)
        counts2 = None if counts2 is None else np.load(counts2)
        kmers = ["".join(t) for t in product(alphabet, repeat=kmer)]
    else:
        kmers = _csv_column_labels(counts)
        counts, names = _read_labelled_csv(counts)
        counts2, names2 = (None, names) if counts2 is None else _read_labelled_csv(counts2)
    if len(kmers) != np.shape(counts)[1]:
        raise ValueError("{} k-mer names for {} columns: -k and -a must be those the counts were made with".format(
            len(kmers), np.shape(counts)[1]))
    rows, cols = explain.read_pairs_csv(pairs, names, names2)
    res = explain.pair_kmers(counts, rows, cols, counts2=counts2, top=top, largest=not smallest, kmers=kmers)
    with open(outfile, "w", newline="") as f:
        out = csv.writer(f, lineterminator="\n")
        out.writerow(["row", "col", "rank", "kmer", "contribution", "z_row", "z_col"])
        for e, words in enumerate(res.words()):
            i, j = int(rows[e]), int(cols[e])
            for t, word in enumerate(words):
                out.writerow([i if names is None else names[i], j if names2 is None else names2[j], t, word,
                              str(res.contribution[e, t]), str(res.z_row[e, t]), str(res.z_col[e, t])])


def _csv_column_labels(path):
    """The column labels of a labelled count file (its header line without the index cell)."""
    import csv
    with open(path, newline="") as f:
        return next(csv.reader(f))[1:]


def console_pair_kmers():
    parser = argparse.ArgumentParser(usage=PAIR_KMERS_DOC, formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    parser.add_argument("files", nargs="+", metavar="counts [counts2] pairs.csv",
                        help="Count file of the rows, optionally the count file of the columns, then the pair list.")
    parser.add_argument("-t", "--top", default=10, help="K-mers per pair (at most %d)." % _lib.TOPK_MERGE_KMAX)
    parser.add_argument("-o", "--outfile", default="pair_kmers.csv",
                        help="Where the list goes (CSV: row,col,rank,kmer,contribution,z_row,z_col).")
    parser.add_argument("-bi", "--binary_input", action="store_true", help="The count files are .npy, not labelled CSV.")
    parser.add_argument("-k", "--kmer", default=6, help="With -bi: the word length the counts were made with.")
    parser.add_argument("-a", "--alphabet", default="AGTC", help="With -bi: the alphabet the counts were made with.")
    parser.add_argument("--smallest", action="store_true", help="List the most negative contributions instead.")
    args = _parse_args_or_exit(parser)
    if len(args.files) not in (2, 3):
        parser.error("expected: counts [counts2] pairs.csv")
    counts, counts2, pairs = (args.files[0], None, args.files[1]) if len(args.files) == 2 else args.files
    _run_pair_kmers(counts, counts2, pairs, int(args.top), args.outfile, args.binary_input, int(args.kmer), args.alphabet,
                    args.smallest)


KMER_LEIDEN_DOC = """
Description
-----------
Leiden communities of the sequences of a FASTA file on an MI355X: k-mer counts, Pearson correlation, threshold and
partition all run on the device.  Flags are those of the reference command of the same name; the network plot is not
built (-pn is refused: write the CSV files with -cf and plot from them), the result is the same on every run (-sd is
accepted and changes nothing), and --edges nonzero writes only the kept edges.

Examples
--------
    communities at r >= 0.05, CSV files:   seekr_kmer_leiden seqs.fa mean.npy std.npy 4 -pco 0.05 -cf out
    modularity, kept edges only:           seekr_kmer_leiden seqs.fa mean.npy std.npy 6 -a ModularityVertexPartition -cf out --edges nonzero
    the strongest 0.1 %% of the pairs:     seekr_kmer_leiden seqs.fa mean.npy std.npy 6 -d 0.001 -cf out
    the union 15-nearest-neighbour graph:  seekr_kmer_leiden seqs.fa mean.npy std.npy 6 -nn 15 -cf out --edges nonzero
"""


def console_kmer_leiden():
    from seekr_amd import kmer_leiden
    parser = argparse.ArgumentParser(usage=KMER_LEIDEN_DOC, formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    parser.add_argument("fasta", help="full path of the input fasta sequence file; the headers label the nodes.")
    parser.add_argument("mean_path", help="full path to the normalization mean vector numpy file.")
    parser.add_argument("std_path", help="full path to the normalization std vector numpy file.")
    parser.add_argument("kmer", help="length of kmers, consistent with the mean and std vector files.")
    parser.add_argument("-a", "--algo", default="RBERVertexPartition",
                        choices=["ModularityVertexPartition", "RBConfigurationVertexPartition", "RBERVertexPartition", "CPMVertexPartition",
                                 "SurpriseVertexPartition", "SignificanceVertexPartition"],
                        help="the quality function the communities maximise (Surprise and Significance are not built).")
    parser.add_argument("-r", "--rs", default=1.0, help="the resolution parameter, larger value leads to more clusters.")
    parser.add_argument("-pco", "--pearsoncutoff", default=0.0, help="set to 0 pearson correlation r values that are less than the pearsoncutoff.")
    parser.add_argument("-sd", "--setseed", action="store_true", help="accepted for compatibility: the result is always reproducible.")
    parser.add_argument("-ec", "--edgecolormethod", default="gradient", choices=["gradient", "threshold"], help="plot option (the plot is not built).")
    parser.add_argument("-et", "--edgethreshold", default=0.1, help="plot option (the plot is not built).")
    parser.add_argument("-lfs", "--labelfontsize", default=12, help="plot option (the plot is not built).")
    parser.add_argument("-pn", "--plotname", default=None, help="not built: any value is refused; use --csvfile.")
    parser.add_argument("-cf", "--csvfile", default=None,
                        help="name and path of the nodes and edges csv files; _nodes_leiden.csv and _edges_leiden.csv are appended.")
    parser.add_argument("--edges", default="all", choices=["all", "nonzero"],
                        help="edges file: every upper-triangle cell, zeros included (the reference), or the kept edges only.")
    parser.add_argument("-kt", "--kmers_top", default=None,
                        help="with --csvfile: also write _kmers_leiden.csv, this many top k-mers (by mean count) per community.")
    parser.add_argument("-d", "--density", default=None,
                        help="instead of -pco: keep this fraction of the pairs, the most correlated ones (the cutoff is found on the device).")
    parser.add_argument("-nn", "--knn", default=None,
                        help="instead of -pco / -d: the graph of every sequence's this many nearest neighbours (positive r only).")
    parser.add_argument("-nm", "--knn_mode", default="union", choices=["mutual", "union"],
                        help="with -nn: keep a pair when either (union) or both (mutual) of its ends lists the other.")
    args = _parse_args_or_exit(parser)
    options = {} if args.density is None else {"density": args.density}
    if args.knn is not None:
        options.update(knn=int(args.knn), knn_mode=args.knn_mode)
    kmer_leiden.kmer_leiden(args.fasta, args.mean_path, args.std_path, int(args.kmer), args.algo, float(args.rs), float(args.pearsoncutoff),
                            args.setseed, args.edgecolormethod, float(args.edgethreshold), int(args.labelfontsize), args.plotname,
                            args.csvfile, edges=args.edges, kmers_top=None if args.kmers_top is None else int(args.kmers_top), **options)


R_DISTRIBUTION_DOC = """
Description
-----------
How the Pearson correlations of the rows of a count file are distributed, on an MI355X and without the all-pairs
matrix: a histogram, exact quantiles, and the cutoff that keeps a given fraction of the pairs.  One file: the pairs of
its rows (each once).  Two files: every row of the first against every row of the second.  The histogram goes to a CSV
file (left,right,count, then the cells below, above and NaN); quantiles and cutoffs are printed as `q,value` lines.

Examples
--------
    200 bins over [-1, 1]:                seekr_r_distribution counts.csv --bins 200 --range -1 1 -o hist.csv
    median and 99th percentile:           seekr_r_distribution counts.npy -bi -q 0.5 0.99
    the cutoff that keeps 0.1 %% of pairs: seekr_r_distribution counts.npy -bi --density 0.001
"""


def _run_r_distribution(counts, counts2, binary_input, bins, value_range, q, densities, outfile, out=None):
    import csv
    from seekr_amd import distribution
    out = sys.stdout if out is None else out
    if binary_input:
        counts = np.load(counts)
        counts2 = None if counts2 is None else np.load(counts2)
    else:
        counts = _read_labelled_csv(counts)[0]
        counts2 = None if counts2 is None else _read_labelled_csv(counts2)[0]
    res = distribution.pearson_distribution(counts, counts2, bins=bins, range=value_range, q=q, densities=densities)
    if res.hist is not None:
        with open(outfile, "w", newline="") as f:
            w = csv.writer(f, lineterminator="\n")
            w.writerow(["left", "right", "count"])
            for left, right, n in zip(res.edges[:-1], res.edges[1:], res.hist.tolist()):
                w.writerow([str(left), str(right), n])
            w.writerow(["-inf", str(res.edges[0]), res.below])
            w.writerow([str(res.edges[-1]), "inf", res.above])
            w.writerow(["nan", "nan", res.nan])
    for x, v in zip(res.q, res.quantiles):
        out.write("{},{}\n".format(x, str(v)))
    for d, v in zip(res.densities, res.cutoffs):
        out.write("density {},{}\n".format(d, str(v)))
    return res


def console_r_distribution():
    parser = argparse.ArgumentParser(usage=R_DISTRIBUTION_DOC, formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    parser.add_argument("counts", help="Count file whose pairs of rows are looked at.")
    parser.add_argument("counts2", nargs="?", default=None,
                        help="Count file whose rows those of `counts` are compared with (default: counts against itself, each pair once).")
    parser.add_argument("-bi", "--binary_input", action="store_true", help="The count files are .npy, not labelled CSV.")
    parser.add_argument("--bins", default=None, help="Equal bins of the histogram (with --range; at most 4096).")
    parser.add_argument("--range", nargs=2, default=None, metavar=("LO", "HI"), help="The histogram's first and last edge.")
    parser.add_argument("-q", "--quantiles", nargs="+", default=[], help="Quantiles in [0, 1] (decimal or a fraction such as 1/3).")
    parser.add_argument("--density", nargs="+", default=[], help="Fractions of the pairs whose cutoff is wanted.")
    parser.add_argument("-o", "--outfile", default="r_histogram.csv", help="Where the histogram goes (CSV: left,right,count).")
    args = _parse_args_or_exit(parser)
    if (args.bins is None) != (args.range is None):
        parser.error("--bins and --range go together")
    if args.bins is None and not args.quantiles and not args.density:
        parser.error("nothing asked for: give --bins with --range, -q or --density")
    _run_r_distribution(args.counts, args.counts2, args.binary_input, None if args.bins is None else int(args.bins),
                        None if args.range is None else (float(args.range[0]), float(args.range[1])), args.quantiles,
                        args.density, args.outfile)


FIND_DIST_DOC = """
Description
-----------
The background distribution of Pearson correlations: counts the k-mers of a background FASTA file on an MI355X,
draws --subset_size of the pairwise correlations of its sequences without building the all-pairs matrix, and either
writes that sample (default) or fits scipy distributions to it on the host (-fm) and writes the fits, best first.
bkg_mean_<k>mers.npy and bkg_std_<k>mers.npy are written to the working directory: seekr_find_pval takes them.  Flags
are those of the reference command of the same name; -pf draws no plot here, and 'default' as the FASTA file is refused
(the default background is not shipped).

Examples
--------
    100 000 sampled correlations:          seekr_find_dist background.fa -k 4 -sbt -sbs 100000 -o bkg_sample
    the ten common models, ranked by KS:   seekr_find_dist background.fa -k 4 -sbt -fm -o bkg_fits
    three models, ranked by AIC:           seekr_find_dist background.fa -mdl norm,gamma,lognorm -sbt -fm -statm aic -o bkg_fits
"""

FIND_PVAL_DOC = """
Description
-----------
p-values of the Pearson correlations between the sequences of two FASTA files on an MI355X, against the output of
seekr_find_dist: a CSV of fitted distributions (-ft distribution: the -bf-th is used; the ten common models have a
device cdf) or a CSV of sampled correlations (-ft npy).  The result is a labelled CSV, rows the headers of the first
file, columns those of the second.  Flags are those of the reference command of the same name.

Examples
--------
    against the best fit:      seekr_find_pval a.fa b.fa bkg_mean_4mers.npy bkg_std_4mers.npy 4 bkg_fits.csv -o pvals
    against the sample itself: seekr_find_pval a.fa b.fa bkg_mean_4mers.npy bkg_std_4mers.npy 4 bkg_sample.csv -ft npy -o pvals
"""


def console_find_dist():
    from seekr_amd import find_dist
    parser = argparse.ArgumentParser(usage=FIND_DIST_DOC, formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    parser.add_argument("fasta", help="full path of the FASTA file of background sequences.")
    parser.add_argument("-k", "--kmer", default=4, help="length of the k-mers.")
    parser.add_argument("-l", "--log2", default="Log2.post", choices=_LOG2, help="if and when the counts are log transformed.")
    parser.add_argument("-mdl", "--models", default="common10",
                        help="the models to fit: 'common10', 'all', or scipy.stats names separated by commas.")
    parser.add_argument("-sbt", "--subsetting", action="store_true", help="use a random subset of the correlations.")
    parser.add_argument("-sbs", "--subset_size", default=100000, help="size of that subset.")
    parser.add_argument("-fm", "--fit_model", action="store_true", help="fit --models to the sample (needs scipy).")
    parser.add_argument("-statm", "--statsmethod", default="ks", choices=["ks", "mse", "aic", "bic"],
                        help="how the goodness of a fit is measured; smaller is better.")
    parser.add_argument("-pb", "--progress_bar", action="store_true", help="show a progress bar over the models.")
    parser.add_argument("-pf", "--plotfit", default=None, help="accepted for compatibility: no plot is drawn.")
    parser.add_argument("-o", "--outputname", default=None, help="where the CSV goes; .csv is appended.  Omitted: nothing is saved.")
    args = _parse_args_or_exit(parser)
    models = args.models if args.models in ("common10", "all") else args.models.split(",")
    find_dist.find_dist(args.fasta, int(args.kmer), args.log2, models, args.subsetting, int(args.subset_size), args.fit_model,
                        args.statsmethod, args.progress_bar, args.plotfit, args.outputname)


def console_find_pval():
    from seekr_amd import find_dist, find_pval
    parser = argparse.ArgumentParser(usage=FIND_PVAL_DOC, formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    parser.add_argument("seq1file", help="full path of the FASTA file whose sequences label the rows.")
    parser.add_argument("seq2file", help="full path of the FASTA file whose sequences label the columns (may be the same file).")
    parser.add_argument("mean_path", help="full path to the normalization mean vector numpy file.")
    parser.add_argument("std_path", help="full path to the normalization std vector numpy file.")
    parser.add_argument("kmer", help="length of the k-mers, consistent with the mean and std vector files.")
    parser.add_argument("fitres_file", help="the CSV file seekr_find_dist wrote: fitted distributions or sampled correlations.")
    parser.add_argument("-ft", "--fitres_type", default="distribution", choices=["distribution", "npy"],
                        help="what fitres_file holds.")
    parser.add_argument("-l", "--log2", default="Log2.post", choices=_LOG2, help="if and when the counts are log transformed.")
    parser.add_argument("-bf", "--bestfit", default=1, help="which of the fitted distributions to use, counted from 1.")
    parser.add_argument("-o", "--outputname", default=None, help="where the CSV goes; .csv is appended.  Omitted: nothing is saved.")
    parser.add_argument("-pb", "--progress_bar", action="store_true", help="accepted for compatibility: there is no loop to show.")
    args = _parse_args_or_exit(parser)
    if args.fitres_type == "distribution":
        fitres = find_dist.read_fit_csv(args.fitres_file)
    else:
        fitres = np.loadtxt(args.fitres_file, delimiter=",")
    find_pval.find_pval(args.seq1file, args.seq2file, args.mean_path, args.std_path, int(args.kmer), fitres, args.log2,
                        int(args.bestfit), args.outputname, args.progress_bar)
