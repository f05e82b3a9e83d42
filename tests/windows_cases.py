"""What the window tests expect — test infrastructure.  The specification of seekr_amd.windows is an equivalence: the row
of a window is the row the reference gives for the window's SUBSTRING.  So the expectation is made here from explicit
substrings, cut by Python slicing in a plain loop, and from the oracle alone (oracle.seekr_oracle, oracle.c_oracle):
nothing in this file imports the package under test."""
import numpy as np

from oracle import c_oracle
from oracle import seekr_oracle as orc

RTOL, ATOL_LOG, ATOL_POST = 1e-5, 1e-6, 2e-6  # the bars of tests/test_gpu_parity.py: log2 outputs, normalised counts


def substrings(seqs, window, slide):
    """(substrings, table) of the sliding windows, sequence by sequence and start by start; table rows are
    (seq_index, start, length)."""
    subs, table = [], []
    for i, seq in enumerate(seqs):
        start = 0
        while True:
            piece = seq[start:start + window]
            subs.append(piece)
            table.append((i, start, len(piece)))
            if start + window >= len(seq):
                break
            start += slide
    return subs, np.asarray(table, dtype=np.int64).reshape(-1, 3)


def has_zero_division(subs, k):
    """Does the reference raise ZeroDivisionError for one of these sequences (kmer_counts.py:144: len == k - 1)?"""
    return any(len(s) == k - 1 for s in subs)


def expected_u32(subs, k):
    blob, offsets = c_oracle.seqs_to_blob(subs)
    return c_oracle.count_u32(blob, offsets, k)


def expected_per_kb(subs, k, log2_pre=False):
    """float32 per-kb rows of the substrings as the oracle counts them; log2_pre: np.log2(x + 1) on top."""
    x = c_oracle.per_kb_f32(expected_u32(subs, k), [len(s) for s in subs], k)
    return orc.log2_plus_one(x) if log2_pre else x


def random_seq(rng, length, letters="ACGT"):
    return "".join(np.asarray(list(letters))[rng.integers(0, len(letters), size=length)])
