"""Cases of the window sweep (tests/test_gpu_window_sweep.py, tests/test_window_sweep_cpu.py) — test infrastructure.

count_windows_kernel (csrc/windows.hip; its sweep is sweep_pair of csrc/count_bins.hpp) has a fast branch for sweeps in which every lane of the workgroup holds 16 whole
k-mers of an all-alphabet sequence, and inside it an aggregated arm for sweeps whose 64 lanes hold the same 32 bases
(homopolymers, repeats whose period divides 16).  The cases here are built to reach them: windows of one and two full
sweeps, repeats of every such period with controls, bins that end at exactly 65 535 and 65 536, one N at every phase, runs
of rows over a ragged table, and FASTA targets whose windows route `domain_pearson`'s chunks differently.

The rule of tests/windows_cases.py holds: nothing here imports the package under test; what a case expects comes from
explicit substrings and the oracle (windows_cases.substrings / expected_u32 / expected_per_kb, oracle.seekr_oracle)."""
import functools

import numpy as np

import windows_cases as wc
from oracle import seekr_oracle as orc

ALPHABET = "AGTC"  # codes A0 G1 T2 C3: k-mers that start with T or C live in the upper 16-bit half of a bin word
SWEEP_KS = (1, 3, 6, 7)


def threads(k):
    """Threads of the workgroup that owns a row: one wave at k <= 6, four at k = 7."""
    return 64 if k <= 6 else 256


def sweep_bases(k):
    """S: the bases of one full sweep — every lane of the workgroup holds 16 whole k-mers."""
    return 16 * threads(k) + k - 1


def fast_sweeps(window, k):
    """How many sweeps of a full window of an all-alphabet sequence take the fast branch (count_bins.hpp: the `whole` arm of sweep_pair)."""
    return max(window - k + 1, 0) // (16 * threads(k))


def homopolymer_column(letter, k):
    return ALPHABET.index(letter) * (4 ** k - 1) // 3


def _seq(seed, length):
    return wc.random_seq(np.random.default_rng(seed), length)


# ---------------------------------------------------------------------------------------------------------------------
# full sweeps on random text
# ---------------------------------------------------------------------------------------------------------------------
SWEEP_SLIDES = (1, 7, 16)


def sweep_windows(k):
    """The last window that takes only the slow branch, the first with one fast sweep, one more base, and the same around
    two fast sweeps plus a partial one."""
    S = sweep_bases(k)
    return (S - 1, S, S + 1, 2 * S - 1, 2 * S, 2 * S + 17)


def sweep_case(k, window, slide):
    return [_seq(100_000 * k + 10 * window + slide, window + 40)], k, window, slide


# ---------------------------------------------------------------------------------------------------------------------
# repeats, each with a control
# ---------------------------------------------------------------------------------------------------------------------
REPEAT_UNITS = (("A", 1), ("G", 1), ("T", 1), ("C", 1),                    # homopolymers: lower, lower, upper, upper half
                ("AG", 2), ("TC", 2), ("GT", 2),                          # period 2: lower only, upper only, both halves
                ("AGTC", 4), ("AAGTCCTG", 8), ("AGTCCTGAATTGCCGA", 16),   # periods that divide 16: all lanes alike
                ("AGT", 3), ("AGTCC", 5))                                 # controls: the lanes differ
REPEAT_SLIDES = (1, 16)
MIXED, WITH_N = "T*1.5 sweeps + random", "GT with one N"


def repeat_window(k):
    return 2 * sweep_bases(k) + 5


def repeat_case(k, slide):
    """(names, (seqs, k, window, slide)): every unit repeated over window + 17 bases; one row of 1.5 sweeps of T followed by
    random text (aggregated arm, plain arm and partial sweep in one row; at k = 7 two of the four waves of the second sweep
    aggregate and two do not); the GT repeat once more with a single N, which sends the same text down the masked branch."""
    window = repeat_window(k)
    L = window + 17
    names = [u for u, _ in REPEAT_UNITS]
    seqs = [(u * (L // len(u) + 1))[:L] for u in names]
    run = 24 * threads(k)
    seqs.append("T" * run + _seq(7000 + k, L - run))
    gt = list(seqs[names.index("GT")])
    gt[24 * threads(k)] = "N"
    seqs.append("".join(gt))
    return names + [MIXED, WITH_N], (seqs, k, window, slide)


def packed_words(seq, start, n_lanes):
    """numpy restatement of the 2-bit packing as a lane sees it: the 32 bases from start + 16 * lane, first base in the top
    bits, as one uint64 per lane."""
    codes = np.array([ALPHABET.index(c) for c in seq[start:start + 16 * n_lanes + 16]], dtype=np.uint64)
    out = np.zeros(n_lanes, dtype=np.uint64)
    for lane in range(n_lanes):
        for c in codes[16 * lane:16 * lane + 32]:
            out[lane] = (out[lane] << np.uint64(2)) | c
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the 65 535 edge
# ---------------------------------------------------------------------------------------------------------------------
EDGE_CASES = [(k, n, letter) for k in (1, 6) for n in (65535, 65536) for letter in ("T", "A")] + [(7, 65536, "T")]


def edge_case(k, n_kmers, letter):
    """A homopolymer window of exactly n_kmers k-mers (65 535: the last of the 16-bit bins; 65 536: the first of the 32-bit
    ones), then 40 random bases: three rows at slide 20."""
    window = n_kmers + k - 1
    return [letter * window + _seq(65 + k, 40)], k, window, 20


# ---------------------------------------------------------------------------------------------------------------------
# one N at every phase
# ---------------------------------------------------------------------------------------------------------------------
N_KS = (3, 7)


def n_phase_case(k):
    """Window 44, slide 1, the N at base 60 of 120: it takes every position of a window, and the window every start & 31."""
    s = list(_seq(300 + k, 120))
    s[60] = "N"
    return ["".join(s)], k, 44, 1


def n_sweep_positions(k):
    """Bases 15, 16 and 17 of lane 5's 16-base group; the last base of the first sweep and the first of the second."""
    return (5 * 16 + 15, 5 * 16 + 16, 5 * 16 + 17, 16 * threads(k) - 1, 16 * threads(k))


def n_sweep_case(k):
    window = sweep_bases(k) + 40
    seqs = []
    for i, p in enumerate(n_sweep_positions(k)):
        s = list(_seq(400 + 10 * k + i, window + 21))
        s[p] = "N"
        seqs.append("".join(s))
    return seqs, k, window, 7


def kmers_in_row(seq, start, length, k):
    """k-mers of the window seq[start : start + length] that do not cover a letter outside the alphabet — from positions
    alone: W minus the k-mers p with start + p <= n <= start + p + k - 1, for the one N of the sequence at n."""
    W = max(length - k + 1, 0)
    n = seq.index("N") - start
    lo, hi = max(n - k + 1, 0), min(n, W - 1)
    return W - max(hi - lo + 1, 0)


# ---------------------------------------------------------------------------------------------------------------------
# runs over a table of many sequences
# ---------------------------------------------------------------------------------------------------------------------
TABLE_K, TABLE_WINDOW, TABLE_SLIDE = 4, 64, 9
TABLE_RUNS = (1, 2, 5, 37)


def table_case():
    """40 sequences of 1 to 300 letters, none of which has a window of k - 1 letters: lengths below k, the window's own
    length, lengths of exactly one row and of exactly two."""
    rng = np.random.default_rng(40)
    lengths = [1, 2, 64, 63, 65, 73, 74, 300, 4, 5]
    while len(lengths) < 40:
        L = int(rng.integers(1, 301))
        if L != TABLE_K - 1:
            lengths.append(L)
    order = rng.permutation(40)
    seqs = [wc.random_seq(rng, lengths[i], "ACGT" if i % 4 else "ACGTACGTN") for i in order]
    return seqs, TABLE_K, TABLE_WINDOW, TABLE_SLIDE


def table_case_with_zero_division():
    """The same table with a sequence of k - 1 letters (its one window is its tail) in the middle: (case, its row)."""
    seqs, k, window, slide = table_case()
    seqs = seqs[:20] + ["ACG"] + seqs[20:]
    table = wc.substrings(seqs, window, slide)[1]
    (row,) = np.nonzero(table[:, 0] == 20)[0]
    return (seqs, k, window, slide), int(row)


def row_begin(seqs, window, slide):
    table = wc.substrings(seqs, window, slide)[1]
    return np.concatenate([[0], np.cumsum(np.bincount(table[:, 0], minlength=len(seqs)))]).astype(np.int64)


def boundary_runs(rb):
    """(first_row, n_rows) of runs that begin and end exactly on the values of row_begin: every sequence alone, everything
    before it, everything from it on."""
    total = int(rb[-1])
    runs = set()
    for i in range(len(rb) - 1):
        runs |= {(int(rb[i]), int(rb[i + 1] - rb[i])), (0, int(rb[i])), (int(rb[i]), total - int(rb[i]))}
    return sorted(r for r in runs if r[1] > 0)


# ---------------------------------------------------------------------------------------------------------------------
# domain_pearson on structured targets
# ---------------------------------------------------------------------------------------------------------------------
DP_WINDOW, DP_SLIDE = 500, 50
DP_CHUNKS = (16, 50)  # and n + 7: one chunk
DP_MODES = [(5, "Log2.post"), (6, "Log2.post"), (7, "Log2.post"), (6, "Log2.pre"), (6, "Log2.none")]
ROUTE_SHARE, SPLIT_SHARE = 1.0 / 8, 1.0 / 32  # the fill's threshold is 1/16: a factor of two clear of it on either side

# the long record, (kind, bases): with slide 50 rows 0-49 and 100-149 lie in random text, 53-85 touch the A run, 151-183 the
# GT run, and the N run (windows 186-195 lie wholly inside it) shares the last chunk of 50 with the GT run
DP_LAYOUT = (("random", 3100), ("A", 1200), ("random", 3700), ("GT", 1200), ("random", 70), ("N", 1010), ("random", 20))
NAN_LAYOUT = (("random", 1500), ("A", 1200), ("random", 800), ("GT", 1200), ("random", 500), ("N", 300), ("random", 700))


def energy_share(tn):
    """max z^2 / K per row of the row-standardised rows, in float64: the share of a row's energy that its largest column
    carries (operand.hip: row_needs_fp32 asks for 1/16)."""
    x = np.asarray(tn, dtype=np.float64)
    with np.errstate(all="ignore"):
        z = (x - x.mean(axis=1, keepdims=True)) / x.std(axis=1, keepdims=True)
        return (z * z).max(axis=1) / x.shape[1]


def long_record(rng, layout):
    parts = []
    for kind, n in layout:
        parts.append(wc.random_seq(rng, n) if kind == "random" else (kind * n)[:n])
    return "".join(parts)


def chunks_of(n_rows, chunk_rows):
    return [(r0, min(chunk_rows, n_rows - r0)) for r0 in range(0, n_rows, chunk_rows)]


def predicted_routes(share, chunk_rows):
    """Per chunk: 'fp32' (a row at share >= 1/8), 'split' (every row below 1/32) or None (not asserted)."""
    out = []
    for r0, n in chunks_of(len(share), chunk_rows):
        s = share[r0:r0 + n]
        out.append("fp32" if np.nanmax(s) >= ROUTE_SHARE else ("split" if np.all(s < SPLIT_SHARE) else None))
    return out


@functools.lru_cache(maxsize=None)
def background(k, log2):
    """mean and std of 150 random 2 kb sequences through the oracle, as dp_case of test_gpu_windows.py makes them."""
    rng = np.random.default_rng(500 + k)
    return orc.get_counts([wc.random_seq(rng, 2000) for _ in range(150)], k=k, log2=log2)[1:]


def repeat_queries(rng):
    """One query that is mostly an A run and one that is mostly GT: their own rows route to float32."""
    return [wc.random_seq(rng, 60) + "A" * 1900 + wc.random_seq(rng, 40), "GT" * 900 + wc.random_seq(rng, 60)]


def _domain(k, log2, layout, mean, std, last_letters):
    rng = np.random.default_rng(906 + k)  # k = 6: a record whose random windows stay below 1/32 in every log2 mode
    records = [long_record(rng, layout), wc.random_seq(rng, 300), wc.random_seq(rng, last_letters)]
    queries = [wc.random_seq(rng, L) for L in (400, 650, 1000, 1500, 2100)] + repeat_queries(rng)
    subs, table = wc.substrings(records, DP_WINDOW, DP_SLIDE)
    qn = orc.get_counts(queries, k=k, mean=mean, std=std, log2=log2)[0]
    tn = orc.get_counts(subs, k=k, mean=mean, std=std, log2=log2)[0]
    return dict(k=k, log2=log2, mean=mean, std=std, records=records, names=["long", "short", "tiny"], queries=queries, subs=subs,
                table=table, qn=qn, tn=tn, ref=orc.pearson(qn, tn), truth=orc.pearson_f64_truth(qn, tn),
                share=energy_share(tn), qshare=energy_share(qn))


@functools.lru_cache(maxsize=None)
def domain_case(k, log2):
    """Three records (the long one of DP_LAYOUT, one shorter than the window, one of k - 2 letters), seven queries (five random:
    set (a); all seven: set (b)), background vectors, the oracle's rows, r and energy shares — computed once and left
    unchanged."""
    mean, std = background(k, log2)
    return _domain(k, log2, DP_LAYOUT, mean, std, k - 2)


def query_set(case, which):
    """The case restricted to query set 'a' (the five random queries) or 'b' (all seven)."""
    n = 5 if which == "a" else 7
    return dict(case, queries=case["queries"][:n], qn=case["qn"][:n], ref=case["ref"][:n], truth=case["truth"][:n],
                qshare=case["qshare"][:n])


@functools.lru_cache(maxsize=None)
def nan_case(k, log2):
    """mean = 0 and std = 1: the window of the k - 2 letter record is a constant row, r is NaN in its column.  The N run is
    shorter than a window here, so that no other window is constant."""
    return _domain(k, log2, NAN_LAYOUT, np.zeros(4 ** k, np.float32), np.ones(4 ** k, np.float32), k - 2)


def zero_division_records(k):
    """A target whose LAST record has k - 1 letters: the failing row is the last row of the last chunk."""
    rng = np.random.default_rng(950 + k)
    return [long_record(rng, NAN_LAYOUT), wc.random_seq(rng, 300), wc.random_seq(rng, k - 1)]
