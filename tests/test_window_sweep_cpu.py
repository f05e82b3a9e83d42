"""The generators of the window sweep (tests/window_sweep_cases.py) pinned without a GPU: that the cases reach the branches
of count_windows_kernel and the routes of domain_pearson they were made for is a property of the inputs, checked here."""
import os

import numpy as np
import pytest

import window_sweep_cases as sc
import windows_cases as wc
from oracle import seekr_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def counting_cases():
    for k in sc.SWEEP_KS:
        for window in sc.sweep_windows(k):
            yield sc.sweep_case(k, window, 7)
        yield sc.repeat_case(k, 16)[1]
    for k in sc.N_KS:
        yield sc.n_phase_case(k)
        yield sc.n_sweep_case(k)
    yield sc.edge_case(1, 65535, "T")
    yield sc.table_case()


def test_expected_rows_come_from_the_oracle_on_explicit_substrings():
    src = open(os.path.join(ROOT, "tests", "window_sweep_cases.py")).read().split('"""', 2)[2]
    assert "seekr_amd" not in src and "import windows_cases as wc" in src and "from oracle import seekr_oracle" in src
    for seqs, k, window, slide in counting_cases():
        subs, table = wc.substrings(seqs, window, slide)
        assert [seqs[i][s:s + window] for i, s, _ in table] == subs and all(len(p) == n for p, n in zip(subs, table[:, 2]))
        rows = list(range(0, len(subs), max(1, len(subs) // 3)))  # the slow structure-faithful loop on a few rows of each
        few = [subs[r] for r in rows]
        assert np.array_equal(wc.expected_u32(few, k), orc.count_kmers_u32(few, k))
        if not wc.has_zero_division(few, k):
            assert np.array_equal(wc.expected_per_kb(few, k).view(np.uint32), orc.raw_counts(few, k).view(np.uint32))


@pytest.mark.parametrize("k", sc.SWEEP_KS)
def test_full_sweep_windows_reach_the_fast_branch_and_their_controls_do_not(k):
    S, T = sc.sweep_bases(k), sc.threads(k)
    assert S == (1024 if k <= 6 else 4096) + k - 1
    want = dict(zip(sc.sweep_windows(k), (0, 1, 1, 1 if k == 1 else 2, 2, 2)))  # 2S - 1 bases are 32 T + k - 2 k-mers
    for window, n_fast in want.items():
        W = window - k + 1
        taken = [W - ((base + T - 1) << 4) >= 16 for base in range(0, (W + 15) >> 4, T)]  # the kernel's loop and its condition
        assert (W >= 16 * T) == (n_fast > 0) and sc.fast_sweeps(window, k) == n_fast == sum(taken)
        assert taken == sorted(taken, reverse=True) and (not taken[-1] or W % (16 * T) == 0)
        for slide in sc.SWEEP_SLIDES:
            seqs, _, _, _ = sc.sweep_case(k, window, slide)
            assert len(seqs[0]) == window + 40 and set(seqs[0]) <= set("ACGT")  # no letter outside the alphabet: no mask
            table = wc.substrings(seqs, window, slide)[1]
            assert (table[:-1, 2] == window).all() and len(table) >= 4  # only the tail window may be shorter
            if slide == 1:
                assert set((table[:, 1] % 16).tolist()) == set(range(16))
    assert want[S - 1] == 0 and S - 1 - k + 1 == 16 * T - 1  # the control misses the branch by one k-mer
    assert sc.sweep_windows(k)[5] - k + 1 == 32 * T + 17 + k - 1  # two fast sweeps and a partial one
    assert sc.fast_sweeps(sc.repeat_window(k), k) == 2 and sc.fast_sweeps(sc.sweep_bases(k) + 40, k) == 1


@pytest.mark.parametrize("k", sc.SWEEP_KS)
def test_repeats_give_every_lane_the_same_words_and_the_controls_do_not(k):
    names, (seqs, _, window, slide) = sc.repeat_case(k, 16)
    T = sc.threads(k)
    assert len(names) == len(seqs) == len(sc.REPEAT_UNITS) + 2 and all(len(s) == window + 17 for s in seqs)
    halves = {}
    for (unit, period), seq in zip(sc.REPEAT_UNITS, seqs):
        assert seq == (unit * len(seq))[:len(seq)]
        assert all(seq[:64] != (seq[:p] * 64)[:64] for p in range(1, period))  # `period` is the shortest one
        for start in (s for s in (0, 1, 5, 16, 17) if s + 32 * T + 16 <= len(seq)):  # rows of slide 1 and 16 whose words lie in the text
            for sweep in range(2):
                words = sc.packed_words(seq, start + sweep * 16 * T, T).reshape(-1, 64)  # wave by wave
                alike = bool((words == words[:, :1]).all())
                assert alike == (16 % period == 0), (unit, start, sweep)
        halves[unit] = {sc.ALPHABET.index(seq[p]) >> 1 for p in range(len(seq) - k + 1)}  # top bit of the k-mer's first letter
    assert halves["A"] == halves["G"] == halves["AG"] == {0} and halves["T"] == halves["C"] == halves["TC"] == {1}
    assert all(halves[u] == {0, 1} for u in ("GT", "AGTC", "AAGTCCTG", "AGTCCTGAATTGCCGA"))
    # the mixed row: the first sweep all T, the second half T and half random (at k = 7 its first two waves all T)
    mixed = seqs[names.index(sc.MIXED)]
    first, second = sc.packed_words(mixed, 0, T), sc.packed_words(mixed, 16 * T, T).reshape(-1, 64)
    assert (first == first[0]).all() and not (second[-1] == second[-1, 0]).all() and len(set(mixed)) == 4
    assert (second[0] == second[0, 0]).all() == (k == 7)
    # the row with the N: the same text as the GT repeat but for one letter, which lies in the second sweep of every row
    with_n, gt = seqs[names.index(sc.WITH_N)], seqs[names.index("GT")]
    assert with_n.count("N") == 1 and sum(a != b for a, b in zip(with_n, gt)) == 1
    assert 16 * T + 17 <= with_n.index("N") < 32 * T


def test_edge_cases_end_at_65535_and_65536():
    assert {(k, n) for k, n, _ in sc.EDGE_CASES} == {(1, 65535), (1, 65536), (6, 65535), (6, 65536), (7, 65536)}
    for k, n, letter in sc.EDGE_CASES:
        seqs, _, window, slide = sc.edge_case(k, n, letter)
        assert window - k + 1 == n and (window - k + 1 > 65535) == (n == 65536)  # the switch of windows.hip
        subs, _ = wc.substrings(seqs, window, slide)
        assert len(subs) == 3 and subs[0] == letter * window and all(len(s) == window for s in subs)
        col, half = sc.homopolymer_column(letter, k), 4 ** k // 2
        assert (col >= half) == (letter == "T")
    u = wc.expected_u32(wc.substrings(*[sc.edge_case(6, 65535, "T")[i] for i in (0, 2, 3)])[0], 6)
    col = sc.homopolymer_column("T", 6)
    assert u[0, col] == 65535 and u[0].sum() == 65535 and u[1, col] >= 65515 and u[1].sum() == 65535


@pytest.mark.parametrize("k", sc.N_KS)
def test_one_n_takes_every_phase(k):
    seqs, _, window, slide = sc.n_phase_case(k)
    table = wc.substrings(seqs, window, slide)[1]
    n = seqs[0].index("N")
    inside = [(n - s) for _, s, L in table if s <= n < s + L]
    assert sorted(inside) == list(range(window)) and set((table[:, 1] % 32).tolist()) == set(range(32))
    T = sc.threads(k)
    seqs, _, window, slide = sc.n_sweep_case(k)
    assert [s.index("N") for s in seqs] == [95, 96, 97, 16 * T - 1, 16 * T] and all(s.count("N") == 1 for s in seqs)
    assert sc.fast_sweeps(window, k) == 1  # the same window on clean text would take the fast branch
    for case in (sc.n_phase_case(k), sc.n_sweep_case(k)):
        seqs, _, window, slide = case
        subs, table = wc.substrings(seqs, window, slide)
        sums = [sc.kmers_in_row(seqs[i], s, L, k) for i, s, L in table]
        assert wc.expected_u32(subs, k).sum(axis=1).tolist() == sums
        assert min(sums) == window - k + 1 - k and max(sums) <= window - k + 1


def test_table_of_many_sequences():
    seqs, k, window, slide = sc.table_case()
    lengths = [len(s) for s in seqs]
    assert len(seqs) == 40 and min(lengths) == 1 and max(lengths) == 300 and k - 1 not in lengths
    assert {1, 2, window, window - 1, window + 1, window + slide} <= set(lengths)
    subs, table = wc.substrings(seqs, window, slide)
    assert not wc.has_zero_division(subs, k) and 100 < len(subs) < 1000
    rb = sc.row_begin(seqs, window, slide)
    assert rb[0] == 0 and rb[-1] == len(subs) and (np.diff(rb) >= 1).all() and (np.diff(rb) == 1).sum() >= 5
    assert all(table[rb[i], 1] == 0 and table[rb[i], 0] == i for i in range(40))
    runs = sc.boundary_runs(rb)
    assert all(r0 in rb and r0 + n in rb for r0, n in runs) and len(runs) > 100
    (seqs2, _, _, _), bad = sc.table_case_with_zero_division()
    subs2, table2 = wc.substrings(seqs2, window, slide)
    assert [i for i, s in enumerate(subs2) if len(s) == k - 1] == [bad] and subs2[bad] == "ACG" and 0 < bad < len(subs2) - 1


@pytest.mark.parametrize("k,log2", sc.DP_MODES)
def test_domain_cases_have_the_energy_shares_the_route_assertions_need(k, log2):
    case = sc.domain_case(k, log2)
    records, share, n = case["records"], case["share"], len(case["table"])
    assert [len(r) < sc.DP_WINDOW for r in records] == [False, True, True] and len(records[2]) == k - 2
    assert 100 <= n <= 200 and n % 50 and n % 16 and len(share) == n
    # windows wholly inside a run, and windows wholly in random text
    pos, inside = 0, {}
    for kind, length in sc.DP_LAYOUT:
        assert kind == "random" or length > 2 * sc.DP_WINDOW
        rows = [r for r, (i, s, L) in enumerate(case["table"]) if i == 0 and pos <= s and s + L <= pos + length]
        inside.setdefault(kind, []).extend(rows)
        pos += length
    assert all(len(inside[kind]) >= 10 for kind in ("A", "GT", "N"))
    assert share[inside["A"]].min() >= sc.ROUTE_SHARE and share[inside["GT"]].min() >= sc.ROUTE_SHARE
    assert share[inside["random"]].max() < sc.SPLIT_SHARE and len(inside["random"]) >= 100
    assert set(case["subs"][r] for r in inside["N"]) == {"N" * sc.DP_WINDOW}
    # queries: the five random ones stay split, the two repeat queries route on their own
    assert case["qshare"][:5].max() < sc.SPLIT_SHARE and case["qshare"][5:].min() >= sc.ROUTE_SHARE
    assert case["ref"][5:].max(axis=1).min() > 0.6  # and they meet the target's own runs
    # chunks: enough of each asserted kind, both kinds in one call, a split chunk after a full-size chunk that routed
    for chunk_rows in sc.DP_CHUNKS:
        routes = sc.predicted_routes(share, chunk_rows)
        sizes = [c[1] for c in sc.chunks_of(n, chunk_rows)]
        assert routes.count("fp32") >= 2 and routes.count("split") >= 2 and sizes[-1] < chunk_rows
        first_routed = min(i for i, (r, s) in enumerate(zip(routes, sizes)) if r == "fp32" and s == chunk_rows)
        assert "split" in routes[first_routed + 1:]
    assert sc.predicted_routes(share, n + 7) == ["fp32"]
    assert np.isfinite(case["ref"]).all() and np.isfinite(case["truth"]).all()


@pytest.mark.parametrize("log2", ["Log2.post", "Log2.pre", "Log2.none"])
def test_nan_case_has_its_one_column(log2):
    case = sc.nan_case(6, log2)
    n = len(case["table"])
    assert (case["mean"] == 0).all() and (case["std"] == 1).all() and len(case["records"][2]) == 4
    assert np.array_equal(np.isnan(case["ref"]), np.arange(n)[None, :] == n - 1 + np.zeros((7, 1), dtype=int))
    assert np.isfinite(case["ref"][:, :n - 1]).all() and np.isfinite(case["truth"][:, :n - 1]).all()
    assert np.ptp(case["tn"][n - 1]) == 0 and all(np.ptp(row) > 0 for row in case["tn"][:n - 1])
    assert n % 16  # the NaN row lies in a tail chunk of 16
    records = sc.zero_division_records(6)
    subs = wc.substrings(records, sc.DP_WINDOW, sc.DP_SLIDE)[0]
    assert [len(s) == 5 for s in subs] == [False] * (len(subs) - 1) + [True] and len(subs) % 16
