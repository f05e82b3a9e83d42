"""tools/count_value_sweep.py without a device: count.hip's per_kb_value restated in numpy against the running sum the
reference computes (kmer_counts.py:144-150), exhaustively where count_rows_kernel's own flush can be, and at every window
count of tests/golden/count_value_pairs.json; the fixture recomputed from scratch; the sequences the sweep builds."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import count_value_sweep as sweep  # noqa: E402

CLASSES = ("mismatch", "guard_only", "small_n", "control")


def python_loop(n, W):
    """kmer_counts.py:144-150 as written: n additions of 1000 / W to a float, stored into a float32 row."""
    inc, acc = 1000 / W, 0
    for _ in range(n):
        acc += inc
    return np.float32(acc)


def test_cumsum_is_the_reference_loop():
    for n, W in ((0, 20), (1, 20), (3, 7), (19, 20), (8192, 8192), (35604, 35747), (25486, 63551), (10, 70000)):
        acc = 0.0
        for _ in range(n):
            acc += 1000 / W
        assert sweep.running_sums(W)[n] == acc, (n, W)
        assert sweep.expected_bits(n, W) == int(python_loop(n, W).view(np.uint32)), (n, W)


def test_no_guard_fire_and_no_mismatch_up_to_8200_windows():
    """An item of count_rows_kernel has at most 8 192 windows: its flush never replays, and never needs to."""
    for W in range(4, 8201):
        n, fire, differ = sweep.scan_w(W)
        assert not fire.any() and not differ.any(), W


def test_model_is_the_running_sum_at_every_window_count_of_the_fixture():
    """No mismatch escapes the slack test at any n <= W, for every W the fixture names; the model (product, or the replayed
    sum where the test fires) is the reference's value everywhere."""
    seen = 0
    for W in sorted({W for _, W, _ in sweep.pairs(*CLASSES)}):
        sums = sweep.running_sums(W)
        for lo in range(0, W + 1, 1 << 22):
            n = np.arange(lo, min(lo + (1 << 22), W + 1), dtype=np.int64)
            got, fire = sweep.per_kb_model(n, W, sums)  # the product, or the replayed sum where the slack test fires
            want = sums[n].astype(np.float32)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), W
            differ = (n.astype(np.float64) * (1000.0 / W)).astype(np.float32) != want
            assert not (differ & ~fire).any() and not fire[n <= 3].any()
            assert not differ[n < sweep.TAB_SIZE].any(), W  # no entry of the kernels' tables needs the replay
            seen += int(differ.sum())
    assert seen >= len(sweep.pairs("mismatch"))


def test_fixture_pairs_recomputed_from_scratch():
    for name in CLASSES:
        for n, W, want_bits in sweep.pairs(name):
            assert 0 <= n <= W
            assert want_bits == sweep.expected_bits(n, W), (name, n, W)
            kind = sweep.classify(n, W)
            if name == "mismatch":
                assert kind == "mismatch", (n, W)
                product = np.float32(np.float64(n) * (1000.0 / W))
                assert int(product.view(np.uint32)) != want_bits
            elif name in ("guard_only", "small_n"):
                assert kind == "guard_only", (name, n, W)
    for n, W, want_bits in sweep.pairs("mismatch")[:3] + sweep.pairs("control"):
        assert want_bits == int(python_loop(n, W).view(np.uint32)), (n, W)


def test_fixture_pools():
    mismatch = [(n, W) for n, W, _ in sweep.pairs("mismatch")]
    assert len([p for p in mismatch if p[1] <= 70_000]) >= 48
    assert {(35604, 35747), (25486, 63551)} <= set(mismatch)
    assert min(W for _, W in mismatch) == 35747 and min(n for n, _ in mismatch) == 25486
    assert len([p for p in mismatch if 100_000 <= p[1] <= 300_000]) >= 12
    assert [p for p in mismatch if p[1] == sweep.W_BIG] and max(W for _, W in mismatch) == sweep.W_BIG
    guard_only = [(n, W) for n, W, _ in sweep.pairs("guard_only")]
    assert len(guard_only) >= 48 and min(W for _, W in guard_only) == 16681
    small_n = [(n, W) for n, W, _ in sweep.pairs("small_n")]
    assert len(small_n) == 2 and all(n == 10 and W <= 30_000_000 for n, W in small_n)
    control = {(n, W) for n, W, _ in sweep.pairs("control")}
    assert control == {(n, W) for W in (20, 1000, 8191, 8192, 8193, 40000) for n in (0, 1, 2, 3, 4, 15, 16, 17, W - 1, W)}
    # what the sites take from the pools
    assert all(W > sweep.ITEM_WINDOWS for _, W in mismatch + guard_only + small_n)
    assert len(sweep.global_pairs()) <= 24
    kinds = [sweep.classify(n, W) for n, W, _ in sweep.global_pairs()]
    assert kinds.count("mismatch") >= 10 and kinds.count("guard_only") >= 10
    assert [W for _, W, _ in sweep.long_pairs(3) if W == sweep.W_BIG] and not [W for _, W, _ in sweep.long_pairs(7) if W == sweep.W_BIG]


SITES = list(dict.fromkeys([("AGTC", k) for k in (1, 3, 6, 7, 8, 9)] + list(sweep.GEN_FAST) + [sweep.GEN_SLOW, sweep.GEN_RANGES, sweep.GEN_HBM]))


@pytest.mark.parametrize("alphabet,k", SITES)
def test_sequences_hold_the_count_and_the_windows(alphabet, k):
    from oracle import c_oracle as co
    wide = len(alphabet) ** k > 70_000
    ps = sweep.some(sweep.upto(sweep.pairs("mismatch"), 70_000), 3 if wide else 6) + sweep.some(sweep.pairs("guard_only"), 2)
    ps += [p for p in sweep.pairs("control") if p[1] in ((20, 8193) if wide else (20, 8192, 8193, 40000))]
    for placement in sweep.PLACEMENTS:
        for last in (False, True):
            seqs = [sweep.build_sequence(n, W, alphabet, k, placement, last, seed=1) for n, W, _ in ps]
            run_letter = ord(alphabet[-1] if last else alphabet[0])
            for (n, W, _), s in zip(ps, seqs):
                assert len(s) == W + k - 1 and set(np.unique(s)) <= set(alphabet.encode())
                at = sweep.run_start(n, W, k, placement)
                run = n + k - 1 if n else 0
                assert (s[at:at + run] == run_letter).all() and (s == run_letter).sum() == run
                if placement == "middle" and 0 < n < W:
                    assert at > 0
                    if n >= 2 and W - n >= sweep.ITEM_WINDOWS:  # the run's windows lie across a tile boundary
                        assert at // sweep.ITEM_WINDOWS != (at + n - 1) // sweep.ITEM_WINDOWS
            offsets = np.concatenate([[0], np.cumsum([len(s) for s in seqs])])
            counts = co.count_u32(np.concatenate(seqs), offsets, k, alphabet)
            assert np.array_equal(counts[:, sweep.target_bin(alphabet, k, last)], [n for n, _, _ in ps])
            assert np.array_equal(counts.sum(axis=1), [W for _, W, _ in ps])  # every window is counted: W of them
    blob, offsets, targets = sweep.build_set(ps, alphabet, k)
    assert len(offsets) == len(ps) + 1 and set(targets) == {0, len(alphabet) ** k - 1}


def test_one_letter_alphabet_is_used_for_homopolymers_only():
    alphabet, k = sweep.GEN_ONE_LETTER
    assert len(alphabet) == 1
    s = sweep.build_sequence(40000, 40000, alphabet, k, "middle", True)
    assert len(s) == 40000 + k - 1 and (s == ord(alphabet)).all()
    with pytest.raises(AssertionError):
        sweep.build_sequence(5, 20, alphabet, k)


def test_c_oracle_adds_sequentially():
    """c_oracle.per_kb_f32 is float32(np.cumsum) on every pair of the fixture: the oracle the device is held to and the
    arithmetic the search used are the same."""
    from oracle import c_oracle as co
    ps = [p for p in sweep.pairs(*CLASSES)]
    counts = np.array([[n, 0, 1] for n, _, _ in ps], dtype=np.uint32)
    got = co.per_kb_f32(counts, [W for _, W, _ in ps], 1)  # k = 1: a sequence of W letters has W windows
    assert np.array_equal(got[:, 0].view(np.uint32), np.array([b for _, _, b in ps], dtype=np.uint32))
    assert not got[:, 1].any()
    assert np.array_equal(got[:, 2], np.array([1000.0 / W for _, W, _ in ps]).astype(np.float32))


def test_launch_geometry_of_the_boundary_cases():
    # any-alphabet LDS path: what the sites are named for
    assert sweep.generic_geometry("ACGTN", 2, 50_000) == (1, 1) and sweep.generic_geometry(sweep.AMINO, 2, 50_000) == (1, 1)
    assert sweep.generic_geometry(*sweep.GEN_SLOW, 50_000) == (1, 0)
    assert sweep.generic_geometry(*sweep.GEN_RANGES, 50_000) == (3, 0)
    # tile batches at k = 8: three batches, the middle sequences with the first, the last larger than a batch
    assert sweep.batch_tiles(sweep.SPLIT_K) == 8192
    lengths = sweep.split_lengths()
    tiles = [-(-(n - sweep.SPLIT_K + 1) // sweep.ITEM_WINDOWS) for n in lengths]
    assert tiles == [4900, 1, 2, 4900, 8300] and lengths[1] - sweep.SPLIT_K + 1 <= sweep.ITEM_WINDOWS and lengths[2] == 9000
    assert all((n - sweep.SPLIT_K + 1) % sweep.ITEM_WINDOWS for n in lengths)
    assert sweep.batches_of(lengths, sweep.SPLIT_K) == [[0, 2], [3], [4]]
    # gridDim.y: 65 535 long sequences, then the other five
    lengths = sweep.gridy_lengths()
    assert len(lengths) == 65544 and (lengths > sweep.ITEM_WINDOWS).sum() == sweep.GRIDY_LONG
    assert all(lengths[i] <= sweep.ITEM_WINDOWS for i in sweep.GRIDY_SHORT_AT)
    assert set(lengths[lengths > sweep.ITEM_WINDOWS]) == set(range(8193, 8201))
    assert [len(b) for b in sweep.batches_of(lengths, sweep.GRIDY_K)] == [65535, 5]
    # the HBM path: more sequences than a batch with the knob, a batch of one above 2^24 columns
    alphabet, k, n = sweep.HBM_KNOB
    assert sweep.hbm_batch(alphabet, k, n) == 419 < n
    alphabet, k, n = sweep.HBM_WIDE
    assert (1 << 24) < len(alphabet) ** k <= (1 << 26) and sweep.hbm_batch(alphabet, k, n) == 1 and n == 3
