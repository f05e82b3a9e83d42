"""Writes tests/golden/count_value_pairs.json: pairs (n, W) of a k-mer count n and a window count W at which
count.hip: per_kb_value has something to decide.  numpy only, no device, about a minute.

The reference stores float32(n sequential float64 additions of 1000 / W) (kmer_counts.py:144-150).  The kernels
return float32(n * (1000 / W)) unless a slack test says the product may round differently, and only then replay the
additions.  The arithmetic (product, slack test, running sum = np.cumsum, which adds sequentially) is
tools/count_value_sweep.py: scan_w.  Four classes:

  mismatch    float32(n * inc) != float32(running sum): the replay changes the stored bits
              >= 48 pairs with W <= 70 000 spread over the whole range of W and of n / W, among them the pair of the
              smallest W and the pair of the smallest n; >= 12 pairs with 10^5 <= W <= 3 10^5; one with W = 5 000 000
  guard_only  the slack test fires, both roundings agree (>= 48 pairs, the first fire among them)
  small_n     n <= 15 (the kernels' 16-entry tables) with a guard fire: W <= 3 10^7 holds two, both at n = 10
  control     n in {0, 1, 2, 3, 4, 15, 16, 17, W - 1, W} at W in {20, 1 000, 8 191, 8 192, 8 193, 40 000}

Every entry is [n, W, bits of the expected float32].

    python tests/golden/make_golden_count_pairs.py
"""
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "tools"))
import count_value_sweep as cv  # noqa: E402

W_SCAN = 70_000
W_MID = (100_000, 300_000)
N_MID = 12
W_BIG = 5_000_000
W_SMALL_N = 30_000_000
N_PER_CLASS = 48


def spread(pairs, count, keep):
    """`count` of `pairs` evenly spaced in the order of W, then those of `keep`."""
    pairs = sorted(pairs, key=lambda p: (p[1], p[0]))
    at = np.unique(np.linspace(0, len(pairs) - 1, count).round().astype(int))
    out = {pairs[i] for i in at} | set(keep)
    return sorted(out, key=lambda p: (p[1], p[0]))


def main():
    t0 = time.time()
    mism, fires = [], []
    for W in range(4, W_SCAN + 1):
        n, fire, differ = cv.scan_w(W)
        assert not (differ & ~fire).any(), "a mismatch the slack test does not see, W=%d" % W
        mism += [(int(x), W) for x in n[differ]]
        fires += [(int(x), W) for x in n[fire & ~differ]]
    print("W <= %d: %d mismatches over %d W, %d guard-only fires, %.0f s" %
          (W_SCAN, len(mism), len({w for _, w in mism}), len(fires), time.time() - t0), flush=True)
    first_w = min(mism, key=lambda p: (p[1], p[0]))
    first_n = min(mism, key=lambda p: (p[0], p[1]))
    print("smallest W with a mismatch:", first_w, " smallest n:", first_n, " first fire:", min(fires, key=lambda p: p[1]))
    mismatch = spread(mism, N_PER_CLASS, [first_w, first_n])
    guard_only = spread(fires, N_PER_CLASS, [min(fires, key=lambda p: (p[1], p[0]))])

    mid = []
    for i in range(N_MID):  # from every 15 384th W upwards, the first W that has a mismatch
        W = W_MID[0] + i * ((W_MID[1] - W_MID[0]) // (N_MID + 1))
        while True:
            n, fire, differ = cv.scan_w(W)
            assert not (differ & ~fire).any(), W
            if differ.any():
                mid.append((int(n[differ][i % int(differ.sum())]), W))
                break
            W += 1
    assert all(W_MID[0] <= w <= W_MID[1] for _, w in mid), mid
    n, fire, differ = cv.scan_w(W_BIG)
    assert not (differ & ~fire).any()
    print("W = %d: %d mismatches, the smallest n %d" % (W_BIG, differ.sum(), n[differ].min()), flush=True)
    mismatch += mid + [(int(n[differ].min()), W_BIG)]

    small_n = []
    for lo in range(16, W_SMALL_N + 1, 1 << 21):
        W = np.arange(lo, min(lo + (1 << 21), W_SMALL_N + 1), dtype=np.int64)
        inc = 1000.0 / W.astype(np.float64)
        s = np.zeros(len(W))
        for n in range(1, 16):
            s = s + inc
            if n <= 3:
                continue
            fire, differ = cv.guard_and_mismatch(np.full(len(W), n, dtype=np.int64), inc, s)
            assert not differ.any(), "a mismatch below n = 16"
            small_n += [(n, int(w)) for w in W[fire]]
    small_n.sort(key=lambda p: (p[1], p[0]))
    print("n = 4 .. 15, W <= %d: guard fires at" % W_SMALL_N, small_n, flush=True)

    control = [(n, W) for W in (20, 1000, 8191, 8192, 8193, 40000) for n in (0, 1, 2, 3, 4, 15, 16, 17, W - 1, W)]
    doc = {"about": "see tests/golden/make_golden_count_pairs.py; entries are [n, W, bits of float32(n sequential float64 additions of 1000 / W)]"}
    for name, pairs in (("mismatch", mismatch), ("guard_only", guard_only), ("small_n", small_n), ("control", control)):
        doc[name] = [[n, W, int(cv.expected_bits(n, W))] for n, W in pairs]
    path = os.path.join(HERE, "count_value_pairs.json")
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join(' "%s": %s' % (key, json.dumps(val)) for key, val in doc.items()) + "\n}\n")
    print("wrote %s: %s, %.0f s" % (path, {key: len(val) for key, val in doc.items() if key != "about"}, time.time() - t0))


if __name__ == "__main__":
    main()
