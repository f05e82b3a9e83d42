"""The per-kb values of every counting kernel (seekr_amd/csrc/count.hip) at counts where the shortcut and the reference's
arithmetic part ways, and the launch boundaries of the same file.

The reference stores float32(n sequential float64 additions of 1000 / W) for a k-mer seen n times in a sequence of W
windows (kmer_counts.py:144-150).  per_kb.hpp: per_kb_value returns float32(n * (1000 / W)) and replays the additions only
when the product lies within p (n + 4) 2^-53 of a float32 rounding boundary.  tests/golden/count_value_pairs.json
(make_golden_count_pairs.py) holds pairs (n, W) where the two differ (`mismatch`: the first one is n = 35 604, W = 35 747),
where the slack test fires for nothing (`guard_only`), where it fires inside the kernels' 16-entry tables (`small_n`) and
the plain ones around the table and tile sizes (`control`).  A pair becomes a sequence: a run of one letter, n + k - 1
long, and W - n filler characters drawn from the other letters, the run at the start or in the middle (across a tile /
chunk boundary), of the alphabet's first letter or of its last (the row's last bin).

  rows1     count_rows_kernel, one wave: "AGTC" k = 1, 3, 6, the control pairs; uint32, float32 and Log2.pre
  rows4     count_rows_kernel, four waves: k = 7, 8, the control pairs
  long      convert_long_kernel: k = 1, 3, 6, 7, 8, mismatch + guard_only + small_n (the W = 5 000 000 pair at k = 3)
  global    count_kmers_kernel<GLOBAL>: k = 9, 12 mismatch and 12 guard_only pairs (rows of 1 MiB)
  f64       count_kmers_kernel<OUT_F64>: float64 output at k = 3 and 7, the mismatch pairs; the target cell equal to np.cumsum
  gen_fast  count_generic_lds_kernel with fast_tab = 1: ACGTN and the 20 amino acids at k = 2, every class, every dtype; one letter
  gen_slow  the same with fast_tab = 0: ACG at k = 9 (19 683 bins, one workgroup per CU), mismatch + guard_only
  gen_ranges  ACGTN at k = 7: 78 125 bins in three launches, the mismatch pairs in bin 0 and in the last bin
  gen_hbm   convert_generic_kernel (SEEKR_COUNT_GENERIC_GLOBAL=1): ACGTN k = 2, mismatch + guard_only + small_n, every dtype,
            Log2.pre bit-identical to the LDS path
  split     k = 8 (8 192 tiles a batch): 4 900 tiles, a short sequence, 9 000 bases, 4 900 tiles, 8 300 tiles: three batches,
            the last one larger than a batch
  gridy     k = 1, 65 540 sequences of 8 193 .. 8 200 bases (two tiles each) and four short ones: the gridDim.y flush
  hbm_batches  the any-alphabet HBM path over several batches (seq0 > 0): 20^4 columns x 430 sequences with the knob,
            ACGTN k = 11 (48 828 125 columns, above 2^24) x 3 sequences without

References: oracle/c_oracle (count_u32, per_kb_f32: a C loop that adds sequentially) and
oracle/seekr_oracle.per_kb_from_counts for float64; nothing of seekr_amd.  Every output is compared bit for bit over the
whole row, Log2.pre within RTOL / ATOL_LOG of numpy's log2.  Every sweep_* returns the list of failing cases.

    python tools/count_value_sweep.py [--only long,gen_fast] [--seed 1] [--lib path/to/libseekr_hip.so]

Exit code 1 and the failing cases on stderr if any check fails.  Needs a real MI355X.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FIXTURE = os.path.join(ROOT, "tests", "golden", "count_value_pairs.json")

RTOL, ATOL_LOG = 1e-5, 1e-6  # tests/test_gpu_parity.py: the bar of every Log2.pre comparison
ITEM_WINDOWS = 8192          # count.hip kItemWindows
GEN_CHUNK = 4096             # count.hip kGenChunk
GEN_LDS_BINS = 36864         # count.hip kGenLdsBins
TAB_SIZE = 16                # per_kb.hpp kTabSize
W_BIG = 5_000_000
AMINO = "ARNDCQEGHILKMFPSTWYV"


class CannotAllocate(Exception):
    """The device (or the host) has no room for a case: the caller skips it."""


def fail(bad, case, what):
    bad.append("%s: %s" % (case, what))
    print("%s  FAIL  %s" % (case, what), file=sys.stderr, flush=True)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def context():
    from seekr_amd import _lib
    return _lib.default_context()


# ---- the arithmetic -------------------------------------------------------------------------------------------------------
def running_sums(W):
    """s[n] = n sequential float64 additions of 1000 / W, n = 0 .. W (np.cumsum adds in index order)."""
    s = np.empty(W + 1)
    s[0] = 0.0
    np.cumsum(np.full(W, 1000.0 / W), out=s[1:])
    return s


def evaluate(n, inc, s):
    """For counts n (int64 array), inc = 1000 / W (scalar or array) and the running sums s of the same shape:
    (the slack test of per_kb_value fires, float32(n * inc), float32(s))."""
    p = n.astype(np.float64) * inc
    f = p.astype(np.float32)
    slack = p * ((n + 4).astype(np.float64) * 2.0 ** -53)
    fire = (n > 3) & (((p - slack).astype(np.float32) != f) | ((p + slack).astype(np.float32) != f))
    return fire, f, s.astype(np.float32)


def guard_and_mismatch(n, inc, s):
    """(the slack test fires, float32(n * inc) != float32(s))."""
    fire, f, s32 = evaluate(n, inc, s)
    return fire, f != s32


def scan_w(W):
    """(n = 1 .. W, guard fires, product != running sum) for one window count."""
    n = np.arange(1, W + 1, dtype=np.int64)
    fire, differ = guard_and_mismatch(n, 1000.0 / W, running_sums(W)[1:])
    return n, fire, differ


def per_kb_model(n, W, sums=None):
    """per_kb.hpp: per_kb_value restated: the product, unless n > 3 and the slack test fires — then the replayed sum.
    n: int64 array of counts <= W.  Returns (float32 values, which of them were replayed)."""
    n = np.asarray(n, dtype=np.int64)
    fire, f, s32 = evaluate(n, 1000.0 / W, (running_sums(W) if sums is None else sums)[n])
    return np.where(fire, s32, f), fire


def expected_bits(n, W):
    """Bits of float32(n sequential additions of 1000 / W)."""
    return int(bits(running_sums(W)[n:n + 1].astype(np.float32))[0])


def classify(n, W, sums=None):
    """'mismatch', 'guard_only' or 'plain' for one pair."""
    s = running_sums(W) if sums is None else sums
    fire, differ = guard_and_mismatch(np.array([n], dtype=np.int64), 1000.0 / W, s[n:n + 1])
    return "mismatch" if differ[0] else ("guard_only" if fire[0] else "plain")


_pairs = None


def pairs(*names):
    """The fixture's (n, W, bits) of the named classes, in the file's order."""
    global _pairs
    if _pairs is None:
        with open(FIXTURE) as f:
            _pairs = json.load(f)
    return [tuple(p) for name in names for p in _pairs[name]]


def upto(ps, w_max):
    return [p for p in ps if p[1] <= w_max]


def some(ps, count):
    """`count` of the pairs, evenly spaced, the first and the last among them."""
    at = np.unique(np.linspace(0, len(ps) - 1, count).round().astype(int))
    return [ps[i] for i in at]


# ---- sequences ------------------------------------------------------------------------------------------------------------
PLACEMENTS = ("start", "middle")


def run_start(n, W, k, placement):
    """Where the run of n + k - 1 letters begins among the W - n filler characters: 0, or the place that puts the middle of its n
    windows on the largest boundary (tile of 8 192 windows, chunk of 4 096, a one-wave sweep of 1 024, a packed word) that fits."""
    filler = W - n
    if placement == "start" or n == 0 or filler == 0:
        return 0
    for boundary in (ITEM_WINDOWS, GEN_CHUNK, 1024, 16):
        at = boundary - n // 2
        if 1 <= at <= filler:
            return at
    return (filler + 1) // 2


def build_sequence(n, W, alphabet, k, placement="start", last_letter=False, seed=1):
    """uint8 array of W + k - 1 characters with exactly W windows, n of them the k-mer of the run letter (the alphabet's first
    or last letter); the other characters are drawn from the other letters."""
    letters = np.frombuffer(alphabet.encode("latin-1"), dtype=np.uint8)
    run_letter = letters[-1] if last_letter else letters[0]
    others = letters[letters != run_letter]
    assert 0 <= n <= W and (len(others) or n == W), (n, W, alphabet)
    run = n + k - 1 if n else 0
    total = W + k - 1
    rng = np.random.default_rng([seed, n, W, k, len(alphabet), PLACEMENTS.index(placement), int(last_letter)])
    seq = others[rng.integers(0, len(others), size=total)] if total > run else np.empty(total, dtype=np.uint8)
    at = run_start(n, W, k, placement)
    seq[at:at + run] = run_letter
    return seq


def target_bin(alphabet, k, last_letter):
    return len(alphabet) ** k - 1 if last_letter else 0


def build_set(ps, alphabet, k, seed=1):
    """One sequence per pair, placements and run letters alternating.  (blob, offsets, target bins)."""
    seqs, targets = [], []
    for i, (n, W, _) in enumerate(ps):
        last = (i // 2) % 2 == 1
        seqs.append(build_sequence(n, W, alphabet, k, PLACEMENTS[i % 2], last, seed))
        targets.append(target_bin(alphabet, k, last))
    offsets = np.zeros(len(seqs) + 1, dtype=np.int64)
    np.cumsum([len(s) for s in seqs], out=offsets[1:])
    return np.concatenate(seqs), offsets, np.array(targets, dtype=np.int64)


def references(ps, blob, offsets, targets, alphabet, k, bad, case, want_f64=False):
    """(uint32 counts, float32 per-kb values, float64 values or None) of the C oracle; the target cells are held to the
    fixture: count n and the recorded bits."""
    from oracle import c_oracle as co
    from oracle import seekr_oracle as orc
    n_ref = co.count_u32(blob, offsets, k, alphabet)
    lens = np.diff(offsets)
    f_ref = co.per_kb_f32(n_ref, lens, k)
    rows = np.arange(len(ps))
    if not np.array_equal(n_ref[rows, targets], [p[0] for p in ps]) or not np.array_equal(lens - k + 1, [p[1] for p in ps]):
        fail(bad, case, "the sequences do not hold the pairs' counts and windows")
    if not np.array_equal(bits(f_ref[rows, targets]), np.array([p[2] for p in ps], dtype=np.uint32)):
        fail(bad, case, "the C oracle's float32 differs from the fixture's bits")
    d_ref = orc.per_kb_from_counts(n_ref, lens, k, dtype=np.float64) if want_f64 else None
    return n_ref, f_ref, d_ref


def compare(bad, case, got, want, ps=None):
    if got.shape != want.shape or got.dtype != want.dtype:
        fail(bad, case, "%s %s, want %s %s" % (got.dtype, got.shape, want.dtype, want.shape))
        return
    differ = bits(got) != bits(want)
    if differ.any():
        r, c = np.argwhere(differ)[0]
        pair = " (n=%d W=%d)" % tuple(ps[r][:2]) if ps is not None else ""
        fail(bad, case, "%d cells differ, the first at row %d%s column %d: got %r want %r" %
             (differ.sum(), r, pair, c, got[r, c], want[r, c]))


def compare_log(bad, case, got, f_ref):
    from oracle import seekr_oracle as orc
    want = orc.log2_plus_one(f_ref)
    if got.shape != want.shape or not np.allclose(got, want, rtol=RTOL, atol=ATOL_LOG):
        fail(bad, case, "Log2.pre off by %g" % float(np.abs(got.astype(np.float64) - want).max()))


def with_knobs(ctx, env, fn):
    """fn() with A/B knobs set (the context reads them once: reload before and after)."""
    old = {key: os.environ.get(key) for key in env}
    os.environ.update(env)
    ctx.reload_knobs()
    try:
        return fn()
    finally:
        for key, v in old.items():
            if v is None:
                os.environ.pop(key, None)
            else:
                os.environ[key] = v
        ctx.reload_knobs()


# ---- the 4-letter kernels -------------------------------------------------------------------------------------------------
def four_letter_case(bad, case, ps, k, seed, dtypes=("uint32", "float32", "log2"), f64_cumsum=False, timing=None):
    from seekr_amd import _lib as L
    ctx = context()

    def timed(what, fn):  # the call, the wait for it and the copy of the rows
        t0 = time.time()
        out = fn().to_numpy()
        if timing is not None:
            timing["%s %s, device" % (case, what)] = time.time() - t0
        return out

    blob, offsets, targets = build_set(ps, "AGTC", k, seed)
    n_ref, f_ref, d_ref = references(ps, blob, offsets, targets, "AGTC", k, bad, case, want_f64="float64" in dtypes)
    packed = L.PackedSeqs.from_buffer(ctx, blob, offsets, "AGTC")
    if "uint32" in dtypes:
        compare(bad, case + " uint32", timed("uint32", lambda: L.count_u32(ctx, packed, k)), n_ref, ps)
    if "float32" in dtypes:
        compare(bad, case + " float32", timed("float32", lambda: L.count_per_kb(ctx, packed, k)), f_ref, ps)
    if "log2" in dtypes:
        compare_log(bad, case + " Log2.pre", L.count_per_kb(ctx, packed, k, log2_pre=True).to_numpy(), f_ref)
    if "float64" in dtypes:
        got = L.count_per_kb(ctx, packed, k, dtype=np.float64).to_numpy()
        compare(bad, case + " float64", got, d_ref, ps)
        if f64_cumsum:
            for i, (n, W, _) in enumerate(ps):
                if got[i, targets[i]] != running_sums(W)[n]:
                    fail(bad, case + " float64", "n=%d W=%d: %r is not np.cumsum's %r" % (n, W, got[i, targets[i]], running_sums(W)[n]))
    packed.free()


ROWS1_KS, ROWS4_KS, LONG_KS, F64_KS = (1, 3, 6), (7, 8), (1, 3, 6, 7, 8), (3, 7)
BIG_PAIR_K = 3
GLOBAL_K, GLOBAL_PER_CLASS = 9, 12


def sweep_rows1(seed=1, ks=ROWS1_KS):
    bad = []
    for k in ks:
        four_letter_case(bad, "rows1 k=%d control" % k, pairs("control"), k, seed)
    return bad


def sweep_rows4(seed=1, ks=ROWS4_KS):
    bad = []
    for k in ks:
        four_letter_case(bad, "rows4 k=%d control" % k, pairs("control"), k, seed)
    return bad


def long_pairs(k):
    """mismatch + guard_only + small_n for convert_long_kernel; the W = 5 000 000 pair at k = 3 only."""
    ps = pairs("mismatch", "guard_only", "small_n")
    assert all(W > ITEM_WINDOWS for _, W, _ in ps)
    return ps if k == BIG_PAIR_K else [p for p in ps if p[1] != W_BIG]


def sweep_long(seed=1, ks=LONG_KS, timing=None):
    bad = []
    for k in ks:
        ps = long_pairs(k)
        small, large = [p for p in ps if p[1] < W_BIG], [p for p in ps if p[1] >= W_BIG]
        four_letter_case(bad, "long k=%d" % k, small, k, seed)
        if large:
            # (the replay of n = 3 826 931 is that many dependent float64 additions in one lane: float32 against uint32)
            four_letter_case(bad, "long k=%d, the %d pairs with W >= %d" % (k, len(large), W_BIG), large, k, seed, timing=timing)
    return bad


def global_pairs():
    return some(upto(pairs("mismatch"), 300_000), GLOBAL_PER_CLASS) + some(pairs("guard_only"), GLOBAL_PER_CLASS)


def sweep_global(seed=1):
    bad = []
    four_letter_case(bad, "global k=%d" % GLOBAL_K, global_pairs(), GLOBAL_K, seed)
    return bad


def sweep_f64(seed=1, ks=F64_KS):
    bad = []
    for k in ks:
        four_letter_case(bad, "f64 k=%d" % k, upto(pairs("mismatch"), 300_000), k, seed, dtypes=("float64",), f64_cumsum=True)
    return bad


# ---- the any-alphabet kernels -----------------------------------------------------------------------------------------------
def generic_case(bad, case, ps, alphabet, k, seed, dtypes=("uint32", "float32", "float64", "log2"), knob=False, same_log=False):
    from seekr_amd import _lib as L
    ctx = context()
    blob, offsets, targets = build_set(ps, alphabet, k, seed)
    n_ref, f_ref, d_ref = references(ps, blob, offsets, targets, alphabet, k, bad, case, want_f64="float64" in dtypes)
    a = L.AsciiSeqs(ctx, blob, offsets)

    def run():
        out = {}
        if "uint32" in dtypes:
            out["uint32"] = L.count_generic_dev(ctx, a, alphabet, k, np.uint32).to_numpy()
        if "float32" in dtypes:
            out["float32"] = L.count_generic_dev(ctx, a, alphabet, k, np.float32).to_numpy()
        if "float64" in dtypes:
            out["float64"] = L.count_generic_dev(ctx, a, alphabet, k, np.float64).to_numpy()
        if "log2" in dtypes:
            out["log2"] = L.count_generic_dev(ctx, a, alphabet, k, log2_pre=True).to_numpy()
        return out

    got = with_knobs(ctx, {"SEEKR_COUNT_GENERIC_GLOBAL": "1"}, run) if knob else run()
    for name, want in (("uint32", n_ref), ("float32", f_ref), ("float64", d_ref)):
        if name in got:
            compare(bad, "%s %s" % (case, name), got[name], want, ps)
    if "log2" in got:
        compare_log(bad, case + " Log2.pre", got["log2"], f_ref)
        if same_log:  # the other device path gives the same bits
            other = L.count_generic_dev(ctx, a, alphabet, k, log2_pre=True).to_numpy()
            compare(bad, case + " Log2.pre, LDS path == HBM path", other, got["log2"], ps)
    a.free()


GEN_FAST = (("ACGTN", 2), (AMINO, 2))
GEN_ONE_LETTER = ("T", 3)
GEN_SLOW = ("ACG", 9)
GEN_RANGES = ("ACGTN", 7)
GEN_HBM = ("ACGTN", 2)


def generic_geometry(alphabet, k, mean_len):
    """(launches, fast_tab) of skr_count_generic_dev's LDS path for rows of len(alphabet)^k bins."""
    nbins = len(alphabet) ** k
    rng = min(nbins, GEN_LDS_BINS)
    lds = ((rng + 3) & ~3) * 4 + TAB_SIZE * 4 + 256 + 2 * (GEN_CHUNK + 64)
    per_cu = max(1, min(2, (160 * 1024) // lds))
    want = 1 if (rng >= 12288 and 2.0 * mean_len < rng) else per_cu
    return -(-nbins // rng), 1 if want > 1 else 0


def sweep_gen_fast(seed=1, cases=GEN_FAST):
    bad = []
    for alphabet, k in cases:
        ps = pairs("mismatch", "guard_only", "small_n", "control")
        generic_case(bad, "gen_fast %d letters k=%d" % (len(alphabet), k), ps, alphabet, k, seed)
    alphabet, k = GEN_ONE_LETTER  # no filler: homopolymers only
    ps = [p for p in pairs("control") if p[0] == p[1]]
    generic_case(bad, "gen_fast one letter k=%d" % k, ps, alphabet, k, seed)
    return bad


def sweep_gen_slow(seed=1):
    bad = []
    alphabet, k = GEN_SLOW
    generic_case(bad, "gen_slow %s k=%d" % (alphabet, k), upto(pairs("mismatch", "guard_only"), 300_000), alphabet, k, seed)
    return bad


def sweep_gen_ranges(seed=1):
    bad = []
    alphabet, k = GEN_RANGES
    generic_case(bad, "gen_ranges %s k=%d" % (alphabet, k), upto(pairs("mismatch"), 300_000), alphabet, k, seed,
                 dtypes=("uint32", "float32", "log2"))
    return bad


def sweep_gen_hbm(seed=1):
    bad = []
    alphabet, k = GEN_HBM
    generic_case(bad, "gen_hbm %s k=%d" % (alphabet, k), pairs("mismatch", "guard_only", "small_n"), alphabet, k, seed,
                 knob=True, same_log=True)
    return bad


# ---- launch boundaries ----------------------------------------------------------------------------------------------------
_FOUR = np.frombuffer(b"ACGT", dtype=np.uint8)
_QUADS = _FOUR[(np.arange(256)[:, None] >> np.array([0, 2, 4, 6])) & 3].copy().view(np.uint32).reshape(-1)  # byte -> 4 letters


def random_bases(rng, n):
    """n letters of ACGT, uniform: four from every random byte."""
    return _QUADS[rng.integers(0, 256, size=(n + 3) // 4, dtype=np.uint8)].view(np.uint8)[:n]


def counts_and_values(bad, case, blob, offsets, k):
    """uint32 counts and float32 per-kb values of the 4-letter path against the C oracle, bit for bit."""
    from oracle import c_oracle as co
    from seekr_amd import _lib as L
    ctx = context()
    n_ref = co.count_u32(blob, offsets, k)
    f_ref = co.per_kb_f32(n_ref, np.diff(offsets), k)
    try:
        packed = L.PackedSeqs.from_buffer(ctx, blob, offsets, "AGTC")
        got_n = L.count_u32(ctx, packed, k).to_numpy()
        got_f = L.count_per_kb(ctx, packed, k).to_numpy()
    except MemoryError as e:
        raise CannotAllocate("%s: %s" % (case, e))
    compare(bad, case + " uint32", got_n, n_ref)
    compare(bad, case + " float32", got_f, f_ref)
    packed.free()


SPLIT_K = 8
SPLIT_TILES = (4900, 0, 2, 4900, 8300)  # of 8 192 windows; 0: a short sequence


def batch_tiles(k):
    """launch_rows: tiles whose partial histograms fill 2 GiB."""
    return max(1, (1 << 31) // (4 ** k * 4))


def split_lengths(k=SPLIT_K):
    """4 900 tiles | short | 9 000 bases (two tiles) | 4 900 tiles | 8 300 tiles, none a whole number of tiles."""
    return [t * ITEM_WINDOWS - 1234 - 77 * i + k - 1 if t > 2 else (9000 if t == 2 else 700) for i, t in enumerate(SPLIT_TILES)]


def batches_of(lengths, k):
    """The batches of long sequences (lists of indices) launch_rows forms: a batch is flushed before a sequence that would
    take it past batch_tiles, and at 65 535 sequences (gridDim.y)."""
    out, cur, tiles_in = [], [], 0
    for i, n in enumerate(lengths):
        W = n - k + 1
        if W <= ITEM_WINDOWS:
            continue
        tiles = -(-W // ITEM_WINDOWS)
        if tiles_in and tiles_in + tiles > batch_tiles(k):
            out.append(cur)
            cur, tiles_in = [], 0
        if len(cur) >= 65535:
            out.append(cur)
            cur, tiles_in = [], 0
        cur.append(i)
        tiles_in += tiles
    return out + [cur] if cur else out


def sweep_split(seed=1):
    bad = []
    rng = np.random.default_rng([seed, 71])
    lengths = split_lengths()
    offsets = np.zeros(len(lengths) + 1, dtype=np.int64)
    np.cumsum(lengths, out=offsets[1:])
    counts_and_values(bad, "split k=%d" % SPLIT_K, random_bases(rng, int(offsets[-1])), offsets, SPLIT_K)
    return bad


GRIDY_K, GRIDY_LONG = 1, 65540
GRIDY_SHORT_AT = (0, 65534, 65535, 65536)


def gridy_lengths():
    """65 540 sequences of 8 193 .. 8 200 bases (k = 1: two tiles each) with short ones at positions 0, 65 534, 65 535 and
    65 536 of the set."""
    n = GRIDY_LONG + len(GRIDY_SHORT_AT)
    lengths = np.empty(n, dtype=np.int64)
    short = np.zeros(n, dtype=bool)
    short[list(GRIDY_SHORT_AT)] = True
    lengths[short] = (5, 8192, 1, 300)
    lengths[~short] = 8193 + np.arange(GRIDY_LONG) % 8
    return lengths


def sweep_gridy(seed=1):
    bad = []
    rng = np.random.default_rng([seed, 73])
    lengths = gridy_lengths()
    offsets = np.zeros(len(lengths) + 1, dtype=np.int64)
    np.cumsum(lengths, out=offsets[1:])
    counts_and_values(bad, "gridy k=%d" % GRIDY_K, random_bases(rng, int(offsets[-1])), offsets, GRIDY_K)
    return bad


HBM_KNOB = (AMINO, 4, 430)   # 160 000 columns: 419 sequences fill 256 MiB of histograms
HBM_WIDE = ("ACGTN", 11, 3)  # 48 828 125 columns > 2^24: the HBM path without the knob, one sequence a batch


def hbm_batch(alphabet, k, n):
    """skr_count_generic_dev: sequences per batch of the HBM path."""
    return max(1, min(n, (256 << 20) // (len(alphabet) ** k * 4)))


def hbm_case(bad, case, alphabet, k, n, knob, seed):
    from oracle import c_oracle as co
    from seekr_amd import _lib as L
    ctx = context()
    rng = np.random.default_rng([seed, 79, k])
    letters = np.frombuffer((alphabet + "x").encode("latin-1"), dtype=np.uint8)  # x: outside the alphabet
    lengths = rng.integers(k, 400, size=n)
    lengths[:3] = (k + 250, k, 399)
    offsets = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lengths, out=offsets[1:])
    weights = np.r_[np.full(len(alphabet), 1.0), 0.05]
    blob = letters[rng.choice(len(letters), size=int(offsets[-1]), p=weights / weights.sum())]
    n_ref = co.count_u32(blob, offsets, k, alphabet)
    try:
        a = L.AsciiSeqs(ctx, blob, offsets)
        run = lambda: [L.count_generic_dev(ctx, a, alphabet, k, dt).to_numpy() for dt in (np.uint32, np.float32)]  # noqa: E731
        got_n, got_f = with_knobs(ctx, {"SEEKR_COUNT_GENERIC_GLOBAL": "1"}, run) if knob else run()
    except MemoryError as e:
        raise CannotAllocate("%s: %s" % (case, e))
    compare(bad, case + " uint32", got_n, n_ref)
    del got_n
    compare(bad, case + " float32", got_f, co.per_kb_f32(n_ref, lengths, k))
    a.free()


def sweep_hbm_batches(seed=1, which=("knob", "wide")):
    bad = []
    if "knob" in which:
        alphabet, k, n = HBM_KNOB
        hbm_case(bad, "hbm_batches knob %d^%d x %d" % (len(alphabet), k, n), alphabet, k, n, True, seed)
    if "wide" in which:
        alphabet, k, n = HBM_WIDE
        hbm_case(bad, "hbm_batches %s k=%d x %d" % (alphabet, k, n), alphabet, k, n, False, seed)
    return bad


SWEEPS = ("rows1", "rows4", "long", "global", "f64", "gen_fast", "gen_slow", "gen_ranges", "gen_hbm", "split", "gridy",
          "hbm_batches")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--only", default=None, help="comma-separated: " + ",".join(SWEEPS))
    ap.add_argument("--lib", default=None, help="another build of libseekr_hip.so to run the sweep against")
    args = ap.parse_args()
    if args.lib:
        from seekr_amd import _lib
        _lib.LIB_PATH = os.path.abspath(args.lib)
    only = set(args.only.split(",")) if args.only else set(SWEEPS)
    counts = {name: len(pairs(name)) for name in ("mismatch", "guard_only", "small_n", "control")}
    what = {
        "rows1": "k %s, %d control pairs" % (ROWS1_KS, counts["control"]),
        "rows4": "k %s, %d control pairs" % (ROWS4_KS, counts["control"]),
        "long": "k %s, %d pairs" % (LONG_KS, len(long_pairs(BIG_PAIR_K))),
        "global": "k = %d, %d pairs" % (GLOBAL_K, len(global_pairs())),
        "f64": "k %s, %d mismatch pairs" % (F64_KS, len(upto(pairs("mismatch"), 300_000))),
        "gen_fast": "%s, %d pairs" % (" / ".join("%d^%d" % (len(a), k) for a, k in GEN_FAST), sum(counts.values())),
        "gen_slow": "%s^%d" % GEN_SLOW, "gen_ranges": "%s^%d" % GEN_RANGES, "gen_hbm": "%s^%d with the knob" % GEN_HBM,
        "split": "tiles %s" % (SPLIT_TILES,), "gridy": "%d long sequences" % GRIDY_LONG,
        "hbm_batches": "%d^%d x %d with the knob, %s^%d x %d" % ((len(HBM_KNOB[0]),) + HBM_KNOB[1:] + HBM_WIDE),
    }
    failing = 0
    for name in SWEEPS:
        if name not in only:
            continue
        t0, timing = time.time(), {}
        try:
            bad = globals()["sweep_" + name](args.seed, timing=timing) if name == "long" else globals()["sweep_" + name](args.seed)
        except CannotAllocate as e:
            print("%s: not run, %s" % (name, e), flush=True)
            continue
        failing += len(bad)
        for key, t in timing.items():
            print("  %s: %.3f s" % (key, t), flush=True)
        print("%s: %s, %d failing, %.1f s" % (name, what[name], len(bad), time.time() - t0), flush=True)
    sys.exit(1 if failing else 0)


if __name__ == "__main__":
    main()
