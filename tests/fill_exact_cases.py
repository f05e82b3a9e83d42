"""Rows whose row statistics are exact in float32 in ANY order, and the numpy model of what every operand fill kernel
must then store (DESIGN_PARITY.md, "Exact row statistics").  numpy only: tests/test_fill_exact_cpu.py and
tests/test_gpu_fill_exact.py share the builders, the model and the case tables below.

A row is x = c + s d: d small integers with sum d = 0 and sum d^2 = q^2 K, s a power of two, c = 3 s (the mean is not 0, so
a padding cell that is counted shows).  Then, whatever the order of the additions,
  sum x = 3 s K            (partial sums are integers below 2^24, in units of s)         mean = 3 s
  sum (x - mean) = 0       (partial sums: integers below 2^24 in units of s)             second centring: 0
  sum (x - mean)^2 = (q s)^2 K   (integers below 2^24 in units of s^2)                   var = (q s)^2, sd = q s
and z = fl32(d / q) is one IEEE division: the four fill kernels, each with its own order of summation and its own form
of the division, must store the same bits.  Class A: q in {1, 2, 4}, z dyadic, sum z^2 = K exactly: diag == 1.0f.
Class B: q = 3 (K even) or 6 (any K: sum d = 0 makes sum d^2 even), z rounded, lo != 0 at the operand's scale.

The flags restate the kernels' rules with the project's constants, compared in float32 as the kernels compare them.
Which kernel serves a (width, mode) is WRITTEN in the case tables (family), never asked of the library."""
import functools

import numpy as np

import exact_sum_cases as ec

F32 = np.float32
ONE_VALUE_SHARE, EQUAL_PAIR_SHARE, EQUAL_PAIR_SHARE_IN_QUADS = F32(0.85), F32(0.70), F32(0.45)   # operand.hip
TWO_LEVELS = 5e-3                                                                               # row_on_two_levels
ROW_SCALES = (2.0 ** -3, 2.0 ** -1, 2.0 ** -2)       # s of row i: ROW_SCALES[i % 3]


def kind_of(precision, cols):
    """Storage kind of an unflagged operand: 0 float32 layout, 1 bf16 halves (1 024 .. 16 384 columns), 2 fp16 halves."""
    if precision == "fp32":
        return 0
    if precision == "bf16x3":
        return 1 if 1024 <= cols <= 16384 else 0
    return 2


# ------------------------------------------------------------------ integer multisets with two prescribed sums
def solve_multiset(m, lo, hi, total, squares, rng):
    """m integers in lo .. hi whose sum is `total` and whose squares sum to `squares` (an int64 array, sorted): a clipped
    normal draw, then unit moves of one cell until the sum is right, then moves of two cells (a + 1, b - 1) or
    (a - 1, b + 1), which keep the sum and change the squares by any even amount."""
    assert m > 0 and (total - squares) % 2 == 0 and lo * m <= total <= hi * m, (m, lo, hi, total, squares)
    mean = total / m
    var = squares / m - mean * mean
    assert var >= 0, (m, total, squares)
    v = np.clip(np.rint(rng.normal(mean, np.sqrt(var), m)), lo, hi).astype(np.int64)
    n = hi - lo + 1
    h = np.bincount(v - lo, minlength=n).astype(np.int64)      # h[i]: cells of value lo + i
    val = np.arange(lo, hi + 1, dtype=np.int64)
    s, q = int((h * val).sum()), int((h * val * val).sum())
    while s != total:
        up, more = s < total, q < squares
        idx = np.nonzero(h[:-1])[0] if up else np.nonzero(h[1:])[0] + 1
        i = int(idx[-1] if up == more else idx[0])          # up: the largest value raises the squares most; down: the smallest
        j = i + 1 if up else i - 1
        h[i] -= 1
        h[j] += 1
        s += int(val[j] - val[i])
        q += int(val[j] ** 2 - val[i] ** 2)
    while q != squares:
        g = abs(squares - q) // 2
        moved = False
        if q < squares:      # (a, b) -> (a + 1, b - 1), a - b = gap >= 0: + 2 (gap + 1)
            for gap in range(min(g, n - 2) - 1, -1, -1):
                i = np.arange(gap + 1, n - 1)
                ok = (h[i] >= 2) if gap == 0 else (h[i] > 0) & (h[i - gap] > 0)
                if ok.any():
                    a = int(i[ok][0])
                    b = a - gap
                    h[a] -= 1; h[a + 1] += 1; h[b] -= 1; h[b - 1] += 1
                    q += 2 * (gap + 1)
                    moved = True
                    break
        else:                # (a, b) -> (a - 1, b + 1), a - b = gap >= 2: - 2 (gap - 1)
            for gap in range(min(g + 1, n - 1), 1, -1):
                i = np.arange(gap, n)
                ok = (h[i] > 0) & (h[i - gap] > 0)
                if ok.any():
                    a = int(i[ok][0])
                    b = a - gap
                    h[a] -= 1; h[a - 1] += 1; h[b] -= 1; h[b + 1] += 1
                    q -= 2 * (gap - 1)
                    moved = True
                    break
        assert moved, ("no multiset", m, lo, hi, total, squares)
    out = np.repeat(val, h)
    assert out.size == m and int(out.sum()) == total and int((out * out).sum()) == squares
    return out


# ------------------------------------------------------------------ rows
class Rows:
    """d: int64 [rows, K]; q: int per row (or one int).  x: the float32 rows to upload, z: what a fill must store."""

    def __init__(self, d, q, family=None, note=""):
        d = np.atleast_2d(np.asarray(d, dtype=np.int64))
        self.d, self.rows, self.cols = d, d.shape[0], d.shape[1]
        self.q = np.broadcast_to(np.asarray(q, dtype=np.int64), (self.rows,)).copy()
        self.s = np.array([ROW_SCALES[i % 3] for i in range(self.rows)])
        self.x = (self.s[:, None] * (3 + d)).astype(F32)
        self.z = d.astype(F32) / self.q.astype(F32)[:, None]            # one IEEE division per cell
        self.dyadic = np.array([int(v) & (int(v) - 1) == 0 for v in self.q])
        self.family, self.note = family, note

    def check(self):
        """The conditions, on the host, before anything is launched: the two sums as Python integers, the partial-sum
        bound, and that x round-trips through float32."""
        K = self.cols
        for i in range(self.rows):
            di = [int(v) for v in self.d[i]] if K <= 4096 else None
            total = sum(di) if di else int(self.d[i].sum())
            squares = sum(v * v for v in di) if di else int((self.d[i] * self.d[i]).sum())
            q = int(self.q[i])
            assert total == 0 and squares == q * q * K, (i, total, squares, q, K)
            # every partial sum, in any order, is an integer below 2^24 in the sum's own unit (s, s, s^2)
            assert int(np.abs(3 + self.d[i]).sum()) < 2 ** 24 and squares < 2 ** 24
            assert np.array_equal(self.x[i].astype(np.float64), self.s[i] * (3.0 + self.d[i]))
        return self

    def take(self, idx):
        r = Rows(self.d[idx], self.q[idx], self.family, self.note)
        r.s = self.s[idx]
        r.x, r.z = self.x[idx], self.z[idx]
        return r


def unflagged_rows(K, qs, seed):
    """One row per entry of qs, each a seeded permutation of a multiset of d in -3 q .. 3 q (|z| <= 3)."""
    d = np.empty((len(qs), K), np.int64)
    for i, q in enumerate(qs):
        pool = _unflagged_pool(K, q)
        d[i] = np.random.default_rng([seed, K, q, i]).permutation(pool)
        if d[i, -1] == -3:    # x = 0 in the last cell: leaving it out of a sum would not show
            j = int(np.argmax(d[i] != -3))
            d[i, -1], d[i, j] = d[i, j], -3
    return Rows(d, qs).check()


@functools.lru_cache(maxsize=None)
def _unflagged_pool(K, q):
    return solve_multiset(K, -3 * q, 3 * q, 0, q * q * K, np.random.default_rng([11, K, q]))


def class_rows(K, cls, rows=5, seed=1):
    """Class A: q alternates 2 and 4.  Class B: 3 and 6 at even K, 6 at odd K (sum d = 0 makes sum d^2 even)."""
    if cls == "A":
        qs = [(2, 4)[i % 2] for i in range(rows)]
    else:
        qs = [6 if K % 2 else (3, 6)[i % 2] for i in range(rows)]
    r = unflagged_rows(K, qs, seed)
    if cls == "B":   # at least half the cells are rounded quotients
        assert all(((r.d[i] % 3) != 0).mean() >= 0.5 for i in range(rows))
    return r


# ------------------------------------------------------------------ the normalisation tail that gives the same rows
def tail_inputs(rows, seed, with_scale=True):
    """(x_raw, centre, scale or None): x_raw = centre + scale * x, per-column float32 vectors, scale a power of two —
    (x_raw - centre) / scale == x bit for bit (asserted), so y == x and the operand is the same one."""
    K = rows.cols
    rng = np.random.default_rng([seed, K, 77])
    unit = min(ROW_SCALES)
    sc = (2.0 ** rng.integers(-1, 3, K)) if with_scale else np.ones(K)
    centre = (sc * unit * rng.integers(-8, 9, K)).astype(F32)
    raw = (centre.astype(np.float64)[None, :] + sc[None, :] * rows.x.astype(np.float64)).astype(F32)
    back = raw - centre[None, :]
    if with_scale:
        back = back / sc.astype(F32)[None, :]
    assert np.array_equal(back.view(np.uint32), rows.x.view(np.uint32))
    return raw, centre, (sc.astype(F32) if with_scale else None)


# ------------------------------------------------------------------ the model of the stored operand
def pad32(a):
    rows, cols = a.shape
    kt = (cols + 31) // 32
    return np.concatenate([a, np.zeros((rows, kt * 32 - cols), a.dtype)], axis=1)


def f16_halves_nearest(z, scale):
    zs = z * scale
    hi = zs.astype(np.float16)
    return hi, (zs - hi.astype(F32)).astype(np.float16)


def stored(z, precision, mutant=None):
    """What as_matrix() must hold, by its bits: uint32 [rows, kt * 32] (float32 layout) or uint16 [rows, kt, 2, 32]
    (halves); the cells that pad the last 32-column tile are +0."""
    K = z.shape[1]
    kind = kind_of(precision, K)
    if kind == 0:
        return pad32(np.ascontiguousarray(z, dtype=F32)).view(np.uint32)
    if kind == 2:
        if mutant == "hi_nearest":
            hi, lo = f16_halves_nearest(z, ec.f16_scale(K))
        else:
            hi, lo, _ = ec.f16_halves(z, ec.f16_scale(K))
        return ec.stored_halves(hi, lo, "f16x3")
    hi, lo = ec.bf16_halves(z)
    return ec.stored_halves(hi, lo, "bf16x3")


def read_back(mat, rows, cols, kind):
    """The same view of what op.as_matrix().to_numpy() returned."""
    kt = (cols + 31) // 32
    return mat.view(np.uint32) if kind == 0 else mat.view(np.uint16).reshape(rows, kt, 2, 32)


def diag_model(r):
    """(value float32 per row, exact): class A rows 1.0 bit for bit; other rows the float64 sum of the stored z^2 over K,
    to hold within K 2^-24 relative — the worst case of any float32 order over K non-negative terms."""
    v = (r.z.astype(np.float64) ** 2).sum(axis=1) / r.cols
    assert np.all(v[r.dyadic] == 1.0)
    return v.astype(F32), r.dyadic.copy()


# ------------------------------------------------------------------ a plain float32 restatement of a fill's arithmetic
def fill_arith(x, mutant=None):
    """z of float32 rows x the way the kernels compute it — mean, second centring, variance, sd, one division — with the
    sums taken in float64 and rounded once (on exact rows every order gives that).  The mutants are the mistakes the
    tests must be able to see: 'last' (last cell left out of the mean), 'pad' (one padding cell, a 0, counted in the
    centred sums), 'km1' (K - 1 for K in the variance), 'recip' (multiplication by a float32 reciprocal)."""
    K = x.shape[1]
    kf = F32(K)
    x64 = x.astype(np.float64)
    f = lambda v: v.astype(F32)
    s = (x64[:, :-1] if mutant == "last" else x64).sum(axis=1)
    mean = f(s) / kf
    c = x - mean[:, None]                                         # float32
    s1 = c.astype(np.float64).sum(axis=1)
    if mutant == "pad":
        s1 = s1 + (F32(0) - mean).astype(np.float64)
    m2 = f(s1) / kf
    dd = c - m2[:, None]
    s2 = (dd.astype(np.float64) ** 2).sum(axis=1)
    if mutant == "pad":
        s2 = s2 + ((F32(0) - mean) - m2).astype(np.float64) ** 2
    var = f(s2) / (F32(K - 1) if mutant == "km1" else kf)
    sd = np.sqrt(var.astype(np.float64)).astype(F32)
    if mutant == "recip":
        return c * (F32(1) / sd)[:, None]
    return c / sd[:, None]


# ------------------------------------------------------------------ the flags
def same_threshold(K):
    return ONE_VALUE_SHARE * F32(K)


def pair_threshold(K):
    return EQUAL_PAIR_SHARE * F32(K - 1)


def quad_threshold(K):
    return EQUAL_PAIR_SHARE_IN_QUADS * F32(K)


def smallest_count(thr):
    """The smallest integer n with float32(n) >= thr."""
    n = int(np.floor(float(thr)))
    while not F32(n) >= thr:
        n += 1
    return n


def counts(v, skip_pair=None):
    """(same, pairs, pairs in quads) per row of v: cells equal to the row minimum, equal neighbours over the whole row,
    equal neighbours inside aligned groups of four cells (None unless K is a multiple of 4).  skip_pair: the mutant that
    does not count the pair (p, p + 1)."""
    rows, K = v.shape
    same = (v == v.min(axis=1, keepdims=True)).sum(axis=1)
    eq = v[:, 1:] == v[:, :-1]
    if skip_pair is not None:
        eq = eq.copy()
        eq[:, skip_pair] = False
    quads = None
    if K % 4 == 0:
        inside = (np.arange(K - 1) % 4) != 3
        quads = (eq & inside[None, :]).sum(axis=1)
    return same, eq.sum(axis=1), quads


def two_level_statistic(z):
    """kurtosis - skewness^2 - 1 of the stored z, float64."""
    z = z.astype(np.float64)
    var, m3, m4 = (z ** 2).mean(axis=1), (z ** 3).mean(axis=1), (z ** 4).mean(axis=1)
    return m4 / var ** 2 - m3 ** 2 / var ** 3 - 1.0


def row_flags(r, family, strict=None, skip_pair=None):
    """Per row: dict of bool arrays same / pairs / levels / outlier, and coherent = same | pairs | levels.  family 'reg'
    counts the pairs inside quads, every other family over the whole row.  strict: the name of ONE rule compared with
    > instead of >= (the mutant)."""
    K = r.cols
    ge = lambda name, a, b: (a > b) if strict == name else (a >= b)
    same, pairs, quads = counts(r.x, skip_pair)
    f = {"same": ge("same", same.astype(F32), same_threshold(K))}
    if family == "reg":
        f["pairs"] = ge("pairs", quads.astype(F32), quad_threshold(K))
    else:
        f["pairs"] = ge("pairs", pairs.astype(F32), pair_threshold(K))
    stat = two_level_statistic(r.z)
    # the 5e-3 boundary itself is not reachable with exact rows: every row is 0 (two levels) or far above it
    assert np.all((stat < 1e-9) | (stat > 0.05)), stat
    f["levels"] = stat < TWO_LEVELS
    zmax2 = (r.z * r.z).max(axis=1)                                # float32
    assert np.all(r.dyadic | (np.abs(F32(16) * zmax2 / F32(K) - 1) > 0.01) | (K < 1024))
    f["outlier"] = ge("outlier", F32(16) * zmax2, F32(K)) & (K >= 1024)
    f["coherent"] = f["same"] | f["pairs"] | f["levels"]
    return f


def assert_unflagged(r, family=None):
    for fam in ([family] if family else (["row"] + (["reg"] if r.cols % 4 == 0 else []))):
        f = row_flags(r, fam)
        assert not f["coherent"].any() and not f["outlier"].any(), (fam, {k: v.tolist() for k, v in f.items()})
    return r


# ------------------------------------------------------------------ threshold rows: a background value and isolated cells
def _signed_singles(n, hi, squares, rng):
    """n non-zero integers in -hi .. hi with sum 0 and the given sum of squares: ceil(n / 2) positive ones and the rest
    negative, the two groups with the same sum."""
    n1, n2 = (n + 1) // 2, n // 2
    s1 = int(round(0.82 * np.sqrt(squares / n) * n2))            # mean magnitude a little below the rms
    q1 = int(round(squares * n1 / n))
    q1 += (q1 - s1) % 2
    pos = solve_multiset(n1, 1, hi, s1, q1, rng)
    neg = -solve_multiset(n2, 1, hi, s1, squares - q1, rng)
    return np.concatenate([pos, neg])


@functools.lru_cache(maxsize=None)
def _pair_pool(K, n):
    """The n cells that are not background (0) of a q = 2 row: non-zero, sum 0, squares 4 K."""
    return _signed_singles(n, 12, 4 * K, np.random.default_rng([23, K, n]))


def _spread(K, n, first=6):
    """n isolated interior positions, evenly spread over first .. K - 7."""
    pos = first + np.floor((np.arange(n) + 0.5) * (K - 6 - first) / n).astype(np.int64)
    assert n == 0 or (np.all(np.diff(pos) >= 4) and pos[0] >= first and pos[-1] <= K - 7), (K, n)
    return pos


def seams(family, K):
    """The neighbour pairs (p, p + 1) at which a fill kernel's equal-neighbour count crosses lanes, waves or pieces."""
    s = {(3, 4), (255, 256), (K - 2, K - 1)}
    if family == "wave":            # row[c + 1] at a 64-lane stride
        m = K // 64
        s |= {(63, 64), (64 * (m // 2) - 1, 64 * (m // 2)), (64 * m - 1, 64 * m)}
    elif family == "rowreg":        # __shfl_down inside a wave, edge[u][wave] between waves, piece u + 1 of wave 0 after the last wave
        s |= {(1791, 1792), (3839, 3840), (4095, 4096), (8191, 8192)}
        if K == 65536:
            s |= {(32767, 32768), (61439, 61440), (65279, 65280)}
        if K % 4:
            s.add((K - K % 4 - 1, K - K % 4))     # the pair that straddles the ragged piece
    else:                           # block kernels: val(c0 + 8) after a thread's group of eight
        last = 8 * ((K - 1) // 8)
        s |= {(7, 8), (2047, 2048), (8191, 8192), (last - 1, last)}
    return sorted(p for p in s if 2 <= p[0] and p[1] <= K - 1)


def pair_row(K, target, seam, family):
    """(tipped, twin) d rows, q = 2, background 0.  tipped: exactly `target` equal pairs over the whole row, one of them a
    pair (e, e) of a non-background value ON `seam`, every other listed seam of the family broken by an isolated cell.
    twin: the same cells with the second e and its right neighbour swapped ([a, e, e, b] -> [a, e, b, e]; at the end of the
    row [a, e, e] -> [e, a, e]): the pair on the seam is broken, nothing else changes, target - 1 pairs."""
    p = seam[0]
    at_end = p + 1 == K - 1
    block = 3 if at_end else 4
    broken = 2 if at_end else 3 if p + 2 == K - 1 else 4         # pairs the block breaks
    tail = p + 4 == K - 1                                        # two cells are left behind the block: cell K - 1 breaks that pair
    want = K - 1 - target - broken - tail                        # boundaries left for the isolated cells: 2 each, 1 at cell 0
    end, n = want % 2, want // 2
    pool = _pair_pool(K, n + end + tail + block)
    vals, cnt = np.unique(pool, return_counts=True)
    e = int(vals[np.argmax(cnt)])
    rest = list(pool)
    rest.remove(e); rest.remove(e)
    others = [v for v in rest if v != e]
    a, b = others[0], others[1 if not at_end else 0]
    rest.remove(a)
    if not at_end:
        rest.remove(b)
    rest = np.random.default_rng([29, K, p]).permutation(np.array(rest, dtype=np.int64))
    # the isolated cells: evenly spread, then one moved onto every other seam, none inside or next to the block
    pos = _spread(K, n)
    lo_b, hi_b = p - 1, p + block - 2                            # the block's cells
    keep = (pos < lo_b - 1) | (pos > hi_b + 1)
    pos = list(pos[keep])
    used = set()
    for other in seams(family, K):
        if other == seam:
            continue
        c = other[0]
        if (c + 1 >= lo_b and c <= hi_b) or (tail and c + 1 == K - 1):
            continue                                             # a cell of the block is in it: broken (checked by the caller)
        if c == hi_b + 1:
            c += 1                                               # (not next to the block: the cell after the pair's first)
        dist = np.abs(np.array(pos) - c)
        dist[list(used)] = K
        near = int(np.argmin(dist))
        pos[near] = c
        used.add(near)
    # cells displaced by the block go where there is room: midway between two neighbours that are far enough apart
    pos = sorted(set(pos))
    while len(pos) < n:
        gaps = np.diff(pos)
        g = int(np.argmax(gaps))
        cand = pos[g] + int(gaps[g]) // 2
        assert gaps[g] >= 4 and not (lo_b - 2 <= cand <= hi_b + 2)
        pos = sorted(pos + [cand])
    pos = np.array(pos, dtype=np.int64)
    assert len(pos) == n and np.all(np.diff(pos) >= 2) and pos[0] >= 2 and pos[-1] <= K - 2
    assert np.all((pos < lo_b - 1) | (pos > hi_b + 1))
    d = np.zeros(K, np.int64)
    d[pos] = rest[:n]
    if end:
        d[0] = rest[n]
    if tail:
        d[K - 1] = rest[n + end]
    twin = None
    if at_end:
        d[K - 3:K] = [a, e, e]
        twin = d.copy()
        twin[K - 3:K] = [e, a, e]
    else:
        d[p - 1:p + 3] = [a, e, e, b]
        twin = d.copy()
        twin[p - 1:p + 3] = [a, e, b, e]
    return d, twin


@functools.lru_cache(maxsize=None)
def _same_pool(K, n):
    """The n cells above the minimum (-1, q = 4) of a row: 0 .. 31, sum K - n, squares 16 K - (K - n)."""
    return solve_multiset(n, 0, 31, K - n, 16 * K - (K - n), np.random.default_rng([31, K, n]))


def same_row(K, n_same, seed=0):
    """q = 4, minimum z = -1/4 in exactly n_same cells; every other cell isolated at position 1 or 2 of a group of four of
    its own (so each breaks two pairs, inside its quad: equal neighbours are as few as `same` allows)."""
    n = K - n_same
    quads = (K - 2) // 4
    assert n <= quads
    rng = np.random.default_rng([37, K, n_same, seed])
    g = np.sort(rng.choice(quads, n, replace=False))
    pos = 4 * g + 1 + rng.integers(0, 2, n)
    d = np.full(K, -1, np.int64)
    d[pos] = rng.permutation(_same_pool(K, n))
    return d


def quad_rows(K, target, g):
    """(tipped, twin) d rows for the register kernel, q = 2, background 0: exactly `target` equal pairs INSIDE aligned
    groups of four.  Quads g and g + 1 hold [a, b, e, e] [c, f, 0, 0]; the twin swaps cells 4 g + 2 and 4 g + 4 —
    [a, b, c, e] [e, f, 0, 0]: the pair (e, e) now straddles the quad boundary and must stop counting (target - 1)."""
    want = 3 * (K // 4) - target - 4                 # pairs the isolated cells break: 2 at position 1 or 2, 1 at position 0
    n_edge, n_mid = want % 2, want // 2
    pool = _pair_pool(K, n_mid + n_edge + 6)
    vals, cnt = np.unique(pool, return_counts=True)
    e = int(vals[np.argmax(cnt)])
    rest = list(pool)
    rest.remove(e); rest.remove(e)
    picks = []
    for _ in range(4):                               # a, b, c, f: pairwise different and different from e
        v = next(v for v in rest if v != e and v not in picks)
        rest.remove(v)
        picks.append(v)
    a, b, c, f = picks
    rest = np.random.default_rng([41, K, g]).permutation(np.array(rest, dtype=np.int64))
    quads = np.array([t for t in range(1, K // 4 - 1) if t not in (g - 1, g, g + 1, g + 2)])
    rng = np.random.default_rng([43, K, g])
    chosen = np.sort(rng.choice(quads, n_mid + n_edge, replace=False))
    d = np.zeros(K, np.int64)
    d[4 * chosen[:n_mid] + 1 + rng.integers(0, 2, n_mid)] = rest[:n_mid]
    if n_edge:
        d[4 * chosen[n_mid]] = rest[n_mid]           # position 0 of its quad: breaks (0, 1) only; the quad before is background
    d[4 * g:4 * g + 8] = [a, b, e, e, c, f, 0, 0]
    twin = d.copy()
    twin[4 * g:4 * g + 8] = [a, b, c, e, e, f, 0, 0]
    return d, twin


def outlier_row(K, two_z, seed=0):
    """q = 2 (z multiples of 1/2): one cell d = two_z (z = two_z / 2), the others -6 .. 6 with the sums that are left."""
    rng = np.random.default_rng([47, K, two_z, seed])
    rest = solve_multiset(K - 1, -6, 6, -two_z, 4 * K - two_z * two_z, rng)
    d = np.empty(K, np.int64)
    col = int(rng.integers(0, K))
    d[np.arange(K) != col] = rng.permutation(rest)
    d[col] = two_z
    return d


def smallest_outlier(K):
    """The smallest d = 2 z (z a multiple of 1/2) with 16 z^2 >= K in float32."""
    t = 1
    while not F32(16) * (F32(t) / F32(2)) ** 2 >= F32(K):
        t += 1
    return t


def two_level_row(K, seed=0):
    """+-1 in equal numbers (q = 1): kurtosis - skewness^2 - 1 == 0."""
    assert K % 2 == 0
    return np.random.default_rng([53, K, seed]).permutation(np.repeat([-1, 1], K // 2))


def three_level_row(K, seed=0):
    """Three levels with sum 0 and sum of squares K (q = 1, z = d): -2, 0, +2 in shares 1 : 6 : 1 (the statistic is 3), or,
    where K is no multiple of 8, -1, 0, +3 in shares 3 : 8 : 1 (the statistic is 2)."""
    if K % 8 == 0:
        cells = np.repeat([-2, 0, 2], [K // 8, 3 * K // 4, K // 8])
    else:
        assert K % 12 == 0
        cells = np.repeat([-1, 0, 3], [K // 4, 2 * K // 3, K // 12])
    return np.random.default_rng([59, K, seed]).permutation(cells)


# ------------------------------------------------------------------ the case tables
# section a: (family, columns, modes).  Modes: "m0" rows as they are; "m1" float32 centre and scale vectors; "m1y" the same
# with y written; "m1a" y aliasing x; "c" a centre vector alone (keeps 1 024 / 4 096 / 8 200 columns off the register routes)
STORE_CASES = [
    ("wave", 64, ("m0",)), ("wave", 96, ("m0",)), ("wave", 100, ("m0", "m1y")), ("wave", 300, ("m0",)),
    ("wave", 1000, ("m0",)), ("wave", 4100, ("m0", "m1y")), ("wave", 8187, ("m0",)),
    ("wave", 1024, ("c",)), ("wave", 4096, ("c",)),
    ("reg", 1024, ("m0", "m1", "m1y")), ("reg", 4096, ("m0", "m1", "m1y")), ("reg", 16384, ("m0", "m1", "m1y")),
    ("rowreg", 8200, ("m0", "m1", "m1y")), ("rowreg", 9999, ("m0", "m1", "m1y")), ("rowreg", 12288, ("m0", "m1y")),
    ("rowreg", 15625, ("m0", "m1y")), ("rowreg", 16383, ("m0", "m1y")), ("rowreg", 65536, ("m0", "m1", "m1y")),
    ("block", 8191, ("m0",)), ("block", 8192, ("m0", "m1y")), ("block", 16807, ("m0", "m1y")), ("block", 19683, ("m0",)),
    ("block", 38400, ("m0",)), ("block", 8200, ("c",)),
    ("wide", 38416, ("m0", "m1", "m1y", "m1a")), ("wide", 40004, ("m0", "m1", "m1y", "m1a")),
]
PRECISIONS = ("fp32", "f16x3", "bf16x3")
# the row loop: (family, columns, rows the launch covers per CU); rows = CUs x that + 3 (the register kernel has no loop:
# one row per wave, four per workgroup — 5 rows there)
ROW_LOOP_CASES = [("wave", 64, 32), ("reg", 4096, 0), ("rowreg", 8200, 1), ("block", 8192, 4), ("wide", 38416, 2)]
# section b: where the thresholds are approached from both sides
# (float32(0.85) * 300 is 255 and float32(0.70) * (K - 1) is an integer at 8 191, 9 991 and 40 001 columns: a threshold met
#  with equality, where `>` for `>=` shows; no such width exists for the register kernel's three)
FLAG_WIDTHS = [("wave", 300), ("block", 8191), ("reg", 1024), ("reg", 16384), ("rowreg", 9999), ("rowreg", 9991),
               ("rowreg", 65536), ("block", 16807), ("wide", 40004), ("wide", 40001)]
# the two-level rule needs +-1 in equal numbers (an even width); the three-level row a multiple of 8 or of 12
LEVEL_WIDTHS = [("wave", 300), ("reg", 1024), ("reg", 16384), ("rowreg", 8200), ("rowreg", 65536), ("block", 8192),
                ("wide", 40008)]
OUTLIER_WIDTHS = [("wave", 4100), ("block", 8191), ("reg", 1024), ("reg", 16384), ("rowreg", 9999), ("rowreg", 65536),
                  ("block", 16807), ("wide", 40004)]
NAN_WIDTHS = [("wave", 300), ("reg", 1024), ("reg", 16384), ("rowreg", 9999), ("rowreg", 65536), ("block", 16807), ("wide", 40004)]


def same_cases(family, K):
    """[(label, Rows of one row, expected coherent)]: `same` at the smallest count that satisfies the float32 comparison
    and at one less."""
    n = smallest_count(same_threshold(K))
    out = []
    for count, flagged in ((n, True), (n - 1, False)):
        r = Rows(same_row(K, count), 4, family, "same = %d" % count).check()
        f = row_flags(r, family)
        assert bool(f["same"][0]) == flagged and not f["levels"][0] and not f["outlier"][0]
        if not flagged:
            assert not f["pairs"][0], "equal neighbours cannot be held clear below the `same` threshold"
        out.append((r.note, r, flagged))
    return out


def pair_cases(family, K):
    """[(label, Rows of one row, expected coherent)]: equal neighbours at the threshold, the pair that tips it on each seam of
    the kernel in turn, and each one's twin at one less."""
    out = []
    if family == "reg":
        target = smallest_count(quad_threshold(K))
        # a quad boundary inside a lane's piece, at the end of a 256-column piece (lane 63 -> lane 0), at the end of the
        # row's first and of its last-but-one 1 024 columns (16 384: another wave)
        for g in sorted(t for t in {5, 63, 255, K // 4 - 3} if t <= K // 4 - 3):
            for d, flagged, what in zip(quad_rows(K, target, g), (True, False), ("inside", "across")):
                r = Rows(d, 2, family, "pair %s the boundary after quad %d" % (what, g)).check()
                out.append((r.note, r, flagged))
    else:
        target = smallest_count(pair_threshold(K))
        for seam in seams(family, K):
            for d, flagged, what in zip(pair_row(K, target, seam, family), (True, False), ("equal", "broken")):
                r = Rows(d, 2, family, "pair %s %s" % (seam, what)).check()
                r.seam = seam
                # every other listed seam is broken
                for other in seams(family, K):
                    assert (d[other[0]] != d[other[1]]) or (other == seam and flagged), (seam, other)
                out.append((r.note, r, flagged))
    for note, r, flagged in out:
        f = row_flags(r, family)
        assert bool(f["pairs"][0]) == flagged and not f["same"][0] and not f["levels"][0] and not f["outlier"][0], note
        same, pairs, quads = counts(r.x)
        assert int(quads[0] if family == "reg" else pairs[0]) == target - (0 if flagged else 1), note
    return out
