"""The two specifications of seekr_amd.explain as numpy models — row-by-row loops in float32 — and the inputs the CPU and
GPU tests share.

pair_model: per pair c = z1[row] * z2[col] (one float32 rounding per cell); the list is the first `top` columns in the
order (value descending, -0 == +0, NaN after every number, ties to the smaller column) of c (largest) or of -c.  The
order is written out here as three explicit sort keys; test_explain_cpu checks that it is np.argsort(-key, kind="stable").

group_model: np.mean(x[sel], axis=0) and np.std(x[sel], axis=0, ddof=1) as the chains numpy runs on a C-contiguous float32
matrix of two or more columns: the rows are added one after the other to one float32 accumulator per column that starts
at +0 (a column of -0 sums to +0); mean = acc / n; the same chain over fl32(fl32(x - mean)^2); sd = sqrt(acc2 / (n - 1)).  At one
column numpy adds pairwise instead, and this model — not numpy — is the specification there.  A NaN result is written as
the quiet NaN 0x7FC00000 (numpy hands on whichever NaN the processor makes; the tests compare numpy's with isnan).
"""
import functools

import numpy as np

PAD_IDX, PAD_BITS = 0xFFFFFFFF, 0x7FC00000


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- pairs ---------------------------------------------------------------------------------------------------------------
def model_order(key):
    """The columns of the float32 vector `key`, best first: value descending, -0 == +0, NaN last, ties to the smaller
    column — three sort keys, no reliance on how a sort treats NaN or signed zeros."""
    key = np.asarray(key, dtype=np.float32)
    nan = np.isnan(key)
    value = np.where(nan | (key == 0), np.float32(0), key)  # one zero; NaN cells are ranked by the first key alone
    with np.errstate(invalid="ignore"):
        return np.lexsort((np.arange(len(key)), -value, nan))


def pair_model(z1, z2, rows, cols, top, largest=True):
    """(idx uint32, val, f1, f2 float32), each [E, top]; pads 0xFFFFFFFF / 0x7FC00000 beyond the width."""
    z1, z2 = np.asarray(z1, dtype=np.float32), np.asarray(z2, dtype=np.float32)
    n = len(rows)
    idx = np.full((n, top), PAD_IDX, np.uint32)
    val, f1, f2 = (np.full((n, top), PAD_BITS, np.uint32).view(np.float32) for _ in range(3))
    m = min(top, z1.shape[1])
    with np.errstate(all="ignore"):
        for e in range(n):
            a, b = z1[int(rows[e])], z2[int(cols[e])]
            c = a * b
            order = model_order(c if largest else -c)[:m]
            idx[e, :m], val[e, :m], f1[e, :m], f2[e, :m] = order, c[order], a[order], b[order]
    return idx, val, f1, f2


PAIR_WIDTHS = [1, 2, 3, 4, 5, 7, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 1027, 2049, 4096, 4099, 15625, 16384]
PAIR_TOPS = [1, 2, 10, 64, 256]


def pair_rows(n, w, seed):
    """n rows of w float32 cells: the first half normal, the second half small multiples of 1/4 with zeros of both signs, so
    that products between them tie and are -0 and +0."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, w)).astype(np.float32)
    q = (rng.integers(-3, 4, (n - n // 2, w)) / 4.0).astype(np.float32)
    q[np.logical_and(q == 0, rng.random(q.shape) < 0.5)] = np.float32(-0.0)
    x[n // 2:] = q
    return x


def all_pairs(n1, n2=None):
    n2 = n1 if n2 is None else n2
    r, c = np.divmod(np.arange(n1 * n2), n2)
    return r.astype(np.uint32), c.astype(np.uint32)


def stress_rows(w=4099):
    """Rows whose products are ascending with the column (every step beats the bound), descending, all equal, and of two
    values: pair (0, 4), (1, 4), (4, 4), (2, 4) and (3, 4)."""
    rng = np.random.default_rng(404)
    up = np.arange(w, dtype=np.float32) - np.float32(w // 2)
    two = rng.choice(np.array([1.0, 2.0], np.float32), w)
    return np.stack([up, up[::-1].copy(), two, -two, np.ones(w, np.float32)])


def special_rows(w=300):
    """(z1, z2): rows that make products NaN, -0 and +0, inf, overflow to inf, subnormal from normal factors, and normal or
    subnormal from subnormal factors; every row of z1 meets every row of z2."""
    rng = np.random.default_rng(505)
    base = rng.standard_normal((6, w)).astype(np.float32)
    z1, z2 = base.copy(), rng.standard_normal((6, w)).astype(np.float32)
    z1[0, ::7] = np.nan
    z1[1, ::3] = 0.0
    z1[1, 1::3] = -0.0
    z1[2, ::5] = np.inf
    z1[2, 1::5] = -np.inf
    z1[3] = base[3] * np.float32(1e30)
    z1[4] = base[4] * np.float32(1e-20)
    z1[5] = base[5] * np.float32(1e-41)  # subnormal factors
    z2[0, 3::11] = np.nan
    z2[1, ::2] = -0.0
    z2[2, ::5] = 0.0  # inf * 0 = NaN
    z2[3] *= np.float32(1e30)
    z2[4] *= np.float32(1e-20)
    z2[5] *= np.float32(1e3)
    return z1, z2


# ---- groups --------------------------------------------------------------------------------------------------------------
def group_model(x, order, starts, want_sd=True):
    """(mean, sd) float32 [G, W] of the rows order[starts[g] : starts[g + 1]] of x; sd None without want_sd."""
    x = np.asarray(x, dtype=np.float32)
    g_n, w = len(starts) - 1, x.shape[1]
    mean = np.empty((g_n, w), np.float32)
    sd = np.empty((g_n, w), np.float32) if want_sd else None
    with np.errstate(all="ignore"):
        for g in range(g_n):
            sel = [int(i) for i in order[int(starts[g]):int(starts[g + 1])]]
            n = len(sel)
            if n == 0:
                mean[g] = np.nan
                if want_sd:
                    sd[g] = np.nan
                continue
            acc = np.zeros(w, np.float32)
            for i in sel:
                acc = acc + x[i]
            mean[g] = acc / np.float32(n)
            if not want_sd:
                continue
            acc2 = np.zeros(w, np.float32)
            for i in sel:
                d = x[i] - mean[g]
                acc2 = acc2 + d * d
            sd[g] = np.sqrt(acc2 / np.float32(n - 1))
    # which NaN an operation hands on (sign, payload) differs between processors: a NaN result is THE quiet NaN 0x7FC00000
    for a in (mean, sd):
        if a is not None:
            a.view(np.uint32)[np.isnan(a)] = PAD_BITS
    return mean, sd


def order_of(labels):
    """(unique, order uint32, starts int64) in np.unique order, rows ascending within a label."""
    uniq, inverse = np.unique(np.asarray(labels), return_inverse=True)
    inverse = inverse.reshape(-1)
    order = np.argsort(inverse, kind="stable").astype(np.uint32)
    starts = np.concatenate([[0], np.cumsum(np.bincount(inverse, minlength=len(uniq)))]).astype(np.int64)
    return uniq, order, starts


GROUP_WIDTHS = [2, 3, 15, 16, 17, 31, 33, 64, 625, 4096, 4099]
# the sizes the issue names, the same three around this kernel's 256-row tile, and the walker's first four rows
GROUP_SIZES = [1, 2, 3, 511, 512, 513, 1025, 255, 256, 257, 4, 5]
GROUP_LABELS = np.array([-7, 1000, 3, -1, 2 ** 40, 10, 5, 17, -300, 64, 0, 2 ** 33], dtype=np.int64)


@functools.lru_cache(maxsize=None)
def interleaved_labels():
    """int64 labels (negative, non-consecutive, beyond 32 bits) of GROUP_SIZES rows each, shuffled into the row order."""
    rng = np.random.default_rng(606)
    labels = np.repeat(GROUP_LABELS, GROUP_SIZES)
    rng.shuffle(labels)
    return labels


def group_matrix(n, w, seed):
    """Values like 10^4 + noise: a float32 chain over them rounds at every step, so the order of the additions shows."""
    rng = np.random.default_rng(seed)
    return (1e4 + 50.0 * rng.standard_normal((n, w))).astype(np.float32)


def discriminating_group(w=16):
    """1 025 rows for one group whose sequential float32 mean differs in bits from float32(float64 mean) in at least one
    column (checked in test_explain_cpu): a kernel that reduced by a tree would not reproduce it."""
    return group_matrix(1025, w, 707)
