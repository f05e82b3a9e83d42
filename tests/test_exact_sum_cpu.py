"""The exact-sum inputs of tests/exact_sum_cases.py, checked without a GPU: every case the GPU tests launch meets the
conditions that make it exact (DESIGN_PARITY.md, "Exact-sum inputs"), the model does not depend on the order of the sum,
and the inputs can see what the GPU tests claim to see — each mutant of the model (a k element skipped or counted twice,
a cross term dropped or doubled, a chunk folded in twice, a `>` for a `>=`) changes the bits of at least half the cells."""
import numpy as np
import pytest

import exact_sum_cases as ec


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def changed(a, b):
    return float((bits(a) != bits(b)).mean())


PAIRS = sorted({(p, k, m, n) for p, k, _, m, n in ec.SPLIT_CASES})


@pytest.mark.parametrize("precision,cols,m,n", PAIRS)
def test_every_gpu_case_meets_the_conditions(precision, cols, m, n):
    a, b = ec.split_case(precision, cols, m, n)
    worst, worst_self = ec.check_split_conditions(a, b), ec.check_split_conditions(a, a)
    cross = ec.cross_share(a, b)
    cross_self = ec.cross_share(a, a) if m <= 300 else cross
    print("%s K=%d %dx%d: bound on the worst subset sum %.2f / %.2f of 2^23 U, cells with a cross term %.2f / %.2f"
          % (precision, cols, m, n, worst, worst_self, cross, cross_self))
    assert min(cross, cross_self) >= 0.5
    if m <= 300 and cols <= 4128:       # the per-pair figure the bound stands for, where it is cheap to form
        exact_ab, exact_aa = ec.worst_subset_sum(a, b), ec.worst_subset_sum(a, a)
        print("    per pair: max(sum of positive products, |sum of negative products|) %.2f / %.2f" % (exact_ab, exact_aa))
        assert exact_ab <= worst and exact_aa <= worst_self
    # the fine cells exist, their lo half is not 0, and both rounding directions occur among them (fp16)
    fine = np.abs(a.n) > 1000
    assert fine.any(axis=1).all() and (a.lo[fine] != 0).all() and (a.lo[~fine] == 0).all()
    if precision == "f16x3" and m >= 40:
        up = a.hi[fine] * np.sign(a.n[fine]) > np.abs(a.n[fine])
        assert up.any() and (~up).any()
    # the stored patterns are the halves
    if precision == "f16x3":
        assert np.array_equal(a.stored[:, :, 0, :].reshape(m, -1)[:, :cols].view(np.float16).astype(np.float32), a.hi)
    # the diagonal of a self-comparison
    value, exact = ec.split_diag_model(a)
    if cols <= 4096:
        assert exact.all()
    # the same sum in float32, in three orders: the bits of the model where it claims them, the derived bound elsewhere
    x2 = a.x[:300].astype(np.float32) ** 2
    value, exact = value[:300], exact[:300]
    for order in (np.arange(cols), np.arange(cols)[::-1], np.random.default_rng(0).permutation(cols)):
        got = np.add.reduce(x2[:, order], axis=1, dtype=np.float32) / np.float32(cols)
        assert np.array_equal(bits(got[exact]), bits(value[exact]))
        assert (np.abs(got - value) <= cols * 2.0 ** -24 * value).all()


SMALL = [c for c in ec.SPLIT_CASES if c[3] <= 300 and c[1] <= 4128 or c[3] <= 5]


@pytest.mark.parametrize("precision,cols,chunk_tiles,m,n", SMALL)
def test_the_model_is_free_of_the_order(precision, cols, chunk_tiles, m, n):
    """Shuffled k (within the chunks, so that the per-chunk division of the widths that are no power of two stays the
    model's), and float32 sums in three blockings: the same bits."""
    a, b = ec.split_case(precision, cols, m, n)
    ct = ec.model_chunk_tiles(chunk_tiles)
    want = ec.split_model(a, b, ct)
    kdiv = ec.split_kdiv(a, b)
    rng = np.random.default_rng(cols)
    for block in ((5, 32, 257) if cols <= 4096 else (32, 257, 1000)):       # float32 running sums, `block` columns at a time, the three products one by one
        sums = []
        for c0, c1 in ec.k_chunks(cols, ct):
            order = c0 + rng.permutation(c1 - c0)
            acc = np.zeros((m, n), np.float32)
            for k0 in range(0, order.size, block):
                k = order[k0:k0 + block]
                for p, q in ec.PRODUCTS:
                    acc = acc + getattr(a, p)[:, k] @ getattr(b, q)[:, k].T   # a float32 matmul, then a float32 add
            sums.append(acc.astype(np.float64))
        assert np.array_equal(bits(ec.fold(sums, kdiv)), bits(want)), block
    if cols & (cols - 1) == 0:          # a power of two: fl32(S / K) whatever the chunking
        for other in (1, 3, 32, 1 << 20):
            assert np.array_equal(bits(ec.split_model(a, b, other)), bits(want)), other


@pytest.mark.parametrize("precision,cols,chunk_tiles,m,n", ec.SPLIT_CASES)
def test_mutants_of_the_model_show(precision, cols, chunk_tiles, m, n):
    a, b = ec.split_case(precision, cols, m, n)
    ct = ec.model_chunk_tiles(chunk_tiles)
    kdiv = ec.split_kdiv(a, b)
    prods = ec.chunk_products(a, b, ct)
    sums = [p[0] + p[1] + p[2] for p in prods]
    want = ec.fold(sums, kdiv)

    def piece(c0, c1):
        return sum(ec._dot(getattr(a, p), getattr(b, q), c0, c1) for p, q in ec.PRODUCTS)

    mutants = {
        "last column dropped": sums[:-1] + [sums[-1] - piece(cols - 1, cols)],
        "first k tile counted twice": [sums[0] + piece(0, 32)] + sums[1:],
        "lo_a hi_b dropped": [p[0] + p[1] for p in prods],
        "hi_a lo_b doubled": [p[0] + 2 * p[1] + p[2] for p in prods],
        "one chunk added twice": sums + [sums[-1]],
    }
    for name, mutant in mutants.items():
        share = changed(ec.fold(mutant, kdiv, exact=False), want)   # (a mutant's sum may leave float32: plainly rounded)
        assert share >= 0.5, (name, share)
    # `>` for `>=`: at a cutoff that occurs in r the two lists differ, one float above it they do not
    cutoff = ec.pick_cutoff(want)
    ge = ec.edges_model(want, cutoff, 7, 11, False)
    gt_rows = ec.edges_model(want, np.nextafter(np.float32(cutoff), np.float32(np.inf)), 7, 11, False)
    assert len(ge[0]) > len(gt_rows[0]) and (ge[2] == cutoff).any() and not (gt_rows[2] == cutoff).any()
    # the zero rule dropped: at cutoff 0 and at the smallest r the list gains the cells of exactly 0 — which exist above
    # the global diagonal in every case of 257 rows and more (the 3 x 5 and 40 x 64 blocks are too small to hold one)
    if m >= ec.ZERO_CELL_ROWS:
        assert ec.zero_cells(want) > 0
        for c in ec.low_cutoffs(want):
            for upper in (False, True):
                kept, mutant = ec.edges_model(want, c, 7, 11, upper), ec.edges_model(want, c, 7, 11, upper, zero_rule=False)
                assert len(mutant[0]) - len(kept[0]) >= ec.zero_cells(want) and not (kept[2] == 0).any() and (mutant[2] == 0).any()


@pytest.mark.parametrize("m,n,cols", ec.F32_SHAPES)
def test_fp32_cases(m, n, cols):
    a, b = ec.f32_case(m, n, cols)
    want = ec.f32_model(a, b)
    got = (a[:, ::-1] @ b[:, ::-1].T) / np.float32(cols)      # float32 sums, another order
    assert np.array_equal(bits(got), bits(want))
    assert changed(ec.f32_model(a[:, :-1], b[:, :-1], cols), want) >= 0.5 or m * n == 1


@pytest.mark.parametrize("cols", ec.F64_WIDTHS)
def test_float64_cases(cols):
    for m, n in ec.F64_SHAPES:
        a, b = ec.f64_case(m, n, cols)
        want = ec.f64_model(a, b)
        af, bf = a.astype(np.float64), b.astype(np.float64)
        assert float((np.abs(af) @ np.abs(bf).T).max()) < 2.0 ** 53
        assert np.array_equal(bits((af[:, ::-1] @ bf[:, ::-1].T) / cols), bits(want))
        if m * n > 1:
            assert changed((a[:, :-1] @ b[:, :-1].T).astype(np.float64) / np.float64(cols), want) >= 0.5
