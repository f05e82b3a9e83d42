"""Every Pearson contraction kernel, mode and A/B knob against integer arithmetic (tests/exact_sum_cases.py): rows whose
products and partial sums are all exactly representable in the accumulator, so that the stored r is one division away
from an int64 sum whatever the tiling, the phase order, the wave geometry, the k chunking, mirror or swapped form.  The
comparisons are uint32 / uint64 equality with a few-line numpy model — no tolerance and no second kernel; only the
patched diagonal of a self-comparison beyond 4 096 columns holds to a derived bound (its float32 sum of squares is not
exact there).  Needs a real MI355X: run with `-m gpu`."""
import contextlib
import os

import numpy as np
import pytest

import exact_sum_cases as ec

pytestmark = pytest.mark.gpu

KNOB_NAMES = ("SEEKR_GEMM_LOOP", "SEEKR_GEMM_EPILOGUE", "SEEKR_GEMM_PERSIST", "SEEKR_GEMM_CHUNK_TILES")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


@pytest.fixture(scope="module")
def L():
    from seekr_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def ctx(L):
    return L.default_context()


@contextlib.contextmanager
def knobs(ctx, **env):
    """The contraction's A/B switches, switched in-process (ctx.reload_knobs) and put back whatever happens."""
    before = {k: os.environ.get(k) for k in KNOB_NAMES}
    try:
        for k in KNOB_NAMES:
            os.environ.pop(k, None)
        for k, v in env.items():
            if v:
                os.environ[k] = str(v)
        ctx.reload_knobs()
        yield
    finally:
        for k, v in before.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        ctx.reload_knobs()


class Tally:
    """Collects every mode of a case before failing, so that one run shows which arms disagree with the model."""

    def __init__(self):
        self.bad = []

    def same(self, label, got, want):
        got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
        if got.shape != want.shape or got.dtype != want.dtype:
            self.bad.append((label, "shape / dtype", got.shape, want.shape))
            return
        diff = bits(got) != bits(want)
        if diff.any():
            at = tuple(int(v) for v in np.argwhere(diff)[0])
            self.bad.append((label, "%d of %d cells differ, first at %s: %r vs the model's %r"
                             % (int(diff.sum()), diff.size, at, got[at], want[at])))

    def done(self):
        assert not self.bad, self.bad


_prepared = {}


def prepared(L, ctx, precision, cols, m, n):
    """The case's rows on the device and what the host knows about them; the last case is kept (the tests of one case
    follow each other)."""
    key = (precision, cols, m, n)
    if key not in _prepared:
        _prepared.clear()
        a, b = ec.split_case(precision, cols, m, n)
        ec.check_split_conditions(a, b)     # the conditions, before anything is launched
        ec.check_split_conditions(a, a)
        ops = []
        for s in (a, b):
            op, _ = L.operand_fill(ctx, ctx.from_numpy(s.x), precision=L.PRECISIONS[precision], row_standardize=False)
            assert op.kind == ec.KIND[precision], ("not on the split kernel", precision, cols, op.kind)
            kt = (cols + 31) // 32
            got = op.as_matrix().to_numpy().view(np.uint16).reshape(s.rows, kt, 2, 32)
            assert np.array_equal(got, s.stored), ("stored halves", np.argwhere(got != s.stored)[:5])
            ops.append(op)
        _prepared[key] = dict(a=a, b=b, za=ops[0], zb=ops[1], models={})
    return _prepared[key]


def models(p, chunk_tiles):
    """(r of a against b, r of a against itself with the patched diagonal, which diagonal cells are exact)."""
    a, b = p["a"], p["b"]
    key = tuple(ec.k_chunks(a.cols, chunk_tiles))
    if key not in p["models"]:
        r_ab = ec.split_model(a, b, chunk_tiles)
        r_aa = ec.split_model(a, a, chunk_tiles)
        assert np.array_equal(bits(r_aa), bits(r_aa.T.copy()))
        diag, exact = ec.split_diag_model(a)
        r_aa[np.arange(a.rows), np.arange(a.rows)] = diag
        p["models"][key] = (r_ab, r_aa, exact)
    return p["models"][key]


def same_self(t, label, got, r_aa, exact, cols):
    """A self-comparison: every cell off the diagonal and every exact diagonal cell by its bits; the other diagonal cells
    (sum of squares beyond 24 bits) within K 2^-24 relative, the worst case of any float32 order over K non-negative terms."""
    i = np.arange(r_aa.shape[0])
    d_got, d_want = got[i, i], r_aa[i, i]
    loose = ~exact
    if loose.any() and not (np.abs(d_got[loose].astype(np.float64) - d_want[loose]) <= cols * 2.0 ** -24 * d_want[loose]).all():
        t.bad.append((label, "diagonal outside K 2^-24"))
    got = got.copy()
    got[i[loose], i[loose]] = d_want[loose]
    t.same(label, got, r_aa)


def self_block(L, ctx, za):
    r = ctx.zeros(za.rows, za.rows)
    L.pearson_gemm_op(ctx, za, za, r, symmetric=True)
    return r.to_numpy()


def plain_block(L, ctx, za, zb):
    r = ctx.zeros(za.rows, zb.rows)
    L.pearson_gemm_op(ctx, za, zb, r)
    return r.to_numpy()


@pytest.mark.parametrize("precision,cols,chunk_tiles,m,n", ec.SPLIT_CASES)
def test_split_modes_give_the_integer_model(L, ctx, precision, cols, chunk_tiles, m, n):
    """SELF, PLAIN, PLAIN at an unaligned column offset, LOWER, both blocks of the mirror call, row stripes of 512 and the
    fused edge list (cutoff ON a value of r and one float above it; cutoff 0 and the smallest value of r, which list a
    cell of exactly 0 unless the `r != 0` rule holds; each with and without upper_only)."""
    from seekr_amd import consumers
    p = prepared(L, ctx, precision, cols, m, n)
    za, zb = p["za"], p["zb"]
    r_ab, r_aa, exact = models(p, ec.model_chunk_tiles(chunk_tiles))
    t = Tally()
    with knobs(ctx, SEEKR_GEMM_CHUNK_TILES=chunk_tiles):
        same_self(t, "self", self_block(L, ctx, za), r_aa, exact, cols)
        t.same("plain", plain_block(L, ctx, za, zb), r_ab)
        wide = ctx.zeros(m, n + 8)           # rows of the target start off a 16-byte boundary; the frame stays zero
        L.pearson_gemm_op(ctx, za, zb, wide, row0=0, col0=3)
        want = np.zeros((m, n + 8), np.float32)
        want[:, 3:3 + n] = r_ab
        t.same("plain at col0 = 3", wide.to_numpy(), want)
        lower = ctx.zeros(m, n)
        L.pearson_gemm_op(ctx, za, zb, lower, lower=True)
        t.same("lower", lower.to_numpy(), r_ab)
        r, rt = ctx.zeros(m, n), ctx.zeros(n, m)
        L.pearson_gemm_op_mirror(ctx, za, zb, r, 0, 0, rt, 0, 0)
        t.same("mirror: block", r.to_numpy(), r_ab)
        t.same("mirror: transposed block", rt.to_numpy(), r_ab.T.copy())
        rows = ctx.zeros(m, m)
        for r0 in range(0, m, 512):
            L.pearson_gemm_op_rows(ctx, za.view(r0, min(512, m - r0)), za, r0, rows, r0)
        same_self(t, "rows in stripes of 512", rows.to_numpy(), r_aa, exact, cols)
        cutoff = ec.pick_cutoff(r_ab)
        above = np.nextafter(cutoff, np.float32(np.inf))
        zero, lowest = ec.low_cutoffs(r_ab)
        if m >= ec.ZERO_CELL_ROWS:           # the zero rule can be seen: cells of exactly 0 that both low cutoffs would list
            assert ec.zero_cells(r_ab) > 0
        names = {0: "on a value", 1: "one float above", 2: "0", 3: "the smallest r"}
        fe = consumers.FusedEdges(ctx)
        try:
            for upper in (False, True):
                for which, c in enumerate((cutoff, above, zero, lowest)):
                    got = ec.sort_edges(*fe.block(za, zb, float(c), row_global0=7, col_global0=11, upper_only=upper))
                    want = ec.edges_model(r_ab, c, 7, 11, upper)
                    label = "edges upper_only=%s cutoff %s" % (upper, names[which])
                    assert (want[2] == cutoff).any() == (which != 1) and not (want[2] == 0).any()
                    for g, w in zip(got, want):
                        t.same(label, g, w)
        finally:
            fe.free()
    t.done()


KNOBS = [dict(SEEKR_GEMM_LOOP="0"), dict(SEEKR_GEMM_EPILOGUE="0"), dict(SEEKR_GEMM_EPILOGUE="1"),
         dict(SEEKR_GEMM_EPILOGUE="2"), dict(SEEKR_GEMM_EPILOGUE="3"), dict(SEEKR_GEMM_PERSIST="0")]


@pytest.mark.parametrize("precision,cols,chunk_tiles,m,n", ec.SPLIT_CASES)
def test_split_knobs_give_the_integer_model(L, ctx, precision, cols, chunk_tiles, m, n):
    """PLAIN and SELF again under every A/B switch of the contraction — the present loop, the general epilogue and each
    run length of the lean one, the non-persistent launch — and with the operand's own chunking (128 k tiles, 32 for
    'coherent' rows, the flag set here by hand): each against the model, never against another arm."""
    p = prepared(L, ctx, precision, cols, m, n)
    za, zb = p["za"], p["zb"]
    t = Tally()
    flags = (za.coherent, zb.coherent)
    try:
        for env in KNOBS:
            r_ab, r_aa, exact = models(p, ec.model_chunk_tiles(chunk_tiles))
            with knobs(ctx, SEEKR_GEMM_CHUNK_TILES=chunk_tiles, **env):
                same_self(t, "self %s" % env, self_block(L, ctx, za), r_aa, exact, cols)
                t.same("plain %s" % env, plain_block(L, ctx, za, zb), r_ab)
        for coherent in (False, True):      # the default chunking: set, not taken from what the fill thought of the rows
            za.coherent = zb.coherent = coherent
            r_ab, r_aa, exact = models(p, 32 if coherent else 128)
            with knobs(ctx):
                same_self(t, "self coherent=%s" % coherent, self_block(L, ctx, za), r_aa, exact, cols)
                t.same("plain coherent=%s" % coherent, plain_block(L, ctx, za, zb), r_ab)
    finally:
        za.coherent, zb.coherent = flags
    t.done()


# ------------------------------------------------------------------ the fp32 kernel
@pytest.mark.parametrize("m,n,cols", ec.F32_SHAPES)
def test_fp32_kernel_gives_the_integer_model(L, ctx, m, n, cols):
    """Through skr_pearson_gemm (PREC_FP32) and through operands of kind 0 (the float32 layout, and bf16 halves asked for
    below their 1 024 columns): plain, self, the mirror call, row stripes, and a self-comparison whose block starts at
    (3, 3) of a wider matrix — rows of r off a 16-byte boundary, the mirror's 16-byte stores with them."""
    a, b = ec.f32_case(m, n, cols)
    r_ab, r_aa = ec.f32_model(a, b), ec.f32_model(a, a)
    da, db = ctx.from_numpy(a), ctx.from_numpy(b)
    t = Tally()
    r = ctx.zeros(m, n)
    L.pearson_gemm(ctx, da, db, r, precision=L.PREC_FP32)
    t.same("gemm plain", r.to_numpy(), r_ab)
    r = ctx.zeros(m, m)
    L.pearson_gemm(ctx, da, da, r, precision=L.PREC_FP32, symmetric=True)
    t.same("gemm self", r.to_numpy(), r_aa)
    wide = ctx.zeros(m + 5, m + 5)
    L.pearson_gemm(ctx, da, da, wide, precision=L.PREC_FP32, symmetric=True, row0=3, col0=3)
    want = np.zeros((m + 5, m + 5), np.float32)
    want[3:3 + m, 3:3 + m] = r_aa
    t.same("gemm self at (3, 3)", wide.to_numpy(), want)
    precisions = [L.PREC_FP32] + ([L.PREC_BF16X3] if cols < 1024 else [])
    for prec in precisions:
        za, _ = L.operand_fill(ctx, da, precision=prec, row_standardize=False)
        zb, _ = L.operand_fill(ctx, db, precision=prec, row_standardize=False)
        assert za.kind == 0 and zb.kind == 0
        r = ctx.zeros(m, n + 8)
        L.pearson_gemm_op(ctx, za, zb, r, col0=3)
        want = np.zeros((m, n + 8), np.float32)
        want[:, 3:3 + n] = r_ab
        t.same("op plain at col0 = 3 (%d)" % prec, r.to_numpy(), want)
        r = ctx.zeros(m, m)
        L.pearson_gemm_op(ctx, za, za, r, symmetric=True)
        t.same("op self (%d)" % prec, r.to_numpy(), r_aa)
        r, rt = ctx.zeros(m, n), ctx.zeros(n, m)
        L.pearson_gemm_op_mirror(ctx, za, zb, r, 0, 0, rt, 0, 0)
        t.same("op mirror (%d)" % prec, r.to_numpy(), r_ab)
        t.same("op mirror, transposed (%d)" % prec, rt.to_numpy(), r_ab.T.copy())
        rows = ctx.zeros(m, m)
        for r0 in range(0, m, 100):
            L.pearson_gemm_op_rows(ctx, za.view(r0, min(100, m - r0)), za, r0, rows, r0)
        t.same("op rows (%d)" % prec, rows.to_numpy(), r_aa)
    t.done()


# ------------------------------------------------------------------ the float64 kernels
def f64_rows(a, stored, beyond):
    """Rows of `stored` >= K columns: the integers, then `beyond` in every column past K."""
    out = np.full((a.shape[0], stored), float(beyond))
    out[:, :a.shape[1]] = a
    return out


@pytest.mark.parametrize("cols", ec.F64_WIDTHS)
def test_float64_kernels_give_the_integer_model(L, ctx, cols):
    """skr_pearson_gemm_f64 on both sides of its kernel choice (whole 16-column stages in rows of even pitch: the tiled
    kernel; anything else: one wave per tile): rows exactly K wide, zero-padded to whole stages, padded to an odd pitch,
    and wider rows that hold 2^20 beyond K — r = <a_i, b_j> / K over the first K columns, so it must not move."""
    t = Tally()
    k16 = (cols + 15) // 16 * 16
    layouts = [(cols, 0.0), (k16, 0.0), (k16 + 1, 0.0), (k16 + 16, 2.0 ** 20), (cols + 1, 2.0 ** 20)]
    for m, n in ec.F64_SHAPES:
        a, b = ec.f64_case(m, n, cols)
        r_ab, r_aa = ec.f64_model(a, b), ec.f64_model(a, a)
        for stored, beyond in layouts:
            label = "%d x %d, K = %d in rows of %d (%g beyond K)" % (m, n, cols, stored, beyond)
            da, db = ctx.from_numpy(f64_rows(a, stored, beyond)), ctx.from_numpy(f64_rows(b, stored, beyond))
            # plain, at an offset inside a wider zeroed matrix
            r = ctx.zeros(m + 3, n + 4, np.float64)
            L.pearson_gemm_f64(ctx, da, db, r, cols, row0=2, col0=3)
            want = np.zeros((m + 3, n + 4))
            want[2:2 + m, 3:3 + n] = r_ab
            t.same("plain, " + label, r.to_numpy(), want)
            # a self-comparison in stripes, as pearson() cuts it: left of the diagonal block, the block itself
            # (symmetric, at col0 = s0), right of it
            stripe = max(1, m // 2 + 1)
            got = np.empty((m, m))
            buf = ctx.zeros(stripe, m, np.float64)
            for s0 in range(0, m, stripe):
                h = min(stripe, m - s0)
                za = da.view(s0, h)
                if s0:
                    L.pearson_gemm_f64(ctx, za, da.view(0, s0), buf, cols)
                L.pearson_gemm_f64(ctx, za, za, buf, cols, symmetric=True, col0=s0)
                if s0 + h < m:
                    L.pearson_gemm_f64(ctx, za, da.view(s0 + h, m - s0 - h), buf, cols, col0=s0 + h)
                got[s0:s0 + h] = buf.to_numpy(0, h)
            t.same("self in stripes, " + label, got, r_aa)
    t.done()


def test_float64_whole_call_gives_the_integer_model(L, ctx):
    """skr_pearson_gemm on float64 matrices (PREC_F64): K = the stored width, symmetric and plain."""
    t = Tally()
    for cols in (12, 48, 1000):
        a, b = ec.f64_case(129, 127, cols)
        da, db = ctx.from_numpy(a.astype(np.float64)), ctx.from_numpy(b.astype(np.float64))
        r = ctx.zeros(129, 127, np.float64)
        L.pearson_gemm(ctx, da, db, r, precision=L.PREC_F64)
        t.same("plain %d" % cols, r.to_numpy(), ec.f64_model(a, b))
        r = ctx.zeros(129, 129, np.float64)
        L.pearson_gemm(ctx, da, da, r, precision=L.PREC_F64, symmetric=True)
        t.same("self %d" % cols, r.to_numpy(), ec.f64_model(a, a))
    t.done()
