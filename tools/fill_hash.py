"""Fingerprints of what skr_operand_fill produces (normalised counts y, and r of the operand against itself) over shapes,
normalisation modes and precisions, on rows that exercise the special cases: zero-variance and NaN columns, a nearly
one-hot row, a constant row, few-valued rows.  Run before and after a change to the fill kernels that must not change
a bit (NaN payloads are canonicalised):  python tools/fill_hash.py > before.txt ; ... ; diff before.txt after.txt
Hashed per case: r (and y where it is kept), and the operand's own bytes; printed next to them the storage kind the operand
ended up with, its coherent flag and whether a NaN was seen.  The default run and --wide together reach all four fill
kernels in every arm (profiles/operand_fill_refactor_hashes.txt)."""
import hashlib, os, sys
sys.path.insert(0, os.getcwd())
import numpy as np
from seekr_amd import _lib as L
if "--lib" in sys.argv:  # another build of the library (before / after across source versions)
    L.LIB_PATH = os.path.abspath(sys.argv[sys.argv.index("--lib") + 1])
WIDE = "--wide" in sys.argv  # the workgroup-per-row kernel: k = 7 rows with float64 vectors (row parked in the LDS), k = 8 rows
ctx = L.default_context()
rng = np.random.default_rng(5)


def canon(m):
    m = m.to_numpy()
    m[np.isnan(m)] = np.float32(np.nan)
    return m.tobytes()


def canon_op(op):
    """The operand's own bytes; NaN cells canonicalised in the element type of the layout (the f16f8 lines as they are)."""
    m = op.as_matrix().to_numpy()
    if op.kind == 0:
        m[np.isnan(m)] = np.float32(np.nan)
    elif op.kind == 1:
        h = m.view(np.uint16)
        h[(h & 0x7FFF) > 0x7F80] = 0x7FC0
    elif op.kind == 2:
        h = m.view(np.float16)
        h[np.isnan(h)] = np.float16(np.nan)
    return m.tobytes()


def data(rows, cols, special=True):
    x = (rng.binomial(1995, 1.0 / 4096, size=(rows, cols)) * np.float32(1000.0 / 1995)).astype(np.float32)
    if special:
        x[5] = 0; x[5, 7] = 3.0                      # nearly one-hot
    x[9, :] = np.float32(0.5)                    # constant row -> NaN after row standardisation
    x[11, ::3] = 7.25
    x[20:20 + rows // 3] = rng.choice([0.0, 0.5, 1.0, 4.0], (rows // 3, cols), p=[0.7, 0.2, 0.09, 0.01]).astype(np.float32)
    return x


def vectors(x, f64, special=True):
    mean = x.mean(0).astype(np.float32); std = x.std(0).astype(np.float32)
    if special:  # a zero-variance and a NaN column: every standardised row is NaN then, y is what these cases pin
        std[3] = 0.0; mean[4] = np.nan
    if f64:  # float64 vectors keep k = 7 rows off the register kernel
        mean, std = mean.astype(np.float64), std.astype(np.float64)
    return mean, std


def case(tag, dx, mean, std, mode, prec, keep_y=True):
    """mode: plain (rows as they are), y (no vectors, normalised counts asked for), zscore, post"""
    rows, cols = dx.rows, dx.cols
    y = ctx.empty(rows, cols) if mode != "plain" and keep_y else None
    kw = {}
    if mode in ("zscore", "post"):
        kw = dict(center=ctx.from_numpy(mean.reshape(1, -1)), scale=ctx.from_numpy(std.reshape(1, -1)))
    if y is not None:
        kw["y"] = y
    if mode == "post":
        kw.update(post=True, shift=7.0)
    op, nan = L.operand_fill(ctx, dx, precision=L.PRECISIONS[prec], want_nan=True, **kw)
    r = ctx.empty(rows, rows)
    L.pearson_gemm_op(ctx, op, op, r, symmetric=True)
    h = hashlib.sha256(canon(r))
    if y is not None:
        h.update(canon(y))
    print(cols, tag, mode if keep_y or mode == "plain" else mode + "-noy", prec, "kind", op.kind, "coherent", int(op.coherent), "nan", nan,
          h.hexdigest()[:16], "operand", hashlib.sha256(canon_op(op)).hexdigest()[:16], flush=True)


for cols, rows in (((16384, 301), (65536, 203), (65544, 57)) if WIDE else ((1024, 3001), (4096, 2503), (16384, 1201), (256, 1500), (729, 900))):
    x = data(rows, cols)
    mean, std = vectors(x, WIDE)
    dx = ctx.from_numpy(x)
    for mode in ("plain", "zscore", "post"):
        for prec in (("f16x3", "fp32") if WIDE else ("f16x3", "bf16x3", "fp32")):
            case("rows", dx, mean, std, mode, prec)
    dx.free()

# ---- the kernels the shapes above do not reach.  "rows": with the nearly one-hot row (the operand is refilled as float32 when
# the width is 1 024 or more), "halves": without it (the split halves themselves are hashed)
if WIDE:
    # row in the registers of sixteen waves, 16 pieces a thread: 4^8 columns with float32 vectors
    x = data(203, 65536, special=False)
    dx = ctx.from_numpy(x)
    mean, std = vectors(x, False, special=False)
    for mode, keep_y in (("plain", True), ("zscore", True), ("post", True), ("post", False)):
        for prec in ("f16x3", "fp32"):
            case("halves", dx, mean, std, mode, prec, keep_y)
    dx.free()
    # workgroup per row: 4^7 columns with y and no vectors (row in the LDS), 7^5 (ragged, row in the LDS), 40 004 (1 024 threads)
    for cols, rows, modes in ((16384, 301, ("y",)), (16807, 257, ("plain", "y", "zscore", "post")), (40004, 131, ("plain", "y", "zscore", "post"))):
        for special in (True, False):
            x = data(rows, cols, special)
            dx = ctx.from_numpy(x)
            mean, std = vectors(x, True, special)
            for mode in modes:
                for prec in ("f16x3", "bf16x3", "fp32"):
                    case("rows" if special else "halves", dx, mean, std, mode, prec)
            dx.free()
else:
    # row in the registers of sixteen waves, 4 pieces a thread: 8 193 .. 16 383 columns, bare and with float32 vectors
    for cols, rows in ((8200, 300), (9999, 300), (15625, 300)):
        for special in (True, False):
            x = data(rows, cols, special)
            dx = ctx.from_numpy(x)
            mean, std = vectors(x, False, special)
            for mode, keep_y in (("plain", True), ("zscore", True), ("zscore", False), ("post", True), ("post", False)):
                for prec in ("f16x3", "bf16x3", "fp32"):
                    case("rows" if special else "halves", dx, mean, std, mode, prec, keep_y)
            dx.free()
    # wave per row, sums in numpy's order
    for cols, rows in ((16, 700), (100, 700)):
        x = data(rows, cols)
        dx = ctx.from_numpy(x)
        mean, std = vectors(x, False)
        for mode in ("plain", "zscore", "post"):
            for prec in ("f16x3", "fp32"):
                case("rows", dx, mean, std, mode, prec)
        dx.free()
    # f16f8: dense Gaussian rows keep the H / X lines (kind 3), the few-valued rows above are routed back (kind 2)
    for cols, rows in ((4096, 1201), (16384, 601)):
        g = rng.standard_normal((rows, cols)).astype(np.float32)
        gm, gs = vectors(g, False, special=False)
        dg = ctx.from_numpy(g)
        for mode in ("plain", "zscore", "post"):
            case("gaussian", dg, gm, gs, mode, "f16f8")
        dg.free()
        x = data(rows, cols, special=False)
        dx = ctx.from_numpy(x)
        mean, std = vectors(x, False, special=False)
        for mode in ("plain", "zscore", "post"):
            case("halves", dx, mean, std, mode, "f16f8")
        dx.free()
