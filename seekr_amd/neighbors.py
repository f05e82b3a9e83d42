"""Nearest neighbours by Pearson correlation on MI355X without the r matrix: for every row of one count matrix the k rows
of another (or of itself) it correlates with most.  The reference has no such function; the specification is

    idx[i], val[i] == the first k entries of np.argsort(-r[i], kind="stable") and their r, r = pearson(counts1, counts2)
    as this package computes it in float32, NaN last, row i's own cell left out of the self-comparison.

r is produced one [stripe, panel] block at a time (consumers.Sweep) and consumed by consumers.pearson_topk, so 10^6 rows
need the operands and a block buffer on the device, not 4 TB.
"""
import numpy as np

from seekr_amd import _lib, consumers
from seekr_amd import pearson as pearson_mod


def _f32(c):
    return np.ascontiguousarray(c, dtype=np.float32)


def _prepare(ctx, c1, c2, same):
    """The operands pearson() contracts for float32 counts: SEEKR_PRECISION's layout, and — as skr_pearson's
    match_layouts — one storage kind for both: float32 layout as soon as a fill routes rows of either side there,
    the three-product split when f16f8 operands do not go together."""
    precision = pearson_mod._precision_for(np.dtype(np.float32), True)
    x1 = ctx.from_numpy(c1)
    z1, _ = _lib.operand_fill(ctx, x1, None, precision)
    if same:
        return z1, None
    x2 = ctx.from_numpy(c2)
    z2, _ = _lib.operand_fill(ctx, x2, None, precision)

    def refill(x, z, prec):
        z.free()
        return _lib.operand_fill(ctx, x, None, prec)[0]

    if z1.kind == 3 and z2.kind == 3 and not z1.x8_pair_bound(z2)[1]:
        z1, z2 = refill(x1, z1, _lib.PREC_F16X3), refill(x2, z2, _lib.PREC_F16X3)
    elif z1.kind != z2.kind:
        if z1.kind != 0 and z2.kind != 0:  # an f16f8 operand beside a three-product one
            z1, z2 = (refill(x1, z1, _lib.PREC_F16X3), z2) if z1.kind == 3 else (z1, refill(x2, z2, _lib.PREC_F16X3))
        else:
            z1, z2 = (z1, refill(x2, z2, _lib.PREC_FP32)) if z1.kind == 0 else (refill(x1, z1, _lib.PREC_FP32), z2)
    return z1, z2


@_lib.api_call
def nearest(counts1, counts2=None, k=10, **kw):
    """(idx uint32 [n1, k], val float32 [n1, k]): the k rows of counts2 most correlated with each row of counts1, best
    first, ties to the smaller row; counts2=None (or counts1 itself): counts1 against itself, a row's own cell excluded.
    Slots beyond the number of candidates hold 0xFFFFFFFF / NaN.  Counts of any dtype are ranked in float32 (the lists
    are float32 on the device); `kw`: stripe_rows, panel_rows of consumers.pearson_topk."""
    k = _lib.check_topk_k(k)
    if counts2 is None:
        counts2 = counts1
    c1, c2, _, _, same = pearson_mod._operands(counts1, counts2)
    ctx = _lib.default_context()
    c1 = _f32(c1)
    z1, z2 = _prepare(ctx, c1, c1 if same else _f32(c2), same)
    try:
        return consumers.pearson_topk(z1, z2, k=k, **kw)
    finally:
        z1.free()
        if z2 is not None:
            z2.free()
