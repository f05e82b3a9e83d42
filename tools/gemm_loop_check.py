"""The phased k loop of the split contraction (pearson_bf16.hip, SEEKR_GEMM_LOOP=1; schedule: gemm_phased_schedule.hpp) against
the present loop (SEEKR_GEMM_LOOP=0): the SAME BITS, compared as uint32, in SELF, PLAIN, PLAIN at an unaligned column
offset, CROSS with mirror, row-stripe (LOWER + SELF + PLAIN) and thresholding mode, for both split precisions, at widths of
1, 2, 3, 5 and 8 k tiles (shorter than, equal to and just past the prefetch depth), 1 024 and 16 384 columns (four k
chunks), 512 columns in k chunks of 1, 3 and 5 tiles, on one partial tile, ragged edges, whole tiles and more than 16
tiles along a side (the persistent instance).  f16x3 plain blocks also against the oracle, within 2e-6 + 1e-5 |r|.

    python tools/gemm_loop_check.py [--precision f16x3|bf16x3] [--first | --repeats | --fullsize]

--first:   the 3 x 5, 64-column case alone (the first run of a changed loop: a wrong barrier count shows as a hang).
--repeats: ten launches of the 4 100-row self case per width, each compared with the first (a late LDS-DMA piece shows as a
           changing tile).
--fullsize: 50 000 x 4 096 self in both arms, 64 seeded rows x all columns (outside the suite; profiles/gemm_phased_loop.log)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
from oracle import seekr_oracle as orc  # noqa: E402  (checker only)
from seekr_amd import _lib as L  # noqa: E402
from seekr_amd import consumers  # noqa: E402

WIDTHS = (32, 64, 96, 160, 256, 1024, 16384)
CHUNKED = ((512, 1), (512, 3), (512, 5))          # columns, SEEKR_GEMM_CHUNK_TILES
SHAPES = ((3, 5), (1500, 1111), (1024, 768), (4100, 300))
SPLIT_KIND = {L.PREC_F16X3: 2, L.PREC_BF16X3: 1}
MIN_COLS = {L.PREC_F16X3: 64, L.PREC_BF16X3: 1024}  # narrower rows take the fp32 kernel in this precision (operand.hip: split_min); kt = 1 launches: the chunked sets


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", default="all", choices=["all", "f16x3", "bf16x3"])
    ap.add_argument("--first", action="store_true")
    ap.add_argument("--repeats", action="store_true")
    ap.add_argument("--fullsize", action="store_true")
    args = ap.parse_args()
    precisions = [L.PREC_F16X3, L.PREC_BF16X3] if args.precision == "all" else [L.PRECISIONS[args.precision]]
    ctx = L.default_context()
    rng = np.random.default_rng(7)
    small = args.first or args.fullsize
    max_rows = 5 if small else max(s[0] for s in SHAPES)
    max_rows_b = 5 if small else max(s[1] for s in SHAPES)
    max_cols = 64 if small else max(WIDTHS)
    pool_a = (rng.binomial(40, 0.06, size=(max_rows, max_cols)) * np.float32(0.5)).astype(np.float32)
    pool_b = (rng.binomial(40, 0.06, size=(max_rows_b, max_cols)) * np.float32(0.5)).astype(np.float32)

    def arms(fn, chunk_tiles=0):
        """[present loop, phased loop]"""
        out = []
        for val in ("0", "1"):
            os.environ["SEEKR_GEMM_LOOP"] = val
            if chunk_tiles:
                os.environ["SEEKR_GEMM_CHUNK_TILES"] = str(chunk_tiles)
            ctx.reload_knobs()
            out.append(fn())
        os.environ.pop("SEEKR_GEMM_LOOP")
        os.environ.pop("SEEKR_GEMM_CHUNK_TILES", None)
        ctx.reload_knobs()
        return out

    def same_bits(a, b):
        return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))

    if args.fullsize:
        # the flagship shape once, outside the suite: 50 000 x 4 096 self in both arms, 64 seeded rows x all columns
        rows, cols = 50000, 4096
        op = L.Operand(ctx, rows, cols, L.PREC_F16X3)
        for r0 in range(0, rows, 8192):
            nr = min(8192, rows - r0)
            c = rng.binomial(1995, 1.0 / 4096, size=(nr, cols)).astype(np.float32) * np.float32(0.5)
            z = (c - c.mean(0)) / np.maximum(c.std(0), 1e-6)
            d = ctx.from_numpy(np.log2(z + np.abs(z.min()) + 1.0).astype(np.float32))
            L.operand_fill(ctx, d, op=op.view(r0, nr), precision=L.PREC_F16X3)
            d.free()
        picks = np.sort(np.random.default_rng(64).choice(rows, size=64, replace=False))
        r = ctx.empty(rows, rows)

        def seeded_rows():
            L.pearson_gemm_op(ctx, op, op, r, symmetric=True)
            return np.concatenate([r.to_numpy(int(i), 1) for i in picks])

        old, new = arms(seeded_rows)
        assert same_bits(old, new), "50 000 x 4 096 self: the arms differ in %d of %d cells" % ((old.view(np.uint32) != new.view(np.uint32)).sum(), old.size)
        print("rows %s ..." % " ".join(str(i) for i in picks[:8]))
        print("gemm loop check ok: 50 000 x 4 096 self, %d seeded rows x %d columns bit-identical in both arms" % (len(picks), rows))
        return
    if args.first:
        widths, shapes = [(64, 0)], [(3, 5)]
    elif args.repeats:
        widths, shapes = [(c, 0) for c in WIDTHS], [(4100, 300)]
    else:
        widths, shapes = [(c, 0) for c in WIDTHS] + list(CHUNKED), SHAPES
    n_checked = 0
    for prec in precisions:
        for cols, chunk_tiles in widths:
            if cols < MIN_COLS[prec]:
                continue
            for rows, rows_b in shapes:
                xa = np.ascontiguousarray(pool_a[:rows, :cols])
                xb = np.ascontiguousarray(pool_b[:rows_b, :cols])
                za, _ = L.operand_fill(ctx, ctx.from_numpy(xa), precision=prec)
                zb, _ = L.operand_fill(ctx, ctx.from_numpy(xb), precision=prec)
                assert za.kind == SPLIT_KIND[prec] and zb.kind == SPLIT_KIND[prec], ("not on the split kernel", prec, cols, za.kind, zb.kind)

                def self_block():
                    r = ctx.zeros(rows, rows)
                    L.pearson_gemm_op(ctx, za, za, r, symmetric=True)
                    return r.to_numpy()

                def plain_block():
                    r = ctx.zeros(rows, rows_b)
                    L.pearson_gemm_op(ctx, za, zb, r)
                    return r.to_numpy()

                def plain_into_wide(col0=3):  # rows of the target start off a 16-byte boundary
                    r = ctx.zeros(rows, rows_b + 8)
                    L.pearson_gemm_op(ctx, za, zb, r, row0=0, col0=col0)
                    return r.to_numpy()

                def cross_block():
                    r, rt = ctx.zeros(rows, rows_b), ctx.zeros(rows_b, rows)
                    L.pearson_gemm_op_mirror(ctx, za, zb, r, 0, 0, rt, 0, 0)
                    return np.concatenate([r.to_numpy().ravel(), rt.to_numpy().ravel()])

                def stripes():  # LOWER left of the diagonal block, SELF on it, PLAIN right of it
                    r = ctx.zeros(rows, rows)
                    for r0 in range(0, rows, 512):
                        nr = min(512, rows - r0)
                        L.pearson_gemm_op_rows(ctx, za.view(r0, nr), za, r0, r, r0)
                    return r.to_numpy()

                def edge_list():
                    fe = consumers.FusedEdges(ctx)
                    got = fe.block(za, zb, 0.02, row_global0=7, col_global0=11)
                    fe.free()
                    return np.concatenate([g.view(np.uint32) for g in got])

                if args.repeats:
                    os.environ["SEEKR_GEMM_LOOP"] = "1"
                    ctx.reload_knobs()
                    first = self_block()
                    for rep in range(1, 10):
                        assert same_bits(first, self_block()), ("launch differs from the first", rep, prec, cols)
                        n_checked += 1
                    os.environ.pop("SEEKR_GEMM_LOOP")
                    ctx.reload_knobs()
                    continue
                cases = [("self", self_block), ("plain", plain_block), ("plain_unaligned", plain_into_wide), ("cross", cross_block),
                         ("stripes", stripes), ("edges", edge_list)]
                for name, fn in cases:
                    old, new = arms(fn, chunk_tiles)
                    assert same_bits(old, new), (name, prec, rows, rows_b, cols, chunk_tiles)
                    n_checked += 1
                    if name == "plain" and prec == L.PREC_F16X3:
                        want = orc.pearson(xa, xb)
                        err = np.abs(new - want) - 1e-5 * np.abs(want)
                        print("oracle %d x %d x %d chunk %d: max |r - oracle| - 1e-5 |oracle| = %.3g" % (rows, rows_b, cols, chunk_tiles, np.nanmax(err)), flush=True)
                        assert np.allclose(new, want, rtol=1e-5, atol=2e-6), (rows, rows_b, cols, float(np.nanmax(err)))
    print("gemm loop check ok: %d comparisons bit-identical" % n_checked)


if __name__ == "__main__":
    main()
