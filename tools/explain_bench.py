"""skr_pair_kmers and skr_group_colstat at the sizes a user runs.  One process, one GPU.

    python tools/explain_bench.py [--rows 50000] [--pairs 1000000] [--group-rows 100000] [--runs 9] [--out profiles/explain_bench.json]

Every time is DEVICE time from the library's own event pairs around its kernels (Context.prof_query), after one warm-up
round, median of --runs with the fastest and the slowest, the arms of a comparison alternating inside one process.

pair_kmers — operands 50 000 x 4 096 (standard normal rows), E = 10^6 pairs in np.nonzero order (sorted by row, as
significant_pairs lists them) and the same pairs in random order, top 10 and 256, without the factor outputs:
  fused      skr_pair_kmers.  `gathered_gbs` = (E * 2 * W * 4 bytes of operand rows + the outputs) / time: bytes GATHERED, not
             bytes from HBM — in the sorted list consecutive pairs share their first row, which then comes from cache.
  two_step   a lower bound of the path the library offered before: the product matrix written chunk by chunk and read back
             by skr_topk_merge_rows.  The library has no kernel that writes the products of gathered rows, so the write is
             stood in for by skr_apply copying a chunk (reads E * W * 4 and writes E * W * 4 bytes; a product kernel would
             read twice that), followed by the real skr_topk_merge_rows over the chunk.  It selects nothing meaningful;
             it moves the bytes the two-step path cannot avoid.
group_kmers — a 100 000 x 4 096 matrix, 33 groups (tools/leiden_bench.py's shape) and 10^4 groups of random membership:
  skr_group_colstat with and without sd against skr_colsum_seq over the same matrix in the same run (one pass of the same
  chain over all rows: the yardstick; `mean_only_over_colsum` is the ratio)."""
import argparse
import json
import os
import socket
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
from seekr_amd import _lib  # noqa: E402

COPY_RATE_TBS = 6.29  # the measured device-to-device copy rate DESIGN.md's byte budgets use (read + write bytes per second)


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def device_ms(ctx, names, fn):
    """Device milliseconds recorded under `names` while fn runs."""
    ctx.prof_reset()
    ctx.prof_enable(True)
    fn()
    ctx.sync()
    ctx.prof_enable(False)
    return sum(ctx.prof_query(n)[0] for n in names)


def alternate(ctx, arms, runs):
    """arms: name -> (prof names, fn); one warm-up round, then `runs` rounds with the arms in turn."""
    ms = {name: [] for name in arms}
    for rep in range(runs + 1):
        for name, (names, fn) in arms.items():
            t = device_ms(ctx, names, fn)
            if rep:
                ms[name].append(t)
    return {name: summary(v) for name, v in ms.items()}


def bench_pairs(ctx, n, w, n_pairs, runs):
    rng = np.random.default_rng(1)
    z = ctx.empty(n, w)
    for r0 in range(0, n, 8192):  # uploaded in pieces: no second copy of the matrix on the host
        z.upload(rng.standard_normal((min(8192, n - r0), w), dtype=np.float32), r0)
    rows = np.sort(rng.integers(0, n, n_pairs)).astype(np.uint32)
    cols = rng.integers(0, n, n_pairs).astype(np.uint32)
    order = np.lexsort((cols, rows))
    lists = {"sorted": (rows[order], cols[order])}
    perm = rng.permutation(n_pairs)
    lists["random"] = (lists["sorted"][0][perm], lists["sorted"][1][perm])
    chunk = min(n, n_pairs)
    buf = ctx.empty(chunk, w)
    out = []
    for top in (10, 256):
        idx, val = ctx.empty(n_pairs, top, np.uint32), ctx.empty(n_pairs, top)
        cidx, cval = ctx.empty(chunk, top, np.uint32), ctx.empty(chunk, top)
        for order_name, (r, c) in lists.items():
            d_r, d_c = ctx.from_numpy(r), ctx.from_numpy(c)

            def fused():
                _lib.pair_kmers(ctx, z, z, d_r, d_c, n_pairs, top, True, idx, val)

            def two_step():
                for e0 in range(0, n_pairs, chunk):
                    m = min(chunk, n_pairs - e0)
                    _lib.apply(ctx, z, y=buf)
                    _lib.topk_merge_rows(ctx, buf, cidx, cval, top, first=True, nrows=m, exclude_diag=False)

            arms = {"fused": (["pair_kmers"], fused)}
            if order_name == "sorted":  # the stand-in does not depend on the order of the list
                arms["two_step"] = (["elementwise_apply", "topk_merge_rows"], two_step)
            res = alternate(ctx, arms, runs)
            gathered = n_pairs * 2 * w * 4 + n_pairs * top * 8
            row = {"order": order_name, "top": top, "pairs": n_pairs, "fused": res["fused"],
                   "gathered_bytes": gathered,
                   "gathered_gbs": round(gathered / res["fused"]["median_ms"] / 1e6, 1),
                   "gathered_over_copy_rate": round(gathered / res["fused"]["median_ms"] / 1e9 / COPY_RATE_TBS, 3)}
            if "two_step" in res:
                row["two_step_lower_bound"] = res["two_step"]
                row["fused_over_two_step"] = round(res["fused"]["median_ms"] / res["two_step"]["median_ms"], 3)
            out.append(row)
            print(json.dumps(row), flush=True)
            d_r.free()
            d_c.free()
        for m in (idx, val, cidx, cval):
            m.free()
    buf.free()
    z.free()
    return out


def bench_groups(ctx, n, w, runs):
    rng = np.random.default_rng(2)
    x = ctx.empty(n, w)
    for r0 in range(0, n, 8192):
        x.upload((1e4 + 50.0 * rng.standard_normal((min(8192, n - r0), w))).astype(np.float32), r0)
    acc = ctx.zeros(1, w)
    out = []
    for g in (33, 10000):
        labels = rng.integers(0, g, n)
        uniq, inverse = np.unique(labels, return_inverse=True)
        order = ctx.from_numpy(np.argsort(inverse, kind="stable").astype(np.uint32))
        starts = np.concatenate([[0], np.cumsum(np.bincount(inverse, minlength=len(uniq)))]).astype(np.int64)
        mean, sd = ctx.empty(len(uniq), w), ctx.empty(len(uniq), w)
        arms = {"colsum_seq": (["colsum_seq"], lambda: _lib.colsum_seq(ctx, x, acc)),
                "mean_only": (["group_colstat"], lambda: _lib.group_colstat(ctx, x, order, starts, mean)),
                "mean_and_sd": (["group_colstat"], lambda: _lib.group_colstat(ctx, x, order, starts, mean, sd))}
        res = alternate(ctx, arms, runs)
        row = {"groups": int(len(uniq)), "rows": n, "cols": w, **res,
               "mean_only_over_colsum": round(res["mean_only"]["median_ms"] / res["colsum_seq"]["median_ms"], 3),
               "mean_and_sd_over_colsum": round(res["mean_and_sd"]["median_ms"] / res["colsum_seq"]["median_ms"], 3),
               "matrix_gbs_mean_only": round(n * w * 4 / res["mean_only"]["median_ms"] / 1e6, 1),
               "matrix_gbs_colsum": round(n * w * 4 / res["colsum_seq"]["median_ms"] / 1e6, 1)}
        out.append(row)
        print(json.dumps(row), flush=True)
        for m in (order, mean, sd):
            m.free()
    acc.free()
    x.free()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=50000)
    ap.add_argument("--cols", type=int, default=4096)
    ap.add_argument("--pairs", type=int, default=1000000)
    ap.add_argument("--group-rows", type=int, default=100000)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ctx = _lib.default_context()
    res = {"box": socket.gethostname(), "runs": args.runs, "timing": "device events of the library (prof_query), median / min / max",
           "copy_rate_tbs_quoted": COPY_RATE_TBS, "operand_rows": args.rows, "cols": args.cols}
    res["pair_kmers"] = bench_pairs(ctx, args.rows, args.cols, args.pairs, args.runs)
    res["group_kmers"] = bench_groups(ctx, args.group_rows, args.cols, args.runs)
    at = [r for r in res["pair_kmers"] if r["order"] == "sorted" and r["top"] == 10][0]
    res["verdict"] = {"fused_not_slower_than_two_step_lower_bound_at_top10": bool(at["fused_over_two_step"] <= 1.0),
                      "fused_over_two_step_at_top10": at["fused_over_two_step"]}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
