"""Nearest neighbours without r, at the benchmark's size: 50 000 synthetic sequences of 2 000 bases, k = 6 (50 000 x 4 096
prepared rows), stripes of 8 192 rows.  One process, one GPU.

    python tools/neighbors_bench.py [--rows 50000] [--runs 5] [--out profiles/neighbors_bench.json] [--skip-domain]

For panel_rows in 8 192, 32 768 and None (all of b) and k in 1, 10, 64, KMAX — wall time of the whole loop over stripes
and panels, ending in a device synchronise, median of --runs after one warm-up, the three arms alternating:
  a   the contraction of every [stripe, panel] block into the reusable buffer, no selection
  b   a, each stripe followed by skr_topk_rows (k passes over the stripe; it cannot merge, so whole-width panels only)
  c   a, each block followed by skr_topk_merge_rows (what consumers.pearson_topk does to each block, without the download)
and the device time of the two selection kernels themselves (the library's event timers), which does not depend on a
difference of two wall times.  `read_once_ms`: the time one read of all of r's cells takes at the copy bandwidth measured
here (a device-to-device copy of 1 GiB moves 2 GiB; skr_peer_copy_rows within one GPU).  The acceptance condition of the kernel (DESIGN_KERNELS.md) is
evaluated and written out as `verdict`, whichever way it falls.  Last: one domain_topk line against domain_pearson,
100 queries against the windows of 50 x 2 Mbases (the input of profiles/window_counts_bench.json): seconds and the bytes
returned to the host."""
import argparse
import json
import os
import socket
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
from seekr_amd import _lib  # noqa: E402
from seekr_amd import pearson as pearson_mod  # noqa: E402
from seekr_amd.synthetic import synthetic_ascii  # noqa: E402

STRIPE = 8192


def copy_bandwidth_gbs(ctx):
    """Bytes moved per second by a device-to-device copy of 1 GiB (read + write), median of 7 after a warm-up."""
    rows, cols = 65536, 4096
    src, dst = ctx.zeros(rows, cols), ctx.zeros(rows, cols)
    ctx.sync()
    ts = []
    for _ in range(8):
        t0 = time.perf_counter()
        _lib.peer_copy_rows(dst, 0, src, 0, rows)  # on the communication stream
        done = _lib.Event(ctx, comm=True)
        done.wait_on(ctx)
        ctx.sync()
        ts.append(time.perf_counter() - t0)
        done.free()
    src.free()
    dst.free()
    return 2.0 * rows * cols * 4 / statistics.median(ts[1:]) / 1e9


def loop(ctx, z, buf, panel, select):
    n = z.rows
    for s0 in range(0, n, STRIPE):
        rows = min(STRIPE, n - s0)
        a = z.view(s0, rows)
        for p0 in range(0, n, panel):
            cols = min(panel, n - p0)
            _lib.pearson_gemm_op(ctx, a, z if cols == n else z.view(p0, cols), buf)
            select(rows, s0, p0, cols)
    ctx.sync()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=50000)
    ap.add_argument("--length", type=int, default=2000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-domain", action="store_true")
    args = ap.parse_args()
    ctx = _lib.default_context()
    kmax = _lib.topk_merge_limits()[0]
    n, K = args.rows, 4096
    res = {"box": socket.gethostname(), "rows": n, "cols": K, "stripe_rows": STRIPE, "runs": args.runs, "kmax": kmax,
           "candidate_cap": _lib.topk_merge_limits()[1]}
    res["copy_gbs"] = round(copy_bandwidth_gbs(ctx), 1)
    res["read_once_ms"] = round(n * n * 4 / res["copy_gbs"] / 1e6, 3)
    blob, offsets = synthetic_ascii(1, n, args.length)
    x = _lib.count_per_kb(ctx, _lib.PackedSeqs.from_buffer(ctx, blob, offsets), 6)
    _lib.normalize(ctx, x, "Log2.post", 1, None, 1, None)
    z, _ = _lib.operand_fill(ctx, x, None, pearson_mod._precision_for(np.dtype(np.float32), True))
    x.free()

    def timed(fn):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3

    def kernel_ms(name, fn):
        ctx.prof_reset()
        ctx.prof_enable(True)
        fn()
        ctx.prof_enable(False)
        return ctx.prof_query(name)[0]

    table = []
    for panel_arg in (8192, 32768, None):
        panel = n if panel_arg is None else min(panel_arg, n)
        buf = ctx.empty(min(STRIPE, n), panel)
        for k in (1, 10, 64, kmax):
            idx, val = ctx.empty(min(STRIPE, n), k, np.uint32), ctx.empty(min(STRIPE, n), k, np.float32)
            arms = {"a": lambda rows, s0, p0, cols: None,
                    "c": lambda rows, s0, p0, cols: _lib.topk_merge_rows(ctx, buf, idx, val, k, first=p0 == 0, nrows=rows, col_end=cols,
                                                                         row_global0=s0, col_global0=p0)}
            if panel == n:
                arms["b"] = lambda rows, s0, p0, cols: _lib.check(_lib.lib().skr_topk_rows(ctx._h, buf._h, rows, 0, cols, s0, 0, k,
                                                                                           idx._h, val._h))
            ms = {name: [] for name in arms}
            for rep in range(args.runs + 1):  # the arms alternate; the first round warms up
                for name, sel in arms.items():
                    t = timed(lambda: loop(ctx, z, buf, panel, sel))
                    if rep:
                        ms[name].append(t)
            row = {"panel_rows": panel_arg, "k": k}
            for name in arms:
                row[name + "_ms"] = round(statistics.median(ms[name]), 3)
                row[name + "_min_ms"] = round(min(ms[name]), 3)
            row["c_minus_a_ms"] = round(row["c_ms"] - row["a_ms"], 3)
            row["merge_kernel_ms"] = round(kernel_ms("topk_merge_rows", lambda: loop(ctx, z, buf, panel, arms["c"])), 3)
            row["c_minus_a_over_read_once"] = round(row["c_minus_a_ms"] / res["read_once_ms"], 3)
            row["merge_kernel_over_read_once"] = round(row["merge_kernel_ms"] / res["read_once_ms"], 3)
            if "b" in arms:
                row["b_minus_a_ms"] = round(row["b_ms"] - row["a_ms"], 3)
                row["old_kernel_ms"] = round(kernel_ms("topk_rows", lambda: loop(ctx, z, buf, panel, arms["b"])), 3)
                row["c_minus_a_over_b_minus_a"] = round(row["c_minus_a_ms"] / row["b_minus_a_ms"], 4) if row["b_minus_a_ms"] > 0 else None
                row["merge_kernel_over_old_kernel"] = round(row["merge_kernel_ms"] / row["old_kernel_ms"], 4)
            table.append(row)
            print(json.dumps(row), flush=True)
            idx.free()
            val.free()
        buf.free()
    res["table"] = table
    whole = {r["k"]: r for r in table if r["panel_rows"] is None}
    flat = max(r["merge_kernel_ms"] for r in whole.values()) / min(r["merge_kernel_ms"] for r in whole.values())
    res["verdict"] = {
        "at_k10_new_not_above_old": bool(whole[10]["c_minus_a_ms"] <= whole[10]["b_minus_a_ms"]),
        "at_k10_new_kernel_not_above_old_kernel": bool(whole[10]["merge_kernel_ms"] <= whole[10]["old_kernel_ms"]),
        "merge_kernel_ms_largest_over_smallest_k": round(flat, 3),
        "old_kernel_ms_kmax_over_k1": round(whole[kmax]["old_kernel_ms"] / whole[1]["old_kernel_ms"], 1),
        "fastest_panel_rows_at_k10": min((r for r in table if r["k"] == 10), key=lambda r: r["c_ms"])["panel_rows"]}
    z.free()

    if not args.skip_domain:
        from seekr_amd.kmer_counts import BasicCounter
        from seekr_amd.windows import domain_pearson, domain_topk
        bg = BasicCounter(k=6, silent=True)
        bg_blob, bg_off = synthetic_ascii(2, 2000, 2000)
        bg.seqs = [bg_blob[bg_off[i]:bg_off[i + 1]].tobytes().decode() for i in range(2000)]
        bg.get_counts()
        mean, std = bg.mean, bg.std
        del bg
        t_blob, t_off = synthetic_ascii(1, 50, 2_000_000)
        q_blob, q_off = synthetic_ascii(3, 100, 1500)
        with tempfile.TemporaryDirectory() as tmp:
            for path, b, o, prefix in ((os.path.join(tmp, "q.fa"), q_blob, q_off, b"q"), (os.path.join(tmp, "t.fa"), t_blob, t_off, b"t")):
                with open(path, "wb") as f:
                    for i in range(len(o) - 1):
                        f.write(b">%s%d\n" % (prefix, i) + b[o[i]:o[i + 1]].tobytes() + b"\n")
            qfa, tfa = os.path.join(tmp, "q.fa"), os.path.join(tmp, "t.fa")
            walls = {"domain_pearson": [], "domain_topk": []}
            for rep in range(4):  # alternating; the first round warms up
                t0 = time.perf_counter()
                r, _ = domain_pearson(qfa, tfa, 6, 1000, 100, mean, std)
                t1 = time.perf_counter()
                frame = domain_topk(qfa, tfa, 6, 1000, 100, mean, std, top=10)
                t2 = time.perf_counter()
                if rep:
                    walls["domain_pearson"].append(t1 - t0)
                    walls["domain_topk"].append(t2 - t1)
            order = np.argsort(-r, axis=1, kind="stable")[:, :10]
            assert np.array_equal(np.take_along_axis(r, order, axis=1).reshape(-1).view(np.uint32),
                                  frame["r"].to_numpy().view(np.uint32)), "domain_topk differs from domain_pearson's r"
            res["domain"] = {"queries": 100, "windows": int(r.shape[1]), "top": 10,
                             "domain_pearson_s": round(statistics.median(walls["domain_pearson"]), 4),
                             "domain_topk_s": round(statistics.median(walls["domain_topk"]), 4),
                             "domain_pearson_bytes_to_host": int(r.nbytes),
                             "domain_topk_bytes_to_host": int(100 * 10 * 8), "same_top10_bitwise": True}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
