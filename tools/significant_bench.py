"""significant_pairs against the full-matrix path, and alone at sizes the full path cannot reach.  One process, one GPU.

    python tools/significant_bench.py [--rows 20000] [--alone 50000] [--length 2000] [--out profiles/significant_bench.json]

Input: synthetic sequences of --length bases, k = 6 (4 096 columns), normalised as the benchmark does; the background is
a `norm` with numpy's mean and standard deviation of a subsample of r (100 000 cells of a 2 000-row block); fdr_bh at
alpha 0.05.

At --rows: pearson_significant on the prepared operand, split into cutoff search, edge list, p-values, selection and
correction (wall seconds, the device synchronised after each), the bytes that crossed PCIe, the peak of device memory in
use (total minus the least free memory a second thread sees, sampled every 2 ms: the operand and whatever workspace a
warm-up left included; every stage runs on a context of its own, closed afterwards) — and the full-matrix path on the
same rows in the same run: pearson_gemm_op -> parametric_pvalues -> adjust_pvalues(symmetric=True) -> the cells
<= alpha, whose pairs must equal the feature's.  At each of --alone: the feature alone, with n_candidates, the number of
significant pairs, the bytes to the host and the path fuse="auto" chose."""
import argparse
import json
import os
import socket
import sys
import threading
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
from seekr_amd import _lib, consumers  # noqa: E402
from seekr_amd import pearson as pearson_mod  # noqa: E402
from seekr_amd import significant as sg  # noqa: E402
from seekr_amd.synthetic import synthetic_ascii  # noqa: E402

ALPHA, METHOD = 0.05, "fdr_bh"


class PeakMemory:
    """The most device memory in use while the block runs, sampled from a second thread (hipMemGetInfo only)."""

    def __init__(self, ctx, every=0.002):
        self.ctx, self.every, self.low = ctx, every, None

    def __enter__(self):
        self.low, self.total = self.ctx.mem_info()
        self.stop = threading.Event()
        self.thread = threading.Thread(target=self._run, daemon=True)
        self.thread.start()
        return self

    def _run(self):
        while not self.stop.wait(self.every):
            self.low = min(self.low, self.ctx.mem_info()[0])

    def __exit__(self, *exc):
        self.stop.set()
        self.thread.join()
        self.peak_bytes = int(self.total - min(self.low, self.ctx.mem_info()[0]))


def operand(ctx, n, length):
    blob, offsets = synthetic_ascii(1, n, length)
    x = _lib.count_per_kb(ctx, _lib.PackedSeqs.from_buffer(ctx, blob, offsets), 6)
    _lib.normalize(ctx, x, "Log2.post", 1, None, 1, None)
    z, _ = _lib.operand_fill(ctx, x, None, pearson_mod._precision_for(np.dtype(np.float32), True))
    x.free()
    return z


def norm_background(ctx, z, seed=7):
    """('norm', 0, (mean, sd)) of 100 000 cells above the diagonal of the first 2 000 rows' r."""
    m = min(2000, z.rows)
    head = z.view(0, m)
    r = ctx.empty(m, m)
    _lib.pearson_gemm_op(ctx, head, head, r)
    tri = consumers.triu_values(r)
    sample = consumers.subsample(tri, min(100000, tri.cols), np.random.RandomState(seed))
    r.free()
    tri.free()
    return [("norm", 0.0, (float(np.mean(sample)), float(np.std(sample))))]


def feature(ctx, z, fitres):
    timings = {}
    ctx.sync()
    with PeakMemory(ctx) as mem:
        t0 = time.perf_counter()
        res = sg.pearson_significant(z, fitres, method=METHOD, alpha=ALPHA, timings=timings)
        ctx.sync()
        wall = time.perf_counter() - t0
    cells = res.n_tests
    row = {"rows": z.rows, "n_tests": cells, "r_cutoff": float(res.r_cutoff) if res.r_cutoff is not None else None,
           "n_candidates": res.n_candidates, "candidates_per_cell": round(res.n_candidates / max(cells, 1), 5),
           "fuse_auto_chose": "fused epilogue" if res.n_candidates <= consumers.FUSE_MAX_DENSITY * cells else
                              "two-step (stripe buffer) after the first dense stripe",
           "significant_pairs": len(res), "wall_s": round(wall, 4), "peak_device_bytes": mem.peak_bytes,
           "bytes_to_device": int(timings.get("bytes_to_device", 0)),
           "bytes_to_host": int(res.n_candidates * 12 + timings.get("bytes_to_host", 0)),
           "bytes_to_host_final_lists": int(timings.get("bytes_to_host", 0))}
    for step in ("cutoff_search", "edge_list", "p_values", "selection", "correction"):
        row[step + "_s"] = round(timings.get(step, 0.0), 4)
    return row, res


def full_path(ctx, z, fitres):
    name, _, params = fitres[0]
    n = z.rows
    ctx.sync()
    steps = {}
    with PeakMemory(ctx) as mem:
        t0 = time.perf_counter()
        r = ctx.empty(n, n)
        _lib.pearson_gemm_op(ctx, z, z, r)
        ctx.sync()
        steps["pearson_s"] = time.perf_counter() - t0
        t1 = time.perf_counter()
        p = consumers.parametric_pvalues(r, name, params)
        ctx.sync()
        steps["p_values_s"] = time.perf_counter() - t1
        t1 = time.perf_counter()
        adj = consumers.adjust_pvalues(p, METHOD, ALPHA, symmetric=True)
        ctx.sync()
        steps["correction_s"] = time.perf_counter() - t1
        t1 = time.perf_counter()
        index, count = consumers.select_le(adj, ALPHA)  # the cells <= alpha, row-major; NaN (outside the triangle) never passes
        flat = np.array(index.to_numpy()).reshape(-1).astype(np.int64) if count else np.empty(0, np.int64)
        ctx.sync()
        steps["selection_s"] = time.perf_counter() - t1
        wall = time.perf_counter() - t0
    for m in (r, p, adj) + ((index,) if count else ()):
        m.free()
    row = {"rows": n, "wall_s": round(wall, 4), "peak_device_bytes": mem.peak_bytes, "significant_pairs": int(count)}
    row.update({k: round(v, 4) for k, v in steps.items()})
    return row, flat


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=20000)
    ap.add_argument("--alone", default="50000", help="comma-separated row counts for the feature alone ('' for none)")
    ap.add_argument("--length", type=int, default=2000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    res = {"box": socket.gethostname(), "method": METHOD, "alpha": ALPHA, "cols": 4096, "stripe_rows": 8192}

    def stage(n, run, warm):
        """run(ctx, z, fitres) on a context of its own (its workspaces go with it), after `warm` unmeasured calls."""
        ctx = _lib.Context(_lib.default_device())
        z = operand(ctx, n, args.length)
        if "background" not in res:
            fit = norm_background(ctx, z)
            res["background"] = {"name": "norm", "mean": fit[0][2][0], "sd": fit[0][2][1]}
        fit = [("norm", 0.0, (res["background"]["mean"], res["background"]["sd"]))]
        for _ in range(warm):
            run(ctx, z, fit)
        out = run(ctx, z, fit)
        z.free()
        ctx.close()
        return out

    res["feature"], got = stage(args.rows, feature, 1)
    print(json.dumps(res["feature"]), flush=True)
    res["full_path"], flat = stage(args.rows, full_path, 1)
    print(json.dumps(res["full_path"]), flush=True)
    res["same_pairs"] = bool(np.array_equal(flat, got.rows.astype(np.int64) * args.rows + got.cols))
    res["feature_over_full_path"] = round(res["feature"]["wall_s"] / res["full_path"]["wall_s"], 3)
    res["alone"] = []
    for n in [int(t) for t in args.alone.split(",") if t.strip()]:
        row, _ = stage(n, feature, 0)
        res["alone"].append(row)
        print(json.dumps(row), flush=True)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
