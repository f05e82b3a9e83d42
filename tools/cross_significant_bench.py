"""The two-set significance functions and the cell-selection kernel behind them.  One process, one GPU.

    python tools/cross_significant_bench.py [--out profiles/cross_significant_bench.json] [--windows 1000000] [--targets 200000]

1. skr_select_cells_ge against skr_edges (unchanged by this work: the stand-in for the parent commit) on the same block
   and cutoff, about 1e-3 of the cells kept, both filling preallocated outputs: median, fastest and slowest of the
   repeats for an 8 192 x 50 000 block and a 100 x 65 536 block.
2. pearson_significant(z1, other=z2) for 1 000 x --targets rows at k = 6 (synthetic 2 000 nt transcripts, prepared as
   tools/significant_bench.py prepares them), a norm background, fdr_bh at 0.05: seconds per step, peak device memory,
   bytes to the host; for 1 000 x 20 000 rows also the full-matrix path (r, p, adjust_pvalues(symmetric=False), the
   cells <= alpha).
3. domain_significant for 100 queries x --windows windows beside domain_topk and domain_pearson on the same input.
4. candidates="device" against "host" on 50 000 rows of tools/significant_bench.py's input."""
import argparse
import ctypes as C
import json
import os
import socket
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
from seekr_amd import _lib, consumers, windows  # noqa: E402
from seekr_amd import significant as sg  # noqa: E402
from seekr_amd.synthetic import synthetic_ascii  # noqa: E402
from significant_bench import ALPHA, METHOD, PeakMemory, norm_background, operand  # noqa: E402

REPEATS = 9


def spread(times):
    t = sorted(times)
    return {"median_ms": round(1e3 * t[len(t) // 2], 4), "min_ms": round(1e3 * t[0], 4), "max_ms": round(1e3 * t[-1], 4)}


def kernel_against_edges(ctx, rows, cols, keep=1e-3):
    rng = np.random.default_rng(rows)
    r = ctx.empty(rows, cols)
    for r0 in range(0, rows, 1024):  # uniform [0, 1): no zeros; the global diagonal is moved out of the block
        n = min(1024, rows - r0)
        r.upload(rng.random((n, cols), dtype=np.float32), row0=r0)
    cutoff, far = C.c_float(1.0 - keep), 1 << 20
    cap = int(rows * cols * keep * 1.5) + 1024
    outs = [ctx.empty(cap, 1, t) for t in (np.uint32, np.uint32, np.float32)]
    lib, count = _lib.lib(), C.c_int64(0)

    def cells():
        _lib.check(lib.skr_select_cells_ge(ctx._h, r._h, rows, 0, cols, 0, far, cutoff, *[m._h for m in outs], 0, C.byref(count), None))

    def edges():
        _lib.check(lib.skr_edges(ctx._h, r._h, rows, 0, cols, 0, far, cutoff, 0, *[m._h for m in outs], C.byref(count)))

    row = {"rows": rows, "cols": cols}
    got = {}
    for name, call in (("skr_edges", edges), ("skr_select_cells_ge", cells), ("skr_edges_again", edges)):
        call()
        ctx.sync()
        got[name] = (count.value, [np.array(m.to_numpy(0, count.value)) for m in outs])
        times = []
        for _ in range(REPEATS):
            t0 = time.perf_counter()
            call()
            ctx.sync()
            times.append(time.perf_counter() - t0)
        row[name] = spread(times)
    assert got["skr_edges"][0] == got["skr_select_cells_ge"][0]
    assert all(np.array_equal(a, b) for a, b in zip(got["skr_edges"][1], got["skr_select_cells_ge"][1]))
    row["cells_kept"] = got["skr_edges"][0]
    row["same_list"] = True
    row["select_cells_over_edges"] = round(row["skr_select_cells_ge"]["median_ms"] / min(row["skr_edges"]["median_ms"],
                                                                                       row["skr_edges_again"]["median_ms"]), 3)
    for m in outs + [r]:
        m.free()
    return row


def two_sets(ctx, z1, z2, fitres):
    timings = {}
    ctx.sync()
    with PeakMemory(ctx) as mem:
        t0 = time.perf_counter()
        res = sg.pearson_significant(z1, fitres, method=METHOD, alpha=ALPHA, other=z2, timings=timings)
        ctx.sync()
        wall = time.perf_counter() - t0
    row = {"queries": z1.rows, "targets": z2.rows, "n_tests": res.n_tests, "r_cutoff": float(res.r_cutoff),
           "n_candidates": res.n_candidates, "significant_cells": len(res), "wall_s": round(wall, 4),
           "peak_device_bytes": mem.peak_bytes, "bytes_to_device": int(timings["bytes_to_device"]),
           "bytes_to_host": int(timings.get("bytes_to_host", 0))}
    for step in ("cutoff_search", "edge_list", "p_values", "selection", "correction"):
        row[step + "_s"] = round(timings.get(step, 0.0), 4)
    return row, res


def two_sets_full(ctx, z1, z2, fitres):
    name, _, params = fitres[0]
    ctx.sync()
    with PeakMemory(ctx) as mem:
        t0 = time.perf_counter()
        r = ctx.empty(z1.rows, z2.rows)
        _lib.pearson_gemm_op(ctx, z1, z2, r)
        p = consumers.parametric_pvalues(r, name, params)
        adj = consumers.adjust_pvalues(p, METHOD, ALPHA, symmetric=False)
        index, count = consumers.select_le(adj, ALPHA)
        flat = np.array(index.to_numpy()).reshape(-1).astype(np.int64) if count else np.empty(0, np.int64)
        ctx.sync()
        wall = time.perf_counter() - t0
    for m in (r, p, adj) + ((index,) if count else ()):
        m.free()
    return {"queries": z1.rows, "targets": z2.rows, "wall_s": round(wall, 4), "peak_device_bytes": mem.peak_bytes,
            "significant_cells": int(count)}, flat


def domain(ctx, n_windows, tmp):
    k, window, slide, n_query = 6, 1000, 100, 100
    length = (n_windows - 1) * slide + window
    paths = {name: os.path.join(tmp, name + ".fa") for name in ("query", "target", "unrelated")}
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    for name, seed, n, size in (("query", 3, n_query, window), ("target", 4, 1, length), ("unrelated", 5, 1, 200 * slide + window)):
        rng = np.random.default_rng(seed)  # (synthetic_ascii draws 10 000 rows at a time: not for one row of 1e8 bases)
        with open(paths[name], "wb") as f:
            for i in range(n):
                f.write(b">%s%d\n" % (name.encode(), i) + letters[rng.integers(0, 4, size=size, dtype=np.uint8)].tobytes() + b"\n")
    from seekr_amd.kmer_counts import BasicCounter
    blob, offsets = synthetic_ascii(6, 2000, 1000)
    vectors = os.path.join(tmp, "vectors.fa")
    with open(vectors, "wb") as f:
        for i in range(2000):
            f.write(b">v%d\n" % i + bytes(blob[offsets[i]:offsets[i + 1]]) + b"\n")
    counter = BasicCounter(vectors, k=k, silent=True)
    counter.get_counts()
    args = (paths["query"], paths["target"], k, window, slide, counter.mean, counter.std)
    bg, _ = windows.domain_pearson(paths["query"], paths["unrelated"], k, window, slide, counter.mean, counter.std)
    fitres = [("norm", 0.0, (float(bg.mean(dtype=np.float64)), float(bg.std(dtype=np.float64))))]
    row = {"queries": n_query, "windows": n_windows, "k": k, "window": window, "slide": slide}
    for name, call in (("domain_significant", lambda: windows.domain_significant(*args, fitres, method=METHOD, alpha=ALPHA)),
                       ("domain_topk", lambda: windows.domain_topk(*args, top=10)),
                       ("domain_pearson", lambda: windows.domain_pearson(*args))):
        ctx.sync()
        with PeakMemory(ctx) as mem:
            t0 = time.perf_counter()
            out = call()
            ctx.sync()
            wall = time.perf_counter() - t0
        row[name] = {"wall_s": round(wall, 3), "peak_device_bytes": mem.peak_bytes}
        if name == "domain_significant":
            row[name].update(significant_cells=len(out), n_candidates=out.attrs["n_candidates"], r_cutoff=float(out.attrs["r_cutoff"]),
                             bytes_to_host=len(out) * 24)
        elif name == "domain_topk":
            row[name]["bytes_to_host"] = n_query * 10 * 8
        else:
            row[name]["bytes_to_host"] = int(out[0].nbytes)
        del out
    return row


def candidates_on_device(ctx, rows):
    z = operand(ctx, rows, 2000)
    fitres = norm_background(ctx, z)
    row, results = {"rows": rows}, {}
    for where in ("host", "device", "host", "device"):  # twice each: the first of either pays for the buffers
        timings = {}
        ctx.sync()
        t0 = time.perf_counter()
        res = sg.pearson_significant(z, fitres, method=METHOD, alpha=ALPHA, timings=timings, candidates=where)
        ctx.sync()
        row[where] = {"wall_s": round(time.perf_counter() - t0, 4), "edge_list_s": round(timings["edge_list"], 4),
                      "bytes_to_device": int(timings["bytes_to_device"]), "n_candidates": res.n_candidates,
                      "significant_pairs": len(res)}
        results[where] = res
    row["same_bytes"] = all(getattr(results["host"], f).tobytes() == getattr(results["device"], f).tobytes()
                            for f in ("rows", "cols", "r", "p", "p_adj"))
    z.free()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--targets", type=int, default=200000)
    ap.add_argument("--windows", type=int, default=1000000)
    ap.add_argument("--self-rows", type=int, default=50000)
    args = ap.parse_args()
    ctx = _lib.default_context()
    res = {"box": socket.gethostname(), "method": METHOD, "alpha": ALPHA, "repeats": REPEATS}

    def save():
        if args.out:
            with open(args.out, "w") as f:
                json.dump(res, f, indent=1)
                f.write("\n")

    res["kernel"] = [kernel_against_edges(ctx, 8192, 50000), kernel_against_edges(ctx, 100, 65536)]
    print(json.dumps(res["kernel"]), flush=True)
    save()

    z = operand(ctx, 1000 + args.targets, 2000)
    fitres = norm_background(ctx, z)
    z1 = z.view(0, 1000)
    res["background"] = {"dist": "norm", "mean": fitres[0][2][0], "sd": fitres[0][2][1]}
    small, got = two_sets(ctx, z1, z.view(1000, 20000), fitres)
    full, flat = two_sets_full(ctx, z1, z.view(1000, 20000), fitres)
    small["equals_full_path"] = bool(np.array_equal(got.rows.astype(np.int64) * 20000 + got.cols, flat))
    res["two_sets_20000"] = {"significant_pairs": small, "full_matrix_path": full}
    res["two_sets"], _ = two_sets(ctx, z1, z.view(1000, args.targets), fitres)
    z.free()
    print(json.dumps({k: res[k] for k in ("two_sets_20000", "two_sets")}), flush=True)
    save()

    with tempfile.TemporaryDirectory() as tmp:
        res["domain"] = domain(ctx, args.windows, tmp)
    print(json.dumps(res["domain"]), flush=True)
    save()

    res["candidates"] = candidates_on_device(ctx, args.self_rows)
    print(json.dumps(res["candidates"]), flush=True)
    save()


if __name__ == "__main__":
    main()
