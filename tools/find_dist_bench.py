"""Where find_dist's time goes when the background is sampled without the r matrix.  One process, one GPU.

    python tools/find_dist_bench.py [--runs 9] [--out profiles/find_dist_bench.json] [--skip-large] [--skip-fits]

Medians of --runs after one warm-up, the arms of a comparison alternating.
  a  kernel cost: 50 000 synthetic sequences of 2 000 bases, k = 6 (50 000 x 4 096 prepared rows), 100 000 samples —
     consumers.pearson_sample against the same Sweep with a visitor that does nothing, both ending in a synchronise; the
     device time of skr_gather_cells itself from the library's event timers.
  b  the reference's shape: 12 996 synthetic sequences, k = 4 — find_dist(fit_model=False) by stage (both counters,
     the operand, the draw, the sweep with its gathers) beside the full-matrix path on the same operand and the same
     index (pearson_gemm_op into an N x N matrix, triu_values, the gather of subsample), with the device memory each
     holds; the whole find_dist call as a median of 2 after one warm-up (said so in the output).  The legacy draw — numpy's permutation of all 8.4e7 indices, which is what makes the sample the reference's —
     is timed on its own with the Generator draw next to it.
  c  a large background: 200 000 x 256 prepared rows, 100 000 samples, Generator draw (2e10 cells: above the legacy
     limit); the full-matrix path would need 160 GB.  One cold run of each arm (said so in the output).
  d  the ten host fits of common10 on b's 100 000 values (scipy on the CPU), once."""
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
from seekr_amd import _lib, consumers, find_dist, neighbors  # noqa: E402
from seekr_amd import pearson as pearson_mod  # noqa: E402
from seekr_amd.kmer_counts import BasicCounter  # noqa: E402
from seekr_amd.synthetic import synthetic_ascii  # noqa: E402

SAMPLES = 100_000


def med(ts):
    return round(statistics.median(ts) * 1e3, 3)


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def alternate(arms, runs):
    """{name: median ms} of callables run in turn, runs + 1 rounds, the first one a warm-up."""
    ts = {name: [] for name in arms}
    for rep in range(runs + 1):
        for name, fn in arms.items():
            t = timed(fn)[0]
            if rep:
                ts[name].append(t)
    return {name: med(v) for name, v in ts.items()}, {name: round(min(v) * 1e3, 3) for name, v in ts.items()}


def prepared_rows(ctx, seed, n, length, k):
    blob, offsets = synthetic_ascii(seed, n, length)
    x = _lib.count_per_kb(ctx, _lib.PackedSeqs.from_buffer(ctx, blob, offsets), k)
    _lib.normalize(ctx, x, "Log2.post", 1, None, 1, None)
    z, _ = _lib.operand_fill(ctx, x, None, pearson_mod._precision_for(np.dtype(np.float32), True))
    x.free()
    return z


def empty_sweep(ctx, z):
    with consumers.Sweep(z) as sweep:
        sweep.run(lambda buf, **where: None)
    ctx.sync()


def used_gib(ctx, free0):
    return round((free0 - ctx.mem_info()[0]) / 2 ** 30, 3)


def part_a(ctx, runs):
    z = prepared_rows(ctx, 1, 50_000, 2000, 6)
    n = z.rows
    index = consumers.draw_index(n * (n - 1) // 2, SAMPLES, np.random.default_rng(1))
    arms = {"sweep_only": lambda: empty_sweep(ctx, z), "pearson_sample": lambda: consumers.pearson_sample(z, None, index)}
    ms, low = alternate(arms, runs)
    ctx.prof_reset()
    ctx.prof_enable(True)
    consumers.pearson_sample(z, None, index)
    ctx.prof_enable(False)
    kernel_ms, launches = ctx.prof_query("gather_cells")
    z.free()
    return {"rows": n, "cols": 4096, "samples": SAMPLES, "stripe_rows": 8192, "sweep_only_ms": ms["sweep_only"],
            "pearson_sample_ms": ms["pearson_sample"], "sweep_only_min_ms": low["sweep_only"],
            "pearson_sample_min_ms": low["pearson_sample"],
            "sample_over_sweep": round(ms["pearson_sample"] / ms["sweep_only"], 4),
            "gather_kernel_ms": round(kernel_ms, 3), "gather_launches": int(launches),
            "gather_kernel_over_sweep": round(kernel_ms / ms["sweep_only"], 5)}


def part_b(ctx, runs, tmp):
    n, k = 12_996, 4
    os.chdir(tmp)  # the bkg_* vectors go to the working directory
    blob, offsets = synthetic_ascii(4, n, 1500)
    fasta = os.path.join(tmp, "bkg.fa")
    with open(fasta, "wb") as f:
        for i in range(n):
            f.write(b">t%d\n" % i + blob[offsets[i]:offsets[i + 1]].tobytes() + b"\n")
    cells = n * (n - 1) // 2
    res = {"rows": n, "k": k, "cells": cells, "samples": SAMPLES}
    state = {}

    def first_counter():
        c = BasicCounter(fasta, log2="Log2.post", k=k, silent=True)
        c.get_counts()
        np.save("bkg_mean_4mers.npy", c.mean)
        np.save("bkg_std_4mers.npy", c.std)

    def second_counter():
        c = BasicCounter(fasta, mean="bkg_mean_4mers.npy", std="bkg_std_4mers.npy", k=k, silent=True)
        c.make_count_file()
        state["counts"] = np.ascontiguousarray(c.counts, dtype=np.float32)

    def operand():
        if state.get("z") is not None:
            state["z"].free()
        state["z"] = neighbors._prepare(ctx, state["counts"], state["counts"], True)[0]

    stages = {}
    for name, fn in (("count_and_statistics", first_counter), ("count_and_normalise", second_counter), ("operand", operand)):
        ts = [timed(fn)[0] for _ in range(runs + 1)][1:]
        stages[name + "_ms"] = med(ts)
    z = state["z"]
    np.random.seed(3)
    draws = {"legacy_draw_ms": [], "generator_draw_ms": []}
    for _ in range(runs):
        t, index = timed(lambda: consumers.draw_index(cells, SAMPLES))
        draws["legacy_draw_ms"].append(t)
        draws["generator_draw_ms"].append(timed(lambda: consumers.draw_index(cells, SAMPLES, np.random.default_rng(3)))[0])
    stages.update({name: med(v) for name, v in draws.items()})
    index = np.ascontiguousarray(index, dtype=np.int64)
    free0 = ctx.mem_info()[0]
    mem = {}

    def sampled():
        with consumers.Sweep(z) as sweep:  # the same sweep, only to read the memory it holds
            sweep.run(lambda buf, **where: None)
            mem["sweep_gib"] = used_gib(ctx, free0)
        return consumers.pearson_sample(z, None, index)

    def full_matrix():
        r = ctx.empty(n, n)
        _lib.pearson_gemm_op(ctx, z, z, r)
        values = consumers.triu_values(r)
        mem["full_matrix_gib"] = used_gib(ctx, free0)
        out = np.empty(len(index), dtype=np.float32)
        _lib.check(_lib.lib().skr_gather_f32(ctx._h, values._h, index.ctypes.data, len(index), out.ctypes.data))
        values.free()
        r.free()
        return out

    a, b = sampled(), full_matrix()
    res["same_values_within_bar"] = bool(np.all(np.abs(a.astype(np.float64) - b) <= 2e-6 + 1e-5 * np.abs(b)))
    res["cells_with_other_bits"] = int((a.view(np.uint32) != b.view(np.uint32)).sum())
    ms, _ = alternate({"sweep_and_gather": lambda: consumers.pearson_sample(z, None, index), "full_matrix_path": full_matrix,
                       "sweep_only": lambda: empty_sweep(ctx, z)}, runs)
    stages["sweep_and_gather_ms"] = ms["sweep_and_gather"]
    stages["sweep_only_ms"] = ms["sweep_only"]
    res["stages"] = stages
    res["full_matrix_path_ms"] = ms["full_matrix_path"]
    res["device_gib"] = mem
    np.random.seed(3)
    whole = [timed(lambda: find_dist.find_dist(fasta, k, fit_model=False))[0] for _ in range(3)]
    res["find_dist_wall_runs"] = "median of 2 after one warm-up (the legacy draw makes each run seconds long)"
    res["find_dist_wall_ms"] = med(whole[1:])
    whole = [timed(lambda: find_dist.find_dist(fasta, k, fit_model=False, rng=np.random.default_rng(3)))[0] for _ in range(3)]
    res["find_dist_wall_generator_ms"] = med(whole[1:])
    z.free()
    return res, a


def part_c(ctx):
    n = 200_000
    z = prepared_rows(ctx, 5, n, 1000, 4)
    cells = n * (n - 1) // 2
    free0 = ctx.mem_info()[0]
    t_draw, index = timed(lambda: consumers.draw_index(cells, SAMPLES))
    t, sample = timed(lambda: consumers.pearson_sample(z, None, index))
    t_empty = timed(lambda: empty_sweep(ctx, z))[0]
    z.free()
    return {"runs": "one cold run of each arm, no warm-up", "rows": n, "cols": 256, "cells": cells, "samples": SAMPLES, "above_legacy_limit": cells > consumers.LEGACY_DRAW_MAX_CELLS,
            "draw_ms": round(t_draw * 1e3, 3), "pearson_sample_ms": round(t * 1e3, 1), "sweep_only_ms": round(t_empty * 1e3, 1),
            "block_buffer_gib": round(8192 * n * 4 / 2 ** 30, 3), "full_matrix_would_need_gib": round(n * n * 4 / 2 ** 30, 1),
            "free_before_gib": round(free0 / 2 ** 30, 1), "nan_in_sample": int(np.isnan(sample).sum())}


def part_d(sample):
    t, fits = timed(lambda: find_dist.fit_distributions(sample, find_dist.COMMON10, "ks", False))
    return {"runs": "once", "values": int(len(sample)), "models": len(find_dist.COMMON10), "fitted": len(fits), "seconds": round(t, 2),
            "best": fits[0][0] if fits else None}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-large", action="store_true")
    ap.add_argument("--skip-fits", action="store_true")
    args = ap.parse_args()
    ctx = _lib.default_context()
    res = {"box": socket.gethostname(), "runs": args.runs}
    res["a_kernel_cost"] = part_a(ctx, args.runs)
    print(json.dumps(res["a_kernel_cost"]), flush=True)
    here = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        res["b_reference_shape"], sample = part_b(ctx, args.runs, tmp)
        os.chdir(here)
    print(json.dumps(res["b_reference_shape"]), flush=True)
    if not args.skip_large:
        res["c_large_background"] = part_c(ctx)
        print(json.dumps(res["c_large_background"]), flush=True)
    if not args.skip_fits:
        res["d_host_fits"] = part_d(sample)
        print(json.dumps(res["d_host_fits"]), flush=True)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
