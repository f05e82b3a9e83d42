"""domain_hits and the run kernel behind it.  One process, one GPU.

    python tools/domain_hits_bench.py [--out profiles/domain_hits_bench.json] [--windows 1000000]

1. skr_run_pieces_ge against skr_select_cells_ge (both with outputs, preallocated) on the same block of real r (k = 6
   profiles of synthetic 2 000 nt transcripts, rows against rows), the same cutoff, in this process: blocks of 100 x 65 536
   and 8 192 x 50 000, cutoffs that keep about 1e-3 and 5 % of the cells (quantiles of the block's first 256 rows),
   max_gap 0 and 2, with and without a sequence vector (a boundary every 997 columns).  Median, fastest and slowest of 9,
   the arms alternating.  Both kernels read the block twice; the run kernel writes fewer outputs and does more LDS work.
2. domain_hits for 100 queries x --windows windows (window 1 000, slide 100) beside domain_significant, domain_topk and
   domain_pearson on the same input in the same run: wall time, bytes to the host, peak device memory."""
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
from seekr_amd import _lib, windows  # noqa: E402
from seekr_amd.synthetic import synthetic_ascii  # noqa: E402
from significant_bench import ALPHA, METHOD, PeakMemory, operand  # noqa: E402

REPEATS = 9


def spread(times):
    t = sorted(times)
    return {"median_ms": round(1e3 * t[len(t) // 2], 4), "min_ms": round(1e3 * t[0], 4), "max_ms": round(1e3 * t[-1], 4)}


def kernel_against_select(ctx, rows, cols):
    z = operand(ctx, rows + cols, 2000)
    r = ctx.empty(rows, cols)
    _lib.pearson_gemm_op(ctx, z.view(0, rows), z.view(rows, cols), r)
    ctx.sync()
    z.free()
    sample = np.array(r.to_numpy(0, min(rows, 256))).reshape(-1)
    seq = ctx.from_numpy((np.arange(cols) // 997).astype(np.uint32))
    lib, count = _lib.lib(), C.c_int64(0)
    out = []
    for keep in (1e-3, 0.05):
        cutoff = float(np.quantile(sample, 1.0 - keep))
        cap = int(rows * cols * keep * 2) + 4096
        cells = [ctx.empty(cap, 1, t) for t in (np.uint32, np.uint32, np.float32)]
        pieces = [ctx.empty(cap, 1, t) for t in (np.uint32, np.uint32, np.uint32, np.uint32, np.float32, np.uint32)]
        head = (ctx._h, r._h, rows, 0, cols, 0, 0, C.c_float(cutoff))

        def select():
            _lib.check(lib.skr_select_cells_ge(*head, *[m._h for m in cells], 0, C.byref(count), None))

        def runs(max_gap, with_seq):
            def call():
                _lib.check(lib.skr_run_pieces_ge(*head, seq._h if with_seq else None, max_gap, *[m._h for m in pieces], 0,
                                                 C.byref(count), None))
            return call

        arms = {"skr_select_cells_ge": select, "run_pieces_gap0": runs(0, False), "run_pieces_gap2": runs(2, False),
                "run_pieces_gap0_seq": runs(0, True), "run_pieces_gap2_seq": runs(2, True)}
        row = {"rows": rows, "cols": cols, "keep_asked": keep, "cutoff": cutoff, "block_bytes": rows * cols * 4}
        times = {name: [] for name in arms}
        for name, call in arms.items():  # once each before the clock: buffers, and the counts
            call()
            ctx.sync()
            row[("cells_kept" if name == "skr_select_cells_ge" else name + "_pieces")] = count.value
            assert count.value <= cap
        for _ in range(REPEATS):  # the arms alternate
            for name, call in arms.items():
                t0 = time.perf_counter()
                call()
                ctx.sync()
                times[name].append(time.perf_counter() - t0)
        for name in arms:
            row[name] = spread(times[name])
            if name != "skr_select_cells_ge":
                row[name]["over_select_cells"] = round(row[name]["median_ms"] / row["skr_select_cells_ge"]["median_ms"], 3)
        row["keep_measured"] = round(row["cells_kept"] / (rows * cols), 6)
        for m in cells + pieces:
            m.free()
        out.append(row)
        print(json.dumps(row), flush=True)
    r.free()
    seq.free()
    return out


def domain(ctx, n_windows, tmp):
    k, window, slide, n_query = 6, 1000, 100, 100
    length = (n_windows - 1) * slide + window
    paths = {name: os.path.join(tmp, name + ".fa") for name in ("query", "target", "unrelated")}
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    for name, seed, n, size in (("query", 3, n_query, window), ("target", 4, 1, length), ("unrelated", 5, 1, 200 * slide + window)):
        rng = np.random.default_rng(seed)
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
    row = {"queries": n_query, "windows": n_windows, "k": k, "window": window, "slide": slide, "alpha": ALPHA,
           "background": {"dist": "norm", "mean": fitres[0][2][0], "sd": fitres[0][2][1]}}
    calls = (("domain_hits_raw_p", lambda: windows.domain_hits(*args, fitres=fitres, alpha=ALPHA, max_gap=1)),
             ("domain_hits_raw_p_again", lambda: windows.domain_hits(*args, fitres=fitres, alpha=ALPHA, max_gap=1)),
             ("domain_hits_fdr_bh", lambda: windows.domain_hits(*args, fitres=fitres, alpha=ALPHA, method=METHOD, max_gap=1)),
             ("domain_significant", lambda: windows.domain_significant(*args, fitres, method=METHOD, alpha=ALPHA)),
             ("domain_topk", lambda: windows.domain_topk(*args, top=10)),
             ("domain_pearson", lambda: windows.domain_pearson(*args)))
    for name, call in calls:
        ctx.sync()
        with PeakMemory(ctx) as mem:
            t0 = time.perf_counter()
            out = call()
            ctx.sync()
            wall = time.perf_counter() - t0
        row[name] = {"wall_s": round(wall, 3), "peak_device_bytes": mem.peak_bytes}
        if name.startswith("domain_hits"):
            row[name].update(hits=len(out), n_pieces=out.attrs["n_pieces"], r_cutoff=out.attrs["r_cutoff"],
                             hot_windows=int(out["n_hot"].sum()),
                             bytes_to_host=out.attrs["n_pieces"] * 24)  # six 4-byte fields a piece; 24 bytes a cell with -m
        elif name == "domain_significant":
            row[name].update(significant_cells=len(out), n_candidates=out.attrs["n_candidates"], bytes_to_host=len(out) * 24)
        elif name == "domain_topk":
            row[name]["bytes_to_host"] = n_query * 10 * 8
        else:
            row[name]["bytes_to_host"] = int(out[0].nbytes)
        del out
        print(json.dumps({name: row[name]}), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--windows", type=int, default=1000000)
    args = ap.parse_args()
    ctx = _lib.default_context()
    res = {"box": socket.gethostname(), "repeats": REPEATS}

    def save():
        if args.out:
            with open(args.out, "w") as f:
                json.dump(res, f, indent=1)
                f.write("\n")

    res["kernel"] = kernel_against_select(ctx, 100, 65536) + kernel_against_select(ctx, 8192, 50000)
    save()
    with tempfile.TemporaryDirectory() as tmp:
        res["domain"] = domain(ctx, args.windows, tmp)
    save()


if __name__ == "__main__":
    main()
