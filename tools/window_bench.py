"""Sliding-window counting and domain_pearson at scale: 50 synthetic sequences of 2 Mbases, k = 6, window 1 000, slide 100
(999 550 rows, 16.4 GB of float32 rows).

    python tools/window_bench.py [--seqs 50] [--length 2000000] [-k 6] [--window 1000] [--slide 100] [--rounds 7]
                                 [--queries 100] [--out profiles/window_counts_bench.json] [--skip-old] [--skip-domain]

Prints one JSON line (and writes it to --out):
  new        kernel time of skr_count_windows_per_kb (HIP events around the launch, median and min of --rounds launches
             after a warm-up) and its bytes written per second as a fraction of the HBM peak bench.py uses
  old        what a caller had to do without it: substrings cut on the host, skr_seqs_pack, skr_count_per_kb — device time
             of the counting kernel (same rounds) and the wall time of cutting + packing + counting once
  domain     domain_pearson of --queries queries against the same target: wall time, and the peak device memory in use
             (hipMemGetInfo sampled from a second thread) at two target sizes that differ by a factor of 4, chunk_rows fixed
A sample of rows of the two counting paths is compared bit for bit."""
import argparse
import json
import os
import socket
import statistics
import sys
import tempfile
import threading
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
from seekr_amd import _lib  # noqa: E402
from seekr_amd.synthetic import synthetic_ascii  # noqa: E402

HBM_GBS = 8000.0  # bench.py: PEAK["hbm_gbs"]


def kernel_ms(ctx, prefix, launch):
    ctx.prof_reset()
    ctx.prof_enable(True)
    launch()
    ctx.sync()
    ctx.prof_enable(False)
    return sum(ctx.prof_query(n)[0] for n in ctx.prof_names() if n.startswith(prefix))


def summary(ms, nbytes):
    med = statistics.median(ms)
    return {"median_ms": round(med, 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "runs": len(ms),
            "gbs": round(nbytes / med / 1e6, 1), "hbm_frac": round(nbytes / med / 1e6 / HBM_GBS, 4)}


def cut_substrings(blob, offsets, window, slide):
    """The old way's host work: every window as a sequence of its own, one concatenated buffer + offsets."""
    pieces, lengths = [], []
    for i in range(len(offsets) - 1):
        seq = blob[offsets[i]:offsets[i + 1]]
        full = np.lib.stride_tricks.sliding_window_view(seq, window)[::slide] if len(seq) >= window else np.empty((0, window), np.uint8)
        pieces.append(np.ascontiguousarray(full).reshape(-1))
        lengths += [window] * len(full)
        last = (len(full) - 1) * slide if len(full) else 0
        if not len(full) or last + window < len(seq):  # the tail window, shorter than the others
            start = last + slide if len(full) else 0
            pieces.append(seq[start:])
            lengths.append(len(seq) - start)
    off = np.zeros(len(lengths) + 1, dtype=np.int64)
    np.cumsum(lengths, out=off[1:])
    return np.concatenate(pieces), off


class PeakMemory:
    """Lowest free device memory seen while the block runs, sampled every 5 ms from a second thread."""

    def __init__(self, ctx):
        self.ctx, self.lowest, self.stop = ctx, None, threading.Event()

    def __enter__(self):
        self.before = self.lowest = self.ctx.mem_info()[0]
        self.thread = threading.Thread(target=self._run, daemon=True)
        self.thread.start()
        return self

    def _run(self):
        while not self.stop.is_set():
            self.lowest = min(self.lowest, self.ctx.mem_info()[0])
            time.sleep(0.005)

    def __exit__(self, *exc):
        self.stop.set()
        self.thread.join()
        self.peak_used = self.before - self.lowest


def write_fasta(path, blob, offsets, prefix):
    with open(path, "wb") as f:
        for i in range(len(offsets) - 1):
            f.write(b">%s%d\n" % (prefix.encode(), i))
            f.write(blob[offsets[i]:offsets[i + 1]].tobytes())
            f.write(b"\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seqs", type=int, default=50)
    ap.add_argument("--length", type=int, default=2_000_000)
    ap.add_argument("-k", type=int, default=6)
    ap.add_argument("--window", type=int, default=1000)
    ap.add_argument("--slide", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--queries", type=int, default=100)
    ap.add_argument("--chunk-rows", type=int, default=65536)
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-old", action="store_true")
    ap.add_argument("--skip-domain", action="store_true")
    args = ap.parse_args()
    from seekr_amd.windows import domain_pearson, window_table
    ctx = _lib.default_context()
    k, window, slide = args.k, args.window, args.slide
    blob, offsets = synthetic_ascii(1, args.seqs, args.length)
    packed = _lib.PackedSeqs.from_buffer(ctx, blob, offsets)
    n_rows = len(window_table(np.diff(offsets), window, slide)[0])
    nbytes = n_rows * 4 ** k * 4
    res = {"box": socket.gethostname(), "seqs": args.seqs, "length": args.length, "k": k, "window": window, "slide": slide,
           "rows": n_rows, "row_bytes_gb": round(nbytes / 1e9, 3), "hbm_peak_gbs": HBM_GBS}
    out = ctx.empty(n_rows, 4 ** k)

    # ---- the new kernel
    times = [kernel_ms(ctx, "count_windows", lambda: _lib.count_windows(ctx, packed, k, window, slide, 0, n_rows, out=out))
             for _ in range(args.rounds + 1)][1:]  # the first launch warms up
    res["new"] = summary(times, nbytes)
    sample = [(0, 1000), (n_rows // 2, 1000), (n_rows - 1000, 1000)]
    new_sample = [out.to_numpy(r0, n).copy() for r0, n in sample]
    print("new:", json.dumps(res["new"]), flush=True)

    # ---- the old way at the same size
    if not args.skip_old:
        t0 = time.perf_counter()
        sub_blob, sub_off = cut_substrings(blob, offsets, window, slide)
        t_cut = time.perf_counter() - t0
        assert len(sub_off) - 1 == n_rows
        sub_packed = _lib.PackedSeqs.from_buffer(ctx, sub_blob, sub_off)
        t_pack = time.perf_counter() - t0 - t_cut
        _lib.count_per_kb(ctx, sub_packed, k, out=out)
        ctx.sync()
        t_wall = time.perf_counter() - t0
        old, alt = [], []  # the two paths alternating in one process: the comparison of the device times is made on these
        for _ in range(args.rounds):
            old.append(kernel_ms(ctx, "count_kmers", lambda: _lib.count_per_kb(ctx, sub_packed, k, out=out)))
            alt.append(kernel_ms(ctx, "count_windows", lambda: _lib.count_windows(ctx, packed, k, window, slide, 0, n_rows, out=out)))
        res["new_alternating_with_old"] = summary(alt, nbytes)
        _lib.count_per_kb(ctx, sub_packed, k, out=out)
        res["old"] = dict(summary(old, nbytes), host_cut_s=round(t_cut, 3), pack_upload_s=round(t_pack, 3),
                          wall_cut_pack_count_s=round(t_wall, 3), text_bytes_gb=round(len(sub_blob) / 1e9, 3))
        for (r0, n), want in zip(sample, new_sample):
            assert np.array_equal(out.to_numpy(r0, n).view(np.uint32), want.view(np.uint32)), "rows differ from the old way"
        res["rows_compared_bitwise"] = sum(n for _, n in sample)
        t0 = time.perf_counter()
        _lib.count_windows(ctx, packed, k, window, slide, 0, n_rows, out=out)
        ctx.sync()
        res["new"]["wall_count_s"] = round(time.perf_counter() - t0, 4)
        res["new_over_old_device_time"] = round(res["new_alternating_with_old"]["median_ms"] / res["old"]["median_ms"], 4)
        del sub_packed, sub_blob
        print("old:", json.dumps(res["old"]), flush=True)
    del out

    # ---- domain_pearson: wall time at the full target, device memory at a quarter of it and at the whole
    if not args.skip_domain:
        from seekr_amd.kmer_counts import BasicCounter
        bg = BasicCounter(k=k, silent=True)
        bg_blob, bg_off = synthetic_ascii(2, 2000, 2000)
        bg.seqs = [bg_blob[bg_off[i]:bg_off[i + 1]].tobytes().decode() for i in range(2000)]
        bg.get_counts()
        mean, std = bg.mean, bg.std
        del bg
        with tempfile.TemporaryDirectory() as tmp:
            q_blob, q_off = synthetic_ascii(3, args.queries, 1500)
            qfa = os.path.join(tmp, "q.fa")
            write_fasta(qfa, q_blob, q_off, "q")
            dom = {"queries": args.queries, "chunk_rows": args.chunk_rows, "targets": []}
            quarter = max(1, args.seqs // 4)
            for n_seqs in (quarter, 4 * quarter, args.seqs):
                if any(t["seqs"] == n_seqs for t in dom["targets"]):
                    continue
                tfa = os.path.join(tmp, "t%d.fa" % n_seqs)
                write_fasta(tfa, blob, offsets[:n_seqs + 1], "t")
                walls = []
                for rep in range(3):
                    with PeakMemory(ctx) as pm:
                        t0 = time.perf_counter()
                        r, table = domain_pearson(qfa, tfa, k, window, slide, mean, std, chunk_rows=args.chunk_rows)
                        walls.append(time.perf_counter() - t0)
                    assert np.isfinite(r).all() and r.shape == (args.queries, len(table))
                dom["targets"].append({"seqs": n_seqs, "windows": int(r.shape[1]), "wall_s": [round(w, 3) for w in walls],
                                       "peak_device_bytes_in_use": int(pm.peak_used),
                                       "packed_target_bytes": int(n_seqs * (args.length // 4 + 8))})
                del r, table
            res["domain_pearson"] = dom
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
