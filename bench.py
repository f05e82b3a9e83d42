#!/usr/bin/env python3
"""Benchmark of the SEEKR hot path on MI355X: k-mer counting -> numpy-order normalisation
(Log2.post) -> row standardisation -> all-pairs Pearson of the set against itself.

    python bench.py --gpus 1 --steps 3 --warmup 1
    python bench.py --gpus N ...                       # starts its own N rank processes (below)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W

One "step" is one pass of that pipeline over one synthetic transcript set whose packed bases
are already resident in HBM; the correlation matrix stays in HBM.  Work per GPU is fixed in
the metric's unit (ordered sequence pairs): N_rows(G) = 50 000 * sqrt(G), so G=1 is
BASELINE.json configs[1] (50k x 2 kb, k=6) and scaling is weak.  Rank 0 prints one JSON line.

A plain run sets up, warms up, times `--steps` steps and prints the line (`value`, `ms_per_step`, and the
roofline and per-kernel figures of the timed steps themselves).  `--full` adds what runs after the timed region:
the check of r against the oracle (`verified`), the f16f8 arm, the CPU baseline, the 200 000-row target and the
`e2e` record at N = 1; the all-reduced check and the opt-in chain A/B at N > 1.  `--dump-outputs DIR` writes
what the last timed step computed (a seeded sample of rows of r and of the normalised counts, the column mean and
std) to DIR/*.npy; the inputs are the same in every run with the same arguments.

On G > 1 GPUs the default result layout is the symmetric one (seekr_amd/distributed.py): each
unordered pair of row shards is multiplied once, by one of its two ranks, which keeps the
block and its transpose; every ordered pair ends up in exactly one GPU's HBM, as on one GPU
(where the lower triangle is the mirror of the upper).  `--layout rowblock` gives every rank
its full rows of r instead, multiplying each off-diagonal block twice across the node; `--layout
allgather` produces the same row blocks after ONE RCCL all-gather of the prepared operands (the
schedule BASELINE.json's north_star names: no overlap, a single collective).

Launching.  With WORLD_SIZE in the environment (torch.distributed.run, or any launcher that sets
RANK / LOCAL_RANK / WORLD_SIZE / MASTER_PORT) this process IS one rank.  Without it and with
--gpus N > 1 this process is only a launcher: it never loads the HIP library or touches a GPU, starts N
fresh child processes of this same script (one per GPU, no exec of a GPU-initialised process), forwards
rank 0's JSON line, and on any rank's failure or after --launch-timeout seconds kills exactly the
process groups it started and exits non-zero with every rank's stderr tail.  A failed first attempt
in the symmetric layout (including a failed self-test of the half-ring schedule, exit code 17) is
retried ONCE, in a new set of children, with the most conservative configuration — row blocks after one
all-gather of the operands (no shifts, no tickets to order) and the column-sum chain over send/recv; the
JSON line then carries "layout_fallback".
"""
import argparse
import hashlib
import json
import math
import os
import re
import signal
import socket
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PEAK = {"hbm_gbs": 8000.0, "fp32_mfma_tflops": 157.3, "bf16_mfma_tflops": 2500.0}  # MI355X_MICROARCH.md
SEED = 2
SELFTEST_EXIT = 17  # the half-ring schedule's self-test disagreed with the row-block result on some rank


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rows", type=int, default=0, help="total transcripts (default 50000*sqrt(gpus))")
    ap.add_argument("--length", type=int, default=2000)
    ap.add_argument("-k", "--k", type=int, default=6, dest="k")
    ap.add_argument("--alphabet", default="AGTC", help="any string the reference accepts (kmer_counts.py:120-122); other than four "
                    "distinct letters the step counts with the any-alphabet kernel from resident ASCII (len^k columns)")
    ap.add_argument("--precision", default=os.environ.get("SEEKR_PRECISION", "f16x3"),
                    choices=["fp32", "bf16x3", "f16x3", "f16f8"],
                    help="Pearson contraction arithmetic; every choice is inside the parity bar "
                         "|dr| <= 2e-6 + 1e-5|r| (tests/test_gpu_parity.py) on the bench data; f16x3 carries float32-grade operands, bf16x3 is ~5 %% faster")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-f16f8-arm", action="store_true", help="skip the opt-in two-product-unit contraction's extra measurement "
                    "after the timed region (f16f8_arm in the line)")
    ap.add_argument("--no-target-200k", action="store_true", help="skip the 200 000-transcript sub-record after the timed region "
                    "(target_200k in the line; default workload at --gpus 1 only)")
    ap.add_argument("--no-symmetry", action="store_true",
                    help="compute both triangles of the self-comparison block instead of mirroring one")
    ap.add_argument("--grouped-shifts", action="store_true",
                    help="symmetric layout: post all half-ring shifts as one grouped exchange (one receive buffer per shift)")
    ap.add_argument("--layout", default="symmetric", choices=["symmetric", "rowblock", "allgather"],
                    help="multi-GPU schedule (see module docstring): symmetric half ring, row blocks by pairwise shifts, or row "
                         "blocks after ONE all-gather of the operands; fp32 / --no-symmetry imply rowblock")
    ap.add_argument("--launch-timeout", type=float, default=300.0,
                    help="launcher mode: seconds after which the rank processes are killed")
    ap.add_argument("--no-selftest", action="store_true", help="skip the half-ring schedule's self-test before the warm-up")
    ap.add_argument("--full", action="store_true",
                    help="after the timed region, also run the extras: the check of r against the oracle (verified; at N > 1 "
                         "on every rank), the f16f8 arm, the CPU baseline, the 200 000-row target, the e2e record and (N > 1, "
                         "opt-in) the chain A/B; without it a run sets up, warms up, times its steps and prints the line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last step computed to DIR/<name>.npy (float32, < 64 MB in all; "
                         "a fixed, seeded sample of rows): counts, mean, std, r (one GPU only)")
    args = ap.parse_args(argv)
    if args.dump_outputs and args.gpus != 1:
        ap.error("--dump-outputs needs --gpus 1 (r is spread over the ranks' HBM at N > 1)")
    return args


# ------------------------------------------------------------------------------------ launcher ----
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _tail(path, n=30):
    try:
        with open(path, "rb") as fh:
            return b"\n".join(fh.read().splitlines()[-n:]).decode("utf-8", "replace")
    except OSError:
        return ""


def _kill_group(proc):
    """Ends exactly the process group this launcher started for `proc` (start_new_session: pgid == pid)."""
    for sig in (signal.SIGTERM, signal.SIGKILL):
        if proc.poll() is not None:
            return
        try:
            os.killpg(proc.pid, sig)
        except (ProcessLookupError, PermissionError):
            return
        try:
            proc.wait(timeout=5)
        except subprocess.TimeoutExpired:
            pass


def _run_rank_set(argv, size, timeout_s, extra_env, log_dir, attempt, program=None):
    """One set of `size` fresh rank processes (`program`: what to run instead of this script — the launcher's own
    tests).  Returns (ok, json_line or failure kind, report)."""
    program = program or [sys.executable, os.path.abspath(__file__)]
    port = _free_port()
    base = dict(os.environ, WORLD_SIZE=str(size), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    base.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    base.update(extra_env)
    procs, logs = [], []
    for rank in range(size):
        out_path = os.path.join(log_dir, "attempt{}_rank{}.out".format(attempt, rank))
        err_path = os.path.join(log_dir, "attempt{}_rank{}.err".format(attempt, rank))
        logs.append((out_path, err_path))
        env = dict(base, RANK=str(rank), LOCAL_RANK=str(rank))
        with open(out_path, "wb") as fo, open(err_path, "wb") as fe:
            procs.append(subprocess.Popen(program + argv, env=env, stdout=fo, stderr=fe,
                                          stdin=subprocess.DEVNULL, start_new_session=True))
    deadline = time.time() + timeout_s
    failed, reason = None, None
    try:
        while True:
            codes = [p.poll() for p in procs]
            bad = [(r, c) for r, c in enumerate(codes) if c not in (None, 0)]
            if bad:
                # the others usually follow with their own message (a failed all-reduce, the self-test's verdict): give
                # them a moment before the groups are killed, so that the report below holds every rank's own words
                grace = time.time() + 3.0
                while time.time() < grace and any(p.poll() is None for p in procs):
                    time.sleep(0.05)
                failed = [(r, c) for r, c in enumerate(p.poll() for p in procs) if c not in (None, 0)]
                reason = "rank {} exited with code {}".format(bad[0][0], bad[0][1])
                break
            if all(c == 0 for c in codes):
                break
            if time.time() > deadline:
                failed = [(r, None) for r, c in enumerate(codes) if c is None]
                reason = "timeout after {:.0f} s (ranks still running: {})".format(timeout_s, [r for r, _ in failed])
                break
            time.sleep(0.05)
    finally:
        for p in procs:
            _kill_group(p)
    if failed is None:
        with open(logs[0][0], "r", errors="replace") as fh:
            lines = [ln for ln in fh.read().splitlines() if ln.startswith("{")]
        if len(lines) == 1:
            return True, lines[0], ""
        reason = "rank 0 printed {} JSON lines".format(len(lines))
    report = ["bench.py launcher, attempt {}: {}".format(attempt, reason)]
    for rank, (out_path, err_path) in enumerate(logs):
        report.append("---- rank {} (exit code {}) stderr tail ----".format(rank, procs[rank].returncode))
        report.append(_tail(err_path) or "(empty)")
        extra = _tail(out_path, 5)
        if extra and rank != 0:
            report.append("---- rank {} stdout tail ----\n{}".format(rank, extra))
    selftest = any(c == SELFTEST_EXIT for _, c in (failed or []))
    return False, ("selftest" if selftest else reason), "\n".join(report)


def launch(args, argv):
    """Launcher mode (no WORLD_SIZE, --gpus N > 1): see the module docstring.  Returns the exit code."""
    size = args.gpus
    symmetric = args.layout == "symmetric" and args.precision != "fp32" and not args.no_symmetry
    with tempfile.TemporaryDirectory(prefix="seekr_bench_") as log_dir:
        # the column sums travel over send/recv (the transport that has run).  The peer-mailbox chain can be measured next
        # to it AFTER the timed region (chain_ab in the line), but only when asked for (SEEKR_BENCH_CHAIN_AB=1): its
        # in-kernel wait has never met a second real GPU, and a hang there would discard the line already measured and —
        # worse — send the launcher into the layout fallback below for a reason that has nothing to do with the layout
        # (ADVICE r4).  A failure of the A/B that does return is reported inside chain_ab, never as a failed attempt.
        ab = os.environ.get("SEEKR_BENCH_CHAIN_AB", "0")
        ok, payload, report = _run_rank_set(argv, size, args.launch_timeout, {"SEEKR_BENCH_CHAIN_AB": ab}, log_dir, 1)
        if not ok and symmetric:
            print(report, file=sys.stderr, flush=True)
            why = ("the half-ring schedule's self-test failed" if payload == "selftest"
                   else "the first attempt failed ({})".format(payload))
            print("bench.py launcher: {}; retrying once in a new set of rank processes with --layout allgather".format(why),
                  file=sys.stderr, flush=True)
            argv2 = [a for a in argv if a != "--grouped-shifts"]
            for i, a in enumerate(argv2):
                if a == "--layout":
                    del argv2[i:i + 2]
                    break
            argv2 = [a for a in argv2 if not a.startswith("--layout=")] + ["--layout", "allgather"]
            # the retry is the most conservative configuration: row blocks, and the column-sum chain over send/recv
            ok, payload, report = _run_rank_set(argv2, size, args.launch_timeout,
                                                {"SEEKR_BENCH_FALLBACK": "symmetric layout abandoned: " + why, "SEEKR_CHAIN": "rccl",
                                                 "SEEKR_BENCH_CHAIN_AB": "0"},
                                                log_dir, 2)
        if ok:
            print(payload, flush=True)
            return 0
        print(report, file=sys.stderr, flush=True)
        return 1


# ------------------------------------------------------------------------------------ one rank ----
def cpu_baseline(k, length, x_norm_head, repeats=3):
    """The oracle (a port with the reference's structure: per-window dict increments in pure
    Python, numpy row standardisation + np.inner) timed on a bounded prefix of the workload:
    `repeats` runs of each leg, median taken."""
    from oracle import seekr_oracle as orc
    from seekr_amd.synthetic import synthetic_codes
    n_count = max(500, int(6000 * 2000 / length))  # ~12 Mbases: ~2 s per repeat of counting on the GPU box's host
    seqs = orc.codes_to_seqs(synthetic_codes(SEED, n_count, length))
    t_counts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        orc.raw_counts_py(seqs, k)
        t_counts.append(time.perf_counter() - t0)
    t_count = float(np.median(t_counts))
    rate_bases = n_count * length / t_count
    n_p = x_norm_head.shape[0]
    orc.pearson(x_norm_head[:512], x_norm_head[:512])  # BLAS warm-up
    t_ps = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        orc.pearson(x_norm_head, x_norm_head)
        t_ps.append(time.perf_counter() - t0)
    t_p = float(np.median(t_ps))
    rate_pairs = n_p * n_p / t_p
    try:
        from threadpoolctl import threadpool_info
        blas_threads = max([p.get("num_threads", 1) for p in threadpool_info()] or [1])
    except Exception:  # noqa: BLE001
        blas_threads = os.cpu_count()
    return {"rate_bases": rate_bases, "rate_pairs": rate_pairs, "t_count": t_count, "t_pearson": t_p,
            "n_count": n_count, "n_pearson": n_p, "blas_threads": blas_threads, "repeats": repeats}


def verify_rows(ctx, r, x_norm, n_check=32, seed=1):
    """After the timed region: `n_check` random rows of the r the bench just produced (all columns, so
    both the multiplied and the mirrored triangle) against the oracle's pearson (pearson.py:35-41) on the
    host copy of the normalised counts.  Returns (ok, worst error / bar); bar = 2e-6 + 1e-5 |r|.
    (Each checked row holds ONE r = 1 cell, its diagonal one, and that cell is written by patch_diag_kernel from the
    fill's tree sum, not by the contraction — VERDICT r4 weak #8: the verdict on the contraction is what the other
    n - 1 cells of the row say.)"""
    from oracle import seekr_oracle as orc
    n = x_norm.shape[0]
    rows = np.sort(np.random.default_rng(seed).choice(n, min(n_check, n), replace=False))
    a = x_norm[rows]
    got = np.stack([r.to_numpy(int(row), 1).reshape(-1) for row in rows])
    worst = 0.0
    for c0 in range(0, n, 16384):
        want = orc.pearson(a, x_norm[c0:c0 + 16384])
        err = np.abs(got[:, c0:c0 + 16384] - want) / (2e-6 + 1e-5 * np.abs(want))
        worst = max(worst, float(np.max(err)))  # a NaN (there is none in this workload) fails the check
        if not np.isfinite(worst):
            return False, worst
    return worst <= 1.0, worst


DUMP_BYTES = {"r": 48e6, "counts": 12e6}  # mean and std (4 B per column) take the rest of 64 MB


def dump_outputs(out_dir, r, x, mean, std):
    """What the last step computed, as a caller of the pipeline receives it (BasicCounter: counts, mean, std; pearson: r),
    written as float32 .npy files: the column mean and std whole, and a fixed, seeded sample of rows (the same rows of the
    normalised counts and of r, all columns of each; as many as fit in DUMP_BYTES, sorted)."""
    n, n_cols = r.shape[1], x.shape[1]
    n_rows = max(1, min(x.shape[0], int(DUMP_BYTES["r"] // (4 * n)), int(DUMP_BYTES["counts"] // (4 * n_cols))))
    rows = np.sort(np.random.default_rng([SEED, 7]).choice(x.shape[0], n_rows, replace=False))
    os.makedirs(out_dir, exist_ok=True)
    arrays = {"counts": np.stack([x.to_numpy(int(i), 1).reshape(-1) for i in rows]),
              "r": np.stack([r.to_numpy(int(i), 1).reshape(-1) for i in rows]),
              "mean": mean.vector(), "std": std.vector()}
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), np.ascontiguousarray(a, dtype=np.float32))


def end_to_end(ctx, k, length, n_seqs, precision):
    """PCIe- and file-inclusive rates through the drop-in API (never `value`): FASTA file -> host
    float32 per-kb counts (BasicCounter: native reader + packer + H2D + kernel + D2H), and host ->
    host pearson() on a prefix (the result copy over PCIe dominates)."""
    from seekr_amd.kmer_counts import BasicCounter
    from seekr_amd.pearson import pearson
    from seekr_amd.synthetic import synthetic_ascii
    blob, _ = synthetic_ascii(SEED, n_seqs, length)
    rows = blob.reshape(n_seqs, length)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "cfg.fa")
        with open(path, "wb") as fh:
            fh.write(b"".join(b">s%d\n" % i + rows[i].tobytes() + b"\n" for i in range(n_seqs)))
        times = []
        for _ in range(3):
            t0 = time.perf_counter()
            c = BasicCounter(path, k=k, mean=False, std=False, log2="Log2.none", silent=True)
            c.get_counts()
            times.append(time.perf_counter() - t0)
        devices = end_to_end_devices(path, k, length, n_seqs, min(12000, n_seqs))
    t_counts = float(np.median(times))
    n_p = min(12000, n_seqs)
    head = np.ascontiguousarray(c.counts[:n_p])
    pearson(head[:256], head[:256])
    times = []
    for _ in range(3):
        t0 = time.perf_counter()
        pearson(head, head)
        times.append(time.perf_counter() - t0)
    t_p = float(np.median(times))
    return {"fasta_to_host_counts_mbases_per_s": round(n_seqs * length / t_counts / 1e6, 1),
            "fasta_to_host_counts_s": round(t_counts, 4),
            "host_to_host_pearson_mpairs_per_s": round(n_p * float(n_p) / t_p / 1e6, 1),
            "host_to_host_pearson_rows": n_p, "host_to_host_pearson_s": round(t_p, 4),
            "seekr_devices_all": devices,
            "note": "median of 3; file read + pack + H2D + kernels + D2H through seekr_amd.BasicCounter / "
                    "seekr_amd.pearson (raw counts; Pearson result copied to the host: PCIe-bound)"}


def target_200k(ctx, comm, engine, cb, peak_tf, n_total=200_000, length=2000, k=6, steps=3):
    """BASELINE.json's target — ">= 100x the reference CPU BasicCounter + pearson throughput on 200k x 2kb synthetic
    transcripts at k = 6" — at ITS size, in the driver's own run: after the timed region (never part of `value`), the same
    step on 200 000 transcripts (160 GB of r + 6.6 GB of counts and operands: fits one GPU), `steps` timed steps, 32 rows x
    200 000 columns of the r it produced against the oracle, and the speed-up against the CPU port's rates of this run."""
    from seekr_amd import _lib
    from seekr_amd.distributed import sharded_normalize_prepare, sharded_pearson_symmetric
    from seekr_amd.synthetic import synthetic_ascii
    t_all = time.perf_counter()
    n_cols = 4 ** k
    blob, offsets = synthetic_ascii(SEED, n_total, length)
    packed = _lib.PackedSeqs.from_buffer(ctx, blob, offsets, "AGTC")
    del blob
    x, z, r = ctx.empty(n_total, n_cols), engine.empty_operand(n_total, n_cols), ctx.zeros(n_total, n_total)
    bounds = [0, n_total]

    def step():
        _lib.count_per_kb(ctx, packed, k, out=x)
        zz = sharded_normalize_prepare(engine, comm, x, n_total, "Log2.post", True, True, keep_counts=True, op=z)[3]
        sharded_pearson_symmetric(engine, comm, zz, bounds, r, None, [None, None])

    step()
    ctx.sync()
    ctx.prof_reset()
    ctx.prof_enable(True)
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    ctx.sync()
    elapsed = time.perf_counter() - t0
    ctx.prof_enable(False)
    gemm_ms = ctx.prof_query("pearson_gemm_f16x3")[0] / steps
    count_ms = ctx.prof_query("count_kmers_f32")[0] / steps
    ok, worst = verify_rows(ctx, r, x.to_numpy())
    pairs = float(n_total) * n_total
    value = pairs * steps / elapsed / 1e6
    t_cpu = n_total * length / cb["rate_bases"] + pairs / cb["rate_pairs"]
    out = {"workload": "{} synthetic {} nt transcripts, k={}, counts + Log2.post normalisation + self Pearson".format(n_total, length, k),
           "steps": steps, "ms_per_step": round(elapsed / steps * 1e3, 2), "value": round(value, 2),
           "unit": "M seq-pairs/s (whole step: count + normalise + Pearson)",
           "pearson_kernel_ms": round(gemm_ms, 2), "count_kernel_ms": round(count_ms, 4),
           "roofline_frac": round(2.0 * n_cols * pairs / (gemm_ms * 1e-3) / 1e12 / peak_tf, 4) if gemm_ms > 0 else None,
           "verified": bool(ok), "verified_detail": {"rows": 32, "columns": n_total, "worst_error_over_bar": round(worst, 4)},
           "cpu_port_m_pairs_per_s": round(pairs / t_cpu / 1e6, 3), "speedup_vs_cpu_port": round(value / (pairs / t_cpu / 1e6), 1),
           "target": ">= 100x the CPU port at this size (BASELINE.json north_star)"}
    for m in (x, z, r, packed):
        m.free()
    out["wall_s"] = round(time.perf_counter() - t_all, 1)
    return out


E2E_DEVICES_CHILD = r'''
import json, os, sys, time
sys.path.insert(0, sys.argv[1])
import numpy as np
from seekr_amd import multi
from seekr_amd.kmer_counts import BasicCounter
from seekr_amd.pearson import pearson
path, k, n_p = sys.argv[2], int(sys.argv[3]), int(sys.argv[4])
out = {"devices": len(multi.requested_devices() or [0])}
t0 = time.perf_counter()
c = BasicCounter(path, k=k, mean=False, std=False, log2="Log2.none", silent=True); c.get_counts()
out["first_call_s"] = round(time.perf_counter() - t0, 3)  # includes the one-off RCCL set-up of the device group
ts = []
for _ in range(3):
    t0 = time.perf_counter(); c = BasicCounter(path, k=k, mean=False, std=False, log2="Log2.none", silent=True); c.get_counts()
    ts.append(time.perf_counter() - t0)
out["fasta_to_host_counts_s"] = round(float(np.median(ts)), 4)
out["n_seqs"], out["bases"] = int(c.counts.shape[0]), None
head = np.ascontiguousarray(c.counts[:n_p])
pearson(head[:512], head[:512])
ts = []
for _ in range(3):
    t0 = time.perf_counter(); pearson(head, head); ts.append(time.perf_counter() - t0)
out["host_to_host_pearson_s"] = round(float(np.median(ts)), 4)
out["host_to_host_pearson_rows"] = int(n_p)
out.update(multi.group_info())  # the transport that carried the data and the ranks its all-reduce counted
print(json.dumps(out), flush=True)
'''


def end_to_end_devices(fasta_path, k, length, n_seqs, n_p, timeout_s=240):
    """The same two host-to-host figures with SEEKR_DEVICES=all — every visible GPU behind BasicCounter / pearson()
    (seekr_amd/multi.py: one host thread and one PCIe link per GPU) — measured in a CHILD process with a time limit, so that
    nothing it does can cost the line measured above.  With one GPU visible there is nothing to compare."""
    from seekr_amd import _lib
    n_dev = _lib.device_count()
    # test hook (tests/test_gpu_multi_devices.py): a device list with repeats, so that the sub-record's code runs on a one-GPU box
    forced = os.environ.get("SEEKR_BENCH_E2E_DEVICES") if os.environ.get("SEEKR_TEST_HOOKS") == "1" else None
    if n_dev < 2 and not forced:
        return {"devices": n_dev, "note": "one GPU visible: SEEKR_DEVICES has nothing to add here"}
    env = {k_: v for k_, v in os.environ.items() if k_ not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "SEEKR_DEVICE")}
    env.update(SEEKR_DEVICES=forced or "all", HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    try:
        res = subprocess.run([sys.executable, "-c", E2E_DEVICES_CHILD, ROOT, fasta_path, str(k), str(n_p)], env=env,
                             capture_output=True, text=True, timeout=timeout_s)
    except subprocess.TimeoutExpired:
        return {"devices": n_dev, "error": "no result after {} s".format(timeout_s)}
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    if res.returncode != 0 or not lines:
        return {"devices": n_dev, "error": "exit code {}: {}".format(res.returncode, res.stderr.strip()[-400:])}
    got = json.loads(lines[-1])
    got["fasta_to_host_counts_mbases_per_s"] = round(n_seqs * length / got["fasta_to_host_counts_s"] / 1e6, 1)
    got["host_to_host_pearson_mpairs_per_s"] = round(n_p * float(n_p) / got["host_to_host_pearson_s"] / 1e6, 1)
    got.pop("bases", None)
    return got


def kernel_symbols_sha256(lib_path):
    """Fingerprint of the set of kernel symbols the library registers (their mangled names sit in its read-only
    data): tools/pmc_summary.py writes it into every summary, and a summary taken with a library whose kernel set
    differs from the one loaded now — a kernel added, removed, re-templated or given other arguments — is refused."""
    with open(lib_path, "rb") as fh:
        blob = fh.read()
    names = sorted({m for m in re.findall(rb"_Z[A-Za-z0-9_]{8,}", blob) if b"kernel" in m and b"__device_stub__" not in m})
    return hashlib.sha256(b"\n".join(names)).hexdigest()


def workload_key(rows, length, k, precision, gpus):
    return "rows={} length={} k={} precision={} gpus={}".format(rows, length, k, precision, gpus)


def pmc_traffic(kernel_key, workload, lib_path, profiles_dir=None):
    """HBM-side bytes per launch of a kernel from a committed rocprofv3 --pmc summary (tools/profile.sh; counters
    cannot be collected inside the timed run): WRITE_SIZE as reported, FETCH_SIZE doubled — gfx950 tallies the
    128-byte requests of wide coalesced reads at 64 bytes (MI355X_MICROARCH.md, HBM).  Only a summary of THIS
    workload (its `# workload:` line) taken with THIS library's kernel set (`# kernel_symbols_sha256:`) is used;
    returns (traffic or None, why-not or None)."""
    import glob
    want_hash = kernel_symbols_sha256(lib_path)
    why = "no profiles/*_pmc_summary.txt for workload '{}'".format(workload)
    for path in sorted(glob.glob(os.path.join(profiles_dir or os.path.join(ROOT, "profiles"), "*_pmc_summary.txt")), reverse=True):
        vals, inside, head = {}, False, {}
        with open(path) as fh:
            for line in fh:
                if line.startswith("#"):
                    m = re.match(r"#\s*(workload|kernel_symbols_sha256):\s*(.+?)\s*$", line)
                    if m:
                        head[m.group(1)] = m.group(2)
                elif not line.startswith(" "):
                    inside = kernel_key in line
                elif inside and line.split()[0] in ("FETCH_SIZE", "WRITE_SIZE"):
                    vals[line.split()[0]] = float(line.split()[1]) * 1024.0  # KiB
        if head.get("workload") != workload or len(vals) != 2:
            continue
        if head.get("kernel_symbols_sha256") != want_hash:
            why = "{} was taken with a library whose kernel set differs from the loaded one: refused".format(
                os.path.relpath(path, ROOT))
            continue
        return {"bytes": 2.0 * vals["FETCH_SIZE"] + vals["WRITE_SIZE"], "fetch_bytes_corrected": 2.0 * vals["FETCH_SIZE"],
                "write_bytes": vals["WRITE_SIZE"], "source": os.path.relpath(path, ROOT),
                "kernel_symbols_sha256": want_hash[:16]}, None
    return None, why


def exclusive_kernel_times(ctx):
    """{name: {ms_total, launches}} of the timed region.  skr_prof_query matches names exactly, so nested names
    ("colsum_seq" / "colsum_seq_sq") need no subtraction."""
    kern = {}
    for name in ctx.prof_names():
        ms, cnt = ctx.prof_query(name)
        kern[name] = {"ms_total": ms, "launches": cnt}
    return kern


def symmetric_selftest(ctx, comm, engine, k, grouped):
    """Before anything is timed: the half-ring schedule (split first shift, grouped shifts if asked for, CROSS-mode
    mirror stores) against the plain row-block schedule on a small set — every block this rank owns must equal the
    row-block result, and every mirrored block its transpose, bit for bit (same kernel arithmetic).  The verdict is
    all-reduced so that every rank leaves together.  Returns None or the reason."""
    from seekr_amd import _lib
    from seekr_amd.distributed import (shard_bounds, sharded_normalize_prepare, sharded_pearson_rowblock,
                                       sharded_pearson_symmetric)
    from seekr_amd.synthetic import synthetic_ascii
    size, rank = comm.size, comm.rank
    n_total = 600 * size + 37  # ragged shards, more than two tiles each
    bounds = shard_bounds(n_total, size)
    lo, hi = bounds[rank], bounds[rank + 1]
    blob, offsets = synthetic_ascii(SEED + 99, hi - lo, 400, start=lo)
    packed = _lib.PackedSeqs.from_buffer(ctx, blob, offsets, "AGTC")
    x = _lib.count_per_kb(ctx, packed, k)
    z = sharded_normalize_prepare(engine, comm, x, n_total, "Log2.post", True, True, keep_counts=False)[3]
    max_shard = max(bounds[g + 1] - bounds[g] for g in range(size))
    n_recv = max(2, size // 2) if grouped else 2
    recv = [engine.empty_operand(max_shard, 4 ** k) for _ in range(n_recv)]
    r_row, r_col, r_rb = ctx.zeros(hi - lo, n_total), ctx.zeros(n_total, hi - lo), ctx.zeros(hi - lo, n_total)
    blocks = sharded_pearson_symmetric(engine, comm, z, bounds, r_row, r_col, recv, grouped=grouped)
    sharded_pearson_rowblock(engine, comm, z, bounds, r_rb, recv[:2])
    ctx.sync()
    row, col, rb = r_row.to_numpy(), r_col.to_numpy(), r_rb.to_numpy()
    reason = None
    for which, br, bc, nr, nc, gr, gc in blocks:
        if which == "row":
            got, want = row[br:br + nr, bc:bc + nc], rb[br:br + nr, gc:gc + nc]
            # same kernel, same operands in the same roles: the same bits, nothing less (a ticket that let a block read a
            # partly written shard could hide inside any tolerance)
            if not np.array_equal(got.view(np.uint32), want.view(np.uint32)):
                reason = "rank {}: block rows {}+{} x cols {}+{} differs from the row-block result (max |d| {:.3g})".format(
                    rank, gr, nr, gc, nc, float(np.nanmax(np.abs(got - want))))
                break
        else:  # the mirror of a block this rank multiplied: r_col[global rows of the peer, own local columns]
            got, want = col[br:br + nr, bc:bc + nc], row[bc:bc + nc, br:br + nr].T
            if not np.array_equal(got.view(np.uint32), np.ascontiguousarray(want).view(np.uint32)):
                reason = "rank {}: mirrored block rows {}+{} is not the transpose of the block it mirrors".format(rank, gr, nr)
                break
    if os.environ.get("SEEKR_TEST_HOOKS") == "1" and os.environ.get("SEEKR_BENCH_FAIL_SELFTEST") == str(rank):
        reason = "rank {}: failure injected by the test hook".format(rank)  # tests/test_gpu_multirank_mock.py
    bad = comm.allreduce([1.0 if reason else 0.0], "max")[0]
    for m in (r_row, r_col, r_rb, x, z, packed, *recv):
        m.free()
    if bad and not reason:
        reason = "rank {}: passed here, failed on another rank".format(rank)
    return reason


def column_chain_ab(ctx, comm, engine, x, n_cols, reps=5):
    """After the timed region (VERDICT r3 #3a): one column-sum pass over all ranks' rows, timed over send/recv and over
    the peer-mailbox chain (set up here, collectively; its own self-test decides whether it is used at all), the two
    results compared bit for bit.  Returns the dict that goes into the line as `chain_ab`."""
    from seekr_amd.distributed import _chain_colsum
    saved_env, saved_chain, saved_note = os.environ.get("SEEKR_CHAIN"), comm._chain, comm._chain_note
    out, vecs = {}, {}
    for name in ("rccl", "mailbox"):
        os.environ["SEEKR_CHAIN"] = name
        if comm._chain:
            comm._chain.free()
        comm._chain = None  # the transport is chosen (and the mailboxes set up) on the next pass, by every rank
        v = _chain_colsum(engine, comm, x, n_cols)  # set-up + warm-up
        ctx.sync()
        comm.barrier()
        t0 = time.perf_counter()
        for _ in range(reps):
            v.free()
            v = _chain_colsum(engine, comm, x, n_cols)
        ctx.sync()
        comm.barrier()
        ms = (time.perf_counter() - t0) / reps * 1e3
        gave_up = comm.allreduce([1.0 if comm.chain_gave_up() else 0.0], "max")[0] > 0
        out[name] = {"ms_per_pass": round(comm.allreduce([ms], "max")[0], 4), "transport": comm._chain_note or "send/recv",
                     "a_link_gave_up_waiting": bool(gave_up)}
        vecs[name] = v.vector().view(np.uint32).copy()
        v.free()
    same = np.array_equal(vecs["rccl"], vecs["mailbox"])
    out["bit_identical"] = bool(comm.allreduce([0.0 if same else 1.0], "max")[0] == 0)
    out["note"] = ("one float32 column-sum pass over all ranks' rows (a step has three), wall time between barriers, max over "
                   "ranks; the timed region above used SEEKR_CHAIN=" + (saved_env or "rccl"))
    if comm._chain:
        comm._chain.free()
    comm._chain, comm._chain_note = (None if saved_chain else saved_chain), saved_note
    if saved_env is None:
        os.environ.pop("SEEKR_CHAIN", None)
    else:
        os.environ["SEEKR_CHAIN"] = saved_env
    return out


def run_rank(args):
    from seekr_amd import _lib, launch as skr_launch
    from seekr_amd.distributed import (HipEngine, half_ring_plan, shard_bounds, sharded_normalize_prepare,
                                       sharded_pearson_allgather, sharded_pearson_rowblock, sharded_pearson_symmetric)
    from seekr_amd.synthetic import synthetic_ascii

    rank, size, _ = skr_launch.world()
    if size != args.gpus:
        raise SystemExit("--gpus {} but WORLD_SIZE={}".format(args.gpus, size))
    stage = ["start", time.monotonic()]

    def beat(name=None):
        """Progress: a new stage, or one more step of the current one."""
        if name is not None:
            stage[0] = name
        stage[1] = time.monotonic()

    watching = [size > 1]
    if size > 1:
        # a rank that makes no progress (a collective one peer never enters) must not hold the whole job until the caller's
        # own limit: --launch-timeout seconds WITHOUT A HEARTBEAT (a stage change or a finished step — not a cap on the run's
        # total time: ADVICE r4) and it says where it stood and leaves; torch.distributed.run (or this script's own
        # launcher) then ends the other ranks
        # (a THREAD, not SIGALRM: a Python signal handler only runs between bytecodes, and a stuck rank sits inside a
        # ctypes call — which releases the GIL, so the thread does get to run)
        import threading

        def watch():
            limit = max(1.0, float(args.launch_timeout))
            while watching[0]:
                quiet = time.monotonic() - stage[1]
                if quiet > limit:
                    print("bench.py rank {}: no progress for {:.0f} s, last stage: {}".format(rank, quiet, stage[0]),
                          file=sys.stderr, flush=True)
                    os._exit(3)
                time.sleep(min(1.0, limit / 4))
        threading.Thread(target=watch, daemon=True, name="bench-watchdog").start()
    beat("RCCL initialisation")
    ctx, comm = skr_launch.init()
    k, length = args.k, args.length
    generic = not (len(args.alphabet) == 4 and len(set(args.alphabet)) == 4)
    n_cols = len(args.alphabet) ** k
    n_total = args.rows or int(round(50_000 * math.sqrt(size) / size)) * size
    bounds = shard_bounds(n_total, size)
    lo, hi = bounds[rank], bounds[rank + 1]
    n_loc = hi - lo
    engine = HipEngine(ctx, _lib.PRECISIONS[args.precision], use_symmetry=not args.no_symmetry)
    symmetric_layout = args.layout == "symmetric" and args.precision != "fp32" and not args.no_symmetry

    beat("half-ring self-test")
    if size > 1 and symmetric_layout and not args.no_selftest:
        why = symmetric_selftest(ctx, comm, engine, k, args.grouped_shifts)
        if why:
            print("symmetric schedule self-test FAILED: " + why, file=sys.stderr, flush=True)
            sys.exit(SELFTEST_EXIT)

    # ---- synthetic input, packed and resident in HBM before the timed region
    blob, offsets = synthetic_ascii(SEED, n_loc, length, start=lo)
    if generic:
        # letters drawn uniformly from the alphabet given (the 4-letter generator has no N): resident ASCII, one byte per base
        letters = np.frombuffer(args.alphabet.encode("latin-1"), dtype=np.uint8)
        blob = letters[np.random.default_rng([SEED, lo]).integers(0, len(letters), size=blob.size)]
        packed = _lib.AsciiSeqs(ctx, blob, offsets)
    else:
        packed = _lib.PackedSeqs.from_buffer(ctx, blob, offsets, args.alphabet)
    del blob
    x = ctx.empty(n_loc, n_cols)
    z = engine.empty_operand(n_loc, n_cols)  # row-standardised shard in the contraction's operand layout
    r = ctx.zeros(n_loc, n_total)
    r_col = ctx.zeros(n_total, n_loc) if (symmetric_layout and size > 1) else None  # mirrored blocks (h, g)
    max_shard = max(bounds[g + 1] - bounds[g] for g in range(size))
    n_recv = max(2, size // 2) if args.grouped_shifts else 2
    use_allgather = args.layout == "allgather" and size > 1
    recv = [engine.empty_operand(max_shard, n_cols) for _ in range(n_recv)] if size > 1 and not use_allgather else [None, None]
    gathered = engine.empty_operand(n_total, n_cols) if use_allgather else None  # every rank's operand rows, kept between steps
    stats = []  # --dump-outputs: the column mean and std of the last step (released when the next step starts)

    def step():
        stats.clear()
        if generic:
            _lib.count_generic_dev(ctx, packed, args.alphabet, k, out=x)
        else:
            _lib.count_per_kb(ctx, packed, k, out=x)
        # column statistics (rank-chained), then ONE pass: normalised counts -> x, standardised rows -> z
        center, scale, _, zz = sharded_normalize_prepare(engine, comm, x, n_total, "Log2.post", True, True, keep_counts=True, op=z)
        if args.dump_outputs:
            stats.extend((center, scale))
        del center, scale
        if symmetric_layout:
            sharded_pearson_symmetric(engine, comm, zz, bounds, r, r_col, recv, grouped=args.grouped_shifts)
        elif use_allgather:
            sharded_pearson_allgather(engine, comm, zz, bounds, r, gathered)
        else:
            sharded_pearson_rowblock(engine, comm, zz, bounds, r, recv[:2])

    beat("warm-up steps")
    for _ in range(args.warmup):
        step()
        beat()
    ctx.sync()
    comm.barrier()
    beat("timed steps")
    ctx.prof_reset()
    ctx.prof_enable(True)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
        if size > 1:
            beat()  # (a store of two floats: nothing a step could notice)
    ctx.sync()
    comm.barrier()
    elapsed = time.perf_counter() - t0
    ctx.prof_enable(False)
    elapsed = comm.allreduce([elapsed], "max")[0]
    beat("after the timed region (per-rank statistics, verification)")
    if args.dump_outputs:  # before anything below reuses x or r (the f16f8 arm does)
        dump_outputs(args.dump_outputs, r, x, *stats)

    # ---- per-kernel device times of the timed region (HIP events on the ctx stream; comm_* on the communication stream)
    kern = exclusive_kernel_times(ctx)
    steps = args.steps
    per_rank = None
    n_ranks_seen = 1
    if size > 1:
        n_ranks_seen = int(round(comm.allreduce([1.0], "sum")[0]))

        def gather(value):  # every rank's value, by rank, through all-reduces of one-hot vectors (<= 16 values each)
            out = []
            for g0 in range(0, size, 16):
                vec = [0.0] * min(16, size - g0)
                if g0 <= rank < g0 + 16:
                    vec[rank - g0] = float(value)
                out += comm.allreduce(vec, "sum")
            return out

        def ms_step(name):
            return kern.get(name, {"ms_total": 0.0})["ms_total"] / steps

        gemm_names = [n for n in kern if n.startswith("pearson_gemm")]
        per_rank = {
            "comm_ms": [round(v, 3) for v in gather(ms_step("comm_xfer"))],
            "exposed_wait_ms": [round(v, 3) for v in gather(ms_step("comm_wait"))],
            "chain_wait_ms": [round(v, 3) for v in gather(ms_step("comm_wait_vec"))],
            "gemm_ms": [round(v, 3) for v in gather(sum(ms_step(n) for n in gemm_names))],
            "colsum_ms": [round(v, 3) for v in gather(sum(ms_step(n) for n in kern if n.startswith("colsum_seq")))],
            "column_sum_chain": getattr(comm, "_chain_note", "") or "send/recv",
            "note": "per step and rank: comm_ms = operand-shard transfers on the communication stream (data ready -> "
                    "arrived, the peer's lateness included); exposed_wait_ms = time the compute stream stood still waiting for a "
                    "shard (what no kernel hid); chain_wait_ms = the same for the rank-to-rank float32 column-sum chain "
                    "(serial by construction: rank g waits for ranks < g); with column_sum_chain = peer mailboxes that wait happens "
                    "inside the column-sum kernels (colsum_ms: rank g's kernels are resident and waiting while ranks < g walk)"}
    multi_verified = None
    if size > 1 and args.full:
        # correctness probe on EVERY rank, outside the timed region: 8 random rows of the rank's own diagonal block of the
        # r this run produced against the oracle on the rank's host copy of its normalised counts (the block needs no other
        # rank's rows; the cross blocks are covered by the schedule's self-test and the mirror checks); verdict all-reduced
        from oracle import seekr_oracle as orc
        worst = 0.0
        if n_loc > 0:
            x_loc = x.to_numpy()
            pick = np.sort(np.random.default_rng(rank + 1).choice(n_loc, min(8, n_loc), replace=False))
            got = np.stack([r.to_numpy(int(i), 1).reshape(-1)[lo:hi] for i in pick])
            try:  # every rank checks at once: share the host's cores instead of each BLAS taking all of them
                from threadpoolctl import threadpool_limits
                limit = threadpool_limits(limits=max(1, (os.cpu_count() or size) // size))
            except Exception:  # noqa: BLE001
                limit = None
            want = orc.pearson(x_loc[pick], x_loc)
            if limit is not None:
                limit.restore_original_limits()
            worst = float(np.max(np.abs(got - want) / (2e-6 + 1e-5 * np.abs(want))))
            worst = worst if np.isfinite(worst) else 1e9
            del x_loc
        multi_verified = comm.allreduce([worst], "max")[0]
    chain_ab = None
    if size > 1 and args.full and os.environ.get("SEEKR_BENCH_CHAIN_AB") == "1":
        beat("chain A/B (opt-in)")
        try:
            chain_ab = column_chain_ab(ctx, comm, engine, x, n_cols)
        except Exception as e:  # noqa: BLE001 - the line measured above is worth more than this extra
            chain_ab = {"error": "{}: {}".format(type(e).__name__, e)}
    gemm_name = {"fp32": "pearson_gemm_f32", "bf16x3": "pearson_gemm_bf16x3",
                 "f16x3": "pearson_gemm_f16x3", "f16f8": "pearson_gemm_f16f8"}[args.precision]
    gemm = kern.get(gemm_name, {"ms_total": 0.0, "launches": 0})
    count = kern.get("count_generic" if generic else "count_kmers_f32", {"ms_total": 0.0, "launches": 0})

    watching[0] = False
    if rank != 0:
        return
    pairs_per_step = float(n_total) * n_total
    value = pairs_per_step * steps / elapsed / 1e6
    # Dominant kernel: the Pearson contraction (MFMA bound), 2*4^k algorithmic flop per pair it
    # actually multiplies.  The self block mirrors one triangle on the bf16 path, so the pairs it
    # multiplies are ~half of the pairs it delivers; both figures are reported.
    sym = not args.no_symmetry  # the fp32 kernel mirrors its own block too (128-row tiles)
    tile = 128 if args.precision == "fp32" else 256
    exec_pairs = n_loc * (n_loc + tile) / 2.0 if sym else float(n_loc) * n_loc
    if symmetric_layout:
        exec_pairs += sum(float(an) * bn for _, _, _, an, _, bn in half_ring_plan(size, rank, bounds))
    else:
        exec_pairs += float(n_loc) * (n_total - n_loc)
    gemm_ms_step = gemm["ms_total"] / steps
    gemm_avg_ms = gemm["ms_total"] / max(gemm["launches"], 1)
    # 2*4^k flop per ORDERED pair delivered (what np.inner spends on it); the symmetric
    # kernel multiplies only ~half of them, so the flops it really issues are reported next to it
    delivered_pairs = float(n_loc) * n_total
    achieved_tf = 2.0 * n_cols * delivered_pairs / (gemm_ms_step * 1e-3) / 1e12 if gemm_ms_step > 0 else 0.0
    multiplied_tf = 2.0 * n_cols * exec_pairs / (gemm_ms_step * 1e-3) / 1e12 if gemm_ms_step > 0 else 0.0
    nprod = {"fp32": 1, "bf16x3": 3, "f16x3": 3, "f16f8": 2}[args.precision]
    peak_tf = PEAK["fp32_mfma_tflops"] if args.precision == "fp32" else PEAK["bf16_mfma_tflops"]
    # PMC traffic: from the committed summary of this very workload, taken with this library's kernel set — else null
    gemm_key = {"fp32": "pearson_gemm_f32_kernel", "bf16x3": "split16_kernelIDF16bLi3",
                "f16x3": "split16_kernelIDF16_Li3", "f16f8": "split16_kernelIDF16_Li2"}[args.precision]
    wl = workload_key(n_total, length, k, args.precision, size) + (" alphabet=" + args.alphabet if generic else "")
    gemm_traffic, gemm_why = (None, "--no-symmetry") if args.no_symmetry else pmc_traffic(gemm_key, wl, _lib.LIB_PATH)
    if gemm_traffic and args.precision != "fp32" and n_cols > 4096:
        # rows of more than 4 096 columns: one launch = one kernel dispatch per 4 096-column k chunk; the summary holds
        # per-dispatch averages
        chunks = -(-n_cols // 4096)
        gemm_traffic = dict(gemm_traffic, bytes=gemm_traffic["bytes"] * chunks, fetch_bytes_corrected=gemm_traffic["fetch_bytes_corrected"] * chunks,
                            write_bytes=gemm_traffic["write_bytes"] * chunks, dispatches_per_launch=chunks)
    count_traffic, count_why = pmc_traffic("count_generic_lds_kernel<float, false>" if generic else "count_rows_kernel<0", wl,
                                           _lib.LIB_PATH)  # <0, ...>: the float32, non-Log2.pre instantiation
    roofline = {"kernel": gemm_name, "bound": "mfma", "achieved": round(achieved_tf, 2), "peak": peak_tf,
                "unit": "TFLOP/s", "frac": round(achieved_tf / peak_tf, 4),
                "traffic": round(gemm_traffic["bytes"] / 1e9, 2) if gemm_traffic else None,
                "traffic_unit": "GB per launch (HBM-side: 2 x FETCH_SIZE + WRITE_SIZE, separate rocprofv3 --pmc passes)",
                "traffic_detail": gemm_traffic if gemm_traffic else {"unavailable": gemm_why},
                "algorithmic_bytes_gb": round((2.0 * n_loc * n_cols * 4 + 4.0 * n_loc * n_total) / 1e9, 2),
                "avg_launch_ms": round(gemm_avg_ms, 4), "launches_per_step": gemm["launches"] // max(steps, 1),
                "multiplied_tflops": round(multiplied_tf, 2), "multiplied_frac": round(multiplied_tf / peak_tf, 4),
                "mfma_executed_tflops": round(multiplied_tf * nprod, 2),
                "mfma_executed_frac": round(multiplied_tf * nprod / peak_tf, 4),
                "pairs_multiplied_per_step": exec_pairs, "pairs_delivered_per_step": delivered_pairs,
                "note": "achieved = 2*4^k flop x ordered pairs delivered / kernel time (SURVEY 8d; HIP events, summed "
                        "over the step's launches). r(j,i) = r(i,j): the kernel multiplies {:.3g} of the {:.3g} pairs it "
                        "delivers (multiplied_*), and the split path issues {} 16-bit MFMA products per multiplication "
                        "(mfma_executed_* = what the matrix cores really run, against the same dense peak)".format(
                            exec_pairs, delivered_pairs, nprod)}
    # Which roof bounds this kernel at this width: at k <= 4 the float32 r it writes (4 B per pair) takes longer at 8 TB/s
    # than 2*4^k flop per pair take on the matrix cores — the contraction is then an HBM-bound kernel and is priced as one
    alg_bytes = 2.0 * n_loc * n_cols * 4 + 4.0 * n_loc * n_total
    alg_flop = 2.0 * n_cols * delivered_pairs
    if alg_bytes / (PEAK["hbm_gbs"] * 1e9) > alg_flop / (peak_tf * 1e12) and gemm_ms_step > 0:
        gbs = alg_bytes / (gemm_ms_step * 1e-3) / 1e9
        roofline.update({"bound": "hbm", "achieved": round(gbs, 1), "peak": PEAK["hbm_gbs"], "unit": "GB/s",
                         "frac": round(gbs / PEAK["hbm_gbs"], 4),
                         "mfma_view": {"achieved_tflops": round(achieved_tf, 2), "peak_tflops": peak_tf, "frac": round(achieved_tf / peak_tf, 4)},
                         "bound_note": "output bound at this width: {:.2f} ms of r and operands at 8 TB/s against {:.2f} ms of "
                                       "matrix work at the dense peak".format(alg_bytes / (PEAK["hbm_gbs"] * 1e9) * 1e3, alg_flop / (peak_tf * 1e12) * 1e3)})
    # counting kernel: HBM bound, 0.25 B/base packed in (1 B/base ASCII for the any-alphabet kernel: SURVEY 8d) + 4 A^k B per
    # sequence out
    count_avg_ms = count["ms_total"] / max(count["launches"], 1)
    count_bytes = n_loc * (length * (1.0 if generic else 0.25) + 8 + 4.0 * n_cols)
    count_gbs = count_bytes / (count_avg_ms * 1e-3) / 1e9 if count_avg_ms > 0 else 0.0
    mbases = n_loc * length / (count_avg_ms * 1e-3) / 1e6 if count_avg_ms > 0 else 0.0
    roofline_count = {"kernel": "count_generic (ASCII in, any alphabet)" if generic else "count_kmers_f32", "bound": "hbm", "achieved": round(count_gbs, 1),
                      "peak": PEAK["hbm_gbs"], "unit": "GB/s", "frac": round(count_gbs / PEAK["hbm_gbs"], 4),
                      "traffic": round(count_traffic["bytes"] / 1e9, 3) if count_traffic else None,
                      "traffic_unit": "GB per launch", "traffic_detail": count_traffic if count_traffic else {"unavailable": count_why},
                      "algorithmic_bytes_gb": round(count_bytes / 1e9, 3), "avg_launch_ms": round(count_avg_ms, 4),
                      "bytes_per_base": round(count_bytes / (n_loc * length), 3)}
    out = {
        "metric": "Mbases/s k-mer counted + M seq-pairs/s Pearson, k=6, 1/2/4/8 GPU",
        "value": round(value, 2),
        "unit": "M seq-pairs/s (whole step: count + normalise + Pearson)",
        "n_gpus": size, "steps": steps, "warmup": args.warmup,
        "ms_per_step": round(elapsed / steps * 1e3, 3),
        # --rows given: the transcript set is fixed whatever N (strong scaling: config 4 is `--gpus 8 --rows 200000`);
        # default: 50 000 x sqrt(N) rows, i.e. a fixed number of ordered pairs per GPU (weak)
        "higher_is_better": True, "scaling": "strong" if args.rows else "weak", "vs_baseline": None,
        "dtype": ("f32" if args.precision == "fp32" else
                  "f32 as 1 fp16 (hi x hi) + 1 block-scaled fp8 (both cross terms) MFMA product, f32 accumulate" if args.precision == "f16f8"
                  else "f32 as {} split-{} MFMA products, f32 accumulate".format(nprod, "fp16" if args.precision == "f16x3" else "bf16")),
        "data": "synthetic",
        "config": {"workload": "{} synthetic {} nt transcripts, k={}, counts + Log2.post normalisation + "
                               "self Pearson ({} x {} r matrix, row-sharded)".format(n_total, length, k, n_total, n_total),
                   "rows_total": n_total, "rows_per_gpu": n_loc, "length": length, "k": k, "alphabet": args.alphabet,
                   "columns": n_cols,
                   "precision": args.precision, "sharding": "rows x{}".format(size),
                   "layout": ("symmetric half-ring: each ordered pair on one GPU" if symmetric_layout else
                              "row blocks after one all-gather of the operands" if use_allgather else "row blocks")},
        "mbases_per_s_counted": round(mbases * size, 1),
        "pearson_kernel_mpairs_per_s": round(pairs_per_step / (gemm_ms_step * 1e-3) / 1e6, 1) if gemm_ms_step > 0 else None,
        "roofline": roofline, "roofline_count": roofline_count,
        "kernels_ms_per_step": {n: round(v["ms_total"] / steps, 4) for n, v in sorted(kern.items())},
    }
    if size > 1:
        out["n_ranks_seen"] = n_ranks_seen
        out["per_rank"] = per_rank
        if chain_ab is not None:
            out["chain_ab"] = chain_ab
        out["selftest"] = ("skipped" if args.no_selftest or not symmetric_layout
                           else "half-ring schedule == row-block schedule on a small set, on every rank")
    if multi_verified is not None:
        out["verified"] = bool(multi_verified <= 1.0)
        out["verified_detail"] = {"rows": "8 per rank", "columns": "the rank's own diagonal block", "worst_error_over_bar": round(multi_verified, 4),
                                  "bar": "|dr| <= 2e-6 + 1e-5 |r| against oracle.pearson (pearson.py:35-41) on every rank, all-reduced"}
    if os.environ.get("SEEKR_BENCH_FALLBACK"):
        out["layout_fallback"] = os.environ["SEEKR_BENCH_FALLBACK"]
    # the extras below run with --full only (a plain run prints the line as it stands)
    if size == 1 and args.full:
        # correctness probe of the r this run produced, outside the timed region: 32 random rows x all columns
        # against the oracle on the host copy of the normalised counts (x holds them: keep_counts=True)
        x_host = x.to_numpy()
        ok, worst = verify_rows(ctx, r, x_host)
        out["verified"] = bool(ok)
        out["verified_detail"] = {"rows": min(32, n_loc), "columns": n_total, "worst_error_over_bar": round(worst, 4),
                                  "bar": "|dr| <= 2e-6 + 1e-5 |r| against oracle.pearson (pearson.py:35-41)"}
    if size == 1 and args.full and args.precision == "f16x3" and not generic and k in (6, 7) and not args.no_symmetry and not args.no_f16f8_arm:
        # The opt-in two-product-unit contraction (SKR_PREC_F16F8), measured in the same run AFTER the timed
        # region and never part of `value`: the same step with the other operand layout, the same number of steps,
        # the same verification against the oracle.
        engine8 = HipEngine(ctx, _lib.PRECISIONS["f16f8"])
        z8 = engine8.empty_operand(n_loc, n_cols)

        def step8():
            _lib.count_per_kb(ctx, packed, k, out=x)
            zz = sharded_normalize_prepare(engine8, comm, x, n_total, "Log2.post", True, True, keep_counts=True, op=z8)[3]
            sharded_pearson_symmetric(engine8, comm, zz, bounds, r, None, [None, None])
            return zz

        steps8 = max(10, steps)  # its own warm-up and step count: the GPU has idled through the verification above
        for _ in range(max(3, args.warmup)):
            zz8 = step8()
        ctx.sync()
        ctx.prof_reset()
        ctx.prof_enable(True)
        t8 = time.perf_counter()
        for _ in range(steps8):
            zz8 = step8()
        ctx.sync()
        t8 = time.perf_counter() - t8
        ctx.prof_enable(False)
        kern8 = exclusive_kernel_times(ctx)
        ok8, worst8 = verify_rows(ctx, r, x.to_numpy())
        g8 = kern8.get("pearson_gemm_f16f8", {"ms_total": 0.0})["ms_total"] / steps8
        out["f16f8_arm"] = {
            "value": round(pairs_per_step * steps8 / t8 / 1e6, 2), "unit": out["unit"], "ms_per_step": round(t8 / steps8 * 1e3, 3),
            "steps": steps8,
            "pearson_kernel_ms": round(g8, 4), "operand_kind": zz8.kind,
            "roofline_frac": round(2.0 * n_cols * float(n_loc) * n_total / (g8 * 1e-3) / 1e12 / peak_tf, 4) if g8 > 0 else None,
            "verified": bool(ok8), "worst_error_over_bar": round(worst8, 4),
            "note": "opt-in SEEKR_PRECISION=f16f8: hi x hi on the fp16 MFMA + both cross terms as one block-scaled fp8 MFMA (2 "
                    "product-units per k instead of 3); measured after the timed region, never part of `value`; operand_kind 3 = "
                    "the fp8 cross layout was kept, 2 = the fill routed these rows back to the three-product split"}
        z8.free()
    if size == 1 and args.full and not args.no_cpu_baseline and not generic:
        head = x_host[:min(12000 if k <= 6 else 4000, n_loc)]
        cb = cpu_baseline(k, length, head)
        t_cpu = n_total * length / cb["rate_bases"] + pairs_per_step / cb["rate_pairs"]
        out["cpu_baseline"] = {
            "value": round(pairs_per_step / t_cpu / 1e6, 3), "unit": "M seq-pairs/s (whole step, extrapolated)",
            "cores": cb["blas_threads"], "kind": "port",
            "sample": "median of {} repeats each: oracle (pure-Python per-window counting, 1 core) on the first {} "
                      "sequences: {:.2f} s = {:.3f} Mbases/s; oracle numpy Pearson ({} BLAS threads of {} cores) on the "
                      "first {} rows: {:.2f} s = {:.2f} M pairs/s; T_cpu(N) = bases/rate_count + N^2/rate_pairs".format(
                          cb["repeats"], cb["n_count"], cb["t_count"], cb["rate_bases"] / 1e6, cb["blas_threads"],
                          os.cpu_count(), cb["n_pearson"], cb["t_pearson"], cb["rate_pairs"] / 1e6),
            "count_mbases_per_s": round(cb["rate_bases"] / 1e6, 4),
            "pearson_mpairs_per_s": round(cb["rate_pairs"] / 1e6, 3),
        }
        out["speedup_vs_cpu_port"] = round(value / out["cpu_baseline"]["value"], 1)
        del x_host, head
        r.free()
        if k == 6 and length == 2000 and n_total == 50000 and args.precision == "f16x3" and not args.no_target_200k:
            for m in (x, z, packed):
                m.free()
            # a sub-record must never cost the measured line: 167 GB of r + counts + operands — skipped with a
            # note on a GPU that does not have them free (a smaller part, another tenant), any failure recorded, not raised
            free_gb = ctx.mem_info()[0] / 1e9
            if free_gb < 175:
                out["target_200k"] = {"skipped": "needs ~170 GB of device memory, {:.0f} GB free".format(free_gb)}
            else:
                try:
                    out["target_200k"] = target_200k(ctx, comm, engine, cb, peak_tf)
                except Exception as e:  # noqa: BLE001
                    out["target_200k"] = {"error": "{}: {}".format(type(e).__name__, str(e)[:300])}
        try:
            out["e2e"] = end_to_end(ctx, k, length, min(n_total, 50000 if k <= 6 else 12000), args.precision)
        except Exception as e:  # noqa: BLE001
            out["e2e"] = {"error": "{}: {}".format(type(e).__name__, str(e)[:300])}
    print(json.dumps(out), flush=True)


def main():
    argv = sys.argv[1:]
    args = parse(argv)
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        sys.exit(launch(args, argv))
    run_rank(args)


if __name__ == "__main__":
    main()
