"""Leiden communities on the device at the sizes the edge list is built for.  One process, one GPU.

    python tools/leiden_bench.py [--sparse-rows 100000] [--dense-rows 20000] [--density 1e-3] [--nx-nodes 20000] [--out profiles/leiden_bench.json]

  sparse   --sparse-rows synthetic transcripts of 2 000 bases, k = 6, at the cutoff that keeps --density of the pairs
           (distribution.density_cutoff: exact over all pairs; profiles/leiden_bench.json was made when this was the
           1 - density quantile of a 2 048 x 2 048 block of r)
  dense    --dense-rows transcripts at cutoff 0, the reference's default, which keeps about half of all cells
For each: seconds for the edge list (consumers.pearson_edges) and for seekr_amd.leiden.communities, the device time of each
phase (the library's event timers: sort = CSR build, move, refine, aggregate, number = numbering and the float64 quality),
levels, sweeps, communities and the quality (RBERVertexPartition, resolution 1).  Where networkx imports, its
louvain_communities runs on the sub-graph of the first --nx-nodes nodes of the sparse case, beside the device on the same
sub-graph: seconds and modularity of both."""
import argparse
import json
import os
import socket
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
from seekr_amd import _lib, consumers, distribution, leiden  # noqa: E402
from seekr_amd import pearson as pearson_mod  # noqa: E402
from seekr_amd.synthetic import synthetic_ascii  # noqa: E402

PHASES = ("leiden_sort", "leiden_move", "leiden_refine", "leiden_aggregate", "leiden_number")


def operand(ctx, n, length=2000, k=6):
    blob, offsets = synthetic_ascii(1, n, length)
    x = _lib.count_per_kb(ctx, _lib.PackedSeqs.from_buffer(ctx, blob, offsets), k)
    _lib.normalize(ctx, x, "Log2.post", 1, None, 1, None)
    z, _ = _lib.operand_fill(ctx, x, None, pearson_mod._precision_for(np.dtype(np.float32), True))
    x.free()
    return z


def cutoff_for(ctx, z, density):
    return float(distribution.density_cutoff(z, density))


def timed_communities(ctx, rows, cols, vals, n, algo="RBERVertexPartition"):
    leiden.communities(rows[:2], cols[:2], vals[:2], n, algo=algo)  # warm-up: loads the kernels
    ctx.prof_reset()
    ctx.prof_enable(True)
    t0 = time.perf_counter()
    mem, q, info = leiden.communities(rows, cols, vals, n, algo=algo)
    wall = time.perf_counter() - t0
    ctx.prof_enable(False)
    out = {"communities_s": round(wall, 4), "quality": q, "algo": algo}
    out.update(info)
    for name in PHASES:
        out[name.replace("leiden_", "") + "_ms"] = round(ctx.prof_query(name)[0], 3)
    return mem, out


def case(ctx, n, cutoff=None, density=None):
    z = operand(ctx, n)
    if cutoff is None:
        cutoff = cutoff_for(ctx, z, density)
    t0 = time.perf_counter()
    rows, cols, vals = consumers.pearson_edges(z, cutoff, upper_only=True)
    edges_s = time.perf_counter() - t0
    z.free()
    keep = vals > 0
    rows, cols, vals = rows[keep].astype(np.uint32), cols[keep].astype(np.uint32), vals[keep].astype(np.float32)
    res = {"rows": n, "cutoff": cutoff, "edges": int(len(vals)), "edges_per_cell": len(vals) / (n * (n - 1) / 2), "pearson_edges_s": round(edges_s, 4)}
    print(json.dumps(res), flush=True)
    _, out = timed_communities(ctx, rows, cols, vals, n)
    res.update(out)
    print(json.dumps(res), flush=True)
    return res, (rows, cols, vals)


def against_networkx(ctx, graph, nodes):
    try:
        import networkx as nx
    except ImportError:
        return None
    rows, cols, vals = graph
    keep = (rows < nodes) & (cols < nodes)
    rows, cols, vals = rows[keep], cols[keep], vals[keep]
    _, dev = timed_communities(ctx, rows, cols, vals, nodes, algo="ModularityVertexPartition")
    g = nx.Graph()
    g.add_nodes_from(range(nodes))
    g.add_weighted_edges_from(zip(rows.tolist(), cols.tolist(), vals.astype(np.float64).tolist()))
    t0 = time.perf_counter()
    parts = nx.community.louvain_communities(g, weight="weight", seed=0)
    nx_s = time.perf_counter() - t0
    return {"nodes": nodes, "edges": int(len(vals)), "device": dev, "networkx_louvain_s": round(nx_s, 3),
            "networkx_modularity": nx.community.modularity(g, parts, weight="weight"), "networkx_communities": len(parts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sparse-rows", type=int, default=100000)
    ap.add_argument("--dense-rows", type=int, default=20000)
    ap.add_argument("--density", type=float, default=1e-3)
    ap.add_argument("--nx-nodes", type=int, default=20000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ctx = _lib.default_context()
    res = {"box": socket.gethostname(), "limits": leiden.limits()}
    if args.sparse_rows:
        res["sparse"], graph = case(ctx, args.sparse_rows, density=args.density)
        if args.nx_nodes:
            res["networkx"] = against_networkx(ctx, graph, min(args.nx_nodes, args.sparse_rows))
            print(json.dumps(res["networkx"]), flush=True)
        del graph
    if args.dense_rows:
        res["dense"], _ = case(ctx, args.dense_rows, cutoff=0.0)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
