"""Writes tests/golden/leiden_cases.json: for each quality case of tests/leiden_cases.py and each (algo, resolution) it
runs at, the sequential Louvain yardstick under 16 visiting orders — minimum and maximum quality and the community
counts.  Where networkx imports, its louvain_communities' modularity over 16 seeds is recorded beside the
configuration-model runs at resolution 1 (never used as a bound).  Run from the repository root:
    python tests/golden/make_golden_leiden.py"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import leiden_cases as lc  # noqa: E402

ORDERS = 16


def yardstick(graph, algo, rs, orders=ORDERS):
    rows, cols, vals, n = graph
    qs, counts = [], []
    for seed in range(orders):
        mem = lc.louvain(rows, cols, vals, n, algo, rs, seed=seed)
        qs.append(lc.quality(rows, cols, vals, n, mem, algo, rs))
        counts.append(int(mem.max()) + 1)
    return {"min": min(qs), "max": max(qs), "communities": sorted(set(counts))}


def networkx_modularity(graph, orders=ORDERS):
    try:
        import networkx as nx
    except ImportError:
        return None
    rows, cols, vals, n = graph
    g = nx.Graph()
    g.add_nodes_from(range(n))
    g.add_weighted_edges_from(zip(rows.tolist(), cols.tolist(), vals.astype(np.float64).tolist()))
    qs = [nx.community.modularity(g, nx.community.louvain_communities(g, weight="weight", seed=s), weight="weight") for s in range(orders)]
    return {"min": min(qs), "max": max(qs)}


def main():
    out = {}
    for name, make in lc.QUALITY_CASES.items():
        graph = make()
        entry = {"nodes": graph[3], "edges": int(len(graph[0])), "runs": {}}
        for algo, rs in lc.QUALITY_RUNS:
            entry["runs"]["{}@{:g}".format(algo, rs)] = yardstick(graph, algo, rs)
        nxq = networkx_modularity(graph)
        if nxq is not None:
            entry["networkx_modularity"] = nxq
        out[name] = entry
        print(name, json.dumps(entry))
    with open(os.path.join(HERE, "leiden_cases.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
