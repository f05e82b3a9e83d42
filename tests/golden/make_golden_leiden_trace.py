"""Writes tests/golden/leiden_trace.json: the sequential model of skr_leiden (tests/leiden_model.py) on every trace case of
tests/leiden_cases.py under every function it runs at — the graph's hash, levels, sweeps, converged, the community count,
the membership (its hash; itself up to 2 500 nodes) and the whole record list, one record per proposal pass, refinement
round and sweep.  For every run both injected faults must change a proposal record of the work unit and level the case
is there for (leiden_cases.TRACE_ROUTES); the index of the first such record is stored.  A case that fails this gets other
parameters; the condition is not relaxed.  The two large cases take a few minutes.  Run from the repository root:
    python tests/golden/make_golden_leiden_trace.py"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import leiden_cases as lc  # noqa: E402
import leiden_model as lm  # noqa: E402

MEMBERSHIP_NODES = 2500
FAULTS = ("drop_last", "lose_key")


def run_key(algo, rs):
    return "{}@{:g}".format(algo, rs)


def pin_run(graph, name, algo, rs):
    """The pinned entry of one case x function, with the fitness conditions asserted."""
    limit, route, level = lc.TRACE_ROUTES[name]
    rows, cols, vals, n = graph
    mem, info, trace = lm.model(rows, cols, vals, n, algo, rs)
    reached = lm.route_records(trace, route, level)
    assert {trace[k][0] for k in reached} == {lm.PROPOSE, lm.REFINE}, (name, algo, "the work unit is not reached in both phases")
    faults = {}
    for fault in FAULTS:
        spoilt = lm.model(rows, cols, vals, n, algo, rs, fault=(fault, limit))[2]
        faults[fault] = lm.first_fault_record(trace, spoilt, route, level)
        assert faults[fault] is not None, (name, algo, fault, "the case cannot see this fault")
    entry = dict(info, membership_hash=lm.fnv1a(mem.astype("<i4")), records=[list(r) for r in trace], first_fault_record=faults)
    if n <= MEMBERSHIP_NODES:
        entry["membership"] = mem.tolist()
    return entry


def dumps(out):
    """json with one record (and one membership) to a line."""
    def flat(x):
        if isinstance(x, dict):
            return {k: flat(v) for k, v in x.items()}
        if isinstance(x, list) and x and isinstance(x[0], list):
            return ["@@" + json.dumps(r, separators=(",", ":")) + "@@" for r in x]
        if isinstance(x, list):
            return "@@" + json.dumps(x, separators=(",", ":")) + "@@"
        return x
    return json.dumps(flat(out), indent=1, sort_keys=True).replace('"@@', "").replace('@@"', "") + "\n"


def main(names=None):
    out = {}
    for name in names or lc.TRACE_CASES:
        graph = lc.TRACE_CASES[name]()
        entry = {"graph_hash": lm.graph_hash(graph), "nodes": graph[3], "edges": int(len(graph[0])), "runs": {}}
        for algo, rs in lc.TRACE_RUNS[name]:
            entry["runs"][run_key(algo, rs)] = run = pin_run(graph, name, algo, rs)
            print(name, run_key(algo, rs), {k: v for k, v in run.items() if k not in ("records", "membership")}, "records", len(run["records"]),
                  flush=True)
        out[name] = entry
    return out


if __name__ == "__main__":
    with open(os.path.join(HERE, "leiden_trace.json"), "w") as f:
        f.write(dumps(main()))
