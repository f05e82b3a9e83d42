"""skr_leiden against its sequential model, pass by pass.  tests/golden/leiden_trace.json pins what tests/leiden_model.py
computes for every trace case of tests/leiden_cases.py: levels, sweeps, the membership and one record per proposal pass,
refinement round and sweep (hashes of the proposals of all nodes, the bits of the sweep's quality).  The device must give
the same, record for record, with no tolerance: every sum that decides a move is an integer sum and every gain one
float64 expression.  The cases put nodes with tables that accumulate on the one-workgroup and the device-memory work
units, at level 0 and on aggregates, in local moving and in refinement.  Nothing here runs the model while the device
agrees with the pins; on a mismatch the model is run once, to name the first node that differs."""
import functools
import json
import os
import time

import numpy as np
import pytest

import leiden_cases as lc
import leiden_model as lm
from test_gpu_leiden import check_result

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUNS = [(name, algo, rs) for name in lc.TRACE_CASES for algo, rs in lc.TRACE_RUNS[name]]


def run_key(algo, rs):
    return "{}@{:g}".format(algo, rs)


@functools.lru_cache(maxsize=None)
def pinned():
    with open(os.path.join(ROOT, "tests", "golden", "leiden_trace.json")) as f:
        return json.load(f)


@functools.lru_cache(maxsize=2)
def trace_graph(name):
    return lc.TRACE_CASES[name]()


def record_time(key, entry):
    path = os.path.join(ROOT, "profiles", "leiden_trace_gpu.json")
    try:
        with open(path) as f:
            table = json.load(f)
    except (OSError, ValueError):
        table = {}
    table.setdefault("tests", {})[key] = entry
    try:
        with open(path, "w") as f:
            json.dump(table, f, indent=1, sort_keys=True)
            f.write("\n")
    except OSError:
        pass


def describe(rec):
    kind = lm.KIND_NAMES.get(rec[0], rec[0])
    if rec[0] == lm.SWEEP:
        return "{} level {} tries {} moves {} quality bits {:#x} labels {} kept {}".format(kind, *rec[1:7])
    return "{} level {} nodes {} n_blk {} n_glb {}".format(kind, *rec[1:5])


def first_difference(records, want):
    for k, (a, b) in enumerate(zip(records, want)):
        if a != b:
            return k
    return min(len(records), len(want)) if len(records) != len(want) else None


def explain(graph, algo, rs, k, records, want):
    """The text of a mismatch at record k: both records and, for a proposal record, the first node whose proposal differs
    with its degree and work unit (the device's arrays by trace_dump, the model's by a run of the model)."""
    from seekr_amd.leiden import communities
    rows, cols, vals, n = graph
    lines = ["record {} differs".format(k), "  device: " + (describe(records[k]) if k < len(records) else "(none)") + "  " + repr(records[k] if k < len(records) else None),
             "  pinned: " + (describe(want[k]) if k < len(want) else "(none)") + "  " + repr(want[k] if k < len(want) else None)]
    if k < len(records) and k < len(want) and records[k][0] == want[k][0] != lm.SWEEP and records[k][:5] == want[k][:5]:
        got = communities(rows, cols, vals, n, algo=algo, rs=rs, trace_dump=k)[2]["trace_arrays"]
        ref = lm.model(rows, cols, vals, n, algo, rs, keep=k)[1].get("trace_arrays")
        level = records[k][1]
        for which, (a, b) in enumerate(zip(got, ref or ())):
            v = lm.first_differing_node(a, b)
            name = "prop" if which == 0 else ("gain" if records[k][0] == lm.PROPOSE else "target")
            if v is not None and v >= 0:
                lines.append("  {}: first differing node {} of level {}: device {!r} model {!r}".format(name, v, level, a[v], b[v]))
                if level == 0:
                    deg = int(np.bincount(np.concatenate([rows, cols]), minlength=n)[v])
                    unit = "one wave" if deg <= lm.WAVE_DEG else ("one workgroup, LDS table" if deg <= lm.LDS_DEG else "device-memory table")
                    lines.append("    degree {} ({})".format(deg, unit))
                else:
                    lines.append("    (an aggregate: its entries are those of the model's level {})".format(level))
    return "\n".join(lines)


def compare(graph, algo, rs, records, want):
    """None, or the text of the first mismatch between the device's records and the pinned ones."""
    k = first_difference(records, want)
    return None if k is None else explain(graph, algo, rs, k, records, want)


def merge_gain_max(graph, mem, algo, rs):
    """The largest gain of merging two communities joined by an edge, in float64 from the input graph alone: w_cd less
    gamma K_c K_d / 2m (configuration model), gamma p n_c n_d (RBER) or gamma n_c n_d (CPM)."""
    rows, cols, vals, n = graph
    q = lc.ALGOS[algo]
    w = vals.astype(np.float64)
    m = w.sum()
    mem = mem.astype(np.int64)
    nc = int(mem.max()) + 1
    a, b = mem[rows.astype(np.int64)], mem[cols.astype(np.int64)]
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    between = np.bincount((lo * nc + hi)[lo != hi], w[lo != hi], nc * nc)
    pairs = np.flatnonzero(between)
    if not len(pairs):
        return -np.inf, m
    c, d = pairs // nc, pairs % nc
    if q <= 1:
        deg = np.bincount(rows, w, n) + np.bincount(cols, w, n)
        size = np.bincount(mem, deg, nc)
        scale = (1.0 if q == 1 else rs) / (2.0 * m)
    else:
        size = np.bincount(mem, minlength=nc).astype(np.float64)
        scale = rs * m / (n * (n - 1) / 2.0) if q == 2 else rs
    return float((between[pairs] - scale * size[c] * size[d]).max()), m


@pytest.mark.parametrize("name,algo,rs", RUNS, ids=["{}-{}".format(n, run_key(a, r)) for n, a, r in RUNS])
def test_trace_equals_the_pins(name, algo, rs):
    from seekr_amd.leiden import communities, table_groups
    t0 = time.perf_counter()
    pin = pinned()[name]
    graph = trace_graph(name)
    rows, cols, vals, n = graph
    assert pin["graph_hash"] == lm.graph_hash(graph), "the case changed: regenerate tests/golden/leiden_trace.json"
    run = pin["runs"][run_key(algo, rs)]
    want = [tuple(r) for r in run["records"]]
    # the end checks of every Leiden test, with the trace off (two runs)
    mem_off, q_off, info_off = check_result(graph, algo, rs)
    t1 = time.perf_counter()
    mem_off2, _, _ = communities(rows, cols, vals, n, algo=algo, rs=rs)
    t2 = time.perf_counter()
    mem, q, info = communities(rows, cols, vals, n, algo=algo, rs=rs, trace=True)
    t3 = time.perf_counter()
    records = info.pop("trace")
    # the trace changes nothing
    assert mem.tobytes() == mem_off.tobytes() == mem_off2.tobytes() and q == q_off and info == info_off
    # record for record
    report = compare(graph, algo, rs, records, want)
    assert report is None, report
    for key in ("levels", "sweeps", "converged", "n_communities"):
        assert info[key] == run[key], key
    assert lm.fnv1a(mem.astype("<i4")) == run["membership_hash"]
    if "membership" in run:
        assert mem.tolist() == run["membership"]
    # the work unit the case is there for, by the device's own counts
    _, route, level = lc.TRACE_ROUTES[name]
    reached = lm.route_records(records, route, level)
    assert {records[k][0] for k in reached} == {lm.PROPOSE, lm.REFINE}
    if name == "many_hubs":
        assert records[0][4] > table_groups(), "no workgroup of the device-memory unit takes a second node"
    # a converged run ends with every community a node of the last level and no node proposing: no merge of two
    # communities joined by an edge gains anything (float64 rounding of sums of size m apart)
    if info["converged"]:
        gain, m = merge_gain_max(graph, mem, algo, rs)
        print("largest merge gain", gain, "allowed", 1e-12 * m)
        assert gain <= 1e-12 * m
    t4 = time.perf_counter()
    record_time("{}/{}".format(name, run_key(algo, rs)), {"nodes": n, "edges": int(len(rows)), "records": len(records), "test_s": round(t4 - t0, 3),
                                                          "run_trace_off_s": round(t2 - t1, 4), "run_trace_on_s": round(t3 - t2, 4)})


def test_an_edited_pin_fails_at_that_record():
    """The comparison is sensitive: one bit of one pinned prop hash, and the report names that record."""
    from seekr_amd.leiden import communities
    name, (algo, rs) = "dense", lc.TRACE_RUNS["dense"][0]
    graph = trace_graph(name)
    want = [tuple(r) for r in pinned()[name]["runs"][run_key(algo, rs)]["records"]]
    k = lm.route_records(want, "blk", 0)[2]
    edited = list(want)
    edited[k] = want[k][:5] + (want[k][5] ^ 1,) + want[k][6:]
    records = communities(*graph[:3], graph[3], algo=algo, rs=rs, trace=True)[2]["trace"]
    assert first_difference(records, want) is None and first_difference(records, edited) == k
    report = explain(graph, algo, rs, k, records, edited)
    print(report)
    assert report.startswith("record {} differs".format(k)) and "n_blk" in report


def test_trace_dump_gives_the_hashed_arrays():
    from seekr_amd.leiden import communities
    name, (algo, rs) = "dense", lc.TRACE_RUNS["dense"][1]
    graph = trace_graph(name)
    want = [tuple(r) for r in pinned()[name]["runs"][run_key(algo, rs)]["records"]]
    for kind in (lm.PROPOSE, lm.REFINE):
        k = [i for i in lm.route_records(want, "blk", 0) if want[i][0] == kind][1]
        info = communities(*graph[:3], graph[3], algo=algo, rs=rs, trace_dump=k)[2]
        a, b = info["trace_arrays"]
        assert a.dtype == np.uint32 and b.dtype == (np.float64 if kind == lm.PROPOSE else np.uint32) and len(a) == len(b) == want[k][2]
        assert (lm.fnv1a(a), lm.fnv1a(b)) == info["trace"][k][5:7] == want[k][5:7]
