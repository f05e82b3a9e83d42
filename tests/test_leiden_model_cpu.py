"""The sequential model of skr_leiden (tests/leiden_model.py) on its own, no GPU: it reproduces the device runs recorded in
profiles/leiden_quality.json, recovers the plants the device tests use, sums in det_sum's order, equals its own pins in
tests/golden/leiden_trace.json, and every pinned case can tell a wrong hash table from a right one."""
import functools
import json
import math
import os
import sys

import numpy as np
import pytest

import leiden_cases as lc
import leiden_model as lm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_golden_leiden_trace as gen  # noqa: E402

CONF = "RBConfigurationVertexPartition"


@functools.lru_cache(maxsize=None)
def recorded():
    with open(os.path.join(ROOT, "profiles", "leiden_quality.json")) as f:
        return json.load(f)


@functools.lru_cache(maxsize=None)
def pinned():
    with open(os.path.join(ROOT, "tests", "golden", "leiden_trace.json")) as f:
        return json.load(f)


@functools.lru_cache(maxsize=None)
def trace_graph(name):
    return lc.TRACE_CASES[name]()


@functools.lru_cache(maxsize=None)
def trace_run(name, algo, rs, fault=None):
    rows, cols, vals, n = trace_graph(name)
    return lm.model(rows, cols, vals, n, algo, rs, fault=fault)


SMALL_RUNS = [(name, algo, rs) for name in lc.TRACE_SMALL for algo, rs in lc.TRACE_RUNS[name]]


# ---- recorded device runs ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo,rs", lc.QUALITY_RUNS)
@pytest.mark.parametrize("name", sorted(lc.QUALITY_CASES))
def test_recorded_device_runs(name, algo, rs):
    """levels, sweeps and the community count of the device's run, and its quality within the 1e-9 rule of check_result."""
    entry = recorded()["{}/{}@{:g}".format(name, algo, rs)]
    rows, cols, vals, n = lc.QUALITY_CASES[name]()
    mem, info, _ = lm.model(rows, cols, vals, n, algo, rs)
    assert (info["levels"], info["sweeps"], info["n_communities"]) == (entry["levels"], entry["sweeps"], entry["communities"])
    q = lc.quality(rows, cols, vals, n, mem, algo, rs)
    print(name, algo, rs, "model", q, "device", entry["device"])
    assert abs(q - entry["device"]) <= 1e-9 * max(abs(entry["device"]), 1e-300) or q == entry["device"]


# ---- existing plants -----------------------------------------------------------------------------------------------
def _valid(graph, mem):
    rows, cols, _, n = graph
    assert mem.dtype == np.int32 and mem.shape == (n,)
    assert lc.size_ordered(mem) and lc.communities_connected(rows, cols, n, mem)


@pytest.mark.parametrize("name", ["ring_of_cliques", "k44", "p300", "p600"])
def test_plants(name):
    graph, plant = {"ring_of_cliques": lc.ring_of_cliques, "k44": lc.k44, "p300": lc.PLANTED_CASES["p300"], "p600": lc.PLANTED_CASES["p600"]}[name]()
    mem, info, _ = lm.model(*graph, CONF, 1.0)
    _valid(graph, mem)
    assert info["converged"] and lc.same_partition(mem, plant)


def test_hierarchy_level():
    graph, levels = lc.hierarchy()
    mem, info, _ = lm.model(*graph, CONF, 1.0)
    _valid(graph, mem)
    assert info["levels"] >= 2 and any(lc.same_partition(mem, lv) for lv in levels)


def test_degenerate():
    for graph in (lc.empty(1), lc.empty(10), lc.from_pairs([(0, 1)], [0.5], 2)):
        mem, info, _ = lm.model(*graph, "RBERVertexPartition", 1.0)
        assert np.array_equal(mem, np.arange(graph[3])) and info["n_communities"] == graph[3]


# ---- the summation order -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 15, 17, 4095, 4096, 4097, 70001, 256 * 4096 + 5])
def test_det_sum(n):
    """Against math.fsum.  A term passes through at most 16 + 8 additions in its workgroup and 16 + 8 in the last one at
    these sizes (<= 257 workgroups: two rounds of the strided loop), so the error is below 48 u sum|x| (u = 2^-53); on
    multiples of 2^-10 below 4 every partial sum is exact and so is the result."""
    rng = np.random.default_rng(n)
    x = rng.standard_normal(n) * np.exp(rng.uniform(-8, 8, n))
    assert abs(lm.det_sum(x) - math.fsum(x)) <= 48 * 2.0 ** -53 * math.fsum(np.abs(x))
    grid = rng.integers(1, 4097, size=n).astype(np.float64) / 1024.0
    assert lm.det_sum(grid) == math.fsum(grid)


def test_det_sum_order_is_the_written_one():
    """Terms chosen so that the order shows: 1.0, then 2^-53 (half an ulp of 1) 4 096 times.  Thread 0 adds 15 of them to
    1.0 one by one and each is lost to the tie; the other 255 threads hold 16 * 2^-53 each, which the tree adds without
    rounding: workgroup 0 gives 1 + 4 080 * 2^-53.  The last term is workgroup 1's sum; added to workgroup 0's at the
    tree's last step it is lost to the tie again.  The exact sum is 1 + 4 096 * 2^-53."""
    x = np.full(4097, 2.0 ** -53)
    x[0] = 1.0
    assert lm.det_sum(x) == 1.0 + 4080 * 2.0 ** -53 and math.fsum(x) == 1.0 + 4096 * 2.0 ** -53


# ---- the pins ------------------------------------------------------------------------------------------------------
def test_weights_are_on_the_grid():
    for name in lc.TRACE_SMALL:
        vals = trace_graph(name)[2].astype(np.float64) * 1024.0
        assert (vals == np.rint(vals)).all() and vals.min() >= 1 and vals.max() <= 4096


@pytest.mark.parametrize("name,algo,rs", SMALL_RUNS)
def test_pins_equal_the_model(name, algo, rs):
    pin = pinned()[name]
    graph = trace_graph(name)
    assert pin["graph_hash"] == lm.graph_hash(graph), "the case changed: regenerate tests/golden/leiden_trace.json"
    run = pin["runs"][gen.run_key(algo, rs)]
    mem, info, trace = trace_run(name, algo, rs)
    _valid(graph, mem)
    for key in ("levels", "sweeps", "converged", "n_communities"):
        assert run[key] == info[key], key
    assert run["membership_hash"] == lm.fnv1a(mem.astype("<i4")) and run["membership"] == mem.tolist()
    assert [tuple(r) for r in run["records"]] == trace


@pytest.mark.parametrize("name", [n for n in lc.TRACE_CASES if n not in lc.TRACE_SMALL])
def test_large_pins(name):
    """Too slow to rerun here: the graph's hash, that every run has records, and that the generator found both faults."""
    pin = pinned()[name]
    assert pin["graph_hash"] == lm.graph_hash(trace_graph(name)), "the case changed: regenerate tests/golden/leiden_trace.json"
    limit, route, level = lc.TRACE_ROUTES[name]
    for algo, rs in lc.TRACE_RUNS[name]:
        run = pin["runs"][gen.run_key(algo, rs)]
        records = [tuple(r) for r in run["records"]]
        assert len(records) > 0 and sum(r[0] == lm.SWEEP for r in records) == run["sweeps"]
        reached = lm.route_records(records, route, level)
        assert {records[k][0] for k in reached} == {lm.PROPOSE, lm.REFINE}
        assert all(run["first_fault_record"][f] in reached for f in gen.FAULTS)


def test_many_hubs_has_more_hubs_than_tables():
    """More nodes above the LDS limit than twice the CU count of any MI355X (256 CUs)."""
    graph = trace_graph("many_hubs")
    deg = np.bincount(np.concatenate([graph[0], graph[1]]), minlength=graph[3])
    assert (deg > lm.LDS_DEG).sum() > 512
    assert pinned()["many_hubs"]["runs"][gen.run_key(CONF, 1.0)]["records"][0][4] > 512


def test_pairs_glb_reaches_the_device_memory_unit_only_on_the_aggregate():
    graph = trace_graph("pairs_glb")
    deg = np.bincount(np.concatenate([graph[0], graph[1]]), minlength=graph[3])
    assert deg.max() <= lm.LDS_DEG
    records = pinned()["pairs_glb"]["runs"][gen.run_key(CONF, 1.0)]["records"]
    assert all(r[4] == 0 for r in records if r[0] != lm.SWEEP and r[1] == 0) and any(r[4] > lm.LDS_DEG for r in records if r[0] != lm.SWEEP and r[1] == 1)


# ---- what the cases are worth ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,algo,rs", SMALL_RUNS)
def test_route_is_reached(name, algo, rs):
    """The work unit the case is there for has nodes at the intended level, in local moving and in refinement."""
    _, route, level = lc.TRACE_ROUTES[name]
    trace = trace_run(name, algo, rs)[2]
    reached = lm.route_records(trace, route, level)
    assert {trace[k][0] for k in reached} == {lm.PROPOSE, lm.REFINE}


def test_boundary_degrees_are_present():
    for name, degrees in (("dense", (lm.WAVE_DEG, lm.WAVE_DEG + 1)), ("hubs", (lm.LDS_DEG, lm.LDS_DEG + 1))):
        graph = trace_graph(name)
        deg = np.bincount(np.concatenate([graph[0], graph[1]]), minlength=graph[3])
        assert all((deg == d).any() for d in degrees), (name, degrees)


@pytest.mark.parametrize("fault", gen.FAULTS)
@pytest.mark.parametrize("name,algo,rs", SMALL_RUNS)
def test_injected_fault_changes_a_record(name, algo, rs, fault):
    """A table that drops an edge, or loses a key, at the nodes of the intended work unit changes a proposal record of that
    unit and level — whether or not the final membership moves (it mostly does not: that is why the records are pinned)."""
    limit, route, level = lc.TRACE_ROUTES[name]
    mem, _, trace = trace_run(name, algo, rs)
    mem_f, _, spoilt = trace_run(name, algo, rs, (fault, limit))
    k = lm.first_fault_record(trace, spoilt, route, level)
    print("fault", name, algo, rs, fault, "first differing record", k, None if k is None else trace[k][:5],
          "membership", "unchanged" if np.array_equal(mem, mem_f) else "changed")
    assert k is not None
    assert k == pinned()[name]["runs"][gen.run_key(algo, rs)]["first_fault_record"][fault]


def test_first_differing_node_compares_bits():
    a = np.array([0.0, 1.5, -0.0, 2.0])
    assert lm.first_differing_node(a, a.copy()) is None
    assert lm.first_differing_node(a, np.array([0.0, 1.5, 0.0, 2.0])) == 2  # -0.0 and 0.0 are equal numbers, other bits
    assert lm.first_differing_node(np.array([1, 2, 3], np.uint32), np.array([1, 2, 4], "<u4")) == 2
    assert lm.first_differing_node(a, a[:3]) == -1
