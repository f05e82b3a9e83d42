"""The host side of the community feature: the yardstick and helpers of tests/leiden_cases.py, the pinned JSON, the CSV
writers, the refusals and the command's registration.  No GPU."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import leiden_cases as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONF = "RBConfigurationVertexPartition"


@pytest.mark.parametrize("make", [lc.disjoint_edges, lc.k44, lc.ring_of_cliques, lc.PLANTED_CASES["p600"], lc.PLANTED_CASES["p300"]],
                         ids=["pairs", "k44", "ring", "p600", "p300"])
def test_yardstick_recovers_the_plant(make):
    (rows, cols, vals, n), plant = make()
    for seed in range(3):
        mem = lc.louvain(rows, cols, vals, n, CONF, 1.0, seed=seed)
        assert lc.same_partition(mem, plant)
        assert lc.communities_connected(rows, cols, n, mem)


def test_k44_partitions_tie():
    # K4,4 at resolution 1: one community, two K2,2 and four pairs all have configuration-model quality 0 (no partition of a
    # complete bipartite graph does better); the yardstick reaches the one community above by its tie rule on aggregates
    (rows, cols, vals, n), plant = lc.k44()
    for mem in (plant, np.arange(8) % 4, np.arange(8) % 2):
        assert lc.quality(rows, cols, vals, n, mem, CONF, 1.0) == 0.0


def test_yardstick_recovers_a_hierarchy_level():
    (rows, cols, vals, n), levels = lc.hierarchy()
    mem = lc.louvain(rows, cols, vals, n, CONF, 1.0, seed=0)
    assert any(lc.same_partition(mem, lv) for lv in levels)


def test_json_matches_a_rerun():
    import make_golden_leiden as mg
    with open(os.path.join(ROOT, "tests", "golden", "leiden_cases.json")) as f:
        pinned = json.load(f)
    assert sorted(pinned) == sorted(lc.QUALITY_CASES)
    graph = lc.QUALITY_CASES["er"]()
    assert pinned["er"]["nodes"] == graph[3] and pinned["er"]["edges"] == len(graph[0])
    again = mg.yardstick(graph, "RBERVertexPartition", 1.0)
    assert again == pinned["er"]["runs"]["RBERVertexPartition@1"]
    for entry in pinned.values():
        assert sorted(entry["runs"]) == sorted("{}@{:g}".format(a, r) for a, r in lc.QUALITY_RUNS)


def test_quality_agrees_with_networkx():
    nx = pytest.importorskip("networkx")
    rows, cols, vals, n = lc.QUALITY_CASES["hardB"]()
    mem = lc.louvain(rows, cols, vals, n, CONF, 1.0, seed=1)
    g = nx.Graph()
    g.add_nodes_from(range(n))
    g.add_weighted_edges_from(zip(rows.tolist(), cols.tolist(), vals.astype(np.float64).tolist()))
    parts = [set(np.nonzero(mem == c)[0].tolist()) for c in range(int(mem.max()) + 1)]
    assert abs(lc.quality(rows, cols, vals, n, mem, "ModularityVertexPartition") - nx.community.modularity(g, parts, weight="weight")) < 1e-12


def test_quality_by_hand():
    # a triangle and a pendant node: {0, 1, 2} and {3}
    rows, cols, vals, n = lc.from_pairs([(0, 1), (1, 2), (0, 2), (2, 3)], [1.0, 1.0, 1.0, 0.5], 4)
    mem = [0, 0, 0, 1]
    m = 3.5
    assert lc.quality(rows, cols, vals, n, mem, CONF, 2.0) == pytest.approx(3.0 - 2.0 * (6.5 ** 2 + 0.5 ** 2) / (4 * m), abs=1e-14)
    assert lc.quality(rows, cols, vals, n, mem, "CPMVertexPartition", 0.5) == pytest.approx(3.0 - 0.5 * 3.0, abs=1e-14)
    assert lc.quality(rows, cols, vals, n, mem, "RBERVertexPartition", 1.0) == pytest.approx(3.0 - (m / 6.0) * 3.0, abs=1e-14)


def test_helpers():
    assert lc.same_partition([0, 0, 1], [5, 5, 2]) and not lc.same_partition([0, 0, 1], [0, 1, 1])
    assert lc.size_ordered([0, 0, 1, 2]) and not lc.size_ordered([1, 1, 0]) and not lc.size_ordered([0, 2, 2, 1, 1])
    assert lc.size_ordered([0, 0, 1, 1, 2]) and not lc.size_ordered([1, 1, 0, 0, 2])  # ties: the smallest node first
    rows, cols, _, n = lc.from_pairs([(0, 1), (2, 3)], [1, 1], 4)
    assert lc.communities_connected(rows, cols, n, [0, 0, 1, 1]) and not lc.communities_connected(rows, cols, n, [0, 0, 0, 1])


def test_csv_writers(tmp_path):
    from seekr_amd.kmer_leiden import write_edges_csv, write_nodes_csv
    names = ["a", "b,1", "c", "d"]
    write_nodes_csv(tmp_path / "n.csv", names, np.array([1, 0, 1, 0], dtype=np.int32))
    assert (tmp_path / "n.csv").read_bytes() == b'Id,Label,Color\n"b,1","b,1",1\nd,d,1\na,a,2\nc,c,2\n'
    rows, cols, vals = np.array([1, 0], np.uint32), np.array([3, 2], np.uint32), np.array([0.5, 0.25], np.float32)
    write_edges_csv(tmp_path / "e.csv", names, rows, cols, vals)
    assert (tmp_path / "e.csv").read_bytes() == (b'Source,Target,Weight\na,"b,1",0.0\na,c,0.25\na,d,0.0\n"b,1",c,0.0\n"b,1",d,0.5\nc,d,0.0\n')
    write_edges_csv(tmp_path / "z.csv", names, rows, cols, vals, edges="nonzero")
    assert (tmp_path / "z.csv").read_bytes() == b'Source,Target,Weight\na,c,0.25\n"b,1",d,0.5\n'
    with pytest.raises(ValueError):
        write_edges_csv(tmp_path / "x.csv", names, rows, cols, vals, edges="some")


def test_all_edges_refused_when_too_many(tmp_path):
    from seekr_amd import kmer_leiden as kl
    names = ["s%d" % i for i in range(20000)]  # 2e8 cells
    with pytest.raises(ValueError, match="nonzero"):
        kl.write_edges_csv(tmp_path / "e.csv", names, np.empty(0, np.uint32), np.empty(0, np.uint32), np.empty(0, np.float32))
    assert not (tmp_path / "e.csv").exists()


def test_not_implemented():
    from seekr_amd.kmer_leiden import kmer_leiden
    from seekr_amd.leiden import algo_code, communities
    with pytest.raises(NotImplementedError, match="csvfile"):
        kmer_leiden("x.fa", "m.npy", "s.npy", 4, plotname="plot")
    for algo in ("SurpriseVertexPartition", "SignificanceVertexPartition"):
        with pytest.raises(NotImplementedError, match=algo):
            algo_code(algo)
        with pytest.raises(NotImplementedError, match=algo):
            communities(np.array([0], np.uint32), np.array([1], np.uint32), np.array([1.0], np.float32), 2, algo=algo)
        with pytest.raises(NotImplementedError, match=algo):
            kmer_leiden("x.fa", "m.npy", "s.npy", 4, algo=algo)
    with pytest.raises(ValueError):
        algo_code("Louvain")


def test_signature_keeps_the_reference_names():
    import inspect
    from seekr_amd.kmer_leiden import kmer_leiden
    params = inspect.signature(kmer_leiden).parameters
    assert list(params)[:13] == ["inputfile", "mean", "std", "k", "algo", "rs", "pearsoncutoff", "setseed", "edgecolormethod", "edgethreshold",
                                 "labelfontsize", "plotname", "csvfile"]
    defaults = {k: v.default for k, v in params.items() if v.default is not inspect.Parameter.empty}
    assert defaults == {"algo": "RBERVertexPartition", "rs": 1.0, "pearsoncutoff": 0, "setseed": False, "edgecolormethod": "gradient",
                        "edgethreshold": 0.1, "labelfontsize": 12, "plotname": None, "csvfile": None, "edges": "all"}


def test_command_help_and_registration():
    code = "import sys; sys.argv = ['seekr_kmer_leiden', '-h']; from seekr_amd.console_scripts import console_kmer_leiden; console_kmer_leiden()"
    proc = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert proc.returncode == 0, proc.stderr
    for flag in ("--algo", "--rs", "--pearsoncutoff", "--setseed", "--edgecolormethod", "--edgethreshold", "--labelfontsize", "--plotname",
                 "--csvfile", "--edges"):
        assert flag in proc.stdout
    with open(os.path.join(ROOT, "setup.py")) as f:
        assert "seekr_kmer_leiden = seekr_amd.console_scripts:console_kmer_leiden" in f.read()


def test_library_declares_the_entry_points():
    from seekr_amd import _lib
    for name in ("skr_leiden", "skr_leiden_last", "skr_leiden_limits"):
        assert name in _lib.SIGNATURES
    with open(os.path.join(ROOT, "include", "seekr_hip.h")) as f:
        header = f.read()
    assert "int skr_leiden(skr_ctx* ctx" in header and "int skr_leiden_limits(" in header
