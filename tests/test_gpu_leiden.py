"""skr_leiden / seekr_amd.leiden / kmer_leiden on the device: exact partitions of planted graphs, the work-unit boundaries,
several levels, quality against the sequential Louvain pinned in tests/golden/leiden_cases.json, the input checks and the
end-to-end paths.  Every result also passes `check_result`: dense size-ordered labels, connected communities, the
reported quality equal to leiden_cases.quality, and the same bytes on a second call."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import leiden_cases as lc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RBER, CONF, CPM, MOD = "RBERVertexPartition", "RBConfigurationVertexPartition", "CPMVertexPartition", "ModularityVertexPartition"


def run(graph, algo=RBER, rs=1.0, **kw):
    from seekr_amd.leiden import communities
    rows, cols, vals, n = graph
    return communities(rows, cols, vals, n, algo=algo, rs=rs, **kw)


def check_result(graph, algo=RBER, rs=1.0, **kw):
    rows, cols, vals, n = graph
    mem, q, info = run(graph, algo, rs, **kw)
    assert mem.dtype == np.int32 and mem.shape == (n,)
    assert lc.size_ordered(mem), "labels are not dense and size-ordered"
    assert info["n_communities"] == (int(mem.max()) + 1 if n else 0)
    assert lc.communities_connected(rows, cols, n, mem), "a community is not connected"
    ref = lc.quality(rows, cols, vals, n, mem, algo, rs)
    print("quality", algo, rs, "device", q, "numpy", ref, "info", info)
    assert abs(q - ref) <= 1e-9 * max(abs(ref), 1e-300) or q == ref
    mem2, q2, info2 = run(graph, algo, rs, **kw)
    assert mem2.tobytes() == mem.tobytes() and q2 == q and info2 == info, "a second call differs"
    return mem, q, info


# ---- exact partitions ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", [lc.empty(1), lc.from_pairs([(0, 1)], [0.5], 2), lc.empty(10)], ids=["n1", "n2", "n10"])
def test_degenerate(graph):
    mem, q, _ = check_result(graph)
    assert np.array_equal(mem, np.arange(graph[3])) and q == 0.0


def test_disjoint_edges_swap_rule():
    graph, plant = lc.disjoint_edges(50, 0.5)
    mem, _, _ = check_result(graph)
    assert lc.same_partition(mem, plant)


def test_k44_one_community():
    """One community, of quality 0.0 = 16 - 32^2 / 64.  Two K2,2 and four pairs score 0 as well, and no partition of K4,4 scores
    more at resolution 1: merging two of its balanced communities gains exactly 0.  Strict gains alone stop at {1, 2, 4, 6},
    {0, 7}, {3, 5}; on the aggregate a node alone in its community joins a neighbour on a tie, which ends in the plant."""
    graph, plant = lc.k44()
    mem, _, _ = check_result(graph, CONF, 1.0)
    assert lc.same_partition(mem, plant)


def test_ring_of_cliques():
    graph, plant = lc.ring_of_cliques()
    mem, _, _ = check_result(graph, CONF, 1.0)
    assert lc.same_partition(mem, plant)


@pytest.mark.parametrize("name", sorted(lc.PLANTED_CASES))
def test_planted(name):
    graph, plant = lc.PLANTED_CASES[name]()
    mem, _, _ = check_result(graph, CONF, 1.0)
    assert lc.same_partition(mem, plant)


def test_numbering():
    graph, plant = lc.numbering_case()
    mem, _, _ = check_result(graph)
    assert np.array_equal(mem, plant)


# ---- work-unit boundaries -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def yardstick_min(make, arg, algo, rs):
    """The worst of 4 visiting orders of the sequential Louvain on a boundary graph."""
    rows, cols, vals, n = make(*arg)
    return min(lc.quality(rows, cols, vals, n, lc.louvain(rows, cols, vals, n, algo, rs, seed=s), algo, rs) for s in range(4))


def boundary_degrees():
    from seekr_amd.leiden import limits
    wave, lds = limits()
    return [d for b in (wave, lds) for d in (b - 1, b, b + 1)]


def test_limits_are_reported():
    from seekr_amd.leiden import limits
    wave, lds = limits()
    assert 1 <= wave < lds


@pytest.mark.parametrize("which", range(6))
@pytest.mark.parametrize("shape", ["star", "double_star"])
def test_boundary(which, shape):
    d = boundary_degrees()[which]
    make, arg = (lc.star, (d,)) if shape == "star" else (lc.double_star, (d - 1, max(d // 2, 1)))  # hub 0 has d neighbours
    graph = make(*arg)
    deg = np.bincount(np.concatenate([graph[0], graph[1]]))
    assert deg.max() == d
    _, q, _ = check_result(graph, CONF, 1.0)
    bar = yardstick_min(make, arg, CONF, 1.0)
    print("boundary", shape, d, "device", q, "yardstick", bar)
    assert q >= bar - 1e-9 * float(graph[2].sum())  # float64 rounding of sums of this size, nothing more


def test_more_communities_than_the_lds_table():
    from seekr_amd.leiden import limits
    graph = lc.hub_over_pairs(limits()[1] + 7)
    _, q, _ = check_result(graph, CONF, 1.0)
    bar = yardstick_min(lc.hub_over_pairs, (limits()[1] + 7,), CONF, 1.0)
    print("hub over pairs: device", q, "yardstick", bar)
    assert q >= bar - 1e-9 * float(graph[2].sum())


# ---- several levels -------------------------------------------------------------------------------------------------
def test_hierarchy():
    graph, levels = lc.hierarchy()
    mem, _, info = check_result(graph, CONF, 1.0)
    assert info["levels"] >= 2
    assert any(lc.same_partition(mem, lv) for lv in levels)


# ---- quality against the yardstick --------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pinned():
    with open(os.path.join(ROOT, "tests", "golden", "leiden_cases.json")) as f:
        return json.load(f)


def record_quality(key, entry):
    path = os.path.join(ROOT, "profiles", "leiden_quality.json")
    try:
        with open(path) as f:
            table = json.load(f)
    except (OSError, ValueError):
        table = {}
    table[key] = entry
    try:
        with open(path, "w") as f:
            json.dump(table, f, indent=1, sort_keys=True)
            f.write("\n")
    except OSError:
        pass


@pytest.mark.parametrize("algo,rs", lc.QUALITY_RUNS)
@pytest.mark.parametrize("name", sorted(lc.QUALITY_CASES))
def test_quality(name, algo, rs):
    graph = lc.QUALITY_CASES[name]()
    pin = pinned()[name]["runs"]["{}@{:g}".format(algo, rs)]
    _, q, info = check_result(graph, algo, rs)
    bar = pin["min"] - (pin["max"] - pin["min"])
    print("quality case", name, algo, rs, "device", q, "pinned", pin, "bar", bar)
    record_quality("{}/{}@{:g}".format(name, algo, rs), {"device": q, "communities": info["n_communities"], "levels": info["levels"],
                                                         "sweeps": info["sweeps"], "pinned_min": pin["min"], "pinned_max": pin["max"], "bar": bar})
    assert q >= bar


def test_modularity_is_configuration_over_m():
    graph = lc.QUALITY_CASES["hardB"]()
    mem_c, q_c, _ = check_result(graph, CONF, 1.0)
    mem_m, q_m, _ = check_result(graph, MOD, 7.0)  # the resolution is ignored
    assert np.array_equal(mem_c, mem_m)
    assert abs(q_m - q_c / graph[2].astype(np.float64).sum()) <= 1e-12


# ---- input checks -------------------------------------------------------------------------------------------------
def test_refuses_row_not_below_col():
    from seekr_amd.leiden import communities
    for r, c in ((3, 1), (2, 2)):
        with pytest.raises(ValueError, match="row < col"):
            communities(np.array([0, r], np.uint32), np.array([1, c], np.uint32), np.array([0.5, 0.5], np.float32), 5)


@pytest.mark.parametrize("bad", [0.0, -0.25, np.nan])
def test_refuses_bad_weight(bad):
    from seekr_amd.leiden import communities
    with pytest.raises(ValueError, match="weights"):
        communities(np.array([0, 1], np.uint32), np.array([1, 2], np.uint32), np.array([0.5, bad], np.float32), 5)


def test_refuses_index_beyond_n():
    from seekr_amd.leiden import communities
    with pytest.raises(ValueError, match="n_nodes"):
        communities(np.array([0, 1], np.uint32), np.array([1, 5], np.uint32), np.array([0.5, 0.5], np.float32), 5)


def test_one_sweep_is_valid_and_not_converged():
    graph, _ = lc.PLANTED_CASES["p300"]()
    _, _, info = check_result(graph, CONF, 1.0, max_sweeps=1)
    assert info["converged"] is False


def test_names_what_is_not_built():
    from seekr_amd.leiden import communities
    for algo in ("SurpriseVertexPartition", "SignificanceVertexPartition"):
        with pytest.raises(NotImplementedError, match=algo):
            communities(np.array([0], np.uint32), np.array([1], np.uint32), np.array([0.5], np.float32), 2, algo=algo)


def test_device_matrices_in():
    from seekr_amd import _lib
    from seekr_amd.leiden import communities
    graph, plant = lc.ring_of_cliques()
    rows, cols, vals, n = graph
    ctx = _lib.default_context()
    mats = [ctx.from_numpy(a.reshape(-1, 1)) for a in (rows, cols, vals)]
    mem, q, _ = communities(mats[0], mats[1], mats[2], n, algo=CONF)
    mem_host, q_host, _ = communities(rows, cols, vals, n, algo=CONF)
    assert np.array_equal(mem, mem_host) and q == q_host and lc.same_partition(mem, plant)


# ---- end to end ---------------------------------------------------------------------------------------------------
E2E_CUTOFF, E2E_K = 0.2, 3


@pytest.fixture(scope="module")
def fasta_case(tmp_path_factory):
    from seekr_amd.kmer_counts import BasicCounter
    from seekr_amd.synthetic import profile_seqs
    d = tmp_path_factory.mktemp("leiden")
    seqs, which = profile_seqs(5, 300, 400)
    fa = d / "seqs.fa"
    with open(fa, "w") as f:
        for i, s in enumerate(seqs):
            f.write(">tx%d\n%s\n" % (i, s))
    c = BasicCounter(str(fa), k=E2E_K, silent=True)
    c.get_counts()
    np.save(d / "mean.npy", c.mean)
    np.save(d / "std.npy", c.std)
    return d, fa, which, np.asarray(c.counts, dtype=np.float32)


def test_pearson_communities(fasta_case):
    from seekr_amd import _lib
    from seekr_amd.leiden import pearson_communities
    _, _, which, counts = fasta_case
    ctx = _lib.default_context()
    x = ctx.from_numpy(counts)
    z, _ = _lib.operand_fill(ctx, x, None, _lib.PREC_F16X3)
    mem, q, info = pearson_communities(z, E2E_CUTOFF)
    z.free()
    x.free()
    assert info["n_communities"] == 3 and lc.same_partition(mem, which)
    rows, cols, vals = info["edges"]
    assert abs(q - lc.quality(rows, cols, vals, 300, mem, RBER, 1.0)) <= 1e-9 * abs(q)


def test_kmer_leiden_csv(fasta_case, capsys):
    import pandas as pd
    from seekr_amd.kmer_leiden import kmer_leiden
    d, fa, which, _ = fasta_case
    mem = kmer_leiden(str(fa), str(d / "mean.npy"), str(d / "std.npy"), E2E_K, pearsoncutoff=E2E_CUTOFF, csvfile=str(d / "out"), edges="nonzero")
    assert lc.same_partition(mem, which)
    nodes = pd.read_csv(d / "out_nodes_leiden.csv")
    assert list(nodes.columns) == ["Id", "Label", "Color"] and len(nodes) == 300
    assert list(nodes["Color"]) == sorted(nodes["Color"]) and list(nodes["Id"]) == list(nodes["Label"])
    for name, color in zip(nodes["Id"], nodes["Color"]):
        assert mem[int(name[2:])] == color - 1
    for c in range(3):
        ids = [int(s[2:]) for s in nodes["Id"][nodes["Color"] == c + 1]]
        assert ids == sorted(ids)
    edges = pd.read_csv(d / "out_edges_leiden.csv")
    assert list(edges.columns) == ["Source", "Target", "Weight"] and (edges["Weight"] >= E2E_CUTOFF).all()
    # the vectors do not fit k: the reference's three lines, and None
    capsys.readouterr()
    assert kmer_leiden(str(fa), str(d / "mean.npy"), str(d / "std.npy"), E2E_K + 1) is None
    assert capsys.readouterr().out.count("\n") == 3


def test_command(fasta_case):
    import pandas as pd
    from seekr_amd.kmer_leiden import kmer_leiden
    d, fa, which, _ = fasta_case
    argv = ["seekr_kmer_leiden", str(fa), str(d / "mean.npy"), str(d / "std.npy"), str(E2E_K), "-pco", str(E2E_CUTOFF), "-cf", str(d / "cmd"),
            "--edges", "nonzero", "-sd"]
    code = "import sys; sys.argv = %r; from seekr_amd.console_scripts import console_kmer_leiden; console_kmer_leiden()" % (argv,)
    proc = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0, proc.stderr
    mem = kmer_leiden(str(fa), str(d / "mean.npy"), str(d / "std.npy"), E2E_K, pearsoncutoff=E2E_CUTOFF)
    nodes = pd.read_csv(d / "cmd_nodes_leiden.csv")
    assert [mem[int(s[2:])] + 1 for s in nodes["Id"]] == list(nodes["Color"])
