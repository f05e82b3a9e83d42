"""Graphs, quality functions and a sequential Louvain for the community tests (plain numpy, no GPU).

A graph is (rows, cols, vals, n): the upper-triangle list pearson_edges(..., upper_only=True) returns — uint32 row < col,
float32 weight > 0.  `louvain` is the yardstick the device result is measured against: local moving in a visiting order
given by a seed, then aggregation, for the four quality functions of skr_leiden."""
import numpy as np

ALGOS = {"RBConfigurationVertexPartition": 0, "ModularityVertexPartition": 1, "RBERVertexPartition": 2, "CPMVertexPartition": 3}


# ------------------------------------------------------------------------------------------------ graphs
def from_pairs(pairs, weights, n):
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    lo, hi = pairs.min(axis=1), pairs.max(axis=1)
    return lo.astype(np.uint32), hi.astype(np.uint32), np.asarray(weights, dtype=np.float32).reshape(-1), int(n)


def empty(n):
    return from_pairs(np.empty((0, 2)), np.empty(0), n)


def disjoint_edges(k=50, w=0.5):
    return from_pairs([(2 * i, 2 * i + 1) for i in range(k)], [w] * k, 2 * k), np.repeat(np.arange(k), 2)


def k44(w=1.0):
    return from_pairs([(i, 4 + j) for i in range(4) for j in range(4)], [w] * 16, 8), np.zeros(8, dtype=np.int64)


def clique_pairs(nodes):
    nodes = list(nodes)
    return [(a, b) for i, a in enumerate(nodes) for b in nodes[i + 1:]]


def ring_of_cliques(cliques=8, size=6, w_in=0.9, w_out=0.05):
    pairs, ws = [], []
    for c in range(cliques):
        p = clique_pairs(range(c * size, (c + 1) * size))
        pairs += p
        ws += [w_in] * len(p)
        pairs.append((c * size + size - 1, ((c + 1) % cliques) * size))
        ws.append(w_out)
    return from_pairs(pairs, ws, cliques * size), np.repeat(np.arange(cliques), size)


def numbering_case():
    """A 5-clique, a 3-clique and two isolated nodes: numbered 0 (the 5), 1 (the 3), 2 and 3 (nodes 8 and 9)."""
    pairs = clique_pairs(range(5)) + clique_pairs(range(5, 8))
    return from_pairs(pairs, [0.8] * len(pairs), 10), np.array([0] * 5 + [1] * 3 + [2, 3])


def planted(n, groups, p_in, p_out, seed, w_in=(0.5, 1.0), w_out=(0.01, 0.2)):
    """Planted partition: node v is in group v % groups; an inner pair is an edge with probability p_in and a weight
    uniform in w_in, an outer pair with p_out and a weight uniform in w_out."""
    rng = np.random.default_rng(seed)
    r, c = np.triu_indices(n, 1)
    g = np.arange(n) % groups
    same = g[r] == g[c]
    u = rng.random(len(r))
    keep = u < np.where(same, p_in, p_out)
    lo, hi = np.where(same, w_in[0], w_out[0]), np.where(same, w_in[1], w_out[1])
    w = lo + (hi - lo) * rng.random(len(r))
    return (r[keep].astype(np.uint32), c[keep].astype(np.uint32), w[keep].astype(np.float32), n), g


def uniform_blocks(n, groups, p_in, p_out, seed):
    """The hard cases: weights uniform in (0.01, 1) whatever the pair; groups = 1: no structure at all."""
    return planted(n, groups, p_in, p_out, seed, w_in=(0.01, 1.0), w_out=(0.01, 1.0))[0]


def star(leaves, w=0.5):
    return from_pairs([(0, 1 + i) for i in range(leaves)], [w] * leaves, leaves + 1)


def double_star(leaves_a, leaves_b, w=0.5):
    """Two hubs (nodes 0 and 1) joined by an edge, with their own leaves."""
    pairs = [(0, 1)] + [(0, 2 + i) for i in range(leaves_a)] + [(1, 2 + leaves_a + i) for i in range(leaves_b)]
    return from_pairs(pairs, [w] * len(pairs), 2 + leaves_a + leaves_b)


def hub_over_pairs(pairs_count, w_pair=0.9, w_hub=0.05):
    """A hub (node 0) tied weakly to one end of each of `pairs_count` strongly tied pairs: at the first sweep every
    neighbour of the hub is a community of its own."""
    pairs, ws = [], []
    for i in range(pairs_count):
        a, b = 1 + 2 * i, 2 + 2 * i
        pairs += [(a, b), (0, a)]
        ws += [w_pair, w_hub]
    return from_pairs(pairs, ws, 1 + 2 * pairs_count)


def hierarchy(w=(0.9, 0.3, 0.05)):
    """64 nodes: 4-cliques (weight w[0]), four cliques to a cluster (one w[1] edge between each pair of its cliques), four
    clusters to the super-cluster (one w[2] edge between each pair of clusters).  Returns the graph and the planted levels."""
    pairs, ws = [], []
    for q in range(16):
        p = clique_pairs(range(4 * q, 4 * q + 4))
        pairs += p
        ws += [w[0]] * len(p)
    for cl in range(4):
        for a in range(4):
            for b in range(a + 1, 4):
                pairs.append((16 * cl + 4 * a + b % 4, 16 * cl + 4 * b + a % 4))
                ws.append(w[1])
    for a in range(4):
        for b in range(a + 1, 4):
            pairs.append((16 * a + b, 16 * b + a))
            ws.append(w[2])
    v = np.arange(64)
    return from_pairs(pairs, ws, 64), [v // 4, v // 16, v // 64]


# ------------------------------------------------------------------------------------------------ checks
def quality(rows, cols, vals, n, membership, algo, rs=1.0):
    """The function skr_leiden maximises, in float64 (include/seekr_hip.h lists the four)."""
    q = ALGOS[algo] if isinstance(algo, str) else int(algo)
    mem = np.asarray(membership, dtype=np.int64)
    w = np.asarray(vals, dtype=np.float64)
    r, c = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    m = w.sum()
    nc = int(mem.max()) + 1 if len(mem) else 0
    inner = w[mem[r] == mem[c]].sum()
    if q <= 1:
        if m == 0:
            return 0.0
        gamma = 1.0 if q == 1 else rs
        deg = np.bincount(r, w, n) + np.bincount(c, w, n)
        K = np.bincount(mem, deg, nc)
        val = inner - gamma * (K * K).sum() / (4.0 * m)
        return val / m if q == 1 else val
    sizes = np.bincount(mem, minlength=nc).astype(np.float64)
    pairs = (sizes * (sizes - 1.0) / 2.0).sum()
    p = m / (n * (n - 1) / 2.0) if (q == 2 and n > 1) else 1.0
    return inner - rs * p * pairs


def _find(parent, v):
    while parent[v] != v:
        parent[v] = parent[parent[v]]
        v = parent[v]
    return v


def communities_connected(rows, cols, n, membership):
    """Is every community connected in the graph?  (union-find over the edges inside communities)"""
    mem = np.asarray(membership)
    parent = list(range(n))
    for a, b in zip(np.asarray(rows).tolist(), np.asarray(cols).tolist()):
        if mem[a] == mem[b]:
            ra, rb = _find(parent, a), _find(parent, b)
            if ra != rb:
                parent[max(ra, rb)] = min(ra, rb)
    roots = {}
    for v in range(n):
        roots.setdefault(int(mem[v]), set()).add(_find(parent, v))
    return all(len(s) == 1 for s in roots.values())


def same_partition(a, b):
    """Equal up to relabelling."""
    a, b = np.asarray(a).reshape(-1), np.asarray(b).reshape(-1)
    if a.shape != b.shape:
        return False
    fwd, back = {}, {}
    for x, y in zip(a.tolist(), b.tolist()):
        if fwd.setdefault(x, y) != y or back.setdefault(y, x) != x:
            return False
    return True


def size_ordered(membership):
    """Dense labels 0..c-1, numbered by size (largest first), ties to the community holding the smallest node."""
    mem = np.asarray(membership, dtype=np.int64)
    if len(mem) == 0:
        return True
    nc = int(mem.max()) + 1
    sizes = np.bincount(mem, minlength=nc)
    if mem.min() < 0 or (sizes == 0).any():
        return False
    first = np.full(nc, len(mem))
    np.minimum.at(first, mem, np.arange(len(mem)))
    keys = list(zip((-sizes).tolist(), first.tolist()))
    return keys == sorted(keys)


# ------------------------------------------------------------------------------------------------ the yardstick
def louvain(rows, cols, vals, n, algo, rs=1.0, seed=0, max_levels=32, max_sweeps=64):
    """Sequential Louvain: nodes visited in the order of `seed`, each moved to the neighbouring community (or to an
    empty one) of largest gain; then communities become nodes; until nothing moves.  A move needs a gain above the
    node's staying; on an aggregate a node alone in its community also joins the neighbouring community of lowest label
    whose gain is exactly 0 (the device's rule for partitions that tie: the coarser one).  Returns the membership."""
    q = ALGOS[algo] if isinstance(algo, str) else int(algo)
    rng = np.random.default_rng(seed)
    w = np.asarray(vals, dtype=np.float64)
    m = float(w.sum())
    member = np.arange(n)
    if m == 0:
        return member
    gamma = 1.0 if q == 1 else rs
    scale = gamma / (2.0 * m) if q <= 1 else (gamma * m / (n * (n - 1) / 2.0) if q == 2 else gamma)
    adj = [dict() for _ in range(n)]
    for a, b, x in zip(np.asarray(rows).tolist(), np.asarray(cols).tolist(), w.tolist()):
        adj[a][b] = adj[a].get(b, 0.0) + x
        adj[b][a] = adj[b].get(a, 0.0) + x
    if q <= 1:
        mass = [sum(d.values()) for d in adj]
    else:
        mass = [1.0] * n
    for level in range(max_levels):
        nn = len(adj)
        comm = list(range(nn))
        tot = list(mass)
        size = [1] * nn
        moved_any = False
        for _ in range(max_sweeps):
            moved = 0
            for v in rng.permutation(nn).tolist():
                own = comm[v]
                to = {}
                for u, x in adj[v].items():
                    if u != v:
                        to[comm[u]] = to.get(comm[u], 0.0) + x
                a = mass[v]
                tot[own] -= a
                best, best_g = own, to.get(own, 0.0) - scale * a * tot[own]
                for d, x in to.items():
                    g = x - scale * a * tot[d]
                    if g > best_g + 1e-15:
                        best, best_g = d, g
                if best_g < -1e-15 and tot[own] > 0:  # better alone: an empty community (the lowest free label)
                    best = next(c for c in range(nn) if tot[c] == 0 and c != own) if any(t == 0 for t in tot) else own
                if level > 0 and best == own and size[own] == 1:
                    ties = [d for d, x in to.items() if d != own and x - scale * a * tot[d] == 0.0]
                    best = min(ties) if ties else own
                comm[v] = best
                tot[best] += a
                size[own] -= 1
                size[best] += 1
                moved += best != own
            moved_any |= moved > 0
            if not moved:
                break
        if not moved_any:
            break
        labels = {c: i for i, c in enumerate(sorted(set(comm)))}
        comm = [labels[c] for c in comm]
        k = len(labels)
        new_adj = [dict() for _ in range(k)]
        new_mass = [0.0] * k
        for v in range(nn):
            new_mass[comm[v]] += mass[v]
            for u, x in adj[v].items():
                new_adj[comm[v]][comm[u]] = new_adj[comm[v]].get(comm[u], 0.0) + x
        member = np.asarray(comm)[member]
        adj, mass = new_adj, new_mass
        if k == nn:
            break
    return member


QUALITY_CASES = {
    "hardA": lambda: uniform_blocks(600, 6, 0.06, 0.03, 11),
    "hardB": lambda: uniform_blocks(400, 8, 0.10, 0.04, 12),
    "er": lambda: uniform_blocks(300, 1, 0.05, 0.05, 13),
}
# (algo, resolution) each quality case runs at
QUALITY_RUNS = [("RBConfigurationVertexPartition", 1.0), ("RBConfigurationVertexPartition", 2.0), ("RBERVertexPartition", 1.0),
                ("CPMVertexPartition", 1.0)]
PLANTED_CASES = {
    "p600": lambda: planted(600, 12, 0.5, 0.02, 21),
    "p300": lambda: planted(300, 30, 0.9, 0.01, 22),
    "p2000": lambda: planted(2000, 40, 0.4, 0.005, 23),
}


# ------------------------------------------------------------------------------------------------ trace cases
# The graphs whose every proposal pass is pinned (tests/leiden_model.py, tests/golden/leiden_trace.json).  All weights are
# k / 1024 with k an integer in [1, 4096]: every float64 sum of them is exact in any order and so is their fixed-point
# form, so the total weight of the model cannot differ from the device's.
def _grid_weights(rng, count, lo=1, hi=4096):
    return rng.integers(lo, hi + 1, size=count).astype(np.float64) / 1024.0


def _from_arrays(r, c, w, n):
    r, c = np.asarray(r, dtype=np.int64), np.asarray(c, dtype=np.int64)
    lo, hi = np.minimum(r, c), np.maximum(r, c)
    order = np.lexsort((hi, lo))
    assert len(np.unique(lo * n + hi)) == len(lo) and (lo < hi).all(), "a duplicate pair or a self-loop"
    return lo[order].astype(np.uint32), hi[order].astype(np.uint32), np.asarray(w, dtype=np.float32)[order], int(n)


def trace_dense(n=300, groups=3, p_in=0.9, p_out=0.45, seed=32):
    """Every node of the planted part has a degree between the two work-unit limits, with many edges to every label; node
    n has exactly 64 neighbours and node n + 1 exactly 65 (the boundary of the one-wave unit, on tables that accumulate)."""
    rng = np.random.default_rng(seed)
    r, c = np.triu_indices(n, 1)
    same = (r % groups) == (c % groups)
    keep = rng.random(len(r)) < np.where(same, p_in, p_out)
    r, c = r[keep], c[keep]
    w = _grid_weights(rng, len(r))
    extra_r, extra_c = [], []
    for node, degree in ((n, 64), (n + 1, 65)):
        extra_r.append(np.sort(rng.choice(n, size=degree, replace=False)))
        extra_c.append(np.full(degree, node))
    r, c = np.concatenate([r] + extra_r), np.concatenate([c] + extra_c)
    w = np.concatenate([w, _grid_weights(rng, 64 + 65)])
    return _from_arrays(r, c, w, n + 2)


def trace_wide(clusters=3, cliques=90, seed=32, bridges=40):
    """clusters x cliques four-cliques; inside a cluster one weak edge between each pair of cliques, between clusters a
    few weak edges.  Level 0 stays in the one-wave unit; the aggregate of the cliques has cliques - 1 neighbours and a
    self-loop entry."""
    rng = np.random.default_rng(seed)
    r, c, w = [], [], []
    n = clusters * cliques * 4
    for q in range(clusters * cliques):
        for a, b in clique_pairs(range(4 * q, 4 * q + 4)):
            r.append(a), c.append(b), w.append(int(rng.integers(3072, 4097)))
    for cl in range(clusters):
        base = cl * cliques
        for a in range(cliques):
            for b in range(a + 1, cliques):
                r.append(4 * (base + a) + int(rng.integers(4))), c.append(4 * (base + b) + int(rng.integers(4)))
                w.append(int(rng.integers(1, 513)))
    seen = set()
    while len(seen) < bridges:
        a, b = int(rng.integers(n)), int(rng.integers(n))
        if a // (4 * cliques) != b // (4 * cliques) and (min(a, b), max(a, b)) not in seen:
            seen.add((min(a, b), max(a, b)))
    for a, b in sorted(seen):
        r.append(a), c.append(b), w.append(int(rng.integers(1, 65)))
    return _from_arrays(r, c, np.asarray(w, dtype=np.float64) / 1024.0, n)


def trace_hubs(groups=6, per=400, hubs=12, p_in=0.03, p_out=0.002, cover=0.9, magnet=24, seed=33, exact=(2048, 2049)):
    """groups x per sparse nodes in planted groups (contiguous blocks of `per`), `hubs` hubs, each tied to about `cover` of
    the sparse nodes by weights up to 0.5, and a magnet: the last `magnet` sparse nodes, a heavy clique with no other
    sparse neighbour, to which every hub is tied by weights in (2, 3].  One edge of each hub weighs the full 4.0 (its
    decoy): the hub first joins that neighbour and moves again when the magnet has gathered, so the sums of its table
    decide a move.  The magnet's labels are the largest in use and every hub's last CSR entry is a magnet node.  The first
    len(exact) hubs have exactly those degrees: the boundary of the LDS-table unit, on tables that accumulate."""
    rng = np.random.default_rng(seed)
    n_s = groups * per
    rest = n_s - magnet
    r, c = np.triu_indices(rest, 1)
    same = (r // per) == (c // per)
    keep = rng.random(len(r)) < np.where(same, p_in, p_out)
    r, c = r[keep], c[keep]
    w = np.where(same[keep], rng.integers(2048, 4097, size=len(r)), rng.integers(1, 1025, size=len(r)))
    mr, mc = np.triu_indices(magnet, 1)
    rs, cs, ws = [r, rest + mr], [c, rest + mc], [w, rng.integers(3072, 4097, size=len(mr))]
    for h in range(hubs):
        degree = exact[h] if h < len(exact) else int(rng.binomial(rest, cover)) + magnet
        nb = np.concatenate([np.sort(rng.choice(rest, size=degree - magnet, replace=False)), np.arange(rest, n_s)])
        wh = np.concatenate([rng.integers(1, 513, size=degree - magnet), rng.integers(2049, 3073, size=magnet)])
        wh[int(rng.integers(degree - magnet))] = 4096
        rs.append(nb), cs.append(np.full(degree, n_s + h)), ws.append(wh)
    return _from_arrays(np.concatenate(rs), np.concatenate(cs), np.concatenate(ws).astype(np.float64) / 1024.0, n_s + hubs)


def trace_many_hubs(hubs=520, leaves=2200, degree=2100, groups=4, seed=34):
    """`hubs` nodes of degree `degree` > 2 048 over `leaves` leaves: more nodes of the device-memory unit than it has
    tables, so every workgroup takes several and clears its table between them.  A hub's edges into its own group
    (h % groups; leaf v: v % groups) are heavy, the others light."""
    rng = np.random.default_rng(seed)
    rs, cs, ws = [], [], []
    for h in range(hubs):
        nb = np.sort(rng.choice(leaves, size=degree, replace=False))
        mine = (nb % groups) == (h % groups)
        rs.append(nb), cs.append(np.full(degree, leaves + h))
        ws.append(np.where(mine, rng.integers(2048, 4097, size=degree), rng.integers(1, 513, size=degree)).astype(np.float64) / 1024.0)
    return _from_arrays(np.concatenate(rs), np.concatenate(cs), np.concatenate(ws), leaves + hubs)


def trace_pairs_glb(pairs=2100, groups=3, seed=35):
    """`pairs` strongly tied pairs and one weak edge between every two pairs — heavier inside a planted group (contiguous
    blocks of pairs, so that the last group holds the largest labels).  No node of level 0 has more than 2 048 entries; every aggregate of a pair has pairs - 1 neighbours and
    a self-loop entry: the single reserved table of the device-memory unit."""
    rng = np.random.default_rng(seed)
    a, b = np.triu_indices(pairs, 1)
    per = -(-pairs // groups)
    same = (a // per) == (b // per)
    r, c = 2 * a + rng.integers(0, 2, size=len(a)), 2 * b + rng.integers(0, 2, size=len(a))
    w = np.where(same, rng.integers(8, 17, size=len(a)), rng.integers(1, 5, size=len(a)))
    p = np.arange(pairs)
    r, c = np.concatenate([2 * p, r]), np.concatenate([2 * p + 1, c])
    w = np.concatenate([np.full(pairs, 4096), w]).astype(np.float64) / 1024.0
    return _from_arrays(r, c, w, 2 * pairs)


TRACE_CASES = {"dense": trace_dense, "wide": trace_wide, "hubs": trace_hubs, "many_hubs": trace_many_hubs, "pairs_glb": trace_pairs_glb}
TRACE_SMALL = ("dense", "wide", "hubs")  # rerun by the CPU tests; the other two are only pinned
# the work unit each case is there for: (fault limit, "blk" or "glb", the 0-based level it must be reached and matter at)
TRACE_ROUTES = {"dense": (64, "blk", 0), "wide": (64, "blk", 1), "hubs": (2048, "glb", 0), "many_hubs": (2048, "glb", 0),
                "pairs_glb": (2048, "glb", 1)}
# (algo, resolution) each trace case runs at; the smallest also under the other two functions, CPM at a resolution where
# something moves (weights reach 4)
TRACE_RUNS = {name: [("RBConfigurationVertexPartition", 1.0), ("RBERVertexPartition", 1.0)] for name in TRACE_CASES}
TRACE_RUNS["dense"] = TRACE_RUNS["dense"] + [("ModularityVertexPartition", 1.0), ("CPMVertexPartition", 1.5)]
