"""Leiden communities of an edge list on MI355X (skr_leiden): the step kmer_leiden.py:131-146 of the reference hands to
leidenalg.find_partition.  The reference draws a random visiting order (setseed=False is its default), so there are no
bits of leidenalg to match: the result here is the same on every run, every community is connected, its quality is
measured against a sequential Louvain (tests/leiden_cases.py), and every proposal pass is compared with the project's own
sequential model (tests/leiden_model.py) through the trace below.  DESIGN_PARITY.md lists the quality functions.
"""
import ctypes as C

import numpy as np

from seekr_amd import _lib

ALGOS = {"RBConfigurationVertexPartition": 0, "ModularityVertexPartition": 1, "RBERVertexPartition": 2, "CPMVertexPartition": 3}
NOT_BUILT = ("SurpriseVertexPartition", "SignificanceVertexPartition")


def algo_code(algo):
    """The `quality` id of skr_leiden; NotImplementedError for the two functions that are not built."""
    if algo in NOT_BUILT:
        raise NotImplementedError("{} is not built on the device (nor is {}); use one of {}".format(
            algo, [a for a in NOT_BUILT if a != algo][0], ", ".join(sorted(ALGOS))))
    if algo not in ALGOS:
        raise ValueError("unknown algo {!r}; one of {}".format(algo, ", ".join(sorted(ALGOS))))
    return ALGOS[algo]


def limits():
    """(wave_degree, lds_degree): the largest degree the one-wave-per-node and the LDS-table work units take, as the
    library reports them (skr_leiden_limits)."""
    a, b = C.c_int(0), C.c_int(0)
    _lib.check(_lib.lib().skr_leiden_limits(C.byref(a), C.byref(b)))
    return a.value, b.value


def table_groups(ctx=None):
    """How many nodes the device-memory work unit handles at once on `ctx` (skr_leiden_table_groups)."""
    g = C.c_int(0)
    _lib.check(_lib.lib().skr_leiden_table_groups((ctx or _lib.default_context())._h, C.byref(g)))
    return g.value


def _column(ctx, x, dtype):
    """A device column of `dtype`: device matrices pass through, anything else is uploaded.  Returns (matrix, owned)."""
    if isinstance(x, _lib.Matrix):
        if x.dtype != np.dtype(dtype):
            raise TypeError("device edge lists are uint32, uint32, float32 (got {})".format(x.dtype))
        return x, False
    a = np.ascontiguousarray(x).reshape(-1)
    if np.dtype(dtype) == np.uint32 and len(a) and (a.min() < 0 or a.max() > 0xFFFFFFFF):
        raise ValueError("node indices must fit 32 bits and be >= 0")
    a = a.astype(dtype, copy=False)
    m = ctx.empty(max(len(a), 1), 1, dtype)
    if len(a):
        m.upload(a.reshape(-1, 1))
    return m, True


TRACE_WORDS = 8
# how many words of a record mean something, by kind (include/seekr_hip.h lists them)
_TRACE_USED = {1: 7, 2: 8, 3: 7}


def _read_trace():
    """(records, dump) of the calling thread's trace: a list of tuples of ints, and the two arrays of the dumped record
    as raw bytes (b"" where none was kept)."""
    lib = _lib.lib()
    words = C.c_int64(0)
    _lib.check(lib.skr_leiden_trace_read(None, 0, C.byref(words)))
    buf = np.zeros(max(words.value, 1), np.uint64)
    _lib.check(lib.skr_leiden_trace_read(buf.ctypes.data, words.value, C.byref(words)))
    recs = buf[:words.value].reshape(-1, TRACE_WORDS)
    records = [tuple(int(x) for x in r[:_TRACE_USED.get(int(r[0]), TRACE_WORDS)]) for r in recs]
    na, nb = C.c_int64(0), C.c_int64(0)
    _lib.check(lib.skr_leiden_trace_dump(None, 0, None, 0, C.byref(na), C.byref(nb)))
    a, b = np.zeros(max(na.value, 1), np.uint8), np.zeros(max(nb.value, 1), np.uint8)
    _lib.check(lib.skr_leiden_trace_dump(a.ctypes.data, na.value, b.ctypes.data, nb.value, C.byref(na), C.byref(nb)))
    return records, (a[:na.value].tobytes(), b[:nb.value].tobytes())


@_lib.api_call
def communities(rows, cols, vals, n_nodes, algo="RBERVertexPartition", rs=1.0, max_levels=32, max_sweeps=64, n_edges=None, trace=False,
                trace_dump=None):
    """(membership int32 [n_nodes], quality float, info dict) of the undirected weighted graph given as the
    upper-triangle list pearson_edges(..., upper_only=True) returns: row < col, weight > 0, any order, no duplicates;
    numpy arrays (uploaded) or device matrices (`n_edges`: how many of their cells are the list; default all).
    Communities are numbered by size, largest first, ties to the community holding the smallest node.  `quality` is the
    function `algo` names (RBConfigurationVertexPartition, ModularityVertexPartition, RBERVertexPartition,
    CPMVertexPartition) for the returned membership; `rs` is its resolution (ignored by ModularityVertexPartition).
    info: n_communities, levels, sweeps, converged (False when max_levels or max_sweeps ended the run).
    `trace` (for tests; off, nothing extra runs): info["trace"] is the list of records skr_leiden_trace describes, one
    tuple per proposal pass ("propose": 1, level, nodes, n_blk, n_glb, hash of prop, hash of the gains), refinement round
    (2, level, nodes, n_blk, n_glb, hash of prop, hash of target, moved) and sweep (3, level, tries, moves, quality bits,
    labels in use, kept).  `trace_dump` = k also gives info["trace_arrays"]: prop (uint32) and the gains (float64) or
    target (uint32) of record k, whole."""
    code = algo_code(algo)
    ctx = _lib.default_context()
    for x in (rows, cols, vals):
        if isinstance(x, _lib.Matrix):
            ctx = x.ctx
    owned = []
    try:
        mats = []
        for x, dt in ((rows, np.uint32), (cols, np.uint32), (vals, np.float32)):
            m, own = _column(ctx, x, dt)
            mats.append(m)
            if own:
                owned.append(m)
        if n_edges is None:
            n_edges = 0 if not isinstance(rows, _lib.Matrix) and np.size(rows) == 0 else mats[0].rows * mats[0].cols
        n_nodes = int(n_nodes)
        mem = ctx.empty(max(n_nodes, 1), 1, np.uint32)
        owned.append(mem)
        q, nc, lv = C.c_double(0), C.c_int64(0), C.c_int64(0)
        tracing = bool(trace) or trace_dump is not None
        records = dump = None
        if tracing:
            _lib.check(_lib.lib().skr_leiden_trace(1, -1 if trace_dump is None else int(trace_dump)))
        try:
            _lib.check(_lib.lib().skr_leiden(ctx._h, mats[0]._h, mats[1]._h, mats[2]._h, int(n_edges), n_nodes, code, C.c_double(float(rs)),
                                             int(max_levels), int(max_sweeps), mem._h, C.byref(q), C.byref(nc), C.byref(lv)))
            if tracing:
                records, dump = _read_trace()
        finally:
            if tracing:
                _lib.check(_lib.lib().skr_leiden_trace(0, -1))
        conv, sweeps = C.c_int(1), C.c_int64(0)
        _lib.check(_lib.lib().skr_leiden_last(C.byref(conv), C.byref(sweeps)))
        membership = mem.to_numpy(0, n_nodes).reshape(-1).view(np.int32).copy() if n_nodes else np.empty(0, np.int32)
    finally:
        for m in owned:
            m.free()
    info = {"n_communities": nc.value, "levels": lv.value, "sweeps": sweeps.value, "converged": bool(conv.value)}
    if tracing:
        info["trace"] = records
        if trace_dump is not None:
            kind = records[int(trace_dump)][0] if 0 <= int(trace_dump) < len(records) else 0
            info["trace_arrays"] = (np.frombuffer(dump[0], np.uint32).copy(), np.frombuffer(dump[1], np.float64 if kind == 1 else np.uint32).copy())
    return membership, q.value, info


def pearson_communities(z, cutoff=0.0, algo="RBERVertexPartition", rs=1.0, max_levels=32, max_sweeps=64, knn=None, knn_mode="union",
                        **kw):
    """communities() of the thresholded self-comparison of the prepared operand `z` (seekr_amd._lib.Operand): edge
    {i, j} weighs r[i, j] where !(r < cutoff), r > 0 and i != j (kmer_leiden.py:94-96, 106-107).  r never stands whole:
    consumers.pearson_edges reduces it to the edge list stripe by stripe.  That function hands the list back in host
    memory (each stripe's edges are downloaded as they are found), so here the finished list is UPLOADED once for
    skr_leiden — it does not stay on the device between the two steps.  `kw`: stripe_rows, fuse of pearson_edges.
    knn=K: the k-nearest-neighbour graph replaces the thresholded one (reciprocal.knn_graph: {u, v} is an edge when v is
    among u's K nearest or — knn_mode "mutual": and — u among v's, and r > 0; at most N K edges); `cutoff` must then be
    at its default, else ValueError, and `kw` is the sweep's stripe_rows, panel_rows.
    Returns (membership, quality, info) with info["n_edges"] added."""
    from seekr_amd import consumers
    algo_code(algo)
    if knn is not None:
        from seekr_amd import reciprocal
        if float(cutoff) != 0:
            raise ValueError("give knn or a non-zero cutoff, not both (knn={!r}, cutoff={!r})".format(knn, cutoff))
        rows, cols, vals = reciprocal.knn_graph(z, knn, mode=knn_mode, **kw)
    else:
        rows, cols, vals = consumers.pearson_edges(z, cutoff, upper_only=True, **kw)
    keep = vals > 0  # a negative cutoff keeps negative cells and NaN passes the mask: neither is an edge weight
    if not keep.all():
        rows, cols, vals = rows[keep], cols[keep], vals[keep]
    membership, quality, info = communities(rows.astype(np.uint32), cols.astype(np.uint32), vals.astype(np.float32), z.rows, algo=algo,
                                            rs=rs, max_levels=max_levels, max_sweeps=max_sweeps)
    info["n_edges"] = int(len(vals))
    info["edges"] = (rows, cols, vals)
    return membership, quality, info
