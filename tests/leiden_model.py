"""A sequential model of skr_leiden (seekr_amd/csrc/leiden.hip) in numpy: no GPU, no tolerance.

Every sum that decides a move on the device is an int64 sum of fixed-point weights, every gain is one float64 expression
compiled without contraction, and the one float64 sum of a sweep (the penalty) has a written-down order.  So the host
loop can be followed statement by statement and must give the same bits: the same proposal of every node in every pass,
the same quality of every sweep, the same membership.  `model` returns the trace skr_leiden_trace records, in the same
words; tests/golden/leiden_trace.json pins it and tests/test_gpu_leiden_trace.py compares the device with the pins.

The integer sums are taken in int64 (the device's own width; (2 m + 2) 2^frac < 2^60 keeps every one of them exact), a
whole pass at a time: sorted (node, label) keys stand for the hash tables.  `fault` spoils the tables of the nodes above
a degree limit — here only, to show that a case can tell a wrong table from a right one."""
import hashlib
import math

import numpy as np

import leiden_cases as lc

NONE = 0xFFFFFFFF
WAVE_DEG, LDS_DEG = 64, 2048  # skr_leiden_limits
SUBSET_TRIES = 4
PROPOSE, REFINE, SWEEP = 1, 2, 3
KIND_NAMES = {PROPOSE: "propose", REFINE: "refine", SWEEP: "sweep"}
_FNV_OFFSET, _FNV_PRIME, _M64 = 0xcbf29ce484222325, 0x100000001b3, (1 << 64) - 1


def fnv1a(data):
    """FNV-1a 64 of the bytes of `data` (bytes, or an array: its bytes as they lie in memory)."""
    if isinstance(data, np.ndarray):
        data = np.ascontiguousarray(data).tobytes()
    h = _FNV_OFFSET
    for b in data:
        h = ((h ^ b) * _FNV_PRIME) & _M64
    return h


def graph_hash(graph):
    """What tells "the case changed" from "the device differs": FNV-1a of the SHA-256 digest of the bytes of rows, cols and
    vals (the byte loop above would take seconds on the two large cases, in every test that checks it)."""
    rows, cols, vals, n = graph
    digest = hashlib.sha256(np.asarray(rows, "<u4").tobytes() + np.asarray(cols, "<u4").tobytes() + np.asarray(vals, "<f4").tobytes()).digest()
    return fnv1a(digest)


# ------------------------------------------------------------------------------------------------ det_sum
_LANES = np.arange(64)


def _block_sum(s):
    """block_sum of leiden.hip for rows of 256 thread values: the xor-shuffle tree over the 64 lanes of each wave (what
    lane 0 ends with), then (l0 + l1) + (l2 + l3)."""
    v = s.reshape(-1, 4, 64)
    for off in (32, 16, 8, 4, 2, 1):
        v = v + v[:, :, _LANES ^ off]
    l = v[:, :, 0]
    return (l[:, 0] + l[:, 1]) + (l[:, 2] + l[:, 3])


def det_sum(x):
    """The float64 sum of x in det_sum's order: 4 096 terms to a workgroup, 16 consecutive terms per thread added in
    sequence, the tree; the workgroup sums by thread i taking i, i + 256, ... in sequence, the tree."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    nb = max(1, -(-len(x) // 4096))
    t = np.zeros(nb * 4096)
    t[:len(x)] = x
    t = t.reshape(nb, 256, 16)
    s = np.zeros((nb, 256))
    for j in range(16):
        s = s + t[:, :, j]
    part = _block_sum(s)
    k = -(-nb // 256)
    p = np.zeros(k * 256)
    p[:nb] = part
    p = p.reshape(k, 256)
    s = np.zeros(256)
    for i in range(k):
        s = s + p[i]
    return float(_block_sum(s)[0])


# ------------------------------------------------------------------------------------------------ pieces
def _offsets(src, n):
    return np.concatenate([[0], np.cumsum(np.bincount(src, minlength=n))]).astype(np.int64)


def _dense(used):
    """Exclusive scan of a 0/1 array: the dense id of every label in use, and how many are."""
    c = np.cumsum(used.astype(np.int64))
    return c - used, int(c[-1]) if len(c) else 0


def chosen(v, tries, salt, only):
    """Which nodes of the array v a sweep applies: all (tries == 0), a hashed 1 / 2^tries of them, or `only`."""
    v = np.asarray(v, dtype=np.uint64)
    if tries > SUBSET_TRIES:
        return v == np.uint64(only)
    h = (((v ^ np.uint64(salt)) * np.uint64(2246822519)) & np.uint64(0xFFFFFFFF)) >> np.uint64(11)  # wraps mod 2^64: the low 32 bits hold
    return (h & np.uint64((1 << tries) - 1)) == 0


class _Level:
    def __init__(self, n, src, dst, w, mass):
        self.n, self.src, self.dst, self.w, self.mass = n, src, dst, w, mass
        self.offs = _offsets(src, n)
        self.deg = np.diff(self.offs)
        self.n_blk = int(((self.deg > WAVE_DEG) & (self.deg <= LDS_DEG)).sum())
        self.n_glb = int((self.deg > LDS_DEG).sum())


def _propose(L, K, label, tot, cnt, bound, refine, ties, fault):
    """node_propose for every node of the level.  K: (wscale, mscale, gp).  Returns prop (uint32), pgain (float64; None in
    refinement) and target (uint32; None in local moving)."""
    n, src, dst, w = L.n, L.src, L.dst, L.w
    wscale, mscale, gp = K
    nodes = np.arange(n, dtype=np.int64)
    own = label
    own_cnt = cnt[own]
    use = dst != src  # the self-loop entry
    if refine:
        use &= bound[dst] == bound[src]
        use &= (own_cnt == 1)[src]  # no longer single: stays where it is
    big = None
    if fault is not None:
        big = L.deg > fault[1]
        if fault[0] == "drop_last":
            use[L.offs[1:][big] - 1] = False
    s, l, ww = src[use], label[dst[use]], w[use]
    if not refine:  # the own label is in the table, with weight 0
        s, l, ww = np.concatenate([s, nodes]), np.concatenate([l, own]), np.concatenate([ww, np.zeros(n, np.int64)])
    span = 2 * n
    key = s * span + l
    order = np.argsort(key, kind="stable")
    key, ww = key[order], ww[order]
    if len(key):
        head = np.flatnonzero(np.concatenate([[True], key[1:] != key[:-1]]))
        tw = np.add.reduceat(ww, head)
        tv, tl = key[head] // span, key[head] % span
    else:
        tw = tv = tl = np.zeros(0, np.int64)
    if fault is not None and fault[0] == "lose_key":
        idx = np.flatnonzero((tl != own[tv]) & big[tv])  # foreign keys of the spoilt nodes, ascending within a node
        if len(idx):
            last = idx[np.concatenate([tv[idx][1:] != tv[idx][:-1], [True]])]
            keep = np.ones(len(tv), bool)
            keep[last] = False
            tw, tv, tl = tw[keep], tv[keep], tl[keep]
    a = L.mass.astype(np.float64) * mscale
    mine = tl == own[tv]
    if refine:
        g_stay = np.zeros(n)
    else:
        w_own = np.zeros(n, np.int64)
        w_own[tv[mine]] = tw[mine]
        g_stay = w_own.astype(np.float64) * wscale - gp * a * ((tot[own] - L.mass).astype(np.float64) * mscale)
    cand = ~mine & ~((own_cnt[tv] == 1) & (cnt[tl] == 1) & (tl > own[tv]))  # single into single only toward the smaller id
    cv, cl = tv[cand], tl[cand]
    cg = tw[cand].astype(np.float64) * wscale - gp * a[cv] * (tot[cl].astype(np.float64) * mscale)
    if not refine:  # the node's own empty community: worth 0
        ev = np.flatnonzero((own_cnt > 1) & (cnt[n + nodes] == 0))
        cv, cl, cg = np.concatenate([cv, ev]), np.concatenate([cl, n + ev]), np.concatenate([cg, np.zeros(len(ev))])
    best_g, best_l = np.full(n, -np.inf), np.full(n, NONE, np.int64)
    if len(cv):
        order = np.lexsort((cl, -cg, cv))  # larger g first, then the smaller label
        cv, cl, cg = cv[order], cl[order], cg[order]
        first = np.flatnonzero(np.concatenate([[True], cv[1:] != cv[:-1]]))
        best_g[cv[first]], best_l[cv[first]] = cg[first], cl[first]
    has = best_l != NONE
    if refine:
        go = has & (best_g >= 0.0)
    else:
        tie = (own_cnt == 1) & (best_g == g_stay) if ties else np.zeros(n, bool)
        go = has & ((best_g > g_stay) | tie)
    prop = np.where(go, best_l, NONE).astype(np.uint32)
    if not refine:
        return prop, np.where(go, np.where(go, best_g, 0.0) - g_stay, 0.0), None
    target = np.zeros(n, np.uint32)
    hit = go & (cnt[np.where(go, best_l, 0)] == 1)
    target[best_l[hit]] = 1
    return prop, None, target


def _totals(label, mass, n):
    tot, cnt = np.zeros(2 * n, np.int64), np.zeros(2 * n, np.int64)
    np.add.at(tot, label, mass)
    np.add.at(cnt, label, 1)
    return tot, cnt


def _measure(L, K, pen_half, by_count, label, tot, cnt):
    wscale, mscale, _ = K
    inner2 = int(L.w[label[L.src] == label[L.dst]].sum())
    A = tot.astype(np.float64) * mscale
    pen = det_sum(A * (A - 1.0) if by_count else A * A)
    return float(inner2) * wscale * 0.5 - pen_half * pen, int(np.count_nonzero(cnt))


# ------------------------------------------------------------------------------------------------ the model
def model(rows, cols, vals, n, quality, resolution=1.0, max_levels=32, max_sweeps=64, fault=None, keep=None):
    """(membership int32 [n], info, trace) as seekr_amd.leiden.communities(..., trace=True) gives them, the reported
    quality apart (leiden_cases.quality computes it).  quality: the name or the id.  fault: ("drop_last", limit) skips the
    last CSR entry of every node with more than `limit` entries; ("lose_key", limit) removes the largest foreign key of
    such a node's table.  keep = k: info["trace_arrays"] holds the two arrays of record k."""
    q = lc.ALGOS[quality] if isinstance(quality, str) else int(quality)
    n0 = int(n)
    rows, cols = np.asarray(rows, dtype=np.int64).reshape(-1), np.asarray(cols, dtype=np.int64).reshape(-1)
    vals = np.asarray(vals, dtype=np.float32).reshape(-1)
    trace = []
    info = {"n_communities": n0, "levels": 0, "sweeps": 0, "converged": True}
    if n0 == 0 or len(rows) == 0:
        return np.arange(n0, dtype=np.int32), info, trace
    gamma = 1.0 if q == 1 else float(resolution)
    m_total = det_sum(vals.astype(np.float64))
    frac = min(40, 60 - int(math.ceil(math.log2(2.0 * m_total + 2.0))))
    wfx = np.rint(vals.astype(np.float64) * math.ldexp(1.0, frac)).astype(np.int64)
    src, dst, w = np.concatenate([rows, cols]), np.concatenate([cols, rows]), np.concatenate([wfx, wfx])
    order = np.lexsort((dst, src))
    src, dst, w = src[order], dst[order], w[order]
    if q >= 2:
        mass = np.ones(n0, np.int64)
    else:
        mass = np.zeros(n0, np.int64)
        np.add.at(mass, src, w)
    wscale = math.ldexp(1.0, -frac)
    mscale = 1.0 if q >= 2 else wscale
    p_er = m_total / (float(n0) * float(n0 - 1) / 2.0)
    gp = gamma / (2.0 * m_total) if q <= 1 else (gamma * p_er if q == 2 else gamma)
    K = (wscale, mscale, gp)
    pen_half = 0.5 * gp
    by_count = q >= 2

    def record(kind, head, a, b, tail=None):
        if keep is not None and len(trace) == keep:
            info["trace_arrays"] = (a.copy(), b.copy())
        rec = (kind,) + head + (fnv1a(a), fnv1a(b))
        trace.append(rec if tail is None else rec + (tail,))

    L = _Level(n0, src, dst, w, mass)
    comm = np.arange(n0, dtype=np.int64)
    map0 = np.arange(n0, dtype=np.int64)
    converged, all_single = True, False
    levels = sweeps_run = 0
    part = None
    while True:
        # ---- local moving
        tot, cnt = _totals(comm, L.mass, L.n)
        q_cur, used_cur = _measure(L, K, pen_half, by_count, comm, tot, cnt)
        levels += 1
        head = (levels - 1, L.n, L.n_blk, L.n_glb)
        tries, proposed, quiet = 0, False, False
        nodes = np.arange(L.n, dtype=np.int64)
        for sweep in range(max_sweeps):
            if not proposed:
                prop, pgain, _ = _propose(L, K, comm, tot, cnt, None, False, levels > 1, fault)
                proposed = True
                record(PROPOSE, head, prop.astype("<u4"), pgain.astype("<f8"))
            only = NONE
            if tries > SUBSET_TRIES:  # the largest gain; ties: the smallest node
                wants = np.flatnonzero(prop != NONE)
                if len(wants):
                    bits = pgain[wants].view(np.uint64)
                    only = int(wants[bits == bits.max()].min())
            salt = (sweep * 0x9E3779B9) & 0xFFFFFFFF
            move = (prop != NONE) & chosen(nodes, tries, salt, only)
            comm_try = np.where(move, prop.astype(np.int64), comm)
            moves = int(move.sum())
            tot_try, cnt_try = _totals(comm_try, L.mass, L.n)
            sweeps_run += 1
            q_try, used_try = _measure(L, K, pen_half, by_count, comm_try, tot_try, cnt_try)
            kept = moves > 0 and (q_try > q_cur or (q_try == q_cur and used_try < used_cur))
            trace.append((SWEEP, levels - 1, tries, moves, int(np.float64(q_try).view(np.uint64)), used_try, int(kept)))
            if moves == 0 and tries == 0:
                quiet = True
                break
            if kept:
                comm, tot, cnt, q_cur, used_cur = comm_try, tot_try, cnt_try, q_try, used_try
                tries = max(0, min(tries, SUBSET_TRIES) - 1)
                proposed = False
            elif tries > SUBSET_TRIES:
                quiet = True
                break
            else:
                tries += 1
        if not quiet:
            converged = False
        used = np.zeros(2 * L.n, bool)
        used[comm] = True
        cid, n_comm = _dense(used)
        all_single = n_comm == L.n
        if all_single:
            break
        # ---- refinement
        part = np.arange(L.n, dtype=np.int64)
        ptot, pcnt = L.mass.copy(), np.ones(L.n, np.int64)
        for _ in range(max_sweeps):
            rprop, _, target = _propose(L, K, part, ptot, pcnt, comm, True, False, fault)
            go = (rprop != NONE) & (target == 0)  # somebody's target stays
            to = rprop[go].astype(np.int64)
            part[go] = to
            np.add.at(ptot, to, L.mass[go])  # the totals of the part that was left are not lowered
            np.add.at(pcnt, to, 1)
            moved = int(go.sum())
            record(REFINE, head, rprop.astype("<u4"), target.astype("<u4"), moved)
            if moved == 0:
                break
        if levels >= max_levels:
            converged = False
            break
        # ---- aggregation
        used = np.zeros(L.n, bool)
        used[part] = True
        newid, n_new = _dense(used)
        if n_new >= L.n:
            converged = False
            break
        pid = newid[part]
        mass_new = np.zeros(n_new, np.int64)
        np.add.at(mass_new, pid, L.mass)
        comm_new = np.zeros(n_new, np.int64)
        comm_new[pid] = cid[comm]
        map0 = pid[map0]
        key = (pid[L.src] << 32) | pid[L.dst]
        order = np.argsort(key, kind="stable")
        key, ww = key[order], L.w[order]
        first = np.flatnonzero(np.concatenate([[True], key[1:] != key[:-1]]))
        L = _Level(n_new, key[first] >> 32, key[first] & 0xFFFFFFFF, np.add.reduceat(ww, first), mass_new)
        comm = comm_new
    # ---- the answer: by size, then by the smallest node
    lab0 = (comm if all_single else part)[map0]
    labels, inv = np.unique(lab0, return_inverse=True)
    size = np.bincount(inv)
    first = np.full(len(labels), n0, np.int64)
    np.minimum.at(first, inv, np.arange(n0))
    rank = np.empty(len(labels), np.int64)
    rank[np.lexsort((first, -size))] = np.arange(len(labels))
    info.update(n_communities=len(labels), levels=levels, sweeps=sweeps_run, converged=converged)
    return rank[inv].astype(np.int32), info, trace


# ------------------------------------------------------------------------------------------------ what a case is worth
def route_records(trace, route, level):
    """The indices of the proposal records (local moving and refinement) of `level` at which the work unit `route` ("blk":
    one workgroup, LDS table; "glb": table in device memory) had nodes."""
    at = 3 if route == "blk" else 4
    return [k for k, r in enumerate(trace) if r[0] in (PROPOSE, REFINE) and r[1] == level and r[at] > 0]


def first_fault_record(trace, spoilt, route, level):
    """The first record of `route` and `level` that an injected fault changed (None: the case cannot see that fault).  Only
    records up to the first difference of any kind count: after it the two runs are no longer in the same state."""
    for k, (a, b) in enumerate(zip(trace, spoilt)):
        if a != b:
            return k if k in route_records(trace, route, level) and a[:5] == b[:5] else None
    return None


def first_differing_node(a, b):
    """The first node at which two arrays of a record differ bit for bit (None: they are the same; -1: other lengths)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype.itemsize != b.dtype.itemsize:
        return -1
    bad = np.flatnonzero((a.view(np.uint8).reshape(len(a), -1) != b.view(np.uint8).reshape(len(b), -1)).any(axis=1))
    return int(bad[0]) if len(bad) else None
