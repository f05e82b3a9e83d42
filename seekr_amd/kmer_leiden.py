"""kmer_leiden of the reference (kmer_leiden.py:66-346) on MI355X: count, correlate, threshold and partition on the device.

Differences, all listed in DESIGN_PARITY.md: the partition is always reproducible (`setseed` is accepted and changes
nothing); edge {i, j} weighs r[i, j]; the membership is returned (the reference returns nothing); the plot is not built
(`plotname` other than None raises NotImplementedError — write `csvfile` and plot from it); `edges="nonzero"` writes
only the kept edges where the reference writes every upper-triangle cell."""
import csv

import numpy as np

from seekr_amd import _lib, leiden
from seekr_amd import pearson as pearson_mod
from seekr_amd.fasta_reader import Reader
from seekr_amd.kmer_counts import BasicCounter

ALL_EDGES_LIMIT = 10 ** 8  # upper-triangle cells edges="all" writes at most


def write_nodes_csv(path, names, membership):
    """`Id,Label,Color`: community by community (0, 1, ...), nodes ascending within each; Color = community + 1
    (kmer_leiden.py:325-335)."""
    membership = np.asarray(membership)
    order = np.lexsort((np.arange(len(membership)), membership))
    with open(path, "w", newline="") as f:
        out = csv.writer(f, lineterminator="\n")
        out.writerow(["Id", "Label", "Color"])
        for v in order.tolist():
            out.writerow([names[v], names[v], int(membership[v]) + 1])


def write_edges_csv(path, names, rows, cols, vals, edges="all"):
    """`Source,Target,Weight`.  edges="all": every upper-triangle cell in row-major order, zeros included, as the
    reference's df.where(mask).stack() (kmer_leiden.py:339-346) — refused above ALL_EDGES_LIMIT cells; "nonzero": the
    kept edges only, in the same order."""
    if edges not in ("all", "nonzero"):
        raise ValueError("edges is 'all' or 'nonzero' (got {!r})".format(edges))
    n = len(names)
    rows, cols, vals = np.asarray(rows, np.int64), np.asarray(cols, np.int64), np.asarray(vals, np.float32)
    order = np.lexsort((cols, rows))
    rows, cols, vals = rows[order], cols[order], vals[order]
    if edges == "all":
        cells = n * (n - 1) // 2
        if cells > ALL_EDGES_LIMIT:
            raise ValueError("edges='all' would write {} upper-triangle cells (more than {}); pass edges='nonzero' to write "
                             "the {} kept edges only".format(cells, ALL_EDGES_LIMIT, len(vals)))
    with open(path, "w", newline="") as f:
        out = csv.writer(f, lineterminator="\n")
        out.writerow(["Source", "Target", "Weight"])
        if edges == "nonzero":
            for r, c, v in zip(rows.tolist(), cols.tolist(), vals):
                out.writerow([names[r], names[c], str(v)])
            return
        at = 0
        zero = str(np.float32(0))
        for i in range(n):
            weights = {}
            while at < len(rows) and rows[at] == i:
                weights[int(cols[at])] = str(vals[at])
                at += 1
            for j in range(i + 1, n):
                out.writerow([names[i], names[j], weights.get(j, zero)])


def write_kmers_csv(path, groups):
    """`Community,Size,Rank,Kmer,Mean,Sd`: for every community (explain.GroupKmers, labels = community numbers) its top
    k-mers by mean count, best first (Rank 0), with the mean and sd of that k-mer over the community's sequences."""
    with open(path, "w", newline="") as f:
        out = csv.writer(f, lineterminator="\n")
        out.writerow(["Community", "Size", "Rank", "Kmer", "Mean", "Sd"])
        for g, words in enumerate(groups.words()):
            for t, word in enumerate(words):
                j = int(groups.idx[g, t])
                out.writerow([int(groups.labels[g]), int(groups.sizes[g]), t, word, str(groups.mean[g, j]), str(groups.sd[g, j])])


@_lib.api_call
def kmer_leiden(inputfile, mean, std, k, algo="RBERVertexPartition", rs=1.0, pearsoncutoff=0, setseed=False,
                edgecolormethod="gradient", edgethreshold=0.1, labelfontsize=12, plotname=None, csvfile=None, edges="all",
                **options):
    """Leiden communities of the sequences of a FASTA file by the Pearson correlation of their k-mer profiles.  Returns
    the membership (int32, one community number per sequence, numbered by size), or None — after the reference's three
    lines — when the mean / std vectors do not fit k.  `csvfile`: writes <csvfile>_nodes_leiden.csv and
    <csvfile>_edges_leiden.csv (see write_nodes_csv / write_edges_csv for `edges`).  kmers_top=N (a keyword
    `options` takes; default None; with a csvfile): also <csvfile>_kmers_leiden.csv, the kmers_top k-mers with the largest mean count of every community with
    their mean and sd over its sequences (explain.group_kmers on the counts already on the device).
    density=d (the other keyword `options` takes; default None): instead of a pearsoncutoff known in advance, keep the
    fraction d of the pairs — the cutoff is distribution.density_cutoff on the operand already filled (ties with the
    cutoff are kept, so at least floor(d N (N - 1) / 2) edges as long as the cutoff is positive); together with a
    non-zero pearsoncutoff it raises ValueError.
    knn=K, knn_mode="union" | "mutual" (keywords `options` takes too; default None, "union"): the k-nearest-neighbour graph
    replaces the thresholded one (reciprocal.knn_graph: at most N K edges, positive r only); pearsoncutoff and density
    must then be at their defaults, else ValueError.  With knn=None nothing changes."""
    if plotname is not None:
        raise NotImplementedError("the network plot is not built here; pass csvfile= and plot the nodes and edges files (plotname={!r})".format(plotname))
    leiden.algo_code(algo)
    kmers_top = options.pop("kmers_top", None)
    density = options.pop("density", None)
    knn = options.pop("knn", None)
    knn_mode = options.pop("knn_mode", "union")
    if options:
        raise TypeError("kmer_leiden() got an unexpected keyword argument {!r}".format(sorted(options)[0]))
    if kmers_top is not None:
        kmers_top = _lib.check_topk_k(kmers_top, "kmers_top")
    if knn is not None:
        from seekr_amd import consumers
        if density is not None or float(pearsoncutoff) != 0:
            raise ValueError("give knn, or density / a non-zero pearsoncutoff, not both (knn={!r}, density={!r}, "
                             "pearsoncutoff={!r})".format(knn, density, pearsoncutoff))
        knn = _lib.check_topk_k(knn, "knn")
        consumers.knn_mode(knn_mode)
    if density is not None:
        from seekr_amd import distribution
        if float(pearsoncutoff) != 0:
            raise ValueError("give density or a non-zero pearsoncutoff, not both (density={!r}, pearsoncutoff={!r})".format(density, pearsoncutoff))
        distribution.density_rank(density, 1)  # a density lies in (0, 1]
    meanfile = np.load(mean) if isinstance(mean, str) else np.asarray(mean)
    stdfile = np.load(std) if isinstance(std, str) else np.asarray(std)
    if len(meanfile) != 4 ** k or len(stdfile) != 4 ** k:
        print("kmer size is not compatible with the normalization mean and/or std files.")
        print("Please make sure the normalization mean and std files are generated using the same kmer size as specified here in k.")
        print("No Leiden community is calculated or plotted. The output is None.")
        return None
    counter = BasicCounter(inputfile, mean=meanfile, std=stdfile, k=k, silent=True)
    counter.get_counts()
    names = [h[1:] for h in Reader(inputfile).get_headers()]
    ctx = _lib.default_context()
    x = ctx.from_numpy(np.ascontiguousarray(counter.counts, dtype=np.float32))
    z, _ = _lib.operand_fill(ctx, x, None, pearson_mod._precision_for(np.dtype(np.float32), True))
    try:
        if density is not None:
            pearsoncutoff = distribution.density_cutoff(z, density)
        membership, _, info = leiden.pearson_communities(z, float(pearsoncutoff), algo=algo, rs=float(rs), knn=knn, knn_mode=knn_mode)
        groups = None
        if kmers_top is not None and csvfile:
            from seekr_amd import explain
            groups = explain.group_kmers_device(ctx, x, membership, top=kmers_top, kmers=counter.kmers)
    finally:
        z.free()
        x.free()
    if csvfile:
        rows, cols, vals = info["edges"]
        write_nodes_csv("{}_nodes_leiden.csv".format(csvfile), names, membership)
        write_edges_csv("{}_edges_leiden.csv".format(csvfile), names, rows, cols, vals, edges=edges)
        if groups is not None:
            write_kmers_csv("{}_kmers_leiden.csv".format(csvfile), groups)
    return membership
