"""Inputs of the two-set significance tests, from fixed seeds (plain numpy, no GPU), and the numpy side of their checks.

  two_sets()          (q, t): 37 noisy copies of the first rows of significant_cases.planted_counts() as queries, its
                      other 263 rows as targets — 9 731 tests
  square_sets()       (q2, t2): 37 targets and a slightly noisy copy of each as its query — every cell (i, i) is significant
  pearson64 / tail_p  r in float64 numpy and the p-values of significant_cases.backgrounds() without scipy
  full_path           the specification in numpy: adj_rule's correction of the whole flattened matrix
  select_block        a matrix for the cell-selection kernel: NaN, +-0, +-inf, cells equal to the cutoff
  domain_sequences    queries of biased composition, targets that hold each of them once, an unrelated target and a
                      background, as FASTA text
"""
import functools
import math

import numpy as np

import adj_rule
import significant_cases as sc

N_QUERY = 37
ALPHAS = (0.05, 0.01)


@functools.lru_cache(maxsize=None)
def two_sets():
    x = sc.planted_counts()
    noise = np.random.default_rng(20261021).standard_normal((N_QUERY, x.shape[1]))
    q = (x[:N_QUERY] + 0.5 * noise).astype(np.float32)
    t = np.array(x[N_QUERY:])
    for a in (q, t):
        a.setflags(write=False)
    return q, t


@functools.lru_cache(maxsize=None)
def square_sets():
    t2 = np.array(two_sets()[1][:N_QUERY])
    noise = np.random.default_rng(20261022).standard_normal(t2.shape)
    q2 = (t2 + 0.05 * noise).astype(np.float32)
    for a in (q2, t2):
        a.setflags(write=False)
    return q2, t2


def pearson64(a, b):
    za = a.astype(np.float64) - a.astype(np.float64).mean(axis=1, keepdims=True)
    zb = b.astype(np.float64) - b.astype(np.float64).mean(axis=1, keepdims=True)
    za /= np.sqrt((za * za).sum(axis=1, keepdims=True))
    zb /= np.sqrt((zb * zb).sum(axis=1, keepdims=True))
    return za @ zb.T


def tail_p(r, fitres):
    """float32 p-values of the float32 values r against one of significant_cases.backgrounds(): the empirical count,
    the normal tail, or the tail of a gamma distribution whose shape is a whole number (a finite sum)."""
    r = np.asarray(r, dtype=np.float32)
    if isinstance(fitres, np.ndarray):
        return sc.empirical_p(r.reshape(-1), fitres).reshape(r.shape)
    name, _, params = fitres[0]
    flat = r.reshape(-1).astype(np.float64)
    if name == "norm":
        loc, scale = params
        p = [0.5 * math.erfc((v - loc) / scale / math.sqrt(2.0)) for v in flat]
    else:
        assert name == "gamma" and float(params[0]).is_integer()
        shape, loc, scale = params
        terms = np.arange(int(shape))
        logfact = np.array([math.lgamma(i + 1.0) for i in terms])
        p = []
        for v in flat:
            z = (v - loc) / scale
            p.append(1.0 if z <= 0 else float(np.exp(terms * math.log(z) - z - logfact).sum()))
    return np.array(p).astype(np.float32).reshape(r.shape)


def full_path(p, method, alpha):
    """(rows, cols, corrected) of the cells whose correction among ALL cells of the matrix p is <= alpha, in np.nonzero
    order: adj_pval on a non-symmetric matrix."""
    with np.errstate(all="ignore"):
        adj = adj_rule.correct(p.reshape(-1), method, alpha).astype(np.float64).reshape(p.shape)
    rows, cols = np.nonzero(adj <= alpha)
    return rows, cols, adj[rows, cols]


def condition(found, cells):
    """What every parity test asserts on the full path before it compares anything."""
    return 1 <= found < cells / 2


SPECIALS = np.array([np.nan, 0.0, -0.0, np.inf, -np.inf], dtype=np.float32)


def select_block(rows, cols, seed, cutoff, special=0.05):
    """float32 [rows, cols] of uniform values in (-1, 1) in which a share `special` of the cells is NaN, +-0, +-inf, the
    cutoff itself or the float32 next to it on either side."""
    rng = np.random.default_rng([seed, rows, cols])
    x = (rng.random((rows, cols)) * 2 - 1).astype(np.float32)
    c = np.float32(cutoff)
    pool = np.concatenate([SPECIALS, [c, np.nextafter(c, np.float32(-2)), np.nextafter(c, np.float32(2))]]).astype(np.float32)
    mask = rng.random((rows, cols)) < special
    x[mask] = pool[rng.integers(0, len(pool), int(mask.sum()))]
    return x


def expected_cells(x, cutoff, nrows, col_begin, col_end, row_global0=0, col_global0=0):
    """(rows, cols, vals) of np.nonzero(~(block < cutoff)) with the global offsets: the column is col_global0 + the
    matrix's own column index."""
    block = x[:nrows, col_begin:col_end]
    with np.errstate(invalid="ignore"):
        i, j = np.nonzero(~(block < np.float32(cutoff)))
    return (i + row_global0).astype(np.uint32), (j + col_begin + col_global0).astype(np.uint32), block[i, j]


def _random_dna(rng, n, probs=(0.25, 0.25, 0.25, 0.25)):
    return "".join(rng.choice(list("ACGT"), size=n, p=probs))


@functools.lru_cache(maxsize=None)
def domain_sequences():
    """dict of FASTA texts: `query` (3 sequences of 600 bases, each of its own biased composition), `target` (6 000 and
    4 100 random bases holding every query once), `unrelated` (a random target without them) and `background` (40
    random sequences of 700 bases, for the norm vectors), plus `embedded`: (query, target sequence, offset)."""
    rng = np.random.default_rng(20261023)
    biases = [(0.55, 0.15, 0.15, 0.15), (0.1, 0.6, 0.2, 0.1), (0.15, 0.1, 0.15, 0.6)]
    queries = [_random_dna(rng, 600, b) for b in biases]
    targets = [_random_dna(rng, 6000), _random_dna(rng, 4100)]
    embedded = [(0, 0, 1000), (1, 0, 3500), (2, 1, 2000)]
    for qi, ti, off in embedded:
        targets[ti] = targets[ti][:off] + queries[qi] + targets[ti][off + 600:]
    assert [len(s) for s in targets] == [6000, 4100]
    unrelated = [_random_dna(rng, 9000), _random_dna(rng, 5000)]
    background = [_random_dna(rng, 700) for _ in range(40)]

    def fasta(seqs, tag):
        return "".join(">{}{}\n{}\n".format(tag, i, s) for i, s in enumerate(seqs))

    return {"query": fasta(queries, "query"), "target": fasta(targets, "target"), "unrelated": fasta(unrelated, "other"),
            "background": fasta(background, "bg"), "embedded": embedded}
