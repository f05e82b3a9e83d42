#!/usr/bin/env python3
"""Golden vectors for adj_pval (adj_pval.py:53-138): the reference's own adj_pval, which calls statsmodels 0.12.2
multipletests, run on float32 / float64 frames.  Run it with the Python 3.9 environment that has statsmodels 0.12.2,
numpy 1.26 and pandas 2.3, with the reference checkout on sys.path:

    SEEKR_REFERENCE=/path/to/seekr python3.9 tests/golden/make_golden_adj.py

Without the reference (or statsmodels) it does nothing, like the other generators.  Writes adj_pval.npz (inputs and
outputs) and adj_pval.json (case list, printed messages, the CSV round trips' bytes).
"""
import contextlib
import io
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
METHODS = ["bonferroni", "sidak", "holm-sidak", "holm", "simes-hochberg", "hommel", "fdr_bh", "fdr_by", "fdr_tsbh",
           "fdr_tsbky", "fdr_gbs"]
DTYPE_KEEPING = ["bonferroni", "sidak", "hommel", "holm", "fdr_bh"]


def _reference():
    ref = os.environ.get("SEEKR_REFERENCE", "/root/reference")
    if not os.path.isdir(os.path.join(ref, "seekr")):
        return None
    sys.path.insert(0, ref)
    try:
        from seekr.adj_pval import adj_pval
    except ImportError:
        return None
    return adj_pval


def _sym(rng, n, dtype):
    a = rng.random((n, n)).astype(dtype)
    a = np.triu(a, 1)
    a = a + a.T
    np.fill_diagonal(a, 1)
    return a.astype(dtype)


def _edge_values(rng, shape, dtype):
    v = (rng.integers(0, 1001, size=shape) / 1000.0).astype(dtype)  # ties on a 1e-3 grid
    flat = v.reshape(-1)
    flat[:5] = 0
    flat[5:9] = 1
    flat[9:12] = np.array([1.5, 2.0, 7.25], dtype=dtype)
    flat[12] = np.inf
    flat[13] = np.nan
    rng.shuffle(flat)
    return v


def _round_disagreements(rng, count):
    """float32 pairs (x, y) on which round(x, 5) == round(y, 5) holds in one dtype's arithmetic and not the other's."""
    f32, f64 = np.float32(1e5), 1e5
    out = []
    while len(out) < count:
        k = rng.integers(1, 99999)
        base = (k + 0.5) / 1e5
        x = np.float32(base)
        cands = [np.nextafter(x, np.float32(-1)), x, np.nextafter(x, np.float32(2))]
        for a in cands:
            for b in cands:
                e32 = np.rint(a * f32) / f32 == np.rint(b * f32) / f32
                e64 = np.rint(np.float64(a) * f64) / f64 == np.rint(np.float64(b) * f64) / f64
                if e32 != e64 and a != b:
                    out.append((a, b, bool(e32)))
    return out[:count]


def main():
    adj_pval = _reference()
    if adj_pval is None:
        print("make_golden_adj: reference seekr / statsmodels not importable here; nothing written")
        return
    import pandas as pd
    rng = np.random.default_rng(20261016)
    arrays, cases = {}, []

    def run(name, values, rows, cols, method, alpha=0.05):
        df = pd.DataFrame(values, index=rows, columns=cols)
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            res = adj_pval(df, method, alpha)
        i = len(cases)
        arrays["in%d" % i] = values
        arrays["out%d" % i] = res.to_numpy()
        cases.append({"name": name, "method": method, "alpha": alpha, "rows": [str(x) for x in rows],
                      "cols": [str(x) for x in cols], "message": buf.getvalue().strip(),
                      "out_dtype": str(res.to_numpy().dtype)})

    sym_labels = ["s%d" % i for i in range(60)]
    rl, cl = ["r%d" % i for i in range(40)], ["c%d" % i for i in range(70)]
    frames = {"sym60_f32": (_sym(rng, 60, np.float32), sym_labels, sym_labels),
              "sym60_f64": (_sym(rng, 60, np.float64), sym_labels, sym_labels),
              "full40x70_f32": (rng.random((40, 70)).astype(np.float32), rl, cl),
              "full40x70_f64": (rng.random((40, 70)), rl, cl)}
    for key, (v, r, c) in frames.items():
        every = key in ("sym60_f32", "full40x70_f64")
        for m in (METHODS if every else DTYPE_KEEPING):
            run(key, v, r, c, m)
    # a square frame whose values are symmetric but whose labels differ
    v = _sym(rng, 20, np.float32)
    for m in ("fdr_bh", "holm"):
        run("labels_differ", v, ["a%d" % i for i in range(20)], ["b%d" % i for i in range(20)], m)
    # ties, exact 0 and 1, values above 1, +inf, one NaN
    for dt in (np.float32, np.float64):
        v = _edge_values(rng, (15, 20), dt)
        for m in METHODS:
            run("edges_" + np.dtype(dt).name, v, ["r%d" % i for i in range(15)], ["c%d" % i for i in range(20)], m)
    # two-stage: r1 = 0, r1 = n, in between; two alphas
    r12, c12 = ["r%d" % i for i in range(10)], ["c%d" % i for i in range(12)]
    stage = {"r1_none": rng.uniform(0.5, 1.0, (10, 12)),
             "r1_all": rng.uniform(0.0, 1e-6, (10, 12)),
             "r1_some": np.where(rng.random((10, 12)) < 0.3, rng.uniform(0, 1e-4, (10, 12)), rng.uniform(0.05, 1, (10, 12)))}
    for key, v in stage.items():
        for dt in (np.float32, np.float64):
            for alpha in (0.05, 0.2):
                for m in ("fdr_tsbh", "fdr_tsbky"):
                    run("%s_%s" % (key, np.dtype(dt).name), v.astype(dt), r12, c12, m, alpha)
    # symmetry edge cases (30 x 30, equal labels); fdr_bh shows which branch was taken
    l30 = ["q%d" % i for i in range(30)]
    base = _sym(rng, 30, np.float32)
    far = base.copy()
    far[29, 0] = np.float32(far[0, 29] + 0.25)
    tiny = base.copy()
    tiny[3, 17] = np.float32(tiny[17, 3] + 2e-7)
    tiny[25, 2] = np.float32(tiny[2, 25] - 3e-7)
    nan_one = base.copy()
    nan_one[4, 9] = np.nan
    diag = base.copy()
    np.fill_diagonal(diag, rng.uniform(-50, 50, 30).astype(np.float32))
    diag[5, 5], diag[6, 6] = np.nan, np.inf
    for key, v in (("sym_far_mismatch", far), ("sym_below_5th_decimal", tiny), ("sym_nan_one_side", nan_one),
                   ("sym_garbage_diagonal", diag)):
        run(key, v, l30, l30, "fdr_bh")
    pairs = _round_disagreements(rng, 8)
    for want32 in (True, False):
        v = base.copy()
        sel = [p for p in pairs if p[2] == want32][:3] or pairs[:1]
        for j, (a, b, _) in enumerate(sel):
            v[j, 20 + j], v[20 + j, j] = a, b
        run("sym_round_f32_%s" % ("equal" if want32 else "differs"), v, l30, l30, "fdr_bh")
        run("sym_round_f32_%s" % ("equal" if want32 else "differs"), v.astype(np.float64), l30, l30, "fdr_bh")
    # hommel: 2 000 tests (float32, whole matrix) and 435 (float64, upper triangle)
    run("hommel_2000", rng.random((40, 50)).astype(np.float32) ** 3, ["r%d" % i for i in range(40)],
        ["c%d" % i for i in range(50)], "hommel")
    run("hommel_sym30", _sym(rng, 30, np.float64) ** 2, l30, l30, "hommel")
    # CSV round trips through the reference command's own path (console_scripts.py:912-920)
    csvs = []
    with tempfile.TemporaryDirectory() as tmp:
        named = ["ENST%04d" % i for i in range(6)]
        trips = [("text_labels_sym", pd.DataFrame(_sym(rng, 6, np.float64), index=named, columns=named), "fdr_bh"),
                 ("numeric_headers", pd.DataFrame(rng.random((5, 7)), index=range(5), columns=range(7)), "holm"),
                 ("repeated_headers", pd.DataFrame(_sym(rng, 6, np.float64), index=named,
                                                   columns=named[:3] + named[:3]), "fdr_tsbky")]
        for key, df, method in trips:
            src = os.path.join(tmp, key + ".csv")
            df.to_csv(src)
            pvals = pd.read_csv(src, header=0, index_col=0)
            buf = io.StringIO()
            with contextlib.redirect_stdout(buf):
                adj_pval(pvals, method, 0.05, os.path.join(tmp, key + "_out"))
            with open(src) as f:
                text_in = f.read()
            with open(os.path.join(tmp, key + "_out.csv")) as f:
                text_out = f.read()
            csvs.append({"name": key, "method": method, "alpha": 0.05, "input": text_in, "output": text_out,
                         "message": buf.getvalue().strip()})
    np.savez_compressed(os.path.join(HERE, "adj_pval.npz"), **arrays)
    with open(os.path.join(HERE, "adj_pval.json"), "w") as f:
        json.dump({"cases": cases, "csv": csvs}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote adj_pval.npz / adj_pval.json:", len(cases), "cases,", len(csvs), "CSV round trips")


if __name__ == "__main__":
    main()
