#!/usr/bin/env python3
"""Golden vectors for find_dist / find_pval by RUNNING THE REFERENCE (same conventions as make_golden.py).  The checkout
of the reference is named by $SEEKR_REFERENCE; without one the script does nothing.  Run it from any directory that is
not this repository (it works in a temporary one):

    SEEKR_REFERENCE=<checkout of the reference> PYTHONDONTWRITEBYTECODE=1 python3 -W ignore make_golden_find_dist.py

Input: inputs.skewed_set(11, 40) written by inputs.write_fasta, k_mer = 3.  Stored in find_dist.npz: the 200-value
sample under np.random.seed(3), the whole 780-value triangle (subset_size 10^6), both bkg_* vectors and the counts the
reference correlates (the rows tests/parity_rule.judge needs).  Stored in find_dist.json: what the reference prints for
the whole triangle, for models ['norm', 'nope', 'expon'] and for a list with a discrete name, find_pval's printed text
and result for each refused fitres and for repeated headers, and the outcome of its length check for six (mean length,
std length) pairs around 4^3.
"""
import contextlib
import io
import json
import os
import sys
import tempfile

import numpy as np

REF = os.environ.get("SEEKR_REFERENCE", "")
HERE = os.path.dirname(os.path.abspath(__file__))
K = 3
LENGTH_PAIRS = [(64, 64), (63, 64), (64, 63), (63, 63), (64, 65), (65, 65)]
BAD_FITRES = {
    "list_wrong_format": [("norm", 0.1, [0.0, 1.0])],
    "list_not_tuples": [("norm", 0.1)],
    "array_2d": np.zeros((3, 2), np.float32),
    "other_type": "norm",
}


def _quiet(fn, *args, **kw):
    out = io.StringIO()
    with contextlib.redirect_stdout(out), contextlib.redirect_stderr(io.StringIO()):
        res = fn(*args, **kw)
    return res, out.getvalue()


def main():
    if not REF or not os.path.isdir(os.path.join(REF, "seekr")):
        print("reference not present; nothing to do")
        return 0
    sys.dont_write_bytecode = True
    sys.path.insert(0, REF)
    sys.path.insert(0, HERE)
    import inputs
    from seekr.find_dist import find_dist
    from seekr.find_pval import find_pval
    from seekr.kmer_counts import BasicCounter
    arrays, text = {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        fa = os.path.join(tmp, "bkg.fa")
        inputs.write_fasta(fa, inputs.skewed_set(11, 40))
        np.random.seed(3)
        arrays["sample200"], text["sample200_stdout"] = _quiet(find_dist, fa, K, "Log2.post", "common10", True, 200, False)
        arrays["bkg_mean"], arrays["bkg_std"] = np.load(f"bkg_mean_{K}mers.npy"), np.load(f"bkg_std_{K}mers.npy")
        np.random.seed(3)
        arrays["triangle"], text["triangle_stdout"] = _quiet(find_dist, fa, K, "Log2.post", "common10", True, 10 ** 6, False)
        counter = BasicCounter(fa, mean=f"bkg_mean_{K}mers.npy", std=f"bkg_std_{K}mers.npy", k=K, silent=True)
        _quiet(counter.make_count_file)
        arrays["counts"] = np.asarray(counter.counts)
        for key, models in (("models_invalid", ["norm", "nope", "expon"]), ("models_discrete", ["norm", "poisson", "gamma"])):
            _, text[key + "_stdout"] = _quiet(find_dist, fa, K, "Log2.post", models, True, 10 ** 6, False)
            text[key] = models
        # find_pval: refused fitres, repeated headers, the length check
        small = os.path.join(tmp, "small.fa")
        with open(small, "w") as fh:
            fh.write(">a\nACGTTGCAAGGCTTAACG\n>b\nGGGTTTAACCCAGTAGCA\n>a\nTTTTACGACGATCAGCAT\n")
        mean_path, std_path = f"bkg_mean_{K}mers.npy", f"bkg_std_{K}mers.npy"
        text["refused"] = {}
        for key, fitres in BAD_FITRES.items():
            res, out = _quiet(find_pval, small, fa, mean_path, std_path, K, fitres, progress_bar=False)
            text["refused"][key] = {"stdout": out, "is_none": res is None}
        text["small_fasta"] = open(small).read()
        text["length_check"] = []
        for n_mean, n_std in LENGTH_PAIRS:
            np.save("m.npy", np.resize(arrays["bkg_mean"], n_mean))
            np.save("s.npy", np.resize(arrays["bkg_std"], n_std))
            try:
                res, out = _quiet(find_pval, small, small, "m.npy", "s.npy", K, "other type", progress_bar=False)
            except Exception as e:  # noqa: BLE001 - passed the check and failed further on
                res, out = "raised " + type(e).__name__, ""
            text["length_check"].append({"mean_len": n_mean, "std_len": n_std,
                                         "refused": out.startswith("k_mer size is not compatible"), "stdout": out})
        os.chdir(HERE)
    np.savez_compressed(os.path.join(HERE, "find_dist.npz"), **arrays)
    with open(os.path.join(HERE, "find_dist.json"), "w") as fh:
        json.dump(text, fh, indent=1)
    print({k: (v.shape, str(v.dtype)) for k, v in arrays.items()})
    print(json.dumps(text, indent=1)[:3000])
    return 0


if __name__ == "__main__":
    sys.exit(main())
