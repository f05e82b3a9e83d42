#!/usr/bin/env python3
"""Golden vectors for the parametric p-values (find_pval.py:118-133): p = 1 - scipy.stats.<dist>(*params).cdf(sim)
written into a float32 matrix, for every distribution of find_dist's `common10` list (find_dist.py:96-98), with
parameters of the kind a fit to Pearson similarities returns and a few harder ones (large shapes, heavy tails, values
outside the support).  scipy is not the reference repo, but it is the library the reference calls; run anywhere scipy is
installed:

    python3 tests/golden/make_golden_pvals.py            # pvals_common10.npz
    python3 tests/golden/make_golden_pvals.py --sweep    # pvals_sweep.npz: fits to four samples, gamma / chi2 shapes up to
                                                         # 1e7, extreme exponpow / lognorm / pareto, invalid shapes
"""
import os

import numpy as np
from scipy import stats

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = [
    ("norm", (0.01, 0.08)), ("norm", (-0.3, 1.7)),
    ("cauchy", (0.005, 0.03)),
    ("expon", (-0.4, 0.25)),
    ("uniform", (-0.5, 1.2)),
    ("rayleigh", (-0.35, 0.3)),
    ("pareto", (3.1, -1.2, 1.0)), ("pareto", (12.5, -2.0, 1.9)),
    ("lognorm", (0.35, -0.6, 0.55)), ("lognorm", (1.4, -0.2, 0.1)),
    ("gamma", (2.3, -0.4, 0.12)), ("gamma", (45.0, -1.5, 0.033)), ("gamma", (0.6, -0.31, 0.2)),
    ("chi2", (3.7, -0.45, 0.11)), ("chi2", (180.0, -3.0, 0.0165)),
    ("exponpow", (1.8, -0.42, 0.6)), ("exponpow", (0.7, -0.3, 0.4)),
]


def main():
    rng = np.random.default_rng(7)
    sim = np.concatenate([rng.normal(0.0, 0.12, 3000), np.linspace(-1, 1, 801), [np.nan, -1.0, 1.0, 0.0]]).astype(np.float32)
    sim = np.clip(sim, -1, 1).reshape(-1, 5)[:760]
    out = {"sim": sim}
    for i, (name, params) in enumerate(CASES):
        dist = getattr(stats, name)(*params)
        p = np.zeros_like(sim)
        flat_p, flat_s = p.reshape(-1), sim.reshape(-1)
        for j in range(flat_s.size):  # the reference's loop: scalar float32 in, float64 arithmetic, float32 store
            flat_p[j] = 1 - dist.cdf(flat_s[j])
        out["p%d" % i] = p
    out["names"] = np.array([c[0] for c in CASES])
    out["params"] = np.array([",".join(repr(float(v)) for v in c[1]) for c in CASES])
    np.savez_compressed(os.path.join(HERE, "pvals_common10.npz"), **out)
    print("wrote pvals_common10.npz:", len(CASES), "cases,", sim.size, "cells each")


# ---- pvals_sweep.npz: the parameters at which the device's cdf formulas can go wrong (tools/consumer_sweep.py) ----------
COMMON10 = ("cauchy", "chi2", "expon", "exponpow", "gamma", "lognorm", "norm", "pareto", "rayleigh", "uniform")
GAMMA_SHAPES = (0.05, 1.0, 3e3, 2e4, 1e5, 187114.0, 3e5, 1e6, 1e7)  # 187 114: gamma.fit on 10 000 draws of N(0, 0.12)
BAD_SHAPES = [("gamma", (0.0, -0.4, 0.12)), ("gamma", (-1.5, -0.4, 0.12)), ("gamma", (float("nan"), -0.4, 0.12)),
              ("chi2", (0.0, -0.45, 0.11)), ("lognorm", (-0.35, -0.6, 0.55))]  # scipy: every cell NaN


def fit_samples():
    """name -> 10 000 values clipped to [-1, 1], fixed seeds: what find_dist hands to dist.fit."""
    rng = np.random.default_rng(11)
    return {
        "N(0, 0.12)": np.clip(rng.normal(0.0, 0.12, 10000), -1, 1),
        "gamma(4) - 0.2": np.clip(rng.gamma(4.0, 0.05, 10000) - 0.2, -1, 1),
        "0.06 t3": np.clip(0.06 * rng.standard_t(3, 10000), -1, 1),
        "float32 N(0.01, 0.08)": np.clip(rng.normal(0.01, 0.08, 10000), -1, 1).astype(np.float32),
    }


def hand_set_cases():
    cases = []
    for a in GAMMA_SHAPES:  # mean 0, sd 0.12 at every shape: the cells sit where x is close to a
        cases.append(("gamma", (a, -0.12 * np.sqrt(a), 0.12 / np.sqrt(a))))
    for a in GAMMA_SHAPES:  # chi2(df) is gamma(df / 2) on z / 2
        cases.append(("chi2", (2 * a, -0.12 * np.sqrt(a), 0.06 / np.sqrt(a))))
    cases += [("exponpow", (0.2, -0.4, 0.5)), ("exponpow", (40.0, -0.5, 0.9)),
              ("exponpow", (40.0, -1.0, 2e-8)),  # z up to 1e8: z ** 40 overflows to inf
              ("lognorm", (0.005, -13.0, 13.0)), ("lognorm", (3.0, -0.3, 0.2)),
              ("pareto", (0.5, -1.3, 1.0))]
    return cases


def sweep_cases():
    """[(distribution, params, where they come from)]"""
    import warnings
    cases = []
    for label, sample in fit_samples().items():
        for name in COMMON10:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                params = getattr(stats, name).fit(sample)
            cases.append((name, tuple(float(v) for v in params), "fit to " + label))
    cases += [(n, tuple(float(v) for v in p), "hand-set") for n, p in hand_set_cases()]
    cases += [(n, p, "bad shape") for n, p in BAD_SHAPES]
    return cases


def sweep_cells(params):
    """(the cells every case shares, the six of this case): 400 normals, a grid, NaN; loc and loc + scale in float32
    with their neighbours one ulp below and above (the edge of the support, and z = 1 for pareto)."""
    rng = np.random.default_rng(13)
    common = np.concatenate([np.clip(rng.normal(0.0, 0.12, 400), -1, 1), np.linspace(-1, 1, 161), [np.nan]]).astype(np.float32)
    loc, scale = params[-2], params[-1]
    own = []
    for v in (np.float32(loc), np.float32(loc + scale)):
        own += [np.nextafter(v, np.float32(-np.inf)), v, np.nextafter(v, np.float32(np.inf))]
    return common, np.array(own, dtype=np.float32)


def main_sweep():
    import scipy
    cases = sweep_cases()
    out = {}
    for i, (name, params, origin) in enumerate(cases):
        common, own = sweep_cells(params)
        out["sim"] = common
        out["own%d" % i] = own
        dist = getattr(stats, name)(*params)
        cells = np.concatenate([common, own])
        p = np.zeros_like(cells)
        with np.errstate(all="ignore"):
            for j in range(cells.size):  # the reference's loop: scalar float32 in, float64 arithmetic, float32 store
                p[j] = 1 - dist.cdf(cells[j])
        out["p%d" % i] = p
        print("%-9s %-26s %s" % (name, origin, ", ".join(repr(v) for v in params)))
    out["names"] = np.array([c[0] for c in cases])
    out["params"] = np.array([",".join(repr(float(v)) for v in c[1]) for c in cases])
    out["origins"] = np.array([c[2] for c in cases])
    out["scipy_version"] = np.array(scipy.__version__)
    path = os.path.join(HERE, "pvals_sweep.npz")
    np.savez_compressed(path, **out)
    print("wrote pvals_sweep.npz with scipy %s: %d cases, %d cells each, %d bytes" % (
        scipy.__version__, len(cases), len(out["sim"]) + 6, os.path.getsize(path)))


if __name__ == "__main__":
    import sys
    if "--sweep" in sys.argv or "--all" in sys.argv:
        main_sweep()
    if "--sweep" not in sys.argv:
        main()
