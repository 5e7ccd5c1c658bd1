#!/usr/bin/env python3
"""The nudge study behind the tolerances of tests/test_essgraph4dof_gpu.py (CPU only), the method of
DESIGN.md §3.19 on the 4-DoF graph.

For every fixture of tests/essgraph4dof_fixtures.py, at the reference's 20 iterations ("full") and at
max_iterations = 1 ("cap1"), tests/pyref_essgraph4dof.py runs on the fixture and on 16 replicas.  Every
replica's input poses and measurements each moved by +-1 ulp; on top of that the replicas in turn move sin / cos /
acos one ulp up and down, take the sums in reverse, normalise rotations by the polar factor instead of the SVD,
and solve through another factorisation (essgraph4dof_fixtures.replicas lists them).  The largest deviation of a
replica from the base run is the spread of each compared quantity.  profiles/essgraph4dof_margins.json keeps the
spreads per fixture and their maxima per group; a GPU tolerance is 10 x its group's maximum, or for the states
and chi2_final the BA floor of DESIGN.md §5 where that is larger.

    python tools/essgraph4dof_margins.py [--out profiles/essgraph4dof_margins.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import essgraph4dof_fixtures as FX  # noqa: E402
from tests import pyref_essgraph4dof as R  # noqa: E402


def study(name, cap):
    P = FX.build(name, cap)
    base = R.optimize(P)
    reps = [R.optimize(Q, v) for Q, v in FX.replicas(name, P)]
    out = R.spreads(base, reps, P)
    out["lm_iterations"] = sorted({base.lm_iterations} | {r.lm_iterations for r in reps})
    out["lm_trials"] = sorted({base.lm_trials} | {r.lm_trials for r in reps})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "essgraph4dof_margins.json"))
    a = ap.parse_args()
    res = {"n_replicas": FX.N_REPLICAS, "full": {}, "cap1": {}, "groups": {}}
    for name in FX.FIXTURES:
        for mode, cap in (("full", 0), ("cap1", 1)):
            res[mode][name] = study(name, cap)
            print(name, mode, {q: "%.2e" % res[mode][name][q] for q in R.KEYS}, res[mode][name]["lm_trials"], flush=True)
    for g in FX.GROUPS:
        members = [k for k, f in FX.FIXTURES.items() if f.group == g]
        res["groups"][g] = {mode + "_max": {q: max(res[mode][k][q] for k in members) for q in R.KEYS}
                            for mode in ("full", "cap1")}
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
