#!/usr/bin/env python3
"""The +-1 ulp nudge study behind the tolerances of tests/test_essgraph_gpu.py (CPU only).

For every fixture of tests/essgraph_fixtures.py, at the reference's 20 iterations ("full") and at
max_iterations = 1 ("cap1"), tests/pyref_essgraph.py runs on the fixture and on 16 replicas whose input Sim3s
and measurements each moved by +-1 ulp; the largest deviation of a replica from the base run is the spread of
each compared quantity.  profiles/essgraph_margins.json keeps the spreads per fixture and their maxima per
group; a GPU tolerance is 10 x its group's maximum, or the BA floor of DESIGN.md §5 where that is larger.

    python tools/essgraph_margins.py [--out profiles/essgraph_margins.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import essgraph_fixtures as FX  # noqa: E402
from tests import pyref_essgraph as R  # noqa: E402

QUANTITIES = ("rot_rad", "t_rel", "s_rel", "chi2_initial_rel", "chi2_rel", "edge_chi2_rel")


def study(name, cap):
    P = FX.build(name, cap)
    base = R.optimize(P)
    reps = [R.optimize(Q) for Q in FX.replicas(name, P)]
    out = R.spreads(base, reps)
    out["lm_iterations"] = sorted({base.lm_iterations} | {r.lm_iterations for r in reps})
    out["lm_trials"] = sorted({base.lm_trials} | {r.lm_trials for r in reps})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "essgraph_margins.json"))
    a = ap.parse_args()
    res = {"n_replicas": FX.N_REPLICAS, "full": {}, "cap1": {}, "groups": {}}
    for name in FX.FIXTURES:
        for mode, cap in (("full", 0), ("cap1", 1)):
            res[mode][name] = study(name, cap)
            print(name, mode, {q: "%.2e" % res[mode][name][q] for q in QUANTITIES}, res[mode][name]["lm_trials"], flush=True)
    for g in FX.GROUPS:
        members = [k for k, f in FX.FIXTURES.items() if f.group == g]
        res["groups"][g] = {mode + "_max": {q: max(res[mode][k][q] for k in members) for q in QUANTITIES}
                            for mode in ("full", "cap1")}
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
