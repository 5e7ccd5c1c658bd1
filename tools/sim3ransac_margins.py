#!/usr/bin/env python3
"""CPU-only: the 16-replica study of every Sim3Solver fixture with the numpy reference
(tests/pyref_sim3solver.py).  Writes profiles/sim3ransac_margins.json: per fixture the largest relative
movement over the replicas of err / bound (matches within +-50 % of the bound) and of R, t, s of the
returned hypothesis, the outcome, and the share of hypotheses with a borderline match; per group of
fixtures the maxima and g = 10 x the group's largest movement of err / bound, the margin at which
tests/sim3solver_fixtures.py's guard is evaluated; and per fixture the guard's verdict at that g.
tests/test_sim3solver_gpu.py takes its R / t / s tolerances from the group maxima (10 x)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from tests import sim3solver_fixtures as FX  # noqa: E402

QUANTITIES = ("ratio_rel", "rot_rad", "t_rel", "s_rel")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=FX.MARGINS)
    ap.add_argument("--only", nargs="*")
    a = ap.parse_args()
    names = a.only or list(FX.FIXTURES)
    fixtures = {}
    for name in names:
        o = FX.outcome(name)
        d = FX.spreads(name)
        d.update(converged=bool(o.converged), hyp=int(o.hyp), n_iterations=int(o.n_iterations), n_best=int(o.n_best))
        fixtures[name] = d
        print(name, json.dumps(d), flush=True)
    groups = {}
    for g in FX.GROUPS:
        members = [k for k in names if FX.FIXTURES[k].group == g]
        if not members:
            continue
        groups[g] = {q + "_max": max(fixtures[k][q] for k in members) for q in QUANTITIES}
        groups[g]["g"] = 10.0 * groups[g]["ratio_rel_max"]
    ok = True
    for name in names:
        g = groups[FX.FIXTURES[name].group]["g"]
        bad = FX.guard(name, g)
        ev = FX.evaluations(name)
        fixtures[name]["borderline_hyp_frac"] = (
            float(np.count_nonzero(FX.borderline(ev[0], g)) / len(ev[0].counts)) if ev else 0.0)
        fixtures[name]["valid"] = not bad
        if bad:
            ok = False
            print("INVALID", name, bad[:8], flush=True)
    out = {"replicas": FX.N_REPLICAS, "groups": groups, "fixtures": fixtures,
           "note": "replicas: points nudged by -1/0/+1 float ulp; odd replicas solve Horn's N in float64 (eigh)"}
    if not a.only:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
            f.write("\n")
    print(json.dumps(groups, indent=1))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
