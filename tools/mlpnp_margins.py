#!/usr/bin/env python3
"""CPU-only: the replica study of every MLPnPsolver fixture with the numpy reference (tests/pyref_mlpnp.py).
Writes profiles/mlpnp_margins.json: per fixture the largest relative movement over the replicas of
err / bound (matches within +-50 % of the bound), of R and t of every compared hypothesis and of the deciding
quantities of computePose, the outcome, and the share of hypotheses that are borderline or excluded; per group
of fixtures the maxima, g = 10 x the group's largest movement of err / bound, m = 10 x its largest movement
of a deciding quantity, and the R, t tolerances (10 x the spreads) that tests/test_mlpnp_gpu.py uses; and per
fixture the verdict of tests/mlpnp_fixtures.py's guard at those margins.  Nothing here is typed in."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from tests import mlpnp_fixtures as FX  # noqa: E402

QUANTITIES = ("ratio_rel", "rot_rad", "t_rel", "quant_rel")


def study(names):
    fixtures = {}
    for name in names:
        o = FX.outcome(name)
        d = FX.spreads(name)
        d.update(converged=bool(o.converged), hyp=int(o.hyp), n_iterations=int(o.n_iterations), n_best=int(o.n_best))
        fixtures[name] = d
    groups = {}
    for g in FX.GROUPS:
        members = [k for k in names if FX.FIXTURES[k].group == g]
        if not members:
            continue
        groups[g] = {q + "_max": max(fixtures[k][q] for k in members) for q in QUANTITIES}
        groups[g]["g"] = 10.0 * groups[g]["ratio_rel_max"]
        groups[g]["m"] = 10.0 * groups[g]["quant_rel_max"]
        groups[g]["rot_tol"] = 10.0 * groups[g]["rot_rad_max"]
        groups[g]["t_tol"] = 10.0 * groups[g]["t_rel_max"]
    for name in names:
        grp = groups[FX.FIXTURES[name].group]
        bad = FX.guard(name, grp["g"], grp["m"])
        ev = FX.evaluations(name)
        if ev:
            flagged = FX.excluded(name, grp["m"]) | (FX.borderline(ev[0], grp["g"]) > 0)
            fixtures[name]["flagged_hyp_frac"] = float(np.count_nonzero(flagged) / len(flagged))
            fixtures[name]["excluded_hyp"] = int(np.count_nonzero(FX.excluded(name, grp["m"])))
        else:
            fixtures[name]["flagged_hyp_frac"], fixtures[name]["excluded_hyp"] = 0.0, 0
        fixtures[name]["valid"] = not bad
        fixtures[name]["violations"] = [list(map(str, b)) for b in bad[:8]]
    return {"replicas": len(FX.REPLICAS), "groups": groups, "fixtures": fixtures,
            "note": "replicas: bearings and points nudged by -1/0/+1 float ulp, null-space bases rotated, eigh for svd, "
                    "planar eigenvectors and the solution vector negated"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=FX.MARGINS)
    ap.add_argument("--only", nargs="*")
    a = ap.parse_args()
    out = study(a.only or list(FX.FIXTURES))
    for name, d in out["fixtures"].items():
        print(name, json.dumps(d), flush=True)
    if not a.only:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
            f.write("\n")
    print(json.dumps(out["groups"], indent=1))
    return 0 if all(d["valid"] for d in out["fixtures"].values()) else 1


if __name__ == "__main__":
    sys.exit(main())
