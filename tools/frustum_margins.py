#!/usr/bin/env python3
"""Measure how far the compared and returned quantities of Frame::isInFrustum move between equally valid
evaluations, per fixture group, and write profiles/frustum_margins.json (CPU only; read by
tests/frustum_fixtures.py).

    python tools/frustum_margins.py

Replicas of every fixture of tests/frustum_fixtures.py are run through tests/pyref_frustum.py: Eigen's 3-term sums
back to front, the norms in float64, atan2f / cosf / sinf of the KannalaBrandt8 projection one ulp up and down, the
pose and the points nudged by one ulp (three times).  Per fixture the largest movement of each kind of quantity is
recorded (z, uv, dist, cos, xr, depth: see tests/frustum_fixtures.py); per group the largest over its fixtures, and
the tolerance 10 x that.  Then every fixture's guard (the level band, and every threshold comparison further from
its threshold than the tolerance) is evaluated at its group's tolerances; the tool fails when one is invalid.
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests import frustum_fixtures as FX  # noqa: E402


def measure():
    fixtures = {name: FX.spreads(name) for name in FX.FIXTURES}
    groups = {}
    for g in FX.GROUPS:
        members = [k for k in FX.FIXTURES if FX.group(k) == g]
        mx = {q: max(fixtures[k][q] for k in members) for q in FX.KINDS}
        groups[g] = {"max": mx, "tol": {q: 10.0 * v for q, v in mx.items()}}
    for name, f in fixtures.items():
        bad = FX.guard(name, groups[FX.group(name)]["tol"])
        f["points"] = int(FX.build(name)[1].n)
        f["n_to_match"] = int(FX.reference(name).n_to_match)
        f["valid"] = not bad
    return {"replicas": [[n, vars(v)] for n, v in FX.REPLICAS], "level_band": FX.LEVEL_BAND, "seeds": FX.SEEDS,
            "fixtures": fixtures, "groups": groups}


def main():
    m = measure()
    bad = [k for k, f in m["fixtures"].items() if not f["valid"]]
    for k in bad:
        print("invalid fixture", k, FX.guard(k, m["groups"][FX.group(k)]["tol"]))
    with open(FX.MARGINS, "w") as f:
        json.dump(m, f, indent=1, sort_keys=True)
        f.write("\n")
    for g, v in m["groups"].items():
        print(g, {q: "%.3g" % t for q, t in v["tol"].items()})
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
