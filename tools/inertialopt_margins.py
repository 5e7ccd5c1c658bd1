#!/usr/bin/env python3
"""The replica study of the InertialOptimization fixtures -> profiles/inertialopt_margins.json (CPU only).

Every fixture of tests/inertialopt_fixtures.py is run through tests/pyref_inertialopt.py as written and through its
replicas: the quadratic forms and chi2 summed back to front, sin / cos / acos / exp one ulp up and one ulp down, the
solve through the Schur complement of the border instead of the dense one, the informations through the other route,
NormalizeRotation by the polar decomposition instead of the SVD, and the inputs nudged by +-1 ulp three times.  Per fixture group it records the largest movement of every compared
output and, per fixture, the number of leading iterations on which all replicas take the restatement's accept /
reject decisions.  The GPU tolerances are 10 x the group's spread, no floor.

A fixture is admitted only if
  * every replica's decisions agree on all iterations up to the one where chi2 is within 1e-6 relative of its final
    value,
  * no Huber edge has chi2 / delta^2 within 10 x the group's relative chi2 spread of 1,
  * no information eigenvalue lies within that margin of 1e-12,
and at least one Levenberg-Marquardt fixture must reject a trial inside its agreed prefix.  The tool fails otherwise:
choose another seed in tests/inertialopt_fixtures.py."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import inertialopt_fixtures as F  # noqa: E402
from tests import pyref_inertialopt as R  # noqa: E402


def main():
    fixtures, groups = {}, {g: {"spread": {q: 0.0 for q in R.QUANTITIES}, "fixtures": []} for g in F.GROUPS}
    for name in F.ALL:
        s = F.study(name)
        fixtures[name] = s
        g = groups[s["group"]]
        g["fixtures"].append(name)
        for q, v in s["spread"].items():
            g["spread"][q] = max(g["spread"][q], v)
        print("%-22s agreed %2d / %2d (settled %2d) rejected in prefix %2d  %s" % (
            name, s["agreed"], s["iterations"], s["settled"], s["rejected_in_prefix"],
            " ".join("%s=%.1e" % kv for kv in s["spread"].items())), flush=True)
    bad = []
    for g in groups.values():
        g["tol"] = {q: 10.0 * v for q, v in g["spread"].items()}
    for name, s in fixtures.items():
        margin = 10.0 * groups[s["group"]]["spread"]["trace_chi2_rel"]
        if s["agreed"] < s["settled"]:
            bad.append("%s: the replicas' decisions part at iteration %d, before chi2 settles (%d)" % (
                name, s["agreed"], s["settled"]))
        if s["huber_margin"] is not None and s["huber_margin"] <= margin:
            bad.append("%s: a Huber edge within %.1e of delta^2" % (name, s["huber_margin"]))
        if s["eig_margin"] is not None and s["eig_margin"] <= margin * 1e-12:
            bad.append("%s: an information eigenvalue at the 1e-12 cut" % name)
    lm_rejects = [n for n, s in fixtures.items() if s["group"] != "scale" and s["rejected_in_prefix"] > 0]
    if not lm_rejects:
        bad.append("no Levenberg-Marquardt fixture rejects a trial inside its agreed prefix")
    out = {"method": __doc__.split("\n\n")[1].replace("\n", " "), "replicas": [k for k, _ in F.REPLICAS] + ["nudge"] * 3,
           "groups": groups, "fixtures": fixtures, "lm_fixtures_rejecting_in_prefix": lm_rejects}
    if bad:
        print("\n".join(bad), file=sys.stderr)
        return 1
    with open(F.MARGINS, "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote", F.MARGINS)
    return 0


if __name__ == "__main__":
    sys.exit(main())
