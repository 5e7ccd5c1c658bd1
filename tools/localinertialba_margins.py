#!/usr/bin/env python3
"""The replica study of the LocalInertialBA fixtures -> profiles/localinertialba_margins.json (CPU only).

Every fixture of tests/localinertialba_fixtures.py is run through tests/pyref_localinertialba.py as written and
through its replicas: the quadratic forms and chi2 summed back to front, sin / cos / acos one ulp up and one ulp down,
the solve through the Schur complement of the points instead of the dense one, the informations through eigh,
NormalizeRotation by the polar factor instead of the SVD, and the inputs nudged by +-1 ulp twice.  Per fixture group
it records the largest movement of every compared output and, per fixture, the number of leading iterations on which
all replicas take the restatement's accept / reject decisions.  The GPU tolerances are 10 x the group's spread, no
floor.

A fixture is admitted only if
  * every replica's decisions agree on all iterations up to the one where chi2 is within 1e-6 relative of its final
    value, and on every iteration of the run (the final state is compared, so it needs a spread),
  * the edges guarded out of the flag comparison (chi2 within 10 x spread of a threshold, depth within 10 x spread of
    0) are at most 1 % of its visual edges and never all of one KeyFrame's,
and at least one fixture must reject a trial inside its agreed prefix.  The tool fails otherwise: choose another seed
in tests/localinertialba_fixtures.py."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import localinertialba_fixtures as F  # noqa: E402
from tests import pyref_localinertialba as R  # noqa: E402


def main():
    fixtures, groups = {}, {g: {"spread": {q: 0.0 for q in R.QUANTITIES}, "fixtures": []} for g in F.GROUPS}
    for name in F.ALL:
        s = F.study(name)
        fixtures[name] = s
        g = groups[s["group"]]
        g["fixtures"].append(name)
        for q, v in s["spread"].items():
            g["spread"][q] = max(g["spread"][q], v)
        print("%-20s agreed %2d / %2d (settled %2d) rejected in prefix %2d  %s" % (
            name, s["agreed"], s["iterations"], s["settled"], s["rejected_in_prefix"],
            " ".join("%s=%.1e" % kv for kv in s["spread"].items())), flush=True)
    bad = []
    for g in groups.values():
        g["tol"] = {q: 10.0 * v for q, v in g["spread"].items()}
    for name, s in fixtures.items():
        if s["agreed"] < s["settled"]:
            bad.append("%s: the replicas' decisions part at iteration %d, before chi2 settles (%d)" % (
                name, s["agreed"], s["settled"]))
        if not s["final_ok"]:
            bad.append("%s: a replica parts from the restatement before the end, so the final state has no spread" % name)
        sp = groups[s["group"]]["spread"]
        P = F.build(name)
        gd = R.guarded(P, F.reference(name), sp["edge_chi2_rel"], sp["xw"])
        s["guarded"] = int(gd.sum())
        if gd.sum() > 0.01 * max(1, len(gd)):
            bad.append("%s: %d of %d visual edges guarded out" % (name, gd.sum(), len(gd)))
        for k in np.unique(P.e_kf):
            if np.all(gd[P.e_kf == k]):
                bad.append("%s: every edge of KeyFrame %d guarded out" % (name, k))
    rejects = [n for n, s in fixtures.items() if s["rejected_in_prefix"] > 0]
    if not rejects:
        bad.append("no fixture rejects a trial inside its agreed prefix")
    out = {"method": __doc__.split("\n\n")[1].replace("\n", " "), "replicas": [k for k, _ in F.REPLICAS] + ["nudge"] * 2,
           "groups": groups, "fixtures": fixtures, "fixtures_rejecting_in_prefix": rejects}
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
