#!/usr/bin/env python3
"""The replica study of the PoseInertialOptimization fixtures (CPU only): for every fixture of
tests/poseinertial_fixtures.py run tests/pyref_poseinertial.py and its replicas (sums back to front, sin / cos /
acos one ulp up and down, NormalizeRotation by the polar decomposition, the solve by Cholesky, the informations by
another inverse, states and points nudged by +-1 ulp three times) and record, per fixture and per group, the
largest movement of every compared output and of every quantity that is compared with a threshold, and each
fixture's admission: the same discrete outcome in every replica, and every thresholded quantity further from its
threshold than 10 x the group's spread.

    python tools/poseinertial_margins.py            # writes profiles/poseinertial_margins.json
    python tools/poseinertial_margins.py lkf_n65    # prints the study of some fixtures, writes nothing
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests import poseinertial_fixtures as FX  # noqa: E402
from tests import pyref_poseinertial as R  # noqa: E402


def main():
    names = sys.argv[1:] or list(FX.FIXTURES)
    fixtures = {}
    for k in names:
        fixtures[k] = FX.study(k)
        print(k, "same" if fixtures[k]["same"] else "DIFFERS", {q: "%.2e" % v for q, v in fixtures[k]["margin"].items()},
              flush=True)
    if sys.argv[1:]:
        print(json.dumps(fixtures, indent=1))
        return 0
    kinds = R.QUANTITIES + FX.THRESHOLD_KINDS
    groups = {}
    for g in FX.GROUPS:
        members = [k for k in FX.FIXTURES if FX.FIXTURES[k].group == g]
        mx = {q: max(fixtures[k]["spread"][q] for k in members) for q in kinds}
        groups[g] = {"max": mx, "tol": {q: 10.0 * mx[q] for q in R.QUANTITIES}}
    bad = []
    for k, s in fixtures.items():
        mx = groups[FX.FIXTURES[k].group]["max"]
        s["valid"] = bool(s["same"] and all(s["margin"][q] > 10.0 * mx[q] for q in FX.THRESHOLD_KINDS))
        if not s["valid"]:
            bad.append(k)
    with open(FX.MARGINS, "w") as f:
        json.dump({"replicas": [r[0] for r in FX.replicas(names[0], FX.build(names[0]))], "groups": groups,
                   "fixtures": fixtures}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("not admitted:", bad)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
