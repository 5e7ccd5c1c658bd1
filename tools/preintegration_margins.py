#!/usr/bin/env python3
"""The replica study of the IMU preintegration fixtures (CPU only): for every fixture of
tests/preintegration_fixtures.py run tests/pyref_preintegration.py and its replicas (every product-add contracted
as an FMA, emulated through float64 accumulation rounded once; inner sums back to front; sin / cos one ulp up, then
one ulp down; NormalizeRotation by the polar factor; every input nudged by +-1 ulp, three times) and record the
largest movement of every compared quantity per fixture and per group (frame, keyframe, long).  The GPU tolerance
is 10 x the group's spread, no floor.

The guard is asserted here: no step of any fixture, in the restatement or any replica, has its rotation angle d
within a relative 1e-3 of the 1e-4 cut of IntegratedRotation.  A seed that violates it is replaced in the fixtures.

    python tools/preintegration_margins.py            # writes profiles/preintegration_margins.json
    python tools/preintegration_margins.py n65        # prints the study of some fixtures, writes nothing
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests import preintegration_fixtures as FX  # noqa: E402
from tests import pyref_preintegration as R  # noqa: E402


def main():
    names = sys.argv[1:] or list(FX.FIXTURES)
    fixtures = {}
    for k in names:
        fixtures[k] = s = FX.study(k)
        print(k, "cut", s["cut_margin"], "below %d/%d" % (s["below"], s["n"]),
              {q: "%.2e" % v for q, v in s["spread"].items()}, flush=True)
    if sys.argv[1:]:
        print(json.dumps(fixtures, indent=1))
        return 0
    near = [k for k, s in fixtures.items() if s["cut_margin"] is not None and not s["cut_margin"] > FX.CUT_GUARD]
    assert not near, "a step within 1e-3 of the 1e-4 cut, replace the seed of: %r" % near
    groups = {}
    for g in FX.GROUPS:
        members = [k for k in FX.FIXTURES if FX.FIXTURES[k].group == g]
        mx = {q: max(fixtures[k]["spread"][q] for k in members) for q in R.QUANTITIES}
        groups[g] = {"max": mx, "tol": {q: 10.0 * mx[q] for q in R.QUANTITIES}}
    with open(FX.MARGINS, "w") as f:
        json.dump({"replicas": [r[0] for r in FX.REPLICAS] + ["nudge"] * 3, "cut_guard": FX.CUT_GUARD,
                   "groups": groups, "fixtures": fixtures}, f, indent=1, sort_keys=True, allow_nan=False)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
