#!/usr/bin/env python3
"""CPU-only: the replica study of every TwoViewReconstruction fixture with the numpy restatement
(tests/pyref_twoview.py).  Writes profiles/twoview_margins.json: per fixture the largest movement over the
replicas (every SVD and Normalize's sums in float64; sums back to front; keypoints nudged by one ulp) of the
per-hypothesis scores (relative to the best score), of H and F (unit Frobenius norm, sign fixed), of R (angle),
t (direction), the triangulated points (relative), the parallax, and of the quantities compared with a
threshold (chi-square / threshold, cosParallax, depth / distance, squared error / th2); per group of fixtures
the maxima; and per fixture the outcome and the verdict of tests/twoview_fixtures.py's guard at 10 x the
group's maxima.  tests/test_twoview_gpu.py allows 10 x the group maxima; no tolerance is typed in."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import twoview_fixtures as FX  # noqa: E402


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
        d.update(ok=bool(o.ok), model=int(o.model), hyp_h=int(o.hyp_h), hyp_f=int(o.hyp_f), cand=int(o.cand),
                 n_inliers=int(o.n_inliers), n_good=[int(c.n_good) for c in o.checks])
        fixtures[name] = d
        print(name, json.dumps(d), flush=True)
    groups = {}
    for g in FX.GROUPS:
        members = [k for k in names if FX.FIXTURES[k].group == g]
        if members:
            groups[g] = {q: max(fixtures[k][q] for k in members) for q in FX.QUANTITIES}
    ok = True
    for name in names:
        tol = {q: FX.FACTOR * v for q, v in groups[FX.FIXTURES[name].group].items()}
        bad = FX.guard(name, tol)
        allb = FX.n_borderline(name, tol)
        fixtures[name]["borderline"] = allb
        fixtures[name]["valid"] = not bad
        if bad:
            ok = False
            print("INVALID", name, bad[:8], flush=True)
    out = {"replicas": 2 + FX.N_NUDGED, "factor": FX.FACTOR, "groups": groups, "fixtures": fixtures,
           "note": "replicas: float64 SVDs and Normalize sums; sums back to front; keypoints nudged by -1/0/+1 float ulp"}
    if not a.only:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
            f.write("\n")
    print(json.dumps(groups, indent=1))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
