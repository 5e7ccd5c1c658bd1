#!/usr/bin/env python3
"""CPU-only: the 16-replica +-1 ulp nudge study of every OptimizeSim3 fixture with the numpy reference
(tests/pyref_sim3opt.py), at the reference's iteration counts and at max_iterations = 1.  Writes
profiles/sim3opt_margins.json: per fixture the guard margin (smallest relative distance of a classified
chi2 to th2), whether the discrete outcome is stable, and the spreads of chi2_final, the Sim3 and the per-pair
chi2; and per quantity the largest spread over the twelve original fixtures (full_max, cap1_max) and over each
later group of fixtures (groups), from which tests/test_sim3opt_gpu.py takes its tolerances (10 x the largest
spread of the fixture's group, or the BA tolerance of DESIGN.md §5 where that states one and it is larger).

--golden rewrites tests/golden/sim3opt_m70.npz (the m70_free fixture's inputs and pyref's outputs) instead."""
import argparse
import concurrent.futures
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from tests import pyref_sim3opt as R  # noqa: E402
from tests import sim3opt_fixtures as FX  # noqa: E402


QUANTITIES = ("chi2_rel", "rot_rad", "t_rel", "s_rel", "pair_chi2_rel")


def study(name, cap):
    P = FX.build(name, cap)
    base = R.optimize_sim3(P)
    reps = [R.optimize_sim3(Q) for Q in FX.replicas(name, P)]
    margin, same = R.guard_report(P, base, reps)
    out = {"guard_margin": None if margin == float("inf") else margin, "stable": bool(same),
           "n_inliers": base.n_inliers, "n_bad_first": base.n_bad_first, "early_return": bool(base.early_return),
           "lm_iterations": [sorted({r.lm_iterations[k] for r in [base] + reps}) for k in range(2)],
           "lm_trials": [sorted({r.lm_trials[k] for r in [base] + reps}) for k in range(2)]}
    out.update(R.spreads(base, reps, P.th2))
    return out


def write_golden(path):
    P = FX.build("m70_free")
    r = R.optimize_sim3(P)
    np.savez_compressed(path, q=P.q, t=P.t, s=P.s, p1c=P.p1c, p2c=P.p2c, obs1=P.obs1, obs2=P.obs2, w1=P.inv_sigma2_1,
                        w2=P.inv_sigma2_2, fix_scale=int(P.fix_scale), th2=np.float32(P.th2),
                        out_pair_state=r.pair_state, out_counts=np.array([r.n_inliers, r.n_bad_first, int(r.early_return)]),
                        out_R=r.R, out_t=r.t, out_s=r.s, out_chi2=r.chi2_final, out_pair_chi2=r.pair_chi2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--golden", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sim3opt_margins.json"))
    ap.add_argument("--only", nargs="*")
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    a = ap.parse_args()
    if a.golden:
        write_golden(os.path.join(ROOT, "tests", "golden", "sim3opt_m70.npz"))
        return
    res = {"replicas": FX.N_REPLICAS, "full": {}, "cap1": {}}
    names = list(a.only or FX.FIXTURES)
    with concurrent.futures.ProcessPoolExecutor(a.jobs) as ex:
        fut = {(name, cap): ex.submit(study, name, cap) for name in names for cap in (0, 1)}
        for name in names:
            res["full"][name] = fut[name, 0].result()
            res["cap1"][name] = fut[name, 1].result()
            print(name, json.dumps(res["full"][name]), json.dumps(res["cap1"][name]), flush=True)

    def maxima(mode, members):
        return {q: max([res[mode][k][q] for k in members if k in res[mode]] + [0.0]) for q in QUANTITIES}

    for mode in ("full", "cap1"):
        res[mode + "_max"] = maxima(mode, FX.ORIGINAL)
    res["groups"] = {g: {mode + "_max": maxima(mode, [k for k, f in FX.FIXTURES.items() if f.group == g])
                         for mode in ("full", "cap1")} for g in FX.GROUPS}
    if not a.only:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
            f.write("\n")
    print(json.dumps({k: res[k] for k in ("full_max", "cap1_max", "groups")}))


if __name__ == "__main__":
    main()
