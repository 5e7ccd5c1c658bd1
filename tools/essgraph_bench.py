#!/usr/bin/env python3
"""Device time of osg_optimize_essential_graph on loop-closed graphs (GPU).

For a 150-KeyFrame and a 1 500-KeyFrame graph of ``synth_essential_graph`` (the reference's style: measurements
from the drifted poses, three corrected KeyFrames) it reports
  * the wall time of one call (host structure build, uploads, every launch and read-back), median of 5;
  * from one more call with the library's phase timing on (HIP events around every launch group, which
    serialises the call): the device time of linearise / assemble / factor / solve / chi2.  The library's
    "factor" phase holds the damping copy, the factorisation and both substitutions, which run in one kernel,
    so factor and solve are one figure here; "update" is the oplus of the trial state.
The project has no CPU baseline of this function: the figures are stated, no speed-up is claimed.

    python tools/essgraph_bench.py [--out profiles/essgraph_latency.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from orb_slam3_comments_ghr_amd import Context  # noqa: E402
from orb_slam3_comments_ghr_amd import optimizer as op  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "essgraph_latency.json"))
    a = ap.parse_args()
    ctx = Context(0)
    opt = op.Optimizer(ctx)
    res = {"device": "MI355X (gfx950)", "graphs": {}}
    for n_kf in (150, 1500):
        P = op.synth_essential_graph(np.random.default_rng(1000 + n_kf), n_kf)
        opt.essential_graph_kernel_times(False)
        opt.optimize_essential_graph(P)  # buffers allocated
        walls = []
        for _ in range(5):
            t0 = time.perf_counter()
            r = opt.optimize_essential_graph(P)
            walls.append(1e3 * (time.perf_counter() - t0))
        opt.essential_graph_kernel_times(True)
        timed = opt.optimize_essential_graph(P)
        ms, store = opt.essential_graph_kernel_times(False)
        assert timed.lm_trials == r.lm_trials and np.array_equal(timed.sim3, r.sim3)
        res["graphs"]["kf%d" % n_kf] = {
            "vertices": P.n, "edges": P.n_edges, "lm_iterations": r.lm_iterations, "lm_trials": r.lm_trials,
            "chi2_initial": r.chi2_initial, "chi2_final": r.chi2_final, "call_wall_ms_median_of_5": float(np.median(walls)),
            "call_wall_ms_all": walls, "device_ms": {"linearise": ms["linearise"], "assemble": ms["assemble"],
                                                     "factor_and_solve": ms["factor"], "update": ms["update"], "chi2": ms["chi2"]},
            "device_ms_per_trial_factor_and_solve": ms["factor"] / max(r.lm_trials, 1),
            "device_ms_per_iteration_linearise": ms["linearise"] / max(r.lm_iterations, 1),
            "matrix_store_bytes": store,
        }
        print(json.dumps(res["graphs"]["kf%d" % n_kf]), flush=True)
    ctx.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
