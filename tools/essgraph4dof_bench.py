#!/usr/bin/env python3
"""Device time of osg_optimize_essential_graph_4dof on loop-closed inertial graphs (GPU), with the Sim3 entry
point on graphs of the same shape in the same run, for scale.

For a 150-KeyFrame and a 1 500-KeyFrame graph of ``synth_essential_graph_4dof`` (the reference's style:
measurements from the drifted poses, three corrected KeyFrames) and the ``synth_essential_graph`` graph of the same
size and edge pattern it reports
  * the wall time of one call (host structure build, uploads, every launch and read-back): after 2 warm-up
    calls, the median and the range of 9;
  * from 3 more calls with the library's phase timing on (HIP events around every launch group, which serialises
    the call): the median device time of linearise / assemble / factor / update / chi2.  "factor" holds the damping
    copy, the factorisation and both substitutions, which run in one kernel.
The project has no CPU time of the reference function: the figures are stated, no speed-up is claimed, and the
bench gates nothing.  The two entry points run different numbers of LM iterations on their graphs, so compare the
per-iteration and per-trial figures.

    python tools/essgraph4dof_bench.py [--out profiles/essgraph4dof_bench.json]
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

WARMUP, CALLS, TIMED = 2, 9, 3
PHASES = ("linearise", "assemble", "factor", "update", "chi2")


def measure(opt, call, P):
    opt.essential_graph_kernel_times(False)
    for _ in range(WARMUP):
        r = call(P)
    walls = []
    for _ in range(CALLS):
        t0 = time.perf_counter()
        r = call(P)
        walls.append(1e3 * (time.perf_counter() - t0))
    phases, store = [], 0
    for _ in range(TIMED):
        opt.essential_graph_kernel_times(True)
        timed = call(P)
        ms, store = opt.essential_graph_kernel_times(False)
        assert timed.lm_trials == r.lm_trials and timed.chi2_final == r.chi2_final
        phases.append(ms)
    dev = {k: float(np.median([p[k] for p in phases])) for k in PHASES}
    return {
        "vertices": P.n, "edges": P.n_edges, "lm_iterations": r.lm_iterations, "lm_trials": r.lm_trials,
        "chi2_initial": r.chi2_initial, "chi2_final": r.chi2_final,
        "call_wall_ms": {"median": float(np.median(walls)), "min": float(min(walls)), "max": float(max(walls)), "n": CALLS,
                         "warmup": WARMUP},
        "device_ms_median_of_%d" % TIMED: dev,
        "device_ms_range": {k: [float(min(p[k] for p in phases)), float(max(p[k] for p in phases))] for k in PHASES},
        "device_ms_per_iteration_linearise": dev["linearise"] / max(r.lm_iterations, 1),
        "device_ms_per_trial_factor": dev["factor"] / max(r.lm_trials, 1),
        "matrix_store_bytes": store,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "essgraph4dof_bench.json"))
    a = ap.parse_args()
    ctx = Context(0)
    opt = op.Optimizer(ctx)
    res = {"device": "MI355X (gfx950)", "graphs": {}}
    for n_kf in (150, 1500):
        P4 = op.synth_essential_graph_4dof(np.random.default_rng(4000 + n_kf), n_kf)
        P7 = op.synth_essential_graph(np.random.default_rng(1000 + n_kf), n_kf)
        assert P4.n_edges == P7.n_edges
        res["graphs"]["kf%d" % n_kf] = {"four_dof": measure(opt, opt.optimize_essential_graph_4dof, P4),
                                        "sim3": measure(opt, opt.optimize_essential_graph, P7)}
        print(json.dumps(res["graphs"]["kf%d" % n_kf]), flush=True)
    ctx.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
