#!/usr/bin/env python3
"""Recorded time of osg_local_inertial_ba (not gated): HIP-event device time and wall time, medians of 10, of a
mono window with N = 10 (10 iterations, lambda 1) and N = 25 (large: 4 iterations, lambda 1e-2) free KeyFrames, the
fixed predecessor and 3 covisible fixed KeyFrames, about 1 500 and 5 000 points, one window and a batch of 64; beside
each the edges, the edge pairs of the reduced system, and the iterations and trials the call ran, since the time is
theirs.  For scale, osg_local_bundle_adjustment on a visual window of the same KeyFrame and point counts: a different
problem (6 unknowns per KeyFrame, no inertial edges, its own stop rule).  No CPU time of the reference exists here, so
no speed-up over it is stated.  The kernel is one launch, so there are no per-phase device times to record.

    python tools/localinertialba_bench.py            # writes profiles/localinertialba_bench.json
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from orb_slam3_comments_ghr_amd import Context  # noqa: E402
from orb_slam3_comments_ghr_amd import optimizer as O  # noqa: E402
from tests import localinertialba_fixtures as FX  # noqa: E402

REPS = 10
BATCH = 64


def measure(ctx, fn, reps=REPS):
    res = fn()
    dev, wall = [], []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        wall.append((time.perf_counter() - t) * 1e6)
        dev.append(ctx.last_kernel_ms() * 1e3)
    return res, {"device_us": float(np.median(dev)), "wall_us": float(np.median(wall))}


def main():
    ctx = Context(0)
    opt = O.Optimizer(ctx)
    out = {"reps": REPS, "batch": BATCH}
    for n in (10, 25):
        for pts in (1500, 5000):
            rng = np.random.default_rng(900 + n + pts)
            truth, pre = FX.trajectory(rng, n + 1, 20, True)
            P = O.synth_local_inertial_window(rng, truth, pre, n_points=pts, n_extra_fixed=3, large=n == 25, p_obs=0.5)
            free = np.array([not k.fixed for k in P.kfs])
            deg = np.bincount(P.e_point[free[P.e_kf]], minlength=pts)
            shape = {"edges": int(P.n_edges), "edge_pairs": int(((deg * (deg + 1)) // 2).sum())}
            for nb in (1, BATCH):
                arg = P if nb == 1 else [P] * nb
                res, t = measure(ctx, lambda: opt.LocalInertialBA(arg))
                r = res if nb == 1 else res[0]
                out["liba_n%d_p%d_x%d" % (n, pts, nb)] = dict(t, iterations=int(r.iterations),
                                                              trials=int(r.trace[:, 2].sum()), **shape)
                print("liba_n%d_p%d_x%d" % (n, pts, nb), out["liba_n%d_p%d_x%d" % (n, pts, nb)], flush=True)
            G = O.synth_lba_graph(np.random.default_rng(n + pts), n_kf=n + 4, n_points=pts, n_fixed=4)
            res, t = measure(ctx, lambda: opt.LocalBundleAdjustment(G))
            # the context's kernel timer is not set by this entry point: wall time only
            out["lba_n%d_p%d_x1" % (n, pts)] = dict(wall_us=t["wall_us"], edges=int(len(G.e_kind)))
            print("lba_n%d_p%d_x1" % (n, pts), out["lba_n%d_p%d_x1" % (n, pts)], flush=True)
    ctx.close()
    with open(os.path.join(ROOT, "profiles", "localinertialba_bench.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
