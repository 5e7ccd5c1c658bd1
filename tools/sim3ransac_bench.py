#!/usr/bin/env python3
"""Device and wall time of osg_sim3_ransac (csrc/sim3ransac.hip): one N = 100, H = 300 problem as
single-call latency, and a batch of 16 such problems in one pair of launches.  Device time is HIP events
around both launches (osg_ctx_last_kernel_ms); wall time is the whole ABI call through ctypes, uploads and
downloads included (the per-hypothesis arrays are requested, as the adapter requests them).  Writes
profiles/sim3ransac_latency.json.  Recorded, not gated: the project has no CPU baseline for this function,
so no speed-up is claimed."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from orb_slam3_comments_ghr_amd import Context  # noqa: E402
from orb_slam3_comments_ghr_amd import sim3solver as S3  # noqa: E402


def timed(ctx, solver, probs, warmup, reps):
    for _ in range(warmup):
        solver.solve(probs)
    dev, wall = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        res = solver.solve(probs)
        wall.append(time.perf_counter() - t0)
        dev.append(ctx.last_kernel_ms())
    dev, wall = np.array(dev) * 1e3, np.array(wall) * 1e6
    res = res if isinstance(res, list) else [res]
    return {"device_median_us": float(np.median(dev)), "device_min_us": float(dev.min()), "device_max_us": float(dev.max()),
            "wall_median_us": float(np.median(wall)), "wall_min_us": float(wall.min()), "reps": reps,
            "converged": [bool(r.converged) for r in res[:4]], "n_iterations": [int(r.n_iterations) for r in res[:4]]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--matches", type=int, default=100)
    ap.add_argument("--hyp", type=int, default=300)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sim3ransac_latency.json"))
    a = ap.parse_args()
    ctx = Context(0)
    solver = S3.Sim3Solver(ctx)
    probs = [S3.synth_sim3_ransac_problem(np.random.default_rng(9100 + b), a.matches, 0.3, False, min_inliers=20,
                                          n_hyp=a.hyp) for b in range(a.batch)]
    single = timed(ctx, solver, probs[0], a.warmup, a.reps)
    batch = timed(ctx, solver, probs, a.warmup, max(5, a.reps // 2))
    batch["device_per_problem_us"] = batch["device_median_us"] / a.batch
    out = {"matches": a.matches, "hypotheses": a.hyp, "single": single, "batch_size": a.batch, "batch": batch,
           "clock": "device: HIP events around both launches (osg_ctx_last_kernel_ms); wall: time.perf_counter "
                    "around Sim3Solver.solve (ctypes call, staging, upload, both launches, download)"}
    ctx.close()
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
