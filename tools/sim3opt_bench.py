#!/usr/bin/env python3
"""Device time of osg_optimize_sim3 (csrc/sim3opt.hip), HIP events around the launch
(osg_ctx_last_kernel_ms): one M = 100 problem as single-call latency, and a batch of 256 such problems in
one launch.  Writes profiles/sim3opt_latency.json.  Recorded, not gated: the project has no CPU baseline
for this function, so no speed-up is claimed."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from orb_slam3_comments_ghr_amd import Context  # noqa: E402
from orb_slam3_comments_ghr_amd import optimizer as op  # noqa: E402


def timed(ctx, opt, probs, warmup, reps):
    for _ in range(warmup):
        opt.OptimizeSim3(probs)
    ms = []
    for _ in range(reps):
        res = opt.OptimizeSim3(probs)
        ms.append(ctx.last_kernel_ms())
    ms = np.array(ms)
    res = res if isinstance(res, list) else [res]
    return {"median_us": float(np.median(ms) * 1e3), "min_us": float(ms.min() * 1e3), "max_us": float(ms.max() * 1e3),
            "reps": reps, "lm_iterations": [int(sum(r.lm_iterations)) for r in res[:4]],
            "lm_trials": [int(sum(r.lm_trials)) for r in res[:4]]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=100)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sim3opt_latency.json"))
    a = ap.parse_args()
    ctx = Context(0)
    opt = op.Optimizer(ctx)
    probs = [op.synth_sim3_problem(np.random.default_rng(9000 + b), a.pairs, 0.1, 0.0, False) for b in range(a.batch)]
    single = timed(ctx, opt, probs[0], a.warmup, a.reps)
    batch = timed(ctx, opt, probs, a.warmup, max(5, a.reps // 5))
    batch["per_problem_us"] = batch["median_us"] / a.batch
    out = {"pairs": a.pairs, "edges": 2 * a.pairs, "single": single, "batch_size": a.batch, "batch": batch,
           "clock": "HIP events around the kernel launch (osg_ctx_last_kernel_ms)"}
    ctx.close()
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
