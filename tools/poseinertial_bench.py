#!/usr/bin/env python3
"""Recorded time of osg_pose_inertial_optimization (not gated): HIP-event device time and wall time, medians of 20,
for one 318-edge pinhole-stereo frame and for batches of 64 and 256 such frames, both modes; beside them, for
context, k_pose_opt (PoseOptimization) on the same edge count in the same run.  No CPU baseline of the reference
exists here, so no speed-up over it is stated.

    python tools/poseinertial_bench.py            # writes profiles/poseinertial_bench.json
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

N_EDGES, REPS = 318, 20


def measure(ctx, fn):
    fn()
    dev, wall = [], []
    for _ in range(REPS):
        t = time.perf_counter()
        fn()
        wall.append((time.perf_counter() - t) * 1e6)
        dev.append(ctx.last_kernel_ms() * 1e3)
    return {"device_us": float(np.median(dev)), "wall_us": float(np.median(wall))}


def main():
    ctx = Context(0)
    opt = O.Optimizer(ctx)
    out = {"n_edges": N_EDGES, "reps": REPS, "camera": "pinhole_stereo"}
    for nb in (1, 64, 256):
        for mode, label in ((0, "last_keyframe"), (1, "last_frame")):
            probs = [O.synth_pose_inertial_problem(np.random.default_rng(1000 + i), N_EDGES, mode, "pinhole_stereo")
                     for i in range(nb)]
            out["%s_x%d" % (label, nb)] = measure(ctx, lambda: opt.pose_inertial_optimization_mixed(probs))
        probs = [O.synth_pose_problem(np.random.default_rng(2000 + i), N_EDGES) for i in range(nb)]
        out["pose_optimization_x%d" % nb] = measure(ctx, lambda: opt.PoseOptimization(probs))
    ctx.close()
    with open(os.path.join(ROOT, "profiles", "poseinertial_bench.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
