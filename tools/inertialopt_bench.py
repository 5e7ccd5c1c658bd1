#!/usr/bin/env python3
"""Recorded time of osg_inertial_optimization (not gated): HIP-event device time and wall time, medians of 10, of
overload 1 (monocular initialisation, Levenberg-Marquardt) for N = 10, 30, 100 and 300 KeyFrames, one map and a batch
of 256 maps, and of overload 3 (scale refinement, Gauss-Newton, 10 iterations) at N = 100; beside each the iterations
and trials the call ran, since the time is theirs.  No CPU time of the reference exists here, so no speed-up over it
is stated.

    python tools/inertialopt_bench.py            # writes profiles/inertialopt_bench.json
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
from tests import inertialopt_fixtures as FX  # noqa: E402

REPS = 10


def measure(ctx, fn):
    res = fn()
    dev, wall = [], []
    for _ in range(REPS):
        t = time.perf_counter()
        fn()
        wall.append((time.perf_counter() - t) * 1e6)
        dev.append(ctx.last_kernel_ms() * 1e3)
    res = res if isinstance(res, list) else [res]
    return {"device_us": float(np.median(dev)), "wall_us": float(np.median(wall)),
            "iterations": int(res[0].iterations), "trials": int(res[0].trace[:, 2].sum())}


def main():
    ctx = Context(0)
    opt = O.Optimizer(ctx)
    out = {"reps": REPS, "batch": 256}
    for n in (10, 30, 100, 300):
        FX.FIXTURES["bench"] = FX.Fixture(n, 50 + n, steps=8)
        FX.build.cache_clear()
        P = FX.build("bench")
        out["init_n%d_x1" % n] = measure(ctx, lambda: opt.InertialOptimization(P))
        batch = [P] * 256
        out["init_n%d_x256" % n] = measure(ctx, lambda: opt.InertialOptimization(batch))
        if n == 100:
            FX.FIXTURES["bench"] = FX.Fixture(n, 50 + n, kind="scale", steps=8)
            FX.build.cache_clear()
            Q = FX.build("bench")
            out["scale_n100_x1"] = measure(ctx, lambda: opt.InertialOptimization(Q))
            out["scale_n100_x256"] = measure(ctx, lambda: opt.InertialOptimization([Q] * 256))
    ctx.close()
    with open(os.path.join(ROOT, "profiles", "inertialopt_bench.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
