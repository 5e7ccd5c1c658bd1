#!/usr/bin/env python3
"""Recorded time of osg_imu_preintegrate_batch (not gated): HIP-event device time of k_imu_preintegrate and wall time
of the C call (the structs prepared beforehand), median and range of 20 after one warm-up call, for (B, n) = (1, 10),
(2, 10), (256, 100), (1024, 100), (4096, 100), (1024, 600).  (2, 10) is Tracking::PreintegrateIMU's call: one list
onto two states.  No binary of the reference exists here, so no speed-up over it is stated.

    python tools/preintegration_bench.py          # writes profiles/preintegration_bench.json
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from orb_slam3_comments_ghr_amd import Context, _abi, imu  # noqa: E402
from tests import preintegration_fixtures as FX  # noqa: E402

SHAPES = ((1, 10), (2, 10), (256, 100), (1024, 100), (4096, 100), (1024, 600))
REPS = 20


def problems(B, n):
    nga, walk = FX.noise()
    rng = np.random.default_rng(B * 1000 + n)
    out = []
    for i in range(B):
        if B == 2 and i == 1:     # the frame's second state: the same list
            out.append(imu.ImuProblem(out[0].meas, out[0].bias + np.float32(1e-3), nga, walk))
            continue
        a, w, t = FX.imu_points(rng, n + 1)
        meas = np.zeros((n, 7), np.float32)
        meas[:, 0:3], meas[:, 3:6] = (a[:-1] + a[1:]) * np.float32(0.5), (w[:-1] + w[1:]) * np.float32(0.5)
        meas[:, 6] = (t[1:] - t[:-1]).astype(np.float32)
        out.append(imu.ImuProblem(meas, rng.normal(0, 0.01, 6), nga, walk))
    return out


def stats(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def measure(ctx, probs):
    keep = []
    ps = (_abi.OsgImuProblem * len(probs))(*[q.struct(keep) for q in probs])
    out = (_abi.OsgImuPreintegrated * len(probs))()
    call = lambda: ctx.check(ctx.lib.osg_imu_preintegrate_batch(ctx.handle, ps, len(probs), out), "bench")  # noqa: E731
    call()
    dev, wall = [], []
    for _ in range(REPS):
        t = time.perf_counter()
        call()
        wall.append((time.perf_counter() - t) * 1e6)
        dev.append(ctx.last_kernel_ms() * 1e3)
    return {"device_us": stats(dev), "wall_us": stats(wall)}


def main():
    ctx = Context(0)
    res = {"reps": REPS, "waves_per_workgroup": imu.WAVES_PER_WORKGROUP, "shapes": {}}
    for B, n in SHAPES:
        probs = problems(B, n)
        row = measure(ctx, probs)
        row["device_us_per_step"] = row["device_us"]["median"] / n
        res["shapes"]["B%d_n%d" % (B, n)] = row
        print(B, n, json.dumps(row), flush=True)
    ctx.close()
    with open(os.path.join(ROOT, "profiles", "preintegration_bench.json"), "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
