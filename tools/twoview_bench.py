#!/usr/bin/env python3
"""Device and wall time of osg_two_view_reconstruct (csrc/twoview.hip): one problem as single-call latency and
a batch of 64 such problems in the same five launches, at n = 300 and n = 2000 matches with 200 hypotheses.
Device time is HIP events around all launches (osg_ctx_last_kernel_ms); the per-kernel split comes from a
second series with events between the launches (osg_two_view_kernel_times), which adds their cost and is
reported apart; wall time is the whole ABI call through ctypes, staging, upload and download included (the
per-hypothesis arrays are requested).  Warm-up calls first, medians over the repetitions, one device.  Writes
profiles/twoview_bench.json.  Recorded, not gated: the project has no CPU baseline for this function, so no
speed-up is claimed and no time is asserted anywhere."""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from orb_slam3_comments_ghr_amd import Context  # noqa: E402
from orb_slam3_comments_ghr_amd import synth as SY  # noqa: E402
from orb_slam3_comments_ghr_amd import twoview as T  # noqa: E402

KERNELS = ("k_tvr_norm", "k_tvr_eval", "k_tvr_select", "k_tvr_checkrt", "k_tvr_final")


def timed(ctx, tv, probs, warmup, reps):
    for _ in range(warmup):
        tv.solve(probs)
    dev, wall = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        res = tv.solve(probs)
        wall.append(time.perf_counter() - t0)
        dev.append(ctx.last_kernel_ms())
    # the split: a series of its own, events between the launches
    ms = (ctypes.c_float * 5)()
    ctx.check(ctx.lib.osg_two_view_kernel_times(ctx.handle, 1, None), "osg_two_view_kernel_times")
    split = []
    for _ in range(max(3, reps // 2)):
        tv.solve(probs)
        ctx.check(ctx.lib.osg_two_view_kernel_times(ctx.handle, 1, ctypes.addressof(ms)), "osg_two_view_kernel_times")
        split.append([1e3 * v for v in ms])
    ctx.check(ctx.lib.osg_two_view_kernel_times(ctx.handle, 0, None), "osg_two_view_kernel_times")
    dev, wall = np.array(dev) * 1e3, np.array(wall) * 1e6
    res = res if isinstance(res, list) else [res]
    nb = len(res)
    return {"device_median_us": float(np.median(dev)), "device_min_us": float(dev.min()), "device_max_us": float(dev.max()),
            "device_per_problem_us": float(np.median(dev)) / nb, "wall_median_us": float(np.median(wall)),
            "wall_min_us": float(wall.min()), "reps": reps,
            "kernel_split_median_us": dict(zip(KERNELS, (float(v) for v in np.median(np.array(split), 0)))),
            "ok": [bool(r.ok) for r in res[:4]], "model": [int(r.model) for r in res[:4]]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--matches", type=int, nargs="*", default=[300, 2000])
    ap.add_argument("--hyp", type=int, default=200)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "twoview_bench.json"))
    a = ap.parse_args()
    ctx = Context(0)
    tv = T.TwoViewReconstruction(ctx, SY.EUROC_K)
    shapes = {}
    for n in a.matches:
        probs = [SY.two_view_scene(np.random.default_rng(7300 + b), n, outlier_frac=0.2, n_hyp=a.hyp, extra1=n // 2, extra2=n // 2)
                 for b in range(a.batch)]
        shapes[str(n)] = {"single": timed(ctx, tv, probs[0], a.warmup, a.reps),
                          "batch": timed(ctx, tv, probs, a.warmup, max(5, a.reps // 3))}
    try:
        import torch
        device = torch.cuda.get_device_name(0)
    except Exception:  # the name only
        device = "unknown"
    out = {"hypotheses": a.hyp, "batch_size": a.batch, "shapes": shapes, "device": device, "devices_used": 1,
           "clock": "device: HIP events around the five launches (osg_ctx_last_kernel_ms); kernel split: events between "
                    "the launches in a separate series; wall: time.perf_counter around TwoViewReconstruction.solve "
                    "(ctypes call, staging, upload, launches, download)"}
    ctx.close()
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
