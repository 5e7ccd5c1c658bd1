#!/usr/bin/env python3
"""Device and wall time of the per-frame projection step of Tracking::SearchLocalPoints (csrc/frustum.hip,
osg_search_local_points in csrc/match.hip): 2 000 and 4 000 local MapPoints against frames of 1 200 keypoints,
pinhole stereo, B = 64 frames per call.

  * k_frustum's device time: HIP events around the launch of osg_frustum_batch (osg_ctx_last_kernel_ms);
  * wall time of the fused osg_search_local_points_batch against the two-step path on the same tree
    (osg_frustum_batch, the host step that forms osg_mp_queries, osg_search_by_projection_mps_batch), through
    ctypes with time.perf_counter around the calls;
  * what the parent commit offers, one frame at a time at the adapter's level (tests/adapter/tracking_driver.cpp in
    its timing mode): the literal isInFrustum loop on the CPU over scattered MapPoint objects, then the
    SearchByProjection adapter call, against the adapter's fused SearchLocalPoints.

Warm-up calls first, medians over the repetitions, one device.  Writes profiles/frustum_bench.json.  Recorded,
not gated: no time is asserted anywhere."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from orb_slam3_comments_ghr_amd import Context  # noqa: E402
from orb_slam3_comments_ghr_amd import tracking as T  # noqa: E402
from orb_slam3_comments_ghr_amd.matcher import ORBmatcher  # noqa: E402
from tests import frustum_fixtures as FX  # noqa: E402
from tests import pyref_frustum as PF  # noqa: E402
from tools.adapter_arrays import read_arrays, write_arrays  # noqa: E402

PKG = os.path.join(ROOT, "orb_slam3_comments_ghr_amd")


def case(n, seed):
    frame, pts = FX.random_fixture(seed, "ps", n, pool_factor=8)
    return FX.make_fused(frame, pts, PF.search_local_points_step2(frame, pts), "ps", seed + 5000, n_kp=1200)


def median_us(f, warmup, reps):
    for _ in range(warmup):
        f()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        t.append(time.perf_counter() - t0)
    return float(np.median(t) * 1e6)


def measure(ctx, n, B, warmup, reps, driver):
    cs = [case(n, 4000 + n + b) for b in range(min(B, 4))]
    cs = [cs[b % len(cs)] for b in range(B)]
    Fs, frames, pts = [c.F for c in cs], [c.frame for c in cs], [c.points for c in cs]
    takens = [c.slot_taken for c in cs]
    c0 = cs[0]
    m = ORBmatcher(ctx, 0.8)
    dev = []

    def frustum_only():
        T.frustum_batch(ctx, frames, pts)
        dev.append(ctx.last_kernel_ms() * 1e3)

    def two_step():
        outs = T.frustum_batch(ctx, frames, pts)
        qs = [T.mp_queries(p, o) for p, o in zip(pts, outs)]
        m.SearchByProjectionBatch(Fs, qs, c0.th, c0.far_points, c0.th_far, slot_mps=[c.slot_mp.copy() for c in cs],
                                  slot_takens=takens)

    def fused():
        T.search_local_points_batch(ctx, Fs, frames, pts, th=c0.th, far_points=c0.far_points, th_far_points=c0.th_far,
                                    slot_mps=[c.slot_mp.copy() for c in cs], slot_takens=takens)

    r = {"points": n, "frames": B, "keypoints": int(c0.F.n), "n_to_match": int(np.mean(
        [PF.search_local_points_step2(c.frame, c.points).n_to_match for c in cs[:1]]))}
    r["frustum_batch_wall_us"] = median_us(frustum_only, warmup, reps)
    r["k_frustum_device_us"] = float(np.median(dev[warmup:]))
    r["two_step_batch_wall_us"] = median_us(two_step, warmup, reps)
    r["fused_batch_wall_us"] = median_us(fused, warmup, reps)
    fused()
    r["fused_device_us"] = ctx.last_kernel_ms() * 1e3
    with tempfile.TemporaryDirectory() as d:
        fi, fo = os.path.join(d, "w.in"), os.path.join(d, "w.out")
        write_arrays(fi, FX.adapter_world(c0, int(c0.th)))
        subprocess.run([driver, fi, fo, str(reps)], check=True, timeout=300)
        b = read_arrays(fo)["bench_us"]
    r["adapter_one_frame_us"] = {"cpu_isInFrustum_loop": float(b[0]), "search_by_projection_call": float(b[1]),
                                 "parent_total": float(b[0] + b[1]), "fused_search_local_points": float(b[2])}
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, nargs="*", default=[2000, 4000])
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frustum_bench.json"))
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as d:
        driver = os.path.join(d, "tracking_driver")
        subprocess.run(["g++", "-std=c++17", "-O2", "-Wno-unused-result", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "adapter", "tracking_driver.cpp"), "-o", driver, "-L" + PKG,
                        "-lorbslam3_amd", "-Wl,-rpath," + PKG], check=True)
        ctx = Context(0)
        res = {"what": __doc__.split("\n\n")[0], "rows": [measure(ctx, n, a.frames, a.warmup, a.reps, driver) for n in a.points]}
        ctx.close()
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    for r in res["rows"]:
        print(json.dumps(r))


if __name__ == "__main__":
    main()
