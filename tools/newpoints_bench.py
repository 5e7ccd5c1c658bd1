#!/usr/bin/env python3
"""Device and wall time of osg_create_new_map_points[_batch] (csrc/newpoints.hip): one current KeyFrame of 1200
keypoints against 10 and 30 neighbours of 1200 keypoints, pinhole monocular and stereo, as a single call and as a
batch of 16 current KeyFrames.

Device time is HIP events around the launches (osg_ctx_last_kernel_ms: k_triang, then k_np_eval + k_np_select).
The split comes from a separate series: the same pairs through osg_search_for_triangulation_batch alone give
k_triang's share, the rest is the two new kernels'.  Wall time is time.perf_counter around the ABI call through
ctypes with the structures prebuilt: the host merge-walk, staging, uploads, launches and downloads.  For context,
in the same run: the matching part alone by the route a caller had before this entry point, B successive
single-pair osg_search_for_triangulation calls (call-time MapPoint state, so the same queries).  Warm-up calls
first, medians over the repetitions, one device.  Writes profiles/newpoints_bench.json.  Recorded, not gated: no
CPU baseline of the reference loop is timed, so no speed-up over it is claimed, and no time is asserted anywhere."""
import argparse
import copy
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from orb_slam3_comments_ghr_amd import Context, _abi  # noqa: E402
from orb_slam3_comments_ghr_amd import localmapping as L  # noqa: E402


def first_neighbours(P, B):
    Q = copy.copy(P)
    Q.kf2, Q.g2, Q.geom = P.kf2[:B], P.g2[:B], P.geom[:B]
    return Q


def stats(dev_ms, wall_s):
    d, w = np.array(dev_ms) * 1e3, np.array(wall_s) * 1e6
    return {"device_median_us": float(np.median(d)), "device_min_us": float(d.min()), "device_max_us": float(d.max()),
            "wall_median_us": float(np.median(w)), "wall_min_us": float(w.min()), "reps": len(d)}


def timed(ctx, probs, warmup, reps):
    lib, h = ctx.lib, ctx.handle
    n = len(probs)
    keep = []
    st = (_abi.OsgNewPointsProblem * n)()
    rs = (_abi.OsgNewPointsResult * n)()
    outs = []
    for c, p in enumerate(probs):
        p.fill(st[c], keep)
        T = p.n_neigh * p.kf1.n
        o = (np.empty(T, np.int32), np.empty(T, np.uint8), np.empty(3 * T, np.float32), np.empty(p.n_neigh, np.uint8),
             np.empty(p.n_neigh, np.int32))
        rs[c].match, rs[c].status, rs[c].x3d, rs[c].skipped, rs[c].n_created = (int(a.ctypes.data) for a in o)
        outs.append(o)

    def call():
        if n == 1:
            return lib.osg_create_new_map_points(h, C.byref(st[0]), C.byref(rs[0]))
        return lib.osg_create_new_map_points_batch(h, C.addressof(st), C.addressof(rs), n)

    for _ in range(warmup):
        ctx.check(call(), "osg_create_new_map_points")
    dev, wall = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        rc = call()
        wall.append(time.perf_counter() - t0)
        dev.append(ctx.last_kernel_ms())
    r = stats(dev, wall)
    r["created"] = int(ctx.check(rc, "osg_create_new_map_points"))
    r["matches"] = int(sum((o[0] >= 0).sum() for o in outs))
    # the matching part alone, (a) as one batch launch: k_triang's share of the device time above
    k1 = (_abi.OsgKfSide * sum(p.n_neigh for p in probs))()
    k2 = (_abi.OsgKfSide * len(k1))()
    g = (_abi.OsgTriangGeom * len(k1))()
    q = 0
    for p in probs:
        for b in range(p.n_neigh):
            k1[q], k2[q], g[q] = p.kf1.struct(), p.kf2[b].struct(), p.geom[b].struct()
            q += 1
    m12 = np.empty(sum(p.n_neigh * p.kf1.n for p in probs), np.int32)
    nm = np.empty(len(k1), np.int32)
    dev_t = []
    for it in range(warmup + reps):
        ctx.check(lib.osg_search_for_triangulation_batch(h, C.addressof(k1), C.addressof(k2), C.addressof(g), len(k1), 0, 0,
                                                         0, m12.ctypes.data, nm.ctypes.data), "triang batch")
        if it >= warmup:
            dev_t.append(ctx.last_kernel_ms())
    r["k_triang_median_us"] = float(np.median(dev_t) * 1e3)
    r["k_np_eval_select_median_us"] = r["device_median_us"] - r["k_triang_median_us"]
    # (b) as the successive single-pair calls a caller made before
    dev_s, wall_s = [], []
    for it in range(warmup + reps):
        d, t0 = 0.0, time.perf_counter()
        off = 0
        for q in range(len(k1)):
            ctx.check(lib.osg_search_for_triangulation(h, C.byref(k1[q]), C.byref(k2[q]), C.byref(g[q]), 0, 0, 0,
                                                       m12.ctypes.data + 4 * off), "triang")
            d += ctx.last_kernel_ms()
            off += k1[q].n
        if it >= warmup:
            wall_s.append(time.perf_counter() - t0)
            dev_s.append(d)
    r["matching_alone_single_pair_calls"] = stats(dev_s, wall_s)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keypoints", type=int, default=1200)
    ap.add_argument("--neighbours", type=int, nargs="*", default=[10, 30])
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "newpoints_bench.json"))
    a = ap.parse_args()
    ctx = Context(0)
    cases = {}
    n = a.keypoints
    for kind, kw in (("mono", dict(common=0.15, mp_frac=0.3)),
                     ("stereo", dict(stereo=True, near_frac=0.2, common=0.15, mp_frac=0.3))):
        full = [L.synth_newpoints_problem(np.random.default_rng(9100 + c), B=max(a.neighbours), n1=n, n2=n, n_nodes=100,
                                          **kw) for c in range(a.batch)]
        for B in a.neighbours:
            probs = [first_neighbours(p, B) for p in full]
            cases["%s_B%d" % (kind, B)] = {"single": timed(ctx, probs[:1], a.warmup, a.reps),
                                           "batch": timed(ctx, probs, a.warmup, max(5, a.reps // 3))}
    try:
        import torch
        device = torch.cuda.get_device_name(0)
    except Exception:  # the name only
        device = "unknown"
    out = {"keypoints": n, "batch_size": a.batch, "cases": cases, "device": device, "devices_used": 1,
           "clock": "device: HIP events around the launches (osg_ctx_last_kernel_ms), k_triang's share from a separate "
                    "series of osg_search_for_triangulation_batch on the same pairs; wall: time.perf_counter around the "
                    "ABI call through ctypes, structures prebuilt"}
    ctx.close()
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
