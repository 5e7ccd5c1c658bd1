#!/usr/bin/env python3
"""The bits of the four RANSAC / Sim3 modules' results on their committed fixtures.

One batched call per module over its BATCH fixture list (tests/sim3solver_fixtures.py, tests/mlpnp_fixtures.py,
tests/twoview_fixtures.py, tests/sim3opt_fixtures.py), every optional per-hypothesis array requested, and a
SHA-256 per fixture and result field: over an array's raw bytes, a scalar packed at its ABI width (int32 for
integers and flags, float32 or double as include/osg.h declares it).  Writes tests/golden/ransac_digests.json,
which tests/test_ransac_bits_gpu.py compares against.  The file is regenerated only by a change that means to
alter these kernels' arithmetic; its header names the commit and the ROCm version it was recorded with."""
import argparse
import dataclasses
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

GOLDEN = os.path.join(ROOT, "tests", "golden", "ransac_digests.json")
# scalars the ABI declares as float (every other floating scalar is a double)
FLOAT32 = {"sim3ransac": {"s"}, "twoview": {"score_h", "score_f"}}


def field_bytes(module, name, v):
    if isinstance(v, np.ndarray):
        return np.ascontiguousarray(v).tobytes()
    if isinstance(v, tuple):
        return np.asarray(v, np.int32).tobytes()
    if isinstance(v, (bool, int, np.bool_, np.integer)):
        return np.int32(v).tobytes()
    if isinstance(v, (float, np.floating)):
        return (np.float32 if name in FLOAT32.get(module, ()) else np.float64)(v).tobytes()
    raise TypeError("%s.%s: no packing for %r" % (module, name, type(v)))


def results(ctx):
    """{module: (fixture names, results of the one batched call)}"""
    from orb_slam3_comments_ghr_amd import mlpnpsolver, optimizer, sim3solver, twoview
    from orb_slam3_comments_ghr_amd.synth import EUROC_K
    from tests import mlpnp_fixtures, sim3opt_fixtures, sim3solver_fixtures, twoview_fixtures

    def run(fx, solve):
        return list(fx.BATCH), solve([fx.build(k) for k in fx.BATCH])

    return {"sim3ransac": run(sim3solver_fixtures, sim3solver.Sim3Solver(ctx).solve),
            "mlpnp": run(mlpnp_fixtures, mlpnpsolver.MLPnPsolver(ctx).solve),
            "twoview": run(twoview_fixtures, twoview.TwoViewReconstruction(ctx, EUROC_K).solve),
            "sim3opt": run(sim3opt_fixtures, optimizer.Optimizer(ctx).OptimizeSim3)}


def digests(ctx):
    """{module: {fixture: {field: sha256 hex}}}"""
    out = {}
    for module, (names, res) in results(ctx).items():
        assert len(names) == len(res)
        out[module] = {name: {f.name: hashlib.sha256(field_bytes(module, f.name, getattr(r, f.name))).hexdigest()
                              for f in dataclasses.fields(r)} for name, r in zip(names, res)}
    return out


def rocm_version():
    try:
        with open("/opt/rocm/.info/version") as f:
            return f.read().strip()
    except OSError:
        return "unknown"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", default=None, help="the commit the loaded library was built from (default: HEAD)")
    ap.add_argument("--out", default=GOLDEN)
    a = ap.parse_args()
    commit = a.commit or subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True,
                                        check=True).stdout.strip()
    from orb_slam3_comments_ghr_amd import Context

    ctx = Context(0)
    out = {"recorded_at_commit": commit, "rocm_version": rocm_version(), "device": "gfx950", "digests": digests(ctx)}
    ctx.close()
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", a.out, {m: len(v) for m, v in out["digests"].items()})


if __name__ == "__main__":
    sys.path.insert(0, ROOT)  # run as a script: the package and tests/ are imported from the repository
    main()
