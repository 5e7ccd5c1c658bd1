"""GPU: the monocular start-up chain of Tracking::MonocularInitialization (ref:src/Tracking.cc:2941-2975) on a
tests/mono_chain.py-style world: two frames of a seeded static scene (EuRoC cam0 intrinsics, points 3 .. 9 m in
front of the trajectory's frames 0 and 25, 0.5 px keypoint noise, descriptors with 3 % flipped bits, 10 %
clutter) go through SearchForInitialization and then TwoViewReconstruction::Reconstruct.

The result must be an initialisation (ok), and T21 must agree with the world's truth as well as the numpy
restatement does on the same matches and sets: its own error is the scene's noise-induced error, and the GPU
may add the recorded spread of the general fixture group (10 x, profiles/twoview_margins.json)."""
import numpy as np
import pytest

from orb_slam3_comments_ghr_amd import frames as fr
from orb_slam3_comments_ghr_amd import twoview as T
from orb_slam3_comments_ghr_amd.matcher import ORBmatcher
from orb_slam3_comments_ghr_amd.synth import EUROC_CX, EUROC_CY, EUROC_FX, EUROC_FY, EUROC_H, EUROC_W
from tests import mono_chain as MC
from tests import pyref_twoview as R
from tests import twoview_fixtures as FX

pytestmark = pytest.mark.gpu


def pose(k):
    """mono_chain.World's trajectory"""
    c = np.array([0.02 * k, 0.004 * np.sin(0.3 * k), 0.01 * k])
    yaw = np.deg2rad(0.15 * k)
    Rm = np.array([[np.cos(yaw), 0, np.sin(yaw)], [0, 1, 0], [-np.sin(yaw), 0, np.cos(yaw)]]).T
    return Rm, -Rm @ c


def frame(rng, P, D, theta, k, n_clutter):
    Rm, t = pose(k)
    Xc = P @ Rm.T + t
    u = EUROC_FX * Xc[:, 0] / Xc[:, 2] + EUROC_CX
    v = EUROC_FY * Xc[:, 1] / Xc[:, 2] + EUROC_CY
    vis = np.flatnonzero((Xc[:, 2] > 0.5) & (u > 8) & (u < EUROC_W - 8) & (v > 8) & (v < EUROC_H - 8))
    n = len(vis)
    x = np.concatenate([u[vis] + rng.normal(0, 0.5, n), rng.uniform(8, EUROC_W - 8, n_clutter)])
    y = np.concatenate([v[vis] + rng.normal(0, 0.5, n), rng.uniform(8, EUROC_H - 8, n_clutter)])
    ang = np.concatenate([(theta[vis] + rng.normal(0, 2, n)) % 360, rng.uniform(0, 360, n_clutter)])
    desc = np.concatenate([D[vis] ^ np.packbits(rng.random((n, 256)) < 0.03, axis=1),
                           rng.integers(0, 256, (n_clutter, 32), dtype=np.uint8)])
    truth = np.concatenate([vis, -np.ones(n_clutter, np.int64)])
    order = rng.permutation(len(x))
    # the initialisation matches level-0 keypoints only (ref:src/ORBmatcher.cc:751-753)
    F = fr.FrameSoA(desc=desc[order], kp_x=x[order], kp_y=y[order], kp_angle=ang[order],
                    kp_octave=np.zeros(len(x), np.int32), min_x=0.0, max_x=float(EUROC_W), min_y=0.0, max_y=float(EUROC_H),
                    scale=MC.SCALES)
    return F, truth[order]


def test_search_for_initialization_then_reconstruct(ctx):
    rng = np.random.default_rng(0x1517)
    n_points = 700
    P = np.stack([rng.uniform(-6, 6, n_points), rng.uniform(-3, 3, n_points), rng.uniform(3, 9, n_points)], 1)
    D = rng.integers(0, 256, (n_points, 32), dtype=np.uint8)
    theta = rng.uniform(0, 360, n_points).astype(np.float32)
    (F1, t1), (F2, t2) = frame(rng, P, D, theta, 0, 40), frame(rng, P, D, theta, 25, 40)
    prev = np.stack([F1.kp_x, F1.kp_y], 1).astype(np.float32)
    n, m12 = ORBmatcher(ctx, nnratio=0.9, checkOri=True).SearchForInitialization(F1, F2, prev, 100)
    right = int(np.sum((m12 >= 0) & (t1 >= 0) & (t1 == t2[np.maximum(m12, 0)])))
    print("matches", n, "of them right", right)
    assert n >= 100 and right >= 0.9 * n  # Tracking asks for 100 (ref:src/Tracking.cc:2959)
    keys1 = np.stack([F1.kp_x, F1.kp_y], 1)
    keys2 = np.stack([F2.kp_x, F2.kp_y], 1)
    tv = T.TwoViewReconstruction(ctx, (EUROC_FX, EUROC_FY, EUROC_CX, EUROC_CY), sigma=1.0, iterations=200)
    prob = tv.problem(keys1, keys2, m12)
    got = tv.solve(prob)
    ref = R.reconstruct(prob)
    R1, c1 = pose(0)
    R2, c2 = pose(25)
    R21 = R2 @ R1.T
    t21 = c2 - R21 @ c1
    tol = FX.tolerances("n100_general")
    rot_ref, t_ref = FX.rot_angle(ref.R, R21), FX.dir_angle(ref.t, t21)
    rot, tdir = FX.rot_angle(got.R, R21), FX.dir_angle(got.t, t21)
    print("ok", got.ok, ref.ok, "model", got.model, ref.model, "rot", rot, "pyref", rot_ref, "+", tol["rot_rad"], "t", tdir, "pyref", t_ref,
          "+", tol["t_rad"], "triangulated", int(got.triangulated.sum()))
    assert ref.ok and got.ok and got.model == ref.model
    assert rot <= rot_ref + tol["rot_rad"] and tdir <= t_ref + tol["t_rad"]
    assert got.triangulated.sum() >= 50 and not got.triangulated[m12 < 0].any()
    # the points are in frame 1 up to the unknown scale (|t21| of the world is the unit): as far from the world's
    # as the restatement's are, plus the recorded spread
    k = np.flatnonzero(got.triangulated & ref.triangulated & (t1 >= 0))
    X1 = (P[t1[k]] @ R1.T + c1) / np.linalg.norm(t21)
    rel = np.linalg.norm(got.p3d[k] - X1, axis=1) / np.linalg.norm(X1, axis=1)
    rel_ref = np.linalg.norm(ref.p3d[k] - X1, axis=1) / np.linalg.norm(X1, axis=1)
    print("median relative point error", float(np.median(rel)), "pyref", float(np.median(rel_ref)), "+", tol["p3d_rel"])
    assert len(k) >= 50 and np.median(rel) <= np.median(rel_ref) + tol["p3d_rel"]
