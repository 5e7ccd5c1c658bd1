"""OptimizeSim3 through the ORB-SLAM3-side adapter (adapters/orbslam3/osg_orbslam3.h: Sim3Gather,
optimize_sim3, apply_optimize_sim3) on the mock KeyFrames / MapPoints of tests/adapter/mock_orbslam3.h,
driven by tests/adapter/sim3opt_driver.cpp.

* CPU: the graph build (pure host code) on a KeyFrame pair that takes every branch of the reference's
  slot filter equals a Python restatement of ref:src/Optimizer.cc:4272-4425, order and vnIndexEdge
  included, with bAllPoints off and on.
* GPU: gather -> ABI -> write-back gives the vpMatches1, the return value, the Sim3 write-back and the
  mAcumHessian handling of the literal flow driven by tests/pyref_sim3opt.py, on a problem that survives
  and on one that takes the < 10 early return.
"""
import os
import subprocess

import numpy as np
import pytest

from orb_slam3_comments_ghr_amd import optimizer as op
from tests import pyref_sim3opt as R
from tools.adapter_arrays import read_arrays, write_arrays

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER_SRC = os.path.join(ROOT, "tests", "adapter", "sim3opt_driver.cpp")
PKG = os.path.join(ROOT, "orb_slam3_comments_ghr_amd")
ISIG = op.inv_level_sigma2()


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sim3opt") / "sim3opt_driver")
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-Wno-unused-result", "-ffp-contract=off",
                        "-I" + os.path.join(ROOT, "include"), DRIVER_SRC, "-o", exe, "-L" + PKG, "-lorbslam3_amd",
                        "-Wl,-rpath," + PKG], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def run(driver, tmp_path, mode, arrays):
    fi, fo = str(tmp_path / f"{mode}.in"), str(tmp_path / f"{mode}.out")
    write_arrays(fi, arrays)
    r = subprocess.run([driver, mode, fi, fo], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    return read_arrays(fo)


# ------------------------------------------------------------------------------------ the mock world
def cam_point(pose, X):
    """The mock hook's Rcw * Xw + tcw: the rotation matrix of pose[:4] in double, everything cast to float,
    the products summed left to right in float."""
    Rf = R.quat_to_rot(pose[:4]).astype(np.float32)
    Xf = np.asarray(X, np.float64).astype(np.float32)
    tf = np.asarray(pose[4:], np.float64).astype(np.float32)
    out = np.zeros(3, np.float32)
    for r in range(3):
        v = Rf[r, 0] * Xf[0]
        v = v + Rf[r, 1] * Xf[1]
        v = v + Rf[r, 2] * Xf[2]
        out[r] = v + tf[r]
    return out


def make_world(seed, n_pairs, outlier_frac, special=True):
    """A KeyFrame pair around a synthetic Sim3 problem: pair i becomes slot i of KeyFrame 1 with its own
    MapPoint and a matched MapPoint observed in KeyFrame 2 at a shuffled index.  ``special`` then rewires a
    few slots so that every branch of the reference's filter is taken."""
    rng = np.random.default_rng(seed)
    P = op.synth_sim3_problem(rng, n_pairs, outlier_frac, 0.0, False)
    n = n_pairs
    pose1 = np.concatenate([op.rot_to_quat(op.small_rotation(rng, 20.0)), rng.normal(0, 1.0, 3)])
    pose2 = np.concatenate([op.rot_to_quat(op.small_rotation(rng, 20.0)), rng.normal(0, 1.0, 3)])
    R1, R2 = R.quat_to_rot(pose1[:4]), R.quat_to_rot(pose2[:4])
    pos = np.concatenate([(P.p1c - pose1[4:]) @ R1, (P.p2c - pose2[4:]) @ R2])  # pool: MP1_i = i, MP2_i = n + i
    bad = np.zeros(2 * n, np.uint8)
    perm = rng.permutation(n)                      # pair i's keypoint index in KeyFrame 2
    kf2idx = np.concatenate([-np.ones(n, np.int32), perm.astype(np.int32)])
    mp1 = np.arange(n, dtype=np.int32)
    match = np.arange(n, 2 * n, dtype=np.int32)
    oct1 = np.array([int(np.nonzero(ISIG == w)[0][0]) for w in P.inv_sigma2_1], np.int32)
    oct2 = np.array([int(np.nonzero(ISIG == w)[0][0]) for w in P.inv_sigma2_2], np.int32)
    kp2 = np.zeros((n, 2), np.float32)
    o2 = np.zeros(n, np.int32)
    kp2[perm] = P.obs2.astype(np.float32)
    o2[perm] = oct2
    if special:
        match[0] = -1                       # no match
        bad[mp1[1]] = 1                     # both MapPoints there, KeyFrame 1's bad
        bad[match[2]] = 1                   # both there, the matched one bad
        mp1[3] = -1                         # no MapPoint in KeyFrame 1: no edges
        mp1[4] = -1
        bad[match[4]] = 1                   # ... whether the matched one is bad or not
        kf2idx[match[5]] = -1               # not observed in KeyFrame 2: kept only under bAllPoints
        kf2idx[match[6]] = -1
        pos[match[7]] = (np.array([0.3, -0.2, -1.5]) - pose2[4:]) @ R2   # behind KeyFrame 2: P3D2c(2) < 0
        pos[mp1[8]] = (np.array([0.2, 0.1, -2.0]) - pose1[4:]) @ R1      # behind KeyFrame 1: NOT tested, kept
    arrays = {"kf1.pose": pose1, "kf2.pose": pose2, "isig": ISIG.astype(np.float32),
              "kf1.cam": np.array([P.cam1.type] + [P.cam1.p[i] for i in range(8)], np.float32),
              "kf2.cam": np.array([P.cam2.type] + [P.cam2.p[i] for i in range(8)], np.float32),
              "kf1.kp": P.obs1.astype(np.float32).reshape(-1), "kf1.oct": oct1,
              "kf2.kp": kp2.reshape(-1), "kf2.oct": o2, "mp.pos": pos.reshape(-1), "mp.bad": bad,
              "mp.kf2idx": kf2idx.astype(np.int32), "slot.mp1": mp1, "slot.match": match,
              "sim3": np.concatenate([P.q, P.t, [P.s]])}
    return P, arrays


def restate_gather(P, a, th2, fix_scale, all_points):
    """ref:src/Optimizer.cc:4272-4425 on the mock world, literally."""
    pos = a["mp.pos"].reshape(-1, 3)
    kp1, kp2 = a["kf1.kp"].reshape(-1, 2), a["kf2.kp"].reshape(-1, 2)
    rows, index, in_kf2 = [], [], []
    for i in range(len(a["slot.match"])):
        if a["slot.match"][i] < 0:
            continue
        m1, m2 = int(a["slot.mp1"][i]), int(a["slot.match"][i])
        i2 = int(a["mp.kf2idx"][m2])
        if m1 >= 0:
            if not a["mp.bad"][m1] and not a["mp.bad"][m2]:
                P1 = cam_point(a["kf1.pose"], pos[m1])
                P2 = cam_point(a["kf2.pose"], pos[m2])
            else:
                continue
        else:
            continue
        if i2 < 0 and not all_points:
            continue
        if P2[2] < 0:
            continue
        w1 = ISIG[a["kf1.oct"][i]]
        if i2 >= 0:
            obs2, w2 = kp2[i2].astype(np.float64), ISIG[a["kf2.oct"][i2]]
        else:
            invz = np.float32(1) / P2[2]
            obs2, w2 = np.array([P2[0] * invz, P2[1] * invz], np.float64), ISIG[0]
        rows.append((P1.astype(np.float64), P2.astype(np.float64), kp1[i].astype(np.float64), obs2, w1, w2))
        index.append(i)
        in_kf2.append(int(i2 >= 0))
    z = lambda k, w: np.array([r[k] for r in rows], np.float64).reshape(-1, w)  # noqa: E731
    Q = op.Sim3Problem(P.q, P.t, P.s, z(0, 3), z(1, 3), z(2, 2), z(3, 2), np.array([r[4] for r in rows], np.float32),
                       np.array([r[5] for r in rows], np.float32), fix_scale=fix_scale, th2=th2, cam1=P.cam1, cam2=P.cam2)
    return Q, np.array(index, np.int32), np.array(in_kf2, np.uint8)


# ------------------------------------------------------------------------------------ CPU: the gather
def test_optimize_sim3_driver_compiles(driver):
    assert os.path.exists(driver)


@pytest.mark.parametrize("all_points", [False, True])
def test_adapter_gather_optimize_sim3(driver, tmp_path, all_points):
    P, a = make_world(4100, 24, 0.1)
    a["params"] = np.array([10.0, 1.0, float(all_points)], np.float32)
    out = run(driver, tmp_path, "gather", a)
    Q, index, in_kf2 = restate_gather(P, a, 10.0, True, all_points)
    # the branches: slots 0-4 and 7 never kept, 5 and 6 only under bAllPoints, 8 kept despite its depth
    assert not set(index) & {0, 1, 2, 3, 4, 7} and 8 in index
    assert ({5, 6} <= set(index)) == all_points
    assert Q.p1c[list(index).index(8), 2] < 0
    np.testing.assert_array_equal(out["index"], index)
    np.testing.assert_array_equal(out["in_kf2"], in_kf2)
    assert list(out["n_pairs"]) == [len(index), 1, P.cam1.type, P.cam2.type]
    assert out["th2"][0] == np.float32(10.0) and out["th2"][1] == np.float32(P.cam1.p[0])
    for k, ref in (("p1c", Q.p1c), ("p2c", Q.p2c), ("obs1", Q.obs1), ("obs2", Q.obs2), ("w1", Q.inv_sigma2_1),
                   ("w2", Q.inv_sigma2_2)):
        np.testing.assert_array_equal(out[k].reshape(ref.shape), ref, err_msg=k)
    if all_points:  # normalised coordinates and the level-0 weight, not pixels
        j = list(index).index(5)
        assert abs(Q.obs2[j]).max() < 2.0 and Q.inv_sigma2_2[j] == ISIG[0] and not in_kf2[j]


# ------------------------------------------------------------------------------------ GPU: the whole call
@pytest.mark.gpu
@pytest.mark.parametrize("seed,n_pairs", [(4200, 70), (4211, 18)])
def test_adapter_optimize_sim3(driver, tmp_path, ctx, seed, n_pairs):
    """70 slots: the second optimisation runs and the Sim3 and mAcumHessian are written; 18 slots of which
    9 are filtered out: the < 10 early return, which keeps the first classification's nullings and leaves
    the Sim3 and mAcumHessian alone."""
    P, a = make_world(seed, n_pairs, 0.1)
    a["params"] = np.array([10.0, 0.0, 1.0], np.float32)
    if n_pairs == 18:  # drop 3 more slots: 18 - 6 (slots 0-4, 7) - 3 = 9 correspondences
        a["slot.match"][[10, 11, 12]] = -1
    Q, index, _ = restate_gather(P, a, 10.0, False, True)
    ref = R.optimize_sim3(Q)
    margin, _ = R.guard_report(Q, ref, [])
    assert margin > 1e-3, "pick another seed: a chi2 sits on the threshold"
    assert ref.early_return == (n_pairs == 18) and (ref.early_return or ref.n_inliers >= 10)
    # the literal flow of :4436-4511 on pyref's classification
    null_ref = a["slot.match"] < 0
    null_ref[index[ref.pair_state != 0]] = True
    assert ref.n_bad_first > 0
    out = run(driver, tmp_path, "optimize", a)
    np.testing.assert_array_equal(out["match_null"].astype(bool), null_ref)
    assert int(out["ret"][0]) == ref.n_inliers
    direct = op.Optimizer(ctx).OptimizeSim3(Q)  # the same graph through the C ABI directly
    if ref.early_return:
        assert int(out["ret"][0]) == 0
        np.testing.assert_array_equal(out["sim3"], a["sim3"])
        np.testing.assert_array_equal(out["hess"], np.full(49, 7.0))
    else:
        np.testing.assert_array_equal(out["sim3"], np.concatenate([direct.q, direct.t, [direct.s]]))
        np.testing.assert_array_equal(out["hess"], np.zeros(49))
        assert R.rot_log_norm(R.quat_to_rot(out["sim3"][:4] / np.linalg.norm(out["sim3"][:4])), ref.R) < 1e-4
