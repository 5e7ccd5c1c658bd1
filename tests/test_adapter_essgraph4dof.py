"""OptimizeEssentialGraph4DoF through the ORB-SLAM3-side adapter (adapters/orbslam3/osg_orbslam3.h:
EssentialGraph4DoFGather, essential_graph_4dof_points, optimize_essential_graph_4dof) on the mock map of
tests/adapter/mock_essgraph4dof.h, driven by tests/adapter/essgraph4dof_driver.cpp.

* CPU: the gathered vertices (both constructors' arithmetic), edge list and measurements (the scale dropped)
  equal a Python restatement of ref:src/Optimizer.cc:4903-5143 bit for bit, on a map that takes every branch
  (asserted below), and so do the MapPoint reference choice of :5182-5183 and the information's quirk.
* GPU: gather -> ABI -> write-back against the literal flow of :5146-5197 driven by
  tests/pyref_essgraph4dof.py.  The poses SetPose received are within the margins rule of
  tests/test_essgraph4dof_gpu.py (10 x the spread of this graph's own 16-replica study, or the floor 1e-6) of
  pyref's, after the float casts.  The MapPoints are within 1 float ulp of the correction driven by the same
  optimised poses the KeyFrames were set from.
"""
import math
import os
import subprocess

import numpy as np
import pytest

from orb_slam3_comments_ghr_amd import optimizer as op
from tests import essgraph4dof_fixtures as FX
from tests import pyref_essgraph as EG
from tests import pyref_essgraph4dof as R
from tests import test_adapter_essgraph as AE
from tools.adapter_arrays import read_arrays, write_arrays

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER_SRC = os.path.join(ROOT, "tests", "adapter", "essgraph4dof_driver.cpp")
PKG = os.path.join(ROOT, "orb_slam3_comments_ghr_amd")
MIN_FEAT = 100
CUR, LOOP, BAD, GONE = AE.CUR, AE.LOOP, AE.BAD, AE.GONE


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("essgraph4dof") / "essgraph4dof_driver")
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


# ------------------------------------------------------------------------------------ Eigen in scalars
def q_to_rot(q):
    """QuaternionBase::toRotationMatrix, operation for operation, rows"""
    x, y, z, w = [float(v) for v in q[:4]]
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return [[1 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1 - (txx + tzz), tyz - twx], [txz - twy, tyz + twx, 1 - (txx + tyy)]]


def rot_to_quat(Rm):
    """the mock's rot_to_quat (the trace or the largest diagonal entry), (x y z w)"""
    Rm = [[float(v) for v in row] for row in np.asarray(Rm).reshape(3, 3)]
    t = Rm[0][0] + Rm[1][1] + Rm[2][2]
    q = [0.0] * 4
    if t > 0:
        t = math.sqrt(t + 1.0)
        q[3] = 0.5 * t
        t = 0.5 / t
        q[0], q[1], q[2] = (Rm[2][1] - Rm[1][2]) * t, (Rm[0][2] - Rm[2][0]) * t, (Rm[1][0] - Rm[0][1]) * t
    else:
        i = 0
        if Rm[1][1] > Rm[0][0]:
            i = 1
        if Rm[2][2] > Rm[i][i]:
            i = 2
        j, k = (i + 1) % 3, (i + 2) % 3
        t = math.sqrt(Rm[i][i] - Rm[j][j] - Rm[k][k] + 1.0)
        q[i] = 0.5 * t
        t = 0.5 / t
        q[3], q[j], q[k] = (Rm[k][j] - Rm[j][k]) * t, (Rm[j][i] + Rm[i][j]) * t, (Rm[k][i] + Rm[i][k]) * t
    return q


def corrected_row(Scw, row):
    """ImuCamPose(Rwc, twc, pKF) on the inverse of the corrected Sim3, with the KeyFrame's Tcb (row[24:36])"""
    Swc = AE.s3_inv(Scw)
    Rwc, twc = q_to_rot(Swc), Swc[4:7]
    Rcb, tcb = [[float(row[24 + 3 * r + c]) for c in range(3)] for r in range(3)], [float(v) for v in row[33:36]]
    twb = [(Rwc[r][0] * tcb[0] + Rwc[r][1] * tcb[1] + Rwc[r][2] * tcb[2]) + twc[r] for r in range(3)]
    Rwb = [[Rwc[r][0] * Rcb[0][c] + Rwc[r][1] * Rcb[1][c] + Rwc[r][2] * Rcb[2][c] for c in range(3)] for r in range(3)]
    Rcw = [[Rwc[c][r] for c in range(3)] for r in range(3)]
    tcw = [-(Rcw[r][0] * twc[0] + Rcw[r][1] * twc[1] + Rcw[r][2] * twc[2]) for r in range(3)]
    return np.array(sum(Rwb, []) + twb + sum(Rcw, []) + tcw + sum(Rcb, []) + tcb)


# ------------------------------------------------------------------------------------ the mock map
def make_world(seed=7):
    """The 15 KeyFrame objects of tests/test_adapter_essgraph.py's world (0 the first KeyFrame, 5 bad but still in
    the map's list, 14 erased from the map but still KeyFrame 8's mPrevKF, 11..13 corrected with a scale that is
    not 1, 13 the current KeyFrame, 1 the loop KeyFrame, sparse ids) with what the inertial overload reads: the
    mPrevKF / mNextKF chain, a body-camera extrinsic and the KeyFrame's own ImuCamPose fields."""
    a = dict(AE.make_world(seed=seed, fix_scale=False))
    n = len(a["kf.id"])
    rng = np.random.default_rng(seed + 1)
    pose = a["kf.pose"].reshape(-1, 7).astype(np.float32).astype(np.float64)      # Tcw.cast<double>()
    a["kf.pose"] = pose.reshape(-1)
    Rcb = op.rodrigues(np.array([1.2, -1.19, 1.21]) + 0.01 * rng.normal(size=3))
    tcb = np.array([0.065, -0.021, 0.009])
    a["kf.imu_row"] = np.array([op.imu_cam_pose_keyframe(op.quat_to_rot(p[:4]), p[4:7], Rcb, tcb) for p in pose]).reshape(-1)
    prev = np.array([-1] + list(range(n - 1)), np.int32)
    nxt = np.array(list(range(1, n)) + [-1], np.int32)
    prev[6], prev[8], prev[GONE], nxt[13], nxt[GONE] = 4, GONE, -1, -1, -1      # 8's mPrevKF has no vertex: dropped
    a["kf.prev"], a["kf.next"] = prev, nxt
    del a["kf.imu"]
    a["loop_edges"] = np.array([[9, 2], [2, 9], [13, 10], [10, 13]], np.int32).reshape(-1)   # smaller id kept, larger skipped
    a["covis"] = np.array([
        [13, 12, 300], [13, 10, 150], [13, 9, 120], [13, 0, 120], [13, 2, 50], [13, 1, 30],   # mPrevKF | loop edge | kept | inserted | < 100 x 2
        [12, 13, 300], [12, 1, 110], [12, 2, 10],                                             # mNextKF | inserted | < 100
        [4, 6, 200], [4, 2, 101],                                                             # child | kept
        [8, 3, 130], [3, 8, 130],                                                             # kept | larger id
        [7, 5, 140], [7, 3, 60],                                                              # bad | < 100
        [11, 9, 105],                                                                         # kept
    ], np.int32).reshape(-1)
    a["params"] = np.array([CUR, LOOP, 31], np.int32)
    for k in ("mp.corr_by", "mp.corr_ref"):
        del a[k]
    return a


def restate_gather(a):
    """ref:src/Optimizer.cc:4903-5143 on the mock map, literally; edges to a KeyFrame without a vertex are dropped
    and counted.  Returns the problem, the vertex ids, index_of_id, vScw per vertex, the drop count and a log of
    the branches taken."""
    ids = a["kf.id"]
    n = len(ids)
    cur, loop, max_id = [int(v) for v in a["params"]]
    pose = a["kf.pose"].reshape(-1, 7)
    rows = a["kf.imu_row"].reshape(-1, 36)
    corrected = {int(k): [float(v) for v in a["corr.sim3"].reshape(-1, 8)[e]] for e, k in enumerate(a["corr.kf"])}
    noncorr = {int(k): [float(v) for v in a["noncorr.sim3"].reshape(-1, 8)[e]] for e, k in enumerate(a["noncorr.kf"])}
    covis = {i: [] for i in range(n)}
    for x, y, w in a["covis"].reshape(-1, 3):
        covis[int(x)].append((int(y), int(w)))
    loop_edges = {i: sorted(int(y) for x, y in a["loop_edges"].reshape(-1, 2) if x == i) for i in range(n)}
    conn = {}
    for x, y in a["conn"].reshape(-1, 2):
        conn.setdefault(int(x), set()).add(int(y))
    children = {i: {j for j in range(n) if a["kf.parent"][j] == i} for i in range(n)}
    vpKFs = [i for i in range(n) if a["kf.in_map"][i]]
    weight = lambda i, j: dict(covis[i]).get(j, 0)  # noqa: E731
    log = set()

    vScw = {int(i): list(AE.IDENTITY) for i in range(max_id + 1)}
    index_of_id = -np.ones(max_id + 1, np.int32)
    vertex, vrow, fixed = [], [], []
    for i in vpKFs:
        if a["kf.bad"][i]:
            log.add("bad KeyFrame in vpKFs")
            continue
        if i in corrected:
            vScw[int(ids[i])] = corrected[i]
            vrow.append(corrected_row(corrected[i], rows[i]))
            log.add("vertex as corrected")
        else:
            vScw[int(ids[i])] = [float(v) for v in pose[i]] + [1.0]
            vrow.append(rows[i].copy())
            log.add("vertex from the KeyFrame")
        index_of_id[ids[i]] = len(vertex)
        vertex.append(i)
        fixed.append(int(i == loop))
    v0, v1, meas, dropped, inserted = [], [], [], [0], set()

    def add_edge(i, j, Sij):
        x, y = index_of_id[ids[i]], index_of_id[ids[j]]
        if x < 0 or y < 0:
            dropped[0] += 1
            log.add("edge to a KeyFrame without a vertex")
            return
        v0.append(x)
        v1.append(y)
        meas.append(sum(q_to_rot(Sij), []) + Sij[4:7])     # the scale is dropped

    def non_corrected(k, who):
        if k in noncorr:
            log.add("NonCorrectedSim3 hit: " + who)
            return noncorr[k]
        log.add("NonCorrectedSim3 miss: " + who)
        return vScw[int(ids[k])]

    for i in sorted(conn):
        Siw = vScw[int(ids[i])]
        for j in sorted(conn[i]):
            if (i != cur or j != loop) and weight(i, j) < MIN_FEAT:
                log.add("LoopConnections entry dropped by weight")
                continue
            if i == cur and j == loop and weight(i, j) < MIN_FEAT:
                log.add("(current, loop) kept despite its weight")
            add_edge(i, j, AE.s3_mul(Siw, AE.s3_inv(vScw[int(ids[j])])))
            inserted.add((min(ids[i], ids[j]), max(ids[i], ids[j])))
    for i in vpKFs:
        Siw = non_corrected(i, "KeyFrame")
        prev, nxt = int(a["kf.prev"][i]), int(a["kf.next"][i])
        if prev >= 0:
            add_edge(i, prev, AE.s3_mul(Siw, AE.s3_inv(non_corrected(prev, "mPrevKF"))))
        for l in loop_edges[i]:
            if ids[l] < ids[i]:
                add_edge(i, l, AE.s3_mul(Siw, AE.s3_inv(non_corrected(l, "loop edge"))))
            else:
                log.add("loop edge to a larger id skipped")
        for k, w in covis[i]:
            if w < MIN_FEAT:
                continue
            if k == prev:
                log.add("covisible skipped as mPrevKF")
                continue
            if k == nxt:
                log.add("covisible skipped as mNextKF")
                continue
            if k in children[i]:
                log.add("covisible skipped as child")
                continue
            if k in loop_edges[i]:
                log.add("covisible skipped as loop edge")
                continue
            if a["kf.bad"][k]:
                log.add("covisible skipped as bad")
                continue
            if not ids[k] < ids[i]:
                log.add("covisible skipped as larger id")
                continue
            if (min(ids[i], ids[k]), max(ids[i], ids[k])) in inserted:
                log.add("covisible skipped as already inserted")
                continue
            log.add("covisible kept")
            add_edge(i, k, AE.s3_mul(Siw, AE.s3_inv(non_corrected(k, "covisible"))))
    matLambda = [1.0] * 6
    matLambda[0] = 1e3
    matLambda[1] = 1e3
    matLambda[0] = 1e3
    P = op.EssentialGraph4DoFProblem(np.array(vrow), np.array(fixed, np.uint8), np.array(v0, np.int32), np.array(v1, np.int32),
                                     np.array(meas).reshape(-1, 12), info_diag=tuple(matLambda))
    before = np.array([vScw[int(ids[i])] for i in vertex])
    return P, ids[vertex], index_of_id, before, dropped[0], log


def restate_points(a, index_of_id):
    """:5173-5183: the non-bad MapPoints and the vertex of each one's reference KeyFrame"""
    ids = a["kf.id"]
    which = [j for j in range(len(a["mp.bad"])) if not a["mp.bad"][j]]
    return np.array(which, np.int32), np.array([index_of_id[ids[a["mp.ref"][j]]] for j in which], np.int32)


EVERY_BRANCH = {
    "bad KeyFrame in vpKFs", "vertex as corrected", "vertex from the KeyFrame", "edge to a KeyFrame without a vertex",
    "LoopConnections entry dropped by weight", "(current, loop) kept despite its weight", "loop edge to a larger id skipped",
    "covisible skipped as mPrevKF", "covisible skipped as mNextKF", "covisible skipped as child",
    "covisible skipped as loop edge", "covisible skipped as bad", "covisible skipped as larger id",
    "covisible skipped as already inserted", "covisible kept",
} | {f"NonCorrectedSim3 {h}: {w}" for h in ("hit", "miss") for w in ("KeyFrame", "mPrevKF")} | {
    "NonCorrectedSim3 miss: loop edge", "NonCorrectedSim3 miss: covisible"}


# ------------------------------------------------------------------------------------ CPU: the gather
def test_essgraph4dof_driver_compiles(driver):
    assert os.path.exists(driver)


def test_adapter_gather_essential_graph_4dof(driver, tmp_path):
    a = make_world()
    P, vertex_id, index_of_id, before, dropped, log = restate_gather(a)
    assert log >= EVERY_BRANCH, EVERY_BRANCH - log
    out = run(driver, tmp_path, "gather", a)
    np.testing.assert_array_equal(out["vertex_id"], vertex_id)
    np.testing.assert_array_equal(out["index_of_id"], index_of_id)
    assert len(index_of_id) == 32 and len(vertex_id) == 13 and a["kf.id"][BAD] not in vertex_id and a["kf.id"][GONE] not in vertex_id
    np.testing.assert_array_equal(out["fixed"], P.fixed)
    assert P.fixed.sum() == 1 and P.fixed[index_of_id[a["kf.id"][LOOP]]] == 1      # the loop KeyFrame, not the first one
    np.testing.assert_array_equal(out["pose"].reshape(-1, 36), P.pose)
    np.testing.assert_array_equal(out["sim3_before"].reshape(-1, 8), before)
    np.testing.assert_array_equal(out["e_v0"], P.e_v0)
    np.testing.assert_array_equal(out["e_v1"], P.e_v1)
    np.testing.assert_array_equal(out["e_meas"].reshape(-1, 12), P.e_meas)
    assert list(out["scalars"]) == [13, P.n_edges, 0, dropped] and dropped >= 2
    # matLambda as the reference leaves it ((2, 2) stays 1) and g2o's own lambda
    assert list(out["info_lambda"]) == [1e3, 1e3, 1.0, 1.0, 1.0, 1.0, 0.0]
    # the LoopConnections come first, the (current, loop) pair among them; vertex(0) is the map's key
    cur_v, loop_v = index_of_id[a["kf.id"][CUR]], index_of_id[a["kf.id"][LOOP]]
    assert (P.e_v0[2], P.e_v1[2]) == (cur_v, loop_v) and P.n_edges == 20
    # both constructors: a corrected vertex is built in double from a Sim3 whose scale is not 1 (its translation
    # keeps that scale's effect, the measurement drops the scale itself), the others are the KeyFrame's floats
    assert np.all(before[:10, 7] == 1.0) and np.all(before[10:, 7] != 1.0)
    assert np.array_equal(P.pose[:10], P.pose[:10].astype(np.float32).astype(np.float64))
    assert not np.array_equal(P.pose[10:, :24], P.pose[10:, :24].astype(np.float32).astype(np.float64))
    Rcb = P.pose[0, 24:33].reshape(3, 3)
    assert np.abs(Rcb - np.eye(3)).max() > 0.5 and np.all(P.pose[:, 24:] == P.pose[0, 24:])
    dR = P.e_meas[:, :9].reshape(-1, 3, 3)
    assert np.abs(dR @ np.swapaxes(dR, 1, 2) - np.eye(3)).max() < 1e-6      # rotations: no scale left in them
    which, ref = restate_points(a, index_of_id)
    np.testing.assert_array_equal(out["point_index"], which)
    np.testing.assert_array_equal(out["point_ref"], ref)
    np.testing.assert_array_equal(out["point_xw"].reshape(-1, 3), a["mp.pos"].reshape(-1, 3)[which])
    assert ref[0] == -1 and 0 in which and len(which) < len(a["mp.bad"])


# ------------------------------------------------------------------------------------ GPU: the whole call
@pytest.mark.gpu
def test_adapter_optimize_essential_graph_4dof(driver, tmp_path, ctx):
    a = make_world()
    P, vertex_id, index_of_id, before, _, _ = restate_gather(a)
    ref = R.optimize(P)
    rng = np.random.default_rng(99)
    V = R.Variant
    variants = [V(), V(), V(), V(), V(trig=1), V(trig=-1), V(reverse_sums=True), V(polar=True), V(other_solver=True),
                V(trig=1, reverse_sums=True), V(trig=-1, polar=True), V(polar=True, other_solver=True),
                V(reverse_sums=True, other_solver=True), V(trig=1, polar=True, reverse_sums=True, other_solver=True),
                V(trig=-1, polar=True, reverse_sums=True, other_solver=True), V(trig=1, other_solver=True)]
    assert len(variants) == FX.N_REPLICAS
    spread = R.spreads(ref, [R.optimize(R.nudged(P, rng), v) for v in variants], P)
    tol = {q: max(10.0 * spread[q], 1e-6) for q in ("rot_rad", "t_rel")}
    out = run(driver, tmp_path, "optimize", a)
    assert list(out["ret"]) == [0, 1, 1]   # no error, the change index incremented once, under the map's lock
    vidx = np.array([int(np.nonzero(a["kf.id"] == v)[0][0]) for v in vertex_id])
    n_set = out["kf.n_set_pose"]
    assert np.all(n_set[vidx] == 1) and n_set.sum() == len(vidx)   # not the bad KeyFrame, not the erased one
    # the same graph through the C ABI directly: the poses are its Rcw, tcw after the quaternion and the float casts
    direct = op.Optimizer(ctx).optimize_essential_graph_4dof(P)
    q_set, t_set = out["kf.set_q"].reshape(-1, 4)[vidx], out["kf.set_t"].reshape(-1, 3)[vidx]
    q_direct = np.array([rot_to_quat(Rm) for Rm in direct.R])
    want_q = np.array([[np.float32(v / math.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])) for v in q] for q in q_direct])
    np.testing.assert_array_equal(q_set, want_q)
    np.testing.assert_array_equal(t_set, direct.t.astype(np.float32))
    # against the literal flow driven by pyref: SetPose(SE3d(Quaterniond(Rcw), tcw).cast<float>())
    t_ref = ref.t.astype(np.float32)
    tmax = float(np.abs(t_ref).max())
    eps = float(np.finfo(np.float32).eps)
    Rset = np.array([op.quat_to_rot(q.astype(np.float64) / np.linalg.norm(q.astype(np.float64))) for q in q_set])
    rot = float(R.rot_angle(Rset, ref.R).max())
    dt = float(np.max(np.linalg.norm(t_set.astype(np.float64) - t_ref.astype(np.float64), axis=1))) / tmax
    print("adapter poses against pyref: rotation", rot, "translation", dt, "tolerances", tol, "gpu iterations",
          direct.lm_iterations, direct.lm_trials, "pyref", ref.lm_iterations, ref.lm_trials)
    assert rot <= tol["rot_rad"] + 4 * eps and dt <= tol["t_rel"] + 4 * eps
    assert direct.chi2_final < direct.chi2_initial
    # the MapPoints: the correction through vScw and the optimised poses as unit-scale Sim3s, 1 float ulp
    which, pref = restate_points(a, index_of_id)
    X = a["mp.pos"].reshape(-1, 3)
    after = np.concatenate([q_direct, direct.t, np.ones((P.n, 1))], 1)
    want = X.copy()
    want[which] = EG.correct_points(X[which], pref, before, after)
    got = out["mp.pos"].reshape(-1, 3)
    ulp = np.spacing(np.abs(want).astype(np.float32))
    print("MapPoint coordinates that differ from pyref's float:", int(np.count_nonzero(got != want)), "of", got.size)
    assert np.all(np.abs(got.astype(np.float64) - want.astype(np.float64)) <= ulp)
    skipped = np.setdiff1d(np.arange(len(X)), which)
    np.testing.assert_array_equal(got[skipped], X[skipped])          # bad MapPoints are not touched
    np.testing.assert_array_equal(got[which[pref < 0]], X[which[pref < 0]])
    assert np.abs(got[which[pref >= 0]] - X[which[pref >= 0]]).max() > 1e-3
    n_update = out["mp.n_update"]
    assert np.all(n_update[which] == 1) and n_update.sum() == len(which)   # once per non-bad point
    np.testing.assert_array_equal(out["mp.n_set_pos"], n_update)
