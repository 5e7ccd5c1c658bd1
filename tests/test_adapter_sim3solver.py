"""Sim3Solver through the ORB-SLAM3-side adapter (adapters/orbslam3/osg_orbslam3.h: Sim3SolverGather,
Sim3Solver) on the mock KeyFrames / MapPoints of tests/adapter/mock_orbslam3.h, driven by
tests/adapter/sim3solver_driver.cpp.

* CPU: the constructor's gather on a KeyFrame window that takes every branch of the reference's slot filter
  equals a Python restatement of ref:src/Sim3Solver.cc:38-118 exactly: order, mvnIndices1, the points and the
  truncated bounds.  The reference raises bDifferentKFs when vpKeyFrameMatchedMP is EMPTY, so a caller's
  vector is never read and the KeyFrame of match 2 is pKF2 in either case; the restatement and the adapter
  keep that, and the test passes the vector both ways.
* GPU: LoopClosing's ``while (!bConverge && !bNoMore) iterate(20, ...)`` through the adapter with a scripted
  RandomInt gives the outputs of tests/pyref_sim3solver.py's sequential solver on one converging and one
  non-converging world, call by call.
"""
import os
import subprocess

import numpy as np
import pytest

from orb_slam3_comments_ghr_amd import optimizer as op
from orb_slam3_comments_ghr_amd import sim3solver as S3
from tests import pyref_sim3opt as RO
from tests import pyref_sim3solver as R
from tests import sim3solver_fixtures as FX
from tools.adapter_arrays import read_arrays, write_arrays

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER_SRC = os.path.join(ROOT, "tests", "adapter", "sim3solver_driver.cpp")
PKG = os.path.join(ROOT, "orb_slam3_comments_ghr_amd")
SIG2 = S3.level_sigma2()
BOUNDS = S3.max_errors(SIG2)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sim3solver") / "sim3solver_driver")
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
    Rf = RO.quat_to_rot(pose[:4]).astype(np.float32)
    Xf = np.asarray(X, np.float64).astype(np.float32)
    tf = np.asarray(pose[4:], np.float64).astype(np.float32)
    out = np.zeros(3, np.float32)
    for r in range(3):
        v = Rf[r, 0] * Xf[0]
        v = v + Rf[r, 1] * Xf[1]
        v = v + Rf[r, 2] * Xf[2]
        out[r] = v + tf[r]
    return out


def make_world(seed, n, outlier_frac, min_inliers, fix_scale=False, pass_kfm=True, cam2=None):
    """A KeyFrame window around a synthetic problem: match i becomes slot i of KeyFrame 1, whose MapPoint is
    observed in KeyFrame 1 at a shuffled keypoint index (the bound comes from that keypoint, not from the
    slot), and a matched MapPoint observed in KeyFrame 2 at another shuffled index.  Slots 0 .. 7 are then
    rewired so that every branch of the constructor's filter is taken."""
    rng = np.random.default_rng(seed)
    P = S3.synth_sim3_ransac_problem(rng, n, outlier_frac, fix_scale, cam2=cam2, min_inliers=min_inliers, n_hyp=1)
    poses = [np.concatenate([op.rot_to_quat(op.small_rotation(rng, 20.0)), rng.normal(0, 1.0, 3)]) for _ in range(3)]
    R1, R2 = RO.quat_to_rot(poses[0][:4]), RO.quat_to_rot(poses[1][:4])
    pos = np.concatenate([(P.p1c.astype(np.float64) - poses[0][4:]) @ R1, (P.p2c.astype(np.float64) - poses[1][4:]) @ R2])
    bad = np.zeros(2 * n, np.uint8)
    perm1, perm2 = rng.permutation(n).astype(np.int32), rng.permutation(n).astype(np.int32)
    none = -np.ones(n, np.int32)
    kfidx = [np.concatenate([perm1, none]), np.concatenate([none, perm2]), -np.ones(2 * n, np.int32)]
    lev1 = np.array([int(np.nonzero(BOUNDS == b)[0][0]) for b in P.max_err1], np.int32)
    lev2 = np.array([int(np.nonzero(BOUNDS == b)[0][0]) for b in P.max_err2], np.int32)
    oct1, oct2 = np.zeros(n, np.int32), np.zeros(n, np.int32)
    oct1[perm1] = lev1
    oct2[perm2] = lev2
    oct3 = np.array([(lev2[6] + 1) % 8, 6], np.int32)  # KeyFrame 3 sees match 6 at another level than pKF2
    mp1 = np.arange(n, dtype=np.int32)
    match = np.arange(n, 2 * n, dtype=np.int32)
    kfm = np.full(n, 2, np.int32)
    match[0] = -1                        # null match
    mp1[1] = -1                          # no MapPoint in KeyFrame 1
    bad[mp1[2]] = 1                      # KeyFrame 1's MapPoint bad
    bad[match[3]] = 1                    # the matched MapPoint bad
    kfidx[0][mp1[4]] = -1                # GetIndexInKeyFrame(pKF1) < 0
    kfidx[1][match[5]] = -1              # GetIndexInKeyFrame(pKFm) < 0
    kfm[6] = 3                           # a match of another KeyFrame of the window, also observed in pKF2:
    kfidx[2][match[6]] = 0               # the reference reads pKF2's keypoint (level lev2[6]), not KeyFrame 3's
    kfm[7] = 3                           # ... observed in that KeyFrame only: index in pKF2 < 0, skipped
    kfidx[2][match[7]] = 1
    kfidx[1][match[7]] = -1
    cams = [np.array([c.type] + [c.p[i] for i in range(8)], np.float32) for c in (P.cam1, P.cam2, P.cam2)]
    a = {"sig2": SIG2, "mp.pos": pos.reshape(-1), "mp.bad": bad, "slot.mp1": mp1, "slot.match": match, "slot.kfm": kfm,
         "params": np.array([int(fix_scale), int(pass_kfm), min_inliers, 300, 20], np.int32),
         "rand": np.zeros(0, np.int32)}
    for k in range(3):
        a[f"kf{k + 1}.pose"] = poses[k]
        a[f"kf{k + 1}.cam"] = cams[k]
        a[f"kf{k + 1}.oct"] = (oct1, oct2, oct3)[k]
        a[f"mp.kf{k + 1}idx"] = kfidx[k].astype(np.int32)
    return P, a


def restate_gather(a):
    """ref:src/Sim3Solver.cc:38-118 on the mock world, literally (bDifferentKFs as the reference sets it)."""
    pos = a["mp.pos"].reshape(-1, 3)
    S = len(a["slot.match"])
    kf_matched = [int(k) for k in a["slot.kfm"]] if a["params"][1] else []
    bDifferentKFs = False
    if not kf_matched:
        bDifferentKFs = True
        kf_matched = [2] * S
    octs = {k: a[f"kf{k}.oct"] for k in (1, 2, 3)}
    idx_in = {k: a[f"mp.kf{k}idx"] for k in (1, 2, 3)}
    p1c, p2c, m1, m2, index = [], [], [], [], []
    kfm = 2
    for i1 in range(S):
        if a["slot.match"][i1] < 0:
            continue
        mp1, mp2 = int(a["slot.mp1"][i1]), int(a["slot.match"][i1])
        if mp1 < 0:
            continue
        if a["mp.bad"][mp1] or a["mp.bad"][mp2]:
            continue
        if bDifferentKFs:
            kfm = kf_matched[i1]
        i1k, i2k = int(idx_in[1][mp1]), int(idx_in[kfm][mp2])
        if i1k < 0 or i2k < 0:
            continue
        s1, s2 = SIG2[octs[1][i1k]], SIG2[octs[kfm][i2k]]
        m1.append(np.float32(int(9.210 * float(s1))))   # vector<size_t>::push_back(double)
        m2.append(np.float32(int(9.210 * float(s2))))
        index.append(i1)
        p1c.append(cam_point(a["kf1.pose"], pos[mp1]))
        p2c.append(cam_point(a["kf2.pose"], pos[mp2]))
    return (np.array(p1c, np.float32).reshape(-1, 3), np.array(p2c, np.float32).reshape(-1, 3), np.array(m1, np.float32),
            np.array(m2, np.float32), np.array(index, np.int32))


# ------------------------------------------------------------------------------------ CPU: the gather
@pytest.mark.parametrize("pass_kfm", [False, True])
def test_adapter_gather_sim3solver(driver, tmp_path, pass_kfm):
    P, a = make_world(5100, 30, 0.1, 12, pass_kfm=pass_kfm, cam2=op.pinhole_camera(380.0, 395.0, 330.0, 250.0))
    out = run(driver, tmp_path, "gather", a)
    p1c, p2c, m1, m2, index = restate_gather(a)
    # slots 0 - 5 and 7 are filtered; slot 6 is kept with pKF2's keypoint whatever vpKeyFrameMatchedMP says
    assert not set(index) & {0, 1, 2, 3, 4, 5, 7} and 6 in index and len(index) == 30 - 7
    np.testing.assert_array_equal(out["index"], index)
    np.testing.assert_array_equal(out["p1c"].reshape(-1, 3), p1c)
    np.testing.assert_array_equal(out["p2c"].reshape(-1, 3), p2c)
    np.testing.assert_array_equal(out["max1"], m1)
    np.testing.assert_array_equal(out["max2"], m2)
    # truncated, not rounded and not the double itself: 9.210 * 1.2^10 = 57.03 -> 57, 9.210 * 1.44 = 13.26 -> 13
    assert set(np.unique(np.concatenate([m1, m2]))) <= set(BOUNDS) and len(set(m1)) > 3
    assert all(b == np.floor(b) for b in BOUNDS) and BOUNDS[1] == 13 and BOUNDS[5] == 57
    j = list(index).index(6)
    assert m2[j] == P.max_err2[6] and m2[j] != BOUNDS[a["kf3.oct"][0]]
    # the bound of slot i comes from the keypoint GetIndexInKeyFrame names, not from keypoint i
    assert np.array_equal(m1, P.max_err1[index]) and np.array_equal(m2, P.max_err2[index])
    assert list(out["shape"]) == [30, P.cam1.type, P.cam2.type]
    assert list(out["cams"]) == [np.float32(P.cam1.p[0]), np.float32(P.cam1.p[2]), np.float32(380.0), np.float32(330.0)]


# ------------------------------------------------------------------------------------ GPU: the loop
def reference_loop(Q, E, its, window):
    """ref:src/LoopClosing.cc:993-997 on pyref's sequential solver."""
    S = R.Solver(Q, E, max_its=its)
    trace, mats = [], []
    conv = no_more = False
    while not conv and not no_more:
        T, no_more, vb, nin, conv = S.iterate(window)
        trace.append([int(conv), int(no_more), nin, S.mnIterations, S.mnBestInliers])
        mats.append(T)
    return S, trace, mats, vb, nin, conv, no_more


@pytest.mark.gpu
@pytest.mark.parametrize("seed,n,outlier_frac,min_inliers,converges", [(5206, 100, 0.6, 20, True), (5300, 100, 0.7, 40, False)])
def test_adapter_sim3solver_loop(driver, tmp_path, ctx, seed, n, outlier_frac, min_inliers, converges):
    P, a = make_world(seed, n, outlier_frac, min_inliers)
    p1c, p2c, m1, m2, index = restate_gather(a)
    N = len(index)
    its = R.ransac_iterations(0.99, min_inliers, N, 300)
    rng = np.random.default_rng(seed + 1)
    rand = np.stack([rng.integers(0, N - j, its) for j in range(3)], 1).astype(np.int32)
    a["rand"] = rand.reshape(-1)
    Q = S3.Sim3RansacProblem(p1c, p2c, m1, m2, R.draw_samples_literal(N, its, rand), min_inliers=min_inliers,
                             cam1=P.cam1, cam2=P.cam2)
    E = R.evaluate(Q)
    S, trace, mats, vb, nin, conv, no_more = reference_loop(Q, E, its, 20)
    assert conv == converges and len(trace) >= 2, (conv, trace)
    # the world is away from the bounds where it matters (conditions 1 and 2 of the fixtures' guard)
    g = FX.margins()["groups"]["n100"]["g"]
    bl = FX.borderline(E, g)
    upto = S.best if conv else its
    assert bl[S.best] == 0 and np.all((E.counts + bl)[:upto] <= min_inliers), "pick another seed"
    out = run(driver, tmp_path, "loop", a)
    bConverge, bNoMore, nInliers, calls, max_its, drawn, rand_bad = (int(v) for v in out["flags"])
    assert (bool(bConverge), bool(bNoMore), nInliers, calls) == (conv, no_more, nin, len(trace))
    assert max_its == its and drawn == 3 * its and rand_bad == 0  # every triple is drawn up front
    np.testing.assert_array_equal(out["trace"].reshape(-1, 5), np.array(trace))
    want_vb = np.zeros(len(a["slot.match"]), bool)
    if conv:
        want_vb[index[vb]] = True
    np.testing.assert_array_equal(out["vbInliers"].astype(bool), want_vb)
    # GetEstimated* and the returned matrices: the same hypothesis's values through the C ABI directly
    direct = S3.Sim3Solver(ctx).solve(Q)
    assert direct.hyp == S.best and direct.converged == conv
    s13 = direct.hyp_sim3
    def T12(h):
        T = np.eye(4, dtype=np.float32)
        T[:3, :3] = s13[h, 12] * s13[h, :9].reshape(3, 3)
        T[:3, 3] = s13[h, 9:12]
        return T
    assert out["T12"].tobytes() == T12(S.best).tobytes() == direct.T12.tobytes()
    assert out["R"].tobytes() == s13[S.best, :9].tobytes() and out["t"].tobytes() == s13[S.best, 9:12].tobytes()
    assert out["s"][0] == s13[S.best, 12]
    # call by call: the best so far (the second overload never returns an uninitialised matrix)
    best_after = []
    b, h = 0, -1
    for k, row in enumerate(trace):
        for i in range(0 if k == 0 else trace[k - 1][3], row[3]):
            if E.counts[i] >= b:
                b, h = int(E.counts[i]), i
        best_after.append(h)
    got = out["returned"].reshape(-1, 4, 4)
    for k, h in enumerate(best_after):
        assert got[k].tobytes() == T12(h).tobytes(), k
        assert FX.rot_angle(got[k][:3, :3] / s13[h, 12], E.R[h]) < 1e-4
    # pyref's matrix of the final best within the float tolerances of the n100 fixtures
    m = FX.margins()["groups"]["n100"]
    assert FX.rot_angle(out["R"].reshape(3, 3), E.R[S.best]) <= 10 * m["rot_rad_max"]
    # find() and the first overload on fresh solvers over the same stream
    S2 = R.Solver(Q, E, max_its=its)
    T, _, _, nin2, conv2 = S2.find()
    assert list(out["find_flags"]) == [nin2, S2.mnIterations, S2.mnBestInliers]
    assert out["find"].tobytes() == (T12(S2.best) if conv2 else np.eye(4, dtype=np.float32)).tobytes()
    S3_ = R.Solver(Q, E, max_its=its)
    T, nm3, _, nin3, conv3 = S3_.iterate(20, second_overload=False)
    assert list(out["iter1_flags"]) == [int(nm3), nin3, S3_.mnIterations]
    assert out["iter1"].tobytes() == (T12(S3_.best) if conv3 else np.eye(4, dtype=np.float32)).tobytes()
