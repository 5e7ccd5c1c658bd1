"""PoseInertialOptimizationLastKeyFrame / LastFrame through the ORB-SLAM3-side adapter (adapters/orbslam3/osg_orbslam3.h)
on the mock objects of tests/adapter/mock_inertial.h, driven by tests/adapter/poseinertial_driver.cpp.

  * CPU: the gather against a Python restatement of the slot rule of ref:src/Optimizer.cc:508-637 on frames that take
    all three branches (left or only mono, stereo, right mono), a rig and a non-rig frame, with empty slots; the
    vertices, the cameras of ImuCamPose(Frame*), both covariances and the prior hand-over.
  * GPU: the round trip: return value, mvbOutlier per slot, SetImuPoseVelocity's float casts, mImuBias' order, the
    new mpcpi (ConstraintPoseImu's constructor on the returned H) and, in LastFrame, the previous frame's mpcpi
    deleted and nulled; LastFrame without a prior returns 0 and leaves the frame untouched.
"""
import copy
import os
import subprocess

import numpy as np
import pytest

from orb_slam3_comments_ghr_amd import _abi
from orb_slam3_comments_ghr_amd import optimizer as O
from tools.adapter_arrays import read_arrays, write_arrays

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "orb_slam3_comments_ghr_amd")
DRIVER_SRC = os.path.join(ROOT, "tests", "adapter", "poseinertial_driver.cpp")
LKF, LF = _abi.OSG_PIO_LAST_KEYFRAME, _abi.OSG_PIO_LAST_FRAME
MONO, STEREO, BODY = _abi.EDGE_MONO, _abi.EDGE_STEREO, _abi.EDGE_BODY


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("poseinertial") / "poseinertial_driver")
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


def preint_row(q):
    return np.concatenate([a.ravel() for a in (q.dR, q.dV, q.dP, q.JRg, q.JVg, q.JVa, q.JPg, q.JPa, q.b)] +
                          [np.array([q.dT], np.float32), q.C.ravel()]).astype(np.float32)


def mock_frame(P, rng, has_prior=True):
    """The Frame the problem P would have been gathered from: P's edges in slot order with empty slots between
    them; a rig frame holds its left keypoints in mvKeys [0, Nleft) and its right ones in mvKeysRight, a non-rig
    frame everything in mvKeysUn.  The arrays a branch must not read hold poison."""
    rig = len(P.cams) == 2
    n = P.n
    if rig:  # slot order: left slots first
        order = np.argsort(P.kind != MONO, kind="stable")
        P.kind, P.xw, P.obs = P.kind[order], P.xw[order], P.obs[order]
        P.inv_sigma2, P.track_depth = P.inv_sigma2[order], P.track_depth[order]
    octave = np.array([int(np.argmin(np.abs(O.inv_level_sigma2() - w))) for w in P.inv_sigma2], np.int32)
    # slots: every edge, and an empty slot after every third
    slots, mp = [], []
    for e in range(n):
        slots.append(e)
        if e % 3 == 2:
            slots.append(-1)
    N = len(slots)
    slot_mp = np.array(slots, np.int32)
    edge_slot = np.array([i for i, s in enumerate(slots) if s >= 0], np.int32)
    poison = np.array([-777.0, -777.0, 0.0], np.float32)
    keys = np.tile(poison, (N, 1))
    keys_un = np.tile(poison, (N, 1))
    uright = np.full(N, -1.0, np.float32)
    Nleft = -1
    keys_right = np.zeros((0, 3), np.float32)
    if rig:
        n_left_edges = int((P.kind == MONO).sum())
        Nleft = int(edge_slot[n_left_edges]) if n_left_edges < n else N
        keys_right = np.tile(poison, (N - Nleft, 1))
        for e, i in enumerate(edge_slot):
            row = [P.obs[e, 0], P.obs[e, 1], octave[e]]
            if i < Nleft:
                keys[i] = row
            else:
                keys_right[i - Nleft] = row
    else:
        for e, i in enumerate(edge_slot):
            keys_un[i] = [P.obs[e, 0], P.obs[e, 1], octave[e]]
            if P.kind[e] == STEREO:
                uright[i] = P.obs[e, 2]
    c0 = P.cams[0]
    Rrl, trl = np.eye(3), np.zeros(3)
    if rig:
        q = np.array(O.TUMVI_TRL[:4]) / np.linalg.norm(O.TUMVI_TRL[:4])
        Rrl, trl = O._f32(O.quat_to_rot(q)), O._f32(O.TUMVI_TRL[4:])
    extr = np.concatenate([np.ravel(a) for a in (c0.Rcw, c0.tcw, c0.Rcb, c0.tcb, c0.tbc, Rrl, trl)]).astype(np.float32)

    def body(S, pre, d):
        d[pre + "Rwb"], d[pre + "twb"], d[pre + "v"] = (np.asarray(a, np.float32).ravel() for a in (S.Rwb, S.twb, S.v))
        d[pre + "bias"] = np.concatenate([S.ba, S.bg]).astype(np.float32)

    other = copy.copy(P.preint)  # the other preintegration: distinct dT and covariance, so a mix-up shows
    other.dT = np.float32(9.0)
    other.C = (P.preint.C * 3).astype(np.float32)
    kf_pre, fr_pre = (other, P.preint) if P.mode == LF else (P.preint, other)
    kf_pre = copy.copy(kf_pre)
    kf_pre.C = P.C_rw  # mpImuPreintegrated->C feeds the random-walk informations in both modes
    if P.mode == LKF:
        kf_pre.C = P.preint.C
        P.C_rw = P.preint.C.copy()
    cam = c0.cam
    d = {
        "params": np.array([P.mode == LF, P.rec_init, N, Nleft, rig, has_prior and P.prior is not None], np.int32),
        "keys": keys.astype(np.float32).ravel(), "keys_un": keys_un.astype(np.float32).ravel(),
        "keys_right": keys_right.astype(np.float32).ravel(), "uright": uright,
        "isig": O.inv_level_sigma2(), "cam": np.array([cam.type, *cam.p[:], P.bf], np.float32), "extr": extr,
        "preint_kf": preint_row(kf_pre), "preint_frame": preint_row(fr_pre),
        "slot.mp": slot_mp, "mp.pos": P.xw.ravel(), "mp.depth": P.track_depth,
    }
    body(P.cur, "cur.", d)
    body(P.prev, "prev.", d)
    if P.prior is not None:
        pr = P.prior
        d["prior"] = np.concatenate([np.ravel(a) for a in (pr.Rwb, pr.twb, pr.vwb, pr.bg, pr.ba, pr.H)]).astype(np.float64)
    return d, edge_slot, N, Nleft


def slot_rule(N, Nleft, has_mp, uright):
    """ref:src/Optimizer.cc:508-637, the branches as written: (slot, kind, key array) per edge."""
    out = []
    bRight = Nleft != -1
    for i in range(N):
        if not has_mp[i]:
            continue
        if (not bRight and uright[i] < 0) or i < Nleft:
            out.append((i, MONO, "keys" if i < Nleft else "keys_un"))
        elif not bRight:
            out.append((i, STEREO, "keys_un"))
        if bRight and i >= Nleft:
            out.append((i, BODY, "keys_right"))
    return out


CASES = [(LKF, "pinhole_stereo", 40, 1), (LF, "pinhole_stereo", 40, 2), (LKF, "kb8_rig", 40, 3), (LF, "kb8_rig", 40, 4),
         (LKF, "pinhole_mono", 7, 5)]


@pytest.mark.parametrize("mode,cam,n,seed", CASES)
def test_gather_follows_the_slot_rule(driver, tmp_path, mode, cam, n, seed):
    P = O.synth_pose_inertial_problem(np.random.default_rng(seed), n, mode, cam, rec_init=bool(seed & 1))
    d, edge_slot, N, Nleft = mock_frame(P, np.random.default_rng(seed))
    out = run(driver, tmp_path, "gather", d)
    rule = slot_rule(N, Nleft, d["slot.mp"] >= 0, d["uright"])
    assert [r[0] for r in rule] == list(out["slot"]) == list(edge_slot)
    assert [r[1] for r in rule] == list(out["kind"].astype(np.int8)) == list(P.kind)
    if cam == "pinhole_stereo":
        assert {MONO, STEREO} <= set(P.kind.tolist())
    if cam == "kb8_rig":
        assert {MONO, BODY} <= set(P.kind.tolist())
    obs = out["obs"].reshape(-1, 3)
    for e, (i, k, arr) in enumerate(rule):
        src = d[arr].reshape(-1, 3)[i - Nleft if arr == "keys_right" else i]
        assert obs[e, 0] == src[0] and obs[e, 1] == src[1]
        assert obs[e, 2] == (d["uright"][i] if k == STEREO else 0.0)
        assert out["isig"][e] == d["isig"][int(src[2])]
    np.testing.assert_array_equal(obs, P.obs)
    np.testing.assert_array_equal(out["xw"].reshape(-1, 3), P.xw)
    np.testing.assert_array_equal(out["depth"], P.track_depth)
    # mvbOutlier: cleared on the gathered slots only
    np.testing.assert_array_equal(out["outlier"] != 0, d["slot.mp"] < 0)
    head = out["head"]
    assert list(head[:4]) == [mode, int(P.rec_init), len(P.cams), P.n] and head[4] == (mode == LF) and head[5] == 0
    st = out["states"].reshape(2, 21)
    for row, S in zip(st, (P.cur, P.prev)):
        np.testing.assert_array_equal(row, np.concatenate([S.Rwb.ravel(), S.twb, S.v, S.bg, S.ba]))
    cams = out["cams"]
    assert cams[-1] == P.bf
    for c, k in enumerate(P.cams):  # ImuCamPose(Frame*), the second camera through Trl
        want = np.concatenate([np.ravel(a) for a in (k.Rcw, k.tcw, k.Rcb, k.tcb, k.tbc)])
        np.testing.assert_allclose(cams[27 * c:27 * c + 27], want, rtol=0, atol=1e-15 if c == 0 else 1e-12)
    # the edge's preintegration is the KeyFrame's or the frame's by mode; the random-walk covariance is always
    # mpImuPreintegrated's
    t = out["preint_dT_b"]
    assert t[0] == P.preint.dT and t[1] == np.float32(P.prev.ba[0]) and t[2] == np.float32(P.prev.bg[2])
    assert t[3] == P.preint.C[0, 0] and t[4] == P.C_rw[0, 0] and t[5] == P.C_rw[14, 14]


def test_last_frame_without_mpcpi_is_refused_by_the_check(driver, tmp_path):
    P = O.synth_pose_inertial_problem(np.random.default_rng(9), 20, LF, "pinhole_stereo")
    d, *_ = mock_frame(P, np.random.default_rng(9), has_prior=False)
    out = run(driver, tmp_path, "gather", d)
    assert out["head"][4] == 0 and out["head"][5] == -1


@pytest.mark.gpu
@pytest.mark.parametrize("mode,cam,n,seed", CASES)
def test_round_trip(driver, tmp_path, mode, cam, n, seed):
    from orb_slam3_comments_ghr_amd import Context
    P = O.synth_pose_inertial_problem(np.random.default_rng(seed), n, mode, cam, rec_init=bool(seed & 1))
    d, edge_slot, N, Nleft = mock_frame(P, np.random.default_rng(seed))
    g = run(driver, tmp_path, "gather", d)
    out = run(driver, tmp_path, "optimize", d)
    # the same problem through the Python mirror: the cameras exactly as the adapter derived them
    cams = g["cams"]
    for c, k in enumerate(P.cams):
        blk = cams[27 * c:27 * c + 27]
        k.Rcw, k.tcw, k.Rcb, k.tcb, k.tbc = blk[0:9].reshape(3, 3), blk[9:12], blk[12:21].reshape(3, 3), blk[21:24], blk[24:27]
    ctx = Context(0)
    ref = O.run_pose_inertial(ctx, [P])[0]
    ctx.close()
    ret, has_new, prev_null, had_prior, live = out["ret"]
    assert ret == ref.n_inliers
    flags = np.ones(N, bool)   # ungathered slots keep what they had
    flags[edge_slot] = ref.outlier != 0
    np.testing.assert_array_equal(out["outlier"] != 0, flags)
    s = ref.state
    want = np.concatenate([s.Rwb.ravel(), s.twb, s.v, s.ba, s.bg]).astype(np.float32)  # IMU::Bias(b[3..5], b[0..2])
    np.testing.assert_array_equal(out["state"], want)
    assert has_new == 1
    cpi = out["mpcpi"]
    np.testing.assert_array_equal(cpi[:21], np.concatenate([s.Rwb.ravel(), s.twb, s.v, s.bg, s.ba]))
    Hc = O.constraint_pose_imu(ref.H)
    np.testing.assert_allclose(cpi[21:].reshape(15, 15), Hc, rtol=0, atol=1e-9 * np.abs(Hc).max())
    if mode == LF:
        assert had_prior == 1 and prev_null == 1 and live == 1   # the old prior deleted, the new one alive
    else:
        assert prev_null == 1 and live == 1


@pytest.mark.gpu
def test_last_frame_without_mpcpi_returns_zero_and_touches_nothing(driver, tmp_path):
    P = O.synth_pose_inertial_problem(np.random.default_rng(9), 20, LF, "pinhole_stereo")
    d, edge_slot, N, _ = mock_frame(P, np.random.default_rng(9), has_prior=False)
    out = run(driver, tmp_path, "optimize", d)
    assert list(out["ret"][:3]) == [0, 0, 1] and "mpcpi" not in out
    np.testing.assert_array_equal(out["state"][:9], np.asarray(P.cur.Rwb, np.float32).ravel())
