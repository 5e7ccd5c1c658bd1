"""Tracking::PreintegrateIMU, the reintegration of InertialOptimization's write-back and MergePrevious through the
ORB-SLAM3-side adapter (adapters/orbslam3/osg_orbslam3.h) on the mock objects of tests/adapter/mock_preintegration.h,
driven by tests/adapter/preintegration_driver.cpp.

  * CPU: the queue after the call, mvImuFromLastFrame, the integrables and setIntegrated against the Python
    restatement of ref:src/Tracking.cc:1771-1901, with every early return; which KeyFrames pass the 0.01 gyro-bias
    test of ref:src/Optimizer.cc:3889 and the biases SetNewBias leaves.
  * GPU: the round trips equal the direct calls bit for bit: both hand-overs of PreintegrateIMU (the state
    continued from the last KeyFrame, the fresh one of the frame), the reintegrated set, MergePrevious.
"""
import os
import subprocess

import numpy as np
import pytest

from orb_slam3_comments_ghr_amd import imu
from tests import preintegration_fixtures as FX
from tests import pyref_preintegration as R
from tools.adapter_arrays import read_arrays, write_arrays

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "orb_slam3_comments_ghr_amd")
DRIVER_SRC = os.path.join(ROOT, "tests", "adapter", "preintegration_driver.cpp")
f = np.float32
STATE = ("dR", "dV", "dP", "JRg", "JVg", "JVa", "JPg", "JPa", "b", "dT", "C", "avgA", "avgW")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("preintegration") / "preintegration_driver")
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


def state_row(s):
    """osg_imu_preintegrated as floats, then bu and db = (dbg, dba)"""
    row = [np.asarray(getattr(s, k), f).ravel() for k in STATE[:9]] + [np.array([s.dT], f), s.C.ravel(), s.avgA, s.avgW]
    bu = np.asarray(s.bu, f)
    db = np.concatenate([bu[3:] - s.b[3:], bu[:3] - s.b[:3]])
    return np.concatenate(row + [bu, db]).astype(f)


def pre_arrays(name, s):
    return {name + ".state": state_row(s)[:298], name + ".bu": np.asarray(s.bu, f), name + ".meas": s.meas.ravel()}


def empty_state(bias, nga, walk):
    z3 = np.zeros((3, 3), f)
    return imu.PreintegratedState(np.eye(3, dtype=f), np.zeros(3, f), np.zeros(3, f), z3, z3, z3, z3, z3, bias, 0.0,
                                  np.zeros((15, 15), f), np.zeros(3, f), np.zeros(3, f), nga=nga, nga_walk=walk)


def tracking_arrays(seed, m_queue=16, lead=-0.0112, has_prev=True, from_kf=None):
    rng = np.random.default_rng(seed)
    nga, walk = FX.noise()
    t_prev, t_cur = 200.0, 200.05
    a, w, t = FX.imu_points(rng, m_queue, t0=t_prev + lead) if m_queue else (np.zeros((0, 3), f),) * 2 + (np.zeros(0),)
    last_bias = rng.normal(0, 0.01, 6).astype(f)
    if from_kf is None:
        from_kf = empty_state(rng.normal(0, 0.01, 6).astype(f), nga, walk)
    d = {"noise": np.concatenate([nga, walk]), "frames": np.array([t_prev, t_cur, float(has_prev)]),
         "last_bias": last_bias, "queue.aw": np.concatenate([a, w], 1).astype(f).ravel(), "queue.t": np.asarray(t, float)}
    d.update(pre_arrays("from_kf", from_kf))
    return d, (a, w, t, t_prev, t_cur, last_bias, from_kf, nga, walk)


# ----------------------------------------------------------------------------------- CPU: the host part
@pytest.mark.parametrize("m_queue,lead", [(16, -0.0112), (16, 0.002), (9, -0.0112), (30, -0.05), (3, 0.0301)])
def test_frame_list_matches_the_restatement(driver, tmp_path, m_queue, lead):
    d, (a, w, t, t_prev, t_cur, *_rest) = tracking_arrays(m_queue, m_queue, lead)
    got = run(driver, tmp_path, "list", d)
    taken, popped = R.select(t, t_prev, t_cur)
    assert got["taken.t"].tobytes() == t[taken].tobytes()
    assert got["queue.t"].tobytes() == t[popped:].tobytes()
    want = R.integrables(a[taken], w[taken], t[taken], t_prev, t_cur)
    assert len(taken) >= 2 and got["ret"][0] == len(taken) - 1
    assert got["meas"].tobytes() == want.tobytes()
    assert got["ret"][1] == 0            # setIntegrated() is the hand-over's
    assert got["from_kf.state"].tobytes() == d_state(d) and got["ret"][5] == 1


def d_state(d):
    z = np.zeros(6, f)
    return np.concatenate([d["from_kf.state"], d["from_kf.bu"], z]).astype(f).tobytes()


def test_early_returns_of_preintegrate_imu(driver, tmp_path):
    # no previous frame: integrated, the queue untouched
    d, (a, w, t, *_rest) = tracking_arrays(1, has_prev=False)
    got = run(driver, tmp_path, "list", d)
    assert list(got["ret"][:2]) == [-1, 1] and got["queue.t"].tobytes() == t.tobytes() and len(got["taken.t"]) == 3
    # an empty queue: integrated, mvImuFromLastFrame cleared
    d, _ = tracking_arrays(2, m_queue=0)
    got = run(driver, tmp_path, "list", d)
    assert list(got["ret"][:2]) == [-1, 1] and len(got["taken.t"]) == 0
    # a single point in the window: "Empty IMU measurements vector", returned without setIntegrated()
    d, (a, w, t, t_prev, t_cur, *_rest) = tracking_arrays(3, m_queue=1, lead=0.06)
    got = run(driver, tmp_path, "list", d)
    assert list(got["ret"][:2]) == [-1, 0] and len(got["taken.t"]) == 1 and len(got["queue.t"]) == 1
    # every point too old: none taken, all popped, zero steps to integrate
    d, _ = tracking_arrays(4, m_queue=5, lead=-0.5)
    got = run(driver, tmp_path, "list", d)
    assert list(got["ret"][:2]) == [0, 0] and len(got["taken.t"]) == 0 and len(got["queue.t"]) == 0


def keyframe_arrays(ctx=None):
    """Six KeyFrames around the 0.01 test: the gyro bias moved by 0.0099, 0.0101 (two of them, one without a
    preintegration), 0.2, 0 and 0.0101 along another axis"""
    nga, walk = FX.noise()
    new_bias = np.array([0.02, -0.01, 0.03, 0.001, -0.002, 0.003], f)
    moves = [(0.0099, 0), (0.0101, 0), (0.0101, 1), (0.2, 2), (0.0, 0), (0.0101, 2)]
    has = np.array([1, 1, 0, 1, 1, 1], np.int32)
    names = ["n10", "n3", None, "n65", "n2", "n10"]
    d = {"noise": np.concatenate([nga, walk]), "n_kf": np.array([6], np.int32), "new_bias": new_bias, "kf.has": has}
    biases, states = [], []
    for i, ((mv, ax), nm) in enumerate(zip(moves, names)):
        b = new_bias.copy()
        b[:3] += f(0.05)                      # the accelerometer bias does not enter the test
        b[3 + ax] += f(mv)
        biases.append(b)
        if nm is None:
            states.append(None)
            continue
        P = FX.build(nm)
        s = imu.preintegrate(ctx, P.meas, b, nga, walk) if ctx is not None else empty_state(b, nga, walk)
        if ctx is None:
            s.meas = np.array(P.meas)
        states.append(s)
        d.update(pre_arrays("kf%d" % i, s))
    d["kf.bias"] = np.concatenate(biases).astype(f)
    g = np.stack(biases)[:, 3:] - new_bias[3:]
    moved = np.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1] + g[:, 2] * g[:, 2]).astype(f)).astype(np.float64) > 0.01
    return d, new_bias, states, moved


def test_the_gyro_bias_test_and_set_new_bias(driver, tmp_path):
    d, new_bias, states, moved = keyframe_arrays()
    assert list(moved) == [False, True, True, True, False, True]
    got = run(driver, tmp_path, "todo", d)
    assert list(got["picked"]) == [1, 3, 5] and got["ret"][0] == 3     # KeyFrame 2 moved but holds no preintegration
    assert got["kf.bias"].tobytes() == np.tile(new_bias, 6).tobytes()  # SetNewBias(b) on every KeyFrame
    for i, s in enumerate(states):
        if s is None:
            continue
        row = got["kf%d.state" % i]
        assert row[:298].tobytes() == state_row(s)[:298].tobytes()      # nothing reintegrated here
        assert row[298:304].tobytes() == new_bias.tobytes()             # bu
        assert row[304:].tobytes() == np.concatenate([new_bias[3:] - s.b[3:], new_bias[:3] - s.b[:3]]).tobytes()


# ----------------------------------------------------------------------------------- GPU: the round trips
@pytest.fixture(scope="module")
def ctx():
    from orb_slam3_comments_ghr_amd import Context

    c = Context(0)
    yield c
    c.close()


@pytest.mark.gpu
def test_preintegrate_imu_equals_the_direct_calls(driver, tmp_path, ctx):
    P = FX.build("n65")
    from_kf = imu.preintegrate(ctx, P.meas, P.bias, P.nga, P.nga_walk)
    from_kf.set_new_bias(P.bias + f(0.001))
    d, (a, w, t, t_prev, t_cur, last_bias, _, nga, walk) = tracking_arrays(7, from_kf=from_kf)
    got = run(driver, tmp_path, "track", d)
    taken, popped = imu.select_imu(t, t_prev, t_cur)
    meas = imu.integrables_from_imu(a[taken], w[taken], t[taken], t_prev, t_cur)
    assert list(got["ret"]) == [len(meas), 1, 1, 1, 1, 2]
    assert got["queue.t"].tobytes() == t[popped:].tobytes() and got["taken.t"].tobytes() == t[taken].tobytes()
    cont, fresh = imu.preintegrate_batch(ctx, [imu.ImuProblem(meas, init=from_kf),
                                               imu.ImuProblem(meas, last_bias, nga, walk)])
    assert got["from_kf.state"].tobytes() == state_row(cont).tobytes()   # bu and db stay those of the KeyFrame's state
    assert got["from_kf.meas"].tobytes() == np.concatenate([P.meas, meas]).tobytes()
    assert got["frame.state"].tobytes() == state_row(fresh).tobytes()
    assert got["frame.meas"].tobytes() == meas.tobytes()
    assert fresh.b.tobytes() == last_bias.tobytes() and cont.b.tobytes() == P.bias.tobytes()


@pytest.mark.gpu
def test_preintegrate_imu_with_every_point_too_old_hands_over_empty_states(driver, tmp_path, ctx):
    d, (a, w, t, t_prev, t_cur, last_bias, from_kf, nga, walk) = tracking_arrays(4, m_queue=5, lead=-0.5)
    got = run(driver, tmp_path, "track", d)
    assert list(got["ret"]) == [0, 1, 1, 1, 1, 2]
    assert got["frame.state"].tobytes() == state_row(empty_state(last_bias, nga, walk)).tobytes()
    assert got["from_kf.state"].tobytes() == state_row(from_kf).tobytes() and len(got["frame.meas"]) == 0


@pytest.mark.gpu
def test_reintegrate_keyframes_equals_the_direct_batch(driver, tmp_path, ctx):
    d, new_bias, states, moved = keyframe_arrays(ctx)
    got = run(driver, tmp_path, "reintegrate", d)
    assert got["ret"][0] == 3 and got["kf.bias"].tobytes() == np.tile(new_bias, 6).tobytes()
    todo = [1, 3, 5]
    again = imu.reintegrate(ctx, [states[i] for i in todo], [new_bias] * 3)
    for i, s in enumerate(states):
        if s is None:
            continue
        row = got["kf%d.state" % i]
        if i in todo:
            want = again[todo.index(i)]
            assert row.tobytes() == state_row(want).tobytes(), i       # b = bu = the new bias, db = 0
            assert want.b.tobytes() == new_bias.tobytes() and not row[304:].any()
        else:
            assert row[:298].tobytes() == state_row(s)[:298].tobytes(), i
            assert row[298:304].tobytes() == new_bias.tobytes()
        assert got["kf%d.meas" % i].tobytes() == s.meas.tobytes()


@pytest.mark.gpu
def test_merge_previous_equals_the_direct_call(driver, tmp_path, ctx):
    Pp, Pc = FX.build("n63"), FX.build("n10")
    prev = imu.preintegrate(ctx, Pp.meas, Pp.bias, Pp.nga, Pp.nga_walk)
    cur = imu.preintegrate(ctx, Pc.meas, Pc.bias, Pc.nga, Pc.nga_walk)
    cur.set_new_bias(Pc.bias + f(0.002))
    d = {"noise": np.concatenate(FX.noise())}
    d.update(pre_arrays("prev", prev))
    d.update(pre_arrays("cur", cur))
    got = run(driver, tmp_path, "merge", d)
    assert got["self.state"].tobytes() == state_row(cur).tobytes()
    merged = imu.merge_previous(ctx, prev, cur)
    assert got["cur.state"].tobytes() == state_row(merged).tobytes()
    assert got["cur.meas"].tobytes() == np.concatenate([Pp.meas, Pc.meas]).tobytes()
    assert got["prev.state"].tobytes() == state_row(prev).tobytes()
