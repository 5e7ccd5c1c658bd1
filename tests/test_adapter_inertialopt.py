"""The three overloads of Optimizer::InertialOptimization through the ORB-SLAM3-side adapter
(adapters/orbslam3/osg_orbslam3.h) on the mock objects of tests/adapter/mock_inertialopt.h, driven by
tests/adapter/inertialopt_driver.cpp.

  * CPU: the gather against a Python restatement of the rules of ref:src/Optimizer.cc:3733-3852 on a map of two chains
    and an edge-less KeyFrame with every excluding case added: a KeyFrame above maxKFid, a bad KeyFrame, an mPrevKF
    above maxKFid, a KeyFrame without a preintegration; the float -> double casts, the start of the bias vertices.
  * GPU: the round trip of each overload against the direct library call on the same problem, bit for bit: the
    reference arguments, SetVelocity's float casts and the bias order on exactly the KeyFrames with a vertex, one
    Reintegrate() where the gyro bias moved by more than 0.01 and none elsewhere; overload 3 writes no KeyFrame.
"""
import os
import subprocess

import numpy as np
import pytest

from orb_slam3_comments_ghr_amd import imu
from orb_slam3_comments_ghr_amd import optimizer as O
from tests import inertialopt_fixtures as FX
from tests.preintegration_fixtures import noise
from tests.test_adapter_preintegration import pre_arrays, state_row
from tools.adapter_arrays import read_arrays, write_arrays

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "orb_slam3_comments_ghr_amd")
DRIVER_SRC = os.path.join(ROOT, "tests", "adapter", "inertialopt_driver.cpp")
f = np.float32


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("inertialopt") / "inertialopt_driver")
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
    return read_arrays(fo), r.stdout


def state_of(q, nga, walk):
    """a restatement's Preintegrated as the package's PreintegratedState"""
    meas = np.array([np.concatenate([a, w, [dt]]) for a, w, dt in q.mvMeasurements], f).reshape(-1, 7)
    return imu.PreintegratedState(q.dR, q.dV, q.dP, q.JRg, q.JVg, q.JVa, q.JPg, q.JPa, q.b, q.dT, q.C, q.avgA, q.avgW,
                                  bu=q.bu, meas=meas, nga=nga, nga_walk=walk)


def mock_map(extras=True):
    """vpKFs of the "chains" fixture (two chains and an edge-less KeyFrame) and, with extras, the excluded cases.
    Returns the driver's arrays and the expected gather: (kept KeyFrames, prev, cur, edge owners)."""
    P = FX.build("chains")
    M = P.map
    nga, walk = noise()
    n = P.n
    ids = list(range(n))
    prev = [-1] * n
    states = [None] * n
    for e in range(len(M.prev)):
        prev[int(M.cur[e])] = int(M.prev[e])
        states[int(M.cur[e])] = state_of(M.preint[e], nga, walk)
    bad = [0] * n
    Rwb, twb, v = M.Rwb.astype(f), M.twb.astype(f), M.v.astype(f)
    rng = np.random.default_rng(12)
    bias = rng.normal(0, 1e-3, (n, 6)).astype(f)
    bias[2, 3:] += f(0.05)          # this KeyFrame's gyro bias will move by more than 0.01
    max_id = n - 1
    if extras:
        donor = states[1]
        def add(i, p, b, s):
            nonlocal Rwb, twb, v, bias
            ids.append(i), prev.append(p), bad.append(b), states.append(s)
            Rwb = np.concatenate([Rwb, Rwb[:1]])
            twb = np.concatenate([twb, twb[:1] + f(1)])
            v = np.concatenate([v, v[:1]])
            bias = np.concatenate([bias, bias[:1]])
        max_id = 40
        add(41, 0, 0, donor)          # above maxKFid: no vertex, no edge
        add(20, n, 0, donor)          # its mPrevKF (41) is above maxKFid: a vertex, no edge
        add(21, 9, 1, donor)          # bad: a vertex, no edge (KeyFrame 9 is the edge-less one)
        add(22, 9, 0, None)           # no preintegration: the reference's message, no edge
    kept = [i for i, k in enumerate(ids) if k <= max_id]
    index = {i: j for j, i in enumerate(kept)}
    own = [i for i in range(len(ids)) if prev[i] >= 0 and ids[i] <= max_id and not bad[i] and ids[prev[i]] <= max_id
           and states[i] is not None and prev[i] in index]
    arrays = {"kf.id": np.array(ids, np.int32), "kf.prev": np.array(prev, np.int32), "kf.bad": np.array(bad, np.int32),
              "kf.has": np.array([s is not None for s in states], np.int32), "kf.Rwb": Rwb.ravel(), "kf.twb": twb.ravel(),
              "kf.v": v.ravel(), "kf.bias": bias.ravel(), "noise": np.concatenate([nga, walk]).astype(f),
              "max_id": np.array([max_id], np.int32)}
    for i, s in enumerate(states):
        if s is not None:
            arrays.update(pre_arrays("kf%d" % i, s))
    exp = dict(kept=kept, prev=[index[prev[i]] for i in own], cur=[index[i] for i in own], own=own, states=states,
               Rwb=Rwb, twb=twb, v=v, bias=bias, ids=ids, P=P)
    return arrays, exp


def args(Rwg, scale, prior_g=1e2, prior_a=1e10, mono=True, fixed_vel=False):
    return np.concatenate([np.asarray(Rwg, np.float64).ravel(), [scale, prior_g, prior_a, float(mono), float(fixed_vel)]])


def test_gather_follows_the_reference_rules(driver, tmp_path):
    arrays, E = mock_map()
    arrays["args"] = args(np.eye(3), 1.0)
    got, stdout = run(driver, tmp_path, "gather", arrays)
    k = E["kept"]
    assert got["kfs"].tolist() == k
    assert np.array_equal(got["Rwb"], E["Rwb"][k].astype(np.float64).ravel())
    assert np.array_equal(got["twb"], E["twb"][k].astype(np.float64).ravel())
    assert np.array_equal(got["v"], E["v"][k].astype(np.float64).ravel())
    assert got["prev"].tolist() == E["prev"] and got["cur"].tolist() == E["cur"]
    assert len(E["own"]) == 7       # the fixture's seven edges, none of the four added cases
    want = np.concatenate([state_row(E["states"][i])[:292] for i in E["own"]])   # osg_pio_preintegrated: 292 floats
    assert got["pre"].tobytes() == want.tobytes()
    b0 = E["bias"][0].astype(np.float64)
    assert np.array_equal(got["start"], np.concatenate([b0[3:], b0[:3]]))       # (bg, ba) of vpKFs.front()
    assert got["check"][0] == 0
    assert stdout.count("Not preintegrated measurement") == 1


@pytest.fixture(scope="module")
def ctx():
    from orb_slam3_comments_ghr_amd import Context
    c = Context(0)
    yield c
    c.close()


def direct(ctx, E, build):
    k = E["kept"]
    own = E["own"]
    b0 = E["bias"][0].astype(np.float64)
    M = O.InertialMap(E["Rwb"][k], E["twb"][k], E["v"][k], E["prev"], E["cur"], [E["states"][i] for i in own],
                      b0[3:], b0[:3])
    return O.Optimizer(ctx).InertialOptimization(build(M))


def check_keyframes(ctx, got, E, r):
    """velocities, biases and preintegrations of every KeyFrame after overloads 1 and 2"""
    k = E["kept"]
    n = len(E["ids"])
    b = np.concatenate([r.ba, r.bg]).astype(f)
    vel, bias, writes = got["kf.v"].reshape(n, 3), got["kf.bias"].reshape(n, 6), got["kf.writes"].reshape(n, 2)
    moved = []
    for i in range(n):
        if i not in k:
            assert vel[i].tobytes() == E["v"][i].tobytes() and bias[i].tobytes() == E["bias"][i].tobytes()
            assert writes[i].tolist() == [0, 0]
            continue
        assert vel[i].tobytes() == r.v[k.index(i)].astype(f).tobytes(), i
        assert bias[i].tobytes() == b.tobytes() and writes[i].tolist() == [1, 1], i
        if np.linalg.norm((E["bias"][i][3:] - b[3:]).astype(f)) > 0.01 and E["states"][i] is not None:
            moved.append(i)
    assert 2 in moved
    # the moved ones reintegrated with b = bu = the new bias; the others keep their integration, bu and db move
    ids_seen = {}
    for i in range(n):
        s = E["states"][i]
        if s is None:
            continue
        row = got["kf%d.state" % i]
        if i in moved:
            if id(s) not in ids_seen:
                ids_seen[id(s)] = imu.reintegrate(ctx, [s], [b])[0]
            assert row.tobytes() == state_row(ids_seen[id(s)]).tobytes(), i
        else:
            assert row[:298].tobytes() == state_row(s)[:298].tobytes(), i
            if i in k:
                assert row[298:304].tobytes() == b.tobytes(), i


@pytest.mark.gpu
def test_initialisation_round_trip(driver, tmp_path, ctx):
    arrays, E = mock_map()
    P = E["P"]
    arrays["args"] = args(P.Rwg, 1.0)
    got, _ = run(driver, tmp_path, "init", arrays)
    r = direct(ctx, E, lambda M: O.inertial_initialization_problem(M, P.Rwg, 1.0, prior_g=1e2, prior_a=1e10))
    assert got["ok"][0] == 1
    assert got["ref"].tobytes() == np.concatenate([r.Rwg.ravel(), [r.scale], r.bg, r.ba]).tobytes()
    check_keyframes(ctx, got, E, r)


@pytest.mark.gpu
def test_bias_only_round_trip(driver, tmp_path, ctx):
    arrays, E = mock_map()
    arrays["args"] = args(np.eye(3), 1.0, 1e2, 1e6)
    got, _ = run(driver, tmp_path, "bias", arrays)
    r = direct(ctx, E, lambda M: O.inertial_bias_problem(M, 1e2, 1e6))
    assert got["ok"][0] == 1
    assert got["ref"][10:].tobytes() == np.concatenate([r.bg, r.ba]).tobytes()
    check_keyframes(ctx, got, E, r)


@pytest.mark.gpu
def test_scale_refinement_writes_no_keyframe(driver, tmp_path, ctx):
    arrays, E = mock_map()
    P = E["P"]
    arrays["args"] = args(P.Rwg, 1.1)
    got, _ = run(driver, tmp_path, "scale", arrays)
    r = direct(ctx, E, lambda M: O.inertial_scale_refinement_problem(M, P.Rwg, 1.1))
    assert got["ok"][0] == 1
    assert got["ref"][:10].tobytes() == np.concatenate([r.Rwg.ravel(), [r.scale]]).tobytes()
    assert got["ref"][10:].tolist() == [-7.0] * 6     # bg and ba are not arguments of this overload
    assert got["kf.v"].tobytes() == E["v"].tobytes() and got["kf.bias"].tobytes() == E["bias"].tobytes()
    assert not got["kf.writes"].any()


@pytest.mark.gpu
def test_a_keyframe_with_two_successors_writes_nothing(driver, tmp_path, ctx):
    arrays, E = mock_map(extras=False)
    prev = arrays["kf.prev"].copy()
    prev[3] = prev[2]                # KeyFrames 2 and 3 share an mPrevKF: the library answers OSG_E_INVALID
    arrays["kf.prev"] = prev
    arrays["args"] = args(np.eye(3), 1.0)
    got, _ = run(driver, tmp_path, "init", arrays)
    assert got["ok"][0] == 0 and not got["kf.writes"].any()
    assert got["ref"][:10].tolist() == np.eye(3).ravel().tolist() + [1.0]
