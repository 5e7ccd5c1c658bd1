"""CPU: the restatement of IMU::Preintegrated (tests/pyref_preintegration.py) pinned on closed forms, the fixtures'
guard against profiles/preintegration_margins.json, the host helpers of include/osg_imu.h bit for bit against their
Python restatement, and the host side under AddressSanitizer and UBSan (tests/host/imu_host.cpp)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from orb_slam3_comments_ghr_amd import imu, load_library
from tests import preintegration_fixtures as FX
from tests import pyref_poseinertial as RP
from tests import pyref_preintegration as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f = np.float32


def constant_motion(n=40, dt=0.005, w=(0.3, -0.2, 0.5), a=(0.4, 9.6, -0.7), bias=np.zeros(6)):
    meas = np.zeros((n, 7), f)
    meas[:, 0:3], meas[:, 3:6], meas[:, 6] = a, w, dt
    nga, walk = FX.noise()
    return meas, np.asarray(bias, f), nga, walk


def exp64(v):
    th = np.linalg.norm(v)
    K = np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])
    if th < 1e-12:
        return np.eye(3) + K
    return np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * K @ K


# ----------------------------------------------------------------------------------- the restatement, pinned
def test_constant_motion_matches_the_closed_forms():
    meas, bias, nga, walk = constant_motion()
    p = R.integrate(meas, bias, nga, walk)
    w, a = meas[0, 3:6].astype(np.float64), meas[0, 0:3].astype(np.float64)
    dts = meas[:, 6].astype(np.float64)
    T = dts.sum()
    # n float32 steps, each rounding its result once: n x 6e-8 relative, and the float sum of dt likewise
    n = len(meas)
    assert abs(float(p.dT) - T) <= n * 6e-8 * T
    assert R.rot_angle(p.dR, exp64(w * T)) < n * 1.2e-7
    # the reference's scheme holds dR over a step: dV and dP are its Riemann sums, computed here in float64
    Rk, dV, dP = np.eye(3), np.zeros(3), np.zeros(3)
    for dt in dts:
        dP = dP + dV * dt + 0.5 * Rk @ a * dt * dt
        dV = dV + Rk @ a * dt
        Rk = Rk @ exp64(w * dt)
    assert np.max(np.abs(p.dV - dV)) < n * 6e-8 * np.abs(dV).max() * 4
    assert np.max(np.abs(p.dP - dP)) < n * 6e-8 * np.abs(dP).max() * 4
    # and they converge to the integrals of Exp(w t) a: first order in dt
    ts = np.linspace(0, T, 20001)
    Ra = np.stack([exp64(w * t) @ a for t in ts])
    V = np.concatenate([[np.zeros(3)], np.cumsum((Ra[1:] + Ra[:-1]) / 2 * np.diff(ts)[:, None], 0)])
    Pint = np.sum((V[1:] + V[:-1]) / 2 * np.diff(ts)[:, None], 0)
    assert np.max(np.abs(p.dV - V[-1])) < np.linalg.norm(w) * 0.005 * np.abs(V[-1]).max()
    assert np.max(np.abs(p.dP - Pint)) < np.linalg.norm(w) * 0.005 * np.abs(Pint).max() * 2
    np.testing.assert_allclose(p.avgW, w, rtol=0, atol=n * 6e-8)
    np.testing.assert_allclose(p.avgA, dV / T, rtol=0, atol=n * 6e-8 * 10)


def test_bias_jacobians_match_central_differences_of_reintegration():
    meas, bias, nga, walk = constant_motion()
    p = R.integrate(meas, bias, nga, walk)
    h = 1e-2   # the float32 states carry ~1e-6; over 2h that is 5e-5, below the second-order term h^2
    for axis in range(6):
        e = np.zeros(6, f)
        e[axis] = h
        plus, minus = R.integrate(meas, bias + e, nga, walk), R.integrate(meas, bias - e, nga, walk)
        dV = (plus.dV.astype(np.float64) - minus.dV) / (2 * h)
        dP = (plus.dP.astype(np.float64) - minus.dP) / (2 * h)
        Jv = (p.JVa if axis < 3 else p.JVg)[:, axis % 3]
        Jp = (p.JPa if axis < 3 else p.JPg)[:, axis % 3]
        scale_v, scale_p = np.abs(p.JVg).max(), np.abs(p.JPg).max()
        assert np.max(np.abs(dV - Jv)) < 2e-3 * scale_v, axis
        assert np.max(np.abs(dP - Jp)) < 2e-3 * scale_p, axis
        if axis >= 3:
            M = minus.dR.astype(np.float64).T @ plus.dR.astype(np.float64)
            rot = np.array([M[2, 1] - M[1, 2], M[0, 2] - M[2, 0], M[1, 0] - M[0, 1]]) / 2 / (2 * h)
            # right perturbation: dR(b + db) = dR Exp(JRg db)
            assert np.max(np.abs(rot - p.JRg[:, axis - 3])) < 2e-3 * np.abs(p.JRg).max(), axis


def test_covariance_is_symmetric_and_positive_definite():
    for name in ("n10", "n65", "biaslarge100"):
        C9 = FX.reference(name).C[:9, :9].astype(np.float64)
        s = np.sqrt(np.diag(C9))
        N = C9 / np.outer(s, s)
        assert np.max(np.abs(N - N.T)) < 1e-5, name     # float products in two orders
        assert np.linalg.eigvalsh((N + N.T) / 2).min() > 1e-6, name
        Cw = FX.reference(name).C[9:, 9:]
        assert np.array_equal(Cw, np.diag(np.diag(Cw))) and (np.diag(Cw) > 0).all()
        assert not FX.reference(name).C[:9, 9:].any() and not FX.reference(name).C[9:, :9].any()


def test_reintegrate_and_merge_previous_of_the_restatement():
    P, Q = FX.build("n10"), FX.build("n3")
    a = R.integrate(P.meas, P.bias, P.nga, P.nga_walk)
    bu = P.bias + f(0.01)
    a.SetNewBias(bu)
    assert np.array_equal(a.db, np.concatenate([bu[3:] - P.bias[3:], bu[:3] - P.bias[:3]]))
    a.Reintegrate()
    b = R.integrate(P.meas, bu, P.nga, P.nga_walk)
    assert a.dR.tobytes() == b.dR.tobytes() and a.C.tobytes() == b.C.tobytes() and len(a.mvMeasurements) == 10
    prev = R.integrate(Q.meas, Q.bias, Q.nga, Q.nga_walk)
    a.MergePrevious(prev)
    c = R.integrate(np.concatenate([Q.meas, P.meas]), bu, P.nga, P.nga_walk)
    assert a.dP.tobytes() == c.dP.tobytes() and a.dT == c.dT and len(a.mvMeasurements) == 13


def test_pose_inertial_informations_accept_an_integrated_covariance():
    lib = load_library()
    for name in ("n10", "n200"):
        C = np.ascontiguousarray(FX.reference(name).C, f)
        info9, ig, ia = np.zeros(81), np.zeros(9), np.zeros(9)
        lib.osg_pose_inertial_informations(C.ctypes.data, C.ctypes.data, info9.ctypes.data, ig.ctypes.data,
                                           ia.ctypes.data)
        info9 = info9.reshape(9, 9)
        assert np.isfinite(info9).all() and np.linalg.eigvalsh((info9 + info9.T) / 2).min() > 0
        # in the metric of C's own scale (sqrt of its diagonal) the product is the identity
        s = np.sqrt(np.diag(C[:9, :9].astype(np.float64)))
        prod = (info9 * np.outer(s, s)) @ (C[:9, :9].astype(np.float64) / np.outer(s, s))
        np.testing.assert_allclose(prod, np.eye(9), rtol=0, atol=1e-6)
        want, _ = RP.inertial_information(C)
        np.testing.assert_allclose(info9 * np.outer(s, s), want * np.outer(s, s), rtol=0, atol=1e-6 * 9)
        nga_walk = FX.build(name).nga_walk.astype(np.float64)
        n = FX.FIXTURES[name].n
        np.testing.assert_allclose(np.diag(ig.reshape(3, 3)), 1 / np.diag(C[9:12, 9:12].astype(np.float64)), rtol=1e-12)
        assert abs(ig[0] * n * nga_walk[0] - 1) < 1e-5


# ----------------------------------------------------------------------------------- fixtures and margins
def test_margins_file_covers_every_fixture_and_holds_the_guard():
    m = FX.margins()
    assert set(m["fixtures"]) == set(FX.FIXTURES) and set(m["groups"]) == set(FX.GROUPS)
    for k, s in m["fixtures"].items():
        assert (s["cut_margin"] is None) == (s["n"] == 0), k     # no step, no angle
        assert s["n"] == 0 or s["cut_margin"] > FX.CUT_GUARD, k
        assert s["group"] == FX.FIXTURES[k].group and s["n"] == FX.FIXTURES[k].n
    for g, v in m["groups"].items():
        for q in R.QUANTITIES:
            assert v["tol"][q] == 10.0 * v["max"][q]
            assert v["max"][q] == max(s["spread"][q] for s in m["fixtures"].values() if s["group"] == g)
    assert {FX.FIXTURES[k].n for k in FX.FIXTURES} >= {0, 1, 2, 3, 10, 63, 64, 65, 200, 600}


@pytest.mark.parametrize("name", ["n3", "n65", "both10"])
def test_recorded_study_is_reproduced(name):
    s, m = FX.study(name), FX.margins()["fixtures"][name]
    assert s["below"] == m["below"]
    assert s["cut_margin"] == pytest.approx(m["cut_margin"], rel=1e-9)
    for q, v in s["spread"].items():
        assert v == pytest.approx(m["spread"][q], rel=1e-6, abs=1e-300)


def test_fixtures_cover_both_sides_of_the_cut():
    m = FX.margins()["fixtures"]
    assert m["below10"]["below"] == 10 and m["below100"]["below"] == 100
    assert m["above10"]["below"] == 0 and m["above100"]["below"] == 0
    assert 0 < m["both10"]["below"] < 10 and 0 < m["both100"]["below"] < 100


# ----------------------------------------------------------------------------------- host helpers, bit for bit
def points(m, seed, t_prev=50.0, lead=0.0013):
    rng = np.random.default_rng(seed)
    a, w, t = FX.imu_points(rng, m, t0=t_prev + lead)
    return a, w, t


@pytest.mark.parametrize("m", [1, 2, 3, 4, 12])
def test_integrables_take_the_four_branches_bit_for_bit(m):
    # m = 2: the single step; m = 3: first and last; m >= 4: first, middle, last
    t_prev = 50.0
    a, w, t = points(m, m)
    t_cur = t[-1] - 0.0021
    got = imu.integrables_from_imu(a, w, t, t_prev, t_cur)
    want = R.integrables(a, w, t, t_prev, t_cur)
    assert got.shape == (m - 1, 7) and got.tobytes() == want.tobytes()
    if m >= 2:
        assert got[0, 6] == (f(t_cur - t_prev) if m == 2 else f(t[1] - t_prev))
    # a first point before the previous frame: tini is negative
    got = imu.integrables_from_imu(a, w, t, t_prev + 0.002, t_cur)
    assert got.tobytes() == R.integrables(a, w, t, t_prev + 0.002, t_cur).tobytes()


def test_integrables_reject_bad_arguments():
    lib = load_library()
    assert lib.osg_imu_integrables(None, None, None, 3, 0.0, 1.0, None) == -1
    a, w, t = points(3, 1)
    assert lib.osg_imu_integrables(a.ctypes.data, w.ctypes.data, t.ctypes.data, 0, 0.0, 1.0, None) == -1


def test_select_takes_the_three_queue_branches():
    t_prev, t_cur = 50.0, 50.05
    tq = t_prev + np.array([-0.0110, -0.0060, -0.00101, -0.00099, 0.004, 0.009, 0.0489, 0.04901, 0.054])
    taken, popped = imu.select_imu(tq, t_prev, t_cur)
    assert (list(taken), popped) == R.select(tq, t_prev, t_cur)
    assert list(taken) == [3, 4, 5, 6, 7] and popped == 7       # three dropped, four popped, one taken and kept
    for upto in range(len(tq) + 1):                             # the queue may end in any branch
        taken, popped = imu.select_imu(tq[:upto], t_prev, t_cur)
        assert (list(taken), popped) == R.select(tq[:upto], t_prev, t_cur), upto
    # a timestamp out of order after the window opened is still tested against both bounds
    tq2 = t_prev + np.array([0.001, -0.02, 0.006, 0.2])
    taken, popped = imu.select_imu(tq2, t_prev, t_cur)
    assert (list(taken), popped) == R.select(tq2, t_prev, t_cur) == ([0, 2, 3], 3)
    rng = np.random.default_rng(3)
    for _ in range(20):
        tq3 = np.sort(t_prev + rng.uniform(-0.02, 0.08, 30))
        taken, popped = imu.select_imu(tq3, t_prev, t_cur, 0.001)
        assert (list(taken), popped) == R.select(tq3, t_prev, t_cur, 0.001)


def as_state(p):
    return imu.PreintegratedState(p.dR, p.dV, p.dP, p.JRg, p.JVg, p.JVa, p.JPg, p.JPa, p.b, p.dT, p.C, p.avgA, p.avgW,
                                  nga=p.Nga, nga_walk=p.NgaWalk)


@pytest.mark.parametrize("name", ["n10", "n200", "biaslarge100"])
def test_delta_and_predict_state_match_the_restatement(name):
    ref = FX.reference(name)
    s = as_state(ref)
    rng = np.random.default_rng(FX.FIXTURES[name].seed)
    for db in (np.zeros(6, f), rng.normal(0, 0.01, 6).astype(f), rng.normal(0, 1e-7, 6).astype(f)):
        bias = ref.b + db      # the last: JRg dbg below Sophus's small-angle cut
        dR, dV, dP = imu.delta(s, bias)
        assert dV.tobytes() == ref.GetDeltaVelocity(bias).tobytes()
        assert dP.tobytes() == ref.GetDeltaPosition(bias).tobytes()
        # exp and the normalisation: a few float roundings on a rotation matrix
        assert R.rot_angle(dR, ref.GetDeltaRotation(bias)) < 5e-7
        Rwb = RP.NormalizeRotation(np.eye(3) + 0.3 * rng.normal(size=(3, 3))).astype(f)
        twb, v = rng.normal(0, 2, 3).astype(f), rng.normal(0, 1, 3).astype(f)
        R2, t2, v2 = imu.predict_state(s, bias, Rwb, twb, v)
        wR, wt, wv = R.predict_state(ref, bias, Rwb, twb, v)
        assert R.rot_angle(R2, wR) < 1e-6
        # Rwb1 dP, Rwb1 dV go through the same float sums; only dR differs, and it does not enter these
        assert t2.tobytes() == wt.tobytes() and v2.tobytes() == wv.tobytes()
    s.set_new_bias(ref.b + f(0.004))
    ref.SetNewBias(ref.b + f(0.004))
    try:
        assert imu.delta(s, s.bu)[1].tobytes() == (ref.dV + R.mm(ref.JVg, ref.db[:3]) + R.mm(ref.JVa, ref.db[3:])).tobytes()
    finally:
        ref.SetNewBias(ref.b)


def test_state_round_trips_through_the_struct_and_feeds_the_pose_step():
    ref = FX.reference("n65")
    s = as_state(ref)
    back = imu.PreintegratedState.of(s.struct())
    for k in ("dR", "dV", "dP", "JRg", "JVg", "JVa", "JPg", "JPa", "b", "C", "avgA", "avgW"):
        assert getattr(back, k).tobytes() == np.asarray(getattr(ref, k), f).tobytes(), k
    assert back.dT == ref.dT
    pio = s.to_pio()
    st = pio.struct()
    assert bytes(st) == bytes(s.struct().pre)   # no conversion between the two


def test_calib_cov_squares_in_float():
    nga, walk = imu.calib_cov(1.7e-4, 2e-3, 1.9e-5, 3e-3)
    assert nga.dtype == f and nga[0] == f(1.7e-4) * f(1.7e-4) and nga[3] == f(2e-3) * f(2e-3)
    assert walk[2] == f(1.9e-5) * f(1.9e-5) and walk[5] == f(3e-3) * f(3e-3)


# ----------------------------------------------------------------------------------- host code
def host_program(tmp_path, flags):
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    exe = str(tmp_path / ("imu_host" + str(len(flags))))
    r = subprocess.run([gxx, "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", *flags,
                        "-I" + os.path.join(ROOT, "orb_slam3_comments_ghr_amd", "csrc"),
                        os.path.join(ROOT, "tests", "host", "imu_host.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def test_host_side_under_sanitizers(tmp_path):
    exe = host_program(tmp_path, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    r = subprocess.run([exe, "check"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-2000:] + r.stderr[-3000:]


def test_host_delta_and_predict_state_have_the_recorded_bits(tmp_path):
    """delta and predict_state on a fixed state at three bias steps (the last below Sophus's small-angle cut), byte
    for byte against what the commit before the shared csrc/so3_common.h produced
    (tests/golden/imu_host_bits.txt): they run the kernels' own SO(3) functions now."""
    with open(os.path.join(ROOT, "tests", "golden", "imu_host_bits.txt")) as f:
        want = f.read()
    for flags in ([], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]):
        r = subprocess.run([host_program(tmp_path, flags), "bits"], capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout == want, r.stdout[-2000:] + r.stderr[-3000:]
