"""CPU: the MLPnPsolver checker and the host parts of the solver.

  * the guard of tests/mlpnp_fixtures.py holds on every fixture at the margins of its group
    (profiles/mlpnp_margins.json, written by tools/mlpnp_margins.py), and the profile is current;
  * osg_mlpnp_ransac_parameters equals pyref's SetRansacParameters over a grid;
  * draw_sets equals pyref's literal list loop under a scripted generator;
  * csrc/mlpnp_select.h, built into a stand-alone host program (with AddressSanitizer and UBSan), replays
    pyref's sequential solver call by call;
  * bad sample indices are refused on the host, before a device is touched.
"""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from orb_slam3_comments_ghr_amd import _abi, load_library
from orb_slam3_comments_ghr_amd import mlpnpsolver as M
from tests import mlpnp_fixtures as FX
from tests import pyref_mlpnp as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "orb_slam3_comments_ghr_amd", "csrc")


# ----------------------------------------------------------------------------------- guard, profile
@pytest.mark.parametrize("name", list(FX.FIXTURES))
def test_fixture_guard_conditions(name):
    t = FX.tolerances(name)
    assert FX.guard(name, t["g"], t["m"]) == []


def test_margins_profile_is_current():
    """The committed profile is what tools/mlpnp_margins.py measures on the committed fixtures: g, m and the
    R, t tolerances are 10 x the largest movements in the group, never chosen numbers."""
    m = FX.margins()
    assert set(m["fixtures"]) == set(FX.FIXTURES) and set(m["groups"]) == set(FX.GROUPS)
    for name in ("n15", "n65", "n80_planar", "n80_kb8"):
        for q, v in FX.spreads(name).items():
            assert m["fixtures"][name][q] == pytest.approx(v, rel=1e-6, abs=1e-15), (name, q)
    for g in FX.GROUPS:
        members = [k for k, f in FX.FIXTURES.items() if f.group == g]
        G = m["groups"][g]
        for q in ("ratio_rel", "rot_rad", "t_rel", "quant_rel"):
            assert G[q + "_max"] == max(m["fixtures"][k][q] for k in members)
        assert (G["g"], G["m"], G["rot_tol"], G["t_tol"]) == (
            10.0 * G["ratio_rel_max"], 10.0 * G["quant_rel_max"], 10.0 * G["rot_rad_max"], 10.0 * G["t_rel_max"])
    assert all(v["valid"] and v["flagged_hyp_frac"] <= FX.MAX_FLAGGED_HYP for v in m["fixtures"].values())


def test_fixture_shapes():
    """What each fixture is there for."""
    o = {k: FX.outcome(k) for k in FX.FIXTURES}
    assert o["n0"].hyp == -1 and o["n5_min6"].hyp == -1
    # count == min is recorded as the best and does not return
    assert not o["n6_min6"].converged and (o["n6_min6"].hyp, o["n6_min6"].n_best, o["n6_min6"].n_inliers) == (0, 6, 6)
    assert o["n7"].converged and o["n200"].converged and o["n15"].converged
    t, P = o["n100_h300"], FX.build("n100_h300")
    same = np.flatnonzero(np.all(P.samples == P.samples[t.hyp], 1))
    assert not t.converged and t.n_iterations == 300 and len(same) == 2 and t.hyp == same[0]  # the earlier slot
    assert t.n_best == P.min_inliers == t.n_inliers
    a = o["n40_all_out"]
    assert (a.converged, a.hyp, a.n_inliers, a.n_iterations) == (False, -1, 0, 20)
    E = FX.evaluations("n80_planar")[0]
    assert np.all(FX.build("n80_planar").p3dw[:, 2] == 0) and all(i.planar for i in E.info) and o["n80_planar"].converged
    assert not any(i.planar for i in FX.evaluations("n200")[0].info)
    K = FX.build("n80_kb8")
    assert K.cam.type == _abi.CAM_KB8 and o["n80_kb8"].converged
    assert np.count_nonzero(np.hypot(K.bearing[:, 0], K.bearing[:, 1]) > 1.0) > 20  # beyond 45 degrees
    B = FX.evaluations("n40_break")[0]
    stable = ~FX.excluded("n40_break", FX.tolerances("n40_break")["m"])
    assert any(i.gn_end == 2 and s for i, s in zip(B.info, stable))
    assert {i.gn_end for i in FX.evaluations("n200")[0].info} >= {1, 2}
    # points behind the camera are inliers like any other
    P, ob = FX.build("n80_behind"), o["n80_behind"]
    zc = P.p3dw.astype(np.float64) @ ob.R[2] + ob.t[2]
    assert ob.converged and np.count_nonzero(ob.inlier & (zc < 0)) >= 5
    a, b = (FX.evaluations(k)[0].counts for k in FX.CAMERA_PAIR)
    assert not np.array_equal(a, b)  # exchanging the camera changes the counts
    assert FX.build("n6400").n > FX.STAGED_MAX and o["n6400"].converged


def test_pyref_recovers_the_truth_without_noise():
    for kw in ({}, {"planar": True}, {"kb8": True}):
        P = M.synth_mlpnp_problem(np.random.default_rng(7), 60, 0.0, n_hyp=4, noise_px=0.0, **kw)
        E = R.evaluate(P)
        Rt, tt, _ = P.truth
        assert np.all(E.counts == 60), kw
        assert np.abs(E.R[0] - Rt).max() < 1e-5 and np.abs(E.t[0] - tt).max() < 1e-4, kw


def test_pyref_pose_is_free_of_the_basis_and_the_signs():
    P = FX.build("n80_planar")
    a = R.evaluate(P)
    for kw in ({"basis_angle": 1.3}, {"flip_planar": True}, {"flip_solution": True}, {"eigh": True}):
        b = R.evaluate(P, **kw)
        ok = ~FX.ill_conditioned("n80_planar")
        assert np.abs(a.R[ok] - b.R[ok]).max() < 1e-6 and np.array_equal(a.counts[ok], b.counts[ok]), kw


# ----------------------------------------------------------------------------------- host functions
def test_ransac_parameters_match_pyref():
    seen = set()
    for prob in (0.5, 0.99):
        for n in (0, 1, 5, 6, 7, 13, 15, 21, 101, 200, 1000):
            for eps in (0.0, 0.3, 0.4, 0.5, 0.9, 1.0, 1.5, float("nan"), float("inf")):
                for mi in (1, 6, 10, 15, n - 1, n, n + 1):
                    for mx in (0, 1, 7, 300):
                        want = R.ransac_parameters(prob, mi, mx, 6, eps, n)
                        assert M.ransac_parameters(prob, mi, mx, 6, eps, n) == want, (prob, mi, mx, eps, n)
                        seen.add(want[1])
    assert {1, 7, 300} <= seen and len(seen) > 8
    # Tracking's call: (0.99, 10, 300, 6, 0.5, 5.991)
    assert M.ransac_parameters(0.99, 10, 300, 6, 0.5, 200) == (100, 35)
    assert M.ransac_parameters(0.99, 10, 300, 6, 0.5, 15) == (10, 14)   # int(7.5) = 7 raised to 10
    assert M.ransac_parameters(0.99, 10, 300, 6, 0.5, 13) == (10, 8)    # the float truncation of n * 0.5
    assert M.ransac_parameters(0.99, 10, 300, 6, 0.5, 10) == (10, 1)    # min == n
    assert M.ransac_parameters(0.99, 10, 300, 6, 0.5, 8) == (10, 300)   # epsilon > 1: the quotient is NaN


def test_draw_sets_matches_the_literal_loop():
    rng = np.random.default_rng(3)
    for n in (6, 7, 8, 15, 100):
        h = 100
        ri = np.stack([rng.integers(0, n - j, h) for j in range(6)], 1)
        # the corner draws: always the last slot, always the first, the last then the first
        ri[0] = [n - 1 - j for j in range(6)]
        ri[1] = 0
        ri[2] = [n - 1, 0, n - 3, 0, n - 5, 0]
        got = M.draw_sets(n, h, ri)
        np.testing.assert_array_equal(got, R.draw_sets_literal(n, h, ri))
        assert np.all((got >= 0) & (got < n)) and all(len(set(r)) == 6 for r in got.tolist())


# ----------------------------------------------------------------------------------- the selection header
@pytest.fixture(scope="module")
def select_exe(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    exe = str(tmp_path_factory.mktemp("mlpnp") / "mlpnp_select")
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-I" + CSRC,
                        os.path.join(ROOT, "tests", "host", "mlpnp_select.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def run_select(exe, text):
    r = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr[-3000:]
    return r.stdout.splitlines()


def pyref_calls(counts, max_its, min_inliers, window, n_calls):
    """pyref's sequential solver driven call by call -> the lines the program must print."""
    counts = np.asarray(counts, np.int32)

    class P:
        p3dw = np.zeros((max(int(min_inliers), 1), 3), np.float32)
        samples = np.zeros((len(counts), 6), np.int32)
    P.min_inliers = min_inliers
    E = R.Evaluation(counts, np.zeros((len(counts), len(P.p3dw)), bool), np.zeros((len(counts), 3, 3)),
                     np.zeros((len(counts), 3)), None, None)
    S = R.Solver(P, E, max_its)
    lines = []
    for _ in range(n_calls):
        S.returned = -1
        ok, no_more, _, nin, _ = S.iterate(window)
        assert ok == (S.returned >= 0) and (not ok or nin == counts[S.returned])
        lines.append(f"{int(ok and not no_more)} {int(no_more)} {S.returned} {S.mnIterations} {S.mnBestInliers}")
    return lines


def consumed(max_its, window, n_calls):
    it = 0
    for _ in range(n_calls):
        it += max(max_its - it, window)
    return it


def test_selection_header_replays_the_sequential_solver(select_exe):
    rng = np.random.default_rng(11)
    cases = []
    for trial in range(300):
        mx = int(rng.choice([1, 2, 3, 7, 20, 35, 300]))
        mi = int(rng.integers(1, 12))
        for window, n_calls in ((1, 4), (5, 3), (mx, 2)):
            n = consumed(mx, window, n_calls)
            # few distinct values: many ties and many counts equal to min_inliers
            hi = mi + 2 if trial % 3 else mi + 1
            counts = rng.integers(max(0, mi - 3), hi, n)
            if trial % 5 == 0:
                counts[:] = np.minimum(counts, mi)   # never converges: count == min is recorded, not returned
            if trial % 7 == 0:
                counts[:] = counts[0]                # all equal: the first one stays the best
            if trial % 11 == 0:
                counts[:] = np.minimum(counts, mi - 1)  # nothing reaches min_inliers: failure
            cases.append((counts, mx, mi, window, n_calls))
    text = "".join(f"W {mx} {mi} {w} {k} " + " ".join(map(str, c)) + "\n" for c, mx, mi, w, k in cases)
    out = run_select(select_exe, text)
    pos = first_longer = later_calls = 0
    for c, mx, mi, w, k in cases:
        want = pyref_calls(c, mx, mi, w, k) + ["end"]
        assert out[pos:pos + len(want)] == want, (c.tolist(), mx, mi, w, k)
        pos += len(want)
        # the OR loop condition: a first call that does not return early runs max(max_its, window) iterations
        first = want[0].split()
        if first[0] == "0":
            assert int(first[3]) == max(mx, w)
            first_longer += mx > w
        later_calls += any(l.split()[0] == "0" and int(l.split()[3]) > max(mx, w) for l in want[1:-1])
    assert pos == len(out) and first_longer > 50 and later_calls > 50
    # replay_window, the form the other tests use, agrees as well
    for c, mx, mi, w, k in cases[:200]:
        it, best, bh = 0, 0, -1
        for line in pyref_calls(c, mx, mi, w, k):
            conv, hyp, its, best, bh = R.replay_window(c, mi, it, max(mx - it, w), best, bh)
            assert f"{conv} {1 - conv} {hyp} {its} {best}" == line
            it = its


def test_selection_header_matches_the_fixtures(select_exe):
    for name in ("n200", "n100_h300", "n6_min6", "n40_all_out", "n15"):
        P, E, o = FX.build(name), FX.evaluations(name)[0], FX.outcome(name)
        out = run_select(select_exe, f"W {P.n_hyp} {P.min_inliers} 1 1 " + " ".join(map(str, E.counts)) + "\n")
        conv, no_more, hyp, its, best = map(int, out[0].split())
        assert (bool(conv), hyp, its, best) == (o.converged, o.hyp, o.n_iterations, o.n_best) and out[1] == "end"


def test_parameters_in_the_header_match_the_library(select_exe):
    grid = [(p, mi, mx, e, n) for p in (0.9, 0.99) for n in (0, 6, 13, 15, 200) for mi in (6, 10, n) for mx in (1, 300)
            for e in (0.4, 0.5, 1.0)]
    out = run_select(select_exe, "".join(f"P {p} {mi} {mx} 6 {e} {n}\n" for p, mi, mx, e, n in grid))
    assert [tuple(map(int, v.split())) for v in out] == [R.ransac_parameters(p, mi, mx, 6, e, n) for p, mi, mx, e, n in grid]


# ----------------------------------------------------------------------------------- validation on the host
def test_bad_sample_indices_are_refused_without_a_device():
    """Indices outside [0, n) or repeated within a set: OSG_E_INVALID from the host check that osg_mlpnp_ransac
    and its batch form make before anything is uploaded (tests/test_mlpnp_gpu.py sees it through them)."""
    lib = load_library()
    P = FX.build("n15")
    st = P.struct()
    assert lib.osg_mlpnp_check_samples(C.byref(st)) == 0
    for bad in ([0, 1, 2, 3, 4, P.n], [0, 1, 2, 3, 4, -1], [0, 1, 2, 3, 4, 4], [7, 1, 2, 3, 7, 5]):
        for slot in (0, 3, P.n_hyp - 1):
            Q = M.MlpnpProblem(P.bearing, P.p3dw, P.p2d, P.max_err, P.samples.copy(), P.min_inliers, P.cam)
            Q.samples[slot] = bad
            st = Q.struct()
            assert lib.osg_mlpnp_check_samples(C.byref(st)) == _abi.OSG_E_INVALID, (bad, slot)
