"""CPU: the TwoViewReconstruction checker and the host parts.

  * the guard of tests/twoview_fixtures.py holds on every fixture at 10 x the spreads of its group
    (profiles/twoview_margins.json, written by tools/twoview_margins.py), and the profile is current;
  * each fixture is what it is there for;
  * draw_sets equals pyref's literal two-list loop;
  * csrc/twoview_select.h, built into a stand-alone host program (with AddressSanitizer and UBSan), gives
    pyref's ReconstructF / ReconstructH decisions, ties and threshold cases included.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

from orb_slam3_comments_ghr_amd import synth as SY
from orb_slam3_comments_ghr_amd import twoview as T
from tests import pyref_twoview as R
from tests import twoview_fixtures as FX

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "orb_slam3_comments_ghr_amd", "csrc")


# ----------------------------------------------------------------------------------- guard, profile
@pytest.mark.parametrize("name", list(FX.FIXTURES))
def test_fixture_guard_conditions(name):
    tol = FX.tolerances(name)
    assert FX.guard(name, tol) == []
    assert FX.n_borderline(name, tol) <= int(FX.MAX_BORDERLINE * FX.build(name).n)


def test_margins_profile_is_current():
    """The committed profile is what tools/twoview_margins.py measures on the committed fixtures: the tolerances
    are 10 x the largest movement in the group, never a chosen number."""
    m = FX.margins()
    assert set(m["fixtures"]) == set(FX.FIXTURES) and set(m["groups"]) == set(FX.GROUPS) and m["factor"] == FX.FACTOR
    for name in ("n9", "n65", "n100_planar", "n100_collinear"):
        s = FX.spreads(name)
        for q, v in s.items():
            assert m["fixtures"][name][q] == pytest.approx(v, rel=1e-6, abs=1e-12), (name, q)
    for g in FX.GROUPS:
        members = [k for k, f in FX.FIXTURES.items() if f.group == g]
        for q in FX.QUANTITIES:
            assert m["groups"][g][q] == max(m["fixtures"][k][q] for k in members)
    assert all(v["valid"] for v in m["fixtures"].values())


def test_fixture_shapes():
    """What each fixture is there for."""
    o = {k: FX.outcome(k) for k in FX.FIXTURES}
    for k in FX.FIXTURES:
        P = FX.build(k)
        assert len(P.keys1) > P.n and len(P.keys2) > P.n  # Normalize runs over the frame, not over the matches
        assert not np.array_equal(P.idx2, np.arange(P.n))
    assert np.all(np.sort(FX.build("n8").sets, 1) == np.arange(8))
    assert o["n8"].hyp_h == -1 and not o["n8"].inlier_h.any()  # every H score 0: an all-false inlier set
    assert FX.build("n100_h1").n_hyp == 1 and FX.build("n100_general").n_hyp == 200
    g = o["n100_general"]
    assert g.ok and g.model == 1 and max(c.n_good for c in g.checks) == 100
    p = o["n100_planar"]
    assert p.ok and p.model == 0 and len(p.cands) == 8
    for k in ("n100_rotation", "n100_tiny"):
        assert not o[k].ok and o[k].model >= 0 and all(c.parallax < 1.0 for c in o[k].checks)
    assert o["n200_o30"].ok and 0.25 < FX.build("n200_o30").truth[2].mean() < 0.35 and o["n200_o30"].n_inliers < 150
    # the min(50, size - 1) edge and minTriangulated
    assert [max(c.n_good for c in o[k].checks) for k in ("good40", "good51", "good52")] == [40, 51, 52]
    assert (o["good40"].ok, o["good51"].ok, o["good52"].ok) == (False, True, True)
    d, Pd = o["n100_dup"], FX.build("n100_dup")
    for hyp in (d.hyp_h, d.hyp_f):
        same = np.flatnonzero(np.all(Pd.sets == Pd.sets[hyp], 1))
        assert len(same) == 2 and hyp == same[0]
    c, Ec = o["n100_collinear"], FX.replicas("n100_collinear")[0][1]
    assert c.ok and 0 not in (c.hyp_h, c.hyp_f)
    assert not (Ec.score_h[0] > 0.5 * c.score_h) and not (Ec.score_f[0] > 0.5 * c.score_f)
    f, Ef = o["n100_flat"], FX.replicas("n100_flat")[0][1]
    assert f.model == -1 and not f.ok and np.isnan(Ef.score_h).all() and np.isnan(Ef.score_f).all()


def test_pyref_recovers_the_truth_without_noise():
    P = SY.two_view_scene(np.random.default_rng(5), 120, noise_px=0.0, n_hyp=20)
    o = R.reconstruct(P)
    Rt, tt, _ = P.truth
    assert o.ok and o.model == 1 and o.n_inliers == 120
    assert FX.rot_angle(o.R, Rt) < 1e-3 and FX.dir_angle(o.t, tt) < 1e-2
    # the points reproject: depth along the true ray of frame 1
    k = P.idx1[0]
    x = o.p3d[k] / o.p3d[k, 2]
    fx, fy, cx, cy = P.K
    assert abs(fx * x[0] + cx - P.keys1[k, 0]) < 0.05 and abs(fy * x[1] + cy - P.keys1[k, 1]) < 0.05


def test_fewer_than_eight_matches():
    P = FX.build("n9")
    m = P.matches12.copy()
    m[P.idx1[7:]] = -1
    o = R.reconstruct(T.TwoViewProblem(P.keys1, P.keys2, m, np.zeros((3, 8), np.int32), K=P.K))
    assert (o.ok, o.model, o.hyp_h, o.hyp_f, o.cand) == (False, -1, -1, -1, -1) and not o.p3d.any()


# ----------------------------------------------------------------------------------- draw
def test_draw_sets_matches_the_literal_loop():
    import orb_slam3_comments_ghr_amd as pkg
    assert pkg.draw_sets is T.draw_sets and pkg.TwoViewReconstruction is T.TwoViewReconstruction
    rng = np.random.default_rng(3)
    for n in (8, 9, 10, 17, 100):
        h = 200
        ri = np.stack([rng.integers(0, n - j, h) for j in range(8)], 1)
        # corner draws: always the last slot, always the first, the same slot again
        ri[0] = [n - 1 - j for j in range(8)]
        ri[1] = 0
        ri[2] = [n - 1, 0, n - 3, 0, 0, n - 6, 1 % (n - 6), 0]
        got = T.draw_sets(n, h, ri)
        np.testing.assert_array_equal(got, R.draw_sets_literal(n, h, ri))
        assert np.all((got >= 0) & (got < n)) and all(len(set(s)) == 8 for s in got.tolist())
    assert np.all(np.sort(T.draw_sets(8, 5, np.zeros(40, int)), 1) == np.arange(8))


# ----------------------------------------------------------------------------------- the selection header
@pytest.fixture(scope="module")
def select_exe(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    exe = str(tmp_path_factory.mktemp("tvr") / "twoview_select")
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-I" + CSRC,
                        os.path.join(ROOT, "tests", "host", "twoview_select.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def run_select(exe, cases):
    text = "".join(f"{k} {ni} {float(mp)!r} {mt} " + " ".join(map(str, g)) + " " + " ".join(repr(float(np.float32(p))) for p in px) + "\n"
                   for k, ni, mp, mt, g, px in cases)
    r = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr[-3000:]
    return [tuple(map(int, l.split())) for l in r.stdout.splitlines()]


def want(case):
    k, ni, mp, mt, g, px = case
    ok, cand = (R.choose_f if k == "F" else R.choose_h)(list(g), list(px), ni, mp, mt)
    return int(ok), cand


def test_selection_header_gives_the_reference_decisions(select_exe):
    cases = [
        # ReconstructF: a clear winner; parallax exactly minParallax is not enough (strict >)
        ("F", 100, 1.0, 50, (0, 97, 0, 1), (0, 4.5, 0, 0.1)),
        ("F", 100, 1.0, 50, (0, 97, 0, 1), (0, 1.0, 0, 0.1)),
        ("F", 100, 1.0, 50, (0, 97, 0, 1), (0, 1.0000001, 0, 0.1)),
        # maxGood below nMinGood = max(int(0.9 N), 50): 89 < 90, 90 passes; N small: 50 rules
        ("F", 100, 1.0, 50, (89, 0, 0, 0), (5, 0, 0, 0)),
        ("F", 100, 1.0, 50, (90, 0, 0, 0), (5, 0, 0, 0)),
        ("F", 51, 1.0, 50, (49, 0, 0, 0), (5, 0, 0, 0)),
        ("F", 51, 1.0, 50, (50, 0, 0, 0), (5, 0, 0, 0)),
        # nsimilar > 1: 70 > 0.7 * 100 is false (== 70.0), 71 is true
        ("F", 100, 1.0, 50, (100, 70, 0, 0), (5, 5, 0, 0)),
        ("F", 100, 1.0, 50, (100, 71, 0, 0), (5, 5, 0, 0)),
        # ties at maxGood: both similar, rejected; all zero: maxGood 0 < nMinGood
        ("F", 100, 1.0, 50, (95, 95, 0, 0), (5, 5, 0, 0)),
        ("F", 0, 1.0, 50, (0, 0, 0, 0), (0, 0, 0, 0)),
        ("F", 60, 1.0, 0, (0, 0, 0, 60), (0, 0, 0, float("nan"))),
        # ReconstructH: secondBest exactly 0.75 best is not below it; 74 is
        ("H", 100, 1.0, 50, (100, 75, 0, 0, 0, 0, 0, 0), (3, 1, 0, 0, 0, 0, 0, 0)),
        ("H", 100, 1.0, 50, (100, 74, 0, 0, 0, 0, 0, 0), (3, 1, 0, 0, 0, 0, 0, 0)),
        ("H", 100, 1.0, 50, (75, 100, 0, 0, 0, 0, 0, 0), (3, 1, 0, 0, 0, 0, 0, 0)),
        # a later tie becomes the second best, the first keeps the index
        ("H", 100, 1.0, 50, (96, 0, 96, 0, 0, 0, 0, 0), (3, 0, 3, 0, 0, 0, 0, 0)),
        # parallax exactly minParallax passes here (>=); best must exceed minTriangulated and 0.9 N strictly
        ("H", 100, 1.0, 50, (0, 0, 0, 95, 0, 0, 0, 1), (0, 0, 0, 1.0, 0, 0, 0, 9)),
        ("H", 100, 1.0, 50, (0, 0, 0, 95, 0, 0, 0, 1), (0, 0, 0, 0.99999994, 0, 0, 0, 9)),
        ("H", 100, 1.0, 50, (90, 0, 0, 0, 0, 0, 0, 0), (3, 0, 0, 0, 0, 0, 0, 0)),
        ("H", 100, 1.0, 50, (91, 0, 0, 0, 0, 0, 0, 0), (3, 0, 0, 0, 0, 0, 0, 0)),
        ("H", 40, 1.0, 50, (50, 0, 0, 0, 0, 0, 0, 0), (3, 0, 0, 0, 0, 0, 0, 0)),
        ("H", 40, 1.0, 50, (51, 0, 0, 0, 0, 0, 0, 0), (3, 0, 0, 0, 0, 0, 0, 0)),
        ("H", 0, 1.0, 50, (0, 0, 0, 0, 0, 0, 0, 0), (0, 0, 0, 0, 0, 0, 0, 0)),
    ]
    rng = np.random.default_rng(17)
    for _ in range(400):
        k = "F" if rng.random() < 0.5 else "H"
        m = 4 if k == "F" else 8
        ni = int(rng.integers(0, 130))
        g = rng.integers(0, ni + 2, m) * (rng.random(m) < 0.6)
        if rng.random() < 0.3:
            g[rng.integers(m)] = g.max()  # a tie at the top
        cases.append((k, ni, 1.0, 50, tuple(int(v) for v in g), tuple(float(v) for v in rng.choice([0.0, 0.5, 1.0, 2.0, 7.0], m))))
    got = run_select(select_exe, cases)
    assert len(got) == len(cases)
    for c, g in zip(cases, got):
        assert g == want(c), c
    w = [want(c) for c in cases]
    assert sum(ok for ok, _ in w) > 20 and sum(1 for ok, c in w if not ok and c >= 0) > 20
    assert [want(c)[0] for c in cases[:23]] == [1, 0, 1, 0, 1, 0, 1, 1, 0, 0, 0, 0, 0, 1, 0, 0, 1, 0, 0, 1, 0, 1, 0]


def test_selection_header_matches_the_fixtures(select_exe):
    names = [k for k in FX.FIXTURES if FX.outcome(k).cands]
    cases = []
    for k in names:
        o, P = FX.outcome(k), FX.build(k)
        cases.append(("H" if o.model == 0 else "F", o.n_inliers, P.min_parallax, P.min_triangulated,
                      tuple(c.n_good for c in o.checks), tuple(0.0 if np.isnan(c.parallax) else c.parallax for c in o.checks)))
    for k, c, g in zip(names, cases, run_select(select_exe, cases)):
        o = FX.outcome(k)
        if not any(np.isnan(ch.parallax) for ch in o.checks):
            assert g == (int(o.ok), o.cand), k
