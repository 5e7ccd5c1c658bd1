"""GPU: osg_optimize_essential_graph_4dof (csrc/essgraph.hip) against tests/pyref_essgraph4dof.py on the fixtures
of tests/essgraph4dof_fixtures.py, and against known answers.

The reference differentiates Edge4DoF numerically, so, as tests/test_essgraph_gpu.py explains for EdgeSim3, the
estimate is defined up to differentiation noise and the LM iteration and trial counts are not defined at all:
they are printed, never asserted, except on the failed-solve graph where nothing depends on differentiation.

Against pyref, per fixture and again at max_iterations = 1 (one linearisation and one solve):
  * per-vertex rotation |LogSO3(Ra Rb')| of Rcw, |d tcw| over the graph's largest |tcw|, and chi2_final
    (relative): 10 x the largest spread of the fixture's group in the 16-replica study of pyref
    (profiles/essgraph4dof_margins.json, tools/essgraph4dof_margins.py), or the BA floor of DESIGN.md §5 (chi2 1e-9
    relative, states 1e-6) where that is larger;
  * tilt, the angle between (Rwb_out Rwb_in') z and z per vertex, compared with pyref's, and edge_chi2 relative to
    the fixture's largest edge chi2: 10 x the group's spread, no floor;
  * chi2_initial, which has no differentiation in it: 1e-12 relative.
Known answers, independent of pyref: see each test.  Every test prints what it measured; DESIGN.md §3.26 quotes
the figures of an MI355X run.
"""
import copy
import ctypes
import functools
import json
import os
import time

import numpy as np
import pytest

from orb_slam3_comments_ghr_amd import Context, _abi
from orb_slam3_comments_ghr_amd import optimizer as op
from tests import essgraph4dof_fixtures as FX
from tests import essgraph_fixtures as FX7
from tests import pyref_essgraph4dof as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOOR = {"chi2_rel": 1e-9, "rot_rad": 1e-6, "t_rel": 1e-6}  # DESIGN.md §5, BA: what tests/test_essgraph_gpu.py uses
NO_FLOOR = ("tilt_rad", "edge_chi2_rel")
CHI2_INITIAL_TOL = 1e-12
# the bounds tests/test_essgraph_gpu.py puts on its consistent graphs
TRUTH_BOUND = {"rot_rad": 1e-9, "t_m": 1e-9, "chi2_final": 1e-18}


@functools.lru_cache(maxsize=None)
def tolerances(name, cap):
    with open(os.path.join(ROOT, "profiles", "essgraph4dof_margins.json")) as f:
        m = json.load(f)["groups"][FX.FIXTURES[name].group]["cap1_max" if cap else "full_max"]
    tol = {q: max(10.0 * m[q], FLOOR[q]) for q in FLOOR}
    for q in NO_FLOOR:
        tol[q] = 10.0 * m[q]
    tol["chi2_initial_rel"] = CHI2_INITIAL_TOL
    return tol


@functools.lru_cache(maxsize=None)
def reference(name, cap, unit_info=False):
    """pyref's result of a fixture, computed once and only read"""
    P = FX.build(name, cap)
    if unit_info:
        P.info_diag = FX.UNIT_INFO
    return R.optimize(P)


def compare(name, cap, P, got, unit_info=False):
    ref = reference(name, cap, unit_info)
    print(f"{name} cap={cap}: lm_iterations gpu {got.lm_iterations} pyref {ref.lm_iterations}, "
          f"lm_trials gpu {got.lm_trials} pyref {ref.lm_trials}, chi2 {got.chi2_initial:.6e} -> {got.chi2_final:.6e}")
    tol = tolerances(name, cap)
    d = R.differences(got, ref, P)
    print("ESSGRAPH4_DIFF", json.dumps({"fixture": name, "cap": cap, "unit_info": unit_info, "differences": d, "tolerances": tol}))
    for q in tol:
        assert d[q] <= tol[q], (q, d[q], tol[q])


def yaw_only_bound(P):
    """Per vertex, what a pure yaw leaves of the tilt of Rwb_out Rwb_in': DR (Rwb_in Rwb_in') z with DR a
    rotation about z is off z by no more than |Rwb_in Rwb_in' - I|_2, the float orthonormality of a KeyFrame's
    Rwb (6e-8) or the double one of a corrected vertex; 1e-12 for the rounding of DR itself over 20 updates."""
    Rin = P.pose[:, :9].reshape(-1, 3, 3)
    S = Rin @ np.swapaxes(Rin, 1, 2) - np.eye(3)
    return np.linalg.norm(S, 2, axis=(1, 2)) + 1e-12


def check_exact(P, got):
    """a fixed vertex is bit-equal to its input; a free one moved in yaw and translation alone and its camera is
    the one of its body pose; chi2_final is the sum of the edges'"""
    fx = P.fixed.astype(bool)
    np.testing.assert_array_equal(got.pose[fx], np.concatenate([P.pose[fx, 12:24], P.pose[fx, 0:12]], 1))
    assert np.all(np.isfinite(got.pose)) and np.all(np.isfinite(got.edge_chi2))
    assert got.chi2_final == pytest.approx(float(got.edge_chi2.sum()), rel=1e-12)
    Rin = P.pose[:, :9].reshape(-1, 3, 3)
    tl = R.tilt(got.Rwb, Rin)
    print("largest tilt of a vertex", float(tl.max()), "bound", float(yaw_only_bound(P).max()))
    assert np.all(tl <= yaw_only_bound(P))
    if got.lm_iterations > 0 and got.chi2_final < got.chi2_initial:    # every free vertex was updated
        Rcb, tcb = P.pose[:, 24:33].reshape(-1, 3, 3), P.pose[:, 33:36]
        Rcw = Rcb @ np.swapaxes(got.Rwb, 1, 2)
        tcw = np.einsum("nij,nj->ni", Rcb, -np.einsum("nji,nj->ni", got.Rwb, got.twb)) + tcb
        assert np.abs(got.R[~fx] - Rcw[~fx]).max() <= 1e-14 and np.abs(got.t[~fx] - tcw[~fx]).max() <= 1e-14


@pytest.mark.parametrize("name", list(FX.FIXTURES))
def test_matches_pyref(ctx, name):
    P = FX.build(name)
    t0 = time.perf_counter()
    got = op.Optimizer(ctx).optimize_essential_graph_4dof(P)
    print(f"{name}: {P.n} vertices, {P.n_edges} edges, call {1e3 * (time.perf_counter() - t0):.2f} ms wall")
    check_exact(P, got)
    assert got.chi2_final < got.chi2_initial
    compare(name, 0, P, got)


@pytest.mark.parametrize("name", list(FX.FIXTURES))
def test_one_iteration_matches_pyref(ctx, name):
    """One linearisation and one solve: nothing hides behind convergence."""
    P = FX.build(name, 1)
    got = op.Optimizer(ctx).optimize_essential_graph_4dof(P)
    assert got.lm_iterations == 1
    check_exact(P, got)
    compare(name, 1, P, got)


@pytest.mark.parametrize("name", ["free5", "kf40x"])
def test_information_is_honoured(ctx, name):
    """the same graph with a unit diagonal gives another result, and pyref's for that diagonal"""
    P = FX.build(name)
    opt = op.Optimizer(ctx)
    weighted = opt.optimize_essential_graph_4dof(P)
    P.info_diag = FX.UNIT_INFO
    unit = opt.optimize_essential_graph_4dof(P)
    assert weighted.chi2_initial > 10 * unit.chi2_initial
    assert R.rot_angle(weighted.R, unit.R).max() > 1e-5
    check_exact(P, unit)
    compare(name, 0, P, unit, unit_info=True)


@pytest.mark.parametrize("name", ["dup_twice", "dup_reversed", "fixed_pair_chain"])
def test_chi2_initial_is_the_sum_over_the_listed_edges(ctx, name):
    """every listed edge counts, a repeated pair twice and an edge between two fixed vertices too; the errors are
    those of the cameras as passed"""
    P = FX.build(name)
    V = R.ImuCamPoses(P.pose)
    e = R.edge_errors(P.e_meas, V.take(P.e_v0), V.take(P.e_v1))
    each = (e * (np.asarray(P.info_diag) * e)).sum(1)
    got = op.Optimizer(ctx).optimize_essential_graph_4dof(P)
    assert abs(got.chi2_initial - each.sum()) <= CHI2_INITIAL_TOL * each.sum()
    if name == "fixed_pair_chain":   # the edge between the fixed vertices keeps its chi2 to the end
        k = int(np.nonzero(P.fixed[P.e_v0].astype(bool) & P.fixed[P.e_v1].astype(bool))[0][0])
        assert each[k] > 0 and abs(got.edge_chi2[k] - each[k]) <= 1e-12 * each[k]
        assert got.chi2_final >= got.edge_chi2[k]
    else:
        assert each[-1] > 0 and P.n_edges > 20


@functools.lru_cache(maxsize=None)
def pyref_truth_distance(name):
    P = FX.build_consistent(*FX.CONSISTENT[name])
    r = R.optimize(P)
    T = R.ImuCamPoses(P.truth)
    return {"rot_rad": float(R.rot_angle(r.R, T.Rcw).max()), "t_m": float(np.abs(r.t - T.tcw).max()),
            "chi2_final": float(r.chi2_final)}


@pytest.mark.parametrize("name", list(FX.CONSISTENT))
def test_consistent_graph_ends_at_its_ground_truth(ctx, name):
    """Independent of pyref's estimate.  The bounds are those of tests/test_essgraph_gpu.py's consistent graphs
    (1e-9 rad, 1e-9 m, chi2 1e-18) where pyref itself meets them on the CPU.  It meets the rotation's (5e-12 rad)
    but not the other two: the yaw row's weight of 1 beside 1e3 on roll and pitch and g2o's lambda leave pyref at
    2e-8 m to 6e-8 m and chi2 1e-15 when the nBad rule stops it, so there the bound is 10 x pyref's own distance.
    A wrong block, a missed edge or a wrong sign leaves 1e-3 or more."""
    P = FX.build_consistent(*FX.CONSISTENT[name])
    got = op.Optimizer(ctx).optimize_essential_graph_4dof(P)
    T = R.ImuCamPoses(P.truth)
    own = pyref_truth_distance(name)
    bound = {q: TRUTH_BOUND[q] if own[q] <= TRUTH_BOUND[q] else 10.0 * own[q] for q in TRUTH_BOUND}
    d = {"rot_rad": float(R.rot_angle(got.R, T.Rcw).max()), "t_m": float(np.abs(got.t - T.tcw).max()),
         "chi2_final": float(got.chi2_final)}
    print("ESSGRAPH4_TRUTH", json.dumps({"graph": name, "chi2_initial": got.chi2_initial, "distance": d, "pyref": own,
                                         "bound": bound, "lm_iterations": got.lm_iterations, "lm_trials": got.lm_trials}))
    check_exact(P, got)
    assert got.chi2_initial > 1e-3
    for q in bound:
        assert d[q] <= bound[q], (q, d[q], bound[q])


def same(a, b):
    return (np.array_equal(a.pose, b.pose) and a.chi2_initial == b.chi2_initial and a.chi2_final == b.chi2_final and
            a.lm_iterations == b.lm_iterations and a.lm_trials == b.lm_trials and np.array_equal(a.edge_chi2, b.edge_chi2))


def same7(a, b):
    return (np.array_equal(a.sim3, b.sim3) and a.chi2_initial == b.chi2_initial and a.chi2_final == b.chi2_final and
            a.lm_iterations == b.lm_iterations and a.lm_trials == b.lm_trials and np.array_equal(a.edge_chi2, b.edge_chi2))


def test_two_runs_are_bit_identical(ctx):
    opt = op.Optimizer(ctx)
    for name in ("kf40x", "dup_reversed", "kf200"):
        P = FX.build(name)
        assert same(opt.optimize_essential_graph_4dof(P), opt.optimize_essential_graph_4dof(P)), name


def test_small_graph_after_a_large_one_equals_a_fresh_context(ctx):
    """the 200-KeyFrame call leaves larger buffers, its slots and its own matrix behind; the 5-KeyFrame call reads
    none of it"""
    opt = op.Optimizer(ctx)
    big, small = FX.build("kf200"), FX.build("free4")
    assert small.n == 5
    opt.optimize_essential_graph_4dof(big)
    after = opt.optimize_essential_graph_4dof(small)
    fresh_ctx = Context(0)
    try:
        fresh = op.Optimizer(fresh_ctx).optimize_essential_graph_4dof(small)
    finally:
        fresh_ctx.close()
    assert same(after, fresh)


def test_sim3_graph_is_untouched_by_a_4dof_call(ctx):
    """osg_optimize_essential_graph before and after a 4-DoF call on the same context (the two share the slots,
    the matrix store and the factorisation): identical bits, also after a Sim3 graph whose slots the 4-DoF call
    reuses without writing their rows 4..6"""
    opt = op.Optimizer(ctx)
    for name7, name4 in (("kf40x_free", "kf40x"), ("free5", "kf200")):
        P7, P4 = FX7.build(name7), FX.build(name4)
        before = opt.optimize_essential_graph(P7)
        first = opt.optimize_essential_graph_4dof(P4)
        after = opt.optimize_essential_graph(P7)
        assert same7(before, after), name7
        assert same(first, opt.optimize_essential_graph_4dof(P4)), name4


def test_failed_solve_terminates_after_ten_trials(ctx):
    """a free vertex without an edge: H = 0, g2o's computeLambdaInit gives 0, the pivot is exactly 0 in every
    trial.  Nothing here is differentiation noise, so the counts and the bits are asserted."""
    P = FX.build_failed_solve()
    got = op.Optimizer(ctx).optimize_essential_graph_4dof(P)
    assert (got.lm_iterations, got.lm_trials) == (1, 10)
    np.testing.assert_array_equal(got.pose, np.concatenate([P.pose[:, 12:24], P.pose[:, 0:12]], 1))
    assert got.chi2_final == got.chi2_initial > 0
    ref = R.optimize(P)
    assert (ref.lm_iterations, ref.lm_trials) == (1, 10)
    assert abs(got.chi2_initial - ref.chi2_initial) <= CHI2_INITIAL_TOL * ref.chi2_initial


def test_nothing_to_optimise_returns_the_input(ctx):
    opt = op.Optimizer(ctx)
    P = FX.build("triangle")
    P.fixed[:] = 1
    got = opt.optimize_essential_graph_4dof(P)
    np.testing.assert_array_equal(got.pose, np.concatenate([P.pose[:, 12:24], P.pose[:, 0:12]], 1))
    assert (got.lm_iterations, got.lm_trials) == (0, 0) and got.chi2_final == got.chi2_initial > 0
    Q = FX.build("triangle")
    Q.e_v0, Q.e_v1, Q.e_meas = Q.e_v0[:0], Q.e_v1[:0], Q.e_meas[:0]
    got = opt.optimize_essential_graph_4dof(Q)
    np.testing.assert_array_equal(got.pose, np.concatenate([Q.pose[:, 12:24], Q.pose[:, 0:12]], 1))
    assert (got.lm_iterations, got.lm_trials, got.chi2_initial, got.chi2_final) == (0, 0, 0.0, 0.0)


def raw_call(ctx, P, handle=True, with_out=True, with_chi2=True, arrays=None, **override):
    """osg_optimize_essential_graph_4dof through ctypes with fields of the problem struct overridden or whole
    arrays replaced: (return code, the output poses, the output edge chi2, the result struct)."""
    Q = copy.copy(P)
    for k, v in (arrays or {}).items():
        setattr(Q, k, v)
    st = Q.struct()
    for k, v in override.items():
        setattr(st, k, v)
    res = _abi.OsgEssGraph4Result()
    out, chi = np.full((max(P.n, 1), 24), -7.0), np.full(max(P.n_edges, 1), -7.0)
    res.pose = out.ctypes.data if with_out else None
    res.edge_chi2 = chi.ctypes.data if with_chi2 else None
    res.chi2_initial = res.chi2_final = -7.0
    res.lm_iterations = res.lm_trials = -7
    rc = ctx.lib.osg_optimize_essential_graph_4dof(ctx.handle if handle else None, ctypes.byref(st), ctypes.byref(res))
    return rc, out, chi, res


def test_rejected_arguments_write_nothing_and_leave_the_context_usable(ctx):
    opt = op.Optimizer(ctx)
    P = FX.build("free5")
    before = opt.optimize_essential_graph_4dof(P)

    def edited(a, i, v):
        b = a.copy()
        b.reshape(-1)[i] = v
        return b

    def info(i, v):
        d = list(P.info_diag)
        d[i] = v
        return {"info_diag": tuple(d)}

    cases = {
        "e_v0 = n": raw_call(ctx, P, arrays={"e_v0": edited(P.e_v0, 2, P.n)}),
        "e_v1 = -1": raw_call(ctx, P, arrays={"e_v1": edited(P.e_v1, 0, -1)}),
        "e_v0 == e_v1": raw_call(ctx, P, arrays={"e_v0": edited(P.e_v0, 1, P.e_v1[1])}),
        "null pose": raw_call(ctx, P, pose=None),
        "null fixed": raw_call(ctx, P, fixed=None),
        "null e_v0": raw_call(ctx, P, e_v0=None),
        "null e_meas": raw_call(ctx, P, e_meas=None),
        "null output": raw_call(ctx, P, with_out=False),
        "lambda_init < 0": raw_call(ctx, P, lambda_init=-1e-16),
        "max_iterations < 0": raw_call(ctx, P, max_iterations=-1),
        "info_diag < 0": raw_call(ctx, P, arrays=info(1, -1.0)),
        "info_diag inf": raw_call(ctx, P, arrays=info(4, float("inf"))),
        "info_diag nan": raw_call(ctx, P, arrays=info(2, float("nan"))),
        "n_vertices = -1": raw_call(ctx, P, n_vertices=-1),
        "n_vertices = 65536": raw_call(ctx, P, n_vertices=65536),
        "n_edges = -1": raw_call(ctx, P, n_edges=-1),
        "null handle": raw_call(ctx, P, handle=False),
    }
    for what, (rc, out, chi, res) in cases.items():
        assert rc < 0, what
        assert np.all(out == -7.0) and np.all(chi == -7.0), what
        assert (res.chi2_initial, res.chi2_final, res.lm_iterations, res.lm_trials) == (-7.0, -7.0, -7, -7), what
    assert cases["e_v0 = n"][0] == _abi.OSG_E_INVALID and cases["info_diag nan"][0] == _abi.OSG_E_INVALID
    with pytest.raises(Exception):
        bad = copy.copy(P)
        bad.lambda_init = -1.0
        opt.optimize_essential_graph_4dof(bad)
    # edge_chi2 is optional, and the valid call gives the bits it gave before
    rc, out, chi, res = raw_call(ctx, P, with_chi2=False)
    assert rc == 0 and np.array_equal(out, before.pose) and np.all(chi == -7.0)
    assert (res.chi2_initial, res.chi2_final) == (before.chi2_initial, before.chi2_final)
    rc, out, chi, res = raw_call(ctx, P)
    assert rc == 0 and np.array_equal(out, before.pose) and np.array_equal(chi, before.edge_chi2)
    assert same(before, opt.optimize_essential_graph_4dof(P))


def test_kernel_times_cover_the_4dof_call(ctx):
    opt = op.Optimizer(ctx)
    P = FX.build("kf40")
    opt.essential_graph_kernel_times(True)
    try:
        timed = opt.optimize_essential_graph_4dof(P)
        ms, store = opt.essential_graph_kernel_times(False)
    finally:
        opt.essential_graph_kernel_times(False)
    print("phases", ms, "matrix store bytes", store)
    assert store > 0 and all(v > 0 for v in ms.values())
    assert same(timed, opt.optimize_essential_graph_4dof(P))
