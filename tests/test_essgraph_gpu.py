"""GPU: osg_optimize_essential_graph / osg_essgraph_correct_points (csrc/essgraph.hip) against
tests/pyref_essgraph.py on the fixtures of tests/essgraph_fixtures.py, and against known answers.

The reference differentiates EdgeSim3 numerically, so the estimate is defined up to differentiation noise and
the LM iteration and trial counts are not defined at all (after the first accepted steps rho is noise): they are
printed, never asserted, except on the failed-solve graph where nothing depends on differentiation.

Against pyref, per fixture and again at max_iterations = 1 (one linearisation and one solve):
  * per-vertex rotation |log(Ra Rb^T)|, translation |dt| over the graph's largest |t|, relative scale, and
    chi2_final (relative): 10 x the largest spread of the fixture's group in the 16-replica +-1 ulp nudge study
    of pyref (profiles/essgraph_margins.json, tools/essgraph_margins.py), or the BA floor of DESIGN.md §5
    (chi2 1e-9 relative, states 1e-6) where that is larger;
  * edge_chi2 relative to the fixture's largest edge chi2: 10 x the group's spread, no floor;
  * chi2_initial, which has no differentiation in it: 1e-12 relative.
Known answers, independent of pyref: the consistent graphs end within 1e-9 of their ground truth (translation
absolute on the 5 m trajectory, rotation in rad, scale relative) with chi2_final <= 1e-18.
Every test prints what it measured; DESIGN.md §3.19 quotes the figures of an MI355X run.
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
from tests import essgraph_fixtures as FX
from tests import pyref_essgraph as R
from tests import pyref_sim3opt as S3

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOOR = {"chi2_rel": 1e-9, "rot_rad": 1e-6, "t_rel": 1e-6, "s_rel": 1e-6}  # DESIGN.md §5, BA
CHI2_INITIAL_TOL = 1e-12


@functools.lru_cache(maxsize=None)
def tolerances(name, cap):
    with open(os.path.join(ROOT, "profiles", "essgraph_margins.json")) as f:
        m = json.load(f)["groups"][FX.FIXTURES[name].group]["cap1_max" if cap else "full_max"]
    tol = {q: max(10.0 * m[q], FLOOR[q]) for q in FLOOR}
    tol["edge_chi2_rel"] = 10.0 * m["edge_chi2_rel"]
    tol["chi2_initial_rel"] = CHI2_INITIAL_TOL
    return tol


@functools.lru_cache(maxsize=None)
def reference(name, cap):
    """pyref's result of a fixture, computed once and only read"""
    return R.optimize(FX.build(name, cap))


def compare(name, cap, got):
    ref = reference(name, cap)
    print(f"{name} cap={cap}: lm_iterations gpu {got.lm_iterations} pyref {ref.lm_iterations}, "
          f"lm_trials gpu {got.lm_trials} pyref {ref.lm_trials}, chi2 {got.chi2_initial:.6e} -> {got.chi2_final:.6e}")
    tol = tolerances(name, cap)
    d = R.differences(got, ref)
    print("ESSGRAPH_DIFF", json.dumps({"fixture": name, "cap": cap, "differences": d, "tolerances": tol}))
    for q in tol:
        assert d[q] <= tol[q], (q, d[q], tol[q])


def check_exact(P, got):
    """a fixed vertex is bit-equal to its input, and under fix_scale every scale"""
    fx = P.fixed.astype(bool)
    np.testing.assert_array_equal(got.sim3[fx], P.sim3[fx])
    if P.fix_scale:
        np.testing.assert_array_equal(got.sim3[:, 7], P.sim3[:, 7])
    assert np.all(np.isfinite(got.sim3)) and np.all(np.isfinite(got.edge_chi2))
    assert got.chi2_final == pytest.approx(float(got.edge_chi2.sum()), rel=1e-12)


@pytest.mark.parametrize("name", list(FX.FIXTURES))
def test_matches_pyref(ctx, name):
    P = FX.build(name)
    t0 = time.perf_counter()
    got = op.Optimizer(ctx).optimize_essential_graph(P)
    print(f"{name}: {P.n} vertices, {P.n_edges} edges, call {1e3 * (time.perf_counter() - t0):.2f} ms wall")
    check_exact(P, got)
    assert got.chi2_final < got.chi2_initial
    compare(name, 0, got)


@pytest.mark.parametrize("name", list(FX.FIXTURES))
def test_one_iteration_matches_pyref(ctx, name):
    """One linearisation and one solve: nothing hides behind convergence."""
    P = FX.build(name, 1)
    got = op.Optimizer(ctx).optimize_essential_graph(P)
    assert got.lm_iterations == 1
    check_exact(P, got)
    compare(name, 1, got)


@pytest.mark.parametrize("name", ["dup_twice", "dup_reversed", "fixed_pair_chain"])
def test_chi2_initial_is_the_sum_over_the_listed_edges(ctx, name):
    """every listed edge counts, a repeated pair twice and an edge between two fixed vertices too"""
    P = FX.build(name)
    S = R.from_rows(P.sim3)
    e = R.edge_errors(R.from_rows(P.e_meas), R.take(S, P.e_v0), R.take(S, P.e_v1))
    each = (e * e).sum(1)
    got = op.Optimizer(ctx).optimize_essential_graph(P)
    assert abs(got.chi2_initial - each.sum()) <= CHI2_INITIAL_TOL * each.sum()
    if name == "fixed_pair_chain":   # the edge between the fixed vertices keeps its chi2 to the end
        k = int(np.nonzero(P.fixed[P.e_v0].astype(bool) & P.fixed[P.e_v1].astype(bool))[0][0])
        assert each[k] > 0 and abs(got.edge_chi2[k] - each[k]) <= 1e-12 * each[k]
        assert got.chi2_final >= got.edge_chi2[k]
    else:
        assert each[-1] > 0 and P.n_edges == FX.build(name).n_edges > 20


def truth_errors(got, truth):
    T = R.from_rows(truth)
    return (max(S3.rot_log_norm(a, b) for a, b in zip(got.R, T[0])), float(np.abs(got.t - T[1]).max()),
            float(np.abs(got.s / T[2] - 1).max()))


@pytest.mark.parametrize("name", list(FX.CONSISTENT))
def test_consistent_graph_ends_at_its_ground_truth(ctx, name):
    """Independent of pyref.  pyref itself reaches 1e-15 and chi2 1e-29 here; a wrong block, a missed edge or a
    wrong sign leaves 1e-3 or more.  The orders in between are for the device libm and the other factorisation."""
    P = FX.build_consistent(*FX.CONSISTENT[name])
    got = op.Optimizer(ctx).optimize_essential_graph(P)
    rot, tr, sc = truth_errors(got, P.truth)
    print("ESSGRAPH_TRUTH", json.dumps({"graph": name, "chi2_initial": got.chi2_initial, "chi2_final": got.chi2_final,
                                        "rot_rad": rot, "t_m": tr, "s_rel": sc, "lm_iterations": got.lm_iterations,
                                        "lm_trials": got.lm_trials}))
    check_exact(P, got)
    assert got.chi2_initial > 1e-3
    assert rot <= 1e-9 and tr <= 1e-9 and sc <= 1e-9
    assert got.chi2_final <= 1e-18


def same(a, b):
    return (np.array_equal(a.sim3, b.sim3) and a.chi2_initial == b.chi2_initial and a.chi2_final == b.chi2_final and
            a.lm_iterations == b.lm_iterations and a.lm_trials == b.lm_trials and np.array_equal(a.edge_chi2, b.edge_chi2))


def test_two_runs_are_bit_identical(ctx):
    opt = op.Optimizer(ctx)
    for name in ("kf40x_free", "dup_reversed"):
        P = FX.build(name)
        assert same(opt.optimize_essential_graph(P), opt.optimize_essential_graph(P)), name


def test_small_graph_after_a_large_one_equals_a_fresh_context(ctx):
    """the 200-KeyFrame call leaves larger buffers and its own matrix behind; the 5-KeyFrame call reads none of it"""
    opt = op.Optimizer(ctx)
    big, small = FX.build("kf200_free"), FX.build("free4")
    assert small.n == 5
    opt.optimize_essential_graph(big)
    after = opt.optimize_essential_graph(small)
    fresh_ctx = Context(0)
    try:
        fresh = op.Optimizer(fresh_ctx).optimize_essential_graph(small)
    finally:
        fresh_ctx.close()
    assert same(after, fresh)


def test_failed_solve_terminates_after_ten_trials(ctx):
    """lambda_init = 0 and a free vertex without an edge: H = 0, g2o's computeLambdaInit gives 0, the pivot is
    exactly 0 in every trial.  Nothing here is differentiation noise, so the counts and the bits are asserted."""
    P = FX.build_failed_solve()
    got = op.Optimizer(ctx).optimize_essential_graph(P)
    assert (got.lm_iterations, got.lm_trials) == (1, 10)
    np.testing.assert_array_equal(got.sim3, P.sim3)
    assert got.chi2_final == got.chi2_initial > 0
    ref = R.optimize(P)
    assert (ref.lm_iterations, ref.lm_trials) == (1, 10)
    assert abs(got.chi2_initial - ref.chi2_initial) <= CHI2_INITIAL_TOL * ref.chi2_initial


def test_nothing_to_optimise_returns_the_input(ctx):
    opt = op.Optimizer(ctx)
    P = FX.build("triangle")
    P.fixed[:] = 1
    got = opt.optimize_essential_graph(P)
    np.testing.assert_array_equal(got.sim3, P.sim3)
    assert (got.lm_iterations, got.lm_trials) == (0, 0) and got.chi2_final == got.chi2_initial > 0
    Q = FX.build("triangle")
    Q.e_v0, Q.e_v1, Q.e_meas = Q.e_v0[:0], Q.e_v1[:0], Q.e_meas[:0]
    got = opt.optimize_essential_graph(Q)
    np.testing.assert_array_equal(got.sim3, Q.sim3)
    assert (got.lm_iterations, got.lm_trials, got.chi2_initial, got.chi2_final) == (0, 0, 0.0, 0.0)


def raw_call(ctx, P, handle=True, with_out=True, with_chi2=True, arrays=None, **override):
    """osg_optimize_essential_graph through ctypes with fields of the problem struct overridden or whole arrays
    replaced: (return code, the output Sim3s, the output edge chi2, the result struct)."""
    Q = copy.copy(P)
    for k, v in (arrays or {}).items():
        setattr(Q, k, v)
    st = Q.struct()
    for k, v in override.items():
        setattr(st, k, v)
    res = _abi.OsgEssGraphResult()
    out, chi = np.full((max(P.n, 1), 8), -7.0), np.full(max(P.n_edges, 1), -7.0)
    res.sim3 = out.ctypes.data if with_out else None
    res.edge_chi2 = chi.ctypes.data if with_chi2 else None
    res.chi2_initial = res.chi2_final = -7.0
    res.lm_iterations = res.lm_trials = -7
    rc = ctx.lib.osg_optimize_essential_graph(ctx.handle if handle else None, ctypes.byref(st), ctypes.byref(res))
    return rc, out, chi, res


def test_rejected_arguments_write_nothing_and_leave_the_context_usable(ctx):
    opt = op.Optimizer(ctx)
    P = FX.build("free5")
    before = opt.optimize_essential_graph(P)

    def edited(a, i, v):
        b = a.copy()
        b.reshape(-1)[i] = v
        return b

    cases = {
        "e_v0 = n": raw_call(ctx, P, arrays={"e_v0": edited(P.e_v0, 2, P.n)}),
        "e_v1 = -1": raw_call(ctx, P, arrays={"e_v1": edited(P.e_v1, 0, -1)}),
        "e_v0 == e_v1": raw_call(ctx, P, arrays={"e_v0": edited(P.e_v0, 1, P.e_v1[1])}),
        "null sim3": raw_call(ctx, P, sim3=None),
        "null fixed": raw_call(ctx, P, fixed=None),
        "null e_v0": raw_call(ctx, P, e_v0=None),
        "null e_meas": raw_call(ctx, P, e_meas=None),
        "null output": raw_call(ctx, P, with_out=False),
        "lambda_init < 0": raw_call(ctx, P, lambda_init=-1e-16),
        "max_iterations < 0": raw_call(ctx, P, max_iterations=-1),
        "vertex scale 0": raw_call(ctx, P, arrays={"sim3": edited(P.sim3, 8 * 3 + 7, 0.0)}),
        "measurement scale < 0": raw_call(ctx, P, arrays={"e_meas": edited(P.e_meas, 8 * 2 + 7, -1.0)}),
        "n_vertices = -1": raw_call(ctx, P, n_vertices=-1),
        "n_vertices = 65536": raw_call(ctx, P, n_vertices=65536),
        "n_edges = -1": raw_call(ctx, P, n_edges=-1),
        "null handle": raw_call(ctx, P, handle=False),
    }
    for what, (rc, out, chi, res) in cases.items():
        assert rc < 0, what
        assert np.all(out == -7.0) and np.all(chi == -7.0), what
        assert (res.chi2_initial, res.chi2_final, res.lm_iterations, res.lm_trials) == (-7.0, -7.0, -7, -7), what
    assert cases["e_v0 = n"][0] == _abi.OSG_E_INVALID
    with pytest.raises(Exception):
        bad = copy.copy(P)
        bad.lambda_init = -1.0
        opt.optimize_essential_graph(bad)
    # edge_chi2 is optional, and the valid call gives the bits it gave before
    rc, out, chi, res = raw_call(ctx, P, with_chi2=False)
    assert rc == 0 and np.array_equal(out, before.sim3) and np.all(chi == -7.0)
    assert (res.chi2_initial, res.chi2_final) == (before.chi2_initial, before.chi2_final)
    rc, out, chi, res = raw_call(ctx, P)
    assert rc == 0 and np.array_equal(out, before.sim3) and np.array_equal(chi, before.edge_chi2)
    assert same(before, opt.optimize_essential_graph(P))
    # the point correction's checks
    X, ref = np.ones((4, 3), np.float32), np.array([0, 1, -1, P.n], np.int32)
    out = np.full((4, 3), -7.0, np.float32)
    rc = ctx.lib.osg_essgraph_correct_points(ctx.handle, 4, X.ctypes.data, ref.ctypes.data, P.n, P.sim3.ctypes.data,
                                             P.sim3.ctypes.data, out.ctypes.data)
    assert rc == _abi.OSG_E_INVALID and np.all(out == -7.0)
    rc = ctx.lib.osg_essgraph_correct_points(ctx.handle, 4, X.ctypes.data, None, P.n, P.sim3.ctypes.data,
                                             P.sim3.ctypes.data, out.ctypes.data)
    assert rc == _abi.OSG_E_INVALID and np.all(out == -7.0)
    assert same(before, opt.optimize_essential_graph(P))


def test_map_scale_graph_accepted(ctx):
    """The 1 500-KeyFrame loop-closed graph with a known optimum (no pyref run at this size): within 1e-9 of the
    ground truth, bit-identical on a second run; the device bytes and the wall time are printed."""
    P = FX.build_consistent(*FX.ACCEPTANCE)
    opt = op.Optimizer(ctx)
    opt.essential_graph_kernel_times(False)
    t0 = time.perf_counter()
    got = opt.optimize_essential_graph(P)
    wall = time.perf_counter() - t0
    _, store = opt.essential_graph_kernel_times(False)
    rot, tr, sc = truth_errors(got, P.truth)
    total = ctypes.c_int64()
    ctx.lib.osg_ctx_device_bytes(ctx.handle, ctypes.byref(total))
    print("ESSGRAPH_TRUTH", json.dumps({"graph": "c1500_free", "vertices": P.n, "edges": P.n_edges, "chi2_initial": got.chi2_initial,
                                        "chi2_final": got.chi2_final, "rot_rad": rot, "t_m": tr, "s_rel": sc,
                                        "lm_iterations": got.lm_iterations, "lm_trials": got.lm_trials, "wall_s": wall,
                                        "matrix_store_bytes": store, "context_device_bytes": total.value}))
    check_exact(P, got)
    assert store > 0
    assert rot <= 1e-9 and tr <= 1e-9 and sc <= 1e-9
    assert got.chi2_final <= 1e-18
    assert same(got, opt.optimize_essential_graph(P))


def test_map_point_correction_matches_pyref(ctx):
    """4 096 points over 40 reference vertices: the double result is cast to float once on both sides, so the
    outputs agree within 1 float ulp; a point without a reference vertex is copied bit for bit."""
    rng = np.random.default_rng(9)
    P = FX.build("kf40_free")
    after = FX.noisy(rng, P.sim3, 1.0, 0.05, 0.02)
    X = rng.normal(0, 3, (4096, 3)).astype(np.float32)
    ref = rng.integers(-1, P.n, 4096).astype(np.int32)
    assert 20 < np.count_nonzero(ref < 0) < 400 and len(np.unique(ref)) == P.n + 1
    got = op.Optimizer(ctx).correct_map_points(X, ref, P.sim3, after)
    want = R.correct_points(X, ref, P.sim3, after)
    np.testing.assert_array_equal(got[ref < 0], X[ref < 0])
    moved = ref >= 0
    assert np.abs(want[moved] - X[moved]).max() > 1e-3
    ulp = np.spacing(np.abs(want).astype(np.float32))
    print("coordinates that differ from pyref's float:", int(np.count_nonzero(got != want)), "of", got.size)
    assert np.all(np.abs(got.astype(np.float64) - want.astype(np.float64)) <= ulp)
