"""GPU: osg_local_inertial_ba[_batch] (csrc/localinertialba.hip) against the numpy restatement
(tests/pyref_localinertialba.py) on the fixtures of tests/localinertialba_fixtures.py: the accept / reject decisions,
lambda and chi2 of the trace over the prefix on which every replica of the restatement agrees; the final KeyFrame
states, points, chi2_initial, chi2_last and edge_chi2 within 10 x the fixture group's recorded replica spread
(profiles/localinertialba_margins.json, no floor); edge_bad identical outside the guarded edges; `failed` identical;
reruns and batches bit-identical.

The entry point defines no canonical order of the KeyFrames and points (its sums run in the caller's insertion
order), so a permuted window is not bit-equal to the ordered one and is not compared.

Measured on an MI355X: see DESIGN.md 3.29."""
from dataclasses import replace

import numpy as np
import pytest

from orb_slam3_comments_ghr_amd import Context, _abi, imu
from orb_slam3_comments_ghr_amd import optimizer as O
from tests import localinertialba_fixtures as FX
from tests import poseinertial_fixtures as PFX2
from tests import preintegration_fixtures as PFX
from tests import pyref_localinertialba as R
from tests import pyref_poseinertial as pp
from tests import pyref_preintegration as PI

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def opt(ctx):
    return O.Optimizer(ctx)


def bits(r):
    return (tuple(a.tobytes() for s in r.states for a in (s.Rwb, s.twb, s.v, s.bg, s.ba)), r.Rcw.tobytes(),
            r.tcw.tobytes(), r.xw.tobytes(), r.edge_bad.tobytes(), r.edge_chi2.tobytes(),
            np.array([r.chi2_initial, r.chi2_last, r.chi2_accepted]).tobytes(), r.iterations, r.trials_rejected,
            r.solve_failed, r.failed, r.trace.tobytes())


@pytest.mark.parametrize("name", list(FX.ALL))
def test_fixture_matches_the_restatement(opt, name):
    P = FX.build(name)
    got = opt.LocalInertialBA(P)
    ref = FX.reference(name)
    print(name, "iterations %d (ref %d) rejected %d (ref %d) prefix %d" % (
        got.iterations, ref.iterations, got.trials_rejected, ref.trials_rejected, FX.agreed(name)))
    print(name, {q: "%.3g (tol %.3g)" % (v, FX.tolerances(name)[q]) for q, v in R.differences(got, ref, FX.agreed(name)).items()})
    assert not got.solve_failed and not ref.solve_failed
    assert FX.compare(name, got) == []
    assert bits(opt.LocalInertialBA(P)) == bits(got)   # the reduction order is fixed


def test_mixed_batch_equals_the_single_calls(opt):
    probs = [FX.build(n) for n in FX.ALL]
    batch = opt.LocalInertialBA(probs)
    for n, P, b in zip(FX.ALL, probs, batch):
        assert bits(b) == bits(opt.LocalInertialBA(P)), n


def test_batch_of_100_equals_the_single_calls(opt):
    names = ("n1_mono", "n2_stereo", "n3_rig_rec", "n10_stereo@2", "n3_wide@1")
    single = {n: bits(opt.LocalInertialBA(FX.build(n))) for n in names}
    order = np.random.default_rng(3).integers(0, len(names), 100)
    batch = opt.LocalInertialBA([FX.build(names[i]) for i in order])
    assert len(batch) == 100
    for i, b in zip(order, batch):
        assert bits(b) == single[names[i]], names[i]


def test_fixed_and_linkless_keyframes_keep_their_bits(opt):
    P = FX.build("n10_mono_fix40")
    got = opt.LocalInertialBA(P)
    moved = 0
    for K, s in zip(P.kfs, got.states):
        a = K.state
        same = all(x.tobytes() == y.tobytes() for x, y in ((a.Rwb, s.Rwb), (a.twb, s.twb), (a.v, s.v), (a.bg, s.bg), (a.ba, s.ba)))
        if K.fixed:
            assert same
        else:
            moved += not same
    assert moved == 10
    for k, K in enumerate(P.kfs):   # a fixed KeyFrame's camera pose is the one passed in
        if K.fixed:
            assert got.Rcw[k].tobytes() == np.asarray(K.cams[0].Rcw, np.float64).tobytes()
            assert got.tcw[k].tobytes() == np.asarray(K.cams[0].tcw, np.float64).tobytes()
    # KeyFrame 0 has visual edges and no link: its pose is optimised, its v, bg, ba are no active vertices
    a, s = P.kfs[0].state, got.states[0]
    assert s.v.tobytes() == a.v.tobytes() and s.bg.tobytes() == a.bg.tobytes() and s.ba.tobytes() == a.ba.tobytes()
    assert not np.array_equal(s.Rwb, a.Rwb) and not np.array_equal(s.twb, a.twb)
    # a linked one's do move
    assert not np.array_equal(got.states[1].v, P.kfs[1].state.v) and not np.array_equal(got.states[1].bg, P.kfs[1].state.bg)


def test_special_points_and_an_edgeless_keyframe(opt):
    """a point seen once and one seen only by fixed KeyFrames still move; a KeyFrame without any visual edge is
    held by its links alone"""
    P = FX.build("n3_rig_rec")
    got = opt.LocalInertialBA(P)
    deg = np.bincount(P.e_point, minlength=P.n_points)
    once = int(np.flatnonzero(deg == 1)[0])
    assert not np.array_equal(got.xw[once], P.xw[once])
    fixed = np.array([k.fixed for k in P.kfs])
    only_fixed = [p for p in range(P.n_points) if deg[p] > 1 and fixed[P.e_kf[P.e_point == p]].all()]
    assert only_fixed and not np.array_equal(got.xw[only_fixed[0]], P.xw[only_fixed[0]])
    keep = P.e_kf != 1
    Q = replace(P, e_point=P.e_point[keep], e_kf=P.e_kf[keep], e_kind=P.e_kind[keep], e_obs=P.e_obs[keep],
                e_inv_sigma2=P.e_inv_sigma2[keep])
    got, ref = opt.LocalInertialBA(Q), R.local_inertial_ba(Q)
    assert R.io.trace_decisions(got.trace) == R.io.trace_decisions(ref.trace)
    d, tol = R.differences(got, ref), FX.tolerances("n3_rig_rec")
    assert all(d[q] <= tol[q] for q in ("rot_rad", "twb", "v", "bg", "ba", "chi2_initial_rel")), d
    assert not np.array_equal(got.states[1].twb, Q.kfs[1].state.twb)


def test_invalid_problem_leaves_the_context_usable(opt):
    P = FX.build("n2_stereo")
    bad = replace(P, e_kf=np.where(np.arange(P.n_edges) == 5, 99, P.e_kf))
    with pytest.raises(Exception):
        opt.LocalInertialBA(bad)
    with pytest.raises(Exception):
        opt.LocalInertialBA([P, bad])
    assert bits(opt.LocalInertialBA(P)) == bits(opt.LocalInertialBA(P))


def _meas(q):
    return np.array([np.concatenate([a, w, [dt]]) for a, w, dt in q.mvMeasurements], np.float32)


def test_chain_preintegrate_local_ba_reintegrate_pose(ctx, opt):
    """osg_imu_preintegrate_batch results fed unconverted into LocalInertialBA, its biases into reintegrate, then
    PoseInertialOptimizationLastKeyFrame of the newest KeyFrame against the window's result: every link against
    the restatement of that link on the same inputs."""
    name = "n10_stereo"
    P = FX.build(name)
    nga, walk = PFX.noise()
    ptol = PFX.margins()["groups"]["keyframe"]["tol"]
    lists = [_meas(l.preint) for l in P.links]
    # link 1: the preintegrations
    states = imu.preintegrate_batch(ctx, [imu.ImuProblem(m, np.asarray(l.preint.b, np.float32), nga, walk)
                                          for m, l in zip(lists, P.links)])
    for s, l in zip(states, P.links):
        d = PI.differences(s, l.preint)
        assert not PI.exact_mismatches(s, l.preint) and all(d[k] <= ptol[k] for k in ptol), d
    # link 2: the window on them
    P1 = replace(P, links=[replace(l, preint=s) for l, s in zip(P.links, states)])
    got, ref = opt.LocalInertialBA(P1), R.local_inertial_ba(P1)
    k, tol = FX.agreed(name), FX.tolerances(name)
    assert R.io.trace_decisions(got.trace[:k]) == R.io.trace_decisions(ref.trace[:k])
    d = R.differences(got, ref, k)
    assert all(d[q] <= tol[q] for q in tol), d
    assert not got.failed
    # link 3: Reintegrate() of every link with its previous KeyFrame's new bias, one launch
    bs = [np.concatenate([got.states[l.prev].ba, got.states[l.prev].bg]).astype(np.float32) for l in P.links]
    states2 = imu.reintegrate(ctx, states, bs)
    for s, m, b in zip(states2, lists, bs):
        q = PI.integrate(m, b, nga, walk)
        d = PI.differences(s, q)
        assert not PI.exact_mismatches(s, q) and all(d[k] <= ptol[k] for k in ptol), d
    # link 4: the pose step of the newest KeyFrame against the previous one, over its own observations
    e = np.flatnonzero(P.e_kf == 0)
    K = P.kfs[0]
    cams = [O.ImuCamera(c.cam, got.Rcw[0] if i == 0 else c.Rcw, got.tcw[0] if i == 0 else c.tcw, c.Rcb, c.tcb, c.tbc)
            for i, c in enumerate(K.cams)]
    Q = O.PoseInertialProblem(_abi.OSG_PIO_LAST_KEYFRAME, got.states[0], got.states[1], cams, K.bf, P.e_kind[e],
                              got.xw[P.e_point[e]], P.e_obs[e], P.e_inv_sigma2[e], P.track_depth[P.e_point[e]],
                              states2[0], np.asarray(states2[0].C, np.float32))
    gq, rq = opt.PoseInertialOptimizationLastKeyFrame(Q), pp.pose_inertial_optimization(Q)
    dq, tq = pp.differences(gq, rq), PFX2.tolerances("lkf_stereo_n255")
    assert pp.same_discrete(gq, rq) and all(dq[q] <= tq[q] for q in tq), dq
