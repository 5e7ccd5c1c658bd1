"""GPU: osg_imu_preintegrate[_batch] (csrc/preintegrate.hip) against the numpy restatement
(tests/pyref_preintegration.py) on the fixtures of tests/preintegration_fixtures.py.  dR, dV, dP, avgA, avgW, the
Jacobians and C[0:9, 0:9] within 10 x the fixture group's recorded replica spread
(profiles/preintegration_margins.json, no floor); dT, b, C[9:15, 9:15] and C's zero blocks bit-equal; continuation,
reintegration, merging, batches and reruns bit-identical to the single fresh call.

Measured on an MI355X (largest over each group, beside the tolerance): DESIGN.md 3.27."""
import ctypes as C

import numpy as np
import pytest

from orb_slam3_comments_ghr_amd import Context, _abi, imu
from orb_slam3_comments_ghr_amd import optimizer as O
from tests import poseinertial_fixtures as PFX
from tests import preintegration_fixtures as FX
from tests import pyref_poseinertial as RP
from tests import pyref_preintegration as R

pytestmark = pytest.mark.gpu
W = imu.WAVES_PER_WORKGROUP
FIELDS = ("dR", "dV", "dP", "JRg", "JVg", "JVa", "JPg", "JPa", "b", "dT", "C", "avgA", "avgW")


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def bits(s):
    return tuple(np.asarray(getattr(s, k), np.float32).tobytes() for k in FIELDS)


def fresh(ctx, name, **kw):
    P = FX.build(name)
    return imu.preintegrate(ctx, kw.pop("meas", P.meas), kw.pop("bias", P.bias), P.nga, P.nga_walk, **kw)


def problem(name, lo=0, hi=None, init=None):
    P = FX.build(name)
    return imu.ImuProblem(P.meas[lo:hi], P.bias, P.nga, P.nga_walk, init)


@pytest.mark.parametrize("name", list(FX.FIXTURES))
def test_fixture_matches_the_restatement(ctx, name):
    got, ref = fresh(ctx, name), FX.reference(name)
    d, tol = R.differences(got, ref), FX.tolerances(name)
    print(name, {q: "%.3g (tol %.3g)" % (d[q], tol[q]) for q in R.QUANTITIES})
    assert not R.exact_mismatches(got, ref), (name, R.exact_mismatches(got, ref))
    over = {q: (d[q], tol[q]) for q in R.QUANTITIES if d[q] > tol[q]}
    assert not over, (name, over)
    assert bits(fresh(ctx, name)) == bits(got)   # two runs are bit-identical


@pytest.mark.parametrize("name", ["n3", "n65", "both100"])
def test_continuation_through_init_is_exact(ctx, name):
    n = FX.FIXTURES[name].n
    whole = bits(fresh(ctx, name))
    for k in sorted({0, 1, n // 2, n - 1, n}):
        head = imu.preintegrate_batch(ctx, [problem(name, 0, k)])[0]
        tail = imu.preintegrate(ctx, FX.build(name).meas[k:], init=head)
        assert bits(tail) == whole, (name, k)
        assert len(tail.meas) == n


def test_reintegrate_equals_a_fresh_integration_at_bu(ctx):
    names = ["n10", "n65", "biaslarge100"]
    states = [fresh(ctx, k) for k in names]
    rng = np.random.default_rng(5)
    bus = [s.b + rng.normal(0, 0.01, 6).astype(np.float32) for s in states]
    for s, bu in zip(states, bus):
        s.set_new_bias(bu)
    again = imu.reintegrate(ctx, states)
    other = imu.reintegrate(ctx, [fresh(ctx, k) for k in names], bus)
    for k, bu, a, o in zip(names, bus, again, other):
        want = bits(fresh(ctx, k, bias=bu))
        assert bits(a) == want and bits(o) == want, k
        assert a.b.tobytes() == bu.tobytes()


def test_merge_previous_equals_the_concatenation(ctx):
    prev, cur = fresh(ctx, "n63"), fresh(ctx, "n10")
    cur.set_new_bias(cur.b + np.float32(0.003))
    merged = imu.merge_previous(ctx, prev, cur)
    both = np.concatenate([FX.build("n63").meas, FX.build("n10").meas])
    assert bits(merged) == bits(fresh(ctx, "n10", meas=both, bias=cur.bu))
    assert len(merged.meas) == 73 and float(merged.dT) > float(prev.dT)
    assert imu.merge_previous(ctx, cur, cur) is cur


@pytest.mark.parametrize("B", [1, W - 1, W, W + 1])
def test_batch_equals_the_single_calls(ctx, B):
    names = (list(FX.FIXTURES) * 2)[3:3 + B]
    batch = imu.preintegrate_batch(ctx, [problem(k) for k in names])
    assert len(batch) == B
    for k, b in zip(names, batch):
        assert bits(b) == bits(fresh(ctx, k)), k


def test_batch_of_256_workgroups_and_one(ctx):
    """256 W + 1 lists of n = 3: the n3 fixture at five biases, so that a result in the wrong place shows"""
    P = FX.build("n3")
    biases = [P.bias + np.float32(0.001 * k) for k in range(5)]
    singles = [bits(fresh(ctx, "n3", bias=b)) for b in biases]
    assert len(set(singles)) == 5
    order = [(5 * i + i // 7) % 5 for i in range(256 * W + 1)]
    batch = imu.preintegrate_batch(ctx, [imu.ImuProblem(P.meas, biases[k], P.nga, P.nga_walk) for k in order])
    assert len(batch) == 256 * W + 1
    for i, (k, b) in enumerate(zip(order, batch)):
        assert bits(b) == singles[k], (i, k)


def test_ragged_batch_with_empty_lists_first_and_last(ctx):
    names = ["n0", "n65", "n1", "n600", "n0", "n10", "n200", "n64", "n0"]
    batch = imu.preintegrate_batch(ctx, [problem(k) for k in names])
    for k, b in zip(names, batch):
        assert bits(b) == bits(fresh(ctx, k)), k
    assert np.array_equal(batch[0].dR, np.eye(3)) and not batch[0].C.any() and float(batch[0].dT) == 0.0
    assert batch[0].b.tobytes() == FX.build("n0").bias.tobytes()


def test_two_problems_share_one_list(ctx):
    """Tracking::PreintegrateIMU: one list onto the state continued from the last KeyFrame and onto a fresh one"""
    P = FX.build("n10")
    from_kf = fresh(ctx, "n65")
    other_bias = P.bias + np.float32(0.002)
    a, b = imu.preintegrate_batch(ctx, [imu.ImuProblem(P.meas, init=from_kf),
                                        imu.ImuProblem(P.meas, other_bias, P.nga, P.nga_walk)])
    assert bits(a) == bits(imu.preintegrate(ctx, P.meas, init=from_kf))
    assert bits(b) == bits(fresh(ctx, "n10", bias=other_bias))
    assert bits(a) != bits(b)
    # a shorter problem on the same list reads its prefix
    c, d = imu.preintegrate_batch(ctx, [problem("n10"), problem("n10", 0, 4)])
    assert bits(c) == bits(fresh(ctx, "n10")) and bits(d) == bits(fresh(ctx, "n10", meas=P.meas[:4]))


# ----------------------------------------------------------------------------------- argument checks, live context
SENTINEL = 0xA5


@pytest.mark.parametrize("what", ["n_neg", "n_big", "meas_null", "dt_zero", "dt_neg", "dt_nan", "dt_inf", "second"])
def test_rejected_arguments_write_nothing_and_the_context_stays_usable(ctx, what):
    P = FX.build("n10")
    meas = np.array(P.meas)
    keep = []
    ps = (_abi.OsgImuProblem * 2)(imu.ImuProblem(meas, P.bias, P.nga, P.nga_walk).struct(keep),
                                  imu.ImuProblem(meas, P.bias, P.nga, P.nga_walk).struct(keep))
    out = (_abi.OsgImuPreintegrated * 2)()
    C.memset(out, SENTINEL, C.sizeof(out))
    bad = ps[1] if what == "second" else ps[0]
    if what in ("n_neg", "second"):
        bad.n = -1
    elif what == "n_big":
        bad.n = _abi.OSG_IMU_MAX_STEPS + 1
    elif what == "meas_null":
        bad.meas = None
    else:
        meas[7, 6] = {"dt_zero": 0.0, "dt_neg": -0.005, "dt_nan": np.nan, "dt_inf": np.inf}[what]
    assert ctx.lib.osg_imu_preintegrate_batch(ctx.handle, ps, 2, out) == -1
    assert bytes(out) == bytes([SENTINEL]) * C.sizeof(out)
    assert ctx.lib.osg_imu_preintegrate_batch(ctx.handle, None, 1, out) == -1
    assert ctx.lib.osg_imu_preintegrate_batch(ctx.handle, ps, -1, out) == -1
    assert bytes(out) == bytes([SENTINEL]) * C.sizeof(out)
    got, ref = fresh(ctx, "n10"), FX.reference("n10")
    assert not R.exact_mismatches(got, ref)
    d, tol = R.differences(got, ref), FX.tolerances("n10")
    assert all(d[q] <= tol[q] for q in R.QUANTITIES)


def test_pose_inertial_bits_are_unchanged_by_a_preintegration_on_the_same_context(ctx):
    from tests.test_poseinertial_gpu import bits as pio_bits

    opt = O.Optimizer(ctx)
    P = PFX.build("lkf_n65")
    before = pio_bits(opt.PoseInertialOptimizationLastKeyFrame(P))
    imu.preintegrate_batch(ctx, [problem("n600"), problem("n10")])
    after = pio_bits(opt.PoseInertialOptimizationLastKeyFrame(PFX.build("lkf_n65")))
    assert before == after


def test_tracking_chain_from_imu_samples_to_the_pose_step(ctx):
    """select -> integrables -> preintegrate -> to_pio() -> PoseInertialOptimizationLastFrame, on the kernel's own
    preintegration, against the restatement of the pose step on that same preintegration, under the tolerances of
    the pose step's group (the chain rule of DESIGN.md 3.25); the preintegration itself against its restatement
    under the frame group's."""
    P, aq, wq, tq, t_prev, t_cur = FX.chain_inputs()
    taken, popped = imu.select_imu(tq, t_prev, t_cur)
    assert (list(taken), popped) == R.select(tq, t_prev, t_cur) and len(taken) == 11
    meas = imu.integrables_from_imu(aq[taken], wq[taken], tq[taken], t_prev, t_cur)
    assert meas.tobytes() == R.integrables(aq[taken], wq[taken], tq[taken], t_prev, t_cur).tobytes()
    nga, walk = FX.noise()
    bias = np.concatenate([P.prev.ba, P.prev.bg]).astype(np.float32)
    state = imu.preintegrate(ctx, meas, bias, nga, walk)
    ref_state = R.integrate(meas, bias, nga, walk)
    assert R.cut_margin(ref_state.ds) > FX.CUT_GUARD
    assert not R.exact_mismatches(state, ref_state)
    d, tol = R.differences(state, ref_state), FX.margins()["groups"]["frame"]["tol"]
    assert all(d[q] <= tol[q] for q in R.QUANTITIES), d
    Q = FX.chain_problem(P, state)
    assert Q.preint.C.tobytes() == state.to_pio().C.tobytes() and Q.preint.dR.tobytes() == state.to_pio().dR.tobytes()
    Q.preint = state.to_pio()
    got, ref = O.Optimizer(ctx).PoseInertialOptimizationLastFrame(Q), RP.pose_inertial_optimization(Q)
    name = FX.CHAIN_GROUP_FIXTURE
    g = PFX.margins()["groups"][PFX.FIXTURES[name].group]["max"]
    assert np.min(np.abs(np.array(ref.ratios) - 1.0)) > 10.0 * g["ratio"], "not a guarded problem: pick another seed"
    assert np.min(np.abs(ref.info_eigs / 1e-12 - 1.0)) > 10.0 * g["info_eig_rel"]
    assert np.min(np.abs(ref.marg_sv / 1e-6 - 1.0)) > 10.0 * g["marg_sv_rel"]
    assert RP.same_discrete(got, ref), (got.n_inliers, ref.n_inliers)
    dd, ptol = RP.differences(got, ref), PFX.tolerances(name)
    print("chain", {q: "%.3g (tol %.3g)" % (dd[q], ptol[q]) for q in RP.QUANTITIES})
    over = {q: (dd[q], ptol[q]) for q in RP.QUANTITIES if dd[q] > ptol[q]}
    assert not over, over
