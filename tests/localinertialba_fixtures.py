"""The fixtures of the LocalInertialBA tests: synthetic windows generated on the CPU (a smooth body trajectory and IMU
samples as tests/inertialopt_fixtures.py makes them, preintegrated by tests/pyref_preintegration.py; points projected
with pixel noise and a share of outliers; poses, velocities and points perturbed), their reference results from
tests/pyref_localinertialba.py (computed once and shared) and the tolerances of profiles/localinertialba_margins.json
(10 x the group's replica spread, no floor).

The shapes are the smallest that can still go wrong, not workload sizes.  A name ``base@k`` is the fixture ``base``
with ``iterations = k``: a converged state hides a wrong Jacobian or lambda rule, the state after one or two
iterations does not."""
import functools
import json
import os
from dataclasses import dataclass, replace

import numpy as np

from orb_slam3_comments_ghr_amd import optimizer as O
from tests import pyref_localinertialba as R
from tests import pyref_poseinertial as pp
from tests import pyref_preintegration as PI
from tests.preintegration_fixtures import noise

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGINS = os.path.join(ROOT, "profiles", "localinertialba_margins.json")
f = np.float32
DT = 0.005                      # 200 Hz
G = float(np.float32(9.81))


@dataclass(frozen=True)
class Fixture:
    n: int                      # free KeyFrames
    seed: int
    cam: str = "pinhole_mono"
    extra_fixed: int = 0        # fixed KeyFrames beside the one before the window
    points: int = 60
    large: bool = False
    rec_init: bool = False
    corrupt: bool = False       # the newest link's preintegration pushed above the Huber delta (with rec_init)
    linkless: bool = False      # the newest free KeyFrame has no inertial link
    wide: bool = False          # point 0 is seen by every KeyFrame in view (more than 64 of them)
    noisy: bool = True
    p_obs: float = 0.8
    steps: int = 20             # IMU steps per KeyFrame interval
    iterations: int = 0         # 0: the reference's own (10, or 4 when large)

    @property
    def group(self):
        return "large" if self.large else ("rig" if self.cam == "kb8_rig" else "pinhole")


FIXTURES = {
    "n1_mono": Fixture(1, 1, points=30),
    "n2_stereo": Fixture(2, 2, cam="pinhole_stereo", extra_fixed=3),
    "n3_rig_rec": Fixture(3, 3, cam="kb8_rig", extra_fixed=3, points=50, rec_init=True),
    "n3_mono_600": Fixture(3, 4, points=600, p_obs=0.9),
    "n10_stereo": Fixture(10, 5, cam="pinhole_stereo", extra_fixed=3, points=100),
    "n10_mono_fix40": Fixture(10, 6, extra_fixed=40, points=80, linkless=True, p_obs=0.5),
    "n10_rig_corrupt": Fixture(10, 7, cam="kb8_rig", points=60, rec_init=True, corrupt=True, p_obs=0.6),
    "n25_large": Fixture(25, 8, extra_fixed=3, points=120, large=True, p_obs=0.5),
    "n3_wide": Fixture(3, 9, extra_fixed=66, points=30, wide=True, p_obs=0.15),
}
EARLY = (1, 2)
GROUPS = ("pinhole", "rig", "large")
ALL = tuple(FIXTURES) + tuple("%s@%d" % (b, k) for b in FIXTURES for k in EARLY)
SMOKE = "n3_rig_rec@2"
NOISE_FREE = {"mono": Fixture(3, 21, points=60, noisy=False), "stereo": Fixture(3, 22, cam="pinhole_stereo", noisy=False)}


def fixture(name):
    if name in NOISE_FREE:
        return NOISE_FREE[name]
    base, _, k = name.partition("@")
    fx = FIXTURES[base]
    return replace(fx, iterations=int(k)) if k else fx


def trajectory(rng, n, steps, noisy):
    """n KeyFrames, oldest first, along a smooth motion: the true states (the biases the floats the preintegrations
    carry) and the n - 1 preintegrations between them"""
    nga, walk = noise()
    bg, ba = rng.normal(0, 5e-3, 3), rng.normal(0, 2e-2, 3)
    b_int = np.concatenate([ba, bg]).astype(f)
    m = (n - 1) * steps
    t = np.arange(m + 1) * DT
    ph = rng.uniform(0, 2 * np.pi, 6)
    th = 0.3 * np.sin(2 * np.pi * 0.35 * t[:, None] + ph[:3]) + np.array([0.0, 0.0, 0.2]) * t[:, None]
    Rs = [pp.ExpSO3(w) for w in th]
    om = 2 * np.pi * np.array([0.45, 0.6, 0.5])
    A = -1.0 * np.sin(om * t[:, None] + ph[3:])
    gw = np.array([0.0, 0.0, -G])
    p, v = rng.normal(0, 0.3, 3), rng.normal(0, 0.3, 3)
    ps, vs = [p.copy()], [v.copy()]
    meas = np.zeros((m, 7))
    for k in range(m):
        meas[k, 0:3] = Rs[k].T @ (A[k] - gw) + ba
        meas[k, 3:6] = pp.LogSO3(Rs[k].T @ Rs[k + 1]) / DT + bg
        meas[k, 6] = DT
        p = p + v * DT + 0.5 * A[k] * DT * DT
        v = v + A[k] * DT
        ps.append(p.copy())
        vs.append(v.copy())
    if noisy:
        meas[:, 0:3] += rng.normal(0, 2.0e-3 * np.sqrt(200.0), (m, 3))
        meas[:, 3:6] += rng.normal(0, 1.7e-4 * np.sqrt(200.0), (m, 3))
    meas = meas.astype(f)
    pre = [PI.integrate(meas[i * steps:(i + 1) * steps], b_int, nga, walk) for i in range(n - 1)]
    idx = np.arange(n) * steps
    truth = [O.ImuState(Rs[i], ps[i], vs[i], b_int[3:].astype(float), b_int[:3].astype(float)) for i in idx]
    return truth, pre


@functools.lru_cache(maxsize=None)
def build(name):
    """The LocalInertialBAProblem of a fixture; shared, so treat it as read-only"""
    fx = fixture(name)
    rng = np.random.default_rng(7000 + fx.seed)
    truth, pre = trajectory(rng, fx.n + 1, fx.steps, fx.noisy)
    if fx.corrupt:
        q = pre[-1]
        q.dV = (q.dV + f(0.08)).astype(f)
    kw = dict(outlier_frac=0.05, pixel_noise=1.0) if fx.noisy else dict(outlier_frac=0.0, pixel_noise=0.0, vel_err=0.005)
    P = O.synth_local_inertial_window(rng, truth, pre, n_points=fx.points, cam=fx.cam, n_extra_fixed=fx.extra_fixed,
                                      large=fx.large, rec_init=fx.rec_init, linkless=fx.linkless, p_obs=fx.p_obs,
                                      wide_point=fx.wide, **kw)
    if fx.iterations:
        P.iterations = fx.iterations
    return P


@functools.lru_cache(maxsize=None)
def reference(name):
    """The restatement's result of a fixture; shared, so treat it as read-only"""
    return R.local_inertial_ba(build(name))


@functools.lru_cache(maxsize=None)
def margins():
    with open(MARGINS) as fh:
        return json.load(fh)


def tolerances(name):
    return margins()["groups"][fixture(name).group]["tol"]


def agreed(name):
    """The number of leading iterations of the fixture on which every replica took the restatement's decisions."""
    return margins()["fixtures"][name]["agreed"]


def guarded(name):
    sp = margins()["groups"][fixture(name).group]["spread"]
    return R.guarded(build(name), reference(name), sp["edge_chi2_rel"], sp["xw"])


def nudged(P, rng):
    """every input one ulp up or down (the floats as floats, the doubles as doubles)"""
    def nd(x):
        x = np.asarray(x, np.float64)
        return np.nextafter(x, np.where(rng.random(x.shape) < 0.5, -np.inf, np.inf))

    def nf(x):
        x = np.asarray(x, f)
        return np.nextafter(x, np.where(rng.random(x.shape) < 0.5, f(-np.inf), f(np.inf)).astype(f))

    kfs = []
    for K in P.kfs:
        s = K.state
        cams = [O.ImuCamera(c.cam, nd(c.Rcw), nd(c.tcw), nd(c.Rcb), nd(c.tcb), nd(c.tbc)) for c in K.cams]
        kfs.append(O.LibaKeyFrame(O.ImuState(nd(s.Rwb), nd(s.twb), nd(s.v), nd(s.bg), nd(s.ba)), cams, K.bf, K.fixed))
    links = []
    for L in P.links:
        q = L.preint
        links.append(O.LibaLink(L.prev, L.cur, O.Preintegrated(nf(q.dR), nf(q.dV), nf(q.dP), nf(q.JRg), nf(q.JVg),
                                                              nf(q.JVa), nf(q.JPg), nf(q.JPa), nf(q.b), nf(q.dT),
                                                              np.asarray(q.C, f)), L.huber, L.downweight))
    return replace(P, kfs=kfs, links=links, xw=nd(P.xw), e_obs=nd(P.e_obs), e_inv_sigma2=nf(P.e_inv_sigma2))


REPLICAS = (("reverse", dict(reverse_sums=True)), ("trig_up", dict(trig_ulp=1)), ("trig_down", dict(trig_ulp=-1)),
            ("schur", dict(block_elim=True)), ("info_alt", dict(info_alt=True)), ("polar", dict(polar=True)))


def study(name, n_nudged=2):
    """The replicas of one fixture against its restatement: the largest movement of every compared output over the
    agreed prefix, the agreed prefix itself, the iteration at which chi2 is within 1e-6 relative of its final value,
    and the rejections inside the prefix."""
    P, base = build(name), reference(name)
    runs = [R.local_inertial_ba(P, R.Variant(**kw)) for _, kw in REPLICAS]
    rng = np.random.default_rng(77 + fixture(name).seed)
    for _ in range(n_nudged):
        runs.append(R.local_inertial_ba(nudged(P, rng)))
    agreed_n = min([R.io.agreed_prefix(r.decisions, base.decisions) for r in runs] + [len(base.decisions)])
    chi = base.trace[:, 0]
    settled = int(np.argmax(np.abs(chi - chi[-1]) <= 1e-6 * abs(chi[-1]))) + 1 if len(chi) else 0
    spread = {q: 0.0 for q in R.QUANTITIES}
    final_ok = agreed_n >= len(base.decisions) and all(len(r.decisions) == len(base.decisions) for r in runs)
    for r in runs:
        d = R.differences(r, base, agreed_n)
        for q, v in d.items():
            if q.startswith("trace") or q == "chi2_initial_rel" or final_ok:
                spread[q] = max(spread[q], v)
    rejected_in_prefix = sum(1 for dec in base.decisions[:agreed_n] for a in dec if not a)
    return {"group": fixture(name).group, "spread": spread, "agreed": agreed_n, "settled": settled,
            "iterations": len(base.decisions), "final_ok": bool(final_ok), "rejected_in_prefix": rejected_in_prefix,
            "failed": bool(base.failed)}


def compare(name, got):
    """The mismatches of a product result against the restatement under the recorded tolerances."""
    P, ref = build(name), reference(name)
    k, tol = agreed(name), tolerances(name)
    bad = []
    if R.io.trace_decisions(got.trace[:k]) != R.io.trace_decisions(ref.trace[:k]):
        bad.append("decisions %r != %r" % (R.io.trace_decisions(got.trace[:k]), R.io.trace_decisions(ref.trace[:k])))
    d = R.differences(got, ref, k)
    # an admitted fixture's replicas agree to the end (the margins tool refuses any other), so every output counts
    if not margins()["fixtures"][name]["final_ok"]:
        bad.append("the recorded margins do not cover the final state")
    for q in tol:
        if not d[q] <= tol[q]:
            bad.append("%s: %.3e > %.3e" % (q, d[q], tol[q]))
    g = guarded(name)
    if np.any((np.asarray(got.edge_bad, bool) != np.asarray(ref.edge_bad, bool)) & ~g):
        bad.append("edge_bad differs outside the guarded edges")
    if bool(got.failed) != bool(ref.failed):
        bad.append("failed")
    return bad
