"""The MLPnPsolver fixtures shared by tests/test_mlpnp.py, tests/test_mlpnp_gpu.py, tests/test_adapter_mlpnp.py and
tools/mlpnp_margins.py, and the guard that makes an exact comparison of discrete outcomes meaningful.

A hypothesis classifies every match by ``err < bound`` in float.  An implementation that differs from the
reference in the last bits of computePose (a Jacobi eigen-solve instead of JacobiSVD, another null-space
basis, another summation order) moves ``err / bound`` by a relative amount that tools/mlpnp_margins.py
measures on replicas of each fixture: bearings and points nudged by one float ulp, the null-space bases rotated
by an arbitrary angle, eigh instead of svd for the 12 x 12, the planar eigenvectors and the solution vector
negated.  With g = 10 x the largest such movement in the fixture's group, a match is *borderline* for a
hypothesis when ``err / bound`` lies within g of 1.  The deciding quantities inside computePose (third pivot
against the rank threshold, the sign choice's error difference, max|dx| against 5, min|dx| against 1,
max|J dx| against 1e-5) have a margin m = 10 x their largest movement, measured the same way.  max|J dx| is
not free of the null-space basis (it lies between max rho / sqrt 2 and max rho, rho the basis-free norm of a
point's residual pair), and the reference's basis is Eigen's: both bounds must lie on the same side of 1e-5.

A hypothesis is *ill-conditioned* when the two smallest eigenvalues of AtA differ by less than 1e-3 relative
(its pose, info and count are not compared), and *unstable* when a discrete decision of computePose differs
between pyref and a replica or a deciding quantity lies within m of its threshold (its info is not compared;
one Gauss-Newton step more or less moves its pose like any other replica does, so its count is compared within
the borderline like everyone's).  A fixture is valid when, for tests/pyref_mlpnp.py and each replica:

  1. the returned hypothesis is neither ill-conditioned nor unstable and has no borderline match;
  2. every hypothesis before it (every hypothesis, when nothing converges) has count + borderline <=
     min_inliers; when nothing converges the winner's count - borderline exceeds count + borderline of every
     other hypothesis (exact copies of the winner's sample set exempt);
  3. every discrete decision of every hypothesis that is neither is the same;
  4. every ill-conditioned hypothesis has count <= min_inliers / 2, so it cannot touch the outcome;
  5. at most 20 % of the hypotheses are borderline, ill-conditioned or unstable.

A seed that fails is replaced here, never excluded in a test."""
from dataclasses import dataclass, replace
import functools
import json
import os

import numpy as np

from orb_slam3_comments_ghr_amd import mlpnpsolver as M
from orb_slam3_comments_ghr_amd import optimizer as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGINS = os.path.join(ROOT, "profiles", "mlpnp_margins.json")
EIG_GAP = 1e-3
MAX_FLAGGED_HYP = 0.20
STAGED_MAX = 6272  # matches that fit the LDS staging of csrc/mlpnp.hip: (160 KiB - the waves' tiles) / 24 B


@dataclass(frozen=True)
class Fixture:
    n: int
    min_inliers: int
    seed: int
    outlier_frac: float = 0.3
    n_hyp: int = 35
    noise_px: float = 0.5
    planar: bool = False
    kb8: bool = False
    behind_frac: float = 0.0
    special: str = ""   # "tie": the best sample set copied into a later slot; "pinhole_b": another pinhole camera
    group: str = "small"


LOW_NOISE = 0.02

FIXTURES = {
    "n0": Fixture(0, 10, 1),                                         # nothing launched
    "n5_min6": Fixture(5, 6, 2),                                     # n < min_inliers: immediate no-more
    "n6_min6": Fixture(6, 6, 3, outlier_frac=0.0, n_hyp=1),          # all six are the sample; count == min: best
    "n7": Fixture(7, 6, 4, outlier_frac=0.0, n_hyp=5),
    "n15": Fixture(15, 10, 5, outlier_frac=0.1),                     # Tracking's floor
    "n64": Fixture(64, 32, 64, group="word_edges"),                  # mask-word edge
    "n65": Fixture(65, 32, 66, group="word_edges"),
    "n200": Fixture(200, 100, 200, group="n200"),                    # Tracking's usual: H = 35
    "n200_b": Fixture(200, 100, 200, special="pinhole_b", group="n200"),  # the same matches, another camera
    "n60_h1": Fixture(60, 30, 61, n_hyp=1),
    # 90 % outliers, min_inliers set to the largest count: no convergence; the best is the first to attain the maximum, and an
    # exact copy of its sample set in a later slot must not replace it
    "n100_h300": Fixture(100, 10, 109, outlier_frac=0.9, n_hyp=300, special="tie", group="h300"),
    "n40_all_out": Fixture(40, 20, 41, outlier_frac=1.0, n_hyp=20),  # bNoMore and failure
    "n80_planar": Fixture(80, 40, 81, planar=True, group="planar"),  # world z == 0 exactly
    "n80_kb8": Fixture(80, 40, 82, kb8=True, group="kb8"),           # rays out to ~70 degrees
    "n40_break": Fixture(40, 15, 43, outlier_frac=0.5, n_hyp=20),    # a hypothesis whose Gauss-Newton breaks
    "n80_behind": Fixture(80, 40, 84, behind_frac=0.25, group="behind"),  # no depth test
    # past the LDS staging limit: the global-memory path.  At thousands of matches some always lie near a
    # bound unless the true matches sit far inside it: low noise
    "n6400": Fixture(6400, 3000, 6400, n_hyp=6, noise_px=LOW_NOISE, group="large"),
}
GROUPS = sorted({f.group for f in FIXTURES.values()})
BATCH = ["n200", "n0", "n80_kb8", "n5_min6", "n65", "n80_planar", "n6_min6", "n40_all_out", "n6400", "n100_h300", "n7"]
CAMERA_PAIR = ("n200", "n200_b")
SMOKE = "n65"
PINHOLE_B = (380.0, 395.0, 330.0, 250.0)
# (nudge by one ulp, pyref switches)
REPLICAS = [(True, {}), (True, {"eigh": True}), (False, {"basis_angle": 0.7}),
            (True, {"basis_angle": 2.1, "eigh": True}), (False, {"flip_solution": True}),
            (False, {"flip_planar": True, "flip_solution": True})]


@functools.lru_cache(maxsize=None)
def build(name):
    from tests import pyref_mlpnp as R
    f = FIXTURES[name]
    rng = np.random.default_rng(f.seed)
    P = M.synth_mlpnp_problem(rng, f.n, f.outlier_frac, f.min_inliers, f.n_hyp, noise_px=f.noise_px, planar=f.planar,
                              kb8=f.kb8, behind_frac=f.behind_frac)
    if f.special == "pinhole_b":
        P.cam = O.pinhole_camera(*PINHOLE_B)
    if f.special == "tie":
        # slot 40 samples six true matches; min_inliers becomes the largest count, so that hypothesis is recorded
        # as the best and does not return (count == min); a copy of its set sits in a later slot
        P.samples[40] = np.flatnonzero(~P.truth[2])[:6]
        c = R.evaluate(P).counts
        first = int(np.argmax(c))
        P.min_inliers = int(c[first])
        later = first + (f.n_hyp - first) // 2
        assert later > first and P.min_inliers >= 6
        P.samples[later] = P.samples[first]
    return P


@functools.lru_cache(maxsize=None)
def replicas(name):
    """The replicas of a fixture as (problem, pyref switches), from the fixture's own seeded stream."""
    from tests import pyref_mlpnp as R
    rng = np.random.default_rng(FIXTURES[name].seed + 77777)
    return [(R.nudged(build(name), rng) if nudge else build(name), kw) for nudge, kw in REPLICAS]


@functools.lru_cache(maxsize=None)
def evaluations(name):
    """[pyref, replica 0, ...] evaluations (None for a fixture that never iterates)."""
    from tests import pyref_mlpnp as R
    P = build(name)
    if P.n == 0 or P.n < P.min_inliers:
        return None
    return [R.evaluate(P)] + [R.evaluate(Q, **kw) for Q, kw in replicas(name)]


@functools.lru_cache(maxsize=None)
def outcome(name):
    from tests import pyref_mlpnp as R
    ev = evaluations(name)
    return R.solve(build(name), ev[0] if ev else None)


def rot_angle(Ra, Rb):
    """|log(Ra Rb^T)|"""
    D = np.asarray(Ra, np.float64) @ np.asarray(Rb, np.float64).T
    skew = np.array([D[2, 1] - D[1, 2], D[0, 2] - D[2, 0], D[1, 0] - D[0, 1]])
    return float(np.arctan2(0.5 * np.linalg.norm(skew), 0.5 * (np.trace(D) - 1.0)))


def ill_conditioned(name):
    """Per hypothesis: the eigenvalue gap is below EIG_GAP in pyref or a replica."""
    ev = evaluations(name)
    return np.array([any(E.info[h].eig_gap < EIG_GAP for E in ev) for h in range(len(ev[0].counts))])


def decisions_differ(name):
    ev = evaluations(name)
    return np.array([any(E.info[h].decisions() != ev[0].info[h].decisions() for E in ev[1:])
                     for h in range(len(ev[0].counts))])


def spreads(name):
    """Over the replicas: the largest relative movement of err / bound (matches within +-50 % of the bound), of
    R and t, and of the deciding quantities, over the hypotheses that are well-conditioned and take the same
    decisions everywhere."""
    from tests import pyref_mlpnp as R
    ev = evaluations(name)
    out = {"ratio_rel": 0.0, "rot_rad": 0.0, "t_rel": 0.0, "quant_rel": 0.0}
    if ev is None:
        return out
    base = ev[0]
    keep = ~ill_conditioned(name)
    same = ~decisions_differ(name)
    for e in ev[1:]:
        for h in np.flatnonzero(keep):
            rb, rr = base.ratio[h], e.ratio[h]
            near = (rb > 0.5) & (rb < 1.5)
            if near.any():
                out["ratio_rel"] = max(out["ratio_rel"], float(np.max(np.abs(rr[near] - rb[near]) / rb[near])))
            if np.all(np.isfinite(base.t[h])) and np.all(np.isfinite(e.t[h])):
                out["rot_rad"] = max(out["rot_rad"], rot_angle(base.R[h], e.R[h]))
                out["t_rel"] = max(out["t_rel"], float(np.linalg.norm(base.t[h] - e.t[h]) / np.linalg.norm(base.t[h])))
            for (a, thr), (b, _) in zip(e.info[h].quant, base.info[h].quant) if same[h] else ():
                out["quant_rel"] = max(out["quant_rel"], R.rel_move(a, b, thr))
    return out


@functools.lru_cache(maxsize=None)
def margins():
    with open(MARGINS) as f:
        return json.load(f)


def tolerances(name):
    """g, m and the R, t tolerances of the fixture's group: 10 x the recorded spreads."""
    grp = margins()["groups"][FIXTURES[name].group]
    return {"g": grp["g"], "m": grp["m"], "rot_rad": grp["rot_tol"], "t_rel": grp["t_tol"]}


def borderline(E, g):
    """Per hypothesis, the number of matches with err / bound within g of 1."""
    with np.errstate(invalid="ignore"):
        return (np.abs(E.ratio - 1) < g).sum(1)


def unstable(name, m):
    """Per hypothesis: a decision differs in a replica or a deciding quantity lies within m of its threshold."""
    ev = evaluations(name)
    near = np.array([any(E.info[h].margin <= m for E in ev) for h in range(len(ev[0].counts))])
    return decisions_differ(name) | near


def excluded(name, m):
    return ill_conditioned(name) | unstable(name, m)


def guard(name, g, m):
    """-> list of violated conditions (empty: the fixture is valid at margins g, m)."""
    from tests import pyref_mlpnp as R
    ev = evaluations(name)
    if ev is None:
        return []
    P = build(name)
    base = outcome(name)
    ex, un = ill_conditioned(name), unstable(name, m)
    bad = []
    flagged = ex | un
    for k, E in enumerate(ev):
        Q = P if k == 0 else replicas(name)[k - 1][0]
        o = R.solve(Q, E)
        if (o.converged, o.hyp, o.n_iterations, o.n_inliers, o.n_best) != (
                base.converged, base.hyp, base.n_iterations, base.n_inliers, base.n_best) or not np.array_equal(o.inlier, base.inlier):
            bad.append((k, "outcome"))
        bl = borderline(E, g)
        c = E.counts
        flagged |= bl > 0
        if o.hyp >= 0 and (bl[o.hyp] or ex[o.hyp] or un[o.hyp]):
            bad.append((k, 1))
        others = np.arange(len(c)) < o.hyp if o.converged else np.ones(len(c), bool)
        if o.hyp >= 0:
            others[o.hyp] = False
        if np.any((c + bl)[others & ~ex] > P.min_inliers):
            bad.append((k, 2))
        if not o.converged and o.hyp >= 0:
            same = np.all(P.samples == P.samples[o.hyp], 1)
            if np.any((c + bl)[others & ~same & ~ex] >= c[o.hyp] - bl[o.hyp]):
                bad.append((k, 2))
        if not o.converged and o.hyp < 0 and np.any((c + bl)[~ex] >= P.min_inliers):
            bad.append((k, 2))
        if np.any(c[ex] > P.min_inliers / 2):
            bad.append((k, 4))
    if np.count_nonzero(flagged) > MAX_FLAGGED_HYP * len(ex):
        bad.append(("all", 5))
    return bad


def compare(name, got, tol=None):
    """The checks of tests/test_mlpnp_gpu.py on one MlpnpResult -> list of mismatches."""
    P, o, ev = build(name), outcome(name), evaluations(name)
    bad = []
    if (got.converged, got.hyp, got.n_iterations, got.n_inliers, got.n_best) != (o.converged, o.hyp, o.n_iterations, o.n_inliers, o.n_best):
        bad.append(("outcome", (got.converged, got.hyp, got.n_iterations, got.n_inliers, got.n_best)))
    if not np.array_equal(got.inlier.astype(bool), o.inlier):
        bad.append(("inlier", int(np.count_nonzero(got.inlier.astype(bool) != o.inlier))))
    T = np.eye(4, dtype=np.float32)
    T[:3, :3], T[:3, 3] = got.R.astype(np.float32), got.t.astype(np.float32)
    if got.Tcw.tobytes() != T.tobytes():
        bad.append(("Tcw", got.Tcw))
    if ev is None:
        if not (np.array_equal(got.R, np.eye(3)) and not got.t.any() and not got.hyp_inliers.any()):
            bad.append(("identity", got.R))
        return bad
    tol = tol or tolerances(name)
    E = ev[0]
    ex, un, bl = ill_conditioned(name), unstable(name, tol["m"]), borderline(E, tol["g"])
    for h in range(P.n_hyp):
        c = int(got.hyp_inliers[h])
        if ex[h]:
            if c >= P.min_inliers:  # whatever an ill-conditioned solve returns, it must not touch the outcome
                bad.append(("ill-conditioned count", h, c))
            continue
        if abs(c - int(E.counts[h])) > bl[h]:
            bad.append(("count", h, c, int(E.counts[h]), int(bl[h])))
        if not un[h] and tuple(got.hyp_info[h]) != (E.info[h].planar, E.info[h].gn_its, E.info[h].gn_end):
            bad.append(("info", h, tuple(got.hyp_info[h])))
    if o.hyp >= 0:
        ang = rot_angle(got.R, o.R)
        dt = float(np.linalg.norm(got.t - o.t) / np.linalg.norm(o.t))
        if not (ang <= tol["rot_rad"] and dt <= tol["t_rel"]):
            bad.append(("pose", ang, dt))
        if not np.array_equal(got.hyp_pose[o.hyp], np.concatenate([got.R.ravel(), got.t])):
            bad.append(("hyp_pose", o.hyp))
    return bad
