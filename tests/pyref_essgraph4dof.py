"""numpy float64 restatement of the g2o part of ``Optimizer::OptimizeEssentialGraph4DoF``
(ref:src/Optimizer.cc:4870-5198), the checker of the 4-DoF kernels of csrc/essgraph.hip.  Written from the
reference, independent of the kernels:

  * ``ImuCamPoses``: the ImuCamPose of every VertexPose4DoF (ref:include/G2oTypes.h:58-111) as arrays over the
    vertices, with ``UpdateW`` as written (ref:src/G2oTypes.cc:252-285): DR = ExpSO3(ur) DR, Rwb = DR Rwb0,
    twb += ut, its++, at its >= 5 four entries of DR zeroed and DR normalised, then the camera re-derived;
  * ExpSO3 / LogSO3 (ref:src/G2oTypes.cc:912-944) and NormalizeRotation (ref:include/G2oTypes.h:67-72) by SVD;
  * Edge4DoF::computeError (ref:include/G2oTypes.h:965-971);
  * g2o's numeric Jacobian (ref:Thirdparty/g2o/g2o/core/base_binary_edge.hpp:147-200) through oplusImpl =
    UpdateW((0, 0, u0, u1, u2, u3)), a fixed vertex's side skipped, all edges at once;
  * the Levenberg-Marquardt loop of tests/pyref_essgraph.py (mirrored: the same rules over another vertex, a
    diagonal information and g2o's own lambda) and its independent solve (``pyref_essgraph._solve``).

A problem is any object with the attributes of orb_slam3_comments_ghr_amd.optimizer.EssentialGraph4DoFProblem.
``Variant`` names the ways tools/essgraph4dof_margins.py perturbs the arithmetic.
"""
import copy
from dataclasses import dataclass

import numpy as np

from tests import pyref_essgraph as EG

DELTA = 1e-9
KEYS = ("rot_rad", "t_rel", "tilt_rad", "chi2_initial_rel", "chi2_rel", "edge_chi2_rel")


@dataclass(frozen=True)
class Variant:
    trig: int = 0                # sin / cos / acos moved by this many ulps
    reverse_sums: bool = False   # the sums over an edge's rows and over the edges taken in reverse
    polar: bool = False          # NormalizeRotation as the polar factor R (R'R)^-1/2 instead of U V' of the SVD
    other_solver: bool = False   # the linear solve through another factorisation


PLAIN = Variant()
_V = PLAIN


def _ulps(a, k):
    for _ in range(abs(k)):
        a = np.nextafter(a, np.inf if k > 0 else -np.inf)
    return a


def _sin(a):
    return _ulps(np.sin(a), _V.trig)


def _cos(a):
    return _ulps(np.cos(a), _V.trig)


def _acos(a):
    return _ulps(np.arccos(a), _V.trig)


# ------------------------------------------------------------------------------------- SO(3), over arrays
def normalize_rotation(R):
    """NormalizeRotation: U V' of the SVD (of every matrix of R)"""
    R = np.asarray(R, float)
    if _V.polar:
        w, V = np.linalg.eigh(np.swapaxes(R, -1, -2) @ R)
        return R @ ((V / np.sqrt(w)[..., None, :]) @ np.swapaxes(V, -1, -2))
    U, _, Vt = np.linalg.svd(R)
    return U @ Vt


def exp_so3(w):
    """ExpSO3 of every row of w (n, 3): both branches normalise their result"""
    w = np.asarray(w, float).reshape(-1, 3)
    x, y, z = w[:, 0], w[:, 1], w[:, 2]
    d2 = x * x + y * y + z * z
    d = np.sqrt(d2)
    W = np.zeros((len(w), 3, 3))
    W[:, 0, 1], W[:, 0, 2] = -z, y
    W[:, 1, 0], W[:, 1, 2] = z, -x
    W[:, 2, 0], W[:, 2, 1] = -y, x
    W2 = W @ W
    small = d < 1e-5
    ds = np.where(small, 1.0, d)
    res = np.where(small[:, None, None], np.eye(3) + W + 0.5 * W2,
                   np.eye(3) + W * (_sin(ds) / ds)[:, None, None] + W2 * ((1.0 - _cos(ds)) / (ds * ds))[:, None, None])
    return normalize_rotation(res)


def log_so3(R):
    """LogSO3 of every matrix of R (n, 3, 3): the 0.5f and both early returns as written"""
    R = np.asarray(R, float).reshape(-1, 3, 3)
    tr = R[:, 0, 0] + R[:, 1, 1] + R[:, 2, 2]
    w = np.stack([(R[:, 2, 1] - R[:, 1, 2]) / 2, (R[:, 0, 2] - R[:, 2, 0]) / 2, (R[:, 1, 0] - R[:, 0, 1]) / 2], 1)
    costheta = (tr - 1.0) * 0.5
    outside = (costheta > 1) | (costheta < -1)
    theta = _acos(np.where(outside, 0.0, costheta))
    s = _sin(theta)
    early = outside | (np.abs(s) < 1e-5)
    return np.where(early[:, None], w, theta[:, None] * w / np.where(early, 1.0, s)[:, None])


# ------------------------------------------------------------------------------------- the vertex estimates
class ImuCamPoses:
    """The ImuCamPose of n vertices.  Rcw / tcw are what the constructor stored until the first UpdateW."""

    def __init__(self, rows):
        a = np.asarray(rows, float).reshape(-1, 36)
        self.Rwb = a[:, 0:9].reshape(-1, 3, 3).copy()
        self.twb = a[:, 9:12].copy()
        self.Rcw = a[:, 12:21].reshape(-1, 3, 3).copy()
        self.tcw = a[:, 21:24].copy()
        self.Rcb = a[:, 24:33].reshape(-1, 3, 3).copy()
        self.tcb = a[:, 33:36].copy()
        self.Rwb0 = self.Rwb.copy()
        self.DR = np.broadcast_to(np.eye(3), self.Rwb.shape).copy()
        self.its = np.zeros(len(a), np.int64)

    def copy(self):
        q = copy.copy(self)
        for k in ("Rwb", "twb", "Rcw", "tcw", "DR", "its"):
            setattr(q, k, getattr(self, k).copy())
        return q

    def take(self, idx):
        q = copy.copy(self)
        for k in ("Rwb", "twb", "Rcw", "tcw", "Rcb", "tcb", "Rwb0", "DR", "its"):
            setattr(q, k, getattr(self, k)[idx].copy())
        return q

    def UpdateW(self, pu, which=None):
        """ImuCamPose::UpdateW of the vertices ``which`` (all) with the rows of pu (m, 6)"""
        idx = np.arange(len(self.its)) if which is None else np.asarray(which, np.int64)
        pu = np.asarray(pu, float).reshape(len(idx), 6)
        dR = exp_so3(pu[:, 0:3])
        DR = dR @ self.DR[idx]
        Rwb = DR @ self.Rwb0[idx]
        twb = self.twb[idx] + pu[:, 3:6]
        its = self.its[idx] + 1
        norm = its >= 5
        if norm.any():
            D = DR[norm]
            D[:, 0, 2] = 0.0
            D[:, 1, 2] = 0.0
            D[:, 2, 0] = 0.0
            D[:, 2, 1] = 0.0
            DR[norm] = normalize_rotation(D)
            its[norm] = 0
        Rbw = np.swapaxes(Rwb, 1, 2)
        tbw = -np.einsum("nij,nj->ni", Rbw, twb)
        self.DR[idx], self.Rwb[idx], self.twb[idx], self.its[idx] = DR, Rwb, twb, its
        self.Rcw[idx] = self.Rcb[idx] @ Rbw
        self.tcw[idx] = np.einsum("nij,nj->ni", self.Rcb[idx], tbw) + self.tcb[idx]

    def oplus(self, u, which=None):
        """VertexPose4DoF::oplusImpl: rows (m, 4) of (yaw, translation)"""
        u = np.asarray(u, float).reshape(-1, 4)
        self.UpdateW(np.concatenate([np.zeros((len(u), 2)), u], 1), which)


def edge_errors(meas, Vi, Vj):
    """Edge4DoF::computeError for arrays of measurements (E, 12) and the ImuCamPoses of both ends -> (E, 6)"""
    meas = np.asarray(meas, float).reshape(-1, 12)
    dR, dt = meas[:, :9].reshape(-1, 3, 3), meas[:, 9:]
    Rjt = np.swapaxes(Vj.Rcw, 1, 2)
    er = log_so3((Vi.Rcw @ Rjt) @ np.swapaxes(dR, 1, 2))
    et = np.einsum("nij,nj->ni", Vi.Rcw, -np.einsum("nij,nj->ni", Rjt, Vj.tcw)) + Vi.tcw - dt
    return np.concatenate([er, et], 1)


def numeric_jacobians(meas, Vi, Vj, fixed_i, fixed_j, delta=DELTA):
    """g2o's central differences through oplusImpl: (J_i, J_j), (E, 6, 4) each; a fixed vertex's side stays 0.
    Every perturbed estimate is a pushed copy, so its counter and DR are the popped ones afterwards."""
    E = len(Vi.its)
    Ji, Jj = np.zeros((E, 6, 4)), np.zeros((E, 6, 4))
    scalar = 1.0 / (2 * delta)
    for d in range(4):
        u = np.zeros((E, 4))
        u[:, d] = delta
        for J, side in ((Ji, 0), (Jj, 1)):
            pair = []
            for sign in (1.0, -1.0):
                T = (Vj if side else Vi).copy()
                T.oplus(sign * u)
                pair.append(edge_errors(meas, Vi if side else T, T if side else Vj))
            J[:, :, d] = scalar * (pair[0] - pair[1])
    Ji[np.asarray(fixed_i, bool)] = 0
    Jj[np.asarray(fixed_j, bool)] = 0
    return Ji, Jj


# ------------------------------------------------------------------------------------- the optimisation
@dataclass
class PyrefResult:
    R: np.ndarray            # Rcw (n, 3, 3)
    t: np.ndarray            # tcw (n, 3)
    Rwb: np.ndarray
    twb: np.ndarray
    chi2_initial: float
    chi2_final: float
    lm_iterations: int
    lm_trials: int
    edge_chi2: np.ndarray
    accepted: int = 0        # accepted steps
    rejected: int = 0        # rejected trials
    its: np.ndarray | None = None


def _other_solve(H, b):
    """(ok, x) through an eigendecomposition of the dense matrix in place of Cholesky / LU"""
    Hd = H.toarray() if hasattr(H, "toarray") else H
    w, V = np.linalg.eigh(Hd)
    if not np.all(w > 0):
        return False, None
    return True, V @ ((V.T @ b) / w)


def _rowsum(a):
    return a[:, ::-1].sum(1) if _V.reverse_sums else a.sum(1)


def _total(c):
    return float(c[::-1].sum()) if _V.reverse_sums else float(c.sum())


def optimize(P, variant=PLAIN):
    """SparseOptimizer::optimize(max_iterations or 20) on the gathered graph."""
    global _V
    _V = variant
    try:
        return _optimize(P)
    finally:
        _V = PLAIN


def _optimize(P):
    import scipy.sparse as sp
    V = ImuCamPoses(P.pose)
    n = len(V.its)
    meas = np.asarray(P.e_meas, float).reshape(-1, 12)
    v0, v1 = np.asarray(P.e_v0, np.int64), np.asarray(P.e_v1, np.int64)
    E = len(v0)
    om = np.asarray(P.info_diag, float)
    fixed = np.asarray(P.fixed, bool)
    free = np.nonzero(~fixed)[0]
    nf = len(free)
    fidx = np.full(n, -1, np.int64)
    fidx[free] = np.arange(nf)
    n_iter = int(P.max_iterations) if int(P.max_iterations) > 0 else 20

    def chi2s(S):
        e = edge_errors(meas, S.take(v0), S.take(v1))
        return _rowsum(e * (om * e))

    def result(S, chi2_initial, c, iters, trials, acc, rej):
        return PyrefResult(S.Rcw, S.tcw, S.Rwb, S.twb, chi2_initial, _total(c), iters, trials, c, acc, rej, S.its)

    c0 = chi2s(V) if E else np.zeros(0)
    chi2_initial = _total(c0)
    if E == 0 or nf == 0:
        return result(V, chi2_initial, c0, 0, 0, 0, 0)
    f0, f1 = fixed[v0], fixed[v1]
    a0, a1 = fidx[v0], fidx[v1]
    lam = ni = 0.0
    n_bad = 0
    x = np.zeros(4 * nf)
    iters = trials = acc = rej = 0
    current = chi2_initial
    rr, cc = np.meshgrid(np.arange(4), np.arange(4), indexing="ij")
    order = slice(None, None, -1) if _V.reverse_sums else slice(None)
    for it in range(n_iter):
        iters += 1
        Vi, Vj = V.take(v0), V.take(v1)
        e = edge_errors(meas, Vi, Vj)
        current = _total(_rowsum(e * (om * e)))
        ini = current
        Ji, Jj = numeric_jacobians(meas, Vi, Vj, f0, f1)
        rows, cols, vals = [], [], []
        b = np.zeros(4 * nf)

        def add(Ja, Jb, ia, ib, m):
            blk = np.einsum("nri,nrj->nij", (Ja[m] * om[None, :, None])[:, order], Jb[m][:, order])
            rows.append((4 * ia[m])[:, None, None] + rr)
            cols.append((4 * ib[m])[:, None, None] + cc)
            vals.append(blk)

        m0, m1 = ~f0, ~f1
        add(Ji, Ji, a0, a0, m0)
        add(Jj, Jj, a1, a1, m1)
        add(Ji, Jj, a0, a1, m0 & m1)
        add(Jj, Ji, a1, a0, m0 & m1)
        we = om * e
        np.add.at(b, (4 * a0[m0])[:, None] + np.arange(4), -np.einsum("nri,nr->ni", Ji[m0][:, order], we[m0][:, order]))
        np.add.at(b, (4 * a1[m1])[:, None] + np.arange(4), -np.einsum("nri,nr->ni", Jj[m1][:, order], we[m1][:, order]))
        H = sp.coo_matrix((np.concatenate([v.ravel() for v in vals])[order],
                           (np.concatenate([r.ravel() for r in rows])[order], np.concatenate([c.ravel() for c in cols])[order])),
                          shape=(4 * nf, 4 * nf)).tocsr()
        if it == 0:
            lam = float(P.lambda_init) if P.lambda_init > 0 else 1e-5 * float(np.max(np.abs(H.diagonal())))
            ni = 2.0
            n_bad = 0
        rho = 0.0
        qmax = 0
        while True:
            trials += 1
            backup = V.copy()          # push
            Hl = H + lam * sp.identity(4 * nf, format="csr")
            ok2, xs = _other_solve(Hl, b) if _V.other_solver else EG._solve(Hl, b, nf)
            if ok2:
                x = xs
            V.oplus(x.reshape(nf, 4), free)
            temp = _total(chi2s(V))
            if not ok2:
                temp = float(np.finfo(float).max)
            rho = current - temp
            scale = float(np.sum(x * (lam * x + b))) + 1e-3
            rho /= scale
            if rho > 0 and np.isfinite(temp):
                alpha = 1. - (2 * rho - 1) ** 3
                alpha = min(alpha, 2. / 3.)
                lam *= max(1. / 3., alpha)
                ni = 2.0
                current = temp
                acc += 1
            else:
                lam *= ni
                ni *= 2
                V = backup             # pop
                rej += 1
            qmax += 1
            if not (rho < 0 and qmax < 10):
                break
        if qmax == 10 or rho == 0:
            break
        if (ini - current) * 1e3 < ini:
            n_bad += 1
        else:
            n_bad = 0
        if n_bad >= 3:
            break
    return result(V, chi2_initial, chi2s(V), iters, trials, acc, rej)


# ------------------------------------------------------------------------------------- write-back
def sim3_rows(R, t):
    """the unit-scale Sim3 rows (q x y z w, t, 1) of camera poses, as osg_essgraph_correct_points reads them"""
    from orb_slam3_comments_ghr_amd.optimizer import rot_to_quat
    return np.array([np.concatenate([rot_to_quat(r), tt, [1.0]]) for r, tt in zip(np.asarray(R), np.asarray(t))]).reshape(-1, 8)


# ------------------------------------------------------------------------------------- nudge study
def nudged(P, rng):
    """A replica whose input poses and measurements each move by +-1 ulp at random (a fixed vertex too)."""
    Q = copy.copy(P)

    def nudge(a):
        a = np.array(a, np.float64)
        up = rng.random(a.shape) < 0.5
        return np.where(up, np.nextafter(a, np.inf), np.nextafter(a, -np.inf))

    Q.pose, Q.e_meas = nudge(P.pose), nudge(P.e_meas)
    return Q


def rot_angle(Ra, Rb):
    """|LogSO3(Ra Rb')| per vertex, by the chord where acos loses its digits"""
    D = np.asarray(Ra) @ np.swapaxes(np.asarray(Rb), -1, -2)
    w = np.stack([D[..., 2, 1] - D[..., 1, 2], D[..., 0, 2] - D[..., 2, 0], D[..., 1, 0] - D[..., 0, 1]], -1) / 2
    s = np.linalg.norm(w, axis=-1)
    c = (D[..., 0, 0] + D[..., 1, 1] + D[..., 2, 2] - 1) / 2
    return np.arctan2(s, c)


def tilt(Rwb_out, Rwb_in):
    """per vertex the angle between (Rwb_out Rwb_in') z and z: what a yaw-only update leaves at 0"""
    z = (np.asarray(Rwb_out) @ np.swapaxes(np.asarray(Rwb_in), -1, -2))[..., :, 2]
    return np.arctan2(np.hypot(z[..., 0], z[..., 1]), z[..., 2])


def differences(got, base, P):
    """The compared quantities of a result (R, t, Rwb, chi2_initial, chi2_final, edge_chi2 attributes) against
    base on the problem P: the largest over the vertices / edges."""
    Rin = np.asarray(P.pose, float).reshape(-1, 36)[:, :9].reshape(-1, 3, 3)
    n = len(base.t)
    tmax = max(float(np.max(np.linalg.norm(base.t, axis=1))) if n else 0.0, 1e-300)
    emax = max(float(np.max(base.edge_chi2)) if len(base.edge_chi2) else 0.0, 1e-300)
    return {
        "rot_rad": float(np.max(rot_angle(got.R, base.R))) if n else 0.0,
        "t_rel": float(np.max(np.linalg.norm(got.t - base.t, axis=1)) / tmax) if n else 0.0,
        "tilt_rad": float(np.max(np.abs(tilt(got.Rwb, Rin) - tilt(base.Rwb, Rin)))) if n else 0.0,
        "chi2_initial_rel": abs(got.chi2_initial - base.chi2_initial) / max(abs(base.chi2_initial), 1e-300),
        "chi2_rel": abs(got.chi2_final - base.chi2_final) / max(abs(base.chi2_final), 1e-300),
        "edge_chi2_rel": float(np.max(np.abs(got.edge_chi2 - base.edge_chi2)) / emax) if len(base.edge_chi2) else 0.0,
    }


def spreads(base, reps, P):
    """Largest deviation of the replicas from the base result, per compared quantity."""
    out = {k: 0.0 for k in KEYS}
    for r in reps:
        for k, v in differences(r, base, P).items():
            out[k] = max(out[k], v)
    return out
