"""numpy restatement of ``ORB_SLAM3::MLPnPsolver`` (ref:src/MLPnPsolver.cpp) as Tracking::Relocalization uses it:
float32 where the reference has float, float64 elsewhere, np.linalg for the decompositions.

``compute_pose`` is computePose (:483-1007) on one 6-point sample, ``evaluate`` runs it and CheckInliers
(:359-397) for every hypothesis of a problem, ``Solver`` is the sequential iterate (:145-301) with its
state across calls.  Refine (:402-470) solves on the best inlier set but never copies the result into
mRi / mti, so the CheckInliers that follows re-tests the current hypothesis: the observable rule is "the
first hypothesis with count > min returns its own pose, flags and count"; the dead solve is not computed.

Replica switches (tools/mlpnp_margins.py): ``basis_angle`` rotates every null-space basis [r s] in its
plane, ``eigh`` takes the smallest eigenvector of AtA from eigh instead of svd, ``flip_planar`` negates the
planar eigenvectors, ``flip_solution`` negates the solution vector of the linear solve.

The analytic Jacobian of mlpnpJacs (:1229-) is the derivative of n^T (R(w) p + T) / |R(w) p + T|; it is
written here in closed form, d(R p)/dw = -R [p]x (w w^T + (R^T - I) [w]x) / |w|^2, which like the
reference's expansion is NaN at w = 0."""
from __future__ import annotations

import math
from dataclasses import dataclass, replace

import numpy as np

from tests.pyref_sim3solver import project  # the float project(cv::Point3f) overloads compute the same

F = np.float32
EPS = np.finfo(np.float64).eps


# ------------------------------------------------------------------------------------ host parts
def ransac_parameters(prob, min_inliers, max_its, min_set, epsilon, n):
    """SetRansacParameters (:314-354) -> (mRansacMinInliers, mRansacMaxIts).  The reference converts the
    quotient to int before clamping, undefined past INT_MAX: a quotient that is not finite or not below
    max_its gives max_its."""
    eps = F(epsilon)
    with np.errstate(all="ignore"):
        prod = F(n) * eps
    nmin = int(prod) if np.isfinite(prod) else 0
    nmin = max(nmin, int(min_inliers), int(min_set))
    if n > 0 and eps < F(nmin) / F(n):
        eps = F(F(nmin) / F(n))
    if nmin == n:
        its = 1.0
    else:
        e3 = float(eps) ** 3
        with np.errstate(all="ignore"):
            den = np.log(np.float64(1.0) - e3)
            its = float(np.ceil(np.log(np.float64(1.0 - prob)) / den))
    if not its < max_its:
        return nmin, max(1, int(max_its))
    return nmin, (int(its) if its > 1 else 1)  # -inf (epsilon = 0) is below the clamp's floor


def draw_sets_literal(n, h, rand_ints, k=6):
    """:177-202 with the list the reference keeps; rand_ints are the RandomInt(0, size - 1) results."""
    r = iter(np.asarray(rand_ints).reshape(-1).tolist())
    out = np.empty((h, k), np.int32)
    for it in range(h):
        avail = list(range(n))
        for j in range(k):
            randi = next(r)
            out[it, j] = avail[randi]
            avail[randi] = avail[-1]
            avail.pop()
    return out


# ------------------------------------------------------------------------------------ computePose
def rodrigues2rot(w):
    R = np.eye(3)
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    n = math.sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]) if np.all(np.isfinite(w)) else float("nan")
    if n > EPS:  # a NaN omega leaves the identity
        R = R + math.sin(n) / n * K + (1 - math.cos(n)) / (n * n) * (K @ K)
    return R


def rot2rodrigues(R):
    w = np.zeros(3)
    c = (np.trace(R) - 1.0) / 2.0
    wn = math.acos(c) if -1.0 <= c <= 1.0 else float("nan")
    if wn > EPS:
        w = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]) * (wn / (2.0 * math.sin(wn)))
    return w


def skew(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def residuals_and_jacs(x, pts, rs):
    """mlpnp_residuals_and_jacs (:1171-1218) -> r (2 m), J (2 m x 6)."""
    w, T = x[:3], x[3:]
    m = len(pts)
    r = np.empty(2 * m)
    J = np.empty((2 * m, 6))
    with np.errstate(all="ignore"):
        R = rodrigues2rot(w)
        th2 = w @ w
        S = (np.outer(w, w) + (R.T - np.eye(3)) @ skew(w)) / th2
        for i in range(m):
            q = R @ pts[i] + T
            nq = np.sqrt(q @ q)
            v = q / nq
            D = (np.eye(3) - np.outer(v, v)) / nq
            dq = np.concatenate([-R @ skew(pts[i]) @ S, np.eye(3)], 1)
            r[2 * i:2 * i + 2] = rs[i].T @ v
            J[2 * i:2 * i + 2] = rs[i].T @ D @ dq
    return r, J


def fullpiv_qr_pivots(M):
    """|R_kk| of Eigen::FullPivHouseholderQR on a 3 x 3 matrix, and the number of non-zero pivots."""
    A = np.array(M, np.float64)
    n = 3
    piv = np.zeros(n)
    prec = EPS * n
    biggest = 0.0
    nonzero = n
    for k in range(n):
        sub = np.abs(A[k:, k:])
        rr, cc = np.unravel_index(np.argmax(sub), sub.shape)
        big = sub[rr, cc]
        if k == 0:
            biggest = big
        if big <= biggest * prec:
            nonzero = k
            break
        A[[k, k + rr]] = A[[k + rr, k]]
        A[:, [k, k + cc]] = A[:, [k + cc, k]]
        x = A[k:, k].copy()
        tail2 = float(x[1:] @ x[1:])
        if tail2 <= np.finfo(np.float64).tiny:
            beta = x[0]
        else:
            beta = math.sqrt(x[0] * x[0] + tail2)
            if x[0] >= 0:
                beta = -beta
            v = x.copy()
            v[0] = x[0] - beta
            v /= v[0]
            tau = (beta - x[0]) / beta
            A[k:, k + 1:] -= tau * np.outer(v, v @ A[k:, k + 1:])
        A[k, k] = beta
        A[k + 1:, k] = 0
        piv[k] = abs(beta)
    return piv, nonzero


def matrix_rank3(M):
    """FullPivHouseholderQR::rank() with the default threshold -> (rank, third pivot / threshold)."""
    piv, nonzero = fullpiv_qr_pivots(M)
    thr = piv.max() * EPS * 3
    rank = int(np.count_nonzero(piv[:nonzero] > thr))
    return rank, (piv[2] / thr if thr > 0 else 0.0)


@dataclass
class PoseInfo:
    planar: int = 0
    gn_its: int = 0          # linear solves of the Gauss-Newton
    gn_end: int = 0          # 0: five iterations, 1: converged, 2: break
    eig_gap: float = 1.0     # (second smallest - smallest eigenvalue of AtA) / second smallest
    margin: float = 1.0      # smallest relative distance of a deciding quantity from its threshold
    det_flip: int = 0
    quant: tuple = ()        # the deciding quantities as (value, threshold): third pivot / rank threshold vs 1,
                             # the sign choice's error difference vs 0, then per solve max|dx| vs 5, min|dx| vs 1,
                             # the basis-free bounds of max|J dx| vs 1e-5

    def decisions(self):
        """det_flip and the index of the sign choice follow the sign of the solution vector, which is the
        eigen-solver's choice (the pose is the same for u and -u): they are recorded, not compared."""
        return (self.planar, self.gn_its, self.gn_end)


def rel_move(a, b, thr):
    """|a - b| relative to the larger of |b| and the threshold: the unit of the margins of the deciding
    quantities (a NaN is as far from every threshold as can be)"""
    if not (np.isfinite(a) and np.isfinite(b)):
        return 0.0 if (np.isnan(a) and np.isnan(b)) or a == b else 1.0
    return abs(a - b) / max(abs(b), abs(a), thr, 1e-300)


def compute_pose(f, p, basis_angle=0.0, eigh=False, flip_planar=False, flip_solution=False):
    """computePose on the 6 bearings f and world points p (float64 rows) -> (R, t, PoseInfo)."""
    info = PoseInfo()
    m = len(f)
    rs = []
    ca, sa = math.cos(basis_angle), math.sin(basis_angle)
    for i in range(m):
        V = np.linalg.svd(f[i].reshape(1, 3))[2].T[:, 1:3]
        if basis_angle:
            V = np.stack([ca * V[:, 0] + sa * V[:, 1], -sa * V[:, 0] + ca * V[:, 1]], 1)
        rs.append(V)
    pts = p.copy()
    planar_test = pts.T @ pts
    rank, ratio = matrix_rank3(planar_test)
    quant = [(float(ratio), 1.0)]
    G = np.eye(3)
    p3 = pts
    if rank == 2:
        info.planar = 1
        G = np.linalg.eigh(planar_test)[1]  # ascending
        if flip_planar:
            G = -G
        p3 = pts @ G  # eigenRot * p with eigenRot = G^T
    cols = 9 if info.planar else 12
    A = np.zeros((2 * m, cols))
    for i in range(m):
        for k in range(2):
            n = rs[i][:, k]
            c = p3[i, 1:] if info.planar else p3[i]
            A[2 * i + k] = np.concatenate([np.outer(n, c).ravel(), n])
    AtA = A.T @ A
    ev = np.linalg.eigvalsh(AtA)
    info.eig_gap = float((ev[1] - ev[0]) / ev[1]) if ev[1] > 0 else 0.0
    u = np.linalg.eigh(AtA)[1][:, 0] if eigh else np.linalg.svd(AtA)[2][-1]
    if flip_solution:
        u = -u
    if info.planar:
        tmp = np.array([[0.0, u[0], u[1]], [0.0, u[2], u[3]], [0.0, u[4], u[5]]])
        tmp[:, 0] = np.cross(tmp[:, 1], tmp[:, 2])
        tmp = tmp.T.copy()
        scale = 1.0 / math.sqrt(abs(np.linalg.norm(tmp[:, 1]) * np.linalg.norm(tmp[:, 2])))
        U, _, Vt = np.linalg.svd(tmp)
        R1 = U @ Vt
        if np.linalg.det(R1) < 0:
            R1 = -R1
            info.det_flip |= 1
        R1 = G @ R1
        t = scale * u[6:9]
        R1 = -R1.T
        if np.linalg.det(R1) < 0:
            R1[:, 2] *= -1
            info.det_flip |= 2
        R2 = R1 * np.array([-1.0, -1.0, 1.0])[None]
        cands = [(R1, t), (R1, -t), (R2, t), (R2, -t)]
        vals = []
        for Rc, tc in cands:
            s = 0.0
            for k in range(6):
                q = Rc @ pts[k] + tc
                q = q / math.sqrt(q @ q)
                s += 1.0 - q @ f[k]
            vals.append(s)
        idx = int(np.argmin(vals))
        so = np.sort(vals)
        quant.append((float((so[1] - so[0]) / max(abs(so[1]), 1e-300)), 0.0))
        Rout, tout = cands[idx]
    else:
        tmp = np.array([[u[0], u[3], u[6]], [u[1], u[4], u[7]], [u[2], u[5], u[8]]])
        scale = 1.0 / abs(np.linalg.norm(tmp[:, 0]) * np.linalg.norm(tmp[:, 1]) * np.linalg.norm(tmp[:, 2])) ** (1.0 / 3.0)
        U, _, Vt = np.linalg.svd(tmp)
        R = U @ Vt
        if np.linalg.det(R) < 0:
            R = -R
            info.det_flip |= 1
        t = R @ (scale * u[9:12])
        err = []
        Ts = []
        for sgn in (1.0, -1.0):
            T = np.eye(4)
            T[:3, :3] = R
            T[:3, 3] = sgn * t
            T = np.linalg.inv(T)
            Ts.append(T)
            e = 0.0
            for k in range(6):
                v = T[:3, :3] @ pts[k] + T[:3, 3]
                v = v / math.sqrt(v @ v)
                e += 1.0 - v @ f[k]
            err.append(e)
        quant.append((float(abs(err[0] - err[1]) / max(abs(err[0]), abs(err[1]), 1e-300)), 0.0))
        tout = Ts[0][:3, 3] if err[0] < err[1] else Ts[1][:3, 3]
        Rout = Ts[0][:3, :3]
    x = np.concatenate([rot2rodrigues(Rout), tout])
    # mlpnp_gn (:1086-1160)
    it = 0
    end = 0
    solves = 0
    straddle = False
    with np.errstate(all="ignore"):
        while it < 5:
            r, J = residuals_and_jacs(x, pts, rs)
            H = J.T @ J
            g = J.T @ r
            solves += 1
            try:
                dx = np.linalg.solve(H, g) if np.all(np.isfinite(H)) else np.full(6, np.nan)
            except np.linalg.LinAlgError:
                dx = np.full(6, np.nan)
            a = np.abs(dx)
            quant += [(float(a.max()), 5.0), (float(a.min()), 1.0)]
            if a.max() > 5.0 or a.min() > 1.0:
                end = 2
                break
            dl = np.abs(J @ dx).max()
            # max|J dx| depends on the null-space bases: per point the pair (r^T, s^T) J dx has a basis-free norm
            # rho, and max|J dx| lies in [max rho / sqrt 2, max rho]
            Jd = (J @ dx).reshape(-1, 2)
            rho = float(np.sqrt((Jd * Jd).sum(1)).max())
            quant += [(rho, 1e-5), (rho / math.sqrt(2.0), 1e-5)]
            if (rho < 1e-5) != (rho / math.sqrt(2.0) < 1e-5):
                straddle = True
            x = x - dx
            if dl < 1e-5:
                end = 1
                break
            it += 1
    info.gn_its, info.gn_end = solves, end
    info.quant = tuple(quant)
    info.margin = min(1.0 if thr == 0.0 and not np.isfinite(v) else (abs(v) if thr == 0.0 else rel_move(v, thr, thr))
                      for v, thr in quant)
    if straddle:
        info.margin = 0.0
    return rodrigues2rot(x[:3]), x[3:].copy(), info


# ------------------------------------------------------------------------------------ CheckInliers
@dataclass
class Evaluation:
    counts: np.ndarray   # H
    inlier: np.ndarray   # H x N bool
    R: np.ndarray        # H x 3 x 3 float64
    t: np.ndarray        # H x 3 float64
    ratio: np.ndarray    # H x N float64: err / max_err
    info: list           # PoseInfo per hypothesis


def check_inliers(P, R, t):
    """CheckInliers -> (flags, err / max_err): double R, t times float point, summed left to right in double,
    rounded once; then float projection and float squared error."""
    X = P.p3dw.astype(np.float64)
    with np.errstate(all="ignore"):
        xc = np.stack([(R[i, 0] * X[:, 0] + R[i, 1] * X[:, 1] + R[i, 2] * X[:, 2] + t[i]) for i in range(3)], 1).astype(F)
        u, v = project(P.cam, xc)
        dx = P.p2d[:, 0] - u.astype(F)
        dy = P.p2d[:, 1] - v.astype(F)
        e = (dx * dx + dy * dy).astype(F)
        return e < P.max_err, e.astype(np.float64) / P.max_err


def evaluate(P, **replica) -> Evaluation:
    H, n = len(P.samples), len(P.p3dw)
    counts = np.zeros(H, np.int32)
    inl = np.zeros((H, n), bool)
    Rs, ts, ratio, infos = np.zeros((H, 3, 3)), np.zeros((H, 3)), np.zeros((H, n)), []
    f64, p64 = P.bearing.astype(np.float64), P.p3dw.astype(np.float64)
    cache = {}
    for h in range(H):
        key = tuple(P.samples[h])
        if key not in cache:
            s = P.samples[h]
            R, t, info = compute_pose(f64[s], p64[s], **replica)
            cache[key] = (R, t, info) + check_inliers(P, R, t)
        Rs[h], ts[h], info, inl[h], ratio[h] = cache[key]
        infos.append(info)
        counts[h] = inl[h].sum()
    return Evaluation(counts, inl, Rs, ts, ratio, infos)


# ------------------------------------------------------------------------------------ iterate
def tcw(R, t):
    T = np.eye(4, dtype=F)
    T[:3, :3] = R.astype(F)
    T[:3, 3] = t.astype(F)
    return T


class Solver:
    """The sequential part of MLPnPsolver over the hypotheses of ``E``: hypothesis h is what iteration h + 1
    draws and evaluates.  ``max_its`` is mRansacMaxIts; E must hold every hypothesis the calls consume."""

    def __init__(self, P, E, max_its=None):
        self.P, self.E = P, E
        self.N = len(P.p3dw)
        self.mRansacMinInliers = int(P.min_inliers)
        self.mRansacMaxIts = len(P.samples) if max_its is None else int(max_its)
        self.mnIterations = 0
        self.mnBestInliers = 0
        self.best = -1
        self.returned = -1

    def iterate(self, nIterations):
        """-> (ok, bNoMore, vbInliers over the N kept matches, nInliers, Tout)."""
        vb = np.zeros(self.N, bool)
        Tout = np.eye(4, dtype=F)
        if self.N < self.mRansacMinInliers:
            return False, True, vb, 0, Tout
        nCurrent = 0
        while self.mnIterations < self.mRansacMaxIts or nCurrent < nIterations:
            nCurrent += 1
            h = self.mnIterations
            self.mnIterations += 1
            c = int(self.E.counts[h])
            if c >= self.mRansacMinInliers:
                if c > self.mnBestInliers:
                    self.mnBestInliers = c
                    self.best = h
                # Refine(): the current hypothesis again
                if c > self.mRansacMinInliers:
                    self.returned = h
                    return True, False, self.E.inlier[h].copy(), c, tcw(self.E.R[h], self.E.t[h])
        if self.mnIterations >= self.mRansacMaxIts:
            if self.mnBestInliers >= self.mRansacMinInliers:
                h = self.best
                self.returned = h
                return True, True, self.E.inlier[h].copy(), self.mnBestInliers, tcw(self.E.R[h], self.E.t[h])
            return False, True, vb, 0, Tout
        return False, False, vb, 0, Tout


@dataclass
class Outcome:
    converged: bool
    hyp: int
    n_iterations: int
    n_inliers: int
    n_best: int
    inlier: np.ndarray
    R: np.ndarray
    t: np.ndarray
    Tcw: np.ndarray


def solve(P, E=None) -> Outcome:
    """One iterate() that consumes all H hypotheses on a fresh solver, as osg_mlpnp_ransac reports it."""
    n = len(P.p3dw)
    none = Outcome(False, -1, 0, 0, 0, np.zeros(n, bool), np.eye(3), np.zeros(3), np.eye(4, dtype=F))
    if n == 0 or n < P.min_inliers:
        return none
    E = E if E is not None else evaluate(P)
    S = Solver(P, E)
    ok, no_more, vb, nin, T = S.iterate(1)
    h = S.returned
    if not ok:
        return replace(none, n_iterations=S.mnIterations)
    return Outcome(not no_more, h, S.mnIterations, nin, S.mnBestInliers, vb, E.R[h], E.t[h], T)


def replay_window(counts, min_inliers, first, length, n_best, best_hyp):
    """What csrc/mlpnp_select.h must return for the window [first, first + length):
    (converged, hyp, n_iterations, n_best, best_hyp)."""
    for h in range(first, first + length):
        c = int(counts[h])
        if c >= min_inliers:
            if c > n_best:
                n_best, best_hyp = c, h
            if c > min_inliers:
                return 1, h, h + 1, int(n_best), best_hyp
    return 0, (best_hyp if n_best >= min_inliers else -1), first + length, int(n_best), best_hyp


def nudged(P, rng):
    """Every bearing and point coordinate moved by -1, 0 or +1 float ulp."""
    def mv(a):
        d = rng.integers(-1, 2, a.shape)
        return np.where(d > 0, np.nextafter(a, F(np.inf)), np.where(d < 0, np.nextafter(a, F(-np.inf)), a)).astype(F)
    return replace(P, bearing=mv(P.bearing), p3dw=mv(P.p3dw))
