"""numpy restatement of ORB_SLAM3::Sim3Solver (ref:src/Sim3Solver.cc), the checker of the HIP solver.

Float32 wherever the reference holds a float (points, M, N as a Matrix4f, the eigenvector, R, t, s, both
projections and the squared errors), double for ``ang``, ``nom / den`` and ``1 / s``; the 4x4 goes through
``np.linalg.eig`` (a general, unsymmetric solver, as Eigen's EigenSolver is).  Three-term sums associate
as Eigen's unrolled reductions do, a + (b + c).

``evaluate`` computes ComputeSim3 + CheckInliers of every sampled triple (independent of each other);
``Solver`` is the sequential part, statement by statement: SetRansacParameters, both ``iterate``
overloads and ``find`` with mnIterations / mnBestInliers carried from call to call.

``nudged`` makes the replicas that bound what an implementation may legitimately differ by: the points
moved by -1 / 0 / +1 float ulp, and (every second replica) the Horn solve in float64 through ``eigh``.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, replace

import numpy as np

F = np.float32


def ransac_iterations(prob, min_inliers, n, max_its):
    """SetRansacParameters (:120-144).  A quotient that is NaN, +inf or not below max_its gives max_its (the
    reference converts it to int before clamping, which is undefined there), -inf (epsilon = 0) gives 1;
    n < min_inliers never iterates: 1."""
    max_its = max(1, int(max_its))
    if n <= 0 or n < min_inliers or min_inliers == n:
        return 1
    eps = float(F(min_inliers) / F(n))
    den = math.log(1 - eps ** 3) if eps ** 3 < 1 else float("-inf")
    if den == 0.0:  # epsilon = 0: the quotient is -inf, below the clamp's floor
        return 1
    x = math.ceil(math.log(1 - prob) / den) if math.isfinite(den) else 0
    if not x < max_its:
        return max_its
    return max(1, int(x))


def draw_samples_literal(n, h, rand_ints):
    """:169-183, with the list the reference keeps."""
    r = iter(np.asarray(rand_ints).reshape(-1).tolist())
    out = np.empty((h, 3), np.int32)
    for it in range(h):
        avail = list(range(n))
        for j in range(3):
            randi = next(r)
            out[it, j] = avail[randi]
            avail[randi] = avail[-1]
            avail.pop()
    return out


def _s3(a, b, c):
    return a + (b + c)


def project(cam, X):
    """GeometricCamera::project(Eigen::Vector3f) of the rows of X (float32) -> (u, v) float32."""
    p = [F(cam.p[i]) for i in range(8)]
    x, y, z = X[..., 0], X[..., 1], X[..., 2]
    with np.errstate(all="ignore"):
        if cam.type == 1:
            th = np.arctan2(np.sqrt(x * x + y * y), z).astype(F)
            ps = np.arctan2(y, x).astype(F)
            th2 = th * th
            th3 = th * th2
            th5 = th3 * th2
            th7 = th5 * th2
            th9 = th7 * th2
            r = th + p[4] * th3 + p[5] * th5 + p[6] * th7 + p[7] * th9
            return p[0] * r * np.cos(ps).astype(F) + p[2], p[1] * r * np.sin(ps).astype(F) + p[3]
        return p[0] * x / z + p[2], p[1] * y / z + p[3]


@dataclass
class Evaluation:
    counts: np.ndarray   # H
    inlier: np.ndarray   # H x N bool
    R: np.ndarray        # H x 3 x 3 float32
    t: np.ndarray        # H x 3
    s: np.ndarray        # H
    ratio1: np.ndarray   # H x N float64: err1 / max_err1
    ratio2: np.ndarray
    eig_gap: np.ndarray  # H: (top - second eigenvalue) / |top|


def _horn(P, horn64):
    """ComputeSim3 (:307-407) for every triple at once -> R, t, s, sR, t, sRinv, tinv, eig gap."""
    T = F if not horn64 else np.float64
    a = P.p1c[P.samples].astype(T)  # H x 3(point) x 3(coord)
    b = P.p2c[P.samples].astype(T)
    three = T(3)
    o1 = _s3(a[:, 0], a[:, 1], a[:, 2]) / three
    o2 = _s3(b[:, 0], b[:, 1], b[:, 2]) / three
    pr1 = np.transpose(a - o1[:, None, :], (0, 2, 1))  # H x coord x point
    pr2 = np.transpose(b - o2[:, None, :], (0, 2, 1))
    H = len(a)
    M = np.empty((H, 3, 3), T)
    for i in range(3):
        for j in range(3):
            M[:, i, j] = _s3(pr2[:, i, 0] * pr1[:, j, 0], pr2[:, i, 1] * pr1[:, j, 1], pr2[:, i, 2] * pr1[:, j, 2])
    N = np.empty((H, 4, 4), T)
    N[:, 0, 0] = M[:, 0, 0] + M[:, 1, 1] + M[:, 2, 2]
    N[:, 0, 1] = N[:, 1, 0] = M[:, 1, 2] - M[:, 2, 1]
    N[:, 0, 2] = N[:, 2, 0] = M[:, 2, 0] - M[:, 0, 2]
    N[:, 0, 3] = N[:, 3, 0] = M[:, 0, 1] - M[:, 1, 0]
    N[:, 1, 1] = M[:, 0, 0] - M[:, 1, 1] - M[:, 2, 2]
    N[:, 1, 2] = N[:, 2, 1] = M[:, 0, 1] + M[:, 1, 0]
    N[:, 1, 3] = N[:, 3, 1] = M[:, 2, 0] + M[:, 0, 2]
    N[:, 2, 2] = -M[:, 0, 0] + M[:, 1, 1] - M[:, 2, 2]
    N[:, 2, 3] = N[:, 3, 2] = M[:, 1, 2] + M[:, 2, 1]
    N[:, 3, 3] = -M[:, 0, 0] - M[:, 1, 1] + M[:, 2, 2]
    if horn64:
        ev, evec = np.linalg.eigh(N)
    else:
        ev, evec = np.linalg.eig(N)
        ev, evec = ev.real.astype(T), evec.real.astype(T)
    top = np.argmax(ev, 1)
    idx = np.arange(H)
    q = evec[idx, :, top]
    evs = np.sort(ev.astype(np.float64), 1)
    with np.errstate(all="ignore"):
        gap = (evs[:, 3] - evs[:, 2]) / np.abs(evs[:, 3])
        vec = q[:, 1:4]
        vn = np.sqrt(_s3(vec[:, 0] * vec[:, 0], vec[:, 1] * vec[:, 1], vec[:, 2] * vec[:, 2]))
        ang = np.arctan2(vn.astype(np.float64), q[:, 0].astype(np.float64))
        f = (2 * ang).astype(T)
        vec = f[:, None] * vec / vn[:, None]
        # Sophus::SO3::exp(vec).matrix()
        th_sq = _s3(vec[:, 0] * vec[:, 0], vec[:, 1] * vec[:, 1], vec[:, 2] * vec[:, 2])
        th = np.sqrt(th_sq)
        half = T(0.5) * th
        small = th_sq < T(1e-10) * T(1e-10)
        po4 = th_sq * th_sq
        imag = np.where(small, T(0.5) - T(1.0 / 48.0) * th_sq + T(1.0 / 3840.0) * po4, np.sin(half) / th).astype(T)
        real = np.where(small, T(1) - T(1.0 / 8.0) * th_sq + T(1.0 / 384.0) * po4, np.cos(half)).astype(T)
        qw, qx, qy, qz = real, imag * vec[:, 0], imag * vec[:, 1], imag * vec[:, 2]
        two, one = T(2), T(1)
        tx, ty, tz = two * qx, two * qy, two * qz
        twx, twy, twz = tx * qw, ty * qw, tz * qw
        txx, txy, txz = tx * qx, ty * qx, tz * qx
        tyy, tyz, tzz = ty * qy, tz * qy, tz * qz
        R = np.empty((H, 3, 3), T)
        R[:, 0, 0] = one - (tyy + tzz)
        R[:, 0, 1] = txy - twz
        R[:, 0, 2] = txz + twy
        R[:, 1, 0] = txy + twz
        R[:, 1, 1] = one - (txx + tzz)
        R[:, 1, 2] = tyz - twx
        R[:, 2, 0] = txz - twy
        R[:, 2, 1] = tyz + twx
        R[:, 2, 2] = one - (txx + tyy)
        if P.fix_scale:
            s = np.ones(H, T)
        else:
            nom = np.zeros(H, T)
            den = np.zeros(H, T)
            for j in range(3):
                for i in range(3):
                    p3 = _s3(R[:, i, 0] * pr2[:, 0, j], R[:, i, 1] * pr2[:, 1, j], R[:, i, 2] * pr2[:, 2, j])
                    nom = nom + pr1[:, i, j] * p3
                    den = den + p3 * p3
            s = (nom.astype(np.float64) / den.astype(np.float64)).astype(T)
        sR = s[:, None, None] * R
        t = np.stack([o1[:, i] - _s3(sR[:, i, 0] * o2[:, 0], sR[:, i, 1] * o2[:, 1], sR[:, i, 2] * o2[:, 2])
                      for i in range(3)], 1)
        inv = (1.0 / s.astype(np.float64)).astype(T)
        sRi = inv[:, None, None] * np.transpose(R, (0, 2, 1))
        ti = np.stack([_s3(-sRi[:, i, 0] * t[:, 0], -sRi[:, i, 1] * t[:, 1], -sRi[:, i, 2] * t[:, 2])
                       for i in range(3)], 1)
    c = lambda x: x.astype(F)
    return c(R), c(t), c(s), c(sR), c(sRi), c(ti), gap


def evaluate(P, horn64=False, chunk=64) -> Evaluation:
    """ComputeSim3 + CheckInliers (:409-433) of every sampled triple."""
    H, n = len(P.samples), len(P.p1c)
    R, t, s, sR, sRi, ti, gap = _horn(P, horn64)
    u1, v1 = project(P.cam1, P.p1c)  # mvP1im1
    u2, v2 = project(P.cam2, P.p2c)  # mvP2im2
    ratio1 = np.empty((H, n))
    ratio2 = np.empty((H, n))
    inl = np.empty((H, n), bool)
    with np.errstate(all="ignore"):
        for h0 in range(0, H, chunk):
            sl = slice(h0, min(H, h0 + chunk))

            def tf(A, tt, X):
                return np.stack([_s3(A[:, None, i, 0] * X[None, :, 0], A[:, None, i, 1] * X[None, :, 1],
                                     A[:, None, i, 2] * X[None, :, 2]) + tt[:, None, i] for i in range(3)], -1)

            pu, pv = project(P.cam1, tf(sR[sl], t[sl], P.p2c))
            d0, d1 = u1[None] - pu, v1[None] - pv
            e1 = d0 * d0 + d1 * d1
            pu, pv = project(P.cam2, tf(sRi[sl], ti[sl], P.p1c))
            d0, d1 = pu - u2[None], pv - v2[None]
            e2 = d0 * d0 + d1 * d1
            inl[sl] = (e1 < P.max_err1[None]) & (e2 < P.max_err2[None])
            ratio1[sl] = e1.astype(np.float64) / P.max_err1[None]
            ratio2[sl] = e2.astype(np.float64) / P.max_err2[None]
    return Evaluation(inl.sum(1).astype(np.int32), inl, R, t, s, ratio1, ratio2, gap)


class Solver:
    """The sequential part of Sim3Solver over the hypotheses of ``E`` (hypothesis h is what iteration
    h + 1 draws and evaluates)."""

    def __init__(self, P, E: Evaluation, prob=0.99, max_its=None):
        self.P, self.E = P, E
        self.N = len(P.p1c)
        self.mRansacMinInliers = int(P.min_inliers)
        # the fixtures give H = mRansacMaxIts directly
        self.mRansacMaxIts = len(P.samples) if max_its is None else max_its
        self.mnIterations = 0
        self.mnBestInliers = 0
        self.best = -1
        self.mBestT12 = np.eye(4, dtype=F)

    def T12(self, h):
        T = np.eye(4, dtype=F)
        T[:3, :3] = self.E.s[h] * self.E.R[h]
        T[:3, 3] = self.E.t[h]
        return T

    def iterate(self, nIterations, second_overload=True):
        """-> (matrix, bNoMore, inlier flags over the N matches, nInliers, bConverge)."""
        bNoMore, bConverge = False, False
        vb = np.zeros(self.N, bool)
        if self.N < self.mRansacMinInliers:
            return np.eye(4, dtype=F), True, vb, 0, False
        nCurrent = 0
        bestSim3 = None
        while self.mnIterations < self.mRansacMaxIts and nCurrent < nIterations:
            nCurrent += 1
            h = self.mnIterations
            self.mnIterations += 1
            n = int(self.E.counts[h])
            if n >= self.mnBestInliers:
                self.mnBestInliers = n
                self.best = h
                self.mBestT12 = self.T12(h)
                if n > self.mRansacMinInliers:
                    return self.mBestT12, False, self.E.inlier[h].copy(), n, True
                bestSim3 = self.mBestT12
        if self.mnIterations >= self.mRansacMaxIts:
            bNoMore = True
        if not second_overload:
            return np.eye(4, dtype=F), bNoMore, vb, 0, False
        # the reference returns an uninitialised matrix when the window brought no new best
        return (bestSim3 if bestSim3 is not None else self.mBestT12), bNoMore, vb, 0, bConverge

    def find(self):
        return self.iterate(self.mRansacMaxIts, second_overload=False)


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
    s: float


def solve(P, E=None) -> Outcome:
    """find() on a fresh solver, as osg_sim3_ransac reports it."""
    n = len(P.p1c)
    if n == 0 or n < P.min_inliers:
        return Outcome(False, -1, 0, 0, 0, np.zeros(n, bool), np.eye(3, dtype=F), np.zeros(3, F), 1.0)
    E = E if E is not None else evaluate(P)
    S = Solver(P, E)
    _, _, _, nin, conv = S.find()
    h = S.best
    return Outcome(conv, h, S.mnIterations, nin, S.mnBestInliers, E.inlier[h].copy(), E.R[h], E.t[h], float(E.s[h]))


def replay_window(counts, n_hyp, min_inliers, start, window, n_best):
    """One iterate(window) call on counts alone -> (converged, no_more, hyp, n_iterations, n_best): what
    csrc/sim3ransac_select.h must return."""
    it, cur, hyp, conv = start, 0, -1, False
    while it < n_hyp and cur < window:
        cur += 1
        n = counts[it]
        h = it
        it += 1
        if n >= n_best:
            n_best = n
            hyp = h
            if n > min_inliers:
                conv = True
                break
    no_more = (not conv) and it >= n_hyp
    return int(conv), int(no_more), hyp, it, int(n_best)


def nudged(P, rng, k):
    """Replica k of a problem: every point coordinate moved by -1, 0 or +1 float ulp; odd k evaluate the
    Horn solve in float64 with eigh.  -> (problem, horn64)."""
    def mv(a):
        d = rng.integers(-1, 2, a.shape)
        up = np.nextafter(a, F(np.inf))
        dn = np.nextafter(a, F(-np.inf))
        return np.where(d > 0, up, np.where(d < 0, dn, a)).astype(F)
    return replace(P, p1c=mv(P.p1c), p2c=mv(P.p2c)), bool(k % 2)
