"""numpy float32 restatement of ``IMU::Preintegrated`` (ref:src/ImuTypes.cc:38-151, 206-456, ref:include/ImuTypes.h)
and of the host rules of ``Tracking::PreintegrateIMU`` / ``PredictStateIMU`` (ref:src/Tracking.cc:1792-1901,
1945-1988): the checker of csrc/preintegrate.hip and csrc/imu_common.h.  Written from the reference, not from the
kernel: one object with the reference's fields, its statements in their order, every operation rounded to float32,
dense 9 x 9 and 9 x 6 matrices with the inner sums in ascending k, ``NormalizeRotation`` by LAPACK's SVD.

``Variant`` switches the replicas of tools/preintegration_margins.py; the default is the restatement itself."""
from dataclasses import dataclass

import numpy as np

from tests.pyref_poseinertial import so3f_exp_matrix

f = np.float32
EPS = f(1e-4)                 # ref:src/ImuTypes.cc:31
GRAVITY_VALUE = f(9.81)
QUANTITIES = ("rot_rad", "dV", "dP", "avgA", "avgW", "JRg_rel", "JVg_rel", "JVa_rel", "JPg_rel", "JPa_rel", "C_rel")


@dataclass
class Variant:
    fma: bool = False            # every product-add contracted: accumulated in float64, rounded once
    reverse_sums: bool = False   # the inner sums back to front
    trig_ulp: int = 0            # sin / cos moved by this many ulp
    polar: bool = False          # NormalizeRotation by the polar factor (eigh of R'R in double) instead of the SVD


V = Variant()


def _ulp(x):
    for _ in range(abs(V.trig_ulp)):
        x = np.nextafter(f(x), f(np.inf if V.trig_ulp > 0 else -np.inf))
    return f(x)


def mad(a, b, c):
    """a + b * c, contracted in the fma replica"""
    a, b, c = (np.asarray(x, f) for x in (a, b, c))
    if V.fma:
        return (a.astype(np.float64) + b.astype(np.float64) * c.astype(np.float64)).astype(f)
    return a + b * c


def mm(A, B):
    """A B with each inner sum in ascending k, every product and every add rounded to float32"""
    A, B = np.asarray(A, f), np.asarray(B, f)
    if B.ndim == 1:
        return mm(A, B.reshape(-1, 1)).reshape(-1)
    ks = range(A.shape[1] - 1, -1, -1) if V.reverse_sums else range(A.shape[1])
    s = None
    for k in ks:
        s = A[:, k:k + 1] * B[k:k + 1, :] if s is None else mad(s, A[:, k:k + 1], B[k:k + 1, :])
    return s


def hat(v):
    z = f(0)
    return np.array([[z, -v[2], v[1]], [v[2], z, -v[0]], [-v[1], v[0], z]], f)


def NormalizeRotation(R):
    R = np.asarray(R, f)
    if V.polar:
        w, Q = np.linalg.eigh((R.T.astype(np.float64) @ R.astype(np.float64)))
        return (R.astype(np.float64) @ (Q / np.sqrt(w)) @ Q.T).astype(f)
    U, _, Vt = np.linalg.svd(R)
    return mm(U.astype(f), Vt.astype(f))


class IntegratedRotation:
    """ref:src/ImuTypes.cc:124-151"""

    def __init__(self, angVel, bg, time):
        x = f((angVel[0] - bg[0]) * time)
        y = f((angVel[1] - bg[1]) * time)
        z = f((angVel[2] - bg[2]) * time)
        d2 = mad(mad(x * x, y, y), z, z)
        d = f(np.sqrt(d2))
        self.d = d
        W = hat((x, y, z))
        I = np.eye(3, dtype=f)
        if d < EPS:
            self.deltaR = I + W
            self.rightJ = I.copy()
        else:
            sd, cd = _ulp(np.sin(d)), _ulp(np.cos(d))
            W2 = mm(W, W)
            self.deltaR = I + W * sd / d + W2 * (f(1.0) - cd) / d2
            self.rightJ = I - W * (f(1.0) - cd) / d2 + W2 * (d - sd) / (d2 * d)


class Preintegrated:
    """ref:include/ImuTypes.h:190-275; the bias is (bax, bay, baz, bwx, bwy, bwz), Nga and NgaWalk the diagonals"""

    def __init__(self, b, nga, nga_walk):
        self.Nga = np.asarray(nga, f).copy()
        self.NgaWalk = np.asarray(nga_walk, f).copy()
        self.ds = []          # the d of every IntegratedRotation, for the guard of the 1e-4 cut
        self.Initialize(b)

    def Initialize(self, b_):
        self.dR = np.eye(3, dtype=f)
        self.dV, self.dP = np.zeros(3, f), np.zeros(3, f)
        self.JRg, self.JVg, self.JVa = np.zeros((3, 3), f), np.zeros((3, 3), f), np.zeros((3, 3), f)
        self.JPg, self.JPa = np.zeros((3, 3), f), np.zeros((3, 3), f)
        self.C = np.zeros((15, 15), f)
        self.db = np.zeros(6, f)
        self.b = np.asarray(b_, f).copy()
        self.bu = np.asarray(b_, f).copy()
        self.avgA, self.avgW = np.zeros(3, f), np.zeros(3, f)
        self.dT = f(0.0)
        self.mvMeasurements = []

    def Reintegrate(self):
        aux = list(self.mvMeasurements)
        self.Initialize(self.bu)
        for a, w, t in aux:
            self.IntegrateNewMeasurement(a, w, t)

    def IntegrateNewMeasurement(self, acceleration, angVel, dt):
        acceleration, angVel, dt = np.asarray(acceleration, f), np.asarray(angVel, f), f(dt)
        self.mvMeasurements.append((acceleration, angVel, dt))
        A = np.eye(9, dtype=f)
        B = np.zeros((9, 6), f)
        acc = acceleration - self.b[:3]
        accW = angVel - self.b[3:]
        dR, dT = self.dR, self.dT
        self.avgA = mad(dT * self.avgA, mm(dR, acc), dt) / (dT + dt)
        self.avgW = mad(dT * self.avgW, accW, dt) / (dT + dt)
        self.dP = mad(self.dP, self.dV, dt) + mm(f(0.5) * dR, acc) * dt * dt
        self.dV = mad(self.dV, mm(dR, acc), dt)
        Wacc = hat(acc)
        A[3:6, 0:3] = mm(-dR * dt, Wacc)
        A[6:9, 0:3] = mm(f(-0.5) * dR * dt * dt, Wacc)
        A[6:9, 3:6] = np.diag(np.array([dt, dt, dt], f))
        B[3:6, 3:6] = dR * dt
        B[6:9, 3:6] = f(0.5) * dR * dt * dt
        self.JPa = mad(self.JPa, self.JVa, dt) - f(0.5) * dR * dt * dt
        self.JPg = mad(self.JPg, self.JVg, dt) - mm(mm(f(0.5) * dR * dt * dt, Wacc), self.JRg)
        self.JVa = self.JVa - dR * dt
        self.JVg = self.JVg - mm(mm(dR * dt, Wacc), self.JRg)
        dRi = IntegratedRotation(angVel, self.b[3:], dt)
        self.ds.append(float(dRi.d))
        self.dR = NormalizeRotation(mm(dR, dRi.deltaR))
        A[0:3, 0:3] = dRi.deltaR.T
        B[0:3, 0:3] = dRi.rightJ * dt
        self.C[0:9, 0:9] = mm(mm(A, self.C[0:9, 0:9]), A.T) + mm(B * self.Nga[None, :], B.T)
        self.C[9:15, 9:15] += np.diag(self.NgaWalk)
        self.JRg = mm(dRi.deltaR.T, self.JRg) - dRi.rightJ * dt
        self.dT = f(self.dT + dt)

    def MergePrevious(self, pPrev):
        if pPrev is self:
            return
        bav = self.bu.copy()
        aux1, aux2 = list(pPrev.mvMeasurements), list(self.mvMeasurements)
        self.Initialize(bav)
        for a, w, t in aux1 + aux2:
            self.IntegrateNewMeasurement(a, w, t)

    def SetNewBias(self, bu_):
        self.bu = np.asarray(bu_, f).copy()
        self.db = np.concatenate([self.bu[3:] - self.b[3:], self.bu[:3] - self.b[:3]])

    def GetDeltaRotation(self, b_):
        dbg = np.asarray(b_, f)[3:] - self.b[3:]
        return NormalizeRotation(mm(self.dR, so3f_exp_matrix(mm(self.JRg, dbg))))

    def GetDeltaVelocity(self, b_):
        b_ = np.asarray(b_, f)
        return self.dV + mm(self.JVg, b_[3:] - self.b[3:]) + mm(self.JVa, b_[:3] - self.b[:3])

    def GetDeltaPosition(self, b_):
        b_ = np.asarray(b_, f)
        return self.dP + mm(self.JPg, b_[3:] - self.b[3:]) + mm(self.JPa, b_[:3] - self.b[:3])


def integrate(meas, bias, nga, nga_walk, init=None):
    """The device call's contract: the list onto ``init`` (a Preintegrated, continued in place of a copy) or onto
    ``Initialize(bias)``."""
    p = Preintegrated(bias, nga, nga_walk) if init is None else init
    for row in np.asarray(meas, f).reshape(-1, 7):
        p.IntegrateNewMeasurement(row[0:3], row[3:6], row[6])
    return p


# ------------------------------------------------------------------------------------- Tracking's host rules
def select(t_queue, t_prev, t_cur, imu_per=0.001):
    """ref:src/Tracking.cc:1792-1829 on the queue's timestamps: (indices taken, entries popped)"""
    taken, at = [], 0
    while at < len(t_queue):
        if t_queue[at] < t_prev - imu_per:
            at += 1
        elif t_queue[at] < t_cur - imu_per:
            taken.append(at)
            at += 1
        else:
            taken.append(at)
            break
    return taken, at


def integrables(a, w, t, t_prev, t_cur):
    """ref:src/Tracking.cc:1851-1901: timestamps double; tab, tini, tend, tstep rounded to float"""
    a, w, t = np.asarray(a, f).reshape(-1, 3), np.asarray(w, f).reshape(-1, 3), np.asarray(t, np.float64)
    n = len(t) - 1
    out = np.zeros((max(n, 0), 7), f)
    for i in range(n):
        if i == 0 and i < n - 1:
            tab, tini = f(t[i + 1] - t[i]), f(t[i] - t_prev)
            acc = (a[i] + a[i + 1] - (a[i + 1] - a[i]) * f(tini / tab)) * f(0.5)
            ang = (w[i] + w[i + 1] - (w[i + 1] - w[i]) * f(tini / tab)) * f(0.5)
            tstep = f(t[i + 1] - t_prev)
        elif i < n - 1:
            acc = (a[i] + a[i + 1]) * f(0.5)
            ang = (w[i] + w[i + 1]) * f(0.5)
            tstep = f(t[i + 1] - t[i])
        elif i > 0 and i == n - 1:
            tab, tend = f(t[i + 1] - t[i]), f(t[i + 1] - t_cur)
            acc = (a[i] + a[i + 1] - (a[i + 1] - a[i]) * f(tend / tab)) * f(0.5)
            ang = (w[i] + w[i + 1] - (w[i + 1] - w[i]) * f(tend / tab)) * f(0.5)
            tstep = f(t_cur - t[i])
        else:
            acc, ang = a[i], w[i]
            tstep = f(t_cur - t_prev)
        out[i, 0:3], out[i, 3:6], out[i, 6] = acc, ang, tstep
    return out


def predict_state(pre, bias, Rwb1, twb1, Vwb1):
    """ref:src/Tracking.cc:1945-1988, either branch: the caller chooses the KeyFrame's or the frame's inputs"""
    Rwb1, twb1, Vwb1 = np.asarray(Rwb1, f), np.asarray(twb1, f), np.asarray(Vwb1, f)
    Gz = np.array([0, 0, -GRAVITY_VALUE], f)
    t12 = pre.dT
    Rwb2 = NormalizeRotation(mm(Rwb1, pre.GetDeltaRotation(bias)))
    twb2 = twb1 + Vwb1 * t12 + f(0.5) * t12 * t12 * Gz + mm(Rwb1, pre.GetDeltaPosition(bias))
    Vwb2 = Vwb1 + t12 * Gz + mm(Rwb1, pre.GetDeltaVelocity(bias))
    return Rwb2, twb2, Vwb2


# ------------------------------------------------------------------------------------- comparison
def rot_angle(Ra, Rb):
    M = np.asarray(Ra, np.float64) @ np.asarray(Rb, np.float64).T
    w = np.array([M[2, 1] - M[1, 2], M[0, 2] - M[2, 0], M[1, 0] - M[0, 1]]) / 2
    return float(np.arctan2(np.linalg.norm(w), (np.trace(M) - 1) / 2))


def differences(got, ref):
    """The tolerance-compared quantities; ``got`` and ``ref`` carry the reference's field names."""
    d = {"rot_rad": rot_angle(got.dR, ref.dR)}
    for k in ("dV", "dP", "avgA", "avgW"):
        d[k] = float(np.max(np.abs(np.asarray(getattr(got, k), np.float64) - getattr(ref, k))))
    for k in ("JRg", "JVg", "JVa", "JPg", "JPa"):
        a, b = np.asarray(getattr(got, k), np.float64), np.asarray(getattr(ref, k), np.float64)
        top = np.max(np.abs(b))
        d[k + "_rel"] = float(np.max(np.abs(a - b)) / top) if top > 0 else float(np.max(np.abs(a)))
    Cg, Cr = np.asarray(got.C, np.float64)[:9, :9], np.asarray(ref.C, np.float64)[:9, :9]
    s = np.sqrt(np.abs(np.diag(Cr)))
    den = np.outer(s, s)
    ok = den > 0
    d["C_rel"] = float(np.max(np.abs(Cg - Cr)[ok] / den[ok])) if ok.any() else 0.0
    if (~ok).any() and np.any(Cg[~ok] != Cr[~ok]):
        d["C_rel"] = float("inf")   # an entry whose variances are zero must be equal
    return d


def exact_mismatches(got, ref):
    """What does not depend on contraction or sum order, bit for bit: dT, b, C[9:15, 9:15], the zero blocks"""
    bad = []
    Cg, Cr = np.asarray(got.C, f), np.asarray(ref.C, f)
    if f(got.dT).tobytes() != f(ref.dT).tobytes():
        bad.append(("dT", float(got.dT), float(ref.dT)))
    if np.asarray(got.b, f).tobytes() != np.asarray(ref.b, f).tobytes():
        bad.append(("b",))
    if Cg[9:, 9:].tobytes() != Cr[9:, 9:].tobytes():
        bad.append(("C_walk",))
    if Cg[:9, 9:].tobytes() != Cr[:9, 9:].tobytes() or Cg[9:, :9].tobytes() != Cr[9:, :9].tobytes():
        bad.append(("C_zero",))
    return bad


def cut_margin(ds):
    """The smallest relative distance of any step's d from the 1e-4 cut (None for an empty list)"""
    if not len(ds):
        return None
    return float(np.min(np.abs(np.asarray(ds, np.float64) - float(EPS)) / float(EPS)))
