"""IMU preintegration: ``IMU::Preintegrated`` (ref:src/ImuTypes.cc) over batches of measurement lists on the GPU
(csrc/preintegrate.hip) and the host rules of ``Tracking::PreintegrateIMU`` / ``PredictStateIMU`` around it
(include/osg_imu.h).  ``Reintegrate``, ``MergePrevious`` and Tracking's two running states are all
``preintegrate_batch`` with different arguments."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field

import numpy as np

from . import Context, _abi, load_library
from .optimizer import Preintegrated

WAVES_PER_WORKGROUP = 4   # IMU_W of csrc/preintegrate.hip: preintegrations per workgroup, one wave each
_M3 = ("dR", "JRg", "JVg", "JVa", "JPg", "JPa")


def _p(a):
    return a.ctypes.data if a is not None and a.size else None


def calib_cov(ng, na, ngw, naw):
    """``IMU::Calib::Set`` (ref:src/ImuTypes.cc:564-579): the diagonals of Cov and CovWalk, squared in float."""
    f = np.float32
    ng2, na2, ngw2, naw2 = f(ng) * f(ng), f(na) * f(na), f(ngw) * f(ngw), f(naw) * f(naw)
    return np.array([ng2] * 3 + [na2] * 3, f), np.array([ngw2] * 3 + [naw2] * 3, f)


@dataclass
class PreintegratedState:
    """``IMU::Preintegrated``: the float32 fields the device integrates, and the host-side members that travel
    with them (``bu``, ``mvMeasurements``, the noise diagonals)."""
    dR: np.ndarray
    dV: np.ndarray
    dP: np.ndarray
    JRg: np.ndarray
    JVg: np.ndarray
    JVa: np.ndarray
    JPg: np.ndarray
    JPa: np.ndarray
    b: np.ndarray             # the bias of the integration: (bax, bay, baz, bwx, bwy, bwz)
    dT: np.float32
    C: np.ndarray             # 15 x 15
    avgA: np.ndarray
    avgW: np.ndarray
    bu: np.ndarray = None     # the updated bias (SetNewBias); b until then
    meas: np.ndarray = field(default_factory=lambda: np.zeros((0, 7), np.float32))  # mvMeasurements
    nga: np.ndarray = None
    nga_walk: np.ndarray = None

    def __post_init__(self):
        for k in _M3:
            setattr(self, k, np.ascontiguousarray(getattr(self, k), np.float32).reshape(3, 3))
        for k in ("dV", "dP", "avgA", "avgW"):
            setattr(self, k, np.ascontiguousarray(getattr(self, k), np.float32).reshape(3))
        self.b = np.ascontiguousarray(self.b, np.float32).reshape(6)
        self.bu = self.b.copy() if self.bu is None else np.ascontiguousarray(self.bu, np.float32).reshape(6)
        self.dT = np.float32(self.dT)
        self.C = np.ascontiguousarray(self.C, np.float32).reshape(15, 15)
        self.meas = np.ascontiguousarray(self.meas, np.float32).reshape(-1, 7)

    def struct(self):
        st = _abi.OsgImuPreintegrated()
        for k in _M3 + ("dV", "dP", "b", "C"):
            C.memmove(getattr(st.pre, k), getattr(self, k).ctypes.data, getattr(self, k).nbytes)
        st.pre.dT = float(self.dT)
        C.memmove(st.avgA, self.avgA.ctypes.data, 12)
        C.memmove(st.avgW, self.avgW.ctypes.data, 12)
        return st

    @staticmethod
    def of(st, **host):
        q = st.pre
        g = lambda a: np.frombuffer(a, np.float32).copy()  # noqa: E731
        return PreintegratedState(g(q.dR), g(q.dV), g(q.dP), g(q.JRg), g(q.JVg), g(q.JVa), g(q.JPg), g(q.JPa),
                                  g(q.b), np.float32(q.dT), g(q.C), g(st.avgA), g(st.avgW), **host)

    def to_pio(self) -> Preintegrated:
        """What ``EdgeInertial`` reads: the input of ``Optimizer.PoseInertialOptimization*``."""
        return Preintegrated(self.dR, self.dV, self.dP, self.JRg, self.JVg, self.JVa, self.JPg, self.JPa, self.b,
                             self.dT, self.C)

    def set_new_bias(self, bu):
        """``SetNewBias``: only ``bu`` moves; ``delta(state, state.bu)`` gives the ``GetUpdated*`` forms."""
        self.bu = np.ascontiguousarray(bu, np.float32).reshape(6).copy()


@dataclass
class ImuProblem:
    """One integration: ``meas`` (n x 7: ax ay az wx wy wz dt) onto ``init`` or onto ``Initialize(bias)``."""
    meas: np.ndarray
    bias: np.ndarray = None   # (ba, bg); read when init is None
    nga: np.ndarray = None    # diagonal of Calib::Cov; defaults to init's
    nga_walk: np.ndarray = None
    init: PreintegratedState | None = None

    def __post_init__(self):
        m = np.asarray(self.meas)
        # a float32 C-contiguous array is used in place, so that two problems can share one list
        self.meas = m.reshape(-1, 7) if m.dtype == np.float32 and m.flags.c_contiguous else \
            np.ascontiguousarray(m, np.float32).reshape(-1, 7)
        if self.init is not None:
            self.nga = self.init.nga if self.nga is None else self.nga
            self.nga_walk = self.init.nga_walk if self.nga_walk is None else self.nga_walk
            self.bias = self.init.b if self.bias is None else self.bias
        self.bias = np.ascontiguousarray(self.bias, np.float32).reshape(6)
        self.nga = np.ascontiguousarray(self.nga, np.float32).reshape(6)
        self.nga_walk = np.ascontiguousarray(self.nga_walk, np.float32).reshape(6)

    @property
    def n(self):
        return len(self.meas)

    def struct(self, keep):
        st = _abi.OsgImuProblem()
        st.meas, st.n = _p(self.meas), self.n
        st.bias[:], st.nga[:], st.nga_walk[:] = self.bias.tolist(), self.nga.tolist(), self.nga_walk.tolist()
        if self.init is not None:
            s0 = self.init.struct()
            keep.append(s0)
            st.init = C.addressof(s0)
        return st


def preintegrate_batch(ctx: Context, problems) -> list:
    """B independent integrations in one launch."""
    nb = len(problems)
    keep = []
    ps = (_abi.OsgImuProblem * max(1, nb))(*[q.struct(keep) for q in problems])
    out = (_abi.OsgImuPreintegrated * max(1, nb))()
    ctx.check(ctx.lib.osg_imu_preintegrate_batch(ctx.handle, ps, nb, out), "IMU preintegration")
    res = []
    for q, o in zip(problems, out[:nb]):
        before = q.init.meas if q.init is not None else np.zeros((0, 7), np.float32)
        res.append(PreintegratedState.of(o, meas=np.concatenate([before, q.meas]), nga=q.nga.copy(),
                                         nga_walk=q.nga_walk.copy(),
                                         bu=None if q.init is None else q.init.bu))
    return res


def preintegrate(ctx: Context, meas, bias=None, nga=None, nga_walk=None, init=None) -> PreintegratedState:
    q = ImuProblem(meas, bias, nga, nga_walk, init)
    keep = []
    st = q.struct(keep)
    out = _abi.OsgImuPreintegrated()
    ctx.check(ctx.lib.osg_imu_preintegrate(ctx.handle, st, out), "IMU preintegration")
    before = init.meas if init is not None else np.zeros((0, 7), np.float32)
    return PreintegratedState.of(out, meas=np.concatenate([before, q.meas]), nga=q.nga.copy(),
                                 nga_walk=q.nga_walk.copy(), bu=None if init is None else init.bu)


def reintegrate(ctx: Context, states, new_biases=None) -> list:
    """``Reintegrate()`` of every state in one launch: ``Initialize(bu)`` plus its whole list.  ``new_biases``
    (one (ba, bg) per state) stands for a ``SetNewBias`` before it."""
    bus = [s.bu for s in states] if new_biases is None else list(new_biases)
    return preintegrate_batch(ctx, [ImuProblem(s.meas, bu, s.nga, s.nga_walk) for s, bu in zip(states, bus)])


def merge_previous(ctx: Context, prev: PreintegratedState, cur: PreintegratedState) -> PreintegratedState:
    """``cur.MergePrevious(prev)``: ``Initialize(cur.bu)`` plus prev's list followed by cur's."""
    if prev is cur:
        return cur
    return preintegrate(ctx, np.concatenate([prev.meas, cur.meas]), cur.bu, cur.nga, cur.nga_walk)


def check(problem: ImuProblem) -> int:
    """``osg_imu_preintegrate_check``: 0 or OSG_E_INVALID; needs no context."""
    keep = []   # what the struct points into, alive across the call
    return load_library().osg_imu_preintegrate_check(problem.struct(keep))


# ---------------------------------------------------------------------------------------------- host rules
def select_imu(t_queue, t_prev, t_cur, imu_per=0.001):
    """The queue rule of ``Tracking::PreintegrateIMU``: the indices taken into mvImuFromLastFrame and how many
    entries leave the queue's front."""
    t = np.ascontiguousarray(t_queue, np.float64)
    taken = np.zeros(max(1, len(t)), np.int32)
    popped = C.c_int32(0)
    n = load_library().osg_imu_select(_p(t), len(t), float(t_prev), float(t_cur), float(imu_per), taken.ctypes.data,
                                      C.addressof(popped))
    if n < 0:
        raise ValueError("osg_imu_select: invalid argument")
    return taken[:n].copy(), int(popped.value)


def integrables_from_imu(a, w, t, t_prev, t_cur) -> np.ndarray:
    """m IMU points between two frames -> the m - 1 steps (n x 7 float32) ``IntegrateNewMeasurement`` receives."""
    a = np.ascontiguousarray(a, np.float32).reshape(-1, 3)
    w = np.ascontiguousarray(w, np.float32).reshape(-1, 3)
    t = np.ascontiguousarray(t, np.float64)
    m = len(t)
    out = np.zeros((max(0, m - 1), 7), np.float32)
    n = load_library().osg_imu_integrables(a.ctypes.data, w.ctypes.data, t.ctypes.data, m, float(t_prev),
                                           float(t_cur), out.ctypes.data)
    if n < 0:
        raise ValueError("osg_imu_integrables: invalid argument")
    return out


def delta(state: PreintegratedState, bias):
    """``GetDeltaRotation / Velocity / Position(bias)``; ``bias = state.bu`` gives the ``GetUpdated*`` forms."""
    b = np.ascontiguousarray(bias, np.float32).reshape(6)
    dR, dV, dP = np.zeros((3, 3), np.float32), np.zeros(3, np.float32), np.zeros(3, np.float32)
    load_library().osg_imu_delta(state.struct(), b.ctypes.data, dR.ctypes.data, dV.ctypes.data, dP.ctypes.data)
    return dR, dV, dP


def predict_state(state: PreintegratedState, bias, Rwb, twb, v):
    """``Tracking::PredictStateIMU``: from the last KeyFrame with mpImuPreintegratedFromLastKF when the map was
    updated, from the last frame with mpImuPreintegratedFrame when it was not."""
    b = np.ascontiguousarray(bias, np.float32).reshape(6)
    R1 = np.ascontiguousarray(Rwb, np.float32).reshape(3, 3)
    t1, v1 = (np.ascontiguousarray(x, np.float32).reshape(3) for x in (twb, v))
    R2, t2, v2 = np.zeros((3, 3), np.float32), np.zeros(3, np.float32), np.zeros(3, np.float32)
    load_library().osg_imu_predict_state(state.struct(), b.ctypes.data, R1.ctypes.data, t1.ctypes.data,
                                         v1.ctypes.data, R2.ctypes.data, t2.ctypes.data, v2.ctypes.data)
    return R2, t2, v2
