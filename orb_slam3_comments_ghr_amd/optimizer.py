"""Host mirror of ``ORB_SLAM3::Optimizer::PoseOptimization`` / ``LocalBundleAdjustment``
(ref:include/Optimizer.h:55,77) on the C ABI in include/osg_ba.h, plus the seeded synthetic
problems of SURVEY.md §8d (C3 PoseOptimization, C4 LocalBA 50 KF x 10k points).

The graph gathering that the reference does from Frame / KeyFrame / MapPoint (window selection,
vertex ids, edge insertion order, float->double casts) is the adapter's job; here a problem is
given directly as those arrays.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field, replace

import numpy as np

from . import Context, _abi
from .synth import EUROC_BF, EUROC_CX, EUROC_CY, EUROC_FX, EUROC_FY, EUROC_H, EUROC_W


def _p(a):
    return None if a is None else int(a.ctypes.data)


def pinhole_camera(fx=EUROC_FX, fy=EUROC_FY, cx=EUROC_CX, cy=EUROC_CY, bf=EUROC_BF, trl=None):
    c = _abi.OsgCamera()
    c.type = _abi.CAM_PINHOLE
    for i, v in enumerate([fx, fy, cx, cy, 0, 0, 0, 0]):
        c.p[i] = v
    c.fx, c.fy, c.cx, c.cy, c.bf = fx, fy, cx, cy, bf
    t = trl if trl is not None else [0, 0, 0, 1, 0, 0, 0]
    for i in range(7):
        c.trl[i] = t[i]
    return c


def kb8_camera(fx=190.98, fy=190.97, cx=254.93, cy=256.90, k=(3.48e-3, 7.15e-4, -2.05e-3, 2.03e-4), trl=None):
    c = _abi.OsgCamera()
    c.type = _abi.CAM_KB8
    for i, v in enumerate([fx, fy, cx, cy, *k]):
        c.p[i] = v
    c.fx, c.fy, c.cx, c.cy, c.bf = fx, fy, cx, cy, 0.0
    t = trl if trl is not None else [0, 0, 0, 1, 0, 0, 0]
    for i in range(7):
        c.trl[i] = t[i]
    return c


# ----------------------------------------------------------------------------- geometry helpers
def rot_to_quat(m):
    """Eigen Quaternion(Matrix3) (trace method), coeffs (x, y, z, w)."""
    q = np.zeros(4)
    t = m[0, 0] + m[1, 1] + m[2, 2]
    if t > 0:
        s = np.sqrt(t + 1.0)
        q[3] = 0.5 * s
        s = 0.5 / s
        q[0] = (m[2, 1] - m[1, 2]) * s
        q[1] = (m[0, 2] - m[2, 0]) * s
        q[2] = (m[1, 0] - m[0, 1]) * s
    else:
        i = 0
        if m[1, 1] > m[0, 0]:
            i = 1
        if m[2, 2] > m[i, i]:
            i = 2
        j, k = (i + 1) % 3, (i + 2) % 3
        s = np.sqrt(m[i, i] - m[j, j] - m[k, k] + 1.0)
        q[i] = 0.5 * s
        s = 0.5 / s
        q[3] = (m[k, j] - m[j, k]) * s
        q[j] = (m[j, i] + m[i, j]) * s
        q[k] = (m[k, i] + m[i, k]) * s
    if q[3] < 0:
        q = -q
    return q / np.linalg.norm(q)


def quat_to_rot(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def look_at(center, target, up=(0, -1, 0)):
    """Tcw (world->camera) for a camera at `center` looking at `target` (z forward, y down)."""
    z = np.asarray(target, float) - np.asarray(center, float)
    z /= np.linalg.norm(z)
    x = np.cross(np.asarray(up, float), z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    Rcw = np.stack([x, y, z])
    tcw = -Rcw @ np.asarray(center, float)
    return Rcw, tcw


def small_rotation(rng, deg):
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    a = np.deg2rad(deg) * rng.normal()
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * K @ K


def pose7(R, t):
    """Sophus SE3f -> g2o SE3Quat as the reference does: float quaternion / translation cast to
    double (ref:src/Optimizer.cc:97)."""
    q = rot_to_quat(R).astype(np.float32).astype(np.float64)
    return np.concatenate([q, np.asarray(t, np.float32).astype(np.float64)])


def inv_level_sigma2(n_levels=8, factor=1.2):
    s = np.ones(n_levels, np.float32)
    for i in range(1, n_levels):
        s[i] = np.float32(s[i - 1] * np.float32(factor))
    return (np.float32(1.0) / (s * s)).astype(np.float32)


# ----------------------------------------------------------------------------- problem containers
@dataclass
class PoseProblem:
    pose: np.ndarray          # 7 doubles (q xyzw, t)
    kind: np.ndarray          # int8 per edge
    xw: np.ndarray            # n x 3 double
    obs: np.ndarray           # n x 3 double
    inv_sigma2: np.ndarray    # float32 per edge
    cam: object = field(default_factory=pinhole_camera)
    cam2: object = field(default_factory=pinhole_camera)

    def __post_init__(self):
        self.pose = np.ascontiguousarray(self.pose, np.float64)
        self.kind = np.ascontiguousarray(self.kind, np.int8)
        self.xw = np.ascontiguousarray(self.xw, np.float64).reshape(-1, 3)
        self.obs = np.ascontiguousarray(self.obs, np.float64).reshape(-1, 3)
        self.inv_sigma2 = np.ascontiguousarray(self.inv_sigma2, np.float32)

    @property
    def n(self):
        return len(self.kind)

    def struct(self):
        s = _abi.OsgPoseProblem()
        for i in range(7):
            s.pose[i] = float(self.pose[i])
        s.n_edges = self.n
        s.kind, s.xw, s.obs, s.inv_sigma2 = _p(self.kind), _p(self.xw), _p(self.obs), _p(self.inv_sigma2)
        s.cam = self.cam
        s.cam2 = self.cam2
        return s


@dataclass
class PoseResult:
    pose: np.ndarray
    outlier: np.ndarray
    n_inliers: int
    lm_iterations: int
    lm_trials: int


@dataclass
class BAGraph:
    pose: np.ndarray          # np x 7
    pose_fixed: np.ndarray    # np uint8
    point: np.ndarray         # npt x 3
    e_point: np.ndarray
    e_pose: np.ndarray
    e_kind: np.ndarray
    e_cam: np.ndarray
    e_obs: np.ndarray         # ne x 3
    e_inv_sigma2: np.ndarray
    cams: list
    iterations: int = 10
    user_lambda_init: float = 0.0
    e_robust: np.ndarray | None = None   # BundleAdjustment: per-edge Huber flag (None: every edge)
    huber_mono: float = 0.0              # deltas as the reference's floats (0: LocalBundleAdjustment's)
    huber_stereo: float = 0.0

    def __post_init__(self):
        self.pose = np.ascontiguousarray(self.pose, np.float64).reshape(-1, 7)
        self.pose_fixed = np.ascontiguousarray(self.pose_fixed, np.uint8)
        self.point = np.ascontiguousarray(self.point, np.float64).reshape(-1, 3)
        self.e_point = np.ascontiguousarray(self.e_point, np.int32)
        self.e_pose = np.ascontiguousarray(self.e_pose, np.int32)
        self.e_kind = np.ascontiguousarray(self.e_kind, np.int8)
        self.e_cam = np.ascontiguousarray(self.e_cam, np.int32)
        self.e_obs = np.ascontiguousarray(self.e_obs, np.float64).reshape(-1, 3)
        self.e_inv_sigma2 = np.ascontiguousarray(self.e_inv_sigma2, np.float32)
        if self.e_robust is not None:
            self.e_robust = np.ascontiguousarray(self.e_robust, np.uint8)
        self._cams = (_abi.OsgCamera * max(1, len(self.cams)))(*self.cams)

    def struct(self):
        s = _abi.OsgBaGraph()
        s.n_poses = len(self.pose)
        s.pose, s.pose_fixed = _p(self.pose), _p(self.pose_fixed)
        s.n_points = len(self.point)
        s.point = _p(self.point)
        s.n_edges = len(self.e_point)
        s.e_point, s.e_pose, s.e_kind = _p(self.e_point), _p(self.e_pose), _p(self.e_kind)
        s.e_cam, s.e_obs, s.e_inv_sigma2 = _p(self.e_cam), _p(self.e_obs), _p(self.e_inv_sigma2)
        s.n_cams = len(self.cams)
        s.cams = C.addressof(self._cams)
        s.iterations = self.iterations
        s.user_lambda_init = self.user_lambda_init
        s.e_robust = _p(self.e_robust)
        s.huber_mono, s.huber_stereo = self.huber_mono, self.huber_stereo
        return s


@dataclass
class BAResult:
    pose: np.ndarray
    point: np.ndarray
    edge_bad: np.ndarray
    iterations: int
    trials: int
    chi2_initial: float
    chi2_final: float
    aborted: int
    edge_chi2: np.ndarray | None = None   # e->chi2() of each edge's last computed error


@dataclass
class Sim3Problem:
    """One ``Optimizer::OptimizeSim3`` call as the adapter gathers it (include/osg_ba.h): the kept
    pairs in slot order, camera-frame points as float-valued doubles."""
    q: np.ndarray             # 4 doubles, g2oS12 rotation (x, y, z, w)
    t: np.ndarray             # 3 doubles
    s: float
    p1c: np.ndarray           # n x 3 double
    p2c: np.ndarray           # n x 3 double
    obs1: np.ndarray          # n x 2 double
    obs2: np.ndarray          # n x 2 double (normalised x/z, y/z for a pair that is not in KeyFrame 2)
    inv_sigma2_1: np.ndarray  # float32 per pair
    inv_sigma2_2: np.ndarray  # float32 per pair
    fix_scale: bool = False
    th2: float = 10.0         # LoopClosing passes 10 (ref:src/LoopClosing.cc:740, 1075)
    cam1: object = field(default_factory=pinhole_camera)
    cam2: object = field(default_factory=pinhole_camera)
    max_iterations: int = 0   # 0: optimize(5), optimize(5 | 10); n > 0 caps both
    truth: tuple | None = None  # generator only: the (R, t, s) the observations were drawn from

    def __post_init__(self):
        self.q = np.ascontiguousarray(self.q, np.float64)
        self.t = np.ascontiguousarray(self.t, np.float64)
        self.p1c = np.ascontiguousarray(self.p1c, np.float64).reshape(-1, 3)
        self.p2c = np.ascontiguousarray(self.p2c, np.float64).reshape(-1, 3)
        self.obs1 = np.ascontiguousarray(self.obs1, np.float64).reshape(-1, 2)
        self.obs2 = np.ascontiguousarray(self.obs2, np.float64).reshape(-1, 2)
        self.inv_sigma2_1 = np.ascontiguousarray(self.inv_sigma2_1, np.float32)
        self.inv_sigma2_2 = np.ascontiguousarray(self.inv_sigma2_2, np.float32)

    @property
    def n(self):
        return len(self.p1c)

    def struct(self):
        st = _abi.OsgSim3Problem()
        for i in range(4):
            st.q[i] = float(self.q[i])
        for i in range(3):
            st.t[i] = float(self.t[i])
        st.s = float(self.s)
        st.fix_scale = int(bool(self.fix_scale))
        st.th2 = float(self.th2)
        st.cam1, st.cam2 = self.cam1, self.cam2
        st.n_pairs = self.n
        st.p1c, st.p2c, st.obs1, st.obs2 = _p(self.p1c), _p(self.p2c), _p(self.obs1), _p(self.obs2)
        st.inv_sigma2_1, st.inv_sigma2_2 = _p(self.inv_sigma2_1), _p(self.inv_sigma2_2)
        st.max_iterations = int(self.max_iterations)
        return st


@dataclass
class Sim3Result:
    q: np.ndarray
    t: np.ndarray
    s: float
    n_inliers: int            # the reference's return value
    pair_state: np.ndarray    # 0 inlier, 1 nulled after the first optimize, 2 nulled by the final check
    n_bad_first: int
    lm_iterations: tuple
    lm_trials: tuple
    chi2_final: float
    pair_chi2: np.ndarray     # n x 2: (e12, e21) chi2 as read by the pair's last classification
    early_return: bool


@dataclass
class EssentialGraphProblem:
    """One ``Optimizer::OptimizeEssentialGraph`` call as the adapter gathers it (include/osg_ba.h): the
    non-bad KeyFrames in the caller's order, the edges in the reference's insertion order."""
    sim3: np.ndarray          # n x 8 double: q (x, y, z, w), t, s  (vScw)
    fixed: np.ndarray         # n uint8
    e_v0: np.ndarray          # E int32, vertex(0) = i
    e_v1: np.ndarray          # E int32, vertex(1) = j
    e_meas: np.ndarray        # E x 8 double, Sji
    fix_scale: bool = False
    max_iterations: int = 0   # 0: the reference's 20
    lambda_init: float = 1e-16
    truth: np.ndarray | None = None  # generator only (consistent=True): the Sim3s the measurements were built from

    def __post_init__(self):
        self.sim3 = np.ascontiguousarray(self.sim3, np.float64).reshape(-1, 8)
        self.fixed = np.ascontiguousarray(self.fixed, np.uint8)
        self.e_v0 = np.ascontiguousarray(self.e_v0, np.int32)
        self.e_v1 = np.ascontiguousarray(self.e_v1, np.int32)
        self.e_meas = np.ascontiguousarray(self.e_meas, np.float64).reshape(-1, 8)

    @property
    def n(self):
        return len(self.sim3)

    @property
    def n_edges(self):
        return len(self.e_v0)

    def struct(self):
        st = _abi.OsgEssGraphProblem()
        st.n_vertices, st.sim3, st.fixed = self.n, _p(self.sim3), _p(self.fixed)
        st.fix_scale = int(bool(self.fix_scale))
        st.n_edges, st.e_v0, st.e_v1, st.e_meas = self.n_edges, _p(self.e_v0), _p(self.e_v1), _p(self.e_meas)
        st.max_iterations = int(self.max_iterations)
        st.lambda_init = float(self.lambda_init)
        return st


@dataclass
class EssentialGraphResult:
    sim3: np.ndarray          # n x 8, a fixed vertex bit-equal to its input
    chi2_initial: float
    chi2_final: float
    lm_iterations: int
    lm_trials: int
    edge_chi2: np.ndarray     # per edge at the returned state

    @property
    def R(self):
        q = self.sim3[:, :4] / np.linalg.norm(self.sim3[:, :4], axis=1)[:, None]
        return np.stack([quat_to_rot(v) for v in q]) if len(q) else np.zeros((0, 3, 3))

    @property
    def t(self):
        return self.sim3[:, 4:7]

    @property
    def s(self):
        return self.sim3[:, 7]


@dataclass
class EssentialGraph4DoFProblem:
    """One ``Optimizer::OptimizeEssentialGraph4DoF`` call as the adapter gathers it (include/osg_ba.h): per
    non-bad KeyFrame the ImuCamPose of its VertexPose4DoF as constructed, the edges in the reference's insertion
    order with their Tij as (dRij, dtij)."""
    pose: np.ndarray          # n x 36 double: Rwb[9] twb[3] Rcw[9] tcw[3] Rcb[9] tcb[3], matrices row-major
    fixed: np.ndarray         # n uint8
    e_v0: np.ndarray          # E int32, vertex(0) = i
    e_v1: np.ndarray          # E int32, vertex(1) = j
    e_meas: np.ndarray        # E x 12 double: dRij row-major, dtij
    info_diag: tuple = (1e3, 1e3, 1.0, 1.0, 1.0, 1.0)   # matLambda as the reference leaves it: (2, 2) stays 1
    max_iterations: int = 0   # 0: the reference's 20
    lambda_init: float = 0.0  # 0: g2o's 1e-5 max |diag H|, the reference's
    truth: np.ndarray | None = None    # generator only (consistent=True): n x 36, the poses the measurements were built from
    built: np.ndarray | None = None    # generator only: per vertex b"C" (the 3-argument constructor) or b"K" (the KeyFrame's)

    def __post_init__(self):
        self.pose = np.ascontiguousarray(self.pose, np.float64).reshape(-1, 36)
        self.fixed = np.ascontiguousarray(self.fixed, np.uint8)
        self.e_v0 = np.ascontiguousarray(self.e_v0, np.int32)
        self.e_v1 = np.ascontiguousarray(self.e_v1, np.int32)
        self.e_meas = np.ascontiguousarray(self.e_meas, np.float64).reshape(-1, 12)

    @property
    def n(self):
        return len(self.pose)

    @property
    def n_edges(self):
        return len(self.e_v0)

    def struct(self):
        st = _abi.OsgEssGraph4Problem()
        st.n_vertices, st.pose, st.fixed = self.n, _p(self.pose), _p(self.fixed)
        st.n_edges, st.e_v0, st.e_v1, st.e_meas = self.n_edges, _p(self.e_v0), _p(self.e_v1), _p(self.e_meas)
        for i in range(6):
            st.info_diag[i] = float(self.info_diag[i])
        st.max_iterations = int(self.max_iterations)
        st.lambda_init = float(self.lambda_init)
        return st


@dataclass
class EssentialGraph4DoFResult:
    pose: np.ndarray          # n x 24: Rcw[9] tcw[3] Rwb[9] twb[3]; a fixed vertex bit-equal to its input
    chi2_initial: float
    chi2_final: float
    lm_iterations: int
    lm_trials: int
    edge_chi2: np.ndarray     # per edge at the returned state

    @property
    def R(self):
        """Rcw, what the write-back reads"""
        return self.pose[:, 0:9].reshape(-1, 3, 3)

    @property
    def t(self):
        return self.pose[:, 9:12]

    @property
    def Rwb(self):
        return self.pose[:, 12:21].reshape(-1, 3, 3)

    @property
    def twb(self):
        return self.pose[:, 21:24]


def run_pose(fn, problems, handle=None):
    """Call a PoseOptimization entry point on problems: the batch API (handle given) or a
    per-problem function fn(problem_structs, result_structs)."""
    res_structs = (_abi.OsgPoseResult * len(problems))()
    outl = [np.zeros(p.n, np.uint8) for p in problems]
    for r, o in zip(res_structs, outl):
        r.outlier = _p(o)
    probs = (_abi.OsgPoseProblem * len(problems))(*[p.struct() for p in problems])
    rc = fn(probs, res_structs) if handle is None else fn(handle, probs, len(problems), res_structs)
    out = [PoseResult(np.array(list(r.pose)), o, r.n_inliers, r.lm_iterations, r.lm_trials)
           for r, o in zip(res_structs, outl)]
    return rc, out


def make_ba_result(G: BAGraph, chi2: bool = True):
    """(osg_ba_result, its output arrays): pose, point, edge_bad, edge_chi2 (None unless `chi2`: the
    per-edge chi2 is read only by the map-merge BA's level-1 marking; LocalMapping's LBA needs the
    classification alone, and each requested array is another device-to-host copy)."""
    R = _abi.OsgBaResult()
    out = (np.zeros_like(G.pose), np.zeros_like(G.point), np.zeros(len(G.e_point), np.uint8),
           np.zeros(len(G.e_point), np.float64) if chi2 else None)
    R.pose, R.point, R.edge_bad, R.edge_chi2 = (_p(a) for a in out)
    return R, out


def finish_ba_result(R, out) -> "BAResult":
    pose, point, bad, chi2 = out
    return BAResult(pose, point, bad, R.iterations, R.trials, R.chi2_initial, R.chi2_final, R.aborted, chi2)


class Optimizer:
    """``Optimizer::PoseOptimization`` / ``LocalBundleAdjustment`` on the GPU."""

    def __init__(self, ctx: Context):
        self.ctx = ctx

    def PoseOptimization(self, problems):
        """Batch form: one launch for all frames.  Returns the per-frame results (the reference's
        return value is ``n_inliers``)."""
        single = isinstance(problems, PoseProblem)
        probs = [problems] if single else list(problems)
        lib, h = self.ctx.lib, self.ctx.handle
        rc, out = run_pose(lib.osg_pose_optimization_batch, probs, handle=h)
        self.ctx.check(rc, "PoseOptimization")
        return out[0] if single else out

    def _pose_inertial(self, problems, mode):
        single = isinstance(problems, PoseInertialProblem)
        probs = [problems] if single else list(problems)
        for q in probs:
            if q.mode != mode:
                raise ValueError("a problem of the other mode")
        out = run_pose_inertial(self.ctx, probs)
        return out[0] if single else out

    def PoseInertialOptimizationLastKeyFrame(self, problems):
        """``Optimizer::PoseInertialOptimizationLastKeyFrame`` (ref:src/Optimizer.cc:435-987) for one
        PoseInertialProblem or a list of them (one launch, a workgroup per frame).  The reference's return value
        is ``n_inliers``; ``constraint_pose_imu(result.H)`` is the new frame's ``mpcpi``."""
        return self._pose_inertial(problems, _abi.OSG_PIO_LAST_KEYFRAME)

    def PoseInertialOptimizationLastFrame(self, problems):
        """``Optimizer::PoseInertialOptimizationLastFrame`` (ref:src/Optimizer.cc:1002-1640), as above; every
        problem carries the previous frame's prior."""
        return self._pose_inertial(problems, _abi.OSG_PIO_LAST_FRAME)

    def pose_inertial_optimization_mixed(self, problems):
        """A batch that mixes both modes in one launch (no reference counterpart; the C batch entry point takes
        any mixture)."""
        return run_pose_inertial(self.ctx, list(problems))

    def InertialOptimization(self, problems):
        """``Optimizer::InertialOptimization`` (ref:src/Optimizer.cc:3706-4197) for one InertialProblem or a list of
        them (one launch, a workgroup per map).  ``inertial_initialization_problem``, ``inertial_bias_problem`` and
        ``inertial_scale_refinement_problem`` set the options of the three overloads."""
        single = isinstance(problems, InertialProblem)
        out = run_inertial(self.ctx, [problems] if single else list(problems))
        return out[0] if single else out

    def LocalInertialBA(self, problems):
        """``Optimizer::LocalInertialBA`` (ref:src/Optimizer.cc:2221-2816), its g2o part, for one
        LocalInertialBAProblem or a list of them (one launch, a workgroup per window)."""
        single = isinstance(problems, LocalInertialBAProblem)
        out = run_local_inertial_ba(self.ctx, [problems] if single else list(problems))
        return out[0] if single else out

    def OptimizeSim3(self, problems):
        """``Optimizer::OptimizeSim3`` (ref:src/Optimizer.cc:4213-4512) for one Sim3Problem or a list of
        them (one launch, a workgroup per problem).  The caller nulls ``vpMatches1`` where ``pair_state``
        is nonzero and takes the Sim3 unless ``early_return``."""
        single = isinstance(problems, Sim3Problem)
        probs = [problems] if single else list(problems)
        nb = len(probs)
        ps = (_abi.OsgSim3Problem * max(1, nb))(*[p.struct() for p in probs])
        rs = (_abi.OsgSim3Result * max(1, nb))()
        state = [np.zeros(p.n, np.uint8) for p in probs]
        chi2 = [np.zeros((p.n, 2), np.float64) for p in probs]
        for r, st, c in zip(rs, state, chi2):
            r.pair_state, r.pair_chi2 = _p(st), _p(c)
        self.ctx.check(self.ctx.lib.osg_optimize_sim3_batch(self.ctx.handle, ps, nb, rs), "OptimizeSim3")
        out = [Sim3Result(np.array(list(r.q)), np.array(list(r.t)), float(r.s), r.n_inliers, st, r.n_bad_first,
                          tuple(r.lm_iterations), tuple(r.lm_trials), r.chi2_final, c, bool(r.early_return))
               for r, st, c in zip(rs, state, chi2)]
        return out[0] if single else out

    def optimize_essential_graph(self, P: EssentialGraphProblem) -> EssentialGraphResult:
        """The g2o part of ``Optimizer::OptimizeEssentialGraph`` (ref:src/Optimizer.cc:4527-4858): the Sim3 pose
        graph the adapter gathered, optimize(20) with the caller's lambda.  The caller writes the poses back
        (``SetPose(R, t / s)``) and corrects the MapPoints with ``correct_map_points``."""
        st = P.struct()
        R = _abi.OsgEssGraphResult()
        out, chi = np.zeros((P.n, 8), np.float64), np.zeros(P.n_edges, np.float64)
        R.sim3, R.edge_chi2 = _p(out), _p(chi)
        self.ctx.check(self.ctx.lib.osg_optimize_essential_graph(self.ctx.handle, C.byref(st), C.byref(R)),
                       "OptimizeEssentialGraph")
        return EssentialGraphResult(out, R.chi2_initial, R.chi2_final, R.lm_iterations, R.lm_trials, chi)

    def optimize_essential_graph_4dof(self, P: EssentialGraph4DoFProblem) -> EssentialGraph4DoFResult:
        """The g2o part of ``Optimizer::OptimizeEssentialGraph4DoF`` (ref:src/Optimizer.cc:4870-5198): the pose
        graph of an inertial map, its vertices updated in yaw and translation alone, optimize(20) with g2o's own
        lambda.  The caller writes ``Rcw``, ``tcw`` back and corrects the MapPoints with ``correct_map_points``
        (unit scales)."""
        st = P.struct()
        R = _abi.OsgEssGraph4Result()
        out, chi = np.zeros((P.n, 24), np.float64), np.zeros(P.n_edges, np.float64)
        R.pose, R.edge_chi2 = _p(out), _p(chi)
        self.ctx.check(self.ctx.lib.osg_optimize_essential_graph_4dof(self.ctx.handle, C.byref(st), C.byref(R)),
                       "OptimizeEssentialGraph4DoF")
        return EssentialGraph4DoFResult(out, R.chi2_initial, R.chi2_final, R.lm_iterations, R.lm_trials, chi)

    def correct_map_points(self, Xw, ref_vertex, sim3_before, sim3_after):
        """``correctedSwr.map(Srw.map(X))`` of every MapPoint through its reference KeyFrame's vertex
        (ref:src/Optimizer.cc:4824-4851); a point with ``ref_vertex < 0`` is copied through."""
        Xw = np.ascontiguousarray(Xw, np.float32).reshape(-1, 3)
        ref = np.ascontiguousarray(ref_vertex, np.int32)
        b = np.ascontiguousarray(sim3_before, np.float64).reshape(-1, 8)
        a = np.ascontiguousarray(sim3_after, np.float64).reshape(-1, 8)
        assert len(ref) == len(Xw) and a.shape == b.shape
        out = np.zeros_like(Xw)
        self.ctx.check(self.ctx.lib.osg_essgraph_correct_points(self.ctx.handle, len(Xw), _p(Xw), _p(ref), len(b), _p(b),
                                                                _p(a), _p(out)), "essgraph_correct_points")
        return out

    def essential_graph_kernel_times(self, enable=True):
        """(ms by phase: linearise, assemble, factor, update, chi2; matrix store bytes) of the last timed call of
        ``optimize_essential_graph`` or ``optimize_essential_graph_4dof``"""
        ms = np.zeros(6, np.float64)
        self.ctx.check(self.ctx.lib.osg_essgraph_kernel_times(self.ctx.handle, int(bool(enable)), _p(ms)), "kernel times")
        return dict(zip(["linearise", "assemble", "factor", "update", "chi2"], ms[:5].tolist())), int(ms[5])

    def LocalBundleAdjustment(self, G: BAGraph, stop_flag: np.ndarray | None = None) -> BAResult:
        lib, h = self.ctx.lib, self.ctx.handle
        R, out = make_ba_result(G, chi2=False)
        gs = G.struct()
        if stop_flag is not None:
            assert stop_flag.dtype == np.uint8, "stop flag is one byte (bool *pbStopFlag)"
        sf = None if stop_flag is None else _p(stop_flag)
        rc = lib.osg_local_bundle_adjustment(h, C.byref(gs), C.byref(R), sf)
        self.ctx.check(rc, "LocalBundleAdjustment")
        return finish_ba_result(R, out)

    def BundleAdjustment(self, G: BAGraph, stop_flag: np.ndarray | None = None) -> BAResult:
        """The g2o part of ``Optimizer::BundleAdjustment`` (global BA, ref:src/Optimizer.cc:2850-3237):
        ``G`` built as the reference builds it (``synth_gba_graph`` / the adapter), optimize(G.iterations).
        The reference reads no outlier flags after a global BA; ``edge_bad`` is informational."""
        lib, h = self.ctx.lib, self.ctx.handle
        R, out = make_ba_result(G)
        gs = G.struct()
        if stop_flag is not None:
            assert stop_flag.dtype == np.uint8, "stop flag is one byte (bool *pbStopFlag)"
        sf = None if stop_flag is None else _p(stop_flag)
        self.ctx.check(lib.osg_bundle_adjustment(h, C.byref(gs), C.byref(R), sf), "BundleAdjustment")
        return finish_ba_result(R, out)

    GlobalBundleAdjustemnt = BundleAdjustment  # the reference's spelling (ref:include/Optimizer.h)

    def LocalBundleAdjustmentMerge(self, G: BAGraph, stop_flag: np.ndarray | None = None, mp_bad=None):
        """``LocalBundleAdjustment(pMainKF, vpAdjustKF, vpFixedKF, pbStopFlag)`` — the map-merge window BA
        (ref:src/Optimizer.cc:5211-5672): two g2o passes on the GPU, see merge_local_bundle_adjustment."""
        return merge_local_bundle_adjustment(G, lambda g, s: self.BundleAdjustment(g, stop_flag=s), stop_flag, mp_bad)

    def LocalBundleAdjustmentBatch(self, graphs, stop_flag: np.ndarray | None = None) -> list:
        """B independent windows in lockstep, one launch per kernel per LM trial for all of them
        (no reference counterpart; each graph follows the single-graph LM exactly)."""
        lib, h = self.ctx.lib, self.ctx.handle
        B = len(graphs)
        made = [make_ba_result(G, chi2=False) for G in graphs]
        gs = (_abi.OsgBaGraph * B)(*[G.struct() for G in graphs])
        rs = (_abi.OsgBaResult * B)(*[m[0] for m in made])
        if stop_flag is not None:
            assert stop_flag.dtype == np.uint8, "stop flag is one byte (bool *pbStopFlag)"
        sf = None if stop_flag is None else _p(stop_flag)
        rc = lib.osg_local_bundle_adjustment_batch(h, C.addressof(gs), B, C.addressof(rs), sf)
        self.ctx.check(rc, "LocalBundleAdjustment batch")
        return [finish_ba_result(R, m[1]) for m, R in zip(made, rs)]


LBA_KERNELS = ["errors", "linearize", "pose_red", "lambda_init", "schur_point", "schur_rows", "schur_pairs",
               "chol", "chol_back", "update", "step_reduce", "classify"]


def lba_kernel_times(ctx, enable: bool) -> dict:
    """osg_lba_kernel_times: per-kernel device time (HIP events) of the LBA engine since the last
    enable, as {kernel: (ms, launch groups)}; enable=True (re)starts the timing, False stops it."""
    ms = np.zeros(len(LBA_KERNELS), np.float64)
    n = np.zeros(len(LBA_KERNELS), np.int64)
    ctx.check(ctx.lib.osg_lba_kernel_times(ctx.handle, int(enable), _p(ms), _p(n)), "lba_kernel_times")
    return {k: (float(ms[i]), int(n[i])) for i, k in enumerate(LBA_KERNELS)}


def lba_structure_counts(G: "BAGraph") -> dict:
    """Sizes of the BlockSolver structure of a graph (ba.hip build_structure): free poses with an
    edge, landmarks, (landmark, free pose) blocks, and Schur contributions sum_l k_l (k_l + 1) / 2
    (k_l = free poses observing landmark l)."""
    fixed = np.asarray(G.pose_fixed).astype(bool)
    ep, et = np.asarray(G.e_pose), np.asarray(G.e_point)
    free = ~fixed[ep]
    blocks = np.unique(et[free].astype(np.int64) * (len(G.pose) + 1) + ep[free])
    k = np.bincount((blocks // (len(G.pose) + 1)).astype(np.int64), minlength=len(G.point))
    return {"free_poses": int(len(np.unique(ep[free]))), "landmarks": int(len(np.unique(et))),
            "blocks": int(len(blocks)), "contributions": int((k * (k + 1) // 2).sum())}


# ----------------------------------------------------------------------------- generators
def kb8_project(cam, Xc):
    """KannalaBrandt8::project (ref:src/CameraModels/KannalaBrandt8.cpp:76-99) in float64."""
    k = [float(cam.p[i]) for i in range(8)]
    th = np.arctan2(np.hypot(Xc[:, 0], Xc[:, 1]), Xc[:, 2])
    ps = np.arctan2(Xc[:, 1], Xc[:, 0])
    r = th + k[4] * th ** 3 + k[5] * th ** 5 + k[6] * th ** 7 + k[7] * th ** 9
    return k[0] * r * np.cos(ps) + k[2], k[1] * r * np.sin(ps) + k[3]


# TUM-VI-like right-from-left extrinsic of the fisheye pair: 10.1 cm baseline, ~0.5 deg rotation
TUMVI_TRL = [0.0021, -0.0023, 0.0011, 0.99999, -0.101, 0.0005, -0.0004]


def synth_pose_problem(rng, n_edges=400, stereo_frac=0.6, outlier_frac=0.1, n_levels=8, cam=None, body_frac=0.0):
    """C3 PoseOptimization: Xw depth U[1,10] m in front of the camera, pose perturbed by
    1 cm / 0.5 deg, pixel noise 1 px * 1.2^octave, 10 % outliers (+20..50 px), stereo u_R for
    60 % of the edges (bf = 47.9).  With a KB8 camera and ``body_frac`` > 0 (C5, two-camera rig),
    that fraction of the edges are right-camera observations (EdgeSE3ProjectXYZOnlyPoseToBody, the
    second camera ``kb8_camera(trl=TUMVI_TRL)``)."""
    cam = cam or pinhole_camera()
    Rcw = small_rotation(rng, 20.0)
    tcw = rng.normal(0, 1.0, 3)
    if cam.type == _abi.CAM_KB8:
        # fisheye (TUM-VI-like 512 x 512): directions up to 70 deg off-axis, projected by KB8
        th = rng.uniform(0.05, 1.2, n_edges)
        ps = rng.uniform(-np.pi, np.pi, n_edges)
        d = rng.uniform(1.0, 10.0, n_edges)
        Xc = np.stack([d * np.sin(th) * np.cos(ps), d * np.sin(th) * np.sin(ps), d * np.cos(th)], 1)
        k = [float(cam.p[i]) for i in range(8)]
        r = th + k[4] * th ** 3 + k[5] * th ** 5 + k[6] * th ** 7 + k[7] * th ** 9
        u = k[0] * r * np.cos(ps) + k[2]
        v = k[1] * r * np.sin(ps) + k[3]
        z = Xc[:, 2]
        stereo_frac = 0.0  # no rectified stereo on a fisheye rig
    else:
        u = rng.uniform(20, EUROC_W - 20, n_edges)
        v = rng.uniform(20, EUROC_H - 20, n_edges)
        z = rng.uniform(1.0, 10.0, n_edges)
        Xc = np.stack([(u - EUROC_CX) / EUROC_FX * z, (v - EUROC_CY) / EUROC_FY * z, z], 1)
    Xw = (Xc - tcw) @ Rcw  # Rcw^T (Xc - t)
    Xw = Xw.astype(np.float32).astype(np.float64)
    octv = rng.choice(n_levels, n_edges, p=np.array([1.2 ** -i for i in range(n_levels)]) / sum(1.2 ** -i for i in range(n_levels)))
    sig = 1.2 ** octv
    obs = np.zeros((n_edges, 3))
    obs[:, 0] = u + rng.normal(0, 1, n_edges) * sig
    obs[:, 1] = v + rng.normal(0, 1, n_edges) * sig
    out = rng.random(n_edges) < outlier_frac
    obs[out, 0] += rng.uniform(20, 50, out.sum()) * rng.choice([-1, 1], out.sum())
    obs[out, 1] += rng.uniform(20, 50, out.sum()) * rng.choice([-1, 1], out.sum())
    stereo = rng.random(n_edges) < stereo_frac
    obs[:, 2] = np.where(stereo, obs[:, 0] - EUROC_BF / z + rng.normal(0, 0.5, n_edges), 0.0)
    obs = obs.astype(np.float32).astype(np.float64)  # keypoints are float
    kind = np.where(stereo, _abi.EDGE_STEREO, _abi.EDGE_MONO).astype(np.int8)
    # perturbed initial pose
    R0 = small_rotation(rng, 0.5) @ Rcw
    t0 = tcw + rng.normal(0, 0.01, 3)
    isig = inv_level_sigma2(n_levels)[octv]
    cam2 = cam
    if cam.type == _abi.CAM_KB8 and body_frac > 0:
        cam2 = kb8_camera(trl=TUMVI_TRL)
        q = np.array(TUMVI_TRL[:4]) / np.linalg.norm(TUMVI_TRL[:4])
        from scipy.spatial.transform import Rotation
        Rrl = Rotation.from_quat(q).as_matrix()
        Xr = Xc @ Rrl.T + np.array(TUMVI_TRL[4:])
        body = (rng.random(n_edges) < body_frac) & (Xr[:, 2] > 0.1)
        ur, vr = kb8_project(cam2, Xr[body])
        sb = sig[body]
        obs[body, 0] = ur + rng.normal(0, 1, body.sum()) * sb
        obs[body, 1] = vr + rng.normal(0, 1, body.sum()) * sb
        obs[body, 2] = 0.0
        ob = body & out
        obs[ob, 0] += rng.uniform(20, 50, ob.sum()) * rng.choice([-1, 1], ob.sum())
        obs = obs.astype(np.float32).astype(np.float64)
        kind = np.where(body, _abi.EDGE_BODY, kind).astype(np.int8)
    return PoseProblem(pose7(R0, t0), kind, Xw, obs, isig, cam=cam, cam2=cam2)


def _project(cam, X):
    """GeometricCamera::project of rows of X in float64 (generators only)."""
    if cam.type == _abi.CAM_KB8:
        u, v = kb8_project(cam, X)
    else:
        u = float(cam.p[0]) * X[:, 0] / X[:, 2] + float(cam.p[2])
        v = float(cam.p[1]) * X[:, 1] / X[:, 2] + float(cam.p[3])
    return np.stack([u, v], 1)


def synth_sim3_problem(rng, n_pairs=100, outlier_frac=0.1, out_of_kf2_frac=0.0, fix_scale=False, cam1=None, cam2=None,
                       n_levels=8, noise_px=1.0, noise_m=0.01, th2=10.0):
    """One loop-closure Sim3 refinement as LoopClosing hands it to OptimizeSim3: points 2 .. 8 m in front
    of KeyFrame 2, the true S12 a few degrees / decimetres / per cent away from identity (scale 1 when
    ``fix_scale``), each KeyFrame's own MapPoint ``noise_m`` off the common point, pixel noise ``noise_px``
    x 1.2^octave, gross outliers (+20 .. 50 px in one image), and an initial S12 0.5 deg / 2 cm / 1 % off.
    ``out_of_kf2_frac`` of the pairs have no keypoint in KeyFrame 2: obs2 is the float (x/z, y/z) of p2c and
    the weight mvInvLevelSigma2[0], as ref:src/Optimizer.cc:4389-4404 builds them.  Points and keypoints are
    float-valued doubles, as the adapter gathers them."""
    cam1 = cam1 or pinhole_camera()
    cam2 = cam2 or pinhole_camera()
    n = int(n_pairs)
    if cam2.type == _abi.CAM_KB8:
        th = rng.uniform(0.05, 0.9, n)
        ps = rng.uniform(-np.pi, np.pi, n)
        d = rng.uniform(2.0, 8.0, n)
        P2 = np.stack([d * np.sin(th) * np.cos(ps), d * np.sin(th) * np.sin(ps), d * np.cos(th)], 1)
    else:
        u = rng.uniform(60, EUROC_W - 60, n)
        v = rng.uniform(60, EUROC_H - 60, n)
        z = rng.uniform(2.0, 8.0, n)
        P2 = np.stack([(u - float(cam2.p[2])) / float(cam2.p[0]) * z, (v - float(cam2.p[3])) / float(cam2.p[1]) * z, z], 1)
    R = small_rotation(rng, 3.0)
    t = rng.normal(0, 0.15, 3)
    s = 1.0 if fix_scale else float(rng.uniform(0.9, 1.1))
    P1 = s * P2 @ R.T + t
    isig = inv_level_sigma2(n_levels)
    lev_p = np.array([1.2 ** -i for i in range(n_levels)])
    lev_p /= lev_p.sum()
    oct1 = rng.choice(n_levels, n, p=lev_p)
    oct2 = rng.choice(n_levels, n, p=lev_p)
    obs1 = _project(cam1, P1) + rng.normal(0, noise_px, (n, 2)) * (1.2 ** oct1)[:, None]
    obs2 = _project(cam2, P2) + rng.normal(0, noise_px, (n, 2)) * (1.2 ** oct2)[:, None]
    out = rng.random(n) < outlier_frac
    side = rng.random(n) < 0.5
    shift = rng.uniform(20, 50, (n, 2)) * rng.choice([-1, 1], (n, 2))
    obs1[out & side] += shift[out & side]
    obs2[out & ~side] += shift[out & ~side]
    p1c = (P1 + rng.normal(0, noise_m, (n, 3))).astype(np.float32)
    p2c = (P2 + rng.normal(0, noise_m, (n, 3))).astype(np.float32)
    obs1 = obs1.astype(np.float32).astype(np.float64)
    obs2 = obs2.astype(np.float32).astype(np.float64)
    w1 = isig[oct1].copy()
    w2 = isig[oct2].copy()
    nokf2 = rng.random(n) < out_of_kf2_frac
    if nokf2.any():
        invz = np.float32(1) / p2c[nokf2, 2]
        obs2[nokf2, 0] = (p2c[nokf2, 0] * invz).astype(np.float64)
        obs2[nokf2, 1] = (p2c[nokf2, 1] * invz).astype(np.float64)
        w2[nokf2] = isig[0]
    R0 = small_rotation(rng, 0.5) @ R
    t0 = t + rng.normal(0, 0.02, 3)
    s0 = s if fix_scale else s * float(1 + rng.normal(0, 0.01))
    return Sim3Problem(rot_to_quat(R0), t0, s0, p1c.astype(np.float64), p2c.astype(np.float64), obs1, obs2, w1, w2,
                       fix_scale=bool(fix_scale), th2=th2, cam1=cam1, cam2=cam2, truth=(R, t, s))


def rodrigues(w):
    w = np.asarray(w, float)
    a = np.linalg.norm(w)
    if a < 1e-300:
        return np.eye(3)
    k = w / a
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * K @ K


def s3_mul(a, b):
    return a[0] @ b[0], a[2] * (a[0] @ b[1]) + a[1], a[2] * b[2]


def s3_inv(a):
    return a[0].T, a[0].T @ (-a[1] / a[2]), 1.0 / a[2]


def s3_row(a):
    return np.concatenate([rot_to_quat(a[0]), a[1], [a[2]]])


def synth_essential_graph(rng, n_kf, n_loop=3, extra_loops=0, fix_scale=False, consistent=False,
                          drift=(3.0, 0.2, 0.05), radius=0.8):
    """The pose graph LoopClosing::CorrectLoop hands to OptimizeEssentialGraph after closing a loop: n_kf
    KeyFrames on a closed trajectory (a circle of ``radius`` m, about 5 m long, cameras looking at its centre),
    KeyFrame 0 fixed (the map's init KeyFrame), the last ``n_loop`` KeyFrames carrying a corrected Sim3.  Edges
    in the reference's insertion order: the LoopConnections (corrected KeyFrame k -> the KeyFrames
    k - (n_kf - n_loop) and k - (n_kf - n_loop) + 1 at the start), then per KeyFrame i its spanning-tree edge
    (i -> i - 1), its earlier loop edges (``extra_loops`` of them between the middle of the map and its first
    third, to the smaller id), and its covisibility edges (i -> i - 2, i -> i - 3).

    The drift grows linearly along the trajectory to ``drift`` = (degrees, metres, relative scale) at its end
    and is applied on the world side (S_i = G_i * D_i).
      consistent=False: as the reference builds it.  The non-corrected poses N_i are the drifted ones with
        scale 1, the corrected Sim3 of the last KeyFrames is N_i * D_end^-1 (with the drifted scale unless
        ``fix_scale``), every non-loop measurement is N_j * N_i^-1 and every loop measurement S_j * S_i^-1 of
        the initial estimates.
      consistent=True: the measurements are G_j * G_i^-1 of a ground truth G (returned as ``truth``; scales
        drawn in [0.95, 1.05] unless ``fix_scale``), the corrected KeyFrames start at the truth and the others
        at G_i * D_i, so the optimum is the truth with chi2 = 0."""
    n, m = int(n_kf), int(n_loop)
    assert n >= 2 and 0 <= m < n
    ang = 2 * np.pi * np.arange(n) / n
    G = []
    for i in range(n):
        c = np.array([radius * np.cos(ang[i]), 0.05 * np.sin(3 * ang[i]), radius * np.sin(ang[i])])
        R, t = look_at(c, [0.0, 0.3 * rng.normal(), 0.0])
        s = 1.0 if (fix_scale or not consistent) else float(rng.uniform(0.95, 1.05))
        G.append((R, s * t, s))
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    tdir = rng.normal(size=3)
    tdir /= np.linalg.norm(tdir)

    def D(f):
        return (rodrigues(np.deg2rad(drift[0]) * f * axis), drift[1] * f * tdir,
                1.0 if fix_scale else float(np.exp(np.log1p(drift[2]) * f)))

    frac = np.arange(n) / max(n - 1, 1)
    corrected = np.zeros(n, bool)
    corrected[n - m:] = True
    if consistent:
        est = [G[i] if corrected[i] or i == 0 else s3_mul(G[i], D(frac[i])) for i in range(n)]
        base = G
    else:
        N = []
        for i in range(n):
            d = D(frac[i])
            N.append(s3_mul(G[i], (d[0], d[1], 1.0)))
        Dinv = s3_inv(D(1.0))
        est = [s3_mul(N[i], Dinv) if corrected[i] else N[i] for i in range(n)]
        base = N
    loops = {}
    for q in range(int(extra_loops)):
        a = n // 2 + 3 * q + 1
        b = n // 5 + 2 * q
        if b < a - 3 and a < n - m:
            loops.setdefault(a, []).append(b)
    v0, v1, meas = [], [], []

    def edge(i, j, src):
        v0.append(i)
        v1.append(j)
        meas.append(s3_row(s3_mul(src[j], s3_inv(src[i]))))

    loop_src = base if consistent else est
    for k in range(n - m, n):
        for j in (k - (n - m), k - (n - m) + 1):
            if 0 <= j < n - m and j != k:
                edge(k, j, loop_src)
    for i in range(n):
        if i >= 1:
            edge(i, i - 1, base)
        for b in loops.get(i, []):
            edge(i, b, base)
        for j in (i - 2, i - 3):
            if j >= 0:
                edge(i, j, base)
    fixed = np.zeros(n, np.uint8)
    fixed[0] = 1
    return EssentialGraphProblem(np.array([s3_row(e) for e in est]), fixed, np.array(v0, np.int32), np.array(v1, np.int32),
                                 np.array(meas).reshape(-1, 8), fix_scale=bool(fix_scale),
                                 truth=np.array([s3_row(g) for g in G]) if consistent else None)


def imu_cam_pose_row(Rwb, twb, Rcw, tcw, Rcb, tcb):
    """the 36 doubles of one vertex of an EssentialGraph4DoFProblem"""
    return np.concatenate([np.asarray(Rwb, np.float64).ravel(), np.asarray(twb, np.float64),
                           np.asarray(Rcw, np.float64).ravel(), np.asarray(tcw, np.float64),
                           np.asarray(Rcb, np.float64).ravel(), np.asarray(tcb, np.float64)])


def imu_cam_pose_corrected(Rwc, twc, Rcb, tcb):
    """ImuCamPose(Rwc, twc, pKF) (ref:src/G2oTypes.cc:132-157), the vertex of a KeyFrame in CorrectedSim3: double
    arithmetic on the inverse of the corrected Sim3, Tcb cast from the KeyFrame's float calibration."""
    Rwc, twc = np.asarray(Rwc, np.float64), np.asarray(twc, np.float64)
    Rcb, tcb = np.asarray(Rcb, np.float32).astype(np.float64), np.asarray(tcb, np.float32).astype(np.float64)
    Rcw = Rwc.T.copy()
    return imu_cam_pose_row(Rwc @ Rcb, Rwc @ tcb + twc, Rcw, -Rcw @ twc, Rcb, tcb)


def imu_cam_pose_keyframe(Rcw, tcw, Rcb, tcb):
    """ImuCamPose(pKF) (ref:src/G2oTypes.cc:29-75): every field cast from the floats KeyFrame::SetPose derived
    (Rwc = Rcw', Ow = -Rwc tcw, Owb = Rwc tcb + Ow, Rwb = Rwc Rcb, ref:src/KeyFrame.cc:90-107), here with numpy's
    float32 products."""
    f = np.float32
    Rcw, tcw, Rcb, tcb = np.asarray(Rcw, f), np.asarray(tcw, f), np.asarray(Rcb, f), np.asarray(tcb, f)
    Rwc = Rcw.T
    Ow = -(Rwc @ tcw)
    return imu_cam_pose_row(Rwc @ Rcb, Rwc @ tcb + Ow, Rcw, tcw, Rcb, tcb)


def synth_essential_graph_4dof(rng, n_kf, n_loop=3, extra_loops=0, consistent=False, drift=(3.0, 0.2),
                               meas_noise=(0.02, 0.002), radius=0.8):
    """The pose graph LoopClosing::CorrectLoop hands to OptimizeEssentialGraph4DoF in an inertial map: n_kf
    KeyFrames on a closed trajectory (a circle of ``radius`` m in the plane across gravity, world z up, cameras
    looking at its centre), a body-camera extrinsic that is not the identity, KeyFrame 0 fixed, the last
    ``n_loop`` KeyFrames built as corrected (the 3-argument constructor), the others from the KeyFrame's floats.
    Edges in the reference's insertion order: the LoopConnections (corrected KeyFrame k -> the KeyFrames
    k - (n_kf - n_loop) and k - (n_kf - n_loop) + 1 at the start), then per KeyFrame i its mPrevKF edge
    (i -> i - 1), its earlier loop edges (``extra_loops`` of them, as ``synth_essential_graph`` places them) and its
    covisibility edges (i -> i - 2, i -> i - 3).  An edge (i, j) measures Tcw_i Tcw_j^-1.

    The drift of an inertial map is in yaw and translation alone (gravity pins roll and pitch): it grows
    linearly along the trajectory to ``drift`` = (degrees of yaw, metres) and moves the body pose as the vertex's
    update does, Rwb <- Rz(yaw) Rwb, twb <- twb + d.
      consistent=False: as the reference builds it.  The non-corrected poses N_i are the drifted ones, the
        corrected KeyFrames are N_i with the drift of the trajectory's end taken out, every non-loop measurement
        is N_i N_j^-1 and every loop measurement that of the initial estimates, each moved by a small rotation
        about a random axis and a translation (``meas_noise`` degrees, metres: the roll / pitch the edges carry).
      consistent=True: double throughout; the measurements are those of a ground truth (returned as ``truth``),
        the corrected KeyFrames and KeyFrame 0 start at it and the others at the truth moved in yaw and
        translation, so the optimum is the truth with chi2 = 0."""
    n, m = int(n_kf), int(n_loop)
    assert n >= 2 and 0 <= m < n
    ang = 2 * np.pi * np.arange(n) / n
    # Tcb as the calibration's floats give it: orthonormal to float precision
    Rcb = rodrigues(np.array([1.2, -1.19, 1.21]) + 0.01 * rng.normal(size=3)).astype(np.float32).astype(np.float64)
    tcb = (np.array([0.065, -0.021, 0.009]) + 0.002 * rng.normal(size=3)).astype(np.float32).astype(np.float64)
    Gb = []                      # ground truth body poses (Rwb, twb)
    for i in range(n):
        c = np.array([radius * np.cos(ang[i]), radius * np.sin(ang[i]), 0.05 * np.sin(3 * ang[i])])
        Rcw, tcw = look_at(c, [0.0, 0.0, 0.3 * rng.normal()], up=(0, 0, 1))
        Rwc, twc = Rcw.T, -Rcw.T @ tcw
        Gb.append((Rwc @ Rcb, Rwc @ tcb + twc))
    tdir = rng.normal(size=3)
    tdir /= np.linalg.norm(tdir)

    def moved(b, f):
        return rodrigues([0.0, 0.0, np.deg2rad(drift[0]) * f]) @ b[0], b[1] + drift[1] * f * tdir

    def cam(b):                  # (Rcw, tcw) of a body pose
        Rcw = Rcb @ b[0].T
        return Rcw, Rcb @ (-(b[0].T @ b[1])) + tcb

    frac = np.arange(n) / max(n - 1, 1)
    corrected = np.zeros(n, bool)
    corrected[n - m:] = True
    N = [moved(Gb[i], frac[i]) for i in range(n)]
    if consistent:
        est_b = [Gb[i] if corrected[i] or i == 0 else N[i] for i in range(n)]
        base = [cam(b) for b in Gb]
    else:
        est_b = [moved(N[i], -1.0) if corrected[i] else N[i] for i in range(n)]
        base = [cam(b) for b in N]
    est_c = [cam(b) for b in est_b]
    rows = []
    for i in range(n):
        Rcw, tcw = est_c[i]
        if corrected[i]:
            rows.append(imu_cam_pose_corrected(Rcw.T, -Rcw.T @ tcw, Rcb, tcb))
        elif consistent:
            rows.append(imu_cam_pose_row(est_b[i][0], est_b[i][1], Rcw, tcw, Rcb, tcb))
        else:
            rows.append(imu_cam_pose_keyframe(Rcw, tcw, Rcb, tcb))
    rows = np.array(rows)
    # the poses the reference's vScw holds: the corrected Sim3's camera or the KeyFrame's float pose
    start = [(rows[i, 12:21].reshape(3, 3), rows[i, 21:24]) for i in range(n)]
    loops = {}
    for q in range(int(extra_loops)):
        a = n // 2 + 3 * q + 1
        b = n // 5 + 2 * q
        if b < a - 3 and a < n - m:
            loops.setdefault(a, []).append(b)
    v0, v1, meas = [], [], []

    def edge(i, j, src):
        dR = src[i][0] @ src[j][0].T
        dt = src[i][1] - dR @ src[j][1]
        if not consistent:
            w = rng.normal(size=3)
            w *= np.deg2rad(meas_noise[0]) * rng.normal() / np.linalg.norm(w)
            dR, dt = rodrigues(w) @ dR, dt + rng.normal(0, meas_noise[1], 3)
        v0.append(i)
        v1.append(j)
        meas.append(np.concatenate([dR.ravel(), dt]))

    loop_src = base if consistent else start
    for k in range(n - m, n):
        for j in (k - (n - m), k - (n - m) + 1):
            if 0 <= j < n - m and j != k:
                edge(k, j, loop_src)
    for i in range(n):
        if i >= 1:
            edge(i, i - 1, base)
        for b in loops.get(i, []):
            edge(i, b, base)
        for j in (i - 2, i - 3):
            if j >= 0:
                edge(i, j, base)
    fixed = np.zeros(n, np.uint8)
    fixed[0] = 1
    truth = None
    if consistent:
        truth = np.array([imu_cam_pose_row(Gb[i][0], Gb[i][1], base[i][0], base[i][1], Rcb, tcb) for i in range(n)])
    return EssentialGraph4DoFProblem(rows, fixed, np.array(v0, np.int32), np.array(v1, np.int32),
                                     np.array(meas).reshape(-1, 12), truth=truth,
                                     built=np.where(corrected, b"C", b"K" if not consistent else b"D"))


def synth_lba_graph(rng, n_kf=50, n_points=10000, k_range=(2, 8), n_fixed=2, stereo_frac=0.0,
                    outlier_frac=0.01, n_levels=8, radius=6.0, arc_deg=50.0):
    """C4 LocalBundleAdjustment: n_kf keyframes on an arc (radius 6 m, ~5 m long) looking at a
    4 x 4 x 2 m box of points; each point observed by k ~ U{2..8} keyframes that see it; pixel
    noise 1 px * 1.2^octave; pose noise 1 cm / 0.3 deg; point noise 2 cm; 1 % gross outliers.
    KeyFrames 0..n_fixed-1 are fixed (init KF + fixed observers)."""
    cam = pinhole_camera()
    ang = np.deg2rad(np.linspace(-arc_deg / 2, arc_deg / 2, n_kf))
    centers = np.stack([radius * np.sin(ang), 0.3 * np.sin(3 * ang), -radius * np.cos(ang)], 1)
    Rs, ts = [], []
    for c in centers:
        R, t = look_at(c, [0, 0, 0])
        Rs.append(R)
        ts.append(t)
    P = np.stack([rng.uniform(-2, 2, n_points), rng.uniform(-2, 2, n_points), rng.uniform(-1, 1, n_points)], 1)
    isig_tab = inv_level_sigma2(n_levels)
    e_point, e_pose, e_obs, e_isig, e_kind = [], [], [], [], []
    for p in range(n_points):
        # keyframes that see the point inside the image
        Xc = np.einsum("kij,j->ki", np.array(Rs), P[p]) + np.array(ts)
        u = EUROC_FX * Xc[:, 0] / Xc[:, 2] + EUROC_CX
        v = EUROC_FY * Xc[:, 1] / Xc[:, 2] + EUROC_CY
        vis = np.nonzero((Xc[:, 2] > 0.5) & (u > 0) & (u < EUROC_W) & (v > 0) & (v < EUROC_H))[0]
        if len(vis) < 2:
            continue
        k = min(len(vis), int(rng.integers(k_range[0], k_range[1] + 1)))
        obs_kf = np.sort(rng.choice(vis, k, replace=False))
        for kf in obs_kf:
            octv = int(rng.choice(n_levels, p=np.array([1.2 ** -i for i in range(n_levels)]) / sum(1.2 ** -i for i in range(n_levels))))
            s = 1.2 ** octv
            uu = u[kf] + rng.normal() * s
            vv = v[kf] + rng.normal() * s
            if rng.random() < outlier_frac:
                uu += rng.uniform(20, 50) * rng.choice([-1, 1])
                vv += rng.uniform(20, 50) * rng.choice([-1, 1])
            st = rng.random() < stereo_frac
            ur = uu - EUROC_BF / Xc[kf, 2] + rng.normal() * 0.5 if st else 0.0
            e_point.append(p)
            e_pose.append(kf)
            e_obs.append([uu, vv, ur])
            e_isig.append(isig_tab[octv])
            e_kind.append(_abi.EDGE_STEREO if st else _abi.EDGE_MONO)
    e_point = np.array(e_point)
    used = np.unique(e_point)
    remap = -np.ones(n_points, int)
    remap[used] = np.arange(len(used))
    e_point = remap[e_point]
    P = P[used]
    poses = []
    for i, (R, t) in enumerate(zip(Rs, ts)):
        if i >= n_fixed:
            R = small_rotation(rng, 0.3) @ R
            t = t + rng.normal(0, 0.01, 3)
        poses.append(pose7(R, t))
    Pn = (P + rng.normal(0, 0.02, P.shape)).astype(np.float32).astype(np.float64)
    fixed = np.zeros(n_kf, np.uint8)
    fixed[:n_fixed] = 1
    obs = np.array(e_obs, np.float32).astype(np.float64)
    return BAGraph(np.array(poses), fixed, Pn, e_point, np.array(e_pose), np.array(e_kind, np.int8),
                   np.zeros(len(e_point), np.int32), obs, np.array(e_isig, np.float32), [cam])


def gba_robust_settings(G: BAGraph, bRobust: bool = True) -> BAGraph:
    """Give an LBA-shaped graph BundleAdjustment's kernels (ref:src/Optimizer.cc:2933-2934,
    3000-3007, 3041-3047, 3083-3085): deltas float(sqrt(5.99)) / float(sqrt(7.815)); mono and stereo
    edges carry them only when bRobust, body edges always."""
    G.huber_mono = float(np.float32(np.sqrt(5.99)))
    G.huber_stereo = float(np.float32(np.sqrt(7.815)))
    G.e_robust = np.where(G.e_kind == _abi.EDGE_BODY, 1, int(bool(bRobust))).astype(np.uint8)
    return G


def synth_gba_graph(rng, n_kf=120, n_points=20000, bRobust=False, iterations=10, stereo_frac=0.0, **kw):
    """A whole-map BA: keyframes on a longer arc, only the map's init KeyFrame fixed, every point with
    its observations.  Defaults: LoopClosing's GlobalBundleAdjustemnt(map, 10, &mbStopGBA, nLoopKF,
    false) (ref:src/LoopClosing.cc:3084); the monocular initialisation runs (map, 20) with bRobust
    true (ref:src/Tracking.cc:3076)."""
    G = synth_lba_graph(rng, n_kf=n_kf, n_points=n_points, n_fixed=1, stereo_frac=stereo_frac,
                        arc_deg=kw.pop("arc_deg", 120.0), **kw)
    G.iterations = iterations
    return gba_robust_settings(G, bRobust)


def synth_map_graph(rng, n_kf=1500, n_points=150000, spacing=0.3, k_range=(2, 6), bRobust=False, iterations=10,
                    stereo_frac=0.0, n_levels=8, loop=False, vectorized=False):
    """A map-scale whole-map BA (GlobalBundleAdjustemnt on a long sequence): n_kf keyframes 'spacing'
    m apart along a 0.45 km path, looking sideways at points 4 .. 6 m away spread along it, so a
    keyframe shares points only with its neighbours (~27 on each side) and the reduced camera
    system is a band, as in an open trajectory without loop closures.  Each point is observed by
    k ~ U{k_range} of the keyframes that see it; pixel noise 1 px * 1.2^octave, pose noise 1 cm /
    0.3 deg, point noise 2 cm; the first keyframe is fixed (the map's init KeyFrame).

    loop=True: the same path closed into a circle (radius n_kf spacing / 2 pi, cameras looking
    outwards at a ring of points), so the last keyframes share points with the first ones — the map
    LoopClosing hands to GlobalBundleAdjustemnt after closing a loop (ref:src/LoopClosing.cc:2436):
    the reduced camera system is the band plus the two corner blocks that join its ends.

    vectorized=True draws each point's observing keyframes and levels array-wise (another random stream
    than the per-point loop, the same distribution): the maps of many thousand keyframes build in
    seconds."""
    cam = pinhole_camera()
    L = spacing * (n_kf - 1)
    cx = np.arange(n_kf) * spacing
    cy = 0.1 * np.sin(np.arange(n_kf) * 0.05)
    yaw = np.deg2rad(rng.normal(0, 2.0, n_kf))
    Rs = np.stack([np.array([[np.cos(a), 0, -np.sin(a)], [0, 1, 0], [np.sin(a), 0, np.cos(a)]]) for a in yaw])
    if loop:
        Rc = spacing * n_kf / (2 * np.pi)
        th = 2 * np.pi * np.arange(n_kf) / n_kf
        # camera axes in world coordinates: x along the tangent, y down (world y), z outwards
        R0 = np.stack([np.array([[np.sin(a), 0, -np.cos(a)], [0, 1, 0], [np.cos(a), 0, np.sin(a)]]) for a in th])
        Rs = np.einsum("kij,kjl->kil", Rs, R0)
        C = np.stack([Rc * np.cos(th), cy, Rc * np.sin(th)], 1)
    else:
        C = np.stack([cx, cy, np.zeros(n_kf)], 1)
    ts = -np.einsum("kij,kj->ki", Rs, C)
    P = np.stack([rng.uniform(-1.0, L + 1.0, n_points), rng.uniform(-1.5, 1.5, n_points),
                  rng.uniform(4.0, 6.0, n_points)], 1)
    if loop:  # the same draws as angle (path position) and distance off the path, on the ring
        phi = 2 * np.pi * P[:, 0] / (spacing * n_kf)
        rho = Rc + P[:, 2]
        P = np.stack([rho * np.cos(phi), P[:, 1], rho * np.sin(phi)], 1)
        pos = phi / (2 * np.pi) * n_kf   # path position in keyframes
    else:
        pos = P[:, 0] / spacing
    isig_tab = inv_level_sigma2(n_levels)
    lev_p = np.array([1.2 ** -i for i in range(n_levels)])
    lev_p /= lev_p.sum()
    W = int(np.ceil(6.0 * 0.85 / spacing)) + 2  # keyframes within reach of a point
    e_point, e_pose, e_obs, e_kind, e_lev = [], [], [], [], []
    for p0 in range(0, n_points, 20000):
        Pc = P[p0:p0 + 20000]
        if loop:
            base = np.round(pos[p0:p0 + 20000]).astype(int) - W
            cand = (base[:, None] + np.arange(2 * W + 1)[None, :]) % n_kf  # (m, 2W+1)
        else:
            base = np.clip(np.round(pos[p0:p0 + 20000]).astype(int) - W, 0, None)
            cand = np.clip(base[:, None] + np.arange(2 * W + 1)[None, :], 0, n_kf - 1)  # (m, 2W+1)
        Xc = np.einsum("mkij,mj->mki", Rs[cand], Pc) + ts[cand]
        u = EUROC_FX * Xc[..., 0] / Xc[..., 2] + EUROC_CX
        v = EUROC_FY * Xc[..., 1] / Xc[..., 2] + EUROC_CY
        vis = (Xc[..., 2] > 0.5) & (u > 0) & (u < EUROC_W) & (v > 0) & (v < EUROC_H)
        vis[:, 1:] &= cand[:, 1:] != cand[:, :-1]  # clipped duplicates
        if vectorized:
            nvis = vis.sum(1)
            kk = np.minimum(nvis, rng.integers(k_range[0], k_range[1] + 1, len(Pc)))
            kk[nvis < 2] = 0
            key = np.where(vis, rng.random(vis.shape), 2.0)   # k uniformly chosen visible candidates
            order = np.argsort(key, 1)
            take = np.arange(vis.shape[1])[None, :] < kk[:, None]
            mi, ji = np.nonzero(take)
            jsel = order[mi, ji]
            srt = np.lexsort((jsel, mi))                       # per point in candidate order, as np.sort
            mi, jsel = mi[srt], jsel[srt]
            e_point.extend((p0 + mi).tolist())
            e_pose.extend(cand[mi, jsel].tolist())
            e_obs.extend(np.stack([u[mi, jsel], v[mi, jsel], Xc[mi, jsel, 2]], 1).tolist())
            e_lev.extend(rng.choice(n_levels, len(mi), p=lev_p).tolist())
            continue
        for m in range(len(Pc)):
            idx = np.nonzero(vis[m])[0]
            if len(idx) < 2:
                continue
            k = min(len(idx), int(rng.integers(k_range[0], k_range[1] + 1)))
            sel = np.sort(rng.choice(idx, k, replace=False))
            for j in sel:
                e_point.append(p0 + m)
                e_pose.append(cand[m, j])
                e_obs.append((u[m, j], v[m, j], Xc[m, j, 2]))
                e_lev.append(int(rng.choice(n_levels, p=lev_p)))
    e_point = np.array(e_point)
    e_pose = np.array(e_pose)
    e_obs = np.array(e_obs)
    e_lev = np.array(e_lev)
    ne = len(e_point)
    s = 1.2 ** e_lev
    obs = np.zeros((ne, 3))
    obs[:, 0] = e_obs[:, 0] + rng.normal(0, 1, ne) * s
    obs[:, 1] = e_obs[:, 1] + rng.normal(0, 1, ne) * s
    st = rng.random(ne) < stereo_frac
    obs[:, 2] = np.where(st, obs[:, 0] - EUROC_BF / e_obs[:, 2] + rng.normal(0, 0.5, ne), 0.0)
    used = np.unique(e_point)
    remap = -np.ones(n_points, int)
    remap[used] = np.arange(len(used))
    e_point = remap[e_point]
    P = P[used]
    poses = []
    for i in range(n_kf):
        R, t = Rs[i], ts[i]
        if i >= 1:  # about the keyframe's own centre: 0.3 deg and 1 cm
            R = small_rotation(rng, 0.3) @ R
            t = -R @ (C[i] + rng.normal(0, 0.01, 3))
        poses.append(pose7(R, t))
    Pn = (P + rng.normal(0, 0.02, P.shape)).astype(np.float32).astype(np.float64)
    fixed = np.zeros(n_kf, np.uint8)
    fixed[0] = 1
    G = BAGraph(np.array(poses), fixed, Pn, e_point, e_pose, np.where(st, _abi.EDGE_STEREO, _abi.EDGE_MONO).astype(np.int8),
                np.zeros(ne, np.int32), obs.astype(np.float32).astype(np.float64),
                isig_tab[e_lev].astype(np.float32), [cam])
    G.iterations = iterations
    return gba_robust_settings(G, bRobust)


def depth_positive(G: BAGraph, pose, point, edges):
    """isDepthPositive of the given edges: z of SE3Quat::map(X) = q X q* + t (Eigen's quaternion-vector
    product), > 0."""
    q = np.asarray(pose, np.float64).reshape(-1, 7)[G.e_pose[edges]]
    X = np.asarray(point, np.float64).reshape(-1, 3)[G.e_point[edges]]
    u, w = q[:, :3], q[:, 3:4]
    uv = 2.0 * np.cross(u, X)
    return (X + w * uv + np.cross(u, uv) + q[:, 4:7])[:, 2] > 0


def merge_local_bundle_adjustment(G: BAGraph, run, stop_flag=None, mp_bad=None):
    """The g2o part of Optimizer::LocalBundleAdjustment(pMainKF, vpAdjustKF, vpFixedKF, pbStopFlag)
    (ref:src/Optimizer.cc:5211-5672) on a graph gathered as it builds it: mono / stereo edges (no
    right-camera edges), BundleAdjustment's Huber deltas, vpFixedKF fixed.  ``run(graph, stop_flag)`` is
    one g2o optimize through the C ABI (Optimizer.BundleAdjustment; the oracle in tests):
      1. optimize(5) with Huber on every edge (:5448-5449);
      2. unless stopped: edges with chi2 > 5.991 / 7.815 or behind the camera go to level 1, every kernel
         is dropped (edges of bad MapPoints are skipped by both steps), and a fresh LM optimize(10) runs on
         the level-0 edges (:5451-5498);
      3. the final classification (:5506-5546): level-0 edges by their second-pass errors, level-1 edges by
         their first-pass chi2 (never recomputed) and the final depth.
    Returns (pose, point, erase flag per edge, stopped before the first pass)."""
    ne = len(G.e_point)
    mp_bad = np.zeros(len(G.point), bool) if mp_bad is None else np.asarray(mp_bad, bool)
    if stop_flag is not None and stop_flag[0]:  # :5444-5446: return before optimising
        return G.pose.copy(), G.point.copy(), np.zeros(ne, np.uint8), True
    G1 = gba_robust_settings(replace(G, iterations=5), True)
    r1 = run(G1, stop_flag)
    skip = mp_bad[G.e_point]
    if stop_flag is not None and stop_flag[0]:  # bDoMore = false: the first pass's classification
        return r1.pose, r1.point, (r1.edge_bad.astype(bool) & ~skip).astype(np.uint8), False
    level1 = r1.edge_bad.astype(bool) & ~skip
    keep = np.nonzero(~level1)[0]
    G2 = BAGraph(r1.pose, G.pose_fixed, r1.point, G.e_point[keep], G.e_pose[keep], G.e_kind[keep], G.e_cam[keep],
                 G.e_obs[keep], G.e_inv_sigma2[keep], G.cams, iterations=10, e_robust=skip[keep].astype(np.uint8),
                 huber_mono=G1.huber_mono, huber_stereo=G1.huber_stereo)
    r2 = run(G2, stop_flag)
    bad = np.zeros(ne, bool)
    bad[keep] = r2.edge_bad.astype(bool)
    l1 = np.nonzero(level1)[0]
    th = np.where(G.e_kind[l1] == _abi.EDGE_STEREO, 7.815, 5.991)
    bad[l1] = (r1.edge_chi2[l1] > th) | ~depth_positive(G, r2.pose, r2.point, l1)
    return r2.pose, r2.point, (bad & ~skip).astype(np.uint8), False


# ----------------------------------------------------------------------------- PoseInertialOptimization
def _f32(a):
    """A Frame / KeyFrame / Preintegrated field: stored as float, read through .cast<double>()."""
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


@dataclass
class ImuState:
    """VertexPose (body pose), VertexVelocity, VertexGyroBias, VertexAccBias of one frame, in double."""
    Rwb: np.ndarray
    twb: np.ndarray
    v: np.ndarray
    bg: np.ndarray
    ba: np.ndarray

    def __post_init__(self):
        self.Rwb = np.ascontiguousarray(self.Rwb, np.float64).reshape(3, 3)
        self.twb, self.v, self.bg, self.ba = (np.ascontiguousarray(a, np.float64).reshape(3)
                                              for a in (self.twb, self.v, self.bg, self.ba))

    def fill(self, st):
        st.Rwb[:] = self.Rwb.ravel().tolist()
        st.twb[:], st.v[:], st.bg[:], st.ba[:] = (a.tolist() for a in (self.twb, self.v, self.bg, self.ba))

    @staticmethod
    def of(st):
        return ImuState(np.array(st.Rwb[:]), np.array(st.twb[:]), np.array(st.v[:]), np.array(st.bg[:]),
                        np.array(st.ba[:]))


@dataclass
class ImuCamera:
    """One camera of ImuCamPose (ref:src/G2oTypes.cc:81-127)."""
    cam: object
    Rcw: np.ndarray
    tcw: np.ndarray
    Rcb: np.ndarray
    tcb: np.ndarray
    tbc: np.ndarray


@dataclass
class Preintegrated:
    """IMU::Preintegrated as EdgeInertial reads it: float32 fields."""
    dR: np.ndarray
    dV: np.ndarray
    dP: np.ndarray
    JRg: np.ndarray
    JVg: np.ndarray
    JVa: np.ndarray
    JPg: np.ndarray
    JPa: np.ndarray
    b: np.ndarray             # (bax, bay, baz, bwx, bwy, bwz)
    dT: float
    C: np.ndarray             # 15 x 15

    def __post_init__(self):
        for k in ("dR", "JRg", "JVg", "JVa", "JPg", "JPa"):
            setattr(self, k, np.ascontiguousarray(getattr(self, k), np.float32).reshape(3, 3))
        self.dV, self.dP = (np.ascontiguousarray(a, np.float32).reshape(3) for a in (self.dV, self.dP))
        self.b = np.ascontiguousarray(self.b, np.float32).reshape(6)
        self.dT = np.float32(self.dT)
        self.C = np.ascontiguousarray(self.C, np.float32).reshape(15, 15)

    def struct(self):
        st = _abi.OsgPioPreintegrated()
        for k in ("dR", "dV", "dP", "JRg", "JVg", "JVa", "JPg", "JPa", "b", "C"):
            getattr(st, k)[:] = getattr(self, k).ravel().tolist()
        st.dT = float(self.dT)
        return st


@dataclass
class ImuPrior:
    """ConstraintPoseImu (ref:include/G2oTypes.h:820-846): H as stored, after the constructor."""
    Rwb: np.ndarray
    twb: np.ndarray
    vwb: np.ndarray
    bg: np.ndarray
    ba: np.ndarray
    H: np.ndarray

    def struct(self):
        st = _abi.OsgPioPrior()
        st.Rwb[:] = np.asarray(self.Rwb, np.float64).ravel().tolist()
        for k in ("twb", "vwb", "bg", "ba"):
            getattr(st, k)[:] = np.asarray(getattr(self, k), np.float64).ravel().tolist()
        st.H[:] = np.asarray(self.H, np.float64).ravel().tolist()
        return st


@dataclass
class PoseInertialProblem:
    """One ``PoseInertialOptimizationLastKeyFrame`` / ``LastFrame`` call as the adapter gathers it
    (include/osg_ba.h): the edges in slot order, every Frame field a float-valued double."""
    mode: int
    cur: ImuState
    prev: ImuState
    cams: list                # one or two ImuCamera
    bf: float
    kind: np.ndarray          # int8 per edge: EDGE_MONO (left / only), EDGE_STEREO, EDGE_BODY (right)
    xw: np.ndarray            # n x 3 double
    obs: np.ndarray           # n x 3 double
    inv_sigma2: np.ndarray    # float32 per edge
    track_depth: np.ndarray   # float32 per edge
    preint: Preintegrated
    C_rw: np.ndarray          # 15 x 15 float32: mpImuPreintegrated->C (the random-walk informations)
    prior: ImuPrior | None = None
    rec_init: bool = False
    truth: ImuState | None = None  # generator only

    def __post_init__(self):
        self.kind = np.ascontiguousarray(self.kind, np.int8)
        self.xw = np.ascontiguousarray(self.xw, np.float64).reshape(-1, 3)
        self.obs = np.ascontiguousarray(self.obs, np.float64).reshape(-1, 3)
        self.inv_sigma2 = np.ascontiguousarray(self.inv_sigma2, np.float32)
        self.track_depth = np.ascontiguousarray(self.track_depth, np.float32)
        self.C_rw = np.ascontiguousarray(self.C_rw, np.float32).reshape(15, 15)

    @property
    def n(self):
        return len(self.kind)

    def struct(self, keep):
        """The C struct; ``keep`` collects the objects whose memory it points into."""
        st = _abi.OsgPoseInertialProblem()
        st.mode, st.rec_init = int(self.mode), int(bool(self.rec_init))
        self.cur.fill(st.cur)
        self.prev.fill(st.prev)
        st.n_cams = len(self.cams)
        for c, k in zip(st.cams, self.cams):
            c.cam = k.cam
            for name in ("Rcw", "tcw", "Rcb", "tcb", "tbc"):
                getattr(c, name)[:] = np.asarray(getattr(k, name), np.float64).ravel().tolist()
        st.bf = float(self.bf)
        st.n_edges = self.n
        st.kind, st.xw, st.obs = _p(self.kind), _p(self.xw), _p(self.obs)
        st.inv_sigma2, st.track_depth = _p(self.inv_sigma2), _p(self.track_depth)
        pre = self.preint.struct()
        keep.append(pre)
        st.preint = C.addressof(pre)
        st.C_rw = _p(self.C_rw)
        if self.prior is not None:
            pr = self.prior.struct()
            keep.append(pr)
            st.prior = C.addressof(pr)
        return st


@dataclass
class PoseInertialResult:
    state: ImuState
    outlier: np.ndarray
    n_inliers: int            # the reference's return value
    rounds_run: int
    iterations: int
    solve_failed: bool
    recovered: bool
    H: np.ndarray             # 15 x 15, as passed to ConstraintPoseImu's constructor
    edge_chi2: np.ndarray     # as read by each edge's last classification


def run_pose_inertial(ctx, probs):
    nb = len(probs)
    keep = []
    ps = (_abi.OsgPoseInertialProblem * max(1, nb))(*[q.struct(keep) for q in probs])
    rs = (_abi.OsgPoseInertialResult * max(1, nb))()
    outl = [np.zeros(q.n, np.uint8) for q in probs]
    chi2 = [np.zeros(q.n, np.float64) for q in probs]
    for r, o, c in zip(rs, outl, chi2):
        r.outlier, r.edge_chi2 = _p(o), _p(c)
    ctx.check(ctx.lib.osg_pose_inertial_optimization_batch(ctx.handle, ps, nb, rs), "PoseInertialOptimization")
    return [PoseInertialResult(ImuState.of(r.state), o, r.n_inliers, r.rounds_run, r.iterations, bool(r.solve_failed),
                               bool(r.recovered), np.array(r.H[:]).reshape(15, 15), c)
            for r, o, c in zip(rs[:nb], outl, chi2)]


def constraint_pose_imu(H):
    """ConstraintPoseImu's constructor (ref:include/G2oTypes.h:825-838) on the H a call returned:
    ``H = (H + H) / 2`` (the upstream line, which symmetrises nothing), then the eigenvalues of the
    self-adjoint solver below 1e-12 set to 0.  Eigen's SelfAdjointEigenSolver reads the lower triangle only,
    and so does ``numpy.linalg.eigh``."""
    H = np.asarray(H, np.float64).reshape(15, 15)
    H = (H + H) / 2
    w, V = np.linalg.eigh(H, UPLO="L")
    w = np.where(w < 1e-12, 0.0, w)
    return (V * w) @ V.T


# EuRoC-like body-from-camera extrinsic (a 90 degree class rotation and a few centimetres)
_TBC_R = np.array([[0.0148655429818, -0.999880929698, 0.00414029679422],
                   [0.999557249008, 0.0149672133247, 0.025715529948],
                   [-0.0257744366974, 0.00375618835797, 0.999660727178]])
_TBC_T = np.array([-0.0216401454975, -0.064676986768, 0.00981073058949])


def _so3_exp(w):
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < 1e-9:
        return np.eye(3) + K
    return np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * K @ K


def _orthonormal(R):
    U, _, Vt = np.linalg.svd(R)
    return U @ Vt


def synth_pose_inertial_problem(rng, n_edges=300, mode=_abi.OSG_PIO_LAST_KEYFRAME, cam="pinhole_mono", outlier_frac=0.1,
                                n_levels=8, rec_init=False, n_behind=0, dt=None, pose_err=(0.3, 0.01),
                                null_prior=False, prior=None, prev=None):
    """A consistent two-state visual-inertial problem: a previous state, a constant body-frame rotation rate and
    acceleration over dt, the current state integrated from them, preintegrated deltas that agree with the pair
    up to noise, a covariance from EuRoC-like noise densities at 200 Hz, and visual edges of the current frame's
    true pose with outliers.  ``cam``: "pinhole_mono", "pinhole_stereo" (60 % stereo edges) or "kb8_rig" (half of
    the edges in the right camera).  ``n_behind`` edges get a point behind the camera.  ``null_prior``
    (LastFrame): the previous accelerometer bias is held by a 5e-7 random-walk information and a 1e-7 prior
    alone, so the block that Marginalize inverts has three eigenvalues of 6e-7, below its 1e-6 cut.  ``prior`` / ``prev`` chain a call after another."""
    last_frame = mode == _abi.OSG_PIO_LAST_FRAME
    if dt is None:
        dt = 0.05 if last_frame else 0.25
    g = np.array([0, 0, -float(np.float32(9.81))])
    # previous state
    if prev is None:
        prev = ImuState(_f32(_orthonormal(small_rotation(rng, 30.0))), _f32(rng.normal(0, 1.0, 3)),
                        _f32(rng.normal(0, 0.5, 3)), _f32(rng.normal(0, 2e-3, 3)), _f32(rng.normal(0, 2e-2, 3)))
    # the true motion and its preintegration (bias of the integration = the previous state's, as Tracking leaves it)
    w, a = rng.normal(0, 0.3, 3), rng.normal(0, 1.0, 3)
    dR = _so3_exp(w * dt)
    dV = a * dt
    dP = 0.5 * a * dt * dt
    R1 = prev.Rwb
    R2 = R1 @ dR
    v2 = prev.v + g * dt + R1 @ dV
    p2 = prev.twb + prev.v * dt + 0.5 * g * dt * dt + R1 @ dP
    n_imu = max(1, int(round(dt * 200)))
    sg, sa = 1.7e-4 * np.sqrt(200.0), 2.0e-3 * np.sqrt(200.0)
    sgw, saw = 1.9e-5 / np.sqrt(200.0), 3.0e-3 / np.sqrt(200.0)
    h = dt / n_imu
    var = np.concatenate([np.full(3, n_imu * (sg * h) ** 2), np.full(3, n_imu * (sa * h) ** 2),
                          np.full(3, n_imu * (0.5 * sa * h * h) ** 2 * n_imu ** 2 / 3 + 1e-14),
                          np.full(3, n_imu * sgw ** 2), np.full(3, n_imu * saw ** 2)])
    M = np.eye(15)
    M[:9, :9] += 0.05 * rng.normal(size=(9, 9))
    Cm = (M * var) @ M.T
    Cm[9:, :9] = 0
    Cm[:9, 9:] = 0
    Cm[9:12, 12:] = 0
    Cm[12:, 9:12] = 0
    if null_prior:
        Cm = Cm * 1e6  # a poor IMU: every information at most ~1e4, which keeps the system solvable in double
    C_rw = Cm.copy()
    if null_prior:
        C_rw[12:, 12:] = np.eye(3) * 2e6
    noise = rng.normal(size=9) * np.sqrt(var[:9])
    pre = Preintegrated(dR @ _so3_exp(noise[:3]), dV + noise[3:6], dP + noise[6:9],
                        -dt * np.eye(3) + 0.01 * dt * rng.normal(size=(3, 3)), 0.5 * dt * dt * rng.normal(size=(3, 3)),
                        (-dt * dR * 0 - dt * np.eye(3) + 0.02 * dt * rng.normal(size=(3, 3))) * (0 if null_prior else 1),
                        0.1 * dt ** 3 * rng.normal(size=(3, 3)),
                        (-0.5 * dt * dt * np.eye(3) + 0.01 * dt * dt * rng.normal(size=(3, 3))) * (0 if null_prior else 1),
                        np.concatenate([prev.ba, prev.bg]), dt, Cm)
    truth = ImuState(R2, p2, v2, prev.bg, prev.ba)
    # the predicted current state (what PredictStateIMU leaves in the Frame): off the truth by pose_err
    Rp = _orthonormal(R2 @ small_rotation(rng, pose_err[0]))
    cur = ImuState(_f32(Rp), _f32(p2 + rng.normal(0, pose_err[1], 3)), _f32(v2 + rng.normal(0, 0.02, 3)),
                   _f32(prev.bg), _f32(prev.ba))
    if last_frame and prior is None:
        D = np.sqrt(np.array([1e6] * 3 + [1e5] * 3 + [1e4] * 3 + [1e8] * 3 + [1e5] * 3))
        B = (np.eye(15) + 0.1 * rng.normal(size=(15, 15))) * D[:, None]
        Hp = B @ B.T
        if null_prior:
            Hp *= 1e-6
            Hp[12:, :] = 0
            Hp[:, 12:] = 0
            Hp[12:, 12:] = 1e-7 * np.eye(3)
        prior = ImuPrior(prev.Rwb @ small_rotation(rng, 0.02), prev.twb + rng.normal(0, 1e-3, 3),
                         prev.v + rng.normal(0, 1e-3, 3), prev.bg + rng.normal(0, 1e-5, 3),
                         prev.ba + rng.normal(0, 1e-4, 3), constraint_pose_imu(Hp))
    # cameras
    Rcb, tcb = _TBC_R.T, -_TBC_R.T @ _TBC_T
    rig = cam == "kb8_rig"
    model = kb8_camera() if rig else pinhole_camera()

    def cam_pose(S, Rcb_, tcb_):
        Rbw = S.Rwb.T
        return Rcb_ @ Rbw, Rcb_ @ (-Rbw @ S.twb) + tcb_

    Rcb0, tcb0, tbc0 = _f32(Rcb), _f32(tcb), _f32(_TBC_T)
    Rcw0, tcw0 = (_f32(a) for a in cam_pose(cur, Rcb0, tcb0))
    cams = [ImuCamera(model, Rcw0, tcw0, Rcb0, tcb0, tbc0)]
    if rig:
        q = np.array(TUMVI_TRL[:4]) / np.linalg.norm(TUMVI_TRL[:4])
        Rrl, trl = _f32(quat_to_rot(q)), _f32(TUMVI_TRL[4:])
        Rcb1 = Rrl @ Rcb0
        tcb1 = Rrl @ tcb0 + trl
        cams.append(ImuCamera(kb8_camera(), Rrl @ Rcw0, Rrl @ tcw0 + trl, Rcb1, tcb1, -Rcb1.T @ tcb1))
    # points seen from the true pose
    n = n_edges
    true_cams = [cam_pose(truth, k.Rcb, k.tcb) for k in cams]
    ci = (rng.random(n) < 0.5).astype(int) if rig else np.zeros(n, int)
    z = rng.uniform(2.0, 20.0, n)
    if rig:
        th, ps = rng.uniform(0.05, 1.1, n), rng.uniform(-np.pi, np.pi, n)
        Xc = np.stack([z * np.sin(th) * np.cos(ps), z * np.sin(th) * np.sin(ps), z * np.cos(th)], 1)
    else:
        u, v = rng.uniform(20, EUROC_W - 20, n), rng.uniform(20, EUROC_H - 20, n)
        Xc = np.stack([(u - EUROC_CX) / EUROC_FX * z, (v - EUROC_CY) / EUROC_FY * z, z], 1)
    Xw = np.zeros((n, 3))
    for c, (Rc, tc) in enumerate(true_cams):
        m = ci == c
        Xw[m] = (Xc[m] - tc) @ Rc
    Xw = _f32(Xw)
    octv = rng.choice(n_levels, n, p=np.array([1.2 ** -i for i in range(n_levels)]) / sum(1.2 ** -i for i in range(n_levels)))
    sig = 1.2 ** octv
    obs = np.zeros((n, 3))
    depth = np.zeros(n)
    for c, (Rc, tc) in enumerate(true_cams):
        m = ci == c
        Xm = Xw[m] @ Rc.T + tc
        obs[m, :2] = _project(cams[c].cam, Xm)
        depth[m] = Xm[:, 2]
    obs[:, 0] += rng.normal(0, 1, n) * sig
    obs[:, 1] += rng.normal(0, 1, n) * sig
    out = rng.random(n) < outlier_frac
    obs[out, 0] += rng.uniform(8, 40, out.sum()) * rng.choice([-1, 1], out.sum())
    obs[out, 1] += rng.uniform(8, 40, out.sum()) * rng.choice([-1, 1], out.sum())
    stereo = (rng.random(n) < 0.6) if cam == "pinhole_stereo" else np.zeros(n, bool)
    bf = float(np.float32(EUROC_BF)) if not rig else 0.0
    obs[:, 2] = np.where(stereo, obs[:, 0] - bf / np.maximum(depth, 0.1) + rng.normal(0, 0.5, n), 0.0)
    kind = np.where(stereo, _abi.EDGE_STEREO, np.where(ci == 1, _abi.EDGE_BODY, _abi.EDGE_MONO)).astype(np.int8)
    for i in range(min(n_behind, n)):  # a wrong match to a point behind the camera, observed where it would mirror
        Rc, tc = true_cams[ci[i]]
        Xb = np.array([rng.normal(0, 0.5), rng.normal(0, 0.5), -rng.uniform(2, 5)])
        Xw[i] = _f32((Xb - tc) @ Rc)
        kind[i] = _abi.EDGE_BODY if ci[i] == 1 else _abi.EDGE_MONO
        obs[i, 2] = 0.0
    return PoseInertialProblem(mode, cur, prev, cams, bf, kind, Xw, _f32(obs), inv_level_sigma2(n_levels)[octv],
                               np.maximum(depth, 0.0).astype(np.float32), pre, C_rw, prior, rec_init, truth)


# ------------------------------------------------------------------------------------- InertialOptimization
@dataclass
class InertialMap:
    """What the three overloads of ``Optimizer::InertialOptimization`` read of a map: the KeyFrames with
    ``mnId <= maxKFid`` (fixed IMU poses, velocities), one edge per KeyFrame with a usable ``mPrevKF``, and
    ``vpKFs.front()``'s bias, the start of the bias vertices."""
    Rwb: np.ndarray           # n x 3 x 3 double
    twb: np.ndarray           # n x 3
    v: np.ndarray             # n x 3
    prev: np.ndarray          # per edge: index of mPrevKF
    cur: np.ndarray           # per edge: index of the KeyFrame that owns the preintegration
    preint: list              # per edge: Preintegrated (or anything with its float32 fields)
    bg: np.ndarray = field(default_factory=lambda: np.zeros(3))
    ba: np.ndarray = field(default_factory=lambda: np.zeros(3))

    def __post_init__(self):
        self.Rwb = np.ascontiguousarray(self.Rwb, np.float64).reshape(-1, 3, 3)
        self.twb = np.ascontiguousarray(self.twb, np.float64).reshape(-1, 3)
        self.v = np.ascontiguousarray(self.v, np.float64).reshape(-1, 3)
        self.prev = np.ascontiguousarray(self.prev, np.int32).reshape(-1)
        self.cur = np.ascontiguousarray(self.cur, np.int32).reshape(-1)
        self.bg = np.ascontiguousarray(self.bg, np.float64).reshape(3)
        self.ba = np.ascontiguousarray(self.ba, np.float64).reshape(3)
        self.preint = list(self.preint)


@dataclass
class InertialProblem:
    """One ``osg_inertial_problem`` (include/osg_ba.h)."""
    map: InertialMap
    Rwg: np.ndarray
    scale: float
    prior_g: float = 0.0
    prior_a: float = 0.0
    has_priors: bool = False
    free_vel_bias: bool = True
    free_gdir: bool = True
    free_scale: bool = True
    algorithm: int = _abi.OSG_INERTIAL_LM
    iterations: int = 200
    lambda_init: float = 0.0
    huber_delta: float = 0.0

    def __post_init__(self):
        self.Rwg = np.ascontiguousarray(self.Rwg, np.float64).reshape(3, 3)

    @property
    def n(self):
        return len(self.map.twb)

    def struct(self, keep):
        """The C struct; ``keep`` collects the objects whose memory it points into."""
        m = self.map
        st = _abi.OsgInertialProblem()
        st.n_kf, st.Rwb, st.twb, st.v = self.n, _p(m.Rwb), _p(m.twb), _p(m.v)
        st.n_edges, st.prev, st.cur = len(m.prev), _p(m.prev), _p(m.cur)
        if len(m.preint) != len(m.prev) or len(m.cur) != len(m.prev):
            raise ValueError("one preintegration, one prev and one cur per edge")
        if m.preint:
            arr = (_abi.OsgPioPreintegrated * len(m.preint))()
            for a, q in zip(arr, m.preint):
                for k in ("dR", "dV", "dP", "JRg", "JVg", "JVa", "JPg", "JPa", "b", "C"):
                    getattr(a, k)[:] = np.asarray(getattr(q, k), np.float32).ravel().tolist()
                a.dT = float(q.dT)
            keep.append(arr)
            st.preint = C.addressof(arr)
        st.bg[:], st.ba[:], st.Rwg[:] = m.bg.tolist(), m.ba.tolist(), self.Rwg.ravel().tolist()
        st.scale, st.prior_g, st.prior_a = float(self.scale), float(self.prior_g), float(self.prior_a)
        st.has_priors, st.free_vel_bias = int(bool(self.has_priors)), int(bool(self.free_vel_bias))
        st.free_gdir, st.free_scale = int(bool(self.free_gdir)), int(bool(self.free_scale))
        st.algorithm, st.iterations = int(self.algorithm), int(self.iterations)
        st.lambda_init, st.huber_delta = float(self.lambda_init), float(self.huber_delta)
        return st


@dataclass
class InertialResult:
    v: np.ndarray             # n x 3, in the problem's KeyFrame order
    bg: np.ndarray
    ba: np.ndarray
    Rwg: np.ndarray
    scale: float
    chi2_initial: float
    chi2_final: float
    iterations: int
    trials_rejected: int
    solve_failed: bool
    trace: np.ndarray         # iterations x (chi2, lambda, trials)


def inertial_initialization_problem(map, Rwg, scale, bg=None, ba=None, mono=True, fixed_vel=False, prior_g=1e2,
                                    prior_a=1e6, iterations=200):
    """Overload 1 (ref:src/Optimizer.cc:3706-3898): Levenberg-Marquardt, lambda_init 1e3 only if ``prior_g`` is not
    zero, velocities and biases free unless ``fixed_vel``, the gravity direction free, the scale free only if
    ``mono``.  ``bg`` / ``ba`` replace the map's (``vpKFs.front()``'s bias) when given."""
    if bg is not None or ba is not None:
        map = replace(map, bg=map.bg if bg is None else bg, ba=map.ba if ba is None else ba)
    pg, pa = float(np.float32(prior_g)), float(np.float32(prior_a))
    return InertialProblem(map, Rwg, scale, pg, pa, True, not fixed_vel, True, bool(mono), _abi.OSG_INERTIAL_LM,
                           iterations, 1e3 if pg != 0.0 else 0.0, 0.0)


def inertial_bias_problem(map, prior_g=1e2, prior_a=1e6, iterations=200):
    """Overload 2 (ref:src/Optimizer.cc:3910-4076): Levenberg-Marquardt with lambda_init 1e3, the gravity direction
    (identity) and the scale (1) fixed, velocities and biases free."""
    pg, pa = float(np.float32(prior_g)), float(np.float32(prior_a))
    return InertialProblem(map, np.eye(3), 1.0, pg, pa, True, True, False, False, _abi.OSG_INERTIAL_LM, iterations,
                           1e3, 0.0)


def inertial_scale_refinement_problem(map, Rwg, scale, iterations=10):
    """Overload 3 (ref:src/Optimizer.cc:4085-4197): Gauss-Newton, only the gravity direction and the scale free,
    Huber with delta 1 on every inertial edge, no prior edges."""
    return InertialProblem(map, Rwg, scale, 0.0, 0.0, False, False, True, True, _abi.OSG_INERTIAL_GN, iterations,
                           0.0, 1.0)


def inertial_check(problem) -> int:
    """``osg_inertial_check``: 0 or OSG_E_INVALID (host only, no context)."""
    from . import load_library

    keep = []
    st = problem.struct(keep)
    return load_library().osg_inertial_check(C.byref(st))


def run_inertial(ctx, probs):
    nb = len(probs)
    keep = []
    ps = (_abi.OsgInertialProblem * max(1, nb))(*[q.struct(keep) for q in probs])
    rs = (_abi.OsgInertialResult * max(1, nb))()
    vs = [np.zeros((q.n, 3), np.float64) for q in probs]
    trs = [np.zeros((max(1, q.iterations), 3), np.float64) for q in probs]
    for r, v, t in zip(rs, vs, trs):
        r.v, r.trace = _p(v), _p(t)
    ctx.check(ctx.lib.osg_inertial_optimization_batch(ctx.handle, ps, nb, rs), "InertialOptimization")
    return [InertialResult(v, np.array(r.bg[:]), np.array(r.ba[:]), np.array(r.Rwg[:]).reshape(3, 3), r.scale,
                           r.chi2_initial, r.chi2_final, r.iterations, r.trials_rejected, bool(r.solve_failed),
                           t[:r.iterations].copy())
            for r, v, t in zip(rs[:nb], vs, trs)]


def initial_gravity_rotation(Rwb_prev, preint):
    """The ``dirG`` -> ``Rwg`` start value of ``LocalMapping::InitializeIMU`` (ref:src/LocalMapping.cc:1606-1654) in
    float32: ``Rwb_prev[i]`` is ``mPrevKF->GetImuRotation()`` and ``preint[i]`` the preintegration of the i-th
    KeyFrame that has both.  Returns the 3 x 3 float32 ``Rwg``, or None where the reference gives up
    (``have_imu_num < 6``).  ``GetUpdatedDeltaVelocity`` is ``dV + JVg db[0:3] + JVa db[3:6]`` with
    ``db = bu - b`` (zero unless the preintegration carries a ``bu``)."""
    f = np.float32
    dirG = np.zeros(3, f)
    n = 0
    for R, q in zip(Rwb_prev, preint):
        dV = np.asarray(q.dV, f)
        bu = getattr(q, "bu", None)
        if bu is not None:
            b, bu = np.asarray(q.b, f), np.asarray(bu, f)
            dV = dV + np.asarray(q.JVg, f) @ (bu[3:] - b[3:]) + np.asarray(q.JVa, f) @ (bu[:3] - b[:3])
        dirG = dirG - np.asarray(R, f).reshape(3, 3) @ dV
        n += 1
    if n < 6:
        return None
    dirG = dirG / f(np.sqrt(f(dirG @ dirG)))
    gI = np.array([0.0, 0.0, -1.0], f)
    v = np.cross(gI, dirG).astype(f)
    nv = f(np.sqrt(f(v @ v)))
    ang = f(np.arccos(f(gI @ dirG)))
    vzg = v * ang / nv
    return _so3f_exp_matrix(vzg)


def _so3f_exp_matrix(w):
    """Sophus::SO3f::exp(w).matrix() in float32 (the unit quaternion of the half angle, then toRotationMatrix)."""
    f = np.float32
    w = np.asarray(w, f)
    theta_sq = f(w @ w)
    if theta_sq < f(1e-5) * f(1e-5):
        po4 = f(theta_sq * theta_sq)
        imag = f(0.5) - f(1.0 / 48.0) * theta_sq + f(1.0 / 3840.0) * po4
        real = f(1.0) - f(1.0 / 8.0) * theta_sq + f(1.0 / 384.0) * po4
    else:
        theta = f(np.sqrt(theta_sq))
        half = f(0.5) * theta
        imag, real = f(np.sin(half)) / theta, f(np.cos(half))
    x, y, z = (f(imag * c) for c in w)
    tx, ty, tz = f(2) * x, f(2) * y, f(2) * z
    twx, twy, twz = tx * real, ty * real, tz * real
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return np.array([[1 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1 - (txx + tzz), tyz - twx],
                     [txz - twy, tyz + twx, 1 - (txx + tyy)]], f)


# ------------------------------------------------------------------------------------- LocalInertialBA
@dataclass
class LibaKeyFrame:
    """One KeyFrame of a LocalInertialBA window: its four vertices and ``ImuCamPose(KeyFrame*)``'s cameras."""
    state: ImuState
    cams: list                # one or two ImuCamera
    bf: float
    fixed: bool = False


@dataclass
class LibaLink:
    """EdgeInertial + EdgeGyroRW + EdgeAccRW between ``prev`` (mPrevKF) and ``cur``."""
    prev: int
    cur: int
    preint: Preintegrated
    huber: bool = False       # i == N - 1 || bRecInit
    downweight: bool = False  # i == N - 1


@dataclass
class LocalInertialBAProblem:
    """One ``osg_local_inertial_ba_problem`` (include/osg_ba.h): the g2o part of ``Optimizer::LocalInertialBA``
    (ref:src/Optimizer.cc:2356-2743) as arrays, in the reference's insertion order."""
    kfs: list                 # LibaKeyFrame
    xw: np.ndarray            # n_points x 3 double
    track_depth: np.ndarray   # float32 per point
    e_point: np.ndarray       # int32 per visual edge
    e_kf: np.ndarray
    e_kind: np.ndarray        # int8: EDGE_MONO (EdgeMono(0)), EDGE_STEREO, EDGE_BODY (EdgeMono(1))
    e_obs: np.ndarray         # n_edges x 3 double
    e_inv_sigma2: np.ndarray  # float32
    links: list               # LibaLink
    iterations: int = 10
    large: bool = False
    lambda_init: float = 1.0
    truth: object = None      # generator only: (list of ImuState, n_points x 3)

    def __post_init__(self):
        self.xw = np.ascontiguousarray(self.xw, np.float64).reshape(-1, 3)
        self.track_depth = np.ascontiguousarray(self.track_depth, np.float32).reshape(-1)
        self.e_point = np.ascontiguousarray(self.e_point, np.int32).reshape(-1)
        self.e_kf = np.ascontiguousarray(self.e_kf, np.int32).reshape(-1)
        self.e_kind = np.ascontiguousarray(self.e_kind, np.int8).reshape(-1)
        self.e_obs = np.ascontiguousarray(self.e_obs, np.float64).reshape(-1, 3)
        self.e_inv_sigma2 = np.ascontiguousarray(self.e_inv_sigma2, np.float32).reshape(-1)

    @property
    def n_kf(self):
        return len(self.kfs)

    @property
    def n_points(self):
        return len(self.xw)

    @property
    def n_edges(self):
        return len(self.e_point)

    def struct(self, keep):
        """The C struct; ``keep`` collects the objects whose memory it points into."""
        st = _abi.OsgLocalInertialBaProblem()
        kf = (_abi.OsgLibaKeyframe * max(1, self.n_kf))()
        for d, k in zip(kf, self.kfs):
            k.state.fill(d.state)
            d.fixed, d.n_cams, d.bf = int(bool(k.fixed)), len(k.cams), float(k.bf)
            for c, m in zip(d.cams, k.cams):
                c.cam = m.cam
                for name in ("Rcw", "tcw", "Rcb", "tcb", "tbc"):
                    getattr(c, name)[:] = np.asarray(getattr(m, name), np.float64).ravel().tolist()
        ln = (_abi.OsgLibaLink * max(1, len(self.links)))()
        for d, l in zip(ln, self.links):
            d.prev, d.cur, d.huber, d.downweight = int(l.prev), int(l.cur), int(bool(l.huber)), int(bool(l.downweight))
            q = l.preint
            for name in ("dR", "dV", "dP", "JRg", "JVg", "JVa", "JPg", "JPa", "b", "C"):
                getattr(d.preint, name)[:] = np.asarray(getattr(q, name), np.float32).ravel().tolist()
            d.preint.dT = float(q.dT)
        keep.extend([kf, ln])
        st.n_kf, st.kf = self.n_kf, C.addressof(kf)
        st.n_points, st.xw, st.track_depth = self.n_points, _p(self.xw), _p(self.track_depth)
        st.n_edges, st.e_point, st.e_kf, st.e_kind = self.n_edges, _p(self.e_point), _p(self.e_kf), _p(self.e_kind)
        st.e_obs, st.e_inv_sigma2 = _p(self.e_obs), _p(self.e_inv_sigma2)
        st.n_links, st.links = len(self.links), C.addressof(ln)
        st.iterations, st.large, st.lambda_init = int(self.iterations), int(bool(self.large)), float(self.lambda_init)
        return st


@dataclass
class LocalInertialBAResult:
    states: list              # ImuState per KeyFrame
    Rcw: np.ndarray           # n_kf x 3 x 3: camera 0, for SetPose
    tcw: np.ndarray           # n_kf x 3
    xw: np.ndarray            # n_points x 3
    edge_bad: np.ndarray      # the function's erase rule per visual edge
    edge_chi2: np.ndarray
    chi2_initial: float       # err
    chi2_last: float          # err_end
    chi2_accepted: float
    iterations: int
    trials_rejected: int
    solve_failed: bool
    failed: bool              # the reference returns before any write
    trace: np.ndarray         # iterations x (chi2, lambda, trials)


def local_inertial_ba_check(problem) -> int:
    """``osg_local_inertial_ba_check``: 0 or OSG_E_INVALID (host only, no context)."""
    from . import load_library

    keep = []
    st = problem.struct(keep)
    return load_library().osg_local_inertial_ba_check(C.byref(st))


def run_local_inertial_ba(ctx, probs):
    nb = len(probs)
    keep = []
    ps = (_abi.OsgLocalInertialBaProblem * max(1, nb))(*[q.struct(keep) for q in probs])
    rs = (_abi.OsgLocalInertialBaResult * max(1, nb))()
    bufs = []
    for r, q in zip(rs, probs):
        b = dict(state=(_abi.OsgPioState * max(1, q.n_kf))(), Rcw=np.zeros((q.n_kf, 3, 3)), tcw=np.zeros((q.n_kf, 3)),
                 xw=np.zeros((q.n_points, 3)), bad=np.zeros(q.n_edges, np.uint8), chi2=np.zeros(q.n_edges),
                 trace=np.zeros((max(1, q.iterations), 3)))
        r.state, r.Rcw, r.tcw, r.xw = C.addressof(b["state"]), _p(b["Rcw"]), _p(b["tcw"]), _p(b["xw"])
        r.edge_bad, r.edge_chi2, r.trace = _p(b["bad"]), _p(b["chi2"]), _p(b["trace"])
        bufs.append(b)
    ctx.check(ctx.lib.osg_local_inertial_ba_batch(ctx.handle, ps, nb, rs), "LocalInertialBA")
    return [LocalInertialBAResult([ImuState.of(s) for s in b["state"][:q.n_kf]], b["Rcw"], b["tcw"], b["xw"], b["bad"],
                                  b["chi2"], r.chi2_initial, r.chi2_last, r.chi2_accepted, r.iterations,
                                  r.trials_rejected, bool(r.solve_failed), bool(r.failed),
                                  b["trace"][:r.iterations].copy())
            for r, q, b in zip(rs[:nb], probs, bufs)]


def synth_local_inertial_window(rng, truth, preints, n_points=100, cam="pinhole_mono", n_extra_fixed=0, large=False,
                                rec_init=False, iterations=None, outlier_frac=0.05, pixel_noise=1.0,
                                pose_err=(0.2, 0.01), vel_err=0.02, point_err=0.02, linkless=False, n_seen_once=1,
                                n_fixed_only=1, p_obs=0.8, n_levels=8, wide_point=False):
    """A LocalInertialBA window around a given trajectory.  ``truth``: the true ImuState of the chain, oldest first;
    ``truth[0]`` is the fixed KeyFrame before the window and the rest are free.  ``preints[i]`` is the
    preintegration from ``truth[i]`` to ``truth[i + 1]``.  KeyFrames are numbered as the reference visits them:
    the free ones from the newest (0) to the oldest (N - 1), the fixed predecessor (N), then ``n_extra_fixed``
    covisible fixed KeyFrames around the trajectory.  Link i joins free KeyFrame i to KeyFrame i + 1; the oldest
    one is downweighted and robust, all are robust under ``rec_init``; ``linkless`` drops the newest one's.
    ``cam``: "pinhole_mono", "pinhole_stereo" or "kb8_rig" (left and right observations, the right ones EdgeMono(1)).
    Points are seen by each KeyFrame in view with probability ``p_obs`` (``wide_point``: point 0 by all of them);
    ``n_seen_once`` points keep one observation and ``n_fixed_only`` points only those of fixed KeyFrames.
    Observations carry pixel noise and a share of outliers; free poses, velocities and points are perturbed."""
    N = len(truth) - 1
    if N < 1 or len(preints) != N:
        raise ValueError("truth holds the fixed predecessor and the free KeyFrames; one preintegration per step")
    rig, stereo = cam == "kb8_rig", cam == "pinhole_stereo"
    model = kb8_camera() if rig else pinhole_camera()
    bf = 0.0 if rig else float(np.float32(EUROC_BF))
    Rcb0, tcb0, tbc0 = _f32(_TBC_R.T), _f32(-_TBC_R.T @ _TBC_T), _f32(_TBC_T)
    ext = [(Rcb0, tcb0, tbc0)]
    if rig:
        q = np.array(TUMVI_TRL[:4]) / np.linalg.norm(TUMVI_TRL[:4])
        Rrl, trl = _f32(quat_to_rot(q)), _f32(TUMVI_TRL[4:])
        Rcb1 = Rrl @ Rcb0
        tcb1 = Rrl @ tcb0 + trl
        ext.append((Rcb1, tcb1, -Rcb1.T @ tcb1))

    def cam_pose(S, e):
        Rbw = S.Rwb.T
        return e[0] @ Rbw, e[0] @ (-Rbw @ S.twb) + e[1]

    order = list(range(N, 0, -1)) + [0]              # KeyFrame index -> position in truth
    true_states = [truth[i] for i in order]
    for _ in range(n_extra_fixed):
        a = true_states[int(rng.integers(0, N + 1))]
        true_states.append(ImuState(_orthonormal(a.Rwb @ small_rotation(rng, 4.0)), a.twb + rng.normal(0, 0.15, 3),
                                    np.zeros(3), np.zeros(3), np.zeros(3)))
    nk = len(true_states)
    fixed = [k >= N for k in range(nk)]
    # points: in view of a random KeyFrame's left camera
    W, Hh = (512, 512) if rig else (EUROC_W, EUROC_H)
    Xw = np.zeros((n_points, 3))
    for p in range(n_points):
        Rc, tc = cam_pose(true_states[int(rng.integers(0, nk))], ext[0])
        z = rng.uniform(2.0, 9.0) if rng.random() < 0.5 else rng.uniform(11.0, 25.0)
        if rig:
            th, ps = rng.uniform(0.05, 0.9), rng.uniform(-np.pi, np.pi)
            Xc = z * np.array([np.sin(th) * np.cos(ps), np.sin(th) * np.sin(ps), np.cos(th)])
        else:
            u, v = rng.uniform(60, W - 60), rng.uniform(60, Hh - 60)
            Xc = np.array([(u - EUROC_CX) / EUROC_FX * z, (v - EUROC_CY) / EUROC_FY * z, z])
        Xw[p] = Rc.T @ (Xc - tc)
    if wide_point:                                   # far away on the optical axis of the middle KeyFrame
        Rc, tc = cam_pose(true_states[N // 2], ext[0])
        Xw[0] = Rc.T @ (np.array([0.0, 0.0, 20.0]) - tc)
    sig2 = inv_level_sigma2(n_levels)
    p_octave = np.array([1.2 ** -i for i in range(n_levels)]) / sum(1.2 ** -i for i in range(n_levels))
    e_point, e_kf, e_kind, e_obs, e_w = [], [], [], [], []
    depth0 = np.zeros(n_points)
    for p in range(n_points):
        seen = []
        for k in range(nk):
            for ci in range(len(ext)):
                Rc, tc = cam_pose(true_states[k], ext[ci])
                Xc = Rc @ Xw[p] + tc
                if Xc[2] < 0.5:
                    continue
                uv = _project(model, Xc[None])[0]
                if not (5 < uv[0] < W - 5 and 5 < uv[1] < Hh - 5):
                    continue
                if k == 0 and ci == 0:
                    depth0[p] = Xc[2]
                if not (wide_point and p == 0 and ci == 0) and rng.random() > p_obs:
                    continue
                seen.append((k, ci, uv, Xc[2]))
        q = p - (1 if wide_point else 0)             # the special points come after the wide one
        if 0 <= q < n_seen_once:
            seen = seen[:1]
        elif n_seen_once <= q < n_seen_once + n_fixed_only:
            seen = [s for s in seen if fixed[s[0]]]
        for k, ci, uv, z in seen:
            octv = int(rng.choice(n_levels, p=p_octave))
            o = np.zeros(3)
            o[:2] = uv + rng.normal(0, pixel_noise, 2) * 1.2 ** octv
            if rng.random() < outlier_frac:
                o[:2] += rng.uniform(8, 40, 2) * rng.choice([-1, 1], 2)
            kind = _abi.EDGE_BODY if ci == 1 else _abi.EDGE_MONO
            if stereo and z < 12.0:
                kind = _abi.EDGE_STEREO
                o[2] = o[0] - bf / z + rng.normal(0, 0.5 * pixel_noise)
            e_point.append(p), e_kf.append(k), e_kind.append(kind), e_obs.append(_f32(o)), e_w.append(sig2[octv])
    depth = np.where(depth0 > 0, depth0, rng.uniform(3.0, 20.0, n_points))
    # the estimates the window starts from
    kfs = []
    for k, S in enumerate(true_states):
        if fixed[k]:
            est = ImuState(_f32(S.Rwb), _f32(S.twb), _f32(S.v), _f32(S.bg), _f32(S.ba))
        else:
            est = ImuState(_f32(_orthonormal(S.Rwb @ small_rotation(rng, pose_err[0]))),
                           _f32(S.twb + rng.normal(0, pose_err[1], 3)), _f32(S.v + rng.normal(0, vel_err, 3)),
                           _f32(S.bg), _f32(S.ba))
        cams = []
        for e in ext:
            Rc, tc = cam_pose(est, e)
            cams.append(ImuCamera(model, _f32(Rc), _f32(tc), e[0], e[1], e[2]))
        kfs.append(LibaKeyFrame(est, cams, bf, fixed[k]))
    links = [LibaLink(i + 1, i, preints[N - 1 - i], huber=(i == N - 1 or rec_init), downweight=(i == N - 1))
             for i in range(N) if not (linkless and i == 0)]
    X0 = _f32(Xw + rng.normal(0, point_err, Xw.shape))
    if iterations is None:
        iterations = 4 if large else 10
    return LocalInertialBAProblem(kfs, X0, depth.astype(np.float32), e_point, e_kf, e_kind,
                                  np.array(e_obs).reshape(-1, 3), np.array(e_w, np.float32), links, iterations, large,
                                  1e-2 if large else 1.0, truth=(true_states, Xw))
