"""Host mirror of ``ORB_SLAM3::MLPnPsolver`` (ref:include/MLPnPsolver.h, ref:src/MLPnPsolver.cpp) on the C
ABI in include/osg_ba.h: every RANSAC hypothesis of every relocalisation candidate is evaluated on the GPU
in one launch and the reference's sequential rule ("the first hypothesis with more than min_inliers inliers
returns; otherwise the first that attains the largest count") is replayed on the inlier counts.

The constructor's gather from the Frame and its MapPoint matches (ref:src/MLPnPsolver.cpp:68-133) is the
adapter's job; here a problem is given directly as the kept matches and the sample sets in draw order.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field

import numpy as np

from . import Context, _abi, load_library, synth
from .optimizer import _p, pinhole_camera
from .sim3solver import level_sigma2

F = np.float32
TH2 = 5.991  # Tracking::Relocalization's th2


@dataclass
class MlpnpProblem:
    bearing: np.ndarray       # n x 3 float32: unproject(kp.pt) / z
    p3dw: np.ndarray          # n x 3 float32: mvP3Dw
    p2d: np.ndarray           # n x 2 float32: mvP2D
    max_err: np.ndarray       # float32 per match: mvMaxError
    samples: np.ndarray       # H x 6 int32, in draw order
    min_inliers: int = 10
    cam: object = field(default_factory=pinhole_camera)
    truth: tuple | None = None  # generator only: (R, t, outlier flags)

    def __post_init__(self):
        self.bearing = np.ascontiguousarray(self.bearing, F).reshape(-1, 3)
        self.p3dw = np.ascontiguousarray(self.p3dw, F).reshape(-1, 3)
        self.p2d = np.ascontiguousarray(self.p2d, F).reshape(-1, 2)
        self.max_err = np.ascontiguousarray(self.max_err, F)
        self.samples = np.ascontiguousarray(self.samples, np.int32).reshape(-1, 6)

    @property
    def n(self):
        return len(self.p3dw)

    @property
    def n_hyp(self):
        return len(self.samples)

    def struct(self):
        st = _abi.OsgMlpnpProblem()
        st.n = self.n
        st.bearing, st.p3dw, st.p2d, st.max_err = _p(self.bearing), _p(self.p3dw), _p(self.p2d), _p(self.max_err)
        st.cam = self.cam
        st.min_inliers = int(self.min_inliers)
        st.n_hyp = self.n_hyp
        st.samples = _p(self.samples)
        return st


@dataclass
class MlpnpResult:
    converged: bool
    hyp: int                  # the returned hypothesis (-1: none reached min_inliers, or nothing evaluated)
    n_iterations: int         # mnIterations
    n_inliers: int            # nInliers
    n_best: int               # mnBestInliers
    Tcw: np.ndarray           # 4 x 4 float32
    R: np.ndarray             # 3 x 3 float64
    t: np.ndarray             # 3 float64
    inlier: np.ndarray        # n flags of hyp
    hyp_inliers: np.ndarray   # H counts
    hyp_pose: np.ndarray      # H x 12 float64: R[9] t[3]
    hyp_info: np.ndarray      # H x 3 int32: planar, Gauss-Newton solves, end (0 five iterations, 1 converged, 2 break)


def ransac_parameters(prob=0.99, min_inliers=10, max_its=300, min_set=6, epsilon=0.5, n=0):
    """``MLPnPsolver::SetRansacParameters`` -> (mRansacMinInliers, mRansacMaxIts) (host code of the library)."""
    a, b = C.c_int32(0), C.c_int32(0)
    load_library().osg_mlpnp_ransac_parameters(float(prob), int(min_inliers), int(max_its), int(min_set), float(epsilon),
                                               int(n), C.byref(a), C.byref(b))
    return a.value, b.value


def draw_sets(n: int, h: int, rand_ints, k: int = 6) -> np.ndarray:
    """The sample sets of ``h`` iterations (ref:src/MLPnPsolver.cpp:177-202): each iteration starts from all
    ``n`` indices and draws ``k`` without replacement, the drawn slot being overwritten by the last available
    index.  ``rand_ints`` is the stream of ``RandomInt(0, available - 1)`` results, k per iteration."""
    r = np.asarray(rand_ints, np.int64).reshape(-1)
    assert len(r) >= k * h and n >= k
    out = np.empty((h, k), np.int32)
    for it in range(h):
        moved = {}  # the available list differs from the identity in at most k - 1 slots
        size = n
        for j in range(k):
            ri = int(r[k * it + j])
            assert 0 <= ri < size
            out[it, j] = moved.get(ri, ri)
            moved[ri] = moved.get(size - 1, size - 1)
            size -= 1
    return out


def unproject(cam, kp):
    """``GeometricCamera::unproject(cv::Point2f)`` of the rows of kp in float (Pinhole.cpp:97-101,
    KannalaBrandt8.cpp:180-217) -> n x 3 float32."""
    kp = np.asarray(kp, F).reshape(-1, 2)
    p = [F(cam.p[i]) for i in range(8)]
    x = (kp[:, 0] - p[2]) / p[0]
    y = (kp[:, 1] - p[3]) / p[1]
    if cam.type != _abi.CAM_KB8:
        return np.stack([x, y, np.ones_like(x)], 1).astype(F)
    out = np.empty((len(kp), 3), F)
    for i in range(len(kp)):
        scale = F(1)
        theta_d = F(np.sqrt(x[i] * x[i] + y[i] * y[i]))
        theta_d = F(min(max(F(-np.pi / 2), theta_d), F(np.pi / 2)))
        if theta_d > 1e-8:
            theta = theta_d
            for _ in range(10):
                t2 = F(theta * theta)
                t4 = F(t2 * t2)
                t6 = F(t4 * t2)
                t8 = F(t4 * t4)
                k0, k1, k2, k3 = F(p[4] * t2), F(p[5] * t4), F(p[6] * t6), F(p[7] * t8)
                fix = F(F(theta * F(1 + k0 + k1 + k2 + k3) - theta_d) / F(1 + 3 * k0 + 5 * k1 + 7 * k2 + 9 * k3))
                theta = F(theta - fix)
                if abs(fix) < 1e-6:
                    break
            scale = F(np.tan(theta) / theta_d)
        out[i] = (x[i] * scale, y[i] * scale, 1)
    return out


def bearings(cam, kp):
    """The constructor's bearing: unproject(kp.pt) divided by its z (not normalised to unit length)."""
    b = unproject(cam, kp)
    return (b / b[:, 2:3]).astype(F)


def max_errors(sigma2, th2=TH2):
    """mvMaxError: ``mvSigma2[i] * th2`` in float."""
    return (np.asarray(sigma2, F) * F(th2)).astype(F)


class MLPnPsolver:
    """``MLPnPsolver::iterate`` for one problem or a list of problems (one pair of launches)."""

    def __init__(self, ctx: Context):
        self.ctx = ctx

    def solve(self, problems):
        single = isinstance(problems, MlpnpProblem)
        probs = [problems] if single else list(problems)
        nb = len(probs)
        ps = (_abi.OsgMlpnpProblem * max(1, nb))(*[p.struct() for p in probs])
        rs = (_abi.OsgMlpnpResult * max(1, nb))()
        inl = [np.zeros(p.n, np.uint8) for p in probs]
        cnt = [np.zeros(p.n_hyp, np.int32) for p in probs]
        pose = [np.zeros((p.n_hyp, 12), np.float64) for p in probs]
        info = [np.zeros((p.n_hyp, 3), np.int32) for p in probs]
        for r, a, b, c, d in zip(rs, inl, cnt, pose, info):
            r.inlier, r.hyp_inliers, r.hyp_pose, r.hyp_info = _p(a), _p(b), _p(c), _p(d)
        self.ctx.check(self.ctx.lib.osg_mlpnp_ransac_batch(self.ctx.handle, ps, nb, rs), "MLPnPsolver")
        out = [MlpnpResult(bool(r.converged), r.hyp, r.n_iterations, r.n_inliers, r.n_best,
                           np.array(list(r.Tcw), F).reshape(4, 4), np.array(list(r.R)).reshape(3, 3),
                           np.array(list(r.t)), a, b, c, d)
               for r, a, b, c, d in zip(rs, inl, cnt, pose, info)]
        return out[0] if single else out


def problem_from_scene(rng, scene, min_inliers=10, n_hyp=300):
    """A synth.reloc_scene as the constructor and SetRansacParameters leave it, with ``n_hyp`` sample sets
    drawn as the reference draws them from a seeded stream."""
    n = len(scene["Xw"])
    sig2 = level_sigma2()[scene["octave"]] if n else np.zeros(0, F)
    if n >= 6:
        ri = np.stack([rng.integers(0, n - j, n_hyp) for j in range(6)], 1)
        samples = draw_sets(n, n_hyp, ri)
    else:
        samples = np.zeros((n_hyp, 6), np.int32)
    return MlpnpProblem(bearings(scene["cam"], scene["kp"]), scene["Xw"], scene["kp"], max_errors(sig2), samples,
                        min_inliers=min_inliers, cam=scene["cam"], truth=(scene["R"], scene["t"], scene["outlier"]))


def synth_mlpnp_problem(rng, n=200, outlier_frac=0.3, min_inliers=10, n_hyp=300, **scene_kw):
    return problem_from_scene(rng, synth.reloc_scene(rng, n, outlier_frac, **scene_kw), min_inliers, n_hyp)
