"""Host mirror of ``ORB_SLAM3::Sim3Solver`` (ref:include/Sim3Solver.h, ref:src/Sim3Solver.cc) on the C
ABI in include/osg_ba.h: every RANSAC hypothesis is evaluated on the GPU in one launch and the
reference's sequential "first good enough / last best" rule is replayed on the inlier counts.

The constructor's gather from KeyFrames and MapPoints (ref:src/Sim3Solver.cc:38-118) is the adapter's
job; here a problem is given directly as the kept matches and the sample triples in draw order.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from . import Context, _abi, load_library
from .optimizer import _p, pinhole_camera, small_rotation
from .synth import EUROC_H, EUROC_W


@dataclass
class Sim3RansacProblem:
    p1c: np.ndarray           # n x 3 float32: mvX3Dc1
    p2c: np.ndarray           # n x 3 float32: mvX3Dc2
    max_err1: np.ndarray      # float32 per match: mvnMaxError1 (9.210 sigma2 truncated to an integer)
    max_err2: np.ndarray
    samples: np.ndarray       # H x 3 int32, in draw order
    min_inliers: int = 20
    fix_scale: bool = False
    cam1: object = field(default_factory=pinhole_camera)
    cam2: object = field(default_factory=pinhole_camera)
    truth: tuple | None = None  # generator only: (R, t, s, outlier flags)

    def __post_init__(self):
        self.p1c = np.ascontiguousarray(self.p1c, np.float32).reshape(-1, 3)
        self.p2c = np.ascontiguousarray(self.p2c, np.float32).reshape(-1, 3)
        self.max_err1 = np.ascontiguousarray(self.max_err1, np.float32)
        self.max_err2 = np.ascontiguousarray(self.max_err2, np.float32)
        self.samples = np.ascontiguousarray(self.samples, np.int32).reshape(-1, 3)

    @property
    def n(self):
        return len(self.p1c)

    @property
    def n_hyp(self):
        return len(self.samples)

    def struct(self):
        st = _abi.OsgSim3RansacProblem()
        st.n = self.n
        st.p1c, st.p2c, st.max_err1, st.max_err2 = _p(self.p1c), _p(self.p2c), _p(self.max_err1), _p(self.max_err2)
        st.cam1, st.cam2 = self.cam1, self.cam2
        st.fix_scale = int(bool(self.fix_scale))
        st.min_inliers = int(self.min_inliers)
        st.n_hyp = self.n_hyp
        st.samples = _p(self.samples)
        return st


@dataclass
class Sim3RansacResult:
    converged: bool
    hyp: int                  # the returned hypothesis (-1: n < min_inliers or n == 0)
    n_iterations: int         # mnIterations
    n_inliers: int            # nInliers (0 unless converged)
    n_best: int               # mnBestInliers
    R: np.ndarray             # 3 x 3 float32
    t: np.ndarray             # 3 float32
    s: float
    T12: np.ndarray           # 4 x 4 float32
    inlier: np.ndarray        # n flags of hyp
    hyp_inliers: np.ndarray   # H counts
    hyp_sim3: np.ndarray      # H x 13 float32: R[9] t[3] s


def ransac_iterations(prob: float, min_inliers: int, n: int, max_its: int) -> int:
    """``Sim3Solver::SetRansacParameters``' mRansacMaxIts (host code of the library)."""
    return int(load_library().osg_sim3_ransac_iterations(float(prob), int(min_inliers), int(n), int(max_its)))


def draw_samples(n: int, h: int, rand_ints) -> np.ndarray:
    """The sample triples of ``h`` iterations (ref:src/Sim3Solver.cc:169-183): each iteration starts from
    all ``n`` indices and draws three without replacement, the drawn slot being overwritten by the last
    available index.  ``rand_ints`` is the stream of ``RandomInt(0, available - 1)`` results, 3 per
    iteration in call order."""
    r = np.asarray(rand_ints, np.int64).reshape(-1)
    assert len(r) >= 3 * h and n >= 3
    out = np.empty((h, 3), np.int32)
    for it in range(h):
        # the available list differs from the identity in at most two slots
        moved = {}
        size = n
        for j in range(3):
            ri = int(r[3 * it + j])
            assert 0 <= ri < size
            out[it, j] = moved.get(ri, ri)
            moved[ri] = moved.get(size - 1, size - 1)
            size -= 1
    return out


class Sim3Solver:
    """``Sim3Solver::find`` for one problem or a list of problems (one pair of launches)."""

    def __init__(self, ctx: Context):
        self.ctx = ctx

    def solve(self, problems):
        single = isinstance(problems, Sim3RansacProblem)
        probs = [problems] if single else list(problems)
        nb = len(probs)
        ps = (_abi.OsgSim3RansacProblem * max(1, nb))(*[p.struct() for p in probs])
        rs = (_abi.OsgSim3RansacResult * max(1, nb))()
        inl = [np.zeros(p.n, np.uint8) for p in probs]
        cnt = [np.zeros(p.n_hyp, np.int32) for p in probs]
        s3 = [np.zeros((p.n_hyp, 13), np.float32) for p in probs]
        for r, a, b, c in zip(rs, inl, cnt, s3):
            r.inlier, r.hyp_inliers, r.hyp_sim3 = _p(a), _p(b), _p(c)
        self.ctx.check(self.ctx.lib.osg_sim3_ransac_batch(self.ctx.handle, ps, nb, rs), "Sim3Solver")
        out = [Sim3RansacResult(bool(r.converged), r.hyp, r.n_iterations, r.n_inliers, r.n_best,
                                np.array(list(r.R), np.float32).reshape(3, 3), np.array(list(r.t), np.float32),
                                float(r.s), np.array(list(r.T12), np.float32).reshape(4, 4), a, b, c)
               for r, a, b, c in zip(rs, inl, cnt, s3)]
        return out[0] if single else out


def level_sigma2(n_levels=8, factor=1.2):
    """mvLevelSigma2 as ORBextractor fills it (float)."""
    s = np.ones(n_levels, np.float32)
    for i in range(1, n_levels):
        s[i] = np.float32(s[i - 1] * np.float32(factor))
    return (s * s).astype(np.float32)


def max_errors(sigma2):
    """mvnMaxError: ``9.210 * sigmaSquare`` (double) stored in a ``size_t`` (ref:include/Sim3Solver.h:72-73)."""
    return np.floor(9.210 * np.asarray(sigma2, np.float32).astype(np.float64)).astype(np.float32)


def synth_sim3_ransac_problem(rng, n=100, outlier_frac=0.1, fix_scale=False, cam1=None, cam2=None, min_inliers=20,
                              n_hyp=300, n_levels=8, noise_m=0.004):
    """One loop candidate as LoopClosing hands it to Sim3Solver: points 2 .. 8 m in front of KeyFrame 2, the
    true S12 a few degrees / decimetres / per cent off identity (scale 1 when ``fix_scale``), each KeyFrame's
    own MapPoint ``noise_m`` off the common point, octaves drawn as the pyramid populates them, and
    ``outlier_frac`` of the matches wrong 3-D associations: their p2c is another, unrelated point.  The
    sample triples are drawn as the reference draws them from a seeded stream."""
    cam1 = cam1 or pinhole_camera()
    cam2 = cam2 or pinhole_camera()
    n = int(n)

    def cloud(m):
        if cam2.type == _abi.CAM_KB8:
            th = rng.uniform(0.05, 0.9, m)
            ps = rng.uniform(-np.pi, np.pi, m)
            d = rng.uniform(2.0, 8.0, m)
            return np.stack([d * np.sin(th) * np.cos(ps), d * np.sin(th) * np.sin(ps), d * np.cos(th)], 1)
        u = rng.uniform(60, EUROC_W - 60, m)
        v = rng.uniform(60, EUROC_H - 60, m)
        z = rng.uniform(2.0, 8.0, m)
        return np.stack([(u - float(cam2.p[2])) / float(cam2.p[0]) * z, (v - float(cam2.p[3])) / float(cam2.p[1]) * z, z], 1)

    P2 = cloud(n)
    R = small_rotation(rng, 3.0)
    t = rng.normal(0, 0.15, 3)
    s = 1.0 if fix_scale else float(rng.uniform(0.9, 1.1))
    P1 = s * P2 @ R.T + t
    out = rng.random(n) < outlier_frac
    wrong = cloud(n)
    p1c = (P1 + rng.normal(0, noise_m, (n, 3))).astype(np.float32)
    p2c = (np.where(out[:, None], wrong, P2) + rng.normal(0, noise_m, (n, 3))).astype(np.float32)
    lev_p = np.array([1.2 ** -i for i in range(n_levels)])
    lev_p /= lev_p.sum()
    sig2 = level_sigma2(n_levels)
    m1 = max_errors(sig2[rng.choice(n_levels, n, p=lev_p)])
    m2 = max_errors(sig2[rng.choice(n_levels, n, p=lev_p)])
    if n >= 3:
        ri = np.stack([rng.integers(0, n - j, n_hyp) for j in range(3)], 1)
        samples = draw_samples(n, n_hyp, ri)
    else:
        samples = np.zeros((n_hyp, 3), np.int32)
    return Sim3RansacProblem(p1c, p2c, m1, m2, samples, min_inliers=min_inliers, fix_scale=bool(fix_scale),
                             cam1=cam1, cam2=cam2, truth=(R, t, s, out))
