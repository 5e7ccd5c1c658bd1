"""Host mirror of ``ORB_SLAM3::TwoViewReconstruction`` (ref:include/TwoViewReconstruction.h,
ref:src/TwoViewReconstruction.cc) on the C ABI in include/osg.h: the monocular initialiser's H / F RANSAC,
the choice between the two models, the motion hypotheses and CheckRT run on the GPU; the sets of eight
matches are drawn on the host and handed over in draw order.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from . import Context, _abi
from .optimizer import _p


def draw_sets(n: int, n_hyp: int, random_ints) -> np.ndarray:
    """``mvSets`` (ref:src/TwoViewReconstruction.cc:94-115): each iteration starts from all ``n`` indices and
    draws eight without replacement, the drawn slot being overwritten by the last available index.
    ``random_ints`` is the stream of ``RandomInt(0, available - 1)`` results, 8 per iteration in call order."""
    r = np.asarray(random_ints, np.int64).reshape(-1)
    assert len(r) >= 8 * n_hyp and n >= 8
    out = np.empty((n_hyp, 8), np.int32)
    for it in range(n_hyp):
        moved = {}  # the available list differs from the identity in at most seven slots
        size = n
        for j in range(8):
            ri = int(r[8 * it + j])
            assert 0 <= ri < size
            out[it, j] = moved.get(ri, ri)
            moved[ri] = moved.get(size - 1, size - 1)
            size -= 1
    return out


def seeded_sets(n: int, n_hyp: int, seed: int = 0) -> np.ndarray:
    """The sets ``reconstruct`` draws when the caller passes none: ``draw_sets`` on a seeded numpy stream (the
    adapter draws with DUtils::Random as the reference does)."""
    if n < 8:
        return np.zeros((n_hyp, 8), np.int32)
    rng = np.random.default_rng(seed)
    return draw_sets(n, n_hyp, np.stack([rng.integers(0, n - j, n_hyp) for j in range(8)], 1))


@dataclass
class TwoViewProblem:
    keys1: np.ndarray         # n_keys1 x 2 float32: mvKeysUn of the reference frame
    keys2: np.ndarray         # n_keys2 x 2 float32: of the current frame
    matches12: np.ndarray     # n_keys1 int32: index into keys2 or -1 (mvIniMatches)
    sets: np.ndarray          # n_hyp x 8 int32 into the kept matches, in draw order
    K: tuple                  # fx fy cx cy
    sigma: float = 1.0
    min_parallax: float = 1.0
    min_triangulated: int = 50
    truth: tuple | None = None  # generator only: (R21, t21, outlier flags per kept match)

    def __post_init__(self):
        self.keys1 = np.ascontiguousarray(self.keys1, np.float32).reshape(-1, 2)
        self.keys2 = np.ascontiguousarray(self.keys2, np.float32).reshape(-1, 2)
        self.matches12 = np.ascontiguousarray(self.matches12, np.int32).reshape(-1)
        assert len(self.matches12) == len(self.keys1)
        self.sets = np.ascontiguousarray(self.sets, np.int32).reshape(-1, 8)
        self.idx1 = np.ascontiguousarray(np.flatnonzero(self.matches12 >= 0), np.int32)
        self.idx2 = np.ascontiguousarray(self.matches12[self.idx1], np.int32)
        self.kp1 = np.ascontiguousarray(self.keys1[self.idx1])
        self.kp2 = np.ascontiguousarray(self.keys2[self.idx2])

    @property
    def n(self):
        return len(self.idx1)

    @property
    def n_hyp(self):
        return len(self.sets)

    def struct(self):
        st = _abi.OsgTwoViewProblem()
        for i in range(4):
            st.K[i] = self.K[i]
        st.sigma, st.n_hyp, st.n = float(self.sigma), self.n_hyp, self.n
        st.kp1, st.kp2 = _p(self.kp1), _p(self.kp2)
        st.n_keys1, st.n_keys2 = len(self.keys1), len(self.keys2)
        st.keys1, st.keys2, st.idx1, st.idx2, st.sets = _p(self.keys1), _p(self.keys2), _p(self.idx1), _p(self.idx2), _p(self.sets)
        st.min_parallax, st.min_triangulated = float(self.min_parallax), int(self.min_triangulated)
        return st


@dataclass
class TwoViewResult:
    ok: bool
    model: int                # 0 H, 1 F, -1 none
    score_h: float
    score_f: float
    hyp_h: int
    hyp_f: int
    H21: np.ndarray
    F21: np.ndarray
    R: np.ndarray             # T21
    t: np.ndarray
    cand: int                 # the motion hypothesis the acceptance rule looked at
    n_inliers: int
    n_good: np.ndarray        # 8
    parallax: np.ndarray      # 8
    cand_Rt: np.ndarray       # 8 x 12
    p3d: np.ndarray           # n_keys1 x 3
    triangulated: np.ndarray  # n_keys1 bool
    inlier_h: np.ndarray      # n bool
    inlier_f: np.ndarray
    hyp_score_h: np.ndarray   # n_hyp
    hyp_score_f: np.ndarray
    hyp_models: np.ndarray    # n_hyp x 2 x 3 x 3


class TwoViewReconstruction:
    """``TwoViewReconstruction(K, sigma, iterations)``; ``reconstruct`` is ``Reconstruct`` for one frame pair,
    ``reconstruct_batch`` for many in the same launches."""

    def __init__(self, ctx: Context, K, sigma: float = 1.0, iterations: int = 200):
        self.ctx = ctx
        K = np.asarray(K, np.float64)
        self.K = (K[0, 0], K[1, 1], K[0, 2], K[1, 2]) if K.shape == (3, 3) else tuple(float(v) for v in K)
        self.sigma = float(sigma)
        self.iterations = int(iterations)

    def problem(self, keys1, keys2, matches12, sets=None) -> TwoViewProblem:
        if sets is None:
            n = int(np.count_nonzero(np.asarray(matches12) >= 0))
            sets = seeded_sets(n, self.iterations)
        return TwoViewProblem(keys1, keys2, matches12, sets, K=self.K, sigma=self.sigma)

    def reconstruct(self, keys1, keys2, matches12, sets=None) -> TwoViewResult:
        return self.solve(self.problem(keys1, keys2, matches12, sets))

    def reconstruct_batch(self, pairs):
        """``pairs``: (keys1, keys2, matches12[, sets]) tuples -> a list of results."""
        return self.solve([self.problem(*p) for p in pairs])

    def solve(self, problems):
        single = isinstance(problems, TwoViewProblem)
        probs = [problems] if single else list(problems)
        nb = len(probs)
        ps = (_abi.OsgTwoViewProblem * max(1, nb))(*[p.struct() for p in probs])
        rs = (_abi.OsgTwoViewResult * max(1, nb))()
        bufs = []
        for p, r in zip(probs, rs):
            b = dict(p3d=np.zeros((len(p.keys1), 3), np.float32), tri=np.zeros(len(p.keys1), np.uint8),
                     ih=np.zeros(p.n, np.uint8), jf=np.zeros(p.n, np.uint8), sh=np.zeros(p.n_hyp, np.float32),
                     sf=np.zeros(p.n_hyp, np.float32), md=np.zeros((p.n_hyp, 2, 3, 3), np.float32))
            r.p3d, r.triangulated, r.inlier_h, r.inlier_f = _p(b["p3d"]), _p(b["tri"]), _p(b["ih"]), _p(b["jf"])
            r.hyp_score_h, r.hyp_score_f, r.hyp_models = _p(b["sh"]), _p(b["sf"]), _p(b["md"])
            bufs.append(b)
        self.ctx.check(self.ctx.lib.osg_two_view_reconstruct_batch(self.ctx.handle, ps, nb, rs), "TwoViewReconstruction")
        f = lambda a, *s: np.array(list(a), np.float32).reshape(*s)  # noqa: E731
        out = [TwoViewResult(bool(r.ok), r.model, float(r.score_h), float(r.score_f), r.hyp_h, r.hyp_f, f(r.H21, 3, 3),
                             f(r.F21, 3, 3), f(r.R, 3, 3), f(r.t, 3), r.cand, r.n_inliers, np.array(list(r.n_good), np.int32),
                             f(r.parallax, 8), f(r.cand_Rt, 8, 12), b["p3d"], b["tri"].astype(bool), b["ih"].astype(bool),
                             b["jf"].astype(bool), b["sh"], b["sf"], b["md"])
               for r, b in zip(rs, bufs)]
        return out[0] if single else out
