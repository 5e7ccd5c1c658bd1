"""The OptimizeEssentialGraph4DoF fixtures shared by tests/test_essgraph4dof.py, tests/test_essgraph4dof_gpu.py and
tools/essgraph4dof_margins.py: seeded graphs of ``synth_essential_graph_4dof`` and a few built by hand, in named
groups that mirror tests/essgraph_fixtures.py at the same sizes.  A fixture is held to the tolerances of its own
group (profiles/essgraph4dof_margins.json).

  tiny        2 vertices and 1 edge with the fixed vertex as vertex(0) and as vertex(1) (6 residual rows against
              4 degrees of freedom: chi2_final is not rounding alone); a triangle; an edge between two fixed
              vertices beside a free chain.
  tile_edges  3, 4, 5, 8 and 9 free vertices (a 32 x 32 tile is four padded vertices), the fixed vertex first;
              8 free vertices with the fixed one in the middle and last.
  band_loop   12 and 40 KeyFrames, 3 corrected ones; both again with an earlier loop in the middle of the map.
  duplicates  the same pair listed twice, and once in each direction.
  larger      200 KeyFrames (pyref takes its sparse solve).

CONSISTENT names the graphs whose optimum is known (``consistent=True``); the failed-solve graph is the one whose
only free vertex has no edge.  No fixture exceeds 200 vertices; the kernels switch no path by size."""
from dataclasses import dataclass

import numpy as np

from orb_slam3_comments_ghr_amd import optimizer as O

N_REPLICAS = 16


@dataclass(frozen=True)
class Fixture:
    kind: str                 # "synth" | "pair" | "triangle" | "fixed_pair" | "dup"
    group: str
    seed: int
    n_kf: int = 0
    n_loop: int = 3
    extra_loops: int = 0
    fixed_at: int = 0         # synth: the fixed vertex
    arg: int = 0              # pair: which end is fixed; dup: 0 listed twice, 1 once in each direction


FIXTURES = {
    "pair_fixed_v0": Fixture("pair", "tiny", 411, arg=0),
    "pair_fixed_v1": Fixture("pair", "tiny", 412, arg=1),
    "triangle": Fixture("triangle", "tiny", 413),
    "fixed_pair_chain": Fixture("fixed_pair", "tiny", 414),
    "free3": Fixture("synth", "tile_edges", 423, n_kf=4, n_loop=2),
    "free4": Fixture("synth", "tile_edges", 424, n_kf=5),
    "free5": Fixture("synth", "tile_edges", 425, n_kf=6),
    "free8": Fixture("synth", "tile_edges", 428, n_kf=9),
    "free9": Fixture("synth", "tile_edges", 429, n_kf=10),
    "free8_fixed_mid": Fixture("synth", "tile_edges", 430, n_kf=9, fixed_at=4),
    "free8_fixed_last": Fixture("synth", "tile_edges", 431, n_kf=9, fixed_at=8),
    "kf12": Fixture("synth", "band_loop", 4112, n_kf=12),
    "kf12x": Fixture("synth", "band_loop", 4113, n_kf=12, n_loop=2, extra_loops=1),
    "kf40": Fixture("synth", "band_loop", 4140, n_kf=40),
    "kf40x": Fixture("synth", "band_loop", 4142, n_kf=40, extra_loops=1),
    "dup_twice": Fixture("dup", "duplicates", 451, n_kf=9, arg=0),
    "dup_reversed": Fixture("dup", "duplicates", 452, n_kf=9, arg=1),
    "kf200": Fixture("synth", "larger", 4200, n_kf=200),
}
GROUPS = sorted({f.group for f in FIXTURES.values()})
# (n_kf, seed) of the graphs with a known optimum
CONSISTENT = {"c24": (24, 4324), "c200": (200, 4326)}
UNIT_INFO = (1.0, 1.0, 1.0, 1.0, 1.0, 1.0)


def moved(rng, rows, deg, metres):
    """every vertex row moved as the vertex's own update moves it: a yaw about world z and a translation of the
    body, the camera re-derived (double)"""
    out = []
    for r in np.asarray(rows, float).reshape(-1, 36):
        Rwb, twb, Rcb, tcb = r[0:9].reshape(3, 3), r[9:12], r[24:33].reshape(3, 3), r[33:36]
        Rwb = O.rodrigues([0.0, 0.0, np.deg2rad(deg) * rng.normal()]) @ Rwb
        twb = twb + rng.normal(0, metres, 3)
        out.append(O.imu_cam_pose_row(Rwb, twb, Rcb @ Rwb.T, Rcb @ (-(Rwb.T @ twb)) + tcb, Rcb, tcb))
    return np.array(out)


def noisy_meas(rng, meas, deg, metres):
    """every (dRij, dtij) moved by a rotation about a random axis and a translation"""
    out = []
    for m in np.asarray(meas, float).reshape(-1, 12):
        w = rng.normal(size=3)
        w *= np.deg2rad(deg) * rng.normal() / np.linalg.norm(w)
        out.append(np.concatenate([(O.rodrigues(w) @ m[:9].reshape(3, 3)).ravel(), m[9:] + rng.normal(0, metres, 3)]))
    return np.array(out)


def relative(rows, i, j):
    """Tcw_i Tcw_j^-1 of two vertex rows as (dRij, dtij)"""
    Ri, ti, Rj, tj = rows[i, 12:21].reshape(3, 3), rows[i, 21:24], rows[j, 12:21].reshape(3, 3), rows[j, 21:24]
    dR = Ri @ Rj.T
    return np.concatenate([dR.ravel(), ti - dR @ tj])


def by_hand(rng, n, edges, fixed):
    """n vertices 1 deg of yaw / 2 cm off a ground truth, measurements 0.2 deg (any axis) / 5 mm off it"""
    G = O.synth_essential_graph_4dof(rng, max(n, 4), n_loop=0, consistent=True).truth[:n]
    est = moved(rng, G, 1.0, 0.02)
    meas = noisy_meas(rng, np.array([relative(G, i, j) for i, j in edges]), 0.2, 0.005)
    fx = np.zeros(n, np.uint8)
    fx[list(fixed)] = 1
    return O.EssentialGraph4DoFProblem(est, fx, np.array([e[0] for e in edges], np.int32),
                                       np.array([e[1] for e in edges], np.int32), meas)


def build(name, max_iterations=0):
    f = FIXTURES[name]
    rng = np.random.default_rng(f.seed)
    if f.kind == "synth":
        P = O.synth_essential_graph_4dof(rng, f.n_kf, n_loop=min(f.n_loop, f.n_kf - 2), extra_loops=f.extra_loops)
        P.fixed[:] = 0
        P.fixed[f.fixed_at] = 1
    elif f.kind == "pair":
        P = by_hand(rng, 2, [(0, 1)], [f.arg])
    elif f.kind == "triangle":
        P = by_hand(rng, 3, [(1, 0), (2, 1), (2, 0)], [0])
    elif f.kind == "fixed_pair":
        P = by_hand(rng, 5, [(1, 0), (2, 1), (3, 2), (4, 3), (4, 2)], [0, 1])
    elif f.kind == "dup":
        P = O.synth_essential_graph_4dof(rng, f.n_kf, n_loop=0)
        P.pose = moved(rng, P.pose, 1.0, 0.02)
        i, j = 6, 3
        k = int(np.nonzero((P.e_v0 == i) & (P.e_v1 == j))[0][0])
        m = noisy_meas(rng, P.e_meas[k], 0.2, 0.005)[0]   # the second listing measures something else
        if f.arg:
            dR = m[:9].reshape(3, 3)
            P.e_v0, P.e_v1 = np.append(P.e_v0, j).astype(np.int32), np.append(P.e_v1, i).astype(np.int32)
            P.e_meas = np.vstack([P.e_meas, np.concatenate([dR.T.ravel(), -dR.T @ m[9:]])])
        else:
            P.e_v0, P.e_v1 = np.append(P.e_v0, i).astype(np.int32), np.append(P.e_v1, j).astype(np.int32)
            P.e_meas = np.vstack([P.e_meas, m])
    else:
        raise KeyError(f.kind)
    P.max_iterations = max_iterations
    return P


def build_consistent(n_kf, seed):
    return O.synth_essential_graph_4dof(np.random.default_rng(seed), n_kf, consistent=True)


def build_failed_solve():
    """two fixed vertices joined by an edge and one free vertex without an edge, lambda_init = 0: H = 0, g2o's
    lambda stays 0 and every solve meets the pivot 0"""
    return by_hand(np.random.default_rng(461), 3, [(1, 0)], [0, 1])


def replicas(name, P):
    """The 16 replicas of a fixture for the nudge study (their own seeded stream): (problem, Variant) pairs.
    Every replica's inputs move by +-1 ulp; on top of that, in turn, sin / cos / acos move one ulp up and down,
    the sums are taken in reverse, NormalizeRotation is the polar factor, the solve goes through another
    factorisation, and the last replicas combine them."""
    from tests import pyref_essgraph4dof as R
    rng = np.random.default_rng(FIXTURES[name].seed + 77777)
    V = R.Variant
    variants = [V(), V(), V(), V(), V(trig=1), V(trig=-1), V(reverse_sums=True), V(polar=True), V(other_solver=True),
                V(trig=1, reverse_sums=True), V(trig=-1, polar=True), V(polar=True, other_solver=True),
                V(reverse_sums=True, other_solver=True), V(trig=1, polar=True, reverse_sums=True, other_solver=True),
                V(trig=-1, polar=True, reverse_sums=True, other_solver=True), V(trig=1, other_solver=True)]
    assert len(variants) == N_REPLICAS
    return [(R.nudged(P, rng), v) for v in variants]
