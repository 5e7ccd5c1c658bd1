"""Hand-built boundary fixtures for the five operators of match.hip ("Matcher decisions"), in the
house style of tests/matcher_boundary_fixtures.py: no RNG, at most 64 keypoints and 64 queries a side, bits(k)
descriptors, every float a case rests on asserted in float32 by its builder.

    mps    SearchByProjection(Frame, MapPoints)   args (F, Q, slot_mp, slot_taken, nn, th, far, thfar)
    last   SearchByProjection(Frame, LastFrame)   args (F, L, slot_mp, slot_taken, th)       modes (mono, ori)
    kf     SearchByProjection(Frame, KeyFrame)    args (F, K, slot_mp, th, orb_dist)         modes ori
    bow    SearchByBoW(KeyFrame, Frame)           args (KF, F, nn)                           modes ori
    bowkk  SearchByBoW(KeyFrame, KeyFrame)        args (K1, K2, nn)                          modes ori

One- and two-camera forms are separate cases (the camera count is the frame's).  tests/test_matcher_boundaries.py
proves each case discriminating on the CPU; tests/test_match_boundaries_gpu.py runs k_match's paths on them."""
import numpy as np

from orb_slam3_comments_ghr_amd import frames as fr
from tests import matcher_boundary_fixtures as mb
from tests import oracle_calls as oc
from tests import pyref_match as pr
from tests.matcher_boundary_fixtures import Case, bits, cell_of, down, up

f32 = np.float32
KINDS = ("mps", "last", "kf", "bow", "bowkk")
LAST_MODES = ((False, True), (False, False), (True, True), (True, False))  # (bMono, checkOri)
ORI_MODES = (True, False)
NN = 0.7            # 50 * 0.7f is 35.0 in float and 34.9999994 in double
NN_UP = 0.6         # 20 * 0.6f is 12.0 in float (a tie to even) and 12.0000005 in double
RIDER_XY = (700.0, 440.0)  # kept free by every two-camera mps case (redo_rider)
assert float(f32(f32(NN) * f32(50))) == 35.0 > float(f32(NN)) * 50.0
assert float(f32(f32(NN_UP) * f32(20))) == 12.0 < float(f32(NN_UP)) * 20.0


# ------------------------------------------------------------------------------------ containers

def _descs(rows):
    return np.stack(rows) if len(rows) else np.zeros((0, 32), np.uint8)


def gframe(left, right=None, u_right=None, l2r=None, r2l=None):
    """left / right: (x, y, octave, descriptor[, angle]) per keypoint; right makes a two-camera frame."""
    kps = list(left) + list(right or [])
    two = right is not None
    nl, nr = len(left), len(right or [])
    return fr.FrameSoA(desc=np.stack([k[3] for k in kps]), kp_x=[k[0] for k in kps], kp_y=[k[1] for k in kps],
                       kp_angle=[k[4] if len(k) > 4 else 0.0 for k in kps], kp_octave=[k[2] for k in kps],
                       u_right=u_right, nleft=nl if two else -1,
                       left_to_right=(np.full(nl, -1, np.int32) if l2r is None else l2r) if two else None,
                       right_to_left=(np.full(nr, -1, np.int32) if r2l is None else r2l) if two else None)


def mpq(rows, two=False):
    """rows: dicts x, y, lvl, d [, cos, xr, depth, obs, view, usable; right camera: rx, ry, rlvl, rcos, rview]."""
    n = len(rows)
    g = lambda k, dflt: [r.get(k, dflt) for r in rows]  # noqa: E731
    return fr.MPQueries(mp_id=1000 + np.arange(n), desc=_descs([r["d"] for r in rows]), usable=g("usable", 1),
                        has_obs=g("obs", 1), in_view=g("view", 1), proj_x=g("x", 0.0), proj_y=g("y", 0.0),
                        proj_xr=[r.get("rx", r.get("xr", -1.0)) for r in rows], view_cos=g("cos", 0.5),
                        pred_level=g("lvl", 0), track_depth=g("depth", 1.0),
                        in_view_r=g("rview", 0) if two else None, proj_yr=g("ry", 0.0) if two else None,
                        view_cos_r=g("rcos", 0.5) if two else None, pred_level_r=g("rlvl", 0) if two else None)


def lastq(rows, tlc_z=0.0, two=False):
    """rows: dicts x, y, o, d [, invz, obs, ang, valid; right camera: rx, ry]."""
    n = len(rows)
    g = lambda k, dflt: [r.get(k, dflt) for r in rows]  # noqa: E731
    return fr.LastQueries(mp_id=2000 + np.arange(n), desc=_descs([r["d"] for r in rows]), valid=g("valid", 1),
                          has_obs=g("obs", 1), u=g("x", 0.0), v=g("y", 0.0), invz=g("invz", 0.1), octave=g("o", 0),
                          angle=g("ang", 0.0), tlc_z=float(tlc_z), u_r=g("rx", -500.0) if two else None,
                          v_r=g("ry", -500.0) if two else None)


def kfq(rows):
    """rows: dicts x, y, lvl, d [, ang, valid]."""
    n = len(rows)
    g = lambda k, dflt: [r.get(k, dflt) for r in rows]  # noqa: E731
    return fr.KFQueries(mp_id=3000 + np.arange(n), desc=_descs([r["d"] for r in rows]), valid=g("valid", 1),
                        u=g("x", 0.0), v=g("y", 0.0), pred_level=g("lvl", 0), angle=g("ang", 0.0))


def bside(feats, nleft=-1, id_base=4000):
    """feats: (descriptor, node[, angle, good, mp_id]) per feature; a node's list is in feature order."""
    n = len(feats)
    nodes = [f[1] for f in feats]
    ids = sorted(set(nodes))
    feat = [i for nd in ids for i in range(n) if nodes[i] == nd]
    start = np.cumsum([0] + [nodes.count(nd) for nd in ids])
    return fr.BowSide(desc=_descs([f[0] for f in feats]), angle=[f[2] if len(f) > 2 else 0.0 for f in feats],
                      mp_id=[f[4] if len(f) > 4 else id_base + i for i, f in enumerate(feats)],
                      mp_good=[f[3] if len(f) > 3 else 1 for f in feats], node_id=ids, node_start=start, feat=feat,
                      nleft=nleft)


def free(F):
    return np.full(F.n, -1, np.int32), np.zeros(F.n, np.uint8)


def without_queries(case):
    """The case's frame (and slot state) with an empty query side: the empty problem of a batch."""
    a = case.args
    empty = {"mps": lambda: mpq([], two_cam(case)), "last": lambda: lastq([], a[1].tlc_z, two_cam(case)),
             "kf": lambda: kfq([]), "bow": lambda: bside([]), "bowkk": lambda: bside([])}[case.kind]()
    return Case(case.name + "-empty", case.kind, (a[0], empty) + a[2:], ())


def size(case):
    a = case.args
    second = a[1].n if hasattr(a[1], "n") else len(a[1].mp_id)
    return max(a[0].n, second)


# ------------------------------------------------------------------------------------ running a case

def modes(case):
    return {"mps": (None,), "last": LAST_MODES}.get(case.kind, ORI_MODES)


def run_oracle(oracle, case, mode):
    a = case.args
    if case.kind == "mps":
        return oc.mps(oracle, a[0], a[1], a[4], a[5], a[6], a[7], a[2], a[3])
    if case.kind == "last":
        return oc.last(oracle, a[0], a[1], a[4], mode[0], mode[1], a[2], a[3])
    if case.kind == "kf":
        return oc.kf(oracle, a[0], a[1], a[3], a[4], mode, a[2])
    if case.kind == "bow":
        return oc.bow_kf_f(oracle, a[0], a[1], a[2], mode)
    return oc.bow_kf_kf(oracle, a[0], a[1], a[2], mode)


def run_pyref(case, mode, flip=None):
    a = case.args
    if case.kind == "mps":
        return pr.search_mps(a[0], a[1], a[4], a[5], a[6], a[7], a[2], a[3], flip=flip)
    if case.kind == "last":
        return pr.search_last(a[0], a[1], a[4], mode[0], mode[1], a[2], a[3], flip=flip)
    if case.kind == "kf":
        return pr.search_kf(a[0], a[1], a[3], a[4], mode, a[2], flip=flip)
    if case.kind == "bow":
        return pr.search_bow_kf_f(a[0], a[1], a[2], mode, flip=flip)
    return pr.search_bow_kf_kf(a[0], a[1], a[2], mode, flip=flip)


# ------------------------------------------------------------------------------------ the area walk

def _area_worlds():
    """The worlds of matcher_boundary_fixtures._area_worlds for a window of r = 3 at level 0 (mps: 4.0 * th with
    th = 0.75; last / kf: th = 3), as (name, keypoints, [(x, y, level)] per query, flips).  The order world
    has its two keypoints on different octaves: at one octave the mps ratio test would reject the pair in
    either order."""
    out = []
    x_in = down(103.0)
    assert f32(f32(4.0) * f32(0.75)) == f32(3.0)
    assert f32(f32(103.0) - f32(100.0)) == f32(3.0) and abs(f32(x_in - f32(100.0))) < f32(3.0)
    out.append(("window", [(103.0, 100.0, 0, bits(1)), (x_in, 100.0, 0, bits(5)), (100.0, 103.0, 0, bits(2))],
                [(100.0, 100.0, 0)], ("area.window",)))
    kps = [(108.0, 94.0, 7, bits(10)), (95.0, 106.0, 6, bits(10))]
    F = gframe(kps)
    (c0, r0), (c1, r1) = cell_of(F, 108.0, 94.0), cell_of(F, 95.0, 106.0)
    assert c1 < c0 and r1 > r0 and f32(3.0) * F.scale[7] > 10
    out.append(("order", kps, [(100.0, 100.0, 7)], ("area.order",)))
    kps = [(1.0, 100.0, 0, bits(5)), (745.0, 100.0, 0, bits(5)), (100.0, 1.0, 0, bits(5)), (100.0, 474.0, 0, bits(5))]
    F = gframe(kps)
    assert cell_of(F, 745.0, 100.0)[0] == 63 and cell_of(F, 100.0, 474.0)[1] == 47
    assert (f32(747.0) + f32(3.0)) * F.inv_w > 63 and (f32(476.0) + f32(3.0)) * F.inv_h > 47
    out.append(("clamp", kps, [(2.0, 100.0, 0), (747.0, 100.0, 0), (100.0, 2.0, 0), (100.0, 476.0, 0),
                               (852.0, 100.0, 0), (-100.0, 100.0, 0), (100.0, 700.0, 0), (100.0, -100.0, 0)],
                ("area.clamp",)))
    return out


def _area_cases():
    out = []
    for name, kps, qs, flips in _area_worlds():
        F = gframe(kps)
        out.append(Case("area_" + name, "mps", (F, mpq([dict(x=x, y=y, lvl=l, d=bits(0)) for x, y, l in qs]), *free(F),
                                                NN, 0.75, False, 0.0), flips))
        out.append(Case("area_" + name, "last", (F, lastq([dict(x=x, y=y, o=l, d=bits(0)) for x, y, l in qs]), *free(F),
                                                 3.0), flips))
        out.append(Case("area_" + name, "kf", (F, kfq([dict(x=x, y=y, lvl=l, d=bits(0)) for x, y, l in qs]),
                                               free(F)[0], 3.0, 100), flips))
    return out + [_right_window_case()]


def _right_window_case():
    """area.window in mGridRight: the right pass takes no th factor, so r = 4 at level 0."""
    x_in = down(104.0)
    assert f32(f32(104.0) - f32(100.0)) == f32(4.0) and abs(f32(x_in - f32(100.0))) < f32(4.0)
    return _mps2("area_window_right", [(600.0, 400.0, 0, bits(0))],
                 [(104.0, 100.0, 0, bits(1)), (x_in, 100.0, 0, bits(5)), (100.0, 104.0, 0, bits(2))], [-1], [-1] * 3,
                 [dict(view=0, rview=1, rx=100.0, ry=100.0, rlvl=0, d=bits(0))], ("area.window",))


# ------------------------------------------------------------------------------------ mps

def _mps_one_cam():
    out = []
    # mps.far: depth exactly thFar stays, one float above it goes.  mps.bad: a bad MapPoint is not searched.
    F = gframe([(100.0, 100.0, 0, bits(5)), (200.0, 100.0, 0, bits(5)), (300.0, 100.0, 0, bits(5))])
    Q = mpq([dict(x=100.0, y=100.0, d=bits(0), depth=20.0), dict(x=200.0, y=100.0, d=bits(0), depth=up(20.0)),
             dict(x=300.0, y=100.0, d=bits(0), usable=0)])
    out.append(Case("gates", "mps", (F, Q, *free(F), NN, 1.0, True, 20.0), ("mps.far", "mps.bad")))
    # mps.radius: float32(0.998) is above the double 0.998 (radius 2.5) and not above the float one (4.0); the
    # keypoint is 3 px away.  One float lower the radius is 4.0 either way.
    c = f32(0.998)
    assert float(c) > 0.998 and not c > f32(0.998) and not float(down(c)) > 0.998
    F = gframe([(103.0, 100.0, 0, bits(5)), (203.0, 100.0, 0, bits(5))])
    Q = mpq([dict(x=100.0, y=100.0, d=bits(0), cos=c), dict(x=200.0, y=100.0, d=bits(0), cos=down(c))])
    out.append(Case("radius", "mps", (F, Q, *free(F), NN, 1.0, False, 0.0), ("mps.radius",)))
    # mps.level: candidates at pred - 2, pred - 1, pred, pred + 1, the outer two closer
    F = gframe([(200.0, 200.0, 0, bits(1)), (201.0, 200.0, 1, bits(8)), (200.0, 201.0, 2, bits(9)),
                (201.0, 201.0, 3, bits(2))])
    Q = mpq([dict(x=200.0, y=200.0, lvl=2, d=bits(0))])
    out.append(Case("level", "mps", (F, Q, *free(F), NN, 1.0, False, 0.0), ("mps.level", "mps.level:narrow")))
    # mps.taken: keypoint 0 holds a MapPoint with observations (blocked: query 0 falls back to keypoint 1),
    # keypoint 2 one without (query 1 overwrites it).  Keypoints 4, 5: query 2 (no observations) takes 4,
    # query 3 takes it again, query 4 finds it blocked by query 3 and takes 5.
    F = gframe([(100.0, 100.0, 0, bits(1)), (101.0, 100.0, 0, bits(20)), (200.0, 100.0, 0, bits(1)),
                (201.0, 100.0, 0, bits(20)), (300.0, 100.0, 0, bits(1)), (301.0, 100.0, 0, bits(20))])
    Q = mpq([dict(x=100.0, y=100.0, d=bits(0)), dict(x=200.0, y=100.0, d=bits(0)),
             dict(x=300.0, y=100.0, d=bits(0), obs=0), dict(x=300.0, y=100.0, d=bits(0)),
             dict(x=300.0, y=100.0, d=bits(0))])
    s, t = free(F)
    s[0], t[0], s[2], t[2] = 7, 1, 8, 0
    out.append(Case("taken", "mps", (F, Q, s, t, NN, 1.0, False, 0.0), ("mps.taken", "mps.taken:never")))
    # mps.stereo: R = 4.  |54 - 50| == R stays, one float further goes; u_right == 0.0 exactly is monocular
    assert abs(f32(f32(54.0) - f32(50.0))) == f32(4.0) and abs(f32(up(54.0) - f32(50.0))) > f32(4.0)
    F = gframe([(100.0, 100.0, 0, bits(5)), (200.0, 100.0, 0, bits(5)), (300.0, 100.0, 0, bits(5))],
               u_right=[50.0, 50.0, 0.0])
    Q = mpq([dict(x=100.0, y=100.0, d=bits(0), xr=54.0), dict(x=200.0, y=100.0, d=bits(0), xr=up(54.0)),
             dict(x=300.0, y=100.0, d=bits(0), xr=54.0)])
    out.append(Case("stereo", "mps", (F, Q, *free(F), NN, 1.0, False, 0.0), ("mps.stereo", "mps.stereo:kpr")))
    # the top-2 and its tests, one query per 100 px:
    #   0 tie: two at 10 on different octaves (no ratio test): the first wins
    #   1 top2: two at 10 on one octave: the second is bestDist2 and 10 > 0.7f * 10 rejects
    #   2, 3 accept: 100 alone, 101 alone
    #   4, 5 ratio: (35, 50) on one octave, 35 > 0.7f * 50 = 35.0f is false; (36, 50) is rejected
    #   6 ratio:level: (30, 31) on two octaves is not tested
    #   7, 8 distance 256: as the only candidate (no match), and as the second best
    kps = [(100.0, 100.0, 0, bits(10)), (101.0, 100.0, 1, bits(10)),
           (200.0, 100.0, 0, bits(10)), (201.0, 100.0, 0, bits(10)),
           (300.0, 100.0, 0, bits(100)), (400.0, 100.0, 0, bits(101)),
           (100.0, 200.0, 0, bits(35)), (101.0, 200.0, 0, bits(50)),
           (200.0, 200.0, 0, bits(36)), (201.0, 200.0, 0, bits(50)),
           (300.0, 200.0, 0, bits(30)), (301.0, 200.0, 1, bits(31)),
           (400.0, 200.0, 0, bits(256)), (500.0, 200.0, 0, bits(10)), (501.0, 200.0, 0, bits(256))]
    F = gframe(kps)
    assert cell_of(F, 100.0, 100.0) == cell_of(F, 101.0, 100.0)
    qs = [(100.0, 100.0, 1), (200.0, 100.0, 0), (300.0, 100.0, 0), (400.0, 100.0, 0), (100.0, 200.0, 0),
          (200.0, 200.0, 0), (300.0, 200.0, 1), (400.0, 200.0, 0), (500.0, 200.0, 0)]
    Q = mpq([dict(x=x, y=y, lvl=l, d=bits(0)) for x, y, l in qs])
    out.append(Case("top2", "mps", (F, Q, *free(F), NN, 1.0, False, 0.0),
                    ("mps.tie", "mps.top2", "mps.accept", "mps.ratio", "mps.ratio:double", "mps.ratio:level")))
    return out


_MPS2_RAW = {}


def _mps2(name, left, right, l2r, r2l, rows, flips, taken=(), far=False, rider=False):
    """A two-camera mps case at th = 2 (left radius 8, right radius 4 at level 0).  taken: (slot, mp, taken).
    rider: one more left / right keypoint pair at RIDER_XY, the right one blocked, and an observation-less
    query that is an exact copy of the left one: its partner write lands on a blocked slot, which forces the
    serial redo of the whole problem (force_redo of tests/test_match_paths_gpu.py)."""
    _MPS2_RAW[name] = (left, right, l2r, r2l, rows, flips, taken, far)
    left, right, l2r, r2l, rows, taken = list(left), list(right), list(l2r), list(r2l), list(rows), list(taken)
    if rider:
        assert all(abs(k[0] - RIDER_XY[0]) > 40 for k in left + right)
        left.append((RIDER_XY[0], RIDER_XY[1], 0, bits(77)))
        right.append((RIDER_XY[0], RIDER_XY[1], 0, bits(200)))
        l2r.append(len(right) - 1)
        r2l.append(len(left) - 1)
        rows.append(dict(x=RIDER_XY[0], y=RIDER_XY[1], d=bits(77), obs=0))
        taken.append((("R", len(right) - 1), 700000, 1))
    F = gframe(left, right=right, l2r=np.array(l2r, np.int32), r2l=np.array(r2l, np.int32))
    s, t = free(F)
    for slot, mp, tk in taken:
        k = slot[1] + (F.nleft if slot[0] == "R" else 0)
        s[k], t[k] = mp, tk
    return Case(name + ("+rider" if rider else ""), "mps", (F, mpq(rows, two=True), s, t, NN, 2.0, far, 20.0), flips)


def _mps_two_cam():
    out = []
    none = lambda n: [-1] * n  # noqa: E731
    # the gates of the one-camera case for MapPoints seen by the right camera alone
    out.append(_mps2("gates_right", [(600.0, 100.0, 0, bits(0))],
                     [(100.0, 100.0, 0, bits(5)), (200.0, 100.0, 0, bits(5)), (300.0, 100.0, 0, bits(5))], none(1), none(3),
                     [dict(view=0, rview=1, rx=100.0, ry=100.0, d=bits(0), depth=20.0),
                      dict(view=0, rview=1, rx=200.0, ry=100.0, d=bits(0), depth=up(20.0)),
                      dict(view=0, rview=1, rx=300.0, ry=100.0, d=bits(0), usable=0)], ("mps.far", "mps.bad"), far=True))
    # mps.skip_right: the left top-2 (10, 10) fails the ratio test, which skips a right pass with a perfect
    # candidate; query 1 has no left candidates at all and its right pass runs
    out.append(_mps2("skip_right", [(100.0, 100.0, 0, bits(10)), (101.0, 100.0, 0, bits(10))],
                     [(100.0, 100.0, 0, bits(0)), (300.0, 100.0, 0, bits(0))], none(2), none(2),
                     [dict(x=100.0, y=100.0, d=bits(0), rview=1, rx=100.0, ry=100.0),
                      dict(x=300.0, y=300.0, d=bits(0), rview=1, rx=300.0, ry=100.0)], ("mps.skip_right",)))
    # mps.partner: the left match's stereo partner is written too (and counted); likewise from the right
    out.append(_mps2("partner", [(100.0, 100.0, 0, bits(3)), (300.0, 100.0, 0, bits(9))],
                     [(120.0, 100.0, 0, bits(90)), (320.0, 100.0, 0, bits(4))], [0, 1], [0, 1],
                     [dict(x=100.0, y=100.0, d=bits(0)),
                      dict(view=0, rview=1, rx=320.0, ry=100.0, d=bits(0))], ("mps.partner", "mps.partner:r2l")))
    # mps.own: each query's left match has its partner (2 away) and another right keypoint (20 away) in the
    # right window.  Query 0 has observations: its own partner write blocks the partner; query 1 has none.
    out.append(_mps2("own", [(100.0, 100.0, 0, bits(1)), (300.0, 100.0, 0, bits(1))],
                     [(100.0, 200.0, 0, bits(2)), (101.0, 200.0, 0, bits(20)),
                      (300.0, 200.0, 0, bits(2)), (301.0, 200.0, 0, bits(20))], [0, 2], [0, -1, 1, -1],
                     [dict(x=100.0, y=100.0, d=bits(0), rview=1, rx=100.0, ry=200.0, obs=1),
                      dict(x=300.0, y=100.0, d=bits(0), rview=1, rx=300.0, ry=200.0, obs=0)],
                     ("mps.own", "mps.own:never")))
    # mps.level_r: mnTrackScaleLevelR == -1 skips the right pass.  mps.radius_r: th = 2 widens the left window
    # only: the right keypoint 5 px from query 1's right projection is out, the one 3 px from query 2's in.
    out.append(_mps2("right_pass", [(600.0, 100.0, 0, bits(0))],
                     [(100.0, 100.0, 3, bits(1)), (205.0, 100.0, 0, bits(1)), (303.0, 100.0, 0, bits(1))],
                     none(1), none(3),
                     [dict(view=0, rview=1, rx=100.0, ry=100.0, rlvl=-1, d=bits(0)),
                      dict(view=0, rview=1, rx=200.0, ry=100.0, rlvl=0, d=bits(0)),
                      dict(view=0, rview=1, rx=300.0, ry=100.0, rlvl=0, d=bits(0))], ("mps.level_r", "mps.radius_r")))
    # mps.level and mps.radius in the right pass, whose window is computed apart from the left one's
    c = f32(0.998)
    out.append(_mps2("right_level_radius", [(600.0, 100.0, 0, bits(0))],
                     [(200.0, 200.0, 0, bits(1)), (201.0, 200.0, 1, bits(8)), (200.0, 201.0, 2, bits(9)),
                      (201.0, 201.0, 3, bits(2)), (103.0, 100.0, 0, bits(5)), (303.0, 100.0, 0, bits(5))],
                     none(1), none(6),
                     [dict(view=0, rview=1, rx=200.0, ry=200.0, rlvl=2, d=bits(0)),
                      dict(view=0, rview=1, rx=100.0, ry=100.0, rlvl=0, rcos=c, d=bits(0)),
                      dict(view=0, rview=1, rx=300.0, ry=100.0, rlvl=0, rcos=down(c), d=bits(0))],
                     ("mps.level", "mps.level:narrow", "mps.radius")))
    # the one-camera top-2 decisions in the right pass, and right slots that hold a MapPoint (8: with
    # observations, blocked; 10: without, taken again)
    out.append(_mps2("right_top2", [(600.0, 100.0, 0, bits(0))],
                     [(100.0, 100.0, 0, bits(10)), (101.0, 100.0, 1, bits(10)),
                      (200.0, 100.0, 0, bits(10)), (201.0, 100.0, 0, bits(10)),
                      (300.0, 100.0, 0, bits(100)), (400.0, 100.0, 0, bits(101)),
                      (100.0, 200.0, 0, bits(35)), (101.0, 200.0, 0, bits(50)),
                      (200.0, 200.0, 0, bits(1)), (201.0, 200.0, 0, bits(20)),
                      (300.0, 200.0, 0, bits(1)), (301.0, 200.0, 0, bits(20))], none(1), none(12),
                     [dict(view=0, rview=1, rx=x, ry=y, rlvl=l, d=bits(0)) for x, y, l in
                      [(100.0, 100.0, 1), (200.0, 100.0, 0), (300.0, 100.0, 0), (400.0, 100.0, 0), (100.0, 200.0, 0),
                       (200.0, 200.0, 0), (300.0, 200.0, 0)]],
                     ("mps.tie", "mps.top2", "mps.accept", "mps.ratio", "mps.ratio:double", "mps.taken",
                      "mps.taken:never"), taken=[(("R", 8), 9, 1), (("R", 10), 8, 0)]))
    return out


def redo_rider(case):
    """A two-camera mps case with the rider of _mps2."""
    left, right, l2r, r2l, rows, flips, taken, far = _MPS2_RAW[case.name]
    return _mps2(case.name, left, right, l2r, r2l, rows, flips, taken, far, rider=True)


# ------------------------------------------------------------------------------------ last

def _last_cases():
    out = []
    # last.invz: invz == 0 stays, below it goes.  last.bounds: u / v exactly on the image bounds stay (level 7,
    # radius > 10: the keypoints of the clamp world are in reach)
    kps = [(100.0, 100.0, 0, bits(5)), (200.0, 100.0, 0, bits(5)), (1.0, 300.0, 7, bits(5)), (745.0, 300.0, 7, bits(5)),
           (300.0, 1.0, 7, bits(5)), (300.0, 474.0, 7, bits(5))]
    F = gframe(kps)
    assert F.min_x == 0.0 and F.max_x == 752.0 and F.min_y == 0.0 and F.max_y == 480.0 and f32(3.0) * F.scale[7] > 10
    L = lastq([dict(x=100.0, y=100.0, d=bits(0), invz=0.0), dict(x=200.0, y=100.0, d=bits(0), invz=-1e-6),
               dict(x=0.0, y=300.0, o=7, d=bits(0)), dict(x=752.0, y=300.0, o=7, d=bits(0)),
               dict(x=300.0, y=0.0, o=7, d=bits(0)), dict(x=300.0, y=480.0, o=7, d=bits(0)),
               dict(x=up(752.0), y=300.0, o=7, d=bits(0)), dict(x=300.0, y=down(0.0), o=7, d=bits(0))])
    out.append(Case("gates", "last", (F, L, *free(F), 3.0), ("last.invz", "last.bounds")))
    # the level windows, query octave 2: forward [2, inf) picks octave 2 (3 away), backward [0, 2] octave 2,
    # otherwise [1, 3] octave 1.  tlc_z exactly +-mb is neither forward nor backward.
    lv =[(100.0, 100.0, 1, bits(1)), (101.0, 100.0, 2, bits(3)), (100.0, 101.0, 4, bits(5))]
    F = gframe(lv)
    mbf = float(f32(F.mb))
    q = [dict(x=100.0, y=100.0, o=2, d=bits(0))]
    out.append(Case("at_mb", "last", (F, lastq(q, tlc_z=mbf), *free(F), 3.0), ("last.forward",)))
    out.append(Case("forward", "last", (F, lastq(q, tlc_z=1.0), *free(F), 3.0),
                    ("last.mono", "last.level:fwd", "last.level:fwd_narrow")))
    lb = [(100.0, 100.0, 3, bits(1)), (101.0, 100.0, 2, bits(3)), (100.0, 101.0, 0, bits(5))]
    F = gframe(lb)
    out.append(Case("at_minus_mb", "last", (F, lastq(q, tlc_z=-mbf), *free(F), 3.0), ("last.backward",)))
    out.append(Case("backward", "last", (F, lastq(q, tlc_z=-1.0), *free(F), 3.0),
                    ("last.level:bwd", "last.level:bwd_narrow")))
    F = gframe([(100.0, 100.0, 0, bits(1)), (101.0, 100.0, 4, bits(2)), (100.0, 101.0, 1, bits(3)),
                (101.0, 101.0, 2, bits(5))])
    out.append(Case("level", "last", (F, lastq(q), *free(F), 3.0), ("last.level", "last.level:narrow")))
    # last.taken as mps.taken; last.tie, last.accept (100 / 101 alone)
    F = gframe([(100.0, 100.0, 0, bits(1)), (101.0, 100.0, 0, bits(20)), (200.0, 100.0, 0, bits(1)),
                (201.0, 100.0, 0, bits(20)), (300.0, 100.0, 0, bits(1)), (301.0, 100.0, 0, bits(20)),
                (400.0, 100.0, 0, bits(10)), (401.0, 100.0, 0, bits(10)), (500.0, 100.0, 0, bits(100)),
                (600.0, 100.0, 0, bits(101))])
    assert cell_of(F, 400.0, 100.0) == cell_of(F, 401.0, 100.0)
    L = lastq([dict(x=100.0, y=100.0, d=bits(0)), dict(x=200.0, y=100.0, d=bits(0)),
               dict(x=300.0, y=100.0, d=bits(0), obs=0), dict(x=300.0, y=100.0, d=bits(0)),
               dict(x=300.0, y=100.0, d=bits(0)), dict(x=400.0, y=100.0, d=bits(0)), dict(x=500.0, y=100.0, d=bits(0)),
               dict(x=600.0, y=100.0, d=bits(0))])
    s, t = free(F)
    s[0], t[0], s[2], t[2] = 7, 1, 8, 0
    out.append(Case("top", "last", (F, L, s, t, 3.0), ("last.taken", "last.taken:never", "last.tie", "last.accept")))
    # last.stereo: ur = u - mbf * invz in float; |ur - u_right| == radius stays, one float further goes;
    # u_right == 0.0 exactly is monocular
    F0 = gframe([(100.0, 100.0, 0, bits(5))])
    ur = f32(f32(100.0) - f32(f32(F0.mbf) * f32(0.1)))
    kr, kr_out = f32(ur - f32(3.0)), down(f32(ur - f32(3.0)))
    assert abs(f32(ur - kr)) == f32(3.0) and abs(f32(ur - kr_out)) > f32(3.0) and kr_out > 0
    F = gframe([(100.0, 100.0, 0, bits(5)), (100.0, 200.0, 0, bits(5)), (100.0, 300.0, 0, bits(5))],
               u_right=[kr, kr_out, 0.0])
    L = lastq([dict(x=100.0, y=y, d=bits(0)) for y in (100.0, 200.0, 300.0)])
    out.append(Case("stereo", "last", (F, L, *free(F), 3.0), ("last.stereo", "last.stereo:kpr")))
    # two cameras.  last.empty_left: query 0's left window is empty, which skips its right pass; query 1's left
    # window holds a keypoint 120 away (no left match) and its right pass runs.  A tie in the right pass.
    # and 100 / 101 alone in the right pass, which has its own accept test.
    F = gframe([(300.0, 100.0, 0, bits(120))],
               right=[(100.0, 100.0, 0, bits(1)), (300.0, 100.0, 0, bits(1)), (500.0, 100.0, 0, bits(10)),
                      (501.0, 100.0, 0, bits(10)), (600.0, 100.0, 0, bits(100)), (700.0, 100.0, 0, bits(101))])
    L = lastq([dict(x=100.0, y=300.0, d=bits(0), rx=100.0, ry=100.0), dict(x=300.0, y=100.0, d=bits(0), rx=300.0, ry=100.0),
               dict(x=300.0, y=100.0, d=bits(0), rx=500.0, ry=100.0), dict(x=300.0, y=100.0, d=bits(0), rx=600.0, ry=100.0),
               dict(x=300.0, y=100.0, d=bits(0), rx=700.0, ry=100.0)], two=True)
    out.append(Case("empty_left", "last", (F, L, *free(F), 3.0), ("last.empty_left", "last.tie", "last.accept")))
    # last.hist_right: bins 0, 2, 3 hold two left matches each; the last query's left match is in bin 0 and
    # its right match in bin 5, which is dropped
    pos = [mb._lattice(i) for i in range(7)]
    ang = [0.0, 0.0, 60.0, 60.0, 90.0, 90.0, 150.0]
    F = gframe([(x, y, 0, bits(0), 0.0 if i < 6 else 150.0) for i, (x, y) in enumerate(pos)],
               right=[(pos[6][0], pos[6][1], 0, bits(0), 0.0)])
    assert pr.rot_bin(150.0, 0.0) == 5 and pr.rot_bin(150.0, 150.0) == 0
    L = lastq([dict(x=x, y=y, d=bits(0), ang=a, rx=(x if i == 6 else -500.0), ry=y)
               for i, ((x, y), a) in enumerate(zip(pos, ang))], two=True)
    out.append(Case("hist_right", "last", (F, L, *free(F), 3.0), ("last.hist_right",)))
    # last.hist_stale: query 6 (no observations, bin 5) and query 7 (bin 0) both take keypoint 6; bin 5 is
    # dropped, and with it the keypoint's MapPoint, although the match that holds it is in bin 0
    F = gframe([(x, y, 0, bits(0), 0.0) for x, y in pos])
    L = lastq([dict(x=x, y=y, d=bits(0), ang=a, obs=int(i != 6)) for i, ((x, y), a) in enumerate(zip(pos, ang))]
              + [dict(x=pos[6][0], y=pos[6][1], d=bits(0), ang=0.0)])
    out.append(Case("hist_stale", "last", (F, L, *free(F), 3.0), ("last.hist_stale",)))
    return out


# ------------------------------------------------------------------------------------ kf

def _kf_cases():
    out = []
    # kf.level: [1, 3] around level 2
    F = gframe([(100.0, 100.0, 0, bits(1)), (101.0, 100.0, 4, bits(2)), (100.0, 101.0, 3, bits(3)),
                (101.0, 101.0, 1, bits(5))])
    K = kfq([dict(x=100.0, y=100.0, lvl=2, d=bits(0))])
    out.append(Case("level", "kf", (F, K, free(F)[0], 3.0, 100), ("kf.level", "kf.level:narrow")))
    # kf.taken: any MapPoint blocks; kf.tie; kf.accept against the parameter: 64 and 65 alone at ORBdist 64
    F = gframe([(100.0, 100.0, 0, bits(1)), (101.0, 100.0, 0, bits(20)), (200.0, 100.0, 0, bits(10)),
                (201.0, 100.0, 0, bits(10)), (300.0, 100.0, 0, bits(64)), (400.0, 100.0, 0, bits(65))])
    assert cell_of(F, 200.0, 100.0) == cell_of(F, 201.0, 100.0)
    K = kfq([dict(x=x, y=100.0, d=bits(0)) for x in (100.0, 200.0, 300.0, 400.0)])
    s = free(F)[0]
    s[0] = 7
    out.append(Case("top", "kf", (F, K, s, 3.0, 64), ("kf.taken", "kf.tie", "kf.accept", "kf.accept:high")))
    return out


# ------------------------------------------------------------------------------------ SearchByBoW

def _bow_case(two):
    """SearchByBoW(KF, F), one decision per vocabulary node.  two: the frame's right-camera features and the
    nodes that need them."""
    kf, fl, fr_ = [], [], []   # (descriptor, node[, angle, good]); frame features: (descriptor, node)
    # node 1, bow.side (first: its right feature has index nleft exactly): the left 20 and the right 1 both match
    if two:
        kf += [(bits(0), 1)]
        fl += [(bits(20), 1)]
        fr_ += [(bits(1), 1)]
    # node 2, bow.good: the feature without a good MapPoint would take the frame feature first
    kf += [(bits(1), 2, 0.0, 0), (bits(5), 2)]
    fl += [(bits(0), 2)]
    # node 3, bow.taken: the second feature finds its best taken and takes the other
    kf += [(bits(1), 3), (bits(2), 3)]
    fl += [(bits(0), 3), (bits(32), 3)]
    # node 4, bow.top2: two at 10, 10 < 0.7f * 10 fails
    kf += [(bits(0), 4)]
    fl += [(bits(10), 4), (bits(10), 4)]
    # nodes 5, 6, bow.accept: 50 alone, 51 alone
    kf += [(bits(0), 5), (bits(0), 6)]
    fl += [(bits(50), 5), (bits(51), 6)]
    # nodes 7, 8, bow.ratio: (35, 50): 35 < 0.7f * 50 = 35.0f is false; (34, 50) passes
    kf += [(bits(0), 7), (bits(0), 8)]
    fl += [(bits(35), 7), (bits(50), 7), (bits(34), 8), (bits(50), 8)]
    # nodes 9, 10, distance 256: as the only candidate, and as the second best
    kf += [(bits(0), 9), (bits(0), 10)]
    fl += [(bits(256), 9), (bits(10), 10), (bits(256), 10)]
    flips = ["bow.good", "bow.taken", "bow.top2", "bow.accept", "bow.ratio", "bow.nodes"]
    if two:
        # node 11, bow.right_gate: left best 60: the right 5 is not looked at
        kf += [(bits(0), 11)]
        fl += [(bits(60), 11)]
        fr_ += [(bits(5), 11)]
        # node 12, bow.right_gate:ratio: left (10, 10) fails the ratio test, the right 5 is still taken
        kf += [(bits(0), 12)]
        fl += [(bits(10), 12), (bits(10), 12)]
        fr_ += [(bits(5), 12)]
        # node 13, bow.right_ratio and bow.tie: left 5 alone; right (10, 10): no ratio test, the first wins
        kf += [(bits(0), 13)]
        fl += [(bits(5), 13)]
        fr_ += [(bits(10), 13), (bits(10), 13)]
        flips += ["bow.side", "bow.right_gate", "bow.right_gate:ratio", "bow.right_ratio", "bow.tie"]
    # bow.nodes: the last node of each side, 20 and 21, is not shared
    kf += [(bits(0), 20)]
    fl += [(bits(1), 21)]
    KF = bside(kf)
    F = bside(fl + fr_, nleft=len(fl) if two else -1, id_base=-1)
    assert len(KF.node_id) == len(F.node_id) and (KF.node_id[:-1] == F.node_id[:-1]).all()
    assert not two or int(F.feat[F.node_start[0] + 1]) == F.nleft
    return Case("two_cam" if two else "one_cam", "bow", (KF, F, NN), tuple(flips))


def _bowkk_case(two):
    """SearchByBoW(KF, KF), one decision per node; K2 features: (descriptor, node, angle, good, mp_id)."""
    k1, k2, r1, r2 = [], [], [], []
    mp = lambda i: 5000 + i  # noqa: E731
    # nodes 1, 2, bowkk.accept: strict: 49 alone, 50 alone
    k1 += [(bits(0), 1), (bits(0), 2)]
    k2 += [(bits(49), 1), (bits(50), 2)]
    # nodes 3, 4, bowkk.ratio: (35, 50) fails, (34, 50) passes
    k1 += [(bits(0), 3), (bits(0), 4)]
    k2 += [(bits(35), 3), (bits(50), 3), (bits(34), 4), (bits(50), 4)]
    # node 5, bowkk.matched2: the second feature finds its best matched and takes the other
    k1 += [(bits(1), 5), (bits(2), 5)]
    k2 += [(bits(0), 5), (bits(32), 5)]
    # nodes 6, 7, bowkk.mp2: the closest K2 feature has no MapPoint / a bad one
    k1 += [(bits(0), 6), (bits(0), 7)]
    k2 += [(bits(1), 6, 0.0, 1, -1), (bits(20), 6), (bits(1), 7, 0.0, 0), (bits(20), 7)]
    # node 8, bowkk.top2: two at 10
    k1 += [(bits(0), 8)]
    k2 += [(bits(10), 8), (bits(10), 8)]
    flips = ["bowkk.accept", "bowkk.ratio", "bowkk.matched2", "bowkk.mp2", "bowkk.mp2:bad", "bowkk.top2"]
    if two:
        # node 9, bowkk.right: a right-camera K1 feature with a perfect partner; node 10, bowkk.right:k2: the
        # closest K2 feature is a right-camera one
        r1 += [(bits(0), 9)]
        k2 += [(bits(0), 9)]
        k1 += [(bits(0), 10)]
        k2 += [(bits(20), 10)]
        r2 += [(bits(1), 10)]
        flips += ["bowkk.right", "bowkk.right:k2"]
    K1 = bside(k1 + r1, nleft=len(k1) if two else -1)
    feats = [f if len(f) > 4 else (f[0], f[1], 0.0, f[3] if len(f) > 3 else 1, mp(i)) for i, f in enumerate(k2 + r2)]
    K2 = bside(feats, nleft=len(k2) if two else -1)
    return Case("two_cam" if two else "one_cam", "bowkk", (K1, K2, NN), tuple(flips))


def _bow_special_cases():
    out = []
    # ratio:double: (12, 20) at 0.6f: the float product is 12.0 (12 < 12 fails), the double one 12.0000005
    KF = bside([(bits(0), 1)])
    F = bside([(bits(12), 1), (bits(20), 1)], id_base=-1)
    out.append(Case("ratio_double", "bow", (KF, F, NN_UP), ("bow.ratio:double", "bow.ratio")))
    K2 = bside([(bits(12), 1), (bits(20), 1)], id_base=5000)
    out.append(Case("ratio_double", "bowkk", (KF, K2, NN_UP), ("bowkk.ratio:double", "bowkk.ratio")))
    # bowkk.tie: every match passes the ratio test, so a tie at the minimum shows only at nnratio > 1
    K2 = bside([(bits(10), 1), (bits(10), 1)], id_base=5000)
    assert f32(10) < f32(1.25) * f32(10)
    out.append(Case("tie", "bowkk", (KF, K2, 1.25), ("bowkk.tie",)))
    return out


# ------------------------------------------------------------------------------------ rotation histogram

def _hist_cases():
    out = []
    for name, pairs, flips in mb._hist_worlds():
        n = len(pairs)
        pos = [mb._lattice(i) for i in range(n)]
        F = gframe([(x, y, 0, bits(0), a[1]) for (x, y), a in zip(pos, pairs)])
        L = lastq([dict(x=x, y=y, d=bits(0), ang=a[0]) for (x, y), a in zip(pos, pairs)])
        out.append(Case("hist_" + name, "last", (F, L, *free(F), 3.0), flips))
        K = kfq([dict(x=x, y=y, d=bits(0), ang=a[0]) for (x, y), a in zip(pos, pairs)])
        out.append(Case("hist_" + name, "kf", (F, K, free(F)[0], 3.0, 100), flips))
        A = bside([(bits(0), i, a[0]) for i, a in enumerate(pairs)])
        B = bside([(bits(0), i, a[1]) for i, a in enumerate(pairs)], id_base=5000)
        out.append(Case("hist_" + name, "bow", (A, B, NN), flips))
        out.append(Case("hist_" + name, "bowkk", (A, B, NN), flips))
    return out


# ------------------------------------------------------------------------------------ claim chains

def chain(kind, n=64):
    """n queries and n slots: query 0 sees slot 0 alone, query q's best is slot q - 1 (1 away) and its
    runner-up slot q (3 away).  Every query finds its best taken by the query before it, so the sequential
    result (query q in slot q) needs one round of the fixed point per query."""
    slot_d = [bits(4 * j) for j in range(n)]
    q_d = [bits(0)] + [bits(4 * q - 3) for q in range(1, n)]
    if kind in ("bow", "bowkk"):
        A = bside([(d, 1) for d in q_d])
        B = bside([(d, 1) for d in slot_d], id_base=5000 if kind == "bowkk" else -1)
        return Case("chain", kind, (A, B, NN), ())
    # grid operators: slot j at x = 100 + 4 j, windows of radius 4 (strict), query q half way between q - 1 and q
    F = gframe([(100.0 + 4.0 * j, 100.0, 0, d) for j, d in enumerate(slot_d)])
    xs = [100.0] + [100.0 + 4.0 * q - 2.0 for q in range(1, n)]
    if kind == "mps":
        return Case("chain", kind, (F, mpq([dict(x=x, y=100.0, d=d) for x, d in zip(xs, q_d)]), *free(F), NN, 1.0,
                                    False, 0.0), ())
    if kind == "last":
        return Case("chain", kind, (F, lastq([dict(x=x, y=100.0, d=d) for x, d in zip(xs, q_d)]), *free(F), 4.0), ())
    return Case("chain", kind, (F, kfq([dict(x=x, y=100.0, d=d) for x, d in zip(xs, q_d)]), free(F)[0], 4.0, 100), ())


# ------------------------------------------------------------------------------------ all of them

def _build():
    out = _area_cases() + _mps_one_cam() + _mps_two_cam() + _last_cases() + _kf_cases()
    out += [_bow_case(False), _bow_case(True), _bowkk_case(False), _bowkk_case(True)] + _bow_special_cases()
    out += _hist_cases()
    assert len({c.id for c in out}) == len(out)
    assert all(size(c) <= 64 for c in out)
    return out


CASES = _build()


def of_kind(kind):
    return [c for c in CASES if c.kind == kind]


def two_cam(case):
    return case.args[0].nleft != -1
