"""CPU: the CreateNewMapPoints fixtures (tests/newpoints_fixtures.py), their guard and margins, the named shapes
they are there for, the select rule restated on the host against the sequential restatement
(tests/pyref_newpoints.py), and the argument checks the entry points make before a device is touched."""
import copy

import numpy as np
import pytest

from orb_slam3_comments_ghr_amd import _abi
from orb_slam3_comments_ghr_amd import localmapping as L
from tests import newpoints_fixtures as FX
from tests import pyref_newpoints as R


def code(o):
    return o.status & 0x7f


@pytest.mark.parametrize("name", list(FX.FIXTURES))
def test_fixture_guard_holds(name):
    assert FX.guard(name) == []
    if name in FX.HAND_MADE:
        assert not FX.borderline(name)


def test_margins_profile_is_current():
    """The committed profile is what tools/newpoints_margins.py measures on the committed fixtures: every tolerance
    is 10 x the largest movement in the group, never a chosen number."""
    m = FX.margins()
    assert set(m["fixtures"]) == set(FX.FIXTURES) and set(m["groups"]) == set(FX.GROUPS)
    for name in ("claim3", "far", "stereo10", "zero_dist", "kb8_4", "rig4"):
        for q, v in FX.spreads(name).items():
            assert m["fixtures"][name][q] == pytest.approx(v, rel=1e-6, abs=1e-15), (name, q)
    for g in FX.GROUPS:
        members = [k for k in FX.FIXTURES if FX.group(k) == g]
        for q in FX.KINDS:
            assert m["groups"][g]["max"][q] == max(m["fixtures"][k][q] for k in members)
            assert m["groups"][g]["tol"][q] == 10.0 * m["groups"][g]["max"][q]
    assert all(v["valid"] and v["borderline"] <= int(FX.MAX_BORDERLINE * v["matches"]) for v in m["fixtures"].values())


def test_pyref_is_cited_in_its_own_terms():
    """The mirror's status codes are the ABI's."""
    assert (R.NONE, R.CREATED, R.LOW_PARALLAX, R.NO_POINT, R.Z1, R.Z2, R.REPROJ1, R.REPROJ2, R.ZERO_DIST, R.FAR,
            R.SCALE, R.STEREO_BIT) == (_abi.NP_NONE, _abi.NP_CREATED, _abi.NP_LOW_PARALLAX, _abi.NP_NO_POINT,
                                       _abi.NP_Z1, _abi.NP_Z2, _abi.NP_REPROJ1, _abi.NP_REPROJ2, _abi.NP_ZERO_DIST,
                                       _abi.NP_FAR, _abi.NP_SCALE, _abi.NP_STEREO_BIT)
    assert tuple(R.HAS_POINT) == tuple(L.NP_HAS_POINT)


# ------------------------------------------------------------------------------------------- what each is for
def test_empty_cases():
    o = FX.reference("b0")
    assert o.match.shape == (0, 40) and o.n_created.shape == (0,)
    for name in ("no_shared_node", "all_mapped"):
        o = FX.reference(name)
        assert not o.skipped.any() and not (o.match >= 0).any() and not o.n_created.any()
    assert FX.build("all_mapped").kf1.has_mp.all()


def test_smallest_case():
    P, o = FX.build("one_query"), FX.reference("one_query")
    assert P.n_neigh == 1 and np.count_nonzero(P.kf1.has_mp == 0) == 1
    assert o.n_created.tolist() == [1] and np.count_nonzero(o.match >= 0) == 1


@pytest.mark.parametrize("n", [255, 256, 257])
def test_workgroup_edges(n):
    P = FX.build("q%d" % n)
    K1, K2 = P.kf1, P.kf2[0]
    shared = np.isin(FX._nodes(K1), K2.node_id)
    assert P.n_neigh == 1 and K1.n == n and np.count_nonzero(shared & (K1.has_mp == 0)) == n  # n queries
    assert FX.reference("q%d" % n).n_created[0] > 100


def test_claim_rule_first_accepted_wins():
    """A keypoint accepted at neighbours 0 and 2 is created at 0 only, and match at 2 is -1."""
    ev, o = FX.call_time("claim3"), FX.reference("claim3")
    ok = code(ev) == R.CREATED
    both = np.flatnonzero(ok[0] & ok[2])
    assert len(both) > 0
    assert np.all(code(o)[0, both] == R.CREATED) and np.all(o.match[2, both] == -1) and np.all(o.status[2, both] == 0)
    assert np.all(o.match[1, both] == -1)


def test_claim_rule_is_first_accepted_not_first_matched():
    """A keypoint matched at 0 but rejected for low parallax and accepted at 1 is created at 1."""
    ev, o = FX.call_time("claim3"), FX.reference("claim3")
    late = np.flatnonzero((code(ev)[0] == R.LOW_PARALLAX) & (code(ev)[1] == R.CREATED))
    assert len(late) > 0
    assert np.all(o.match[0, late] >= 0) and np.all(code(o)[0, late] == R.LOW_PARALLAX)
    assert np.all(code(o)[1, late] == R.CREATED) and np.all(o.match[1, late] == ev.match[1, late])


def test_two_keypoints_may_share_a_kf2_keypoint():
    """Two KF1 keypoints both matched to the same KF2 keypoint and both accepted are both created."""
    o = FX.reference("claim3")
    shared = []
    for b in range(3):
        made = np.flatnonzero(code(o)[b] == R.CREATED)
        idx2, cnt = np.unique(o.match[b, made], return_counts=True)
        shared += [(b, int(j)) for j in idx2[cnt > 1]]
    assert shared


def test_mono30_shape():
    P, o = FX.build("mono30"), FX.reference("mono30")
    assert P.monocular and P.n_neigh == 30 and P.kf1.n == 300
    assert o.skipped.tolist() == [0] * 14 + [1] + [0] * 15 and not (o.match[14] >= 0).any()
    assert o.n_created[15:].sum() > 0   # the loop goes on behind the skipped neighbour


def test_stereo10_shape():
    P, o = FX.build("stereo10"), FX.reference("stereo10")
    assert not P.monocular and P.n_neigh == 10
    assert o.skipped.tolist() == [0, 0, 1] + [0] * 7   # baseline < mb
    made = code(o) == R.CREATED
    st_bit = (o.status & R.STEREO_BIT) != 0
    s1 = np.broadcast_to(P.kf1.u_right >= 0, made.shape)
    assert (made & ~st_bit).any()          # triangulated
    assert (made & st_bit & s1).any()      # UnprojectStereo of the current KeyFrame
    assert (made & st_bit & ~s1).any()     # UnprojectStereo of the neighbour (if / else if of :757-765)
    assert (made & ~st_bit & s1).any()     # the 7.8 test applied to a triangulated point
    assert (o.status == (R.NO_POINT | R.STEREO_BIT)).any()   # a zero mvDepth


def test_stereo_mbf_quirk_decides_a_match():
    """ref:src/LocalMapping.cc:875 reads mpCurrentKeyFrame->mbf for the second KeyFrame; a restatement that reads
    pKF2->mbf instead disagrees where the two differ."""
    P, o = FX.build("stereo10"), FX.reference("stereo10")
    assert P.g2[3].mbf == FX.STEREO_MBF != P.g1.mbf
    fixed = R.run(P, R.Variant(fix_mbf=True))
    b, _ = np.nonzero(fixed.status != o.status)
    assert len(b) > 0 and b.min() == 3
    assert (code(o)[3] == R.REPROJ2).sum() > (code(fixed)[3] == R.REPROJ2).sum()


def test_kb8_shape():
    P = FX.build("kb8_4")
    assert P.n_neigh == 4 and P.g1.cam_type == _abi.CAM_KB8 and not P.kf1.two_cam and P.coarse


def test_rig_shape_and_ow1_quirk():
    P, o = FX.build("rig4"), FX.reference("rig4")
    assert P.n_neigh == 4 and P.kf1.two_cam and P.g1.cam_type == _abi.CAM_KB8
    pairs = {(R._right(P.kf1, i), R._right(P.kf2[b], int(o.match[b, i]))) for b, i in zip(*np.nonzero(o.match >= 0))}
    assert len(pairs) == 4
    last = int(np.flatnonzero(o.match[0] >= 0)[-1])
    assert R._right(P.kf1, last)   # the last match of neighbour 0 is a right-camera keypoint
    left, right = (R.baseline_test(P, 1, ow)[0] for ow in (P.g1.Ow, P.g1.Ow_r))
    assert (left, right) == (False, True)   # mb between the two baselines
    assert o.skipped.tolist() == [0, 1, 0, 0]   # the centre the last match left behind decides


def test_far_points_shape():
    P, o = FX.build("far"), FX.reference("far")
    assert P.far_points and (code(o) == R.FAR).any() and (code(o) == R.CREATED).any()
    Q = copy.copy(P)
    Q.far_points = False
    assert R.run(Q).n_created.sum() > o.n_created.sum()


def test_inertial_shape():
    """A match whose rays' cosine lies between 0.9996 and 0.9998 is decided the other way."""
    P, o = FX.build("inertial"), FX.reference("inertial")
    between = [k for k, q in o.quant.items() if "cos_limit" in q and 0 < q["cos_limit"] < 0.0002]
    assert P.inertial and between and all(code(o)[k] == R.LOW_PARALLAX for k in between)
    Q = copy.copy(P)
    Q.inertial = False
    other = R.run(Q)
    assert any(code(other)[k] != R.LOW_PARALLAX for k in between)


def test_every_status_code_occurs():
    seen = set()
    for name in FX.FIXTURES:
        o = FX.reference(name)
        seen |= set(code(o)[o.match >= 0].tolist())
    assert seen == set(range(1, 11))
    assert any((FX.reference(k).match < 0).any() for k in FX.FIXTURES)   # code 0


# ------------------------------------------------------------------------------------------- the select rule
@pytest.mark.parametrize("name", list(FX.FIXTURES))
def test_select_rule_equals_the_sequential_restatement(name):
    """Evaluate-all from pyref's per-pair function in, the sequential outputs out: the formulation of
    csrc/newpoints.hip (k_np_select), restated on the host, against the loop."""
    P, ref = FX.build(name), FX.reference(name)
    got = FX.select(P, FX.call_time(name))
    for arr in ("match", "status", "x3d", "skipped", "n_created"):
        assert getattr(got, arr).tobytes() == getattr(ref, arr).tobytes(), arr


def test_first_only_is_neighbour_zero():
    P = FX.build("claim3")
    o, f = FX.reference("claim3"), R.run(P, first_only=True)
    assert np.array_equal(f.match[0], o.match[0]) and not (f.match[1:] >= 0).any()


# ------------------------------------------------------------------------------------------- validation on the host
def test_bad_arguments_are_refused_without_a_device():
    P = FX.build("claim3")
    assert L.check_problem(P) == 0 and L.check_problem(FX.build("b0")) == 0

    def variant(**kw):
        Q = copy.copy(P)
        for k, v in kw.items():
            setattr(Q, k, v)
        return Q

    k = _abi.NEWPOINTS_MAX_NEIGHBOURS
    assert L.check_problem(variant(kf2=[P.kf2[0]] * k, g2=[P.g2[0]] * k, geom=[P.geom[0]] * k)) == 0
    k += 1
    assert L.check_problem(variant(kf2=[P.kf2[0]] * k, g2=[P.g2[0]] * k, geom=[P.geom[0]] * k)) == _abi.OSG_E_INVALID
    rig = copy.copy(P.kf2[1])
    rig.two_cam, rig.nleft = 1, rig.n // 2
    assert L.check_problem(variant(kf2=[P.kf2[0], rig, P.kf2[2]])) == _abi.OSG_E_UNSUPPORTED
    # negative counts and null arrays with positive counts, through the raw structure
    for field, value in (("n_neigh", -1), ("kf2", None), ("g2", None), ("geom", None)):
        s = P.struct()
        setattr(s, field, value)
        assert L.load_library().osg_create_new_map_points_check(s) == _abi.OSG_E_INVALID, field
    for field, value in (("n", -1), ("kp_x", None), ("desc", None), ("has_mp", None), ("level_sigma2", None)):
        s = P.struct()
        setattr(s.kf1, field, value)
        assert L.load_library().osg_create_new_map_points_check(s) == _abi.OSG_E_INVALID, field
    S = FX.build("stereo10").struct()
    S.g1.depth = None   # stereo keypoints without mvDepth
    assert L.load_library().osg_create_new_map_points_check(S) == _abi.OSG_E_INVALID
    assert L.load_library().osg_create_new_map_points_check(None) == _abi.OSG_E_INVALID
