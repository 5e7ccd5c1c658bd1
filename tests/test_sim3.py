"""The Sim3 projection matchers of LoopClosing (ref:src/ORBmatcher.cc:498-733): the oracle pinned by the
pure-Python restatement and a hand case (CPU); the GPU fixed-point greedy bit-exact against the oracle."""
import numpy as np
import pytest

from orb_slam3_comments_ghr_amd import frames as fr
from orb_slam3_comments_ghr_amd.matcher import ORBmatcher
from tests import oracle_calls as oc
from tests import pyref_match as pr

# LoopClosing's calls: (th, ratioHamming) at ref:src/LoopClosing.cc:1062, 1091, 1368
CALLS = [(8, 1.5), (5, 1.0), (3, 1.5)]


def world(seed, n=1000, m=3000, taken=0.1):
    rng = np.random.default_rng(seed)
    F = fr.synth_frame(rng, n=n, stereo=False)
    Q = fr.synth_fuse_queries(rng, F, m=m, match_frac=0.7)
    sq = np.where(rng.random(F.n) < taken, -2, -1).astype(np.int32)
    return F, Q, sq


@pytest.mark.parametrize("seed", range(3))
@pytest.mark.parametrize("th,ratio", CALLS)
def test_oracle_vs_python(oracle, seed, th, ratio):
    F, Q, sq = world(9000 + seed, n=250, m=500)
    ref = oc.sim3(oracle, F, Q, th, ratio, sq)
    got = pr.search_sim3(F, Q, th, ratio, sq)
    assert ref[0] == got[0] and ref[0] > 20
    np.testing.assert_array_equal(ref[1], got[1])


def bits(k):
    b = np.zeros(256, np.uint8)
    b[:k] = 1
    return np.packbits(b)


def hand_case():
    """Keypoints 0 (100, 100) and 1 (102, 100) share a window; keypoint 2 (300, 100) is taken before the
    call.  MapPoint 0 (d 3 to keypoint 0, 38 to 1) takes keypoint 0; MapPoint 1 (d 1 and 40) finds 0 taken
    and falls back to 1 (40 <= 50 * 1.0); MapPoints 2 and 3 see only the taken keypoint 2."""
    F = fr.FrameSoA(desc=np.stack([bits(0), bits(41), bits(0)]), kp_x=np.array([100.0, 102.0, 300.0], np.float32),
                    kp_y=np.array([100.0, 100.0, 100.0], np.float32), kp_angle=np.zeros(3, np.float32),
                    kp_octave=np.zeros(3, np.int32))
    Q = fr.FuseQueries(desc=np.stack([bits(3), bits(1), bits(0), bits(60)]), valid=np.ones(4, np.uint8),
                       u=np.array([101, 101, 300, 300], np.float32), v=np.array([100, 100, 100, 100], np.float32),
                       ur=None, pred_level=np.zeros(4, np.int32), inv_level_sigma2=fr.inv_level_sigma2(F.scale))
    return F, Q, np.array([-1, -1, -2], np.int32)


def test_oracle_hand_case(oracle):
    F, Q, sq = hand_case()
    n, s_ = oc.sim3(oracle, F, Q, 3, 1.0, sq)
    assert n == 2 and s_.tolist() == [0, 1, -2]
    assert pr.search_sim3(F, Q, 3, 1.0, sq)[1].tolist() == [0, 1, -2]
    # ratioHamming 0.7: 40 > 35, MapPoint 1 gets nothing
    assert oc.sim3(oracle, F, Q, 3, 0.7, sq)[1].tolist() == [0, -1, -2]


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(3))
@pytest.mark.parametrize("th,ratio", CALLS)
def test_gpu_vs_oracle(ctx, oracle, seed, th, ratio):
    """LoopClosing shape: a 1200-keypoint keyframe, 3000-6000 projected MapPoints with slot collisions."""
    F, Q, sq = world(9100 + seed, n=1200, m=3000 * (1 + seed))
    n_ref, s_ref = oc.sim3(oracle, F, Q, th, ratio, sq)
    mp_id = 100000 + np.arange(Q.n, dtype=np.int32)
    vpMatched = np.where(sq == -2, 7, -1).astype(np.int32)
    kfs = np.arange(Q.n, dtype=np.int32) % 17
    vpMatchedKF = np.full(F.n, -1, np.int32)
    n = ORBmatcher(ctx).SearchByProjectionSim3(F, Q, mp_id, vpMatched, th, ratio, kfs, vpMatchedKF)
    assert n == n_ref and n > 300
    new = s_ref >= 0
    np.testing.assert_array_equal(vpMatched[new], mp_id[s_ref[new]])
    np.testing.assert_array_equal(vpMatched[s_ref == -2], 7)
    np.testing.assert_array_equal(vpMatched[s_ref == -1], -1)
    np.testing.assert_array_equal(vpMatchedKF[new], kfs[s_ref[new]])
    assert ctx.match_last_stats()["rounds"] >= 2  # collisions exercised the resolve


@pytest.mark.gpu
def test_gpu_hand_case_and_edges(ctx, oracle):
    F, Q, sq = hand_case()
    vp = np.where(sq == -2, 9, -1).astype(np.int32)
    assert ORBmatcher(ctx).SearchByProjectionSim3(F, Q, np.arange(4), vp, 3, 1.0) == 2
    assert vp.tolist() == [0, 1, 9]
    m = ORBmatcher(ctx)
    F, Q, sq = world(9200, n=600, m=0)
    assert m.SearchByProjectionSim3(F, Q, [], np.full(F.n, -1, np.int32), 3, 1.5) == 0
    F, Q, sq = world(9201, n=600, m=500)
    Q.valid[:] = 0
    assert m.SearchByProjectionSim3(F, Q, np.arange(500), np.full(F.n, -1, np.int32), 3, 1.5) == 0
    F, Q, sq = world(9202, n=600, m=500)
    vp = np.full(F.n, 5, np.int32)  # every slot taken before the call
    assert m.SearchByProjectionSim3(F, Q, np.arange(500), vp, 8, 1.5) == 0


# ---- ORBmatcher::SearchBySim3 (ref:src/ORBmatcher.cc:1696-1939)
SIM3_TH = [7.5, 10.0]  # no caller in this fork (ref:include/ORBmatcher.h:78); ORB-SLAM2's LoopClosing::ComputeSim3 used 7.5


@pytest.mark.parametrize("seed", range(3))
@pytest.mark.parametrize("th", SIM3_TH)
def test_search_by_sim3_oracle_vs_python(oracle, seed, th):
    K1, K2, q12, q21 = fr.synth_sim3_pair(np.random.default_rng(9300 + seed), n1=200, n2=260)
    ref = oc.search_by_sim3(oracle, K1, K2, q12, q21, th)
    got = pr.search_by_sim3(K1, K2, q12, q21, th)
    assert ref[0] == got[0] and ref[0] > 10
    np.testing.assert_array_equal(ref[1], got[1])


def test_search_by_sim3_hand_case(oracle):
    """KF1 keypoint 0 <-> KF2 keypoint 0 mutual (d 3 / 2); KF1 keypoint 1 -> KF2 keypoint 0 (d 1, a
    better one-way match, but KF2 keypoint 0 points back at KF1 keypoint 0): not mutual; KF1 keypoint 2
    -> KF2 keypoint 1 at d 101 > TH_HIGH: rejected."""
    F1 = fr.FrameSoA(desc=np.stack([bits(0), bits(90), bits(0)]), kp_x=np.array([100.0, 103.0, 300.0], np.float32),
                     kp_y=np.array([100.0, 100.0, 100.0], np.float32), kp_angle=np.zeros(3, np.float32),
                     kp_octave=np.zeros(3, np.int32))
    F2 = fr.FrameSoA(desc=np.stack([bits(2), bits(101)]), kp_x=np.array([200.0, 400.0], np.float32),
                     kp_y=np.array([200.0, 200.0], np.float32), kp_angle=np.zeros(2, np.float32),
                     kp_octave=np.zeros(2, np.int32))
    isg = fr.inv_level_sigma2(F1.scale)
    q12 = fr.FuseQueries(desc=np.stack([bits(3), bits(1), bits(0)]), valid=np.ones(3, np.uint8),
                         u=np.array([200, 200, 400], np.float32), v=np.array([200, 200, 200], np.float32), ur=None,
                         pred_level=np.zeros(3, np.int32), inv_level_sigma2=isg)
    q21 = fr.FuseQueries(desc=np.stack([bits(2), bits(0)]), valid=np.ones(2, np.uint8),
                         u=np.array([101, 300], np.float32), v=np.array([100, 100], np.float32), ur=None,
                         pred_level=np.zeros(2, np.int32), inv_level_sigma2=isg)
    n, m12 = oc.search_by_sim3(oracle, F1, F2, q12, q21, 7.5)
    assert n == 1 and m12.tolist() == [0, -1, -1]
    assert pr.search_by_sim3(F1, F2, q12, q21, 7.5)[1].tolist() == [0, -1, -1]


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(3))
@pytest.mark.parametrize("th", SIM3_TH)
def test_search_by_sim3_gpu_vs_oracle(ctx, oracle, seed, th):
    K1, K2, q12, q21 = fr.synth_sim3_pair(np.random.default_rng(9400 + seed), n1=1200, n2=1100 + 100 * seed)
    n_ref, m_ref = oc.search_by_sim3(oracle, K1, K2, q12, q21, th)
    n, m12 = ORBmatcher(ctx).SearchBySim3(K1, K2, q12, q21, th)
    assert n == n_ref and n > 200
    np.testing.assert_array_equal(m12, m_ref)


@pytest.mark.gpu
def test_search_by_sim3_gpu_empty(ctx):
    K1, K2, q12, q21 = fr.synth_sim3_pair(np.random.default_rng(1), n1=50, n2=60)
    q12.valid[:] = 0
    n, m12 = ORBmatcher(ctx).SearchBySim3(K1, K2, q12, q21, 7.5)
    assert n == 0 and (m12 == -1).all()


@pytest.mark.gpu
def test_gpu_projection_batch_of_three_with_an_empty_middle(ctx, oracle):
    """osg_search_by_projection_sim3_batch: 64-keypoint keyframes with 32 / 0 / 32 MapPoints; every problem equals
    its single call and the oracle, the middle one (nothing packed) keeps its slots."""
    import ctypes as C
    from orb_slam3_comments_ghr_amd import _abi
    worlds = [world(9250 + b, n=64, m=m) for b, m in enumerate((32, 0, 32))]
    fa = (_abi.OsgFrame * 3)(*[F.struct() for F, _, _ in worlds])
    qa = (_abi.OsgFuseQueries * 3)(*[Q.struct() for _, Q, _ in worlds])
    sq = np.concatenate([s for _, _, s in worlds])
    nm = np.full(3, -7, np.int32)
    ctx.check(ctx.lib.osg_search_by_projection_sim3_batch(ctx.handle, C.addressof(fa), C.addressof(qa), 3, 8.0, 1.5,
                                                          sq.ctypes.data, nm.ctypes.data), "Sim3 projection batch")
    for b, (F, Q, s0) in enumerate(worlds):
        n_ref, s_ref = oc.sim3(oracle, F, Q, 8, 1.5, s0)
        assert nm[b] == n_ref
        np.testing.assert_array_equal(sq[64 * b:64 * (b + 1)], s_ref)
        s1 = s0.copy()
        fs, qs = F.struct(), Q.struct()
        assert ctx.check(ctx.lib.osg_search_by_projection_sim3(ctx.handle, C.byref(fs), C.byref(qs), 8.0, 1.5,
                                                               s1.ctypes.data), "Sim3 projection") == n_ref
        np.testing.assert_array_equal(s1, s_ref)
    assert nm[0] > 0 and nm[1] == 0 and nm[2] > 0
