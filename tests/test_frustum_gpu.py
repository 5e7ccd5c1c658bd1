"""GPU: osg_frustum[_batch] (csrc/frustum.hip) and osg_search_local_points[_batch] against the float32 restatement
tests/pyref_frustum.py on the fixtures of tests/frustum_fixtures.py (whose guards tests/test_frustum.py checks on
the CPU).

  * pinhole mono and stereo: status, level, n_to_match and the bit patterns of proj_x / y / xr, view_cos and depth
    equal the restatement's, the -1 and partial writes of the Nleft == -1 path included;
  * the KannalaBrandt8 rig: status, levels and n_to_match equal, the floats within 10 x the recorded spreads;
  * replaying the documented writes of each status byte gives the restatement's MapPoints;
  * a batch equals its single calls, the fused call equals frustum -> host -> osg_search_by_projection_mps, both bit
    for bit; n_to_match == 0 leaves slot_mp alone; a rerun is identical."""
import functools

import numpy as np
import pytest

from orb_slam3_comments_ghr_amd import tracking as T
from orb_slam3_comments_ghr_amd.matcher import ORBmatcher
from tests import frustum_fixtures as FX
from tests import pyref_frustum as PF

pytestmark = pytest.mark.gpu
SINGLE = [n for n in FX.FIXTURES]


@functools.lru_cache(maxsize=None)
def single(ctx, name):
    frame, pts = FX.build(name)
    out = T.frustum(ctx, frame, pts)
    print(name, "k_frustum device ms", ctx.last_kernel_ms())
    return out


@pytest.mark.parametrize("name", SINGLE)
def test_single_call_matches_pyref(ctx, name):
    got = single(ctx, name)
    want = FX.expected(name)
    print(name, "n_to_match", got.n_to_match, "want", want.n_to_match, "statuses",
          [np.bincount(s, minlength=6).tolist() for s in got.status])
    assert FX.compare(name, got) == []


@pytest.mark.parametrize("name", SINGLE)
def test_replayed_writes_give_the_reference_mappoints(ctx, name):
    """the status bytes tell the caller which writes the reference made, stale fields included"""
    frame, pts = FX.build(name)
    got, ref = single(ctx, name), FX.reference(name)
    mp, proj = PF.replay(frame, pts, got)
    exact = FX.group(name) == "pinhole"
    tol = None if exact else FX.tolerances(name)
    for f in PF.MapPoints.FIELDS:
        a, b = getattr(mp, f), getattr(ref.mp, f)
        if a.dtype == np.float32 and not exact:
            kind = "uv" if f.startswith("proj") else "cos" if f.startswith("view") else "depth"
            assert np.all(np.abs(a.astype(np.float64) - b) <= tol[kind]), f
        elif a.dtype == np.float32:
            assert np.array_equal(FX.bits(a), FX.bits(b)), f
        else:
            assert np.array_equal(a, b), f
    assert sorted(proj) == sorted(ref.project_points)


def test_hand_made_points(ctx):
    got = single(ctx, "hand")
    assert tuple(got.status[0]) == FX.HAND_STATUS
    assert (got.proj_x[0, 0], got.proj_y[0, 0]) == (0.0, 480.0)
    assert got.view_cos[0, 3] == np.float32(0.5)
    assert (got.proj_x[0, 4], got.proj_y[0, 4]) == (-1.0, -1.0)  # u = +inf: rejected before :713


@pytest.mark.parametrize("batch", list(FX.BATCHES))
def test_batch_equals_singles(ctx, batch):
    names = FX.BATCHES[batch]
    frames, pts = zip(*[FX.build(n) for n in names])
    outs = T.frustum_batch(ctx, list(frames), list(pts))
    for n, o in zip(names, outs):
        assert FX.same_bits(o, single(ctx, n)) == [], n
        assert FX.compare(n, o) == [], n


def test_rerun_is_identical(ctx):
    for name in ("ps_n257", "kr_n257"):
        frame, pts = FX.build(name)
        assert FX.same_bits(T.frustum(ctx, frame, pts), single(ctx, name)) == []


def two_step(ctx, c):
    out = T.frustum(ctx, c.frame, c.points)
    slot = c.slot_mp.copy()
    n = 0
    if out.n_to_match > 0:  # ref:src/Tracking.cc:4154
        n = ORBmatcher(ctx, 0.8).SearchByProjection(c.F, T.mp_queries(c.points, out), c.th, c.far_points, c.th_far,
                                                    slot_mp=slot, slot_taken=c.slot_taken)
    return n, slot, out


def fused(ctx, c):
    slot = c.slot_mp.copy()
    n, out = T.search_local_points(ctx, c.F, c.frame, c.points, th=c.th, nnratio=0.8, far_points=c.far_points,
                                   th_far_points=c.th_far, slot_mp=slot, slot_taken=c.slot_taken)
    return n, slot, out


@pytest.mark.parametrize("name", FX.FUSED)
def test_fused_equals_two_step(ctx, name):
    c = FX.build_fused(name)
    n2, slot2, out2 = two_step(ctx, c)
    n1, slot1, out1 = fused(ctx, c)
    print(name, "n_to_match", out1.n_to_match, "nmatches fused", n1, "two-step", n2, "keypoints", c.F.n)
    assert n2 > 0 and (slot2 != c.slot_mp).any()  # the fixture matches something
    assert FX.same_bits(out1, out2) == []
    assert n1 == n2 and np.array_equal(slot1, slot2)
    assert FX.compare(name, out1) == []


def test_fused_batch_equals_singles(ctx):
    cs = [FX.build_fused(n) for n in FX.FUSED]
    slots = [c.slot_mp.copy() for c in cs]
    nm, outs = T.search_local_points_batch(ctx, [c.F for c in cs], [c.frame for c in cs], [c.points for c in cs],
                                           th=1.0, slot_mps=slots, slot_takens=[c.slot_taken for c in cs])
    for b, c in enumerate(cs):
        slot = c.slot_mp.copy()
        n, out = T.search_local_points(ctx, c.F, c.frame, c.points, th=1.0, slot_mp=slot, slot_taken=c.slot_taken)
        assert n == nm[b] and np.array_equal(slot, slots[b]) and FX.same_bits(out, outs[b]) == [], b


def test_nothing_to_match_leaves_slots_alone(ctx):
    frame, pts = FX.build("none")
    c = FX.build_fused("fused_pm")
    n = pts.n
    rng = np.random.default_rng(5)
    pts.mp_id, pts.has_obs = np.arange(n, dtype=np.int32), np.ones(n, np.uint8)
    pts.desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    slot = c.slot_mp.copy()
    nm, out = T.search_local_points(ctx, c.F, frame, pts, th=15.0, slot_mp=slot, slot_taken=c.slot_taken)
    assert out.n_to_match == 0 and nm == 0 and np.array_equal(slot, c.slot_mp)
    assert FX.compare("none", out) == []


def test_fused_batch_of_three_with_an_empty_middle(ctx):
    """a one-camera and a two-camera problem around one without local points (no query array reserved or bound):
    every problem equals its single call and the reference, the middle one keeps its slots"""
    names = ("fused_ps", "kr_n0", "fused_kr")
    cs = [FX.build_fused(n) for n in names]
    assert [c.points.n > 0 for c in cs] == [True, False, True]
    slots = [c.slot_mp.copy() for c in cs]
    nm, outs = T.search_local_points_batch(ctx, [c.F for c in cs], [c.frame for c in cs], [c.points for c in cs],
                                           th=1.0, slot_mps=slots, slot_takens=[c.slot_taken for c in cs])
    for b, (name, c) in enumerate(zip(names, cs)):
        slot = c.slot_mp.copy()
        n, out = T.search_local_points(ctx, c.F, c.frame, c.points, th=1.0, slot_mp=slot, slot_taken=c.slot_taken)
        assert n == nm[b] and np.array_equal(slot, slots[b]) and FX.same_bits(out, outs[b]) == [], b
        assert FX.compare(name, outs[b]) == []
    assert nm[0] > 0 and nm[2] > 0 and nm[1] == 0 and np.array_equal(slots[1], cs[1].slot_mp)
