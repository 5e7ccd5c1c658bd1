"""GPU: osg_create_new_map_points[_batch] (csrc/newpoints.hip) against the sequential restatement
tests/pyref_newpoints.py on the fixtures of tests/newpoints_fixtures.py.

The guard of the fixtures (checked on the CPU by tests/test_newpoints.py) makes the discrete outcome well defined
against another null-vector solver, summation order and libm, so per fixture, in a single call:
  * identical: match, status, skipped and n_created, apart from borderline matches;
  * x3D within 10 x the spread of the fixture's group (profiles/newpoints_margins.json).
The match rows are also tied bit for bit to the matcher that oracle/oracle_triang.c pins: neighbour by neighbour, the
existing SearchForTriangulation with the MapPoint state updated from the GPU's own created flags gives them."""
import copy
import functools

import numpy as np
import pytest

from orb_slam3_comments_ghr_amd import OsgError, _abi
from orb_slam3_comments_ghr_amd import localmapping as L
from orb_slam3_comments_ghr_amd.matcher import ORBmatcher
from tests import newpoints_fixtures as FX
from tests import pyref_newpoints as R

pytestmark = pytest.mark.gpu
ARRAYS = ("match", "status", "x3d", "skipped", "n_created")


@functools.lru_cache(maxsize=None)
def single(ctx, name):
    out = L.CreateNewMapPoints(ctx).run(FX.build(name))
    print(name, "device ms (k_triang + k_np_eval + k_np_select)", ctx.last_kernel_ms())
    return out


@pytest.mark.parametrize("name", list(FX.FIXTURES))
def test_single_call_matches_pyref(ctx, name):
    got, ref = single(ctx, name), FX.reference(name)
    tol, bl = FX.tolerances(name), FX.borderline(name)
    diff = np.nonzero((got.match != ref.match) | (got.status != ref.status))
    print(name, "created", got.n_created.tolist(), "want", ref.n_created.tolist(), "skipped", got.skipped.tolist(),
          "borderline", sorted(bl), "differing (b, i)", list(zip(*map(np.ndarray.tolist, diff)))[:10])
    worst = max([FX.x3d_rel(FX.build(name), ref, b, i, got.x3d[b, i])
                 for b, i in zip(*np.nonzero(np.isin(ref.status & 0x7f, R.HAS_POINT) & (got.match == ref.match)))],
                default=0.0)
    print(name, "largest x3D difference", worst, "tolerance", tol["x3d"])
    assert FX.compare(name, got) == []
    assert got.total == int(got.n_created.sum())


def test_zero_distance_is_exact(ctx):
    """UnprojectStereo is float arithmetic in a fixed order: the GPU's point is the neighbour's stored centre too."""
    got, ref = single(ctx, "zero_dist"), FX.reference("zero_dist")
    (key,) = FX.exact_equality("zero_dist")
    assert got.status[key] == ref.status[key] == (_abi.NP_ZERO_DIST | _abi.NP_STEREO_BIT)
    assert got.x3d[key].tobytes() == FX.build("zero_dist").g2[0].Ow.tobytes()


def _non_coarse(name):
    """The KannalaBrandt8 fixtures with the epipolar test on (the restatement has none: GPU composition only)."""
    P = copy.copy(FX.build(name))
    P.coarse = False
    return P


@pytest.mark.parametrize("name", ["claim3", "one_query", "mono30", "stereo10", "kb8_4", "rig4", "kb8_4/epipolar",
                                  "rig4/epipolar"])
def test_match_rows_are_the_pinned_matchers(ctx, name):
    """Composition: for each neighbour in order the existing SearchForTriangulation (checkOri = False), with KF1's
    MapPoint state updated from the GPU's own created flags and the skipped neighbours left out, gives the match
    rows exactly."""
    if name.endswith("/epipolar"):
        P = _non_coarse(name.split("/")[0])
        got = L.CreateNewMapPoints(ctx).run(P)
    else:
        P, got = FX.build(name), single(ctx, name)
    m = ORBmatcher(ctx, 0.6, checkOri=False)
    K1 = copy.copy(P.kf1)
    K1.has_mp = P.kf1.has_mp.copy()
    for b in range(P.n_neigh):
        want = np.full(P.kf1.n, -1, np.int32)
        if not got.skipped[b]:
            _, pairs = m.SearchForTriangulation(K1, P.kf2[b], P.geom[b], False, P.coarse)
            want[pairs[:, 0]] = pairs[:, 1]
        assert np.array_equal(got.match[b], want), (name, b)
        K1.has_mp[(got.status[b] & 0x7f) == _abi.NP_CREATED] = 1
    assert got.n_created.sum() > 0


def test_batch_equals_single_calls_and_its_repeat(ctx):
    run = L.CreateNewMapPoints(ctx).run
    ps = [FX.build(k) for k in FX.BATCH]
    a, b = run(ps), run(ps)
    for name, x, y in zip(FX.BATCH, a, b):
        s = single(ctx, name)
        for arr in ARRAYS:
            assert getattr(x, arr).tobytes() == getattr(y, arr).tobytes(), (name, arr, "repeat")
            assert getattr(x, arr).tobytes() == getattr(s, arr).tobytes(), (name, arr, "single")
    assert [o.total for o in a] == [single(ctx, k).total for k in FX.BATCH]


def test_mixed_coarse_batch(ctx):
    """bCoarse is per problem: a batch that mixes both values gives each problem its own."""
    run = L.CreateNewMapPoints(ctx).run
    ps = [FX.build("kb8_4"), _non_coarse("kb8_4"), FX.build("claim3")]
    for got, want in zip(run(ps), [run(p) for p in ps]):
        for arr in ARRAYS:
            assert getattr(got, arr).tobytes() == getattr(want, arr).tobytes(), arr


def test_optional_outputs_may_be_null(ctx):
    full = single(ctx, "stereo10")
    for keep in ARRAYS:
        got = L.CreateNewMapPoints(ctx).run(FX.build("stereo10"), outputs=(keep,))
        assert got.total == full.total
        assert getattr(got, keep).tobytes() == getattr(full, keep).tobytes()
        assert all(getattr(got, a) is None for a in ARRAYS if a != keep)
    assert L.CreateNewMapPoints(ctx).run(FX.build("stereo10"), outputs=()).total == full.total


def test_rig_with_non_rig_is_unsupported(ctx):
    P = copy.copy(FX.build("rig4"))
    P.kf2 = list(P.kf2)
    P.kf2[2] = copy.copy(P.kf2[2])
    P.kf2[2].two_cam = 0
    with pytest.raises(OsgError) as e:
        L.CreateNewMapPoints(ctx).run(P)
    assert e.value.code == _abi.OSG_E_UNSUPPORTED


def test_too_many_neighbours_is_invalid(ctx):
    P = copy.copy(FX.build("claim3"))
    k = _abi.NEWPOINTS_MAX_NEIGHBOURS + 1
    P.kf2, P.g2, P.geom = [P.kf2[0]] * k, [P.g2[0]] * k, [P.geom[0]] * k
    with pytest.raises(OsgError) as e:
        L.CreateNewMapPoints(ctx).run(P)
    assert e.value.code == _abi.OSG_E_INVALID
