"""GPU: osg_two_view_reconstruct[_batch] (csrc/twoview.hip) against tests/pyref_twoview.py on the fixtures of
tests/twoview_fixtures.py.

The guard of the fixtures (checked on the CPU by tests/test_twoview.py) makes the discrete outcome well defined
against another SVD, so, per fixture, in a single call and in a batch:
  * identical: ok, model, both winning hypotheses (a set drawn in another order counts as the same one), the
    chosen motion hypothesis (paired by R, t), the inlier bytes, the triangulated flags and the set of
    triangulated points except at borderline matches, every nGood to within its borderline matches;
  * within 10 x the recorded spread of the fixture's group (profiles/twoview_margins.json): the
    per-hypothesis scores and models, H21 and F21 (up to scale and sign), R, t, the points, the parallaxes;
  * batch results equal to the single calls bit for bit, and a rerun equal bit for bit.
"""
import copy
import functools

import numpy as np
import pytest

from orb_slam3_comments_ghr_amd import OsgError
from orb_slam3_comments_ghr_amd import twoview as T
from orb_slam3_comments_ghr_amd.synth import EUROC_K
from tests import twoview_fixtures as FX

pytestmark = pytest.mark.gpu

BITWISE = ("H21", "F21", "R", "t", "n_good", "parallax", "cand_Rt", "p3d", "triangulated", "inlier_h", "inlier_f",
           "hyp_score_h", "hyp_score_f", "hyp_models")


@functools.lru_cache(maxsize=None)
def single(ctx, name):
    return T.TwoViewReconstruction(ctx, EUROC_K).solve(FX.build(name))


def compare(name, r):
    P, E, o = FX.replicas(name)[0]
    ref, got, tol = FX.reference(name), FX.view_gpu(r), FX.tolerances(name)
    print(name, "got", (r.ok, r.model, r.hyp_h, r.hyp_f, r.cand, list(r.n_good)), "want",
          (ref["ok"], ref["model"], ref["hyp_h"], ref["hyp_f"], ref["cand"], ref["n_good"]))
    if E is None:  # n < 8: nothing evaluated
        assert (r.ok, r.model, r.hyp_h, r.hyp_f, r.cand) == (False, -1, -1, -1, -1)
        assert not r.p3d.any() and not r.triangulated.any() and not r.hyp_score_h.any() and not r.hyp_score_f.any()
        return
    bad = FX.discrete_mismatches(P, ref, got, FX.borderline(E, o, tol))
    assert bad == []
    d = FX.continuous(ref, got, FX.exempt_hyps(name))
    print(name, {q: (v, tol[q]) for q, v in d.items()})
    for q, v in d.items():
        assert v <= tol[q], (q, v, tol[q])
    assert np.isfinite(r.hyp_score_h).all() and np.isfinite(r.hyp_score_f).all()
    # the returned models are those of the winning hypotheses; T21 is the chosen motion hypothesis
    if r.hyp_h >= 0:
        assert r.H21.tobytes() == r.hyp_models[r.hyp_h, 0].tobytes() and r.score_h == r.hyp_score_h[r.hyp_h]
    if r.hyp_f >= 0:
        assert r.F21.tobytes() == r.hyp_models[r.hyp_f, 1].tobytes() and r.score_f == r.hyp_score_f[r.hyp_f]
    if r.ok:
        assert np.concatenate([r.R.ravel(), r.t]).tobytes() == r.cand_Rt[r.cand].tobytes()
        assert not r.triangulated[P.matches12 < 0].any() and not r.p3d[P.matches12 < 0].any()
    else:
        assert not r.p3d.any() and not r.triangulated.any() and np.array_equal(r.R, np.eye(3, dtype=np.float32))


@pytest.mark.parametrize("name", list(FX.FIXTURES))
def test_single_call_matches_pyref(ctx, name):
    compare(name, single(ctx, name))


def test_duplicated_set_lower_slot_wins_and_models_are_bit_equal(ctx):
    P, r = FX.build("n100_dup"), single(ctx, "n100_dup")
    for hyp, m, sc in ((r.hyp_h, 0, r.hyp_score_h), (r.hyp_f, 1, r.hyp_score_f)):
        same = np.flatnonzero(np.all(P.sets == P.sets[hyp], 1))
        assert len(same) == 2 and hyp == same[0]
        assert r.hyp_models[same[0], m].tobytes() == r.hyp_models[same[1], m].tobytes() and sc[same[0]] == sc[same[1]]


def test_degenerate_set_does_not_poison_the_choice(ctx):
    r, ref = single(ctx, "n100_collinear"), FX.reference("n100_collinear")
    assert np.isfinite(r.hyp_score_h[0]) and np.isfinite(r.hyp_score_f[0])
    assert r.hyp_score_h[0] < 0.5 * r.score_h and r.hyp_score_f[0] < 0.5 * r.score_f
    assert (r.hyp_h, r.hyp_f) == (ref["hyp_h"], ref["hyp_f"]) and 0 not in (r.hyp_h, r.hyp_f)


def test_nan_models_score_zero_and_no_model_is_chosen(ctx):
    r = single(ctx, "n100_flat")
    assert (r.ok, r.model, r.hyp_h, r.hyp_f) == (False, -1, -1, -1) and r.score_h == 0 and r.score_f == 0
    assert not r.hyp_score_h.any() and not r.hyp_score_f.any() and not r.inlier_h.any() and not r.inlier_f.any()
    assert not r.H21.any() and not r.F21.any()


def test_fewer_than_eight_matches_evaluate_nothing(ctx):
    P = FX.build("n9")
    m = P.matches12.copy()
    m[P.idx1[7:]] = -1  # seven matches left
    Q = T.TwoViewProblem(P.keys1, P.keys2, m, np.zeros((5, 8), np.int32), K=P.K)
    assert Q.n == 7
    for r in (T.TwoViewReconstruction(ctx, EUROC_K).solve(Q), T.TwoViewReconstruction(ctx, EUROC_K).solve([FX.build("n64"), Q])[1]):
        assert (r.ok, r.model, r.hyp_h, r.hyp_f, r.cand, r.n_inliers) == (False, -1, -1, -1, -1, 0)
        assert not r.p3d.any() and not r.hyp_models.any() and not r.n_good.any()


def test_batch_matches_pyref_and_the_single_calls_and_repeats_bitwise(ctx):
    probs = [FX.build(k) for k in FX.BATCH]
    tv = T.TwoViewReconstruction(ctx, EUROC_K)
    first, second = tv.solve(probs), tv.solve(probs)
    for name, r, r2 in zip(FX.BATCH, first, second):
        compare(name, r)
        for q in (r2, single(ctx, name)):
            assert (r.ok, r.model, r.hyp_h, r.hyp_f, r.cand, r.n_inliers) == (q.ok, q.model, q.hyp_h, q.hyp_f, q.cand, q.n_inliers)
            assert (np.float32(r.score_h).tobytes(), np.float32(r.score_f).tobytes()) == (
                np.float32(q.score_h).tobytes(), np.float32(q.score_f).tobytes())
            for f in BITWISE:
                assert getattr(r, f).tobytes() == getattr(q, f).tobytes(), (name, f)


def test_class_interface(ctx):
    P = FX.build("n100_general")
    tv = T.TwoViewReconstruction(ctx, np.array([[P.K[0], 0, P.K[2]], [0, P.K[1], P.K[3]], [0, 0, 1]]), sigma=1.0, iterations=200)
    r = tv.reconstruct(P.keys1, P.keys2, P.matches12, P.sets)
    one = single(ctx, "n100_general")
    assert r.ok and r.p3d.tobytes() == one.p3d.tobytes() and r.R.tobytes() == one.R.tobytes()
    rb = tv.reconstruct_batch([(P.keys1, P.keys2, P.matches12, P.sets), (P.keys1, P.keys2, P.matches12)])
    assert rb[0].R.tobytes() == one.R.tobytes() and rb[1].hyp_score_f.shape == (200,)
    # without sets the class draws them itself: 200 sets from the seeded stream
    drawn = tv.problem(P.keys1, P.keys2, P.matches12)
    assert np.array_equal(drawn.sets, T.seeded_sets(P.n, 200)) and not np.array_equal(drawn.sets, P.sets)
    again = tv.solve(drawn)
    assert again.hyp_score_f.tobytes() == rb[1].hyp_score_f.tobytes() and again.R.tobytes() == rb[1].R.tobytes()


@pytest.mark.parametrize("bad", [(0, 1, 2, 3, 4, 5, 6, 6), (0, 1, 2, 3, 4, 5, 6, 65), (-1, 1, 2, 3, 4, 5, 6, 7),
                                 (3, 1, 2, 3, 4, 5, 6, 7), (0, 1, 2, 3, 4, 5, 6, 2**31 - 1)])
def test_bad_sets_are_an_error(ctx, bad):
    P = copy.copy(FX.build("n65"))
    P.sets = P.sets.copy()
    P.sets[17] = bad
    with pytest.raises(OsgError, match="set index"):
        T.TwoViewReconstruction(ctx, EUROC_K).solve(P)
    with pytest.raises(OsgError, match="set index"):
        T.TwoViewReconstruction(ctx, EUROC_K).solve([FX.build("n64"), P])


def test_bad_keypoint_indices_are_an_error(ctx):
    tv = T.TwoViewReconstruction(ctx, EUROC_K)
    P = copy.copy(FX.build("n65"))
    P.idx1 = P.idx1.copy()
    P.idx1[[3, 4]] = P.idx1[[4, 3]]  # not increasing
    with pytest.raises(OsgError, match="idx1 not strictly increasing"):
        tv.solve(P)
    P.idx1 = FX.build("n65").idx1.copy()
    P.idx1[5] = P.idx1[4]  # repeated: two matches would write one keypoint
    with pytest.raises(OsgError, match="idx1 not strictly increasing"):
        tv.solve([FX.build("n64"), P])
    P.idx1 = FX.build("n65").idx1.copy()
    P.idx1[-1] = len(P.keys1)
    with pytest.raises(OsgError, match="idx1 not strictly increasing"):
        tv.solve(P)
    P.idx1 = FX.build("n65").idx1
    for bad in (-1, len(P.keys2)):
        P.idx2 = FX.build("n65").idx2.copy()
        P.idx2[7] = bad
        with pytest.raises(OsgError, match="idx2 outside"):
            tv.solve(P)


def test_kernel_time_is_reported(ctx):
    T.TwoViewReconstruction(ctx, EUROC_K).solve(FX.build("n100_general"))
    ms = ctx.last_kernel_ms()
    assert ms > 0.0 and np.isfinite(ms)
