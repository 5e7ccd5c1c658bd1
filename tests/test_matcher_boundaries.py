"""The boundary fixtures of tests/matcher_boundary_fixtures.py on the CPU: the Python restatement equals the C
oracle on every case, and for every named decision ("Matcher decisions") the restatement with that
one decision flipped leaves the oracle on every case that claims to sit on it."""
import pytest

from tests import match_boundary_fixtures as xb
from tests import matcher_boundary_fixtures as mb
from tests import pyref_match as pr

CASES = mb.CASES + xb.CASES

# Literal on purpose: a decision that loses its flip or its fixture shows up here in review.
DECISIONS = (
    "area.window", "area.order", "area.clamp",
    "fuse.level", "fuse.level:narrow", "fuse.chi2_mono", "fuse.chi2_stereo", "fuse.chi2_stereo:kpr", "fuse.tie",
    "fuse.accept", "fuse.right_index",
    "sim3.accept", "sim3.accept:double", "sim3.taken", "sim3.taken:never", "sim3.tie", "sim3.level",
    "sim3.level:narrow",
    "bysim3.accept", "bysim3.mutual",
    "tri.tie", "tri.accept", "tri.epipole", "tri.epipole:always", "tri.epipolar", "tri.filters", "tri.filters:mp1",
    "tri.filters:stereo1", "tri.filters:stereo2", "tri.filters:coarse",
    "rot.round", "rot.round:wrap", "maxima.order", "maxima.tenth",
    "init.level0", "init.level0:f2", "init.md", "init.top2", "init.accept", "init.accept:ratio", "init.steal_hist",
    "mps.far", "mps.bad", "mps.radius", "mps.level", "mps.level:narrow", "mps.taken", "mps.taken:never", "mps.stereo",
    "mps.stereo:kpr", "mps.tie", "mps.top2", "mps.accept", "mps.ratio", "mps.ratio:level", "mps.ratio:double",
    "mps.skip_right", "mps.partner", "mps.partner:r2l", "mps.own", "mps.own:never", "mps.level_r", "mps.radius_r",
    "last.invz", "last.bounds", "last.forward", "last.backward", "last.mono", "last.level", "last.level:narrow",
    "last.level:fwd", "last.level:fwd_narrow", "last.level:bwd", "last.level:bwd_narrow", "last.taken",
    "last.taken:never", "last.stereo", "last.stereo:kpr", "last.tie", "last.accept", "last.empty_left",
    "last.hist_right", "last.hist_stale",
    "kf.level", "kf.level:narrow", "kf.taken", "kf.tie", "kf.accept", "kf.accept:high",
    "bow.good", "bow.taken", "bow.tie", "bow.top2", "bow.accept", "bow.ratio", "bow.ratio:double", "bow.side",
    "bow.right_gate", "bow.right_gate:ratio", "bow.right_ratio", "bow.nodes",
    "bowkk.accept", "bowkk.ratio", "bowkk.ratio:double", "bowkk.matched2", "bowkk.mp2", "bowkk.mp2:bad", "bowkk.right",
    "bowkk.right:k2", "bowkk.tie", "bowkk.top2",
)
# where each shared decision has to be pinned: the area walk under every matcher that walks it, the histogram
# under every matcher that keeps one
KINDS = {"area": ("fuse", "sim3", "bysim3", "mps", "last", "kf"), "rot": ("tri", "init", "last", "kf", "bow", "bowkk"),
         "maxima": ("tri", "init", "last", "kf", "bow", "bowkk")}


def test_every_flip_is_listed():
    assert set(DECISIONS) == set(pr.FLIPS) and len(DECISIONS) == len(set(DECISIONS))
    assert {f for c in CASES for f in c.flips} == set(DECISIONS)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_python_equals_oracle(oracle, case):
    assert mb.size(case) <= 64
    for mode in mb.modes(case):
        ref, got = mb.run_oracle(oracle, case, mode), mb.run_pyref(case, mode)
        assert mb.same(ref, got), (mode, ref, got)


@pytest.mark.parametrize("name", DECISIONS)
def test_flip_leaves_the_oracle(oracle, name):
    cases = [c for c in CASES if name in c.flips]
    family = name.split(".")[0]
    assert {c.kind for c in cases} == set(KINDS.get(family, (family,)))
    for case in cases:
        differs = [mode for mode in mb.modes(case)
                   if not mb.same(mb.run_oracle(oracle, case, mode), mb.run_pyref(case, mode, flip=name))]
        assert differs, f"{case.id}: flip {name} ({pr.FLIPS[name]}) gives the oracle's result in every mode"


def test_the_pile_up_leaves_a_case_its_decisions(oracle):
    """pile_up adds histogram entries of its own; the cases still equal the oracle with it (the GPU test runs
    them through k_init's serial walk this way)."""
    for case in mb.of_kind("init"):
        piled = mb.pile_up(case)
        assert mb.same(mb.run_oracle(oracle, piled, None), mb.run_pyref(piled, None))


def test_the_redo_rider_leaves_a_case_its_decisions(oracle):
    """redo_rider adds a keypoint pair and a query of its own, far from the case's; the two-camera mps cases
    still equal the oracle with it and still sit on their decisions (the GPU test runs them through both
    serial walks of k_match this way)."""
    cases = [c for c in xb.of_kind("mps") if xb.two_cam(c)]
    assert len(cases) >= 5
    for case in cases:
        ridden = xb.redo_rider(case)
        assert mb.size(ridden) <= 64
        ref = mb.run_oracle(oracle, ridden, None)
        assert mb.same(ref, mb.run_pyref(ridden, None))
        F = ridden.args[0]
        assert ref[1][F.nleft - 1] == ridden.args[1].mp_id[-1] == ref[1][F.n - 1]  # the rider matched, partner included
        for name in case.flips:
            assert not mb.same(ref, mb.run_pyref(ridden, None, flip=name)), (case.id, name)


@pytest.mark.parametrize("kind", xb.KINDS)
def test_the_claim_chain_displaces_every_query(oracle, kind):
    """xb.chain: the sequential result is query q in slot q, and the fixed point started from every query's
    unclaimed best needs one round per query: iterated as k_match does (each query against the claims of the
    earlier queries in the previous round), round r leaves exactly the queries from r on displaced."""
    n = 64
    case = xb.chain(kind, n)
    assert mb.size(case) == n
    for mode in mb.modes(case):
        nm, slots = mb.run_oracle(oracle, case, mode)
        assert mb.same((nm, slots), mb.run_pyref(case, mode))
        want = case.args[0].mp_id if kind == "bow" else case.args[1].mp_id
        assert nm == n and slots.tolist() == list(want)
    # every query's candidates (SearchByBoW: the whole node; a grid operator: its window of radius 4) in order
    # of distance: slot q - 1, then slot q; query 0 has slot 0 first
    if kind in ("bow", "bowkk"):
        qd, sd = case.args[0].desc, case.args[1].desc
        cands = [list(range(n))] * n
    else:
        F, Q = case.args[0], case.args[1]
        qd, sd = Q.desc, F.desc
        xs = Q.proj_x if kind == "mps" else Q.u
        cands = [pr.features_in_area(F, xs[q], 100.0, 4.0) for q in range(n)]
        assert cands == [[0]] + [[q - 1, q] for q in range(1, n)]
    order = [sorted(cands[q], key=lambda s: pr.dist(qd[q], sd[s])) for q in range(n)]
    assert all(order[q][:2] == [q - 1, q] for q in range(1, n)) and order[0][0] == 0
    best = [o[0] for o in order]
    rounds = 0
    while True:
        claim = {}
        for q, s in enumerate(best):
            claim[s] = min(claim.get(s, q), q)
        new = [s + 1 if claim[s] < q and s == q - 1 else s for q, s in enumerate(best)]
        if new == best:
            break
        best, rounds = new, rounds + 1
    assert best == list(range(n)) and rounds == n - 1
