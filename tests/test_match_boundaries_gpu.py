"""match.hip's five operators on the boundary fixtures of tests/match_boundary_fixtures.py (tests/test_matcher_boundaries.py
proves on the CPU that each sits on its decisions), bit for bit against the oracle, on every path that holds a
copy of a decision, with the path read back from Context.match_last_path() / match_last_stats() and asserted:

* every mps / last / kf case as a single call at staging level 0, 1 and 2, with and without the k_grid_prepass
  (enum_grid at the three stagings, enum_grid_group; eval_query, eval_query_group).  Cases with slots taken
  before the call (mps taken / right_top2, last top, kf top) make the Jacobi rounds re-evaluate after the
  first evaluation on the initial slot state;
* the two-camera mps cases with the redo rider: staged, the speculative walk (eval_mps_lds); unstaged, the
  one-thread walk;
* every bow / bowkk case as a single call (eval_bow_group from k_bow_fill, k_bow_round and k_match).  SearchByBoW
  starts from an empty slot array, so there is no "taken before the call"; the cases' own claims (bow.taken,
  bowkk.matched2) make k_bow_round and k_match's rounds re-evaluate, which the round count shows;
* all cases of one operator and parameter set as one launch with an empty problem in the middle;
* the 64-query claim chains."""
import numpy as np
import pytest

from orb_slam3_comments_ghr_amd.matcher import ORBmatcher
from tests import match_boundary_fixtures as xb
from tests import matcher_boundary_fixtures as mb

pytestmark = pytest.mark.gpu

GRID = [c for c in xb.CASES if c.kind in ("mps", "last", "kf")]
BOW = [c for c in xb.CASES if c.kind in ("bow", "bowkk")]
MPS2 = [c for c in xb.of_kind("mps") if xb.two_cam(c)]


@pytest.fixture(scope="module")
def ref(oracle):
    """The oracle's answer for (case, mode), computed once."""
    made = {}

    def get(case, mode):
        if (case.id, mode) not in made:
            made[case.id, mode] = mb.run_oracle(oracle, case, mode)
        return made[case.id, mode]
    return get


def matcher(ctx, case, mode):
    a = case.args
    if case.kind == "mps":
        return ORBmatcher(ctx, a[4])
    if case.kind == "last":
        return ORBmatcher(ctx, 0.9, mode[1])
    return ORBmatcher(ctx, a[2] if case.kind in ("bow", "bowkk") else 0.75, mode)


def run_gpu(ctx, case, mode):
    a = case.args
    m = matcher(ctx, case, mode)
    if case.kind in ("bow", "bowkk"):
        return m.SearchByBoW(a[0], a[1], kf2=case.kind == "bowkk")
    s = a[2].copy()
    if case.kind == "mps":
        n = m.SearchByProjection(a[0], a[1], a[5], a[6], a[7], slot_mp=s, slot_taken=a[3])
    elif case.kind == "last":
        n = m.SearchByProjection(a[0], a[1], a[4], mode[0], slot_mp=s, slot_taken=a[3])
    else:
        n = m.SearchByProjection(a[0], a[1], a[3], a[4], slot_mp=s)
    return n, s


def run_gpu_batch(ctx, cases, mode):
    """The cases (one operator, one parameter set) as one launch: (count, slots) per problem."""
    c0 = cases[0]
    m = matcher(ctx, c0, mode)
    A, B = [c.args[0] for c in cases], [c.args[1] for c in cases]
    if c0.kind in ("bow", "bowkk"):
        nm, outs = m.SearchByBoWBatch(A, B, kf2=c0.kind == "bowkk")
        return [(int(n), o) for n, o in zip(nm, outs)]
    s = [c.args[2].copy() for c in cases]
    if c0.kind == "mps":
        nm = m.SearchByProjectionBatch(A, B, c0.args[5], c0.args[6], c0.args[7], slot_mps=s,
                                       slot_takens=[c.args[3] for c in cases])
    elif c0.kind == "last":
        nm = m.SearchByProjectionBatch(A, B, c0.args[4], mode[0], slot_mps=s, slot_takens=[c.args[3] for c in cases])
    else:
        nm = m.SearchByProjectionBatch(A, B, c0.args[3], c0.args[4], slot_mps=s)
    return [(int(n), x) for n, x in zip(nm, s)]


def check(got, want, what):
    np.testing.assert_array_equal(np.asarray(got[1]), np.asarray(want[1]), err_msg=f"{what}: slots")
    assert got[0] == want[0], f"{what}: nmatches {got[0]} != {want[0]}"


def resolve_bytes(n):
    return 12 * n + 2 * ((n + 15) // 16 * 16)


# ---- grid operators: one case, one call, every staging level, with and without the prepass

@pytest.mark.parametrize("prepass", ["0", "1"])
@pytest.mark.parametrize("cap", [0, 1, 2])
@pytest.mark.parametrize("case", GRID, ids=lambda c: c.id)
def test_grid_case_on_every_path(ctx, ref, monkeypatch, case, cap, prepass):
    monkeypatch.setenv("OSG_MATCH_STAGE", str(cap))
    monkeypatch.setenv("OSG_MATCH_PREPASS", prepass)
    for mode in mb.modes(case):
        got = run_gpu(ctx, case, mode)
        p = ctx.match_last_path()
        assert (p["stage"], p["prepass"], p["problems"]) == (cap, prepass == "1", 1), p
        assert (p["walk_lds"], p["walk_thread"]) == (0, 0) and not ctx.match_last_stats()["serial"], p
        check(got, ref(case, mode), f"{case.id} {mode} stage {cap} prepass {prepass}")


@pytest.mark.parametrize("case", GRID, ids=lambda c: c.id)
def test_prepass_first_evaluation_is_k_match_s_own(ctx, monkeypatch, case):
    """k_match's rounds re-evaluate every query with eval_query, so a wrong first evaluation by the prepass
    (eval_query_group) never reaches the slots: it shows only as a first round that changes results.  The
    round count with the prepass therefore has to be the one without it."""
    monkeypatch.delenv("OSG_MATCH_STAGE", raising=False)
    for mode in mb.modes(case):
        rounds = []
        for prepass in ("0", "1"):
            monkeypatch.setenv("OSG_MATCH_PREPASS", prepass)
            run_gpu(ctx, case, mode)
            assert ctx.match_last_path()["prepass"] == (prepass == "1")
            rounds.append(ctx.match_last_stats()["rounds"])
        assert rounds[0] == rounds[1] >= 1, f"{case.id} {mode}: rounds without / with the prepass {rounds}"


# ---- the two-camera a5 redo: both serial walks on the cases' decisions

@pytest.mark.parametrize("prepass", ["0", "1"])
@pytest.mark.parametrize("cap,walk", [(2, "lds"), (1, "lds"), (0, "thread")])
@pytest.mark.parametrize("case", MPS2, ids=lambda c: c.id)
def test_two_camera_mps_case_on_the_serial_walks(ctx, ref, monkeypatch, case, cap, walk, prepass):
    monkeypatch.setenv("OSG_MATCH_STAGE", str(cap))
    monkeypatch.setenv("OSG_MATCH_PREPASS", prepass)
    ridden = xb.redo_rider(case)
    got = run_gpu(ctx, ridden, None)
    p = ctx.match_last_path()
    assert ctx.match_last_stats()["serial"], p
    assert (p["stage"], p["walk_lds"], p["walk_thread"]) == (cap, int(walk == "lds"), int(walk == "thread")), p
    check(got, ref(ridden, None), f"{ridden.id} stage {cap} prepass {prepass}")


# ---- SearchByBoW: one case, one call

@pytest.mark.parametrize("case", BOW, ids=lambda c: c.id)
def test_bow_case(ctx, ref, case):
    for mode in mb.modes(case):
        got = run_gpu(ctx, case, mode)
        p = ctx.match_last_path()
        assert (p["stage"], p["prepass"], p["problems"]) == (0, False, 1), p
        assert p["lds_bytes"] == resolve_bytes(case.args[1].n)
        check(got, ref(case, mode), f"{case.id} {mode}")
        if case.name in ("one_cam", "two_cam"):
            # a query finds its first choice claimed by an earlier one: k_bow_round changes a result and
            # k_match's rounds run (and end on a round that changes nothing)
            assert ctx.match_last_stats()["rounds"] >= 2


# ---- all cases of one operator in one launch

def groups(kind):
    """The cases of one operator by the scalar parameters a launch shares."""
    out = {}
    for c in xb.of_kind(kind):
        out.setdefault(tuple(x for x in c.args if isinstance(x, (bool, int, float))), []).append(c)
    return sorted(out.items())


BATCHES = [(kind, key, mode) for kind in xb.KINDS for key, cases in groups(kind) for mode in mb.modes(cases[0])]


@pytest.mark.parametrize("kind,key,mode", BATCHES, ids=lambda v: str(v).replace(" ", ""))
def test_batch_equals_single_calls_and_oracle(ctx, ref, monkeypatch, kind, key, mode):
    monkeypatch.delenv("OSG_MATCH_STAGE", raising=False)
    monkeypatch.delenv("OSG_MATCH_PREPASS", raising=False)
    cases = dict(groups(kind))[key]
    if len(cases) == 1:
        cases = cases * 2
    mid = len(cases) // 2
    cases = cases[:mid] + [xb.without_queries(cases[mid])] + cases[mid:]
    singles = [run_gpu(ctx, c, mode) for c in cases]
    got = run_gpu_batch(ctx, cases, mode)
    p = ctx.match_last_path()
    grid = kind in ("mps", "last", "kf")
    assert (p["stage"], p["prepass"], p["problems"]) == (2 if grid else 0, grid, len(cases)), p
    for c, g, s in zip(cases, got, singles):
        check(g, ref(c, mode), f"{c.id} {mode} in the batch")
        check(g, s, f"{c.id} {mode}: batch against the single call")
    n, s = got[mid]
    assert n == 0, "the empty problem matches nothing"
    if grid:
        np.testing.assert_array_equal(s, cases[mid].args[2], err_msg="and leaves its slots alone")
    else:
        assert (np.asarray(s) == -1).all()


# ---- claim chains

# (SearchByBoW has no grid prepass)
CHAINS = [(kind, prepass) for kind in xb.KINDS for prepass in ("0", "1") if prepass == "0" or kind in ("mps", "last", "kf")]


@pytest.mark.parametrize("kind,prepass", CHAINS)
def test_claim_chain_takes_a_round_per_query(ctx, ref, monkeypatch, kind, prepass):
    """xb.chain: 64 queries, each displaced by the one before it (tests/test_matcher_boundaries.py shows that
    the fixed point needs a round per query)."""
    n = 64
    monkeypatch.setenv("OSG_MATCH_PREPASS", prepass)
    monkeypatch.delenv("OSG_MATCH_STAGE", raising=False)
    case = xb.chain(kind, n)
    for mode in mb.modes(case):
        want = ref(case, mode)
        assert want[0] == n
        got = run_gpu(ctx, case, mode)
        check(got, want, f"{kind} chain {mode}")
        assert ctx.match_last_stats()["rounds"] >= n
        assert ctx.match_last_path()["prepass"] == (prepass == "1")
