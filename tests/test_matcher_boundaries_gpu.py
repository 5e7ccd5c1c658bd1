"""fuse.hip, sim3.hip, triang.hip's k_triang and init.hip on the boundary fixtures (tests/matcher_boundary_fixtures.py;
tests/test_matcher_boundaries.py proves on the CPU that each sits on a decision): every case through the C ABI
equals the oracle bit for bit, as a single call and in one batch per matcher; then the claim chains and the
capacity edges of k_sim3 and k_init."""
import ctypes as C

import numpy as np
import pytest

from orb_slam3_comments_ghr_amd import _abi
from orb_slam3_comments_ghr_amd.matcher import ORBmatcher
from tests import matcher_boundary_fixtures as mb
from tests import oracle_calls as oc

pytestmark = pytest.mark.gpu


def check(got, ref, what):
    assert len(got) == len(ref)
    for k, (g, r) in enumerate(zip(got, ref)):
        np.testing.assert_array_equal(np.asarray(g), np.asarray(r), err_msg=f"{what}: output {k}")


# ---- one case, one call

def sim3_call(ctx, F, Q, ratio, slots):
    s = np.ascontiguousarray(slots, np.int32).copy()
    fs, qs = F.struct(), Q.struct()
    rc = ctx.lib.osg_search_by_projection_sim3(ctx.handle, C.byref(fs), C.byref(qs), mb.TH, float(ratio), s.ctypes.data)
    return rc, s


def init_call(ctx, F1, F2, prev):
    p = np.ascontiguousarray(prev, np.float32).copy()
    m12 = np.full(F1.n, -1, np.int32)
    a, b = F1.struct(), F2.struct()
    rc = ctx.lib.osg_search_for_initialization(ctx.handle, C.byref(a), C.byref(b), p.ctypes.data, mb.WINDOW, mb.NNRATIO,
                                               1, m12.ctypes.data)
    return rc, m12, p


def run_gpu(ctx, case, mode):
    a = case.args
    m = ORBmatcher(ctx, nnratio=mb.NNRATIO, checkOri=True)
    if case.kind == "fuse":
        return m.Fuse(a[0], a[1], mb.TH, bRight=mode[0], sim3=not mode[1])
    if case.kind == "sim3":
        rc, s = sim3_call(ctx, a[0], a[1], mode, a[2])
        return ctx.check(rc, "Sim3 projection"), s
    if case.kind == "bysim3":
        return m.SearchBySim3(*a, mb.TH)
    if case.kind == "tri":
        return m.SearchForTriangulation(*a, bOnlyStereo=mode[0], bCoarse=mode[1])
    rc, m12, p = init_call(ctx, *a)
    return ctx.check(rc, "SearchForInitialization"), m12, p


@pytest.mark.parametrize("case", mb.CASES, ids=lambda c: c.id)
def test_single_call_equals_oracle(ctx, oracle, case):
    for mode in mb.modes(case):
        check(run_gpu(ctx, case, mode), mb.run_oracle(oracle, case, mode), f"{case.id} {mode}")
    if case.kind == "init":
        assert not ctx.match_last_stats()["serial"]  # the fixed point decided it


# ---- all of one matcher's cases in one launch

@pytest.mark.parametrize("right,gated", mb.FUSE_MODES)
def test_fuse_batch_equals_oracle(ctx, oracle, right, gated):
    cases = [c for c in mb.of_kind("fuse") if (right, gated) in mb.modes(c)]
    assert len(cases) >= 2
    nf, bis, bds = ORBmatcher(ctx).FuseBatch([c.args[0] for c in cases], [c.args[1] for c in cases], mb.TH,
                                             bRight=right, sim3=not gated)
    for c, n, bi, bd in zip(cases, nf, bis, bds):
        check((n, bi, bd), mb.run_oracle(oracle, c, (right, gated)), c.id)


@pytest.mark.parametrize("ratio", mb.SIM3_MODES)
def test_sim3_batch_equals_oracle(ctx, oracle, ratio):
    cases = mb.of_kind("sim3")
    B = len(cases)
    fa = (_abi.OsgFrame * B)(*[c.args[0].struct() for c in cases])
    qa = (_abi.OsgFuseQueries * B)(*[c.args[1].struct() for c in cases])
    sq = np.concatenate([c.args[2] for c in cases]).astype(np.int32)
    nm = np.full(B, -7, np.int32)
    ctx.check(ctx.lib.osg_search_by_projection_sim3_batch(ctx.handle, C.addressof(fa), C.addressof(qa), B, mb.TH,
                                                          float(ratio), sq.ctypes.data, nm.ctypes.data), "Sim3 batch")
    cuts = np.cumsum([0] + [c.args[0].n for c in cases])
    for b, c in enumerate(cases):
        check((nm[b], sq[cuts[b]:cuts[b + 1]]), mb.run_oracle(oracle, c, ratio), c.id)


@pytest.mark.parametrize("only_stereo,coarse", mb.TRI_MODES)
def test_triangulation_batch_equals_oracle(ctx, oracle, only_stereo, coarse):
    cases = mb.of_kind("tri")
    nm, pairs = ORBmatcher(ctx, checkOri=True).SearchForTriangulationBatch(
        [c.args[0] for c in cases], [c.args[1] for c in cases], [c.args[2] for c in cases], only_stereo, coarse)
    for c, n, p in zip(cases, nm, pairs):
        check((n, p), mb.run_oracle(oracle, c, (only_stereo, coarse)), c.id)


def init_batch(ctx, cases):
    B = len(cases)
    fa = (_abi.OsgFrame * B)(*[c.args[0].struct() for c in cases])
    fb = (_abi.OsgFrame * B)(*[c.args[1].struct() for c in cases])
    prev = np.ascontiguousarray(np.concatenate([c.args[2] for c in cases]), np.float32)
    m12 = np.full(len(prev), -9, np.int32)
    nm = np.full(B, -7, np.int32)
    ctx.check(ctx.lib.osg_search_for_initialization_batch(ctx.handle, C.addressof(fa), C.addressof(fb), B,
                                                          prev.ctypes.data, mb.WINDOW, mb.NNRATIO, 1, m12.ctypes.data,
                                                          nm.ctypes.data), "SearchForInitialization batch")
    cuts = np.cumsum([0] + [c.args[0].n for c in cases])
    return [(nm[b], m12[cuts[b]:cuts[b + 1]], prev[cuts[b]:cuts[b + 1]]) for b in range(B)]


def test_initialization_batch_equals_oracle(ctx, oracle):
    cases = mb.of_kind("init")
    for c, got in zip(cases, init_batch(ctx, cases)):
        check(got, mb.run_oracle(oracle, c, None), c.id)
    assert not ctx.match_last_stats()["serial"]


def test_initialization_cases_on_the_serial_walk(ctx, oracle):
    """Every initialisation case again with a five-claimant pile-up far from its keypoints: the claim list of
    that F2 keypoint overflows and the whole problem is redone by k_init's one-wave sequential walk."""
    piled = [mb.pile_up(c) for c in mb.of_kind("init")]
    for c in piled:
        rc, m12, p = init_call(ctx, *c.args)
        check((ctx.check(rc, c.id), m12, p), mb.run_oracle(oracle, c, None), c.id)
        assert ctx.match_last_stats()["serial"], c.id
    for c, got in zip(piled, init_batch(ctx, piled)):
        check(got, mb.run_oracle(oracle, c, None), c.id + " batch")


# ---- claim chains

def test_sim3_claim_chain_across_the_lane_stride(ctx, oracle):
    L = 40
    F, Q, slots, at = mb.sim3_chain(L)
    assert at[:5] == [0, 1023, 1024, 2047, 2048] and int(Q.valid.sum()) == L
    ref = oc.sim3(oracle, F, Q, mb.TH, 1.0, slots)
    assert ref[0] == L and ref[1].tolist() == at  # MapPoint i ends in slot i
    rc, s = sim3_call(ctx, F, Q, 1.0, slots)
    check((ctx.check(rc, "chain"), s), ref, "chain")
    assert ctx.match_last_stats()["rounds"] >= L


@pytest.mark.parametrize("k,serial", [(4, False), (5, True)])
def test_init_claim_list_at_its_capacity(ctx, oracle, k, serial):
    """FP_K = 4 claimants of one F2 keypoint in one round fit k_init's claim list; the fifth overflows it."""
    F1, F2, prev = mb.init_claimants(k)
    ref = oc.initialization(oracle, F1, F2, prev, mb.WINDOW, mb.NNRATIO, True)
    assert ref[1].tolist() == [-1] * (k - 1) + [0]  # each stole from the one before
    rc, m12, p = init_call(ctx, F1, F2, prev)
    check((ctx.check(rc, "claimants"), m12, p), ref, f"{k} claimants")
    assert ctx.match_last_stats()["serial"] == serial


# ---- capacity edges

def test_sim3_keyframe_of_8192_keypoints(ctx, oracle):
    F = mb.lattice_frame(8192, 128, level=3)
    Q = mb.lattice_queries(F, lvl=4)
    slots = np.full(F.n, -1, np.int32)
    slots[::3] = -2
    ref = oc.sim3(oracle, F, Q, mb.TH, 1.0, slots)
    assert 0 < ref[0] and ref[1][F.n - 1] >= 0  # a match in the last entry of the claim table
    rc, s = sim3_call(ctx, F, Q, 1.0, slots)
    check((ctx.check(rc, "8192 keypoints"), s), ref, "8192 keypoints")


def test_sim3_keyframe_of_8193_keypoints_is_refused(ctx):
    F = mb.lattice_frame(8193, 128, level=3)
    Q = mb.lattice_queries(F, lvl=4)
    slots = np.full(F.n, -1, np.int32)
    slots[::3] = -2
    rc, s = sim3_call(ctx, F, Q, 1.0, slots)
    assert rc == _abi.OSG_E_INVALID
    np.testing.assert_array_equal(s, slots)


@pytest.mark.parametrize("n2,serial", [(4096, False), (4097, True)])
def test_init_level0_keypoints_at_the_claim_table_size(ctx, oracle, n2, serial):
    F1, F2, prev = mb.lattice_init_pair(n2)
    ref = oc.initialization(oracle, F1, F2, prev, mb.WINDOW, mb.NNRATIO, True)
    assert ref[0] > 0
    rc, m12, p = init_call(ctx, F1, F2, prev)
    check((ctx.check(rc, "lattice"), m12, p), ref, f"{n2} level-0 F2 keypoints")
    assert ctx.match_last_stats()["serial"] == serial


def test_init_8193_level0_keypoints_are_refused(ctx):
    F1, F2, prev = mb.lattice_init_pair(8193)
    rc, m12, p = init_call(ctx, F1, F2, prev)
    assert rc == _abi.OSG_E_INVALID
    assert (m12 == -1).all()
    np.testing.assert_array_equal(p, prev)
