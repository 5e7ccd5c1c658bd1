"""GPU: osg_kfdb_* (csrc/kfdb.hip) and orb_slam3_comments_ghr_amd.keyframedb against the literal restatement
tests/pyref_kfdb.py.  Every comparison is exact: integers, and the bit patterns of the float and double scores.

  * every fixture of tests/kfdb_fixtures.py through the Python class (candidates, n_sharing, max / min common
    words, the scored list in order with float and double bits, all six fields of every KeyFrame after each
    query) and through the raw C ABI (the same without the candidates, the fields as the state arrays);
  * random sessions of 300 KeyFrames;
  * the shapes at which a kernel can go wrong: an empty database, one entry of one word, a query of one word,
    entries of 63 / 64 / 65 words, a query and an entry of 5 000 words (past the 4 096 words staged on chip)
    with word ids up to 999 999 in a vocabulary of more than 10^6 words, 1 / 64 / 65 / 300 entries, and a
    database after the erase of its first, a middle and its last entry and after clear_map;
  * a sequence run twice gives the same bits;
  * ORBVocabulary.transform -> add -> query against tests/pyref_bow.py -> tests/pyref_kfdb.py;
  * what the host refuses.
"""
import ctypes as C

import numpy as np
import pytest

from orb_slam3_comments_ghr_amd import OsgError, _abi
from orb_slam3_comments_ghr_amd import keyframedb as K
from orb_slam3_comments_ghr_amd import vocabulary as vb
from tests import kfdb_fixtures as FX
from tests import pyref_bow as pb

pytestmark = pytest.mark.gpu


full_vocabulary = K.complete_vocabulary


@pytest.fixture(scope="module")
def voc(ctx):
    v = vb.ORBVocabulary(ctx, full_vocabulary(10, 3))
    assert v.info()["n_words"] == FX.N_WORDS
    yield v
    v.close()


@pytest.fixture(scope="module")
def voc_big(ctx):
    v = vb.ORBVocabulary(ctx, full_vocabulary(32, 4))
    assert v.info()["n_words"] == 32 ** 4 >= 10 ** 6
    yield v
    v.close()


def check(ctx, voc, S, want=None):
    db = K.KeyFrameDatabase(ctx, voc)
    try:
        got = FX.run_product(db, S)
    finally:
        db.close()
    want = FX.run_ref(S) if want is None else want
    d = FX.same(got, want)
    assert not d, d[:10]
    return got


# ----------------------------------------------------------------------------------- the fixtures
@pytest.mark.parametrize("name", list(FX.BUILDERS))
def test_fixture_through_the_class(ctx, voc, name):
    got = check(ctx, voc, FX.build(name), FX.reference(name))
    print(name, got[-1].candidates, got[-1].n_sharing, got[-1].max_common_words, got[-1].min_common_words)


def run_raw(ctx, voc, S):
    """The session's adds, erases and steps 1 and 2 of its queries through the C ABI alone.  -> per query
    (n_sharing, max, min, scored, {id: six fields} of the KeyFrames in the database)"""
    lib, p = ctx.lib, lambda a: int(a.ctypes.data)
    h = C.c_void_p()
    ctx.check(lib.osg_kfdb_create(ctx.handle, voc.handle, C.byref(h)), "create")
    entry, key, parked, out = {}, {}, {}, []

    def state(which, es):
        e = np.array(es, np.int32)
        q, w, s = np.zeros(len(e), np.int64), np.zeros(len(e), np.int32), np.zeros(len(e), np.float32)
        ctx.check(lib.osg_kfdb_state_get(ctx.handle, h, which, len(e), p(e), p(q), p(w), p(s)), "state_get")
        return q, w, s

    def fields(ks):
        if not ks:
            return {}
        a, b = state(0, [entry[k] for k in ks]), state(1, [entry[k] for k in ks])
        return {k: (int(a[0][i]), int(a[1][i]), FX.f32bits(a[2][i]), int(b[0][i]), int(b[1][i]), FX.f32bits(b[2][i]))
                for i, k in enumerate(ks)}

    def leave(ks):
        for k, f in fields(ks).items():
            parked[k] = f
            del key[entry.pop(k)]

    try:
        for op in S.ops:
            if op[0] == "add":
                w, v, m = S.kfs[op[1]]
                w, v = np.array(w, np.int32), np.array(v, np.float64)
                st = None
                if op[1] in parked:
                    f = parked.pop(op[1])
                    st = _abi.OsgKfdbState(f[0], f[3], f[1], f[4], FX.bits_f32(f[2]), FX.bits_f32(f[5]))
                e = C.c_int32(-1)
                ctx.check(lib.osg_kfdb_add(ctx.handle, h, len(w), p(w), p(v), m, C.byref(st) if st else None,
                                           C.byref(e)), "add")
                entry[op[1]], key[e.value] = e.value, op[1]
            elif op[0] == "erase":
                e = entry[op[1]]
                leave([op[1]])
                ctx.check(lib.osg_kfdb_erase(ctx.handle, h, e), "erase")
            elif op[0] == "clear":
                leave(list(entry))
                ctx.check(lib.osg_kfdb_clear(ctx.handle, h), "clear")
            elif op[0] == "clear_map":
                leave([k for k in entry if S.kfs[k][2] == op[1]])
                ctx.check(lib.osg_kfdb_clear_map(ctx.handle, h, op[1]), "clear_map")
            else:
                q = op[1]
                which = 0 if op[0] == "place" else 1
                w, v = np.array(q.words, np.int32), np.array(q.values, np.float64)
                conn = np.array([entry[c] for c in q.connected if c in entry], np.int32)
                n = C.c_int32(0)
                ctx.check(lib.osg_kfdb_size(h, C.byref(n)), "size")
                assert n.value == len(entry)
                cap = max(n.value, 1)
                bufs = (np.zeros(cap, np.int32), np.zeros(cap, np.int32), np.zeros(cap, np.float32), np.zeros(cap))
                o = _abi.OsgKfdbQueryOut()
                o.capacity = n.value
                o.entry, o.words, o.score, o.score_f64 = (p(b) for b in bufs)
                ctx.check(lib.osg_kfdb_query(ctx.handle, h, which, q.id, len(w), p(w), p(v), len(conn),
                                             p(conn) if len(conn) else None, C.byref(o)), "query")
                scored = [(key[int(bufs[0][i])], int(bufs[1][i]), FX.f32bits(bufs[2][i]), FX.f64bits(bufs[3][i]))
                          for i in range(o.n_scored)]
                f = fields(list(entry))
                f.update(parked)
                out.append((o.n_sharing, o.max_common_words, o.min_common_words, scored, f))
    finally:
        lib.osg_kfdb_destroy(h)
    return out


@pytest.mark.parametrize("name", list(FX.BUILDERS))
def test_fixture_through_the_c_abi(ctx, voc, name):
    S = FX.build(name)
    got, want = run_raw(ctx, voc, S), FX.reference(name)
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g[:4] == (w.n_sharing, w.max_common_words, w.min_common_words, w.scored)
        for k, f in g[4].items():
            assert f == w.fields[k], (k, f, w.fields[k])


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_sessions(ctx, voc, seed):
    S = FX.random_session(seed, n_kf=300, n_vocab=FX.N_WORDS, n_ops=500, max_words=200)
    got = check(ctx, voc, S)
    assert sum(any(o.candidates) for o in got) > 10


# ----------------------------------------------------------------------------------- shapes
def shape_session(seed, lengths, n_vocab, q_len, id_hi=None, ops_after=(), maps=1):
    """Entries of the given lengths drawn from a pool a little larger than the longest, so that they share
    words with the query (drawn from the same pool); ``id_hi``: the pool ends at that word id."""
    rng = np.random.default_rng(seed)
    pool_n = min(int(max(max(lengths, default=1), q_len) * 1.25) + 2, n_vocab)
    pool = np.sort(rng.choice(n_vocab, pool_n, replace=False))
    if id_hi is not None:
        pool[-1] = id_hi
        pool = np.unique(pool)

    def draw(n):
        w = np.sort(rng.choice(pool, min(n, len(pool)), replace=False))
        v = rng.uniform(0.1, 1.0, len(w))
        return [int(x) for x in w], [float(x) for x in v / v.sum()]
    kfs = {i: (*draw(n), i % maps) for i, n in enumerate(lengths)}
    if id_hi is not None and kfs:
        w, v, m = kfs[0]
        if w[-1] != id_hi:
            w[-1] = id_hi
    qw, qv = draw(q_len)
    if id_hi is not None:
        qw[-1] = id_hi
    nb = {i: [j for j in range(max(0, i - 5), min(len(lengths), i + 6)) if j != i] for i in kfs}
    ops = [("add", i) for i in kfs]
    ops.append(("place", FX.Query(7000, qw, qv, 0, tuple(range(0, len(lengths), 9))), 3))
    ops.append(("reloc", FX.Query(7001, qw, qv, 0)))
    for op in ops_after:
        ops.append(op)
        if op[0] != "add":
            ops.append(("place", FX.Query(7002 + len(ops), qw, qv, 0), 3))
            ops.append(("reloc", FX.Query(7001, qw, qv, 0)))
    return FX.Session(None, kfs, ops, neighbours=nb, n_words=n_vocab)


def test_empty_database(ctx, voc):
    S = FX.Session(None, {1: ([3], [1.0], 0)}, [("place", FX.Query(5, [3, 4], [0.5, 0.5]), 3),
                                                ("reloc", FX.Query(5, [3, 4], [0.5, 0.5])),
                                                ("add", 1), ("erase", 1), ("place", FX.Query(6, [3], [1.0]), 3),
                                                ("add", 1), ("place", FX.Query(7, [], []), 3),
                                                ("place", FX.Query(8, [4, 5], [0.5, 0.5]), 3)])
    got = check(ctx, voc, S)
    assert all(o.n_sharing == 0 and not o.scored for o in got)
    assert got[-1].fields[1] == (0, 0, 0, 0, 0, 0)       # no shared word: nothing changed


@pytest.mark.parametrize("lengths,q_len", [((1,), 1), ((1,), 40), ((40, 30, 7), 1), ((63, 64, 65, 64, 63, 65, 1, 128, 129), 64),
                                           ((200,) * 3, 200)])
def test_word_counts(ctx, voc, lengths, q_len):
    got = check(ctx, voc, shape_session(11, lengths, FX.N_WORDS, q_len))
    print(lengths, q_len, [(o.n_sharing, o.max_common_words, len(o.scored)) for o in got])


@pytest.mark.parametrize("n", [1, 64, 65, 300])
def test_entry_counts(ctx, voc, n):
    rng = np.random.default_rng(n)
    got = check(ctx, voc, shape_session(12 + n, [int(x) for x in rng.integers(20, 60, n)], FX.N_WORDS, 50, maps=3))
    assert got[1].n_sharing > 0 and got[1].scored        # the relocalisation query: nothing is connected


def test_past_the_staging_limit_and_word_id_999999(ctx, voc_big):
    """A query and an entry of 5 000 words (more than the 4 096 query words kept on chip: the words are read
    from global memory), beside short and staged-size ones, with word id 999 999 in common."""
    got = check(ctx, voc_big, shape_session(13, (5000, 4097, 4096, 900, 5000, 64), 10 ** 6, 5000, id_hi=999999))
    assert got[1].max_common_words > 3000 and got[1].scored   # the relocalisation query: nothing is connected
    got = check(ctx, voc_big, shape_session(14, (5000, 4097, 4096, 900), 10 ** 6, 4096, id_hi=999999))
    assert got[1].max_common_words > 3000 and got[1].scored


def test_after_erase_and_clear_map(ctx, voc):
    n = 70
    ops = [("erase", 0), ("erase", n // 2), ("erase", n - 1), ("add", n // 2), ("add", 0), ("clear_map", 1),
           ("clear_map", 0), ("add", 3)]
    rng = np.random.default_rng(3)
    S = shape_session(15, [int(x) for x in rng.integers(20, 60, n)], FX.N_WORDS, 50, ops_after=ops, maps=3)
    got = check(ctx, voc, S)
    assert len(got) == 2 + 2 * sum(op[0] != "add" for op in ops) and got[-2].scored
    assert got[-1].n_sharing == 0                        # the relocalisation id is repeated: visited, words only grow


def test_two_runs_give_the_same_bits(ctx, voc):
    S = FX.random_session(9, n_kf=120, n_vocab=FX.N_WORDS, n_ops=200, max_words=150)
    db1, db2 = K.KeyFrameDatabase(ctx, voc), K.KeyFrameDatabase(ctx, voc)
    a, b = FX.run_product(db1, S), FX.run_product(db2, S)
    db1.close()
    db2.close()
    assert a == b


# ----------------------------------------------------------------------------------- the chain
def test_transform_add_query_chain(ctx):
    rng = np.random.default_rng(21)
    tree = vb.synth_vocabulary(rng, k=6, L=3, min_children=4)
    voc = vb.ORBVocabulary(ctx, tree)
    base = [vb.synth_features(rng, tree, n=120) for _ in range(3)]
    sets = []
    for i in range(9):                                  # three places, three noisy views of each
        f = vb._flip(rng, base[i % 3], 0.02)
        f[rng.random(len(f)) < 0.2] = rng.integers(0, 256, 32, dtype=np.uint8)
        sets.append(f)
    query_desc = vb._flip(rng, base[1], 0.02)
    kfs, got_bows = {}, {}
    for i, f in enumerate(sets):
        bw, _ = pb.transform(tree, f)
        kfs[i] = (sorted(bw), [bw[w] for w in sorted(bw)], 0)
        got_bows[i] = voc.transform(f)
    qb, _ = pb.transform(tree, query_desc)
    q = FX.Query(77, sorted(qb), [qb[w] for w in sorted(qb)], 0, (8,))
    S = FX.Session(None, kfs, [("add", i) for i in kfs] + [("place", q, 3), ("reloc", FX.Query(78, q.words, q.values))],
                   neighbours={i: [j for j in kfs if j % 3 == i % 3 and j != i] for i in kfs},
                   n_words=voc.info()["n_words"])
    want = FX.run_ref(S)
    db = K.KeyFrameDatabase(ctx, voc)
    for i in kfs:
        db.add(i, got_bows[i], 0)
    gq = voc.transform(query_desc)
    loop, merge = db.detect_n_best_candidates(gq, 77, 0, (8,), S.neighbours, 3)
    r1 = db.last
    reloc = db.detect_relocalization_candidates(gq, 78, 0, S.neighbours)
    r2 = db.last
    assert ((tuple(loop), tuple(merge)), (tuple(reloc),)) == (want[0].candidates, want[1].candidates)
    for r, w in ((r1, want[0]), (r2, want[1])):
        assert (r.n_sharing, r.max_common_words, r.min_common_words) == (w.n_sharing, w.max_common_words,
                                                                         w.min_common_words)
        assert [(int(e), int(n), FX.f32bits(s), FX.f64bits(d)) for e, n, s, d in
                zip(r.entry, r.words, r.score, r.score_f64)] == w.scored
    assert want[0].scored and want[0].candidates[0]
    db.close()
    voc.close()


# ----------------------------------------------------------------------------------- what the host refuses
def test_invalid_arguments(ctx, voc):
    db = K.KeyFrameDatabase(ctx, voc)
    db.add("a", ([1, 5], [0.5, 0.5]))
    with pytest.raises(OsgError, match="invalid"):
        db.add("a", ([1, 5], [0.5, 0.5]))               # a KeyFrame added twice
    for words in ([5, 1], [1, 1], [-1, 2], [3, FX.N_WORDS]):
        with pytest.raises(OsgError, match="invalid"):
            db.add("b", (words, [0.5, 0.5]))
        with pytest.raises(OsgError, match="invalid"):
            db.query(K.PLACE, (words, [0.5, 0.5]), 1)
    db.add("b", ([0, FX.N_WORDS - 1], [0.5, 0.5]))
    with pytest.raises(OsgError, match="invalid"):
        db.erase("zzz")
    e = db._entry["b"]
    db.erase("b")
    assert ctx.lib.osg_kfdb_erase(ctx.handle, db.handle, e) == _abi.OSG_E_INVALID
    assert ctx.lib.osg_kfdb_erase(ctx.handle, db.handle, 12345) == _abi.OSG_E_INVALID
    assert len(db) == 1 and db.keyframes() == ["a"]
    assert db.add("b", ([7], [1.0])) == e + 1           # ids are never reused
    db.close()
    l2 = vb.ORBVocabulary(ctx, full_vocabulary(4, 2, scoring=vb.L2_NORM))
    h = C.c_void_p()
    assert ctx.lib.osg_kfdb_create(ctx.handle, l2.handle, C.byref(h)) == _abi.OSG_E_UNSUPPORTED
    l2.close()


def test_state_accessors(ctx, voc):
    db = K.KeyFrameDatabase(ctx, voc)
    for i in range(5):
        db.add(i, ([i, i + 10], [0.5, 0.5]), i % 2)
    db.set_state(K.PLACE, [3, 1], [2 ** 40 + 3, -1], [7, 8], [0.25, 0.5])
    db.set_state(K.RELOC, [4], [9], [1], [0.125])
    q, w, s = db.state(K.PLACE)
    assert q.tolist() == [0, -1, 0, 2 ** 40 + 3, 0] and w.tolist() == [0, 8, 0, 7, 0] and s.tolist() == [0, .5, 0, .25, 0]
    assert db.fields(4) == (0, 0, 0.0, 9, 1, 0.125)
    db.erase(3)
    assert db.fields(3)[:3] == (2 ** 40 + 3, 7, 0.25)
    db.add(3, ([3, 13], [0.5, 0.5]), 1)                  # keeps its fields, goes to the back
    assert db.keyframes() == [0, 1, 2, 4, 3] and db.fields(3)[:3] == (2 ** 40 + 3, 7, 0.25)
    db.close()
