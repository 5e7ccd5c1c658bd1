"""Scripted KeyFrameDatabase sessions for tests/test_kfdb.py (CPU), tests/test_kfdb_gpu.py and smoke().

A Session is a set of KeyFrames (id -> BowVector, map), their covisibility top-10, and a list of operations:
    ("add", id)  ("erase", id)  ("clear",)  ("clear_map", map)
    ("place", Query, n)     DetectNBestCandidates of a KeyFrame that is not in the database
    ("reloc", Query)        DetectRelocalizationCandidates of a Frame
``rule`` names the reference rule the session is there for: tests/pyref_kfdb.py with that rule switched off
must return other candidates for the session's last query (``bites``), or the fixture is useless.

run_ref plays a session on the restatement, run_product on orb_slam3_comments_ghr_amd.keyframedb; both
return one Outcome per query, which ``same`` compares exactly (integers and float / double bit patterns).

Every fixture has at most 300 entries of at most 200 words (tests/test_kfdb_gpu.py builds the larger shapes
it states).
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

from tests import pyref_kfdb as R

N_WORDS = 1000      # vocabulary words of the hand-made fixtures


@dataclass
class Query:
    id: int
    words: list
    values: list
    map_id: int = 0
    connected: tuple = ()


@dataclass
class Session:
    rule: str | None
    kfs: dict                       # id -> (words, values, map_id)
    ops: list
    neighbours: dict = field(default_factory=dict)   # id -> ids (top-10); ids need not be in the database
    bad: tuple = ()
    bad_maps: tuple = ()
    n_words: int = N_WORDS
    doc: str = ""


@dataclass
class Outcome:
    kind: str
    candidates: tuple               # place: (loop ids, merge ids); reloc: (ids,)
    n_sharing: int
    max_common_words: int
    min_common_words: int
    scored: list                    # (id, words, float32 bits, float64 bits)
    fields: dict                    # id -> (pq, pw, ps bits, rq, rw, rs bits) of every KeyFrame of the session


def f32bits(x):
    return int(np.float32(x).view(np.uint32))


def f64bits(x):
    return int(np.float64(x).view(np.uint64))


def field_bits(f):
    return (int(f[0]), int(f[1]), f32bits(f[2]), int(f[3]), int(f[4]), f32bits(f[5]))


# ---------------------------------------------------------------------------------------- runners
def run_ref(S: Session, rules=()):
    """The session on the restatement; ``rules`` are switched off in the LAST query only."""
    db = R.KeyFrameDatabase(S.n_words)
    db.bad_maps = set(S.bad_maps)
    kf = {k: R.KeyFrame(k, w, v, m) for k, (w, v, m) in S.kfs.items()}
    for k, x in kf.items():
        x.bad = k in S.bad
    for k, l in S.neighbours.items():
        kf[k].neighbours = [kf[j] for j in l]
    last = max(i for i, op in enumerate(S.ops) if op[0] in ("place", "reloc"))
    out = []
    for i, op in enumerate(S.ops):
        r = tuple(rules) if i == last else ()
        if op[0] == "add":
            db.add(kf[op[1]])
        elif op[0] == "erase":
            db.erase(kf[op[1]])
        elif op[0] == "clear":
            db.clear()
        elif op[0] == "clear_map":
            db.clear_map(op[1])
        elif op[0] == "place":
            q = op[1]
            qk = R.KeyFrame(q.id, q.words, q.values, q.map_id)
            qk.connected = {kf[c] for c in q.connected}
            lo, me, t = db.detect_n_best_candidates(qk, op[2], r)
            out.append(_outcome("place", ([x.mnId for x in lo], [x.mnId for x in me]), t, kf))
        elif op[0] == "reloc":
            q = op[1]
            c, t = db.detect_relocalization_candidates(q.words, q.values, q.id, q.map_id, r)
            out.append(_outcome("reloc", ([x.mnId for x in c],), t, kf))
        else:
            raise ValueError(op)
    return out


def _outcome(kind, cands, t, kf):
    return Outcome(kind, tuple(tuple(c) for c in cands), t.n_sharing, t.max_common_words, t.min_common_words,
                   [(k.mnId, n, f32bits(si), f64bits(d)) for k, n, si, d in t.scored],
                   {k: field_bits(x.fields()) for k, x in kf.items()})


def run_product(db, S: Session):
    """The session on a orb_slam3_comments_ghr_amd.keyframedb.KeyFrameDatabase (empty at entry)."""
    out = []
    for op in S.ops:
        if op[0] == "add":
            w, v, m = S.kfs[op[1]]
            db.add(op[1], (w, v), m)
        elif op[0] == "erase":
            db.erase(op[1])
        elif op[0] == "clear":
            db.clear()
        elif op[0] == "clear_map":
            db.clear_map(op[1])
        elif op[0] in ("place", "reloc"):
            q = op[1]
            if op[0] == "place":
                c = db.detect_n_best_candidates((q.words, q.values), q.id, q.map_id, q.connected, S.neighbours, op[2],
                                                bad=S.bad, bad_maps=S.bad_maps)
            else:
                c = (db.detect_relocalization_candidates((q.words, q.values), q.id, q.map_id, S.neighbours),)
            r = db.last
            keys = [db._key[int(e)] for e in r.entry]
            out.append(Outcome(op[0], tuple(tuple(x) for x in c), r.n_sharing, r.max_common_words, r.min_common_words,
                               [(keys[i], int(r.words[i]), f32bits(r.score[i]), f64bits(r.score_f64[i]))
                                for i in range(r.n_scored)],
                               {k: field_bits(db.fields(k)) for k in S.kfs}))
        else:
            raise ValueError(op)
    return out


def same(got, want):
    """-> list of differences between two runs (empty: identical)"""
    d = []
    if len(got) != len(want):
        return [f"{len(got)} queries, expected {len(want)}"]
    for i, (g, w) in enumerate(zip(got, want)):
        for name in ("kind", "candidates", "n_sharing", "max_common_words", "min_common_words", "scored"):
            if getattr(g, name) != getattr(w, name):
                d.append(f"query {i}: {name} {getattr(g, name)!r} != {getattr(w, name)!r}")
        for k in w.fields:
            if g.fields.get(k) != w.fields[k]:
                d.append(f"query {i}: fields of KeyFrame {k}: {g.fields.get(k)!r} != {w.fields[k]!r}")
    return d


def bits_f32(b):
    return float(np.array([b], np.uint32).view(np.float32)[0])


def select_problem(S: Session, op, o: Outcome):
    """What step 3 is given after steps 1 and 2 of query ``op`` left Outcome ``o``: the scored KeyFrames and
    their neighbours as the tuples (query, score, handle, map, bad, map_bad) of keyframedb.select_nbest, with
    the KeyFrame ids as handles."""
    qi, si = (0, 2) if o.kind == "place" else (3, 5)

    def kf(k, score_bits=None):
        f = o.fields[k]
        m = S.kfs[k][2]
        return (f[qi], bits_f32(f[si] if score_bits is None else score_bits), k, m, int(k in S.bad),
                int(m in S.bad_maps))
    cands = [kf(k, sb) for k, _, sb, _ in o.scored]
    neighs = [[kf(j) for j in S.neighbours.get(k, [])[:10]] for k, _, _, _ in o.scored]
    return cands, neighs, op[1].id, op[1].map_id


def bites(name):
    """The candidates of the fixture's last query with its rule on and off."""
    S = build(name)
    return run_ref(S)[-1].candidates, run_ref(S, (S.rule,))[-1].candidates


# ---------------------------------------------------------------------------------------- hand-made fixtures
def bow(pairs):
    """{word: value} -> (ascending words, values)"""
    w = sorted(pairs)
    return [int(x) for x in w], [float(pairs[x]) for x in w]


def uniform(words, total=1.0):
    return {w: total / len(words) for w in words}


def _stale():
    q1w = list(range(100, 120))                       # first query = N's BowVector
    q2w = list(range(200, 220))
    A = bow(uniform(q2w))
    Bp = {w: 0.03 for w in q2w[:18]}
    Bp.update({300: 0.23, 301: 0.23})
    B = bow(Bp)
    Np = uniform(q1w[:19], 0.95)
    Np[200] = 0.05                                    # one word of the second query: visited, under the threshold
    N = bow(Np)
    kfs = {1: (*A, 0), 2: (*B, 0), 3: (*N, 0)}
    q1 = Query(50, *bow(Np))
    q2 = Query(51, *bow(uniform(q2w)))
    return Session("stale", kfs, [("add", 1), ("add", 2), ("add", 3), ("place", q1, 3), ("place", q2, 1)],
                   neighbours={2: [3]},
                   doc="KeyFrame 3 is scored by the first query; the second visits it under the threshold, and its "
                       "stale score makes KeyFrame 2's group (and 3 as its best member) beat KeyFrame 1")


def _connected(winner_only):
    qw = list(range(10, 30))
    C = bow(uniform(qw))                              # the query itself: would win
    Dp = {w: 0.04 for w in qw[:18]}
    Dp.update({400: 0.28})
    D = bow(Dp)
    Ep = {w: 0.03 for w in qw[2:20]}
    Ep.update({401: 0.46})
    E = bow(Ep)
    kfs = {1: (*C, 0), 2: (*D, 0), 3: (*E, 0)}
    if winner_only:
        q = Query(60, *bow(uniform(qw)), 0, (1,))
        return Session("connected", kfs, [("add", 1), ("add", 2), ("add", 3), ("place", q, 1)],
                       doc="the connected KeyFrame 1 equals the query and would win")
    C2 = bow({w: 0.05 for w in qw})
    kfs[4] = (*C2, 0)
    q = Query(60, *bow(uniform(qw)), 0, (1, 4, 99))
    kfs[99] = (*bow({500: 1.0}), 0)                   # connected, never added
    return Session("connected", kfs, [("add", 1), ("add", 2), ("add", 4), ("add", 3), ("place", q, 2)],
                   neighbours={2: [1, 4], 3: [4, 1, 2]},
                   doc="connected KeyFrames 1 and 4 are not listed, are left at words = 1 with their query field "
                       "untouched, and are skipped as neighbours of 2 and 3")


def _threshold(max_words):
    if max_words == 5:
        qp = {1: 0.3, 2: 0.3, 3: 0.2, 4: 0.1, 5: 0.1}
        X = bow({1: 0.3, 2: 0.3, 3: 0.2, 4: 0.1, 600: 0.1})          # 4 common words, score 0.9
        Y = bow({1: 0.02, 2: 0.02, 3: 0.02, 4: 0.02, 5: 0.02, 601: 0.9})  # 5 common words, score 0.1
        kfs = {1: (*X, 0), 2: (*Y, 0)}
        return Session("strict", kfs, [("add", 1), ("add", 2), ("place", Query(70, *bow(qp)), 1)],
                       doc="maxCommonWords 5, minCommonWords 4: KeyFrame 1 with exactly 4 is left out")
    qp = {1: 0.5, 2: 0.5}
    X = bow({1: 0.5, 700: 0.5})
    Y = bow({2: 0.25, 701: 0.75})
    kfs = {1: (*X, 0), 2: (*Y, 0)}
    return Session("trunc", kfs, [("add", 1), ("add", 2), ("place", Query(70, *bow(qp)), 3)],
                   doc="maxCommonWords 1: minCommonWords = int(0.8f) = 0, so every sharing KeyFrame is scored")


def _tie_identical():
    b = bow(uniform(range(40, 50)))
    kfs = {10: (*b, 0), 5: (*b, 0), 8: (*b, 0)}
    return Session("order", kfs, [("add", 10), ("add", 5), ("add", 8), ("place", Query(80, *b), 2)],
                   doc="identical BowVectors added as 10, 5, 8: equal scores keep the order of the adds")


def _tie_acc():
    q = bow({1: 0.5, 2: 0.5})
    X = bow({2: 0.5, 800: 0.5})      # added first, first common word 2
    Y = bow({1: 0.5, 801: 0.5})      # added second, first common word 1: visited first
    kfs = {1: (*X, 0), 2: (*Y, 0)}
    return Session("order", kfs, [("add", 1), ("add", 2), ("place", Query(81, *q), 1)],
                   doc="equal accScore: the KeyFrame met first in the walk over the query's words stays first")


def _tie_readd():
    b = bow(uniform(range(40, 50)))
    kfs = {1: (*b, 0), 2: (*b, 0)}
    return Session("order", kfs, [("add", 1), ("add", 2), ("erase", 1), ("add", 1), ("place", Query(82, *b), 1)],
                   doc="erase and add again moves KeyFrame 1 behind KeyFrame 2")


def _id_zero():
    b = bow(uniform(range(40, 50)))
    kfs = {1: (*b, 0), 2: (*bow(uniform(range(45, 55))), 0)}
    return Session("visited", kfs, [("add", 1), ("add", 2), ("place", Query(0, *b), 3)],
                   doc="query id 0 on fresh KeyFrames (fields 0): all count as visited, nothing is listed")


def _id_repeated():
    b = bow(uniform(range(40, 50)))
    kfs = {1: (*b, 0), 2: (*bow(uniform(range(41, 51))), 0), 3: (*bow(uniform(range(42, 53))), 0)}
    return Session("visited", kfs, [("add", 1), ("add", 2), ("place", Query(9, *b), 3), ("add", 3),
                                    ("place", Query(9, *b), 3)],
                   neighbours={3: [2]},
                   doc="the same query id again: KeyFrames 1 and 2 only gain words, the new KeyFrame 3 is listed "
                       "alone and takes KeyFrame 2's score of the first call into its group")


def _maps(kind):
    qw = list(range(10, 30))
    q = bow(uniform(qw))

    def near(k, extra):
        p = {w: 0.05 - 0.001 * k for w in qw[:19]}
        p[extra] = 1.0 - sum(p.values())
        return bow(p)
    if kind == "badmap":
        kfs = {1: (*near(1, 901), 0), 2: (*near(2, 902), 2), 3: (*near(3, 903), 1), 4: (*near(4, 904), 2),
               5: (*near(5, 905), 0)}
        return Session("badmap", kfs, [("add", k) for k in (1, 2, 3, 4, 5)] + [("place", Query(90, *q, 0), 3)],
                       bad_maps=(2,), doc="maps 0 (the query's), 1 and the bad map 2: its KeyFrames are no merge candidates")
    if kind == "dedup":
        kfs = {1: (*near(5, 901), 0), 2: (*near(6, 902), 0), 3: (*near(1, 903), 0), 4: (*near(9, 904), 0)}
        return Session("dedup", kfs, [("add", k) for k in (1, 2, 3, 4)] + [("place", Query(91, *q, 0), 2)],
                       neighbours={1: [3], 2: [3], 4: []},
                       doc="KeyFrame 3 is the best member of the groups of 1, 2 and its own: listed once")
    if kind == "few":
        kfs = {1: (*near(1, 901), 0), 2: (*near(2, 902), 1)}
        return Session(None, kfs, [("add", 1), ("add", 2), ("place", Query(92, *q, 0), 3)],
                       doc="fewer than N candidates: one loop and one merge candidate (no rule to switch off: the "
                           "walk ends with the list)")
    kfs = {1: (*near(1, 901), 0), 2: (*near(2, 902), 0), 3: (*near(3, 903), 0)}
    return Session("badkf", kfs, [("add", k) for k in (1, 2, 3)] + [("place", Query(93, *q, 0), 2)], bad=(1,),
                   doc="the best KeyFrame is bad: skipped, and the walk goes on (the reference would not return)")


def _reloc(kind):
    q = bow({1: 0.5, 2: 0.125, 3: 0.125, 4: 0.125, 5: 0.125})
    K1 = q                                                                        # score 1.0
    K2 = bow({1: 0.25, 2: 0.125, 3: 0.125, 4: 0.125, 5: 0.125, 950: 0.25})       # score 0.75 exactly
    K3 = bow({1: 0.5, 2: 0.125, 3: 0.125, 4: 0.0625, 5: 0.0625, 951: 0.125})     # score 0.875, another map
    if kind == "strict":
        kfs = {1: (*K1, 0), 2: (*K2, 0)}
        return Session("strict", kfs, [("add", 1), ("add", 2), ("reloc", Query(100, *q, 0))],
                       doc="accScore == 0.75f * bestAccScore is not retained")
    kfs = {1: (*K1, 0), 2: (*K2, 0), 3: (*K3, 1), 4: (*K2, 0)}
    return Session("mapfilter", kfs, [("add", 1), ("add", 3), ("add", 2), ("add", 4), ("reloc", Query(101, *q, 0))],
                   neighbours={1: [2], 4: [3]},
                   doc="KeyFrame 3 of another map is the best member of KeyFrame 4's group, which passes the bound: "
                       "dropped")


BUILDERS = {
    "stale_score": _stale,
    "connected_excluded": lambda: _connected(False),
    "connected_winner": lambda: _connected(True),
    "threshold_max5": lambda: _threshold(5),
    "threshold_max1": lambda: _threshold(1),
    "tie_identical": _tie_identical,
    "tie_acc_score": _tie_acc,
    "tie_readd": _tie_readd,
    "id_zero": _id_zero,
    "id_repeated": _id_repeated,
    "maps_bad_map": lambda: _maps("badmap"),
    "best_duplicates": lambda: _maps("dedup"),
    "fewer_than_n": lambda: _maps("few"),
    "bad_best": lambda: _maps("badkf"),
    "reloc_strict": lambda: _reloc("strict"),
    "reloc_map_filter": lambda: _reloc("mapfilter"),
}
SMOKE = "stale_score"


@functools.lru_cache(maxsize=None)
def build(name) -> Session:
    return BUILDERS[name]()


@functools.lru_cache(maxsize=None)
def reference(name):
    return run_ref(build(name))


# ---------------------------------------------------------------------------------------- random sessions
def random_session(seed, n_kf=60, n_vocab=400, n_ops=120, max_words=40) -> Session:
    """add / erase / re-add / clear_map / query operations in random order over a place database, with
    repeated query ids, id 0 and connected sets."""
    from orb_slam3_comments_ghr_amd.keyframedb import synth_place_db
    rng = np.random.default_rng(seed)
    P = synth_place_db(rng, n_kf=n_kf, n_vocab_words=n_vocab, words_per_kf=int(rng.integers(1, max_words + 1)),
                       n_places=5, n_maps=3)
    kfs = {i: ([int(x) for x in P.words[i]], [float(x) for x in P.values[i]], int(P.map_id[i])) for i in range(n_kf)}
    inside, ops, nq = set(), [], 0
    for _ in range(n_ops):
        u = rng.random()
        if u < 0.45 or not inside:
            k = int(rng.integers(0, n_kf))
            if k not in inside:
                ops.append(("add", k))
                inside.add(k)
        elif u < 0.55:
            k = int(rng.choice(sorted(inside)))
            ops.append(("erase", k))
            inside.discard(k)
        elif u < 0.58:
            m = int(rng.integers(0, 3))
            ops.append(("clear_map", m))
            inside = {k for k in inside if kfs[k][2] != m}
        else:
            k = int(rng.integers(0, n_kf))
            qid = int(rng.choice([0, 1, 2, 3, 1000 + nq]))
            nq += 1
            if rng.random() < 0.6:
                q = Query(qid, kfs[k][0], kfs[k][1], kfs[k][2], tuple(sorted(P.connected[k])))
                ops.append(("place", q, int(rng.integers(1, 4))))
            else:
                ops.append(("reloc", Query(qid, kfs[k][0], kfs[k][1], kfs[k][2])))
    k = int(rng.integers(0, n_kf))
    ops.append(("place", Query(5000, kfs[k][0], kfs[k][1], kfs[k][2], tuple(sorted(P.connected[k]))), 3))
    bad = tuple(int(x) for x in rng.choice(n_kf, 3, replace=False))
    return Session(None, kfs, ops, neighbours={i: list(P.neighbours[i]) for i in range(n_kf)}, bad=bad, bad_maps=(2,),
                   n_words=n_vocab)
