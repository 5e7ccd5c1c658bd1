"""``KeyFrameDatabase`` (ref:src/KeyFrameDatabase.cc) on the GPU: the BoW place-recognition query that
chooses the KeyFrames LoopClosing and relocalisation run on.

``detect_n_best_candidates`` mirrors DetectNBestCandidates (:669-880) and ``detect_relocalization_candidates``
DetectRelocalizationCandidates (:920-1031).  The words in common, the per-KeyFrame fields
(mnPlaceRecognitionQuery / Words / Score, mnRelocQuery / Words / Score), the 0.8 threshold and the L1 scores
are computed by csrc/kfdb.hip (osg_kfdb_query); the covisibility groups and the choice of candidates by
csrc/kfdb_select.h on the neighbours the caller names.  The fields persist from call to call as they do in
the reference (a neighbour that shared a word but was not scored contributes the score an earlier call
left), and a KeyFrame that is erased and added again keeps them.

KeyFrames are named by any hashable key of the caller's.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field

import numpy as np

from . import Context, OsgError, _abi
from .vocabulary import ORBVocabulary

PLACE, RELOC = _abi.OSG_KFDB_PLACE, _abi.OSG_KFDB_RELOC


def _p(a):
    return None if a is None else int(a.ctypes.data)


def _bow(bow):
    """(words int32 ascending, values float64) of a BowResult or a (words, values) pair."""
    w, v = (bow.word, bow.value) if hasattr(bow, "word") else bow
    return np.ascontiguousarray(w, np.int32).reshape(-1), np.ascontiguousarray(v, np.float64).reshape(-1)


@dataclass
class QueryResult:
    """Steps 1 and 2 of a detector: the scored entries in the reference's list order."""
    n_sharing: int
    max_common_words: int
    min_common_words: int
    entry: np.ndarray       # int32
    words: np.ndarray       # int32
    score: np.ndarray       # float32 si
    score_f64: np.ndarray   # the double si was converted from

    @property
    def n_scored(self):
        return len(self.entry)


def _kf_arrays(cands, neighs):
    n = len(cands)
    cand = (_abi.OsgKfdbKf * max(n, 1))(*[_abi.OsgKfdbKf(*c) for c in cands])
    nn = np.array([len(l) for l in neighs] + [0] * (n == 0), np.int32)
    ne = (_abi.OsgKfdbKf * (max(n, 1) * _abi.OSG_KFDB_MAX_NEIGH))()
    for i, l in enumerate(neighs):
        assert len(l) <= _abi.OSG_KFDB_MAX_NEIGH
        for j, k in enumerate(l):
            ne[i * _abi.OSG_KFDB_MAX_NEIGH + j] = _abi.OsgKfdbKf(*k)
    return n, cand, nn, ne


def _rc(rc, what):
    if rc < 0:
        raise OsgError(f"{what}: error {rc}")


def select_nbest(cands, neighs, query_id, query_map, n=3):
    """Step 3 of DetectNBestCandidates (csrc/kfdb_select.h; host only, no device): ``cands`` the scored
    KeyFrames in list order and ``neighs[i]`` the top-10 neighbours of the i-th, each a tuple (query, score,
    handle, map_id, bad, map_bad) of the fields after the query.  -> (loop handles, merge handles)"""
    from . import load_library
    ns, cand, nn, ne = _kf_arrays(cands, neighs)
    lo, me = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32)
    nl, nm = C.c_int32(0), C.c_int32(0)
    _rc(load_library().osg_kfdb_select_nbest(ns, C.addressof(cand), _p(nn), C.addressof(ne), int(query_id),
                                             int(query_map), int(n), _p(lo), C.addressof(nl), _p(me), C.addressof(nm)),
        "keyframe database select")
    return [int(h) for h in lo[:nl.value]], [int(h) for h in me[:nm.value]]


def select_reloc(cands, neighs, frame_id, map_id):
    """Step 3 of DetectRelocalizationCandidates, as select_nbest.  -> handles"""
    from . import load_library
    ns, cand, nn, ne = _kf_arrays(cands, neighs)
    out = np.zeros(max(ns, 1), np.int32)
    no = C.c_int32(0)
    _rc(load_library().osg_kfdb_select_reloc(ns, C.addressof(cand), _p(nn), C.addressof(ne), int(frame_id), int(map_id),
                                             _p(out), C.addressof(no)), "keyframe database select")
    return [int(h) for h in out[:no.value]]


class KeyFrameDatabase:
    def __init__(self, ctx: Context, voc: ORBVocabulary):
        self.ctx = ctx
        self.voc = voc
        h = C.c_void_p()
        ctx.check(ctx.lib.osg_kfdb_create(ctx.handle, voc.handle, C.byref(h)), "keyframe database")
        self.handle = h
        self._entry = {}      # key -> entry id, while in the database
        self._key = {}        # entry id -> key
        self._map = {}        # key -> map id (kept after an erase)
        self._parked = {}     # key -> the six fields of a KeyFrame that left the database
        self.last = None      # QueryResult of the last detect call

    # ---- add / erase / clear / clearMap ----------------------------------------------------------
    def add(self, kf, bow, map_id=0) -> int:
        """add(pKF).  A KeyFrame that is already in the database is an error (the reference would list it
        twice and count each of its words twice)."""
        if kf in self._entry:
            raise OsgError(f"keyframe database add: invalid argument (KeyFrame {kf!r} is already in the database)")
        w, v = _bow(bow)
        if len(w) != len(v):
            raise OsgError("keyframe database add: invalid argument (words and values differ in length)")
        st = None
        if kf in self._parked:
            pq, pw, ps, rq, rw, rs = self._parked[kf]
            st = _abi.OsgKfdbState(int(pq), int(rq), int(pw), int(rw), float(ps), float(rs))
        e = C.c_int32(-1)
        rc = self.ctx.lib.osg_kfdb_add(self.ctx.handle, self.handle, len(w), _p(w), _p(v), int(map_id),
                                       C.byref(st) if st is not None else None, C.byref(e))
        self.ctx.check(rc, "keyframe database add")
        self._parked.pop(kf, None)
        self._entry[kf] = e.value
        self._key[e.value] = kf
        self._map[kf] = int(map_id)
        return e.value

    def _park(self, kfs):
        kfs = list(kfs)
        if not kfs:
            return
        f = self._fields_of_entries([self._entry[k] for k in kfs])
        for i, k in enumerate(kfs):
            self._parked[k] = tuple(x[i] for x in f)

    def _forget(self, kf):
        del self._key[self._entry.pop(kf)]

    def erase(self, kf):
        if kf not in self._entry:
            raise OsgError(f"keyframe database erase: invalid argument (KeyFrame {kf!r} is not in the database)")
        self._park([kf])
        self.ctx.check(self.ctx.lib.osg_kfdb_erase(self.ctx.handle, self.handle, self._entry[kf]),
                       "keyframe database erase")
        self._forget(kf)

    def clear(self):
        self._park(list(self._entry))
        self.ctx.check(self.ctx.lib.osg_kfdb_clear(self.ctx.handle, self.handle), "keyframe database clear")
        self._entry.clear()
        self._key.clear()

    def clear_map(self, map_id):
        gone = [k for k in self._entry if self._map[k] == int(map_id)]
        self._park(gone)
        self.ctx.check(self.ctx.lib.osg_kfdb_clear_map(self.ctx.handle, self.handle, int(map_id)),
                       "keyframe database clear_map")
        for k in gone:
            self._forget(k)

    def __len__(self):
        n = C.c_int32(0)
        self.ctx.check(self.ctx.lib.osg_kfdb_size(self.handle, C.byref(n)), "keyframe database size")
        return n.value

    def keyframes(self):
        """The KeyFrames in list order: the order of the adds (entry ids grow with every add)."""
        return [self._key[e] for e in sorted(self._key)]

    def __contains__(self, kf):
        return kf in self._entry

    # ---- the per-KeyFrame fields -----------------------------------------------------------------
    def _state_of_entries(self, which, entries):
        e = np.ascontiguousarray(entries, np.int32)
        q, w, s = np.zeros(len(e), np.int64), np.zeros(len(e), np.int32), np.zeros(len(e), np.float32)
        self.ctx.check(self.ctx.lib.osg_kfdb_state_get(self.ctx.handle, self.handle, which, len(e), _p(e), _p(q), _p(w),
                                                       _p(s)), "keyframe database state_get")
        return q, w, s

    def _fields_of_entries(self, entries):
        return self._state_of_entries(PLACE, entries) + self._state_of_entries(RELOC, entries)

    def state(self, which, kfs=None):
        """(query int64, words int32, score float32) of detector ``which`` for the KeyFrames ``kfs`` (default:
        all, in list order); every one of them is in the database."""
        kfs = self.keyframes() if kfs is None else list(kfs)
        return self._state_of_entries(which, [self._entry[k] for k in kfs])

    def set_state(self, which, kfs, query, words, score):
        e = np.ascontiguousarray([self._entry[k] for k in kfs], np.int32)
        q, w, s = (np.ascontiguousarray(query, np.int64), np.ascontiguousarray(words, np.int32),
                   np.ascontiguousarray(score, np.float32))
        assert len(q) == len(w) == len(s) == len(e)
        self.ctx.check(self.ctx.lib.osg_kfdb_state_set(self.ctx.handle, self.handle, which, len(e), _p(e), _p(q), _p(w),
                                                       _p(s)), "keyframe database state_set")

    def fields(self, kf):
        """The six fields of one KeyFrame, in the database or not: (place query, words, score, reloc query,
        words, score)."""
        if kf in self._entry:
            return tuple(x[0] for x in self._fields_of_entries([self._entry[kf]]))
        return self._parked.get(kf, (0, 0, np.float32(0), 0, 0, np.float32(0)))

    # ---- steps 1 and 2 ---------------------------------------------------------------------------
    def query(self, which, bow, query_id, connected=()) -> QueryResult:
        w, v = _bow(bow)
        if len(w) != len(v):
            raise OsgError("keyframe database query: invalid argument (words and values differ in length)")
        conn = np.ascontiguousarray([self._entry[k] for k in connected if k in self._entry], np.int32)
        cap = len(self._entry)
        bufs = (np.zeros(max(cap, 1), np.int32), np.zeros(max(cap, 1), np.int32), np.zeros(max(cap, 1), np.float32),
                np.zeros(max(cap, 1), np.float64))
        o = _abi.OsgKfdbQueryOut()
        o.capacity = cap
        o.entry, o.words, o.score, o.score_f64 = (_p(b) for b in bufs)
        rc = self.ctx.lib.osg_kfdb_query(self.ctx.handle, self.handle, which, int(query_id), len(w), _p(w), _p(v),
                                         len(conn), _p(conn) if len(conn) else None, C.byref(o))
        self.ctx.check(rc, "keyframe database query")
        n = o.n_scored
        return QueryResult(o.n_sharing, o.max_common_words, o.min_common_words, *(b[:n].copy() for b in bufs))

    # ---- step 3 ----------------------------------------------------------------------------------
    def _select_args(self, which, r, neighbours, bad, bad_maps):
        """The scored KeyFrames and their top-10 neighbours as the tuples of select_nbest; handles index
        the returned keys."""
        scored = [self._key[int(e)] for e in r.entry]
        neigh = [list(neighbours.get(k, ()))[:_abi.OSG_KFDB_MAX_NEIGH] for k in scored]
        keys, handle = [], {}
        for k in scored + [x for l in neigh for x in l]:
            if k not in handle:
                handle[k] = len(keys)
                keys.append(k)
        live = [k for k in keys if k in self._entry]
        q, _, s = self._state_of_entries(which, [self._entry[k] for k in live]) if live else ((), (), ())
        fq = {k: (int(q[i]), float(s[i])) for i, k in enumerate(live)}
        off = 0 if which == PLACE else 3

        def kf_tuple(k, score=None):
            if k in fq:
                qq, ss = fq[k]
            else:
                f = self._parked.get(k, (0, 0, 0.0, 0, 0, 0.0))
                qq, ss = int(f[off]), float(f[off + 2])
            m = self._map.get(k, -1)
            return (qq, ss if score is None else float(score), handle[k], m, int(k in bad), int(m in bad_maps))

        return ([kf_tuple(k, r.score[i]) for i, k in enumerate(scored)], [[kf_tuple(k) for k in l] for l in neigh],
                keys)

    def detect_n_best_candidates(self, bow, query_id, map_id, connected, neighbours, n=3, bad=(), bad_maps=()):
        """DetectNBestCandidates(pKF, vpLoopCand, vpMergeCand, n): ``bow`` / ``query_id`` / ``map_id`` are pKF's
        mBowVec, mnId and map, ``connected`` its GetConnectedKeyFrames(), ``neighbours[kf]`` the
        GetBestCovisibilityKeyFrames(10) of KeyFrame kf, ``bad`` the KeyFrames and ``bad_maps`` the maps whose
        isBad() / IsBad() holds.  A bad best KeyFrame is skipped (the reference would not return).
        -> (loop candidates, merge candidates)"""
        r = self.last = self.query(PLACE, bow, query_id, connected)
        if r.n_scored == 0:
            return [], []
        cands, neighs, keys = self._select_args(PLACE, r, neighbours, set(bad), set(bad_maps))
        lo, me = select_nbest(cands, neighs, query_id, map_id, n)
        return [keys[h] for h in lo], [keys[h] for h in me]

    def detect_relocalization_candidates(self, bow, frame_id, map_id, neighbours):
        """DetectRelocalizationCandidates(F, pMap) -> the candidate KeyFrames"""
        r = self.last = self.query(RELOC, bow, frame_id)
        if r.n_scored == 0:
            return []
        cands, neighs, keys = self._select_args(RELOC, r, neighbours, set(), set())
        return [keys[h] for h in select_reloc(cands, neighs, frame_id, map_id)]

    def close(self):
        if getattr(self, "handle", None):
            self.ctx.lib.osg_kfdb_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def complete_vocabulary(k, L, scoring=0, seed=5):
    """A complete k-ary vocabulary tree of L levels in breadth-first file order (k ** L words) with random
    descriptors and leaf weights, built without a Python loop over the nodes: 32 ** 4 words stand in for
    ORBvoc's 10 ** 6 where only the word count matters."""
    from .vocabulary import TF_IDF, Vocabulary
    rng = np.random.default_rng(seed)
    sizes = [k ** d for d in range(L + 1)]
    off = np.concatenate([[0], np.cumsum(sizes)])
    n = int(off[-1])
    parent = np.zeros(n, np.int32)
    for d in range(1, L + 1):
        parent[off[d]:off[d + 1]] = off[d - 1] + np.arange(sizes[d]) // k
    leaf = np.zeros(n, np.uint8)
    leaf[off[L]:] = 1
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    desc[0] = 0
    weight = np.where(leaf == 1, rng.uniform(0.5, 8.0, n), 0.0)
    return Vocabulary(k, L, scoring, TF_IDF, parent, leaf, desc, weight)


# ---- synthetic place-recognition sessions ------------------------------------------------------------
@dataclass
class PlaceDb:
    """A session for the database: KeyFrame i has BowVector (words[i], values[i]) and map map_id[i];
    neighbours[i] is its covisibility top-10 and connected[i] its connected set (KeyFrame indices)."""
    n_words: int
    words: list
    values: list
    map_id: np.ndarray
    place: np.ndarray
    neighbours: dict = field(default_factory=dict)
    connected: dict = field(default_factory=dict)


def synth_place_db(rng, n_kf=200, n_vocab_words=100000, words_per_kf=150, n_places=12, n_maps=2, overlap=0.7,
                   n_covis=10, n_connected=6) -> PlaceDb:
    """BowVectors generated directly, as sorted word subsets with L1-normalised weights: a trajectory that
    walks over ``n_places`` places and comes back to them, cut into ``n_maps`` maps.  A KeyFrame takes
    about ``overlap`` of its words from its place's pool and the rest at random; its covisibility top-10
    and connected set are its nearest KeyFrames along the trajectory inside its map."""
    pool = max(int(words_per_kf * 1.3), 1)
    pools = [np.sort(rng.choice(n_vocab_words, min(pool, n_vocab_words), replace=False)) for _ in range(n_places)]
    place = (np.arange(n_kf) * 3 // 7) % n_places        # slow walk that wraps around: revisits
    map_id = (np.arange(n_kf) * n_maps // max(n_kf, 1)).astype(np.int32)
    words, values = [], []
    for i in range(n_kf):
        n_own = min(int(round(words_per_kf * overlap)), len(pools[place[i]]))
        w = set(rng.choice(pools[place[i]], n_own, replace=False).tolist())
        while len(w) < min(words_per_kf, n_vocab_words):
            w.add(int(rng.integers(0, n_vocab_words)))
        w = np.array(sorted(w), np.int32)
        v = rng.uniform(0.2, 1.0, len(w))
        words.append(w)
        values.append(v / v.sum())
    db = PlaceDb(n_vocab_words, words, values, map_id, place)
    for i in range(n_kf):
        near = sorted((j for j in range(n_kf) if j != i and map_id[j] == map_id[i]), key=lambda j: (abs(j - i), j))
        db.neighbours[i] = near[:n_covis]
        db.connected[i] = set(near[:n_connected])
    return db
