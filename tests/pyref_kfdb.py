"""A literal restatement of KeyFrameDatabase (ref:src/KeyFrameDatabase.cc:28-111, :655-880, :920-1031) and
of L1Scoring::score (ref:Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68): the checker of csrc/kfdb.hip,
csrc/kfdb_select.h and the Python class.

It keeps a real inverted file (one Python list of KeyFrames per word), marks KeyFrames hit by hit while it
walks the query's words and each word's list, merges the two BowVectors with Python floats in the
reference's operand order, holds np.float32 wherever the reference holds a float, and sorts stably.  It
does not use the closed form of the marking that the device code relies on: that is what it checks.

``rules`` names the reference rules that a call switches OFF, so that a fixture can show it bites
(tests/kfdb_fixtures.py): the restatement with the rule off must return other candidates.
    stale        a neighbour counts only when this call scored it
    connected    GetConnectedKeyFrames is ignored
    strict       words >= minCommonWords (relocalisation: si >= 0.75f * best) instead of >
    trunc        minCommonWords is rounded to nearest instead of truncated
    order        the sharing list is taken in KeyFrame id order instead of first-visit order
    visited      every KeyFrame is treated as not yet visited by this query id
    dedup        no spAlreadyAddedKF
    badmap       a bad map's KeyFrames are merge candidates
    badkf        a bad best KeyFrame is taken (the reference neither takes nor passes it: see below)
    mapfilter    relocalisation returns KeyFrames of every map
    sort         no sort of the groups
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

F32 = np.float32


class KeyFrame:
    """The fields of ORB_SLAM3::KeyFrame the database reads and writes."""

    def __init__(self, kid, words, values, map_id=0):
        self.mnId = kid
        self.words = [int(w) for w in words]          # mBowVec, ascending
        self.values = [float(v) for v in values]
        self.map_id = map_id
        self.bad = False
        self.neighbours = []                          # GetBestCovisibilityKeyFrames(10)
        self.connected = set()                        # GetConnectedKeyFrames()
        self.mnPlaceRecognitionQuery = 0
        self.mnPlaceRecognitionWords = 0
        self.mPlaceRecognitionScore = F32(0)
        self.mnRelocQuery = 0
        self.mnRelocWords = 0
        self.mRelocScore = F32(0)

    def fields(self):
        return (self.mnPlaceRecognitionQuery, self.mnPlaceRecognitionWords, F32(self.mPlaceRecognitionScore),
                self.mnRelocQuery, self.mnRelocWords, F32(self.mRelocScore))

    def __repr__(self):
        return f"KF{self.mnId}"


def l1_score(v1w, v1v, v2w, v2v):
    """L1Scoring::score(v1, v2) as a double; lower_bound moves are plain steps on sorted lists."""
    i = j = 0
    score = 0.0
    while i < len(v1w) and j < len(v2w):
        if v1w[i] == v2w[j]:
            vi, wi = v1v[i], v2v[j]
            score += abs(vi - wi) - abs(vi) - abs(wi)
            i += 1
            j += 1
        elif v1w[i] < v2w[j]:
            while i < len(v1w) and v1w[i] < v2w[j]:
                i += 1
        else:
            while j < len(v2w) and v2w[j] < v1w[i]:
                j += 1
    return -score / 2.0


@dataclass
class Trace:
    """What steps 1 and 2 leave: the figures osg_kfdb_query returns."""
    n_sharing: int = 0
    max_common_words: int = 0
    min_common_words: int = 0
    scored: list = field(default_factory=list)        # (KeyFrame, words, np.float32 si, float double)
    groups: list = field(default_factory=list)        # (np.float32 accScore, best KeyFrame), after the sort


class KeyFrameDatabase:
    def __init__(self, n_words):
        self.n_words = n_words
        self.mvInvertedFile = {}                      # word -> list of KeyFrames (an empty list is absent)
        self.bad_maps = set()

    # ---- ref:src/KeyFrameDatabase.cc:42-111
    def add(self, kf):
        for w in kf.words:
            self.mvInvertedFile.setdefault(w, []).append(kf)

    def erase(self, kf):
        for w in kf.words:
            l = self.mvInvertedFile.get(w, [])
            for k, x in enumerate(l):
                if x is kf:
                    del l[k]
                    break

    def clear(self):
        self.mvInvertedFile = {}

    def clear_map(self, map_id):
        for w, l in self.mvInvertedFile.items():
            l[:] = [x for x in l if x.map_id != map_id]

    def size(self):
        return len({id(x) for l in self.mvInvertedFile.values() for x in l})

    # ---- steps 1 and 2
    def _share_and_score(self, words, values, qid, connected, place, rules, t):
        Q, W, S = (("mnPlaceRecognitionQuery", "mnPlaceRecognitionWords", "mPlaceRecognitionScore") if place else
                   ("mnRelocQuery", "mnRelocWords", "mRelocScore"))
        if "connected" in rules:
            connected = set()
        lKFsSharingWords = []
        fresh = set()
        for w in words:
            for pKFi in self.mvInvertedFile.get(w, []):
                visited = getattr(pKFi, Q) == qid
                if "visited" in rules:
                    visited = id(pKFi) in fresh
                if not visited:
                    setattr(pKFi, W, 0)
                    if not place or pKFi not in connected:
                        setattr(pKFi, Q, qid)
                        fresh.add(id(pKFi))
                        lKFsSharingWords.append(pKFi)
                setattr(pKFi, W, getattr(pKFi, W) + 1)
        if "order" in rules:
            lKFsSharingWords.sort(key=lambda k: k.mnId)
        t.n_sharing = len(lKFsSharingWords)
        if not lKFsSharingWords:
            return False
        maxCommonWords = 0
        for k in lKFsSharingWords:
            if getattr(k, W) > maxCommonWords:
                maxCommonWords = getattr(k, W)
        minCommonWords = int(F32(maxCommonWords) * F32(0.8))
        if "trunc" in rules:
            minCommonWords = int(round(float(F32(maxCommonWords) * F32(0.8))))
        t.max_common_words, t.min_common_words = maxCommonWords, minCommonWords
        for pKFi in lKFsSharingWords:
            n = getattr(pKFi, W)
            if n > minCommonWords or ("strict" in rules and n >= minCommonWords):
                d = l1_score(words, values, pKFi.words, pKFi.values)
                si = F32(d)
                setattr(pKFi, S, si)
                t.scored.append((pKFi, n, si, d))
        return bool(t.scored)

    def _groups(self, t, qid, place, rules):
        Q, S = ("mnPlaceRecognitionQuery", "mPlaceRecognitionScore") if place else ("mnRelocQuery", "mRelocScore")
        scored_now = {id(k) for k, _, _, _ in t.scored}
        lAcc = []
        bestAccScore = F32(0)
        for pKFi, _, si, _ in t.scored:
            bestScore = F32(si)
            accScore = F32(si)
            pBestKF = pKFi
            for pKF2 in pKFi.neighbours[:10]:
                if getattr(pKF2, Q) != qid:
                    continue
                if "stale" in rules and id(pKF2) not in scored_now:
                    continue
                s2 = F32(getattr(pKF2, S))
                accScore = F32(accScore + s2)
                if s2 > bestScore:
                    pBestKF = pKF2
                    bestScore = s2
            lAcc.append((accScore, pBestKF))
            if accScore > bestAccScore:
                bestAccScore = accScore
        return lAcc, bestAccScore

    # ---- ref:src/KeyFrameDatabase.cc:669-880
    def detect_n_best_candidates(self, kf, n=3, rules=()):
        """-> (vpLoopCand, vpMergeCand, Trace).  ``kf`` has mnId, words, values, map_id and connected.

        ref:src/KeyFrameDatabase.cc:854-855 ``continue``s on a bad KeyFrame without advancing the
        iterator, so the reference never returns once it meets one.  The documented variant here, which the
        product follows: the bad KeyFrame is skipped and the walk advances."""
        t = Trace()
        if not self._share_and_score(kf.words, kf.values, kf.mnId, kf.connected, True, rules, t):
            return [], [], t
        lAcc, _ = self._groups(t, kf.mnId, True, rules)
        if "sort" not in rules:
            lAcc = sorted(lAcc, key=lambda p: -float(p[0]))   # stable; float32 -> float is exact
        t.groups = lAcc
        loop, merge, added = [], [], set()
        i = 0
        while i < len(lAcc) and (len(loop) < n or len(merge) < n):
            pKFi = lAcc[i][1]
            if pKFi.bad and "badkf" not in rules:
                i += 1
                continue
            if id(pKFi) not in added or "dedup" in rules:
                if kf.map_id == pKFi.map_id and len(loop) < n:
                    loop.append(pKFi)
                elif (kf.map_id != pKFi.map_id and len(merge) < n and
                      (pKFi.map_id not in self.bad_maps or "badmap" in rules)):
                    merge.append(pKFi)
                added.add(id(pKFi))
            i += 1
        return loop, merge, t

    # ---- ref:src/KeyFrameDatabase.cc:920-1031
    def detect_relocalization_candidates(self, words, values, frame_id, map_id, rules=()):
        """-> (vpRelocCandidates, Trace)"""
        t = Trace()
        if not self._share_and_score(words, values, frame_id, set(), False, rules, t):
            return [], t
        lAcc, bestAccScore = self._groups(t, frame_id, False, rules)
        t.groups = lAcc
        minScoreToRetain = F32(F32(0.75) * bestAccScore)
        out, added = [], set()
        for si, pKFi in lAcc:
            if si > minScoreToRetain or ("strict" in rules and si >= minScoreToRetain):
                if pKFi.map_id != map_id and "mapfilter" not in rules:
                    continue
                if id(pKFi) not in added or "dedup" in rules:
                    out.append(pKFi)
                    added.add(id(pKFi))
        return out, t
