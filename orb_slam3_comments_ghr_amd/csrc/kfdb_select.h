// kfdb_select.h — step 3 of KeyFrameDatabase::DetectNBestCandidates (ref:src/KeyFrameDatabase.cc:778-880)
// and of DetectRelocalizationCandidates (:979-1030) over plain arrays: the covisibility groups of the
// scored KeyFrames, the sort, and the choice of candidates.
//
// The caller reads each scored KeyFrame's neighbours (GetBestCovisibilityKeyFrames(10)) from wherever its
// KeyFrames live and passes their query / score fields as they are after the query.  A neighbour counts
// when its query field equals the query's id, whether or not this call scored it: its score is then
// whatever an earlier call left (or 0 on a fresh KeyFrame), as in the reference.
//
// Host only; compiled by the library (kfdb.hip), the ORB-SLAM3 adapter and tests/host/kfdb_select.cpp.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <set>
#include <utility>
#include <vector>

#include "../../include/osg_dbow.h"

// lAccScoreAndMatch: per scored KeyFrame (accScore, pBestKF) in list order; returns bestAccScore
inline float osg_kfdb_groups(int32_t n, const osg_kfdb_kf *cand, const int32_t *n_neigh, const osg_kfdb_kf *neigh,
                             int64_t query_id, std::vector<std::pair<float, osg_kfdb_kf>> &groups)
{
    float best_acc = 0;
    groups.clear();
    groups.reserve(n > 0 ? n : 0);
    for (int32_t i = 0; i < n; i++) {
        float best_score = cand[i].score;
        float acc = best_score;
        osg_kfdb_kf best = cand[i];
        const int32_t nn = std::min<int32_t>(std::max<int32_t>(n_neigh ? n_neigh[i] : 0, 0), OSG_KFDB_MAX_NEIGH);
        for (int32_t j = 0; j < nn; j++) {
            const osg_kfdb_kf &k2 = neigh[(size_t)OSG_KFDB_MAX_NEIGH * i + j];
            if (k2.query != query_id) continue;
            acc += k2.score;
            if (k2.score > best_score) {
                best = k2;
                best_score = k2.score;
            }
        }
        groups.emplace_back(acc, best);
        if (acc > best_acc) best_acc = acc;
    }
    return best_acc;
}

// DetectNBestCandidates' tail: list::sort(compFirst) is a stable merge sort on float >, then the walk
// that fills the loop list (same map) and the merge list (another map that is not bad) up to
// n_candidates each.  Departure: a bad best KeyFrame is skipped and the walk advances
// (ref:src/KeyFrameDatabase.cc:854-855 `continue`s without advancing and would never return).
inline void osg_kfdb_nbest(int32_t n, const osg_kfdb_kf *cand, const int32_t *n_neigh, const osg_kfdb_kf *neigh,
                           int64_t query_id, int32_t query_map, int32_t n_candidates, std::vector<int32_t> &loop,
                           std::vector<int32_t> &merge)
{
    loop.clear();
    merge.clear();
    std::vector<std::pair<float, osg_kfdb_kf>> g;
    osg_kfdb_groups(n, cand, n_neigh, neigh, query_id, g);
    std::stable_sort(g.begin(), g.end(),
                     [](const std::pair<float, osg_kfdb_kf> &a, const std::pair<float, osg_kfdb_kf> &b) {
                         return a.first > b.first;
                     });
    std::set<int32_t> added;
    const size_t want = n_candidates > 0 ? (size_t)n_candidates : 0;
    for (size_t i = 0; i < g.size() && (loop.size() < want || merge.size() < want); i++) {
        const osg_kfdb_kf &k = g[i].second;
        if (k.bad) continue;
        if (!added.count(k.handle)) {
            if (query_map == k.map_id && loop.size() < want)
                loop.push_back(k.handle);
            else if (query_map != k.map_id && merge.size() < want && !k.map_bad)
                merge.push_back(k.handle);
            added.insert(k.handle);
        }
    }
}

// DetectRelocalizationCandidates' tail: no sort; accScore > 0.75f * bestAccScore in float, the map test,
// then the dedup set.
inline void osg_kfdb_reloc(int32_t n, const osg_kfdb_kf *cand, const int32_t *n_neigh, const osg_kfdb_kf *neigh,
                           int64_t query_id, int32_t map_id, std::vector<int32_t> &out)
{
    out.clear();
    std::vector<std::pair<float, osg_kfdb_kf>> g;
    const float best_acc = osg_kfdb_groups(n, cand, n_neigh, neigh, query_id, g);
    const float min_score = 0.75f * best_acc;
    std::set<int32_t> added;
    for (size_t i = 0; i < g.size(); i++) {
        if (g[i].first > min_score) {
            const osg_kfdb_kf &k = g[i].second;
            if (k.map_id != map_id) continue;
            if (!added.count(k.handle)) {
                out.push_back(k.handle);
                added.insert(k.handle);
            }
        }
    }
}
