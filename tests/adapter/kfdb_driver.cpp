// kfdb_driver.cpp — osg_orbslam3::KeyFrameDatabase on the mock KeyFrames of mock_kfdb.h
// (tests/test_adapter_kfdb.py), and the single-threaded CPU baseline of tools/kfdb_bench.py.
//
//   kfdb_driver session in out   a scripted session: "V.*" the vocabulary; KeyFrames "kf.id/map/bad",
//       BowVectors CSR "kf.bow_start/word/value", covisibility top-10 "kf.neigh_start/neigh" (KeyFrame
//       indices); "map.bad"; queries "q.id/map", "q.bow_start/word/value", "q.conn_start/conn"; operations
//       "op.kind" (0 add, 1 erase, 2 clear, 3 clearMap, 4 DetectNBestCandidates, 5
//       DetectRelocalizationCandidates), "op.arg" (KeyFrame index, map, or query index), "op.n".
//       out: per query "cand" {n_loop, ids.., n_merge, ids..} (reloc: {n, ids..}), "trace" {n_sharing, max,
//       min, n_scored}, "fields" the six fields of every KeyFrame as doubles.
//   kfdb_driver baseline in out  the reference's list walk and map merge on the CPU, one thread: "kf.*" as
//       above are added, then query 0 runs "reps" times with fresh ids; out: "ms" per repetition, "cand".
#include <chrono>
#include <list>

#include "driver_common.h"
#include "mock_kfdb.h"

using DB = osg_orbslam3::KeyFrameDatabase<mockdb::KeyFrame, mockdb::Frame, mockdb::Map>;

struct World {
    std::vector<mockdb::Map> maps;
    std::vector<mockdb::KeyFrame> kf;
    std::vector<mockdb::KeyFrame> qkf;  // the queries as KeyFrames (and as Frames: id and BowVector)
};

static void fill_bow(const Arrays &in, const std::string &pre, int i, std::map<unsigned int, double> &bow)
{
    const int32_t *bs = get(in, pre + "bow_start").p<int32_t>();
    for (int j = bs[i]; j < bs[i + 1]; j++)
        bow[(unsigned)get(in, pre + "word").p<int32_t>()[j]] = get(in, pre + "value").p<double>()[j];
}

static void build_world(const Arrays &in, World &W)
{
    const int nk = (int)get(in, "kf.id").n, nq = (int)get(in, "q.id").n, nm = (int)get(in, "map.bad").n;
    W.maps.resize(nm);
    for (int m = 0; m < nm; m++) W.maps[m].bad = get(in, "map.bad").p<uint8_t>()[m] != 0;
    W.kf.resize(nk);
    for (int i = 0; i < nk; i++) {
        mockdb::KeyFrame &k = W.kf[i];
        k.mnId = (unsigned long)get(in, "kf.id").p<int32_t>()[i];
        k.map = &W.maps[get(in, "kf.map").p<int32_t>()[i]];
        k.bad = get(in, "kf.bad").p<uint8_t>()[i] != 0;
        fill_bow(in, "kf.", i, k.mBowVec);
        const int32_t *ns = get(in, "kf.neigh_start").p<int32_t>();
        for (int j = ns[i]; j < ns[i + 1]; j++) k.covis.push_back(&W.kf[get(in, "kf.neigh").p<int32_t>()[j]]);
    }
    W.qkf.resize(nq);
    for (int i = 0; i < nq; i++) {
        mockdb::KeyFrame &k = W.qkf[i];
        k.mnId = (unsigned long)get(in, "q.id").p<int32_t>()[i];
        k.map = &W.maps[get(in, "q.map").p<int32_t>()[i]];
        fill_bow(in, "q.", i, k.mBowVec);
        const int32_t *cs = get(in, "q.conn_start").p<int32_t>();
        for (int j = cs[i]; j < cs[i + 1]; j++) k.connected.insert(&W.kf[get(in, "q.conn").p<int32_t>()[j]]);
    }
}

static int run_session(const Arrays &in, Arrays &out)
{
    World W;
    build_world(in, W);
    osg_vocabulary *voc = build_vocabulary(in);
    std::vector<int32_t> cand, trace;
    std::vector<double> fields;
    {
        DB db(voc);
        const int nops = (int)get(in, "op.kind").n;
        for (int o = 0; o < nops; o++) {
            const int kind = get(in, "op.kind").p<int32_t>()[o], arg = get(in, "op.arg").p<int32_t>()[o];
            if (kind == 0) db.add(&W.kf[arg]);
            else if (kind == 1) db.erase(&W.kf[arg]);
            else if (kind == 2) db.clear();
            else if (kind == 3) db.clearMap(&W.maps[arg]);
            else {
                if (kind == 4) {
                    std::vector<mockdb::KeyFrame *> loop, merge;
                    db.DetectNBestCandidates(&W.qkf[arg], loop, merge, get(in, "op.n").p<int32_t>()[o]);
                    cand.push_back((int32_t)loop.size());
                    for (auto *k : loop) cand.push_back((int32_t)k->mnId);
                    cand.push_back((int32_t)merge.size());
                    for (auto *k : merge) cand.push_back((int32_t)k->mnId);
                } else {
                    mockdb::Frame F;
                    F.mnId = W.qkf[arg].mnId;
                    F.mBowVec = W.qkf[arg].mBowVec;
                    const std::vector<mockdb::KeyFrame *> r = db.DetectRelocalizationCandidates(&F, W.qkf[arg].map);
                    cand.push_back((int32_t)r.size());
                    for (auto *k : r) cand.push_back((int32_t)k->mnId);
                }
                const osg_kfdb_query_out &l = db.last();
                trace.insert(trace.end(), {l.n_sharing, l.max_common_words, l.min_common_words, l.n_scored});
                for (const mockdb::KeyFrame &k : W.kf) {
                    fields.insert(fields.end(), {(double)k.mnPlaceRecognitionQuery, (double)k.mnPlaceRecognitionWords,
                                                 (double)k.mPlaceRecognitionScore, (double)k.mnRelocQuery,
                                                 (double)k.mnRelocWords, (double)k.mRelocScore});
                }
            }
        }
    }
    osg_vocabulary_destroy(voc);
    out["cand"] = make('i', cand);
    out["trace"] = make('i', trace);
    out["fields"] = make('d', fields);
    return 0;
}

// ---- the CPU baseline: ref:src/KeyFrameDatabase.cc:42-50, :669-880 and L1Scoring::score as the reference
// has them (an inverted file of std::list per word, std::map BowVectors merged with lower_bound), one thread
namespace cpu {
using KF = mockdb::KeyFrame;

static double l1_score(const std::map<unsigned int, double> &v1, const std::map<unsigned int, double> &v2)
{
    auto v1_it = v1.begin(), v2_it = v2.begin();
    double score = 0;
    while (v1_it != v1.end() && v2_it != v2.end()) {
        const double &vi = v1_it->second, &wi = v2_it->second;
        if (v1_it->first == v2_it->first) {
            score += fabs(vi - wi) - fabs(vi) - fabs(wi);
            ++v1_it;
            ++v2_it;
        } else if (v1_it->first < v2_it->first) {
            v1_it = v1.lower_bound(v2_it->first);
        } else {
            v2_it = v2.lower_bound(v1_it->first);
        }
    }
    return -score / 2.0;
}

struct Database {
    std::vector<std::list<KF *>> mvInvertedFile;
    explicit Database(size_t n_words) : mvInvertedFile(n_words) {}
    void add(KF *pKF)
    {
        for (const auto &kv : pKF->mBowVec) mvInvertedFile[kv.first].push_back(pKF);
    }
    void DetectNBestCandidates(KF *pKF, std::vector<KF *> &vpLoopCand, std::vector<KF *> &vpMergeCand, int nNumCandidates)
    {
        std::list<KF *> lKFsSharingWords;
        const std::set<KF *> spConnectedKF = pKF->GetConnectedKeyFrames();
        for (const auto &kv : pKF->mBowVec) {
            for (KF *pKFi : mvInvertedFile[kv.first]) {
                if (pKFi->mnPlaceRecognitionQuery != pKF->mnId) {
                    pKFi->mnPlaceRecognitionWords = 0;
                    if (!spConnectedKF.count(pKFi)) {
                        pKFi->mnPlaceRecognitionQuery = pKF->mnId;
                        lKFsSharingWords.push_back(pKFi);
                    }
                }
                pKFi->mnPlaceRecognitionWords++;
            }
        }
        if (lKFsSharingWords.empty()) return;
        int maxCommonWords = 0;
        for (KF *k : lKFsSharingWords)
            if (k->mnPlaceRecognitionWords > maxCommonWords) maxCommonWords = k->mnPlaceRecognitionWords;
        const int minCommonWords = maxCommonWords * 0.8f;
        std::list<std::pair<float, KF *>> lScoreAndMatch;
        for (KF *pKFi : lKFsSharingWords)
            if (pKFi->mnPlaceRecognitionWords > minCommonWords) {
                const float si = (float)l1_score(pKF->mBowVec, pKFi->mBowVec);
                pKFi->mPlaceRecognitionScore = si;
                lScoreAndMatch.push_back(std::make_pair(si, pKFi));
            }
        if (lScoreAndMatch.empty()) return;
        std::list<std::pair<float, KF *>> lAccScoreAndMatch;
        for (auto &sm : lScoreAndMatch) {
            KF *pKFi = sm.second;
            float bestScore = sm.first, accScore = bestScore;
            KF *pBestKF = pKFi;
            for (KF *pKF2 : pKFi->GetBestCovisibilityKeyFrames(10)) {
                if (pKF2->mnPlaceRecognitionQuery != pKF->mnId) continue;
                accScore += pKF2->mPlaceRecognitionScore;
                if (pKF2->mPlaceRecognitionScore > bestScore) {
                    pBestKF = pKF2;
                    bestScore = pKF2->mPlaceRecognitionScore;
                }
            }
            lAccScoreAndMatch.push_back(std::make_pair(accScore, pBestKF));
        }
        lAccScoreAndMatch.sort([](const std::pair<float, KF *> &a, const std::pair<float, KF *> &b) { return a.first > b.first; });
        std::set<KF *> spAlreadyAddedKF;
        for (auto it = lAccScoreAndMatch.begin(); it != lAccScoreAndMatch.end() &&
                                                  ((int)vpLoopCand.size() < nNumCandidates || (int)vpMergeCand.size() < nNumCandidates);
             ++it) {
            KF *pKFi = it->second;
            if (pKFi->isBad()) continue;  // the documented departure: skip and advance
            if (!spAlreadyAddedKF.count(pKFi)) {
                if (pKF->GetMap() == pKFi->GetMap() && (int)vpLoopCand.size() < nNumCandidates)
                    vpLoopCand.push_back(pKFi);
                else if (pKF->GetMap() != pKFi->GetMap() && (int)vpMergeCand.size() < nNumCandidates && !pKFi->GetMap()->IsBad())
                    vpMergeCand.push_back(pKFi);
                spAlreadyAddedKF.insert(pKFi);
            }
        }
    }
};
}  // namespace cpu

static int run_baseline(const Arrays &in, Arrays &out)
{
    World W;
    build_world(in, W);
    const int reps = get(in, "reps").p<int32_t>()[0], n_words = get(in, "n_words").p<int32_t>()[0];
    cpu::Database db((size_t)n_words);
    for (auto &k : W.kf) db.add(&k);
    std::vector<double> ms;
    std::vector<int32_t> cand;
    for (int r = 0; r < reps; r++) {
        W.qkf[0].mnId = 100000 + (unsigned long)r;
        std::vector<mockdb::KeyFrame *> loop, merge;
        const auto t0 = std::chrono::steady_clock::now();
        db.DetectNBestCandidates(&W.qkf[0], loop, merge, 3);
        ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
        if (r == reps - 1) {
            for (auto *k : loop) cand.push_back((int32_t)k->mnId);
            for (auto *k : merge) cand.push_back((int32_t)k->mnId);
        }
    }
    out["ms"] = make('d', ms);
    out["cand"] = make('i', cand);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc != 4) {
        std::fprintf(stderr, "usage: kfdb_driver session|baseline in out\n");
        return 2;
    }
    try {
        const Arrays in = read_arrays(argv[2]);
        Arrays out;
        const std::string mode = argv[1];
        const int rc = mode == "session" ? run_session(in, out) : mode == "baseline" ? run_baseline(in, out) : 2;
        if (rc) return rc;
        write_arrays(argv[3], out);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "kfdb_driver: %s\n", e.what());
        return 1;
    }
    return 0;
}
