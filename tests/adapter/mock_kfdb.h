// mock_kfdb.h — POD stand-ins with the member names KeyFrameDatabase reads and writes
// (ref:src/KeyFrameDatabase.cc:28-111, :669-880, :920-1031): Map, KeyFrame, Frame (test-only;
// tests/adapter/kfdb_driver.cpp, tests/test_adapter_kfdb.py).
#ifndef OSG_MOCK_KFDB_H
#define OSG_MOCK_KFDB_H
#include <map>
#include <set>
#include <vector>

namespace mockdb {

struct Map {
    bool bad = false;
    bool IsBad() const { return bad; }
};

struct KeyFrame {
    long unsigned int mnId = 0;
    std::map<unsigned int, double> mBowVec;  // DBoW2::BowVector
    Map *map = nullptr;
    bool bad = false;
    std::set<KeyFrame *> connected;
    std::vector<KeyFrame *> covis;  // by decreasing weight
    // ref:include/KeyFrame.h: the fields of the place-recognition and relocalisation queries
    long unsigned int mnPlaceRecognitionQuery = 0;
    int mnPlaceRecognitionWords = 0;
    float mPlaceRecognitionScore = 0;
    long unsigned int mnRelocQuery = 0;
    int mnRelocWords = 0;
    float mRelocScore = 0;

    Map *GetMap() const { return map; }
    bool isBad() const { return bad; }
    std::set<KeyFrame *> GetConnectedKeyFrames() const { return connected; }
    std::vector<KeyFrame *> GetBestCovisibilityKeyFrames(const int &N) const
    {
        if ((int)covis.size() < N) return covis;
        return std::vector<KeyFrame *>(covis.begin(), covis.begin() + N);
    }
};

struct Frame {
    long unsigned int mnId = 0;
    std::map<unsigned int, double> mBowVec;
};

}  // namespace mockdb
#endif
