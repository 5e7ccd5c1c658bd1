// mock_essgraph.h — POD stand-ins with the member names Optimizer::OptimizeEssentialGraph reads and writes
// (ref:src/Optimizer.cc:4527-4858): Map, KeyFrame, MapPoint, g2o::Sim3 and the hook policy (test-only;
// tests/adapter/essgraph_driver.cpp, tests/test_adapter_essgraph.py).
#ifndef OSG_MOCK_ESSGRAPH_H
#define OSG_MOCK_ESSGRAPH_H
#include <cstring>
#include <map>
#include <mutex>
#include <set>
#include <utility>
#include <vector>

namespace mockeg {

struct Sim3 {  // g2o::Sim3's members
    double r[4] = {0, 0, 0, 1}, t[3] = {0, 0, 0}, s = 1;
};

struct Map;

struct KeyFrame {
    unsigned long mnId = 0;
    bool bad = false;
    double pose[7] = {0, 0, 0, 1, 0, 0, 0};  // Tcw: unit quaternion (x y z w), translation
    KeyFrame *parent = nullptr;
    std::set<KeyFrame *> children, loop_edges;
    std::vector<std::pair<KeyFrame *, int>> covis;  // by decreasing weight
    bool bImu = false;
    KeyFrame *mPrevKF = nullptr;
    // what SetPose received
    int n_set_pose = 0;
    float set_q[4] = {0, 0, 0, 0}, set_t[3] = {0, 0, 0};

    bool isBad() const { return bad; }
    KeyFrame *GetParent() const { return parent; }
    bool hasChild(KeyFrame *k) const { return children.count(k) != 0; }
    std::set<KeyFrame *> GetLoopEdges() const { return loop_edges; }
    std::vector<KeyFrame *> GetCovisiblesByWeight(int w) const
    {
        std::vector<KeyFrame *> v;
        for (const auto &c : covis)
            if (c.second >= w) v.push_back(c.first);
        return v;
    }
    int GetWeight(KeyFrame *k) const
    {
        for (const auto &c : covis)
            if (c.first == k) return c.second;
        return 0;
    }
};

struct MapPoint {
    bool bad = false;
    float pos[3] = {0, 0, 0};
    unsigned long mnCorrectedByKF = 0, mnCorrectedReference = 0;
    KeyFrame *ref = nullptr;
    int n_update = 0, n_set_pos = 0;
    bool isBad() const { return bad; }
    KeyFrame *GetReferenceKeyFrame() const { return ref; }
    void UpdateNormalAndDepth() { n_update++; }
};

struct Map {
    std::vector<KeyFrame *> kfs;
    std::vector<MapPoint *> mps;
    unsigned long max_kf_id = 0, init_kf_id = 0;
    std::mutex mMutexMapUpdate;
    int change_index = 0;
    bool locked_at_change = false;
    std::vector<KeyFrame *> GetAllKeyFrames() const { return kfs; }
    std::vector<MapPoint *> GetAllMapPoints() const { return mps; }
    unsigned long GetMaxKFid() const { return max_kf_id; }
    unsigned long GetInitKFid() const { return init_kf_id; }
    void IncreaseChangeIndex()
    {
        change_index++;
        locked_at_change = !mMutexMapUpdate.try_lock();  // the write-back runs under the lock
        if (!locked_at_change) mMutexMapUpdate.unlock();
    }
};

using KeyFrameAndPose = std::map<KeyFrame *, Sim3>;
using LoopConnections = std::map<KeyFrame *, std::set<KeyFrame *>>;

struct Hooks {
    static void sim3_get(const Sim3 &S, double q[4], double t[3], double &s)
    {
        std::memcpy(q, S.r, sizeof S.r);
        std::memcpy(t, S.t, sizeof S.t);
        s = S.s;
    }
    static void kf_pose_sim3(KeyFrame *k, double q[4], double t[3])
    {
        std::memcpy(q, k->pose, 32);
        std::memcpy(t, k->pose + 4, 24);
    }
    // SE3f(r.cast<float>(), t.cast<float>() / s): Eigen divides the float vector by s converted to float
    static void kf_set_pose_sim3(KeyFrame *k, const double q[4], const double t[3], double s)
    {
        for (int i = 0; i < 4; i++) k->set_q[i] = (float)q[i];
        for (int i = 0; i < 3; i++) k->set_t[i] = (float)t[i] / (float)s;
        k->n_set_pose++;
    }
    static void mp_world_pos(MapPoint *p, float x[3]) { std::memcpy(x, p->pos, 12); }
    static void mp_set_world_pos(MapPoint *p, const float x[3])
    {
        std::memcpy(p->pos, x, 12);
        p->n_set_pos++;
    }
};

}  // namespace mockeg
#endif
