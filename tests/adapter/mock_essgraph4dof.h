// mock_essgraph4dof.h — POD stand-ins with the member names Optimizer::OptimizeEssentialGraph4DoF reads and
// writes (ref:src/Optimizer.cc:4870-5198): Map, KeyFrame, MapPoint, g2o::Sim3 and the hook policy (test-only;
// tests/adapter/essgraph4dof_driver.cpp, tests/test_adapter_essgraph4dof.py).
#ifndef OSG_MOCK_ESSGRAPH4DOF_H
#define OSG_MOCK_ESSGRAPH4DOF_H
#include <cmath>
#include <cstring>
#include <map>
#include <mutex>
#include <set>
#include <utility>
#include <vector>

namespace mockeg4 {

struct Sim3 {  // g2o::Sim3's members
    double r[4] = {0, 0, 0, 1}, t[3] = {0, 0, 0}, s = 1;
};

struct KeyFrame {
    unsigned long mnId = 0;
    bool bad = false;
    double pose[7] = {0, 0, 0, 1, 0, 0, 0};  // Tcw.cast<double>(): unit quaternion (x y z w), translation
    double imu_row[36] = {};                 // what ImuCamPose(pKF) reads, cast to double
    std::set<KeyFrame *> children, loop_edges;
    std::vector<std::pair<KeyFrame *, int>> covis;  // by decreasing weight
    KeyFrame *mPrevKF = nullptr, *mNextKF = nullptr;
    // what SetPose received
    int n_set_pose = 0;
    float set_q[4] = {0, 0, 0, 0}, set_t[3] = {0, 0, 0};

    bool isBad() const { return bad; }
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
    KeyFrame *ref = nullptr;
    int n_update = 0, n_set_pos = 0;
    bool isBad() const { return bad; }
    KeyFrame *GetReferenceKeyFrame() const { return ref; }
    void UpdateNormalAndDepth() { n_update++; }
};

struct Map {
    std::vector<KeyFrame *> kfs;
    std::vector<MapPoint *> mps;
    unsigned long max_kf_id = 0;
    std::mutex mMutexMapUpdate;
    int change_index = 0;
    bool locked_at_change = false;
    std::vector<KeyFrame *> GetAllKeyFrames() const { return kfs; }
    std::vector<MapPoint *> GetAllMapPoints() const { return mps; }
    unsigned long GetMaxKFid() const { return max_kf_id; }
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
    static void kf_imu_cam_pose(KeyFrame *k, double row[36]) { std::memcpy(row, k->imu_row, sizeof k->imu_row); }
    // a rotation matrix's quaternion by the trace or the largest diagonal entry (Shepperd's choice), (x y z w)
    static void rot_to_quat(const double R[9], double q[4])
    {
        double t = R[0] + R[4] + R[8];
        if (t > 0) {
            t = std::sqrt(t + 1.0);
            q[3] = 0.5 * t;
            t = 0.5 / t;
            q[0] = (R[7] - R[5]) * t;
            q[1] = (R[2] - R[6]) * t;
            q[2] = (R[3] - R[1]) * t;
        } else {
            int i = 0;
            if (R[4] > R[0]) i = 1;
            if (R[8] > R[4 * i]) i = 2;
            const int j = (i + 1) % 3, k = (j + 1) % 3;
            t = std::sqrt(R[4 * i] - R[4 * j] - R[4 * k] + 1.0);
            q[i] = 0.5 * t;
            t = 0.5 / t;
            q[3] = (R[3 * k + j] - R[3 * j + k]) * t;
            q[j] = (R[3 * j + i] + R[3 * i + j]) * t;
            q[k] = (R[3 * k + i] + R[3 * i + k]) * t;
        }
    }
    // SE3d(q, t).cast<float>(): the quaternion normalised in double, then both cast
    static void kf_set_pose_se3d(KeyFrame *k, const double q[4], const double t[3])
    {
        const double n = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
        for (int i = 0; i < 4; i++) k->set_q[i] = (float)(q[i] / n);
        for (int i = 0; i < 3; i++) k->set_t[i] = (float)t[i];
        k->n_set_pose++;
    }
    static void mp_world_pos(MapPoint *p, float x[3]) { std::memcpy(x, p->pos, 12); }
    static void mp_set_world_pos(MapPoint *p, const float x[3])
    {
        std::memcpy(p->pos, x, 12);
        p->n_set_pos++;
    }
};

}  // namespace mockeg4
#endif
