// mock_preintegration.h — Tracking, Frame, KeyFrame, IMU::Point and IMU::Preintegrated as far as
// osg_orbslam3::preintegrate_imu, reintegrate_keyframes and merge_previous use them (test-only;
// tests/adapter/preintegration_driver.cpp).  Float where the reference stores float.
#pragma once
#include <cstring>
#include <list>
#include <mutex>
#include <vector>

#include "../../include/osg_imu.h"

namespace mockimu {

struct Point {
    float a[3], w[3];
    double t;
};

// IMU::Preintegrated: the stored fields as the ABI lays them out, Nga / NgaWalk, bu, db and mvMeasurements
struct Preintegrated {
    osg_imu_preintegrated st{};
    float nga[6] = {}, walk[6] = {}, bu[6] = {}, db[6] = {};
    std::vector<float> meas;          // 7 floats per step
    static inline int live = 0;       // test-only: constructed minus destroyed
    Preintegrated(const float b[6], const float nga_[6], const float walk_[6])
    {
        live++;
        std::memcpy(nga, nga_, sizeof nga);
        std::memcpy(walk, walk_, sizeof walk);
        Initialize(b);
    }
    ~Preintegrated() { live--; }
    void Initialize(const float b[6])  // ref:src/ImuTypes.cc:206-225
    {
        st = osg_imu_preintegrated{};
        st.pre.dR[0] = st.pre.dR[4] = st.pre.dR[8] = 1.f;
        std::memcpy(st.pre.b, b, sizeof st.pre.b);
        std::memcpy(bu, b, sizeof bu);
        std::memset(db, 0, sizeof db);
        meas.clear();
    }
    void SetNewBias(const float b[6])  // ref:src/ImuTypes.cc:358-369: db = (dbg, dba)
    {
        std::memcpy(bu, b, sizeof bu);
        for (int i = 0; i < 3; i++) db[i] = b[3 + i] - st.pre.b[3 + i], db[3 + i] = b[i] - st.pre.b[i];
    }
};

struct KeyFrame {
    float bias[6] = {};               // (ba, bg)
    Preintegrated *mpImuPreintegrated = nullptr;
};

struct Frame {
    double mTimeStamp = 0;
    Frame *mpPrevFrame = nullptr;
    float bias[6] = {};               // mImuBias
    float nga[6] = {}, walk[6] = {};  // mImuCalib.Cov / CovWalk
    Preintegrated *mpImuPreintegrated = nullptr, *mpImuPreintegratedFrame = nullptr;
    KeyFrame *mpLastKeyFrame = nullptr;
    bool integrated = false;
    void setIntegrated() { integrated = true; }
};

struct Tracking {
    Frame mCurrentFrame, mLastFrame;
    std::list<Point> mlQueueImuData;
    std::vector<Point> mvImuFromLastFrame;
    std::mutex mMutexImuQueue;
    double mImuPer = 0.001;
    Preintegrated *mpImuPreintegratedFromLastKF = nullptr;
    KeyFrame *mpLastKeyFrame = nullptr;
};

struct Hooks {
    static void imu_point(const Point &m, float a[3], float w[3], double &t)
    {
        std::memcpy(a, m.a, 12), std::memcpy(w, m.w, 12);
        t = m.t;
    }
    static void frame_bias(const Frame &F, float b[6]) { std::memcpy(b, F.bias, 24); }
    static Preintegrated *new_preintegrated(const Frame &last, const Frame &cur)
    {
        return new Preintegrated(last.bias, cur.nga, cur.walk);
    }
    static void preint_get(const Preintegrated *p, osg_imu_preintegrated &st, float nga[6], float walk[6], float bu[6])
    {
        st = p->st;
        std::memcpy(nga, p->nga, 24), std::memcpy(walk, p->walk, 24), std::memcpy(bu, p->bu, 24);
    }
    static void preint_measurements(const Preintegrated *p, std::vector<float> &out)
    {
        out.insert(out.end(), p->meas.begin(), p->meas.end());
    }
    static void preint_continue(Preintegrated *p, const osg_imu_preintegrated &st, const float *meas, int n)
    {
        p->st = st;
        p->meas.insert(p->meas.end(), meas, meas + 7 * (size_t)n);
    }
    static void preint_restart(Preintegrated *p, const osg_imu_preintegrated &st, const float *meas, int n)
    {
        const std::vector<float> list(meas, meas + 7 * (size_t)n);  // meas may alias p->meas
        p->Initialize(st.pre.b);
        p->st = st;
        p->meas = list;
    }
    static void gyro_bias(const KeyFrame &K, float g[3]) { std::memcpy(g, K.bias + 3, 12); }
    static void set_new_bias(KeyFrame &K, const float b[6])  // KeyFrame::SetNewBias
    {
        std::memcpy(K.bias, b, 24);
        if (K.mpImuPreintegrated) K.mpImuPreintegrated->SetNewBias(b);
    }
};

}  // namespace mockimu
