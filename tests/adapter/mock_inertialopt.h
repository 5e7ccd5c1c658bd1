// mock_inertialopt.h — KeyFrame and the hooks as far as osg_orbslam3::inertial_optimization_init / _bias / _scale use
// them (test-only; tests/adapter/inertialopt_driver.cpp).  The preintegration is mock_preintegration.h's.  Float where
// the reference stores float.
#pragma once
#include "mock_preintegration.h"

namespace mockio {

using mockimu::Preintegrated;

struct KeyFrame {
    unsigned long mnId = 0;
    KeyFrame *mPrevKF = nullptr;
    bool bad = false;
    float Rwb[9] = {}, twb[3] = {}, vel[3] = {};
    float bias[6] = {};               // (ba, bg)
    Preintegrated *mpImuPreintegrated = nullptr;
    int velocity_writes = 0, bias_writes = 0;  // test-only
};

struct Hooks : mockimu::Hooks {
    static void imu_state(const KeyFrame &K, osg_pio_state &s)
    {
        for (int i = 0; i < 9; i++) s.Rwb[i] = (double)K.Rwb[i];
        for (int i = 0; i < 3; i++) {
            s.twb[i] = (double)K.twb[i], s.v[i] = (double)K.vel[i];
            s.bg[i] = (double)K.bias[3 + i], s.ba[i] = (double)K.bias[i];
        }
    }
    static void preintegrated(const Preintegrated *p, osg_pio_preintegrated &q) { q = p->st.pre; }
    static bool is_bad(const KeyFrame &K) { return K.bad; }
    static void set_velocity(KeyFrame &K, const double v[3])
    {
        for (int i = 0; i < 3; i++) K.vel[i] = (float)v[i];
        K.velocity_writes++;
    }
    static void gyro_bias(const KeyFrame &K, float g[3]) { std::memcpy(g, K.bias + 3, 12); }
    static void set_new_bias(KeyFrame &K, const float b[6])
    {
        std::memcpy(K.bias, b, 24);
        K.bias_writes++;
        if (K.mpImuPreintegrated) K.mpImuPreintegrated->SetNewBias(b);
    }
};

}  // namespace mockio
