// mock_localinertialba.h — Map, KeyFrame, MapPoint and the hooks as far as osg_orbslam3::local_inertial_ba /
// apply_local_inertial_ba use them (test-only; tests/adapter/localinertialba_driver.cpp).  The KeyFrames of a test
// live in one array, so the pointer order of a MapPoint's observations map is their index order.  The preintegration
// is mock_preintegration.h's.  Float where the reference stores float.
#pragma once
#include <map>
#include <tuple>
#include <utility>

#include "mock_preintegration.h"

namespace mockliba {

using mockimu::Preintegrated;

struct KeyFrame;

struct Map {
    long n_kfs = 0;
    int change_index = 0;
    long KeyFramesInMap() const { return n_kfs; }
    void IncreaseChangeIndex() { change_index++; }
};

struct MapPoint {
    float pos[3] = {};
    float mTrackDepth = 0.f;
    bool bad = false;
    unsigned long mnBALocalForKF = 0;
    std::map<KeyFrame *, std::tuple<int, int>> obs;
    int pos_writes = 0, normal_updates = 0;  // test-only
    bool isBad() const { return bad; }
    std::map<KeyFrame *, std::tuple<int, int>> GetObservations() const { return obs; }
};

struct KeyFrame {
    unsigned long mnId = 0, mnBALocalForKF = 0, mnBAFixedForKF = 0;
    KeyFrame *mPrevKF = nullptr;
    bool bad = false, bImu = true, mpCamera2 = false;
    Map *map = nullptr;
    Preintegrated *mpImuPreintegrated = nullptr;
    osg_liba_keyframe raw{};          // the state (float-valued doubles) and ImuCamPose(KeyFrame*)'s cameras
    std::vector<MapPoint *> matches;  // GetMapPointMatches(), with null slots
    std::vector<float> un, right, mvuRight, mvInvLevelSigma2;  // (x, y, octave) per left key | (x, y) per right key
    int NLeft = 0;
    float unc2 = 1.f;
    // what the write-back left (test-only)
    float pose_R[9] = {}, pose_t[3] = {}, vel[3] = {}, bias[6] = {};
    int pose_writes = 0, velocity_writes = 0, bias_writes = 0;
    Map *GetMap() const { return map; }
    bool isBad() const { return bad; }
    const std::vector<MapPoint *> &GetMapPointMatches() const { return matches; }
};

inline std::vector<std::pair<int, MapPoint *>> &erased()  // test-only: (KeyFrame mnId, point) in call order
{
    static std::vector<std::pair<int, MapPoint *>> v;
    return v;
}

struct Hooks : mockimu::Hooks {
    static void imu_state(const KeyFrame &K, osg_pio_state &s) { s = K.raw.state; }
    static void liba_cameras(const KeyFrame &K, osg_liba_keyframe &k)
    {
        k.n_cams = K.raw.n_cams, k.bf = K.raw.bf;
        k.cams[0] = K.raw.cams[0], k.cams[1] = K.raw.cams[1];
    }
    static void preint_take_prev_bias(KeyFrame &K)
    {
        float b[6];
        for (int i = 0; i < 3; i++) b[i] = (float)K.mPrevKF->raw.state.ba[i], b[3 + i] = (float)K.mPrevKF->raw.state.bg[i];
        K.mpImuPreintegrated->SetNewBias(b);
    }
    static void preintegrated(const Preintegrated *p, osg_pio_preintegrated &q) { q = p->st.pre; }
    static void keypoint_un(const KeyFrame &K, int i, float xy[2], int &octave)
    {
        xy[0] = K.un[3 * i], xy[1] = K.un[3 * i + 1], octave = (int)K.un[3 * i + 2];
    }
    static void keypoint_right(const KeyFrame &K, int i, float xy[2]) { xy[0] = K.right[2 * i], xy[1] = K.right[2 * i + 1]; }
    static float uncertainty2(const KeyFrame &K, float, float) { return K.unc2; }
    static void mp_world_pos(const MapPoint *p, float x[3]) { std::memcpy(x, p->pos, 12); }
    static float track_depth(const MapPoint *p) { return p->mTrackDepth; }
    static void mp_set_world_pos(MapPoint *p, const float x[3])
    {
        std::memcpy(p->pos, x, 12);
        p->pos_writes++;
    }
    static void mp_update_normal_and_depth(MapPoint *p) { p->normal_updates++; }
    static void kf_set_pose_rt(KeyFrame &K, const float R[9], const float t[3])
    {
        std::memcpy(K.pose_R, R, 36), std::memcpy(K.pose_t, t, 12);
        K.pose_writes++;
    }
    static void set_velocity(KeyFrame &K, const double v[3])
    {
        for (int i = 0; i < 3; i++) K.vel[i] = (float)v[i];
        K.velocity_writes++;
    }
    static void set_new_bias(KeyFrame &K, const float b[6])
    {
        std::memcpy(K.bias, b, 24);
        K.bias_writes++;
    }
    static void erase_match(KeyFrame *K, MapPoint *p)
    {
        erased().push_back(std::make_pair((int)K->mnId, p));
        p->obs.erase(K);
    }
};

}  // namespace mockliba
