// mock_localmapping.h — what the CreateNewMapPoints adapter needs beyond mock_orbslam3.h (test-only): a KeyFrame
// with the members LocalMapping::CreateNewMapPoints reads (ref:include/KeyFrame.h), a MapPoint that counts what
// is done to it, and a LocalMapping whose CreateNewMapPoints is the body of adapters/orbslam3/LocalMapping_osg.cc
// on these types.  Geometry the reference takes from Sophus / Eigen is stored on the objects and returned by the
// hooks.
#pragma once
#include <algorithm>
#include <list>

#include "mock_orbslam3.h"

struct LmKeyFrame : mock::KeyFrame {
    std::vector<float> mvDepth;
    float invfx = 0, invfy = 0, mfScaleFactor = 1.2f;
    LmKeyFrame *mPrevKF = nullptr;
    std::vector<LmKeyFrame *> covisible;  // test-only: the covisibility order
    std::vector<float> scene_depths;      // test-only: the MapPoint depths ComputeSceneMedianDepth sorts
    osg_np_kf geometry{};                 // test-only: LmHooks::np_kf
    osg_triang_geom pair_geometry{};      // test-only: LmHooks::triang_geom of (current KeyFrame, this)
    std::vector<LmKeyFrame *> GetBestCovisibilityKeyFrames(const int &N)
    {  // ref:src/KeyFrame.cc:334-343
        if ((int)covisible.size() < N) return covisible;
        return std::vector<LmKeyFrame *>(covisible.begin(), covisible.begin() + N);
    }
    float ComputeSceneMedianDepth(const int q)
    {  // ref:src/KeyFrame.cc:944-986: sort, vDepths[(size - 1) / q]
        std::vector<float> v = scene_depths;
        if (v.empty()) return -1.0f;
        std::sort(v.begin(), v.end());
        return v[(v.size() - 1) / q];
    }
};

struct LmMapPoint : mock::MapPoint {
    float x3d[3] = {0, 0, 0};
    LmKeyFrame *ref_kf = nullptr;
    int n_distinctive = 0, n_update = 0;
    std::vector<std::pair<mock::KeyFrame *, int>> added;  // AddObservation calls in order
    void AddObservation(mock::KeyFrame *k, int idx)
    {
        added.emplace_back(k, idx);
        mock::MapPoint::AddObservation(k, idx);
    }
    void ComputeDistinctiveDescriptors() { n_distinctive++; }
    void UpdateNormalAndDepth() { n_update++; }
};

struct LmHooks : mock::MockHooks {
    static void np_kf(LmKeyFrame *p, osg_np_kf &k) { k = p->geometry; }
    static void triang_geom(LmKeyFrame *, LmKeyFrame *pKF2, osg_triang_geom &g) { g = pKF2->pair_geometry; }
};

struct LmAtlas {
    std::vector<LmMapPoint *> points;
    void AddMapPoint(LmMapPoint *p) { points.push_back(p); }
};

struct LocalMappingMock {
    LmKeyFrame *mpCurrentKeyFrame = nullptr;
    bool mbMonocular = false, mbInertial = false, mbFarPoints = false, coarse = false, new_keyframes = false;
    float mThFarPoints = 0;
    int n_checks = 0;
    LmAtlas atlas, *mpAtlas = &atlas;
    std::list<LmMapPoint *> mlpRecentAddedMapPoints;
    std::vector<std::unique_ptr<LmMapPoint>> pool;
    bool CheckNewKeyFrames()
    {
        n_checks++;
        return new_keyframes;
    }
    int CreateNewMapPoints()
    {  // adapters/orbslam3/LocalMapping_osg.cc
        const bool bNewKeyFrames = CheckNewKeyFrames();
        return osg_orbslam3::create_new_map_points<LmHooks, LmKeyFrame>(
            mpCurrentKeyFrame, mbMonocular, mbInertial, coarse, mbFarPoints, mThFarPoints, bNewKeyFrames,
            [&](LmKeyFrame *pKF2, int idx1, int idx2, const float *x) {
                pool.emplace_back(new LmMapPoint());
                LmMapPoint *pMP = pool.back().get();
                pMP->mnId = pool.size() - 1;
                std::copy(x, x + 3, pMP->x3d);
                pMP->ref_kf = mpCurrentKeyFrame;
                pMP->AddObservation(mpCurrentKeyFrame, idx1);
                pMP->AddObservation(pKF2, idx2);
                mpCurrentKeyFrame->AddMapPoint(pMP, idx1);
                pKF2->AddMapPoint(pMP, idx2);
                pMP->ComputeDistinctiveDescriptors();
                pMP->UpdateNormalAndDepth();
                mpAtlas->AddMapPoint(pMP);
                mlpRecentAddedMapPoints.push_back(pMP);
            });
    }
};
