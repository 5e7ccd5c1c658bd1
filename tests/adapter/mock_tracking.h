// mock_tracking.h — what the SearchLocalPoints adapter needs beyond mock_orbslam3.h (test-only): a MapPoint with
// the members Tracking::SearchLocalPoints and Frame::isInFrustum touch (ref:include/MapPoint.h), a Frame with
// mnId, mmProjectPoints and slots of that MapPoint type, and a Tracking whose SearchLocalPoints is the body of
// adapters/orbslam3/Tracking_osg.cc on these types.  Geometry the reference takes from Sophus / Eigen is stored on
// the objects and returned by the hooks.
#pragma once
#include <map>

#include "mock_orbslam3.h"

struct TrMapPoint : mock::MapPoint {
    unsigned long mnLastFrameSeen = 0;
    int mnVisible = 1;
    float world[3] = {0, 0, 0}, normal[3] = {0, 0, 0};  // GetWorldPos(), GetNormal()
    float mfMaxDistance = 0, mfMinDistance = 0;
    void IncreaseVisible(int n = 1) { mnVisible += n; }
};

struct TrFrame : mock::Frame {
    unsigned long mnId = 0;
    std::vector<TrMapPoint *> mvpMapPoints;  // in place of the base's: SearchLocalPoints marks these MapPoints
    std::map<unsigned long, cv::Point2f> mmProjectPoints;
    float mfLogScaleFactor = 0;
    osg_frustum_frame frustum{};  // test-only: TrHooks::frustum_frame
};

struct TrHooks : mock::MockHooks {
    static void frustum_frame(TrFrame &F, osg_frustum_frame &f) { f = F.frustum; }
    static void mp_frustum(TrMapPoint *p, float pos[3], float normal[3], float &max_dist, float &min_dist)
    {
        for (int k = 0; k < 3; k++) pos[k] = p->world[k], normal[k] = p->normal[k];
        max_dist = p->mfMaxDistance, min_dist = p->mfMinDistance;
    }
};

struct TrackingMock {
    TrFrame mCurrentFrame;
    std::vector<TrMapPoint *> mvpLocalMapPoints;
    int th = 1;  // what ref:src/Tracking.cc:4157-4178 would choose
    bool mbFarPoints = false;
    float mThFarPoints = 0;
    int SearchLocalPoints()
    {  // adapters/orbslam3/Tracking_osg.cc
        return osg_orbslam3::search_local_points<TrHooks>(mCurrentFrame, mvpLocalMapPoints, (float)th, mbFarPoints,
                                                          mThFarPoints, 0.8f);
    }
};
