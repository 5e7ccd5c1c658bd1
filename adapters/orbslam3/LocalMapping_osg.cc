// LocalMapping_osg.cc — drop-in body for ORB_SLAM3::LocalMapping::CreateNewMapPoints on the MI355X path
// (ORB-SLAM3 tree built with -DORB_SLAM3_OSG; see INTEGRATION.md, the opt-in LocalMapping paragraph).
// Signature: ref:include/LocalMapping.h (void CreateNewMapPoints()); body: ref:src/LocalMapping.cc:526-934.
// The neighbour list, the gather and the one osg_create_new_map_points call are osg_orbslam3::
// create_new_map_points; the MapPoints are constructed here, in its output order, which is the reference's.
#include "LocalMapping.h"
#include "osg_hooks_orbslam3.h"

namespace ORB_SLAM3 {

void LocalMapping::CreateNewMapPoints()
{
    // ref:src/LocalMapping.cc:627
    const bool bCoarse = mbInertial && mpTracker->mState == Tracking::RECENTLY_LOST &&
                         mpCurrentKeyFrame->GetMap()->GetIniertialBA2();
    // :588 reads CheckNewKeyFrames() before every neighbour but the first; here it is read once: up -> neighbour 0
    // only, down -> every neighbour
    const bool bNewKeyFrames = CheckNewKeyFrames();
    osg_orbslam3::create_new_map_points<OsgHooks, KeyFrame>(
        mpCurrentKeyFrame, mbMonocular, mbInertial, bCoarse, mbFarPoints, mThFarPoints, bNewKeyFrames,
        [&](KeyFrame *pKF2, int idx1, int idx2, const float *x) {  // :910-931
            const Eigen::Vector3f x3D(x[0], x[1], x[2]);
            MapPoint *pMP = new MapPoint(x3D, mpCurrentKeyFrame, mpAtlas->GetCurrentMap());
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

}  // namespace ORB_SLAM3
