// Tracking_osg.cc — drop-in bodies for ORB_SLAM3::Tracking::SearchLocalPoints and Tracking::PreintegrateIMU on the
// MI355X path (ORB-SLAM3 tree built with -DORB_SLAM3_OSG; see INTEGRATION.md, the SearchLocalPoints and the
// IMU preintegration paragraphs).
// Signature: ref:include/Tracking.h (void SearchLocalPoints()); body: ref:src/Tracking.cc:4097-4182.
// The marking loop, the gather, the one osg_search_local_points call (Frame::isInFrustum over the local
// MapPoints and SearchByProjection) and the write-back are osg_orbslam3::search_local_points; the choice of the
// search radius stays here, in the reference's words.
#include "Tracking.h"
#include "osg_hooks_orbslam3.h"

namespace ORB_SLAM3 {

void Tracking::SearchLocalPoints()
{
    // ref:src/Tracking.cc:4157-4178 (the reference evaluates it only when nToMatch > 0; it reads no state the
    // loop before it writes)
    int th = 1;
    if (mSensor == System::RGBD || mSensor == System::IMU_RGBD)
        th = 3;
    if (mpAtlas->isImuInitialized()) {
        if (mpAtlas->GetCurrentMap()->GetIniertialBA2())
            th = 2;
        else
            th = 6;
    } else if (!mpAtlas->isImuInitialized() &&
               (mSensor == System::IMU_MONOCULAR || mSensor == System::IMU_STEREO || mSensor == System::IMU_RGBD)) {
        th = 10;
    }
    if (mCurrentFrame.mnId < mnLastRelocFrameId + 2)
        th = 5;
    if (mState == LOST || mState == RECENTLY_LOST)
        th = 15;
    // ORBmatcher matcher(0.8), :4156
    osg_orbslam3::search_local_points<OsgHooks>(mCurrentFrame, mvpLocalMapPoints, (float)th, mpLocalMapper->mbFarPoints,
                                                mpLocalMapper->mThFarPoints, 0.8f);
}

// Signature: ref:include/Tracking.h (void PreintegrateIMU()); body: ref:src/Tracking.cc:1771-1918.  The queue
// selection and the integrables run on the host, the two running states (from the last KeyFrame, from the last
// frame) are integrated over the same list in one osg_imu_preintegrate_batch call, and the hand-over to
// mpImuPreintegratedFrame / mpImuPreintegrated is the reference's: osg_orbslam3::preintegrate_imu.  mvMeasurements
// stays a host vector on IMU::Preintegrated.
void Tracking::PreintegrateIMU()
{
    osg_orbslam3::preintegrate_imu<OsgHooks>(*this);
}

}  // namespace ORB_SLAM3
