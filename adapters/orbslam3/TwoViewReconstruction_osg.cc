// TwoViewReconstruction_osg.cc — drop-in body for ORB_SLAM3::TwoViewReconstruction::Reconstruct on the
// MI355X path (ORB-SLAM3 tree built with -DORB_SLAM3_OSG).  Signature:
// ref:include/TwoViewReconstruction.h:39-41.  Pinhole::ReconstructWithTwoViews and
// KannalaBrandt8::ReconstructWithTwoViews (which undistorts with cv::fisheye::undistortPoints on the host
// first) both reach this body; the reference's protected members (FindHomography ... DecomposeE) are not
// used.
#include "TwoViewReconstruction.h"
#include "osg_hooks_orbslam3.h"

namespace ORB_SLAM3 {

bool TwoViewReconstruction::Reconstruct(const std::vector<cv::KeyPoint> &vKeys1, const std::vector<cv::KeyPoint> &vKeys2,
                                        const std::vector<int> &vMatches12, Sophus::SE3f &T21,
                                        std::vector<cv::Point3f> &vP3D, std::vector<bool> &vbTriangulated)
{  // ref:src/TwoViewReconstruction.cc:49-151
    osg_orbslam3::TwoViewReconstruction<OsgHooks, cv::KeyPoint, cv::Point3f> tv(mK(0, 0), mK(1, 1), mK(0, 2), mK(1, 2),
                                                                                mSigma, mMaxIterations);
    float R[9], t[3];
    if (!tv.Reconstruct(vKeys1, vKeys2, vMatches12, R, t, vP3D, vbTriangulated)) return false;
    T21 = Sophus::SE3f(OsgHooks::mat3(R), OsgHooks::vec3(t));
    return true;
}

}  // namespace ORB_SLAM3
