// Sim3Solver_osg.cc — drop-in bodies for ORB_SLAM3::Sim3Solver's public members on the MI355X path
// (ORB-SLAM3 tree built with -DORB_SLAM3_OSG).  Signatures:
// ref:include/Sim3Solver.h:34-47.  The class gains one member under ORB_SLAM3_OSG,
//   std::shared_ptr<osg_orbslam3::Sim3Solver<OsgHooks, KeyFrame, MapPoint>> mpOsg;
// (LoopClosing copies its solver, ref:src/LoopClosing.cc:982; the copies share the state), and none of
// the reference's protected members is used.
#include "Sim3Solver.h"
#include "osg_hooks_orbslam3.h"

namespace ORB_SLAM3 {

Sim3Solver::Sim3Solver(KeyFrame *pKF1, KeyFrame *pKF2, const std::vector<MapPoint *> &vpMatched12, const bool bFixScale,
                       std::vector<KeyFrame *> vpKeyFrameMatchedMP)
    : mpOsg(std::make_shared<osg_orbslam3::Sim3Solver<OsgHooks, KeyFrame, MapPoint>>(pKF1, pKF2, vpMatched12, bFixScale,
                                                                                     vpKeyFrameMatchedMP))
{  // ref:src/Sim3Solver.cc:33-118
}

void Sim3Solver::SetRansacParameters(double probability, int minInliers, int maxIterations)
{  // :120-144
    mpOsg->SetRansacParameters(probability, minInliers, maxIterations);
}

Eigen::Matrix4f Sim3Solver::iterate(int nIterations, bool &bNoMore, std::vector<bool> &vbInliers, int &nInliers)
{  // :146-213
    return mpOsg->iterate(nIterations, bNoMore, vbInliers, nInliers);
}

Eigen::Matrix4f Sim3Solver::iterate(int nIterations, bool &bNoMore, std::vector<bool> &vbInliers, int &nInliers,
                                    bool &bConverge)
{  // :215-291
    return mpOsg->iterate(nIterations, bNoMore, vbInliers, nInliers, bConverge);
}

Eigen::Matrix4f Sim3Solver::find(std::vector<bool> &vbInliers12, int &nInliers)
{  // :293-297
    return mpOsg->find(vbInliers12, nInliers);
}

Eigen::Matrix4f Sim3Solver::GetEstimatedTransformation() { return mpOsg->GetEstimatedTransformation(); }
Eigen::Matrix3f Sim3Solver::GetEstimatedRotation() { return mpOsg->GetEstimatedRotation(); }
Eigen::Vector3f Sim3Solver::GetEstimatedTranslation() { return mpOsg->GetEstimatedTranslation(); }
float Sim3Solver::GetEstimatedScale() { return mpOsg->GetEstimatedScale(); }

}  // namespace ORB_SLAM3
