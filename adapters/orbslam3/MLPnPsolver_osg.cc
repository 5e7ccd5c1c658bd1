// MLPnPsolver_osg.cc — drop-in bodies for ORB_SLAM3::MLPnPsolver's public members on the MI355X path
// (ORB-SLAM3 tree built with -DORB_SLAM3_OSG).  Signatures:
// ref:include/MLPnPsolver.h:65-74.  The class gains one member under ORB_SLAM3_OSG,
//   std::unique_ptr<osg_orbslam3::MLPnPsolver<OsgHooks, Frame, MapPoint>> mpOsg;
// (Tracking::Relocalization keeps its solvers by pointer, ref:src/Tracking.cc:4508), and none of the
// reference's private members is used.
#include "MLPnPsolver.h"
#include "osg_hooks_orbslam3.h"

namespace ORB_SLAM3 {

MLPnPsolver::MLPnPsolver(const Frame &F, const vector<MapPoint *> &vpMapPointMatches)
    : mpOsg(new osg_orbslam3::MLPnPsolver<OsgHooks, Frame, MapPoint>(F, vpMapPointMatches))
{  // ref:src/MLPnPsolver.cpp:68-133
}

MLPnPsolver::~MLPnPsolver() {}

void MLPnPsolver::SetRansacParameters(double probability, int minInliers, int maxIterations, int minSet, float epsilon,
                                      float th2)
{  // :314-354
    mpOsg->SetRansacParameters(probability, minInliers, maxIterations, minSet, epsilon, th2);
}

bool MLPnPsolver::iterate(int nIterations, bool &bNoMore, vector<bool> &vbInliers, int &nInliers, Eigen::Matrix4f &Tout)
{  // :145-301
    return mpOsg->iterate(nIterations, bNoMore, vbInliers, nInliers, Tout);
}

}  // namespace ORB_SLAM3
