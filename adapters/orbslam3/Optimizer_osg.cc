// Optimizer_osg.cc — drop-in bodies for Optimizer::PoseOptimization, Optimizer::PoseInertialOptimizationLastKeyFrame /
// LastFrame, the three overloads of Optimizer::InertialOptimization, the g2o part of
// Optimizer::LocalBundleAdjustment (both overloads), Optimizer::BundleAdjustment (global BA) and
// Optimizer::OptimizeSim3, Optimizer::OptimizeEssentialGraph (the loop-closure overload) and
// Optimizer::OptimizeEssentialGraph4DoF on the MI355X path (ORB-SLAM3 tree built with -DORB_SLAM3_OSG;
// see INTEGRATION.md).  Signatures: ref:include/Optimizer.h:54-90.
#include "Optimizer.h"
#include "osg_hooks_orbslam3.h"

namespace ORB_SLAM3 {

int Optimizer::PoseOptimization(Frame *pFrame)
{  // ref:src/Optimizer.cc:71-420; MapPoint::mGlobalMutex is held only while the edges are gathered
   // (:128-286), released before the GPU solve and the write-back
    return osg_orbslam3::pose_optimization<OsgHooks>(pFrame, &MapPoint::mGlobalMutex);
}

int Optimizer::PoseInertialOptimizationLastKeyFrame(Frame *pFrame, bool bRecInit)
{  // ref:src/Optimizer.cc:435-987; MapPoint::mGlobalMutex is held while the edges are gathered (:506-635)
    return osg_orbslam3::pose_inertial_optimization_last_keyframe<OsgHooks>(pFrame, bRecInit, &MapPoint::mGlobalMutex);
}

int Optimizer::PoseInertialOptimizationLastFrame(Frame *pFrame, bool bRecInit)
{  // ref:src/Optimizer.cc:1002-1640; a previous frame without mpcpi is refused by the library (the reference
   // dereferences null at :1275) and 0 is returned with the frame untouched
    return osg_orbslam3::pose_inertial_optimization_last_frame<OsgHooks>(pFrame, bRecInit, &MapPoint::mGlobalMutex);
}

namespace {
void rwg_to_rows(const Eigen::Matrix3d &Rwg, double r[9])
{
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) r[3 * i + j] = Rwg(i, j);
}
}  // namespace

void Optimizer::InertialOptimization(Map *pMap, Eigen::Matrix3d &Rwg, double &scale, Eigen::Vector3d &bg,
                                     Eigen::Vector3d &ba, bool bMono, Eigen::MatrixXd &covInertial, bool bFixedVel,
                                     bool bGauss, float priorG, float priorA)
{  // ref:src/Optimizer.cc:3706-3898 (LocalMapping::InitializeIMU); covInertial and bGauss are unused there too
    double r[9], g[3], a[3];
    rwg_to_rows(Rwg, r);
    if (!osg_orbslam3::inertial_optimization_init<OsgHooks>(pMap->GetAllKeyFrames(), pMap->GetMaxKFid(), r, scale, g, a,
                                                            bMono, bFixedVel, priorG, priorA))
        return;
    Rwg = Eigen::Map<const Eigen::Matrix<double, 3, 3, Eigen::RowMajor>>(r);
    bg = Eigen::Vector3d(g[0], g[1], g[2]);
    ba = Eigen::Vector3d(a[0], a[1], a[2]);
}

void Optimizer::InertialOptimization(Map *pMap, Eigen::Vector3d &bg, Eigen::Vector3d &ba, float priorG, float priorA)
{  // ref:src/Optimizer.cc:3910-4076 (LoopClosing::MergeLocal2)
    double g[3], a[3];
    if (!osg_orbslam3::inertial_optimization_bias<OsgHooks>(pMap->GetAllKeyFrames(), pMap->GetMaxKFid(), g, a, priorG,
                                                            priorA))
        return;
    bg = Eigen::Vector3d(g[0], g[1], g[2]);
    ba = Eigen::Vector3d(a[0], a[1], a[2]);
}

void Optimizer::InertialOptimization(Map *pMap, Eigen::Matrix3d &Rwg, double &scale)
{  // ref:src/Optimizer.cc:4085-4197 (LocalMapping::ScaleRefinement)
    double r[9];
    rwg_to_rows(Rwg, r);
    if (!osg_orbslam3::inertial_optimization_scale<OsgHooks>(pMap->GetAllKeyFrames(), pMap->GetMaxKFid(), r, scale))
        return;
    Rwg = Eigen::Map<const Eigen::Matrix<double, 3, 3, Eigen::RowMajor>>(r);
}

// The local window (ref:src/Optimizer.cc:1762-1873) is the reference's code unchanged; it ends with
// lLocalKeyFrames, lLocalMapPoints, lFixedCameras and the no-fixed-KeyFrame early return.  Call
// this instead of the g2o graph build + optimize + classification (ref:src/Optimizer.cc:1877-2203).
void OsgLocalBundleAdjustmentTail(KeyFrame *pKF, bool *pbStopFlag, Map *pMap,
                                  std::list<KeyFrame *> &lLocalKeyFrames, std::list<KeyFrame *> &lFixedCameras,
                                  std::list<MapPoint *> &lLocalMapPoints, int &num_fixedKF, int &num_OptKF,
                                  int &num_MPs, int &num_edges)
{
    Map *pCurrentMap = pKF->GetMap();
    auto out = osg_orbslam3::local_bundle_adjustment<OsgHooks>(lLocalKeyFrames, lFixedCameras, lLocalMapPoints,
                                                               pCurrentMap, pMap->GetInitKFid(), pbStopFlag,
                                                               pMap->IsInertial());
    num_fixedKF = out.num_fixedKF;
    num_OptKF = out.num_OptKF;
    num_MPs = out.num_MPs;
    num_edges = out.num_edges;
    if (out.aborted && out.poses.empty()) return;  // stop flag before optimize (ref:src/Optimizer.cc:2112-2114)
    std::unique_lock<std::mutex> lock(pMap->mMutexMapUpdate);  // ref:src/Optimizer.cc:2171
    osg_orbslam3::apply_local_bundle_adjustment<OsgHooks>(out);
    pMap->IncreaseChangeIndex();
}

void Optimizer::BundleAdjustment(const std::vector<KeyFrame *> &vpKFs, const std::vector<MapPoint *> &vpMP,
                                 int nIterations, bool *pbStopFlag, const unsigned long nLoopKF, const bool bRobust)
{  // ref:src/Optimizer.cc:2850-3237 (GlobalBundleAdjustemnt, :2831-2839, passes the whole map)
    Map *pMap = vpKFs[0]->GetMap();
    auto out = osg_orbslam3::bundle_adjustment<OsgHooks>(vpKFs, vpMP, pMap->GetInitKFid(), nIterations, pbStopFlag,
                                                         bRobust);
    osg_orbslam3::apply_bundle_adjustment<OsgHooks>(out, nLoopKF, nLoopKF == pMap->GetOriginKF()->mnId);
}

void Optimizer::LocalBundleAdjustment(KeyFrame *pMainKF, std::vector<KeyFrame *> vpAdjustKF,
                                      std::vector<KeyFrame *> vpFixedKF, bool *pbStopFlag)
{  // ref:src/Optimizer.cc:5211-5672 (LoopClosing's map merge)
    auto out = osg_orbslam3::merge_local_bundle_adjustment<OsgHooks, KeyFrame, MapPoint>(pMainKF, vpAdjustKF, vpFixedKF,
                                                                                        pbStopFlag);
    if (out.aborted) return;  // :5444-5446
    std::unique_lock<std::mutex> lock(pMainKF->GetMap()->mMutexMapUpdate);  // :5551
    osg_orbslam3::apply_merge_local_bundle_adjustment<OsgHooks>(out);
}

int Optimizer::OptimizeSim3(KeyFrame *pKF1, KeyFrame *pKF2, std::vector<MapPoint *> &vpMatches1, g2o::Sim3 &g2oS12,
                            const float th2, const bool bFixScale, Eigen::Matrix<double, 7, 7> &mAcumHessian,
                            const bool bAllPoints)
{  // ref:src/Optimizer.cc:4213-4512 (LoopClosing's Sim3 refinement of a loop / merge candidate)
    return osg_orbslam3::optimize_sim3<OsgHooks>(pKF1, pKF2, vpMatches1, g2oS12, th2, bFixScale, mAcumHessian,
                                                 bAllPoints);
}

void Optimizer::OptimizeEssentialGraph(Map *pMap, KeyFrame *pLoopKF, KeyFrame *pCurKF,
                                       const LoopClosing::KeyFrameAndPose &NonCorrectedSim3,
                                       const LoopClosing::KeyFrameAndPose &CorrectedSim3,
                                       const map<KeyFrame *, set<KeyFrame *>> &LoopConnections, const bool &bFixScale)
{  // ref:src/Optimizer.cc:4527-4858 (LoopClosing::CorrectLoop's pose-graph optimisation); the lock of :4801 is
   // taken inside, after the optimisation and before the write-back
    osg_orbslam3::optimize_essential_graph<OsgHooks>(pMap, pLoopKF, pCurKF, NonCorrectedSim3, CorrectedSim3,
                                                     LoopConnections, bFixScale);
}

void Optimizer::OptimizeEssentialGraph4DoF(Map *pMap, KeyFrame *pLoopKF, KeyFrame *pCurKF,
                                           const LoopClosing::KeyFrameAndPose &NonCorrectedSim3,
                                           const LoopClosing::KeyFrameAndPose &CorrectedSim3,
                                           const map<KeyFrame *, set<KeyFrame *>> &LoopConnections)
{  // ref:src/Optimizer.cc:4870-5198 (LoopClosing::CorrectLoop's pose graph in an inertial map); the lock of :5150
   // is taken inside, after the optimisation and before the write-back
    osg_orbslam3::optimize_essential_graph_4dof<OsgHooks>(pMap, pLoopKF, pCurKF, NonCorrectedSim3, CorrectedSim3,
                                                          LoopConnections);
}

void Optimizer::LocalInertialBA(KeyFrame *pKF, bool *pbStopFlag, Map *pMap, int &num_fixedKF, int &num_OptKF,
                                int &num_MPs, int &num_edges, bool bLarge, bool bRecInit)
{  // ref:src/Optimizer.cc:2221-2816 (LocalMapping::Run once the IMU is initialised); the stop flag is set after
   // optimize() in the reference and never read, and the four counters are never written there
    auto out = osg_orbslam3::local_inertial_ba<OsgHooks, KeyFrame, MapPoint>(pKF, bLarge, bRecInit);
    std::unique_lock<std::mutex> lock(pMap->mMutexMapUpdate);  // :2746
    osg_orbslam3::apply_local_inertial_ba<OsgHooks>(out, pMap);
}

}  // namespace ORB_SLAM3
