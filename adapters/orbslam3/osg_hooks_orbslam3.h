// osg_hooks_orbslam3.h — the hook policy of osg_orbslam3.h written with ORB-SLAM3's own Sophus /
// Eigen / GeometricCamera calls, so every float the reference computes before its matching and
// optimisation loops is computed by the same code.  Compiled only inside an ORB-SLAM3 tree.
#ifndef OSG_HOOKS_ORBSLAM3_H
#define OSG_HOOKS_ORBSLAM3_H

#include "Frame.h"
#include "G2oTypes.h"
#include "KeyFrame.h"
#include "MapPoint.h"
#include "Thirdparty/DBoW2/DUtils/Random.h"
#include "Thirdparty/g2o/g2o/types/sim3.h"
#include "osg_orbslam3.h"

namespace ORB_SLAM3 {

struct OsgHooks {
    template <class T>
    static void pose(T &o, double q[7])
    {
        const Sophus::SE3<float> Tcw = const_cast<T &>(o).GetPose();
        const Eigen::Quaterniond qd = Tcw.unit_quaternion().cast<double>();
        const Eigen::Vector3d t = Tcw.translation().cast<double>();
        q[0] = qd.x(); q[1] = qd.y(); q[2] = qd.z(); q[3] = qd.w();
        q[4] = t.x(); q[5] = t.y(); q[6] = t.z();
    }
    template <class T>
    static void set_pose(T &o, const double q[7])
    {  // ref:src/Optimizer.cc:413-416 / 2187-2195: SE3Quat estimate -> SE3f
        const Eigen::Quaternionf qf(Eigen::Quaterniond(q[3], q[0], q[1], q[2]).cast<float>());
        o.SetPose(Sophus::SE3<float>(qf, Eigen::Vector3d(q[4], q[5], q[6]).cast<float>()));
    }
    static void world_pos(MapPoint *p, double x[3])
    {
        const Eigen::Vector3d X = p->GetWorldPos().cast<double>();
        x[0] = X.x(); x[1] = X.y(); x[2] = X.z();
    }
    static void set_world_pos(MapPoint *p, const double x[3])
    {  // ref:src/Optimizer.cc:2197-2203
        p->SetWorldPos(Eigen::Vector3d(x[0], x[1], x[2]).cast<float>());
        p->UpdateNormalAndDepth();
    }
    static void set_gba_pose(KeyFrame &k, const double q[7], unsigned long nLoopKF)
    {  // ref:src/Optimizer.cc:3144-3145: SE3d(SE3quat.rotation(), SE3quat.translation()).cast<float>()
        const Eigen::Quaterniond qd(q[3], q[0], q[1], q[2]);
        k.mTcwGBA = Sophus::SE3d(qd, Eigen::Vector3d(q[4], q[5], q[6])).cast<float>();
        k.mnBAGlobalForKF = nLoopKF;
    }
    static void set_gba_pos(MapPoint *p, const double x[3], unsigned long nLoopKF)
    {  // ref:src/Optimizer.cc:3233-3234
        p->mPosGBA = Eigen::Vector3d(x[0], x[1], x[2]).cast<float>();
        p->mnBAGlobalForKF = nLoopKF;
    }
    template <class T>
    static void camera(const T &o, bool right, osg_camera &c)
    {
        std::memset(&c, 0, sizeof c);
        GeometricCamera *cam = right ? o.mpCamera2 : o.mpCamera;
        c.type = (cam->GetType() == GeometricCamera::CAM_FISHEYE) ? OSG_CAM_KB8 : OSG_CAM_PINHOLE;
        for (size_t i = 0; i < cam->size() && i < 8; i++) c.p[i] = cam->getParameter((int)i);
        c.fx = o.fx; c.fy = o.fy; c.cx = o.cx; c.cy = o.cy; c.bf = o.mbf;
        c.trl[3] = 1.0;
        if (right) {
            const Sophus::SE3f Trl = const_cast<T &>(o).GetRelativePoseTrl();
            const Eigen::Quaterniond qd = Trl.unit_quaternion().cast<double>();
            const Eigen::Vector3d t = Trl.translation().cast<double>();
            c.trl[0] = qd.x(); c.trl[1] = qd.y(); c.trl[2] = qd.z(); c.trl[3] = qd.w();
            c.trl[4] = t.x(); c.trl[5] = t.y(); c.trl[6] = t.z();
        }
    }
    // ref:src/ORBmatcher.cc:1052-1083 and Pinhole.cpp:194-197: the epipole and F12 = K1^-T [t12]x R12 K2^-1
    // for each camera pair (ll, lr, rl, rr), evaluated with the reference's own Sophus / Eigen expressions
    static void triang_geom(KeyFrame *pKF1, KeyFrame *pKF2, osg_triang_geom &g)
    {
        std::memset(&g, 0, sizeof g);
        const Sophus::SE3f T1w = pKF1->GetPose(), T2w = pKF2->GetPose(), Tw2 = pKF2->GetPoseInverse();
        const Eigen::Vector3f Cw = pKF1->GetCameraCenter();
        const Eigen::Vector3f C2 = T2w * Cw;
        const Eigen::Vector2f ep = pKF2->mpCamera->project(C2);
        g.ep_x = ep(0);
        g.ep_y = ep(1);
        Sophus::SE3f T[4];
        int nk = 1;
        T[0] = T1w * Tw2;
        if (pKF1->mpCamera2 || pKF2->mpCamera2) {
            const Sophus::SE3f Tr1w = pKF1->GetRightPose(), Twr2 = pKF2->GetRightPoseInverse();
            T[1] = T1w * Twr2;
            T[2] = Tr1w * Tw2;
            T[3] = Tr1w * Twr2;
            nk = 4;
        }
        GeometricCamera *c1[2] = {pKF1->mpCamera, pKF1->mpCamera2}, *c2[2] = {pKF2->mpCamera, pKF2->mpCamera2};
        g.pinhole = 1;
        for (int k = 0; k < nk; k++)
            if (c1[k >> 1]->GetType() != GeometricCamera::CAM_PINHOLE ||
                c2[k & 1]->GetType() != GeometricCamera::CAM_PINHOLE)
                g.pinhole = 0;
        if (!g.pinhole) {  // KannalaBrandt8: R12 / t12 per pair and the four cameras' parameters
            for (int k = 0; k < nk; k++) {
                const Eigen::Matrix3f R12 = T[k].rotationMatrix();
                const Eigen::Vector3f t12 = T[k].translation();
                for (int r = 0; r < 3; r++) {
                    for (int c = 0; c < 3; c++) g.R12[k][3 * r + c] = R12(r, c);
                    g.t12[k][r] = t12(r);
                }
            }
            GeometricCamera *cams[4] = {c1[0], c1[1], c2[0], c2[1]};
            for (int i = 0; i < 4; i++)
                if (cams[i])
                    for (int j = 0; j < 8 && j < (int)cams[i]->size(); j++) g.kb[i][j] = cams[i]->getParameter(j);
            return;
        }
        for (int k = 0; k < nk; k++) {
            const Eigen::Matrix3f R12 = T[k].rotationMatrix();
            const Eigen::Vector3f t12 = T[k].translation();
            const Eigen::Matrix3f t12x = Sophus::SO3f::hat(t12);
            const Eigen::Matrix3f K1 = c1[k >> 1]->toK_();
            const Eigen::Matrix3f K2 = c2[k & 1]->toK_();
            const Eigen::Matrix3f F12 = K1.transpose().inverse() * t12x * R12 * K2.inverse();
            for (int r = 0; r < 3; r++)
                for (int c = 0; c < 3; c++) g.F12[k][3 * r + c] = F12(r, c);
        }
    }
    // ref:src/MapPoint.cc:530-534: mDescriptor = vDescriptors[BestIdx].clone() under mMutexFeatures
    // (OsgHooks is a friend of MapPoint under ORB_SLAM3_OSG)
    static void set_descriptor(MapPoint *pMP, const uint8_t *row)
    {
        std::unique_lock<std::mutex> lock(pMP->mMutexFeatures);
        pMP->mDescriptor = cv::Mat(1, 32, CV_8UC1, const_cast<uint8_t *>(row)).clone();
    }
    // ref:src/ORBmatcher.cc:1993-2009; the invz < 0 and image-bounds tests stay in the kernel
    static bool project_last(const Frame &CF, MapPoint *pMP, float &u, float &v, float &invz)
    {
        const Sophus::SE3f Tcw = const_cast<Frame &>(CF).GetPose();
        const Eigen::Vector3f x3Dw = pMP->GetWorldPos();
        const Eigen::Vector3f x3Dc = Tcw * x3Dw;
        invz = 1.0 / x3Dc(2);
        const Eigen::Vector2f uv = CF.mpCamera->project(x3Dc);
        u = uv(0);
        v = uv(1);
        return true;
    }
    // ref:src/ORBmatcher.cc:2096-2097: right-camera projection of a two-camera current frame (the
    // reference projects Trl * x3Dc with mpCamera)
    static void project_last_right(const Frame &CF, MapPoint *pMP, float &u, float &v)
    {
        Frame &F = const_cast<Frame &>(CF);
        const Eigen::Vector3f x3Dc = F.GetPose() * pMP->GetWorldPos();
        const Eigen::Vector3f x3Dr = F.GetRelativePoseTrl() * x3Dc;
        const Eigen::Vector2f uv = CF.mpCamera->project(x3Dr);
        u = uv(0);
        v = uv(1);
    }
    // ref:src/ORBmatcher.cc:1972-1980
    static float tlc_z(const Frame &CF, const Frame &LF)
    {
        const Sophus::SE3f Tcw = const_cast<Frame &>(CF).GetPose();
        const Eigen::Vector3f twc = Tcw.inverse().translation();
        const Sophus::SE3f Tlw = const_cast<Frame &>(LF).GetPose();
        const Eigen::Vector3f tlc = Tlw * twc;
        return tlc(2);
    }
    // ref:src/ORBmatcher.cc:2238-2262: projection, image bounds, scale-invariance range, PredictScale
    static bool kf_query(const Frame &CF, MapPoint *pMP, float &u, float &v, int &level)
    {
        Frame &F = const_cast<Frame &>(CF);
        const Sophus::SE3f Tcw = F.GetPose();
        const Eigen::Vector3f Ow = Tcw.inverse().translation();
        const Eigen::Vector3f x3Dw = pMP->GetWorldPos();
        const Eigen::Vector3f x3Dc = Tcw * x3Dw;
        const Eigen::Vector2f uv = CF.mpCamera->project(x3Dc);
        if (uv(0) < CF.mnMinX || uv(0) > CF.mnMaxX) return false;
        if (uv(1) < CF.mnMinY || uv(1) > CF.mnMaxY) return false;
        const float dist3D = (x3Dw - Ow).norm();
        if (dist3D < pMP->GetMinDistanceInvariance() || dist3D > pMP->GetMaxDistanceInvariance()) return false;
        level = pMP->PredictScale(dist3D, &F);
        u = uv(0);
        v = uv(1);
        return true;
    }
    // ref:src/ORBmatcher.cc:1336-1347, 1385-1433 (Fuse): pose / centre / camera of the chosen side,
    // depth, projection, IsInImage, ur, scale-invariance range, viewing angle, PredictScale
    static bool fuse_query(KeyFrame *pKF, MapPoint *pMP, bool bRight, float &u, float &v, float &ur, int &level)
    {
        const Sophus::SE3f Tcw = bRight ? pKF->GetRightPose() : pKF->GetPose();
        const Eigen::Vector3f Ow = bRight ? pKF->GetRightCameraCenter() : pKF->GetCameraCenter();
        GeometricCamera *pCamera = bRight ? pKF->mpCamera2 : pKF->mpCamera;
        const float &bf = pKF->mbf;
        const Eigen::Vector3f p3Dw = pMP->GetWorldPos();
        const Eigen::Vector3f p3Dc = Tcw * p3Dw;
        if (p3Dc(2) < 0.0f) return false;
        const float invz = 1 / p3Dc(2);
        const Eigen::Vector2f uv = pCamera->project(p3Dc);
        if (!pKF->IsInImage(uv(0), uv(1))) return false;
        ur = uv(0) - bf * invz;
        const float maxDistance = pMP->GetMaxDistanceInvariance();
        const float minDistance = pMP->GetMinDistanceInvariance();
        const Eigen::Vector3f PO = p3Dw - Ow;
        const float dist3D = PO.norm();
        if (dist3D < minDistance || dist3D > maxDistance) return false;
        const Eigen::Vector3f Pn = pMP->GetNormal();
        if (PO.dot(Pn) < 0.5 * dist3D) return false;
        level = pMP->PredictScale(dist3D, pKF);
        u = uv(0);
        v = uv(1);
        return true;
    }
    // ref:src/ORBmatcher.cc:1560-1562, 1587-1622 (Fuse with Sim3): the same tests with Tcw from Scw
    // ref:src/ORBmatcher.cc:1589-1622 (Fuse, Sim3) and :530-572 / :649-688 (SearchByProjection, Sim3):
    // depth, image, distance and viewing-angle tests, the projection and PredictScale.  The second
    // SearchByProjection overload projects with its own pinhole formula (invz = 1 / z; u = fx * x * invz
    // + cx, :661-667) instead of mpCamera->project — different float rounding, so it is kept apart.
    // ref:src/ORBmatcher.cc:1747-1772 (dir12: KF1's MapPoint into KF2 by S21 * T1w) and :1823-1850
    // (KF2's into KF1 by S12 * T2w); both directions use pKF1's intrinsics, as the reference does
    static int index_in_keyframe(MapPoint *pMP, KeyFrame *pKF) { return std::get<0>(pMP->GetIndexInKeyFrame(pKF)); }
    static bool sim3_pair_query(KeyFrame *pKF1, KeyFrame *pKF2, MapPoint *pMP, const Sophus::Sim3f &S12, bool dir12,
                                float &u, float &v, int &level)
    {
        KeyFrame *from = dir12 ? pKF1 : pKF2, *to = dir12 ? pKF2 : pKF1;
        const Sophus::Sim3f S = dir12 ? S12.inverse() : S12;
        const Eigen::Vector3f p3Dw = pMP->GetWorldPos();
        const Eigen::Vector3f pc = S * (from->GetPose() * p3Dw);
        if (pc(2) < 0.0) return false;
        const float invz = 1.0 / pc(2);
        const float x = pc(0) * invz;
        const float y = pc(1) * invz;
        u = pKF1->fx * x + pKF1->cx;
        v = pKF1->fy * y + pKF1->cy;
        if (!to->IsInImage(u, v)) return false;
        const float maxDistance = pMP->GetMaxDistanceInvariance();
        const float minDistance = pMP->GetMinDistanceInvariance();
        const float dist3D = pc.norm();
        if (dist3D < minDistance || dist3D > maxDistance) return false;
        level = pMP->PredictScale(dist3D, to);
        return true;
    }
    static bool sim3_query(KeyFrame *pKF, const Sophus::Sim3f &Scw, MapPoint *pMP, bool pinhole_formula, float &u,
                           float &v, int &level)
    {
        const Sophus::SE3f Tcw = Sophus::SE3f(Scw.rotationMatrix(), Scw.translation() / Scw.scale());
        const Eigen::Vector3f Ow = Tcw.inverse().translation();
        const Eigen::Vector3f p3Dw = pMP->GetWorldPos();
        const Eigen::Vector3f p3Dc = Tcw * p3Dw;
        if (p3Dc(2) < 0.0f) return false;
        if (pinhole_formula) {
            const float invz = 1 / p3Dc(2);
            const float x = p3Dc(0) * invz;
            const float y = p3Dc(1) * invz;
            u = pKF->fx * x + pKF->cx;
            v = pKF->fy * y + pKF->cy;
        } else {
            const Eigen::Vector2f uv = pKF->mpCamera->project(p3Dc);
            u = uv(0);
            v = uv(1);
        }
        if (!pKF->IsInImage(u, v)) return false;
        const float maxDistance = pMP->GetMaxDistanceInvariance();
        const float minDistance = pMP->GetMinDistanceInvariance();
        const Eigen::Vector3f PO = p3Dw - Ow;
        const float dist3D = PO.norm();
        if (dist3D < minDistance || dist3D > maxDistance) return false;
        const Eigen::Vector3f Pn = pMP->GetNormal();
        if (PO.dot(Pn) < 0.5 * dist3D) return false;
        level = pMP->PredictScale(dist3D, pKF);
        return true;
    }
    static bool fuse_sim3_query(KeyFrame *pKF, const Sophus::Sim3f &Scw, MapPoint *pMP, float &u, float &v,
                                int &level)
    {
        return sim3_query(pKF, Scw, pMP, false, u, v, level);
    }
    // OptimizeSim3, ref:src/Optimizer.cc:4232-4235, 4297-4307: P3Dc = Rcw * P3Dw + tcw in float, cast to double
    static void cam_point(KeyFrame *pKF, MapPoint *pMP, double x[3])
    {
        const Eigen::Matrix3f Rcw = pKF->GetRotation();
        const Eigen::Vector3f tcw = pKF->GetTranslation();
        const Eigen::Vector3f P3Dw = pMP->GetWorldPos();
        const Eigen::Vector3f P3Dc = Rcw * P3Dw + tcw;
        const Eigen::Vector3d d = P3Dc.cast<double>();
        x[0] = d.x(); x[1] = d.y(); x[2] = d.z();
    }
    static void sim3_get(const g2o::Sim3 &S, double q[4], double t[3], double &s)
    {
        const Eigen::Quaterniond &r = S.rotation();
        q[0] = r.x(); q[1] = r.y(); q[2] = r.z(); q[3] = r.w();
        for (int i = 0; i < 3; i++) t[i] = S.translation()[i];
        s = S.scale();
    }
    static void sim3_set(g2o::Sim3 &S, const double q[4], const double t[3], double s)
    {  // the estimate's own members: g2o::Sim3 never renormalises its quaternion
        S = g2o::Sim3(Eigen::Quaterniond(q[3], q[0], q[1], q[2]), Eigen::Vector3d(t[0], t[1], t[2]), s);
    }
    static void zero_hessian(Eigen::Matrix<double, 7, 7> &H) { H = Eigen::MatrixXd::Zero(7, 7); }  // :4483
    // OptimizeEssentialGraph, ref:src/Optimizer.cc:4595-4596, 4816-4817, 4848-4851
    static void kf_pose_sim3(KeyFrame *pKF, double q[4], double t[3])
    {
        const Sophus::SE3d Tcw = pKF->GetPose().cast<double>();
        const Eigen::Quaterniond r = Tcw.unit_quaternion();
        q[0] = r.x(); q[1] = r.y(); q[2] = r.z(); q[3] = r.w();
        for (int i = 0; i < 3; i++) t[i] = Tcw.translation()[i];
    }
    static void kf_set_pose_sim3(KeyFrame *pKF, const double q[4], const double t[3], double s)
    {
        const Eigen::Quaterniond r(q[3], q[0], q[1], q[2]);
        const Eigen::Vector3d tr(t[0], t[1], t[2]);
        Sophus::SE3f Tiw(r.cast<float>(), tr.cast<float>() / s);
        pKF->SetPose(Tiw);
    }
    // OptimizeEssentialGraph4DoF, ref:src/G2oTypes.cc:29-75, ref:src/Optimizer.cc:5164-5168
    static void kf_imu_cam_pose(KeyFrame *pKF, double row[36])
    {
        using RowM = Eigen::Matrix<double, 3, 3, Eigen::RowMajor>;
        Eigen::Map<RowM>(row) = pKF->GetImuRotation().cast<double>();
        Eigen::Map<Eigen::Vector3d>(row + 9) = pKF->GetImuPosition().cast<double>();
        Eigen::Map<RowM>(row + 12) = pKF->GetRotation().cast<double>();
        Eigen::Map<Eigen::Vector3d>(row + 21) = pKF->GetTranslation().cast<double>();
        Eigen::Map<RowM>(row + 24) = pKF->mImuCalib.mTcb.rotationMatrix().cast<double>();
        Eigen::Map<Eigen::Vector3d>(row + 33) = pKF->mImuCalib.mTcb.translation().cast<double>();
    }
    static void rot_to_quat(const double R[9], double q[4])
    {
        const Eigen::Matrix3d M = Eigen::Map<const Eigen::Matrix<double, 3, 3, Eigen::RowMajor>>(R);
        const Eigen::Quaterniond r(M);
        q[0] = r.x(); q[1] = r.y(); q[2] = r.z(); q[3] = r.w();
    }
    static void kf_set_pose_se3d(KeyFrame *pKF, const double q[4], const double t[3])
    {
        const Sophus::SE3d Tiw(Eigen::Quaterniond(q[3], q[0], q[1], q[2]), Eigen::Vector3d(t[0], t[1], t[2]));
        pKF->SetPose(Tiw.cast<float>());
    }
    static void mp_world_pos(MapPoint *pMP, float x[3])
    {
        const Eigen::Vector3f p = pMP->GetWorldPos();
        x[0] = p.x(); x[1] = p.y(); x[2] = p.z();
    }
    static void mp_set_world_pos(MapPoint *pMP, const float x[3]) { pMP->SetWorldPos(Eigen::Vector3f(x[0], x[1], x[2])); }
    // Sim3Solver (ref:src/Sim3Solver.cc): the returned Eigen types and the reference's random source
    using Matrix4f = Eigen::Matrix4f;
    using Matrix3f = Eigen::Matrix3f;
    using Vector3f = Eigen::Vector3f;
    static Eigen::Matrix4f mat4(const float *m) { return Eigen::Map<const Eigen::Matrix<float, 4, 4, Eigen::RowMajor>>(m); }
    static Eigen::Matrix3f mat3(const float *m) { return Eigen::Map<const Eigen::Matrix<float, 3, 3, Eigen::RowMajor>>(m); }
    static Eigen::Vector3f vec3(const float *v) { return Eigen::Vector3f(v[0], v[1], v[2]); }
    static int random_int(int min, int max) { return DUtils::Random::RandomInt(min, max); }  // :174
    // MLPnPsolver (ref:src/MLPnPsolver.cpp:109): the Frame's own camera model
    static void unproject(const Frame &F, float u, float v, float ray[3])
    {
        const cv::Point3f r = F.mpCamera->unproject(cv::Point2f(u, v));
        ray[0] = r.x; ray[1] = r.y; ray[2] = r.z;
    }
    // TwoViewReconstruction (ref:src/TwoViewReconstruction.cc:96)
    static void seed_rand_once(int seed) { DUtils::Random::SeedRandOnce(seed); }
    // CreateNewMapPoints (ref:src/LocalMapping.cc:559-565, 633-637, 683-728; ref:src/KeyFrame.cc:935): the poses and
    // camera centres of both cameras, mRwc / mTwc.translation() and the cameras' parameters, as the reference's own
    // Sophus / Eigen values (OsgHooks is a friend of KeyFrame under ORB_SLAM3_OSG for mRwc / mTwc)
    static void np_kf(KeyFrame *pKF, osg_np_kf &k)
    {
        const bool rig = pKF->mpCamera2 != nullptr;
        for (int c = 0; c < (rig ? 2 : 1); c++) {
            const Eigen::Matrix<float, 3, 4> T = (c ? pKF->GetRightPose() : pKF->GetPose()).matrix3x4();
            const Eigen::Vector3f O = c ? pKF->GetRightCameraCenter() : pKF->GetCameraCenter();
            for (int r = 0; r < 3; r++) {
                for (int j = 0; j < 4; j++) k.Tcw[c][4 * r + j] = T(r, j);
                k.Ow[c][r] = O(r);
            }
            GeometricCamera *cam = c ? pKF->mpCamera2 : pKF->mpCamera;
            for (int j = 0; j < 8 && j < (int)cam->size(); j++) k.cam[c][j] = cam->getParameter(j);
        }
        k.cam_type = pKF->mpCamera->GetType() == GeometricCamera::CAM_PINHOLE ? 0 : 1;
        std::unique_lock<std::mutex> lock(pKF->mMutexPose);
        const Eigen::Vector3f twc = pKF->mTwc.translation();
        for (int r = 0; r < 3; r++) {
            for (int j = 0; j < 3; j++) k.Rwc[3 * r + j] = pKF->mRwc(r, j);
            k.twc[r] = twc(r);
        }
    }
    // SearchLocalPoints: the constants Frame::isInFrustum[Checks] reads (ref:src/Frame.cc:694, 723, 1618-1628).  mRcw /
    // mtcw are what UpdatePoseMatrices stored (:601-602: mTcw.rotationMatrix(), mTcw.translation()); the right
    // camera's mR, mt and twc are formed by the reference's own Eigen expressions
    static void frustum_frame(Frame &F, osg_frustum_frame &f)
    {
        std::memset(&f, 0, sizeof f);
        const Sophus::SE3f Tcw = F.GetPose();
        Eigen::Matrix3f mR[2];
        Eigen::Vector3f mt[2], twc[2];
        mR[0] = Tcw.rotationMatrix();
        mt[0] = Tcw.translation();
        twc[0] = F.GetOw();
        f.two_cam = F.Nleft != -1;
        if (f.two_cam) {
            const Sophus::SE3f Trl = F.GetRelativePoseTrl();
            const Eigen::Matrix3f Rrl = Trl.rotationMatrix();
            const Eigen::Vector3f trl = Trl.translation();
            mR[1] = Rrl * mR[0];
            mt[1] = Rrl * mt[0] + trl;
            twc[1] = F.GetRwc() * F.GetRelativePoseTlr().translation() + twc[0];
        }
        for (int c = 0; c < (f.two_cam ? 2 : 1); c++) {
            for (int r = 0; r < 3; r++) {
                for (int j = 0; j < 3; j++) f.cam[c].R[3 * r + j] = mR[c](r, j);
                f.cam[c].t[r] = mt[c](r);
                f.cam[c].c[r] = twc[c](r);
            }
            GeometricCamera *cam = c ? F.mpCamera2 : F.mpCamera;
            f.cam[c].cam_type = cam->GetType() == GeometricCamera::CAM_PINHOLE ? 0 : 1;
            for (int j = 0; j < 8 && j < (int)cam->size(); j++) f.cam[c].cam[j] = cam->getParameter(j);
        }
        f.min_x = Frame::mnMinX, f.max_x = Frame::mnMaxX, f.min_y = Frame::mnMinY, f.max_y = Frame::mnMaxY;
        f.mbf = F.mbf;
        f.log_scale_factor = F.mfLogScaleFactor;
        f.n_levels = F.mnScaleLevels;
    }
    // GetDistanceRange: the integration's accessor of the raw mfMaxDistance / mfMinDistance under mMutexPos
    // (GetMaxDistanceInvariance() / 1.2f is not the stored value)
    static void mp_frustum(MapPoint *p, float pos[3], float normal[3], float &max_dist, float &min_dist)
    {
        const Eigen::Vector3f P = p->GetWorldPos(), Pn = p->GetNormal();
        for (int k = 0; k < 3; k++) pos[k] = P(k), normal[k] = Pn(k);
        p->GetDistanceRange(max_dist, min_dist);
    }
    // ---- PoseInertialOptimization ("PoseInertialOptimization")
    static void imu_state_from(const Eigen::Matrix3f &Rwb, const Eigen::Vector3f &twb, const Eigen::Vector3f &v,
                               const Eigen::Vector3d &bg, const Eigen::Vector3d &ba, osg_pio_state &s)
    {
        const Eigen::Matrix3d R = Rwb.cast<double>();
        const Eigen::Vector3d t = twb.cast<double>(), vd = v.cast<double>();
        for (int r = 0; r < 3; r++) {
            for (int c = 0; c < 3; c++) s.Rwb[3 * r + c] = R(r, c);
            s.twb[r] = t(r), s.v[r] = vd(r), s.bg[r] = bg(r), s.ba[r] = ba(r);
        }
    }
    // VertexPose / VertexVelocity / VertexGyroBias / VertexAccBias of a Frame (ref:src/G2oTypes.cc:81-127, 537-564)
    static void imu_state(Frame &F, osg_pio_state &s)
    {
        Eigen::Vector3d bg, ba;
        bg << F.mImuBias.bwx, F.mImuBias.bwy, F.mImuBias.bwz;
        ba << F.mImuBias.bax, F.mImuBias.bay, F.mImuBias.baz;
        imu_state_from(F.GetImuRotation(), F.GetImuPosition(), F.GetVelocity(), bg, ba, s);
    }
    // ... and of a KeyFrame (ref:src/G2oTypes.cc:29-75, 532-557)
    static void imu_state(KeyFrame &K, osg_pio_state &s)
    {
        imu_state_from(K.GetImuRotation(), K.GetImuPosition(), K.GetVelocity(), K.GetGyroBias().cast<double>(),
                       K.GetAccBias().cast<double>(), s);
    }
    // ImuCamPose(Frame*) (ref:src/G2oTypes.cc:81-127)
    static void imu_cameras(Frame &F, osg_pose_inertial_problem &p)
    {
        auto put3 = [](const Eigen::Matrix3d &M, double *o) {
            for (int r = 0; r < 3; r++)
                for (int c = 0; c < 3; c++) o[3 * r + c] = M(r, c);
        };
        auto putv = [](const Eigen::Vector3d &v, double *o) {
            for (int r = 0; r < 3; r++) o[r] = v(r);
        };
        p.n_cams = F.mpCamera2 ? 2 : 1;
        const Eigen::Vector3d tcw0 = F.GetPose().translation().cast<double>();
        const Eigen::Matrix3d Rcw0 = F.GetPose().rotationMatrix().cast<double>();
        const Eigen::Vector3d tcb0 = F.mImuCalib.mTcb.translation().cast<double>();
        const Eigen::Matrix3d Rcb0 = F.mImuCalib.mTcb.rotationMatrix().cast<double>();
        camera(F, false, p.cams[0].cam);
        put3(Rcw0, p.cams[0].Rcw), putv(tcw0, p.cams[0].tcw), put3(Rcb0, p.cams[0].Rcb), putv(tcb0, p.cams[0].tcb);
        putv(F.mImuCalib.mTbc.translation().cast<double>(), p.cams[0].tbc);
        p.bf = F.mbf;
        if (p.n_cams > 1) {
            const Eigen::Matrix4d Trl = F.GetRelativePoseTrl().matrix().cast<double>();
            const Eigen::Matrix3d Rrl = Trl.block<3, 3>(0, 0);
            const Eigen::Vector3d trl = Trl.block<3, 1>(0, 3);
            const Eigen::Matrix3d Rcb1 = Rrl * Rcb0;
            const Eigen::Vector3d tcb1 = Rrl * tcb0 + trl;
            camera(F, true, p.cams[1].cam);
            put3(Rrl * Rcw0, p.cams[1].Rcw), putv(Rrl * tcw0 + trl, p.cams[1].tcw);
            put3(Rcb1, p.cams[1].Rcb), putv(tcb1, p.cams[1].tcb);
            putv(-Rcb1.transpose() * tcb1, p.cams[1].tbc);
        }
    }
    // ImuCamPose(KeyFrame*) (ref:src/G2oTypes.cc:34-78)
    static void liba_cameras(KeyFrame &K, osg_liba_keyframe &k)
    {
        auto put3 = [](const Eigen::Matrix3d &M, double *o) {
            for (int r = 0; r < 3; r++)
                for (int c = 0; c < 3; c++) o[3 * r + c] = M(r, c);
        };
        auto putv = [](const Eigen::Vector3d &v, double *o) {
            for (int r = 0; r < 3; r++) o[r] = v(r);
        };
        k.n_cams = K.mpCamera2 ? 2 : 1;
        const Eigen::Vector3d tcw0 = K.GetTranslation().cast<double>();
        const Eigen::Matrix3d Rcw0 = K.GetRotation().cast<double>();
        const Eigen::Vector3d tcb0 = K.mImuCalib.mTcb.translation().cast<double>();
        const Eigen::Matrix3d Rcb0 = K.mImuCalib.mTcb.rotationMatrix().cast<double>();
        camera(K, false, k.cams[0].cam);
        put3(Rcw0, k.cams[0].Rcw), putv(tcw0, k.cams[0].tcw), put3(Rcb0, k.cams[0].Rcb), putv(tcb0, k.cams[0].tcb);
        putv(K.mImuCalib.mTbc.translation().cast<double>(), k.cams[0].tbc);
        k.bf = K.mbf;
        if (k.n_cams > 1) {
            const Eigen::Matrix4d Trl = K.GetRelativePoseTrl().matrix().cast<double>();
            const Eigen::Matrix3d Rrl = Trl.block<3, 3>(0, 0);
            const Eigen::Vector3d trl = Trl.block<3, 1>(0, 3);
            const Eigen::Matrix3d Rcb1 = Rrl * Rcb0;
            const Eigen::Vector3d tcb1 = Rrl * tcb0 + trl;
            camera(K, true, k.cams[1].cam);
            put3(Rrl * Rcw0, k.cams[1].Rcw), putv(Rrl * tcw0 + trl, k.cams[1].tcw);
            put3(Rcb1, k.cams[1].Rcb), putv(tcb1, k.cams[1].tcb);
            putv(-Rcb1.transpose() * tcb1, k.cams[1].tbc);
        }
    }
    static void preint_take_prev_bias(KeyFrame &K) { K.mpImuPreintegrated->SetNewBias(K.mPrevKF->GetImuBias()); }
    static void keypoint_un(KeyFrame &K, int i, float xy[2], int &octave)
    {
        const cv::KeyPoint &kp = K.mvKeysUn[i];
        xy[0] = kp.pt.x, xy[1] = kp.pt.y, octave = kp.octave;
    }
    static void keypoint_right(KeyFrame &K, int i, float xy[2])
    {
        const cv::KeyPoint &kp = K.mvKeysRight[i];
        xy[0] = kp.pt.x, xy[1] = kp.pt.y;
    }
    static float uncertainty2(KeyFrame &K, float x, float y)
    {
        return K.mpCamera->uncertainty2(Eigen::Matrix<double, 2, 1>((double)x, (double)y));
    }
    static void mp_update_normal_and_depth(MapPoint *pMP) { pMP->UpdateNormalAndDepth(); }
    static void kf_set_pose_rt(KeyFrame &K, const float R[9], const float t[3])
    {
        K.SetPose(Sophus::SE3f(mat3(R), vec3(t)));
    }
    static void erase_match(KeyFrame *pKF, MapPoint *pMP)
    {
        pKF->EraseMapPointMatch(pMP);
        pMP->EraseObservation(pKF);
    }
    static void preintegrated(IMU::Preintegrated *pInt, osg_pio_preintegrated &q)
    {
        auto put3 = [](const Eigen::Matrix3f &M, float *o) {
            for (int r = 0; r < 3; r++)
                for (int c = 0; c < 3; c++) o[3 * r + c] = M(r, c);
        };
        put3(pInt->dR, q.dR), put3(pInt->JRg, q.JRg), put3(pInt->JVg, q.JVg), put3(pInt->JVa, q.JVa);
        put3(pInt->JPg, q.JPg), put3(pInt->JPa, q.JPa);
        for (int r = 0; r < 3; r++) q.dV[r] = pInt->dV(r), q.dP[r] = pInt->dP(r);
        const IMU::Bias b = pInt->GetOriginalBias();
        q.b[0] = b.bax, q.b[1] = b.bay, q.b[2] = b.baz, q.b[3] = b.bwx, q.b[4] = b.bwy, q.b[5] = b.bwz;
        q.dT = pInt->dT;
        for (int r = 0; r < 15; r++)
            for (int c = 0; c < 15; c++) q.C[15 * r + c] = pInt->C(r, c);
    }
    static void constraint(const ConstraintPoseImu *c, osg_pio_prior &pr)
    {
        for (int r = 0; r < 3; r++) {
            for (int k = 0; k < 3; k++) pr.Rwb[3 * r + k] = c->Rwb(r, k);
            pr.twb[r] = c->twb(r), pr.vwb[r] = c->vwb(r), pr.bg[r] = c->bg(r), pr.ba[r] = c->ba(r);
        }
        for (int r = 0; r < 15; r++)
            for (int k = 0; k < 15; k++) pr.H[15 * r + k] = c->H(r, k);
    }
    static float track_depth(MapPoint *p) { return p->mTrackDepth; }
    // ref:src/Optimizer.cc:883-887 / 1466-1470
    static void set_imu_state(Frame &F, const osg_pio_state &s)
    {
        const Eigen::Matrix3d R = Eigen::Map<const Eigen::Matrix<double, 3, 3, Eigen::RowMajor>>(s.Rwb);
        const Eigen::Vector3d t(s.twb[0], s.twb[1], s.twb[2]), v(s.v[0], s.v[1], s.v[2]);
        F.SetImuPoseVelocity(R.cast<float>(), t.cast<float>(), v.cast<float>());
        Eigen::Matrix<double, 6, 1> b;
        b << s.bg[0], s.bg[1], s.bg[2], s.ba[0], s.ba[1], s.ba[2];
        F.mImuBias = IMU::Bias(b[3], b[4], b[5], b[0], b[1], b[2]);
    }
    static ConstraintPoseImu *new_constraint(const osg_pio_state &s, const double H[225])
    {
        const Eigen::Matrix3d R = Eigen::Map<const Eigen::Matrix<double, 3, 3, Eigen::RowMajor>>(s.Rwb);
        const Eigen::Matrix<double, 15, 15> Hm = Eigen::Map<const Eigen::Matrix<double, 15, 15, Eigen::RowMajor>>(H);
        return new ConstraintPoseImu(R, Eigen::Vector3d(s.twb[0], s.twb[1], s.twb[2]), Eigen::Vector3d(s.v[0], s.v[1], s.v[2]),
                                     Eigen::Vector3d(s.bg[0], s.bg[1], s.bg[2]), Eigen::Vector3d(s.ba[0], s.ba[1], s.ba[2]), Hm);
    }
    // ---- IMU preintegration ("IMU preintegration"); IMU::Preintegrated names OsgHooks a friend
    static void imu_point(const IMU::Point &m, float a[3], float w[3], double &t)
    {
        for (int k = 0; k < 3; k++) a[k] = m.a(k), w[k] = m.w(k);
        t = m.t;
    }
    static void bias6(const IMU::Bias &b, float o[6])
    {
        o[0] = b.bax, o[1] = b.bay, o[2] = b.baz, o[3] = b.bwx, o[4] = b.bwy, o[5] = b.bwz;
    }
    static void frame_bias(Frame &F, float b[6]) { bias6(F.mImuBias, b); }
    static IMU::Preintegrated *new_preintegrated(Frame &last, Frame &cur)
    {
        return new IMU::Preintegrated(last.mImuBias, cur.mImuCalib);
    }
    static void preint_get(IMU::Preintegrated *pInt, osg_imu_preintegrated &st, float nga[6], float walk[6], float bu[6])
    {
        preintegrated(pInt, st.pre);  // GetOriginalBias() takes mMutex itself, and so does GetUpdatedBias()
        for (int k = 0; k < 3; k++) st.avgA[k] = pInt->avgA(k), st.avgW[k] = pInt->avgW(k);
        for (int k = 0; k < 6; k++) nga[k] = pInt->Nga.diagonal()(k), walk[k] = pInt->NgaWalk.diagonal()(k);
        bias6(pInt->GetUpdatedBias(), bu);
    }
    static void preint_measurements(IMU::Preintegrated *pInt, std::vector<float> &out)
    {
        std::unique_lock<std::mutex> lock(pInt->mMutex);
        for (const auto &m : pInt->mvMeasurements) {
            for (int k = 0; k < 3; k++) out.push_back(m.a(k));
            for (int k = 0; k < 3; k++) out.push_back(m.w(k));
            out.push_back(m.t);
        }
    }
    // the integrated fields of a result, under the caller's lock
    static void preint_fields(IMU::Preintegrated *pInt, const osg_imu_preintegrated &st)
    {
        using M3 = Eigen::Map<const Eigen::Matrix<float, 3, 3, Eigen::RowMajor>>;
        const osg_pio_preintegrated &q = st.pre;
        pInt->dR = M3(q.dR), pInt->JRg = M3(q.JRg), pInt->JVg = M3(q.JVg), pInt->JVa = M3(q.JVa);
        pInt->JPg = M3(q.JPg), pInt->JPa = M3(q.JPa);
        for (int k = 0; k < 3; k++) {
            pInt->dV(k) = q.dV[k], pInt->dP(k) = q.dP[k];
            pInt->avgA(k) = st.avgA[k], pInt->avgW(k) = st.avgW[k];
        }
        pInt->dT = q.dT;
        pInt->C = Eigen::Map<const Eigen::Matrix<float, 15, 15, Eigen::RowMajor>>(q.C);
    }
    static void preint_append(IMU::Preintegrated *pInt, const float *meas, int n)
    {
        for (int i = 0; i < n; i++) {
            const float *m = meas + 7 * i;
            pInt->mvMeasurements.emplace_back(Eigen::Vector3f(m[0], m[1], m[2]), Eigen::Vector3f(m[3], m[4], m[5]), m[6]);
        }
    }
    static void preint_continue(IMU::Preintegrated *pInt, const osg_imu_preintegrated &st, const float *meas, int n)
    {
        std::unique_lock<std::mutex> lock(pInt->mMutex);
        preint_fields(pInt, st);
        preint_append(pInt, meas, n);
    }
    static void preint_restart(IMU::Preintegrated *pInt, const osg_imu_preintegrated &st, const float *meas, int n)
    {
        std::unique_lock<std::mutex> lock(pInt->mMutex);
        const std::vector<float> list(meas, meas + 7 * (size_t)n);
        const float *b = st.pre.b;
        pInt->Initialize(IMU::Bias(b[0], b[1], b[2], b[3], b[4], b[5]));
        preint_fields(pInt, st);
        preint_append(pInt, list.data(), n);
    }
    static void gyro_bias(KeyFrame &K, float g[3])
    {
        const Eigen::Vector3f v = K.GetGyroBias();
        for (int k = 0; k < 3; k++) g[k] = v(k);
    }
    static void set_new_bias(KeyFrame &K, const float b[6]) { K.SetNewBias(IMU::Bias(b[0], b[1], b[2], b[3], b[4], b[5])); }
    // ---- InertialOptimization ("InertialOptimization")
    static bool is_bad(KeyFrame &K) { return K.isBad(); }
    static void set_velocity(KeyFrame &K, const double v[3])
    {
        const Eigen::Vector3d Vw(v[0], v[1], v[2]);
        K.SetVelocity(Vw.cast<float>());
    }
    // KeyFrameDatabase: the vocabulary on the device, set by System right after it loads ORBvoc
    // (osg_vocabulary_load_text) and before it constructs the database
    static const osg_vocabulary *&device_vocabulary()
    {
        static const osg_vocabulary *voc = nullptr;
        return voc;
    }
};

}  // namespace ORB_SLAM3
#endif
