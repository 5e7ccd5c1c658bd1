// mock_inertial.h — the inertial members of Frame / KeyFrame, IMU::Preintegrated and ConstraintPoseImu as far as
// osg_orbslam3::pose_inertial_optimization_last_keyframe / _last_frame use them (test-only;
// tests/adapter/poseinertial_driver.cpp).  Float where the reference stores float.
#pragma once
#include <cmath>
#include <cstring>

#include "mock_orbslam3.h"

namespace mock {

// IMU::Preintegrated: the stored float fields (matrices row-major); b = (bax, bay, baz, bwx, bwy, bwz)
struct Preintegrated {
    float dR[9], dV[3], dP[3], JRg[9], JVg[9], JVa[9], JPg[9], JPa[9], b[6], dT, C[225];
};

// ConstraintPoseImu with its constructor (ref:include/G2oTypes.h:825-838): H = (H + H) / 2, which symmetrises
// nothing, then the eigenvalues below 1e-12 of the self-adjoint solver, which reads the lower triangle, set to 0
struct ConstraintPoseImu {
    double Rwb[9], twb[3], vwb[3], bg[3], ba[3], H[225];
    static inline int live = 0;  // test-only: constructed minus destroyed
    ConstraintPoseImu(const double *Rwb_, const double *twb_, const double *vwb_, const double *bg_, const double *ba_,
                      const double *H_)
    {
        live++;
        std::memcpy(Rwb, Rwb_, sizeof Rwb);
        std::memcpy(twb, twb_, sizeof twb);
        std::memcpy(vwb, vwb_, sizeof vwb);
        std::memcpy(bg, bg_, sizeof bg);
        std::memcpy(ba, ba_, sizeof ba);
        double A[15][15], V[15][15];
        for (int i = 0; i < 15; i++)
            for (int j = 0; j < 15; j++) {
                const double lo = i >= j ? H_[15 * i + j] : H_[15 * j + i];
                A[i][j] = (lo + lo) / 2;
                V[i][j] = i == j ? 1.0 : 0.0;
            }
        for (int sweep = 0; sweep < 60; sweep++) {  // cyclic Jacobi
            double off = 0, diag = 0;
            for (int i = 0; i < 15; i++) {
                diag += A[i][i] * A[i][i];
                for (int j = i + 1; j < 15; j++) off += A[i][j] * A[i][j];
            }
            if (!(off > 1e-36 * diag)) break;
            for (int p = 0; p < 14; p++)
                for (int q = p + 1; q < 15; q++) {
                    const double apq = A[p][q];
                    if (apq == 0.0) continue;
                    const double th = (A[q][q] - A[p][p]) / (2.0 * apq);
                    const double tt = (th >= 0 ? 1.0 : -1.0) / (std::fabs(th) + std::sqrt(th * th + 1.0));
                    const double c = 1.0 / std::sqrt(tt * tt + 1.0), s = tt * c;
                    for (int k = 0; k < 15; k++) {
                        const double akp = A[k][p], akq = A[k][q];
                        A[k][p] = c * akp - s * akq, A[k][q] = s * akp + c * akq;
                    }
                    for (int k = 0; k < 15; k++) {
                        const double apk = A[p][k], aqk = A[q][k];
                        A[p][k] = c * apk - s * aqk, A[q][k] = s * apk + c * aqk;
                    }
                    for (int k = 0; k < 15; k++) {
                        const double vkp = V[k][p], vkq = V[k][q];
                        V[k][p] = c * vkp - s * vkq, V[k][q] = s * vkp + c * vkq;
                    }
                }
        }
        for (int i = 0; i < 15; i++)
            for (int j = 0; j < 15; j++) {
                double s = 0;
                for (int k = 0; k < 15; k++) s += V[i][k] * (A[k][k] < 1e-12 ? 0.0 : A[k][k]) * V[j][k];
                H[15 * i + j] = s;
            }
    }
    ~ConstraintPoseImu() { live--; }
};

// GetImuRotation / GetImuPosition / GetVelocity and the bias (mImuBias of a Frame, GetGyroBias / GetAccBias of a KeyFrame)
struct ImuBody {
    float Rwb[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, twb[3] = {0, 0, 0}, vel[3] = {0, 0, 0};
    float bias[6] = {0, 0, 0, 0, 0, 0};  // bax, bay, baz, bwx, bwy, bwz
};

struct ImuKeyFrame : KeyFrame, ImuBody {};

struct ImuFrame : Frame, ImuBody {
    float Rcw[9], tcw[3];            // GetPose() as a matrix
    float Rcb[9], tcb[3], tbc[3];    // mImuCalib.mTcb, mTbc
    float Rrl[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, trl[3] = {0, 0, 0};  // GetRelativePoseTrl()
    ImuKeyFrame *mpLastKeyFrame = nullptr;
    ImuFrame *mpPrevFrame = nullptr;
    Preintegrated *mpImuPreintegrated = nullptr, *mpImuPreintegratedFrame = nullptr;
    ConstraintPoseImu *mpcpi = nullptr;
};

struct InertialHooks : MockHooks {
    static void imu_state(const ImuBody &o, osg_pio_state &s)
    {
        for (int i = 0; i < 9; i++) s.Rwb[i] = (double)o.Rwb[i];
        for (int i = 0; i < 3; i++) {
            s.twb[i] = (double)o.twb[i], s.v[i] = (double)o.vel[i];
            s.bg[i] = (double)o.bias[3 + i], s.ba[i] = (double)o.bias[i];
        }
    }
    // ImuCamPose(Frame*) (ref:src/G2oTypes.cc:81-127) in double from the float members
    static void imu_cameras(const ImuFrame &F, osg_pose_inertial_problem &p)
    {
        p.n_cams = F.mpCamera2 ? 2 : 1;
        osg_pio_camera &a = p.cams[0];
        camera(F, false, a.cam);
        for (int i = 0; i < 9; i++) a.Rcw[i] = F.Rcw[i], a.Rcb[i] = F.Rcb[i];
        for (int i = 0; i < 3; i++) a.tcw[i] = F.tcw[i], a.tcb[i] = F.tcb[i], a.tbc[i] = F.tbc[i];
        p.bf = F.mbf;
        if (p.n_cams < 2) return;
        osg_pio_camera &b = p.cams[1];
        camera(F, true, b.cam);
        double R[9], t[3];
        for (int i = 0; i < 9; i++) R[i] = F.Rrl[i];
        for (int i = 0; i < 3; i++) t[i] = F.trl[i];
        for (int r = 0; r < 3; r++) {
            for (int c = 0; c < 3; c++) {
                b.Rcw[3 * r + c] = R[3 * r] * a.Rcw[c] + R[3 * r + 1] * a.Rcw[3 + c] + R[3 * r + 2] * a.Rcw[6 + c];
                b.Rcb[3 * r + c] = R[3 * r] * a.Rcb[c] + R[3 * r + 1] * a.Rcb[3 + c] + R[3 * r + 2] * a.Rcb[6 + c];
            }
            b.tcw[r] = R[3 * r] * a.tcw[0] + R[3 * r + 1] * a.tcw[1] + R[3 * r + 2] * a.tcw[2] + t[r];
            b.tcb[r] = R[3 * r] * a.tcb[0] + R[3 * r + 1] * a.tcb[1] + R[3 * r + 2] * a.tcb[2] + t[r];
        }
        for (int r = 0; r < 3; r++)  // tbc = -Rbc tcb, Rbc = Rcb'
            b.tbc[r] = -(b.Rcb[r] * b.tcb[0] + b.Rcb[3 + r] * b.tcb[1] + b.Rcb[6 + r] * b.tcb[2]);
    }
    static void preintegrated(const Preintegrated *q, osg_pio_preintegrated &o)
    {
        std::memcpy(o.dR, q->dR, sizeof o.dR), std::memcpy(o.dV, q->dV, sizeof o.dV), std::memcpy(o.dP, q->dP, sizeof o.dP);
        std::memcpy(o.JRg, q->JRg, sizeof o.JRg), std::memcpy(o.JVg, q->JVg, sizeof o.JVg);
        std::memcpy(o.JVa, q->JVa, sizeof o.JVa), std::memcpy(o.JPg, q->JPg, sizeof o.JPg);
        std::memcpy(o.JPa, q->JPa, sizeof o.JPa), std::memcpy(o.b, q->b, sizeof o.b), std::memcpy(o.C, q->C, sizeof o.C);
        o.dT = q->dT;
    }
    static void constraint(const ConstraintPoseImu *c, osg_pio_prior &pr)
    {
        std::memcpy(pr.Rwb, c->Rwb, sizeof pr.Rwb), std::memcpy(pr.twb, c->twb, sizeof pr.twb);
        std::memcpy(pr.vwb, c->vwb, sizeof pr.vwb), std::memcpy(pr.bg, c->bg, sizeof pr.bg);
        std::memcpy(pr.ba, c->ba, sizeof pr.ba), std::memcpy(pr.H, c->H, sizeof pr.H);
    }
    static float track_depth(MapPoint *p) { return p->mTrackDepth; }
    // SetImuPoseVelocity(Rwb.cast<float>(), ...) and mImuBias = IMU::Bias(b[3], b[4], b[5], b[0], b[1], b[2]), b = (bg, ba)
    static void set_imu_state(ImuFrame &F, const osg_pio_state &s)
    {
        for (int i = 0; i < 9; i++) F.Rwb[i] = (float)s.Rwb[i];
        for (int i = 0; i < 3; i++) F.twb[i] = (float)s.twb[i], F.vel[i] = (float)s.v[i];
        const double b[6] = {s.bg[0], s.bg[1], s.bg[2], s.ba[0], s.ba[1], s.ba[2]};
        const float acc_gyro[6] = {(float)b[3], (float)b[4], (float)b[5], (float)b[0], (float)b[1], (float)b[2]};
        std::memcpy(F.bias, acc_gyro, sizeof F.bias);
    }
    static ConstraintPoseImu *new_constraint(const osg_pio_state &s, const double H[225])
    {
        return new ConstraintPoseImu(s.Rwb, s.twb, s.v, s.bg, s.ba, H);
    }
};

}  // namespace mock
