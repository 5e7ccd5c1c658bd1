// inertialba_edges.h — the vertices and edges that the inertial bundle adjustments share (LocalInertialBA in
// localinertialba.hip; FullInertialBA and MergeInertialBA use the same ones): ImuCamPose as a flat state with its
// Update, the two-vertex visual edges EdgeMono / EdgeStereo (ref:src/G2oTypes.cc:398-436, 469-499,
// ref:include/G2oTypes.h:400-541) and the six-vertex EdgeInertial with its 24 Jacobian columns
// (ref:src/G2oTypes.cc:599-689).  Device code over ba_common.h (the camera models, Huber) and so3_common.h.
#pragma once
#include "ba_common.h"
#include "so3_common.h"

namespace osgiba {

using namespace osgla;
using namespace osgso3;

// offsets inside a KeyFrame's mutable state (doubles)
constexpr int K_RWB = 0, K_TWB = 9, K_V = 12, K_BG = 15, K_BA = 18, K_RCW = 21, K_TCW = 39, K_ITS = 45, K_N = 46;

// ImuCamPose::Update (ref:src/G2oTypes.cc:221-249) on the state st; cams: the KeyFrame's one or two cameras
__device__ inline void pose_update(double *st, const osg_pio_camera *cams, int n_cams, const double *pu)
{
    double Rwb[9], E[9], Rn[9], dt[3];
#pragma unroll
    for (int i = 0; i < 9; i++) Rwb[i] = st[K_RWB + i];
    m3_vec(Rwb, pu + 3, dt);
#pragma unroll
    for (int i = 0; i < 3; i++) st[K_TWB + i] += dt[i];
    exp_so3(pu, E);
    m3_mul(Rwb, E, Rn);
    int its = (int)st[K_ITS] + 1;
    if (its >= 3) {
        normalize_rotation<double>(Rn);
        its = 0;
    }
    st[K_ITS] = (double)its;
#pragma unroll
    for (int i = 0; i < 9; i++) st[K_RWB + i] = Rn[i];
    double Rbw[9], tbw[3], twb[3];
    m3_t(Rn, Rbw);
#pragma unroll
    for (int i = 0; i < 3; i++) twb[i] = st[K_TWB + i];
    m3_vec(Rbw, twb, tbw);
#pragma unroll
    for (int i = 0; i < 3; i++) tbw[i] = -tbw[i];
    for (int c = 0; c < n_cams; c++) {
        double Rcb[9], Rcw[9], t[3];
#pragma unroll
        for (int i = 0; i < 9; i++) Rcb[i] = cams[c].Rcb[i];
        m3_mul(Rcb, Rbw, Rcw);
        m3_vec(Rcb, tbw, t);
#pragma unroll
        for (int i = 0; i < 9; i++) st[K_RCW + 9 * c + i] = Rcw[i];
#pragma unroll
        for (int i = 0; i < 3; i++) st[K_TCW + 3 * c + i] = t[i] + cams[c].tcb[i];
    }
}

// Xc of point X in camera ci of the state st
__device__ __forceinline__ void visual_xc(const double *st, int ci, const double *X, double *Xc)
{
    const double *R = st + K_RCW + 9 * ci, *t = st + K_TCW + 3 * ci;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        double s = R[3 * i] * X[0];
        s += R[3 * i + 1] * X[1];
        s += R[3 * i + 2] * X[2];
        Xc[i] = s + t[i];
    }
}

// EdgeMono / EdgeStereo computeError: obs - Project / ProjectStereo (ref:src/G2oTypes.cc:188-207); err[2] = 0 for mono
__device__ __forceinline__ void visual_error(const osg_camera &cam, double bf, int kind, const double *Xc,
                                             const double *obs, double *err)
{
    double uv[2];
    osgba::cam_project(cam, Xc, uv);
    err[0] = obs[0] - uv[0];
    err[1] = obs[1] - uv[1];
    err[2] = 0.0;
    if (kind == OSG_EDGE_STEREO) {
        const double invZ = 1 / Xc[2];
        err[2] = obs[2] - (uv[0] - bf * invZ);
    }
}

// linearizeOplus of the two-vertex edges: Jl = -proj_jac Rcw (the point), Jp = proj_jac Rcb SE3deriv(Xb) (the pose);
// row 2 is zero for mono edges
__device__ inline void visual_jacobians(const double *st, const osg_pio_camera &K, double bf, int kind, int ci,
                                        const double *Xc, double Jp[3][6], double Jl[3][3])
{
    double Xb[3];
#pragma unroll
    for (int i = 0; i < 3; i++) {  // Rbc = Rcb'
        double s = K.Rcb[i] * Xc[0];
        s += K.Rcb[3 + i] * Xc[1];
        s += K.Rcb[6 + i] * Xc[2];
        Xb[i] = s + K.tbc[i];
    }
    double PJ[3][3];
    {
        double PJ2[2][3];
        osgba::cam_project_jac(K.cam, Xc, PJ2);
#pragma unroll
        for (int j = 0; j < 3; j++) {
            PJ[0][j] = PJ2[0][j];
            PJ[1][j] = PJ2[1][j];
            PJ[2][j] = 0.0;
        }
    }
    if (kind == OSG_EDGE_STEREO) {
        const double inv_z2 = 1.0 / (Xc[2] * Xc[2]);
#pragma unroll
        for (int j = 0; j < 3; j++) PJ[2][j] = PJ[0][j];
        PJ[2][2] += bf * inv_z2;
    }
    const double *Rcw = st + K_RCW + 9 * ci;
    const double x = Xb[0], y = Xb[1], z = Xb[2];
#pragma unroll
    for (int r = 0; r < 3; r++) {
        double M[3];
#pragma unroll
        for (int j = 0; j < 3; j++) {
            double s = PJ[r][0] * K.Rcb[j];
            s += PJ[r][1] * K.Rcb[3 + j];
            s += PJ[r][2] * K.Rcb[6 + j];
            M[j] = s;
            double l = -PJ[r][0] * Rcw[j];
            l += -PJ[r][1] * Rcw[3 + j];
            l += -PJ[r][2] * Rcw[6 + j];
            Jl[r][j] = l;
        }
        Jp[r][0] = M[1] * -z + M[2] * y;
        Jp[r][1] = M[0] * z + M[2] * -x;
        Jp[r][2] = M[0] * -y + M[1] * x;
        Jp[r][3] = M[0];
        Jp[r][4] = M[1];
        Jp[r][5] = M[2];
    }
}

// IMU::Preintegrated as EdgeInertial reads it
struct Preint {
    const float *dR, *dV, *dP, *JRg, *JVg, *JVa, *JPg, *JPa, *b;
    float dT;
};

// EdgeInertial::computeError into e[9] and, with J, linearizeOplus into the row-major 9 x 24 J over the columns
// VP1 6 | VV1 3 | VG1 3 | VA1 3 | VP2 6 | VV2 3 (J is zeroed here).  s1, s2: the states of the two KeyFrames.
__device__ inline void inertial_edge(const double *s1, const double *s2, const Preint &P, double *e, double *J)
{
    // IMU::Bias holds floats; the preintegration getters work in float (ref:src/ImuTypes.cc:376-426)
    float dbg[3], dba[3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        dbg[i] = (float)s1[K_BG + i] - P.b[3 + i];
        dba[i] = (float)s1[K_BA + i] - P.b[i];
    }
    float wf[3], Ef[9], dRf[9], t1[3], t2[3];
    m3_vec(P.JRg, dbg, wf);
    so3f_exp_matrix(wf, Ef);
    m3_mul(P.dR, Ef, dRf);
    normalize_rotation<float>(dRf);
    double dR[9], dV[3], dP[3];
    m3_vec(P.JVg, dbg, t1);
    m3_vec(P.JVa, dba, t2);
#pragma unroll
    for (int i = 0; i < 3; i++) dV[i] = (double)((P.dV[i] + t1[i]) + t2[i]);
    m3_vec(P.JPg, dbg, t1);
    m3_vec(P.JPa, dba, t2);
#pragma unroll
    for (int i = 0; i < 3; i++) dP[i] = (double)((P.dP[i] + t1[i]) + t2[i]);
#pragma unroll
    for (int i = 0; i < 9; i++) dR[i] = (double)dRf[i];

    const double dt = (double)P.dT;
    const double g[3] = {0.0, 0.0, -(double)9.81f};
    double Rwb1[9], Rbw1[9], Rwb2[9], dRt[9], A[9], eR[9], er[3];
#pragma unroll
    for (int i = 0; i < 9; i++) {
        Rwb1[i] = s1[K_RWB + i];
        Rwb2[i] = s2[K_RWB + i];
    }
    m3_t(Rwb1, Rbw1);
    m3_t(dR, dRt);
    m3_mul(dRt, Rbw1, A);
    m3_mul(A, Rwb2, eR);
    log_so3(eR, er);
    double a[3], bvec[3], ra[3], rb[3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        a[i] = s2[K_V + i] - s1[K_V + i] - g[i] * dt;
        bvec[i] = s2[K_TWB + i] - s1[K_TWB + i] - s1[K_V + i] * dt - g[i] * dt * dt / 2;
    }
    m3_vec(Rbw1, a, ra);
    m3_vec(Rbw1, bvec, rb);
#pragma unroll
    for (int i = 0; i < 3; i++) {
        e[i] = er[i];
        e[3 + i] = ra[i] - dV[i];
        e[6 + i] = rb[i] - dP[i];
    }
    if (!J) return;
    for (int i = 0; i < 9 * 24; i++) J[i] = 0.0;
    double invJr[9], R12[9], Rbw2[9], B[9], C[9], Hh[9];
    inv_right_jacobian_so3(er, invJr);
    m3_mul(Rbw1, Rwb2, R12);
    m3_t(Rwb2, Rbw2);
    m3_mul(invJr, Rbw2, B);
    m3_mul(B, Rwb1, C);  // invJr Rwb2' Rwb1
    // the reference writes 0.5 * g * dt * dt here and g * dt * dt / 2 in computeError
#pragma unroll
    for (int i = 0; i < 3; i++) bvec[i] = s2[K_TWB + i] - s1[K_TWB + i] - s1[K_V + i] * dt - 0.5 * g[i] * dt * dt;
    m3_vec(Rbw1, bvec, rb);
    // gyro bias: -invJr eR' RightJacobianSO3(JRg dbg) JRg, with GetDeltaBias' float difference cast to double
    double JRg[9], dbgd[3], w[3], Jr[9], eRt[9], D[9], E2[9], F[9];
#pragma unroll
    for (int i = 0; i < 9; i++) JRg[i] = (double)P.JRg[i];
#pragma unroll
    for (int i = 0; i < 3; i++) dbgd[i] = (double)dbg[i];
    m3_vec(JRg, dbgd, w);
    right_jacobian_so3(w, Jr);
    m3_t(eR, eRt);
    m3_mul(invJr, eRt, D);
    m3_mul(D, Jr, E2);
    m3_mul(E2, JRg, F);
    hat3(ra, Hh);
    double Hb[9];
    hat3(rb, Hb);
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const int q = 3 * i + j;
            // pose 1
            J[24 * i + j] = -C[q];
            J[24 * (3 + i) + j] = Hh[q];
            J[24 * (6 + i) + j] = Hb[q];
            J[24 * (6 + i) + 3 + j] = i == j ? -1.0 : 0.0;
            // velocity 1
            J[24 * (3 + i) + 6 + j] = -Rbw1[q];
            J[24 * (6 + i) + 6 + j] = -Rbw1[q] * dt;
            // gyro bias 1
            J[24 * i + 9 + j] = -F[q];
            J[24 * (3 + i) + 9 + j] = -(double)P.JVg[q];
            J[24 * (6 + i) + 9 + j] = -(double)P.JPg[q];
            // accelerometer bias 1
            J[24 * (3 + i) + 12 + j] = -(double)P.JVa[q];
            J[24 * (6 + i) + 12 + j] = -(double)P.JPa[q];
            // pose 2
            J[24 * i + 15 + j] = invJr[q];
            J[24 * (6 + i) + 18 + j] = R12[q];
            // velocity 2
            J[24 * (3 + i) + 21 + j] = Rbw1[q];
        }
}

}  // namespace osgiba
