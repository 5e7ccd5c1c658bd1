// so3_common.h — NormalizeRotation and the SO(3) functions of ref:src/G2oTypes.cc:906-984, and Sophus's SO3f exp,
// shared by the inertial kernels (poseinertial.hip, preintegrate.hip, the 4-DoF pose graph of essgraph.hip) and
// the host entry points of imu_common.h.  Plain OSG_HD code over small_linalg.h, no HIP runtime header: host and
// device run the same functions.  Row-major.
#pragma once
#include <cmath>

#include "small_linalg.h"

namespace osgso3 {

using namespace osgla;

// NormalizeRotation (ref:include/G2oTypes.h:67-72): U V' of the SVD of R, here as the polar factor
// R (R'R)^(-1/2) with R'R diagonalised by three-by-three cyclic Jacobi, in T's arithmetic
template <class T>
OSG_HD inline void normalize_rotation(T *R)
{
    using std::fabs;
    using std::sqrt;
    T B[3][3], V[3][3];
    OSG_UNROLL
    for (int i = 0; i < 3; i++)
        OSG_UNROLL
        for (int j = 0; j < 3; j++) {
            T s = R[i] * R[j];
            s += R[3 + i] * R[3 + j];
            s += R[6 + i] * R[6 + j];
            B[i][j] = s;
            V[i][j] = i == j ? T(1) : T(0);
        }
    // jacobi_sym<T, 3>'s loop, kept in line: through the call the same arithmetic costs k_imu_preintegrate 20
    // bytes of scratch per lane and k_eg4_update eight VGPRs
    const T tol = sizeof(T) == 8 ? T(1e-34) : T(1e-16);
    OSG_UNROLL1
    for (int sweep = 0; sweep < 12; sweep++) {
        const T off = B[0][1] * B[0][1] + B[0][2] * B[0][2] + B[1][2] * B[1][2];
        const T diag = B[0][0] * B[0][0] + B[1][1] * B[1][1] + B[2][2] * B[2][2];
        if (!(off > tol * diag)) break;
        OSG_UNROLL
        for (int p = 0; p < 2; p++)
            OSG_UNROLL
            for (int q = p + 1; q < 3; q++) {
                const T apq = B[p][q];
                if (apq == T(0)) continue;
                const T th = (B[q][q] - B[p][p]) / (T(2) * apq);
                const T tt = (th >= T(0) ? T(1) : T(-1)) / (fabs(th) + sqrt(th * th + T(1)));
                const T c = T(1) / sqrt(tt * tt + T(1)), s = tt * c;
                OSG_UNROLL
                for (int k = 0; k < 3; k++) {
                    const T akp = B[k][p], akq = B[k][q];
                    B[k][p] = c * akp - s * akq;
                    B[k][q] = s * akp + c * akq;
                }
                OSG_UNROLL
                for (int k = 0; k < 3; k++) {
                    const T apk = B[p][k], aqk = B[q][k];
                    B[p][k] = c * apk - s * aqk;
                    B[q][k] = s * apk + c * aqk;
                }
                OSG_UNROLL
                for (int k = 0; k < 3; k++) {
                    const T vkp = V[k][p], vkq = V[k][q];
                    V[k][p] = c * vkp - s * vkq;
                    V[k][q] = s * vkp + c * vkq;
                }
            }
    }
    T isq[3], M[9], O[9];
    OSG_UNROLL
    for (int k = 0; k < 3; k++) isq[k] = T(1) / sqrt(B[k][k]);
    OSG_UNROLL
    for (int i = 0; i < 3; i++)
        OSG_UNROLL
        for (int j = 0; j < 3; j++) {
            T s = V[i][0] * isq[0] * V[j][0];
            s += V[i][1] * isq[1] * V[j][1];
            s += V[i][2] * isq[2] * V[j][2];
            M[3 * i + j] = s;
        }
    m3_mul(R, M, O);
    OSG_UNROLL
    for (int i = 0; i < 9; i++) R[i] = O[i];
}

// ref:src/G2oTypes.cc:912-928
OSG_HD inline void exp_so3(const double *w, double *R)
{
    using std::cos;
    using std::sin;
    using std::sqrt;
    const double x = w[0], y = w[1], z = w[2];
    const double d2 = x * x + y * y + z * z;
    const double d = sqrt(d2);
    double W[9], W2[9];
    hat3(w, W);
    m3_mul(W, W, W2);
    if (d < 1e-5) {
        OSG_UNROLL
        for (int i = 0; i < 9; i++) R[i] = ((i % 4 == 0) ? 1.0 : 0.0) + W[i] + 0.5 * W2[i];
    } else {
        const double sd = sin(d), cd = cos(d);
        OSG_UNROLL
        for (int i = 0; i < 9; i++) R[i] = ((i % 4 == 0) ? 1.0 : 0.0) + W[i] * sd / d + W2[i] * (1.0 - cd) / d2;
    }
    normalize_rotation<double>(R);
}
// ref:src/G2oTypes.cc:930-944, the 0.5f and both early returns as written
OSG_HD inline void log_so3(const double *R, double *w)
{
    using std::acos;
    using std::fabs;
    using std::sin;
    const double tr = R[0] + R[4] + R[8];
    w[0] = (R[7] - R[5]) / 2;
    w[1] = (R[2] - R[6]) / 2;
    w[2] = (R[3] - R[1]) / 2;
    const double costheta = (tr - 1.0) * 0.5f;
    if (costheta > 1 || costheta < -1) return;
    const double theta = acos(costheta);
    const double s = sin(theta);
    if (fabs(s) < 1e-5) return;
    OSG_UNROLL
    for (int i = 0; i < 3; i++) w[i] = theta * w[i] / s;
}

// ref:src/G2oTypes.cc:951-962
OSG_HD inline void inv_right_jacobian_so3(const double *v, double *J)
{
    using std::cos;
    using std::sin;
    using std::sqrt;
    const double d2 = v[0] * v[0] + v[1] * v[1] + v[2] * v[2];
    const double d = sqrt(d2);
    double W[9], W2[9];
    hat3(v, W);
    m3_mul(W, W, W2);
    if (d < 1e-5) {
        OSG_UNROLL
        for (int i = 0; i < 9; i++) J[i] = (i % 4 == 0) ? 1.0 : 0.0;
    } else {
        const double f = 1.0 / d2 - (1.0 + cos(d)) / (2.0 * d * sin(d));
        OSG_UNROLL
        for (int i = 0; i < 9; i++) J[i] = ((i % 4 == 0) ? 1.0 : 0.0) + W[i] / 2 + W2[i] * f;
    }
}
// ref:src/G2oTypes.cc:969-984
OSG_HD inline void right_jacobian_so3(const double *v, double *J)
{
    using std::cos;
    using std::sin;
    using std::sqrt;
    const double d2 = v[0] * v[0] + v[1] * v[1] + v[2] * v[2];
    const double d = sqrt(d2);
    double W[9], W2[9];
    hat3(v, W);
    m3_mul(W, W, W2);
    if (d < 1e-5) {
        OSG_UNROLL
        for (int i = 0; i < 9; i++) J[i] = (i % 4 == 0) ? 1.0 : 0.0;
    } else {
        const double sd = sin(d), cd = cos(d);
        OSG_UNROLL
        for (int i = 0; i < 9; i++) J[i] = ((i % 4 == 0) ? 1.0 : 0.0) - W[i] * (1.0 - cd) / d2 + W2[i] * (d - sd) / (d2 * d);
    }
}

// Sophus::SO3f::exp(w).matrix(): the unit quaternion (cos(theta / 2), sin(theta / 2) w / theta), Taylor below
// theta^2 < 1e-10, then Eigen's toRotationMatrix
OSG_HD inline void so3f_exp_matrix(const float *w, float *R)
{
    const float theta_sq = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
    float imag, real;
    if (theta_sq < 1e-5f * 1e-5f) {
        const float theta_po4 = theta_sq * theta_sq;
        imag = 0.5f - (1.0f / 48.0f) * theta_sq + (1.0f / 3840.0f) * theta_po4;
        real = 1.0f - (1.0f / 8.0f) * theta_sq + (1.0f / 384.0f) * theta_po4;
    } else {
        const float theta = std::sqrt(theta_sq);
        const float half = 0.5f * theta;
        imag = std::sin(half) / theta;
        real = std::cos(half);
    }
    const float x = imag * w[0], y = imag * w[1], z = imag * w[2], qw = real;
    const float tx = 2 * x, ty = 2 * y, tz = 2 * z;
    const float twx = tx * qw, twy = ty * qw, twz = tz * qw;
    const float txx = tx * x, txy = ty * x, txz = tz * x;
    const float tyy = ty * y, tyz = tz * y, tzz = tz * z;
    R[0] = 1 - (tyy + tzz); R[1] = txy - twz; R[2] = txz + twy;
    R[3] = txy + twz; R[4] = 1 - (txx + tzz); R[5] = tyz - twx;
    R[6] = txz - twy; R[7] = tyz + twx; R[8] = 1 - (txx + tyy);
}

}  // namespace osgso3
