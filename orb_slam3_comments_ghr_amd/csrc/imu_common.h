// imu_common.h — the host side of osg_imu_* that needs no device: the argument checks, the queue and
// interpolation rules of Tracking::PreintegrateIMU (ref:src/Tracking.cc:1792-1901), the bias-corrected deltas
// (ref:src/ImuTypes.cc:387-426), Tracking::PredictStateIMU (ref:src/Tracking.cc:1945-1988) and the per-problem
// block the kernel reads.  Plain C++ in float, built without FMA contraction (tests/host/imu_host.cpp compiles
// it with the host sanitizers).
#pragma once
#include <cmath>
#include <cstring>

#include "../../include/osg_imu.h"

namespace osgimu {

// what the kernel reads of one problem (the measurement lists are concatenated over the batch, shared ones once)
struct ProbDev {
    int32_t n, meas_off, has_init, pad;
    float bias[6], nga[6], nga_walk[6], padf[2];
    osg_imu_preintegrated init;
};

// 0, or OSG_E_INVALID with *why naming the first violated condition
inline int check(const osg_imu_problem *p, const char **why)
{
    const char *dummy;
    if (!why) why = &dummy;
#define OSGIMU_BAD(cond, msg) \
    if (cond) {               \
        *why = msg;           \
        return OSG_E_INVALID; \
    }
    OSGIMU_BAD(!p, "null problem");
    OSGIMU_BAD(p->n < 0, "negative n");
    OSGIMU_BAD(p->n > OSG_IMU_MAX_STEPS, "more than OSG_IMU_MAX_STEPS steps");
    OSGIMU_BAD(p->n > 0 && !p->meas, "null measurement list");
    for (int i = 0; i < p->n; i++) {
        const float dt = p->meas[7 * i + 6];
        OSGIMU_BAD(!std::isfinite(dt) || !(dt > 0.f), "a dt that is not finite or not positive");
    }
#undef OSGIMU_BAD
    return 0;
}

inline void pack(const osg_imu_problem &p, int meas_off, ProbDev &d)
{
    std::memset(&d, 0, sizeof d);
    d.n = p.n;
    d.meas_off = meas_off;
    d.has_init = p.init != nullptr;
    std::memcpy(d.bias, p.bias, sizeof d.bias);
    std::memcpy(d.nga, p.nga, sizeof d.nga);
    std::memcpy(d.nga_walk, p.nga_walk, sizeof d.nga_walk);
    if (p.init) d.init = *p.init;
}

inline int select(const double *t, int32_t n_queue, double t_prev, double t_cur, double imu_per, int32_t *taken,
                  int32_t *n_popped)
{
    if (n_queue < 0 || (n_queue > 0 && (!t || !taken)) || !n_popped) return OSG_E_INVALID;
    int n_taken = 0, at = 0;
    while (at < n_queue) {
        if (t[at] < t_prev - imu_per) {
            at++;
        } else if (t[at] < t_cur - imu_per) {
            taken[n_taken++] = at++;
        } else {
            taken[n_taken++] = at;
            break;
        }
    }
    *n_popped = at;
    return n_taken;
}

inline int integrables(const float *a, const float *w, const double *t, int32_t m, double t_prev, double t_cur,
                       float *meas)
{
    if (m < 1 || !a || !w || !t || (m > 1 && !meas)) return OSG_E_INVALID;
    const int n = m - 1;
    for (int i = 0; i < n; i++) {
        const float *a0 = a + 3 * i, *a1 = a0 + 3, *w0 = w + 3 * i, *w1 = w0 + 3;
        float *o = meas + 7 * i;
        float tstep;
        if (i == 0 && i < n - 1) {
            const float tab = (float)(t[i + 1] - t[i]);
            const float tini = (float)(t[i] - t_prev);
            const float r = tini / tab;
            for (int k = 0; k < 3; k++) {
                o[k] = ((a0[k] + a1[k]) - (a1[k] - a0[k]) * r) * 0.5f;
                o[3 + k] = ((w0[k] + w1[k]) - (w1[k] - w0[k]) * r) * 0.5f;
            }
            tstep = (float)(t[i + 1] - t_prev);
        } else if (i < n - 1) {
            for (int k = 0; k < 3; k++) {
                o[k] = (a0[k] + a1[k]) * 0.5f;
                o[3 + k] = (w0[k] + w1[k]) * 0.5f;
            }
            tstep = (float)(t[i + 1] - t[i]);
        } else if (i > 0) {
            const float tab = (float)(t[i + 1] - t[i]);
            const float tend = (float)(t[i + 1] - t_cur);
            const float r = tend / tab;
            for (int k = 0; k < 3; k++) {
                o[k] = ((a0[k] + a1[k]) - (a1[k] - a0[k]) * r) * 0.5f;
                o[3 + k] = ((w0[k] + w1[k]) - (w1[k] - w0[k]) * r) * 0.5f;
            }
            tstep = (float)(t_cur - t[i]);
        } else {
            for (int k = 0; k < 3; k++) {
                o[k] = a0[k];
                o[3 + k] = w0[k];
            }
            tstep = (float)(t_cur - t_prev);
        }
        o[6] = tstep;
    }
    return n;
}

inline void m3_mul(const float *A, const float *B, float *C)
{
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            float s = A[3 * i] * B[j];
            s += A[3 * i + 1] * B[3 + j];
            s += A[3 * i + 2] * B[6 + j];
            C[3 * i + j] = s;
        }
}
inline void m3_vec(const float *A, const float *x, float *y)
{
    for (int i = 0; i < 3; i++) {
        float s = A[3 * i] * x[0];
        s += A[3 * i + 1] * x[1];
        s += A[3 * i + 2] * x[2];
        y[i] = s;
    }
}

// IMU::NormalizeRotation as the polar factor R (R'R)^(-1/2), R'R diagonalised by cyclic Jacobi: the host
// twin of osgso3::normalize_rotation<float>
inline void normalize_rotation(float *R)
{
    float B[3][3], V[3][3];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            float s = R[i] * R[j];
            s += R[3 + i] * R[3 + j];
            s += R[6 + i] * R[6 + j];
            B[i][j] = s;
            V[i][j] = i == j ? 1.f : 0.f;
        }
    for (int sweep = 0; sweep < 12; sweep++) {
        const float off = B[0][1] * B[0][1] + B[0][2] * B[0][2] + B[1][2] * B[1][2];
        const float diag = B[0][0] * B[0][0] + B[1][1] * B[1][1] + B[2][2] * B[2][2];
        if (!(off > 1e-16f * diag)) break;
        for (int p = 0; p < 2; p++)
            for (int q = p + 1; q < 3; q++) {
                const float apq = B[p][q];
                if (apq == 0.f) continue;
                const float th = (B[q][q] - B[p][p]) / (2.f * apq);
                const float tt = (th >= 0.f ? 1.f : -1.f) / (std::fabs(th) + std::sqrt(th * th + 1.f));
                const float c = 1.f / std::sqrt(tt * tt + 1.f), s = tt * c;
                for (int k = 0; k < 3; k++) {
                    const float akp = B[k][p], akq = B[k][q];
                    B[k][p] = c * akp - s * akq;
                    B[k][q] = s * akp + c * akq;
                }
                for (int k = 0; k < 3; k++) {
                    const float apk = B[p][k], aqk = B[q][k];
                    B[p][k] = c * apk - s * aqk;
                    B[q][k] = s * apk + c * aqk;
                }
                for (int k = 0; k < 3; k++) {
                    const float vkp = V[k][p], vkq = V[k][q];
                    V[k][p] = c * vkp - s * vkq;
                    V[k][q] = s * vkp + c * vkq;
                }
            }
    }
    float isq[3], M[9], O[9];
    for (int k = 0; k < 3; k++) isq[k] = 1.f / std::sqrt(B[k][k]);
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            float s = V[i][0] * isq[0] * V[j][0];
            s += V[i][1] * isq[1] * V[j][1];
            s += V[i][2] * isq[2] * V[j][2];
            M[3 * i + j] = s;
        }
    m3_mul(R, M, O);
    for (int i = 0; i < 9; i++) R[i] = O[i];
}

// Sophus::SO3f::exp(w).matrix(): the unit quaternion of the half angle (Taylor below theta^2 < 1e-10), then
// Eigen's toRotationMatrix; the host twin of so3f_exp_matrix in poseinertial.hip
inline void so3f_exp_matrix(const float *w, float *R)
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
    R[0] = 1 - (tyy + tzz), R[1] = txy - twz, R[2] = txz + twy;
    R[3] = txy + twz, R[4] = 1 - (txx + tzz), R[5] = tyz - twx;
    R[6] = txz - twy, R[7] = tyz + twx, R[8] = 1 - (txx + tyy);
}

inline void delta(const osg_imu_preintegrated *s, const float *bias, float *dR, float *dV, float *dP)
{
    const osg_pio_preintegrated &q = s->pre;
    float dba[3], dbg[3];
    for (int i = 0; i < 3; i++) {
        dba[i] = bias[i] - q.b[i];
        dbg[i] = bias[3 + i] - q.b[3 + i];
    }
    if (dR) {
        float w[3], E[9];
        m3_vec(q.JRg, dbg, w);
        so3f_exp_matrix(w, E);
        m3_mul(q.dR, E, dR);
        normalize_rotation(dR);
    }
    float t1[3], t2[3];
    if (dV) {
        m3_vec(q.JVg, dbg, t1);
        m3_vec(q.JVa, dba, t2);
        for (int i = 0; i < 3; i++) dV[i] = (q.dV[i] + t1[i]) + t2[i];
    }
    if (dP) {
        m3_vec(q.JPg, dbg, t1);
        m3_vec(q.JPa, dba, t2);
        for (int i = 0; i < 3; i++) dP[i] = (q.dP[i] + t1[i]) + t2[i];
    }
}

inline void predict_state(const osg_imu_preintegrated *s, const float *bias, const float *Rwb1, const float *twb1,
                          const float *vwb1, float *Rwb2, float *twb2, float *vwb2)
{
    const float Gz[3] = {0.f, 0.f, -9.81f};
    const float t12 = s->pre.dT;
    float dR[9], dV[3], dP[3], r[3];
    delta(s, bias, dR, dV, dP);
    m3_mul(Rwb1, dR, Rwb2);
    normalize_rotation(Rwb2);
    m3_vec(Rwb1, dP, r);
    for (int i = 0; i < 3; i++) twb2[i] = ((twb1[i] + vwb1[i] * t12) + ((0.5f * t12) * t12) * Gz[i]) + r[i];
    m3_vec(Rwb1, dV, r);
    for (int i = 0; i < 3; i++) vwb2[i] = (vwb1[i] + t12 * Gz[i]) + r[i];
}

}  // namespace osgimu
