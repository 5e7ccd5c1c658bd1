// imu_common.h — the host side of osg_imu_* that needs no device: the argument checks, the queue and
// interpolation rules of Tracking::PreintegrateIMU (ref:src/Tracking.cc:1792-1901), the bias-corrected deltas
// (ref:src/ImuTypes.cc:387-426), Tracking::PredictStateIMU (ref:src/Tracking.cc:1945-1988) and the per-problem
// block the kernel reads.  Plain C++ in float, built without FMA contraction (tests/host/imu_host.cpp compiles
// it with the host sanitizers).
#pragma once
#include <cmath>
#include <cstring>

#include "../../include/osg_imu.h"
#include "so3_common.h"

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

// the bias-corrected deltas and PredictStateIMU, on the SO(3) functions the kernels run (so3_common.h)
using osgla::m3_mul;
using osgla::m3_vec;
using osgso3::normalize_rotation;
using osgso3::so3f_exp_matrix;

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
        normalize_rotation<float>(dR);
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
    normalize_rotation<float>(Rwb2);
    m3_vec(Rwb1, dP, r);
    for (int i = 0; i < 3; i++) twb2[i] = ((twb1[i] + vwb1[i] * t12) + ((0.5f * t12) * t12) * Gz[i]) + r[i];
    m3_vec(Rwb1, dV, r);
    for (int i = 0; i < 3; i++) vwb2[i] = (vwb1[i] + t12 * Gz[i]) + r[i];
}

}  // namespace osgimu
