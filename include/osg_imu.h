/* osg_imu.h — IMU preintegration: IMU::Preintegrated (ref:src/ImuTypes.cc:38-151, 206-456) in float32, as the
 * reference is, and the host rules around it of Tracking::PreintegrateIMU and Tracking::PredictStateIMU.
 *
 * The device has one job: integrate B independent measurement lists in one launch, each either continued from
 * an existing state or started from Initialize(bias).  Reintegrate() is Initialize(bu) plus the whole list;
 * MergePrevious() is Initialize(bu) plus the previous list followed by the own one; Tracking::PreintegrateIMU
 * integrates one list onto two states (the one continued from the last KeyFrame, the one fresh from the last
 * frame's bias).  All three are the same call with different arguments.  Parity with the reference is
 * tolerance-based. */
#ifndef OSG_IMU_H
#define OSG_IMU_H

#include "osg.h"
#include "osg_ba.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the longest list of one problem: the reference allows 3 s between KeyFrames, 600 steps at 200 Hz */
#define OSG_IMU_MAX_STEPS 65536
/* the steps of one batch, shared lists counted once */
#define OSG_IMU_MAX_BATCH_STEPS (1 << 24)

/* IMU::Preintegrated: what EdgeInertial reads (pre feeds osg_pose_inertial_problem.preint with no conversion)
 * and the two running means (Tracking::NeedNewKeyFrame's siblings read avgA, ref:src/Tracking.cc:2768). */
typedef struct osg_imu_preintegrated {
    osg_pio_preintegrated pre;
    float avgA[3], avgW[3];
} osg_imu_preintegrated;

typedef struct osg_imu_problem {
    const float *meas;        /* 7 floats per step: ax ay az wx wy wz dt (mvMeasurements); two problems may point
                                 at the same list */
    int32_t n;                /* steps; 0 returns the initial state */
    float bias[6];            /* (bax, bay, baz, bwx, bwy, bwz); read when init is NULL */
    float nga[6];             /* diagonal of Calib::Cov: (ng2, ng2, ng2, na2, na2, na2) */
    float nga_walk[6];        /* diagonal of Calib::CovWalk: (ngw2 x 3, naw2 x 3) */
    const osg_imu_preintegrated *init; /* NULL: Initialize(bias).  Otherwise continue from *init, and the bias of
                                 the integration is init->pre.b */
} osg_imu_problem;

/* 0 or a negative OSG_E_* code.  OSG_E_INVALID (nothing written, the context stays usable): a null pointer, a
 * negative n, n above OSG_IMU_MAX_STEPS, meas NULL with n > 0, a dt that is not finite or not > 0 (the
 * reference divides 0 by 0 in avgA on a first step with dt == 0; this call refuses it instead). */
int osg_imu_preintegrate(struct osg_ctx *ctx, const osg_imu_problem *p, osg_imu_preintegrated *out);
/* n independent integrations in one launch; additionally OSG_E_INVALID when the lists together exceed
 * OSG_IMU_MAX_BATCH_STEPS.  Returns 0 or a negative OSG_E_* code. */
int osg_imu_preintegrate_batch(struct osg_ctx *ctx, const osg_imu_problem *p, int32_t n,
                               osg_imu_preintegrated *out);
/* The argument checks of one problem alone (host only, needs no context): 0 or OSG_E_INVALID. */
int osg_imu_preintegrate_check(const osg_imu_problem *p);

/* ---- host helpers (no context, no GPU) ------------------------------------------------------------------ */

/* The queue rule of Tracking::PreintegrateIMU (ref:src/Tracking.cc:1792-1829) over the n_queue timestamps of
 * mlQueueImuData from its front: a point before t_prev - imu_per is dropped, one before t_cur - imu_per is taken
 * and popped, the next is taken, left in the queue, and ends the walk.  taken[] (capacity n_queue) receives the
 * queue indices of mvImuFromLastFrame in order, *n_popped how many entries left the queue's front.  Returns the
 * number taken, or OSG_E_INVALID for null pointers or a negative n_queue. */
int osg_imu_select(const double *t, int32_t n_queue, double t_prev, double t_cur, double imu_per, int32_t *taken,
                   int32_t *n_popped);
/* The midpoint and interpolation rule of ref:src/Tracking.cc:1851-1901: m IMU points (a, w: 3 floats each, t
 * double) between the frames at t_prev and t_cur give m - 1 steps of 7 floats in meas.  Timestamps are double;
 * tab, tini, tend and tstep are rounded to float, as in the reference.  Returns m - 1, or OSG_E_INVALID for
 * null pointers or m < 1. */
int osg_imu_integrables(const float *a, const float *w, const double *t, int32_t m, double t_prev, double t_cur,
                        float *meas);
/* GetDeltaRotation / GetDeltaVelocity / GetDeltaPosition(bias) (ref:src/ImuTypes.cc:387-426), bias as
 * (ba, bg); passing bu serves the GetUpdated* forms.  dR[9] row-major, dV[3], dP[3]; any output may be NULL. */
void osg_imu_delta(const osg_imu_preintegrated *pre, const float *bias, float *dR, float *dV, float *dP);
/* Tracking::PredictStateIMU (ref:src/Tracking.cc:1945-1988): the caller passes the last KeyFrame's body pose,
 * velocity and bias with mpImuPreintegratedFromLastKF (the map was updated), or the last frame's with
 * mpImuPreintegratedFrame (it was not).  GRAVITY_VALUE is the float 9.81f. */
void osg_imu_predict_state(const osg_imu_preintegrated *pre, const float *bias, const float *Rwb1,
                           const float *twb1, const float *vwb1, float *Rwb2, float *twb2, float *vwb2);

#ifdef __cplusplus
}
#endif
#endif
