/*
 * osg_ba.h — C ABI of the bundle-adjustment half of the hot path.
 *
 *   osg_pose_optimization[_batch]  ← Optimizer::PoseOptimization(Frame*)        ref:src/Optimizer.cc:71-420
 *   osg_pose_inertial_optimization[_batch]
 *                                  ← Optimizer::PoseInertialOptimizationLastKeyFrame / LastFrame
 *                                    (ref:src/Optimizer.cc:435-987, 1002-1744)
 *   osg_local_bundle_adjustment    ← the g2o part of Optimizer::LocalBundleAdjustment
 *                                    (ref:src/Optimizer.cc:1877-2203: graph → optimize(10) →
 *                                    outlier classification → estimates out)
 *   osg_bundle_adjustment          ← the g2o part of Optimizer::BundleAdjustment (global BA,
 *                                    ref:src/Optimizer.cc:2850-3237)
 *   osg_optimize_sim3[_batch]      ← Optimizer::OptimizeSim3                   ref:src/Optimizer.cc:4213-4512
 *   osg_sim3_ransac[_batch]        ← Sim3Solver::find / iterate                 ref:src/Sim3Solver.cc:146-433
 *   osg_mlpnp_ransac[_batch]       ← MLPnPsolver::iterate                       ref:src/MLPnPsolver.cpp:145-1160
 *
 * The caller (the ORB-SLAM3 side adapter) gathers the graph exactly as the
 * reference builds it — the same vertices, the same edges in the same insertion order, the same
 * float→double casts — and applies the returned estimates / outlier flags under the reference's
 * locks.  Inside, the g2o LM + BlockSolver_6_3 semantics are reproduced:
 * ref:Thirdparty/g2o/g2o/core/optimization_algorithm_levenberg.cpp:61-194,
 * ref:Thirdparty/g2o/g2o/core/block_solver.hpp:143-604, ref:Thirdparty/g2o/g2o/core/sparse_optimizer.cpp:61-552.
 *
 * Poses are SE3 as 7 doubles {qx, qy, qz, qw, tx, ty, tz} (g2o::SE3Quat; Tcw = world→camera).
 */
#ifndef OSG_BA_H
#define OSG_BA_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

struct osg_ctx;

/* camera model, ref:include/CameraModels/GeometricCamera.h:115 (vector<float> mvParameters) */
#define OSG_CAM_PINHOLE 0 /* ref:src/CameraModels/Pinhole.cpp:50-133 */
#define OSG_CAM_KB8 1     /* ref:src/CameraModels/KannalaBrandt8.cpp:62-260 */

/* edge kinds (ref:include/OptimizableTypes.h:32-158, ref:Thirdparty/g2o/g2o/types/types_six_dof_expmap.h:146-235) */
#define OSG_EDGE_MONO 0   /* EdgeSE3ProjectXYZ[OnlyPose]: 2-D, pCamera->project */
#define OSG_EDGE_STEREO 1 /* EdgeStereoSE3ProjectXYZ[OnlyPose]: 3-D (u, v, ur), fx fy cx cy bf */
#define OSG_EDGE_BODY 2   /* EdgeSE3ProjectXYZ[OnlyPose]ToBody: 2-D, right camera through mTrl */

typedef struct osg_camera {
    int32_t type;        /* OSG_CAM_* */
    float p[8];          /* mvParameters: fx fy cx cy [k1 k2 k3 k4] */
    float fx, fy, cx, cy, bf; /* Frame/KeyFrame fx..mbf (stereo edges copy these into doubles) */
    double trl[7];       /* right-from-left SE3 (GetRelativePoseTrl) for BODY edges */
} osg_camera;

/* ---- PoseOptimization ---------------------------------------------------------------------- */
typedef struct osg_pose_problem {
    double pose[7];           /* pFrame->GetPose() cast to double */
    int32_t n_edges;          /* one per Frame slot with a MapPoint, in slot order */
    const int8_t *kind;       /* OSG_EDGE_* per edge */
    const double *xw;         /* 3 per edge: GetWorldPos().cast<double>() */
    const double *obs;        /* 3 per edge: (u, v, ur) — ur only read for STEREO */
    const float *inv_sigma2;  /* mvInvLevelSigma2[octave] per edge */
    osg_camera cam;           /* mpCamera + stereo parameters */
    osg_camera cam2;          /* mpCamera2 + mTrl (BODY edges) */
} osg_pose_problem;

typedef struct osg_pose_result {
    double pose[7];           /* optimised Tcw (input pose when fewer than 3 edges) */
    uint8_t *outlier;         /* n_edges flags (mvbOutlier of each edge's slot) */
    int32_t n_inliers;        /* the reference's return value: nInitial - nBad */
    int32_t lm_iterations;    /* solve() calls over the 4 rounds */
    int32_t lm_trials;        /* linear solves (incl. rejected steps) */
} osg_pose_result;

int osg_pose_optimization(struct osg_ctx *ctx, const osg_pose_problem *p, osg_pose_result *r);
/* n independent frames in one launch (frame-batched tracking, sequences sharded over GPUs). */
int osg_pose_optimization_batch(struct osg_ctx *ctx, const osg_pose_problem *p, int32_t n,
                                osg_pose_result *r);

/* ---- PoseInertialOptimization ---------------------------------------------------------------
 * Optimizer::PoseInertialOptimizationLastKeyFrame (ref:src/Optimizer.cc:435-987) and
 * Optimizer::PoseInertialOptimizationLastFrame (ref:src/Optimizer.cc:1002-1640): what Tracking::TrackLocalMap
 * calls in place of PoseOptimization once the IMU is initialised.  The current frame's VertexPose (body pose
 * Rwb, twb), VertexVelocity, VertexGyroBias and VertexAccBias are free; the same four of the previous KeyFrame
 * are fixed (LAST_KEYFRAME) or of the previous frame free (LAST_FRAME).  Edges: one EdgeMonoOnlyPose /
 * EdgeStereoOnlyPose per gathered slot (Huber sqrt(5.991) / sqrt(7.815), removed after the third round),
 * EdgeInertial over the preintegration, EdgeGyroRW, EdgeAccRW, and in LAST_FRAME EdgePriorPoseImu (Huber 5)
 * on the previous frame.  g2o's Gauss-Newton (no damping, no trial loop) on the dense 15 x 15 / 30 x 30
 * system, four rounds of optimize(10) with the reference's classification after each, the recovery pass, and
 * the new prior's H (LAST_FRAME: marginalised onto the current frame) run in one launch, one workgroup per
 * problem.  Parity with the reference is tolerance-based. */
#define OSG_PIO_LAST_KEYFRAME 0
#define OSG_PIO_LAST_FRAME 1

typedef struct osg_pio_state {
    double Rwb[9];            /* row-major, GetImuRotation().cast<double>() */
    double twb[3];            /* GetImuPosition() */
    double v[3];              /* GetVelocity() */
    double bg[3];             /* gyro bias (bwx, bwy, bwz) */
    double ba[3];             /* accelerometer bias (bax, bay, baz) */
} osg_pio_state;

/* one camera of ImuCamPose(Frame*) (ref:src/G2oTypes.cc:81-127); the second camera of a rig through Trl */
typedef struct osg_pio_camera {
    osg_camera cam;           /* pCamera[i]: type and p[] are read */
    double Rcw[9], tcw[3];    /* as constructed from the Frame's pose; re-derived from Rwb, twb at every update */
    double Rcb[9], tcb[3];
    double tbc[3];            /* Rbc is Rcb transposed */
} osg_pio_camera;

/* IMU::Preintegrated as EdgeInertial reads it: the stored float fields (matrices row-major) */
typedef struct osg_pio_preintegrated {
    float dR[9], dV[3], dP[3];
    float JRg[9], JVg[9], JVa[9], JPg[9], JPa[9];
    float b[6];               /* the bias of the integration: (bax, bay, baz, bwx, bwy, bwz) */
    float dT;
    float C[225];             /* 15 x 15 covariance; EdgeInertial's information is derived from C[0:9, 0:9] */
} osg_pio_preintegrated;

/* ConstraintPoseImu of the previous frame (pFp->mpcpi), H as stored (after the constructor) */
typedef struct osg_pio_prior {
    double Rwb[9], twb[3], vwb[3], bg[3], ba[3];
    double H[225];
} osg_pio_prior;

typedef struct osg_pose_inertial_problem {
    int32_t mode;             /* OSG_PIO_* */
    int32_t rec_init;         /* bRecInit: no recovery pass */
    osg_pio_state cur;        /* pFrame */
    osg_pio_state prev;       /* pFrame->mpLastKeyFrame (LAST_KEYFRAME) or pFrame->mpPrevFrame (LAST_FRAME) */
    int32_t n_cams;           /* 1, or 2 when mpCamera2 */
    osg_pio_camera cams[2];
    double bf;                /* mbf cast to double */
    int32_t n_edges;          /* one per gathered slot, in slot order */
    const int8_t *kind;       /* OSG_EDGE_MONO: left or only camera; OSG_EDGE_STEREO; OSG_EDGE_BODY: right camera */
    const double *xw;         /* 3 per edge: GetWorldPos().cast<double>() */
    const double *obs;        /* 3 per edge: (u, v, ur), ur read for STEREO only */
    const float *inv_sigma2;  /* mvInvLevelSigma2[octave] / uncertainty2 */
    const float *track_depth; /* mTrackDepth, read for MONO and BODY edges only */
    const osg_pio_preintegrated *preint; /* mpImuPreintegrated (LAST_KEYFRAME) / mpImuPreintegratedFrame (LAST_FRAME) */
    const float *C_rw;        /* 225: mpImuPreintegrated->C, whose blocks (9, 9) and (12, 12) give the random-walk
                                 informations in BOTH modes (ref:src/Optimizer.cc:688, 701, 1252, 1265) */
    const osg_pio_prior *prior; /* LAST_FRAME only; NULL there is OSG_E_INVALID */
} osg_pose_inertial_problem;

typedef struct osg_pose_inertial_result {
    osg_pio_state state;      /* the current frame after the optimisation (bg, ba: mImuBias in double) */
    uint8_t *outlier;         /* n_edges: mvbOutlier of each edge's slot */
    int32_t n_inliers;        /* the reference's return value: nInitialCorrespondences - nBad */
    int32_t rounds_run;       /* 1..4 (the edges().size() < 10 break ends after the first) */
    int32_t iterations;       /* linear solves performed */
    int32_t solve_failed;     /* a pivot of the unpivoted LDL^T was not positive in some round */
    int32_t recovered;        /* the recovery pass ran (nInliers < 30 and not rec_init) */
    double H[225];            /* as passed to ConstraintPoseImu's constructor, whose own post-processing is the
                                 caller's (constraint_pose_imu in the Python package, the adapter in C++) */
    double *edge_chi2;        /* optional (NULL: not written), n_edges: as read by each edge's last classification */
} osg_pose_inertial_result;

/* Returns n_inliers or a negative OSG_E_* code.  OSG_E_INVALID (nothing written, the context stays usable): a
 * null pointer, a negative count, an unknown mode or edge kind, n_cams outside {1, 2}, a BODY edge with one
 * camera, LAST_FRAME without a prior, more than 16 384 edges. */
int osg_pose_inertial_optimization(struct osg_ctx *ctx, const osg_pose_inertial_problem *p,
                                   osg_pose_inertial_result *r);
/* n independent frames in one launch (sequences sharded over a GPU).  Returns the summed n_inliers or a
 * negative OSG_E_* code.  No reference counterpart. */
int osg_pose_inertial_optimization_batch(struct osg_ctx *ctx, const osg_pose_inertial_problem *p, int32_t n,
                                         osg_pose_inertial_result *r);
/* The argument checks alone (needs no context): 0 or OSG_E_INVALID. */
int osg_pose_inertial_check(const osg_pose_inertial_problem *p);
/* EdgeInertial's information (ref:src/G2oTypes.cc:582-593) from a 15 x 15 float C: the inverse of its leading
 * 9 x 9 in double, symmetrised, eigenvalues below 1e-12 set to 0 -> info9[81]; the inverses of blocks (9, 9)
 * and (12, 12) of C_rw -> info_g[9], info_a[9].  Host only; any output may be NULL. */
void osg_pose_inertial_informations(const float *C, const float *C_rw, double *info9, double *info_g,
                                    double *info_a);

/* ---- InertialOptimization ------------------------------------------------------------------
 * Optimizer::InertialOptimization (ref:src/Optimizer.cc:3706-3898, 3910-4076, 4085-4197): the IMU
 * initialisation of LocalMapping::InitializeIMU, the bias-only form of LoopClosing::MergeLocal2 and
 * LocalMapping::ScaleRefinement as one problem type.  Per KeyFrame a fixed pose and a velocity; one gyro bias,
 * one accelerometer bias, one gravity direction (2 unknowns, Rwg = Rwg ExpSO3(u0, u1, 0)) and one scale
 * (s = s exp(u)) shared by every edge; one 9-row EdgeInertialGS (ref:src/G2oTypes.cc:692-837) per KeyFrame
 * with a predecessor, EdgePriorAcc and EdgePriorGyro towards a zero prior.  g2o's Levenberg-Marquardt or
 * Gauss-Newton runs inside one launch, one workgroup per problem, on the block-arrowhead system (a
 * block-tridiagonal chain of velocity blocks bordered by the shared unknowns).  Parity with the reference is
 * tolerance-based. */
#define OSG_INERTIAL_LM 0
#define OSG_INERTIAL_GN 1
#define OSG_INERTIAL_MAX_KF 4096
#define OSG_INERTIAL_MAX_ITERATIONS 1000

typedef struct osg_inertial_problem {
    int32_t n_kf;             /* KeyFrames with mnId <= maxKFid, in any order */
    const double *Rwb;        /* 9 per KeyFrame, row-major: GetImuRotation().cast<double>() */
    const double *twb;        /* 3 per KeyFrame: GetImuPosition().cast<double>() */
    const double *v;          /* 3 per KeyFrame: GetVelocity().cast<double>() */
    int32_t n_edges;          /* one per KeyFrame with a usable mPrevKF */
    const int32_t *prev;      /* per edge: index of mPrevKF */
    const int32_t *cur;       /* per edge: index of the KeyFrame that owns the preintegration */
    const osg_pio_preintegrated *preint; /* per edge: mpImuPreintegrated */
    double bg[3], ba[3];      /* start of the two bias vertices: vpKFs.front()'s bias in all three overloads */
    double Rwg[9];            /* row-major start of VertexGDir */
    double scale;             /* start of VertexScale */
    double prior_g, prior_a;  /* informations of EdgePriorGyro / EdgePriorAcc (float arguments cast to double) */
    int32_t has_priors;       /* the two prior edges exist (overloads 1 and 2) */
    int32_t free_vel_bias;    /* velocities and both biases are free (!bFixedVel) */
    int32_t free_gdir;        /* VertexGDir is free */
    int32_t free_scale;       /* VertexScale is free (bMono) */
    int32_t algorithm;        /* OSG_INERTIAL_LM or OSG_INERTIAL_GN */
    int32_t iterations;       /* optimize(its): 200, 200, 10 in the reference */
    double lambda_init;       /* setUserLambdaInit; 0: g2o's own 1e-5 * max |diag H| */
    double huber_delta;       /* Huber delta of every inertial edge; 0: no robust kernel */
} osg_inertial_problem;

typedef struct osg_inertial_result {
    double *v;                /* 3 per KeyFrame, in the problem's order; an edge-less KeyFrame keeps its bits */
    double bg[3], ba[3], Rwg[9], scale;
    double chi2_initial;      /* activeRobustChi2 of the first computeActiveErrors */
    double chi2_final;        /* of the last accepted state */
    int32_t iterations;       /* outer iterations run */
    int32_t trials_rejected;  /* LM trials that were popped */
    int32_t solve_failed;     /* a pivot of the block LDL^T was not positive at least once */
    double *trace;            /* optional (NULL: not written): (chi2, lambda, trials) per iteration run, room for
                                 3 * problem.iterations */
} osg_inertial_result;

/* Returns the number of iterations run or a negative OSG_E_* code.  OSG_E_INVALID (nothing written, the context
 * stays usable): a null pointer, a negative count, more than OSG_INERTIAL_MAX_KF KeyFrames, an edge index out of
 * range or prev == cur, a KeyFrame that is cur of two edges or prev of two edges, a cycle, an unknown algorithm,
 * iterations outside [0, OSG_INERTIAL_MAX_ITERATIONS], nothing free. */
int osg_inertial_optimization(struct osg_ctx *ctx, const osg_inertial_problem *p, osg_inertial_result *r);
/* n independent problems in one launch.  Returns the summed iterations or a negative OSG_E_* code.  No reference
 * counterpart. */
int osg_inertial_optimization_batch(struct osg_ctx *ctx, const osg_inertial_problem *p, int32_t n,
                                    osg_inertial_result *r);
/* The argument checks alone (host only, needs no context): 0 or OSG_E_INVALID. */
int osg_inertial_check(const osg_inertial_problem *p);

/* ---- LocalInertialBA -----------------------------------------------------------------------
 * The g2o part of Optimizer::LocalInertialBA (ref:src/Optimizer.cc:2356-2743): what LocalMapping::Run calls in
 * place of LocalBundleAdjustment once the IMU is initialised.  Per KeyFrame a VertexPose (ImuCamPose),
 * VertexVelocity, VertexGyroBias and VertexAccBias, free (15 unknowns) or fixed; per MapPoint a marginalised
 * VertexSBAPointXYZ; per observation an EdgeMono / EdgeStereo (ref:src/G2oTypes.cc:398-436, 469-499) with a
 * Huber kernel (sqrt(5.991) / sqrt(7.815), held as floats); per inertial link one EdgeInertial over six
 * vertices, one EdgeGyroRW and one EdgeAccRW.  g2o's Levenberg-Marquardt over BlockSolverX with the points
 * eliminated runs inside one launch, one workgroup per window.  Everything is gathered by the
 * caller in the reference's insertion order.  Parity with the reference is tolerance-based. */
#define OSG_LIBA_MAX_FREE_KF 32
#define OSG_LIBA_MAX_FIXED_KF 512
#define OSG_LIBA_MAX_POINTS 65536
#define OSG_LIBA_MAX_EDGES 524288
#define OSG_LIBA_MAX_PAIRS 16777216 /* sum over the points of (edges on free KeyFrames)^2 */
#define OSG_LIBA_MAX_ITERATIONS 100

typedef struct osg_liba_keyframe {
    osg_pio_state state;      /* GetImuRotation / GetImuPosition / GetVelocity / GetGyroBias / GetAccBias in double */
    int32_t fixed;            /* 0: 15 unknowns (pose 6, v 3, bg 3, ba 3); else every vertex of it is fixed */
    int32_t n_cams;           /* 1, or 2 when mpCamera2 */
    osg_pio_camera cams[2];   /* ImuCamPose(KeyFrame*); Rcw / tcw are read as passed until the first update */
    double bf;                /* mbf cast to double */
} osg_liba_keyframe;

typedef struct osg_liba_link {
    int32_t prev, cur;        /* KeyFrame indices: mPrevKF and the KeyFrame that owns the preintegration */
    int32_t huber;            /* RobustKernelHuber with delta sqrt(16.92) on the EdgeInertial (i == N - 1 || bRecInit) */
    int32_t downweight;       /* EdgeInertial's information times 1e-2 (i == N - 1) */
    osg_pio_preintegrated preint; /* after SetNewBias(mPrevKF->GetImuBias()); the informations come from its C */
} osg_liba_link;

typedef struct osg_local_inertial_ba_problem {
    int32_t n_kf;
    const osg_liba_keyframe *kf;
    int32_t n_points;
    const double *xw;          /* 3 per point: GetWorldPos().cast<double>() */
    const float *track_depth;  /* per point: mTrackDepth (the classification of mono edges) */
    int32_t n_edges;           /* visual edges in insertion order */
    const int32_t *e_point;
    const int32_t *e_kf;
    const int8_t *e_kind;      /* OSG_EDGE_MONO: EdgeMono(0); OSG_EDGE_STEREO: EdgeStereo(0); OSG_EDGE_BODY: EdgeMono(1) */
    const double *e_obs;       /* 3 per edge: (u, v, ur), ur read for STEREO only */
    const float *e_inv_sigma2; /* mvInvLevelSigma2[octave] / uncertainty2 */
    int32_t n_links;
    const osg_liba_link *links;
    int32_t iterations;        /* optimize(opt_it): 10, or 4 when large */
    int32_t large;             /* bLarge: `failed` is never set */
    double lambda_init;        /* setUserLambdaInit: 1e0, or 1e-2 when large; must be positive */
} osg_local_inertial_ba_problem;

typedef struct osg_local_inertial_ba_result {
    osg_pio_state *state;      /* n_kf; a fixed KeyFrame's is bit-equal to its input, and so are v, bg, ba of a
                                  free KeyFrame without a link */
    double *Rcw;               /* 9 per KeyFrame: camera 0, for SetPose */
    double *tcw;               /* 3 per KeyFrame */
    double *xw;                /* 3 per point */
    uint8_t *edge_bad;         /* n_edges: the function's own erase rule (ref:src/Optimizer.cc:2713-2743) */
    double *edge_chi2;         /* optional (NULL: not written), n_edges: e->chi2() of the last computed errors */
    double chi2_initial;       /* err: activeRobustChi2 before optimize() */
    double chi2_last;          /* err_end: activeRobustChi2 of the last computed errors (a popped trial's included) */
    double chi2_accepted;      /* of the last accepted state */
    int32_t iterations;        /* outer iterations run */
    int32_t trials_rejected;
    int32_t solve_failed;      /* a pivot of the reduced system's Cholesky factor was not positive at least once */
    int32_t failed;            /* (2 * err < err_end || isnan(err) || isnan(err_end)) && !large, on the float casts */
    double *trace;             /* optional: (chi2, lambda, trials) per iteration run, room for 3 * iterations */
} osg_local_inertial_ba_result;

/* Returns the number of iterations run or a negative OSG_E_* code.  OSG_E_INVALID (nothing uploaded, nothing
 * written, the context stays usable): a null pointer, a negative count, a count above the caps above, an index out
 * of range, a link with prev == cur, a KeyFrame that is cur of two links, n_cams outside {1, 2}, a BODY edge on a
 * one-camera KeyFrame, an unknown edge kind, more than OSG_LIBA_MAX_PAIRS edge pairs, iterations outside
 * [0, OSG_LIBA_MAX_ITERATIONS], a lambda_init that is not positive, no free KeyFrame. */
int osg_local_inertial_ba(struct osg_ctx *ctx, const osg_local_inertial_ba_problem *p,
                          osg_local_inertial_ba_result *r);
/* n independent windows in one launch, each with its own lambda, decisions and stop; bit-equal to the single
 * calls.  Returns the summed iterations or a negative OSG_E_* code.  No reference counterpart. */
int osg_local_inertial_ba_batch(struct osg_ctx *ctx, const osg_local_inertial_ba_problem *p, int32_t n,
                                osg_local_inertial_ba_result *r);
/* The argument checks alone (host only, needs no context): 0 or OSG_E_INVALID. */
int osg_local_inertial_ba_check(const osg_local_inertial_ba_problem *p);

/* ---- OptimizeSim3 --------------------------------------------------------------------------
 * Optimizer::OptimizeSim3 (ref:src/Optimizer.cc:4213-4512), LoopClosing's Sim3 refinement between two
 * KeyFrames: one free g2o::Sim3 vertex S12, per kept match a pair of fixed camera-frame points and the
 * two reprojection edges
 *   e12 = obs1 - cam1.project(S12.map(p2c)),   e21 = obs2 - cam2.project(S12.inverse().map(p1c)),
 * both Huber with delta = sqrt(th2) (a float).  The reference writes no Jacobians for these edges, so
 * g2o differentiates them numerically (central differences, delta = 1e-9, through
 * Sim3(update) * estimate); the kernel does the same, and the result is defined up to that
 * differentiation noise: parity with the reference is tolerance-based.  The flow —
 * optimize(5), pair classification on the last computed errors, the < 10 survivors early return,
 * optimize(5 | 10) without Huber, the final classification — runs in one launch.
 *
 * The caller applies the reference's slot filter (ref:src/Optimizer.cc:4272-4350) and passes the kept
 * pairs in slot order; a pair whose MapPoint is not observed in KeyFrame 2 carries the normalised
 * (x/z, y/z) of p2c as obs2 and mvInvLevelSigma2[0], as the reference does (:4389-4404). */
typedef struct osg_sim3_problem {
    double q[4];              /* g2oS12 in: rotation (x, y, z, w) */
    double t[3];              /*            translation */
    double s;                 /*            scale */
    int32_t fix_scale;        /* bFixScale */
    float th2;                /* chi2 threshold; Huber delta = sqrt(th2) */
    osg_camera cam1, cam2;    /* pKF1->mpCamera, pKF2->mpCamera (type and p[] are read) */
    int32_t n_pairs;          /* nCorrespondences */
    const double *p1c;        /* 3 per pair: R1w X1w + t1w computed in float, cast to double */
    const double *p2c;        /* 3 per pair: R2w X2w + t2w computed in float, cast to double */
    const double *obs1;       /* 2 per pair: kpUn1.pt */
    const double *obs2;       /* 2 per pair: kpUn2.pt, or (x/z, y/z) of p2c when not in KeyFrame 2 */
    const float *inv_sigma2_1; /* pKF1->mvInvLevelSigma2[kpUn1.octave] */
    const float *inv_sigma2_2; /* pKF2->mvInvLevelSigma2[kpUn2.octave] */
    int32_t max_iterations;   /* 0: the reference's optimize(5) and optimize(5 | 10); n > 0 caps both at n */
} osg_sim3_problem;

typedef struct osg_sim3_result {
    double q[4], t[3], s;     /* g2oS12 out (the input when early_return) */
    int32_t n_inliers;        /* the reference's return value (0 when early_return) */
    uint8_t *pair_state;      /* n_pairs: 0 inlier, 1 nulled after the first optimize, 2 nulled by the final check */
    int32_t n_bad_first;      /* nBad of the first classification */
    int32_t lm_iterations[2]; /* solve() calls of the two optimize() */
    int32_t lm_trials[2];     /* linear solves incl. rejected steps */
    double chi2_final;        /* sum of both edges' e'Omega e over the pairs of state 0, at the returned Sim3 */
    double *pair_chi2;        /* optional (NULL: not written), 2 per pair: (e12, e21) chi2 as read by the pair's
                                 last classification */
    int32_t early_return;     /* nCorrespondences - nBad < 10: Sim3 and mAcumHessian stay untouched */
} osg_sim3_result;

/* Returns n_inliers or a negative OSG_E_* code. */
int osg_optimize_sim3(struct osg_ctx *ctx, const osg_sim3_problem *p, osg_sim3_result *r);
/* n independent problems in one launch, one workgroup each (e.g. every loop / merge candidate of a
 * KeyFrame at once).  Returns the summed n_inliers or a negative OSG_E_* code.  No reference
 * counterpart. */
int osg_optimize_sim3_batch(struct osg_ctx *ctx, const osg_sim3_problem *p, int32_t n, osg_sim3_result *r);

/* ---- Sim3Solver ----------------------------------------------------------------------------
 * Sim3Solver's RANSAC (ref:src/Sim3Solver.cc:146-433): every hypothesis — Horn's closed form on three
 * sampled matches, then the two-way reprojection test of every match — is evaluated in parallel, and
 * the reference's sequential rule (the first hypothesis in draw order with more than min_inliers
 * inliers ends the search; otherwise the last one that attains the largest count is the best) is then
 * replayed on the integer counts.  The caller applies the constructor's slot filter
 * (ref:src/Sim3Solver.cc:38-118) and draws the sample triples. */
typedef struct osg_sim3_ransac_problem {
    int32_t n;                /* N: kept matches */
    const float *p1c;         /* 3 per match: mvX3Dc1 */
    const float *p2c;         /* 3 per match: mvX3Dc2 */
    const float *max_err1;    /* mvnMaxError1: 9.210 sigma2 truncated to an integer, as a float */
    const float *max_err2;    /* mvnMaxError2 */
    osg_camera cam1, cam2;    /* pKF1->mpCamera, pKF2->mpCamera (type and p[] are read) */
    int32_t fix_scale;        /* mbFixScale */
    int32_t min_inliers;      /* mRansacMinInliers */
    int32_t n_hyp;            /* H = mRansacMaxIts (>= 1) */
    const int32_t *samples;   /* 3 per hypothesis, in draw order: distinct indices into [0, n) */
} osg_sim3_ransac_problem;

typedef struct osg_sim3_ransac_result {
    int32_t converged;        /* a hypothesis with more than min_inliers inliers was found */
    int32_t hyp;              /* that hypothesis, else the best one; -1 when n < min_inliers or n == 0
                                 (nothing evaluated: identity and zeros out) */
    int32_t n_iterations;     /* mnIterations after find() */
    int32_t n_inliers;        /* nInliers: the count of hyp when converged, else 0 */
    int32_t n_best;           /* mnBestInliers */
    float R[9], t[3], s;      /* of hyp, R row-major */
    float T12[16];            /* [sR | t; 0 0 0 1], row-major */
    uint8_t *inlier;          /* n flags of hyp (mvbBestInliers) */
    int32_t *hyp_inliers;     /* optional (NULL: not written), n_hyp: the count of every hypothesis */
    float *hyp_sim3;          /* optional (NULL: not written), 13 per hypothesis: R[9] t[3] s */
} osg_sim3_ransac_result;

/* Returns n_inliers or a negative OSG_E_* code (sample indices outside [0, n) or repeated within a
 * triple: OSG_E_INVALID). */
int osg_sim3_ransac(struct osg_ctx *ctx, const osg_sim3_ransac_problem *p, osg_sim3_ransac_result *r);
/* n independent problems in one pair of launches (e.g. every loop / merge candidate of a KeyFrame).
 * Returns the number of converged problems or a negative OSG_E_* code.  No reference counterpart. */
int osg_sim3_ransac_batch(struct osg_ctx *ctx, const osg_sim3_ransac_problem *p, int32_t n,
                          osg_sim3_ransac_result *r);
/* Sim3Solver::SetRansacParameters' mRansacMaxIts (ref:src/Sim3Solver.cc:120-144), host only: float
 * epsilon = min_inliers / n, ceil(log(1 - prob) / log(1 - epsilon^3)) clamped to [1, max_its], 1 when
 * min_inliers == n.  A quotient that is not finite or exceeds max_its gives max_its; n < min_inliers
 * (the solver never iterates) gives 1. */
int32_t osg_sim3_ransac_iterations(double prob, int32_t min_inliers, int32_t n, int32_t max_its);

/* ---- MLPnPsolver ---------------------------------------------------------------------------
 * MLPnPsolver's RANSAC as Tracking::Relocalization runs it (ref:src/MLPnPsolver.cpp:145-1160): every
 * hypothesis — computePose on six sampled matches (null-space linear solve, planar branch, sign choice,
 * five-step Gauss-Newton, all in double), then the float reprojection test of every match — is evaluated
 * in parallel, and the reference's sequential rule is replayed on the integer counts: the first
 * hypothesis in draw order with more than min_inliers inliers ends the search and returns its own pose
 * (Refine() re-tests the current hypothesis); otherwise the first one that attains the
 * largest count >= min_inliers is the best.  The caller applies the constructor's slot filter
 * (ref:src/MLPnPsolver.cpp:68-133) and draws the sample sets. */
typedef struct osg_mlpnp_problem {
    int32_t n;                /* N: kept matches */
    const float *bearing;     /* 3 per match: unproject(kp.pt) / z, as the constructor leaves it */
    const float *p3dw;        /* 3 per match: mvP3Dw */
    const float *p2d;         /* 2 per match: mvP2D */
    const float *max_err;     /* mvMaxError: sigma2 * th2, float */
    osg_camera cam;           /* F.mpCamera (type and p[] are read) */
    int32_t min_inliers;      /* mRansacMinInliers */
    int32_t n_hyp;            /* H: the iterations one iterate() consumes (>= 1) */
    const int32_t *samples;   /* 6 per hypothesis, in draw order: distinct indices into [0, n) */
} osg_mlpnp_problem;

typedef struct osg_mlpnp_result {
    int32_t converged;        /* a hypothesis with more than min_inliers inliers ended the search */
    int32_t hyp;              /* that hypothesis, else the first one that attains the largest count
                                 >= min_inliers; -1 when there is none or nothing was evaluated
                                 (n < min_inliers or n == 0): identity and zeros out */
    int32_t n_iterations;     /* mnIterations after iterate() */
    int32_t n_inliers;        /* nInliers: the count of hyp (0 when hyp is -1) */
    int32_t n_best;           /* mnBestInliers */
    float Tcw[16];            /* [R | t; 0 0 0 1] row-major, R and t rounded from double */
    double R[9], t[3];        /* of hyp, R row-major */
    uint8_t *inlier;          /* n flags of hyp */
    int32_t *hyp_inliers;     /* optional (NULL: not written), n_hyp: the count of every hypothesis */
    double *hyp_pose;         /* optional, 12 per hypothesis: R[9] t[3] */
    int32_t *hyp_info;        /* optional, 3 per hypothesis: planar flag, Gauss-Newton linear solves,
                                 how it ended (0 five iterations, 1 converged, 2 break) */
} osg_mlpnp_result;

/* Returns n_inliers or a negative OSG_E_* code (sample indices outside [0, n) or repeated within a
 * set: OSG_E_INVALID, before anything is uploaded). */
int osg_mlpnp_ransac(struct osg_ctx *ctx, const osg_mlpnp_problem *p, osg_mlpnp_result *r);
/* n independent problems in one pair of launches (every relocalisation candidate of a frame).  Returns
 * the number of problems with hyp >= 0 or a negative OSG_E_* code.  No reference counterpart. */
int osg_mlpnp_ransac_batch(struct osg_ctx *ctx, const osg_mlpnp_problem *p, int32_t n, osg_mlpnp_result *r);
/* The host check that both calls make before anything is uploaded: 0 when every sample set holds six distinct
 * indices into [0, n), else OSG_E_INVALID.  Needs no context. */
int osg_mlpnp_check_samples(const osg_mlpnp_problem *p);
/* MLPnPsolver::SetRansacParameters (ref:src/MLPnPsolver.cpp:314-354), host only: nMin = int(n * epsilon)
 * in float raised to min_inliers and min_set, epsilon raised to float(nMin) / n,
 * ceil(log(1 - prob) / log(1 - epsilon^3)) clamped to [1, max_its], 1 when nMin == n.  A quotient that
 * is not finite or not below max_its gives max_its. */
void osg_mlpnp_ransac_parameters(double prob, int32_t min_inliers, int32_t max_its, int32_t min_set, float epsilon,
                                 int32_t n, int32_t *min_inliers_out, int32_t *max_its_out);

/* ---- OptimizeEssentialGraph -----------------------------------------------------------------
 * The g2o part of Optimizer::OptimizeEssentialGraph (ref:src/Optimizer.cc:4527-4858): a pose graph of
 * VertexSim3Expmap vertices and EdgeSim3 edges (identity information, no robust kernel, numeric
 * Jacobians), Levenberg-Marquardt with a user lambda, optimize(20).  The adapter gathers the vertices
 * and the edge list in the reference's insertion order; the same pair may be listed several times and in
 * both directions. */
typedef struct osg_essgraph_problem {
    int32_t n_vertices;       /* non-bad KeyFrames, caller's order; at most 65 535 */
    const double *sim3;       /* 8 per vertex: q (x, y, z, w), t, s  (vScw) */
    const uint8_t *fixed;     /* per vertex */
    int32_t fix_scale;        /* bFixScale */
    int32_t n_edges;
    const int32_t *e_v0, *e_v1; /* vertex(0) = i, vertex(1) = j; i != j */
    const double *e_meas;     /* 8 per edge: Sji */
    int32_t max_iterations;   /* 0: the reference's 20 */
    double lambda_init;       /* the reference passes 1e-16; >= 0 (0: g2o's 1e-5 max |diag H|) */
} osg_essgraph_problem;

typedef struct osg_essgraph_result {
    double *sim3;             /* 8 per vertex out; a fixed vertex bit-equal to its input */
    double chi2_initial, chi2_final;
    int32_t lm_iterations, lm_trials;
    double *edge_chi2;        /* optional (NULL: not written), per edge at the returned state */
} osg_essgraph_result;

/* Returns 0 or a negative OSG_E_* code.  OSG_E_INVALID (nothing written): an index outside
 * [0, n_vertices), e_v0 == e_v1, a null array with a positive count, a negative count, lambda_init or
 * max_iterations, a scale that is not positive, more than 65 535 vertices.  OSG_E_NOMEM: the matrix
 * store (the lower 32 x 32 tiles inside the row-block envelope, twice) could not be allocated; the
 * context stays usable.  n_edges == 0 or no free vertex: the output is the input, 0 iterations. */
int osg_optimize_essential_graph(struct osg_ctx *ctx, const osg_essgraph_problem *p, osg_essgraph_result *r);
/* The MapPoint correction of the write-back (ref:src/Optimizer.cc:4824-4851):
 * Xw_out = float(inverse(sim3_after[r]).map(sim3_before[r].map(double(Xw)))) with r = ref_vertex of the
 * point; r < 0: copied through.  Xw / Xw_out: 3 floats per point (may be the same array); sim3_before /
 * sim3_after: 8 doubles per vertex.  Returns 0 or a negative OSG_E_* code (r >= n_vertices, a scale that
 * is not positive: OSG_E_INVALID, nothing written). */
int osg_essgraph_correct_points(struct osg_ctx *ctx, int32_t n_points, const float *Xw, const int32_t *ref_vertex,
                                int32_t n_vertices, const double *sim3_before, const double *sim3_after,
                                float *Xw_out);
/* ---- OptimizeEssentialGraph4DoF --------------------------------------------------------------
 * The g2o part of Optimizer::OptimizeEssentialGraph4DoF (ref:src/Optimizer.cc:4870-5198), the pose graph
 * LoopClosing::CorrectLoop optimises in an inertial map: VertexPose4DoF vertices (an ImuCamPose updated in
 * yaw and translation by UpdateW) and Edge4DoF edges (6 rows, diagonal information, no robust kernel,
 * numeric Jacobians), Levenberg-Marquardt with g2o's own lambda, optimize(20).
 * A vertex is 36 doubles, the ImuCamPose as its constructor leaves it, 3 x 3 matrices row-major:
 *   Rwb[9] twb[3] Rcw[9] tcw[3] Rcb[9] tcb[3].
 * Rcw / tcw are read as passed until the vertex's first update re-derives them from Rwb / twb. */
#define OSG_EG4_POSE_IN 36
#define OSG_EG4_POSE_OUT 24
typedef struct osg_essgraph4_problem {
    int32_t n_vertices;       /* non-bad KeyFrames, caller's order; at most 65 535 */
    const double *pose;       /* OSG_EG4_POSE_IN per vertex */
    const uint8_t *fixed;     /* per vertex */
    int32_t n_edges;
    const int32_t *e_v0, *e_v1; /* vertex(0) = i, vertex(1) = j; i != j */
    const double *e_meas;     /* 12 per edge: dRij[9] row-major, dtij[3] */
    double info_diag[6];      /* the diagonal of the edges' information: rotation x, y, z, translation x, y, z */
    int32_t max_iterations;   /* 0: the reference's 20 */
    double lambda_init;       /* >= 0; 0: g2o's 1e-5 max |diag H|, what the reference runs with */
} osg_essgraph4_problem;

typedef struct osg_essgraph4_result {
    double *pose;             /* OSG_EG4_POSE_OUT per vertex out: Rcw[9] tcw[3] Rwb[9] twb[3]; a fixed vertex
                                 bit-equal to its input */
    double chi2_initial, chi2_final;   /* sum of e' diag(info_diag) e */
    int32_t lm_iterations, lm_trials;
    double *edge_chi2;        /* optional (NULL: not written), per edge at the returned state */
} osg_essgraph4_result;

/* Returns 0 or a negative OSG_E_* code.  OSG_E_INVALID (nothing written, the context stays usable): an
 * index outside [0, n_vertices), e_v0 == e_v1, a null array with a positive count, a negative count,
 * lambda_init or max_iterations, more than 65 535 vertices, an info_diag entry that is negative or not
 * finite.  OSG_E_NOMEM as osg_optimize_essential_graph.  n_edges == 0 or no free vertex: the output is the
 * input, 0 iterations. */
int osg_optimize_essential_graph_4dof(struct osg_ctx *ctx, const osg_essgraph4_problem *p, osg_essgraph4_result *r);
/* The host check of the call above alone: 0 or OSG_E_INVALID.  Needs no context. */
int osg_essgraph4_check(const osg_essgraph4_problem *p, const osg_essgraph4_result *r);

/* Diagnostics: per-phase device time of osg_optimize_essential_graph and osg_optimize_essential_graph_4dof.  enable = 1: every later call
 * brackets its launches with HIP events (one pair per phase and launch group, read after the call);
 * 0 stops.  ms (may be NULL) receives the sums of the last timed call, in ms: linearise, assemble,
 * factor (damping copy, factorisation, both substitutions), update, chi2, and as the sixth value the
 * device bytes of the matrix store. */
#define OSG_ESSGRAPH_NK 6
int osg_essgraph_kernel_times(struct osg_ctx *ctx, int32_t enable, double *ms);

/* ---- LocalBundleAdjustment ------------------------------------------------------------------
 * Vertices are given sorted by g2o vertex id (KeyFrames: mnId; MapPoints: mnId + maxKFid + 1),
 * which fixes the Hessian index order (ref:Thirdparty/g2o/g2o/core/sparse_optimizer.cpp:181-211,
 * 547-552).  Edges are given in insertion order (internalId order). */
typedef struct osg_ba_graph {
    int32_t n_poses;
    const double *pose;        /* 7 per pose */
    const uint8_t *pose_fixed; /* setFixed(...) */
    int32_t n_points;
    const double *point;       /* 3 per point (marginalised) */
    int32_t n_edges;
    const int32_t *e_point;    /* point index per edge (vertex 0) */
    const int32_t *e_pose;     /* pose index per edge (vertex 1) */
    const int8_t *e_kind;      /* OSG_EDGE_* */
    const int32_t *e_cam;      /* index into cams */
    const double *e_obs;       /* 3 per edge */
    const float *e_inv_sigma2;
    int32_t n_cams;
    const osg_camera *cams;
    int32_t iterations;        /* optimize(iterations): 10 in LocalBundleAdjustment */
    double user_lambda_init;   /* 0 → tau·max(diag H); 100 when the map is inertial */
    /* Huber kernels.  Zero-initialised these are LocalBundleAdjustment's: every edge robust, deltas
     * thHuberMono = sqrt(5.991) (mono and body) / thHuberStereo = sqrt(7.815) as floats
     * (ref:src/Optimizer.cc:1951-1952).  BundleAdjustment (ref:src/Optimizer.cc:2933-2934, 3000-3007,
     * 3041-3047, 3083-3085) uses sqrt(5.99) / sqrt(7.815) and attaches them to mono / stereo edges
     * only when bRobust (body edges always). */
    const uint8_t *e_robust;   /* per edge: a Huber kernel attached (NULL: every edge) */
    float huber_mono, huber_stereo; /* the deltas as stored by the reference (0: the LBA values) */
} osg_ba_graph;

typedef struct osg_ba_result {
    double *pose;              /* 7 per pose (fixed poses returned unchanged) */
    double *point;             /* 3 per point */
    uint8_t *edge_bad;         /* chi2 > 5.991 (mono/body) / 7.815 (stereo) || !isDepthPositive() */
    int32_t iterations;        /* LM solve() calls executed */
    int32_t trials;            /* linear solves incl. rejected steps */
    double chi2_initial;       /* activeRobustChi2 before the first iteration */
    double chi2_final;         /* activeRobustChi2 of the accepted state */
    int32_t aborted;           /* stop flag observed */
    double *edge_chi2;         /* optional (NULL: not written): per edge e'Ωe of its last computed error, the
                                  e->chi2() the classification reads (the merge BA's second pass needs it) */
} osg_ba_result;

/* stop_flag: the reference's bool *pbStopFlag read as one byte (nonzero = stop), polled between LM
 * iterations and trials (may be NULL). */
int osg_local_bundle_adjustment(struct osg_ctx *ctx, const osg_ba_graph *g, osg_ba_result *r,
                                const volatile uint8_t *stop_flag);

/* Optimizer::BundleAdjustment / GlobalBundleAdjustemnt (ref:src/Optimizer.cc:2831-3237): the same
 * engine on the whole map — every KeyFrame (only the map's init KeyFrame fixed), every MapPoint with
 * an edge, optimize(nIterations) with the caller's e_robust / Huber deltas, no outlier pass (edge_bad
 * is filled but the reference does not read it).  The reduced camera system is dense up to 64 free
 * KeyFrames; past that it is stored and factored on its envelope (banded maps and their loop rows).
 * Tested up to about 9 000 free KeyFrames (tests/test_ba_gpu.py::test_gba_9000_kf_loop_map_accepted,
 * no parity check at that size; parity is checked on the 1 500-KF maps).  The host structure build
 * still fills two dense pose-pair tables of nhp (nhp + 1) / 2 int32 entries each (about 160 MB each at
 * 9 000 KF, 8.6 GB each at 65 535) and walks every pair, so host memory and build time grow with nhp^2
 * (DESIGN.md §3.11). */
int osg_bundle_adjustment(struct osg_ctx *ctx, const osg_ba_graph *g, osg_ba_result *r,
                          const volatile uint8_t *stop_flag);

/* Batched form: n_graphs independent windows (e.g. the LocalMapping windows of several maps or
 * sequences) optimised in lockstep, every kernel launched once per LM trial for all of them; each
 * graph follows exactly the single-graph LM (its own lambda, accept / reject, stop rules).
 * Whole-map graphs (osg_bundle_adjustment's) are accepted too: bench.py's global_ba line runs 16
 * independent maps per batch.  Returns the summed LM iterations or a negative OSG_E_* code.  No
 * reference counterpart. */
int osg_local_bundle_adjustment_batch(struct osg_ctx *ctx, const osg_ba_graph *graphs, int32_t n_graphs,
                                      osg_ba_result *results, const volatile uint8_t *stop_flag);

/* Diagnostics: per-kernel device time of the LBA / BA engine.  enable = 1 starts timing every
 * kernel of every lockstep step with HIP events on the context's stream (and clears the sums);
 * 0 stops.  ms[OSG_LBA_NK] and steps[OSG_LBA_NK] (either may be NULL) receive the summed time and
 * the number of timed launch groups since the last enable, indexed errors, linearize, pose_red,
 * lambda_init, schur_point, schur_rows, schur_pairs, chol (every k_chol_col + k_chol_trail of a
 * step), chol_back, update, step_reduce, classify. */
#define OSG_LBA_NK 12
int osg_lba_kernel_times(struct osg_ctx *ctx, int32_t enable, double *ms, int64_t *steps);

#ifdef __cplusplus
}
#endif
#endif
