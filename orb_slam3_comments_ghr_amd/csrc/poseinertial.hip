// poseinertial.hip — Optimizer::PoseInertialOptimizationLastKeyFrame (ref:src/Optimizer.cc:435-987) and
// Optimizer::PoseInertialOptimizationLastFrame (ref:src/Optimizer.cc:1002-1640) for a batch of frames.
//
// One workgroup of NT = 256 lanes (four waves) per frame, persistent over the whole call: four rounds of
// g2o's Gauss-Newton optimize(10) (ref:Thirdparty/g2o/g2o/core/optimization_algorithm_gauss_newton.cpp:50-93:
// computeActiveErrors, buildSystem, solve, update; no damping, no trial loop), the classification after each
// round, the recovery pass and the new prior's H, in one launch.
//
//   * The state is the reference's vertices in double: ImuCamPose (Rwb, twb, the cameras' Rcw / tcw, the
//     its counter), velocity, gyro bias and accelerometer bias of the current frame [0] and of the previous
//     KeyFrame (fixed) or frame (free) [1].  The dense system is ordered by vertex id: VP VV VG VA of the
//     current frame (15), then of the previous frame (30, LastFrame only).
//   * Visual edge i lives on lane i % NT of chunk i / NT.  A lane adds its edges' 6 x 6 upper block, 6-vector
//     and robust chi2 to private accumulators; a wave butterfly and then the four waves in wave order in LDS
//     sum them: the same order every run, not the reference's edge order.
//   * The inertial edges (EdgeInertial; EdgeGyroRW and EdgeAccRW as one 6-row edge with a block-diagonal
//     information; EdgePriorPoseImu) are "dense edges": lane 0 writes the error and the Jacobian over the
//     whole state into LDS, all lanes form J' Omega J and J' Omega e, one entry per lane.
//   * The system is factored in LDS by a right-looking unpivoted LDL^T, the trailing update spread over the
//     lanes; a pivot <= 0 is the failed solve(): the solver's x keeps what the last successful solve left
//     (zeros before the first), update() is still applied, and optimize() stops the round
//     (ref:Thirdparty/g2o/g2o/solvers/linear_solver_dense.h:104-112, ref:Thirdparty/g2o/g2o/core/
//     sparse_optimizer.cpp:429-476).
//   * Classification reads an inlier's chi2 from the start of the round's last iteration (the kernel keeps
//     it per edge), recomputes a current outlier's at the estimate, and reads isDepthPositive at the
//     estimate, as the reference does.
#include <cstring>
#include <vector>

#include "ba_common.h"
#include "batch_io.h"
#include "poseinertial_common.h"
#include "ransac_common.h"
#include "so3_common.h"

using namespace osgba;
using namespace osgso3;
using osgpio::OutDev;
using osgpio::ProbDev;

namespace {

constexpr int NT = 256;       // lanes per frame
constexpr int NWV = NT / 64;  // waves per frame
constexpr int NS = 28;        // H upper (21) | b (6) | robust chi2 (1)
constexpr int MD = 30;        // the largest system
constexpr int MR = 15;        // the most rows of a dense edge

struct PioShared {
    double Rwb[2][9], twb[2][3], v[2][3], bg[2][3], ba[2][3];
    double Rcw[2][9], tcw[2][3];  // the current frame's cameras
    int its[2];
    osg_camera cam[2];
    double H[MD][MD], b[MD], x[MD];
    double J[MR][MD], WJ[MR][MD], e[MR], we[MR], Om[MR][MR];
    double red[NWV][NS], sys[NS];
    int cnt[NWV];
    int ok;
};

// ImuCamPose::Update (ref:src/G2oTypes.cc:221-249) on vertex k; the cameras belong to the current frame
__device__ inline void pose_update(PioShared &S, const ProbDev &P, int k, const double *pu)
{
    double Rwb[9], E[9], Rn[9], dt[3];
#pragma unroll
    for (int i = 0; i < 9; i++) Rwb[i] = S.Rwb[k][i];
    m3_vec(Rwb, pu + 3, dt);
#pragma unroll
    for (int i = 0; i < 3; i++) S.twb[k][i] += dt[i];
    exp_so3(pu, E);
    m3_mul(Rwb, E, Rn);
    S.its[k]++;
    if (S.its[k] >= 3) {
        normalize_rotation<double>(Rn);
        S.its[k] = 0;
    }
#pragma unroll
    for (int i = 0; i < 9; i++) S.Rwb[k][i] = Rn[i];
    if (k != 0) return;
    double Rbw[9], tbw[3], twb[3];
    m3_t(Rn, Rbw);
#pragma unroll
    for (int i = 0; i < 3; i++) twb[i] = S.twb[0][i];
    m3_vec(Rbw, twb, tbw);
#pragma unroll
    for (int i = 0; i < 3; i++) tbw[i] = -tbw[i];
    for (int c = 0; c < P.n_cams; c++) {
        double Rcb[9], Rcw[9], t[3];
#pragma unroll
        for (int i = 0; i < 9; i++) Rcb[i] = P.cams[c].Rcb[i];
        m3_mul(Rcb, Rbw, Rcw);
        m3_vec(Rcb, tbw, t);
#pragma unroll
        for (int i = 0; i < 9; i++) S.Rcw[c][i] = Rcw[i];
#pragma unroll
        for (int i = 0; i < 3; i++) S.tcw[c][i] = t[i] + P.cams[c].tcb[i];
    }
}

// EdgeInertial::computeError and linearizeOplus (ref:src/G2oTypes.cc:599-689) into S.e[0..9), S.J[0..9)[*]
// (zeroed by the caller); vertices 0..3 are the previous frame's, 4 and 5 the current pose and velocity
__device__ inline void inertial_edge(PioShared &S, const ProbDev &P, bool prev_free)
{
    // IMU::Bias holds floats; the preintegration getters work in float (ref:src/ImuTypes.cc:376-426)
    float dbg[3], dba[3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        dbg[i] = (float)S.bg[1][i] - P.b[3 + i];
        dba[i] = (float)S.ba[1][i] - P.b[i];
    }
    float wf[3], Ef[9], dRf[9];
    m3_vec(P.JRg, dbg, wf);
    so3f_exp_matrix(wf, Ef);
    m3_mul(P.dR, Ef, dRf);
    normalize_rotation<float>(dRf);
    float t1[3], t2[3];
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
        Rwb1[i] = S.Rwb[1][i];
        Rwb2[i] = S.Rwb[0][i];
    }
    m3_t(Rwb1, Rbw1);
    m3_t(dR, dRt);
    m3_mul(dRt, Rbw1, A);
    m3_mul(A, Rwb2, eR);
    log_so3(eR, er);
    double a[3], bvec[3], ra[3], rb[3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        a[i] = S.v[0][i] - S.v[1][i] - g[i] * dt;
        bvec[i] = S.twb[0][i] - S.twb[1][i] - S.v[1][i] * dt - g[i] * dt * dt / 2;
    }
    m3_vec(Rbw1, a, ra);
    m3_vec(Rbw1, bvec, rb);
#pragma unroll
    for (int i = 0; i < 3; i++) {
        S.e[i] = er[i];
        S.e[3 + i] = ra[i] - dV[i];
        S.e[6 + i] = rb[i] - dP[i];
    }
    // Jacobians
    double invJr[9], R12[9];
    inv_right_jacobian_so3(er, invJr);
    m3_mul(Rbw1, Rwb2, R12);
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            S.J[i][j] = invJr[3 * i + j];          // pose 2, rotation
            S.J[6 + i][3 + j] = R12[3 * i + j];    // pose 2, translation
            S.J[3 + i][6 + j] = Rbw1[3 * i + j];   // velocity 2
        }
    if (!prev_free) return;
    double Rbw2[9], B[9], C[9], Hh[9];
    m3_t(Rwb2, Rbw2);
    m3_mul(invJr, Rbw2, B);
    m3_mul(B, Rwb1, C);  // invJr Rwb2' Rwb1
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) S.J[i][15 + j] = -C[3 * i + j];
    // the reference writes 0.5 * g * dt * dt here and g * dt * dt / 2 in computeError
#pragma unroll
    for (int i = 0; i < 3; i++) bvec[i] = S.twb[0][i] - S.twb[1][i] - S.v[1][i] * dt - 0.5 * g[i] * dt * dt;
    m3_vec(Rbw1, bvec, rb);
    hat3(ra, Hh);
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) S.J[3 + i][15 + j] = Hh[3 * i + j];
    hat3(rb, Hh);
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            S.J[6 + i][15 + j] = Hh[3 * i + j];
            S.J[6 + i][18 + j] = i == j ? -1.0 : 0.0;
            S.J[3 + i][21 + j] = -Rbw1[3 * i + j];
            S.J[6 + i][21 + j] = -Rbw1[3 * i + j] * dt;
        }
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
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            S.J[i][24 + j] = -F[3 * i + j];
            S.J[3 + i][24 + j] = -(double)P.JVg[3 * i + j];
            S.J[6 + i][24 + j] = -(double)P.JPg[3 * i + j];
            S.J[3 + i][27 + j] = -(double)P.JVa[3 * i + j];
            S.J[6 + i][27 + j] = -(double)P.JPa[3 * i + j];
        }
}

// EdgePriorPoseImu (ref:src/G2oTypes.cc:856-892) on the previous frame's vertices (columns 15..29)
__device__ inline void prior_edge(PioShared &S, const ProbDev &P)
{
    double Rp[9], Rpt[9], Rk[9], D[9], er[3], d[3], et[3], iJ[9];
#pragma unroll
    for (int i = 0; i < 9; i++) {
        Rp[i] = P.prior.Rwb[i];
        Rk[i] = S.Rwb[1][i];
    }
    m3_t(Rp, Rpt);
    m3_mul(Rpt, Rk, D);
    log_so3(D, er);
#pragma unroll
    for (int i = 0; i < 3; i++) d[i] = S.twb[1][i] - P.prior.twb[i];
    m3_vec(Rpt, d, et);
    inv_right_jacobian_so3(er, iJ);
#pragma unroll
    for (int i = 0; i < 3; i++) {
        S.e[i] = er[i];
        S.e[3 + i] = et[i];
        S.e[6 + i] = S.v[1][i] - P.prior.vwb[i];
        S.e[9 + i] = S.bg[1][i] - P.prior.bg[i];
        S.e[12 + i] = S.ba[1][i] - P.prior.ba[i];
#pragma unroll
        for (int j = 0; j < 3; j++) {
            S.J[i][15 + j] = iJ[3 * i + j];
            S.J[3 + i][18 + j] = D[3 * i + j];
        }
        S.J[6 + i][21 + i] = 1.0;
        S.J[9 + i][24 + i] = 1.0;
        S.J[12 + i][27 + i] = 1.0;
    }
}

struct VEdge {
    double xw[3], obs[3], w;
    int kind;
};

// Xc of the edge's camera at the current estimate
__device__ __forceinline__ void edge_xc(const PioShared &S, const VEdge &E, int ci, double *Xc)
{
#pragma unroll
    for (int i = 0; i < 3; i++) {
        double s = S.Rcw[ci][3 * i] * E.xw[0];
        s += S.Rcw[ci][3 * i + 1] * E.xw[1];
        s += S.Rcw[ci][3 * i + 2] * E.xw[2];
        Xc[i] = s + S.tcw[ci][i];
    }
}
// EdgeMonoOnlyPose / EdgeStereoOnlyPose computeError: obs - Project / ProjectStereo (ref:src/G2oTypes.cc:188-207)
__device__ __forceinline__ void edge_err(const PioShared &S, const ProbDev &P, const VEdge &E, const double *Xc,
                                         int ci, double *err)
{
    double uv[2];
    cam_project(S.cam[ci], Xc, uv);
    err[0] = E.obs[0] - uv[0];
    err[1] = E.obs[1] - uv[1];
    err[2] = 0.0;
    if (E.kind == OSG_EDGE_STEREO) {
        const double invZ = 1 / Xc[2];
        err[2] = E.obs[2] - (uv[0] - P.bf * invZ);
    }
}
// linearizeOplus: proj_jac Rcb SE3deriv(Xb) (ref:src/G2oTypes.cc:442-462, 505-530); row 2 is zero for mono edges
__device__ __forceinline__ void edge_jac(const PioShared &S, const ProbDev &P, const VEdge &E, const double *Xc,
                                         int ci, double Jp[3][6])
{
    const osg_pio_camera &K = P.cams[ci];
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
        cam_project_jac(S.cam[ci], Xc, PJ2);
#pragma unroll
        for (int j = 0; j < 3; j++) {
            PJ[0][j] = PJ2[0][j];
            PJ[1][j] = PJ2[1][j];
            PJ[2][j] = 0.0;
        }
    }
    if (E.kind == OSG_EDGE_STEREO) {
        const double inv_z2 = 1.0 / (Xc[2] * Xc[2]);
#pragma unroll
        for (int j = 0; j < 3; j++) PJ[2][j] = PJ[0][j];
        PJ[2][2] += P.bf * inv_z2;
    }
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
        }
        Jp[r][0] = M[1] * -z + M[2] * y;
        Jp[r][1] = M[0] * z + M[2] * -x;
        Jp[r][2] = M[0] * -y + M[1] * x;
        Jp[r][3] = M[0];
        Jp[r][4] = M[1];
        Jp[r][5] = M[2];
    }
}

__global__ __launch_bounds__(NT) void k_pose_inertial(const ProbDev *__restrict__ probs,
                                                      const int8_t *__restrict__ a_kind,
                                                      const double *__restrict__ a_xw,
                                                      const double *__restrict__ a_obs,
                                                      const float *__restrict__ a_w,
                                                      const float *__restrict__ a_depth,
                                                      uint8_t *__restrict__ a_outlier,
                                                      double *__restrict__ a_chi2, OutDev *__restrict__ out)
{
    __shared__ PioShared S;
    const ProbDev &P = probs[blockIdx.x];
    const int n = P.n_edges;
    const size_t off = (size_t)P.edge_off;
    const int8_t *kind = a_kind + off;
    const double *xw = a_xw + 3 * off, *obs = a_obs + 3 * off;
    const float *wgt = a_w + off, *depth = a_depth + off;
    uint8_t *outlier = a_outlier + off;
    double *pchi2 = a_chi2 + off;
    const int tid = threadIdx.x, wave = tid / 64, lane = tid % 64;
    const int nch = (n + NT - 1) / NT;  // <= 64 (checked by the host)
    const bool last_frame = P.mode == OSG_PIO_LAST_FRAME;
    const int dim = last_frame ? 30 : 15;
    const int n_graph_edges = n + (last_frame ? 4 : 3);  // optimizer.edges().size()

    if (tid == 0) {
        for (int k = 0; k < 2; k++) {
            const osg_pio_state &st = k == 0 ? P.cur : P.prev;
            for (int i = 0; i < 9; i++) S.Rwb[k][i] = st.Rwb[i];
            for (int i = 0; i < 3; i++) {
                S.twb[k][i] = st.twb[i];
                S.v[k][i] = st.v[i];
                S.bg[k][i] = st.bg[i];
                S.ba[k][i] = st.ba[i];
            }
            S.its[k] = 0;
        }
        for (int c = 0; c < P.n_cams; c++) {
            S.cam[c] = P.cams[c].cam;
            for (int i = 0; i < 9; i++) S.Rcw[c][i] = P.cams[c].Rcw[i];
            for (int i = 0; i < 3; i++) S.tcw[c][i] = P.cams[c].tcw[i];
        }
    }
    if (tid < MD) S.x[tid] = 0.0;
    __syncthreads();

    uint64_t lvl = 0;  // bit c: this lane's edge of chunk c has level 1 (is an outlier)
    auto edge_of = [&](int c) { return c * NT + tid; };
    auto load_edge = [&](int i) {
        VEdge E;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            E.xw[k] = xw[3 * i + k];
            E.obs[k] = obs[3 * i + k];
        }
        E.w = (double)wgt[i];
        E.kind = kind[i];
        return E;
    };
    auto block_sum = [&](double *acc, int nq, double *dst) {
        for (int q = 0; q < nq; q++) {
            const double s = wave_sum(acc[q]);
            if (lane == 0) S.red[wave][q] = s;
        }
        __syncthreads();
        if (tid < nq) {
            double s = S.red[0][tid];
#pragma unroll
            for (int w = 1; w < NWV; w++) s += S.red[w][tid];
            dst[tid] = s;
        }
        __syncthreads();
    };
    auto block_count = [&](int c) -> int {
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) c += __shfl_xor(c, o);
        if (lane == 0) S.cnt[wave] = c;
        __syncthreads();
        int t = 0;
#pragma unroll
        for (int w = 0; w < NWV; w++) t += S.cnt[w];
        __syncthreads();
        return t;
    };
    // the visual edges' sums at the estimate: level-0 edges with the round's kernel (solve), or the edges that
    // are not outliers with their plain information (the new prior's H)
    auto visual_pass = [&](bool robust, bool for_prior) {
        double acc[NS];
#pragma unroll
        for (int q = 0; q < NS; q++) acc[q] = 0.0;
        for (int c = 0; c < nch; c++) {
            const int i = edge_of(c);
            if (i >= n || ((lvl >> c) & 1)) continue;
            const VEdge E = load_edge(i);
            const int ci = E.kind == OSG_EDGE_BODY ? 1 : 0;
            double Xc[3], err[3], Jp[3][6];
            edge_xc(S, E, ci, Xc);
            edge_jac(S, P, E, Xc, ci, Jp);
            double r1 = 1.0;
            if (!for_prior) {
                edge_err(S, P, E, Xc, ci, err);
                const double chi2 = chi2_of(err, 3, E.w);
                pchi2[i] = chi2;
                double r0 = chi2;
                if (robust) {
                    // const float thHuberMono = sqrt(5.991), thHuberStereo = sqrt(7.815)
                    const float df = E.kind == OSG_EDGE_STEREO ? (float)2.7955321496988725 : (float)2.4476519360399265;
                    huber(chi2, (double)df, (float)((double)df * (double)df), r0, r1);
                }
                acc[27] += r0;
#pragma unroll
                for (int a = 0; a < 6; a++) {
                    double sb = 0;
                    sb += Jp[0][a] * (E.w * err[0]);
                    sb += Jp[1][a] * (E.w * err[1]);
                    sb += Jp[2][a] * (E.w * err[2]);
                    acc[21 + a] -= r1 * sb;
                }
            }
            const double ww = r1 * E.w;
            int q = 0;
#pragma unroll
            for (int a = 0; a < 6; a++)
#pragma unroll
                for (int b = a; b < 6; b++) {
                    double h = 0;
                    h += Jp[0][a] * ww * Jp[0][b];
                    h += Jp[1][a] * ww * Jp[1][b];
                    h += Jp[2][a] * ww * Jp[2][b];
                    acc[q++] += h;
                }
        }
        block_sum(acc, NS, S.sys);
    };
    auto zero_dense = [&]() {
        for (int idx = tid; idx < MR * MD; idx += NT) (&S.J[0][0])[idx] = 0.0;
        __syncthreads();
    };
    // a dense edge's J' (rho1 Omega) J into H and -rho1 J' Omega e into b; S.J, S.e and S.Om are filled
    auto dense_edge = [&](int m, double delta, bool add_b) {
        for (int idx = tid; idx < m * dim; idx += NT) {
            const int r = idx / dim, c = idx % dim;
            double s = 0;
            for (int k = 0; k < m; k++) s += S.Om[r][k] * S.J[k][c];
            S.WJ[r][c] = s;
        }
        if (tid < m) {
            double s = 0;
            for (int k = 0; k < m; k++) s += S.Om[tid][k] * S.e[k];
            S.we[tid] = s;
        }
        __syncthreads();
        double r1 = 1.0;
        if (delta > 0.0) {
            double chi2 = 0;
            for (int k = 0; k < m; k++) chi2 += S.e[k] * S.we[k];
            double r0;
            huber(chi2, delta, (float)(delta * delta), r0, r1);
        }
        for (int idx = tid; idx < dim * dim; idx += NT) {
            const int i = idx / dim, j = idx % dim;
            double s = 0;
            for (int k = 0; k < m; k++) s += S.J[k][i] * S.WJ[k][j];
            S.H[i][j] += r1 * s;
        }
        if (add_b && tid < dim) {
            double s = 0;
            for (int k = 0; k < m; k++) s += S.J[k][tid] * S.we[k];
            S.b[tid] -= r1 * s;
        }
        __syncthreads();
    };
    // H (and b) of the whole graph at the estimate
    auto build = [&](bool robust, bool for_prior) {
        for (int idx = tid; idx < MD * MD; idx += NT) (&S.H[0][0])[idx] = 0.0;
        if (tid < MD) S.b[tid] = 0.0;
        visual_pass(robust, for_prior);
        // EdgeInertial
        zero_dense();
        if (tid == 0) inertial_edge(S, P, last_frame);
        for (int idx = tid; idx < 81; idx += NT) S.Om[idx / 9][idx % 9] = P.info9[idx];
        __syncthreads();
        dense_edge(9, 0.0, !for_prior);
        // EdgeGyroRW and EdgeAccRW
        zero_dense();
        if (tid < 6) {
            const int k = tid % 3;
            const bool gyro = tid < 3;
            S.e[tid] = gyro ? S.bg[0][k] - S.bg[1][k] : S.ba[0][k] - S.ba[1][k];
            S.J[tid][9 + tid] = 1.0;
            if (last_frame) S.J[tid][24 + tid] = -1.0;
        }
        if (tid < 36) S.Om[tid / 6][tid % 6] = P.info_rw[tid];
        __syncthreads();
        dense_edge(6, 0.0, !for_prior);
        if (last_frame) {  // EdgePriorPoseImu, Huber delta 5 while solving
            zero_dense();
            if (tid == 0) prior_edge(S, P);
            for (int idx = tid; idx < 225; idx += NT) S.Om[idx / 15][idx % 15] = P.prior.H[idx];
            __syncthreads();
            dense_edge(15, for_prior ? 0.0 : 5.0, !for_prior);
        }
        if (tid < 36) {
            const int i = tid / 6, j = tid % 6;
            const int a = i < j ? i : j, b = i < j ? j : i;
            S.H[i][j] += S.sys[a * 6 - a * (a - 1) / 2 + (b - a)];
        }
        if (tid < 6) S.b[tid] += S.sys[21 + tid];
        __syncthreads();
    };
    // unpivoted LDL' of S.H in place (column j keeps L(:, j) d_j until it is scaled), then both substitutions into S.x
    auto solve = [&]() -> bool {
        bool ok = true;
        for (int j = 0; j < dim; j++) {
            const double d = S.H[j][j];
            if (!(d > 0.0)) {
                ok = false;  // uniform: every lane reads the same pivot
                break;
            }
            for (int idx = tid; idx < dim * dim; idx += NT) {
                const int i = idx / dim, k = idx % dim;
                if (i > j && k > j && k <= i) S.H[i][k] -= (S.H[i][j] / d) * S.H[k][j];
            }
            __syncthreads();
        }
        if (ok) {  // L(i, k) = H(i, k) / d_k, every quotient on its own lane: lane 0's substitutions divide by nothing
            for (int idx = tid; idx < dim * dim; idx += NT) {
                const int i = idx / dim, k = idx % dim;
                if (k < i) S.H[i][k] = S.H[i][k] / S.H[k][k];
            }
            __syncthreads();
        }
        if (ok && tid == 0) {
            double *y = S.WJ[0];  // free between two dense edges
            for (int i = 0; i < dim; i++) {
                double s = S.b[i];
                for (int k = 0; k < i; k++) s -= S.H[i][k] * y[k];
                y[i] = s;
            }
            for (int i = 0; i < dim; i++) y[i] /= S.H[i][i];
            for (int i = dim - 1; i >= 0; i--) {
                double s = y[i];
                for (int k = i + 1; k < dim; k++) s -= S.H[k][i] * y[k];
                y[i] = s;
            }
            for (int i = 0; i < dim; i++) S.x[i] = y[i];
        }
        __syncthreads();
        return ok;
    };
    // SparseOptimizer::update in _ivMap (vertex id) order
    auto update = [&]() {
        if (tid == 0) {
            for (int k = 0; k < (last_frame ? 2 : 1); k++) {
                double pu[6];
#pragma unroll
                for (int i = 0; i < 6; i++) pu[i] = S.x[15 * k + i];
                pose_update(S, P, k, pu);
                for (int i = 0; i < 3; i++) {
                    S.v[k][i] += S.x[15 * k + 6 + i];
                    S.bg[k][i] += S.x[15 * k + 9 + i];
                    S.ba[k][i] += S.x[15 * k + 12 + i];
                }
            }
        }
        __syncthreads();
    };

    int iterations = 0, rounds = 0, failed = 0, recovered = 0;
    int nInliers = 0, nBad = 0;
    for (int it = 0; it < 4; it++) {
        rounds++;
        const bool robust = it <= 2;  // setRobustKernel(0) in the classification of it == 2
        for (int iter = 0; iter < 10; iter++) {
            build(robust, false);
            const bool ok = solve();
            iterations++;
            update();
            if (!ok) {
                failed = 1;
                break;
            }
        }
        // classification (ref:src/Optimizer.cc:731-841, 1316-1423)
        const float chi2Mono = last_frame ? 5.991f : (it == 0 ? 12.f : it == 1 ? 7.5f : 5.991f);
        const float chi2Stereo = it == 0 ? 15.6f : it == 1 ? 9.8f : 7.815f;
        const float chi2close = (float)(1.5 * chi2Mono);
        int bad = 0, in = 0;
        for (int c = 0; c < nch; c++) {
            const int i = edge_of(c);
            if (i >= n) continue;
            const VEdge E = load_edge(i);
            const int ci = E.kind == OSG_EDGE_BODY ? 1 : 0;
            double Xc[3];
            edge_xc(S, E, ci, Xc);
            double chi2d = pchi2[i];
            if ((lvl >> c) & 1) {  // a current outlier: computeError() at the estimate
                double err[3];
                edge_err(S, P, E, Xc, ci, err);
                chi2d = chi2_of(err, 3, E.w);
                pchi2[i] = chi2d;
            }
            const float chi2 = (float)chi2d;
            bool b;
            if (E.kind == OSG_EDGE_STEREO) {
                b = chi2 > chi2Stereo;
            } else {
                const bool bClose = depth[i] < 10.f;
                b = (chi2 > chi2Mono && !bClose) || (bClose && chi2 > chi2close) || !(Xc[2] > 0.0);
            }
            if (b) lvl |= uint64_t(1) << c;
            else lvl &= ~(uint64_t(1) << c);
            bad += b ? 1 : 0;
            in += b ? 0 : 1;
        }
        nBad = block_count(bad);
        nInliers = block_count(in);
        if (n_graph_edges < 10) break;
    }
    // the recovery pass (ref:src/Optimizer.cc:845-877): a flag is only ever cleared, nBad counts every edge
    // whose recomputed chi2 is not below the bound
    uint64_t outl = lvl;
    if (nInliers < 30 && !P.rec_init) {
        recovered = 1;
        int bad = 0;
        for (int c = 0; c < nch; c++) {
            const int i = edge_of(c);
            if (i >= n) continue;
            const VEdge E = load_edge(i);
            const int ci = E.kind == OSG_EDGE_BODY ? 1 : 0;
            double Xc[3], err[3];
            edge_xc(S, E, ci, Xc);
            edge_err(S, P, E, Xc, ci, err);
            const double chi2d = chi2_of(err, 3, E.w);
            pchi2[i] = chi2d;
            const float chi2 = (float)chi2d;
            if (chi2 < (E.kind == OSG_EDGE_STEREO ? 24.f : 18.f)) outl &= ~(uint64_t(1) << c);
            else bad++;
        }
        nBad = block_count(bad);
    }
    for (int c = 0; c < nch; c++) {
        const int i = edge_of(c);
        if (i < n) outlier[i] = (outl >> c) & 1;
    }
    // the new prior (ref:src/Optimizer.cc:891-960, 1475-1635): plain informations, relinearised at the estimate,
    // the visual edges that are not outliers
    lvl = outl;
    build(false, true);
    OutDev &o = out[blockIdx.x];
    if (!last_frame) {
        for (int idx = tid; idx < 225; idx += NT) o.H[idx] = S.H[idx / 15][idx % 15];
    } else {
        // Marginalize(H, previous frame) (ref:src/Optimizer.cc:1663-1744): H_cc - H_cp pinv(H_pp) H_pc, the
        // pseudo-inverse through a cyclic Jacobi eigen-decomposition of the symmetric H_pp, |values| <= 1e-6 dropped
        double (*A)[MD] = S.J;    // A[i][j], i, j < 15: H_pp -> diagonal
        double (*V)[MD] = S.WJ;   // eigenvectors in columns
        for (int idx = tid; idx < 225; idx += NT) {
            const int i = idx / 15, j = idx % 15;
            A[i][j] = S.H[15 + i][15 + j];
            V[i][j] = i == j ? 1.0 : 0.0;
        }
        __syncthreads();
        for (int sweep = 0; sweep < 30; sweep++) {
            double offd = 0, diag = 0;  // uniform
            for (int i = 0; i < 15; i++) {
                diag += A[i][i] * A[i][i];
                for (int j = i + 1; j < 15; j++) offd += A[i][j] * A[i][j];
            }
            __syncthreads();
            if (!(offd > 1e-34 * diag)) break;
            for (int p = 0; p < 14; p++)
                for (int q = p + 1; q < 15; q++) {
                    const double apq = A[p][q];
                    const double app = A[p][p], aqq = A[q][q];
                    __syncthreads();
                    if (apq == 0.0) continue;
                    double c, s;
                    jacobi_rotation(app, aqq, apq, c, s);
                    if (tid < 15) {
                        const double akp = A[tid][p], akq = A[tid][q];
                        A[tid][p] = c * akp - s * akq;
                        A[tid][q] = s * akp + c * akq;
                        const double vkp = V[tid][p], vkq = V[tid][q];
                        V[tid][p] = c * vkp - s * vkq;
                        V[tid][q] = s * vkp + c * vkq;
                    }
                    __syncthreads();
                    if (tid < 15) {
                        const double apk = A[p][tid], aqk = A[q][tid];
                        A[p][tid] = c * apk - s * aqk;
                        A[q][tid] = s * apk + c * aqk;
                    }
                    __syncthreads();
                }
        }
        // pinv = V diag(1 / lambda where |lambda| > 1e-6) V' -> S.Om
        if (tid < 225) {
            const int i = tid / 15, j = tid % 15;
            double s = 0;
            for (int k = 0; k < 15; k++) {
                const double l = A[k][k];  // singular value |l|, and U = V sign(l): V diag(1 / l) V'
                const double inv = fabs(l) > 1e-6 ? 1.0 / l : 0.0;
                s += V[i][k] * inv * V[j][k];
            }
            S.Om[i][j] = s;
        }
        __syncthreads();
        // T = H_cp pinv -> S.H's lower-right block is no longer needed: keep T in it
        if (tid < 225) {
            const int i = tid / 15, j = tid % 15;
            double s = 0;
            for (int k = 0; k < 15; k++) s += S.H[i][15 + k] * S.Om[k][j];
            A[i][j] = s;
        }
        __syncthreads();
        if (tid < 225) {
            const int i = tid / 15, j = tid % 15;
            double s = 0;
            for (int k = 0; k < 15; k++) s += A[i][k] * S.H[15 + k][j];
            o.H[tid] = S.H[i][j] - s;
        }
    }
    if (tid == 0) {
        for (int i = 0; i < 9; i++) o.state.Rwb[i] = S.Rwb[0][i];
        for (int i = 0; i < 3; i++) {
            o.state.twb[i] = S.twb[0][i];
            o.state.v[i] = S.v[0][i];
            o.state.bg[i] = S.bg[0][i];
            o.state.ba[i] = S.ba[0][i];
        }
        o.n_inliers = n - nBad;
        o.rounds_run = rounds;
        o.iterations = iterations;
        o.solve_failed = failed;
        o.recovered = recovered;
    }
}

}  // namespace

extern "C" {

int osg_pose_inertial_check(const osg_pose_inertial_problem *p) { return osgpio::check(p, nullptr); }

void osg_pose_inertial_informations(const float *C, const float *C_rw, double *info9, double *info_g, double *info_a)
{
    osgpio::informations(C, C_rw, info9, info_g, info_a);
}

int osg_pose_inertial_optimization_batch(osg_ctx *ctx, const osg_pose_inertial_problem *p, int32_t nb,
                                         osg_pose_inertial_result *r)
{
    if (!ctx) return OSG_E_INVALID;
    OSG_REQUIRE(ctx, nb >= 0 && (nb == 0 || (p && r)), "null argument");
    if (nb == 0) return 0;
    size_t total = 0;
    for (int b = 0; b < nb; b++) {
        const char *why = "";
        if (osgpio::check(&p[b], &why) < 0) return osg_set_error(ctx, OSG_E_INVALID, "problem %d: %s", b, why);
        OSG_REQUIRE(ctx, p[b].n_edges == 0 || r[b].outlier, "problem %d: null outlier array", b);
        total += (size_t)p[b].n_edges;
    }
    OSG_REQUIRE(ctx, total < (size_t(1) << 28), "too many edges in one batch");
    std::vector<ProbDev> hp(nb);
    size_t at = 0;
    for (int b = 0; b < nb; b++) {
        osgpio::pack(p[b], (int)at, hp[b]);
        at += (size_t)p[b].n_edges;
    }
    osg_batch_io io(ctx);
    const osg_seg i_pr = io.in(sizeof(ProbDev), nb), i_k = io.in(1, total), i_x = io.in(3 * sizeof(double), total);
    const osg_seg i_o = io.in(3 * sizeof(double), total), i_w = io.in(sizeof(float), total);
    const osg_seg i_d = io.in(sizeof(float), total);
    const osg_seg o_out = io.out(1, total), o_chi = io.out(sizeof(double), total), o_res = io.out(sizeof(OutDev), nb);
    io.in(1, 256), io.out(1, 256);  // slack behind both blocks
    OSG_RC(io.stage());
    io.put(i_pr, 0, hp.data(), nb);
    for (int b = 0; b < nb; b++) {
        const size_t off = hp[b].edge_off, m = p[b].n_edges;
        io.put(i_k, off, p[b].kind, m);
        io.put(i_x, off, p[b].xw, m);
        io.put(i_o, off, p[b].obs, m);
        io.put(i_w, off, p[b].inv_sigma2, m);
        io.put(i_d, off, p[b].track_depth, m);
    }
    OSG_RC(io.upload());
    OSG_RC(io.start());
    hipLaunchKernelGGL(k_pose_inertial, dim3(nb), dim3(NT), 0, ctx->stream, io.dev_in<const ProbDev>(i_pr),
                       io.dev_in<const int8_t>(i_k), io.dev_in<const double>(i_x), io.dev_in<const double>(i_o),
                       io.dev_in<const float>(i_w), io.dev_in<const float>(i_d), io.dev_out<uint8_t>(o_out),
                       io.dev_out<double>(o_chi), io.dev_out<OutDev>(o_res));
    OSG_HIP_CHECK(ctx, hipGetLastError());
    OSG_RC(io.finish(io.out_bytes));
    const OutDev *res = io.result<OutDev>(o_res);
    int sum = 0;
    for (int b = 0; b < nb; b++) {
        const OutDev &o = res[b];
        r[b].state = o.state;
        r[b].n_inliers = o.n_inliers;
        r[b].rounds_run = o.rounds_run;
        r[b].iterations = o.iterations;
        r[b].solve_failed = o.solve_failed;
        r[b].recovered = o.recovered;
        std::memcpy(r[b].H, o.H, sizeof o.H);
        io.get(r[b].outlier, o_out, hp[b].edge_off, p[b].n_edges);
        if (r[b].edge_chi2) io.get(r[b].edge_chi2, o_chi, hp[b].edge_off, p[b].n_edges);
        sum += o.n_inliers;
    }
    return sum;
}

int osg_pose_inertial_optimization(osg_ctx *ctx, const osg_pose_inertial_problem *p, osg_pose_inertial_result *r)
{
    const int rc = osg_pose_inertial_optimization_batch(ctx, p, 1, r);
    return rc < 0 ? rc : r->n_inliers;
}

}  // extern "C"
