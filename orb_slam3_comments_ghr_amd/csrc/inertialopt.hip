// inertialopt.hip — Optimizer::InertialOptimization (ref:src/Optimizer.cc:3706-3898, 3910-4076, 4085-4197) for a
// batch of maps: the IMU initialisation, the bias-only form of the map merge and the scale refinement as one
// problem type (include/osg_ba.h).
//
// One workgroup of NT = 256 lanes per problem, persistent over the whole call: every iteration and every
// Levenberg-Marquardt trial of g2o's optimize() runs inside the one launch.
//
//   * The host orders the KeyFrames along their mPrevKF chains (inertialopt_common.h), so the edge of chain
//     position k links the velocities k and k + 1 and the system is a block arrowhead: a block-tridiagonal
//     chain of 3 x 3 velocity blocks bordered by the 9 shared unknowns bg | ba | gdir | scale.  A fixed
//     unknown keeps its place with a zeroed Jacobian column and a unit diagonal; a velocity without an edge
//     is an identity block with a zero right-hand side and is never updated.
//   * Edge phase: one lane per edge, strided past the workgroup: EdgeInertialGS::computeError and
//     linearizeOplus (ref:src/G2oTypes.cc:719-837), the Huber weight, and the edge's 15 x 15 J' W J, J' W e
//     into the problem's global workspace.
//   * Assembly without atomics: a velocity block is the sum of its incoming and its outgoing edge's
//     contribution, in that order; the border block, the border right-hand side and chi2 are per-lane sums
//     over the lane's edges, a wave butterfly and then the four waves in wave order.  Two runs are bit-identical.
//   * Solve: block LDL^T down the chain (13 lanes of wave 0, one per column of [O_k | C_k | b_k], the 3 x 3
//     pivot block handed on with wave shuffles), the Schur complement of the border as a fixed-order
//     reduction over the positions, the dense 9 x 9 LDL^T, and the back substitution up the chain.  The chain
//     factors live in the global workspace (117 doubles per KeyFrame): at the 4 096-KeyFrame cap they would
//     need 3.7 MiB, far more than the 160 KiB of LDS.  A non-positive pivot is g2o's failed solve.
//   * Control: g2o's Levenberg-Marquardt (lambda, rho, up to 10 trials, the nBad stop) and Gauss-Newton on
//     lane 0, as in sim3opt.hip.
#include <cfloat>
#include <cstring>
#include <vector>

#include "ba_common.h"
#include "batch_io.h"
#include "inertialopt_common.h"
#include "so3_common.h"

using namespace osgba;
using namespace osgso3;
using osgio::EdgeDev;
using osgio::KfDev;
using osgio::NB;
using osgio::NE;
using osgio::NJ;
using osgio::NP;
using osgio::OutDev;
using osgio::ProbDev;

namespace {

constexpr int NT = 256;
constexpr int NWV = NT / 64;
constexpr int NS = 56;  // border upper triangle (45) | border right-hand side (9) | chi2 (1) | spare
// offsets inside a chain position's block of the workspace
constexpr int P_D = 0, P_O = 9, P_C = 18, P_B = 45, P_Y = 48, P_CP = 87, P_BP = 114;

struct State {
    double bg[3], ba[3], Rwg[9], s;
};

struct IoShared {
    State est, backup;
    double B[NB][NB], bb[NB], xb[NB];
    double red[NWV][NS], sys[NS];
    double lambda;
    int ok, ctl;
    uint8_t has[OSG_INERTIAL_MAX_KF];
};

// index of (a, b), a <= b, in the packed upper triangle of a 15 x 15
__device__ __forceinline__ int tri15(int a, int b) { return a * NJ - a * (a - 1) / 2 + (b - a); }
__device__ __forceinline__ int tri9(int a, int b) { return a * NB - a * (a - 1) / 2 + (b - a); }

// EdgeInertialGS::computeError, and with J its linearizeOplus over the columns v1 | v2 | bg | ba | gdir | scale
__device__ inline void edge_eval(const State &X, const KfDev &K1, const KfDev &K2, const double *v1,
                                 const double *v2, const EdgeDev &E, double *e, double (*J)[NJ])
{
    // IMU::Bias holds floats; the preintegration getters work in float (ref:src/ImuTypes.cc:376-426)
    float dbg[3], dba[3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        dbg[i] = (float)X.bg[i] - E.b[3 + i];
        dba[i] = (float)X.ba[i] - E.b[i];
    }
    float wf[3], Ef[9], dRf[9], t1[3], t2[3];
    m3_vec(E.JRg, dbg, wf);
    so3f_exp_matrix(wf, Ef);
    m3_mul(E.dR, Ef, dRf);
    normalize_rotation<float>(dRf);
    double dR[9], dV[3], dP[3];
    m3_vec(E.JVg, dbg, t1);
    m3_vec(E.JVa, dba, t2);
#pragma unroll
    for (int i = 0; i < 3; i++) dV[i] = (double)((E.dV[i] + t1[i]) + t2[i]);
    m3_vec(E.JPg, dbg, t1);
    m3_vec(E.JPa, dba, t2);
#pragma unroll
    for (int i = 0; i < 3; i++) dP[i] = (double)((E.dP[i] + t1[i]) + t2[i]);
#pragma unroll
    for (int i = 0; i < 9; i++) dR[i] = (double)dRf[i];

    const double dt = (double)E.dT, s = X.s;
    const double G = (double)9.81f;
    const double gI[3] = {0.0, 0.0, -G};
    double g[3], Rbw1[9], dRt[9], A[9], eR[9], er[3];
    m3_vec(X.Rwg, gI, g);
    m3_t(K1.Rwb, Rbw1);
    m3_t(dR, dRt);
    m3_mul(dRt, Rbw1, A);
    m3_mul(A, K2.Rwb, eR);
    log_so3(eR, er);
    double dv[3], dp[3], a[3], b[3], ra[3], rb[3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        dv[i] = v2[i] - v1[i];
        dp[i] = K2.twb[i] - K1.twb[i] - v1[i] * dt;
        a[i] = s * dv[i] - g[i] * dt;
        b[i] = s * dp[i] - g[i] * dt * dt / 2;
    }
    m3_vec(Rbw1, a, ra);
    m3_vec(Rbw1, b, rb);
#pragma unroll
    for (int i = 0; i < 3; i++) {
        e[i] = er[i];
        e[3 + i] = ra[i] - dV[i];
        e[6 + i] = rb[i] - dP[i];
    }
    if (!J) return;
    for (int r = 0; r < 9; r++)
        for (int c = 0; c < NJ; c++) J[r][c] = 0.0;
    // gyro bias, rotation rows: -invJr eR' RightJacobianSO3(JRg dbg) JRg
    double invJr[9], JRg[9], dbgd[3], w[3], Jr[9], eRt[9], D[9], E2[9], F[9];
    inv_right_jacobian_so3(er, invJr);
#pragma unroll
    for (int i = 0; i < 9; i++) JRg[i] = (double)E.JRg[i];
#pragma unroll
    for (int i = 0; i < 3; i++) dbgd[i] = (double)dbg[i];
    m3_vec(JRg, dbgd, w);
    right_jacobian_so3(w, Jr);
    m3_t(eR, eRt);
    m3_mul(invJr, eRt, D);
    m3_mul(D, Jr, E2);
    m3_mul(E2, JRg, F);
    // gravity direction: dGdTheta = Rwg Gm, Gm(0, 1) = -G, Gm(1, 0) = G
    double dG[3][2], RdG[3][2];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        dG[i][0] = X.Rwg[3 * i + 1] * G;
        dG[i][1] = X.Rwg[3 * i] * -G;
    }
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 2; j++) {
            double t = Rbw1[3 * i] * dG[0][j];
            t += Rbw1[3 * i + 1] * dG[1][j];
            t += Rbw1[3 * i + 2] * dG[2][j];
            RdG[i][j] = t;
        }
    // scale: Rbw1 (v2 - v1) s and Rbw1 (p2 - p1 - v1 dt) s
    double sv[3], sp[3];
    m3_vec(Rbw1, dv, sv);
    m3_vec(Rbw1, dp, sp);
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const double R = Rbw1[3 * i + j];
            J[3 + i][j] = -s * R;
            J[6 + i][j] = -s * R * dt;
            J[3 + i][3 + j] = s * R;
            J[i][6 + j] = -F[3 * i + j];
            J[3 + i][6 + j] = -(double)E.JVg[3 * i + j];
            J[6 + i][6 + j] = -(double)E.JPg[3 * i + j];
            J[3 + i][9 + j] = -(double)E.JVa[3 * i + j];
            J[6 + i][9 + j] = -(double)E.JPa[3 * i + j];
        }
#pragma unroll
        for (int j = 0; j < 2; j++) {
            J[3 + i][12 + j] = -RdG[i][j] * dt;
            J[6 + i][12 + j] = -0.5 * RdG[i][j] * dt * dt;
        }
        J[3 + i][14] = sv[i] * s;
        J[6 + i][14] = sp[i] * s;
    }
}

__global__ __launch_bounds__(NT) void k_inertial_opt(const ProbDev *__restrict__ probs,
                                                     const KfDev *__restrict__ a_kf,
                                                     const EdgeDev *__restrict__ a_edge,
                                                     const double *__restrict__ a_vin, double *__restrict__ a_v,
                                                     double *__restrict__ a_trace, double *__restrict__ a_ws,
                                                     OutDev *__restrict__ out)
{
    __shared__ IoShared S;
    const ProbDev &P = probs[blockIdx.x];
    const int n = P.n_kf;
    const KfDev *kf = a_kf + P.kf_off;
    const EdgeDev *edge = a_edge + P.kf_off;
    const double *vin = a_vin + 3 * (size_t)P.kf_off;
    double *v = a_v + 3 * (size_t)P.kf_off;
    double *trace = a_trace + P.trace_off;
    double *Ew = a_ws + P.ws_off;
    double *Pw = Ew + (size_t)n * NE;
    double *xv = Pw + (size_t)n * NP;
    double *vbak = xv + 3 * (size_t)n;
    const int tid = threadIdx.x, wave = tid / 64, lane = tid % 64;
    const bool free_vb = P.free_vb != 0, free_gd = P.free_gdir != 0, free_sc = P.free_scale != 0;
    const bool gn = P.algorithm == OSG_INERTIAL_GN;
    const double delta = P.huber_delta;

    for (int k = tid; k < n; k += NT) {
        S.has[k] = edge[k].has ? 1 : 0;
#pragma unroll
        for (int i = 0; i < 3; i++) {
            v[3 * k + i] = vin[3 * k + i];
            xv[3 * k + i] = 0.0;
        }
    }
    if (tid == 0) {
        for (int i = 0; i < 3; i++) {
            S.est.bg[i] = P.bg[i];
            S.est.ba[i] = P.ba[i];
        }
        for (int i = 0; i < 9; i++) S.est.Rwg[i] = P.Rwg[i];
        S.est.s = P.scale;
        for (int i = 0; i < NB; i++) S.xb[i] = 0.0;
    }
    __syncthreads();

    auto is_free = [&](int c) { return c < 6 ? free_vb : c < 8 ? free_gd : free_sc; };  // border entry c
    auto active = [&](int k) { return free_vb && (S.has[k] || (k > 0 && S.has[k - 1])); };
    auto block_sum = [&](double *acc, int nq) {
        for (int q = 0; q < nq; q++) {
            const double s = wave_sum(acc[q]);
            if (lane == 0) S.red[wave][q] = s;
        }
        __syncthreads();
        if (tid < nq) {
            double s = S.red[0][tid];
#pragma unroll
            for (int w = 1; w < NWV; w++) s += S.red[w][tid];
            S.sys[tid] = s;
        }
        __syncthreads();
    };
    auto block_max = [&](double m) -> double {
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) m = fmax(m, __shfl_xor(m, o));
        if (lane == 0) S.red[wave][0] = m;
        __syncthreads();
        double r = S.red[0][0];
#pragma unroll
        for (int w = 1; w < NWV; w++) r = fmax(r, S.red[w][0]);
        __syncthreads();
        return r;
    };
    // computeActiveErrors (and with sys the edges' part of buildSystem) at the estimate: S.sys
    auto edge_pass = [&](bool sys) {
        double acc[NS];
        for (int q = 0; q < NS; q++) acc[q] = 0.0;
        const State X = S.est;
        for (int k = tid; k + 1 < n; k += NT) {
            if (!S.has[k]) continue;
            const EdgeDev &E = edge[k];
            double e[9], J[9][NJ], we[9];
            edge_eval(X, kf[k], kf[k + 1], v + 3 * k, v + 3 * k + 3, E, e, sys ? J : nullptr);
            double chi2 = 0;
            for (int r = 0; r < 9; r++) {
                double s = 0;
                for (int c = 0; c < 9; c++) s += E.info[9 * r + c] * e[c];
                we[r] = s;
            }
            for (int r = 0; r < 9; r++) chi2 += e[r] * we[r];
            double r0 = chi2, r1 = 1.0;
            if (delta > 0.0) huber(chi2, delta, (float)(delta * delta), r0, r1);
            acc[54] += r0;
            if (!sys) continue;
            for (int c = 0; c < NJ; c++) {
                const bool fr = c < 6 ? free_vb : is_free(c - 6);
                if (!fr)
                    for (int r = 0; r < 9; r++) J[r][c] = 0.0;
            }
            double *M = Ew + (size_t)k * NE;
            for (int b = 0; b < NJ; b++) {
                double w[9];
                for (int r = 0; r < 9; r++) {
                    double s = 0;
                    for (int c = 0; c < 9; c++) s += E.info[9 * r + c] * J[c][b];
                    w[r] = s;
                }
                for (int a = 0; a <= b; a++) {
                    double s = 0;
                    for (int r = 0; r < 9; r++) s += J[r][a] * w[r];
                    s *= r1;
                    M[tri15(a, b)] = s;
                    if (a >= 6) acc[tri9(a - 6, b - 6)] += s;
                }
                double s = 0;
                for (int r = 0; r < 9; r++) s += J[r][b] * we[r];
                s = -(r1 * s);
                M[120 + b] = s;
                if (b >= 6) acc[45 + b - 6] += s;
            }
            M[135] = r0;
        }
        block_sum(acc, 55);
    };
    // the chain's blocks from the edges' and the border from S.sys and the prior edges; returns max |diag H|
    auto assemble = [&]() -> double {
        double md = 0.0;
        for (int k = tid; k < n; k += NT) {
            double *Q = Pw + (size_t)k * NP;
            const bool hin = k > 0 && S.has[k - 1], hout = S.has[k] != 0;
            if (!free_vb || (!hin && !hout)) {
                for (int i = 0; i < 48; i++) Q[i] = 0.0;
                Q[P_D] = Q[P_D + 4] = Q[P_D + 8] = 1.0;
                continue;
            }
            const double *Mi = Ew + (size_t)(k > 0 ? k - 1 : 0) * NE, *Mo = Ew + (size_t)k * NE;
            for (int i = 0; i < 3; i++) {
                for (int j = i; j < 3; j++) {
                    double s = 0.0;
                    if (hin) s += Mi[tri15(3 + i, 3 + j)];
                    if (hout) s += Mo[tri15(i, j)];
                    Q[P_D + 3 * i + j] = s;
                    Q[P_D + 3 * j + i] = s;
                }
                md = fmax(md, fabs(Q[P_D + 4 * i]));
                for (int j = 0; j < 3; j++) Q[P_O + 3 * i + j] = hout ? Mo[tri15(i, 3 + j)] : 0.0;
                for (int c = 0; c < NB; c++) {
                    double s = 0.0;
                    if (hin) s += Mi[tri15(3 + i, 6 + c)];
                    if (hout) s += Mo[tri15(i, 6 + c)];
                    Q[P_C + NB * i + c] = s;
                }
                double s = 0.0;
                if (hin) s += Mi[120 + 3 + i];
                if (hout) s += Mo[120 + i];
                Q[P_B + i] = s;
            }
        }
        if (tid < NB * NB) {
            const int i = tid / NB, j = tid % NB;
            const int a = i < j ? i : j, b = i < j ? j : i;
            double h = S.sys[tri9(a, b)];
            if (i == j) {
                if (P.has_priors && i < 6) h += i < 3 ? P.prior_g : P.prior_a;
                if (!is_free(i)) h = 1.0;
            }
            S.B[i][j] = h;
        }
        if (tid < NB) {
            double s = S.sys[45 + tid];
            // EdgePriorGyro / EdgePriorAcc: e = bprior - estimate, J = -I: b -= J' (prior e)
            if (P.has_priors && tid < 6) {
                const double e = 0.0 - (tid < 3 ? S.est.bg[tid] : S.est.ba[tid - 3]);
                s += (tid < 3 ? P.prior_g : P.prior_a) * e;
            }
            S.bb[tid] = is_free(tid) ? s : 0.0;
        }
        __syncthreads();
        for (int i = 0; i < NB; i++)
            if (is_free(i)) md = fmax(md, fabs(S.B[i][i]));
        return block_max(md);
    };
    // the chi2 of the two prior edges at the estimate
    auto prior_chi2 = [&]() -> double {
        double c = 0.0;
        if (P.has_priors) {
            for (int i = 0; i < 3; i++) {
                const double e = 0.0 - S.est.ba[i];
                c += e * (P.prior_a * e);
            }
            for (int i = 0; i < 3; i++) {
                const double e = 0.0 - S.est.bg[i];
                c += e * (P.prior_g * e);
            }
        }
        return c;
    };
    // (H + lambda I) x = b by block elimination; false (x untouched) when a pivot is not positive
    auto solve = [&](double lambda) -> bool {
        if (tid == 0) S.ok = 1;
        __syncthreads();
        if (wave == 0) {
            const int col = lane < 12 ? lane : 12;
            double py[3] = {0, 0, 0};
            bool ok = true;
            for (int k = 0; k < n; k++) {
                double *Q = Pw + (size_t)k * NP;
                double D[3][3], rhs[3], y[3];
#pragma unroll
                for (int i = 0; i < 3; i++) {
#pragma unroll
                    for (int j = 0; j < 3; j++) D[i][j] = Q[P_D + 3 * i + j];
                    rhs[i] = col < 3 ? Q[P_O + 3 * i + col] : col < 12 ? Q[P_C + NB * i + col - 3] : Q[P_B + i];
                }
                if (active(k))
#pragma unroll
                    for (int i = 0; i < 3; i++) D[i][i] += lambda;
                if (k > 0 && S.has[k - 1] && free_vb) {
                    const double *Op = Pw + (size_t)(k - 1) * NP + P_O;
                    double Yo[3][3];
#pragma unroll
                    for (int i = 0; i < 3; i++)
#pragma unroll
                        for (int j = 0; j < 3; j++) Yo[i][j] = __shfl(py[i], j);
#pragma unroll
                    for (int a = 0; a < 3; a++) {
#pragma unroll
                        for (int b = 0; b < 3; b++) {
                            double s = Op[a] * Yo[0][b];
                            s += Op[3 + a] * Yo[1][b];
                            s += Op[6 + a] * Yo[2][b];
                            D[a][b] -= s;
                        }
                        if (col >= 3) {
                            double s = Op[a] * py[0];
                            s += Op[3 + a] * py[1];
                            s += Op[6 + a] * py[2];
                            rhs[a] -= s;
                        }
                    }
                }
                ok = osgla::ldlt_solve<3>(D, rhs, y);  // uniform: every lane factors the same block
                if (!ok) break;
                if (lane < 13) {
#pragma unroll
                    for (int i = 0; i < 3; i++) {
                        Q[P_Y + 13 * i + col] = y[i];
                        if (col >= 3 && col < 12) Q[P_CP + NB * i + col - 3] = rhs[i];
                        if (col == 12) Q[P_BP + i] = rhs[i];
                    }
                }
#pragma unroll
                for (int i = 0; i < 3; i++) py[i] = y[i];
            }
            if (!ok && lane == 0) S.ok = 0;
        }
        __syncthreads();
        if (!S.ok) return false;
        // the border's Schur complement: sum over the positions of C'_k' Y_k
        double acc[NS];
        for (int q = 0; q < NS; q++) acc[q] = 0.0;
        for (int k = tid; k < n; k += NT) {
            if (!active(k)) continue;
            const double *Q = Pw + (size_t)k * NP;
            for (int a = 0; a < NB; a++) {
                for (int c = a; c < NB; c++) {
                    double s = Q[P_CP + a] * Q[P_Y + 3 + c];
                    s += Q[P_CP + NB + a] * Q[P_Y + 13 + 3 + c];
                    s += Q[P_CP + 2 * NB + a] * Q[P_Y + 26 + 3 + c];
                    acc[tri9(a, c)] += s;
                }
                double s = Q[P_CP + a] * Q[P_Y + 12];
                s += Q[P_CP + NB + a] * Q[P_Y + 13 + 12];
                s += Q[P_CP + 2 * NB + a] * Q[P_Y + 26 + 12];
                acc[45 + a] += s;
            }
        }
        block_sum(acc, 54);
        if (tid == 0) {
            double A[NB][NB], r[NB], x[NB];
            for (int i = 0; i < NB; i++) {
                for (int j = 0; j < NB; j++) {
                    const int a = i < j ? i : j, b = i < j ? j : i;
                    A[i][j] = (S.B[i][j] + (i == j && is_free(i) ? lambda : 0.0)) - S.sys[tri9(a, b)];
                }
                r[i] = S.bb[i] - S.sys[45 + i];
            }
            if (osgla::ldlt_solve<NB>(A, r, x)) {
                for (int i = 0; i < NB; i++) S.xb[i] = x[i];
            } else {
                S.ok = 0;
            }
        }
        __syncthreads();
        if (!S.ok) return false;
        // back substitution: x_k = Y_b - Y_C x_border - Y_O x_{k + 1}
        for (int k = tid; k < n; k += NT) {
            const double *Q = Pw + (size_t)k * NP;
#pragma unroll
            for (int i = 0; i < 3; i++) {
                double s = Q[P_Y + 13 * i + 12];
                for (int c = 0; c < NB; c++) s -= Q[P_Y + 13 * i + 3 + c] * S.xb[c];
                xv[3 * k + i] = s;
            }
        }
        __syncthreads();
        if (tid == 0 && free_vb) {
            for (int k = n - 2; k >= 0; k--) {
                if (!S.has[k]) continue;
                const double *Q = Pw + (size_t)k * NP;
                const double x0 = xv[3 * k + 3], x1 = xv[3 * k + 4], x2 = xv[3 * k + 5];
#pragma unroll
                for (int i = 0; i < 3; i++) {
                    double s = Q[P_Y + 13 * i] * x0;
                    s += Q[P_Y + 13 * i + 1] * x1;
                    s += Q[P_Y + 13 * i + 2] * x2;
                    xv[3 * k + i] -= s;
                }
            }
        }
        __syncthreads();
        return true;
    };
    // computeScale: sum of x_j (lambda x_j + b_j)
    auto lm_scale = [&](double lambda) -> double {
        double acc[1] = {0.0};
        for (int k = tid; k < n; k += NT) {
            if (!active(k)) continue;
            const double *Q = Pw + (size_t)k * NP;
#pragma unroll
            for (int i = 0; i < 3; i++) acc[0] += xv[3 * k + i] * (lambda * xv[3 * k + i] + Q[P_B + i]);
        }
        block_sum(acc, 1);
        double s = S.sys[0];
        for (int i = 0; i < NB; i++)
            if (is_free(i)) s += S.xb[i] * (lambda * S.xb[i] + S.bb[i]);
        __syncthreads();
        return s;
    };
    // SparseOptimizer::update on the free, active vertices
    auto update = [&]() {
        for (int k = tid; k < n; k += NT) {
            if (!active(k)) continue;
#pragma unroll
            for (int i = 0; i < 3; i++) v[3 * k + i] += xv[3 * k + i];
        }
        if (tid == 0) {
            if (free_vb)
                for (int i = 0; i < 3; i++) {
                    S.est.bg[i] += S.xb[i];
                    S.est.ba[i] += S.xb[3 + i];
                }
            if (free_gd) {  // GDirection::Update: Rwg = Rwg ExpSO3(u0, u1, 0)
                const double u[3] = {S.xb[6], S.xb[7], 0.0};
                double Ex[9], R[9], Rn[9];
                exp_so3(u, Ex);
                for (int i = 0; i < 9; i++) R[i] = S.est.Rwg[i];
                m3_mul(R, Ex, Rn);
                for (int i = 0; i < 9; i++) S.est.Rwg[i] = Rn[i];
            }
            if (free_sc) S.est.s = S.est.s * exp(S.xb[8]);
        }
        __syncthreads();
    };
    auto push = [&]() {
        for (int k = tid; k < 3 * n; k += NT) vbak[k] = v[k];
        if (tid == 0) S.backup = S.est;
        __syncthreads();
    };
    auto pop = [&]() {
        for (int k = tid; k < 3 * n; k += NT) v[k] = vbak[k];
        if (tid == 0) S.est = S.backup;
        __syncthreads();
    };

    // lane 0's control state; what the other lanes need goes through S.ctl and S.lambda
    double lambda = 0, ni = 2, currentChi = 0, iniChi = 0, chi2_initial = 0;
    int nBadLM = 0, iterations = 0, rejected = 0, failed = 0;
    for (int it = 0; it < P.iterations; it++) {
        edge_pass(true);
        const double chi_edges = S.sys[54];
        const double md = assemble();
        iterations++;
        iniChi = prior_chi2() + chi_edges;
        currentChi = iniChi;
        if (it == 0) chi2_initial = iniChi;
        if (gn) {
            const bool ok = solve(0.0);
            update();
            if (tid == 0) {
                trace[3 * it] = iniChi;
                trace[3 * it + 1] = 0.0;
                trace[3 * it + 2] = 1.0;
            }
            if (!ok) {
                failed = 1;
                break;
            }
            continue;
        }
        if (it == 0) {  // computeLambdaInit
            lambda = P.lambda_init > 0.0 ? P.lambda_init : 1e-5 * md;
            ni = 2;
            nBadLM = 0;
        }
        int qmax = 0, ctl = 0;
        do {
            push();
            const bool ok2 = solve(lambda);
            if (!ok2) failed = 1;
            update();  // applied before ok2 is read, with the x of the last successful solve
            edge_pass(false);
            const double chi_trial = S.sys[54];
            const double scale0 = lm_scale(lambda);
            if (tid == 0) {
                double tempChi = prior_chi2() + chi_trial;
                if (!ok2) tempChi = DBL_MAX;
                double rho = currentChi - tempChi;
                const double scale = scale0 + 1e-3;
                rho /= scale;
                int c = 0;
                if (rho > 0 && isfinite(tempChi)) {
                    double alpha = 1. - osgx::cube_rn(2 * rho - 1);
                    alpha = fmin(alpha, 2. / 3.);
                    const double scaleFactor = fmax(1. / 3., alpha);
                    lambda *= scaleFactor;
                    ni = 2;
                    currentChi = tempChi;
                } else {
                    lambda *= ni;
                    ni *= 2;
                    c = 4;  // pop
                }
                qmax++;
                if (!(rho < 0 && qmax < 10)) {
                    c |= 1;
                    if (qmax == 10 || rho == 0) c |= 2;
                    else {
                        if ((iniChi - currentChi) * 1e3 < iniChi) nBadLM++;
                        else nBadLM = 0;
                        if (nBadLM >= 3) c |= 2;
                    }
                }
                S.ctl = c;
                S.lambda = lambda;
            }
            __syncthreads();
            ctl = S.ctl;
            lambda = S.lambda;
            if (ctl & 4) {
                rejected++;
                pop();
            }
            __syncthreads();
        } while (!(ctl & 1));
        if (tid == 0) {
            trace[3 * it] = currentChi;
            trace[3 * it + 1] = lambda;
            trace[3 * it + 2] = (double)qmax;
        }
        if (ctl & 2) break;
    }
    double chi2_final = currentChi;
    if (gn || P.iterations == 0) {
        edge_pass(false);
        chi2_final = prior_chi2() + S.sys[54];
        if (P.iterations == 0) chi2_initial = chi2_final;
    }
    if (tid == 0) {
        OutDev &o = out[blockIdx.x];
        for (int i = 0; i < 3; i++) {
            o.bg[i] = S.est.bg[i];
            o.ba[i] = S.est.ba[i];
        }
        for (int i = 0; i < 9; i++) o.Rwg[i] = S.est.Rwg[i];
        o.scale = S.est.s;
        o.chi2_initial = chi2_initial;
        o.chi2_final = chi2_final;
        o.iterations = iterations;
        o.trials_rejected = rejected;
        o.solve_failed = failed;
        o.pad = 0;
    }
}

}  // namespace

extern "C" {

int osg_inertial_check(const osg_inertial_problem *p) { return osgio::check(p, nullptr); }

int osg_inertial_optimization_batch(osg_ctx *ctx, const osg_inertial_problem *p, int32_t nb, osg_inertial_result *r)
{
    if (!ctx) return OSG_E_INVALID;
    OSG_REQUIRE(ctx, nb >= 0 && (nb == 0 || (p && r)), "null argument");
    if (nb == 0) return 0;
    std::vector<std::vector<int>> order(nb), edge_at(nb);
    std::vector<ProbDev> hp(nb);
    size_t n_kf = 0, n_ws = 0, n_tr = 0;
    for (int b = 0; b < nb; b++) {
        const char *why = "";
        if (osgio::check(&p[b], &why, &order[b], &edge_at[b]) < 0)
            return osg_set_error(ctx, OSG_E_INVALID, "problem %d: %s", b, why);
        OSG_REQUIRE(ctx, p[b].n_kf == 0 || r[b].v, "problem %d: null velocity array", b);
        osgio::pack(p[b], (int)n_kf, (int64_t)n_ws, (int64_t)n_tr, hp[b]);
        n_kf += (size_t)p[b].n_kf;
        n_ws += osgio::workspace_doubles(p[b].n_kf);
        n_tr += 3 * (size_t)p[b].iterations;
    }
    OSG_REQUIRE(ctx, n_kf < (size_t(1) << 24), "too many KeyFrames in one batch");
    osg_batch_io io(ctx);
    const osg_seg i_pr = io.in(sizeof(ProbDev), nb), i_kf = io.in(sizeof(KfDev), n_kf);
    const osg_seg i_ed = io.in(sizeof(EdgeDev), n_kf), i_v = io.in(3 * sizeof(double), n_kf);
    const osg_seg o_res = io.out(sizeof(OutDev), nb), o_v = io.out(3 * sizeof(double), n_kf);
    const osg_seg o_tr = io.out(sizeof(double), n_tr);
    io.in(1, 256), io.out(1, 256);  // slack behind both blocks
    OSG_RC(io.stage());
    io.put(i_pr, 0, hp.data(), nb);
    for (int b = 0; b < nb; b++) {
        const size_t off = hp[b].kf_off;
        KfDev *kd = io.host_in<KfDev>(i_kf, off);
        EdgeDev *ed = io.host_in<EdgeDev>(i_ed, off);
        double *vd = io.host_in<double>(i_v, off);
        for (int k = 0; k < p[b].n_kf; k++) {
            const int i = order[b][k], e = edge_at[b][k];
            std::memcpy(kd[k].Rwb, p[b].Rwb + 9 * i, sizeof kd[k].Rwb);
            std::memcpy(kd[k].twb, p[b].twb + 3 * i, sizeof kd[k].twb);
            std::memcpy(vd + 3 * k, p[b].v + 3 * i, 3 * sizeof(double));
            std::memset(&ed[k], 0, sizeof ed[k]);
            if (e >= 0) osgio::pack_edge(p[b].preint[e], ed[k]);
        }
    }
    OSG_RC(io.upload());
    double *ws = nullptr;
    OSG_ALLOC(ctx, ws, SLOT_BA2, (n_ws + 32) * sizeof(double));
    OSG_RC(io.start());
    hipLaunchKernelGGL(k_inertial_opt, dim3(nb), dim3(NT), 0, ctx->stream, io.dev_in<const ProbDev>(i_pr),
                       io.dev_in<const KfDev>(i_kf), io.dev_in<const EdgeDev>(i_ed), io.dev_in<const double>(i_v),
                       io.dev_out<double>(o_v), io.dev_out<double>(o_tr), ws, io.dev_out<OutDev>(o_res));
    OSG_HIP_CHECK(ctx, hipGetLastError());
    OSG_RC(io.finish(io.out_bytes));
    const OutDev *res = io.result<OutDev>(o_res);
    int sum = 0;
    for (int b = 0; b < nb; b++) {
        const OutDev &o = res[b];
        std::memcpy(r[b].bg, o.bg, sizeof o.bg);
        std::memcpy(r[b].ba, o.ba, sizeof o.ba);
        std::memcpy(r[b].Rwg, o.Rwg, sizeof o.Rwg);
        r[b].scale = o.scale;
        r[b].chi2_initial = o.chi2_initial;
        r[b].chi2_final = o.chi2_final;
        r[b].iterations = o.iterations;
        r[b].trials_rejected = o.trials_rejected;
        r[b].solve_failed = o.solve_failed;
        const double *vd = io.result<double>(o_v, hp[b].kf_off);
        for (int k = 0; k < p[b].n_kf; k++) std::memcpy(r[b].v + 3 * order[b][k], vd + 3 * k, 3 * sizeof(double));
        if (r[b].trace) io.get(r[b].trace, o_tr, hp[b].trace_off, 3 * (size_t)o.iterations);
        sum += o.iterations;
    }
    return sum;
}

int osg_inertial_optimization(osg_ctx *ctx, const osg_inertial_problem *p, osg_inertial_result *r)
{
    const int rc = osg_inertial_optimization_batch(ctx, p, 1, r);
    return rc < 0 ? rc : r->iterations;
}

}  // extern "C"
