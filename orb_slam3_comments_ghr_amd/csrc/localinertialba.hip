// localinertialba.hip — the g2o part of Optimizer::LocalInertialBA (ref:src/Optimizer.cc:2356-2743) for a batch of
// windows (include/osg_ba.h).
//
// One workgroup of NT = 512 lanes per window, persistent over the whole call: every iteration and every
// Levenberg-Marquardt trial of g2o's optimize() runs inside the one launch, as in inertialopt.hip.  A batch is a
// grid of such workgroups, each following its own lambda, decisions and stop, so it is bit-equal to the single
// calls by construction.  The window's working set lives in a global workspace (localinertialba_common.h).
//
//   * Edge phase: one lane per visual edge, strided past the workgroup: EdgeMono / EdgeStereo computeError and
//     linearizeOplus (inertialba_edges.h), the Huber weight, and the edge's blocks (pose 6 x 6, coupling 6 x 3,
//     point 3 x 3, both gradients) into the workspace.  One lane per inertial link: EdgeInertial's error, its
//     9 x 24 Jacobian, rho1 Omega J and the two random-walk edges.
//   * Assembly without atomics: a point's block and gradient are the sum over its edge list, a KeyFrame's pose
//     block over its edge list, both in insertion order (host-built CSR); the links are added one after the
//     other, all lanes on the 24 x 24 entries of one link.  H and b are built once per iteration.
//   * Per trial: the damped point blocks are inverted (one lane per point), Y = W V^-1 per edge, and the reduced
//     system of order 15 N is H + lambda I minus, per pair of free KeyFrames, the sum over the host-built list
//     of their edge pairs on a shared point of Y_a W_b' (one lane per entry of the 6 x 6 block, in list order).
//   * Factor and solve: right-looking Cholesky of the lower triangle in the workspace with the right-hand side
//     carried as an extra row, rows over the waves and columns over the lanes; a pivot that is not positive is
//     g2o's failed solve.  Then the KeyFrame update (ImuCamPose::Update with its three-update normalisation) and
//     the points' back substitution.
//   * Control: g2o's Levenberg-Marquardt (lambda on every diagonal entry, the points' included, computeScale over
//     all active unknowns, rho with the [1/3, 2/3] clamp and ni, up to 10 trials, the nBad stop) on lane 0, as in
//     sim3opt.hip and inertialopt.hip.  No stop flag: the reference sets it after optimize().
//   * Every sum runs in a fixed order: two runs are bit-identical.
#include <cfloat>
#include <cstring>
#include <vector>

#include "batch_io.h"
#include "inertialba_edges.h"
#include "localinertialba_common.h"

using namespace osgba;
using namespace osgiba;
using namespace osgliba;

namespace {

constexpr int NT = 512;
constexpr int NWV = NT / 64;

struct Args {
    const ProbDev *probs;
    const KfDev *kf;
    const LinkDev *links;
    const BlockDev *blocks;
    const int32_t *pairs, *pt_beg, *pt_edges, *kf_edges, *e_point, *e_kf;
    const int8_t *e_kind;
    const double *e_obs, *xw;
    const float *e_w, *depth;
    osg_pio_state *o_state;
    double *o_cam, *o_xw, *o_chi2, *o_trace, *ws;
    uint8_t *o_bad;
    OutDev *out;
};

struct Shared {
    double red[NWV], sum;
    double lambda;
    int ctl, ok;
    int fk[OSG_LIBA_MAX_FREE_KF], fflags[OSG_LIBA_MAX_FREE_KF];
};

// index (a, b), a <= b, of the packed upper triangle of a 6 x 6 / 3 x 3
__device__ __forceinline__ int tri6(int a, int b) { return a * 6 - a * (a - 1) / 2 + (b - a); }
__device__ __forceinline__ int tri3(int a, int b) { return a * 3 - a * (a - 1) / 2 + (b - a); }

__global__ __launch_bounds__(NT) void k_local_inertial_ba(const Args A)
{
    __shared__ Shared S;
    const ProbDev &P = A.probs[blockIdx.x];
    const int nk = P.n_kf, nf = P.n_free, np = P.n_pts, ne = P.n_edges, nl = P.n_links, n = NU * nf;
    const KfDev *kf = A.kf + P.kf_off;
    const LinkDev *links = A.links + P.link_off;
    const BlockDev *blocks = A.blocks + P.block_off;
    const int32_t *pairs = A.pairs + 2 * P.pair_off;
    const int32_t *pt_beg = A.pt_beg + P.ptb_off, *pt_edges = A.pt_edges + P.edge_off;
    const int32_t *kf_edges = A.kf_edges + P.edge_off;
    const int32_t *e_point = A.e_point + P.edge_off, *e_kf = A.e_kf + P.edge_off;
    const int8_t *e_kind = A.e_kind + P.edge_off;
    const double *e_obs = A.e_obs + 3 * (size_t)P.edge_off;
    const float *e_w = A.e_w + P.edge_off;
    // workspace
    double *KS = A.ws + P.ws_off, *KB = KS + (size_t)KST * nk;
    double *X = KB + (size_t)KST * nk, *XB = X + 3 * (size_t)np;
    double *EW = XB + 3 * (size_t)np, *EY = EW + (size_t)EWN * ne;
    double *PW = EY + (size_t)EYN * ne, *LW = PW + (size_t)PWN * np;
    double *H = LW + (size_t)LWN * nl, *Sm = H + (size_t)n * n;
    double *bv = Sm + (size_t)(n + 1) * n, *xv = bv + n;
#define EWQ(q, e) EW[(size_t)(q) * ne + (e)]
#define EYQ(q, e) EY[(size_t)(q) * ne + (e)]
#define PWQ(q, p) PW[(size_t)(q) * np + (p)]
    const int tid = threadIdx.x, wave = tid / 64, lane = tid % 64;

    for (int k = tid; k < nk; k += NT) {
        const KfDev &K = kf[k];
        double *st = KS + (size_t)KST * k;
        for (int i = 0; i < 9; i++) st[K_RWB + i] = K.state.Rwb[i];
        for (int i = 0; i < 3; i++) {
            st[K_TWB + i] = K.state.twb[i];
            st[K_V + i] = K.state.v[i];
            st[K_BG + i] = K.state.bg[i];
            st[K_BA + i] = K.state.ba[i];
        }
        for (int c = 0; c < 2; c++) {
            for (int i = 0; i < 9; i++) st[K_RCW + 9 * c + i] = c < K.n_cams ? K.cams[c].Rcw[i] : 0.0;
            for (int i = 0; i < 3; i++) st[K_TCW + 3 * c + i] = c < K.n_cams ? K.cams[c].tcw[i] : 0.0;
        }
        st[K_ITS] = 0.0;
        if (K.free_idx >= 0) {
            S.fk[K.free_idx] = k;
            S.fflags[K.free_idx] = K.flags;
        }
    }
    for (int i = tid; i < 3 * np; i += NT) {
        X[i] = A.xw[3 * (size_t)P.pt_off + i];
        PWQ(P_X + i / np, i % np) = 0.0;
    }
    for (int i = tid; i < n; i += NT) xv[i] = 0.0;
    __syncthreads();

    auto col_active = [&](int c) { return (S.fflags[c / NU] & (c % NU < 6 ? KF_POSE : KF_LINKED)) != 0; };
    auto pt_active = [&](int p) { return pt_beg[p + 1] > pt_beg[p]; };
    auto block_sum = [&](double v) -> double {
        v = wave_sum(v);
        if (lane == 0) S.red[wave] = v;
        __syncthreads();
        if (tid == 0) {
            double s = S.red[0];
#pragma unroll
            for (int w = 1; w < NWV; w++) s += S.red[w];
            S.sum = s;
        }
        __syncthreads();
        const double r = S.sum;
        __syncthreads();
        return r;
    };
    // computeError of every active edge at the estimate (and with jac its linearizeOplus and quadratic form)
    auto edge_pass = [&](bool jac) {
        for (int e = tid; e < ne; e += NT) {
            const int k = e_kf[e], kind = e_kind[e], ci = kind == OSG_EDGE_BODY ? 1 : 0;
            const KfDev &K = kf[k];
            const double *st = KS + (size_t)KST * k, *Xp = X + 3 * (size_t)e_point[e];
            const double w = (double)e_w[e];
            const double Xw[3] = {Xp[0], Xp[1], Xp[2]}, obs[3] = {e_obs[3 * e], e_obs[3 * e + 1], e_obs[3 * e + 2]};
            double Xc[3], err[3];
            visual_xc(st, ci, Xw, Xc);
            visual_error(K.cams[ci].cam, K.bf, kind, Xc, obs, err);
            const double chi2 = chi2_of(err, 3, w);
            // const float thHuberMono = sqrt(5.991), thHuberStereo = sqrt(7.815)
            const float df = kind == OSG_EDGE_STEREO ? (float)2.7955321496988725 : (float)2.4476519360399265;
            double r0, r1;
            huber(chi2, (double)df, (float)((double)df * (double)df), r0, r1);
            EWQ(E_R0, e) = r0;
            EWQ(E_CHI, e) = chi2;
            if (!jac) continue;
            double Jp[3][6], Jl[3][3];
            visual_jacobians(st, K.cams[ci], K.bf, kind, ci, Xc, Jp, Jl);
            const double ww = r1 * w;
            const double we[3] = {w * err[0], w * err[1], w * err[2]};
#pragma unroll
            for (int a = 0; a < 3; a++) {
#pragma unroll
                for (int b = a; b < 3; b++) {
                    double h = Jl[0][a] * ww * Jl[0][b];
                    h += Jl[1][a] * ww * Jl[1][b];
                    h += Jl[2][a] * ww * Jl[2][b];
                    EWQ(E_HLL + tri3(a, b), e) = h;
                }
                double s = Jl[0][a] * we[0];
                s += Jl[1][a] * we[1];
                s += Jl[2][a] * we[2];
                EWQ(E_BL + a, e) = -(r1 * s);
            }
            if (K.free_idx < 0) continue;
#pragma unroll
            for (int a = 0; a < 6; a++) {
#pragma unroll
                for (int b = a; b < 6; b++) {
                    double h = Jp[0][a] * ww * Jp[0][b];
                    h += Jp[1][a] * ww * Jp[1][b];
                    h += Jp[2][a] * ww * Jp[2][b];
                    EWQ(E_HPP + tri6(a, b), e) = h;
                }
#pragma unroll
                for (int b = 0; b < 3; b++) {
                    double h = Jp[0][a] * ww * Jl[0][b];
                    h += Jp[1][a] * ww * Jl[1][b];
                    h += Jp[2][a] * ww * Jl[2][b];
                    EWQ(E_W + 3 * a + b, e) = h;
                }
                double s = Jp[0][a] * we[0];
                s += Jp[1][a] * we[1];
                s += Jp[2][a] * we[2];
                EWQ(E_BP + a, e) = -(r1 * s);
            }
        }
        for (int l = tid; l < nl; l += NT) {
            const LinkDev &L = links[l];
            double *W = LW + (size_t)LWN * l;
            if (!L.active) {
                W[L_R0] = W[L_R0 + 1] = W[L_R0 + 2] = 0.0;
                continue;
            }
            const double *s1 = KS + (size_t)KST * L.prev, *s2 = KS + (size_t)KST * L.cur;
            const Preint Q = {L.dR, L.dV, L.dP, L.JRg, L.JVg, L.JVa, L.JPg, L.JPa, L.b, L.dT};
            double e[9], oe[9];
            inertial_edge(s1, s2, Q, e, jac ? W + L_J : nullptr);
            double chi2 = 0;
            for (int r = 0; r < 9; r++) {
                double s = 0;
                for (int c = 0; c < 9; c++) s += L.info9[9 * r + c] * e[c];
                oe[r] = s;
            }
            for (int r = 0; r < 9; r++) chi2 += e[r] * oe[r];
            double r0 = chi2, r1 = 1.0;
            const double delta = 4.1133927602406267;  // sqrt(16.92)
            if (L.huber) huber(chi2, delta, (float)(delta * delta), r0, r1);
            W[L_R0] = r0;
            // EdgeGyroRW / EdgeAccRW: e = b2 - b1
            for (int which = 0; which < 2; which++) {
                const int o = which == 0 ? K_BG : K_BA;
                const double *I3 = which == 0 ? L.info_g : L.info_a;
                double d[3], od[3];
                for (int i = 0; i < 3; i++) d[i] = s2[o + i] - s1[o + i];
                m3_vec(I3, d, od);
                double c = 0;
                for (int i = 0; i < 3; i++) c += d[i] * od[i];
                W[L_R0 + 1 + which] = c;
                if (jac)
                    for (int i = 0; i < 3; i++) W[L_RWB + 6 * which + i] = od[i], W[L_RWB + 6 * which + 3 + i] = -od[i];
            }
            if (!jac) continue;
            const double *J = W + L_J;
            for (int c = 0; c < LJ; c++) {
                double s = 0;
                for (int r = 0; r < 9; r++) {
                    double t = 0;
                    for (int q = 0; q < 9; q++) t += L.info9[9 * r + q] * J[LJ * q + c];
                    W[L_WJ + LJ * r + c] = r1 * t;
                    s += J[LJ * r + c] * oe[r];
                }
                W[L_B + c] = -(r1 * s);
            }
        }
        __syncthreads();
    };
    // activeRobustChi2 of the errors the last edge_pass left
    auto chi_total = [&]() -> double {
        double acc = 0.0;
        for (int e = tid; e < ne; e += NT) acc += EWQ(E_R0, e);
        for (int l = tid; l < nl; l += NT) {
            const double *W = LW + (size_t)LWN * l;
            acc += W[L_R0];
            acc += W[L_R0 + 1];
            acc += W[L_R0 + 2];
        }
        return block_sum(acc);
    };
    // buildSystem: H, b of the KeyFrames and the points' sums, from what edge_pass(true) left
    auto assemble = [&]() {
        for (size_t i = tid; i < (size_t)n * n; i += NT) H[i] = 0.0;
        for (int i = tid; i < n; i += NT) bv[i] = 0.0;
        for (int p = tid; p < np; p += NT) {
            double s[9];
#pragma unroll
            for (int q = 0; q < 9; q++) s[q] = 0.0;
            for (int i = pt_beg[p]; i < pt_beg[p + 1]; i++) {
                const int e = pt_edges[i];
#pragma unroll
                for (int q = 0; q < 9; q++) s[q] += EWQ(q < 6 ? E_HLL + q : E_BL + q - 6, e);
            }
#pragma unroll
            for (int q = 0; q < 9; q++) PWQ(q < 6 ? P_H + q : P_B + q - 6, p) = s[q];
        }
        __syncthreads();
        for (int t = tid; t < nf * 27; t += NT) {
            const int f = t / 27, q = t % 27;
            const KfDev &K = kf[S.fk[f]];
            double s = 0.0;
            for (int i = K.e_beg; i < K.e_end; i++) s += EWQ(q < 21 ? E_HPP + q : E_BP + q - 21, kf_edges[i]);
            if (q < 21) {
                int a = 0, r = q;
                while (r >= 6 - a) {
                    r -= 6 - a;
                    a++;
                }
                const int b = a + r;
                H[(size_t)(NU * f + a) * n + NU * f + b] = s;
                H[(size_t)(NU * f + b) * n + NU * f + a] = s;
            } else {
                bv[NU * f + q - 21] = s;
            }
        }
        __syncthreads();
        for (int l = 0; l < nl; l++) {
            const LinkDev &L = links[l];
            if (!L.active) continue;
            const double *W = LW + (size_t)LWN * l;
            const int f1 = kf[L.prev].free_idx, f2 = kf[L.cur].free_idx;
            auto col = [&](int a) { return a < 15 ? (f1 < 0 ? -1 : NU * f1 + a) : (f2 < 0 ? -1 : NU * f2 + a - 15); };
            for (int idx = tid; idx < LJ * LJ + LJ; idx += NT) {
                if (idx < LJ * LJ) {
                    const int a = idx / LJ, c = idx % LJ, ca = col(a), cc = col(c);
                    if (ca < 0 || cc < 0) continue;
                    double s = 0;
                    for (int r = 0; r < 9; r++) s += W[L_J + LJ * r + a] * W[L_WJ + LJ * r + c];
                    H[(size_t)ca * n + cc] += s;
                } else {
                    const int a = idx - LJ * LJ, ca = col(a);
                    if (ca >= 0) bv[ca] += W[L_B + a];
                }
            }
            __syncthreads();
            // the random-walk edges: J = [-I, I] over (b1, b2)
            for (int idx = tid; idx < 2 * 36 + 12; idx += NT) {
                if (idx < 72) {
                    const int which = idx / 36, i = (idx % 36) / 6, j = idx % 6;
                    const int fi = i < 3 ? f1 : f2, fj = j < 3 ? f1 : f2;
                    if (fi < 0 || fj < 0) continue;
                    const double *I3 = which == 0 ? L.info_g : L.info_a;
                    const double v = I3[3 * (i % 3) + j % 3];
                    H[(size_t)(NU * fi + 9 + 3 * which + i % 3) * n + NU * fj + 9 + 3 * which + j % 3] +=
                        (i < 3) == (j < 3) ? v : -v;
                } else {
                    const int which = (idx - 72) / 6, i = (idx - 72) % 6, fi = i < 3 ? f1 : f2;
                    if (fi >= 0) bv[NU * fi + 9 + 3 * which + i % 3] += W[L_RWB + 6 * which + i];
                }
            }
            __syncthreads();
        }
    };
    // (H + lambda I) x = b with the points eliminated; false (x untouched) when a pivot is not positive
    auto solve = [&](double lambda) -> bool {
        for (int p = tid; p < np; p += NT) {
            if (!pt_active(p)) continue;
            const double a = PWQ(P_H, p) + lambda, b = PWQ(P_H + 1, p), c = PWQ(P_H + 2, p);
            const double d = PWQ(P_H + 3, p) + lambda, e = PWQ(P_H + 4, p), f = PWQ(P_H + 5, p) + lambda;
            // the symmetric 3 x 3 inverse by cofactors
            const double c00 = d * f - e * e, c01 = c * e - b * f, c02 = b * e - c * d;
            const double det = a * c00 + b * c01 + c * c02, id = 1.0 / det;
            PWQ(P_VI, p) = c00 * id;
            PWQ(P_VI + 1, p) = c01 * id;
            PWQ(P_VI + 2, p) = c02 * id;
            PWQ(P_VI + 3, p) = (a * f - c * c) * id;
            PWQ(P_VI + 4, p) = (b * c - a * e) * id;
            PWQ(P_VI + 5, p) = (a * d - b * b) * id;
        }
        for (size_t i = tid; i < (size_t)n * n; i += NT) {
            const int r = (int)(i / n), c = (int)(i % n);
            double h = H[i];
            if (r == c) h = col_active(r) ? h + lambda : 1.0;
            Sm[i] = h;
        }
        for (int i = tid; i < n; i += NT) Sm[(size_t)n * n + i] = bv[i];
        __syncthreads();
        for (int e = tid; e < ne; e += NT) {
            if (kf[e_kf[e]].free_idx < 0) continue;
            const int p = e_point[e];
            double V[6];
#pragma unroll
            for (int q = 0; q < 6; q++) V[q] = PWQ(P_VI + q, p);
#pragma unroll
            for (int r = 0; r < 6; r++) {
                const double w0 = EWQ(E_W + 3 * r, e), w1 = EWQ(E_W + 3 * r + 1, e), w2 = EWQ(E_W + 3 * r + 2, e);
                EYQ(3 * r, e) = (w0 * V[0] + w1 * V[1]) + w2 * V[2];
                EYQ(3 * r + 1, e) = (w0 * V[1] + w1 * V[3]) + w2 * V[4];
                EYQ(3 * r + 2, e) = (w0 * V[2] + w1 * V[4]) + w2 * V[5];
            }
        }
        __syncthreads();
        // the Schur complement, block by block of the lower triangle
        for (int t = tid; t < P.n_blocks * 36; t += NT) {
            const BlockDev B = blocks[t / 36];
            const int r = (t % 36) / 6, c = t % 6;
            if (B.fi == B.fj && c > r) continue;
            double s = 0.0;
            for (int i = B.beg; i < B.end; i++) {
                const int a = pairs[2 * i], b = pairs[2 * i + 1];
                double t2 = EYQ(3 * r, a) * EWQ(E_W + 3 * c, b);
                t2 += EYQ(3 * r + 1, a) * EWQ(E_W + 3 * c + 1, b);
                t2 += EYQ(3 * r + 2, a) * EWQ(E_W + 3 * c + 2, b);
                s += t2;
            }
            // rows of the later KeyFrame: entry (fj, c | fi, r) of the lower triangle is (fi, r | fj, c) transposed
            const size_t at = B.fi == B.fj ? (size_t)(NU * B.fi + r) * n + NU * B.fi + c
                                           : (size_t)(NU * B.fj + c) * n + NU * B.fi + r;
            Sm[at] -= s;
        }
        for (int t = tid; t < nf * 6; t += NT) {
            const int f = t / 6, r = t % 6;
            const KfDev &K = kf[S.fk[f]];
            double s = 0.0;
            for (int i = K.e_beg; i < K.e_end; i++) {
                const int e = kf_edges[i], p = e_point[e];
                double t2 = EYQ(3 * r, e) * PWQ(P_B, p);
                t2 += EYQ(3 * r + 1, e) * PWQ(P_B + 1, p);
                t2 += EYQ(3 * r + 2, e) * PWQ(P_B + 2, p);
                s += t2;
            }
            Sm[(size_t)n * n + NU * f + r] -= s;
        }
        __syncthreads();
        // Cholesky of the lower triangle; row n carries the right-hand side and ends as L^-1 b
        for (int j = 0; j < n; j++) {
            const double d = Sm[(size_t)j * n + j];
            if (!(d > 0.0)) return false;  // uniform: every lane reads the same entry
            const double l = sqrt(d);
            __syncthreads();
            for (int i = j + 1 + tid; i <= n; i += NT) Sm[(size_t)i * n + j] /= l;
            if (tid == 0) Sm[(size_t)j * n + j] = l;
            __syncthreads();
            for (int i = j + 1 + wave; i <= n; i += NWV) {
                const double lij = Sm[(size_t)i * n + j];
                const int kend = i < n ? i : n - 1;
                for (int k = j + 1 + lane; k <= kend; k += 64) Sm[(size_t)i * n + k] -= lij * Sm[(size_t)k * n + j];
            }
            __syncthreads();
        }
        // L' x = y, down the rows of L
        double *y = Sm + (size_t)n * n;
        for (int j = n - 1; j >= 0; j--) {
            const double xj = y[j] / Sm[(size_t)j * n + j];
            __syncthreads();
            for (int i = tid; i < j; i += NT) y[i] -= Sm[(size_t)j * n + i] * xj;
            if (tid == 0) y[j] = xj;
            __syncthreads();
        }
        for (int i = tid; i < n; i += NT) xv[i] = y[i];
        __syncthreads();
        // the points: x_p = V^-1 (b_p - sum W_e' x_kf)
        for (int p = tid; p < np; p += NT) {
            if (!pt_active(p)) continue;
            double r[3] = {PWQ(P_B, p), PWQ(P_B + 1, p), PWQ(P_B + 2, p)};
            for (int i = pt_beg[p]; i < pt_beg[p + 1]; i++) {
                const int e = pt_edges[i], f = kf[e_kf[e]].free_idx;
                if (f < 0) continue;
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    double s = 0.0;
#pragma unroll
                    for (int a = 0; a < 6; a++) s += EWQ(E_W + 3 * a + c, e) * xv[NU * f + a];
                    r[c] -= s;
                }
            }
            const double V0 = PWQ(P_VI, p), V1 = PWQ(P_VI + 1, p), V2 = PWQ(P_VI + 2, p);
            const double V3 = PWQ(P_VI + 3, p), V4 = PWQ(P_VI + 4, p), V5 = PWQ(P_VI + 5, p);
            PWQ(P_X, p) = (V0 * r[0] + V1 * r[1]) + V2 * r[2];
            PWQ(P_X + 1, p) = (V1 * r[0] + V3 * r[1]) + V4 * r[2];
            PWQ(P_X + 2, p) = (V2 * r[0] + V4 * r[1]) + V5 * r[2];
        }
        __syncthreads();
        return true;
    };
    // computeScale: sum of x_j (lambda x_j + b_j) over the active unknowns
    auto lm_scale = [&](double lambda) -> double {
        double acc = 0.0;
        for (int i = tid; i < n; i += NT)
            if (col_active(i)) acc += xv[i] * (lambda * xv[i] + bv[i]);
        for (int p = tid; p < np; p += NT) {
            if (!pt_active(p)) continue;
#pragma unroll
            for (int c = 0; c < 3; c++) acc += PWQ(P_X + c, p) * (lambda * PWQ(P_X + c, p) + PWQ(P_B + c, p));
        }
        return block_sum(acc);
    };
    // SparseOptimizer::update on the free, active vertices
    auto update = [&]() {
        for (int f = tid; f < nf; f += NT) {
            const int k = S.fk[f];
            double *st = KS + (size_t)KST * k;
            const double *u = xv + NU * f;
            if (S.fflags[f] & KF_POSE) {
                const double pu[6] = {u[0], u[1], u[2], u[3], u[4], u[5]};
                pose_update(st, kf[k].cams, kf[k].n_cams, pu);
            }
            if (S.fflags[f] & KF_LINKED)
                for (int i = 0; i < 9; i++) st[K_V + i] += u[6 + i];  // v | bg | ba are contiguous
        }
        for (int p = tid; p < np; p += NT) {
            if (!pt_active(p)) continue;
#pragma unroll
            for (int c = 0; c < 3; c++) X[3 * (size_t)p + c] += PWQ(P_X + c, p);
        }
        __syncthreads();
    };
    auto copy_state = [&](double *ks_to, const double *ks_from, double *x_to, const double *x_from) {
        for (int i = tid; i < KST * nk; i += NT) ks_to[i] = ks_from[i];
        for (int i = tid; i < 3 * np; i += NT) x_to[i] = x_from[i];
        __syncthreads();
    };

    // lane 0's control state; what the other lanes need goes through S.ctl and S.lambda
    double lambda = 0, ni = 2, currentChi = 0, iniChi = 0, chi_last = 0;
    int nBadLM = 0, iterations = 0, rejected = 0, failed = 0;
    edge_pass(false);  // optimizer.computeActiveErrors() before optimize()
    const double chi2_initial = chi_total();
    currentChi = chi_last = chi2_initial;
    for (int it = 0; it < P.iterations; it++) {
        edge_pass(true);
        iniChi = chi_total();
        currentChi = chi_last = iniChi;
        assemble();
        iterations++;
        if (it == 0) {  // computeLambdaInit with a user value
            lambda = P.lambda_init;
            ni = 2;
            nBadLM = 0;
        }
        int qmax = 0, ctl = 0;
        do {
            copy_state(KB, KS, XB, X);  // push
            const bool ok2 = solve(lambda);
            if (!ok2) failed = 1;
            update();  // applied before ok2 is read, with the x of the last successful solve
            edge_pass(false);
            const double chi_trial = chi_total();
            chi_last = chi_trial;
            const double scale0 = lm_scale(lambda);
            if (tid == 0) {
                double tempChi = chi_trial;
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
            __syncthreads();
            if (ctl & 4) {
                rejected++;
                copy_state(KS, KB, X, XB);  // pop
            }
        } while (!(ctl & 1));
        if (tid == 0) {
            double *trace = A.o_trace + P.trace_off;
            trace[3 * it] = currentChi;
            trace[3 * it + 1] = lambda;
            trace[3 * it + 2] = (double)qmax;
        }
        if (ctl & 2) break;
    }

    // the estimates, and the erase rule of ref:src/Optimizer.cc:2713-2743 on the last computed errors
    for (int k = tid; k < nk; k += NT) {
        const double *st = KS + (size_t)KST * k;
        osg_pio_state &o = A.o_state[P.kf_off + k];
        for (int i = 0; i < 9; i++) o.Rwb[i] = st[K_RWB + i];
        for (int i = 0; i < 3; i++) {
            o.twb[i] = st[K_TWB + i];
            o.v[i] = st[K_V + i];
            o.bg[i] = st[K_BG + i];
            o.ba[i] = st[K_BA + i];
        }
        double *oc = A.o_cam + 12 * (size_t)(P.kf_off + k);
        for (int i = 0; i < 9; i++) oc[i] = st[K_RCW + i];
        for (int i = 0; i < 3; i++) oc[9 + i] = st[K_TCW + i];
    }
    for (int i = tid; i < 3 * np; i += NT) A.o_xw[3 * (size_t)P.pt_off + i] = X[i];
    for (int e = tid; e < ne; e += NT) {
        const int kind = e_kind[e], p = e_point[e];
        const double chi2 = EWQ(E_CHI, e);
        A.o_chi2[P.edge_off + e] = chi2;
        bool bad;
        if (kind == OSG_EDGE_STEREO) {
            bad = chi2 > (double)7.815f;
        } else {
            const bool close = A.depth[P.pt_off + p] < 10.f;
            const double *Xp = X + 3 * (size_t)p;
            const double Xw[3] = {Xp[0], Xp[1], Xp[2]};
            double Xc[3];
            visual_xc(KS + (size_t)KST * e_kf[e], kind == OSG_EDGE_BODY ? 1 : 0, Xw, Xc);
            bad = (chi2 > (double)5.991f && !close) || (chi2 > (double)(1.5f * 5.991f) && close) || !(Xc[2] > 0.0);
        }
        A.o_bad[P.edge_off + e] = bad ? 1 : 0;
    }
    if (tid == 0) {
        OutDev &o = A.out[blockIdx.x];
        o.chi2_initial = chi2_initial;
        o.chi2_last = chi_last;
        o.chi2_accepted = currentChi;
        o.iterations = iterations;
        o.trials_rejected = rejected;
        o.solve_failed = failed;
        o.pad = 0;
    }
#undef EWQ
#undef EYQ
#undef PWQ
}

}  // namespace

extern "C" {

int osg_local_inertial_ba_check(const osg_local_inertial_ba_problem *p) { return osgliba::check(p, nullptr); }

int osg_local_inertial_ba_batch(osg_ctx *ctx, const osg_local_inertial_ba_problem *p, int32_t nb,
                                osg_local_inertial_ba_result *r)
{
    if (!ctx) return OSG_E_INVALID;
    OSG_REQUIRE(ctx, nb >= 0 && (nb == 0 || (p && r)), "null argument");
    if (nb == 0) return 0;
    std::vector<Structure> st(nb);
    std::vector<ProbDev> hp(nb);
    size_t n_kf = 0, n_pt = 0, n_ptb = 0, n_ed = 0, n_ln = 0, n_bl = 0, n_pr = 0, n_ws = 0, n_tr = 0;
    for (int b = 0; b < nb; b++) {
        const char *why = "";
        if (osgliba::check(&p[b], &why) < 0) return osg_set_error(ctx, OSG_E_INVALID, "problem %d: %s", b, why);
        OSG_REQUIRE(ctx, r[b].state && r[b].Rcw && r[b].tcw && (p[b].n_points == 0 || r[b].xw) &&
                             (p[b].n_edges == 0 || r[b].edge_bad),
                    "problem %d: null result array", b);
        OSG_REQUIRE(ctx, build_structure(p[b], st[b]), "problem %d: too many edge pairs", b);
        ProbDev &d = hp[b];
        std::memset(&d, 0, sizeof d);
        d.n_kf = p[b].n_kf, d.n_free = st[b].n_free, d.n_pts = p[b].n_points, d.n_edges = p[b].n_edges;
        d.n_links = p[b].n_links, d.n_blocks = (int32_t)st[b].blocks.size();
        d.iterations = p[b].iterations, d.large = p[b].large != 0;
        d.kf_off = (int32_t)n_kf, d.pt_off = (int32_t)n_pt, d.ptb_off = (int32_t)n_ptb, d.edge_off = (int32_t)n_ed;
        d.link_off = (int32_t)n_ln, d.block_off = (int32_t)n_bl;
        d.pair_off = (int64_t)n_pr, d.ws_off = (int64_t)n_ws, d.trace_off = (int64_t)n_tr;
        d.lambda_init = p[b].lambda_init;
        n_kf += d.n_kf, n_pt += d.n_pts, n_ptb += d.n_pts + 1, n_ed += d.n_edges, n_ln += d.n_links;
        n_bl += st[b].blocks.size(), n_pr += st[b].pairs.size() / 2;
        n_ws += workspace_doubles(d.n_kf, d.n_free, d.n_pts, d.n_edges, d.n_links);
        n_tr += 3 * (size_t)d.iterations;
    }
    OSG_REQUIRE(ctx, n_ed < (size_t(1) << 30) && n_pr < (size_t(1) << 30) && n_pt < (size_t(1) << 28),
                "too many edges in one batch");
    osg_batch_io io(ctx);
    const osg_seg i_pr = io.in(sizeof(ProbDev), nb), i_kf = io.in(sizeof(KfDev), n_kf);
    const osg_seg i_ln = io.in(sizeof(LinkDev), n_ln), i_bl = io.in(sizeof(BlockDev), n_bl);
    const osg_seg i_pa = io.in(2 * sizeof(int32_t), n_pr), i_pb = io.in(sizeof(int32_t), n_ptb);
    const osg_seg i_pe = io.in(sizeof(int32_t), n_ed), i_ke = io.in(sizeof(int32_t), n_ed);
    const osg_seg i_ep = io.in(sizeof(int32_t), n_ed), i_ek = io.in(sizeof(int32_t), n_ed);
    const osg_seg i_kd = io.in(sizeof(int8_t), n_ed), i_ob = io.in(3 * sizeof(double), n_ed);
    const osg_seg i_ew = io.in(sizeof(float), n_ed), i_xw = io.in(3 * sizeof(double), n_pt);
    const osg_seg i_dp = io.in(sizeof(float), n_pt);
    const osg_seg o_res = io.out(sizeof(OutDev), nb), o_st = io.out(sizeof(osg_pio_state), n_kf);
    const osg_seg o_cm = io.out(12 * sizeof(double), n_kf), o_xw = io.out(3 * sizeof(double), n_pt);
    const osg_seg o_c2 = io.out(sizeof(double), n_ed), o_bd = io.out(sizeof(uint8_t), n_ed);
    const osg_seg o_tr = io.out(sizeof(double), n_tr);
    io.in(1, 256), io.out(1, 256);  // slack behind both blocks
    OSG_RC(io.stage());
    io.put(i_pr, 0, hp.data(), nb);
    for (int b = 0; b < nb; b++) {
        const ProbDev &d = hp[b];
        const osg_local_inertial_ba_problem &q = p[b];
        const Structure &s = st[b];
        KfDev *kd = io.host_in<KfDev>(i_kf, d.kf_off);
        for (int k = 0; k < d.n_kf; k++) {
            std::memset(&kd[k], 0, sizeof kd[k]);
            kd[k].state = q.kf[k].state;
            kd[k].fixed = q.kf[k].fixed != 0;
            kd[k].n_cams = q.kf[k].n_cams;
            kd[k].free_idx = s.free_idx[k];
            kd[k].flags = s.flags[k];
            kd[k].e_beg = s.kf_beg[k];
            kd[k].e_end = s.kf_beg[k + 1];
            for (int c = 0; c < q.kf[k].n_cams; c++) kd[k].cams[c] = q.kf[k].cams[c];
            kd[k].bf = q.kf[k].bf;
        }
        LinkDev *ld = io.host_in<LinkDev>(i_ln, d.link_off);
        for (int l = 0; l < d.n_links; l++) {
            pack_link(q.links[l], ld[l]);
            ld[l].active = !(q.kf[q.links[l].prev].fixed && q.kf[q.links[l].cur].fixed);
        }
        io.put(i_bl, d.block_off, s.blocks.data(), s.blocks.size());
        io.put(i_pa, d.pair_off, s.pairs.data(), s.pairs.size() / 2);
        io.put(i_pb, d.ptb_off, s.pt_beg.data(), s.pt_beg.size());
        io.put(i_pe, d.edge_off, s.pt_edges.data(), d.n_edges);
        io.put(i_ke, d.edge_off, s.kf_edges.data(), d.n_edges);
        io.put(i_ep, d.edge_off, q.e_point, d.n_edges);
        io.put(i_ek, d.edge_off, q.e_kf, d.n_edges);
        io.put(i_kd, d.edge_off, q.e_kind, d.n_edges);
        io.put(i_ob, d.edge_off, q.e_obs, d.n_edges);
        io.put(i_ew, d.edge_off, q.e_inv_sigma2, d.n_edges);
        io.put(i_xw, d.pt_off, q.xw, d.n_pts);
        io.put(i_dp, d.pt_off, q.track_depth, d.n_pts);
    }
    OSG_RC(io.upload());
    double *ws = nullptr;
    OSG_ALLOC(ctx, ws, SLOT_BA2, (n_ws + 32) * sizeof(double));
    OSG_RC(io.start());
    Args A;
    A.probs = io.dev_in<const ProbDev>(i_pr), A.kf = io.dev_in<const KfDev>(i_kf);
    A.links = io.dev_in<const LinkDev>(i_ln), A.blocks = io.dev_in<const BlockDev>(i_bl);
    A.pairs = io.dev_in<const int32_t>(i_pa), A.pt_beg = io.dev_in<const int32_t>(i_pb);
    A.pt_edges = io.dev_in<const int32_t>(i_pe), A.kf_edges = io.dev_in<const int32_t>(i_ke);
    A.e_point = io.dev_in<const int32_t>(i_ep), A.e_kf = io.dev_in<const int32_t>(i_ek);
    A.e_kind = io.dev_in<const int8_t>(i_kd), A.e_obs = io.dev_in<const double>(i_ob);
    A.xw = io.dev_in<const double>(i_xw), A.e_w = io.dev_in<const float>(i_ew), A.depth = io.dev_in<const float>(i_dp);
    A.o_state = io.dev_out<osg_pio_state>(o_st), A.o_cam = io.dev_out<double>(o_cm), A.o_xw = io.dev_out<double>(o_xw);
    A.o_chi2 = io.dev_out<double>(o_c2), A.o_trace = io.dev_out<double>(o_tr), A.ws = ws;
    A.o_bad = io.dev_out<uint8_t>(o_bd), A.out = io.dev_out<OutDev>(o_res);
    hipLaunchKernelGGL(k_local_inertial_ba, dim3(nb), dim3(NT), 0, ctx->stream, A);
    OSG_HIP_CHECK(ctx, hipGetLastError());
    OSG_RC(io.finish(io.out_bytes));
    const OutDev *res = io.result<OutDev>(o_res);
    int sum = 0;
    for (int b = 0; b < nb; b++) {
        const OutDev &o = res[b];
        const ProbDev &d = hp[b];
        r[b].chi2_initial = o.chi2_initial;
        r[b].chi2_last = o.chi2_last;
        r[b].chi2_accepted = o.chi2_accepted;
        r[b].iterations = o.iterations;
        r[b].trials_rejected = o.trials_rejected;
        r[b].solve_failed = o.solve_failed;
        r[b].failed = failed_rule(o.chi2_initial, o.chi2_last, d.large);
        io.get(r[b].state, o_st, d.kf_off, d.n_kf);
        const double *cm = io.result<double>(o_cm, d.kf_off);
        for (int k = 0; k < d.n_kf; k++) {
            std::memcpy(r[b].Rcw + 9 * k, cm + 12 * k, 9 * sizeof(double));
            std::memcpy(r[b].tcw + 3 * k, cm + 12 * k + 9, 3 * sizeof(double));
        }
        if (d.n_pts) io.get(r[b].xw, o_xw, d.pt_off, d.n_pts);
        if (d.n_edges) io.get(r[b].edge_bad, o_bd, d.edge_off, d.n_edges);
        if (r[b].edge_chi2) io.get(r[b].edge_chi2, o_c2, d.edge_off, d.n_edges);
        if (r[b].trace) io.get(r[b].trace, o_tr, d.trace_off, 3 * (size_t)o.iterations);
        sum += o.iterations;
    }
    return sum;
}

int osg_local_inertial_ba(osg_ctx *ctx, const osg_local_inertial_ba_problem *p, osg_local_inertial_ba_result *r)
{
    const int rc = osg_local_inertial_ba_batch(ctx, p, 1, r);
    return rc < 0 ? rc : r->iterations;
}

}  // extern "C"
