// poseinertial_common.h — the host side of osg_pose_inertial_optimization[_batch] that needs no device: the
// argument checks, the information matrices of EdgeInertial / EdgeGyroRW / EdgeAccRW
// (ref:src/G2oTypes.cc:582-593, ref:src/Optimizer.cc:688, 701) and the per-problem block the kernel reads.
// Plain C++ (tests/host/poseinertial_host.cpp compiles it with the host sanitizers).
#pragma once
#include <cmath>
#include <cstring>

#include "../../include/osg.h"
#include "../../include/osg_ba.h"
#include "small_linalg.h"

namespace osgpio {

constexpr int MAX_EDGES = 16384;  // 64 chunks of 256 lanes: one bit per chunk in the lane's level mask

// what the kernel reads of one problem (the edge arrays are concatenated over the batch)
struct ProbDev {
    int32_t mode, rec_init, n_cams, n_edges;
    int32_t edge_off, pad[3];
    osg_pio_state cur, prev;
    osg_pio_camera cams[2];
    double bf;
    float dR[9], dV[3], dP[3], JRg[9], JVg[9], JVa[9], JPg[9], JPa[9], b[6], dT, padf;
    double info9[81];   // EdgeInertial
    double info_rw[36]; // EdgeGyroRW and EdgeAccRW as one 6 x 6 block-diagonal information
    osg_pio_prior prior;
};

struct OutDev {
    osg_pio_state state;
    double H[225];
    int32_t n_inliers, rounds_run, iterations, solve_failed, recovered, pad[3];
};

// 0, or OSG_E_INVALID with *why naming the first violated condition
inline int check(const osg_pose_inertial_problem *p, const char **why)
{
    const char *dummy;
    if (!why) why = &dummy;
#define OSGPIO_BAD(cond, msg) \
    if (cond) {               \
        *why = msg;           \
        return OSG_E_INVALID; \
    }
    OSGPIO_BAD(!p, "null problem");
    OSGPIO_BAD(p->mode != OSG_PIO_LAST_KEYFRAME && p->mode != OSG_PIO_LAST_FRAME, "unknown mode");
    OSGPIO_BAD(p->n_cams != 1 && p->n_cams != 2, "n_cams must be 1 or 2");
    OSGPIO_BAD(p->n_edges < 0, "negative n_edges");
    OSGPIO_BAD(p->n_edges > MAX_EDGES, "too many edges");
    OSGPIO_BAD(!p->preint || !p->C_rw, "null preintegration");
    OSGPIO_BAD(p->mode == OSG_PIO_LAST_FRAME && !p->prior, "PoseInertialOptimizationLastFrame needs the prior");
    OSGPIO_BAD(p->n_edges > 0 && (!p->kind || !p->xw || !p->obs || !p->inv_sigma2 || !p->track_depth),
               "null edge array");
    for (int i = 0; i < p->n_edges; i++) {
        const int k = p->kind[i];
        OSGPIO_BAD(k != OSG_EDGE_MONO && k != OSG_EDGE_STEREO && k != OSG_EDGE_BODY, "unknown edge kind");
        OSGPIO_BAD(k == OSG_EDGE_BODY && p->n_cams != 2, "a right-camera edge without a second camera");
    }
#undef OSGPIO_BAD
    return 0;
}

// inverse of the n x n row-major A (n <= 9) by Gauss-Jordan with partial pivoting; a zero pivot leaves inf / nan
// behind as a division by zero does in the reference
template <int N>
inline void inverse(const double *A, double *inv)
{
    double M[N][2 * N];
    for (int i = 0; i < N; i++)
        for (int j = 0; j < N; j++) {
            M[i][j] = A[i * N + j];
            M[i][N + j] = i == j ? 1.0 : 0.0;
        }
    for (int c = 0; c < N; c++) {
        int piv = c;
        for (int r = c + 1; r < N; r++)
            if (std::fabs(M[r][c]) > std::fabs(M[piv][c])) piv = r;
        if (piv != c)
            for (int j = 0; j < 2 * N; j++) {
                const double t = M[c][j];
                M[c][j] = M[piv][j];
                M[piv][j] = t;
            }
        const double d = M[c][c];
        for (int j = 0; j < 2 * N; j++) M[c][j] /= d;
        for (int r = 0; r < N; r++) {
            if (r == c) continue;
            const double f = M[r][c];
            if (f == 0.0) continue;
            for (int j = 0; j < 2 * N; j++) M[r][j] -= f * M[c][j];
        }
    }
    for (int i = 0; i < N; i++)
        for (int j = 0; j < N; j++) inv[i * N + j] = M[i][N + j];
}

inline void informations(const float *C, const float *C_rw, double *info9, double *info_g, double *info_a)
{
    if (info9 && C) {
        double A[81], inv[81], S[9][9], V[9][9];
        for (int i = 0; i < 9; i++)
            for (int j = 0; j < 9; j++) A[i * 9 + j] = (double)C[i * 15 + j];
        inverse<9>(A, inv);
        for (int i = 0; i < 9; i++)
            for (int j = 0; j < 9; j++) S[i][j] = (inv[i * 9 + j] + inv[j * 9 + i]) / 2;
        osgla::jacobi_sym<double, 9>(S, V, 60, 1e-36);
        double eig[9];
        for (int i = 0; i < 9; i++) eig[i] = S[i][i] < 1e-12 ? 0.0 : S[i][i];
        for (int i = 0; i < 9; i++)
            for (int j = 0; j < 9; j++) {
                double s = 0;
                for (int k = 0; k < 9; k++) s += V[i][k] * eig[k] * V[j][k];
                info9[i * 9 + j] = s;
            }
    }
    for (int which = 0; which < 2; which++) {
        double *out = which == 0 ? info_g : info_a;
        if (!out || !C_rw) continue;
        const int o = which == 0 ? 9 : 12;
        double A[9];
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) A[i * 3 + j] = (double)C_rw[(o + i) * 15 + o + j];
        inverse<3>(A, out);
    }
}

// the kernel's view of problem p (edge_off: where its edges start in the concatenated arrays)
inline void pack(const osg_pose_inertial_problem &p, int edge_off, ProbDev &d)
{
    std::memset(&d, 0, sizeof d);
    d.mode = p.mode;
    d.rec_init = p.rec_init != 0;
    d.n_cams = p.n_cams;
    d.n_edges = p.n_edges;
    d.edge_off = edge_off;
    d.cur = p.cur;
    d.prev = p.prev;
    for (int c = 0; c < p.n_cams; c++) d.cams[c] = p.cams[c];
    d.bf = p.bf;
    const osg_pio_preintegrated &q = *p.preint;
    std::memcpy(d.dR, q.dR, sizeof d.dR);
    std::memcpy(d.dV, q.dV, sizeof d.dV);
    std::memcpy(d.dP, q.dP, sizeof d.dP);
    std::memcpy(d.JRg, q.JRg, sizeof d.JRg);
    std::memcpy(d.JVg, q.JVg, sizeof d.JVg);
    std::memcpy(d.JVa, q.JVa, sizeof d.JVa);
    std::memcpy(d.JPg, q.JPg, sizeof d.JPg);
    std::memcpy(d.JPa, q.JPa, sizeof d.JPa);
    std::memcpy(d.b, q.b, sizeof d.b);
    d.dT = q.dT;
    double ig[9], ia[9];
    informations(q.C, p.C_rw, d.info9, ig, ia);
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            d.info_rw[i * 6 + j] = ig[i * 3 + j];
            d.info_rw[(3 + i) * 6 + 3 + j] = ia[i * 3 + j];
        }
    if (p.prior) d.prior = *p.prior;
}

}  // namespace osgpio
