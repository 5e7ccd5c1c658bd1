// inertialopt_common.h — the host side of osg_inertial_optimization[_batch] that needs no device: the argument
// checks, the order of the KeyFrames along their mPrevKF chains, and the blocks the kernel reads.  Plain C++.
#pragma once
#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/osg.h"
#include "../../include/osg_ba.h"
#include "poseinertial_common.h"

namespace osgio {

constexpr int NB = 9;    // the border: bg (3) | ba (3) | gdir (2) | scale (1)
constexpr int NJ = 15;   // an edge's columns: v1 (3) | v2 (3) | border (9)
constexpr int NE = 136;  // per edge: upper triangle of J' W J (120) | -J' W e (15) | robust chi2 (1)
constexpr int NP = 117;  // per chain position: D (9) | O (9) | C (27) | b (3) | Y (39) | C' (27) | b' (3)

// one KeyFrame in chain order
struct KfDev {
    double Rwb[9], twb[3];
};

// the edge between chain positions k and k + 1 (has == 0: none)
struct EdgeDev {
    float dR[9], dV[3], dP[3], JRg[9], JVg[9], JVa[9], JPg[9], JPa[9], b[6], dT;
    int32_t has;
    double info[81];
};

struct ProbDev {
    int32_t n_kf, kf_off, algorithm, iterations;
    int32_t has_priors, free_vb, free_gdir, free_scale;
    int64_t ws_off, trace_off;  // in doubles
    double bg[3], ba[3], Rwg[9], scale;
    double prior_g, prior_a, lambda_init, huber_delta;
};

struct OutDev {
    double bg[3], ba[3], Rwg[9], scale, chi2_initial, chi2_final;
    int32_t iterations, trials_rejected, solve_failed, pad;
};

// doubles of device workspace behind one problem: the edges' blocks, the chain's blocks, x, the velocity backup
inline size_t workspace_doubles(int n_kf) { return (size_t)n_kf * (NE + NP + 3 + 3); }

// 0, or OSG_E_INVALID with *why naming the first violated condition.  With order / edge_at: the KeyFrames along
// their chains (order[k]: the KeyFrame at position k) and the edge from position k to k + 1 (-1: none).  The chains
// with an edge come first, sorted by their head's (twb, Rwb, v) so that the order does not depend on the caller's
// numbering; the edge-less KeyFrames follow.
inline int check(const osg_inertial_problem *p, const char **why, std::vector<int> *order = nullptr,
                 std::vector<int> *edge_at = nullptr)
{
    const char *dummy;
    if (!why) why = &dummy;
#define OSGIO_BAD(cond, msg)  \
    if (cond) {               \
        *why = msg;           \
        return OSG_E_INVALID; \
    }
    OSGIO_BAD(!p, "null problem");
    OSGIO_BAD(p->n_kf < 0 || p->n_edges < 0, "negative count");
    OSGIO_BAD(p->n_kf > OSG_INERTIAL_MAX_KF, "too many KeyFrames");
    OSGIO_BAD(p->n_kf > 0 && (!p->Rwb || !p->twb || !p->v), "null KeyFrame array");
    OSGIO_BAD(p->n_edges > 0 && (!p->prev || !p->cur || !p->preint), "null edge array");
    OSGIO_BAD(p->algorithm != OSG_INERTIAL_LM && p->algorithm != OSG_INERTIAL_GN, "unknown algorithm");
    OSGIO_BAD(p->iterations < 0 || p->iterations > OSG_INERTIAL_MAX_ITERATIONS, "iterations out of range");
    OSGIO_BAD(!p->free_vel_bias && !p->free_gdir && !p->free_scale, "nothing is free");
    OSGIO_BAD(!(p->lambda_init >= 0.0) || !(p->huber_delta >= 0.0), "negative lambda_init or huber_delta");
    const int n = p->n_kf;
    std::vector<int> next(n, -1), pred(n, -1);
    for (int e = 0; e < p->n_edges; e++) {
        const int a = p->prev[e], b = p->cur[e];
        OSGIO_BAD(a < 0 || a >= n || b < 0 || b >= n, "edge index out of range");
        OSGIO_BAD(a == b, "an edge from a KeyFrame to itself");
        OSGIO_BAD(next[a] >= 0, "a KeyFrame is prev of two edges");
        OSGIO_BAD(pred[b] >= 0, "a KeyFrame is cur of two edges");
        next[a] = e;
        pred[b] = e;
    }
    std::vector<int> heads, ord, eat;
    for (int i = 0; i < n; i++)
        if (pred[i] < 0 && next[i] >= 0) heads.push_back(i);
    auto key_less = [&](int a, int b) {
        for (int i = 0; i < 3; i++)
            if (p->twb[3 * a + i] != p->twb[3 * b + i]) return p->twb[3 * a + i] < p->twb[3 * b + i];
        for (int i = 0; i < 9; i++)
            if (p->Rwb[9 * a + i] != p->Rwb[9 * b + i]) return p->Rwb[9 * a + i] < p->Rwb[9 * b + i];
        for (int i = 0; i < 3; i++)
            if (p->v[3 * a + i] != p->v[3 * b + i]) return p->v[3 * a + i] < p->v[3 * b + i];
        return a < b;
    };
    std::sort(heads.begin(), heads.end(), key_less);
    ord.reserve(n);
    eat.reserve(n);
    for (int h : heads) {
        int i = h;
        while (true) {
            ord.push_back(i);
            const int e = next[i];
            eat.push_back(e);
            if (e < 0) break;
            i = p->cur[e];
        }
    }
    int in_chain = 0;
    for (int i = 0; i < n; i++) in_chain += (pred[i] >= 0 || next[i] >= 0) ? 1 : 0;
    OSGIO_BAD((int)ord.size() != in_chain, "the edges form a cycle");
    for (int i = 0; i < n; i++)
        if (pred[i] < 0 && next[i] < 0) {
            ord.push_back(i);
            eat.push_back(-1);
        }
#undef OSGIO_BAD
    if (order) order->swap(ord);
    if (edge_at) edge_at->swap(eat);
    return 0;
}

inline void pack(const osg_inertial_problem &p, int kf_off, int64_t ws_off, int64_t trace_off, ProbDev &d)
{
    std::memset(&d, 0, sizeof d);
    d.n_kf = p.n_kf;
    d.kf_off = kf_off;
    d.algorithm = p.algorithm;
    d.iterations = p.iterations;
    d.free_vb = p.free_vel_bias != 0;
    d.free_gdir = p.free_gdir != 0;
    d.free_scale = p.free_scale != 0;
    // a prior edge whose only vertex is fixed is not active (g2o's initializeOptimization skips it)
    d.has_priors = p.has_priors != 0 && d.free_vb;
    d.ws_off = ws_off;
    d.trace_off = trace_off;
    std::memcpy(d.bg, p.bg, sizeof d.bg);
    std::memcpy(d.ba, p.ba, sizeof d.ba);
    std::memcpy(d.Rwg, p.Rwg, sizeof d.Rwg);
    d.scale = p.scale;
    d.prior_g = p.prior_g;
    d.prior_a = p.prior_a;
    d.lambda_init = p.lambda_init;
    d.huber_delta = p.huber_delta;
}

inline void pack_edge(const osg_pio_preintegrated &q, EdgeDev &d)
{
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
    d.has = 1;
    osgpio::informations(q.C, nullptr, d.info, nullptr, nullptr);
}

}  // namespace osgio
