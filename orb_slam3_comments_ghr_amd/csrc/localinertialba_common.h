// localinertialba_common.h — the host side of osg_local_inertial_ba[_batch] that needs no device: the argument
// checks, the fixed-order structure of a window (the edge lists per point and per KeyFrame, the lists of edge
// pairs per pair of free KeyFrames that the reduced system is assembled from), the per-problem blocks the kernel
// reads, the workspace layout, and the `failed` rule of ref:src/Optimizer.cc:2701-2703, 2749 on its float casts.
// Plain C++ (tests/host/localinertialba_host.cpp compiles it with the host sanitizers).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/osg.h"
#include "../../include/osg_ba.h"
#include "poseinertial_common.h"

namespace osgliba {

constexpr int NU = 15;    // unknowns of a free KeyFrame: pose 6 | v 3 | bg 3 | ba 3
constexpr int KST = 46;   // a KeyFrame's mutable state: Rwb 9 | twb 3 | v 3 | bg 3 | ba 3 | Rcw 2 x 9 | tcw 2 x 3 | its
constexpr int EWN = 56;   // per visual edge: Hpp 21 | W 18 | Hll 6 | bp 6 | bl 3 | rho0 | chi2
constexpr int E_HPP = 0, E_W = 21, E_HLL = 39, E_BP = 45, E_BL = 51, E_R0 = 54, E_CHI = 55;
constexpr int EYN = 18;   // per visual edge: Y = W V^-1
constexpr int PWN = 18;   // per point: sum Hll 6 | sum bl 3 | V^-1 6 | x 3
constexpr int P_H = 0, P_B = 6, P_VI = 9, P_X = 15;
constexpr int LJ = 24;    // EdgeInertial's columns: VP1 6 | VV1 3 | VG1 3 | VA1 3 | VP2 6 | VV2 3
constexpr int LWN = 2 * 9 * LJ + LJ + 12 + 4;  // per link: J | rho1 Omega J | -rho1 J' Omega e | RW b (6 + 6) | rho0 x 3, spare
constexpr int L_J = 0, L_WJ = 9 * LJ, L_B = 2 * 9 * LJ, L_RWB = L_B + LJ, L_R0 = L_RWB + 12;

// KeyFrame flags
constexpr int KF_LINKED = 1;  // prev or cur of a link: v, bg, ba are active vertices
constexpr int KF_POSE = 2;    // the pose is an active vertex: a visual edge or a link

struct ProbDev {
    int32_t n_kf, n_free, n_pts, n_edges, n_links, n_blocks, iterations, large;
    int32_t kf_off, pt_off, edge_off, link_off, block_off, ptb_off;  // ptb_off: the points' CSR (n_pts + 1 entries)
    int64_t pair_off, ws_off, trace_off;
    double lambda_init;
};

struct KfDev {
    osg_pio_state state;
    int32_t fixed, n_cams, free_idx, flags;
    int32_t e_beg, e_end;  // its edges in the per-KeyFrame edge list, insertion order
    osg_pio_camera cams[2];
    double bf;
};

struct LinkDev {
    int32_t prev, cur, huber, active;  // active: not all of its vertices are fixed
    float dR[9], dV[3], dP[3], JRg[9], JVg[9], JVa[9], JPg[9], JPa[9], b[6], dT, padf;
    double info9[81], info_g[9], info_a[9];
};

// the edge pairs (a on free KeyFrame fi, b on free KeyFrame fj >= fi, same point) of one block of the reduced system
struct BlockDev {
    int32_t fi, fj, beg, end;
};

struct OutDev {
    double chi2_initial, chi2_last, chi2_accepted;
    int32_t iterations, trials_rejected, solve_failed, pad;
};

// the fixed-order structure of one window
struct Structure {
    std::vector<int32_t> free_idx, flags;        // per KeyFrame
    std::vector<int32_t> pt_beg, pt_edges;       // CSR over the points (n_pts + 1 | n_edges), insertion order
    std::vector<int32_t> kf_beg, kf_edges;       // CSR over the KeyFrames
    std::vector<BlockDev> blocks;                // sorted by (fi, fj)
    std::vector<int32_t> pairs;                  // 2 per pair: (edge a, edge b)
    int n_free = 0;
};

// the entries of the edge-pair lists of a problem whose indices are in range: per point, with c_f of its edges on
// free KeyFrame f, sum over f < g of c_f c_g plus sum over f of c_f^2
inline int64_t count_pairs(const osg_local_inertial_ba_problem &p)
{
    std::vector<int64_t> key;
    key.reserve((size_t)p.n_edges);
    for (int i = 0; i < p.n_edges; i++)
        if (!p.kf[p.e_kf[i]].fixed) key.push_back((int64_t)p.e_point[i] * p.n_kf + p.e_kf[i]);
    std::sort(key.begin(), key.end());
    int64_t total = 0, sum = 0, squares = 0;
    for (size_t i = 0; i < key.size();) {
        size_t j = i;
        while (j < key.size() && key[j] == key[i]) j++;
        const int64_t c = (int64_t)(j - i);
        sum += c, squares += c * c;
        if (j == key.size() || key[j] / p.n_kf != key[i] / p.n_kf) {  // the point's last KeyFrame
            total += (sum * sum + squares) / 2;
            sum = squares = 0;
        }
        i = j;
    }
    return total;
}

// 0, or OSG_E_INVALID with *why naming the first violated condition
inline int check(const osg_local_inertial_ba_problem *p, const char **why)
{
    const char *dummy;
    if (!why) why = &dummy;
#define OSGLIBA_BAD(cond, msg) \
    if (cond) {                \
        *why = msg;            \
        return OSG_E_INVALID;  \
    }
    OSGLIBA_BAD(!p, "null problem");
    OSGLIBA_BAD(p->n_kf < 0 || p->n_points < 0 || p->n_edges < 0 || p->n_links < 0, "negative count");
    OSGLIBA_BAD(p->n_points > OSG_LIBA_MAX_POINTS, "too many points");
    OSGLIBA_BAD(p->n_edges > OSG_LIBA_MAX_EDGES, "too many edges");
    OSGLIBA_BAD(p->n_kf > OSG_LIBA_MAX_FREE_KF + OSG_LIBA_MAX_FIXED_KF, "too many KeyFrames");
    OSGLIBA_BAD(p->n_links > p->n_kf, "too many links");
    OSGLIBA_BAD(p->iterations < 0 || p->iterations > OSG_LIBA_MAX_ITERATIONS, "iterations out of range");
    OSGLIBA_BAD(!(p->lambda_init > 0.0) || !std::isfinite(p->lambda_init), "lambda_init must be positive");
    OSGLIBA_BAD(p->n_kf > 0 && !p->kf, "null KeyFrame array");
    OSGLIBA_BAD(p->n_points > 0 && (!p->xw || !p->track_depth), "null point array");
    OSGLIBA_BAD(p->n_edges > 0 && (!p->e_point || !p->e_kf || !p->e_kind || !p->e_obs || !p->e_inv_sigma2),
                "null edge array");
    OSGLIBA_BAD(p->n_links > 0 && !p->links, "null link array");
    int n_free = 0, n_fixed = 0;
    for (int k = 0; k < p->n_kf; k++) {
        OSGLIBA_BAD(p->kf[k].n_cams != 1 && p->kf[k].n_cams != 2, "n_cams must be 1 or 2");
        (p->kf[k].fixed ? n_fixed : n_free)++;
    }
    OSGLIBA_BAD(n_free == 0, "nothing free");
    OSGLIBA_BAD(n_free > OSG_LIBA_MAX_FREE_KF, "too many free KeyFrames");
    OSGLIBA_BAD(n_fixed > OSG_LIBA_MAX_FIXED_KF, "too many fixed KeyFrames");
    for (int i = 0; i < p->n_edges; i++) {
        OSGLIBA_BAD(p->e_point[i] < 0 || p->e_point[i] >= p->n_points, "edge point index out of range");
        OSGLIBA_BAD(p->e_kf[i] < 0 || p->e_kf[i] >= p->n_kf, "edge KeyFrame index out of range");
        const int k = p->e_kind[i];
        OSGLIBA_BAD(k != OSG_EDGE_MONO && k != OSG_EDGE_STEREO && k != OSG_EDGE_BODY, "unknown edge kind");
        OSGLIBA_BAD(k == OSG_EDGE_BODY && p->kf[p->e_kf[i]].n_cams != 2, "a right-camera edge on a one-camera KeyFrame");
    }
    std::vector<uint8_t> is_cur((size_t)p->n_kf, 0);
    for (int l = 0; l < p->n_links; l++) {
        const osg_liba_link &L = p->links[l];
        OSGLIBA_BAD(L.prev < 0 || L.prev >= p->n_kf || L.cur < 0 || L.cur >= p->n_kf, "link index out of range");
        OSGLIBA_BAD(L.prev == L.cur, "a link from a KeyFrame to itself");
        OSGLIBA_BAD(is_cur[L.cur], "a KeyFrame that is cur of two links");
        is_cur[L.cur] = 1;
    }
    OSGLIBA_BAD(count_pairs(*p) > OSG_LIBA_MAX_PAIRS, "too many edge pairs");
#undef OSGLIBA_BAD
    return 0;
}

// the structure of a checked problem; false when the pair lists would pass OSG_LIBA_MAX_PAIRS
inline bool build_structure(const osg_local_inertial_ba_problem &p, Structure &s)
{
    const int nk = p.n_kf, np = p.n_points, ne = p.n_edges;
    s.free_idx.assign(nk, -1);
    s.flags.assign(nk, 0);
    s.n_free = 0;
    for (int k = 0; k < nk; k++)
        if (!p.kf[k].fixed) s.free_idx[k] = s.n_free++;
    // g2o keeps no edge whose vertices are all fixed (allVerticesFixed)
    for (int l = 0; l < p.n_links; l++) {
        const osg_liba_link &L = p.links[l];
        if (p.kf[L.prev].fixed && p.kf[L.cur].fixed) continue;
        s.flags[L.prev] |= KF_LINKED | KF_POSE;
        s.flags[L.cur] |= KF_LINKED | KF_POSE;
    }
    s.pt_beg.assign(np + 1, 0);
    s.kf_beg.assign(nk + 1, 0);
    for (int i = 0; i < ne; i++) {
        s.pt_beg[p.e_point[i] + 1]++;
        s.kf_beg[p.e_kf[i] + 1]++;
        s.flags[p.e_kf[i]] |= KF_POSE;
    }
    for (int i = 0; i < np; i++) s.pt_beg[i + 1] += s.pt_beg[i];
    for (int k = 0; k < nk; k++) s.kf_beg[k + 1] += s.kf_beg[k];
    s.pt_edges.assign(ne, 0);
    s.kf_edges.assign(ne, 0);
    {
        std::vector<int32_t> pa(s.pt_beg.begin(), s.pt_beg.end() - 1), ka(s.kf_beg.begin(), s.kf_beg.end() - 1);
        for (int i = 0; i < ne; i++) {
            s.pt_edges[pa[p.e_point[i]]++] = i;
            s.kf_edges[ka[p.e_kf[i]]++] = i;
        }
    }
    // pairs per block: count, then fill in point order (and within a point in insertion order of a, then b)
    const int nf = s.n_free;
    std::vector<int64_t> cnt((size_t)nf * nf, 0);
    int64_t total = 0;
    auto each_pair = [&](auto &&f) {
        for (int q = 0; q < np; q++)
            for (int ia = s.pt_beg[q]; ia < s.pt_beg[q + 1]; ia++) {
                const int a = s.pt_edges[ia], fa = s.free_idx[p.e_kf[a]];
                if (fa < 0) continue;
                for (int ib = s.pt_beg[q]; ib < s.pt_beg[q + 1]; ib++) {
                    const int b = s.pt_edges[ib], fb = s.free_idx[p.e_kf[b]];
                    if (fb < fa) continue;  // fixed, or the transposed block's pair
                    f(a, b, fa, fb);
                }
            }
    };
    each_pair([&](int, int, int fa, int fb) {
        cnt[(size_t)fa * nf + fb]++;
        total++;
    });
    if (total > OSG_LIBA_MAX_PAIRS) return false;
    s.blocks.clear();
    std::vector<int64_t> at((size_t)nf * nf, -1);
    int64_t off = 0;
    for (int fi = 0; fi < nf; fi++)
        for (int fj = fi; fj < nf; fj++) {
            const int64_t c = cnt[(size_t)fi * nf + fj];
            if (!c) continue;
            at[(size_t)fi * nf + fj] = off;
            s.blocks.push_back({fi, fj, (int32_t)off, (int32_t)(off + c)});
            off += c;
        }
    s.pairs.assign(2 * (size_t)total, 0);
    each_pair([&](int a, int b, int fa, int fb) {
        int64_t &w = at[(size_t)fa * nf + fb];
        s.pairs[2 * w] = a;
        s.pairs[2 * w + 1] = b;
        w++;
    });
    return true;
}

// doubles of workspace of one window
inline size_t workspace_doubles(int n_kf, int n_free, int n_pts, int n_edges, int n_links)
{
    const size_t n = (size_t)NU * n_free;
    return 2 * (size_t)KST * n_kf + 6 * (size_t)n_pts + (size_t)(EWN + EYN) * n_edges + (size_t)PWN * n_pts +
           (size_t)LWN * n_links + 2 * n * n + 4 * n + 64;
}

inline void pack_link(const osg_liba_link &L, LinkDev &d)
{
    std::memset(&d, 0, sizeof d);
    d.prev = L.prev;
    d.cur = L.cur;
    d.huber = L.huber != 0;
    const osg_pio_preintegrated &q = L.preint;
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
    osgpio::informations(q.C, q.C, d.info9, d.info_g, d.info_a);
    if (L.downweight)  // vei[i]->setInformation(vei[i]->information() * 1e-2)
        for (int i = 0; i < 81; i++) d.info9[i] = d.info9[i] * 1e-2;
}

// float err = chi2_initial, err_end = chi2_last: (2 * err < err_end || isnan(err) || isnan(err_end)) && !bLarge
inline int failed_rule(double chi2_initial, double chi2_last, int large)
{
    const float err = (float)chi2_initial, err_end = (float)chi2_last;
    return ((2 * err < err_end || std::isnan(err) || std::isnan(err_end)) && !large) ? 1 : 0;
}

}  // namespace osgliba
