// essgraph4_common.h — the host side of osg_optimize_essential_graph_4dof that needs no device: the argument
// checks, the per-vertex state the kernels carry (an ImuCamPose as VertexPose4DoF holds it,
// ref:include/G2oTypes.h:58-111) and the way back to the caller's arrays.  Plain C++
// (tests/host/essgraph4_host.cpp compiles it with the host sanitizers).
#pragma once
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/osg.h"
#include "../../include/osg_ba.h"

namespace osgeg4 {

// state per vertex, in doubles: Rwb0 | DR | twb | Rcw | tcw | Rwb | its | pad.  Rcw / tcw are the cameras as
// passed until the first update re-derives them; Rwb is DR Rwb0 of the last update.
constexpr int VS = 48;
constexpr int V_RWB0 = 0, V_DR = 9, V_TWB = 18, V_RCW = 21, V_TCW = 30, V_RWB = 33, V_ITS = 42;
// constants per vertex: Rcb | tcb
constexpr int VC = 12;
// the caller's rows (include/osg_ba.h)
constexpr int I_RWB = 0, I_TWB = 9, I_RCW = 12, I_TCW = 21, I_RCB = 24, I_TCB = 33;
constexpr int O_RCW = 0, O_TCW = 9, O_RWB = 12, O_TWB = 21;

// 0, or OSG_E_INVALID with *why naming the first violated condition
inline int check(const osg_essgraph4_problem *p, const osg_essgraph4_result *r, const char **why)
{
    const char *dummy;
    if (!why) why = &dummy;
#define OSGEG4_BAD(cond, msg) \
    if (cond) {               \
        *why = msg;           \
        return OSG_E_INVALID; \
    }
    OSGEG4_BAD(!p || !r, "null argument");
    const int n = p->n_vertices, E = p->n_edges;
    OSGEG4_BAD(n < 0 || n > 65535, "n_vertices must be in [0, 65535]");
    OSGEG4_BAD(E < 0 || E > (1 << 24), "n_edges must be in [0, 2^24]");
    OSGEG4_BAD(n > 0 && (!p->pose || !p->fixed || !r->pose), "null vertex array");
    OSGEG4_BAD(E > 0 && (!p->e_v0 || !p->e_v1 || !p->e_meas), "null edge array");
    OSGEG4_BAD(p->max_iterations < 0, "negative max_iterations");
    OSGEG4_BAD(!(p->lambda_init >= 0.0), "lambda_init must not be negative");
    for (int i = 0; i < 6; i++) OSGEG4_BAD(!std::isfinite(p->info_diag[i]) || p->info_diag[i] < 0.0, "info_diag must be finite and not negative");
    for (int e = 0; e < E; e++) {
        const int a = p->e_v0[e], b = p->e_v1[e];
        OSGEG4_BAD(a < 0 || a >= n || b < 0 || b >= n, "an edge's vertex index is out of range");
        OSGEG4_BAD(a == b, "an edge joins a vertex to itself");
    }
#undef OSGEG4_BAD
    return 0;
}

// the device state and constants of every vertex as its constructor leaves them: Rwb0 = Rwb, DR = I, its = 0
inline void pack(const osg_essgraph4_problem &p, std::vector<double> &state, std::vector<double> &consts)
{
    const size_t n = (size_t)p.n_vertices;
    state.assign(VS * n, 0.0);
    consts.assign(VC * n, 0.0);
    for (size_t v = 0; v < n; v++) {
        const double *in = p.pose + OSG_EG4_POSE_IN * v;
        double *s = state.data() + VS * v, *c = consts.data() + VC * v;
        std::memcpy(s + V_RWB0, in + I_RWB, 9 * sizeof(double));
        s[V_DR] = s[V_DR + 4] = s[V_DR + 8] = 1.0;
        std::memcpy(s + V_TWB, in + I_TWB, 3 * sizeof(double));
        std::memcpy(s + V_RCW, in + I_RCW, 9 * sizeof(double));
        std::memcpy(s + V_TCW, in + I_TCW, 3 * sizeof(double));
        std::memcpy(s + V_RWB, in + I_RWB, 9 * sizeof(double));
        std::memcpy(c, in + I_RCB, 9 * sizeof(double));
        std::memcpy(c + 9, in + I_TCB, 3 * sizeof(double));
    }
}

// vertex v's output row: the returned state, or for a fixed vertex its input, bit for bit
inline void unpack(const osg_essgraph4_problem &p, int v, const double *state, double *out)
{
    if (p.fixed[v]) {
        const double *in = p.pose + OSG_EG4_POSE_IN * (size_t)v;
        std::memcpy(out + O_RCW, in + I_RCW, 9 * sizeof(double));
        std::memcpy(out + O_TCW, in + I_TCW, 3 * sizeof(double));
        std::memcpy(out + O_RWB, in + I_RWB, 9 * sizeof(double));
        std::memcpy(out + O_TWB, in + I_TWB, 3 * sizeof(double));
        return;
    }
    const double *s = state + VS * (size_t)v;
    std::memcpy(out + O_RCW, s + V_RCW, 9 * sizeof(double));
    std::memcpy(out + O_TCW, s + V_TCW, 3 * sizeof(double));
    std::memcpy(out + O_RWB, s + V_RWB, 9 * sizeof(double));
    std::memcpy(out + O_TWB, s + V_TWB, 3 * sizeof(double));
}

}  // namespace osgeg4
