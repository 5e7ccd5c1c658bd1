// essgraph4_host.cpp — the host side of osg_optimize_essential_graph_4dof without a device (test-only;
// tests/test_essgraph4dof.py builds it plain and with the host sanitizers and compares what both print).
//   layout   the size and the field offsets of osg_essgraph4_problem / osg_essgraph4_result
//   pack     csrc/essgraph4_common.h on a 3-vertex, 2-edge problem whose vertex v holds the values 100 v + k:
//            check() on it and on every rejected variant, then the packed state and constants and the
//            unpacked rows of a state the "device" filled with 1000 v + k
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "essgraph4_common.h"

#define F(st, f) std::printf(#st "." #f " %zu\n", offsetof(st, f))

static int layout()
{
    std::printf("osg_essgraph4_problem %zu\n", sizeof(osg_essgraph4_problem));
    F(osg_essgraph4_problem, n_vertices); F(osg_essgraph4_problem, pose); F(osg_essgraph4_problem, fixed);
    F(osg_essgraph4_problem, n_edges); F(osg_essgraph4_problem, e_v0); F(osg_essgraph4_problem, e_v1);
    F(osg_essgraph4_problem, e_meas); F(osg_essgraph4_problem, info_diag); F(osg_essgraph4_problem, max_iterations);
    F(osg_essgraph4_problem, lambda_init);
    std::printf("osg_essgraph4_result %zu\n", sizeof(osg_essgraph4_result));
    F(osg_essgraph4_result, pose); F(osg_essgraph4_result, chi2_initial); F(osg_essgraph4_result, chi2_final);
    F(osg_essgraph4_result, lm_iterations); F(osg_essgraph4_result, lm_trials); F(osg_essgraph4_result, edge_chi2);
    return 0;
}

static int pack()
{
    const int n = 3, E = 2;
    std::vector<double> pose(OSG_EG4_POSE_IN * n), meas(12 * E, 0.25), out(OSG_EG4_POSE_OUT * n, -7.0);
    for (int v = 0; v < n; v++)
        for (int k = 0; k < OSG_EG4_POSE_IN; k++) pose[OSG_EG4_POSE_IN * v + k] = 100.0 * v + k;
    const uint8_t fixed[n] = {0, 1, 0};
    int32_t v0[E] = {1, 2}, v1[E] = {0, 1};
    osg_essgraph4_problem p;
    std::memset(&p, 0, sizeof p);
    p.n_vertices = n; p.pose = pose.data(); p.fixed = fixed;
    p.n_edges = E; p.e_v0 = v0; p.e_v1 = v1; p.e_meas = meas.data();
    for (int i = 0; i < 6; i++) p.info_diag[i] = 1.0 + i;
    osg_essgraph4_result r;
    std::memset(&r, 0, sizeof r);
    r.pose = out.data();
    const char *why = "";
    std::printf("valid %d\n", osgeg4::check(&p, &r, &why));
    auto bad = [&](const char *name, osg_essgraph4_problem q, osg_essgraph4_result s) {
        const char *w = "";
        const int rc = osgeg4::check(&q, &s, &w);
        std::printf("%s %d %s\n", name, rc, rc ? w : "-");
    };
    { auto q = p; q.n_vertices = -1; bad("n_vertices_negative", q, r); }
    { auto q = p; q.n_vertices = 65536; bad("n_vertices_65536", q, r); }
    { auto q = p; q.n_edges = -1; bad("n_edges_negative", q, r); }
    { auto q = p; q.pose = nullptr; bad("null_pose", q, r); }
    { auto q = p; q.fixed = nullptr; bad("null_fixed", q, r); }
    { auto q = p; q.e_v0 = nullptr; bad("null_e_v0", q, r); }
    { auto q = p; q.e_v1 = nullptr; bad("null_e_v1", q, r); }
    { auto q = p; q.e_meas = nullptr; bad("null_e_meas", q, r); }
    { auto s = r; s.pose = nullptr; bad("null_output", p, s); }
    { auto q = p; q.max_iterations = -1; bad("max_iterations_negative", q, r); }
    { auto q = p; q.lambda_init = -1e-16; bad("lambda_negative", q, r); }
    { auto q = p; q.lambda_init = std::nan(""); bad("lambda_nan", q, r); }
    { auto q = p; q.info_diag[2] = -1.0; bad("info_negative", q, r); }
    { auto q = p; q.info_diag[5] = std::numeric_limits<double>::infinity(); bad("info_inf", q, r); }
    { auto q = p; q.info_diag[0] = std::nan(""); bad("info_nan", q, r); }
    v0[1] = n; bad("e_v0_is_n", p, r); v0[1] = 2;
    v1[0] = -1; bad("e_v1_negative", p, r); v1[0] = 0;
    v0[0] = 0; bad("self_edge", p, r); v0[0] = 1;
    std::printf("null_problem %d\n", osgeg4::check(nullptr, &r, nullptr));
    std::printf("null_result %d\n", osgeg4::check(&p, nullptr, nullptr));
    { auto q = p; q.n_vertices = 0; q.n_edges = 0; q.pose = nullptr; q.fixed = nullptr; bad("empty_graph_is_valid", q, r); }

    std::vector<double> state, consts;
    osgeg4::pack(p, state, consts);
    std::printf("state %zu consts %zu\n", state.size(), consts.size());
    for (int v = 0; v < n; v++) {
        std::printf("s%d", v);
        for (int k = 0; k < osgeg4::VS; k++) std::printf(" %g", state[osgeg4::VS * v + k]);
        std::printf("\nc%d", v);
        for (int k = 0; k < osgeg4::VC; k++) std::printf(" %g", consts[osgeg4::VC * v + k]);
        std::printf("\n");
    }
    for (int v = 0; v < n; v++)
        for (int k = 0; k < osgeg4::VS; k++) state[osgeg4::VS * v + k] = 1000.0 * v + k;
    for (int v = 0; v < n; v++) {
        osgeg4::unpack(p, v, state.data(), out.data() + OSG_EG4_POSE_OUT * v);
        std::printf("o%d", v);
        for (int k = 0; k < OSG_EG4_POSE_OUT; k++) std::printf(" %g", out[OSG_EG4_POSE_OUT * v + k]);
        std::printf("\n");
    }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 2 && !std::strcmp(argv[1], "layout")) return layout();
    if (argc == 2 && !std::strcmp(argv[1], "pack")) return pack();
    std::fprintf(stderr, "usage: essgraph4_host layout|pack\n");
    return 2;
}
