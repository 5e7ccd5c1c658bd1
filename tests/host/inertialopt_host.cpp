// inertialopt_host.cpp — the host side of osg_inertial_optimization that needs no device (csrc/inertialopt_common.h)
// as a stand-alone program, for the host sanitizers (test-only; tests/test_inertialopt.py):
//   check    the chain order of a map of two chains and an edge-less KeyFrame, the same map with KeyFrames and edges
//            shuffled (the same KeyFrames at the same positions), and every malformed shape the check refuses
#include <cstdio>
#include <numeric>
#include <string>

#include "inertialopt_common.h"

namespace {

struct Map {
    std::vector<double> Rwb, twb, v;
    std::vector<int32_t> prev, cur;
    std::vector<osg_pio_preintegrated> pre;
    osg_inertial_problem p{};
    void bind()
    {
        p.n_kf = (int32_t)(twb.size() / 3);
        p.Rwb = Rwb.data(), p.twb = twb.data(), p.v = v.data();
        p.n_edges = (int32_t)prev.size();
        p.prev = prev.data(), p.cur = cur.data(), p.preint = pre.data();
        p.free_vel_bias = p.free_gdir = p.free_scale = 1;
        p.algorithm = OSG_INERTIAL_LM;
        p.iterations = 200;
    }
};

Map two_chains()
{
    Map m;
    const int n = 10;
    for (int i = 0; i < n; i++) {
        const double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
        m.Rwb.insert(m.Rwb.end(), R, R + 9);
        // the second chain's head (KeyFrame 5) lies before the first's (KeyFrame 0) in the key order
        for (int k = 0; k < 3; k++) m.twb.push_back(i == 5 ? -3.0 + k : 0.5 * i + k);
        for (int k = 0; k < 3; k++) m.v.push_back(0.1 * i - k);
    }
    for (int i = 1; i < 5; i++) m.prev.push_back(i - 1), m.cur.push_back(i);
    for (int i = 6; i < 9; i++) m.prev.push_back(i - 1), m.cur.push_back(i);
    m.pre.resize(m.prev.size());
    m.bind();
    return m;
}

int fail(const char *what)
{
    std::printf("FAILED: %s\n", what);
    return 1;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc < 2 || std::string(argv[1]) != "check") return 2;
    const char *why = "";
    std::vector<int> order, edge_at;
    Map m = two_chains();
    if (osgio::check(&m.p, &why, &order, &edge_at) != 0) return fail(why);
    const std::vector<int> want = {5, 6, 7, 8, 0, 1, 2, 3, 4, 9};
    const std::vector<int> want_e = {4, 5, 6, -1, 0, 1, 2, 3, -1, -1};
    if (order != want || edge_at != want_e) return fail("chain order");
    // shuffle: new KeyFrame j is old KeyFrame perm[j]; the edges in another order
    const std::vector<int> perm = {7, 2, 9, 0, 5, 4, 8, 1, 6, 3}, eperm = {3, 6, 0, 5, 1, 4, 2};
    std::vector<int> inv(10);
    for (int j = 0; j < 10; j++) inv[perm[j]] = j;
    Map s;
    for (int j = 0; j < 10; j++) {
        s.Rwb.insert(s.Rwb.end(), m.Rwb.begin() + 9 * perm[j], m.Rwb.begin() + 9 * perm[j] + 9);
        s.twb.insert(s.twb.end(), m.twb.begin() + 3 * perm[j], m.twb.begin() + 3 * perm[j] + 3);
        s.v.insert(s.v.end(), m.v.begin() + 3 * perm[j], m.v.begin() + 3 * perm[j] + 3);
    }
    for (int e : eperm) s.prev.push_back(inv[m.prev[e]]), s.cur.push_back(inv[m.cur[e]]);
    s.pre.resize(s.prev.size());
    s.bind();
    std::vector<int> order2, edge2;
    if (osgio::check(&s.p, &why, &order2, &edge2) != 0) return fail(why);
    for (int k = 0; k < 10; k++) {
        if (perm[order2[k]] != order[k]) return fail("the shuffled map puts another KeyFrame at a position");
        if ((edge2[k] < 0) != (edge_at[k] < 0) || (edge2[k] >= 0 && eperm[edge2[k]] != edge_at[k]))
            return fail("the shuffled map puts another edge at a position");
    }
    // the refusals
    if (osgio::check(nullptr, &why) != OSG_E_INVALID) return fail("null problem");
    struct Case {
        const char *name;
        void (*edit)(Map &);
    };
    const Case cases[] = {
        {"two successors", [](Map &q) { q.prev[3] = q.prev[2]; }},
        {"two predecessors", [](Map &q) { q.cur[3] = q.cur[2]; }},
        {"index below range", [](Map &q) { q.cur[6] = -1; }},
        {"index above range", [](Map &q) { q.prev[0] = 10; }},
        {"self edge", [](Map &q) { q.cur[0] = q.prev[0]; }},
        {"cycle", [](Map &q) { q.prev.push_back(4), q.cur.push_back(0), q.pre.resize(q.prev.size()), q.bind(); }},
        {"over the cap", [](Map &q) { q.p.n_kf = OSG_INERTIAL_MAX_KF + 1; }},
        {"unknown algorithm", [](Map &q) { q.p.algorithm = 7; }},
        {"negative iterations", [](Map &q) { q.p.iterations = -1; }},
        {"nothing free", [](Map &q) { q.p.free_vel_bias = q.p.free_gdir = q.p.free_scale = 0; }},
        {"null edge array", [](Map &q) { q.p.preint = nullptr; }},
        {"null KeyFrame array", [](Map &q) { q.p.twb = nullptr; }},
    };
    for (const Case &c : cases) {
        Map q = two_chains();
        c.edit(q);
        std::vector<int> o = {1, 2, 3}, e = {4};
        if (osgio::check(&q.p, &why, &o, &e) != OSG_E_INVALID) return fail(c.name);
        if (o != std::vector<int>{1, 2, 3} || e != std::vector<int>{4}) return fail("outputs written on a refusal");
    }
    // the device blocks
    osgio::ProbDev d;
    osgio::pack(m.p, 3, 17, 19, d);
    if (d.n_kf != 10 || d.kf_off != 3 || d.ws_off != 17 || d.trace_off != 19 || d.has_priors) return fail("pack");
    osgio::EdgeDev ed;
    std::memset(&ed, 0, sizeof ed);
    osg_pio_preintegrated q{};
    for (int i = 0; i < 15; i++) q.C[16 * i] = 1e-4f * (i + 1);
    osgio::pack_edge(q, ed);
    if (!ed.has || !(ed.info[0] > 9.9e3 && ed.info[0] < 1.01e4)) return fail("pack_edge");
    if (osgio::workspace_doubles(10) != 10u * (osgio::NE + osgio::NP + 6)) return fail("workspace");
    std::printf("ok\n");
    return 0;
}
