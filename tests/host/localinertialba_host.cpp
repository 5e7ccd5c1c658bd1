// localinertialba_host.cpp — the host side of osg_local_inertial_ba that needs no device
// (csrc/localinertialba_common.h) as a stand-alone program, for the host sanitizers (test-only;
// tests/test_localinertialba.py):
//   check    the fixed-order structure of a small window (the edge lists per point and per KeyFrame, the pair lists
//            per block of the reduced system, the flags), every malformed shape the check refuses, the link block
//            with its informations and the downweight, and the `failed` rule on the float casts
#include <cstdio>
#include <limits>
#include <string>

#include "localinertialba_common.h"

namespace {

struct Window {
    std::vector<osg_liba_keyframe> kf;
    std::vector<double> xw, obs;
    std::vector<float> depth, w;
    std::vector<int32_t> ep, ek;
    std::vector<int8_t> kind;
    std::vector<osg_liba_link> links;
    osg_local_inertial_ba_problem p{};
    void bind()
    {
        p.n_kf = (int32_t)kf.size(), p.kf = kf.data();
        p.n_points = (int32_t)depth.size(), p.xw = xw.data(), p.track_depth = depth.data();
        p.n_edges = (int32_t)ep.size(), p.e_point = ep.data(), p.e_kf = ek.data(), p.e_kind = kind.data();
        p.e_obs = obs.data(), p.e_inv_sigma2 = w.data();
        p.n_links = (int32_t)links.size(), p.links = links.data();
        p.iterations = 10, p.large = 0, p.lambda_init = 1.0;
    }
    void edge(int point, int k, int kd)
    {
        ep.push_back(point), ek.push_back(k), kind.push_back((int8_t)kd), w.push_back(1.f);
        for (int i = 0; i < 3; i++) obs.push_back(0.0);
    }
};

osg_liba_link link(int prev, int cur, int downweight)
{
    osg_liba_link L{};
    L.prev = prev, L.cur = cur, L.huber = downweight, L.downweight = downweight;
    for (int i = 0; i < 15; i++) L.preint.C[16 * i] = 1e-4f * (float)(i + 1);
    L.preint.C[1] = L.preint.C[15] = 2e-5f;
    L.preint.dT = 0.1f;
    return L;
}

// KeyFrames 0, 1 free (1 with two cameras), 2 free without link or edge, 3, 4 fixed; 4 points
Window window()
{
    Window m;
    m.kf.resize(5);
    for (int k = 0; k < 5; k++) {
        m.kf[k] = osg_liba_keyframe{};
        m.kf[k].n_cams = k == 1 ? 2 : 1;
        m.kf[k].fixed = k >= 3;
        for (int i = 0; i < 3; i++) m.kf[k].state.Rwb[4 * i] = 1.0;
    }
    for (int q = 0; q < 4; q++) {
        m.depth.push_back(5.f + 3 * q);
        for (int i = 0; i < 3; i++) m.xw.push_back(q + 0.1 * i);
    }
    m.edge(0, 0, OSG_EDGE_MONO);   // 0
    m.edge(0, 1, OSG_EDGE_MONO);   // 1
    m.edge(0, 1, OSG_EDGE_BODY);   // 2: the same point and KeyFrame through the other camera
    m.edge(0, 3, OSG_EDGE_MONO);   // 3
    m.edge(1, 3, OSG_EDGE_STEREO); // 4: a point seen by fixed KeyFrames only
    m.edge(1, 4, OSG_EDGE_MONO);   // 5
    m.edge(2, 1, OSG_EDGE_MONO);   // 6: a point seen once
    m.edge(3, 1, OSG_EDGE_MONO);   // 7
    m.edge(3, 0, OSG_EDGE_MONO);   // 8: the later KeyFrame first
    m.links.push_back(link(1, 0, 0));
    m.links.push_back(link(3, 1, 1));
    m.bind();
    return m;
}

int fails = 0;
#define EXPECT(cond)                                                  \
    if (!(cond)) {                                                    \
        std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
        fails++;                                                      \
    }

void refusals()
{
    const char *why = nullptr;
    EXPECT(osgliba::check(nullptr, &why) == OSG_E_INVALID);
    {
        Window m = window();
        EXPECT(osgliba::check(&m.p, &why) == 0);
    }
#define REFUSED(mutation, text)                                        \
    {                                                                  \
        Window m = window();                                           \
        mutation;                                                      \
        why = "";                                                      \
        EXPECT(osgliba::check(&m.p, &why) == OSG_E_INVALID);           \
        EXPECT(std::string(why).find(text) != std::string::npos);      \
    }
    REFUSED(m.p.kf = nullptr, "null KeyFrame");
    REFUSED(m.p.xw = nullptr, "null point");
    REFUSED(m.p.track_depth = nullptr, "null point");
    REFUSED(m.p.e_kind = nullptr, "null edge");
    REFUSED(m.p.e_obs = nullptr, "null edge");
    REFUSED(m.p.links = nullptr, "null link");
    REFUSED(m.p.n_kf = -1, "negative");
    REFUSED(m.p.n_points = -1, "negative");
    REFUSED(m.p.n_edges = -1, "negative");
    REFUSED(m.p.n_links = -1, "negative");
    REFUSED(m.ep[2] = 4, "point index");
    REFUSED(m.ep[2] = -1, "point index");
    REFUSED(m.ek[2] = 5, "KeyFrame index");
    REFUSED(m.links[0].prev = 5, "link index");
    REFUSED(m.links[0].cur = -1, "link index");
    REFUSED(m.links[0].prev = 0, "itself");
    REFUSED(m.links[1].cur = 0, "cur of two");
    REFUSED(m.kind[0] = OSG_EDGE_BODY, "one-camera");
    REFUSED(m.kind[0] = 3, "unknown edge kind");
    REFUSED(m.kf[0].n_cams = 3, "n_cams");
    REFUSED(m.p.n_points = OSG_LIBA_MAX_POINTS + 1, "too many points");
    REFUSED(m.p.n_edges = OSG_LIBA_MAX_EDGES + 1, "too many edges");
    REFUSED(m.p.n_kf = OSG_LIBA_MAX_FREE_KF + OSG_LIBA_MAX_FIXED_KF + 1, "too many KeyFrames");
    REFUSED(m.p.iterations = OSG_LIBA_MAX_ITERATIONS + 1, "iterations");
    REFUSED(m.p.lambda_init = 0.0, "lambda_init");
    REFUSED(m.p.lambda_init = std::numeric_limits<double>::quiet_NaN(), "lambda_init");
    REFUSED(for (auto &k : m.kf) k.fixed = 1, "nothing free");
    {
        Window m = window();
        m.kf.resize(OSG_LIBA_MAX_FREE_KF + 3, m.kf[0]);  // 33 free, 2 fixed
        m.bind();
        why = "";
        EXPECT(osgliba::check(&m.p, &why) == OSG_E_INVALID && std::string(why).find("free KeyFrames") != std::string::npos);
        m.kf.assign(OSG_LIBA_MAX_FIXED_KF + 2, m.kf[3]);
        m.kf[0].fixed = 0;
        m.ek.assign(m.ek.size(), 0), m.kind.assign(m.kind.size(), OSG_EDGE_MONO), m.links.clear();
        m.bind();
        EXPECT(osgliba::check(&m.p, &why) == OSG_E_INVALID && std::string(why).find("fixed KeyFrames") != std::string::npos);
        m.kf.resize(257);  // 256 fixed KeyFrames must be accepted
        m.bind();
        EXPECT(osgliba::check(&m.p, &why) == 0);
    }
    {   // 4 097 edges of one point on one free KeyFrame: 4 097^2 pair entries, above the cap
        Window m = window();
        for (int i = 0; i < 4097; i++) m.edge(0, 0, OSG_EDGE_MONO);
        m.bind();
        why = "";
        EXPECT(osgliba::check(&m.p, &why) == OSG_E_INVALID && std::string(why).find("edge pairs") != std::string::npos);
        for (size_t i = m.ek.size() - 4097; i < m.ek.size(); i++) m.ek[i] = 3;  // on a fixed KeyFrame they make no pair
        EXPECT(osgliba::check(&m.p, &why) == 0);
    }
#undef REFUSED
}

void structure()
{
    Window m = window();
    osgliba::Structure s;
    EXPECT(osgliba::build_structure(m.p, s));
    EXPECT(s.n_free == 3);
    EXPECT(osgliba::count_pairs(m.p) == 11 && (int64_t)s.pairs.size() == 22);
    EXPECT(s.free_idx == (std::vector<int32_t>{0, 1, 2, -1, -1}));
    using namespace osgliba;
    EXPECT(s.flags[0] == (KF_LINKED | KF_POSE) && s.flags[1] == (KF_LINKED | KF_POSE));
    EXPECT(s.flags[2] == 0);                         // neither a link nor an edge: nothing of it is active
    EXPECT(s.flags[3] == (KF_LINKED | KF_POSE) && s.flags[4] == KF_POSE);
    EXPECT(s.pt_beg == (std::vector<int32_t>{0, 4, 6, 7, 9}));
    EXPECT(s.pt_edges == (std::vector<int32_t>{0, 1, 2, 3, 4, 5, 6, 7, 8}));
    EXPECT(s.kf_beg == (std::vector<int32_t>{0, 2, 6, 6, 8, 9}));
    EXPECT(s.kf_edges == (std::vector<int32_t>{0, 8, 1, 2, 6, 7, 3, 4, 5}));
    // blocks (0, 0), (0, 1), (1, 1) in that order
    EXPECT(s.blocks.size() == 3);
    if (s.blocks.size() == 3) {
        EXPECT(s.blocks[0].fi == 0 && s.blocks[0].fj == 0 && s.blocks[0].end - s.blocks[0].beg == 2);
        EXPECT(s.blocks[1].fi == 0 && s.blocks[1].fj == 1 && s.blocks[1].end - s.blocks[1].beg == 3);
        EXPECT(s.blocks[2].fi == 1 && s.blocks[2].fj == 1 && s.blocks[2].end - s.blocks[2].beg == 6);
        EXPECT(s.pairs == (std::vector<int32_t>{0, 0, 8, 8,             // (0, 0)
                                                0, 1, 0, 2, 8, 7,       // (0, 1): a on KeyFrame 0, b on KeyFrame 1
                                                1, 1, 1, 2, 2, 1, 2, 2, 6, 6, 7, 7}));
    }
    // a link between two fixed KeyFrames is no edge of the graph
    m.links.push_back(link(3, 4, 0));
    m.bind();
    EXPECT(osgliba::check(&m.p, nullptr) == 0);
    EXPECT(osgliba::build_structure(m.p, s) && s.flags[4] == KF_POSE);
    EXPECT(osgliba::workspace_doubles(5, 3, 4, 9, 2) > 2 * 45 * 45);
}

void link_block()
{
    osgliba::LinkDev a, b;
    osgliba::pack_link(link(1, 0, 0), a);
    osgliba::pack_link(link(1, 0, 1), b);
    EXPECT(a.huber == 0 && b.huber == 1 && a.dT == 0.1f);
    for (int i = 0; i < 81; i++) EXPECT(b.info9[i] == a.info9[i] * 1e-2);
    EXPECT(a.info9[80] > 0 && a.info_g[0] > 0 && a.info_a[8] > 0);
    for (int i = 0; i < 9; i++) EXPECT(a.info_g[i] == b.info_g[i] && a.info_a[i] == b.info_a[i]);
}

void failed_rule()
{
    using osgliba::failed_rule;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    EXPECT(failed_rule(10.0, 19.0, 0) == 0);
    EXPECT(failed_rule(10.0, 21.0, 0) == 1);
    EXPECT(failed_rule(10.0, 21.0, 1) == 0);
    EXPECT(failed_rule(nan, 1.0, 0) == 1 && failed_rule(1.0, nan, 0) == 1 && failed_rule(nan, nan, 1) == 0);
    // decided on the float casts: 2 * 1 < 2 + 1e-9 in double, equal as floats
    EXPECT(failed_rule(1.0, 2.0 + 1e-9, 0) == 0);
    // 2 * err overflows to +inf as a float and is not below a finite err_end
    EXPECT(failed_rule(3e38, 3.3e38, 0) == 0);
    // an err_end beyond the float range is +inf
    EXPECT(failed_rule(1.0, 1e39, 0) == 1);
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc < 2 || std::string(argv[1]) != "check") {
        std::printf("usage: localinertialba_host check\n");
        return 2;
    }
    refusals();
    structure();
    link_block();
    failed_rule();
    std::printf(fails ? "%d failed\n" : "ok\n", fails);
    return fails ? 1 : 0;
}
