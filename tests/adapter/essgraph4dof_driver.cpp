// essgraph4dof_driver.cpp — OptimizeEssentialGraph4DoF through the ORB-SLAM3-side adapter on the mock objects of
// mock_essgraph4dof.h (test-only; tests/test_adapter_essgraph4dof.py).  Builds a map from an array file, then
//   gather   <in> <out>   runs the graph build alone (pure host code, no device) and dumps the problem;
//   optimize <in> <out>   runs gather -> ABI -> write-back and dumps what the map's objects received.
// KeyFrames live in one vector, so pointer order (the order of LoopConnections and of the KeyFrameAndPose
// maps in the reference) is index order.
#include "driver_common.h"
#include "mock_essgraph4dof.h"

namespace eg = mockeg4;

namespace {

// Optimizer::OptimizeEssentialGraph4DoF with the reference's parameter list, the body Optimizer_osg.cc gives it
int OptimizeEssentialGraph4DoF(eg::Map *pMap, eg::KeyFrame *pLoopKF, eg::KeyFrame *pCurKF,
                               const eg::KeyFrameAndPose &NonCorrectedSim3, const eg::KeyFrameAndPose &CorrectedSim3,
                               const eg::LoopConnections &LoopConnections)
{
    return osg_orbslam3::optimize_essential_graph_4dof<eg::Hooks>(pMap, pLoopKF, pCurKF, NonCorrectedSim3, CorrectedSim3,
                                                                  LoopConnections);
}

eg::Sim3 sim3_of(const double *p)
{
    eg::Sim3 S;
    std::memcpy(S.r, p, 32);
    std::memcpy(S.t, p + 4, 24);
    S.s = p[7];
    return S;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc != 4) {
        std::fprintf(stderr, "usage: essgraph4dof_driver gather|optimize <in> <out>\n");
        return 2;
    }
    const std::string mode = argv[1];
    const Arrays in = read_arrays(argv[2]);
    const Arr &ids = get(in, "kf.id");
    const int nk = (int)ids.n;
    std::vector<eg::KeyFrame> kf(nk);
    eg::Map map;
    for (int i = 0; i < nk; i++) {
        eg::KeyFrame &k = kf[i];
        k.mnId = (unsigned long)ids.p<int32_t>()[i];
        k.bad = get(in, "kf.bad").p<uint8_t>()[i] != 0;
        std::memcpy(k.pose, get(in, "kf.pose").p<double>() + 7 * i, 56);
        std::memcpy(k.imu_row, get(in, "kf.imu_row").p<double>() + 36 * i, sizeof k.imu_row);
        const int par = get(in, "kf.parent").p<int32_t>()[i], prev = get(in, "kf.prev").p<int32_t>()[i];
        const int next = get(in, "kf.next").p<int32_t>()[i];
        if (par >= 0) kf[par].children.insert(&k);
        if (prev >= 0) k.mPrevKF = &kf[prev];
        if (next >= 0) k.mNextKF = &kf[next];
        if (get(in, "kf.in_map").p<uint8_t>()[i]) map.kfs.push_back(&k);
    }
    const Arr &le = get(in, "loop_edges");  // pairs (a, b): b is in a's GetLoopEdges()
    for (size_t e = 0; e < le.n / 2; e++) kf[le.p<int32_t>()[2 * e]].loop_edges.insert(&kf[le.p<int32_t>()[2 * e + 1]]);
    const Arr &cv = get(in, "covis");       // triples (a, b, weight), a's list by decreasing weight
    for (size_t e = 0; e < cv.n / 3; e++)
        kf[cv.p<int32_t>()[3 * e]].covis.emplace_back(&kf[cv.p<int32_t>()[3 * e + 1]], cv.p<int32_t>()[3 * e + 2]);
    eg::KeyFrameAndPose corrected, non_corrected;
    const Arr &ck = get(in, "corr.kf"), &nck = get(in, "noncorr.kf");
    for (size_t e = 0; e < ck.n; e++) corrected[&kf[ck.p<int32_t>()[e]]] = sim3_of(get(in, "corr.sim3").p<double>() + 8 * e);
    for (size_t e = 0; e < nck.n; e++)
        non_corrected[&kf[nck.p<int32_t>()[e]]] = sim3_of(get(in, "noncorr.sim3").p<double>() + 8 * e);
    eg::LoopConnections conn;
    const Arr &cn = get(in, "conn");        // pairs (a, b): b is in LoopConnections[a]
    for (size_t e = 0; e < cn.n / 2; e++) conn[&kf[cn.p<int32_t>()[2 * e]]].insert(&kf[cn.p<int32_t>()[2 * e + 1]]);
    const int32_t *par = get(in, "params").p<int32_t>();  // cur, loop, max id
    eg::KeyFrame *pCurKF = &kf[par[0]], *pLoopKF = &kf[par[1]];
    map.max_kf_id = (unsigned long)par[2];
    const Arr &mpos = get(in, "mp.pos");
    const int nm = (int)(mpos.n / 3);
    std::vector<eg::MapPoint> mp(nm);
    for (int j = 0; j < nm; j++) {
        std::memcpy(mp[j].pos, mpos.p<float>() + 3 * j, 12);
        mp[j].bad = get(in, "mp.bad").p<uint8_t>()[j] != 0;
        mp[j].ref = &kf[get(in, "mp.ref").p<int32_t>()[j]];
        map.mps.push_back(&mp[j]);
    }
    Arrays out;
    if (mode == "gather") {
        osg_orbslam3::EssentialGraph4DoFGather<eg::Hooks, eg::Map, eg::KeyFrame, eg::MapPoint> g;
        g.assign(&map, pLoopKF, pCurKF, non_corrected, corrected, conn);
        std::vector<int32_t> vid;
        for (auto *k : g.vertex_kf) vid.push_back((int32_t)k->mnId);
        out["vertex_id"] = make('i', vid);
        out["index_of_id"] = make('i', g.index_of_id);
        out["pose"] = make('d', g.pose);
        out["sim3_before"] = make('d', g.sim3_before);
        out["fixed"] = make('b', g.fixed);
        out["e_v0"] = make('i', g.e_v0);
        out["e_v1"] = make('i', g.e_v1);
        out["e_meas"] = make('d', g.e_meas);
        out["scalars"] = make('i', std::vector<int32_t>{g.p.n_vertices, g.p.n_edges, g.p.max_iterations, g.n_dropped});
        out["info_lambda"] = make('d', std::vector<double>{g.p.info_diag[0], g.p.info_diag[1], g.p.info_diag[2], g.p.info_diag[3],
                                                           g.p.info_diag[4], g.p.info_diag[5], g.p.lambda_init});
        std::vector<eg::MapPoint *> mps;
        std::vector<float> Xw;
        std::vector<int32_t> ref;
        osg_orbslam3::essential_graph_4dof_points<eg::Hooks>(g, mps, Xw, ref);
        std::vector<int32_t> which;
        for (auto *m : mps) which.push_back((int32_t)(m - mp.data()));
        out["point_index"] = make('i', which);
        out["point_ref"] = make('i', ref);
        out["point_xw"] = make('f', Xw);
    } else if (mode == "optimize") {
        const int rc = OptimizeEssentialGraph4DoF(&map, pLoopKF, pCurKF, non_corrected, corrected, conn);
        if (osg_orbslam3::thread_ctx() == nullptr) {
            std::fprintf(stderr, "no device context\n");
            return 3;
        }
        std::vector<int32_t> n_set(nk), n_upd(nm), n_pos(nm);
        std::vector<float> q(4 * (size_t)nk), t(3 * (size_t)nk), pos(3 * (size_t)nm);
        for (int i = 0; i < nk; i++) {
            n_set[i] = kf[i].n_set_pose;
            std::memcpy(&q[4 * (size_t)i], kf[i].set_q, 16);
            std::memcpy(&t[3 * (size_t)i], kf[i].set_t, 12);
        }
        for (int j = 0; j < nm; j++) {
            n_upd[j] = mp[j].n_update;
            n_pos[j] = mp[j].n_set_pos;
            std::memcpy(&pos[3 * (size_t)j], mp[j].pos, 12);
        }
        out["ret"] = make('i', std::vector<int32_t>{rc, map.change_index, map.locked_at_change ? 1 : 0});
        out["kf.n_set_pose"] = make('i', n_set);
        out["kf.set_q"] = make('f', q);
        out["kf.set_t"] = make('f', t);
        out["mp.n_update"] = make('i', n_upd);
        out["mp.n_set_pos"] = make('i', n_pos);
        out["mp.pos"] = make('f', pos);
    } else {
        std::fprintf(stderr, "unknown mode %s\n", mode.c_str());
        return 2;
    }
    write_arrays(argv[3], out);
    return 0;
}
