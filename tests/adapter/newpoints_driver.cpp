// newpoints_driver.cpp — LocalMapping::CreateNewMapPoints through the ORB-SLAM3-side adapter on mock objects
// (test-only; tests/test_adapter_newpoints.py).  Builds a current KeyFrame ("K0.") and a pool of other KeyFrames
// ("K1." ...) with a covisibility order and an mPrevKF chain from an array file, then
//   gather <in> <out>   builds the neighbour list and NewPointsGather alone (pure host code, no device) and dumps
//                       what they hold;
//   run    <in> <out>   LocalMappingMock::CreateNewMapPoints (the body of adapters/orbslam3/LocalMapping_osg.cc)
//                       and dumps the map it leaves.
#include "driver_common.h"
#include "mock_localmapping.h"

namespace {

using Gather = osg_orbslam3::NewPointsGather<LmHooks, LmKeyFrame>;

template <class T>
void raw(const Arr &a, T &dst)
{
    if (a.b.size() != sizeof(T)) {
        std::fprintf(stderr, "structure size %zu, expected %zu\n", a.b.size(), sizeof(T));
        std::exit(2);
    }
    std::memcpy(&dst, a.b.data(), sizeof(T));
}

void build_kf(const Arrays &in, const std::string &pre, LmKeyFrame &K, Camera cams[2], std::vector<std::unique_ptr<MapPoint>> &pool)
{
    build_triang_kf(in, pre, K, pool);
    raw(get(in, pre + "geometry"), K.geometry);
    raw(get(in, pre + "pair_geometry"), K.pair_geometry);
    const osg_np_kf &g = K.geometry;
    K.fx = g.fx, K.fy = g.fy, K.cx = g.cx, K.cy = g.cy, K.invfx = g.invfx, K.invfy = g.invfy, K.mb = g.mb, K.mbf = g.mbf;
    K.mfScaleFactor = get(in, pre + "scale").p<float>()[1];
    K.mpCamera = &cams[0];
    if (K.mpCamera2) K.mpCamera2 = &cams[1];
    if (has(in, pre + "depth")) {
        const Arr &d = get(in, pre + "depth"), &kx = get(in, pre + "keys_x"), &ky = get(in, pre + "keys_y");
        K.mvDepth.assign(d.p<float>(), d.p<float>() + d.n);
        for (int i = 0; i < K.N; i++) {  // mvKeys differs from mvKeysUn
            K.mvKeys[i].pt.x = kx.p<float>()[i];
            K.mvKeys[i].pt.y = ky.p<float>()[i];
        }
    }
    const Arr &sd = get(in, pre + "scene_depths");
    K.scene_depths.assign(sd.p<float>(), sd.p<float>() + sd.n);
}

void dump_side(Arrays &out, const std::string &pre, const osg_kf_side &s, osg_np_kf g)
{
    out[pre + "head"] = make('i', std::vector<int32_t>{s.n, s.nleft, s.two_cam, s.n_levels, s.u_right != nullptr, g.depth != nullptr});
    out[pre + "kp_x"] = make('f', std::vector<float>(s.kp_x, s.kp_x + s.n));
    out[pre + "kp_y"] = make('f', std::vector<float>(s.kp_y, s.kp_y + s.n));
    out[pre + "kp_octave"] = make('i', std::vector<int32_t>(s.kp_octave, s.kp_octave + s.n));
    out[pre + "has_mp"] = make('b', std::vector<uint8_t>(s.has_mp, s.has_mp + s.n));
    out[pre + "desc"] = make('b', std::vector<uint8_t>(s.desc, s.desc + 32 * (size_t)s.n));
    if (s.u_right) out[pre + "u_right"] = make('f', std::vector<float>(s.u_right, s.u_right + s.n));
    if (g.depth) {
        out[pre + "depth"] = make('f', std::vector<float>(g.depth, g.depth + s.n));
        out[pre + "keys_x"] = make('f', std::vector<float>(g.keys_x, g.keys_x + s.n));
        out[pre + "keys_y"] = make('f', std::vector<float>(g.keys_y, g.keys_y + s.n));
    }
    g.depth = g.keys_x = g.keys_y = nullptr;
    out[pre + "geometry"] = make('b', std::vector<uint8_t>((const uint8_t *)&g, (const uint8_t *)&g + sizeof g));
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc != 4) {
        std::fprintf(stderr, "usage: newpoints_driver gather|run <in> <out>\n");
        return 2;
    }
    const std::string mode = argv[1];
    const Arrays in = read_arrays(argv[2]);
    const int32_t *pr = get(in, "params").p<int32_t>();  // KeyFrames, monocular, inertial, far, new keyframes, coarse
    const int nkf = pr[0];
    std::vector<std::unique_ptr<LmKeyFrame>> kfs;
    std::vector<std::unique_ptr<MapPoint>> old_points;
    Camera cams[2];
    for (int k = 0; k < nkf; k++) {
        kfs.emplace_back(new LmKeyFrame());
        kfs.back()->mnId = k;
        build_kf(in, "K" + std::to_string(k) + ".", *kfs.back(), cams, old_points);
    }
    const Arr &cov = get(in, "covisible"), &prev = get(in, "prev");
    for (size_t j = 0; j < cov.n; j++) kfs[0]->covisible.push_back(kfs[cov.p<int32_t>()[j]].get());
    for (int k = 0; k < nkf; k++)
        if (prev.p<int32_t>()[k] >= 0) kfs[k]->mPrevKF = kfs[prev.p<int32_t>()[k]].get();
    LocalMappingMock lm;
    lm.mpCurrentKeyFrame = kfs[0].get();
    lm.mbMonocular = pr[1], lm.mbInertial = pr[2], lm.mbFarPoints = pr[3], lm.new_keyframes = pr[4], lm.coarse = pr[5];
    lm.mThFarPoints = get(in, "th_far").p<float>()[0];
    Arrays out;
    if (mode == "gather") {
        const std::vector<LmKeyFrame *> neigh = Gather::neighbours(kfs[0].get(), lm.mbMonocular, lm.mbInertial);
        Gather G(kfs[0].get(), neigh, lm.mbMonocular, lm.mbInertial, lm.coarse, lm.mbFarPoints, lm.mThFarPoints);
        std::vector<int32_t> ids;
        for (LmKeyFrame *k : neigh) ids.push_back((int32_t)k->mnId);
        out["neighbours"] = make('i', ids);
        const osg_newpoints_problem &p = G.problem;
        out["flags"] = make('i', std::vector<int32_t>{p.n_neigh, p.monocular, p.inertial, p.coarse, p.far_points});
        out["floats"] = make('f', std::vector<float>{p.th_far_points, p.ratio_factor});
        dump_side(out, "S0.", p.kf1, p.g1);
        for (int b = 0; b < p.n_neigh; b++) {
            dump_side(out, "S" + std::to_string(b + 1) + ".", p.kf2[b], p.g2[b]);
            const uint8_t *g = (const uint8_t *)&p.geom[b];
            out["S" + std::to_string(b + 1) + ".pair_geometry"] = make('b', std::vector<uint8_t>(g, g + sizeof(osg_triang_geom)));
        }
    } else if (mode == "run") {
        const int rc = lm.CreateNewMapPoints();
        if (osg_orbslam3::thread_ctx() == nullptr) {
            std::fprintf(stderr, "no device context\n");
            return 3;
        }
        std::vector<int32_t> pts, recent, atlas;  // per point: KF2 id, idx1, idx2, n_distinctive, n_update, observations
        std::vector<float> x3d;
        for (const auto &p : lm.pool) {
            const bool order = p->added.size() == 2 && p->added[0].first == kfs[0].get() && p->ref_kf == kfs[0].get();
            for (int v : {(int)p->added.back().first->mnId, p->added.front().second, p->added.back().second, p->n_distinctive,
                          p->n_update, (int)p->obs.size(), (int)order})
                pts.push_back(v);
            x3d.insert(x3d.end(), p->x3d, p->x3d + 3);
        }
        for (LmMapPoint *p : lm.mlpRecentAddedMapPoints) recent.push_back((int32_t)p->mnId);
        for (LmMapPoint *p : lm.atlas.points) atlas.push_back((int32_t)p->mnId);
        out["rc"] = make('i', std::vector<int32_t>{rc, lm.n_checks});
        out["points"] = make('i', pts);
        out["x3d"] = make('f', x3d);
        out["recent"] = make('i', recent);
        out["atlas"] = make('i', atlas);
        for (int k = 0; k < nkf; k++) {  // slot -> new MapPoint id, -2 an old MapPoint, -1 none
            std::vector<int32_t> slots(kfs[k]->N, -1);
            for (int i = 0; i < kfs[k]->N; i++)
                if (MapPoint *q = kfs[k]->mvpMapPoints[i]) {
                    slots[i] = -2;
                    for (const auto &p : lm.pool)
                        if (p.get() == q) slots[i] = (int32_t)p->mnId;
                }
            out["slots" + std::to_string(k)] = make('i', slots);
        }
    } else {
        std::fprintf(stderr, "unknown mode %s\n", mode.c_str());
        return 2;
    }
    write_arrays(argv[3], out);
    return 0;
}
