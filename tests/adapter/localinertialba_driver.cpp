// localinertialba_driver.cpp — Optimizer::LocalInertialBA through the ORB-SLAM3-side adapter on mock objects
// (test-only; tests/test_adapter_localinertialba.py).
//   gather <in> <out>   LocalInertialBAGather alone (host code, no device): the window, the marks and the problem
//   run <in> <out>      the whole call and the write-back: KeyFrames, MapPoints, erasures and the map afterwards
// Input: per KeyFrame "kf.id", "kf.prev" (index or -1), "kf.bad", "kf.map" (0: the current map), "kf.imu", "kf.nleft",
// "kf.raw" (osg_liba_keyframe bytes), "kf.sigma" (8 per KeyFrame), "kf<i>.un", ".uright", ".right", ".matches" (point
// index or -1); "link.cur" and "link.raw" (osg_liba_link bytes) of every preintegration; "mp.pos", "mp.depth",
// "mp.bad"; the observations "ob.mp", "ob.kf", "ob.left", "ob.right"; "noise"; "args" = KeyFramesInMap, bLarge, bRecInit.
#include "driver_common.h"
#include "mock_localinertialba.h"

using mockliba::Hooks;
using KF = mockliba::KeyFrame;
using MP = mockliba::MapPoint;

int main(int argc, char **argv)
{
    if (argc != 4) {
        std::fprintf(stderr, "usage: localinertialba_driver gather|run <in> <out>\n");
        return 2;
    }
    const std::string mode = argv[1];
    const Arrays in = read_arrays(argv[2]);
    const float *noise = get(in, "noise").p<float>();
    const Arr &ids = get(in, "kf.id");
    const int n = (int)ids.n;
    const int32_t *prev = get(in, "kf.prev").p<int32_t>(), *bad = get(in, "kf.bad").p<int32_t>();
    const int32_t *map_of = get(in, "kf.map").p<int32_t>(), *has_imu = get(in, "kf.imu").p<int32_t>();
    const int32_t *nleft = get(in, "kf.nleft").p<int32_t>();
    const int32_t *args = get(in, "args").p<int32_t>();
    mockliba::Map maps[2];
    maps[0].n_kfs = args[0];
    const Arr &mpos = get(in, "mp.pos");
    const int np = (int)(mpos.n / 3);
    std::vector<MP> mps(np);
    for (int q = 0; q < np; q++) {
        std::memcpy(mps[q].pos, mpos.p<float>() + 3 * q, 12);
        mps[q].mTrackDepth = get(in, "mp.depth").p<float>()[q];
        mps[q].bad = get(in, "mp.bad").p<int32_t>()[q] != 0;
    }
    std::vector<KF> kfs(n);
    for (int i = 0; i < n; i++) {
        KF &K = kfs[i];
        const std::string pre = "kf" + std::to_string(i);
        K.mnId = (unsigned long)ids.p<int32_t>()[i];
        K.mPrevKF = prev[i] >= 0 ? &kfs[prev[i]] : nullptr;
        K.bad = bad[i] != 0, K.bImu = has_imu[i] != 0, K.map = &maps[map_of[i]], K.NLeft = nleft[i];
        std::memcpy(&K.raw, get(in, "kf.raw").p<uint8_t>() + sizeof K.raw * i, sizeof K.raw);
        K.mpCamera2 = K.raw.n_cams == 2;
        const float *sg = get(in, "kf.sigma").p<float>() + 8 * i;
        K.mvInvLevelSigma2.assign(sg, sg + 8);
        const Arr &un = get(in, pre + ".un"), &ur = get(in, pre + ".uright"), &rt = get(in, pre + ".right");
        K.un.assign(un.p<float>(), un.p<float>() + un.n);
        K.mvuRight.assign(ur.p<float>(), ur.p<float>() + ur.n);
        K.right.assign(rt.p<float>(), rt.p<float>() + rt.n);
        const Arr &mt = get(in, pre + ".matches");
        for (size_t j = 0; j < mt.n; j++) K.matches.push_back(mt.p<int32_t>()[j] >= 0 ? &mps[mt.p<int32_t>()[j]] : nullptr);
    }
    const Arr &lc = get(in, "link.cur");
    for (size_t l = 0; l < lc.n; l++) {
        osg_liba_link L;
        std::memcpy(&L, get(in, "link.raw").p<uint8_t>() + sizeof L * l, sizeof L);
        auto *p = new mockliba::Preintegrated(L.preint.b, noise, noise + 6);
        p->st.pre = L.preint;
        kfs[lc.p<int32_t>()[l]].mpImuPreintegrated = p;
    }
    const Arr &om = get(in, "ob.mp");
    for (size_t j = 0; j < om.n; j++)
        mps[om.p<int32_t>()[j]].obs[&kfs[get(in, "ob.kf").p<int32_t>()[j]]] =
            std::make_tuple((int)get(in, "ob.left").p<int32_t>()[j], (int)get(in, "ob.right").p<int32_t>()[j]);
    const bool bLarge = args[1] != 0, bRecInit = args[2] != 0;
    auto kf_index = [&](const std::vector<KF *> &v) {
        std::vector<int32_t> o;
        for (KF *k : v) o.push_back((int32_t)(k - kfs.data()));
        return o;
    };
    auto marks = [&]() {
        std::vector<int32_t> m;
        for (const KF &K : kfs) m.push_back((int32_t)K.mnBALocalForKF), m.push_back((int32_t)K.mnBAFixedForKF);
        return m;
    };
    Arrays out;
    if (mode == "gather") {
        osg_orbslam3::LocalInertialBAGather<Hooks, KF, MP> g;
        g.build(&kfs[0], bLarge, bRecInit);
        std::vector<int32_t> pts, fixed, links;
        std::vector<float> bu;
        for (MP *p : g.points) pts.push_back((int32_t)(p - mps.data()));
        for (const auto &k : g.kf) fixed.push_back(k.fixed);
        for (const auto &L : g.links) {
            links.push_back(L.prev), links.push_back(L.cur), links.push_back(L.huber), links.push_back(L.downweight);
            const float *f = kfs[(size_t)(g.opt_kfs[L.cur] - kfs.data())].mpImuPreintegrated->bu;
            bu.insert(bu.end(), f, f + 6);
        }
        std::vector<uint8_t> kind(g.kind.begin(), g.kind.end());
        out["opt"] = make('i', kf_index(g.opt_kfs)), out["fixed"] = make('i', kf_index(g.fixed_kfs));
        out["points"] = make('i', pts), out["kf_fixed"] = make('i', fixed), out["links"] = make('i', links);
        out["links_bu"] = make('f', bu);
        out["ep"] = make('i', g.ep), out["ek"] = make('i', g.ek), out["kind"] = make('b', kind);
        out["obs"] = make('d', g.obs), out["w"] = make('f', g.w), out["xw"] = make('d', g.xw);
        out["depth"] = make('f', g.depth), out["marks"] = make('i', marks());
        out["options"] = make('d', std::vector<double>{(double)g.p.iterations, (double)g.p.large, g.p.lambda_init});
        out["check"] = make('i', std::vector<int32_t>{osg_local_inertial_ba_check(&g.p)});
    } else if (mode == "run") {
        auto r = osg_orbslam3::local_inertial_ba<Hooks, KF, MP>(&kfs[0], bLarge, bRecInit);
        if (osg_orbslam3::thread_ctx() == nullptr) {
            std::fprintf(stderr, "no device context\n");
            return 3;
        }
        osg_orbslam3::apply_local_inertial_ba<Hooks>(r, &maps[0]);
        std::vector<float> pose, vel, bias, pos;
        std::vector<int32_t> writes, pwrites, er;
        for (const KF &K : kfs) {
            pose.insert(pose.end(), K.pose_R, K.pose_R + 9), pose.insert(pose.end(), K.pose_t, K.pose_t + 3);
            vel.insert(vel.end(), K.vel, K.vel + 3), bias.insert(bias.end(), K.bias, K.bias + 6);
            writes.push_back(K.pose_writes), writes.push_back(K.velocity_writes), writes.push_back(K.bias_writes);
        }
        for (const MP &p : mps) {
            pos.insert(pos.end(), p.pos, p.pos + 3);
            pwrites.push_back(p.pos_writes), pwrites.push_back(p.normal_updates);
        }
        for (const auto &e : mockliba::erased()) er.push_back(e.first), er.push_back((int32_t)(e.second - mps.data()));
        out["ok"] = make('i', std::vector<int32_t>{r.ok, r.failed, maps[0].change_index});
        out["opt"] = make('i', kf_index(r.opt_kfs)), out["fixed"] = make('i', kf_index(r.fixed_kfs));
        out["kf.pose"] = make('f', pose), out["kf.v"] = make('f', vel), out["kf.bias"] = make('f', bias);
        out["kf.writes"] = make('i', writes), out["mp.pos"] = make('f', pos), out["mp.writes"] = make('i', pwrites);
        out["erased"] = make('i', er), out["marks"] = make('i', marks());
    } else {
        std::fprintf(stderr, "unknown mode %s\n", mode.c_str());
        return 2;
    }
    for (auto &K : kfs) delete K.mpImuPreintegrated;
    write_arrays(argv[3], out);
    return 0;
}
