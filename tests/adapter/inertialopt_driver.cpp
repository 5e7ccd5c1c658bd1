// inertialopt_driver.cpp — the three overloads of Optimizer::InertialOptimization through the ORB-SLAM3-side adapter
// on mock objects (test-only; tests/test_adapter_inertialopt.py).
//   gather <in> <out>            InertialGather alone (host code, no device): the problem as the library would get it
//   init|bias|scale <in> <out>   the whole call: the reference arguments and the KeyFrames afterwards
// Input: "kf.id" (mnId), "kf.prev" (index into the list or -1), "kf.bad", "kf.has" (a preintegration), "kf.Rwb",
// "kf.twb", "kf.v", "kf.bias" per KeyFrame in vpKFs order; "kf<i>.state" / ".bu" / ".meas" of every preintegration;
// "noise"; "max_id"; "args" = Rwg (9), scale, priorG, priorA, bMono, bFixedVel.
#include "driver_common.h"
#include "mock_inertialopt.h"

namespace {

using mockio::Hooks;
using KF = mockio::KeyFrame;
using mockio::Preintegrated;

std::vector<float> state_row(const Preintegrated &p)
{
    const float *f = reinterpret_cast<const float *>(&p.st);
    std::vector<float> v(f, f + sizeof p.st / sizeof(float));
    v.insert(v.end(), p.bu, p.bu + 6), v.insert(v.end(), p.db, p.db + 6);
    return v;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc != 4) {
        std::fprintf(stderr, "usage: inertialopt_driver gather|init|bias|scale <in> <out>\n");
        return 2;
    }
    const std::string mode = argv[1];
    const Arrays in = read_arrays(argv[2]);
    const float *noise = get(in, "noise").p<float>();
    const Arr &ids = get(in, "kf.id");
    const int n = (int)ids.n;
    const int32_t *prev = get(in, "kf.prev").p<int32_t>(), *bad = get(in, "kf.bad").p<int32_t>();
    const int32_t *has_pre = get(in, "kf.has").p<int32_t>();
    std::vector<KF> kfs(n);
    std::vector<KF *> vp;
    for (int i = 0; i < n; i++) {
        KF &K = kfs[i];
        K.mnId = (unsigned long)ids.p<int32_t>()[i];
        K.mPrevKF = prev[i] >= 0 ? &kfs[prev[i]] : nullptr;
        K.bad = bad[i] != 0;
        std::memcpy(K.Rwb, get(in, "kf.Rwb").p<float>() + 9 * i, 36);
        std::memcpy(K.twb, get(in, "kf.twb").p<float>() + 3 * i, 12);
        std::memcpy(K.vel, get(in, "kf.v").p<float>() + 3 * i, 12);
        std::memcpy(K.bias, get(in, "kf.bias").p<float>() + 6 * i, 24);
        if (has_pre[i]) {
            const float zero[6] = {};
            const std::string pre = "kf" + std::to_string(i);
            auto *p = new Preintegrated(zero, noise, noise + 6);
            std::memcpy(&p->st, get(in, pre + ".state").p<float>(), sizeof p->st);
            p->SetNewBias(get(in, pre + ".bu").p<float>());
            const Arr &m = get(in, pre + ".meas");
            p->meas.assign(m.p<float>(), m.p<float>() + m.n);
            K.mpImuPreintegrated = p;
        }
        vp.push_back(&K);
    }
    const unsigned long max_id = (unsigned long)get(in, "max_id").p<int32_t>()[0];
    const double *args = get(in, "args").p<double>();
    double Rwg[9], scale = args[9], bg[3] = {-7, -7, -7}, ba[3] = {-7, -7, -7};
    std::memcpy(Rwg, args, sizeof Rwg);
    const float priorG = (float)args[10], priorA = (float)args[11];
    const bool bMono = args[12] != 0, bFixedVel = args[13] != 0;
    Arrays out;
    if (mode == "gather") {
        osg_orbslam3::InertialOptions o;
        osg_orbslam3::InertialGather<Hooks, KF> g;
        g.assign(vp, max_id, o, Rwg, scale);
        std::vector<int32_t> who;
        for (auto *k : g.kfs) who.push_back((int32_t)(k - kfs.data()));
        std::vector<float> pre;
        for (const auto &q : g.pre) {
            const float *f = reinterpret_cast<const float *>(&q);
            pre.insert(pre.end(), f, f + sizeof q / sizeof(float));
        }
        out["kfs"] = make('i', who);
        out["Rwb"] = make('d', g.Rwb), out["twb"] = make('d', g.twb), out["v"] = make('d', g.v);
        out["prev"] = make('i', g.prev), out["cur"] = make('i', g.cur);
        out["pre"] = make('f', pre);
        out["start"] = make('d', std::vector<double>{g.p.bg[0], g.p.bg[1], g.p.bg[2], g.p.ba[0], g.p.ba[1], g.p.ba[2]});
        out["check"] = make('i', std::vector<int32_t>{osg_inertial_check(&g.p)});
    } else {
        bool ok;
        if (mode == "init")
            ok = osg_orbslam3::inertial_optimization_init<Hooks>(vp, max_id, Rwg, scale, bg, ba, bMono, bFixedVel, priorG,
                                                                 priorA);
        else if (mode == "bias")
            ok = osg_orbslam3::inertial_optimization_bias<Hooks>(vp, max_id, bg, ba, priorG, priorA);
        else if (mode == "scale")
            ok = osg_orbslam3::inertial_optimization_scale<Hooks>(vp, max_id, Rwg, scale);
        else {
            std::fprintf(stderr, "unknown mode %s\n", mode.c_str());
            return 2;
        }
        if (osg_orbslam3::thread_ctx() == nullptr) {
            std::fprintf(stderr, "no device context\n");
            return 3;
        }
        std::vector<double> ref(Rwg, Rwg + 9);
        ref.push_back(scale);
        ref.insert(ref.end(), bg, bg + 3), ref.insert(ref.end(), ba, ba + 3);
        out["ok"] = make('i', std::vector<int32_t>{ok ? 1 : 0});
        out["ref"] = make('d', ref);
        std::vector<float> vel, bias;
        std::vector<int32_t> writes;
        for (int i = 0; i < n; i++) {
            vel.insert(vel.end(), kfs[i].vel, kfs[i].vel + 3);
            bias.insert(bias.end(), kfs[i].bias, kfs[i].bias + 6);
            writes.push_back(kfs[i].velocity_writes), writes.push_back(kfs[i].bias_writes);
            if (kfs[i].mpImuPreintegrated)
                out["kf" + std::to_string(i) + ".state"] = make('f', state_row(*kfs[i].mpImuPreintegrated));
        }
        out["kf.v"] = make('f', vel), out["kf.bias"] = make('f', bias), out["kf.writes"] = make('i', writes);
    }
    for (auto &K : kfs) delete K.mpImuPreintegrated;
    write_arrays(argv[3], out);
    return 0;
}
