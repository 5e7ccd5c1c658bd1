// poseinertial_driver.cpp — PoseInertialOptimizationLastKeyFrame / LastFrame through the ORB-SLAM3-side adapter on
// mock objects (test-only; tests/test_adapter_poseinertial.py).  Builds the frame, its previous KeyFrame or frame,
// the preintegrations and the prior from an array file, then
//   gather   <in> <out>   runs the gather alone (pure host code, no device) and dumps the problem;
//   optimize <in> <out>   runs gather -> osg_pose_inertial_optimization -> write-back and dumps what the caller sees.
#include "driver_common.h"
#include "mock_inertial.h"

namespace {

void body(const Arrays &in, const std::string &pre, ImuBody &b)
{
    std::memcpy(b.Rwb, get(in, pre + "Rwb").p<float>(), sizeof b.Rwb);
    std::memcpy(b.twb, get(in, pre + "twb").p<float>(), sizeof b.twb);
    std::memcpy(b.vel, get(in, pre + "v").p<float>(), sizeof b.vel);
    std::memcpy(b.bias, get(in, pre + "bias").p<float>(), sizeof b.bias);
}

void preint(const Arrays &in, const std::string &pre, Preintegrated &q)
{
    const float *f = get(in, pre).p<float>();  // dR dV dP JRg JVg JVa JPg JPa b dT C
    std::memcpy(&q, f, sizeof(float) * (9 + 3 + 3 + 45 + 6 + 1 + 225));
}

// Optimizer::PoseInertialOptimizationLastKeyFrame / LastFrame with the reference's parameter list, the bodies
// adapters/orbslam3/Optimizer_osg.cc gives them
int PoseInertialOptimizationLastKeyFrame(ImuFrame *pFrame, bool bRecInit = false)
{
    return osg_orbslam3::pose_inertial_optimization_last_keyframe<InertialHooks>(pFrame, bRecInit);
}
int PoseInertialOptimizationLastFrame(ImuFrame *pFrame, bool bRecInit = false)
{
    return osg_orbslam3::pose_inertial_optimization_last_frame<InertialHooks>(pFrame, bRecInit);
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc != 4) {
        std::fprintf(stderr, "usage: poseinertial_driver gather|optimize <in> <out>\n");
        return 2;
    }
    static_assert(sizeof(Preintegrated) == sizeof(float) * 292, "packed float fields");
    const std::string mode = argv[1];
    const Arrays in = read_arrays(argv[2]);
    const int32_t *par = get(in, "params").p<int32_t>();  // last_frame, rec_init, N, Nleft, two cameras, has prior
    const bool last_frame = par[0] != 0, rec_init = par[1] != 0, two = par[4] != 0, has_prior = par[5] != 0;
    ImuFrame F, Fp;
    ImuKeyFrame KF;
    Camera c1, c2;
    F.N = par[2];
    F.Nleft = par[3];
    const float *kl = get(in, "keys").p<float>(), *ku = get(in, "keys_un").p<float>(), *kr = get(in, "keys_right").p<float>();
    auto keys = [](const float *k, size_t n, std::vector<cv::KeyPoint> &v) {
        v.resize(n);
        for (size_t i = 0; i < n; i++) v[i].pt.x = k[3 * i], v[i].pt.y = k[3 * i + 1], v[i].octave = (int)k[3 * i + 2];
    };
    keys(kl, get(in, "keys").n / 3, F.mvKeys);
    keys(ku, get(in, "keys_un").n / 3, F.mvKeysUn);
    keys(kr, get(in, "keys_right").n / 3, F.mvKeysRight);
    F.mvuRight.assign(get(in, "uright").p<float>(), get(in, "uright").p<float>() + get(in, "uright").n);
    F.mvInvLevelSigma2.assign(get(in, "isig").p<float>(), get(in, "isig").p<float>() + get(in, "isig").n);
    const float *cp = get(in, "cam").p<float>();  // type, 8 parameters, bf
    c1.type = c2.type = (int)cp[0];
    c1.params.assign(cp + 1, cp + 9);
    c2.params = c1.params;
    F.mbf = cp[9];
    F.fx = cp[1], F.fy = cp[2], F.cx = cp[3], F.cy = cp[4];
    F.mpCamera = &c1;
    if (two) F.mpCamera2 = &c2;
    const float *ex = get(in, "extr").p<float>();  // Rcw tcw Rcb tcb tbc Rrl trl
    std::memcpy(F.Rcw, ex, 36), std::memcpy(F.tcw, ex + 9, 12), std::memcpy(F.Rcb, ex + 12, 36);
    std::memcpy(F.tcb, ex + 21, 12), std::memcpy(F.tbc, ex + 24, 12), std::memcpy(F.Rrl, ex + 27, 36);
    std::memcpy(F.trl, ex + 36, 12);
    body(in, "cur.", F);
    body(in, "prev.", Fp);
    body(in, "prev.", KF);
    F.mpPrevFrame = &Fp;
    F.mpLastKeyFrame = &KF;
    Preintegrated pkf, pfr;
    preint(in, "preint_kf", pkf);
    preint(in, "preint_frame", pfr);
    F.mpImuPreintegrated = &pkf;
    F.mpImuPreintegratedFrame = &pfr;
    if (has_prior) {
        const double *pr = get(in, "prior").p<double>();  // Rwb twb vwb bg ba H, stored as is
        Fp.mpcpi = new ConstraintPoseImu(pr, pr + 9, pr + 12, pr + 15, pr + 18, pr + 21);
        std::memcpy(Fp.mpcpi->H, pr + 21, sizeof Fp.mpcpi->H);
    }
    // slots: MapPoint index per slot (-1: none); every slot's outlier flag starts true
    const int32_t *slot = get(in, "slot.mp").p<int32_t>();
    const Arr &pos = get(in, "mp.pos");
    std::vector<MapPoint> pool(pos.n / 3);
    for (size_t j = 0; j < pool.size(); j++) {
        std::memcpy(pool[j].pos, pos.p<double>() + 3 * j, sizeof pool[j].pos);
        pool[j].mTrackDepth = get(in, "mp.depth").p<float>()[j];
    }
    F.mvpMapPoints.assign(F.N, nullptr);
    F.mvbOutlier.assign(F.N, true);
    for (int i = 0; i < F.N; i++)
        if (slot[i] >= 0) F.mvpMapPoints[i] = &pool[slot[i]];
    Arrays out;
    auto flags = [&] {
        std::vector<uint8_t> o(F.N);
        for (int i = 0; i < F.N; i++) o[i] = F.mvbOutlier[i];
        return o;
    };
    if (mode == "gather") {
        osg_orbslam3::PoseInertialGather<InertialHooks, ImuFrame> g;
        g.assign(&F, last_frame, rec_init, (osg_orbslam3::NoMutex *)nullptr);
        const osg_pose_inertial_problem &p = g.p;
        out["head"] = make('i', std::vector<int32_t>{p.mode, p.rec_init, p.n_cams, p.n_edges, p.prior != nullptr,
                                                     osg_pose_inertial_check(&p)});
        out["kind"] = make('b', std::vector<uint8_t>(g.kind.begin(), g.kind.end()));
        out["slot"] = make('i', std::vector<int32_t>(g.slot.begin(), g.slot.end()));
        out["xw"] = make('d', g.xw);
        out["obs"] = make('d', g.obs);
        out["isig"] = make('f', g.isig);
        out["depth"] = make('f', g.depth);
        out["outlier"] = make('b', flags());
        std::vector<double> st;
        for (const osg_pio_state *s : {&p.cur, &p.prev}) {
            st.insert(st.end(), s->Rwb, s->Rwb + 9), st.insert(st.end(), s->twb, s->twb + 3);
            st.insert(st.end(), s->v, s->v + 3), st.insert(st.end(), s->bg, s->bg + 3), st.insert(st.end(), s->ba, s->ba + 3);
        }
        out["states"] = make('d', st);
        std::vector<double> cm;
        for (int c = 0; c < p.n_cams; c++) {
            const osg_pio_camera &k = p.cams[c];
            cm.insert(cm.end(), k.Rcw, k.Rcw + 9), cm.insert(cm.end(), k.tcw, k.tcw + 3), cm.insert(cm.end(), k.Rcb, k.Rcb + 9);
            cm.insert(cm.end(), k.tcb, k.tcb + 3), cm.insert(cm.end(), k.tbc, k.tbc + 3);
        }
        cm.push_back(p.bf);
        out["cams"] = make('d', cm);
        out["preint_dT_b"] = make('f', std::vector<float>{p.preint->dT, p.preint->b[0], p.preint->b[5], p.preint->C[0],
                                                          p.C_rw[0], p.C_rw[224]});
    } else if (mode == "optimize") {
        ConstraintPoseImu *before = Fp.mpcpi;
        const int ret = last_frame ? PoseInertialOptimizationLastFrame(&F, rec_init)
                                   : PoseInertialOptimizationLastKeyFrame(&F, rec_init);
        if (osg_orbslam3::thread_ctx() == nullptr) {
            std::fprintf(stderr, "no device context\n");
            return 3;
        }
        out["ret"] = make('i', std::vector<int32_t>{ret, F.mpcpi != nullptr, Fp.mpcpi == nullptr, before != nullptr,
                                                    ConstraintPoseImu::live});
        out["outlier"] = make('b', flags());
        std::vector<float> st(F.Rwb, F.Rwb + 9);
        st.insert(st.end(), F.twb, F.twb + 3), st.insert(st.end(), F.vel, F.vel + 3), st.insert(st.end(), F.bias, F.bias + 6);
        out["state"] = make('f', st);
        if (F.mpcpi) {
            const ConstraintPoseImu &c = *F.mpcpi;
            std::vector<double> v(c.Rwb, c.Rwb + 9);
            v.insert(v.end(), c.twb, c.twb + 3), v.insert(v.end(), c.vwb, c.vwb + 3), v.insert(v.end(), c.bg, c.bg + 3);
            v.insert(v.end(), c.ba, c.ba + 3), v.insert(v.end(), c.H, c.H + 225);
            out["mpcpi"] = make('d', v);
        }
        delete F.mpcpi;
        delete Fp.mpcpi;
    } else {
        std::fprintf(stderr, "unknown mode %s\n", mode.c_str());
        return 2;
    }
    write_arrays(argv[3], out);
    return 0;
}
