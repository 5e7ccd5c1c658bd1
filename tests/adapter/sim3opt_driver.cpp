// sim3opt_driver.cpp — OptimizeSim3 through the ORB-SLAM3-side adapter on mock objects (test-only;
// tests/test_adapter_sim3opt.py).  Builds a KeyFrame pair and its MapPoints from an array file, then
//   gather   <in> <out>   runs the graph build alone (pure host code, no device) and dumps the problem;
//   optimize <in> <out>   runs gather -> osg_optimize_sim3 -> write-back and dumps what the caller sees.
// The hooks derive from MockHooks; the Sim3 stand-in carries r, t, s like g2o::Sim3.
#include "driver_common.h"

namespace {

struct MockSim3 {  // g2o::Sim3's members
    double r[4] = {0, 0, 0, 1}, t[3] = {0, 0, 0}, s = 1;
};
struct MockHessian {  // Eigen::Matrix<double, 7, 7>
    double a[49];
};

struct Sim3Hooks : MockHooks {
    // Rcw * Xw + tcw in float from pose[7], as ref:src/Optimizer.cc:4297-4307 evaluates it
    static void cam_point(KeyFrame *k, MapPoint *p, double x[3])
    {
        const double qx = k->pose[0], qy = k->pose[1], qz = k->pose[2], qw = k->pose[3];
        const double R[3][3] = {{1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qz * qw), 2 * (qx * qz + qy * qw)},
                                {2 * (qx * qy + qz * qw), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - qx * qw)},
                                {2 * (qx * qz - qy * qw), 2 * (qy * qz + qx * qw), 1 - 2 * (qx * qx + qy * qy)}};
        const float X[3] = {(float)p->pos[0], (float)p->pos[1], (float)p->pos[2]};
        for (int r = 0; r < 3; r++) {
            float v = (float)R[r][0] * X[0];
            v = v + (float)R[r][1] * X[1];
            v = v + (float)R[r][2] * X[2];
            v = v + (float)k->pose[4 + r];
            x[r] = (double)v;
        }
    }
    static void sim3_get(const MockSim3 &S, double q[4], double t[3], double &s)
    {
        std::memcpy(q, S.r, sizeof S.r);
        std::memcpy(t, S.t, sizeof S.t);
        s = S.s;
    }
    static void sim3_set(MockSim3 &S, const double q[4], const double t[3], double s)
    {
        std::memcpy(S.r, q, sizeof S.r);
        std::memcpy(S.t, t, sizeof S.t);
        S.s = s;
    }
    static void zero_hessian(MockHessian &H) { std::memset(H.a, 0, sizeof H.a); }
};

// Optimizer::OptimizeSim3 with the reference's parameter list (ref:include/Optimizer.h:98-100), the body
// adapters/orbslam3/Optimizer_osg.cc gives it
int OptimizeSim3(KeyFrame *pKF1, KeyFrame *pKF2, std::vector<MapPoint *> &vpMatches1, MockSim3 &g2oS12, const float th2,
                 const bool bFixScale, MockHessian &mAcumHessian, const bool bAllPoints = false)
{
    return osg_orbslam3::optimize_sim3<Sim3Hooks>(pKF1, pKF2, vpMatches1, g2oS12, th2, bFixScale, mAcumHessian,
                                                  bAllPoints);
}

void build_kf(const Arrays &in, const std::string &pre, KeyFrame &K, Camera &cam)
{
    const Arr &kp = get(in, pre + "kp");
    K.N = (int)(kp.n / 2);
    K.mvKeysUn.resize(K.N);
    const int32_t *oct = get(in, pre + "oct").p<int32_t>();
    for (int i = 0; i < K.N; i++) {
        K.mvKeysUn[i].pt.x = kp.p<float>()[2 * i];
        K.mvKeysUn[i].pt.y = kp.p<float>()[2 * i + 1];
        K.mvKeysUn[i].octave = oct[i];
    }
    const Arr &is = get(in, "isig");
    K.mvInvLevelSigma2.assign(is.p<float>(), is.p<float>() + is.n);
    std::memcpy(K.pose, get(in, pre + "pose").p<double>(), sizeof K.pose);
    const Arr &cp = get(in, pre + "cam");
    cam.type = (int)cp.p<float>()[0];
    cam.params.assign(cp.p<float>() + 1, cp.p<float>() + cp.n);
    K.mpCamera = &cam;
    K.fx = cam.params[0];
    K.fy = cam.params[1];
    K.cx = cam.params[2];
    K.cy = cam.params[3];
    K.mvpMapPoints.assign(K.N, nullptr);
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc != 4) {
        std::fprintf(stderr, "usage: sim3opt_driver gather|optimize <in> <out>\n");
        return 2;
    }
    const std::string mode = argv[1];
    const Arrays in = read_arrays(argv[2]);
    KeyFrame K1, K2;
    Camera c1, c2;
    build_kf(in, "kf1.", K1, c1);
    build_kf(in, "kf2.", K2, c2);
    const Arr &pos = get(in, "mp.pos");
    const int M = (int)(pos.n / 3);
    std::vector<MapPoint> pool(M);
    const int32_t *kf2idx = get(in, "mp.kf2idx").p<int32_t>();
    for (int j = 0; j < M; j++) {
        pool[j].mnId = j;
        std::memcpy(pool[j].pos, pos.p<double>() + 3 * j, sizeof pool[j].pos);
        pool[j].bad = get(in, "mp.bad").p<uint8_t>()[j] != 0;
        pool[j].mnTrackScaleLevel = 3;  // must not reach the weight: kpUn2.octave stays 0 (:4400)
        if (kf2idx[j] >= 0) pool[j].AddObservation(&K2, kf2idx[j]);
    }
    const int32_t *mp1 = get(in, "slot.mp1").p<int32_t>(), *match = get(in, "slot.match").p<int32_t>();
    std::vector<MapPoint *> vpMatches1(K1.N, nullptr);
    for (int i = 0; i < K1.N; i++) {
        if (mp1[i] >= 0) K1.mvpMapPoints[i] = &pool[mp1[i]];
        if (match[i] >= 0) vpMatches1[i] = &pool[match[i]];
    }
    const float *par = get(in, "params").p<float>();
    const float th2 = par[0];
    const bool bFixScale = par[1] != 0, bAllPoints = par[2] != 0;
    Arrays out;
    if (mode == "gather") {
        osg_orbslam3::Sim3Gather<Sim3Hooks, KeyFrame, MapPoint> g;
        osg_orbslam3::gather_optimize_sim3<Sim3Hooks>(g, &K1, &K2, vpMatches1, th2, bFixScale, bAllPoints);
        out["n_pairs"] = make('i', std::vector<int32_t>{g.p.n_pairs, g.p.fix_scale, g.p.cam1.type, g.p.cam2.type});
        out["th2"] = make('f', std::vector<float>{g.p.th2, g.p.cam1.p[0], g.p.cam2.p[0]});
        out["p1c"] = make('d', g.p1c);
        out["p2c"] = make('d', g.p2c);
        out["obs1"] = make('d', g.obs1);
        out["obs2"] = make('d', g.obs2);
        out["w1"] = make('f', g.w1);
        out["w2"] = make('f', g.w2);
        out["index"] = make('i', std::vector<int32_t>(g.vnIndexEdge.begin(), g.vnIndexEdge.end()));
        out["in_kf2"] = make('b', g.vbIsInKF2);
    } else if (mode == "optimize") {
        MockSim3 S;
        const double *s8 = get(in, "sim3").p<double>();
        std::memcpy(S.r, s8, sizeof S.r);
        std::memcpy(S.t, s8 + 4, sizeof S.t);
        S.s = s8[7];
        MockHessian H;
        for (double &v : H.a) v = 7.0;  // a sentinel: the early return must leave it
        const int ret = OptimizeSim3(&K1, &K2, vpMatches1, S, th2, bFixScale, H, bAllPoints);
        if (osg_orbslam3::thread_ctx() == nullptr) {
            std::fprintf(stderr, "no device context\n");
            return 3;
        }
        std::vector<uint8_t> null_after(K1.N);
        for (int i = 0; i < K1.N; i++) null_after[i] = vpMatches1[i] == nullptr;
        out["ret"] = make('i', std::vector<int32_t>{ret});
        out["match_null"] = make('b', null_after);
        out["sim3"] = make('d', std::vector<double>{S.r[0], S.r[1], S.r[2], S.r[3], S.t[0], S.t[1], S.t[2], S.s});
        out["hess"] = make('d', std::vector<double>(H.a, H.a + 49));
    } else {
        std::fprintf(stderr, "unknown mode %s\n", mode.c_str());
        return 2;
    }
    write_arrays(argv[3], out);
    return 0;
}
