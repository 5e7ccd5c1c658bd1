// sim3solver_driver.cpp — Sim3Solver through the ORB-SLAM3-side adapter on mock objects (test-only;
// tests/test_adapter_sim3solver.py).  Builds three KeyFrames (pKF1, pKF2 and another KeyFrame of the
// window) and their MapPoints from an array file, then
//   gather <in> <out>   runs the constructor alone (pure host code, no device) and dumps what it kept;
//   loop   <in> <out>   SetRansacParameters, then LoopClosing's
//                       while (!bConverge && !bNoMore) iterate(window, ...) (ref:src/LoopClosing.cc:993-997)
//                       and dumps what the caller sees.
// The hooks derive from MockHooks; RandomInt is scripted from the array file.
#include "driver_common.h"

namespace {

struct M4 { float a[16]; };
struct M3 { float a[9]; };
struct V3 { float a[3]; };

std::vector<int32_t> g_rand;
size_t g_rand_pos = 0;
int g_rand_bad = 0;

struct SolverHooks : MockHooks {
    using Matrix4f = M4;
    using Matrix3f = M3;
    using Vector3f = V3;
    static M4 mat4(const float *m) { M4 r; std::memcpy(r.a, m, sizeof r.a); return r; }
    static M3 mat3(const float *m) { M3 r; std::memcpy(r.a, m, sizeof r.a); return r; }
    static V3 vec3(const float *m) { V3 r; std::memcpy(r.a, m, sizeof r.a); return r; }
    static int random_int(int lo, int hi)
    {
        const int v = g_rand_pos < g_rand.size() ? g_rand[g_rand_pos] : lo;
        if (g_rand_pos >= g_rand.size() || v < lo || v > hi) g_rand_bad++;
        g_rand_pos++;
        return v < lo ? lo : v > hi ? hi : v;
    }
    // Rcw * Xw + tcw in float from pose[7], as ref:src/Sim3Solver.cc:103-107 evaluates it
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
};

using Solver = osg_orbslam3::Sim3Solver<SolverHooks, KeyFrame, MapPoint>;

void build_kf(const Arrays &in, const std::string &pre, KeyFrame &K, Camera &cam)
{
    const Arr &oct = get(in, pre + "oct");
    K.N = (int)oct.n;
    K.mvKeysUn.resize(K.N);
    for (int i = 0; i < K.N; i++) K.mvKeysUn[i].octave = oct.p<int32_t>()[i];
    const Arr &s2 = get(in, "sig2");
    K.mvLevelSigma2.assign(s2.p<float>(), s2.p<float>() + s2.n);
    std::memcpy(K.pose, get(in, pre + "pose").p<double>(), sizeof K.pose);
    const Arr &cp = get(in, pre + "cam");
    cam.type = (int)cp.p<float>()[0];
    cam.params.assign(cp.p<float>() + 1, cp.p<float>() + cp.n);
    K.mpCamera = &cam;
    K.mvpMapPoints.assign(K.N, nullptr);
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc != 4) {
        std::fprintf(stderr, "usage: sim3solver_driver gather|loop <in> <out>\n");
        return 2;
    }
    const std::string mode = argv[1];
    const Arrays in = read_arrays(argv[2]);
    KeyFrame K[3];
    Camera cam[3];
    for (int k = 0; k < 3; k++) build_kf(in, "kf" + std::to_string(k + 1) + ".", K[k], cam[k]);
    const Arr &pos = get(in, "mp.pos");
    const int M = (int)(pos.n / 3);
    std::vector<MapPoint> pool(M);
    for (int j = 0; j < M; j++) {
        pool[j].mnId = j;
        std::memcpy(pool[j].pos, pos.p<double>() + 3 * j, sizeof pool[j].pos);
        pool[j].bad = get(in, "mp.bad").p<uint8_t>()[j] != 0;
        for (int k = 0; k < 3; k++) {
            const int idx = get(in, "mp.kf" + std::to_string(k + 1) + "idx").p<int32_t>()[j];
            if (idx >= 0) pool[j].AddObservation(&K[k], idx);
        }
    }
    const Arr &mp1 = get(in, "slot.mp1");
    const int S = (int)mp1.n;
    const int32_t *match = get(in, "slot.match").p<int32_t>(), *kfm = get(in, "slot.kfm").p<int32_t>();
    K[0].mvpMapPoints.assign(S, nullptr);  // the slots of pKF1 (GetMapPointMatches)
    std::vector<MapPoint *> vpMatched12(S, nullptr);
    std::vector<KeyFrame *> vpKeyFrameMatchedMP;
    const int32_t *par = get(in, "params").p<int32_t>();
    const bool bFixScale = par[0] != 0, pass_kfm = par[1] != 0;
    const int minInliers = par[2], maxIterations = par[3], window = par[4];
    for (int i = 0; i < S; i++) {
        if (mp1.p<int32_t>()[i] >= 0) K[0].mvpMapPoints[i] = &pool[mp1.p<int32_t>()[i]];
        if (match[i] >= 0) vpMatched12[i] = &pool[match[i]];
        if (pass_kfm) vpKeyFrameMatchedMP.push_back(&K[kfm[i] - 1]);
    }
    const Arr &rnd = get(in, "rand");
    g_rand.assign(rnd.p<int32_t>(), rnd.p<int32_t>() + rnd.n);

    Solver solver = Solver(&K[0], &K[1], vpMatched12, bFixScale, vpKeyFrameMatchedMP);
    Arrays out;
    const auto &g = solver.gather();
    out["p1c"] = make('f', g.p1c);
    out["p2c"] = make('f', g.p2c);
    out["max1"] = make('f', g.max_err1);
    out["max2"] = make('f', g.max_err2);
    out["index"] = make('i', std::vector<int32_t>(g.mvnIndices1.begin(), g.mvnIndices1.end()));
    out["shape"] = make('i', std::vector<int32_t>{g.mN1, g.cam1.type, g.cam2.type});
    out["cams"] = make('f', std::vector<float>{g.cam1.p[0], g.cam1.p[2], g.cam2.p[0], g.cam2.p[2]});
    if (mode == "loop") {
        solver.SetRansacParameters(0.99, minInliers, maxIterations);
        bool bNoMore = false, bConverge = false;
        std::vector<bool> vbInliers;
        int nInliers = 0, calls = 0;
        M4 last{};
        std::vector<float> returned;  // every call's matrix
        std::vector<int32_t> trace;   // per call: bConverge, bNoMore, nInliers, mnIterations, mnBestInliers
        while (!bConverge && !bNoMore) {
            last = solver.iterate(window, bNoMore, vbInliers, nInliers, bConverge);
            calls++;
            returned.insert(returned.end(), last.a, last.a + 16);
            for (int v : {(int)bConverge, (int)bNoMore, nInliers, solver.iterations(), solver.best_inliers()})
                trace.push_back(v);
            if (calls > 1000) return 4;
        }
        if (minInliers <= (int)g.mvnIndices1.size() && osg_orbslam3::thread_ctx() == nullptr) {
            std::fprintf(stderr, "no device context\n");
            return 3;
        }
        std::vector<uint8_t> vb(vbInliers.size());
        for (size_t i = 0; i < vb.size(); i++) vb[i] = vbInliers[i];
        out["flags"] = make('i', std::vector<int32_t>{(int)bConverge, (int)bNoMore, nInliers, calls, solver.max_iterations(),
                                                        (int)g_rand_pos, g_rand_bad});
        out["vbInliers"] = make('b', vb);
        out["returned"] = make('f', returned);
        out["trace"] = make('i', trace);
        const M4 T = solver.GetEstimatedTransformation();
        const M3 R = solver.GetEstimatedRotation();
        const V3 t = solver.GetEstimatedTranslation();
        out["T12"] = make('f', std::vector<float>(T.a, T.a + 16));
        out["R"] = make('f', std::vector<float>(R.a, R.a + 9));
        out["t"] = make('f', std::vector<float>(t.a, t.a + 3));
        out["s"] = make('f', std::vector<float>{solver.GetEstimatedScale()});
        // the first overload and find() on fresh solvers over the same stream
        g_rand_pos = 0;
        Solver s2 = Solver(&K[0], &K[1], vpMatched12, bFixScale, vpKeyFrameMatchedMP);
        s2.SetRansacParameters(0.99, minInliers, maxIterations);
        bool nm2 = false;
        std::vector<bool> vb2;
        int ni2 = 0;
        const M4 f = s2.find(vb2, ni2);
        out["find"] = make('f', std::vector<float>(f.a, f.a + 16));
        out["find_flags"] = make('i', std::vector<int32_t>{ni2, s2.iterations(), s2.best_inliers()});
        g_rand_pos = 0;
        Solver s3 = Solver(&K[0], &K[1], vpMatched12, bFixScale, vpKeyFrameMatchedMP);
        s3.SetRansacParameters(0.99, minInliers, maxIterations);
        const M4 f1 = s3.iterate(window, nm2, vb2, ni2);
        out["iter1"] = make('f', std::vector<float>(f1.a, f1.a + 16));
        out["iter1_flags"] = make('i', std::vector<int32_t>{(int)nm2, ni2, s3.iterations()});
    } else if (mode != "gather") {
        std::fprintf(stderr, "unknown mode %s\n", mode.c_str());
        return 2;
    }
    write_arrays(argv[3], out);
    return 0;
}
