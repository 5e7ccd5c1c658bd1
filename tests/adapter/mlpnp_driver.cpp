// mlpnp_driver.cpp — MLPnPsolver through the ORB-SLAM3-side adapter on mock objects (test-only;
// tests/test_adapter_mlpnp.py).  Builds a Frame and its MapPoint matches from an array file, then
//   gather <in> <out>   runs the constructor and SetRansacParameters alone (pure host code, no device) and
//                       dumps what they kept;
//   loop   <in> <out>   SetRansacParameters(0.99, 10, 300, 6, 0.5, 5.991), then Tracking's iterate(5, ...)
//                       (ref:src/Tracking.cc:4520-4540) `calls` times, and dumps what the caller sees per call.
// The hooks derive from MockHooks; RandomInt is scripted from the array file.
#include "driver_common.h"
#include "mock_mlpnp.h"

namespace {

struct M4 { float a[16]; };

std::vector<int32_t> g_rand;
size_t g_rand_pos = 0;
int g_rand_bad = 0;

struct SolverHooks : MockHooks {
    using Matrix4f = M4;
    static M4 mat4(const float *m) { M4 r; std::memcpy(r.a, m, sizeof r.a); return r; }
    static int random_int(int lo, int hi)
    {
        const int v = g_rand_pos < g_rand.size() ? g_rand[g_rand_pos] : lo;
        if (g_rand_pos >= g_rand.size() || v < lo || v > hi) g_rand_bad++;
        g_rand_pos++;
        return v < lo ? lo : v > hi ? hi : v;
    }
    static void unproject(const Frame &F, float u, float v, float ray[3]) { mock_unproject(*F.mpCamera, u, v, ray); }
    static void mp_world_pos(MapPoint *p, float x[3])
    {
        for (int k = 0; k < 3; k++) x[k] = (float)p->pos[k];
    }
};

using Solver = osg_orbslam3::MLPnPsolver<SolverHooks, Frame, MapPoint>;

}  // namespace

int main(int argc, char **argv)
{
    if (argc != 4) {
        std::fprintf(stderr, "usage: mlpnp_driver gather|loop <in> <out>\n");
        return 2;
    }
    const std::string mode = argv[1];
    const Arrays in = read_arrays(argv[2]);
    Frame F;
    Camera cam;
    const Arr &kp = get(in, "kp"), &oct = get(in, "oct"), &s2 = get(in, "sig2"), &cp = get(in, "cam");
    F.N = (int)oct.n;
    F.mvKeysUn.resize(F.N);
    for (int i = 0; i < F.N; i++) {
        F.mvKeysUn[i].pt.x = kp.p<float>()[2 * i];
        F.mvKeysUn[i].pt.y = kp.p<float>()[2 * i + 1];
        F.mvKeysUn[i].octave = oct.p<int32_t>()[i];
    }
    F.mvLevelSigma2.assign(s2.p<float>(), s2.p<float>() + s2.n);
    cam.type = (int)cp.p<float>()[0];
    cam.params.assign(cp.p<float>() + 1, cp.p<float>() + cp.n);
    F.mpCamera = &cam;
    const Arr &pos = get(in, "mp.pos");
    const int M = (int)(pos.n / 3);
    std::vector<MapPoint> pool(M);
    for (int j = 0; j < M; j++) {
        pool[j].mnId = j;
        std::memcpy(pool[j].pos, pos.p<double>() + 3 * j, sizeof pool[j].pos);
        pool[j].bad = get(in, "mp.bad").p<uint8_t>()[j] != 0;
    }
    const Arr &slot = get(in, "slot.mp");  // may be longer than mvKeysUn
    std::vector<MapPoint *> vpMapPointMatches(slot.n, nullptr);
    for (size_t i = 0; i < slot.n; i++)
        if (slot.p<int32_t>()[i] >= 0) vpMapPointMatches[i] = &pool[slot.p<int32_t>()[i]];
    const Arr &rnd = get(in, "rand");
    g_rand.assign(rnd.p<int32_t>(), rnd.p<int32_t>() + rnd.n);
    const int calls = get(in, "params").p<int32_t>()[0];

    Solver solver(F, vpMapPointMatches);
    solver.SetRansacParameters(0.99, 10, 300, 6, 0.5, 5.991);
    Arrays out;
    const auto &g = solver.gather();
    out["bearing"] = make('f', g.bearing);
    out["p3dw"] = make('f', g.p3dw);
    out["p2d"] = make('f', g.p2d);
    out["max_err"] = make('f', solver.max_errors());
    out["index"] = make('i', std::vector<int32_t>(g.mvKeyPointIndices.begin(), g.mvKeyPointIndices.end()));
    out["shape"] = make('i', std::vector<int32_t>{(int)g.n_slots, g.cam.type, solver.min_inliers(), solver.max_iterations()});
    if (mode == "loop") {
        std::vector<float> returned;
        std::vector<int32_t> trace;   // per call: return value, bNoMore, nInliers, mnIterations, mnBestInliers, draws so far
        std::vector<uint8_t> flags;   // per call: vbInliers (empty vectors as zeros)
        for (int c = 0; c < calls; c++) {
            bool bNoMore = false;
            std::vector<bool> vbInliers;
            int nInliers = 0;
            M4 T{};
            const bool ok = solver.iterate(5, bNoMore, vbInliers, nInliers, T);
            returned.insert(returned.end(), T.a, T.a + 16);
            for (int v : {(int)ok, (int)bNoMore, nInliers, solver.iterations(), solver.best_inliers(), (int)g_rand_pos,
                          (int)vbInliers.size()})
                trace.push_back(v);
            for (size_t i = 0; i < g.n_slots; i++) flags.push_back(i < vbInliers.size() && vbInliers[i] ? 1 : 0);
        }
        if (osg_orbslam3::thread_ctx() == nullptr) {
            std::fprintf(stderr, "no device context\n");
            return 3;
        }
        out["returned"] = make('f', returned);
        out["trace"] = make('i', trace);
        out["vbInliers"] = make('b', flags);
        out["rand_bad"] = make('i', std::vector<int32_t>{g_rand_bad});
    } else if (mode != "gather") {
        std::fprintf(stderr, "unknown mode %s\n", mode.c_str());
        return 2;
    }
    write_arrays(argv[3], out);
    return 0;
}
