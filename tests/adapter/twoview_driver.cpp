// twoview_driver.cpp — TwoViewReconstruction::Reconstruct through the ORB-SLAM3-side adapter on mock keypoints
// (test-only; tests/test_adapter_twoview.py).
//   twoview_driver <in> <out>
// in:  keys1, keys2 (n x 2 float, undistorted), matches12 (int per frame-1 keypoint), K (fx fy cx cy), params
//      (sigma as float bits are not needed: iterations), rand (the RandomInt stream).
// out: what the caller of Reconstruct sees (ok, T21, vP3D, vbTriangulated, which start as sentinels), and the
//      reference's members the body builds (mvMatches12, mvbMatched1, mvSets).
#include "driver_common.h"
#include "mock_twoview.h"

int main(int argc, char **argv)
{
    if (argc != 3) {
        std::fprintf(stderr, "usage: twoview_driver <in> <out>\n");
        return 2;
    }
    const Arrays in = read_arrays(argv[1]);
    auto keys = [&](const char *name) {
        const Arr &a = get(in, name);
        std::vector<cv::KeyPoint> v(a.n / 2);
        for (size_t i = 0; i < v.size(); i++) v[i].pt.x = a.p<float>()[2 * i], v[i].pt.y = a.p<float>()[2 * i + 1];
        return v;
    };
    const std::vector<cv::KeyPoint> vKeys1 = keys("keys1"), vKeys2 = keys("keys2");
    const Arr &m = get(in, "matches12");
    const std::vector<int> vMatches12(m.p<int32_t>(), m.p<int32_t>() + m.n);
    const float *K = get(in, "K").p<float>();
    const int iterations = get(in, "params").p<int32_t>()[0];
    const Arr &rnd = get(in, "rand");
    TwoViewRandom &R = twoview_random();
    R.stream.assign(rnd.p<int32_t>(), rnd.p<int32_t>() + rnd.n);

    osg_orbslam3::TwoViewReconstruction<TwoViewHooks, cv::KeyPoint, cv::Point3f> tv(K[0], K[1], K[2], K[3], 1.0f, iterations);
    // sentinels: the reference leaves its outputs untouched when it returns false
    float R21[9], t21[3];
    for (float &v : R21) v = -7.f;
    for (float &v : t21) v = -7.f;
    std::vector<cv::Point3f> vP3D(3);
    std::vector<bool> vbTriangulated(5, true);
    const bool ok = tv.Reconstruct(vKeys1, vKeys2, vMatches12, R21, t21, vP3D, vbTriangulated);
    if ((int)tv.matches12().size() >= 8 && osg_orbslam3::thread_ctx() == nullptr) {
        std::fprintf(stderr, "no device context\n");
        return 3;
    }
    Arrays out;
    const osg_two_view_result &r = tv.result();
    out["flags"] = make('i', std::vector<int32_t>{(int)ok, r.model, r.hyp_h, r.hyp_f, r.cand, (int)R.pos, R.bad, R.seeded, R.seed,
                                                    R.draws_before_seed});
    out["R"] = make('f', std::vector<float>(R21, R21 + 9));
    out["t"] = make('f', std::vector<float>(t21, t21 + 3));
    std::vector<float> p3d;
    for (const auto &p : vP3D) p3d.insert(p3d.end(), {p.x, p.y, p.z});
    out["vP3D"] = make('f', p3d);
    std::vector<uint8_t> tri(vbTriangulated.size());
    for (size_t i = 0; i < tri.size(); i++) tri[i] = vbTriangulated[i];
    out["vbTriangulated"] = make('b', tri);
    std::vector<int32_t> m12;
    for (const auto &pr : tv.matches12()) m12.insert(m12.end(), {pr.first, pr.second});
    out["mvMatches12"] = make('i', m12);
    std::vector<uint8_t> matched(tv.matched1().size());
    for (size_t i = 0; i < matched.size(); i++) matched[i] = tv.matched1()[i];
    out["mvbMatched1"] = make('b', matched);
    out["mvSets"] = make('i', tv.sets());
    out["n_good"] = make('i', std::vector<int32_t>(r.n_good, r.n_good + 8));
    write_arrays(argv[2], out);
    return 0;
}
