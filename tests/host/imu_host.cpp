// imu_host.cpp — stand-alone host program over csrc/imu_common.h (test-only).
//   imu_host layout      prints sizeof / offsetof of the osg_imu_* structs of include/osg_imu.h, for the ctypes mirrors
//   imu_host check       runs the host side of osg_imu_* without a device: every argument check, the queue rule,
//                        the four interpolation branches, the deltas, PredictStateIMU and the packing of the
//                        kernel's per-problem block; prints "ok"
//   imu_host bits        prints the raw bytes, as hex, of delta and predict_state on a fixed state at three bias
//                        steps (none, 1e-2, and one that puts JRg dbg below Sophus's small-angle cut), for
//                        tests/golden/imu_host_bits.txt
// Plain host C++: tests/test_preintegration.py builds it with -fsanitize=address,undefined and runs it directly.
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "imu_common.h"

#define EXPECT(cond)                                                       \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("FAILED %s (line %d)\n", #cond, __LINE__);         \
            return 1;                                                      \
        }                                                                  \
    } while (0)

static int layout()
{
#define SZ(T) std::printf(#T " %zu\n", sizeof(T))
#define OFF(T, f) std::printf(#T "." #f " %zu\n", offsetof(T, f))
    SZ(osg_imu_preintegrated);
    OFF(osg_imu_preintegrated, pre), OFF(osg_imu_preintegrated, avgA), OFF(osg_imu_preintegrated, avgW);
    SZ(osg_imu_problem);
    OFF(osg_imu_problem, meas), OFF(osg_imu_problem, n), OFF(osg_imu_problem, bias), OFF(osg_imu_problem, nga);
    OFF(osg_imu_problem, nga_walk), OFF(osg_imu_problem, init);
    return 0;
}

static int check()
{
    // ---- argument checks: each refuses before anything past the struct is read
    std::vector<float> meas(7 * 5, 0.25f);
    for (int i = 0; i < 5; i++) meas[7 * i + 6] = 0.005f;
    osg_imu_problem p;
    std::memset(&p, 0, sizeof p);
    p.meas = meas.data(), p.n = 5;
    const char *why = nullptr;
    EXPECT(osgimu::check(&p, &why) == 0);
    EXPECT(osgimu::check(nullptr, &why) == OSG_E_INVALID);
    EXPECT(osgimu::check(&p, nullptr) == 0);
    osg_imu_problem q = p;
    q.n = -1;
    EXPECT(osgimu::check(&q, &why) == OSG_E_INVALID);
    q = p, q.n = OSG_IMU_MAX_STEPS + 1;
    EXPECT(osgimu::check(&q, &why) == OSG_E_INVALID);
    q = p, q.meas = nullptr;
    EXPECT(osgimu::check(&q, &why) == OSG_E_INVALID);
    q.n = 0;  // an empty list needs no pointer
    EXPECT(osgimu::check(&q, &why) == 0);
    const float bad_dt[] = {0.f, -0.005f, std::numeric_limits<float>::quiet_NaN(),
                            std::numeric_limits<float>::infinity(), -std::numeric_limits<float>::infinity()};
    for (float dt : bad_dt) {
        std::vector<float> m2 = meas;
        m2[7 * 4 + 6] = dt;
        q = p, q.meas = m2.data();
        EXPECT(osgimu::check(&q, &why) == OSG_E_INVALID);
        q.n = 4;  // the bad step is past the list
        EXPECT(osgimu::check(&q, &why) == 0);
    }

    // ---- the queue rule: dropped, taken and popped, taken and kept
    const double tq[] = {0.990, 0.9989, 0.9991, 1.004, 1.009, 1.0489, 1.0491, 1.054};
    int32_t taken[8], popped = -1;
    EXPECT(osgimu::select(tq, 8, 1.0, 1.05, 0.001, taken, &popped) == 5);
    EXPECT(taken[0] == 2 && taken[3] == 5 && taken[4] == 6 && popped == 6);
    EXPECT(osgimu::select(tq, 4, 1.0, 1.05, 0.001, taken, &popped) == 2 && popped == 4);  // the queue runs out
    EXPECT(osgimu::select(tq, 0, 1.0, 1.05, 0.001, nullptr, &popped) == 0 && popped == 0);
    EXPECT(osgimu::select(tq, 8, 2.0, 2.05, 0.001, taken, &popped) == 0 && popped == 8);  // all too old
    EXPECT(osgimu::select(tq, -1, 1.0, 1.05, 0.001, taken, &popped) == OSG_E_INVALID);
    EXPECT(osgimu::select(tq, 8, 1.0, 1.05, 0.001, taken, nullptr) == OSG_E_INVALID);

    // ---- the interpolation rule: a single step, two steps (first, last), four (first, middle, last)
    const float a[] = {1, 2, 3, 2, 3, 4, 4, 5, 6, 8, 9, 10, 16, 17, 18};
    const float w[] = {0.1f, 0.2f, 0.3f, 0.2f, 0.3f, 0.4f, 0.4f, 0.5f, 0.6f, 0.8f, 0.9f, 1.0f, 1.6f, 1.7f, 1.8f};
    const double t[] = {1.001, 1.006, 1.011, 1.016, 1.021};
    float out[28];
    EXPECT(osgimu::integrables(a, w, t, 1, 1.0, 1.02, out) == 0);
    EXPECT(osgimu::integrables(a, w, t, 2, 1.0, 1.02, out) == 1);
    EXPECT(out[0] == 1.f && out[5] == 0.3f && out[6] == (float)(1.02 - 1.0));
    EXPECT(osgimu::integrables(a, w, t, 5, 1.0, 1.02, out) == 4);
    {
        const float tab = (float)(t[1] - t[0]), tini = (float)(t[0] - 1.0);
        EXPECT(out[0] == ((1.f + 2.f) - (2.f - 1.f) * (tini / tab)) * 0.5f);
        EXPECT(out[6] == (float)(t[1] - 1.0));
        EXPECT(out[7] == 3.f && out[13] == (float)(t[2] - t[1]));
        const float tab3 = (float)(t[4] - t[3]), tend = (float)(t[4] - 1.02);
        EXPECT(out[21] == ((8.f + 16.f) - (16.f - 8.f) * (tend / tab3)) * 0.5f);
        EXPECT(out[27] == (float)(1.02 - t[3]));
    }
    EXPECT(osgimu::integrables(a, w, t, 0, 1.0, 1.02, out) == OSG_E_INVALID);
    EXPECT(osgimu::integrables(nullptr, w, t, 2, 1.0, 1.02, out) == OSG_E_INVALID);

    // ---- the deltas and PredictStateIMU on the identity: b == bias leaves dR, dV, dP as stored
    osg_imu_preintegrated s;
    std::memset(&s, 0, sizeof s);
    for (int i = 0; i < 3; i++) {
        s.pre.dR[4 * i] = 1.f;
        s.pre.JRg[4 * i] = -0.05f;
        s.pre.JVa[4 * i] = -0.05f;
        s.pre.dV[i] = 0.1f * (i + 1);
        s.pre.dP[i] = 0.01f * (i + 1);
    }
    s.pre.dT = 0.05f;
    float bias[6] = {0, 0, 0, 0, 0, 0}, dR[9], dV[3], dP[3];
    osgimu::delta(&s, bias, dR, dV, dP);
    for (int i = 0; i < 9; i++) EXPECT(std::fabs(dR[i] - (i % 4 == 0 ? 1.f : 0.f)) < 1e-6f);
    EXPECT(dV[1] == s.pre.dV[1] && dP[2] == s.pre.dP[2]);
    osgimu::delta(&s, bias, nullptr, nullptr, nullptr);  // every output is optional
    bias[0] = 0.5f, bias[5] = 0.2f;  // ba_x, bg_z
    osgimu::delta(&s, bias, dR, dV, dP);
    EXPECT(dV[0] == s.pre.dV[0] + -0.05f * 0.5f);
    EXPECT(std::fabs(dR[1] - std::sin(0.01f)) < 1e-6f && std::fabs(dR[0] - std::cos(0.01f)) < 1e-6f);
    const float R1[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, t1[3] = {1, 2, 3}, v1[3] = {0.5f, 0, 0};
    float R2[9], t2[3], v2[3];
    bias[0] = 0.f, bias[5] = 0.f;
    osgimu::predict_state(&s, bias, R1, t1, v1, R2, t2, v2);
    EXPECT(t2[0] == (1.f + 0.5f * 0.05f) + s.pre.dP[0]);
    EXPECT(v2[2] == (0.f + 0.05f * -9.81f) + s.pre.dV[2]);
    EXPECT(t2[2] == ((3.f + 0.f * 0.05f) + ((0.5f * 0.05f) * 0.05f) * -9.81f) + s.pre.dP[2]);
    for (int i = 0; i < 9; i++) EXPECT(std::fabs(R2[i] - R1[i]) < 1e-6f);

    // ---- packing
    q = p, q.init = &s;
    q.bias[2] = 3.f, q.nga[5] = 4.f, q.nga_walk[0] = 5.f;
    osgimu::ProbDev d;
    osgimu::pack(q, 17, d);
    EXPECT(d.n == 5 && d.meas_off == 17 && d.has_init == 1 && d.bias[2] == 3.f && d.nga[5] == 4.f);
    EXPECT(d.nga_walk[0] == 5.f && d.init.pre.dT == 0.05f && d.init.pre.dV[2] == s.pre.dV[2]);
    osgimu::pack(p, 0, d);
    EXPECT(d.has_init == 0 && d.init.pre.dT == 0.f);
    std::printf("ok\n");
    return 0;
}

static void hex(const char *name, const float *v, int n)
{
    std::printf("%s", name);
    for (int i = 0; i < n; i++) {
        uint32_t u;
        std::memcpy(&u, v + i, 4);
        std::printf(" %08x", u);
    }
    std::printf("\n");
}

static int bits()
{
    // a state like a 65-step preintegration: a rotation of 0.2 rad about a skew axis, Jacobians of mixed sign
    uint32_t lcg = 12345u;
    auto next = [&lcg]() {
        lcg = lcg * 1664525u + 1013904223u;
        return (float)(lcg >> 8) / 16777216.0f - 0.5f;
    };
    osg_imu_preintegrated s;
    std::memset(&s, 0, sizeof s);
    const float c = 0.98006658f, sn = 0.19866933f;
    const float R0[9] = {c, -sn, 0.f, sn, c, 0.f, 0.f, 0.f, 1.f};
    const float R1[9] = {1.f, 0.f, 0.f, 0.f, c, -sn, 0.f, sn, c};
    float Rwb[9];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            float a = 0.f, b = 0.f;
            for (int k = 0; k < 3; k++) a += R0[3 * i + k] * R1[3 * k + j], b += R1[3 * i + k] * R0[3 * k + j];
            s.pre.dR[3 * i + j] = a, Rwb[3 * i + j] = b;
        }
    for (int i = 0; i < 9; i++) {
        s.pre.JRg[i] = (i % 4 == 0 ? -0.3f : 0.f) + 0.02f * next();
        s.pre.JVg[i] = 0.5f * next(), s.pre.JVa[i] = (i % 4 == 0 ? -0.3f : 0.f) + 0.05f * next();
        s.pre.JPg[i] = 0.1f * next(), s.pre.JPa[i] = (i % 4 == 0 ? -0.05f : 0.f) + 0.01f * next();
        Rwb[i] += 1e-4f * next();   // a stored rotation, not exactly orthonormal
    }
    for (int i = 0; i < 3; i++) s.pre.dV[i] = 2.f * next(), s.pre.dP[i] = 0.4f * next();
    for (int i = 0; i < 6; i++) s.pre.b[i] = 0.05f * next();
    s.pre.dT = 0.325f;
    const float twb[3] = {1.5f, -2.25f, 0.75f}, vwb[3] = {0.3f, -0.1f, 0.9f};
    const float step[3] = {0.f, 1e-2f, 1e-7f};
    for (int k = 0; k < 3; k++) {
        float bias[6], dR[9], dV[3], dP[3], R2[9], t2[3], v2[3];
        for (int i = 0; i < 6; i++) bias[i] = s.pre.b[i] + step[k] * (2.f * next());
        osgimu::delta(&s, bias, dR, dV, dP);
        osgimu::predict_state(&s, bias, Rwb, twb, vwb, R2, t2, v2);
        std::printf("step %d\n", k);
        hex("dR", dR, 9), hex("dV", dV, 3), hex("dP", dP, 3), hex("Rwb2", R2, 9), hex("twb2", t2, 3), hex("vwb2", v2, 3);
    }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc >= 2 && !std::strcmp(argv[1], "layout")) return layout();
    if (argc >= 2 && !std::strcmp(argv[1], "check")) return check();
    if (argc >= 2 && !std::strcmp(argv[1], "bits")) return bits();
    std::printf("usage: imu_host layout | check | bits\n");
    return 2;
}
