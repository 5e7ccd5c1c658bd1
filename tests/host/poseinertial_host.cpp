// poseinertial_host.cpp — stand-alone host program over csrc/poseinertial_common.h (test-only).
//   poseinertial_host layout      prints sizeof / offsetof of the osg_pio_* and osg_pose_inertial_* structs of
//                                 include/osg_ba.h, for the ctypes mirrors
//   poseinertial_host check       runs the host side of osg_pose_inertial_optimization without a device: every
//                                 argument check, the information matrices against their defining identities, and
//                                 the packing of the kernel's per-problem block; prints "ok"
//   poseinertial_host bits        prints the raw bytes, as hex, of info9, info_g and info_a of two fixed covariances,
//                                 for tests/golden/poseinertial_host_bits.txt
//   poseinertial_host info FILE   FILE holds C and C_rw (2 x 225 float32); prints info9, info_g, info_a
// Plain host C++: tests/test_poseinertial.py builds it with -fsanitize=address,undefined and runs it directly.
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "poseinertial_common.h"

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
    SZ(osg_pio_state);
    OFF(osg_pio_state, Rwb), OFF(osg_pio_state, twb), OFF(osg_pio_state, v), OFF(osg_pio_state, bg), OFF(osg_pio_state, ba);
    SZ(osg_pio_camera);
    OFF(osg_pio_camera, cam), OFF(osg_pio_camera, Rcw), OFF(osg_pio_camera, tcw), OFF(osg_pio_camera, Rcb);
    OFF(osg_pio_camera, tcb), OFF(osg_pio_camera, tbc);
    SZ(osg_pio_preintegrated);
    OFF(osg_pio_preintegrated, dR), OFF(osg_pio_preintegrated, dV), OFF(osg_pio_preintegrated, dP);
    OFF(osg_pio_preintegrated, JRg), OFF(osg_pio_preintegrated, JVg), OFF(osg_pio_preintegrated, JVa);
    OFF(osg_pio_preintegrated, JPg), OFF(osg_pio_preintegrated, JPa), OFF(osg_pio_preintegrated, b);
    OFF(osg_pio_preintegrated, dT), OFF(osg_pio_preintegrated, C);
    SZ(osg_pio_prior);
    OFF(osg_pio_prior, Rwb), OFF(osg_pio_prior, twb), OFF(osg_pio_prior, vwb), OFF(osg_pio_prior, bg);
    OFF(osg_pio_prior, ba), OFF(osg_pio_prior, H);
    SZ(osg_pose_inertial_problem);
    OFF(osg_pose_inertial_problem, mode), OFF(osg_pose_inertial_problem, rec_init), OFF(osg_pose_inertial_problem, cur);
    OFF(osg_pose_inertial_problem, prev), OFF(osg_pose_inertial_problem, n_cams), OFF(osg_pose_inertial_problem, cams);
    OFF(osg_pose_inertial_problem, bf), OFF(osg_pose_inertial_problem, n_edges), OFF(osg_pose_inertial_problem, kind);
    OFF(osg_pose_inertial_problem, xw), OFF(osg_pose_inertial_problem, obs), OFF(osg_pose_inertial_problem, inv_sigma2);
    OFF(osg_pose_inertial_problem, track_depth), OFF(osg_pose_inertial_problem, preint);
    OFF(osg_pose_inertial_problem, C_rw), OFF(osg_pose_inertial_problem, prior);
    SZ(osg_pose_inertial_result);
    OFF(osg_pose_inertial_result, state), OFF(osg_pose_inertial_result, outlier), OFF(osg_pose_inertial_result, n_inliers);
    OFF(osg_pose_inertial_result, rounds_run), OFF(osg_pose_inertial_result, iterations);
    OFF(osg_pose_inertial_result, solve_failed), OFF(osg_pose_inertial_result, recovered);
    OFF(osg_pose_inertial_result, H), OFF(osg_pose_inertial_result, edge_chi2);
    return 0;
}

// a covariance like the preintegration's: diagonal variances over nine decades with a little coupling
static void make_C(float *C, unsigned seed)
{
    std::srand(seed);
    double M[15][15], var[15];
    for (int i = 0; i < 15; i++) {
        var[i] = std::pow(10.0, -6.0 - (i % 5));
        for (int j = 0; j < 15; j++) M[i][j] = (i == j ? 1.0 : 0.0) + 0.05 * (std::rand() / (double)RAND_MAX - 0.5);
    }
    for (int i = 0; i < 15; i++)
        for (int j = 0; j < 15; j++) {
            double s = 0;
            for (int k = 0; k < 15; k++) s += M[i][k] * var[k] * M[j][k];
            C[i * 15 + j] = (float)s;
        }
}

static int check()
{
    // ---- argument checks: each refuses before anything is read past the struct
    std::vector<int8_t> kind = {OSG_EDGE_MONO, OSG_EDGE_STEREO, OSG_EDGE_MONO};
    std::vector<double> xw(9, 1.0), obs(9, 2.0);
    std::vector<float> w(3, 1.f), depth(3, 5.f), Crw(225);
    osg_pio_preintegrated pre;
    std::memset(&pre, 0, sizeof pre);
    make_C(pre.C, 1);
    make_C(Crw.data(), 2);
    osg_pio_prior prior;
    std::memset(&prior, 0, sizeof prior);
    osg_pose_inertial_problem p;
    std::memset(&p, 0, sizeof p);
    p.mode = OSG_PIO_LAST_KEYFRAME;
    p.n_cams = 1;
    p.n_edges = 3;
    p.kind = kind.data(), p.xw = xw.data(), p.obs = obs.data(), p.inv_sigma2 = w.data(), p.track_depth = depth.data();
    p.preint = &pre, p.C_rw = Crw.data();
    const char *why = nullptr;
    EXPECT(osgpio::check(&p, &why) == 0);
    EXPECT(osgpio::check(nullptr, &why) == OSG_E_INVALID);
    osg_pose_inertial_problem q = p;
    q.mode = 2;
    EXPECT(osgpio::check(&q, &why) == OSG_E_INVALID);
    q = p, q.mode = -1;
    EXPECT(osgpio::check(&q, &why) == OSG_E_INVALID);
    q = p, q.n_cams = 0;
    EXPECT(osgpio::check(&q, &why) == OSG_E_INVALID);
    q = p, q.n_cams = 3;
    EXPECT(osgpio::check(&q, &why) == OSG_E_INVALID);
    q = p, q.n_edges = -1;
    EXPECT(osgpio::check(&q, &why) == OSG_E_INVALID);
    q = p, q.n_edges = osgpio::MAX_EDGES + 1;
    EXPECT(osgpio::check(&q, &why) == OSG_E_INVALID);
    q = p, q.preint = nullptr;
    EXPECT(osgpio::check(&q, &why) == OSG_E_INVALID);
    q = p, q.C_rw = nullptr;
    EXPECT(osgpio::check(&q, &why) == OSG_E_INVALID);
    q = p, q.kind = nullptr;
    EXPECT(osgpio::check(&q, &why) == OSG_E_INVALID);
    q = p, q.xw = nullptr;
    EXPECT(osgpio::check(&q, &why) == OSG_E_INVALID);
    q = p, q.obs = nullptr;
    EXPECT(osgpio::check(&q, &why) == OSG_E_INVALID);
    q = p, q.inv_sigma2 = nullptr;
    EXPECT(osgpio::check(&q, &why) == OSG_E_INVALID);
    q = p, q.track_depth = nullptr;
    EXPECT(osgpio::check(&q, &why) == OSG_E_INVALID);
    q = p, q.mode = OSG_PIO_LAST_FRAME;  // no prior
    EXPECT(osgpio::check(&q, &why) == OSG_E_INVALID);
    q.prior = &prior;
    EXPECT(osgpio::check(&q, &why) == 0);
    std::vector<int8_t> k2 = kind;
    k2[2] = OSG_EDGE_BODY;  // a right-camera edge with one camera
    q = p, q.kind = k2.data();
    EXPECT(osgpio::check(&q, &why) == OSG_E_INVALID);
    q.n_cams = 2;
    EXPECT(osgpio::check(&q, &why) == 0);
    k2[1] = 3;
    EXPECT(osgpio::check(&q, &why) == OSG_E_INVALID);
    k2[1] = -1;
    EXPECT(osgpio::check(&q, &why) == OSG_E_INVALID);
    q = p, q.n_edges = 0, q.kind = nullptr, q.xw = nullptr, q.obs = nullptr, q.inv_sigma2 = nullptr, q.track_depth = nullptr;
    EXPECT(osgpio::check(&q, &why) == 0);

    // ---- information matrices: Info C9 = I to rounding, symmetric; the 3 x 3 inverses
    double info9[81], ig[9], ia[9];
    osgpio::informations(pre.C, Crw.data(), info9, ig, ia);
    double scale = 0;
    for (int i = 0; i < 81; i++) scale = std::fmax(scale, std::fabs(info9[i]));
    for (int i = 0; i < 9; i++)
        for (int j = 0; j < 9; j++) {
            double s = 0;
            for (int k = 0; k < 9; k++) s += info9[i * 9 + k] * (double)pre.C[k * 15 + j];
            EXPECT(std::fabs(s - (i == j ? 1.0 : 0.0)) < 1e-6);
            EXPECT(std::fabs(info9[i * 9 + j] - info9[j * 9 + i]) <= 1e-12 * scale);
        }
    for (int o = 0; o < 2; o++)
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) {
                const double *inv = o == 0 ? ig : ia;
                const int at = o == 0 ? 9 : 12;
                double s = 0;
                for (int k = 0; k < 3; k++) s += inv[i * 3 + k] * (double)Crw[(at + k) * 15 + at + j];
                EXPECT(std::fabs(s - (i == j ? 1.0 : 0.0)) < 1e-9);
            }
    osgpio::informations(pre.C, Crw.data(), nullptr, nullptr, nullptr);  // every output is optional
    // an eigenvalue of the information below 1e-12 is cut to 0: C = 1e13 I
    osg_pio_preintegrated big = pre;
    for (int i = 0; i < 225; i++) big.C[i] = (i / 15 == i % 15) ? 1e13f : 0.f;
    osgpio::informations(big.C, nullptr, info9, nullptr, nullptr);
    for (int i = 0; i < 81; i++) EXPECT(info9[i] == 0.0);

    // ---- packing
    q = p, q.mode = OSG_PIO_LAST_FRAME, q.prior = &prior, q.rec_init = 7, q.bf = 47.5;
    prior.H[224] = 3.0;
    pre.dT = 0.05f, pre.b[5] = 0.25f, pre.JPa[8] = -1.5f;
    q.cur.twb[2] = 4.0, q.prev.ba[2] = 5.0, q.cams[0].tbc[2] = 6.0;
    osgpio::ProbDev d;
    osgpio::pack(q, 17, d);
    EXPECT(d.mode == OSG_PIO_LAST_FRAME && d.rec_init == 1 && d.n_cams == 1 && d.n_edges == 3 && d.edge_off == 17);
    EXPECT(d.bf == 47.5 && d.dT == 0.05f && d.b[5] == 0.25f && d.JPa[8] == -1.5f);
    EXPECT(d.cur.twb[2] == 4.0 && d.prev.ba[2] == 5.0 && d.cams[0].tbc[2] == 6.0 && d.cams[1].tbc[2] == 0.0);
    EXPECT(d.prior.H[224] == 3.0);
    EXPECT(d.info_rw[0] == ig[0] && d.info_rw[3 * 6 + 3] == ia[0] && d.info_rw[3] == 0.0 && d.info_rw[5 * 6 + 5] == ia[8]);
    osgpio::pack(p, 0, d);  // LastKeyFrame: no prior to copy
    EXPECT(d.prior.H[224] == 0.0);
    std::printf("ok\n");
    return 0;
}

static int info(const char *path)
{
    std::vector<float> buf(450);
    FILE *f = std::fopen(path, "rb");
    if (!f || std::fread(buf.data(), sizeof(float), 450, f) != 450) return 2;
    std::fclose(f);
    double out[99];
    osgpio::informations(buf.data(), buf.data() + 225, out, out + 81, out + 90);
    for (double v : out) std::printf("%.17g\n", v);
    return 0;
}

static int bits()
{
    // covariances like make_C's, from a generator and powers that do not depend on the C library
    uint32_t lcg = 2024u;
    auto next = [&lcg]() {
        lcg = lcg * 1664525u + 1013904223u;
        return (double)(lcg >> 8) / 16777216.0 - 0.5;
    };
    for (int which = 0; which < 2; which++) {
        std::vector<float> C(450);
        for (int m = 0; m < 2; m++) {
            double M[15][15], var[15];
            for (int i = 0; i < 15; i++) {
                var[i] = 1e-6;
                for (int k = 0; k < (i + which) % 5; k++) var[i] /= 10.0;
                for (int j = 0; j < 15; j++) M[i][j] = (i == j ? 1.0 : 0.0) + 0.05 * next();
            }
            for (int i = 0; i < 15; i++)
                for (int j = 0; j < 15; j++) {
                    double s = 0;
                    for (int k = 0; k < 15; k++) s += M[i][k] * var[k] * M[j][k];
                    C[225 * m + i * 15 + j] = (float)s;
                }
        }
        double out[99];
        osgpio::informations(C.data(), C.data() + 225, out, out + 81, out + 90);
        for (int i = 0; i < 99; i++) {
            uint64_t u;
            std::memcpy(&u, out + i, 8);
            std::printf("%016llx%c", (unsigned long long)u, i % 9 == 8 ? '\n' : ' ');
        }
    }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc >= 2 && !std::strcmp(argv[1], "layout")) return layout();
    if (argc >= 2 && !std::strcmp(argv[1], "check")) return check();
    if (argc >= 2 && !std::strcmp(argv[1], "bits")) return bits();
    if (argc >= 3 && !std::strcmp(argv[1], "info")) return info(argv[2]);
    std::printf("usage: poseinertial_host layout | check | bits | info FILE\n");
    return 2;
}
