// frustum_host.cpp — stand-alone host program over csrc/frustum_common.h and osg_packer::reserve (test-only).
//   frustum_host layout   prints sizeof / offsetof of the osg_frustum_* structs of include/osg.h, for the ctypes mirrors
//   frustum_host check    runs the host side of osg_frustum / osg_search_local_points without a device: the
//                         argument checks, the block layout, packing into and unpacking from buffers of exactly the
//                         computed size, the kernel arguments' addresses, and a packer with reserved regions;
//                         prints "ok"
// Plain host C++ (the HIP headers are only declarations here): tests/test_frustum.py builds it with
// -fsanitize=address,undefined and runs it directly.
#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "frustum_common.h"
#include "match_common.h"

// the two library functions the headers call (runtime.hip); the messages are not under test here
int osg_set_error(osg_ctx *, int code, const char *, ...) { return code; }
void osg_parallel_run(int n, int, void (*fn)(void *, int), void *arg)
{
    for (int i = 0; i < n; i++) fn(arg, i);
}

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
    SZ(osg_frustum_camera);
    OFF(osg_frustum_camera, R), OFF(osg_frustum_camera, t), OFF(osg_frustum_camera, c);
    OFF(osg_frustum_camera, cam_type), OFF(osg_frustum_camera, cam);
    SZ(osg_frustum_frame);
    OFF(osg_frustum_frame, two_cam), OFF(osg_frustum_frame, cam), OFF(osg_frustum_frame, min_x);
    OFF(osg_frustum_frame, max_x), OFF(osg_frustum_frame, min_y), OFF(osg_frustum_frame, max_y);
    OFF(osg_frustum_frame, mbf), OFF(osg_frustum_frame, log_scale_factor), OFF(osg_frustum_frame, n_levels);
    SZ(osg_frustum_points);
    OFF(osg_frustum_points, n), OFF(osg_frustum_points, pos), OFF(osg_frustum_points, normal);
    OFF(osg_frustum_points, max_dist), OFF(osg_frustum_points, min_dist), OFF(osg_frustum_points, candidate);
    OFF(osg_frustum_points, prev_depth);
    SZ(osg_frustum_result);
    OFF(osg_frustum_result, status), OFF(osg_frustum_result, proj_x), OFF(osg_frustum_result, proj_y);
    OFF(osg_frustum_result, proj_xr), OFF(osg_frustum_result, view_cos), OFF(osg_frustum_result, depth);
    OFF(osg_frustum_result, level), OFF(osg_frustum_result, n_to_match);
    SZ(osg_local_points);
    OFF(osg_local_points, pts), OFF(osg_local_points, mp_id), OFF(osg_local_points, desc);
    OFF(osg_local_points, has_obs);
    return 0;
}

static int check_one(int n, bool rig, bool with_prev)
{
    std::vector<float> pos(3 * (size_t)n), nrm(3 * (size_t)n), maxd(n), mind(n), prev(n);
    std::vector<uint8_t> cand(n);
    for (int i = 0; i < n; i++) {
        for (int k = 0; k < 3; k++) pos[3 * i + k] = 10.f * i + k, nrm[3 * i + k] = -(10.f * i + k);
        maxd[i] = 100.f + i, mind[i] = 200.f + i, prev[i] = 300.f + i, cand[i] = i & 1;
    }
    osg_frustum_points pts{};
    pts.n = n;
    pts.pos = pos.data(), pts.normal = nrm.data(), pts.max_dist = maxd.data(), pts.min_dist = mind.data();
    pts.candidate = cand.data(), pts.prev_depth = with_prev ? prev.data() : nullptr;
    osg_frustum_frame f{};
    f.two_cam = rig, f.n_levels = 8, f.cam[1].cam_type = 1;
    EXPECT(osg_frustum_check_args(nullptr, &f, &pts, 0) == OSG_OK);

    const FrBlock L = osg_frustum_block(n, rig);
    EXPECT(L.in_end % 256 == 0 && L.total % 256 == 0 && L.total >= L.in_end);
    std::vector<char> in(L.in_end), out(L.total - L.in_end);  // exactly the computed sizes
    osg_frustum_pack_inputs(in.data(), L, &pts);
    for (int i = 0; i < n; i++) {
        EXPECT(((const float *)(in.data() + L.py))[i] == pos[3 * i + 1]);
        EXPECT(((const float *)(in.data() + L.nz))[i] == nrm[3 * i + 2]);
        EXPECT(((const float *)(in.data() + L.prev_depth))[i] == (with_prev ? prev[i] : 0.f));
        EXPECT(((const uint8_t *)(in.data() + L.cand))[i] == cand[i]);
    }
    if (n == 0) return 0;  // empty blocks: no lane is active, no address is used
    // the kernel's addresses stay inside the two buffers
    const FrProb P = osg_frustum_prob(&f, n, 0.5f, L, in.data(), out.data());
    const char *i0 = in.data(), *i1 = i0 + in.size(), *o0 = out.data(), *o1 = o0 + out.size();
    const size_t n4 = sizeof(float) * (size_t)n;
    for (const float *p : {P.px, P.py, P.pz, P.nx, P.ny, P.nz, P.maxd, P.mind, P.prev_depth})
        EXPECT((const char *)p >= i0 && (const char *)p + n4 <= i1);
    EXPECT((const char *)P.cand >= i0 && (const char *)P.cand + n <= i1);
    for (int c = 0; c < 2; c++) {
        const bool have = c == 0 || rig;
        EXPECT((P.status[c] != nullptr) == have && (P.level[c] != nullptr) == have);
        if (!have) continue;
        for (const void *p : {(const void *)P.proj_x[c], (const void *)P.proj_y[c], (const void *)P.view_cos[c],
                              (const void *)P.depth[c], (const void *)P.level[c]})
            EXPECT((const char *)p >= o0 && (const char *)p + n4 <= o1);
        for (const uint8_t *p : {P.status[c], P.in_view[c]}) EXPECT((const char *)p >= o0 && (const char *)p + n <= o1);
    }
    EXPECT((P.proj_xr != nullptr) == !rig);
    // results: what a kernel would have written, back into arrays of exactly n elements
    for (size_t k = 0; k < out.size(); k++) out[k] = (char)(k * 7);
    std::vector<uint8_t> st0(n), st1(n);
    std::vector<float> x0(n), x1(n), xr(n);
    std::vector<int32_t> l0(n), l1(n);
    osg_frustum_result r{};
    r.status[0] = st0.data(), r.status[1] = st1.data(), r.proj_x[0] = x0.data(), r.proj_x[1] = x1.data();
    r.proj_xr = xr.data(), r.level[0] = l0.data(), r.level[1] = l1.data();
    osg_frustum_unpack(out.data(), L, n, rig, &r);
    if (n > 0) EXPECT(std::memcmp(l0.data(), out.data() + (L.level[0] - L.in_end), n4) == 0);
    if (n > 0 && rig) EXPECT(std::memcmp(st1.data(), out.data() + (L.status[1] - L.in_end), n) == 0);
    return 0;
}

static int check()
{
    for (int n : {0, 1, 63, 64, 65, 257})
        for (int rig = 0; rig < 2; rig++)
            if (check_one(n, rig != 0, (n & 1) != 0)) return 1;
    // what the entry points refuse before any launch
    osg_frustum_frame f{};
    f.n_levels = 8;
    osg_frustum_points pts{};
    EXPECT(osg_frustum_check_args(nullptr, &f, &pts, 0) == OSG_OK);  // n == 0: no arrays needed
    EXPECT(osg_frustum_check_args(nullptr, nullptr, &pts, 0) == OSG_E_INVALID);
    EXPECT(osg_frustum_check_args(nullptr, &f, nullptr, 0) == OSG_E_INVALID);
    pts.n = 4;
    EXPECT(osg_frustum_check_args(nullptr, &f, &pts, 0) == OSG_E_INVALID);  // null arrays
    pts.n = -1;
    EXPECT(osg_frustum_check_args(nullptr, &f, &pts, 0) == OSG_E_INVALID);
    pts.n = (1 << 24) + 1;
    EXPECT(osg_frustum_check_args(nullptr, &f, &pts, 0) == OSG_E_INVALID);
    pts.n = 0;
    f.n_levels = 0;
    EXPECT(osg_frustum_check_args(nullptr, &f, &pts, 0) == OSG_E_INVALID);
    f.n_levels = 8, f.cam[0].cam_type = 2;
    EXPECT(osg_frustum_check_args(nullptr, &f, &pts, 0) == OSG_E_INVALID);
    f.cam[0].cam_type = 0, f.cam[1].cam_type = 7;
    EXPECT(osg_frustum_check_args(nullptr, &f, &pts, 0) == OSG_OK);  // not a rig: camera 1 is not read
    f.two_cam = 1;
    EXPECT(osg_frustum_check_args(nullptr, &f, &pts, 0) == OSG_E_INVALID);

    // a packer with reserved regions between copied items: the fill leaves them alone
    osg_packer pk;
    const char a[5] = {1, 2, 3, 4, 5}, b[3] = {6, 7, 8};
    const size_t oa = pk.add(a, sizeof a), r1 = pk.reserve(300), ob = pk.add(b, sizeof b), r0 = pk.reserve(0);
    const size_t r2 = pk.reserve(1);
    EXPECT(oa == 0 && r1 == 256 && ob == 768 && r0 == SIZE_MAX && r2 == 1024 && pk.total == 1280);
    std::vector<char> block(pk.total, (char)0x55);
    pk.fill(block.data());
    EXPECT(std::memcmp(block.data() + oa, a, sizeof a) == 0 && std::memcmp(block.data() + ob, b, sizeof b) == 0);
    for (size_t k = r1; k < r1 + 300; k++) EXPECT(block[k] == 0x55);
    EXPECT(block[r2] == 0x55);
    std::vector<char> block2(pk.total, (char)0x55);
    pk.fill_parallel(block2.data(), 4);
    EXPECT(block == block2);
    std::printf("ok\n");
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 2 && !std::strcmp(argv[1], "layout")) return layout();
    if (argc == 2 && !std::strcmp(argv[1], "check")) return check();
    std::fprintf(stderr, "usage: frustum_host layout|check\n");
    return 2;
}
