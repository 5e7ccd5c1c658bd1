// newpoints.hip — LocalMapping::CreateNewMapPoints on gfx950 (ref:src/LocalMapping.cc:584-933).
//
// The reference walks the neighbours one by one: after each it adds MapPoints to the current KeyFrame, and
// the next neighbour's SearchForTriangulation skips those keypoints.  Here every (KF1 keypoint, neighbour)
// is evaluated for the MapPoint state at call time, then the sequential rule is replayed on small integers:
//   1. osg_search_for_triangulation_batch (k_triang, unchanged, check_orientation = 0): the match of every
//      KF1 keypoint in every neighbour, one workgroup per pair;
//   2. k_np_eval, grid (neighbour, problem), one lane per KF1 keypoint: the triangulation or UnprojectStereo
//      of its match and every acceptance test of :649-906, in the reference's float expressions and order
//      (built with -ffp-contract=off) -> status code and x3D;
//   3. k_np_select, one workgroup per problem: the neighbours in order; the baseline skip of :595-621 with
//      the Ow1 the reference's locals would hold, the claim of a keypoint by its first accepted match, the
//      sequential-state outputs and counts.
// It is exact because in this fork no KF2 keypoint is claimed (ref:src/ORBmatcher.cc:1262) and
// CreateNewMapPoints' matcher has no orientation check (:556): a match and its tests depend on
// (keypoint, neighbour) and the call-time state alone.
//
// cos(2 * atan2(mb / 2, depth)) of :762-765 resolves to the float overloads (std::cos / std::atan2 through
// the DBoW2 header's "using namespace std"): atan2f by glibc_math.h, cosf as kb8_epipolar.h's double
// kernel rounded once.  Triangulate's JacobiSVD null vector is the smallest-eigenvalue eigenvector of the
// Gram matrix by the register Jacobi in double, as twoview.hip's k_tvr_checkrt takes it.
#include <vector>

#include "batch_io.h"
#include "kb8_epipolar.h"
#include "ransac_common.h"

namespace {

constexpr int NT = 256;
constexpr int NP_SWEEPS = 24;      // as twoview.hip
constexpr double NP_TOL = 1e-34;

// one KeyFrame on the device: osg_np_kf's values and where its arrays start in the float / int pools
struct KfDev {
    float Tcw[2][12], Ow[2][3], Rwc[9], twc[3], cam[2][8];
    float fx, fy, cx, cy, invfx, invfy, mb, mbf, median_depth;
    int32_t cam_type, n, nleft, two_cam, n_levels;
    int32_t o_x, o_y, o_ur, o_depth, o_kx, o_ky, o_scale, o_sigma;  // float pool; -1: absent
    int32_t o_oct;                                                  // int pool
};

struct ProbDev {
    int32_t kf1, first_pair, B, n1;
    int32_t out_off;    // first (b, i) element of this problem in the concatenated outputs
    int32_t claim_off;  // first element in the claimed bytes
    int32_t monocular, inertial, far_points;
    float th_far, ratio_factor;
};

struct NpArgs {
    const ProbDev *prob;
    const KfDev *kf;        // [C] current KeyFrames, then the neighbours pair by pair
    const float *fpool;
    const int32_t *ipool;
    const int32_t *match_call;  // k_triang's matches for the call-time state
    int32_t C;
    int32_t *match;
    uint8_t *status;
    float *x3d;
    uint8_t *skipped;
    int32_t *n_created;
    uint8_t *claimed;
};

__device__ __forceinline__ float norm3(float x, float y, float z) { return sqrtf(x * x + y * y + z * z); }

// GeometricCamera::unprojectEig
__device__ __forceinline__ void unproject_cam(int kb8cam, const float *p, float u, float v, float r[3])
{
    if (kb8cam) {
        kb8::unproject(p, u, v, r);
    } else {  // ref:src/CameraModels/Pinhole.cpp:97-102
        r[0] = (u - p[2]) / p[0];
        r[1] = (v - p[3]) / p[1];
        r[2] = 1.f;
    }
}

// GeometricCamera::project(cv::Point3f)
__device__ __forceinline__ void project_cam(int kb8cam, const float *p, float x, float y, float z, float uv[2])
{
    if (kb8cam) {
        const float X[3] = {x, y, z};
        kb8::project(p, X, uv);
    } else {  // ref:src/CameraModels/Pinhole.cpp:39-43
        uv[0] = p[0] * x / z + p[2];
        uv[1] = p[1] * y / z + p[3];
    }
}

// cos(2 * atan2(mb / 2, depth)) in float, :762 / :765
__device__ __forceinline__ float cos_stereo(float mb, float depth)
{
    const float a = 2 * osgm::atan2f_fd(mb / 2, depth);
    double s, c;
    kb8::sincos_d((double)a, s, c);  // a in [0, 2 pi): within the kernel's reduction range
    return (float)c;
}

// KeyFrame::UnprojectStereo, ref:src/KeyFrame.cc:921-940
__device__ __forceinline__ bool unproject_stereo(const KfDev &K, const float *fp, int i, float X[3])
{
    const float z = fp[K.o_depth + i];
    if (!(z > 0)) return false;
    const float u = fp[K.o_kx + i], v = fp[K.o_ky + i];
    const float x = (u - K.cx) * z * K.invfx;
    const float y = (v - K.cy) * z * K.invfy;
#pragma unroll
    for (int r = 0; r < 3; r++) X[r] = (K.Rwc[3 * r] * x + K.Rwc[3 * r + 1] * y + K.Rwc[3 * r + 2] * z) + K.twc[r];
    return true;
}

__global__ __launch_bounds__(NT) void k_np_eval(const NpArgs A)
{
    const ProbDev P = A.prob[blockIdx.y];
    const int b = blockIdx.x;
    if (b >= P.B) return;
    const KfDev &K1 = A.kf[P.kf1];
    const KfDev &K2 = A.kf[A.C + P.first_pair + b];
    const float *fp = A.fpool;
    const int32_t *ip = A.ipool;
    const bool rig = K1.two_cam && K2.two_cam;
    for (int i = threadIdx.x; i < P.n1; i += NT) {
        const size_t e = (size_t)P.out_off + (size_t)b * P.n1 + i;
        int idx2 = A.match_call[e];
        if (idx2 >= K2.n) idx2 = -1;
        uint8_t st = OSG_NP_NONE;
        float X[3] = {0.f, 0.f, 0.f};
        bool have_x = false;
        if (idx2 >= 0) {
            const float kp1x = fp[K1.o_x + i], kp1y = fp[K1.o_y + i];
            const float kp2x = fp[K2.o_x + idx2], kp2y = fp[K2.o_y + idx2];
            const float kp1_ur = K1.o_ur >= 0 ? fp[K1.o_ur + i] : -1.f;
            const float kp2_ur = K2.o_ur >= 0 ? fp[K2.o_ur + idx2] : -1.f;
            const bool stereo1 = !K1.two_cam && kp1_ur >= 0, stereo2 = !K2.two_cam && kp2_ur >= 0;
            const int r1 = rig && !(K1.nleft == -1 || i < K1.nleft), r2 = rig && !(K2.nleft == -1 || idx2 < K2.nleft);
            const float *T1 = K1.Tcw[r1], *T2 = K2.Tcw[r2];  // :683-738
            const float *O1 = K1.Ow[r1], *O2 = K2.Ow[r2];
            const float *c1 = K1.cam[r1], *c2 = K2.cam[r2];
            float xn1[3], xn2[3];
            unproject_cam(K1.cam_type, c1, kp1x, kp1y, xn1);
            unproject_cam(K2.cam_type, c2, kp2x, kp2y, xn2);
            float ray1[3], ray2[3];  // Rwc = Rcw^T
#pragma unroll
            for (int r = 0; r < 3; r++) {
                ray1[r] = (T1[r] * xn1[0] + T1[4 + r] * xn1[1]) + T1[8 + r] * xn1[2];
                ray2[r] = (T2[r] * xn2[0] + T2[4 + r] * xn2[1]) + T2[8 + r] * xn2[2];
            }
            const float cosRays = ((ray1[0] * ray2[0] + ray1[1] * ray2[1]) + ray1[2] * ray2[2]) /
                                  (norm3(ray1[0], ray1[1], ray1[2]) * norm3(ray2[0], ray2[1], ray2[2]));
            float cosS1 = cosRays + 1, cosS2 = cosS1;
            if (stereo1) cosS1 = cos_stereo(K1.mb, fp[K1.o_depth + i]);
            else if (stereo2) cosS2 = cos_stereo(K2.mb, fp[K2.o_depth + idx2]);
            const float cosS = fminf(cosS1, cosS2);
            bool good = false, point_stereo = false;
            int way = 0;  // 1 triangulate, 2 UnprojectStereo KF1, 3 UnprojectStereo KF2
            if (cosRays < cosS && cosRays > 0 &&
                (stereo1 || stereo2 || ((double)cosRays < 0.9996 && P.inertial) || ((double)cosRays < 0.9998 && !P.inertial)))
                way = 1;
            else if (stereo1 && cosS1 < cosS2)
                way = 2;
            else if (stereo2 && cosS2 < cosS1)
                way = 3;
            if (way == 1) {  // GeometricTools::Triangulate, ref:src/GeometricTools.cc:62-89
                float M[4][4];
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    M[0][j] = xn1[0] * T1[8 + j] - T1[j];
                    M[1][j] = xn1[1] * T1[8 + j] - T1[4 + j];
                    M[2][j] = xn2[0] * T2[8 + j] - T2[j];
                    M[3][j] = xn2[1] * T2[8 + j] - T2[4 + j];
                }
                double G[4][4], E[4][4];
#pragma unroll
                for (int a = 0; a < 4; a++)
#pragma unroll
                    for (int c = 0; c < 4; c++)
                        G[a][c] = (double)M[0][a] * M[0][c] + (double)M[1][a] * M[1][c] + (double)M[2][a] * M[2][c] +
                                  (double)M[3][a] * M[3][c];
                jacobi_sym<double, 4>(G, E, NP_SWEEPS, NP_TOL);
                int m = 0;
                double lm = G[0][0];
#pragma unroll
                for (int a = 1; a < 4; a++)
                    if (G[a][a] < lm) lm = G[a][a], m = a;
                float xh[4];
#pragma unroll
                for (int a = 0; a < 4; a++) xh[a] = (float)(m == 0 ? E[a][0] : m == 1 ? E[a][1] : m == 2 ? E[a][2] : E[a][3]);
                if (xh[3] != 0.f) {
                    good = true;
                    X[0] = xh[0] / xh[3], X[1] = xh[1] / xh[3], X[2] = xh[2] / xh[3];
                }
            } else if (way == 2) {
                point_stereo = true;
                good = unproject_stereo(K1, fp, i, X);
            } else if (way == 3) {
                point_stereo = true;
                good = unproject_stereo(K2, fp, idx2, X);
            }
            if (way == 0) {
                st = OSG_NP_LOW_PARALLAX;
            } else if (!good) {
                st = OSG_NP_NO_POINT;
            } else {
                have_x = true;
                const int oct1 = ip[K1.o_oct + i], oct2 = ip[K2.o_oct + idx2];
                const float z1 = ((T1[8] * X[0] + T1[9] * X[1]) + T1[10] * X[2]) + T1[11];
                const float z2 = ((T2[8] * X[0] + T2[9] * X[1]) + T2[10] * X[2]) + T2[11];
                st = OSG_NP_CREATED;
                if (z1 <= 0) st = OSG_NP_Z1;
                else if (z2 <= 0) st = OSG_NP_Z2;
                if (st == OSG_NP_CREATED) {  // :825-856
                    const float sig1 = fp[K1.o_sigma + oct1];
                    const float x1 = ((T1[0] * X[0] + T1[1] * X[1]) + T1[2] * X[2]) + T1[3];
                    const float y1 = ((T1[4] * X[0] + T1[5] * X[1]) + T1[6] * X[2]) + T1[7];
                    const float invz1 = (float)(1.0 / (double)z1);
                    if (!stereo1) {
                        float uv[2];
                        project_cam(K1.cam_type, c1, x1, y1, z1, uv);
                        const float ex = uv[0] - kp1x, ey = uv[1] - kp1y;
                        if ((double)(ex * ex + ey * ey) > 5.991 * (double)sig1) st = OSG_NP_REPROJ1;
                    } else {
                        const float u1 = K1.fx * x1 * invz1 + K1.cx;
                        const float u1_r = u1 - K1.mbf * invz1;
                        const float v1 = K1.fy * y1 * invz1 + K1.cy;
                        const float ex = u1 - kp1x, ey = v1 - kp1y, er = u1_r - kp1_ur;
                        if ((double)((ex * ex + ey * ey) + er * er) > 7.8 * (double)sig1) st = OSG_NP_REPROJ1;
                    }
                }
                if (st == OSG_NP_CREATED) {  // :858-882, mpCurrentKeyFrame->mbf kept (:875)
                    const float sig2 = fp[K2.o_sigma + oct2];
                    const float x2 = ((T2[0] * X[0] + T2[1] * X[1]) + T2[2] * X[2]) + T2[3];
                    const float y2 = ((T2[4] * X[0] + T2[5] * X[1]) + T2[6] * X[2]) + T2[7];
                    const float invz2 = (float)(1.0 / (double)z2);
                    if (!stereo2) {
                        float uv[2];
                        project_cam(K2.cam_type, c2, x2, y2, z2, uv);
                        const float ex = uv[0] - kp2x, ey = uv[1] - kp2y;
                        if ((double)(ex * ex + ey * ey) > 5.991 * (double)sig2) st = OSG_NP_REPROJ2;
                    } else {
                        const float u2 = K2.fx * x2 * invz2 + K2.cx;
                        const float u2_r = u2 - K1.mbf * invz2;
                        const float v2 = K2.fy * y2 * invz2 + K2.cy;
                        const float ex = u2 - kp2x, ey = v2 - kp2y, er = u2_r - kp2_ur;
                        if ((double)((ex * ex + ey * ey) + er * er) > 7.8 * (double)sig2) st = OSG_NP_REPROJ2;
                    }
                }
                if (st == OSG_NP_CREATED) {  // :884-906
                    const float dist1 = norm3(X[0] - O1[0], X[1] - O1[1], X[2] - O1[2]);
                    const float dist2 = norm3(X[0] - O2[0], X[1] - O2[1], X[2] - O2[2]);
                    if (dist1 == 0 || dist2 == 0) {
                        st = OSG_NP_ZERO_DIST;
                    } else if (P.far_points && (dist1 >= P.th_far || dist2 >= P.th_far)) {
                        st = OSG_NP_FAR;
                    } else {
                        const float ratioDist = dist2 / dist1;
                        const float ratioOctave = fp[K1.o_scale + oct1] / fp[K2.o_scale + oct2];
                        if (ratioDist * P.ratio_factor < ratioOctave || ratioDist > ratioOctave * P.ratio_factor)
                            st = OSG_NP_SCALE;
                    }
                }
            }
            if (point_stereo) st |= OSG_NP_STEREO_BIT;
        }
        A.match[e] = idx2;
        A.status[e] = st;
        A.x3d[3 * e] = have_x ? X[0] : 0.f;
        A.x3d[3 * e + 1] = have_x ? X[1] : 0.f;
        A.x3d[3 * e + 2] = have_x ? X[2] : 0.f;
    }
}

// The reference's neighbour loop on k_np_eval's outputs, in place.  Lane t owns the keypoints t, t + NT, ...
// for every neighbour, so a claimed byte is only ever touched by one lane.
__global__ __launch_bounds__(NT) void k_np_select(const NpArgs A)
{
    const ProbDev P = A.prob[blockIdx.x];
    const KfDev &K1 = A.kf[P.kf1];
    __shared__ float s_ow1[3];
    __shared__ int s_skip, s_last, s_cnt;
    const int tid = threadIdx.x;
    uint8_t *claimed = A.claimed + P.claim_off;
    for (int i = tid; i < P.n1; i += NT) claimed[i] = 0;
    if (tid == 0) {
        s_ow1[0] = K1.Ow[0][0];
        s_ow1[1] = K1.Ow[0][1];
        s_ow1[2] = K1.Ow[0][2];
    }
    __syncthreads();
    for (int b = 0; b < P.B; b++) {
        const KfDev &K2 = A.kf[A.C + P.first_pair + b];
        if (tid == 0) {  // :595-621
            const float dx = K2.Ow[0][0] - s_ow1[0], dy = K2.Ow[0][1] - s_ow1[1], dz = K2.Ow[0][2] - s_ow1[2];
            const float baseline = norm3(dx, dy, dz);
            bool skip;
            if (!P.monocular) {
                skip = baseline < K2.mb;
            } else {
                const float ratioBaselineDepth = baseline / K2.median_depth;
                skip = (double)ratioBaselineDepth < 0.01;
            }
            s_skip = skip;
            s_last = -1;
            s_cnt = 0;
        }
        __syncthreads();
        const bool skip = s_skip;
        int last = -1, cnt = 0;
        for (int i = tid; i < P.n1; i += NT) {
            const size_t e = (size_t)P.out_off + (size_t)b * P.n1 + i;
            if (skip || claimed[i]) {
                if (A.match[e] >= 0) {
                    A.match[e] = -1;
                    A.status[e] = OSG_NP_NONE;
                    A.x3d[3 * e] = A.x3d[3 * e + 1] = A.x3d[3 * e + 2] = 0.f;
                }
                continue;
            }
            if (A.match[e] < 0) continue;
            last = i;  // ascending within the lane
            if ((A.status[e] & 0x7f) == OSG_NP_CREATED) {
                claimed[i] = 1;
                cnt++;
            }
        }
        if (last >= 0) atomicMax(&s_last, last);
        if (cnt) atomicAdd(&s_cnt, cnt);
        __syncthreads();
        if (tid == 0) {
            A.skipped[P.first_pair + b] = skip;
            A.n_created[P.first_pair + b] = s_cnt;
            // a rig's Ow1 stays that of the last match of vMatchedIndices, accepted or not (:683-728)
            if (K1.two_cam && K2.two_cam && s_last >= 0) {
                const int r1 = !(K1.nleft == -1 || s_last < K1.nleft);
                s_ow1[0] = K1.Ow[r1][0];
                s_ow1[1] = K1.Ow[r1][1];
                s_ow1[2] = K1.Ow[r1][2];
            }
        }
        __syncthreads();
    }
}

int check_problem(osg_ctx *ctx, const osg_newpoints_problem *p, int c)
{
    OSG_REQUIRE(ctx, p, "problem %d: null", c);
    OSG_REQUIRE(ctx, p->kf1.n >= 0 && p->n_neigh >= 0, "problem %d: negative count", c);
    OSG_REQUIRE(ctx, p->n_neigh <= OSG_NEWPOINTS_MAX_NEIGHBOURS, "problem %d: %d neighbours (limit %d)", c, p->n_neigh,
                OSG_NEWPOINTS_MAX_NEIGHBOURS);
    OSG_REQUIRE(ctx, p->n_neigh == 0 || (p->kf2 && p->g2 && p->geom), "problem %d: null neighbour arrays", c);
    for (int b = -1; b < p->n_neigh; b++) {
        const osg_kf_side *s = b < 0 ? &p->kf1 : &p->kf2[b];
        const osg_np_kf *g = b < 0 ? &p->g1 : &p->g2[b];
        OSG_REQUIRE(ctx, s->n >= 0, "problem %d: KeyFrame %d n", c, b);
        OSG_REQUIRE(ctx, s->nleft == -1 || (s->nleft >= 0 && s->nleft <= s->n), "problem %d: KeyFrame %d nleft", c, b);
        OSG_REQUIRE(ctx, s->n == 0 || (s->desc && s->kp_x && s->kp_y && s->kp_angle && s->kp_octave && s->has_mp),
                    "problem %d: KeyFrame %d keypoint arrays", c, b);
        OSG_REQUIRE(ctx, s->n_levels > 0 && s->n_levels <= 128 && s->level_sigma2 && s->scale_factors,
                    "problem %d: KeyFrame %d level tables", c, b);
        for (int i = 0; i < s->n; i++)
            OSG_REQUIRE(ctx, s->kp_octave[i] >= 0 && s->kp_octave[i] < s->n_levels, "problem %d: KeyFrame %d octave[%d]", c,
                        b, i);
        OSG_REQUIRE(ctx, g->cam_type == 0 || g->cam_type == 1, "problem %d: KeyFrame %d camera type", c, b);
        if (s->n > 0 && s->u_right && !s->two_cam)
            OSG_REQUIRE(ctx, g->depth && g->keys_x && g->keys_y, "problem %d: KeyFrame %d stereo arrays", c, b);
        if (b >= 0 && (s->two_cam != 0) != (p->kf1.two_cam != 0))
            return osg_set_error(ctx, OSG_E_UNSUPPORTED, "problem %d: neighbour %d: a rig KeyFrame paired with a non-rig one",
                                 c, b);
    }
    return OSG_OK;
}

struct Pools {
    std::vector<float> f;
    std::vector<int32_t> i;
    int32_t addf(const float *p, size_t n)
    {
        if (!p || n == 0) return -1;
        const int32_t o = (int32_t)f.size();
        f.insert(f.end(), p, p + n);
        return o;
    }
};

KfDev make_kf(const osg_kf_side &s, const osg_np_kf &g, Pools &pl)
{
    KfDev k{};
    std::memcpy(k.Tcw, g.Tcw, sizeof k.Tcw);
    std::memcpy(k.Ow, g.Ow, sizeof k.Ow);
    std::memcpy(k.Rwc, g.Rwc, sizeof k.Rwc);
    std::memcpy(k.twc, g.twc, sizeof k.twc);
    std::memcpy(k.cam, g.cam, sizeof k.cam);
    k.fx = g.fx, k.fy = g.fy, k.cx = g.cx, k.cy = g.cy, k.invfx = g.invfx, k.invfy = g.invfy;
    k.mb = g.mb, k.mbf = g.mbf, k.median_depth = g.median_depth;
    k.cam_type = g.cam_type, k.n = s.n, k.nleft = s.nleft, k.two_cam = s.two_cam != 0, k.n_levels = s.n_levels;
    k.o_x = pl.addf(s.kp_x, s.n);
    k.o_y = pl.addf(s.kp_y, s.n);
    const bool st = s.u_right && !s.two_cam;  // bStereo is false in a rig whatever mvuRight holds
    k.o_ur = st ? pl.addf(s.u_right, s.n) : -1;
    k.o_depth = st ? pl.addf(g.depth, s.n) : -1;
    k.o_kx = st ? pl.addf(g.keys_x, s.n) : -1;
    k.o_ky = st ? pl.addf(g.keys_y, s.n) : -1;
    k.o_scale = pl.addf(s.scale_factors, s.n_levels);
    k.o_sigma = pl.addf(s.level_sigma2, s.n_levels);
    k.o_oct = (int32_t)pl.i.size();
    if (s.n > 0) pl.i.insert(pl.i.end(), s.kp_octave, s.kp_octave + s.n);
    return k;
}

int newpoints_run(osg_ctx *ctx, const osg_newpoints_problem *probs, osg_newpoints_result *res, int C)
{
    if (!ctx) return OSG_E_INVALID;
    OSG_REQUIRE(ctx, C >= 0 && (C == 0 || (probs && res)), "null argument");
    size_t T = 0, n_pairs = 0, n_claim = 0;
    for (int c = 0; c < C; c++) {
        OSG_RC(check_problem(ctx, &probs[c], c));
        T += (size_t)probs[c].n_neigh * probs[c].kf1.n;
        n_pairs += probs[c].n_neigh;
        n_claim += probs[c].kf1.n;
    }
    OSG_REQUIRE(ctx, T < (size_t(1) << 29), "batch too large");
    ctx->last_kernel_ms = 0;
    for (int c = 0; c < C; c++) {
        for (int b = 0; b < probs[c].n_neigh; b++) {
            if (res[c].skipped) res[c].skipped[b] = 0;
            if (res[c].n_created) res[c].n_created[b] = 0;
        }
    }
    if (n_pairs == 0) return 0;
    // 1. the matches of every pair for the call-time state: k_triang, one call per bCoarse value in the batch
    std::vector<int32_t> match_call(T, -1);
    std::vector<size_t> out_off(C + 1, 0);
    for (int c = 0; c < C; c++) out_off[c + 1] = out_off[c] + (size_t)probs[c].n_neigh * probs[c].kf1.n;
    double triang_ms = 0;
    for (int coarse = 0; coarse < 2; coarse++) {
        std::vector<osg_kf_side> k1, k2;
        std::vector<osg_triang_geom> g;
        std::vector<int> owner;
        for (int c = 0; c < C; c++) {
            if ((probs[c].coarse != 0) != (coarse != 0)) continue;
            for (int b = 0; b < probs[c].n_neigh; b++) {
                k1.push_back(probs[c].kf1);
                k2.push_back(probs[c].kf2[b]);
                g.push_back(probs[c].geom[b]);
                owner.push_back(c);
            }
        }
        if (k1.empty()) continue;
        size_t tot = 0;
        for (const osg_kf_side &s : k1) tot += (size_t)s.n;
        std::vector<int32_t> m(tot + 1, -1), nm(k1.size(), 0);
        const double before = ctx->last_kernel_ms;
        ctx->last_kernel_ms = 0;
        OSG_RC(osg_search_for_triangulation_batch(ctx, k1.data(), k2.data(), g.data(), (int32_t)k1.size(), 0, coarse, 0,
                                                  m.data(), nm.data()));
        triang_ms += ctx->last_kernel_ms;
        ctx->last_kernel_ms = before;
        size_t src = 0;
        std::vector<int> seen(C, 0);
        for (size_t q = 0; q < k1.size(); q++) {
            const int c = owner[q], n1 = probs[c].kf1.n;
            std::copy(m.begin() + src, m.begin() + src + n1, match_call.begin() + out_off[c] + (size_t)seen[c] * n1);
            seen[c]++;
            src += n1;
        }
    }
    // 2. geometry and keypoint arrays of every KeyFrame
    Pools pl;
    std::vector<KfDev> kf(C + n_pairs);
    std::vector<ProbDev> pd(C);
    size_t pair = 0, claim = 0;
    for (int c = 0; c < C; c++) {
        const osg_newpoints_problem &p = probs[c];
        kf[c] = make_kf(p.kf1, p.g1, pl);
        ProbDev &d = pd[c];
        d.kf1 = c, d.first_pair = (int32_t)pair, d.B = p.n_neigh, d.n1 = p.kf1.n;
        d.out_off = (int32_t)out_off[c], d.claim_off = (int32_t)claim;
        d.monocular = p.monocular != 0, d.inertial = p.inertial != 0, d.far_points = p.far_points != 0;
        d.th_far = p.th_far_points, d.ratio_factor = p.ratio_factor;
        for (int b = 0; b < p.n_neigh; b++) kf[C + pair + b] = make_kf(p.kf2[b], p.g2[b], pl);
        pair += p.n_neigh;
        claim += p.kf1.n;
    }
    OSG_REQUIRE(ctx, pl.f.size() < (size_t(1) << 30) && pl.i.size() < (size_t(1) << 30), "batch too large");
    osg_batch_io io(ctx);
    const osg_seg s_prob = io.in(sizeof(ProbDev), C), s_kf = io.in(sizeof(KfDev), kf.size());
    const osg_seg s_f = io.in(4, pl.f.size() + 1), s_i = io.in(4, pl.i.size() + 1), s_mc = io.in(4, T);
    const osg_seg s_match = io.out(4, T), s_status = io.out(1, T), s_x3d = io.out(12, T);
    const osg_seg s_skip = io.out(1, n_pairs), s_ncr = io.out(4, n_pairs);
    const size_t dl_bytes = io.out_bytes;
    const osg_seg s_claim = io.out(1, n_claim + 1);
    OSG_RC(io.stage());
    io.put(s_prob, 0, pd.data(), C);
    io.put(s_kf, 0, kf.data(), kf.size());
    io.put(s_f, 0, pl.f.data(), pl.f.size());
    io.put(s_i, 0, pl.i.data(), pl.i.size());
    io.put(s_mc, 0, match_call.data(), T);
    OSG_RC(io.upload());
    NpArgs A{};
    A.prob = io.dev_in<ProbDev>(s_prob);
    A.kf = io.dev_in<KfDev>(s_kf);
    A.fpool = io.dev_in<float>(s_f);
    A.ipool = io.dev_in<int32_t>(s_i);
    A.match_call = io.dev_in<int32_t>(s_mc);
    A.C = C;
    A.match = io.dev_out<int32_t>(s_match);
    A.status = io.dev_out<uint8_t>(s_status);
    A.x3d = io.dev_out<float>(s_x3d);
    A.skipped = io.dev_out<uint8_t>(s_skip);
    A.n_created = io.dev_out<int32_t>(s_ncr);
    A.claimed = io.dev_out<uint8_t>(s_claim);
    int maxB = 0;
    for (int c = 0; c < C; c++) maxB = std::max(maxB, (int)probs[c].n_neigh);
    OSG_RC(io.start());
    hipLaunchKernelGGL(k_np_eval, dim3(maxB, C), dim3(NT), 0, ctx->stream, A);
    OSG_HIP_CHECK(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_np_select, dim3(C), dim3(NT), 0, ctx->stream, A);
    OSG_HIP_CHECK(ctx, hipGetLastError());
    OSG_RC(io.finish(dl_bytes));
    ctx->last_kernel_ms += triang_ms;
    // 3. copy back
    int total = 0;
    for (int c = 0; c < C; c++) {
        const osg_newpoints_problem &p = probs[c];
        const size_t n = (size_t)p.n_neigh * p.kf1.n;
        if (res[c].match) io.get(res[c].match, s_match, out_off[c], n);
        if (res[c].status) io.get(res[c].status, s_status, out_off[c], n);
        if (res[c].x3d) io.get(res[c].x3d, s_x3d, out_off[c], n);
        if (res[c].skipped) io.get(res[c].skipped, s_skip, pd[c].first_pair, p.n_neigh);
        if (res[c].n_created) io.get(res[c].n_created, s_ncr, pd[c].first_pair, p.n_neigh);
        const int32_t *ncr = io.result<int32_t>(s_ncr, pd[c].first_pair);
        for (int b = 0; b < p.n_neigh; b++) total += ncr[b];
    }
    return total;
}

}  // namespace

extern "C" {

int osg_create_new_map_points(osg_ctx *ctx, const osg_newpoints_problem *problem, osg_newpoints_result *result)
{
    return newpoints_run(ctx, problem, result, 1);
}

int osg_create_new_map_points_batch(osg_ctx *ctx, const osg_newpoints_problem *problems, osg_newpoints_result *results,
                                    int32_t n_problems)
{
    return newpoints_run(ctx, problems, results, n_problems);
}

int osg_create_new_map_points_check(const osg_newpoints_problem *problem) { return check_problem(nullptr, problem, 0); }

}  // extern "C"
