// sim3ransac.hip — Sim3Solver's RANSAC (ref:src/Sim3Solver.cc:146-433) for a batch of problems.
//
// Two launches in stream order:
//   k_s3r_eval    grid (hypothesis chunks, problems), 256 lanes.  The workgroup stages the problem's
//                 matches in LDS (both camera-frame points, their own-image projections and the two
//                 bounds, 12 floats per match) while they fit; past that it reads the points from
//                 global memory and projects them again per use.  Each wave owns HPW hypotheses: all
//                 64 lanes compute the 3-point Horn solve redundantly (uniform, no hand-off), then
//                 stride over the matches, 64 at a time: transform and project both ways, compare
//                 with the reference's `<` (NaN is never an inlier), __ballot -> one mask word,
//                 __popcll -> the count.  Per hypothesis: count, R t s, mask words -> scratch.
//   k_s3r_select  one wave per problem: lane 0 replays the reference's sequential rule on the counts
//                 (sim3ransac_select.h), the wave expands the chosen hypothesis's mask words to N
//                 bytes and copies its R, t, s, T12.
// No atomics and no in-launch hand-off: the result is the same bits every run.
//
// Arithmetic follows the reference's types: float points, matrices and projections; Horn's N is built
// from float sums; its eigenvector comes from a cyclic Jacobi iteration in double (the reference:
// Eigen's general EigenSolver in float), rounded to float; ang, nom / den and 1 / s are double.
#include <cstring>
#include <vector>

#include "batch_io.h"
#include "ransac_common.h"
#include "sim3ransac_select.h"

namespace {

constexpr int NT = 256;          // lanes per workgroup
constexpr int NWV = NT / 64;     // waves per workgroup
constexpr int HPW = 2;           // hypotheses per wave
constexpr int HPB = NWV * HPW;   // hypotheses per workgroup
constexpr int FPM = 12;          // staged floats per match
constexpr int LDS_CAP = 160 * 1024;

struct RProbDev {
    int n, n_hyp, fix_scale, min_inliers;
    int pt_off;         // first match in the concatenated match arrays
    int hyp_off;        // first hypothesis in the concatenated hypothesis arrays
    int words;          // mask words per hypothesis: ceil(n / 64)
    int staged;         // matches live in LDS
    long long mask_off; // first mask word
    osg_camera cam1, cam2;
};

struct RSelOut {
    int converged, hyp, n_iterations, n_inliers, n_best, pad[3];
    float R[9], t[3], s;
    float T12[16];
    float pad2[3];
};

struct V3 {
    float x, y, z;
};

// a 3-term sum the way Eigen's unrolled reduction associates it: a + (b + c)
__device__ __forceinline__ float sum3(float a, float b, float c) { return a + (b + c); }
__device__ __forceinline__ float dot3(float a0, float a1, float a2, float b0, float b1, float b2)
{
    return sum3(a0 * b0, a1 * b1, a2 * b2);
}

struct Hyp {
    float R[9], t[3], s;  // T12 = [sR | t]
    float A[9], a[3];     // s R, t
    float B[9], b[3];     // T21 = [(1/s) R^T | -(1/s) R^T t]
};

// eigenvector of the largest eigenvalue of the symmetric 4x4 n (upper triangle given): cyclic Jacobi
// in double.  A zero matrix returns (1, 0, 0, 0), as Eigen's solver does.
__device__ inline void top_eigenvector(const double n[10], double q[4])
{
    double A[4][4] = {{n[0], n[1], n[2], n[3]}, {n[1], n[4], n[5], n[6]}, {n[2], n[5], n[7], n[8]}, {n[3], n[6], n[8], n[9]}};
    double V[4][4];
    jacobi_sym<double, 4>(A, V, 16, 1e-40);  // stops when converged, zero, or NaN
    int top = 0;
    double best = A[0][0];
#pragma unroll
    for (int i = 1; i < 4; i++)
        if (A[i][i] > best) {
            best = A[i][i];
            top = i;
        }
#pragma unroll
    for (int k = 0; k < 4; k++) q[k] = top == 0 ? V[k][0] : top == 1 ? V[k][1] : top == 2 ? V[k][2] : V[k][3];
}

// Sim3Solver::ComputeSim3 (ref:src/Sim3Solver.cc:307-407) on the columns P1 = (a0 a1 a2), P2 = (b0 b1 b2)
__device__ inline void compute_sim3(const V3 *a, const V3 *b, bool fix_scale, Hyp &h)
{
    // centroids and relative coordinates
    const float o1[3] = {sum3(a[0].x, a[1].x, a[2].x) / 3.f, sum3(a[0].y, a[1].y, a[2].y) / 3.f, sum3(a[0].z, a[1].z, a[2].z) / 3.f};
    const float o2[3] = {sum3(b[0].x, b[1].x, b[2].x) / 3.f, sum3(b[0].y, b[1].y, b[2].y) / 3.f, sum3(b[0].z, b[1].z, b[2].z) / 3.f};
    float p1[3][3], p2[3][3];  // [row][point]
#pragma unroll
    for (int i = 0; i < 3; i++) {
        p1[0][i] = a[i].x - o1[0];
        p1[1][i] = a[i].y - o1[1];
        p1[2][i] = a[i].z - o1[2];
        p2[0][i] = b[i].x - o2[0];
        p2[1][i] = b[i].y - o2[1];
        p2[2][i] = b[i].z - o2[2];
    }
    // M = Pr2 Pr1^T
    float M[3][3];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) M[i][j] = dot3(p2[i][0], p2[i][1], p2[i][2], p1[j][0], p1[j][1], p1[j][2]);
    // N: float sums (the reference's doubles receive float expressions, the Matrix4f rounds them back)
    double n[10];
    n[0] = M[0][0] + M[1][1] + M[2][2];
    n[1] = M[1][2] - M[2][1];
    n[2] = M[2][0] - M[0][2];
    n[3] = M[0][1] - M[1][0];
    n[4] = M[0][0] - M[1][1] - M[2][2];
    n[5] = M[0][1] + M[1][0];
    n[6] = M[2][0] + M[0][2];
    n[7] = -M[0][0] + M[1][1] - M[2][2];
    n[8] = M[1][2] + M[2][1];
    n[9] = -M[0][0] - M[1][1] + M[2][2];
    double qd[4];
    top_eigenvector(n, qd);
    const float e0 = (float)qd[0];
    float v[3] = {(float)qd[1], (float)qd[2], (float)qd[3]};
    const float vn = sqrtf(sum3(v[0] * v[0], v[1] * v[1], v[2] * v[2]));
    const double ang = atan2((double)vn, (double)e0);
    const float f = (float)(2 * ang);
#pragma unroll
    for (int k = 0; k < 3; k++) v[k] = f * v[k] / vn;
    // Sophus::SO3f::exp(vec).matrix()
    const float theta_sq = sum3(v[0] * v[0], v[1] * v[1], v[2] * v[2]);
    float imag, real;
    if (theta_sq < 1e-10f * 1e-10f) {
        const float theta_po4 = theta_sq * theta_sq;
        imag = 0.5f - (1.0f / 48.0f) * theta_sq + (1.0f / 3840.0f) * theta_po4;
        real = 1.f - (1.0f / 8.0f) * theta_sq + (1.0f / 384.0f) * theta_po4;
    } else {
        const float theta = sqrtf(theta_sq);
        const float half = 0.5f * theta;
        imag = sinf(half) / theta;
        real = cosf(half);
    }
    const float qw = real, qx = imag * v[0], qy = imag * v[1], qz = imag * v[2];
    {
        const float tx = 2.f * qx, ty = 2.f * qy, tz = 2.f * qz;
        const float twx = tx * qw, twy = ty * qw, twz = tz * qw;
        const float txx = tx * qx, txy = ty * qx, txz = tz * qx;
        const float tyy = ty * qy, tyz = tz * qy, tzz = tz * qz;
        h.R[0] = 1.f - (tyy + tzz);
        h.R[1] = txy - twz;
        h.R[2] = txz + twy;
        h.R[3] = txy + twz;
        h.R[4] = 1.f - (txx + tzz);
        h.R[5] = tyz - twx;
        h.R[6] = txz - twy;
        h.R[7] = tyz + twx;
        h.R[8] = 1.f - (txx + tyy);
    }
    // P3 = R Pr2; s = nom / den
    float s = 1.0f;
    if (!fix_scale) {
        float nomf = 0.f, denf = 0.f;
#pragma unroll
        for (int j = 0; j < 3; j++)
#pragma unroll
            for (int i = 0; i < 3; i++) {
                const float p3 = dot3(h.R[3 * i], h.R[3 * i + 1], h.R[3 * i + 2], p2[0][j], p2[1][j], p2[2][j]);
                nomf += p1[i][j] * p3;
                denf += p3 * p3;
            }
        s = (float)((double)nomf / (double)denf);
    }
    h.s = s;
#pragma unroll
    for (int k = 0; k < 9; k++) h.A[k] = s * h.R[k];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        h.t[i] = o1[i] - dot3(h.A[3 * i], h.A[3 * i + 1], h.A[3 * i + 2], o2[0], o2[1], o2[2]);
        h.a[i] = h.t[i];
    }
    const float is = (float)(1.0 / (double)s);
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) h.B[3 * i + j] = is * h.R[3 * j + i];
#pragma unroll
    for (int i = 0; i < 3; i++) h.b[i] = dot3(-h.B[3 * i], -h.B[3 * i + 1], -h.B[3 * i + 2], h.t[0], h.t[1], h.t[2]);
}

__global__ __launch_bounds__(NT) void k_s3r_eval(const RProbDev *__restrict__ probs, const float *__restrict__ a_p1c,
                                                 const float *__restrict__ a_p2c, const float *__restrict__ a_m1,
                                                 const float *__restrict__ a_m2, const int *__restrict__ a_samples,
                                                 int *__restrict__ o_count, float *__restrict__ o_sim3,
                                                 unsigned long long *__restrict__ o_mask)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const RProbDev &P = probs[blockIdx.y];
    const int h_first = blockIdx.x * HPB;
    if (h_first >= P.n_hyp) return;  // the whole workgroup: no barrier is skipped by a part of it
    const int n = P.n;
    const int tid = threadIdx.x, wave = tid / 64, lane = tid % 64;
    const float *p1c = a_p1c + 3 * (size_t)P.pt_off, *p2c = a_p2c + 3 * (size_t)P.pt_off;
    const float *m1 = a_m1 + P.pt_off, *m2 = a_m2 + P.pt_off;
    const bool staged = P.staged != 0;
    if (staged) {
        for (int i = tid; i < n; i += NT) {
            // field k of match i at lds[k n + i]: consecutive lanes read consecutive banks
            const float x1 = p1c[3 * i], y1 = p1c[3 * i + 1], z1 = p1c[3 * i + 2];
            const float x2 = p2c[3 * i], y2 = p2c[3 * i + 1], z2 = p2c[3 * i + 2];
            float u1, v1, u2, v2;
            project_f(P.cam1, x1, y1, z1, u1, v1);  // mvP1im1
            project_f(P.cam2, x2, y2, z2, u2, v2);  // mvP2im2
            lds[i] = x1, lds[n + i] = y1, lds[2 * n + i] = z1;
            lds[3 * n + i] = x2, lds[4 * n + i] = y2, lds[5 * n + i] = z2;
            lds[6 * n + i] = u1, lds[7 * n + i] = v1, lds[8 * n + i] = u2, lds[9 * n + i] = v2;
            lds[10 * n + i] = m1[i];
            lds[11 * n + i] = m2[i];
        }
        __syncthreads();
    }
    const int *samples = a_samples + 3 * (size_t)P.hyp_off;
    for (int k = 0; k < HPW; k++) {
        const int h = h_first + wave * HPW + k;  // wave-uniform
        if (h >= P.n_hyp) break;
        V3 a[3], b[3];
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const int idx = samples[3 * h + j];  // checked by the host: in [0, n)
            a[j] = {p1c[3 * idx], p1c[3 * idx + 1], p1c[3 * idx + 2]};
            b[j] = {p2c[3 * idx], p2c[3 * idx + 1], p2c[3 * idx + 2]};
        }
        Hyp H;
        compute_sim3(a, b, P.fix_scale != 0, H);
        // CheckInliers (ref:src/Sim3Solver.cc:409-433)
        int count = 0;
        unsigned long long *mask = o_mask + P.mask_off + (size_t)h * P.words;
        for (int w = 0; w < P.words; w++) {
            const int i = w * 64 + lane;
            bool in = false;
            if (i < n) {
                float x1, y1, z1, x2, y2, z2, u1, v1, u2, v2, e1max, e2max;
                if (staged) {
                    x1 = lds[i], y1 = lds[n + i], z1 = lds[2 * n + i];
                    x2 = lds[3 * n + i], y2 = lds[4 * n + i], z2 = lds[5 * n + i];
                    u1 = lds[6 * n + i], v1 = lds[7 * n + i], u2 = lds[8 * n + i], v2 = lds[9 * n + i];
                    e1max = lds[10 * n + i], e2max = lds[11 * n + i];
                } else {
                    x1 = p1c[3 * i], y1 = p1c[3 * i + 1], z1 = p1c[3 * i + 2];
                    x2 = p2c[3 * i], y2 = p2c[3 * i + 1], z2 = p2c[3 * i + 2];
                    project_f(P.cam1, x1, y1, z1, u1, v1);
                    project_f(P.cam2, x2, y2, z2, u2, v2);
                    e1max = m1[i], e2max = m2[i];
                }
                // set 2 through T12 into camera 1
                float pu, pv;
                project_f(P.cam1, dot3(H.A[0], H.A[1], H.A[2], x2, y2, z2) + H.a[0],
                          dot3(H.A[3], H.A[4], H.A[5], x2, y2, z2) + H.a[1],
                          dot3(H.A[6], H.A[7], H.A[8], x2, y2, z2) + H.a[2], pu, pv);
                const float d1x = u1 - pu, d1y = v1 - pv;
                const float err1 = d1x * d1x + d1y * d1y;
                // set 1 through T21 into camera 2
                project_f(P.cam2, dot3(H.B[0], H.B[1], H.B[2], x1, y1, z1) + H.b[0],
                          dot3(H.B[3], H.B[4], H.B[5], x1, y1, z1) + H.b[1],
                          dot3(H.B[6], H.B[7], H.B[8], x1, y1, z1) + H.b[2], pu, pv);
                const float d2x = pu - u2, d2y = pv - v2;
                const float err2 = d2x * d2x + d2y * d2y;
                in = err1 < e1max && err2 < e2max;
            }
            const unsigned long long word = __ballot(in);
            count += __popcll(word);
            if (lane == 0) mask[w] = word;
        }
        if (lane == 0) {
            const size_t g = (size_t)P.hyp_off + h;
            o_count[g] = count;
            float *o = o_sim3 + 13 * g;
#pragma unroll
            for (int j = 0; j < 9; j++) o[j] = H.R[j];
#pragma unroll
            for (int j = 0; j < 3; j++) o[9 + j] = H.t[j];
            o[12] = H.s;
        }
    }
}

__global__ __launch_bounds__(64) void k_s3r_select(const RProbDev *__restrict__ probs, const int *__restrict__ counts,
                                                   const float *__restrict__ sim3,
                                                   const unsigned long long *__restrict__ masks,
                                                   RSelOut *__restrict__ out, uint8_t *__restrict__ inlier)
{
    const RProbDev &P = probs[blockIdx.x];
    const int lane = threadIdx.x;
    int hyp = 0;
    if (lane == 0) {
        const osg_s3r_window w = osg_s3r_replay(counts + P.hyp_off, P.n_hyp, P.min_inliers, 0, P.n_hyp, 0);
        hyp = w.hyp;  // >= 0: counts are >= 0 and n_hyp >= 1
        RSelOut &o = out[blockIdx.x];
        o.converged = w.converged;
        o.hyp = hyp;
        o.n_iterations = w.n_iterations;
        o.n_best = w.n_best;
        o.n_inliers = w.converged ? counts[P.hyp_off + hyp] : 0;
        const float *s = sim3 + 13 * ((size_t)P.hyp_off + hyp);
        for (int j = 0; j < 9; j++) o.R[j] = s[j];
        for (int j = 0; j < 3; j++) o.t[j] = s[9 + j];
        o.s = s[12];
        for (int i = 0; i < 3; i++) {
            for (int j = 0; j < 3; j++) o.T12[4 * i + j] = s[12] * s[3 * i + j];
            o.T12[4 * i + 3] = s[9 + i];
        }
        o.T12[12] = o.T12[13] = o.T12[14] = 0.f;
        o.T12[15] = 1.f;
    }
    hyp = __shfl(hyp, 0);
    expand_mask(masks + P.mask_off + (size_t)hyp * P.words, P.n, inlier + P.pt_off, lane);
}

}  // namespace

extern "C" {

int32_t osg_sim3_ransac_iterations(double prob, int32_t min_inliers, int32_t n, int32_t max_its)
{
    return osg_s3r_iterations(prob, min_inliers, n, max_its);
}

int osg_sim3_ransac_batch(osg_ctx *ctx, const osg_sim3_ransac_problem *p, int32_t nb, osg_sim3_ransac_result *r)
{
    if (!ctx) return OSG_E_INVALID;
    OSG_REQUIRE(ctx, nb >= 0 && (nb == 0 || (p && r)), "null argument");
    if (nb == 0) return 0;
    const size_t lds_budget = (size_t)std::min(ctx->lds_per_block, LDS_CAP);
    std::vector<RProbDev> hp;
    std::vector<int> src;  // hp[k] is problem src[k]
    hp.reserve(nb);
    size_t n_pts = 0, n_hyp = 0, n_words = 0, lds = 0;
    int max_hyp = 0;
    for (int b = 0; b < nb; b++) {
        const osg_sim3_ransac_problem &q = p[b];
        OSG_REQUIRE(ctx, q.n >= 0 && q.n_hyp >= 1 && q.min_inliers >= 0, "n, n_hyp or min_inliers");
        OSG_REQUIRE(ctx, q.n == 0 || r[b].inlier, "inlier array");
        if (q.n == 0 || q.n < q.min_inliers) continue;
        OSG_REQUIRE(ctx, q.p1c && q.p2c && q.max_err1 && q.max_err2 && q.samples, "match arrays");
        int h_bad = -1;
        int why = check_sets(q.samples, 3, q.n_hyp, q.n, &h_bad);
        for (int j = 0; why == 2 && j < 3; j++)  // a set with both faults reports the index outside
            if (q.samples[3 * (size_t)h_bad + j] < 0 || q.samples[3 * (size_t)h_bad + j] >= q.n) why = 1;
        OSG_REQUIRE(ctx, why != 1, "sample index outside [0, n) in hypothesis %d of problem %d", h_bad, b);
        OSG_REQUIRE(ctx, why != 2, "repeated sample index in hypothesis %d of problem %d", h_bad, b);
        RProbDev d;
        std::memset(&d, 0, sizeof d);
        d.n = q.n;
        d.n_hyp = q.n_hyp;
        d.fix_scale = q.fix_scale;
        d.min_inliers = q.min_inliers;
        d.pt_off = (int)n_pts;
        d.hyp_off = (int)n_hyp;
        d.words = (q.n + 63) / 64;
        d.mask_off = (long long)n_words;
        const size_t need = sizeof(float) * FPM * (size_t)q.n;
        d.staged = need <= lds_budget;
        if (d.staged) lds = std::max(lds, need);
        d.cam1 = q.cam1;
        d.cam2 = q.cam2;
        n_pts += (size_t)q.n;
        n_hyp += (size_t)q.n_hyp;
        n_words += (size_t)d.words * q.n_hyp;
        max_hyp = std::max(max_hyp, q.n_hyp);
        hp.push_back(d);
        src.push_back(b);
        OSG_REQUIRE(ctx, n_pts < (size_t(1) << 28) && n_hyp < (size_t(1) << 24), "too many matches or hypotheses in one batch");
    }
    const int na = (int)hp.size();
    // the problems that never iterate: identity and zeros
    for (int b = 0; b < nb; b++) {
        osg_sim3_ransac_result &o = r[b];
        o.converged = 0;
        o.hyp = -1;
        o.n_iterations = o.n_inliers = o.n_best = 0;
        for (int j = 0; j < 9; j++) o.R[j] = (j % 4 == 0) ? 1.f : 0.f;
        for (int j = 0; j < 3; j++) o.t[j] = 0.f;
        o.s = 1.f;
        for (int j = 0; j < 16; j++) o.T12[j] = (j % 5 == 0) ? 1.f : 0.f;
        if (p[b].n > 0) std::memset(o.inlier, 0, (size_t)p[b].n);
        if (o.hyp_inliers) std::memset(o.hyp_inliers, 0, sizeof(int32_t) * (size_t)p[b].n_hyp);
        if (o.hyp_sim3)
            for (int h = 0; h < p[b].n_hyp; h++)
                for (int j = 0; j < 13; j++) o.hyp_sim3[13 * (size_t)h + j] = (j < 9 && j % 4 == 0) || j == 12 ? 1.f : 0.f;
    }
    if (na == 0) return 0;
    bool want_hyp = false;
    for (int k = 0; k < na; k++) want_hyp = want_hyp || r[src[k]].hyp_inliers || r[src[k]].hyp_sim3;
    osg_batch_io io(ctx);
    const osg_seg i_pr = io.in(sizeof(RProbDev), na), i_p1 = io.in(3 * sizeof(float), n_pts), i_p2 = io.in(3 * sizeof(float), n_pts);
    const osg_seg i_m1 = io.in(sizeof(float), n_pts), i_m2 = io.in(sizeof(float), n_pts), i_sm = io.in(3 * sizeof(int32_t), n_hyp);
    // the counts and the Sim3s are downloaded on request
    const osg_seg o_res = io.out(sizeof(RSelOut), na), o_in = io.out(1, n_pts), o_cnt = io.out(sizeof(int32_t), n_hyp);
    const osg_seg o_s3 = io.out(13 * sizeof(float), n_hyp);
    const size_t dl_bytes = want_hyp ? io.out_bytes : o_cnt.off;
    OSG_RC(io.stage());
    io.put(i_pr, 0, hp.data(), na);
    for (int k = 0; k < na; k++) {
        const osg_sim3_ransac_problem &q = p[src[k]];
        io.put(i_p1, hp[k].pt_off, q.p1c, q.n);
        io.put(i_p2, hp[k].pt_off, q.p2c, q.n);
        io.put(i_m1, hp[k].pt_off, q.max_err1, q.n);
        io.put(i_m2, hp[k].pt_off, q.max_err2, q.n);
        io.put(i_sm, hp[k].hyp_off, q.samples, q.n_hyp);
    }
    OSG_RC(io.upload());
    unsigned long long *dmask = nullptr;
    OSG_ALLOC(ctx, dmask, SLOT_BA2, 8 * n_words);
    if (lds > 48 * 1024)
        OSG_HIP_CHECK(ctx, hipFuncSetAttribute((const void *)k_s3r_eval, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    OSG_RC(io.start());
    const RProbDev *dp = io.dev_in<const RProbDev>(i_pr);
    hipLaunchKernelGGL(k_s3r_eval, dim3((max_hyp + HPB - 1) / HPB, na), dim3(NT), lds, ctx->stream, dp,
                       io.dev_in<const float>(i_p1), io.dev_in<const float>(i_p2), io.dev_in<const float>(i_m1),
                       io.dev_in<const float>(i_m2), io.dev_in<const int>(i_sm), io.dev_out<int>(o_cnt),
                       io.dev_out<float>(o_s3), dmask);
    OSG_HIP_CHECK(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_s3r_select, dim3(na), dim3(64), 0, ctx->stream, dp, io.dev_out<const int>(o_cnt),
                       io.dev_out<const float>(o_s3), (const unsigned long long *)dmask, io.dev_out<RSelOut>(o_res),
                       io.dev_out<uint8_t>(o_in));
    OSG_HIP_CHECK(ctx, hipGetLastError());
    OSG_RC(io.finish(dl_bytes));
    const RSelOut *res = io.result<RSelOut>(o_res);
    int conv = 0;
    for (int k = 0; k < na; k++) {
        const RSelOut &s = res[k];
        osg_sim3_ransac_result &o = r[src[k]];
        o.converged = s.converged;
        o.hyp = s.hyp;
        o.n_iterations = s.n_iterations;
        o.n_inliers = s.n_inliers;
        o.n_best = s.n_best;
        std::memcpy(o.R, s.R, sizeof o.R);
        std::memcpy(o.t, s.t, sizeof o.t);
        o.s = s.s;
        std::memcpy(o.T12, s.T12, sizeof o.T12);
        io.get(o.inlier, o_in, hp[k].pt_off, hp[k].n);
        if (o.hyp_inliers) io.get(o.hyp_inliers, o_cnt, hp[k].hyp_off, hp[k].n_hyp);
        if (o.hyp_sim3) io.get(o.hyp_sim3, o_s3, hp[k].hyp_off, hp[k].n_hyp);
        conv += s.converged ? 1 : 0;
    }
    return conv;
}

int osg_sim3_ransac(osg_ctx *ctx, const osg_sim3_ransac_problem *p, osg_sim3_ransac_result *r)
{
    const int rc = osg_sim3_ransac_batch(ctx, p, 1, r);
    return rc < 0 ? rc : r->n_inliers;
}

}  // extern "C"
