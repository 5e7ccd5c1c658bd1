// twoview.hip — TwoViewReconstruction::Reconstruct (ref:src/TwoViewReconstruction.cc:49-1223,
// ref:src/GeometricTools.cc:62-89) for a batch of problems.
//
// Five launches in stream order, no host round trip between them:
//   k_tvr_norm     grid (frame, problem): Normalize's mean and mean absolute deviation over all keypoints of
//                  the frame; double partial sums, a fixed-order tree.
//   k_tvr_eval     grid (hypothesis, model, problem), 256 lanes.  Lanes 0-7 write the rows of the DLT matrix
//                  of the normalised 8-point sample (16 x 9 for H, 8 x 9 for F) to LDS, 81 lanes form A^T A in
//                  double, and the workgroup runs a Jacobi iteration on it in LDS in the round-robin ordering:
//                  four disjoint rotations per round, their (c, s) from lanes 0-3, then one lane per (row,
//                  pair) for S J and V J and one per (column, pair) for J^T S, so no two lanes touch the same
//                  entry between two barriers; nine rounds make a sweep.  The
//                  eigenvector of the smallest eigenvalue, rounded to float, is the model; F is projected to
//                  rank 2 by removing its smallest singular triple (3 x 3 Jacobi in double, every lane
//                  redundantly); both are denormalised in float.  Then every lane scores matches 256 apart,
//                  in float as the reference, and the partial sums are added by a fixed tree: no float
//                  atomics, a rerun gives the same bits.  Inlier flags leave as __ballot words.
//   k_tvr_select   one wave per problem: lane 0 takes the lowest hypothesis of maximal score per model
//                  (`currentScore > score` from 0), RH = SH / (SH + SF), and decomposes the chosen model:
//                  DecomposeE's four or Faugeras' eight motion hypotheses.  The wave expands both winners'
//                  mask words to bytes.
//   k_tvr_checkrt  grid (motion hypothesis, problem): per inlier match Triangulate (the null vector of the
//                  4 x 4 system by Jacobi on its Gram matrix in double) and CheckRT's tests; nGood; the
//                  parallax from the order statistic min(50, nGood - 1) of cosParallax, found by bisection
//                  on the ordered bit patterns (counts only, no sort).
//   k_tvr_final    one workgroup per problem: the acceptance rule (twoview_select.h) and the scatter of the
//                  chosen hypothesis' points to frame-1 keypoint order.
//
// Each match is read once per workgroup, straight from global memory (16 bytes, coalesced): there is no reuse
// that staging in LDS would serve, and n is not bounded by LDS.
#include <cstring>
#include <vector>

#include "batch_io.h"
#include "ransac_common.h"
#include "twoview_select.h"

namespace {

constexpr int NT = 256;

struct TProbDev {
    int n, n_hyp, n_keys1, n_keys2;
    int pt_off, key1_off, key2_off, hyp_off;
    int words, min_triangulated;
    long long mask_off;  // first mask word; layout [model][hypothesis][word]
    float K[4];
    float sigma, min_parallax;
};

struct TOut {
    int ok, model, hyp_h, hyp_f, cand, n_inliers, n_cand, pad;
    float score_h, score_f;
    float H21[9], F21[9], R[9], t[3];
    int n_good[8];
    float parallax[8];
    float cand_Rt[96];
};

// ---- small dense algebra -------------------------------------------------------------------------
// the register Jacobi (ransac_common.h) with this module's sweep limit and convergence constant
constexpr int JS_SWEEPS = 24;
constexpr double JS_TOL = 1e-34;

__device__ __forceinline__ void mul3(const float *a, const float *b, float *c)
{
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) c[3 * i + j] = a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j] + a[3 * i + 2] * b[6 + j];
}

__device__ __forceinline__ float det3(const float *m)
{
    return m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]);
}

// the cofactor inverse (a singular matrix gives inf / NaN, as the reference's does)
__device__ __forceinline__ void inv3(const float *m, float *o)
{
    const float c00 = m[4] * m[8] - m[5] * m[7], c10 = m[5] * m[6] - m[3] * m[8], c20 = m[3] * m[7] - m[4] * m[6];
    const float det = c00 * m[0] + c10 * m[1] + c20 * m[2];
    const float id = 1.f / det;
    o[0] = c00 * id;
    o[1] = (m[2] * m[7] - m[1] * m[8]) * id;
    o[2] = (m[1] * m[5] - m[2] * m[4]) * id;
    o[3] = c10 * id;
    o[4] = (m[0] * m[8] - m[2] * m[6]) * id;
    o[5] = (m[2] * m[3] - m[0] * m[5]) * id;
    o[6] = c20 * id;
    o[7] = (m[1] * m[6] - m[0] * m[7]) * id;
    o[8] = (m[0] * m[4] - m[1] * m[3]) * id;
}

// M = U diag(w) V^T with w descending, from the eigenvectors of M^T M in double; U's columns are M v / w, the
// third one the cross product of the first two when w2 is (numerically) zero.  Rounded to float at the end.
__device__ inline void svd3(const float *M, float *U, float *w, float *V)
{
    double G[3][3], E[3][3];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++)
            G[i][j] = (double)M[i] * M[j] + (double)M[3 + i] * M[3 + j] + (double)M[6 + i] * M[6 + j];
    jacobi_sym<double, 3>(G, E, JS_SWEEPS, JS_TOL);
    int o0 = 0, o1 = 1, o2 = 2;
    double l0 = G[0][0], l1 = G[1][1], l2 = G[2][2];
    if (l1 > l0) { double x = l0; l0 = l1; l1 = x; int y = o0; o0 = o1; o1 = y; }
    if (l2 > l0) { double x = l0; l0 = l2; l2 = x; int y = o0; o0 = o2; o2 = y; }
    if (l2 > l1) { double x = l1; l1 = l2; l2 = x; int y = o1; o1 = o2; o2 = y; }
    const int ord[3] = {o0, o1, o2};
    const double sv[3] = {sqrt(fmax(l0, 0.0)), sqrt(fmax(l1, 0.0)), sqrt(fmax(l2, 0.0))};
    double Vd[3][3], Ud[3][3];  // [row][column]
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const int e = ord[c];
#pragma unroll
        for (int r = 0; r < 3; r++) Vd[r][c] = e == 0 ? E[r][0] : e == 1 ? E[r][1] : E[r][2];
    }
#pragma unroll
    for (int c = 0; c < 3; c++) {
        double u[3];
#pragma unroll
        for (int r = 0; r < 3; r++) u[r] = (double)M[3 * r] * Vd[0][c] + (double)M[3 * r + 1] * Vd[1][c] + (double)M[3 * r + 2] * Vd[2][c];
        const double nu = sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
#pragma unroll
        for (int r = 0; r < 3; r++) Ud[r][c] = u[r] / nu;
    }
    if (!(sv[2] > 1e-6 * sv[0])) {
        Ud[0][2] = Ud[1][0] * Ud[2][1] - Ud[2][0] * Ud[1][1];
        Ud[1][2] = Ud[2][0] * Ud[0][1] - Ud[0][0] * Ud[2][1];
        Ud[2][2] = Ud[0][0] * Ud[1][1] - Ud[1][0] * Ud[0][1];
    }
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) {
            U[3 * r + c] = (float)Ud[r][c];
            V[3 * r + c] = (float)Vd[r][c];
        }
    w[0] = (float)sv[0], w[1] = (float)sv[1], w[2] = (float)sv[2];
}

// ---- Normalize -----------------------------------------------------------------------------------
// out[8 b + 4 f + (0..3)] = meanX, meanY, sX, sY of frame f of problem b
__global__ __launch_bounds__(NT) void k_tvr_norm(const TProbDev *__restrict__ probs, const float *__restrict__ keys1,
                                                 const float *__restrict__ keys2, float *__restrict__ out)
{
    __shared__ double rx[NT], ry[NT];
    __shared__ float mean[2];
    const TProbDev &P = probs[blockIdx.y];
    const int f = blockIdx.x, tid = threadIdx.x;
    const int nk = f == 0 ? P.n_keys1 : P.n_keys2;
    const float *k = f == 0 ? keys1 + 2 * (size_t)P.key1_off : keys2 + 2 * (size_t)P.key2_off;
    double sx = 0, sy = 0;
    for (int i = tid; i < nk; i += NT) sx += k[2 * i], sy += k[2 * i + 1];
    rx[tid] = sx, ry[tid] = sy;
    for (int s = NT / 2; s > 0; s >>= 1) {
        __syncthreads();
        if (tid < s) rx[tid] += rx[tid + s], ry[tid] += ry[tid + s];
    }
    __syncthreads();
    if (tid == 0) mean[0] = (float)(rx[0] / nk), mean[1] = (float)(ry[0] / nk);
    __syncthreads();
    const float mx = mean[0], my = mean[1];
    sx = sy = 0;
    for (int i = tid; i < nk; i += NT) sx += fabsf(k[2 * i] - mx), sy += fabsf(k[2 * i + 1] - my);
    __syncthreads();
    rx[tid] = sx, ry[tid] = sy;
    for (int s = NT / 2; s > 0; s >>= 1) {
        __syncthreads();
        if (tid < s) rx[tid] += rx[tid + s], ry[tid] += ry[tid + s];
    }
    __syncthreads();
    if (tid == 0) {
        float *o = out + 8 * (size_t)blockIdx.y + 4 * f;
        const float dx = (float)(rx[0] / nk), dy = (float)(ry[0] / nk);
        o[0] = mx, o[1] = my;
        o[2] = (float)(1.0 / (double)dx);
        o[3] = (float)(1.0 / (double)dy);
    }
}

// ---- hypotheses ----------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void k_tvr_eval(const TProbDev *__restrict__ probs, const float4 *__restrict__ kp,
                                                 const int *__restrict__ a_sets, const float *__restrict__ norm,
                                                 float *__restrict__ o_score, float *__restrict__ o_model,
                                                 unsigned long long *__restrict__ o_mask)
{
    __shared__ float Am[16][9];
    __shared__ double S[9][9], V[9][9], cs[4][2];
    __shared__ float red[NT];
    const TProbDev &P = probs[blockIdx.z];
    const int h = blockIdx.x, model = blockIdx.y;
    if (h >= P.n_hyp) return;  // the whole workgroup
    const int n = P.n, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const float4 *m = kp + P.pt_off;
    const float *nr = norm + 8 * (size_t)blockIdx.z;
    const float m1x = nr[0], m1y = nr[1], s1x = nr[2], s1y = nr[3], m2x = nr[4], m2y = nr[5], s2x = nr[6], s2y = nr[7];
    const int rows = model == 0 ? 16 : 8;
    if (tid < 8) {
        const int idx = a_sets[8 * ((size_t)P.hyp_off + h) + tid];  // checked by the host: in [0, n)
        const float4 q = m[idx];
        const float u1 = (q.x - m1x) * s1x, v1 = (q.y - m1y) * s1y, u2 = (q.z - m2x) * s2x, v2 = (q.w - m2y) * s2y;
        if (model == 0) {
            float *a = Am[2 * tid], *b = Am[2 * tid + 1];
            a[0] = 0.f, a[1] = 0.f, a[2] = 0.f, a[3] = -u1, a[4] = -v1, a[5] = -1.f, a[6] = v2 * u1, a[7] = v2 * v1, a[8] = v2;
            b[0] = u1, b[1] = v1, b[2] = 1.f, b[3] = 0.f, b[4] = 0.f, b[5] = 0.f, b[6] = -u2 * u1, b[7] = -u2 * v1, b[8] = -u2;
        } else {
            float *a = Am[tid];
            a[0] = u2 * u1, a[1] = u2 * v1, a[2] = u2, a[3] = v2 * u1, a[4] = v2 * v1, a[5] = v2, a[6] = u1, a[7] = v1, a[8] = 1.f;
        }
    }
    __syncthreads();
    if (tid < 81) {
        const int i = tid / 9, j = tid % 9;
        double s = 0;
        for (int r = 0; r < rows; r++) s += (double)Am[r][i] * (double)Am[r][j];
        S[i][j] = s;
        V[i][j] = i == j ? 1.0 : 0.0;
    }
    __syncthreads();
    // Jacobi in LDS with the round-robin ordering: round r rotates the four disjoint pairs
    // ((r + k) mod 9, (r - k) mod 9), k = 1 .. 4 (index r sits out); nine rounds visit every pair once.  Lanes
    // 0-3 compute the four (c, s); then S <- S J and V <- V J (lane = (row, pair): its own two entries), then
    // S <- J^T S (lane = (column, pair)).  Every branch is workgroup-uniform.
    for (int sweep = 0; sweep < 30; sweep++) {
        double off = 0, diag = 0;
        for (int i = 0; i < 9; i++) {
            diag += S[i][i] * S[i][i];
            for (int j = i + 1; j < 9; j++) off += S[i][j] * S[i][j];
        }
        if (!(off > 1e-32 * diag)) break;  // converged, zero, or NaN
        for (int r = 0; r < 9; r++) {
            const int k = (tid & 3) + 1;
            const int i0 = (r + k) % 9, i1 = (r + 9 - k) % 9;
            const int p = i0 < i1 ? i0 : i1, q = i0 < i1 ? i1 : i0;  // the pair of this lane's task
            if (tid < 4) {
                const double spq = S[p][q];
                double c = 1.0, s = 0.0;
                if (spq != 0.0) jacobi_rotation(S[p][p], S[q][q], spq, c, s);
                cs[tid][0] = c, cs[tid][1] = s;
            }
            __syncthreads();
            const double c = cs[tid & 3][0], s = cs[tid & 3][1];
            if (tid < 72) {  // columns p, q of row a: S for tasks 0-35, V for 36-71
                const int a = (tid % 36) >> 2;
                double(*M)[9] = tid < 36 ? S : V;
                const double x = M[a][p], y = M[a][q];
                M[a][p] = c * x - s * y;
                M[a][q] = s * x + c * y;
            }
            __syncthreads();
            if (tid < 36) {  // rows p, q of column b
                const int b = tid >> 2;
                const double x = S[p][b], y = S[q][b];
                S[p][b] = c * x - s * y;
                S[q][b] = s * x + c * y;
            }
            __syncthreads();
        }
    }
    int best = 0;
    double lmin = S[0][0];
    for (int i = 1; i < 9; i++)
        if (S[i][i] < lmin) lmin = S[i][i], best = i;
    float Mn[9];
#pragma unroll
    for (int k = 0; k < 9; k++) Mn[k] = (float)V[k][best];
    const float T1[9] = {s1x, 0.f, -m1x * s1x, 0.f, s1y, -m1y * s1y, 0.f, 0.f, 1.f};
    const float T2[9] = {s2x, 0.f, -m2x * s2x, 0.f, s2y, -m2y * s2y, 0.f, 0.f, 1.f};
    float M21[9], M12[9], tmp[9];
    if (model == 0) {
        float T2inv[9];
        inv3(T2, T2inv);
        mul3(T2inv, Mn, tmp);
        mul3(tmp, T1, M21);
        inv3(M21, M12);
    } else {
        // rank 2: Fpre minus its smallest singular triple, (Fpre v3) v3^T
        double G[3][3], E[3][3];
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++)
                G[i][j] = (double)Mn[i] * Mn[j] + (double)Mn[3 + i] * Mn[3 + j] + (double)Mn[6 + i] * Mn[6 + j];
        jacobi_sym<double, 3>(G, E, JS_SWEEPS, JS_TOL);
        int e = 0;
        double lm = G[0][0];
        if (G[1][1] < lm) lm = G[1][1], e = 1;
        if (G[2][2] < lm) lm = G[2][2], e = 2;
        double v3[3], w3[3];
#pragma unroll
        for (int r = 0; r < 3; r++) v3[r] = e == 0 ? E[r][0] : e == 1 ? E[r][1] : E[r][2];
#pragma unroll
        for (int r = 0; r < 3; r++) w3[r] = (double)Mn[3 * r] * v3[0] + (double)Mn[3 * r + 1] * v3[1] + (double)Mn[3 * r + 2] * v3[2];
        float Fn[9];
#pragma unroll
        for (int r = 0; r < 3; r++)
#pragma unroll
            for (int cc = 0; cc < 3; cc++) Fn[3 * r + cc] = (float)((double)Mn[3 * r + cc] - w3[r] * v3[cc]);
        const float T2t[9] = {T2[0], T2[3], T2[6], T2[1], T2[4], T2[7], T2[2], T2[5], T2[8]};
        mul3(T2t, Fn, tmp);
        mul3(tmp, T1, M21);
#pragma unroll
        for (int k = 0; k < 9; k++) M12[k] = 0.f;
    }
    // CheckHomography / CheckFundamental
    const float inv_sigma2 = (float)(1.0 / (double)(P.sigma * P.sigma));
    unsigned long long *mask = o_mask + P.mask_off + ((size_t)model * P.n_hyp + h) * P.words;
    float acc = 0.f;
    for (int base = 0; base < n; base += NT) {
        const int i = base + tid;
        bool in = false;
        if (i < n) {
            const float4 q = m[i];
            const float u1 = q.x, v1 = q.y, u2 = q.z, v2 = q.w;
            in = true;
            if (model == 0) {
                const float th = 5.991f;
                const float w2 = (float)(1.0 / (double)(M12[6] * u2 + M12[7] * v2 + M12[8]));
                const float u2in1 = (M12[0] * u2 + M12[1] * v2 + M12[2]) * w2;
                const float v2in1 = (M12[3] * u2 + M12[4] * v2 + M12[5]) * w2;
                const float chi1 = ((u1 - u2in1) * (u1 - u2in1) + (v1 - v2in1) * (v1 - v2in1)) * inv_sigma2;
                if (chi1 > th) in = false;
                else acc += th - chi1;
                const float w1 = (float)(1.0 / (double)(M21[6] * u1 + M21[7] * v1 + M21[8]));
                const float u1in2 = (M21[0] * u1 + M21[1] * v1 + M21[2]) * w1;
                const float v1in2 = (M21[3] * u1 + M21[4] * v1 + M21[5]) * w1;
                const float chi2 = ((u2 - u1in2) * (u2 - u1in2) + (v2 - v1in2) * (v2 - v1in2)) * inv_sigma2;
                if (chi2 > th) in = false;
                else acc += th - chi2;
            } else {
                const float th = 3.841f, th_score = 5.991f;
                const float a2 = M21[0] * u1 + M21[1] * v1 + M21[2];
                const float b2 = M21[3] * u1 + M21[4] * v1 + M21[5];
                const float c2 = M21[6] * u1 + M21[7] * v1 + M21[8];
                const float num2 = a2 * u2 + b2 * v2 + c2;
                const float chi1 = num2 * num2 / (a2 * a2 + b2 * b2) * inv_sigma2;
                if (chi1 > th) in = false;
                else acc += th_score - chi1;
                const float a1 = M21[0] * u2 + M21[3] * v2 + M21[6];
                const float b1 = M21[1] * u2 + M21[4] * v2 + M21[7];
                const float c1 = M21[2] * u2 + M21[5] * v2 + M21[8];
                const float num1 = a1 * u1 + b1 * v1 + c1;
                const float chi2 = num1 * num1 / (a1 * a1 + b1 * b1) * inv_sigma2;
                if (chi2 > th) in = false;
                else acc += th_score - chi2;
            }
        }
        const unsigned long long word = __ballot(in);
        const int w = (base >> 6) + wave;
        if (lane == 0 && w < P.words) mask[w] = word;
    }
    red[tid] = acc;
    for (int s = NT / 2; s > 0; s >>= 1) {
        __syncthreads();
        if (tid < s) red[tid] += red[tid + s];
    }
    if (tid == 0) {
        const size_t g = (size_t)P.hyp_off + h;
        const float sc = red[0];
        o_score[2 * g + model] = (sc - sc == 0.f) ? sc : 0.f;  // NaN or inf: never a winner
        float *o = o_model + 18 * g + 9 * model;
#pragma unroll
        for (int k = 0; k < 9; k++) o[k] = M21[k];
    }
}

// ---- choice of the model, motion hypotheses ---------------------------------------------------------
__device__ inline void set_cand(TOut &o, int c, const float *R, const float *t)
{
    for (int k = 0; k < 9; k++) o.cand_Rt[12 * c + k] = R[k];
    for (int k = 0; k < 3; k++) o.cand_Rt[12 * c + 9 + k] = t[k];
}

// ReconstructF up to the four (R, t): E = K^T F K, DecomposeE
__device__ inline void decompose_f(const float *F, const float *K, TOut &o)
{
    const float Kt[9] = {K[0], K[3], K[6], K[1], K[4], K[7], K[2], K[5], K[8]};
    float tmp[9], E[9], U[9], w[3], V[9];
    mul3(Kt, F, tmp);
    mul3(tmp, K, E);
    svd3(E, U, w, V);
    float t[3] = {U[2], U[5], U[8]};
    const float nt = sqrtf(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]);
    for (int k = 0; k < 3; k++) t[k] = t[k] / nt;
    const float W[9] = {0.f, -1.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f};
    const float Wt[9] = {0.f, 1.f, 0.f, -1.f, 0.f, 0.f, 0.f, 0.f, 1.f};
    const float Vt[9] = {V[0], V[3], V[6], V[1], V[4], V[7], V[2], V[5], V[8]};
    float R1[9], R2[9];
    mul3(U, W, tmp);
    mul3(tmp, Vt, R1);
    if (det3(R1) < 0)
        for (int k = 0; k < 9; k++) R1[k] = -R1[k];
    mul3(U, Wt, tmp);
    mul3(tmp, Vt, R2);
    if (det3(R2) < 0)
        for (int k = 0; k < 9; k++) R2[k] = -R2[k];
    const float t2[3] = {-t[0], -t[1], -t[2]};
    set_cand(o, 0, R1, t);
    set_cand(o, 1, R2, t);
    set_cand(o, 2, R1, t2);
    set_cand(o, 3, R2, t2);
    o.n_cand = 4;
}

// ReconstructH up to the eight (R, t) (Faugeras); n_cand = 0 on the early return
__device__ inline void decompose_h(const float *H, const float *K, TOut &o)
{
    float invK[9], tmp[9], A[9], U[9], w[3], V[9];
    inv3(K, invK);
    mul3(invK, H, tmp);
    mul3(tmp, K, A);
    svd3(A, U, w, V);
    const float Vt[9] = {V[0], V[3], V[6], V[1], V[4], V[7], V[2], V[5], V[8]};
    const float s = det3(U) * det3(Vt);
    const float d1 = w[0], d2 = w[1], d3 = w[2];
    o.n_cand = 0;
    // singular values that are not finite (a NaN or inf homography): the reference goes on to eight NaN
    // hypotheses, none of which triangulates anything; here, as in the restatement, there are none
    if (!(isfinite(d1) && isfinite(d2) && isfinite(d3))) return;
    if (d1 / d2 < 1.00001 || d2 / d3 < 1.00001) return;
    const float aux1 = sqrtf((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3));
    const float aux3 = sqrtf((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3));
    const float x1[4] = {aux1, aux1, -aux1, -aux1};
    const float x3[4] = {aux3, -aux3, aux3, -aux3};
    const float aux_stheta = sqrtf((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 + d3) * d2);
    const float ctheta = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2);
    const float stheta[4] = {aux_stheta, -aux_stheta, -aux_stheta, aux_stheta};
    const float aux_sphi = sqrtf((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 - d3) * d2);
    const float cphi = (d1 * d3 - d2 * d2) / ((d1 - d3) * d2);
    const float sphi[4] = {aux_sphi, -aux_sphi, -aux_sphi, aux_sphi};
    float sU[9];
    for (int k = 0; k < 9; k++) sU[k] = s * U[k];
    for (int c = 0; c < 8; c++) {
        const int i = c & 3;
        float Rp[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        float tp[3];
        if (c < 4) {
            Rp[0] = ctheta, Rp[2] = -stheta[i], Rp[4] = 1.f, Rp[6] = stheta[i], Rp[8] = ctheta;
            tp[0] = x1[i] * (d1 - d3), tp[1] = 0.f * (d1 - d3), tp[2] = -x3[i] * (d1 - d3);
        } else {
            Rp[0] = cphi, Rp[2] = sphi[i], Rp[4] = -1.f, Rp[6] = sphi[i], Rp[8] = -cphi;
            tp[0] = x1[i] * (d1 + d3), tp[1] = 0.f * (d1 + d3), tp[2] = x3[i] * (d1 + d3);
        }
        float R[9], t[3];
        mul3(sU, Rp, tmp);
        mul3(tmp, Vt, R);
        for (int r = 0; r < 3; r++) t[r] = U[3 * r] * tp[0] + U[3 * r + 1] * tp[1] + U[3 * r + 2] * tp[2];
        const float nt = sqrtf(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]);
        for (int r = 0; r < 3; r++) t[r] = t[r] / nt;
        set_cand(o, c, R, t);
    }
    o.n_cand = 8;
}

__global__ __launch_bounds__(64) void k_tvr_select(const TProbDev *__restrict__ probs, const float *__restrict__ scores,
                                                   const float *__restrict__ models,
                                                   const unsigned long long *__restrict__ masks, TOut *__restrict__ out,
                                                   uint8_t *__restrict__ inl_h, uint8_t *__restrict__ inl_f)
{
    __shared__ int sh[3];
    const TProbDev &P = probs[blockIdx.x];
    const int lane = threadIdx.x;
    TOut &o = out[blockIdx.x];
    if (lane == 0) {
        float best[2] = {0.f, 0.f};
        int hyp[2] = {-1, -1};
        for (int h = 0; h < P.n_hyp; h++)
            for (int md = 0; md < 2; md++) {
                const float sc = scores[2 * ((size_t)P.hyp_off + h) + md];
                if (sc > best[md]) best[md] = sc, hyp[md] = h;
            }
        o.ok = 0, o.cand = -1, o.n_cand = 0, o.n_inliers = 0, o.pad = 0;
        o.hyp_h = hyp[0], o.hyp_f = hyp[1], o.score_h = best[0], o.score_f = best[1];
        for (int k = 0; k < 9; k++) {
            o.H21[k] = hyp[0] >= 0 ? models[18 * ((size_t)P.hyp_off + hyp[0]) + k] : 0.f;
            o.F21[k] = hyp[1] >= 0 ? models[18 * ((size_t)P.hyp_off + hyp[1]) + 9 + k] : 0.f;
            o.R[k] = k % 4 == 0 ? 1.f : 0.f;
        }
        o.t[0] = o.t[1] = o.t[2] = 0.f;
        for (int c = 0; c < 8; c++) o.n_good[c] = 0, o.parallax[c] = 0.f;
        for (int k = 0; k < 96; k++) o.cand_Rt[k] = 0.f;
        const float K[9] = {P.K[0], 0.f, P.K[2], 0.f, P.K[1], P.K[3], 0.f, 0.f, 1.f};
        if (best[0] + best[1] == 0.f) {
            o.model = -1;
        } else {
            const float RH = best[0] / (best[0] + best[1]);
            if (RH > 0.50) {
                o.model = 0;
                decompose_h(o.H21, K, o);
            } else {
                o.model = 1;
                decompose_f(o.F21, K, o);
            }
        }
        sh[0] = hyp[0], sh[1] = hyp[1], sh[2] = o.model;
    }
    __syncthreads();
    const int hh = sh[0], hf = sh[1], model = sh[2];
    const unsigned long long *mh = masks + P.mask_off + (size_t)(hh < 0 ? 0 : hh) * P.words;
    const unsigned long long *mf = masks + P.mask_off + ((size_t)P.n_hyp + (hf < 0 ? 0 : hf)) * P.words;
    const int ch = expand_mask(hh < 0 ? nullptr : mh, P.n, inl_h + P.pt_off, lane);
    const int cf = expand_mask(hf < 0 ? nullptr : mf, P.n, inl_f + P.pt_off, lane);
    int cnt = model == 0 ? ch : model == 1 ? cf : 0;
    for (int d = 32; d > 0; d >>= 1) cnt += __shfl_xor(cnt, d);
    if (lane == 0) o.n_inliers = cnt;
}

// ---- CheckRT ---------------------------------------------------------------------------------------
// floats ordered as unsigned integers (NaN above everything finite)
__device__ __forceinline__ unsigned ordered_key(float f)
{
    const unsigned b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float from_ordered_key(unsigned k)
{
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// per match and motion hypothesis: flag 0 = not counted, 1 = counted in nGood, 3 = counted and vbGood
__global__ __launch_bounds__(NT) void k_tvr_checkrt(const TProbDev *__restrict__ probs, const float4 *__restrict__ kp,
                                                    const uint8_t *__restrict__ inl_h, const uint8_t *__restrict__ inl_f,
                                                    TOut *__restrict__ out, float *__restrict__ w_p3d,
                                                    unsigned *__restrict__ w_cos, uint8_t *__restrict__ w_flag)
{
    __shared__ int s_cnt;
    const TProbDev &P = probs[blockIdx.y];
    TOut &o = out[blockIdx.y];
    const int c = blockIdx.x;
    if (c >= o.n_cand) return;  // the whole workgroup
    const int n = P.n, tid = threadIdx.x;
    const float4 *m = kp + P.pt_off;
    const uint8_t *inl = (o.model == 0 ? inl_h : inl_f) + P.pt_off;
    float *p3d = w_p3d + 3 * (8 * (size_t)P.pt_off + (size_t)c * n);
    unsigned *cosk = w_cos + 8 * (size_t)P.pt_off + (size_t)c * n;
    uint8_t *flag = w_flag + 8 * (size_t)P.pt_off + (size_t)c * n;
    float R[9], t[3];
    for (int k = 0; k < 9; k++) R[k] = o.cand_Rt[12 * c + k];
    for (int k = 0; k < 3; k++) t[k] = o.cand_Rt[12 * c + 9 + k];
    const float fx = P.K[0], fy = P.K[1], cx = P.K[2], cy = P.K[3];
    const float th2 = (float)(4.0 * (double)(P.sigma * P.sigma));
    // P2 = K [R | t]
    float P2[12];
    for (int j = 0; j < 4; j++) {
        const float r0 = j < 3 ? R[j] : t[0], r1 = j < 3 ? R[3 + j] : t[1], r2 = j < 3 ? R[6 + j] : t[2];
        P2[j] = fx * r0 + 0.f * r1 + cx * r2;
        P2[4 + j] = 0.f * r0 + fy * r1 + cy * r2;
        P2[8 + j] = 0.f * r0 + 0.f * r1 + 1.f * r2;
    }
    // O2 = -R^T t
    float O2[3];
    for (int j = 0; j < 3; j++) O2[j] = -R[j] * t[0] + -R[3 + j] * t[1] + -R[6 + j] * t[2];
    if (tid == 0) s_cnt = 0;
    __syncthreads();
    int mine = 0;
    for (int base = 0; base < n; base += NT) {
        const int i = base + tid;
        if (i >= n) break;
        uint8_t fl = 0;
        unsigned key = 0xffffffffu;
        float X = 0.f, Y = 0.f, Z = 0.f;
        if (inl[i]) {
            const float4 q = m[i];
            // Triangulate: rows x P.row(2) - P.row(0), y P.row(2) - P.row(1) of both cameras
            float A[4][4];
            A[0][0] = q.x * 0.f - fx, A[0][1] = q.x * 0.f - 0.f, A[0][2] = q.x * 1.f - cx, A[0][3] = q.x * 0.f - 0.f;
            A[1][0] = q.y * 0.f - 0.f, A[1][1] = q.y * 0.f - fy, A[1][2] = q.y * 1.f - cy, A[1][3] = q.y * 0.f - 0.f;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                A[2][j] = q.z * P2[8 + j] - P2[j];
                A[3][j] = q.w * P2[8 + j] - P2[4 + j];
            }
            double G[4][4], E[4][4];
#pragma unroll
            for (int a = 0; a < 4; a++)
#pragma unroll
                for (int b = 0; b < 4; b++)
                    G[a][b] = (double)A[0][a] * A[0][b] + (double)A[1][a] * A[1][b] + (double)A[2][a] * A[2][b] + (double)A[3][a] * A[3][b];
            jacobi_sym<double, 4>(G, E, JS_SWEEPS, JS_TOL);
            int e = 0;
            double lm = G[0][0];
#pragma unroll
            for (int a = 1; a < 4; a++)
                if (G[a][a] < lm) lm = G[a][a], e = a;
            float xh[4];
#pragma unroll
            for (int a = 0; a < 4; a++) xh[a] = (float)(e == 0 ? E[a][0] : e == 1 ? E[a][1] : e == 2 ? E[a][2] : E[a][3]);
            if (xh[3] != 0.f) {  // Triangulate fails on w == 0
                X = xh[0] / xh[3], Y = xh[1] / xh[3], Z = xh[2] / xh[3];
                if (isfinite(X) && isfinite(Y) && isfinite(Z)) {
                    const float dist1 = sqrtf(X * X + Y * Y + Z * Z);
                    const float n2x = X - O2[0], n2y = Y - O2[1], n2z = Z - O2[2];
                    const float dist2 = sqrtf(n2x * n2x + n2y * n2y + n2z * n2z);
                    const float cosp = (X * n2x + Y * n2y + Z * n2z) / (dist1 * dist2);
                    bool good = !(Z <= 0 && cosp < 0.99998);
                    const float X2 = R[0] * X + R[1] * Y + R[2] * Z + t[0];
                    const float Y2 = R[3] * X + R[4] * Y + R[5] * Z + t[1];
                    const float Z2 = R[6] * X + R[7] * Y + R[8] * Z + t[2];
                    good = good && !(Z2 <= 0 && cosp < 0.99998);
                    const float invZ1 = (float)(1.0 / (double)Z);
                    const float im1x = fx * X * invZ1 + cx, im1y = fy * Y * invZ1 + cy;
                    const float e1 = (im1x - q.x) * (im1x - q.x) + (im1y - q.y) * (im1y - q.y);
                    good = good && !(e1 > th2);
                    const float invZ2 = (float)(1.0 / (double)Z2);
                    const float im2x = fx * X2 * invZ2 + cx, im2y = fy * Y2 * invZ2 + cy;
                    const float e2 = (im2x - q.z) * (im2x - q.z) + (im2y - q.w) * (im2y - q.w);
                    good = good && !(e2 > th2);
                    if (good) {
                        fl = cosp < 0.99998 ? 3 : 1;
                        key = ordered_key(cosp);
                        mine++;
                    }
                }
            }
        }
        flag[i] = fl;
        cosk[i] = key;
        p3d[3 * i] = X, p3d[3 * i + 1] = Y, p3d[3 * i + 2] = Z;
    }
    atomicAdd(&s_cnt, mine);  // integers: the order does not matter
    __syncthreads();
    const int n_good = s_cnt;
    float parallax = 0.f;
    if (n_good > 0) {
        // the key of rank k = min(50, nGood - 1): the smallest v with #(key <= v) >= k + 1
        const int k = n_good - 1 < 50 ? n_good - 1 : 50;
        unsigned lo = 0u, hi = 0xffffffffu;
        while (lo < hi) {  // workgroup-uniform
            const unsigned mid = lo + ((hi - lo) >> 1);
            __syncthreads();
            if (tid == 0) s_cnt = 0;
            __syncthreads();
            int cn = 0;
            for (int i = tid; i < n; i += NT) cn += cosk[i] <= mid ? 1 : 0;
            if (cn) atomicAdd(&s_cnt, cn);
            __syncthreads();
            if (s_cnt >= k + 1) hi = mid;
            else lo = mid + 1;
        }
        const float cosv = from_ordered_key(lo);
        parallax = (float)((double)(acosf(cosv) * 180.f) / 3.1415926535897932384626433832795);
    }
    if (tid == 0) o.n_good[c] = n_good, o.parallax[c] = parallax;
}

// ---- acceptance and scatter ------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void k_tvr_final(const TProbDev *__restrict__ probs, TOut *__restrict__ out,
                                                  const int *__restrict__ idx1, const float *__restrict__ w_p3d,
                                                  const uint8_t *__restrict__ w_flag, float *__restrict__ o_p3d,
                                                  uint8_t *__restrict__ o_tri)
{
    __shared__ int s_ok, s_cand;
    const TProbDev &P = probs[blockIdx.x];
    TOut &o = out[blockIdx.x];
    const int tid = threadIdx.x;
    if (tid == 0) {
        osg_tvr_choice ch;
        ch.ok = 0, ch.cand = -1;
        if (o.n_cand == 4) ch = osg_tvr_choose_f(o.n_good, o.parallax, o.n_inliers, P.min_parallax, P.min_triangulated);
        if (o.n_cand == 8) ch = osg_tvr_choose_h(o.n_good, o.parallax, o.n_inliers, P.min_parallax, P.min_triangulated);
        o.ok = ch.ok, o.cand = ch.cand;
        if (ch.ok) {
            for (int k = 0; k < 9; k++) o.R[k] = o.cand_Rt[12 * ch.cand + k];
            for (int k = 0; k < 3; k++) o.t[k] = o.cand_Rt[12 * ch.cand + 9 + k];
        }
        s_ok = ch.ok, s_cand = ch.cand;
    }
    float *p3d = o_p3d + 3 * (size_t)P.key1_off;
    uint8_t *tri = o_tri + P.key1_off;
    for (int i = tid; i < P.n_keys1; i += NT) p3d[3 * i] = 0.f, p3d[3 * i + 1] = 0.f, p3d[3 * i + 2] = 0.f, tri[i] = 0;
    __syncthreads();
    if (!s_ok) return;
    const int n = P.n, c = s_cand;
    const float *src = w_p3d + 3 * (8 * (size_t)P.pt_off + (size_t)c * n);
    const uint8_t *flag = w_flag + 8 * (size_t)P.pt_off + (size_t)c * n;
    const int *ix = idx1 + P.pt_off;
    for (int i = tid; i < n; i += NT) {
        const uint8_t fl = flag[i];
        if (!fl) continue;
        const int k = ix[i];  // checked by the host: strictly increasing in [0, n_keys1)
        p3d[3 * k] = src[3 * i], p3d[3 * k + 1] = src[3 * i + 1], p3d[3 * k + 2] = src[3 * i + 2];
        tri[k] = fl == 3 ? 1 : 0;
    }
}

// osg_two_view_kernel_times: per-launch HIP events of this thread's calls (tools/twoview_bench.py)
struct KernelEvents {
    hipEvent_t e[4] = {nullptr, nullptr, nullptr, nullptr};
    ~KernelEvents()
    {
        for (hipEvent_t x : e)
            if (x) (void)hipEventDestroy(x);
    }
};
thread_local bool tv_ktime = false;
thread_local float tv_kms[5] = {0.f, 0.f, 0.f, 0.f, 0.f};

}  // namespace

extern "C" {

int osg_two_view_kernel_times(osg_ctx *ctx, int32_t enable, float *ms)
{
    if (!ctx) return OSG_E_INVALID;
    tv_ktime = enable != 0;
    if (ms)
        for (int k = 0; k < 5; k++) ms[k] = tv_kms[k];
    return 0;
}

int osg_two_view_reconstruct_batch(osg_ctx *ctx, const osg_two_view_problem *p, int32_t nb, osg_two_view_result *r)
{
    if (!ctx) return OSG_E_INVALID;
    OSG_REQUIRE(ctx, nb >= 0 && (nb == 0 || (p && r)), "null argument");
    if (nb == 0) return 0;
    std::vector<TProbDev> hp;
    std::vector<int> src;  // hp[k] is problem src[k]
    hp.reserve(nb);
    size_t n_pts = 0, n_hyp = 0, n_words = 0, n_k1 = 0, n_k2 = 0;
    int max_hyp = 0;
    for (int b = 0; b < nb; b++) {
        const osg_two_view_problem &q = p[b];
        OSG_REQUIRE(ctx, q.n >= 0 && q.n_hyp >= 1 && q.n_keys1 >= 0 && q.n_keys2 >= 0, "n, n_hyp or n_keys");
        OSG_REQUIRE(ctx, q.n == 0 || (r[b].inlier_h && r[b].inlier_f), "inlier arrays");
        OSG_REQUIRE(ctx, q.n_keys1 == 0 || (r[b].p3d && r[b].triangulated), "p3d / triangulated arrays");
        if (q.n < 8) continue;
        OSG_REQUIRE(ctx, q.kp1 && q.kp2 && q.keys1 && q.keys2 && q.idx1 && q.idx2 && q.sets, "match arrays");
        for (int i = 0; i < q.n; i++) {
            OSG_REQUIRE(ctx, q.idx1[i] >= 0 && q.idx1[i] < q.n_keys1 && (i == 0 || q.idx1[i] > q.idx1[i - 1]),
                        "idx1 not strictly increasing in [0, n_keys1) at match %d of problem %d", i, b);
            OSG_REQUIRE(ctx, q.idx2[i] >= 0 && q.idx2[i] < q.n_keys2, "idx2 outside [0, n_keys2) at match %d of problem %d", i, b);
        }
        int h_bad = -1;
        const int why = check_sets(q.sets, 8, q.n_hyp, q.n, &h_bad);
        OSG_REQUIRE(ctx, why != 1, "set index outside [0, n) in hypothesis %d of problem %d", h_bad, b);
        OSG_REQUIRE(ctx, why != 2, "repeated set index in hypothesis %d of problem %d", h_bad, b);
        TProbDev d;
        std::memset(&d, 0, sizeof d);
        d.n = q.n, d.n_hyp = q.n_hyp, d.n_keys1 = q.n_keys1, d.n_keys2 = q.n_keys2;
        d.pt_off = (int)n_pts, d.key1_off = (int)n_k1, d.key2_off = (int)n_k2, d.hyp_off = (int)n_hyp;
        d.words = (q.n + 63) / 64;
        d.min_triangulated = q.min_triangulated;
        d.mask_off = (long long)n_words;
        std::memcpy(d.K, q.K, sizeof d.K);
        d.sigma = q.sigma, d.min_parallax = q.min_parallax;
        n_pts += (size_t)q.n, n_k1 += (size_t)q.n_keys1, n_k2 += (size_t)q.n_keys2, n_hyp += (size_t)q.n_hyp;
        n_words += 2 * (size_t)d.words * q.n_hyp;
        max_hyp = std::max(max_hyp, q.n_hyp);
        hp.push_back(d);
        src.push_back(b);
        OSG_REQUIRE(ctx, n_pts < (size_t(1) << 24) && n_hyp < (size_t(1) << 22) && n_k1 < (size_t(1) << 26) && n_k2 < (size_t(1) << 26),
                    "too many matches, keypoints or hypotheses in one batch");
    }
    const int na = (int)hp.size();
    OSG_REQUIRE(ctx, na <= 65535, "too many problems in one batch");
    osg_batch_io io(ctx);
    // kp: a float4 (kp1, kp2) per match
    const osg_seg i_pr = io.in(sizeof(TProbDev), na), i_kp = io.in(sizeof(float4), n_pts), i_k1 = io.in(2 * sizeof(float), n_k1);
    const osg_seg i_k2 = io.in(2 * sizeof(float), n_k2), i_ix = io.in(sizeof(int32_t), n_pts), i_st = io.in(8 * sizeof(int32_t), n_hyp);
    // the scores (an H, F pair per hypothesis) and the models are downloaded on request
    const osg_seg o_res = io.out(sizeof(TOut), na), o_ih = io.out(1, n_pts), o_if = io.out(1, n_pts), o_tr = io.out(1, n_k1);
    const osg_seg o_p3 = io.out(3 * sizeof(float), n_k1), o_sc = io.out(2 * sizeof(float), n_hyp), o_md = io.out(18 * sizeof(float), n_hyp);
    // every problem starts as one that evaluates nothing
    for (int b = 0; b < nb; b++) {
        osg_two_view_result &o = r[b];
        const osg_two_view_problem &q = p[b];
        o.ok = 0, o.model = -1, o.score_h = o.score_f = 0.f, o.hyp_h = o.hyp_f = -1, o.cand = -1, o.n_inliers = 0;
        for (int j = 0; j < 9; j++) o.H21[j] = o.F21[j] = 0.f, o.R[j] = (j % 4 == 0) ? 1.f : 0.f;
        o.t[0] = o.t[1] = o.t[2] = 0.f;
        for (int j = 0; j < 8; j++) o.n_good[j] = 0, o.parallax[j] = 0.f;
        std::memset(o.cand_Rt, 0, sizeof o.cand_Rt);
        if (q.n_keys1 > 0) std::memset(o.p3d, 0, o_p3.elem * q.n_keys1), std::memset(o.triangulated, 0, (size_t)q.n_keys1);
        if (q.n > 0) std::memset(o.inlier_h, 0, (size_t)q.n), std::memset(o.inlier_f, 0, (size_t)q.n);
        if (o.hyp_score_h) std::memset(o.hyp_score_h, 0, o_sc.elem / 2 * q.n_hyp);
        if (o.hyp_score_f) std::memset(o.hyp_score_f, 0, o_sc.elem / 2 * q.n_hyp);
        if (o.hyp_models) std::memset(o.hyp_models, 0, o_md.elem * q.n_hyp);
    }
    if (na == 0) return 0;
    bool want_hyp = false;
    for (int k = 0; k < na; k++) want_hyp = want_hyp || r[src[k]].hyp_score_h || r[src[k]].hyp_score_f || r[src[k]].hyp_models;
    const size_t dl_bytes = want_hyp ? io.out_bytes : o_sc.off;
    // work: norm | p3d of 8 candidates | cos keys | flags
    size_t work_bytes = 0;
    osg_seg_add(work_bytes, 8 * sizeof(float), na);
    const size_t w_p3 = osg_seg_add(work_bytes, 8 * 3 * sizeof(float), n_pts).off;
    const size_t w_cs = osg_seg_add(work_bytes, 8 * sizeof(unsigned), n_pts).off;
    const size_t w_fl = osg_seg_add(work_bytes, 8, n_pts).off;
    OSG_RC(io.stage());
    io.put(i_pr, 0, hp.data(), na);
    for (int k = 0; k < na; k++) {
        const osg_two_view_problem &q = p[src[k]];
        float *kp = io.host_in<float>(i_kp, hp[k].pt_off);
        for (int i = 0; i < q.n; i++) {
            kp[4 * i] = q.kp1[2 * i], kp[4 * i + 1] = q.kp1[2 * i + 1];
            kp[4 * i + 2] = q.kp2[2 * i], kp[4 * i + 3] = q.kp2[2 * i + 1];
        }
        io.put(i_k1, hp[k].key1_off, q.keys1, q.n_keys1);
        io.put(i_k2, hp[k].key2_off, q.keys2, q.n_keys2);
        io.put(i_ix, hp[k].pt_off, q.idx1, q.n);
        io.put(i_st, hp[k].hyp_off, q.sets, q.n_hyp);
    }
    OSG_RC(io.upload());
    char *dwork = nullptr;
    unsigned long long *dmask = nullptr;
    OSG_ALLOC(ctx, dmask, SLOT_BA2, 8 * n_words);
    OSG_ALLOC(ctx, dwork, SLOT_BA3, work_bytes);
    OSG_RC(io.start());
    hipEvent_t *ev = io.ev;
    KernelEvents kevs;  // between the five launches, on request; destroyed on every way out
    hipEvent_t(&kev)[4] = kevs.e;
    const bool ktime = tv_ktime;
    if (ktime)
        for (auto &e : kev) OSG_HIP_CHECK(ctx, hipEventCreate(&e));
    const TProbDev *dp = io.dev_in<const TProbDev>(i_pr);
    const float4 *dkp = io.dev_in<const float4>(i_kp);
    TOut *dres = io.dev_out<TOut>(o_res);
    hipLaunchKernelGGL(k_tvr_norm, dim3(2, na), dim3(NT), 0, ctx->stream, dp, io.dev_in<const float>(i_k1),
                       io.dev_in<const float>(i_k2), (float *)dwork);
    OSG_HIP_CHECK(ctx, hipGetLastError());
    if (ktime) OSG_HIP_CHECK(ctx, hipEventRecord(kev[0], ctx->stream));
    hipLaunchKernelGGL(k_tvr_eval, dim3(max_hyp, 2, na), dim3(NT), 0, ctx->stream, dp, dkp, io.dev_in<const int>(i_st),
                       (const float *)dwork, io.dev_out<float>(o_sc), io.dev_out<float>(o_md), dmask);
    OSG_HIP_CHECK(ctx, hipGetLastError());
    if (ktime) OSG_HIP_CHECK(ctx, hipEventRecord(kev[1], ctx->stream));
    hipLaunchKernelGGL(k_tvr_select, dim3(na), dim3(64), 0, ctx->stream, dp, io.dev_out<const float>(o_sc),
                       io.dev_out<const float>(o_md), (const unsigned long long *)dmask, dres, io.dev_out<uint8_t>(o_ih),
                       io.dev_out<uint8_t>(o_if));
    OSG_HIP_CHECK(ctx, hipGetLastError());
    if (ktime) OSG_HIP_CHECK(ctx, hipEventRecord(kev[2], ctx->stream));
    hipLaunchKernelGGL(k_tvr_checkrt, dim3(8, na), dim3(NT), 0, ctx->stream, dp, dkp, io.dev_out<const uint8_t>(o_ih),
                       io.dev_out<const uint8_t>(o_if), dres, (float *)(dwork + w_p3), (unsigned *)(dwork + w_cs),
                       (uint8_t *)(dwork + w_fl));
    OSG_HIP_CHECK(ctx, hipGetLastError());
    if (ktime) OSG_HIP_CHECK(ctx, hipEventRecord(kev[3], ctx->stream));
    hipLaunchKernelGGL(k_tvr_final, dim3(na), dim3(NT), 0, ctx->stream, dp, dres, io.dev_in<const int>(i_ix),
                       (const float *)(dwork + w_p3), (const uint8_t *)(dwork + w_fl), io.dev_out<float>(o_p3),
                       io.dev_out<uint8_t>(o_tr));
    OSG_HIP_CHECK(ctx, hipGetLastError());
    OSG_RC(io.finish(dl_bytes));
    if (ktime) {
        const hipEvent_t seq[6] = {ev[0], kev[0], kev[1], kev[2], kev[3], ev[1]};
        for (int k = 0; k < 5; k++) OSG_HIP_CHECK(ctx, hipEventElapsedTime(&tv_kms[k], seq[k], seq[k + 1]));
    }
    const TOut *res = io.result<TOut>(o_res);
    int n_ok = 0;
    for (int k = 0; k < na; k++) {
        const TOut &s = res[k];
        const TProbDev &d = hp[k];
        osg_two_view_result &o = r[src[k]];
        o.ok = s.ok, o.model = s.model, o.score_h = s.score_h, o.score_f = s.score_f, o.hyp_h = s.hyp_h, o.hyp_f = s.hyp_f;
        o.cand = s.cand, o.n_inliers = s.n_inliers;
        std::memcpy(o.H21, s.H21, sizeof o.H21);
        std::memcpy(o.F21, s.F21, sizeof o.F21);
        std::memcpy(o.R, s.R, sizeof o.R);
        std::memcpy(o.t, s.t, sizeof o.t);
        std::memcpy(o.n_good, s.n_good, sizeof o.n_good);
        std::memcpy(o.parallax, s.parallax, sizeof o.parallax);
        std::memcpy(o.cand_Rt, s.cand_Rt, sizeof o.cand_Rt);
        io.get(o.inlier_h, o_ih, d.pt_off, d.n);
        io.get(o.inlier_f, o_if, d.pt_off, d.n);
        io.get(o.triangulated, o_tr, d.key1_off, d.n_keys1);
        io.get(o.p3d, o_p3, d.key1_off, d.n_keys1);
        if (o.hyp_models) io.get(o.hyp_models, o_md, d.hyp_off, d.n_hyp);
        const float *sc = io.result<float>(o_sc, d.hyp_off);
        for (int h = 0; h < d.n_hyp && (o.hyp_score_h || o.hyp_score_f); h++) {
            if (o.hyp_score_h) o.hyp_score_h[h] = sc[2 * h];
            if (o.hyp_score_f) o.hyp_score_f[h] = sc[2 * h + 1];
        }
        n_ok += s.ok ? 1 : 0;
    }
    return n_ok;
}

int osg_two_view_reconstruct(osg_ctx *ctx, const osg_two_view_problem *p, osg_two_view_result *r)
{
    const int rc = osg_two_view_reconstruct_batch(ctx, p, 1, r);
    return rc < 0 ? rc : r->ok;
}

}  // extern "C"
