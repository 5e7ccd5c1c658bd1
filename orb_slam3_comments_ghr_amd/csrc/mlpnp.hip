// mlpnp.hip — MLPnPsolver's RANSAC (ref:src/MLPnPsolver.cpp:145-1160) for a batch of problems.
//
// Two launches in stream order:
//   k_mlpnp_eval    grid (hypothesis chunks, problems), 256 lanes = 4 waves, one hypothesis per wave.  The
//                   workgroup stages the problem's matches in LDS (world point, keypoint, bound: 6 floats
//                   per match) while they fit; past that the waves read global memory.  A wave runs
//                   computePose on its six sampled matches in double: the scalar steps (null-space bases,
//                   rank test, 3 x 3 eigen / SVD, sign choice, Gauss-Newton with a 6 x 6 LDL^T) are
//                   computed by all 64 lanes alike, the 12 x 12 (planar: 9 x 9) normal matrix is filled by
//                   the lanes in parallel and its smallest eigenvector comes from a cyclic Jacobi iteration
//                   on the wave's LDS tile, six disjoint pairs rotating at once (11 rounds per sweep).  Then
//                   the wave strides over the matches, 64 at a time: CheckInliers as written (double
//                   transform rounded once to float, float projection, `<`), __ballot -> one mask word,
//                   __popcll -> the count.  Per hypothesis: count, R t, info, mask words -> scratch.
//   k_mlpnp_select  one wave per problem: lane 0 replays the reference's sequential rule on the counts
//                   (mlpnp_select.h), the wave expands the chosen hypothesis's mask words to N bytes and
//                   writes its R, t and Tcw.
// No atomics and no in-launch hand-off: the result is the same bits every run.
#include <cfloat>
#include <cstring>
#include <vector>

#include "batch_io.h"
#include "mlpnp_select.h"
#include "ransac_common.h"

namespace {

constexpr int NT = 256;        // lanes per workgroup
constexpr int HPB = NT / 64;   // hypotheses per workgroup: one per wave
constexpr int FPM = 6;         // staged floats per match
constexpr int LDS_CAP = 160 * 1024;
// per-wave LDS tile, in doubles: A[12][12], V[12][12], r s per point [6][6], points [6][3], J [12][6]
constexpr int T_A = 0, T_V = 144, T_RS = 288, T_P = 324, T_J = 342, TILE = 416;
constexpr int TILE_BYTES = HPB * TILE * 8;

struct MProbDev {
    int n, n_hyp, min_inliers;
    int pt_off;          // first match in the concatenated match arrays
    int hyp_off;         // first hypothesis in the concatenated hypothesis arrays
    int words;           // mask words per hypothesis: ceil(n / 64)
    int staged;          // matches live in LDS
    int pad;
    long long mask_off;  // first mask word
    osg_camera cam;
};

struct MSelOut {
    int converged, hyp, n_iterations, n_inliers, n_best, pad[3];
    double R[9], t[3];
    float Tcw[16];
};

// the lanes of one wave exchange data through their LDS tile: order the accesses for the compiler (the
// hardware executes one wave's LDS instructions in order)
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ double det3(const double *m)
{
    return m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]);
}
__device__ __forceinline__ void cross3(const double *a, const double *b, double *c)
{
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}
__device__ __forceinline__ double norm3(const double *a) { return sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]); }

// an orthonormal basis r, s of null(f^T): r = f x e / |f x e| with e the axis of f's smallest component,
// s = f x r / |f x r|
__device__ inline void null_basis(const double *f, double *r, double *s)
{
    const double ax = fabs(f[0]), ay = fabs(f[1]), az = fabs(f[2]);
    double e[3] = {0, 0, 0};
    if (ax <= ay && ax <= az) e[0] = 1;
    else if (ay <= az) e[1] = 1;
    else e[2] = 1;
    cross3(f, e, r);
    double n = norm3(r);
    r[0] /= n, r[1] /= n, r[2] /= n;
    cross3(f, r, s);
    n = norm3(s);
    s[0] /= n, s[1] /= n, s[2] /= n;
}

// Eigen::FullPivHouseholderQR<Matrix3d>(M).rank() with the default threshold: pivots above
// epsilon * 3 * |largest pivot| count
__device__ inline int rank3(const double *M)
{
    double A[3][3] = {{M[0], M[1], M[2]}, {M[3], M[4], M[5]}, {M[6], M[7], M[8]}};
    double piv[3] = {0, 0, 0};
    const double prec = DBL_EPSILON * 3;
    double biggest = 0;
    int nonzero = 3;
    for (int k = 0; k < 3; k++) {
        int bi = k, bj = k;
        double big = fabs(A[k][k]);
        for (int j = k; j < 3; j++)
            for (int i = k; i < 3; i++)
                if (fabs(A[i][j]) > big) big = fabs(A[i][j]), bi = i, bj = j;
        if (k == 0) biggest = big;
        if (big <= biggest * prec) {
            nonzero = k;
            break;
        }
        for (int j = 0; j < 3; j++) {
            const double tmp = A[k][j];
            A[k][j] = A[bi][j], A[bi][j] = tmp;
        }
        for (int i = 0; i < 3; i++) {
            const double tmp = A[i][k];
            A[i][k] = A[i][bj], A[i][bj] = tmp;
        }
        const double x0 = A[k][k];
        double tail2 = 0;
        for (int i = k + 1; i < 3; i++) tail2 += A[i][k] * A[i][k];
        double beta = x0;
        if (!(tail2 <= DBL_MIN)) {
            beta = sqrt(x0 * x0 + tail2);
            if (x0 >= 0) beta = -beta;
            double v[3] = {0, 0, 0};
            v[k] = 1;
            for (int i = k + 1; i < 3; i++) v[i] = A[i][k] / (x0 - beta);
            const double tau = (beta - x0) / beta;
            for (int j = k + 1; j < 3; j++) {
                double dot = 0;
                for (int i = k; i < 3; i++) dot += v[i] * A[i][j];
                for (int i = k; i < 3; i++) A[i][j] -= tau * v[i] * dot;
            }
        }
        piv[k] = fabs(beta);
    }
    double maxp = 0;
    for (int k = 0; k < 3; k++)
        if (piv[k] > maxp) maxp = piv[k];
    const double thr = maxp * DBL_EPSILON * 3;
    int rank = 0;
    for (int k = 0; k < nonzero; k++) rank += piv[k] > thr;
    return rank;
}

// eigen-decomposition of the symmetric 3 x 3 S (row-major), ascending: cyclic Jacobi in double
__device__ inline void eig3_ascending(const double *S, double *G /* columns = eigenvectors, row-major */)
{
    double A[3][3] = {{S[0], S[1], S[2]}, {S[3], S[4], S[5]}, {S[6], S[7], S[8]}};
    double V[3][3];
    jacobi_sym<double, 3>(A, V, 16, 1e-40);
    // ascending order of the three diagonal entries
    int o0 = 0, o1 = 1, o2 = 2;
    double d0 = A[0][0], d1 = A[1][1], d2 = A[2][2];
    if (d1 < d0) { double t = d0; d0 = d1; d1 = t; int i = o0; o0 = o1; o1 = i; }
    if (d2 < d1) { double t = d1; d1 = d2; d2 = t; int i = o1; o1 = o2; o2 = i; }
    if (d1 < d0) { double t = d0; d0 = d1; d1 = t; int i = o0; o0 = o1; o1 = i; }
#pragma unroll
    for (int k = 0; k < 3; k++) {
        G[3 * k + 0] = o0 == 0 ? V[k][0] : o0 == 1 ? V[k][1] : V[k][2];
        G[3 * k + 1] = o1 == 0 ? V[k][0] : o1 == 1 ? V[k][1] : V[k][2];
        G[3 * k + 2] = o2 == 0 ? V[k][0] : o2 == 1 ? V[k][1] : V[k][2];
    }
}

// U V^T of the SVD of the 3 x 3 M (row-major): one-sided Jacobi on the columns, M J = U S, V = J.  A column
// that vanishes is replaced by the cross product of the other two.
__device__ inline void polar_uvt(const double *M, double *R)
{
    double m[3][3], v[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};  // [column][row]
#pragma unroll
    for (int j = 0; j < 3; j++)
#pragma unroll
        for (int i = 0; i < 3; i++) m[j][i] = M[3 * i + j];
#pragma unroll 1
    for (int sweep = 0; sweep < 30; sweep++) {
        bool rotated = false;
#pragma unroll
        for (int p = 0; p < 2; p++)
#pragma unroll
            for (int q = p + 1; q < 3; q++) {
                const double al = m[p][0] * m[p][0] + m[p][1] * m[p][1] + m[p][2] * m[p][2];
                const double be = m[q][0] * m[q][0] + m[q][1] * m[q][1] + m[q][2] * m[q][2];
                const double ga = m[p][0] * m[q][0] + m[p][1] * m[q][1] + m[p][2] * m[q][2];
                if (!(ga * ga > 1e-32 * al * be)) continue;
                double c, s;
                jacobi_rotation(al, be, ga, c, s);
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    const double a = m[p][k], b = m[q][k];
                    m[p][k] = c * a - s * b;
                    m[q][k] = s * a + c * b;
                    const double va = v[p][k], vb = v[q][k];
                    v[p][k] = c * va - s * vb;
                    v[q][k] = s * va + c * vb;
                }
                rotated = true;
            }
        if (!rotated) break;
    }
    double nrm[3], big = 0;
#pragma unroll
    for (int j = 0; j < 3; j++) {
        nrm[j] = norm3(m[j]);
        if (nrm[j] > big) big = nrm[j];
    }
#pragma unroll
    for (int j = 0; j < 3; j++)
        if (nrm[j] > 1e-14 * big) m[j][0] /= nrm[j], m[j][1] /= nrm[j], m[j][2] /= nrm[j];
    if (!(nrm[0] > 1e-14 * big)) cross3(m[1], m[2], m[0]);
    if (!(nrm[1] > 1e-14 * big)) cross3(m[2], m[0], m[1]);
    if (!(nrm[2] > 1e-14 * big)) cross3(m[0], m[1], m[2]);
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) R[3 * i + j] = m[0][i] * v[0][j] + m[1][i] * v[1][j] + m[2][i] * v[2][j];
}

// MLPnPsolver::rodrigues2rot (:1014-1033); a NaN omega leaves the identity, as there
__device__ inline void rodrigues2rot(const double *w, double *R)
{
    const double n = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
    const double K[9] = {0.0, -w[2], w[1], w[2], 0.0, -w[0], -w[1], w[0], 0.0};
#pragma unroll
    for (int k = 0; k < 9; k++) R[k] = (k % 4 == 0) ? 1.0 : 0.0;
    if (n > DBL_EPSILON) {
        const double a = sin(n) / n, b = (1 - cos(n)) / (n * n);
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++)
                R[3 * i + j] += a * K[3 * i + j] + b * (K[3 * i] * K[j] + K[3 * i + 1] * K[3 + j] + K[3 * i + 2] * K[6 + j]);
    }
}

// MLPnPsolver::rot2rodrigues (:1047-1076)
__device__ inline void rot2rodrigues(const double *R, double *w)
{
    w[0] = w[1] = w[2] = 0.0;
    const double trace = R[0] + R[4] + R[8] - 1.0;
    const double wnorm = acos(trace / 2.0);
    if (wnorm > DBL_EPSILON) {
        const double sc = wnorm / (2.0 * sin(wnorm));
        w[0] = (R[7] - R[5]) * sc;
        w[1] = (R[2] - R[6]) * sc;
        w[2] = (R[3] - R[1]) * sc;
    }
}

// sum over the six sample points of 1 - v^T f with v = (R p + t) / |R p + t|
__device__ inline double bearing_error(const double *R, const double *t, const double *tile, const double (*f)[3])
{
    double e = 0;
#pragma unroll 1
    for (int k = 0; k < 6; k++) {
        const double *p = tile + T_P + 3 * k;
        double v[3];
#pragma unroll
        for (int i = 0; i < 3; i++) v[i] = R[3 * i] * p[0] + R[3 * i + 1] * p[1] + R[3 * i + 2] * p[2] + t[i];
        const double n = norm3(v);
        e += 1.0 - (v[0] / n * f[k][0] + v[1] / n * f[k][1] + v[2] / n * f[k][2]);
    }
    return e;
}

// the larger of m and |a|, NaN sticking
__device__ __forceinline__ double amax_nan(double m, double a)
{
    a = fabs(a);
    return (a > m || a != a) ? a : m;
}

// computePose (ref:src/MLPnPsolver.cpp:483-1007) of one wave's sample: f, p the six bearings and world
// points (uniform over the wave), tile the wave's LDS tile.  -> R, t, info = planar, solves, end
__device__ inline void compute_pose(const double (*f)[3], const double (*p)[3], double *tile, int lane, double *Rout,
                                    double *tout, int *info, long long *prof)
{
#ifdef OSG_MLPNP_PROF
#define MLPNP_STAMP(k) prof[k] = wall_clock64()
#else
#define MLPNP_STAMP(k) (void)prof
#endif
    // 1. null-space bases; the points and bases go to the tile for the indexed reads below
    double S3[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < 6; i++)
#pragma unroll
        for (int a = 0; a < 3; a++)
#pragma unroll
            for (int b = 0; b < 3; b++) S3[3 * a + b] += p[i][a] * p[i][b];
    // 2. planar test
    const bool planar = rank3(S3) == 2;
    double G[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    if (planar) eig3_ascending(S3, G);
    if (lane < 6) {
        double r[3], s[3];
        null_basis(f[lane], r, s);
#pragma unroll
        for (int k = 0; k < 3; k++) {
            tile[T_RS + 6 * lane + k] = r[k];
            tile[T_RS + 6 * lane + 3 + k] = s[k];
            tile[T_P + 3 * lane + k] = p[lane][k];
        }
    }
    wave_sync();
    // 3., 4. AtA: A's row of point i and basis vector n is [n (x) c_i, n] with c_i the (rotated) point, planar:
    // its last two coordinates
    const int N = planar ? 9 : 12, nc = planar ? 2 : 3;
    for (int e = lane; e < 144; e += 64) {
        const int a = e / 12, b = e % 12;
        double acc = 0;
        if (a < N && b < N) {
            const int ra = a < 3 * nc ? a / nc : a - 3 * nc, rb = b < 3 * nc ? b / nc : b - 3 * nc;
            for (int i = 0; i < 6; i++) {
                const double *rs = tile + T_RS + 6 * i, *pt = tile + T_P + 3 * i;
                double ca = 1.0, cb = 1.0;
                if (a < 3 * nc) {
                    const int j = a % nc + (3 - nc);
                    ca = planar ? G[j] * pt[0] + G[3 + j] * pt[1] + G[6 + j] * pt[2] : pt[j];
                }
                if (b < 3 * nc) {
                    const int j = b % nc + (3 - nc);
                    cb = planar ? G[j] * pt[0] + G[3 + j] * pt[1] + G[6 + j] * pt[2] : pt[j];
                }
                acc += (rs[ra] * ca) * (rs[rb] * cb) + (rs[3 + ra] * ca) * (rs[3 + rb] * cb);
            }
        }
        tile[T_A + e] = acc;
        tile[T_V + e] = a == b ? 1.0 : 0.0;
    }
    wave_sync();
    MLPNP_STAMP(1);
    // 5. smallest eigenvector: cyclic Jacobi on the tile, the 66 pairs of a sweep taken as 11 rounds of 6 disjoint
    // pairs (round-robin order) that rotate at once: lanes 0..5 work out one angle each, then all lanes apply
    // A <- J^T A J and V <- V J element by element.  A pair with an index past N is skipped.
    {
        double *A = tile + T_A, *V = tile + T_V;
        double *cc = tile + T_J, *ss = tile + T_J + 12, *pa = tile + T_J + 24;  // per index: c, +-s, partner
#pragma unroll 1
        for (int sweep = 0; sweep < 16; sweep++) {
            double off = 0, diag = 0;
            for (int i = 0; i < N; i++) {
                diag += A[13 * i] * A[13 * i];
                for (int j = i + 1; j < N; j++) off += A[12 * i + j] * A[12 * i + j];
            }
            if (!(off > 1e-40 * diag)) break;  // converged, zero, or NaN
#pragma unroll 1
            for (int round = 0; round < 11; round++) {
                if (lane < 6) {
                    int p = lane == 0 ? 11 : (round + lane) % 11, q = lane == 0 ? round : (round + 11 - lane) % 11;
                    if (p > q) {
                        const int tmp = p;
                        p = q, q = tmp;
                    }
                    double c = 1.0, sn = 0.0;
                    const double apq = q < N ? A[12 * p + q] : 0.0;
                    if (apq != 0.0) jacobi_rotation(A[13 * p], A[13 * q], apq, c, sn);
                    const bool rot = apq != 0.0;
                    cc[p] = c, ss[p] = -sn, pa[p] = rot ? (double)q : (double)p;
                    cc[q] = c, ss[q] = sn, pa[q] = rot ? (double)p : (double)q;
                }
                wave_sync();
                // B = A J and V J
                double nb[3], nv[3];
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    const int e = lane + 64 * k;
                    if (e < 144) {
                        const int i = e / 12, j = e % 12, jp = (int)pa[j];
                        nb[k] = cc[j] * A[e] + ss[j] * A[12 * i + jp];
                        nv[k] = cc[j] * V[e] + ss[j] * V[12 * i + jp];
                    }
                }
                wave_sync();
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    const int e = lane + 64 * k;
                    if (e < 144) A[e] = nb[k], V[e] = nv[k];
                }
                wave_sync();
                // A = J^T B; the rotated pair's own entry is zero by construction
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    const int e = lane + 64 * k;
                    if (e < 144) {
                        const int i = e / 12, j = e % 12, ip = (int)pa[i];
                        nb[k] = (ip != i && j == ip) ? 0.0 : cc[i] * A[e] + ss[i] * A[12 * ip + j];
                    }
                }
                wave_sync();
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    const int e = lane + 64 * k;
                    if (e < 144) A[e] = nb[k];
                }
                wave_sync();
            }
        }
    }
    double u[12];
    {
        const double *A = tile + T_A, *V = tile + T_V;
        int col = 0;
        double best = A[0];
        for (int i = 1; i < N; i++)
            if (A[13 * i] < best) best = A[13 * i], col = i;
        for (int i = 0; i < 12; i++) u[i] = i < N ? V[12 * i + col] : 0.0;
    }
    MLPNP_STAMP(2);
    // 6., 7. rotation, translation and the sign choice
    double R0[9], t0[3];
    if (planar) {
        double tmp[9] = {0.0, u[0], u[1], 0.0, u[2], u[3], 0.0, u[4], u[5]};
        {
            const double c1[3] = {tmp[1], tmp[4], tmp[7]}, c2[3] = {tmp[2], tmp[5], tmp[8]};
            double c0[3];
            cross3(c1, c2, c0);
            tmp[0] = c0[0], tmp[3] = c0[1], tmp[6] = c0[2];
        }
        double tt[9];
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) tt[3 * i + j] = tmp[3 * j + i];
        const double n1 = sqrt(tt[1] * tt[1] + tt[4] * tt[4] + tt[7] * tt[7]);
        const double n2 = sqrt(tt[2] * tt[2] + tt[5] * tt[5] + tt[8] * tt[8]);
        const double scale = 1.0 / sqrt(fabs(n1 * n2));
        double R1[9];
        polar_uvt(tt, R1);
        if (det3(R1) < 0)
#pragma unroll
            for (int k = 0; k < 9; k++) R1[k] = -R1[k];
        // Rout1 = eigenRot^T Rout1 = G Rout1, transposed, negated
        double Rb[9];
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) Rb[3 * j + i] = -(G[3 * i] * R1[j] + G[3 * i + 1] * R1[3 + j] + G[3 * i + 2] * R1[6 + j]);
        if (det3(Rb) < 0.0) Rb[2] = -Rb[2], Rb[5] = -Rb[5], Rb[8] = -Rb[8];
        const double t[3] = {scale * u[6], scale * u[7], scale * u[8]};
        double best = 0;
#pragma unroll 1
        for (int c = 0; c < 4; c++) {
            double Rc[9], tc[3];
            const double sr = c >= 2 ? -1.0 : 1.0, st = (c & 1) ? -1.0 : 1.0;
#pragma unroll
            for (int i = 0; i < 3; i++) {
                Rc[3 * i] = sr * Rb[3 * i], Rc[3 * i + 1] = sr * Rb[3 * i + 1], Rc[3 * i + 2] = Rb[3 * i + 2];
                tc[i] = st * t[i];
            }
            const double e = bearing_error(Rc, tc, tile, f);
            // std::min_element: the first minimum
            if (c == 0 || e < best) {
                best = e;
#pragma unroll
                for (int k = 0; k < 9; k++) R0[k] = Rc[k];
#pragma unroll
                for (int k = 0; k < 3; k++) t0[k] = tc[k];
            }
        }
    } else {
        const double tmp[9] = {u[0], u[3], u[6], u[1], u[4], u[7], u[2], u[5], u[8]};
        const double n0 = sqrt(tmp[0] * tmp[0] + tmp[3] * tmp[3] + tmp[6] * tmp[6]);
        const double n1 = sqrt(tmp[1] * tmp[1] + tmp[4] * tmp[4] + tmp[7] * tmp[7]);
        const double n2 = sqrt(tmp[2] * tmp[2] + tmp[5] * tmp[5] + tmp[8] * tmp[8]);
        const double scale = 1.0 / pow(fabs(n0 * n1 * n2), 1.0 / 3.0);
        double R[9];
        polar_uvt(tmp, R);
        if (det3(R) < 0)
#pragma unroll
            for (int k = 0; k < 9; k++) R[k] = -R[k];
        double t[3];
#pragma unroll
        for (int i = 0; i < 3; i++) t[i] = R[3 * i] * (scale * u[9]) + R[3 * i + 1] * (scale * u[10]) + R[3 * i + 2] * (scale * u[11]);
        // [R | +-t]^-1 = [R^T | -+R^T t]
        double ti[3];
#pragma unroll
        for (int i = 0; i < 3; i++) {
            R0[3 * i] = R[i], R0[3 * i + 1] = R[3 + i], R0[3 * i + 2] = R[6 + i];
            ti[i] = -(R[i] * t[0] + R[3 + i] * t[1] + R[6 + i] * t[2]);
        }
        const double tn[3] = {-ti[0], -ti[1], -ti[2]};
        const double e0 = bearing_error(R0, ti, tile, f), e1 = bearing_error(R0, tn, tile, f);
#pragma unroll
        for (int i = 0; i < 3; i++) t0[i] = e0 < e1 ? ti[i] : tn[i];
    }
    MLPNP_STAMP(3);
    // 8. mlpnp_gn (:1086-1160)
    double x[6];
    rot2rodrigues(R0, x);
    x[3] = t0[0], x[4] = t0[1], x[5] = t0[2];
    int solves = 0, end = 0;
#pragma unroll 1
    for (int it = 0; it < 5; it++) {
        double R[9];
        rodrigues2rot(x, R);
        const double th2 = x[0] * x[0] + x[1] * x[1] + x[2] * x[2];
        // S = (w w^T + (R^T - I) [w]x) / |w|^2
        const double K[9] = {0.0, -x[2], x[1], x[2], 0.0, -x[0], -x[1], x[0], 0.0};
        double S[9];
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) {
                double acc = x[i] * x[j];
#pragma unroll
                for (int k = 0; k < 3; k++) acc += (R[3 * k + i] - (k == i ? 1.0 : 0.0)) * K[3 * k + j];
                S[3 * i + j] = acc / th2;
            }
        double H[6][6], g[6];
#pragma unroll
        for (int a = 0; a < 6; a++) {
            g[a] = 0;
#pragma unroll
            for (int b = 0; b < 6; b++) H[a][b] = 0;
        }
        wave_sync();  // the previous iteration's reads of J are done
#pragma unroll 1
        for (int i = 0; i < 6; i++) {
            const double *pt = tile + T_P + 3 * i, *rs = tile + T_RS + 6 * i;
            double q[3];
#pragma unroll
            for (int a = 0; a < 3; a++) q[a] = R[3 * a] * pt[0] + R[3 * a + 1] * pt[1] + R[3 * a + 2] * pt[2] + x[3 + a];
            const double nq = norm3(q);
            const double v[3] = {q[0] / nq, q[1] / nq, q[2] / nq};
            // dq/dw = -R [p]x S
            const double PX[9] = {0.0, -pt[2], pt[1], pt[2], 0.0, -pt[0], -pt[1], pt[0], 0.0};
            double RP[9], dq[9];
#pragma unroll
            for (int a = 0; a < 3; a++)
#pragma unroll
                for (int b = 0; b < 3; b++) RP[3 * a + b] = R[3 * a] * PX[b] + R[3 * a + 1] * PX[3 + b] + R[3 * a + 2] * PX[6 + b];
#pragma unroll
            for (int a = 0; a < 3; a++)
#pragma unroll
                for (int b = 0; b < 3; b++) dq[3 * a + b] = -(RP[3 * a] * S[b] + RP[3 * a + 1] * S[3 + b] + RP[3 * a + 2] * S[6 + b]);
#pragma unroll
            for (int k = 0; k < 2; k++) {
                const double *n = rs + 3 * k;
                const double nv = n[0] * v[0] + n[1] * v[1] + n[2] * v[2];
                // n^T (I - v v^T) / |q|
                const double a3[3] = {(n[0] - nv * v[0]) / nq, (n[1] - nv * v[1]) / nq, (n[2] - nv * v[2]) / nq};
                double J[6];
#pragma unroll
                for (int b = 0; b < 3; b++) {
                    J[b] = a3[0] * dq[b] + a3[1] * dq[3 + b] + a3[2] * dq[6 + b];
                    J[3 + b] = a3[b];
                }
#pragma unroll
                for (int a = 0; a < 6; a++) {
                    g[a] += J[a] * nv;
#pragma unroll
                    for (int b = a; b < 6; b++) H[a][b] += J[a] * J[b];
                    if (lane == 0) tile[T_J + 6 * (2 * i + k) + a] = J[a];
                }
            }
        }
        wave_sync();
        solves++;
        // dx = H^-1 g by LDL^T (no pivoting)
        double L[6][6], d[6], dx[6];
#pragma unroll
        for (int j = 0; j < 6; j++) {
            double dj = H[j][j];
#pragma unroll
            for (int k = 0; k < j; k++) dj -= L[j][k] * L[j][k] * d[k];
            d[j] = dj;
#pragma unroll
            for (int i = j + 1; i < 6; i++) {
                double l = H[j][i];
#pragma unroll
                for (int k = 0; k < j; k++) l -= L[i][k] * L[j][k] * d[k];
                L[i][j] = l / dj;
            }
        }
#pragma unroll
        for (int i = 0; i < 6; i++) {
            double y = g[i];
#pragma unroll
            for (int k = 0; k < i; k++) y -= L[i][k] * dx[k];
            dx[i] = y;
        }
#pragma unroll
        for (int i = 0; i < 6; i++) dx[i] /= d[i];
#pragma unroll
        for (int i = 5; i >= 0; i--)
#pragma unroll
            for (int k = i + 1; k < 6; k++) dx[i] -= L[k][i] * dx[k];
        double mx = 0, mn = fabs(dx[0]);
#pragma unroll
        for (int i = 0; i < 6; i++) {
            mx = amax_nan(mx, dx[i]);
            if (fabs(dx[i]) < mn) mn = fabs(dx[i]);
        }
        if (mx > 5.0 || mn > 1.0) {
            end = 2;
            break;
        }
        double dl = 0;
#pragma unroll 1
        for (int r = 0; r < 12; r++) {
            const double *J = tile + T_J + 6 * r;
            dl = amax_nan(dl, J[0] * dx[0] + J[1] * dx[1] + J[2] * dx[2] + J[3] * dx[3] + J[4] * dx[4] + J[5] * dx[5]);
        }
#pragma unroll
        for (int i = 0; i < 6; i++) x[i] -= dx[i];
        if (dl < 1e-5) {
            end = 1;
            break;
        }
    }
    rodrigues2rot(x, Rout);
    MLPNP_STAMP(4);
    tout[0] = x[3], tout[1] = x[4], tout[2] = x[5];
    info[0] = planar ? 1 : 0;
    info[1] = solves;
    info[2] = end;
}

__global__ __launch_bounds__(NT) void k_mlpnp_eval(const MProbDev *__restrict__ probs, const float *__restrict__ a_bearing,
                                                   const float *__restrict__ a_p3d, const float *__restrict__ a_p2d,
                                                   const float *__restrict__ a_max, const int *__restrict__ a_samples,
                                                   int *__restrict__ o_count, double *__restrict__ o_pose,
                                                   int *__restrict__ o_info, unsigned long long *__restrict__ o_mask)
{
    extern __shared__ __attribute__((aligned(16))) double lds_d[];
    const MProbDev &P = probs[blockIdx.y];
    const int h_first = blockIdx.x * HPB;
    if (h_first >= P.n_hyp) return;  // the whole workgroup: no barrier is skipped by a part of it
    const int n = P.n;
    const int tid = threadIdx.x, wave = tid / 64, lane = tid % 64;
    const float *bearing = a_bearing + 3 * (size_t)P.pt_off, *p3d = a_p3d + 3 * (size_t)P.pt_off;
    const float *p2d = a_p2d + 2 * (size_t)P.pt_off, *mx = a_max + P.pt_off;
    float *lds = (float *)(lds_d + HPB * TILE);
    const bool staged = P.staged != 0;
    if (staged) {
        for (int i = tid; i < n; i += NT) {
            // field k of match i at lds[k n + i]: consecutive lanes read consecutive banks
            lds[i] = p3d[3 * i], lds[n + i] = p3d[3 * i + 1], lds[2 * n + i] = p3d[3 * i + 2];
            lds[3 * n + i] = p2d[2 * i], lds[4 * n + i] = p2d[2 * i + 1];
            lds[5 * n + i] = mx[i];
        }
        __syncthreads();
    }
    const int h = h_first + wave;  // wave-uniform
    if (h >= P.n_hyp) return;      // no workgroup barrier below
    const int *samples = a_samples + 6 * ((size_t)P.hyp_off + h);
    double f[6][3], p[6][3];
#pragma unroll
    for (int j = 0; j < 6; j++) {
        const int idx = samples[j];  // checked by the host: in [0, n)
#pragma unroll
        for (int k = 0; k < 3; k++) {
            f[j][k] = (double)bearing[3 * idx + k];
            p[j][k] = (double)p3d[3 * idx + k];
        }
    }
    double R[9], t[3];
    int info[3];
    long long prof[6] = {0, 0, 0, 0, 0, 0};
    MLPNP_STAMP(0);
    compute_pose(f, p, lds_d + wave * TILE, lane, R, t, info, prof);
    // CheckInliers (ref:src/MLPnPsolver.cpp:359-397)
    int count = 0;
    unsigned long long *mask = o_mask + P.mask_off + (size_t)h * P.words;
    for (int w = 0; w < P.words; w++) {
        const int i = w * 64 + lane;
        bool in = false;
        if (i < n) {
            float X, Y, Z, u2, v2, emax;
            if (staged) {
                X = lds[i], Y = lds[n + i], Z = lds[2 * n + i];
                u2 = lds[3 * n + i], v2 = lds[4 * n + i], emax = lds[5 * n + i];
            } else {
                X = p3d[3 * i], Y = p3d[3 * i + 1], Z = p3d[3 * i + 2];
                u2 = p2d[2 * i], v2 = p2d[2 * i + 1], emax = mx[i];
            }
            const float xc = (float)(R[0] * X + R[1] * Y + R[2] * Z + t[0]);
            const float yc = (float)(R[3] * X + R[4] * Y + R[5] * Z + t[1]);
            const float zc = (float)(R[6] * X + R[7] * Y + R[8] * Z + t[2]);
            float pu, pv;
            project_f(P.cam, xc, yc, zc, pu, pv);
            const float dx = u2 - pu, dy = v2 - pv;
            const float err = dx * dx + dy * dy;
            in = err < emax;  // NaN is never an inlier
        }
        const unsigned long long word = __ballot(in);
        count += __popcll(word);
        if (lane == 0) mask[w] = word;
    }
    MLPNP_STAMP(5);
    if (lane == 0) {
        const size_t g = (size_t)P.hyp_off + h;
        o_count[g] = count;
        double *o = o_pose + 12 * g;
#pragma unroll
        for (int j = 0; j < 9; j++) o[j] = R[j];
#pragma unroll
        for (int j = 0; j < 3; j++) o[9 + j] = t[j];
        o_info[3 * g] = info[0], o_info[3 * g + 1] = info[1], o_info[3 * g + 2] = info[2];
#ifdef OSG_MLPNP_PROF
        // make MLPNP_PROF=1 (tools/mlpnp_prof.py): the pose slots carry the stage durations in 100 MHz ticks:
        // bases + rank test + AtA, Jacobi, rotation + sign choice, Gauss-Newton, CheckInliers
        for (int j = 0; j < 5; j++) o[j] = (double)(prof[j + 1] - prof[j]);
#endif
    }
}

__global__ __launch_bounds__(64) void k_mlpnp_select(const MProbDev *__restrict__ probs, const int *__restrict__ counts,
                                                     const double *__restrict__ pose,
                                                     const unsigned long long *__restrict__ masks,
                                                     MSelOut *__restrict__ out, uint8_t *__restrict__ inlier)
{
    const MProbDev &P = probs[blockIdx.x];
    const int lane = threadIdx.x;
    int hyp = 0;
    if (lane == 0) {
        const osg_mlpnp_window w = osg_mlpnp_replay(counts + P.hyp_off, P.min_inliers, 0, P.n_hyp, 0, -1);
        hyp = w.hyp;
        MSelOut &o = out[blockIdx.x];
        o.converged = w.converged;
        o.hyp = hyp;
        o.n_iterations = w.n_iterations;
        o.n_best = w.n_best;
        o.n_inliers = hyp >= 0 ? counts[P.hyp_off + hyp] : 0;
        for (int j = 0; j < 9; j++) o.R[j] = (j % 4 == 0) ? 1.0 : 0.0;
        for (int j = 0; j < 3; j++) o.t[j] = 0.0;
        if (hyp >= 0) {
            const double *s = pose + 12 * ((size_t)P.hyp_off + hyp);
            for (int j = 0; j < 9; j++) o.R[j] = s[j];
            for (int j = 0; j < 3; j++) o.t[j] = s[9 + j];
        }
        for (int i = 0; i < 3; i++) {
            for (int j = 0; j < 3; j++) o.Tcw[4 * i + j] = (float)o.R[3 * i + j];
            o.Tcw[4 * i + 3] = (float)o.t[i];
        }
        o.Tcw[12] = o.Tcw[13] = o.Tcw[14] = 0.f;
        o.Tcw[15] = 1.f;
    }
    hyp = __shfl(hyp, 0);
    expand_mask(hyp < 0 ? nullptr : masks + P.mask_off + (size_t)hyp * P.words, P.n, inlier + P.pt_off, lane);
}

}  // namespace

extern "C" {

int osg_mlpnp_check_samples(const osg_mlpnp_problem *p)
{
    int h_bad = -1;
    if (!p || p->n < 0 || p->n_hyp < 1 || !p->samples) return OSG_E_INVALID;
    return check_sets(p->samples, 6, p->n_hyp, p->n, &h_bad) ? OSG_E_INVALID : 0;
}

void osg_mlpnp_ransac_parameters(double prob, int32_t min_inliers, int32_t max_its, int32_t min_set, float epsilon,
                                 int32_t n, int32_t *min_inliers_out, int32_t *max_its_out)
{
    int32_t a = 0, b = 0;
    osg_mlpnp_parameters(prob, min_inliers, max_its, min_set, epsilon, n, &a, &b);
    if (min_inliers_out) *min_inliers_out = a;
    if (max_its_out) *max_its_out = b;
}

int osg_mlpnp_ransac_batch(osg_ctx *ctx, const osg_mlpnp_problem *p, int32_t nb, osg_mlpnp_result *r)
{
    if (!ctx) return OSG_E_INVALID;
    OSG_REQUIRE(ctx, nb >= 0 && (nb == 0 || (p && r)), "null argument");
    if (nb == 0) return 0;
    const size_t lds_budget = (size_t)std::min(ctx->lds_per_block, LDS_CAP) - TILE_BYTES;
    std::vector<MProbDev> hp;
    std::vector<int> src;  // hp[k] is problem src[k]
    hp.reserve(nb);
    size_t n_pts = 0, n_hyp = 0, n_words = 0, lds = 0;
    int max_hyp = 0;
    for (int b = 0; b < nb; b++) {
        const osg_mlpnp_problem &q = p[b];
        OSG_REQUIRE(ctx, q.n >= 0 && q.n_hyp >= 1 && q.min_inliers >= 0, "n, n_hyp or min_inliers");
        OSG_REQUIRE(ctx, q.n == 0 || r[b].inlier, "inlier array");
        if (q.n == 0 || q.n < q.min_inliers) continue;
        OSG_REQUIRE(ctx, q.n >= 6, "fewer than 6 matches");
        OSG_REQUIRE(ctx, q.bearing && q.p3dw && q.p2d && q.max_err && q.samples, "match arrays");
        int h_bad = -1;
        const int why = check_sets(q.samples, 6, q.n_hyp, q.n, &h_bad);
        OSG_REQUIRE(ctx, why != 1, "sample index outside [0, n) in hypothesis %d of problem %d", h_bad, b);
        OSG_REQUIRE(ctx, why != 2, "repeated sample index in hypothesis %d of problem %d", h_bad, b);
        MProbDev d;
        std::memset(&d, 0, sizeof d);
        d.n = q.n;
        d.n_hyp = q.n_hyp;
        d.min_inliers = q.min_inliers;
        d.pt_off = (int)n_pts;
        d.hyp_off = (int)n_hyp;
        d.words = (q.n + 63) / 64;
        d.mask_off = (long long)n_words;
        const size_t need = sizeof(float) * FPM * (size_t)q.n;
        d.staged = need <= lds_budget;
        if (d.staged) lds = std::max(lds, need);
        d.cam = q.cam;
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
        osg_mlpnp_result &o = r[b];
        o.converged = 0;
        o.hyp = -1;
        o.n_iterations = o.n_inliers = o.n_best = 0;
        for (int j = 0; j < 9; j++) o.R[j] = (j % 4 == 0) ? 1.0 : 0.0;
        for (int j = 0; j < 3; j++) o.t[j] = 0.0;
        for (int j = 0; j < 16; j++) o.Tcw[j] = (j % 5 == 0) ? 1.f : 0.f;
        if (p[b].n > 0) std::memset(o.inlier, 0, (size_t)p[b].n);
        if (o.hyp_inliers) std::memset(o.hyp_inliers, 0, sizeof(int32_t) * (size_t)p[b].n_hyp);
        if (o.hyp_info) std::memset(o.hyp_info, 0, sizeof(int32_t) * 3 * (size_t)p[b].n_hyp);
        if (o.hyp_pose)
            for (int h = 0; h < p[b].n_hyp; h++)
                for (int j = 0; j < 12; j++) o.hyp_pose[12 * (size_t)h + j] = (j < 9 && j % 4 == 0) ? 1.0 : 0.0;
    }
    if (na == 0) return 0;
    bool want_hyp = false;
    for (int k = 0; k < na; k++) want_hyp = want_hyp || r[src[k]].hyp_inliers || r[src[k]].hyp_pose || r[src[k]].hyp_info;
    osg_batch_io io(ctx);
    const osg_seg i_pr = io.in(sizeof(MProbDev), na), i_br = io.in(3 * sizeof(float), n_pts), i_p3 = io.in(3 * sizeof(float), n_pts);
    const osg_seg i_p2 = io.in(2 * sizeof(float), n_pts), i_mx = io.in(sizeof(float), n_pts), i_sm = io.in(6 * sizeof(int32_t), n_hyp);
    // the counts, the info and the poses are downloaded on request
    const osg_seg o_res = io.out(sizeof(MSelOut), na), o_in = io.out(1, n_pts), o_cnt = io.out(sizeof(int32_t), n_hyp);
    const osg_seg o_inf = io.out(3 * sizeof(int32_t), n_hyp), o_ps = io.out(12 * sizeof(double), n_hyp);
    const size_t dl_bytes = want_hyp ? io.out_bytes : o_cnt.off;
    OSG_RC(io.stage());
    io.put(i_pr, 0, hp.data(), na);
    for (int k = 0; k < na; k++) {
        const osg_mlpnp_problem &q = p[src[k]];
        io.put(i_br, hp[k].pt_off, q.bearing, q.n);
        io.put(i_p3, hp[k].pt_off, q.p3dw, q.n);
        io.put(i_p2, hp[k].pt_off, q.p2d, q.n);
        io.put(i_mx, hp[k].pt_off, q.max_err, q.n);
        io.put(i_sm, hp[k].hyp_off, q.samples, q.n_hyp);
    }
    OSG_RC(io.upload());
    unsigned long long *dmask = nullptr;
    OSG_ALLOC(ctx, dmask, SLOT_BA2, 8 * n_words);
    const size_t lds_bytes = TILE_BYTES + lds;
    if (lds_bytes > 48 * 1024)
        OSG_HIP_CHECK(ctx, hipFuncSetAttribute((const void *)k_mlpnp_eval, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
    OSG_RC(io.start());
    const MProbDev *dp = io.dev_in<const MProbDev>(i_pr);
    hipLaunchKernelGGL(k_mlpnp_eval, dim3((max_hyp + HPB - 1) / HPB, na), dim3(NT), lds_bytes, ctx->stream, dp,
                       io.dev_in<const float>(i_br), io.dev_in<const float>(i_p3), io.dev_in<const float>(i_p2),
                       io.dev_in<const float>(i_mx), io.dev_in<const int>(i_sm), io.dev_out<int>(o_cnt),
                       io.dev_out<double>(o_ps), io.dev_out<int>(o_inf), dmask);
    OSG_HIP_CHECK(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_mlpnp_select, dim3(na), dim3(64), 0, ctx->stream, dp, io.dev_out<const int>(o_cnt),
                       io.dev_out<const double>(o_ps), (const unsigned long long *)dmask, io.dev_out<MSelOut>(o_res),
                       io.dev_out<uint8_t>(o_in));
    OSG_HIP_CHECK(ctx, hipGetLastError());
    OSG_RC(io.finish(dl_bytes));
    const MSelOut *res = io.result<MSelOut>(o_res);
    int found = 0;
    for (int k = 0; k < na; k++) {
        const MSelOut &s = res[k];
        osg_mlpnp_result &o = r[src[k]];
        o.converged = s.converged;
        o.hyp = s.hyp;
        o.n_iterations = s.n_iterations;
        o.n_inliers = s.n_inliers;
        o.n_best = s.n_best;
        std::memcpy(o.R, s.R, sizeof o.R);
        std::memcpy(o.t, s.t, sizeof o.t);
        std::memcpy(o.Tcw, s.Tcw, sizeof o.Tcw);
        io.get(o.inlier, o_in, hp[k].pt_off, hp[k].n);
        if (o.hyp_inliers) io.get(o.hyp_inliers, o_cnt, hp[k].hyp_off, hp[k].n_hyp);
        if (o.hyp_info) io.get(o.hyp_info, o_inf, hp[k].hyp_off, hp[k].n_hyp);
        if (o.hyp_pose) io.get(o.hyp_pose, o_ps, hp[k].hyp_off, hp[k].n_hyp);
        found += s.hyp >= 0 ? 1 : 0;
    }
    return found;
}

int osg_mlpnp_ransac(osg_ctx *ctx, const osg_mlpnp_problem *p, osg_mlpnp_result *r)
{
    const int rc = osg_mlpnp_ransac_batch(ctx, p, 1, r);
    return rc < 0 ? rc : r->n_inliers;
}

}  // extern "C"
