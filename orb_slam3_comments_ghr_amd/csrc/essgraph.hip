// essgraph.hip — the g2o part of Optimizer::OptimizeEssentialGraph (ref:src/Optimizer.cc:4527-4858):
// a pose graph of VertexSim3Expmap vertices and EdgeSim3 edges (error log(C * S_i * S_j^-1), identity
// information, no robust kernel), optimised by g2o's Levenberg-Marquardt with a user lambda, and the
// MapPoint correction of its write-back.  DESIGN.md §3.19.  The same lists, assembly, factorisation and loop serve
// the g2o part of Optimizer::OptimizeEssentialGraph4DoF (ref:src/Optimizer.cc:4870-5198; VertexPose4DoF, Edge4DoF)
// with its own k_eg4_linearize, k_eg4_update and k_eg4_chi2.  DESIGN.md §3.26.
//
// Per LM iteration (device):
//   k_eg_linearize  16 lanes per edge, four edges per wave: lane 0 the central error, lanes 1..14 the
//                   +-delta pair of one (side, dimension) through oplusImpl, as g2o differentiates an edge
//                   without linearizeOplus (ref:Thirdparty/g2o/g2o/core/base_binary_edge.hpp:147-200;
//                   a fixed vertex's side is skipped).  J_i, J_j meet in LDS; the edge's J_i^T J_i,
//                   J_i^T J_j, J_j^T J_j, -J_i^T e, -J_j^T e, e^T e go to its own slot.
//   k_eg_assemble   one 64-lane workgroup per diagonal block and per connected pair: the slots of its
//                   edges summed in edge order (host-built CSR lists, no atomics) into the matrix store.
// Per LM trial:
//   k_eg_copy, k_eg_damp   L = H, lambda added to the 7 real diagonal entries of every free vertex
//   k_eg_factor     one workgroup: blocked Cholesky of the lower 32 x 32 tiles inside the row-block
//                   envelope, row block by row block, tile products on FP64 MFMA
//                   (v_mfma_f64_16x16x4f64), the diagonal tile factored and inverted in LDS, the forward
//                   substitution fused, then the backward substitution and g2o's scale sum
//   k_eg_update     oplusImpl per free vertex into the trial buffer
//   k_eg_chi2, k_eg_reduce   e^T e per edge, summed in a fixed order
// The host reads back three scalars per trial (failed pivot, scale sum, chi2) and runs g2o's accept /
// reject / lambda / stop rules (ref:Thirdparty/g2o/g2o/core/optimization_algorithm_levenberg.cpp:61-169);
// push / pop is a swap of the current and the trial state buffers.
//
// A free vertex takes 8 rows of the system (7 + a pad row with pivot 1 and right-hand side 0), so a
// tile is four vertices.  In the caller's vertex order the spanning-tree and covisibility edges of a map
// form a band and a loop edge a row block that reaches back to the loop KeyFrame's block; the envelope
// holds both, and Cholesky fills nothing outside it.
#include <cfloat>
#include <cstring>
#include <vector>

#include "essgraph4_common.h"
#include "osg_internal.h"
#include "sim3_common.h"
#include "so3_common.h"

using osgs3::Sim3;

namespace {

constexpr int TB = 32;             // tile edge
constexpr int TE = TB * TB;        // tile elements
constexpr int ES = 162;            // edge slot: Hii 49 | Hij 49 | Hjj 49 | b_i 7 | b_j 7 | chi2
constexpr int S_HIJ = 49, S_HJJ = 98, S_B = 147, S_CHI = 161;
constexpr double DELTA = 1e-9;
typedef double d4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ Sim3 load_s3(const double *__restrict__ p)
{
    Sim3 S;
    S.q[0] = p[0]; S.q[1] = p[1]; S.q[2] = p[2]; S.q[3] = p[3];
    S.t[0] = p[4]; S.t[1] = p[5]; S.t[2] = p[6];
    S.s = p[7];
    return S;
}
__device__ __forceinline__ void store_s3(double *__restrict__ p, const Sim3 &S)
{
    p[0] = S.q[0]; p[1] = S.q[1]; p[2] = S.q[2]; p[3] = S.q[3];
    p[4] = S.t[0]; p[5] = S.t[1]; p[6] = S.t[2];
    p[7] = S.s;
}
// EdgeSim3::computeError
__device__ __forceinline__ void edge_error(const Sim3 &C, const Sim3 &Si, const Sim3 &Sj, double *e)
{
    osgs3::sim3_log(osgs3::sim3_mul(osgs3::sim3_mul(C, Si), osgs3::sim3_inverse(Sj)), e);
}

__global__ __launch_bounds__(64) void k_eg_linearize(const double *__restrict__ state, const double *__restrict__ meas,
                                                     const int *__restrict__ v0, const int *__restrict__ v1,
                                                     const int *__restrict__ fidx, int n_edges, int fix_scale,
                                                     double *__restrict__ slots)
{
    __shared__ double sJ[4][2][7][7];  // [edge of the wave][side][error row][update column]
    __shared__ double sE[4][7];
    const int g = threadIdx.x >> 4, k = threadIdx.x & 15;
    const int e = blockIdx.x * 4 + g;
    const bool valid = e < n_edges && k < 15;
    const int side = k >= 8 ? 1 : 0, d = k == 0 ? 0 : (k - 1) - 7 * side;
    double col[7] = {0, 0, 0, 0, 0, 0, 0};
    bool skip = true;
    if (valid) {
        const int a = v0[e], b = v1[e];
        const Sim3 C = load_s3(meas + 8 * (size_t)e), Si = load_s3(state + 8 * (size_t)a), Sj = load_s3(state + 8 * (size_t)b);
        if (k == 0) {
            edge_error(C, Si, Sj, col);
#pragma unroll
            for (int r = 0; r < 7; r++) sE[g][r] = col[r];
        } else {
            skip = (side ? fidx[b] : fidx[a]) < 0;
            if (!skip) {
#pragma unroll 1
                for (int sgn = 0; sgn < 2; sgn++) {
                    double upd[7];
#pragma unroll
                    for (int i = 0; i < 7; i++) upd[i] = i == d ? (sgn ? -DELTA : DELTA) : 0.0;
                    const Sim3 T = osgs3::sim3_oplus(side ? Sj : Si, upd, fix_scale != 0);
                    double er[7];
                    edge_error(C, side ? Si : T, side ? T : Sj, er);
                    const double scalar = 1.0 / (2 * DELTA);
#pragma unroll
                    for (int r = 0; r < 7; r++) col[r] = sgn ? scalar * (col[r] - er[r]) : er[r];
                }
            }
#pragma unroll
            for (int r = 0; r < 7; r++) sJ[g][side][r][d] = col[r];
        }
    }
    __syncthreads();
    if (!valid) return;
    double *slot = slots + (size_t)ES * e;
    if (k == 0) {
        double c = 0;
#pragma unroll
        for (int r = 0; r < 7; r++) c += col[r] * col[r];
        slot[S_CHI] = c;
        return;
    }
    // row d of J_s^T J_s, of J_i^T J_j (side 0), and entry d of -J_s^T e
    for (int c = 0; c < 7; c++) {
        double h = 0, x = 0;
#pragma unroll
        for (int r = 0; r < 7; r++) {
            h += col[r] * sJ[g][side][r][c];
            x += col[r] * sJ[g][1][r][c];
        }
        slot[(side ? S_HJJ : 0) + 7 * d + c] = h;
        if (!side) slot[S_HIJ + 7 * d + c] = x;
    }
    double bs = 0;
#pragma unroll
    for (int r = 0; r < 7; r++) bs += col[r] * sE[g][r];
    slot[S_B + 7 * side + d] = -bs;
}

struct EgStruct {
    const int *d_ptr, *d_ent;    // per free vertex: its (edge << 1 | side) contributions, in edge order
    const int *p_ptr, *p_ent;    // per connected pair: (edge << 1 | transpose)
    const int *p_hi, *p_lo;      // the pair's free indices, hi > lo
    const int *first;            // per tile row: its first column tile
    const long long *row_off;    // per tile row: the tile index of (t, first[t]) in the store
    int nf, nfp, n_pairs, T;
};

__device__ __forceinline__ size_t tile_at(const EgStruct &G, int t, int j)
{
    return (size_t)(G.row_off[t] + (j - G.first[t])) * TE;
}

// grid: nfp diagonal blocks (the ghosts that fill the last tile become the identity), then the pairs
__global__ __launch_bounds__(64) void k_eg_assemble(EgStruct G, const double *__restrict__ slots, double *__restrict__ H,
                                                    double *__restrict__ bvec, double *__restrict__ diagmax)
{
    const int bx = blockIdx.x, r = threadIdx.x >> 3, c = threadIdx.x & 7;
    const bool real = r < 7 && c < 7;
    if (bx < G.nfp) {
        const int a = bx, t = a >> 2, o = 8 * (a & 3);
        double *tile = H + tile_at(G, t, t);
        const bool ghost = a >= G.nf;
        double v = r == c ? 1.0 : 0.0;
        const int p0 = ghost ? 0 : G.d_ptr[a], p1 = ghost ? 0 : G.d_ptr[a + 1];
        if (real && !ghost) {
            v = 0.0;
            for (int p = p0; p < p1; p++) {
                const int en = G.d_ent[p];
                v += slots[(size_t)ES * (en >> 1) + ((en & 1) ? S_HJJ : 0) + 7 * r + c];
            }
        }
        tile[(o + r) * TB + o + c] = v;
        if (r == 7) {  // the right-hand side, and on the last lane the largest |diagonal entry|
            double s = 0.0;
            if (c < 7) {
                for (int p = p0; p < p1; p++) {
                    const int en = G.d_ent[p];
                    s += slots[(size_t)ES * (en >> 1) + S_B + 7 * (en & 1) + c];
                }
                bvec[8 * a + c] = s;
            } else {
                bvec[8 * a + 7] = 0.0;
                double md = 0.0;
                for (int q = 0; q < 7; q++) {
                    double dv = 0.0;
                    for (int p = p0; p < p1; p++) {
                        const int en = G.d_ent[p];
                        dv += slots[(size_t)ES * (en >> 1) + ((en & 1) ? S_HJJ : 0) + 8 * q];
                    }
                    md = fmax(md, fabs(dv));
                }
                if (!ghost) diagmax[a] = md;
            }
        }
        return;
    }
    const int pr = bx - G.nfp;
    if (pr >= G.n_pairs) return;
    const int hi = G.p_hi[pr], lo = G.p_lo[pr];
    double v = 0.0;
    if (real) {
        for (int p = G.p_ptr[pr]; p < G.p_ptr[pr + 1]; p++) {
            const int en = G.p_ent[p];
            v += slots[(size_t)ES * (en >> 1) + S_HIJ + ((en & 1) ? 7 * c + r : 7 * r + c)];
        }
    }
    double *tile = H + tile_at(G, hi >> 2, lo >> 2);
    tile[(8 * (hi & 3) + r) * TB + 8 * (lo & 3) + c] = v;
}

__global__ __launch_bounds__(256) void k_eg_copy(const double *__restrict__ src, double *__restrict__ dst, size_t n)
{
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) dst[i] = src[i];
}

__global__ __launch_bounds__(256) void k_eg_damp(EgStruct G, const double *__restrict__ H, double *__restrict__ L, double lambda)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= 8 * G.nf || (i & 7) == 7) return;
    const int a = i >> 3, t = a >> 2, o = 8 * (a & 3) + (i & 7);
    const size_t at = tile_at(G, t, t) + (size_t)o * (TB + 1);
    L[at] = H[at] + lambda;
}

// D += A B^T for the wave's 16 x 16 quadrant (qr, qc) of a tile product.  Lane l holds row l & 15 and
// the k-group l >> 4 of both operands; D's entry q of lane l is row qr + (l >> 4) + 4 q, column
// qc + (l & 15).
template <class PA, class PB>
__device__ __forceinline__ d4 tile_mma(PA a_at, PB b_at, d4 acc, int l)
{
#pragma unroll
    for (int ks = 0; ks < TB / 4; ks++) {
        const int kk = 4 * ks + (l >> 4);
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a_at(l & 15, kk), b_at(l & 15, kk), acc, 0, 0, 0);
    }
    return acc;
}

// sum of v over the 8 consecutive lanes of a group, in every lane of it
__device__ __forceinline__ double sum8(double v)
{
    v += __shfl_xor(v, 1);
    v += __shfl_xor(v, 2);
    v += __shfl_xor(v, 4);
    return v;
}

// One workgroup.  out[0]: 1 when a pivot was not positive (g2o's failed solve; x keeps its previous
// value then), out[1]: sum_j x_j (lambda x_j + b_j).
__global__ __launch_bounds__(256) void k_eg_factor(EgStruct G, double *__restrict__ L, double *__restrict__ Linv,
                                                   const double *__restrict__ bvec, double *__restrict__ y,
                                                   double *__restrict__ xt, double *__restrict__ x, double lambda,
                                                   int fix_scale, double *__restrict__ out)
{
    __shared__ double sT[TB][TB + 1], sM[TB][TB + 1];
    __shared__ double sDi[TB], s_rhs[TB], s_red[256];
    __shared__ int s_bad;
    const int tid = threadIdx.x, w = tid >> 6, l = tid & 63;
    const int qr = (w >> 1) * 16, qc = (w & 1) * 16;
    const int gi = tid >> 3, gp = tid & 7;  // row / column gi, part gp of the 8-lane groups
    if (tid == 0) s_bad = 0;
    __syncthreads();
    for (int t = 0; t < G.T; t++) {
        const int ft = G.first[t];
        double *rowp = L + (size_t)G.row_off[t] * TE;
        for (int j = ft; j < t; j++) {
            const int fj = G.first[j], k0 = max(ft, fj);
            const double *Lj = L + (size_t)G.row_off[j] * TE;
            d4 acc = {0.0, 0.0, 0.0, 0.0};
            for (int k = k0; k < j; k++) {
                const double *A = rowp + (size_t)(k - ft) * TE, *B = Lj + (size_t)(k - fj) * TE;
                acc = tile_mma([&](int r, int kk) { return A[(qr + r) * TB + kk]; },
                               [&](int r, int kk) { return B[(qc + r) * TB + kk]; }, acc, l);
            }
            double *Atj = rowp + (size_t)(j - ft) * TE;
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int r = qr + (l >> 4) + 4 * q, c = qc + (l & 15);
                sT[r][c] = Atj[r * TB + c] - acc[q];
            }
            __syncthreads();
            // L_tj = X L_jj^-T
            const double *Lv = Linv + (size_t)j * TE;
            d4 acc2 = {0.0, 0.0, 0.0, 0.0};
            acc2 = tile_mma([&](int r, int kk) { return sT[qr + r][kk]; },
                            [&](int r, int kk) { return Lv[(qc + r) * TB + kk]; }, acc2, l);
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int r = qr + (l >> 4) + 4 * q, c = qc + (l & 15);
                Atj[r * TB + c] = acc2[q];
            }
            __syncthreads();
        }
        // the diagonal tile: T = A_tt - sum_k L_tk L_tk^T
        {
            d4 acc = {0.0, 0.0, 0.0, 0.0};
            for (int k = ft; k < t; k++) {
                const double *A = rowp + (size_t)(k - ft) * TE;
                acc = tile_mma([&](int r, int kk) { return A[(qr + r) * TB + kk]; },
                               [&](int r, int kk) { return A[(qc + r) * TB + kk]; }, acc, l);
            }
            const double *Att = rowp + (size_t)(t - ft) * TE;
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int r = qr + (l >> 4) + 4 * q, c = qc + (l & 15);
                sT[r][c] = Att[r * TB + c] - acc[q];
                sM[r][c] = r == c ? 1.0 : 0.0;
            }
        }
        __syncthreads();
        // T = L D L^T (L unit lower) by rank-1 updates of the unscaled columns, and in the same barrier interval
        // Y = L^-1 by the same eliminations applied to the identity: one barrier per column, no square root in
        // the chain.  The Cholesky factor's inverse is then D^-1/2 Y.
        for (int c = 0; c < TB; c++) {
            double dv = sT[c][c];
            if (!(dv > 0.0)) {
                if (tid == 0) s_bad = 1;
                dv = 1.0;
            }
            const double inv = 1.0 / dv;
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int el = tid + 256 * q, r = el >> 5, cc = el & 31;
                if (r > c) {
                    const double l = sT[r][c] * inv;
                    if (cc > c) {
                        if (r >= cc) sT[r][cc] -= l * sT[cc][c];
                    } else {
                        sM[r][cc] -= l * sM[c][cc];
                    }
                }
            }
            __syncthreads();
        }
        if (tid < TB) {
            double dv = sT[tid][tid];
            if (!(dv > 0.0)) dv = 1.0;
            sDi[tid] = 1.0 / sqrt(dv);
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int el = tid + 256 * q, r = el >> 5, cc = el & 31;
            sM[r][cc] = r >= cc ? sM[r][cc] * sDi[r] : 0.0;
        }
        __syncthreads();
        {
            double *Lv = Linv + (size_t)t * TE;
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int el = tid + 256 * q, r = el >> 5, c = el & 31;
                Lv[el] = sM[r][c];
            }
        }
        // forward substitution: y_t = L_tt^-1 (b_t - sum_k L_tk y_k)
        {
            double s = 0.0;
            for (int k = ft; k < t; k++) {
                const double *A = rowp + (size_t)(k - ft) * TE + gi * TB;
                const double *yk = y + (size_t)TB * k;
#pragma unroll
                for (int q = 0; q < 4; q++) s += A[gp + 8 * q] * yk[gp + 8 * q];
            }
            s = sum8(s);
            if (gp == 0) s_rhs[gi] = bvec[(size_t)TB * t + gi] - s;
        }
        __syncthreads();
        {
            double s = 0.0;
#pragma unroll
            for (int q = 0; q < 4; q++) s += sM[gi][gp + 8 * q] * s_rhs[gp + 8 * q];
            s = sum8(s);
            if (gp == 0) y[(size_t)TB * t + gi] = s;
        }
        __syncthreads();
    }
    // backward substitution, row block by row block: x_u = L_uu^-T y_u, then y_k -= L_uk^T x_u
    for (int u = G.T - 1; u >= 0; u--) {
        const int fu = G.first[u];
        const double *Lv = Linv + (size_t)u * TE;
        {
            double s = 0.0;
#pragma unroll
            for (int q = 0; q < 4; q++) s += Lv[(gp + 8 * q) * TB + gi] * y[(size_t)TB * u + gp + 8 * q];
            s = sum8(s);
            if (gp == 0) {
                s_rhs[gi] = s;
                xt[(size_t)TB * u + gi] = s;
            }
        }
        __syncthreads();
        const double *rowp = L + (size_t)G.row_off[u] * TE;
        for (int k = fu; k < u; k++) {
            const double *A = rowp + (size_t)(k - fu) * TE;
            double s = 0.0;
#pragma unroll
            for (int q = 0; q < 4; q++) s += A[(gp + 8 * q) * TB + gi] * s_rhs[gp + 8 * q];
            s = sum8(s);
            if (gp == 0) y[(size_t)TB * k + gi] -= s;
        }
        __syncthreads();
    }
    // x (kept on a failed solve; oplusImpl zeroes the solver's own x[6] under fix_scale) and the scale sum
    const bool bad = s_bad != 0;
    const int n = TB * G.T;
    double part = 0.0;
    for (int i = tid; i < n; i += 256) {
        double xv = bad ? x[i] : xt[i];
        if (fix_scale && (i & 7) == 6) xv = 0.0;
        x[i] = xv;
        part += xv * (lambda * xv + bvec[i]);
    }
    s_red[tid] = part;
    __syncthreads();
    for (int o = 128; o >= 1; o >>= 1) {
        if (tid < o) s_red[tid] += s_red[tid + o];
        __syncthreads();
    }
    if (tid == 0) {
        out[0] = bad ? 1.0 : 0.0;
        out[1] = s_red[0];
    }
}

__global__ __launch_bounds__(256) void k_eg_update(const double *__restrict__ cur, const double *__restrict__ x,
                                                   const int *__restrict__ fidx, int n, int fix_scale,
                                                   double *__restrict__ trial)
{
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= n) return;
    const int f = fidx[v];
    Sim3 S = load_s3(cur + 8 * (size_t)v);
    if (f >= 0) {
        double u[7];
#pragma unroll
        for (int i = 0; i < 7; i++) u[i] = x[8 * (size_t)f + i];
        S = osgs3::sim3_oplus(S, u, fix_scale != 0);
    }
    store_s3(trial + 8 * (size_t)v, S);
}

__global__ __launch_bounds__(256) void k_eg_chi2(const double *__restrict__ state, const double *__restrict__ meas,
                                                 const int *__restrict__ v0, const int *__restrict__ v1, int n_edges,
                                                 double *__restrict__ edge_chi)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n_edges) return;
    double er[7];
    edge_error(load_s3(meas + 8 * (size_t)e), load_s3(state + 8 * (size_t)v0[e]), load_s3(state + 8 * (size_t)v1[e]), er);
    double c = 0;
#pragma unroll
    for (int r = 0; r < 7; r++) c += er[r] * er[r];
    edge_chi[e] = c;
}

// ---- OptimizeEssentialGraph4DoF (ref:src/Optimizer.cc:4870-5198): VertexPose4DoF / Edge4DoF
// in place of VertexSim3Expmap / EdgeSim3.  The lists, k_eg_assemble, k_eg_damp, k_eg_factor and the host loop
// are the ones above.
using namespace osgeg4;

struct Info6 {
    double w[6] = {1, 1, 1, 1, 1, 1};  // the diagonal of Edge4DoF's information
};
struct Cam4 {
    double Rcw[9], tcw[3];
};

// ImuCamPose::UpdateW (ref:src/G2oTypes.cc:252-285) for VertexPose4DoF::oplusImpl's (0, 0, u0, u1, u2, u3), from
// the state st and the constants cst of a vertex: the new DR, Rwb, twb and the camera re-derived from them.
// The its counter and the normalisation that follows it act on DR alone and are k_eg4_update's.
__device__ inline void eg4_update_w(const double *__restrict__ st, const double *__restrict__ cst, const double *u, double *DR,
                                    double *Rwb, double *twb, Cam4 &C)
{
    const double w[3] = {0.0, 0.0, u[0]};
    double dR[9], DR0[9], Rwb0[9], Rcb[9], Rbw[9], tbw[3];
#pragma unroll
    for (int i = 0; i < 9; i++) {
        DR0[i] = st[V_DR + i];
        Rwb0[i] = st[V_RWB0 + i];
        Rcb[i] = cst[i];
    }
    osgso3::exp_so3(w, dR);
    osgso3::m3_mul(dR, DR0, DR);
    osgso3::m3_mul(DR, Rwb0, Rwb);
#pragma unroll
    for (int i = 0; i < 3; i++) twb[i] = st[V_TWB + i] + u[1 + i];
    osgso3::m3_t(Rwb, Rbw);
    osgso3::m3_vec(Rbw, twb, tbw);
#pragma unroll
    for (int i = 0; i < 3; i++) tbw[i] = -tbw[i];
    osgso3::m3_mul(Rcb, Rbw, C.Rcw);
    osgso3::m3_vec(Rcb, tbw, C.tcw);
#pragma unroll
    for (int i = 0; i < 3; i++) C.tcw[i] += cst[9 + i];
}
__device__ __forceinline__ Cam4 load_cam4(const double *__restrict__ st)
{
    Cam4 C;
#pragma unroll
    for (int i = 0; i < 9; i++) C.Rcw[i] = st[V_RCW + i];
#pragma unroll
    for (int i = 0; i < 3; i++) C.tcw[i] = st[V_TCW + i];
    return C;
}
// Edge4DoF::computeError (ref:include/G2oTypes.h:965-971); m: dRij row-major, dtij
__device__ inline void eg4_error(const double *__restrict__ m, const Cam4 &Ci, const Cam4 &Cj, double *e)
{
    double Rjt[9], A[9], Mt[9], B[9], M[9], p[3], q[3];
#pragma unroll
    for (int i = 0; i < 9; i++) M[i] = m[i];
    osgso3::m3_t(Cj.Rcw, Rjt);
    osgso3::m3_mul(Ci.Rcw, Rjt, A);
    osgso3::m3_t(M, Mt);
    osgso3::m3_mul(A, Mt, B);
    osgso3::log_so3(B, e);
    osgso3::m3_vec(Rjt, Cj.tcw, p);
#pragma unroll
    for (int i = 0; i < 3; i++) p[i] = -p[i];
    osgso3::m3_vec(Ci.Rcw, p, q);
#pragma unroll
    for (int i = 0; i < 3; i++) e[3 + i] = q[i] + Ci.tcw[i] - m[9 + i];
}

// 16 lanes per edge, four edges per wave, as k_eg_linearize: lane 0 the central error at the stored cameras,
// lanes 1..8 the +-delta pair of one (side, dimension) through UpdateW, lanes 9..15 idle.  The slot keeps the
// 7 x 7 layout of ES; only its rows and columns 0..3 are written (the host zeroes the slots once).
__global__ __launch_bounds__(64) void k_eg4_linearize(const double *__restrict__ state, const double *__restrict__ cst,
                                                      const double *__restrict__ meas, const int *__restrict__ v0,
                                                      const int *__restrict__ v1, const int *__restrict__ fidx, int n_edges,
                                                      Info6 info, double *__restrict__ slots)
{
    __shared__ double sJ[4][2][6][4];  // [edge of the wave][side][error row][update column]
    __shared__ double sE[4][6];
    const int g = threadIdx.x >> 4, k = threadIdx.x & 15;
    const int e = blockIdx.x * 4 + g;
    const bool valid = e < n_edges && k < 9;
    const int side = k >= 5 ? 1 : 0, d = k == 0 ? 0 : (k - 1) - 4 * side;
    double col[6] = {0, 0, 0, 0, 0, 0};
    if (valid) {
        const int a = v0[e], b = v1[e];
        const double *m = meas + 12 * (size_t)e, *sa = state + VS * (size_t)a, *sb = state + VS * (size_t)b;
        const Cam4 Ci = load_cam4(sa), Cj = load_cam4(sb);
        if (k == 0) {
            eg4_error(m, Ci, Cj, col);
#pragma unroll
            for (int r = 0; r < 6; r++) sE[g][r] = col[r];
        } else {
            const bool skip = (side ? fidx[b] : fidx[a]) < 0;
            if (!skip) {
                const double *sv = side ? sb : sa, *cv = cst + VC * (size_t)(side ? b : a);
#pragma unroll 1
                for (int sgn = 0; sgn < 2; sgn++) {
                    double upd[4], DR[9], Rwb[9], twb[3], er[6];
#pragma unroll
                    for (int i = 0; i < 4; i++) upd[i] = i == d ? (sgn ? -DELTA : DELTA) : 0.0;
                    Cam4 T;
                    eg4_update_w(sv, cv, upd, DR, Rwb, twb, T);
                    eg4_error(m, side ? Ci : T, side ? T : Cj, er);
                    const double scalar = 1.0 / (2 * DELTA);
#pragma unroll
                    for (int r = 0; r < 6; r++) col[r] = sgn ? scalar * (col[r] - er[r]) : er[r];
                }
            }
#pragma unroll
            for (int r = 0; r < 6; r++) sJ[g][side][r][d] = col[r];
        }
    }
    __syncthreads();
    if (!valid) return;
    double *slot = slots + (size_t)ES * e;
    if (k == 0) {
        double c = 0;
#pragma unroll
        for (int r = 0; r < 6; r++) c += col[r] * (info.w[r] * col[r]);
        slot[S_CHI] = c;
        return;
    }
    // row d of J_s^T W J_s, of J_i^T W J_j (side 0), and entry d of -J_s^T W e
    double wc[6];
#pragma unroll
    for (int r = 0; r < 6; r++) wc[r] = col[r] * info.w[r];
    for (int c = 0; c < 4; c++) {
        double h = 0, x = 0;
#pragma unroll
        for (int r = 0; r < 6; r++) {
            h += wc[r] * sJ[g][side][r][c];
            x += wc[r] * sJ[g][1][r][c];
        }
        slot[(side ? S_HJJ : 0) + 7 * d + c] = h;
        if (!side) slot[S_HIJ + 7 * d + c] = x;
    }
    double bs = 0;
#pragma unroll
    for (int r = 0; r < 6; r++) bs += col[r] * (info.w[r] * sE[g][r]);
    slot[S_B + 7 * side + d] = -bs;
}

// VertexPose4DoF::oplusImpl per vertex into the trial buffer: UpdateW with its counter, the four zeroed
// entries and the normalisation of DR in the reference's order (they act on the next update's rotation)
__global__ __launch_bounds__(256) void k_eg4_update(const double *__restrict__ cur, const double *__restrict__ cst,
                                                    const double *__restrict__ x, const int *__restrict__ fidx, int n,
                                                    double *__restrict__ trial)
{
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= n) return;
    const double *st = cur + VS * (size_t)v;
    double *out = trial + VS * (size_t)v;
    const int f = fidx[v];
    if (f < 0) {
        for (int i = 0; i < VS; i++) out[i] = st[i];
        return;
    }
    double u[4], DR[9], Rwb[9], twb[3];
#pragma unroll
    for (int i = 0; i < 4; i++) u[i] = x[8 * (size_t)f + i];
    Cam4 C;
    eg4_update_w(st, cst + VC * (size_t)v, u, DR, Rwb, twb, C);
    int its = (int)st[V_ITS] + 1;
    if (its >= 5) {
        DR[2] = 0.0;
        DR[5] = 0.0;
        DR[6] = 0.0;
        DR[7] = 0.0;
        osgso3::normalize_rotation<double>(DR);
        its = 0;
    }
#pragma unroll
    for (int i = 0; i < 9; i++) {
        out[V_RWB0 + i] = st[V_RWB0 + i];
        out[V_DR + i] = DR[i];
        out[V_RCW + i] = C.Rcw[i];
        out[V_RWB + i] = Rwb[i];
    }
#pragma unroll
    for (int i = 0; i < 3; i++) {
        out[V_TWB + i] = twb[i];
        out[V_TCW + i] = C.tcw[i];
    }
    out[V_ITS] = (double)its;
    for (int i = V_ITS + 1; i < VS; i++) out[i] = 0.0;
}

__global__ __launch_bounds__(256) void k_eg4_chi2(const double *__restrict__ state, const double *__restrict__ meas,
                                                  const int *__restrict__ v0, const int *__restrict__ v1, int n_edges, Info6 info,
                                                  double *__restrict__ edge_chi)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n_edges) return;
    double er[6];
    eg4_error(meas + 12 * (size_t)e, load_cam4(state + VS * (size_t)v0[e]), load_cam4(state + VS * (size_t)v1[e]), er);
    double c = 0;
#pragma unroll
    for (int r = 0; r < 6; r++) c += er[r] * (info.w[r] * er[r]);
    edge_chi[e] = c;
}

// one workgroup: the sum (mode 0) or the maximum (mode 1) of src[0 .. n) in a fixed order
__global__ __launch_bounds__(256) void k_eg_reduce(const double *__restrict__ src, int n, int mode, double *__restrict__ dst)
{
    __shared__ double s_red[256];
    const int tid = threadIdx.x;
    double a = 0.0;
    for (int i = tid; i < n; i += 256) a = mode ? fmax(a, src[i]) : a + src[i];
    s_red[tid] = a;
    __syncthreads();
    for (int o = 128; o >= 1; o >>= 1) {
        if (tid < o) s_red[tid] = mode ? fmax(s_red[tid], s_red[tid + o]) : s_red[tid] + s_red[tid + o];
        __syncthreads();
    }
    if (tid == 0) dst[0] = s_red[0];
}

__global__ __launch_bounds__(256) void k_eg_correct_points(int n_points, const float *__restrict__ Xw,
                                                           const int *__restrict__ ref_vertex,
                                                           const double *__restrict__ before,
                                                           const double *__restrict__ after, float *__restrict__ out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_points) return;
    const float x0 = Xw[3 * (size_t)i], x1 = Xw[3 * (size_t)i + 1], x2 = Xw[3 * (size_t)i + 2];
    const int r = ref_vertex[i];
    if (r < 0) {
        out[3 * (size_t)i] = x0;
        out[3 * (size_t)i + 1] = x1;
        out[3 * (size_t)i + 2] = x2;
        return;
    }
    const double X[3] = {(double)x0, (double)x1, (double)x2};
    double Y[3], Z[3];
    osgs3::sim3_map(load_s3(before + 8 * (size_t)r), X, Y);
    osgs3::sim3_map(osgs3::sim3_inverse(load_s3(after + 8 * (size_t)r)), Y, Z);
    out[3 * (size_t)i] = (float)Z[0];
    out[3 * (size_t)i + 1] = (float)Z[1];
    out[3 * (size_t)i + 2] = (float)Z[2];
}

struct EgState {
    bool timing = false;
    double ms[OSG_ESSGRAPH_NK] = {};
};

EgState *eg_state(osg_ctx *ctx)
{
    if (!ctx->essgraph_state) ctx->essgraph_state = std::make_shared<EgState>();
    return static_cast<EgState *>(ctx->essgraph_state.get());
}

enum { PH_LIN = 0, PH_ASM, PH_FACTOR, PH_UPDATE, PH_CHI };

// brackets the launches of one phase with the context's two events when timing is on
struct Phase {
    osg_ctx *ctx;
    EgState *st;
    int ph;
    hipEvent_t *ev = nullptr;
    Phase(osg_ctx *c, EgState *s, int p) : ctx(c), st(s), ph(p)
    {
        if (st->timing && (ev = osg_ctx_events(ctx))) (void)hipEventRecord(ev[0], ctx->stream);
    }
    ~Phase()
    {
        if (!ev) return;
        float ms = 0.f;
        if (hipEventRecord(ev[1], ctx->stream) == hipSuccess && hipEventSynchronize(ev[1]) == hipSuccess &&
            hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess)
            st->ms[ph] += ms;
    }
};

inline size_t al256(size_t v) { return (v + 255) & ~size_t(255); }

}  // namespace

extern "C" {

int osg_essgraph_kernel_times(osg_ctx *ctx, int32_t enable, double *ms)
{
    if (!ctx) return OSG_E_INVALID;
    EgState *st = eg_state(ctx);
    if (ms)
        for (int i = 0; i < OSG_ESSGRAPH_NK; i++) ms[i] = st->ms[i];
    st->timing = enable != 0;
    return OSG_OK;
}

}  // extern "C"

namespace {

// The checked graph of either entry point as the shared driver reads it, and what it returns.
struct EgIn {
    int n_vertices, n_edges;
    const uint8_t *fixed;
    const int32_t *e_v0, *e_v1;
    const double *state, *e_meas, *consts;  // K::SD, K::MD, K::CD doubles per vertex / edge / vertex
    int max_iterations;
    double lambda_init;
    int fix_scale;
    Info6 info;
    bool want_edge_chi2;
};
struct EgOut {
    std::vector<double> state, edge_chi2;  // every vertex's returned state; per edge when asked for
    double chi2_initial = 0.0, chi2_final = 0.0;
    int lm_iterations = 0, lm_trials = 0;
};

// what the kernels of a graph kind read
struct EgDev {
    const double *meas, *consts;
    const int *v0, *v1, *fidx;
    int n, E, fix_scale;
    Info6 info;
    hipStream_t stream;
};

// VertexSim3Expmap / EdgeSim3
struct Sim3Graph {
    static constexpr int SD = 8, MD = 8, CD = 0;
    static constexpr bool SPARSE_SLOTS = false;
    static void linearize(const EgDev &D, const double *cur, double *slots)
    {
        hipLaunchKernelGGL(k_eg_linearize, dim3((D.E + 3) / 4), dim3(64), 0, D.stream, cur, D.meas, D.v0, D.v1, D.fidx, D.E,
                           D.fix_scale, slots);
    }
    static void update(const EgDev &D, const double *cur, const double *x, double *trial)
    {
        hipLaunchKernelGGL(k_eg_update, dim3((D.n + 255) / 256), dim3(256), 0, D.stream, cur, x, D.fidx, D.n, D.fix_scale, trial);
    }
    static void chi2(const EgDev &D, const double *state, double *edge_chi)
    {
        hipLaunchKernelGGL(k_eg_chi2, dim3((D.E + 255) / 256), dim3(256), 0, D.stream, state, D.meas, D.v0, D.v1, D.E, edge_chi);
    }
};

// VertexPose4DoF / Edge4DoF.  Its slots keep the 7 x 7 layout with the rows and columns 4..6 left zero, so
// k_eg_assemble, k_eg_damp and k_eg_factor run as they are: those rows of the damped system are lambda on the
// diagonal and 0 elsewhere, their x is 0, and they add nothing to any other entry, to lambda's start or to
// the scale sum.
struct Pose4Graph {
    static constexpr int SD = VS, MD = 12, CD = VC;
    static constexpr bool SPARSE_SLOTS = true;
    static void linearize(const EgDev &D, const double *cur, double *slots)
    {
        hipLaunchKernelGGL(k_eg4_linearize, dim3((D.E + 3) / 4), dim3(64), 0, D.stream, cur, D.consts, D.meas, D.v0, D.v1,
                           D.fidx, D.E, D.info, slots);
    }
    static void update(const EgDev &D, const double *cur, const double *x, double *trial)
    {
        hipLaunchKernelGGL(k_eg4_update, dim3((D.n + 255) / 256), dim3(256), 0, D.stream, cur, D.consts, x, D.fidx, D.n, trial);
    }
    static void chi2(const EgDev &D, const double *state, double *edge_chi)
    {
        hipLaunchKernelGGL(k_eg4_chi2, dim3((D.E + 255) / 256), dim3(256), 0, D.stream, state, D.meas, D.v0, D.v1, D.E, D.info,
                           edge_chi);
    }
};

// SparseOptimizer::optimize on a checked graph of kind K: the structure, the device memory and g2o's
// Levenberg-Marquardt.  Nothing of the caller's is written here.
template <class K>
int eg_solve(osg_ctx *ctx, const EgIn *p, EgOut *r)
{
    const int n = p->n_vertices, E = p->n_edges;
    constexpr size_t SB = 8 * (size_t)K::SD, MB = 8 * (size_t)K::MD, CB = 8 * (size_t)K::CD;
    EgState *st = eg_state(ctx);
    for (int i = 0; i < OSG_ESSGRAPH_NK; i++) st->ms[i] = 0.0;
    if (n == 0) return OSG_OK;

    // ---- host structure: free numbering, CSR lists in edge order, the envelope
    std::vector<int> fidx(n, -1);
    int nf = 0;
    for (int v = 0; v < n; v++)
        if (!p->fixed[v]) fidx[v] = nf++;
    const bool solve = nf > 0 && E > 0;
    const int T = (nf + 3) / 4, nfp = 4 * T;
    std::vector<int> d_ptr(nf + 1, 0), d_ent, p_ptr(1, 0), p_ent, p_hi, p_lo, first(T);
    std::vector<long long> row_off(T);
    size_t n_tiles = 0;
    if (solve) {
        for (int e = 0; e < E; e++) {
            const int a = fidx[p->e_v0[e]], b = fidx[p->e_v1[e]];
            if (a >= 0) d_ptr[a + 1]++;
            if (b >= 0) d_ptr[b + 1]++;
        }
        for (int a = 0; a < nf; a++) d_ptr[a + 1] += d_ptr[a];
        d_ent.resize(d_ptr[nf]);
        std::vector<int> fill(d_ptr.begin(), d_ptr.end() - 1);
        std::vector<std::pair<uint64_t, int>> keyed;  // ((hi, lo), edge << 1 | transpose)
        for (int e = 0; e < E; e++) {
            const int a = fidx[p->e_v0[e]], b = fidx[p->e_v1[e]];
            if (a >= 0) d_ent[fill[a]++] = 2 * e;
            if (b >= 0) d_ent[fill[b]++] = 2 * e + 1;
            if (a >= 0 && b >= 0) {
                // the slot holds J_i^T J_j, block (a, b); the store keeps the lower block (hi, lo)
                const int hi = std::max(a, b), lo = std::min(a, b);
                keyed.emplace_back(((uint64_t)hi << 32) | (uint32_t)lo, 2 * e + (a < b ? 1 : 0));
            }
        }
        std::stable_sort(keyed.begin(), keyed.end(),
                         [](const std::pair<uint64_t, int> &x, const std::pair<uint64_t, int> &y) { return x.first < y.first; });
        for (int t = 0; t < T; t++) first[t] = t;
        for (size_t i = 0; i < keyed.size(); i++) {
            if (i == 0 || keyed[i].first != keyed[i - 1].first) {
                if (i) p_ptr.push_back((int)i);
                const int hi = (int)(keyed[i].first >> 32), lo = (int)(uint32_t)keyed[i].first;
                p_hi.push_back(hi);
                p_lo.push_back(lo);
                first[hi >> 2] = std::min(first[hi >> 2], lo >> 2);
            }
            p_ent.push_back(keyed[i].second);
        }
        p_ptr.push_back((int)keyed.size());
        for (int t = 0; t < T; t++) {
            row_off[t] = (long long)n_tiles;
            n_tiles += (size_t)(t - first[t] + 1);
        }
    }
    const int n_pairs = (int)p_hi.size();

    // ---- device memory.  in: the constant arrays; work: states, vectors, scalars; then the slots and the store
    const size_t o_state = 0, o_meas = o_state + al256(SB * n), o_v0 = o_meas + al256(MB * E);
    const size_t o_v1 = o_v0 + al256(4 * (size_t)E), o_fidx = o_v1 + al256(4 * (size_t)E);
    const size_t o_dptr = o_fidx + al256(4 * (size_t)n), o_dent = o_dptr + al256(4 * d_ptr.size());
    const size_t o_pptr = o_dent + al256(4 * d_ent.size()), o_pent = o_pptr + al256(4 * p_ptr.size());
    const size_t o_phi = o_pent + al256(4 * p_ent.size()), o_plo = o_phi + al256(4 * p_hi.size());
    const size_t o_first = o_plo + al256(4 * p_lo.size()), o_roff = o_first + al256(4 * first.size());
    const size_t o_const = o_roff + al256(8 * row_off.size());
    const size_t in_bytes = o_const + al256(CB * n) + 256;
    const size_t N = (size_t)TB * T;
    const size_t w_trial = al256(SB * n), w_chi = w_trial + al256(SB * n);
    const size_t w_b = w_chi + al256(8 * (size_t)E), w_y = w_b + al256(8 * N), w_xt = w_y + al256(8 * N);
    const size_t w_x = w_xt + al256(8 * N), w_dmax = w_x + al256(8 * N), w_ctl = w_dmax + al256(8 * (size_t)nf);
    const size_t work_bytes = w_ctl + 256;
    char *din = nullptr, *dwork = nullptr;
    double *dslots = nullptr, *dH = nullptr, *dL = nullptr, *dLinv = nullptr;
    OSG_RC(osg_idle(ctx));
    OSG_ALLOC(ctx, din, SLOT_BA0, in_bytes);
    OSG_ALLOC(ctx, dwork, SLOT_BA1, work_bytes);
    const size_t store_bytes = solve ? n_tiles * TE * 8 : 0;
    if (solve) {
        OSG_ALLOC(ctx, dslots, SLOT_BA2, (size_t)ES * 8 * E);
        dH = (double *)osg_scratch(ctx, SLOT_BA3, store_bytes);
        dL = dH ? (double *)osg_scratch(ctx, SLOT_BA4, store_bytes) : nullptr;
        dLinv = dL ? (double *)osg_scratch(ctx, SLOT_BA5, (size_t)T * TE * 8) : nullptr;
        if (!dLinv) {
            (void)hipGetLastError();
            return osg_set_error(ctx, OSG_E_NOMEM, "the matrix store of %zu tiles (2 x %zu B) could not be allocated",
                                 n_tiles, store_bytes);
        }
    }
    st->ms[5] = (double)(2 * store_bytes + (solve ? (size_t)T * TE * 8 : 0));
    std::vector<char> hin(in_bytes, 0);
    std::memcpy(hin.data() + o_state, p->state, SB * n);
    if (CB) std::memcpy(hin.data() + o_const, p->consts, CB * n);
    if (E) {
        std::memcpy(hin.data() + o_meas, p->e_meas, MB * E);
        std::memcpy(hin.data() + o_v0, p->e_v0, 4 * (size_t)E);
        std::memcpy(hin.data() + o_v1, p->e_v1, 4 * (size_t)E);
    }
    std::memcpy(hin.data() + o_fidx, fidx.data(), 4 * (size_t)n);
    auto put = [&](size_t off, const void *src, size_t bytes) {
        if (bytes) std::memcpy(hin.data() + off, src, bytes);
    };
    put(o_dptr, d_ptr.data(), 4 * d_ptr.size());
    put(o_dent, d_ent.data(), 4 * d_ent.size());
    put(o_pptr, p_ptr.data(), 4 * p_ptr.size());
    put(o_pent, p_ent.data(), 4 * p_ent.size());
    put(o_phi, p_hi.data(), 4 * p_hi.size());
    put(o_plo, p_lo.data(), 4 * p_lo.size());
    put(o_first, first.data(), 4 * first.size());
    put(o_roff, row_off.data(), 8 * row_off.size());
    OSG_HIP_CHECK(ctx, hipMemcpyAsync(din, hin.data(), in_bytes, hipMemcpyHostToDevice, ctx->stream));
    OSG_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));  // hin is pageable memory

    const double *d_meas = (const double *)(din + o_meas);
    const int *d_v0 = (const int *)(din + o_v0), *d_v1 = (const int *)(din + o_v1), *d_fidx = (const int *)(din + o_fidx);
    double *cur = (double *)(din + o_state), *trial = (double *)(dwork + 0);
    double *d_chi = (double *)(dwork + w_chi), *d_b = (double *)(dwork + w_b), *d_y = (double *)(dwork + w_y);
    double *d_xt = (double *)(dwork + w_xt), *d_x = (double *)(dwork + w_x), *d_dmax = (double *)(dwork + w_dmax);
    double *d_ctl = (double *)(dwork + w_ctl);
    EgStruct G;
    G.d_ptr = (const int *)(din + o_dptr); G.d_ent = (const int *)(din + o_dent);
    G.p_ptr = (const int *)(din + o_pptr); G.p_ent = (const int *)(din + o_pent);
    G.p_hi = (const int *)(din + o_phi); G.p_lo = (const int *)(din + o_plo);
    G.first = (const int *)(din + o_first); G.row_off = (const long long *)(din + o_roff);
    G.nf = nf; G.nfp = nfp; G.n_pairs = n_pairs; G.T = T;

    double *pin = (double *)osg_pinned(ctx, 4096);
    if (!pin) return osg_set_error(ctx, OSG_E_NOMEM, "pinned alloc failed");
    const int fs = p->fix_scale ? 1 : 0;
    const EgDev D = {d_meas, (const double *)(din + o_const), d_v0, d_v1, d_fidx, n, E, fs, p->info, ctx->stream};
    // computeActiveErrors + activeChi2 at a state -> d_chi, d_ctl[2]
    auto chi_pass = [&](const double *state) -> int {
        Phase ph(ctx, st, PH_CHI);
        K::chi2(D, state, d_chi);
        hipLaunchKernelGGL(k_eg_reduce, dim3(1), dim3(256), 0, ctx->stream, (const double *)d_chi, E, 0, d_ctl + 2);
        OSG_HIP_CHECK(ctx, hipGetLastError());
        return OSG_OK;
    };
    auto read_ctl = [&]() -> int {
        OSG_RC(osg_download(ctx, pin, d_ctl, 64));
        return osg_wait(ctx);
    };
    int iters = 0, trials = 0;
    double chi_init = 0.0, chi_final = 0.0;
    if (E > 0) {
        OSG_RC(chi_pass(cur));
        OSG_RC(read_ctl());
        chi_init = chi_final = pin[2];
    }
    if (solve) {
        OSG_HIP_CHECK(ctx, hipMemsetAsync(dH, 0, store_bytes, ctx->stream));
        OSG_HIP_CHECK(ctx, hipMemsetAsync(d_x, 0, 8 * N, ctx->stream));
        if (K::SPARSE_SLOTS) {
            OSG_HIP_CHECK(ctx, hipMemsetAsync(dslots, 0, (size_t)ES * 8 * E, ctx->stream));
        }
        const int n_iter = p->max_iterations > 0 ? p->max_iterations : 20;
        double lambda = 0, ni = 2, currentChi = chi_init;
        int nBad = 0;
        for (int it = 0; it < n_iter; it++) {
            iters++;
            {
                Phase ph(ctx, st, PH_LIN);
                K::linearize(D, cur, dslots);
            }
            {
                Phase ph(ctx, st, PH_ASM);
                hipLaunchKernelGGL(k_eg_assemble, dim3(nfp + n_pairs), dim3(64), 0, ctx->stream, G, (const double *)dslots, dH,
                                   d_b, d_dmax);
            }
            OSG_HIP_CHECK(ctx, hipGetLastError());
            const double iniChi = currentChi;
            if (it == 0) {
                if (p->lambda_init > 0) {
                    lambda = p->lambda_init;
                } else {  // computeLambdaInit: tau * max |diag H|
                    hipLaunchKernelGGL(k_eg_reduce, dim3(1), dim3(256), 0, ctx->stream, (const double *)d_dmax, nf, 1, d_ctl + 3);
                    OSG_RC(read_ctl());
                    lambda = 1e-5 * pin[3];
                }
                ni = 2;
                nBad = 0;
            }
            double rho = 0;
            int qmax = 0;
            do {
                trials++;
                {
                    Phase ph(ctx, st, PH_FACTOR);
                    hipLaunchKernelGGL(k_eg_copy, dim3((unsigned)std::min<size_t>(1024, (n_tiles * TE + 255) / 256)), dim3(256),
                                       0, ctx->stream, (const double *)dH, dL, n_tiles * TE);
                    hipLaunchKernelGGL(k_eg_damp, dim3((8 * nf + 255) / 256), dim3(256), 0, ctx->stream, G, (const double *)dH,
                                       dL, lambda);
                    hipLaunchKernelGGL(k_eg_factor, dim3(1), dim3(256), 0, ctx->stream, G, dL, dLinv, (const double *)d_b, d_y,
                                       d_xt, d_x, lambda, fs, d_ctl);
                }
                {
                    Phase ph(ctx, st, PH_UPDATE);
                    K::update(D, cur, d_x, trial);
                }
                OSG_HIP_CHECK(ctx, hipGetLastError());
                OSG_RC(chi_pass(trial));
                OSG_RC(read_ctl());
                const bool ok2 = pin[0] == 0.0;
                double tempChi = pin[2];
                if (!ok2) tempChi = DBL_MAX;
                rho = (currentChi - tempChi);
                const double scale = pin[1] + 1e-3;
                rho /= scale;
                if (rho > 0 && std::isfinite(tempChi)) {
                    double alpha = 1. - (2 * rho - 1) * (2 * rho - 1) * (2 * rho - 1);
                    alpha = std::min(alpha, 2. / 3.);
                    const double scaleFactor = std::max(1. / 3., alpha);
                    lambda *= scaleFactor;
                    ni = 2;
                    currentChi = tempChi;
                    std::swap(cur, trial);  // the update is kept
                } else {
                    lambda *= ni;
                    ni *= 2;  // pop: cur is untouched
                }
                qmax++;
            } while (rho < 0 && qmax < 10);
            if (qmax == 10 || rho == 0) break;
            if ((iniChi - currentChi) * 1e3 < iniChi) nBad++;
            else nBad = 0;
            if (nBad >= 3) break;
        }
        OSG_RC(chi_pass(cur));  // the errors of the returned state
        OSG_RC(read_ctl());
        chi_final = pin[2];
    }
    r->state.resize((size_t)K::SD * n);
    r->edge_chi2.resize(p->want_edge_chi2 ? (size_t)E : 0);
    OSG_HIP_CHECK(ctx, hipMemcpyAsync(r->state.data(), cur, SB * n, hipMemcpyDeviceToHost, ctx->stream));
    if (p->want_edge_chi2 && E)
        OSG_HIP_CHECK(ctx, hipMemcpyAsync(r->edge_chi2.data(), d_chi, 8 * (size_t)E, hipMemcpyDeviceToHost, ctx->stream));
    OSG_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    r->chi2_initial = chi_init;
    r->chi2_final = chi_final;
    r->lm_iterations = iters;
    r->lm_trials = trials;
    return OSG_OK;
}

}  // namespace

extern "C" {

int osg_optimize_essential_graph(osg_ctx *ctx, const osg_essgraph_problem *p, osg_essgraph_result *r)
{
    if (!ctx) return OSG_E_INVALID;
    OSG_REQUIRE(ctx, p && r, "null argument");
    const int n = p->n_vertices, E = p->n_edges;
    OSG_REQUIRE(ctx, n >= 0 && n <= 65535, "n_vertices must be in [0, 65535]");
    OSG_REQUIRE(ctx, E >= 0 && E <= (1 << 24), "n_edges must be in [0, 2^24]");
    OSG_REQUIRE(ctx, n == 0 || (p->sim3 && p->fixed && r->sim3), "vertex arrays");
    OSG_REQUIRE(ctx, E == 0 || (p->e_v0 && p->e_v1 && p->e_meas), "edge arrays");
    OSG_REQUIRE(ctx, p->max_iterations >= 0, "max_iterations");
    OSG_REQUIRE(ctx, p->lambda_init >= 0.0, "lambda_init must not be negative");
    for (int v = 0; v < n; v++) OSG_REQUIRE(ctx, p->sim3[8 * (size_t)v + 7] > 0.0, "the scale of vertex %d is not positive", v);
    for (int e = 0; e < E; e++) {
        const int a = p->e_v0[e], b = p->e_v1[e];
        OSG_REQUIRE(ctx, a >= 0 && a < n && b >= 0 && b < n && a != b, "edge %d joins vertices %d and %d", e, a, b);
        OSG_REQUIRE(ctx, p->e_meas[8 * (size_t)e + 7] > 0.0, "the scale of measurement %d is not positive", e);
    }
    EgIn in = {n, E, p->fixed, p->e_v0, p->e_v1, p->sim3, p->e_meas, nullptr, p->max_iterations, p->lambda_init,
               p->fix_scale ? 1 : 0, Info6(), r->edge_chi2 != nullptr};
    EgOut out;
    OSG_RC(eg_solve<Sim3Graph>(ctx, &in, &out));
    // ---- results: written only now, after every step that can fail
    for (int v = 0; v < n; v++)
        std::memcpy(r->sim3 + 8 * (size_t)v, (p->fixed[v] ? p->sim3 : out.state.data()) + 8 * (size_t)v, 64);
    if (r->edge_chi2 && E) std::memcpy(r->edge_chi2, out.edge_chi2.data(), 8 * (size_t)E);
    r->chi2_initial = out.chi2_initial;
    r->chi2_final = out.chi2_final;
    r->lm_iterations = out.lm_iterations;
    r->lm_trials = out.lm_trials;
    return OSG_OK;
}

int osg_essgraph4_check(const osg_essgraph4_problem *p, const osg_essgraph4_result *r)
{
    return osgeg4::check(p, r, nullptr);
}

int osg_optimize_essential_graph_4dof(osg_ctx *ctx, const osg_essgraph4_problem *p, osg_essgraph4_result *r)
{
    if (!ctx) return OSG_E_INVALID;
    const char *why = nullptr;
    if (osgeg4::check(p, r, &why) != 0) return osg_set_error(ctx, OSG_E_INVALID, "%s", why);
    const int n = p->n_vertices, E = p->n_edges;
    std::vector<double> state, consts;
    osgeg4::pack(*p, state, consts);
    EgIn in = {n, E, p->fixed, p->e_v0, p->e_v1, state.data(), p->e_meas, consts.data(), p->max_iterations, p->lambda_init,
               0, Info6(), r->edge_chi2 != nullptr};
    for (int i = 0; i < 6; i++) in.info.w[i] = p->info_diag[i];
    EgOut out;
    OSG_RC(eg_solve<Pose4Graph>(ctx, &in, &out));
    for (int v = 0; v < n; v++) osgeg4::unpack(*p, v, out.state.data(), r->pose + OSG_EG4_POSE_OUT * (size_t)v);
    if (r->edge_chi2 && E) std::memcpy(r->edge_chi2, out.edge_chi2.data(), 8 * (size_t)E);
    r->chi2_initial = out.chi2_initial;
    r->chi2_final = out.chi2_final;
    r->lm_iterations = out.lm_iterations;
    r->lm_trials = out.lm_trials;
    return OSG_OK;
}

int osg_essgraph_correct_points(osg_ctx *ctx, int32_t n_points, const float *Xw, const int32_t *ref_vertex,
                                int32_t n_vertices, const double *sim3_before, const double *sim3_after, float *Xw_out)
{
    if (!ctx) return OSG_E_INVALID;
    OSG_REQUIRE(ctx, n_points >= 0 && n_vertices >= 0, "negative count");
    OSG_REQUIRE(ctx, n_points == 0 || (Xw && ref_vertex && Xw_out), "point arrays");
    OSG_REQUIRE(ctx, n_vertices == 0 || (sim3_before && sim3_after), "vertex arrays");
    for (int i = 0; i < n_points; i++) OSG_REQUIRE(ctx, ref_vertex[i] < n_vertices, "ref_vertex[%d] = %d", i, ref_vertex[i]);
    for (int v = 0; v < n_vertices; v++)
        OSG_REQUIRE(ctx, sim3_before[8 * (size_t)v + 7] > 0.0 && sim3_after[8 * (size_t)v + 7] > 0.0,
                    "the scale of vertex %d is not positive", v);
    if (n_points == 0) return OSG_OK;
    const size_t o_ref = al256(12 * (size_t)n_points), o_b = o_ref + al256(4 * (size_t)n_points);
    const size_t o_a = o_b + al256(64 * (size_t)n_vertices), in_bytes = o_a + al256(64 * (size_t)n_vertices) + 256;
    char *din = nullptr;
    float *dout = nullptr;
    OSG_RC(osg_idle(ctx));
    OSG_ALLOC(ctx, din, SLOT_BA0, in_bytes);
    OSG_ALLOC(ctx, dout, SLOT_BA1, 12 * (size_t)n_points);
    std::vector<char> hin(in_bytes, 0);
    std::memcpy(hin.data(), Xw, 12 * (size_t)n_points);
    std::memcpy(hin.data() + o_ref, ref_vertex, 4 * (size_t)n_points);
    if (n_vertices) {
        std::memcpy(hin.data() + o_b, sim3_before, 64 * (size_t)n_vertices);
        std::memcpy(hin.data() + o_a, sim3_after, 64 * (size_t)n_vertices);
    }
    OSG_HIP_CHECK(ctx, hipMemcpyAsync(din, hin.data(), in_bytes, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_eg_correct_points, dim3((n_points + 255) / 256), dim3(256), 0, ctx->stream, n_points,
                       (const float *)din, (const int *)(din + o_ref), (const double *)(din + o_b),
                       (const double *)(din + o_a), dout);
    OSG_HIP_CHECK(ctx, hipGetLastError());
    std::vector<float> out(3 * (size_t)n_points);
    OSG_HIP_CHECK(ctx, hipMemcpyAsync(out.data(), dout, 12 * (size_t)n_points, hipMemcpyDeviceToHost, ctx->stream));
    OSG_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    std::memcpy(Xw_out, out.data(), 12 * (size_t)n_points);
    return OSG_OK;
}

}  // extern "C"
