// sim3opt.hip — Optimizer::OptimizeSim3 (ref:src/Optimizer.cc:4213-4512) for a batch of problems.
//
// One workgroup of NT = 128 lanes (two waves) per problem, persistent over the whole call:
// optimize(5) with Huber -> pair classification -> (early return | optimize(5 | 10) without Huber ->
// computeError + classification), with g2o's Levenberg-Marquardt control flow
// (ref:Thirdparty/g2o/g2o/core/optimization_algorithm_levenberg.cpp:61-169) executed in-kernel, one
// launch per call or batch.
//
//   * The graph has one free vertex, the 7-DoF VertexSim3Expmap, and the reference gives its edges no
//     linearizeOplus: g2o differentiates them numerically (ref:Thirdparty/g2o/g2o/core/
//     base_binary_edge.hpp:147-200), column d = (err(S (+) delta e_d) - err(S (+) -delta e_d)) / (2 delta)
//     with delta = 1e-9 and (+) = Sim3(update) * S.  Once per linearisation lanes 0..14 build the
//     central state, the 14 perturbed ones and all 15 inverses in LDS; the pair lanes only read them.
//   * Pair i lives on lane i % NT of chunk i / NT.  A lane evaluates both edges of its pair at the 15
//     states, forms the two 2x7 Jacobians and adds the pair's 28 + 7 + 1 terms (H upper, b, robust
//     chi2) to private accumulators over its chunks.  The accumulators are then summed by a wave
//     butterfly and the two waves' sums added in wave order in LDS: the same order every run
//     (deterministic), not the reference's edge order (the result is defined up to the differentiation
//     noise anyway).
//   * Lane 0 runs the damped 7x7 LDL^T, the update and the lambda / rho control and broadcasts the
//     state and a control word through LDS.
//   * The pairs nulled by the first classification are a per-lane bit mask (bit c <-> chunk c).
//     Classification reads each pair's errors at the state of the LAST error evaluation (a rejected
//     trial's, when the last trial of optimize() was rejected), as the reference reads e->chi2().
#include <cfloat>
#include <cstring>
#include <vector>

#include "ba_common.h"
#include "batch_io.h"
#include "sim3_common.h"
#include "small_linalg.h"

using namespace osgba;
using osgs3::Sim3;

namespace {

constexpr int NT = 128;        // lanes per problem
constexpr int NWV = NT / 64;   // waves per problem
constexpr int NS = 36;         // H upper (28) | b (7) | robust chi2 (1)
constexpr int NST = 15;        // central | +delta e_0, -delta e_0, ..., +delta e_6, -delta e_6

struct S3ProbDev {
    double q[4], t[3], s;
    int fix_scale;
    float th2;
    int n_pairs, pair_off, max_iterations, pad;
    osg_camera cam1, cam2;
};

struct S3Out {
    double q[4], t[3], s;
    double chi2_final;
    int n_inliers, n_bad_first, early_return, pad;
    int lm_iterations[2], lm_trials[2];
};

struct S3Shared {
    osg_camera cam1, cam2;
    Sim3 st[NST], inv[NST];  // [0]: the state of the last error evaluation
    Sim3 est;                // the vertex estimate
    double red[NWV][NS];
    double sys[NS];          // the last buildSystem sums
    double chi;              // the last chi2-only pass
    int cnt[NWV];
    int ctl;                 // lane 0's decision after a trial: 0 next trial, 1 next iteration, 2 terminate
};

struct S3Pair {
    double p1[3], p2[3], o1[2], o2[2];
    double w1, w2;
};

struct E4 {
    double a0, a1, b0, b1;  // e12, e21
};

// EdgeSim3ProjectXYZ / EdgeInverseSim3ProjectXYZ computeError (ref:include/OptimizableTypes.h:201-230)
// at state k
__device__ __forceinline__ E4 pair_errors(const S3Pair &P, const S3Shared *S, int k)
{
    double x[3], uv[2];
    E4 e;
    osgs3::sim3_map(S->st[k], P.p2, x);
    cam_project(S->cam1, x, uv);
    e.a0 = P.o1[0] - uv[0];
    e.a1 = P.o1[1] - uv[1];
    osgs3::sim3_map(S->inv[k], P.p1, x);
    cam_project(S->cam2, x, uv);
    e.b0 = P.o2[0] - uv[0];
    e.b1 = P.o2[1] - uv[1];
    return e;
}

__device__ inline double chi2_2(double e0, double e1, double w)
{
    double s = 0;
    s += e0 * (w * e0);
    s += e1 * (w * e1);
    return s;
}

__global__ __launch_bounds__(NT) void k_sim3_opt(const S3ProbDev *__restrict__ probs,
                                                 const double *__restrict__ a_p1c,
                                                 const double *__restrict__ a_p2c,
                                                 const double *__restrict__ a_obs1,
                                                 const double *__restrict__ a_obs2,
                                                 const float *__restrict__ a_w1,
                                                 const float *__restrict__ a_w2,
                                                 uint8_t *__restrict__ a_state,
                                                 double *__restrict__ a_chi2, S3Out *__restrict__ out)
{
    __shared__ S3Shared S;
    // the lanes' 4 x 7 Jacobians, entry (r, d) of lane t at s_J[(7 r + d) NT + t]: the loop over the
    // perturbed states stays rolled (one copy of the camera model) without a dynamic register index
    __shared__ double s_J[28 * NT];
    const S3ProbDev &P = probs[blockIdx.x];
    const int n = P.n_pairs;
    const size_t off = (size_t)P.pair_off;
    const double *p1c = a_p1c + 3 * off, *p2c = a_p2c + 3 * off;
    const double *obs1 = a_obs1 + 2 * off, *obs2 = a_obs2 + 2 * off;
    const float *w1 = a_w1 + off, *w2 = a_w2 + off;
    uint8_t *pstate = a_state + off;
    double *pchi2 = a_chi2 + 2 * off;
    const int tid = threadIdx.x, wave = tid / 64, lane = tid % 64;
    const int nch = (n + NT - 1) / NT;  // <= 64 (checked by the host)
    const bool fix_scale = P.fix_scale != 0;
    const double th2 = (double)P.th2;
    // const float deltaHuber = sqrt(th2); RobustKernelHuber keeps delta^2 as a float (ba_common.h huber)
    const float delta_f = sqrtf(P.th2);
    const double hdelta = delta_f;
    const float hdsqr = (float)((double)delta_f * (double)delta_f);

    if (tid == 0) {
        S.cam1 = P.cam1;
        S.cam2 = P.cam2;
        for (int i = 0; i < 4; i++) S.est.q[i] = P.q[i];
        for (int i = 0; i < 3; i++) S.est.t[i] = P.t[i];
        S.est.s = P.s;
        S.st[0] = S.est;
        S.inv[0] = osgs3::sim3_inverse(S.est);
    }
    __syncthreads();

    uint64_t dead = 0;  // bit c: this lane's pair of chunk c was nulled by the first classification
    auto pair_of = [&](int c) { return c * NT + tid; };
    auto active = [&](int c) { return pair_of(c) < n && !((dead >> c) & 1); };
    auto load_pair = [&](int i) {
        S3Pair Q;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            Q.p1[k] = p1c[3 * i + k];
            Q.p2[k] = p2c[3 * i + k];
        }
        Q.o1[0] = obs1[2 * i];
        Q.o1[1] = obs1[2 * i + 1];
        Q.o2[0] = obs2[2 * i];
        Q.o2[1] = obs2[2 * i + 1];
        Q.w1 = (double)w1[i];
        Q.w2 = (double)w2[i];
        return Q;
    };
    // the NQ private sums of every lane -> dst[0..NQ): wave butterfly, then the waves in order
    auto block_sum = [&](double *acc, int nq, double *dst) {
        for (int q = 0; q < nq; q++) {
            const double v = wave_sum(acc[q]);
            if (lane == 0) S.red[wave][q] = v;
        }
        __syncthreads();
        if (tid < nq) {
            double s = S.red[0][tid];
#pragma unroll
            for (int w = 1; w < NWV; w++) s += S.red[w][tid];
            dst[tid] = s;
        }
        __syncthreads();
    };
    auto block_count = [&](int v) -> int {
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
        if (lane == 0) S.cnt[wave] = v;
        __syncthreads();
        int t = 0;
#pragma unroll
        for (int w = 0; w < NWV; w++) t += S.cnt[w];
        __syncthreads();
        return t;
    };
    // computeActiveErrors + activeRobustChi2 at st[0] -> S.chi
    auto chi_pass = [&](bool robust) {
        double acc = 0.0;
        for (int c = 0; c < nch; c++) {
            if (!active(c)) continue;
            const S3Pair Q = load_pair(pair_of(c));
            const E4 e = pair_errors(Q, &S, 0);
            double ca = chi2_2(e.a0, e.a1, Q.w1), cb = chi2_2(e.b0, e.b1, Q.w2);
            if (robust) {
                double r1;
                huber(ca, hdelta, hdsqr, ca, r1);
                huber(cb, hdelta, hdsqr, cb, r1);
            }
            acc += ca;
            acc += cb;
        }
        block_sum(&acc, 1, &S.chi);
    };
    // the 15 states of a linearisation at S.est (lanes 0..14), then activeRobustChi2 + buildSystem
    auto sys_pass = [&](bool robust) {
        if (tid < NST) {
            Sim3 T = S.est;
            if (tid > 0) {
                const int d = (tid - 1) >> 1;
                double upd[7] = {0, 0, 0, 0, 0, 0, 0};
                const double dl = (tid & 1) ? 1e-9 : -1e-9;
#pragma unroll
                for (int k = 0; k < 7; k++)
                    if (k == d) upd[k] = dl;
                T = osgs3::sim3_oplus(T, upd, fix_scale);
            }
            S.st[tid] = T;
            S.inv[tid] = osgs3::sim3_inverse(T);
        }
        __syncthreads();
        double acc[NS];
#pragma unroll
        for (int q = 0; q < NS; q++) acc[q] = 0.0;
        for (int c = 0; c < nch; c++) {
            if (!active(c)) continue;
            const S3Pair Q = load_pair(pair_of(c));
            const E4 e = pair_errors(Q, &S, 0);
            const double ca = chi2_2(e.a0, e.a1, Q.w1), cb = chi2_2(e.b0, e.b1, Q.w2);
            double r0a = ca, r1a = 1.0, r0b = cb, r1b = 1.0;
            if (robust) {
                huber(ca, hdelta, hdsqr, r0a, r1a);
                huber(cb, hdelta, hdsqr, r0b, r1b);
            }
            acc[35] += r0a;
            acc[35] += r0b;
            const double scalar = 1.0 / (2 * 1e-9);
#pragma unroll 1
            for (int d = 0; d < 7; d++) {
                const E4 ep = pair_errors(Q, &S, 1 + 2 * d);
                const E4 em = pair_errors(Q, &S, 2 + 2 * d);
                s_J[(0 + d) * NT + tid] = scalar * (ep.a0 - em.a0);
                s_J[(7 + d) * NT + tid] = scalar * (ep.a1 - em.a1);
                s_J[(14 + d) * NT + tid] = scalar * (ep.b0 - em.b0);
                s_J[(21 + d) * NT + tid] = scalar * (ep.b1 - em.b1);
            }
            double J[4][7];  // each lane reads back only what it wrote
#pragma unroll
            for (int r = 0; r < 4; r++)
#pragma unroll
                for (int d = 0; d < 7; d++) J[r][d] = s_J[(7 * r + d) * NT + tid];
            const double wa = r1a * Q.w1, wb = r1b * Q.w2;
            int q = 0;
#pragma unroll
            for (int i = 0; i < 7; i++)
#pragma unroll
                for (int j = i; j < 7; j++) {
                    double h = 0;
                    h += J[0][i] * wa * J[0][j];
                    h += J[1][i] * wa * J[1][j];
                    h += J[2][i] * wb * J[2][j];
                    h += J[3][i] * wb * J[3][j];
                    acc[q++] += h;
                }
#pragma unroll
            for (int i = 0; i < 7; i++) {
                double sb = 0;
                sb += r1a * J[0][i] * (Q.w1 * e.a0);
                sb += r1a * J[1][i] * (Q.w1 * e.a1);
                sb += r1b * J[2][i] * (Q.w2 * e.b0);
                sb += r1b * J[3][i] * (Q.w2 * e.b1);
                acc[28 + i] -= sb;
            }
        }
        block_sum(acc, NS, S.sys);
    };

    int iters[2] = {0, 0}, trials[2] = {0, 0};
    int n_bad_first = 0, n_in = 0, early = 0;
    // lane 0's LM state
    double lambda = 0, ni = 2, currentChi = 0, iniChi = 0, rho = 0;
    double xs[7] = {0, 0, 0, 0, 0, 0, 0};
    Sim3 backup = S.est;
    int nBadLM = 0, qmax = 0;

    for (int pass = 0; pass < 2; pass++) {
        const bool robust = pass == 0;
        int niter = pass == 0 ? 5 : (n_bad_first > 0 ? 10 : 5);
        if (P.max_iterations > 0) niter = min(niter, P.max_iterations);
        if (n == 0) niter = 0;  // optimize() on an empty graph does nothing
        for (int iter = 0; iter < niter; iter++) {
            iters[pass]++;
            sys_pass(robust);
            if (tid == 0) {
                iniChi = S.sys[35];
                currentChi = iniChi;
                if (iter == 0) {  // computeLambdaInit: tau * max |diag H|
                    double md = 0;
                    int q = 0;
                    for (int i = 0; i < 7; i++) {
                        md = fmax(fabs(S.sys[q]), md);
                        q += 7 - i;
                    }
                    lambda = 1e-5 * md;
                    ni = 2;
                    nBadLM = 0;
                }
                rho = 0;
                qmax = 0;
            }
            int ctl = 0;
            do {
                trials[pass]++;
                bool ok2 = true;
                if (tid == 0) {
                    backup = S.est;  // push
                    double A[7][7], bvec[7];
                    int q = 0;
#pragma unroll
                    for (int i = 0; i < 7; i++)
#pragma unroll
                        for (int j = i; j < 7; j++) {
                            A[i][j] = S.sys[q] + (i == j ? lambda : 0.0);
                            A[j][i] = A[i][j];
                            q++;
                        }
#pragma unroll
                    for (int i = 0; i < 7; i++) bvec[i] = S.sys[28 + i];
                    double x[7];
                    ok2 = osgla::ldlt_solve<7>(A, bvec, x);
                    if (ok2)
#pragma unroll
                        for (int i = 0; i < 7; i++) xs[i] = x[i];
                    // oplusImpl zeroes update[6] in the solver's own x under _fix_scale
                    if (fix_scale) xs[6] = 0;
                    S.est = osgs3::sim3_oplus(S.est, xs, fix_scale);  // applied before ok2 is read
                    S.st[0] = S.est;
                    S.inv[0] = osgs3::sim3_inverse(S.est);
                }
                __syncthreads();
                chi_pass(robust);
                if (tid == 0) {
                    double tempChi = S.chi;
                    if (!ok2) tempChi = DBL_MAX;
                    rho = (currentChi - tempChi);
                    double scale = 0.;
#pragma unroll
                    for (int j = 0; j < 7; j++) scale += xs[j] * (lambda * xs[j] + S.sys[28 + j]);
                    scale += 1e-3;
                    rho /= scale;
                    if (rho > 0 && isfinite(tempChi)) {
                        double alpha = 1. - osgx::cube_rn(2 * rho - 1);
                        alpha = fmin(alpha, 2. / 3.);
                        const double scaleFactor = fmax(1. / 3., alpha);
                        lambda *= scaleFactor;
                        ni = 2;
                        currentChi = tempChi;
                    } else {
                        lambda *= ni;
                        ni *= 2;
                        S.est = backup;  // pop (the errors stay those of the rejected trial)
                    }
                    qmax++;
                    int c = 0;
                    if (!(rho < 0 && qmax < 10)) {
                        c = 1;
                        if (qmax == 10 || rho == 0) c = 2;
                        else {
                            if ((iniChi - currentChi) * 1e3 < iniChi) nBadLM++;
                            else nBadLM = 0;
                            if (nBadLM >= 3) c = 2;
                        }
                    }
                    S.ctl = c;
                }
                __syncthreads();
                ctl = S.ctl;
            } while (ctl == 0);
            if (ctl == 2) break;
        }
        if (pass == 1) break;
        // first classification (ref:src/Optimizer.cc:4436-4465) on the last computed errors
        int bad = 0;
        for (int c = 0; c < nch; c++) {
            const int i = pair_of(c);
            if (i >= n) continue;
            const S3Pair Q = load_pair(i);
            const E4 e = pair_errors(Q, &S, 0);
            const double ca = chi2_2(e.a0, e.a1, Q.w1), cb = chi2_2(e.b0, e.b1, Q.w2);
            pchi2[2 * i] = ca;
            pchi2[2 * i + 1] = cb;
            const bool b = ca > th2 || cb > th2;
            pstate[i] = b ? 1 : 0;
            if (b) dead |= uint64_t(1) << c;
            bad += b ? 1 : 0;
        }
        n_bad_first = block_count(bad);
        if (n - n_bad_first < 10) {  // :4474-4475, g2oS12 is not written
            early = 1;
            break;
        }
    }
    // the returned state: the estimate, or the input on the early return; computeError() there
    __syncthreads();
    if (tid == 0) {
        if (early) {
            for (int i = 0; i < 4; i++) S.est.q[i] = P.q[i];
            for (int i = 0; i < 3; i++) S.est.t[i] = P.t[i];
            S.est.s = P.s;
        }
        S.st[0] = S.est;
        S.inv[0] = osgs3::sim3_inverse(S.est);
    }
    __syncthreads();
    int nin = 0;
    double csum = 0.0;
    for (int c = 0; c < nch; c++) {
        if (!active(c)) continue;
        const int i = pair_of(c);
        const S3Pair Q = load_pair(i);
        const E4 e = pair_errors(Q, &S, 0);
        const double ca = chi2_2(e.a0, e.a1, Q.w1), cb = chi2_2(e.b0, e.b1, Q.w2);
        if (early) {  // no final check: the survivors of the first classification keep state 0
            csum += ca;
            csum += cb;
            continue;
        }
        pchi2[2 * i] = ca;
        pchi2[2 * i + 1] = cb;
        if (ca > th2 || cb > th2) pstate[i] = 2;
        else {
            nin++;
            csum += ca;
            csum += cb;
        }
    }
    n_in = early ? 0 : block_count(nin);
    block_sum(&csum, 1, &S.chi);
    if (tid == 0) {
        S3Out &o = out[blockIdx.x];
        for (int i = 0; i < 4; i++) o.q[i] = S.est.q[i];
        for (int i = 0; i < 3; i++) o.t[i] = S.est.t[i];
        o.s = S.est.s;
        o.chi2_final = S.chi;
        o.n_inliers = n_in;
        o.n_bad_first = n_bad_first;
        o.early_return = early;
        for (int k = 0; k < 2; k++) {
            o.lm_iterations[k] = iters[k];
            o.lm_trials[k] = trials[k];
        }
    }
}

}  // namespace

extern "C" {

int osg_optimize_sim3_batch(osg_ctx *ctx, const osg_sim3_problem *p, int32_t nb, osg_sim3_result *r)
{
    if (!ctx) return OSG_E_INVALID;
    OSG_REQUIRE(ctx, nb >= 0 && (nb == 0 || (p && r)), "null argument");
    if (nb == 0) return 0;
    std::vector<S3ProbDev> hp(nb);
    size_t total = 0;
    for (int b = 0; b < nb; b++) {
        const osg_sim3_problem &q = p[b];
        OSG_REQUIRE(ctx, q.n_pairs >= 0 && q.n_pairs <= 64 * NT, "n_pairs must be in [0, %d]", 64 * NT);
        OSG_REQUIRE(ctx, q.n_pairs == 0 || (q.p1c && q.p2c && q.obs1 && q.obs2 && q.inv_sigma2_1 && q.inv_sigma2_2 &&
                                            r[b].pair_state),
                    "pair arrays");
        OSG_REQUIRE(ctx, q.max_iterations >= 0, "max_iterations");
        OSG_REQUIRE(ctx, q.th2 > 0.f && q.s > 0.0, "th2 and the scale must be positive");
        S3ProbDev &d = hp[b];
        std::memset(&d, 0, sizeof d);
        for (int i = 0; i < 4; i++) d.q[i] = q.q[i];
        for (int i = 0; i < 3; i++) d.t[i] = q.t[i];
        d.s = q.s;
        d.fix_scale = q.fix_scale;
        d.th2 = q.th2;
        d.n_pairs = q.n_pairs;
        d.pair_off = (int)total;
        d.max_iterations = q.max_iterations;
        d.cam1 = q.cam1;
        d.cam2 = q.cam2;
        total += (size_t)q.n_pairs;
    }
    OSG_REQUIRE(ctx, total < (size_t(1) << 28), "too many pairs in one batch");
    osg_batch_io io(ctx);
    const osg_seg i_pr = io.in(sizeof(S3ProbDev), nb), i_p1 = io.in(3 * sizeof(double), total), i_p2 = io.in(3 * sizeof(double), total);
    const osg_seg i_o1 = io.in(2 * sizeof(double), total), i_o2 = io.in(2 * sizeof(double), total);
    const osg_seg i_w1 = io.in(sizeof(float), total), i_w2 = io.in(sizeof(float), total);
    const osg_seg o_st = io.out(1, total), o_chi = io.out(2 * sizeof(double), total), o_res = io.out(sizeof(S3Out), nb);
    io.in(1, 256), io.out(1, 256);  // slack behind both blocks
    OSG_RC(io.stage());
    io.put(i_pr, 0, hp.data(), nb);
    for (int b = 0; b < nb; b++) {
        const size_t off = hp[b].pair_off, m = p[b].n_pairs;
        io.put(i_p1, off, p[b].p1c, m);
        io.put(i_p2, off, p[b].p2c, m);
        io.put(i_o1, off, p[b].obs1, m);
        io.put(i_o2, off, p[b].obs2, m);
        io.put(i_w1, off, p[b].inv_sigma2_1, m);
        io.put(i_w2, off, p[b].inv_sigma2_2, m);
    }
    OSG_RC(io.upload());
    OSG_RC(io.start());
    hipLaunchKernelGGL(k_sim3_opt, dim3(nb), dim3(NT), 0, ctx->stream, io.dev_in<const S3ProbDev>(i_pr),
                       io.dev_in<const double>(i_p1), io.dev_in<const double>(i_p2), io.dev_in<const double>(i_o1),
                       io.dev_in<const double>(i_o2), io.dev_in<const float>(i_w1), io.dev_in<const float>(i_w2),
                       io.dev_out<uint8_t>(o_st), io.dev_out<double>(o_chi), io.dev_out<S3Out>(o_res));
    OSG_HIP_CHECK(ctx, hipGetLastError());
    OSG_RC(io.finish(io.out_bytes));
    const S3Out *res = io.result<S3Out>(o_res);
    int sum = 0;
    for (int b = 0; b < nb; b++) {
        const S3Out &o = res[b];
        for (int i = 0; i < 4; i++) r[b].q[i] = o.q[i];
        for (int i = 0; i < 3; i++) r[b].t[i] = o.t[i];
        r[b].s = o.s;
        r[b].n_inliers = o.n_inliers;
        r[b].n_bad_first = o.n_bad_first;
        r[b].early_return = o.early_return;
        r[b].chi2_final = o.chi2_final;
        for (int k = 0; k < 2; k++) {
            r[b].lm_iterations[k] = o.lm_iterations[k];
            r[b].lm_trials[k] = o.lm_trials[k];
        }
        io.get(r[b].pair_state, o_st, hp[b].pair_off, p[b].n_pairs);
        if (r[b].pair_chi2) io.get(r[b].pair_chi2, o_chi, hp[b].pair_off, p[b].n_pairs);
        sum += o.n_inliers;
    }
    return sum;
}

int osg_optimize_sim3(osg_ctx *ctx, const osg_sim3_problem *p, osg_sim3_result *r)
{
    const int rc = osg_optimize_sim3_batch(ctx, p, 1, r);
    return rc < 0 ? rc : r->n_inliers;
}

}  // extern "C"
