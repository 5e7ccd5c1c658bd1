// preintegrate.hip — IMU::Preintegrated::IntegrateNewMeasurement (ref:src/ImuTypes.cc:246-323) over B independent
// measurement lists in one launch, and the host helpers of include/osg_imu.h.
//
// k_imu_preintegrate: one wave per preintegration, IMU_W waves per workgroup, no cross-wave synchronisation.
// The step loop is sequential as in the reference (dR is normalised at every step, float products do not
// reassociate).  Per step the 3 x 3 chain (avgA, avgW, dP, dV, the blocks of A and B, the five Jacobians,
// IntegratedRotation, NormalizeRotation) runs in registers, redundantly on every lane (DESIGN.md 3.27 has the
// times of this and of the chain on lane 0 alone, which is slower for few lists); lane 0 leaves the six 3 x 3
// blocks of A and B in the wave's LDS, and the 81 outputs of (A C) A' + (B Nga) B' are spread over the lanes, two
// passes of 64 and 17.  Terms that multiply a structural zero of A or B are skipped and its identity blocks are
// added unmultiplied; the kept terms are summed in ascending k.  Built without FMA contraction; parity is
// tolerance-based.
#include <cstring>
#include <unordered_map>
#include <vector>

#include "batch_io.h"
#include "imu_common.h"
#include "so3_common.h"

using namespace osgso3;
using osgimu::ProbDev;

namespace {

constexpr int IMU_W = 4;          // preintegrations (waves) per workgroup
constexpr int NT = 64 * IMU_W;
constexpr float IMU_EPS = 1e-4f;  // ref:src/ImuTypes.cc:31

// the blocks of A and B a step leaves for the covariance update, 9 floats each, row-major
enum { M_DRT = 0, M_A30, M_A60, M_BG, M_B33, M_B63, M_COUNT };

struct WaveLds {
    float C[225];
    float T[81];
    float M[M_COUNT * 9];
    float dt;
};

struct Chain {
    float dR[9], dV[3], dP[3], JRg[9], JVg[9], JVa[9], JPg[9], JPa[9], avgA[3], avgW[3], b[6], dT;
};

// everything of one wave that goes through LDS is written and read by that wave alone: program order is
// enough for the hardware, the fences keep the compiler from moving accesses across
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ref:src/ImuTypes.cc:264-305, 318-322 on the registers of one lane; M receives the blocks of A and B
__device__ __forceinline__ void chain_step(Chain &s, const float *m, float *M)
{
    const float dt = m[6];
    float acc[3], accW[3], Racc[3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        acc[i] = m[i] - s.b[i];
        accW[i] = m[3 + i] - s.b[3 + i];
    }
    m3_vec(s.dR, acc, Racc);
    const float dTn = s.dT + dt;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        s.avgA[i] = (s.dT * s.avgA[i] + Racc[i] * dt) / dTn;
        s.avgW[i] = (s.dT * s.avgW[i] + accW[i] * dt) / dTn;
    }
    // dP from the old dV and dR, then dV from the old dR
    float hR[9], hRacc[3];
#pragma unroll
    for (int i = 0; i < 9; i++) hR[i] = 0.5f * s.dR[i];
    m3_vec(hR, acc, hRacc);
#pragma unroll
    for (int i = 0; i < 3; i++) {
        s.dP[i] = (s.dP[i] + s.dV[i] * dt) + (hRacc[i] * dt) * dt;
        s.dV[i] = s.dV[i] + Racc[i] * dt;
    }
    // the velocity and position blocks of A and B
    float Wacc[9], X[9], Rdt[9], hRdt2[9];
    hat3(acc, Wacc);
#pragma unroll
    for (int i = 0; i < 9; i++) X[i] = -s.dR[i] * dt;
    m3_mul(X, Wacc, M + 9 * M_A30);
#pragma unroll
    for (int i = 0; i < 9; i++) X[i] = ((-0.5f * s.dR[i]) * dt) * dt;
    m3_mul(X, Wacc, M + 9 * M_A60);
#pragma unroll
    for (int i = 0; i < 9; i++) {
        Rdt[i] = s.dR[i] * dt;
        hRdt2[i] = (hR[i] * dt) * dt;
        M[9 * M_B33 + i] = Rdt[i];
        M[9 * M_B63 + i] = hRdt2[i];
    }
    // JPa, JPg, JVa, JVg from the old JRg
    float Y[9], Z[9];
    m3_mul(hRdt2, Wacc, Y);
    m3_mul(Y, s.JRg, Z);
#pragma unroll
    for (int i = 0; i < 9; i++) {
        s.JPa[i] = (s.JPa[i] + s.JVa[i] * dt) - hRdt2[i];
        s.JPg[i] = (s.JPg[i] + s.JVg[i] * dt) - Z[i];
    }
    m3_mul(Rdt, Wacc, Y);
    m3_mul(Y, s.JRg, Z);
#pragma unroll
    for (int i = 0; i < 9; i++) {
        s.JVa[i] = s.JVa[i] - Rdt[i];
        s.JVg[i] = s.JVg[i] - Z[i];
    }
    // IntegratedRotation (ref:src/ImuTypes.cc:124-151)
    float v[3];
#pragma unroll
    for (int i = 0; i < 3; i++) v[i] = accW[i] * dt;
    const float d2 = v[0] * v[0] + v[1] * v[1] + v[2] * v[2];
    const float d = sqrtf(d2);
    float Wv[9], deltaR[9], rightJ[9];
    hat3(v, Wv);
    if (d < IMU_EPS) {
#pragma unroll
        for (int i = 0; i < 9; i++) {
            deltaR[i] = ((i % 4 == 0) ? 1.f : 0.f) + Wv[i];
            rightJ[i] = (i % 4 == 0) ? 1.f : 0.f;
        }
    } else {
        float W2[9];
        m3_mul(Wv, Wv, W2);
        const float sd = sinf(d), cd = cosf(d);
        const float omc = 1.0f - cd, dms = d - sd, d3 = d2 * d;
#pragma unroll
        for (int i = 0; i < 9; i++) {
            const float I = (i % 4 == 0) ? 1.f : 0.f;
            deltaR[i] = (I + Wv[i] * sd / d) + W2[i] * omc / d2;
            rightJ[i] = (I - Wv[i] * omc / d2) + W2[i] * dms / d3;
        }
    }
    float Rn[9];
    m3_mul(s.dR, deltaR, Rn);
    normalize_rotation<float>(Rn);
#pragma unroll
    for (int i = 0; i < 9; i++) s.dR[i] = Rn[i];
    // the rotation blocks of A and B, then JRg
    float dRt[9], Jdt[9];
    m3_t(deltaR, dRt);
#pragma unroll
    for (int i = 0; i < 9; i++) {
        Jdt[i] = rightJ[i] * dt;
        M[9 * M_DRT + i] = dRt[i];
        M[9 * M_BG + i] = Jdt[i];
    }
    m3_mul(dRt, s.JRg, Y);
#pragma unroll
    for (int i = 0; i < 9; i++) s.JRg[i] = Y[i] - Jdt[i];
    s.dT = dTn;
}

// output o of T = A C: row i = 3 bi + ii of A is [M_bi(ii, :), then dt or 1 at column 3 + ii, 1 at 6 + ii]
__device__ __forceinline__ float row_times_C(const WaveLds &L, int o)
{
    const int i = o / 9, j = o - 9 * i, bi = i / 3, ii = i - 3 * bi;
    const float *a = L.M + 9 * bi + 3 * ii;  // M_DRT, M_A30, M_A60 are blocks 0, 1, 2
    float s = a[0] * L.C[j];
    s += a[1] * L.C[15 + j];
    s += a[2] * L.C[30 + j];
    if (bi == 1) s += L.C[15 * (3 + ii) + j];
    if (bi == 2) {
        s += L.dt * L.C[15 * (3 + ii) + j];
        s += L.C[15 * (6 + ii) + j];
    }
    return s;
}

// output o of (T A') + (B Nga) B'
__device__ __forceinline__ float new_C(const WaveLds &L, const float *nga, int o)
{
    const int i = o / 9, j = o - 9 * i, bi = i / 3, ii = i - 3 * bi, bj = j / 3, jj = j - 3 * bj;
    const float *t = L.T + 9 * i, *a = L.M + 9 * bj + 3 * jj;
    float u = t[0] * a[0];
    u += t[1] * a[1];
    u += t[2] * a[2];
    if (bj == 1) u += t[3 + jj];
    if (bj == 2) {
        u += t[3 + jj] * L.dt;
        u += t[6 + jj];
    }
    float v = 0.f;
    if ((bi == 0) == (bj == 0)) {
        const float *bl = L.M + 9 * (M_BG + bi) + 3 * ii, *br = L.M + 9 * (M_BG + bj) + 3 * jj;
        const float *g = nga + (bi == 0 ? 0 : 3);
        v = (bl[0] * g[0]) * br[0];
        v += (bl[1] * g[1]) * br[1];
        v += (bl[2] * g[2]) * br[2];
    }
    return u + v;
}

// Two waves per SIMD: left to itself the compiler takes 256 VGPRs and 2 AGPRs, which allows one; capped at 256
// registers it spills 7 of them to scratch, costs 1 % up to 1 024 lists and is 22 % faster at 4 096
// (DESIGN.md 3.27).
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(2))) void k_imu_preintegrate(
    const ProbDev *__restrict__ probs, const float *__restrict__ meas, osg_imu_preintegrated *__restrict__ out, int nb)
{
    __shared__ WaveLds lds[IMU_W];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int b = blockIdx.x * IMU_W + wave;
    if (b >= nb) return;  // whole waves leave; nothing below synchronises across waves
    WaveLds &L = lds[wave];
    const ProbDev &P = probs[b];
    const bool cont = P.has_init != 0;
    const osg_pio_preintegrated &I = P.init.pre;

    Chain s;
#pragma unroll
    for (int i = 0; i < 9; i++) {
        s.dR[i] = cont ? I.dR[i] : ((i % 4 == 0) ? 1.f : 0.f);
        s.JRg[i] = cont ? I.JRg[i] : 0.f;
        s.JVg[i] = cont ? I.JVg[i] : 0.f;
        s.JVa[i] = cont ? I.JVa[i] : 0.f;
        s.JPg[i] = cont ? I.JPg[i] : 0.f;
        s.JPa[i] = cont ? I.JPa[i] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < 3; i++) {
        s.dV[i] = cont ? I.dV[i] : 0.f;
        s.dP[i] = cont ? I.dP[i] : 0.f;
        s.avgA[i] = cont ? P.init.avgA[i] : 0.f;
        s.avgW[i] = cont ? P.init.avgW[i] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < 6; i++) s.b[i] = cont ? I.b[i] : P.bias[i];
    s.dT = cont ? I.dT : 0.f;
    for (int o = lane; o < 225; o += 64) L.C[o] = cont ? I.C[o] : 0.f;
    float nga[6];
#pragma unroll
    for (int i = 0; i < 6; i++) nga[i] = P.nga[i];
    const float walk = lane < 6 ? P.nga_walk[lane] : 0.f;
    wave_sync();

    const int n = P.n;
    const float *mp = meas + (size_t)7 * P.meas_off;
    float cur[7], nxt[7];
    if (n > 0) {
#pragma unroll
        for (int i = 0; i < 7; i++) nxt[i] = mp[i];
    }
#pragma unroll 1
    for (int step = 0; step < n; step++) {
#pragma unroll
        for (int i = 0; i < 7; i++) cur[i] = nxt[i];
        if (step + 1 < n) {  // the next step's measurement travels while this one is integrated
#pragma unroll
            for (int i = 0; i < 7; i++) nxt[i] = mp[7 * (step + 1) + i];
        }
        float M[M_COUNT * 9];
        chain_step(s, cur, M);
        if (lane == 0) {
#pragma unroll
            for (int i = 0; i < M_COUNT * 9; i++) L.M[i] = M[i];
            L.dt = cur[6];
        }
        wave_sync();
        const float t0 = row_times_C(L, lane);
        const float t1 = lane < 17 ? row_times_C(L, 64 + lane) : 0.f;
        L.T[lane] = t0;
        if (lane < 17) L.T[64 + lane] = t1;
        wave_sync();
        const float c0 = new_C(L, nga, lane);
        const float c1 = lane < 17 ? new_C(L, nga, 64 + lane) : 0.f;
        {
            const int i = lane / 9, j = lane - 9 * i;
            L.C[15 * i + j] = c0;
        }
        if (lane < 17) {
            const int o = 64 + lane, i = o / 9, j = o - 9 * i;
            L.C[15 * i + j] = c1;
        }
        if (lane < 6) L.C[16 * (9 + lane)] += walk;  // C.block<6, 6>(9, 9) += NgaWalk, a diagonal
        wave_sync();
    }

    osg_imu_preintegrated &O = out[b];
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < 9; i++) {
            O.pre.dR[i] = s.dR[i];
            O.pre.JRg[i] = s.JRg[i];
            O.pre.JVg[i] = s.JVg[i];
            O.pre.JVa[i] = s.JVa[i];
            O.pre.JPg[i] = s.JPg[i];
            O.pre.JPa[i] = s.JPa[i];
        }
#pragma unroll
        for (int i = 0; i < 3; i++) {
            O.pre.dV[i] = s.dV[i];
            O.pre.dP[i] = s.dP[i];
            O.avgA[i] = s.avgA[i];
            O.avgW[i] = s.avgW[i];
        }
#pragma unroll
        for (int i = 0; i < 6; i++) O.pre.b[i] = s.b[i];
        O.pre.dT = s.dT;
    }
    for (int o = lane; o < 225; o += 64) O.pre.C[o] = L.C[o];
}

}  // namespace

extern "C" {

int osg_imu_preintegrate_check(const osg_imu_problem *p) { return osgimu::check(p, nullptr); }

int osg_imu_select(const double *t, int32_t n_queue, double t_prev, double t_cur, double imu_per, int32_t *taken,
                   int32_t *n_popped)
{
    return osgimu::select(t, n_queue, t_prev, t_cur, imu_per, taken, n_popped);
}

int osg_imu_integrables(const float *a, const float *w, const double *t, int32_t m, double t_prev, double t_cur,
                        float *meas)
{
    return osgimu::integrables(a, w, t, m, t_prev, t_cur, meas);
}

void osg_imu_delta(const osg_imu_preintegrated *pre, const float *bias, float *dR, float *dV, float *dP)
{
    osgimu::delta(pre, bias, dR, dV, dP);
}

void osg_imu_predict_state(const osg_imu_preintegrated *pre, const float *bias, const float *Rwb1,
                           const float *twb1, const float *vwb1, float *Rwb2, float *twb2, float *vwb2)
{
    osgimu::predict_state(pre, bias, Rwb1, twb1, vwb1, Rwb2, twb2, vwb2);
}

int osg_imu_preintegrate_batch(osg_ctx *ctx, const osg_imu_problem *p, int32_t nb, osg_imu_preintegrated *out)
{
    if (!ctx) return OSG_E_INVALID;
    OSG_REQUIRE(ctx, nb >= 0 && (nb == 0 || (p && out)), "null argument");
    if (nb == 0) return 0;
    // a list that several problems point at is uploaded once
    std::unordered_map<const float *, std::pair<int, int>> seen;  // list -> (offset, steps)
    std::vector<ProbDev> hp(nb);
    std::vector<std::pair<const float *, int>> lists;
    size_t total = 0;
    for (int b = 0; b < nb; b++) {
        const char *why = "";
        if (osgimu::check(&p[b], &why) < 0) return osg_set_error(ctx, OSG_E_INVALID, "problem %d: %s", b, why);
        int off = 0;
        if (p[b].n > 0) {
            auto it = seen.find(p[b].meas);
            if (it != seen.end() && it->second.second >= p[b].n) {
                off = it->second.first;
            } else {
                off = (int)total;
                seen[p[b].meas] = {off, p[b].n};
                lists.push_back({p[b].meas, p[b].n});
                total += (size_t)p[b].n;
                OSG_REQUIRE(ctx, total <= (size_t)OSG_IMU_MAX_BATCH_STEPS, "too many steps in one batch");
            }
        }
        osgimu::pack(p[b], off, hp[b]);
    }
    osg_batch_io io(ctx);
    const osg_seg i_pr = io.in(sizeof(ProbDev), nb), i_m = io.in(7 * sizeof(float), total);
    const osg_seg o_res = io.out(sizeof(osg_imu_preintegrated), nb);
    io.in(1, 256), io.out(1, 256);  // slack behind both blocks
    OSG_RC(io.stage());
    io.put(i_pr, 0, hp.data(), nb);
    size_t at = 0;
    for (const auto &l : lists) {
        io.put(i_m, at, l.first, l.second);
        at += (size_t)l.second;
    }
    OSG_RC(io.upload());
    OSG_RC(io.start());
    hipLaunchKernelGGL(k_imu_preintegrate, dim3((nb + IMU_W - 1) / IMU_W), dim3(NT), 0, ctx->stream,
                       io.dev_in<const ProbDev>(i_pr), io.dev_in<const float>(i_m),
                       io.dev_out<osg_imu_preintegrated>(o_res), nb);
    OSG_HIP_CHECK(ctx, hipGetLastError());
    OSG_RC(io.finish(io.out_bytes));
    io.get(out, o_res, 0, nb);
    return 0;
}

int osg_imu_preintegrate(osg_ctx *ctx, const osg_imu_problem *p, osg_imu_preintegrated *out)
{
    return osg_imu_preintegrate_batch(ctx, p, 1, out);
}

}  // extern "C"
