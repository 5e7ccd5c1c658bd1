// sim3_common.h — g2o::Sim3 as OptimizeSim3 uses it (ref:Thirdparty/g2o/g2o/types/sim3.h:41-292):
// the exponential Sim3(Vector7d) with its four branches on |sigma| < 1e-5 and theta < 1e-5,
// operator* (the quaternion is NOT renormalised), inverse() and map().  The rotation is an Eigen
// Quaterniond there: products are Hamilton products, r * x is Eigen's _transformVector, and
// Quaterniond(Matrix3d) is the trace method without a final normalisation.
//
// Plain __host__ __device__ code over <cmath> and exact_math.h only (no HIP runtime header), so a
// stand-alone host program can call the same functions the kernel runs (tests/test_sim3opt.py builds
// one).  That is why the three quaternion helpers are spelled out here instead of taken from
// ba_common.h, which pulls in the HIP runtime.
#pragma once
#include <cmath>

#include "exact_math.h"

namespace osgs3 {

struct Sim3 {
    double q[4];  // x y z w
    double t[3];
    double s;
};

OSG_HD inline void q_mul(const double *a, const double *b, double *o)
{
    double r[4];
    r[3] = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
    r[0] = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
    r[1] = a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2];
    r[2] = a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0];
    o[0] = r[0]; o[1] = r[1]; o[2] = r[2]; o[3] = r[3];
}
// Eigen QuaternionBase::_transformVector
OSG_HD inline void q_rot(const double *q, const double *v, double *o)
{
    double uv0 = q[1] * v[2] - q[2] * v[1], uv1 = q[2] * v[0] - q[0] * v[2], uv2 = q[0] * v[1] - q[1] * v[0];
    uv0 += uv0; uv1 += uv1; uv2 += uv2;
    const double c0 = q[1] * uv2 - q[2] * uv1, c1 = q[2] * uv0 - q[0] * uv2, c2 = q[0] * uv1 - q[1] * uv0;
    const double r0 = v[0] + q[3] * uv0 + c0, r1 = v[1] + q[3] * uv1 + c1, r2 = v[2] + q[3] * uv2 + c2;
    o[0] = r0; o[1] = r1; o[2] = r2;
}
// Eigen quaternionbase_assign_impl<Matrix3>; the largest-diagonal branch takes its indices as
// template constants (a dynamic subscript would send the matrix to scratch on the device)
template <int I>
OSG_HD inline void q_from_R_branch(const double m[3][3], double *q)
{
    constexpr int J = (I + 1) % 3, K = (J + 1) % 3;
    double s = sqrt(m[I][I] - m[J][J] - m[K][K] + 1.0);
    q[I] = 0.5 * s;
    s = 0.5 / s;
    q[3] = (m[K][J] - m[J][K]) * s;
    q[J] = (m[J][I] + m[I][J]) * s;
    q[K] = (m[K][I] + m[I][K]) * s;
}
OSG_HD inline void q_from_R(const double m[3][3], double *q)
{
    const double tr = m[0][0] + m[1][1] + m[2][2];
    if (tr > 0) {
        double s = sqrt(tr + 1.0);
        q[3] = 0.5 * s;
        s = 0.5 / s;
        q[0] = (m[2][1] - m[1][2]) * s;
        q[1] = (m[0][2] - m[2][0]) * s;
        q[2] = (m[1][0] - m[0][1]) * s;
    } else if (m[2][2] > (m[1][1] > m[0][0] ? m[1][1] : m[0][0])) {
        q_from_R_branch<2>(m, q);
    } else if (m[1][1] > m[0][0]) {
        q_from_R_branch<1>(m, q);
    } else {
        q_from_R_branch<0>(m, q);
    }
}

// Sim3(const Vector7d &update): update = (omega, upsilon, sigma)
OSG_HD inline Sim3 sim3_exp(const double *u)
{
    const double w0 = u[0], w1 = u[1], w2 = u[2];
    const double sigma = u[6];
    const double theta = sqrt(w0 * w0 + w1 * w1 + w2 * w2);
    const double Om[3][3] = {{0, -w2, w1}, {w2, 0, -w0}, {-w1, w0, 0}};
    double Om2[3][3];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) Om2[i][j] = Om[i][0] * Om[0][j] + Om[i][1] * Om[1][j] + Om[i][2] * Om[2][j];
    Sim3 O;
    O.s = exp(sigma);
    const double eps = 0.00001;
    double A, B, C;
    double ra = 1.0, rb = 1.0;  // R = I + ra Omega + rb Omega^2
    double st = 0.0, ct = 1.0;
    if (!(theta < eps)) {  // sin(theta), cos(theta) of the two large-angle branches (exact_math.h)
        osgx::sincos_ref<false>(theta, st, ct);
        ra = st / theta;
        rb = (1 - ct) / (theta * theta);
    }
    if (fabs(sigma) < eps) {
        C = 1;
        if (theta < eps) {
            A = 1. / 2.;
            B = 1. / 6.;
        } else {
            const double theta2 = theta * theta;
            A = (1 - ct) / (theta2);
            B = (theta - st) / (theta2 * theta);
        }
    } else {
        C = (O.s - 1) / sigma;
        if (theta < eps) {
            const double sigma2 = sigma * sigma;
            A = ((sigma - 1) * O.s + 1) / sigma2;
            B = ((0.5 * sigma2 - sigma + 1) * O.s) / (sigma2 * sigma);
        } else {
            const double a = O.s * st;
            const double b = O.s * ct;
            const double theta2 = theta * theta;
            const double sigma2 = sigma * sigma;
            const double c = theta2 + sigma2;
            A = (a * sigma + (1 - b) * theta) / (theta * c);
            B = (C - ((b - 1) * sigma + a * theta) / (c)) * 1. / (theta2);
        }
    }
    double R[3][3], W[3][3];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            const double I = i == j ? 1.0 : 0.0;
            R[i][j] = I + ra * Om[i][j] + rb * Om2[i][j];
            W[i][j] = A * Om[i][j] + B * Om2[i][j] + C * I;
        }
    q_from_R(R, O.q);
    for (int i = 0; i < 3; i++) O.t[i] = W[i][0] * u[3] + W[i][1] * u[4] + W[i][2] * u[5];
    return O;
}

// ret.r = r * other.r; ret.t = s * (r * other.t) + t; ret.s = s * other.s
OSG_HD inline Sim3 sim3_mul(const Sim3 &a, const Sim3 &b)
{
    Sim3 o;
    double rt[3];
    q_rot(a.q, b.t, rt);
    for (int i = 0; i < 3; i++) o.t[i] = a.s * rt[i] + a.t[i];
    q_mul(a.q, b.q, o.q);
    o.s = a.s * b.s;
    return o;
}

// Sim3(r.conjugate(), r.conjugate() * ((-1. / s) * t), 1. / s)
OSG_HD inline Sim3 sim3_inverse(const Sim3 &a)
{
    Sim3 o;
    o.q[0] = -a.q[0]; o.q[1] = -a.q[1]; o.q[2] = -a.q[2]; o.q[3] = a.q[3];
    const double k = -1. / a.s;
    const double v[3] = {k * a.t[0], k * a.t[1], k * a.t[2]};
    q_rot(o.q, v, o.t);
    o.s = 1. / a.s;
    return o;
}

// s * (r * xyz) + t
OSG_HD inline void sim3_map(const Sim3 &a, const double *x, double *o)
{
    double r[3];
    q_rot(a.q, x, r);
    for (int i = 0; i < 3; i++) o[i] = a.s * r[i] + a.t[i];
}

// VertexSim3Expmap::oplusImpl (ref:include/OptimizableTypes.h:176-185): update[6] = 0 under
// _fix_scale, then Sim3(update) * estimate
OSG_HD inline Sim3 sim3_oplus(const Sim3 &est, const double *upd, bool fix_scale)
{
    double u[7];
    for (int i = 0; i < 7; i++) u[i] = upd[i];
    if (fix_scale) u[6] = 0;
    return sim3_mul(sim3_exp(u), est);
}

// 3 x 3 PartialPivLU solve (Eigen's W.lu().solve(t)): the first largest |entry| of the column is the
// pivot, the multipliers are quotients.  Rows are exchanged by value (a dynamic row index would send the
// matrix to scratch on the device).
OSG_HD inline void lu3_solve(const double W[3][3], const double *t, double *x)
{
    double a0[4] = {W[0][0], W[0][1], W[0][2], t[0]};
    double a1[4] = {W[1][0], W[1][1], W[1][2], t[1]};
    double a2[4] = {W[2][0], W[2][1], W[2][2], t[2]};
    auto swap_rows = [](double *p, double *q) {
        for (int i = 0; i < 4; i++) {
            const double v = p[i];
            p[i] = q[i];
            q[i] = v;
        }
    };
    if (fabs(a1[0]) > fabs(a0[0]) && !(fabs(a2[0]) > fabs(a1[0]))) swap_rows(a0, a1);
    else if (fabs(a2[0]) > fabs(a0[0])) swap_rows(a0, a2);
    const double l1 = a1[0] / a0[0], l2 = a2[0] / a0[0];
    for (int i = 1; i < 4; i++) {
        a1[i] -= l1 * a0[i];
        a2[i] -= l2 * a0[i];
    }
    if (fabs(a2[1]) > fabs(a1[1])) swap_rows(a1, a2);
    const double l21 = a2[1] / a1[1];
    for (int i = 2; i < 4; i++) a2[i] -= l21 * a1[i];
    const double x2 = a2[3] / a2[2];
    const double x1 = (a1[3] - a1[2] * x2) / a1[1];
    const double x0 = (a0[3] - a0[1] * x1 - a0[2] * x2) / a0[0];
    x[0] = x0; x[1] = x1; x[2] = x2;
}

// Sim3::log (ref:Thirdparty/g2o/g2o/types/sim3.h:148-230): out = (omega, upsilon, sigma), the four
// branches on |sigma| < 1e-5 and d > 1 - 1e-5.  R is Eigen's toRotationMatrix of the quaternion as it
// is stored (not normalised), omega comes from deltaR(R).
OSG_HD inline void sim3_log(const Sim3 &S, double *out)
{
    const double sigma = log(S.s);
    const double tx = 2 * S.q[0], ty = 2 * S.q[1], tz = 2 * S.q[2];
    const double twx = tx * S.q[3], twy = ty * S.q[3], twz = tz * S.q[3];
    const double txx = tx * S.q[0], txy = ty * S.q[0], txz = tz * S.q[0];
    const double tyy = ty * S.q[1], tyz = tz * S.q[1], tzz = tz * S.q[2];
    const double R00 = 1 - (tyy + tzz), R01 = txy - twz, R02 = txz + twy;
    const double R10 = txy + twz, R11 = 1 - (txx + tzz), R12 = tyz - twx;
    const double R20 = txz - twy, R21 = tyz + twx, R22 = 1 - (txx + tyy);
    const double d = 0.5 * (R00 + R11 + R22 - 1);
    const double dR0 = R21 - R12, dR1 = R02 - R20, dR2 = R10 - R01;  // deltaR
    const double eps = 0.00001;
    double A, B, C, k;
    if (fabs(sigma) < eps) {
        C = 1;
        if (d > 1 - eps) {
            k = 0.5;
            A = 1. / 2.;
            B = 1. / 6.;
        } else {
            const double theta = acos(d);
            const double theta2 = theta * theta;
            double st, ct;
            osgx::sincos_ref<false>(theta, st, ct);
            k = theta / (2 * sqrt(1 - d * d));
            A = (1 - ct) / (theta2);
            B = (theta - st) / (theta2 * theta);
        }
    } else {
        C = (S.s - 1) / sigma;
        if (d > 1 - eps) {
            const double sigma2 = sigma * sigma;
            k = 0.5;
            A = ((sigma - 1) * S.s + 1) / (sigma2);
            B = ((0.5 * sigma2 - sigma + 1) * S.s) / (sigma2 * sigma);
        } else {
            const double theta = acos(d);
            k = theta / (2 * sqrt(1 - d * d));
            const double theta2 = theta * theta;
            double st, ct;
            osgx::sincos_ref<false>(theta, st, ct);
            const double a = S.s * st;
            const double b = S.s * ct;
            const double c = theta2 + sigma * sigma;
            A = (a * sigma + (1 - b) * theta) / (theta * c);
            B = (C - ((b - 1) * sigma + a * theta) / (c)) * 1. / (theta2);
        }
    }
    const double w0 = k * dR0, w1 = k * dR1, w2 = k * dR2;
    const double Om[3][3] = {{0, -w2, w1}, {w2, 0, -w0}, {-w1, w0, 0}};
    double W[3][3];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++)
            W[i][j] = A * Om[i][j] + B * (Om[i][0] * Om[0][j] + Om[i][1] * Om[1][j] + Om[i][2] * Om[2][j]) +
                      (i == j ? C : 0.0);
    out[0] = w0; out[1] = w1; out[2] = w2;
    lu3_solve(W, S.t, out + 3);
    out[6] = sigma;
}

}  // namespace osgs3
