// so3_common.h — the 3 x 3 helpers and the SO(3) functions of ref:src/G2oTypes.cc:906-944 shared by the
// inertial kernels (poseinertial.hip, the 4-DoF pose graph of essgraph.hip).  Device code, row-major.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

namespace osgso3 {

template <class T>
__device__ __forceinline__ void m3_mul(const T *A, const T *B, T *C)
{
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            T s = A[3 * i] * B[j];
            s += A[3 * i + 1] * B[3 + j];
            s += A[3 * i + 2] * B[6 + j];
            C[3 * i + j] = s;
        }
}
template <class T>
__device__ __forceinline__ void m3_t(const T *A, T *B)
{
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) B[3 * i + j] = A[3 * j + i];
}
template <class T>
__device__ __forceinline__ void m3_vec(const T *A, const T *x, T *y)
{
#pragma unroll
    for (int i = 0; i < 3; i++) {
        T s = A[3 * i] * x[0];
        s += A[3 * i + 1] * x[1];
        s += A[3 * i + 2] * x[2];
        y[i] = s;
    }
}
__device__ __forceinline__ void hat3(const double *w, double *W)
{
    W[0] = 0.0; W[1] = -w[2]; W[2] = w[1];
    W[3] = w[2]; W[4] = 0.0; W[5] = -w[0];
    W[6] = -w[1]; W[7] = w[0]; W[8] = 0.0;
}

// NormalizeRotation (ref:include/G2oTypes.h:67-72): U V' of the SVD of R, here as the polar factor
// R (R'R)^(-1/2) with R'R diagonalised by three-by-three cyclic Jacobi, in T's arithmetic
template <class T>
__device__ inline void normalize_rotation(T *R)
{
    T B[3][3], V[3][3];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            T s = R[i] * R[j];
            s += R[3 + i] * R[3 + j];
            s += R[6 + i] * R[6 + j];
            B[i][j] = s;
            V[i][j] = i == j ? T(1) : T(0);
        }
    const T tol = sizeof(T) == 8 ? T(1e-34) : T(1e-16);
#pragma unroll 1
    for (int sweep = 0; sweep < 12; sweep++) {
        const T off = B[0][1] * B[0][1] + B[0][2] * B[0][2] + B[1][2] * B[1][2];
        const T diag = B[0][0] * B[0][0] + B[1][1] * B[1][1] + B[2][2] * B[2][2];
        if (!(off > tol * diag)) break;
#pragma unroll
        for (int p = 0; p < 2; p++)
#pragma unroll
            for (int q = p + 1; q < 3; q++) {
                const T apq = B[p][q];
                if (apq == T(0)) continue;
                const T th = (B[q][q] - B[p][p]) / (T(2) * apq);
                const T tt = (th >= T(0) ? T(1) : T(-1)) / (fabs(th) + sqrt(th * th + T(1)));
                const T c = T(1) / sqrt(tt * tt + T(1)), s = tt * c;
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    const T akp = B[k][p], akq = B[k][q];
                    B[k][p] = c * akp - s * akq;
                    B[k][q] = s * akp + c * akq;
                }
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    const T apk = B[p][k], aqk = B[q][k];
                    B[p][k] = c * apk - s * aqk;
                    B[q][k] = s * apk + c * aqk;
                }
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    const T vkp = V[k][p], vkq = V[k][q];
                    V[k][p] = c * vkp - s * vkq;
                    V[k][q] = s * vkp + c * vkq;
                }
            }
    }
    T isq[3], M[9], O[9];
#pragma unroll
    for (int k = 0; k < 3; k++) isq[k] = T(1) / sqrt(B[k][k]);
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            T s = V[i][0] * isq[0] * V[j][0];
            s += V[i][1] * isq[1] * V[j][1];
            s += V[i][2] * isq[2] * V[j][2];
            M[3 * i + j] = s;
        }
    m3_mul(R, M, O);
#pragma unroll
    for (int i = 0; i < 9; i++) R[i] = O[i];
}

// ref:src/G2oTypes.cc:912-928
__device__ inline void exp_so3(const double *w, double *R)
{
    const double x = w[0], y = w[1], z = w[2];
    const double d2 = x * x + y * y + z * z;
    const double d = sqrt(d2);
    double W[9], W2[9];
    hat3(w, W);
    m3_mul(W, W, W2);
    if (d < 1e-5) {
#pragma unroll
        for (int i = 0; i < 9; i++) R[i] = ((i % 4 == 0) ? 1.0 : 0.0) + W[i] + 0.5 * W2[i];
    } else {
        const double sd = sin(d), cd = cos(d);
#pragma unroll
        for (int i = 0; i < 9; i++) R[i] = ((i % 4 == 0) ? 1.0 : 0.0) + W[i] * sd / d + W2[i] * (1.0 - cd) / d2;
    }
    normalize_rotation<double>(R);
}
// ref:src/G2oTypes.cc:930-944, the 0.5f and both early returns as written
__device__ inline void log_so3(const double *R, double *w)
{
    const double tr = R[0] + R[4] + R[8];
    w[0] = (R[7] - R[5]) / 2;
    w[1] = (R[2] - R[6]) / 2;
    w[2] = (R[3] - R[1]) / 2;
    const double costheta = (tr - 1.0) * 0.5f;
    if (costheta > 1 || costheta < -1) return;
    const double theta = acos(costheta);
    const double s = sin(theta);
    if (fabs(s) < 1e-5) return;
#pragma unroll
    for (int i = 0; i < 3; i++) w[i] = theta * w[i] / s;
}

}  // namespace osgso3
