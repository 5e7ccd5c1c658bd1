// small_linalg.h — the small dense routines of the optimiser and RANSAC kernels, each defined once: the 3 x 3
// products, the cyclic symmetric Jacobi, the unpivoted LDL^T solve.  Plain OSG_HD code over <cmath>, no HIP
// runtime header, so that the host entry points (imu_common.h, poseinertial_common.h) and the host test programs
// (tests/host/imu_host.cpp, tests/host/poseinertial_host.cpp) run the very functions the kernels run.  Every unit
// that includes it is compiled with -ffp-contract=off and without fast-math: a routine performs the same IEEE
// operations in the same order wherever it is called, in T's arithmetic (the std:: overloads keep T = float in
// float on the host as on the device); tests/test_ransac_bits_gpu.py and tests/test_optimizer_bits_gpu.py pin
// the bits.
//
// Not here, because their arithmetic differs: mlpnp.hip's in-line 6 x 6 LDL^T (no pivot test, another operand
// order), poseinertial.hip's LDS-parallel LDL^T, ba.hip's Cholesky, and the hand-rolled Jacobi sweeps of
// twoview.hip, mlpnp.hip and poseinertial.hip, which keep their loops and call jacobi_rotation.
#pragma once
#include <cmath>

#include "osg_hd.h"

namespace osgla {

// 3 x 3, row-major
template <class T>
OSG_HD_FORCEINLINE void m3_mul(const T *A, const T *B, T *C)
{
    OSG_UNROLL
    for (int i = 0; i < 3; i++)
        OSG_UNROLL
        for (int j = 0; j < 3; j++) {
            T s = A[3 * i] * B[j];
            s += A[3 * i + 1] * B[3 + j];
            s += A[3 * i + 2] * B[6 + j];
            C[3 * i + j] = s;
        }
}
template <class T>
OSG_HD_FORCEINLINE void m3_t(const T *A, T *B)
{
    OSG_UNROLL
    for (int i = 0; i < 3; i++)
        OSG_UNROLL
        for (int j = 0; j < 3; j++) B[3 * i + j] = A[3 * j + i];
}
template <class T>
OSG_HD_FORCEINLINE void m3_vec(const T *A, const T *x, T *y)
{
    OSG_UNROLL
    for (int i = 0; i < 3; i++) {
        T s = A[3 * i] * x[0];
        s += A[3 * i + 1] * x[1];
        s += A[3 * i + 2] * x[2];
        y[i] = s;
    }
}
template <class T>
OSG_HD_FORCEINLINE void hat3(const T *w, T *W)
{
    W[0] = T(0); W[1] = -w[2]; W[2] = w[1];
    W[3] = w[2]; W[4] = T(0); W[5] = -w[0];
    W[6] = -w[1]; W[7] = w[0]; W[8] = T(0);
}

// the Jacobi rotation that annihilates apq of the pair (app, aqq, apq), apq != 0: c = cos, s = sin
template <class T>
OSG_HD_FORCEINLINE void jacobi_rotation(T app, T aqq, T apq, T &c, T &s)
{
    using std::fabs;
    using std::sqrt;
    const T th = (aqq - app) / (T(2) * apq);
    const T tt = (th >= T(0) ? T(1) : T(-1)) / (fabs(th) + sqrt(th * th + T(1)));
    c = T(1) / sqrt(tt * tt + T(1));
    s = tt * c;
}

// cyclic Jacobi on the symmetric N x N matrix A (registers, fully unrolled): A -> diagonal, V -> eigenvectors
// in columns.  At most max_sweeps sweeps, until the squared off-diagonal part is within tol of the squared
// diagonal; a zero matrix or one with a NaN stops at once.  The sweep limit and tol are the caller's: each
// module's margins were measured with its own.
template <class T, int N>
OSG_HD inline void jacobi_sym(T (&A)[N][N], T (&V)[N][N], int max_sweeps, T tol)
{
    OSG_UNROLL
    for (int i = 0; i < N; i++)
        OSG_UNROLL
        for (int j = 0; j < N; j++) V[i][j] = i == j ? T(1) : T(0);
    OSG_UNROLL1
    for (int sweep = 0; sweep < max_sweeps; sweep++) {
        T off = 0, diag = 0;
        OSG_UNROLL
        for (int i = 0; i < N; i++) {
            diag += A[i][i] * A[i][i];
            OSG_UNROLL
            for (int j = i + 1; j < N; j++) off += A[i][j] * A[i][j];
        }
        if (!(off > tol * diag)) break;
        OSG_UNROLL
        for (int p = 0; p < N - 1; p++)
            OSG_UNROLL
            for (int q = p + 1; q < N; q++) {
                const T apq = A[p][q];
                if (apq == T(0)) continue;
                T c, s;
                jacobi_rotation(A[p][p], A[q][q], apq, c, s);
                OSG_UNROLL
                for (int k = 0; k < N; k++) {
                    const T akp = A[k][p], akq = A[k][q];
                    A[k][p] = c * akp - s * akq;
                    A[k][q] = s * akp + c * akq;
                }
                OSG_UNROLL
                for (int k = 0; k < N; k++) {
                    const T apk = A[p][k], aqk = A[q][k];
                    A[p][k] = c * apk - s * aqk;
                    A[q][k] = s * apk + c * aqk;
                }
                OSG_UNROLL
                for (int k = 0; k < N; k++) {
                    const T vkp = V[k][p], vkq = V[k][q];
                    V[k][p] = c * vkp - s * vkq;
                    V[k][q] = s * vkp + c * vkq;
                }
            }
    }
}

// unpivoted LDL^T solve of the damped N x N system A x = b (A is overwritten); false when a pivot is not
// positive, the oracle's ldlt_solve (require_positive).  Eigen's LDLT, which the reference's LinearSolverDense
// uses, pivots on the largest remaining diagonal entry; the solutions agree to rounding.
template <int N>
OSG_HD inline bool ldlt_solve(double A[N][N], const double *b, double *x)
{
    OSG_UNROLL
    for (int j = 0; j < N; j++) {
        double d = A[j][j];
        OSG_UNROLL
        for (int k = 0; k < j; k++) d -= A[j][k] * A[j][k] * A[k][k];
        if (!(d > 0.0)) return false;
        A[j][j] = d;
        OSG_UNROLL
        for (int i = j + 1; i < N; i++) {
            double s = A[i][j];
            OSG_UNROLL
            for (int k = 0; k < j; k++) s -= A[i][k] * A[j][k] * A[k][k];
            A[i][j] = s / d;
        }
    }
    double y[N];
    OSG_UNROLL
    for (int i = 0; i < N; i++) {
        double s = b[i];
        OSG_UNROLL
        for (int k = 0; k < i; k++) s -= A[i][k] * y[k];
        y[i] = s;
    }
    OSG_UNROLL
    for (int i = 0; i < N; i++) y[i] /= A[i][i];
    OSG_UNROLL
    for (int i = N - 1; i >= 0; i--) {
        double s = y[i];
        OSG_UNROLL
        for (int k = i + 1; k < N; k++) s -= A[k][i] * y[k];
        y[i] = s;
    }
    OSG_UNROLL
    for (int i = 0; i < N; i++) x[i] = y[i];
    return true;
}

}  // namespace osgla
