// ransac_common.h — device helpers and the sample-set check shared by the RANSAC solvers (sim3ransac.hip,
// mlpnp.hip, twoview.hip).  Every unit that includes it is compiled with -ffp-contract=off and without
// fast-math: a helper performs the same IEEE operations in the same order wherever it is called, so the bits
// of a result do not depend on which unit called it (tests/test_ransac_bits_gpu.py pins them).  The Jacobi
// routines they share with the optimisers are small_linalg.h's.
#pragma once
#include "glibc_math.h"
#include "osg_internal.h"
#include "small_linalg.h"

using osgla::jacobi_rotation;
using osgla::jacobi_sym;

// GeometricCamera::project in float, of an Eigen::Vector3f (ref:src/CameraModels/Pinhole.cpp:64-71,
// ref:src/CameraModels/KannalaBrandt8.cpp:87-104) and of a cv::Point3f (ref:src/CameraModels/Pinhole.cpp:39-43,
// ref:src/CameraModels/KannalaBrandt8.cpp:40-55): the same arithmetic
__device__ __forceinline__ void project_f(const osg_camera &c, float x, float y, float z, float &u, float &v)
{
    if (c.type == OSG_CAM_KB8) {
        const float x2_plus_y2 = x * x + y * y;
        const float theta = osgm::atan2f_fd(sqrtf(x2_plus_y2), z);
        const float psi = osgm::atan2f_fd(y, x);
        const float theta2 = theta * theta;
        const float theta3 = theta * theta2;
        const float theta5 = theta3 * theta2;
        const float theta7 = theta5 * theta2;
        const float theta9 = theta7 * theta2;
        const float r = theta + c.p[4] * theta3 + c.p[5] * theta5 + c.p[6] * theta7 + c.p[7] * theta9;
        u = c.p[0] * r * cosf(psi) + c.p[2];
        v = c.p[1] * r * sinf(psi) + c.p[3];
    } else {
        u = c.p[0] * x / z + c.p[2];
        v = c.p[1] * y / z + c.p[3];
    }
}

// one wave expands a hypothesis's __ballot mask words to n bytes, one per match (a null mask: zeros); returns
// the number of set bytes this lane wrote.  dst must not overlap the mask: with that and the unroll the loads of
// four words are in flight at once, which a caller that expands several masks in turn (k_tvr_select) relies on.
__device__ __forceinline__ int expand_mask(const unsigned long long *__restrict__ mask, int n, uint8_t *__restrict__ dst,
                                           int lane)
{
    if (!mask) {
        for (int i = lane; i < n; i += 64) dst[i] = 0;
        return 0;
    }
    int set = 0;
#pragma unroll 4
    for (int i = lane; i < n; i += 64) {
        const uint8_t b = (uint8_t)((mask[i >> 6] >> (i & 63)) & 1ull);
        dst[i] = b;
        set += b;
    }
    return set;
}

// the n_hyp sets of k indices each: 0 when every set holds k distinct indices into [0, n); else *h_bad is the
// first offending set and the value 1 for an index outside, 2 for a repeated index, whichever comes first in
// the set.  Inlined, so that k is a constant of the loops at each call: a batch checks thousands of sets per call.
__attribute__((always_inline)) inline int check_sets(const int32_t *sets, int k, int n_hyp, int n, int *h_bad)
{
    for (int h = 0; h < n_hyp; h++) {
        const int32_t *s = sets + (size_t)k * h;
        for (int i = 0; i < k; i++) {
            if (s[i] < 0 || s[i] >= n) return *h_bad = h, 1;
            for (int j = 0; j < i; j++)
                if (s[i] == s[j]) return *h_bad = h, 2;
        }
    }
    return 0;
}
