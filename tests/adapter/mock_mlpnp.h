// mock_mlpnp.h — what the MLPnPsolver adapter needs beyond mock_orbslam3.h (test-only): the camera models'
// float unproject (ref:src/CameraModels/Pinhole.cpp:97-101, KannalaBrandt8.cpp:180-217) on the mock Camera.
#pragma once
#include <cmath>

#include "mock_orbslam3.h"

inline void mock_unproject(const Camera &c, float u, float v, float ray[3])
{
    const float *k = c.params.data();  // fx fy cx cy k0 k1 k2 k3
    const float mx = (u - k[2]) / k[0], my = (v - k[3]) / k[1];
    float gain = 1.f;
    if (c.type == OSG_CAM_KB8) {
        const float half_pi = (float)M_PI / 2.f;
        const float rd = fminf(fmaxf(-half_pi, sqrtf(mx * mx + my * my)), half_pi);  // the distorted angle
        if (rd > 1e-8) {
            float th = rd;  // Newton on th (1 + k0 th^2 + k1 th^4 + k2 th^6 + k3 th^8) = rd, at most 10 steps, float
            for (int step = 0; step < 10; step++) {
                const float p2 = th * th, p4 = p2 * p2, p6 = p4 * p2, p8 = p4 * p4;
                const float a = k[4] * p2, b = k[5] * p4, cc = k[6] * p6, d = k[7] * p8;
                const float delta = (th * (1 + a + b + cc + d) - rd) / (1 + 3 * a + 5 * b + 7 * cc + 9 * d);
                th = th - delta;
                if (fabsf(delta) < 1e-6f) break;
            }
            gain = std::tan(th) / rd;
        }
    }
    ray[0] = mx * gain, ray[1] = my * gain, ray[2] = 1.f;
}
