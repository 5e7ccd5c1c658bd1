// mock_twoview.h — what TwoViewReconstruction's adapter needs beside mock_orbslam3.h (test-only):
// cv::Point3f and hooks whose random source is scripted from the array file.
#ifndef MOCK_TWOVIEW_H
#define MOCK_TWOVIEW_H

#include <cstdint>
#include <vector>

#include "mock_orbslam3.h"

namespace cv {
struct Point3f {
    float x = 0, y = 0, z = 0;
};
}  // namespace cv

namespace mock {

struct TwoViewRandom {
    std::vector<int32_t> stream;
    size_t pos = 0;
    int bad = 0;        // draws outside [lo, hi] or past the end of the stream
    int seeded = 0;     // calls of seed_rand_once
    int seed = -1;      // the last seed asked for
    int draws_before_seed = 0;
};
inline TwoViewRandom &twoview_random()
{
    static TwoViewRandom r;
    return r;
}

struct TwoViewHooks {
    static void seed_rand_once(int seed)
    {
        TwoViewRandom &r = twoview_random();
        if (r.seeded == 0) r.draws_before_seed = (int)r.pos;
        r.seeded++;
        r.seed = seed;
    }
    static int random_int(int lo, int hi)
    {
        TwoViewRandom &r = twoview_random();
        const int v = r.pos < r.stream.size() ? r.stream[r.pos] : lo;
        if (r.pos >= r.stream.size() || v < lo || v > hi) r.bad++;
        r.pos++;
        return v < lo ? lo : v > hi ? hi : v;
    }
};

}  // namespace mock
#endif
