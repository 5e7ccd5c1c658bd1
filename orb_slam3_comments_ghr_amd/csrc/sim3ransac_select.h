// sim3ransac_select.h — the sequential part of Sim3Solver::iterate (ref:src/Sim3Solver.cc:146-291),
// replayed on the integer inlier counts of hypotheses that were evaluated in parallel.
//
// The reference evaluates one hypothesis per iteration and, after each count n,
//   if (n >= mnBestInliers) { best = this one; if (n > mRansacMinInliers) return converged; }
// so a later tie replaces an earlier best and the first count above min_inliers ends the call.
// mnIterations and mnBestInliers persist from call to call; bNoMore is set when a call ends without
// convergence at mnIterations >= mRansacMaxIts.  Hypothesis h is the one iteration h + 1 draws, so a
// call that starts at mnIterations = it looks at counts[it], counts[it + 1], ...
//
// Plain C++ for the host, the device (sim3ransac.hip's selection launch) and the adapter.
#pragma once
#include <stdint.h>

#include <cmath>

#include "osg_hd.h"

struct osg_s3r_window {
    int32_t converged;     // bConverge: counts[hyp] > min_inliers ended the window
    int32_t no_more;       // bNoMore
    int32_t hyp;           // the last hypothesis of this window that became the best (-1: none did)
    int32_t n_iterations;  // mnIterations after the window
    int32_t n_best;        // mnBestInliers after the window
};

// counts[0..n_hyp): inlier count per hypothesis in draw order (n_hyp = mRansacMaxIts).  One call of
// iterate(window, ...) entered with mnIterations = start_iteration and mnBestInliers = n_best.
OSG_HD inline osg_s3r_window osg_s3r_replay(const int32_t *counts, int32_t n_hyp, int32_t min_inliers,
                                                int32_t start_iteration, int32_t window, int32_t n_best)
{
    osg_s3r_window w;
    w.converged = 0;
    w.no_more = 0;
    w.hyp = -1;
    int32_t it = start_iteration, cur = 0;
    while (it < n_hyp && cur < window) {
        cur++;
        const int32_t n = counts[it];
        const int32_t h = it++;
        if (n >= n_best) {
            n_best = n;
            w.hyp = h;
            if (n > min_inliers) {
                w.converged = 1;
                break;
            }
        }
    }
    if (!w.converged && it >= n_hyp) w.no_more = 1;
    w.n_iterations = it;
    w.n_best = n_best;
    return w;
}

// Sim3Solver::SetRansacParameters' mRansacMaxIts (ref:src/Sim3Solver.cc:120-144): float epsilon, then
// ceil(log(1 - p) / log(1 - epsilon^3)) in double, clamped to [1, max_its]; 1 when min_inliers == n.  The
// reference converts the quotient to int before clamping, which is undefined past INT_MAX: a quotient
// that is not finite or not below max_its gives max_its here.  n < min_inliers never iterates: 1.
inline int32_t osg_s3r_iterations(double prob, int32_t min_inliers, int32_t n, int32_t max_its)
{
    if (max_its < 1) max_its = 1;
    if (n <= 0 || n < min_inliers) return 1;
    if (min_inliers == n) return 1;
    const float epsilon = (float)min_inliers / n;
    const double x = std::ceil(std::log(1 - prob) / std::log(1 - std::pow((double)epsilon, 3)));
    if (!(x < (double)max_its)) return max_its;
    return x < 1.0 ? 1 : (int32_t)x;
}
