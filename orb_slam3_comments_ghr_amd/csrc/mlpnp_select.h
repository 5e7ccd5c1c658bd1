// mlpnp_select.h — the sequential part of MLPnPsolver::iterate (ref:src/MLPnPsolver.cpp:145-301), replayed
// on the integer inlier counts of hypotheses that were evaluated in parallel.
//
// The reference evaluates one hypothesis per iteration and, after each count n with n >= mRansacMinInliers,
//   if (n > mnBestInliers) best = this one;          // strict: the first to attain the maximum stays
//   if (Refine()) return this one;                   // Refine re-tests the current pose: n > mRansacMinInliers
// Its loop runs while (mnIterations < mRansacMaxIts || nCurrentIterations < nIterations), so a call entered
// at mnIterations = it consumes max(mRansacMaxIts - it, nIterations) hypotheses unless it returns early,
// and always leaves mnIterations >= mRansacMaxIts behind: a call that does not return early sets bNoMore
// and returns the best when mnBestInliers >= mRansacMinInliers.  Hypothesis h is the one iteration h + 1
// draws, so a call that starts at mnIterations = it looks at counts[it], counts[it + 1], ...
//
// Plain C++ for the host, the device (mlpnp.hip's selection launch) and the adapter.
#pragma once
#include <stdint.h>

#include <cmath>

#include "osg_hd.h"

struct osg_mlpnp_window {
    int32_t converged;     // counts[hyp] > min_inliers ended the window (bNoMore stays false)
    int32_t hyp;           // the returned hypothesis: that one, else the best when n_best >= min_inliers, else -1
    int32_t n_iterations;  // mnIterations after the window
    int32_t n_best;        // mnBestInliers after the window
    int32_t best_hyp;      // the hypothesis that holds n_best (-1: none yet)
};

// the iterations one iterate(n_iterations) consumes when entered at mnIterations = it and not ended early
OSG_HD inline int32_t osg_mlpnp_window_length(int32_t it, int32_t max_its, int32_t n_iterations)
{
    const int32_t a = max_its - it;
    return a > n_iterations ? a : n_iterations;
}

// counts[first .. first + len): inlier counts in draw order; n_best / best_hyp: mnBestInliers and its slot
// as the previous call left them (0, -1 on a fresh solver).
OSG_HD inline osg_mlpnp_window osg_mlpnp_replay(const int32_t *counts, int32_t min_inliers, int32_t first,
                                                      int32_t len, int32_t n_best, int32_t best_hyp)
{
    osg_mlpnp_window w;
    w.converged = 0;
    int32_t h = first;
    for (; h < first + len; h++) {
        const int32_t n = counts[h];
        if (n >= min_inliers) {
            if (n > n_best) {
                n_best = n;
                best_hyp = h;
            }
            if (n > min_inliers) {
                w.converged = 1;
                break;
            }
        }
    }
    w.hyp = w.converged ? h : (n_best >= min_inliers ? best_hyp : -1);
    w.n_iterations = w.converged ? h + 1 : first + len;
    w.n_best = n_best;
    w.best_hyp = best_hyp;
    return w;
}

// MLPnPsolver::SetRansacParameters (ref:src/MLPnPsolver.cpp:314-354) -> mRansacMinInliers, mRansacMaxIts.
// The reference converts the quotient to int before clamping, which is undefined past INT_MAX: a quotient
// that is not finite or not below max_its gives max_its.
inline void osg_mlpnp_parameters(double prob, int32_t min_inliers, int32_t max_its, int32_t min_set, float epsilon,
                                 int32_t n, int32_t *min_inliers_out, int32_t *max_its_out)
{
    const float prod = (float)n * epsilon;
    int32_t n_min = (prod == prod && std::fabs(prod) < 2.0e9f) ? (int32_t)prod : 0;
    if (n_min < min_inliers) n_min = min_inliers;
    if (n_min < min_set) n_min = min_set;
    if (n > 0 && epsilon < (float)n_min / n) epsilon = (float)n_min / n;
    if (max_its < 1) max_its = 1;
    int32_t its = max_its;
    if (n_min == n) {
        its = 1;
    } else {
        const double x = std::ceil(std::log(1 - prob) / std::log(1 - std::pow((double)epsilon, 3)));
        if (x < (double)max_its) its = x < 1.0 ? 1 : (int32_t)x;
    }
    *min_inliers_out = n_min;
    *max_its_out = its;
}
