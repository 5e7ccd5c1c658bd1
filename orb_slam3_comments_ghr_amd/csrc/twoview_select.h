// twoview_select.h — the two acceptance rules that end TwoViewReconstruction::ReconstructF
// (ref:src/TwoViewReconstruction.cc:604-673) and ReconstructH (:898-940), on the integer nGood counts and
// the parallaxes of motion hypotheses that were checked in parallel.
//
//   F: nMinGood = max(int(0.9 N), minTriangulated); reject when maxGood < nMinGood or when more than one
//      of the four counts exceeds 0.7 maxGood (double arithmetic on the right); otherwise the first
//      candidate in order whose count equals maxGood, accepted only if its parallax > minParallax.
//   H: best / second best tracked in order with strict `>` (a later tie becomes the second best);
//      accepted when secondBest < 0.75 best, parallax >= minParallax, best > minTriangulated and
//      best > 0.9 N.
// N is the number of inliers of the chosen model.
//
// Plain C++ for the host, the device (twoview.hip's last launch) and the adapter tests.
#pragma once
#include <stdint.h>

#include "osg_hd.h"

struct osg_tvr_choice {
    int32_t ok;    // the reference's return value
    int32_t cand;  // the candidate the rule looked at last (F: first with maxGood; H: bestSolutionIdx; -1: none)
};

OSG_HD inline osg_tvr_choice osg_tvr_choose_f(const int32_t n_good[4], const float parallax[4], int32_t n_inliers,
                                                  float min_parallax, int32_t min_triangulated)
{
    osg_tvr_choice c;
    c.ok = 0;
    c.cand = -1;
    int32_t max_good = n_good[0];
    for (int i = 1; i < 4; i++)
        if (n_good[i] > max_good) max_good = n_good[i];
    const int32_t n09 = (int32_t)(0.9 * n_inliers);
    const int32_t n_min_good = n09 > min_triangulated ? n09 : min_triangulated;
    int nsimilar = 0;
    for (int i = 0; i < 4; i++)
        if (n_good[i] > 0.7 * max_good) nsimilar++;
    if (max_good < n_min_good || nsimilar > 1) return c;
    for (int i = 0; i < 4; i++)
        if (n_good[i] == max_good) {
            c.cand = i;
            c.ok = parallax[i] > min_parallax ? 1 : 0;
            break;
        }
    return c;
}

OSG_HD inline osg_tvr_choice osg_tvr_choose_h(const int32_t n_good[8], const float parallax[8], int32_t n_inliers,
                                                  float min_parallax, int32_t min_triangulated)
{
    osg_tvr_choice c;
    c.ok = 0;
    c.cand = -1;
    int32_t best = 0, second = 0;
    float best_parallax = -1.f;
    for (int i = 0; i < 8; i++) {
        if (n_good[i] > best) {
            second = best;
            best = n_good[i];
            c.cand = i;
            best_parallax = parallax[i];
        } else if (n_good[i] > second) {
            second = n_good[i];
        }
    }
    if (second < 0.75 * best && best_parallax >= min_parallax && best > min_triangulated && best > 0.9 * n_inliers)
        c.ok = 1;
    return c;
}
