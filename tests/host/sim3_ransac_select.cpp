// Stand-alone host program over csrc/sim3ransac_select.h (the replay of Sim3Solver's sequential rule and
// osg_sim3_ransac_iterations' arithmetic, osg_s3r_iterations), driven by tests/test_sim3solver.py.
//
// stdin:  lines "W n_hyp min_inliers window c0 c1 ..."  -> the solver is driven from mnIterations = 0,
//         mnBestInliers = 0 with iterate(window) calls until converged or no-more; one output line per call:
//         "converged no_more hyp n_iterations n_best"; then "end".
//         lines "I prob min_inliers n max_its"          -> one line with mRansacMaxIts.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "sim3ransac_select.h"

int main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        char kind;
        if (!(in >> kind)) continue;
        if (kind == 'I') {
            double prob;
            int mi, n, mx;
            in >> prob >> mi >> n >> mx;
            std::printf("%d\n", osg_s3r_iterations(prob, mi, n, mx));
            continue;
        }
        int n_hyp, min_inliers, window;
        in >> n_hyp >> min_inliers >> window;
        std::vector<int32_t> counts(n_hyp);  // exactly n_hyp entries: a read past the end is a sanitizer error
        for (auto &c : counts) in >> c;
        int32_t it = 0, best = 0;
        for (int guard = 0; guard <= n_hyp + 1; guard++) {
            const osg_s3r_window w = osg_s3r_replay(counts.data(), n_hyp, min_inliers, it, window, best);
            std::printf("%d %d %d %d %d\n", w.converged, w.no_more, w.hyp, w.n_iterations, w.n_best);
            it = w.n_iterations;
            best = w.n_best;
            if (w.converged || w.no_more) break;
        }
        std::printf("end\n");
    }
    return 0;
}
