// Stand-alone host program over csrc/mlpnp_select.h (the replay of MLPnPsolver's sequential rule and
// SetRansacParameters' arithmetic), driven by tests/test_mlpnp.py.
//
// stdin:  lines "W max_its min_inliers window n_calls c0 c1 ..."  -> the solver is driven from mnIterations = 0,
//         mnBestInliers = 0 with n_calls iterate(window) calls, the state carried from call to call; one output
//         line per call: "converged no_more hyp n_iterations n_best"; then "end".  The counts are exactly those
//         the calls consume when none returns early.
//         lines "P prob min_inliers max_its min_set epsilon n"      -> one line "min_inliers max_its".
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "mlpnp_select.h"

int main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        char kind;
        if (!(in >> kind)) continue;
        if (kind == 'P') {
            double prob;
            float eps;
            int mi, mx, ms, n;
            in >> prob >> mi >> mx >> ms >> eps >> n;
            int32_t a = 0, b = 0;
            osg_mlpnp_parameters(prob, mi, mx, ms, eps, n, &a, &b);
            std::printf("%d %d\n", a, b);
            continue;
        }
        int max_its, min_inliers, window, n_calls;
        in >> max_its >> min_inliers >> window >> n_calls;
        std::vector<int32_t> counts;  // exactly what was given: a read past the end is a sanitizer error
        for (int32_t c; in >> c;) counts.push_back(c);
        int32_t it = 0, best = 0, best_hyp = -1;
        for (int call = 0; call < n_calls; call++) {
            const int32_t len = osg_mlpnp_window_length(it, max_its, window);
            if (it + len > (int32_t)counts.size()) {
                std::printf("short\n");
                break;
            }
            const osg_mlpnp_window w = osg_mlpnp_replay(counts.data(), min_inliers, it, len, best, best_hyp);
            std::printf("%d %d %d %d %d\n", w.converged, !w.converged, w.hyp, w.n_iterations, w.n_best);
            it = w.n_iterations;
            best = w.n_best;
            best_hyp = w.best_hyp;
        }
        std::printf("end\n");
    }
    return 0;
}
