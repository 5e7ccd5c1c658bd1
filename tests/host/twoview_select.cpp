// Stand-alone host program over csrc/twoview_select.h (the acceptance rules that end ReconstructF and
// ReconstructH), driven by tests/test_twoview.py.
//
// stdin:  lines "F n_inliers min_parallax min_triangulated g0 g1 g2 g3 p0 p1 p2 p3"
//         lines "H n_inliers min_parallax min_triangulated g0 .. g7 p0 .. p7"
// stdout: one line "ok cand" per input line.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "twoview_select.h"

int main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        char kind;
        if (!(in >> kind)) continue;
        const int k = kind == 'F' ? 4 : 8;
        int n_inliers, min_tri;
        float min_parallax;
        in >> n_inliers >> min_parallax >> min_tri;
        std::vector<int32_t> good(k);  // exactly k entries: a read past the end is a sanitizer error
        std::vector<float> par(k);
        for (auto &g : good) in >> g;
        for (auto &p : par) in >> p;
        const osg_tvr_choice c = kind == 'F' ? osg_tvr_choose_f(good.data(), par.data(), n_inliers, min_parallax, min_tri)
                                             : osg_tvr_choose_h(good.data(), par.data(), n_inliers, min_parallax, min_tri);
        std::printf("%d %d\n", c.ok, c.cand);
    }
    return 0;
}
