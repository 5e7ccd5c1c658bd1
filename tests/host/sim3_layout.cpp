// sim3_layout.cpp — prints sizeof / offsetof of osg_sim3_problem and osg_sim3_result as the C++
// compiler lays them out (test-only; tests/test_sim3opt.py compares with the ctypes mirrors).
#include <cstddef>
#include <cstdio>

#include "osg_ba.h"

#define F(T, f) std::printf(#T "." #f " %zu\n", offsetof(T, f))

int main()
{
    std::printf("osg_sim3_problem %zu\n", sizeof(osg_sim3_problem));
    F(osg_sim3_problem, q); F(osg_sim3_problem, t); F(osg_sim3_problem, s); F(osg_sim3_problem, fix_scale);
    F(osg_sim3_problem, th2); F(osg_sim3_problem, cam1); F(osg_sim3_problem, cam2); F(osg_sim3_problem, n_pairs);
    F(osg_sim3_problem, p1c); F(osg_sim3_problem, p2c); F(osg_sim3_problem, obs1); F(osg_sim3_problem, obs2);
    F(osg_sim3_problem, inv_sigma2_1); F(osg_sim3_problem, inv_sigma2_2); F(osg_sim3_problem, max_iterations);
    std::printf("osg_sim3_result %zu\n", sizeof(osg_sim3_result));
    F(osg_sim3_result, q); F(osg_sim3_result, t); F(osg_sim3_result, s); F(osg_sim3_result, n_inliers);
    F(osg_sim3_result, pair_state); F(osg_sim3_result, n_bad_first); F(osg_sim3_result, lm_iterations);
    F(osg_sim3_result, lm_trials); F(osg_sim3_result, chi2_final); F(osg_sim3_result, pair_chi2);
    F(osg_sim3_result, early_return);
    return 0;
}
