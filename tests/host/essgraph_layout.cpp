// essgraph_layout.cpp — prints the size and the field offsets of osg_essgraph_problem / osg_essgraph_result
// as the C++ compiler lays them out (test-only; tests/test_essgraph.py compares them with the ctypes mirrors).
#include <cstddef>
#include <cstdio>

#include "osg_ba.h"

#define F(st, f) std::printf(#st "." #f " %zu\n", offsetof(st, f))

int main()
{
    std::printf("osg_essgraph_problem %zu\n", sizeof(osg_essgraph_problem));
    F(osg_essgraph_problem, n_vertices); F(osg_essgraph_problem, sim3); F(osg_essgraph_problem, fixed);
    F(osg_essgraph_problem, fix_scale); F(osg_essgraph_problem, n_edges); F(osg_essgraph_problem, e_v0);
    F(osg_essgraph_problem, e_v1); F(osg_essgraph_problem, e_meas); F(osg_essgraph_problem, max_iterations);
    F(osg_essgraph_problem, lambda_init);
    std::printf("osg_essgraph_result %zu\n", sizeof(osg_essgraph_result));
    F(osg_essgraph_result, sim3); F(osg_essgraph_result, chi2_initial); F(osg_essgraph_result, chi2_final);
    F(osg_essgraph_result, lm_iterations); F(osg_essgraph_result, lm_trials); F(osg_essgraph_result, edge_chi2);
    return 0;
}
