// sim3_algebra.cpp — stand-alone host program over csrc/sim3_common.h (test-only): evaluates the Sim3
// exponential in its four branches, operator*, inverse() and map() on fixed inputs and prints every
// double as a hex float.  tests/test_sim3opt.py compares the lines with tests/pyref_sim3opt.py.
// Plain host C++: it may be built with -fsanitize=address,undefined and run directly.
#include <cstdio>

#include "sim3_common.h"

using osgs3::Sim3;

static void put(const char *name, const double *v, int n)
{
    std::printf("%s", name);
    for (int i = 0; i < n; i++) std::printf(" %a", v[i]);
    std::printf("\n");
}
static void put_sim3(const char *name, const Sim3 &S)
{
    double v[8] = {S.q[0], S.q[1], S.q[2], S.q[3], S.t[0], S.t[1], S.t[2], S.s};
    put(name, v, 8);
}

int main()
{
    // (omega, upsilon, sigma): small sigma / small theta, small sigma / large theta, large sigma / small
    // theta, large sigma / large theta
    const double U[4][7] = {{3e-6, 2e-6, 4e-6, 0.4, 0.5, 0.6, 2e-6},
                            {0.07, 0.05, 0.04, 0.4, 0.5, 0.6, -3e-6},
                            {2e-6, 5e-6, 1e-6, 0.4, 0.5, 0.6, 0.04},
                            {0.06, 0.09, 0.05, 0.6, 0.5, 0.4, -0.07}};
    const char *names[4] = {"exp_ss", "exp_sl", "exp_ls", "exp_ll"};
    Sim3 E[4];
    for (int k = 0; k < 4; k++) {
        E[k] = osgs3::sim3_exp(U[k]);
        put_sim3(names[k], E[k]);
    }
    put_sim3("mul", osgs3::sim3_mul(E[3], E[1]));
    put_sim3("inverse", osgs3::sim3_inverse(E[3]));
    const double x[3] = {1.1, 1.3, 1.7};
    double y[3];
    osgs3::sim3_map(E[3], x, y);
    put("map", y, 3);
    const double upd[7] = {1e-9, 0, 0, 0, 0, 0, 0.5};
    put_sim3("oplus_fix", osgs3::sim3_oplus(E[1], upd, true));
    return 0;
}
