// sim3_log.cpp — stand-alone host program over csrc/sim3_common.h (test-only).  Reads lines from stdin:
//   L q0 q1 q2 q3 t0 t1 t2 s   -> Sim3::log of that Sim3
//   E u0 .. u6                 -> log(exp(u))
// (hex floats accepted) and prints the seven doubles of each as hex floats.  tests/test_essgraph.py compares
// them with tests/pyref_essgraph.py.  Plain host C++: it may be built with -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "sim3_common.h"

using osgs3::Sim3;

int main()
{
    char line[1024];
    while (std::fgets(line, sizeof line, stdin)) {
        char *p = line + 1;
        double v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        const int n = line[0] == 'L' ? 8 : line[0] == 'E' ? 7 : 0;
        if (!n) continue;
        for (int i = 0; i < n; i++) v[i] = std::strtod(p, &p);
        Sim3 S;
        if (n == 8) {
            for (int i = 0; i < 4; i++) S.q[i] = v[i];
            for (int i = 0; i < 3; i++) S.t[i] = v[4 + i];
            S.s = v[7];
        } else {
            S = osgs3::sim3_exp(v);
        }
        double out[7];
        osgs3::sim3_log(S, out);
        for (int i = 0; i < 7; i++) std::printf("%a%c", out[i], i == 6 ? '\n' : ' ');
    }
    return 0;
}
