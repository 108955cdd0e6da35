// Host harness of the half-space closed form (csrc/halfspace.hpp), compiled
// with the host compiler alone (tests/test_halfspace_host.py).
//   stdin:  one case per line: type p0 p1 p2, the shape's pose (12: R
//           row-major, then p), the half-space's pose (12)
//   stdout: d, the shape's witness (3), the half-space's witness (3), %.17g
#include <cstdio>

#include "../dyros_robot_controller_amd/csrc/halfspace.hpp"

int main() {
  int type;
  double p[3], T[12], P[12];
  for (;;) {
    if (std::scanf("%d %lf %lf %lf", &type, &p[0], &p[1], &p[2]) != 4) break;
    for (int i = 0; i < 12; ++i)
      if (std::scanf("%lf", &T[i]) != 1) return 1;
    for (int i = 0; i < 12; ++i)
      if (std::scanf("%lf", &P[i]) != 1) return 1;
    double ps[3], pp[3];
    const double* Tc = T;
    const double* Pc = P;
    const double d = drc_amd::halfspace_distance(type, Tc, p[0], p[1], p[2], Pc, ps, pp);
    std::printf("%.17g %.17g %.17g %.17g %.17g %.17g %.17g\n", d, ps[0], ps[1], ps[2], pp[0], pp[1], pp[2]);
  }
  return 0;
}
