// Host harness of the reach error and thresholds (csrc/reach.hpp), compiled
// with the host compiler alone (tests/test_reach_host.py).
//   stdin:  one case per line: "e" pose (12) target (12), both in the API's
//           layout (R column-major, then p); or "t" pos_tol rot_tol
//   stdout: per "e" line e_p e_R and whether they lie within the thresholds of
//           the last "t" line (0 / 1); per "t" line tau_p tau_R; %.17g
#include <cstdio>

#include "../dyros_robot_controller_amd/csrc/reach.hpp"

int main() {
  char kind;
  double tau[2] = {0.0, 0.0};
  while (std::scanf(" %c", &kind) == 1) {
    if (kind == 't') {
      double pos_tol, rot_tol;
      if (std::scanf("%lf %lf", &pos_tol, &rot_tol) != 2) return 1;
      drc_amd::reach_thresholds(pos_tol, rot_tol, tau);
      std::printf("%.17g %.17g\n", tau[0], tau[1]);
    } else if (kind == 'e') {
      double pose[12], target[12], err[2];
      for (int i = 0; i < 12; ++i)
        if (std::scanf("%lf", &pose[i]) != 1) return 1;
      for (int i = 0; i < 12; ++i)
        if (std::scanf("%lf", &target[i]) != 1) return 1;
      const double* pc = pose;
      const double* tc = target;
      drc_amd::reach_error(pc, tc, err);
      std::printf("%.17g %.17g %d\n", err[0], err[1], drc_amd::reach_within(err, tau[0], tau[1]) ? 1 : 0);
    } else {
      return 1;
    }
  }
  return 0;
}
