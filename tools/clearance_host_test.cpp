// Host harness of the path-clearance sample states and fold rule
// (csrc/clearance.hpp), compiled with the host compiler alone
// (tests/test_clearance_host.py).
//   stdin:  one case per line:
//             "s" qa qb substeps          (doubles as %la hex floats)
//             "f" d_stop n d_0 .. d_{n-1} (the distances in order; pair_k = 100 + k)
//   stdout: per "s" line the samples i = 1 .. substeps of the segment, %a;
//           per "f" line "result sample_stop d_min sample_min pair_min seen":
//           d_min %a, seen = how many distances the walk took before it stopped
#include <cstdio>
#include <vector>

#include "../dyros_robot_controller_amd/csrc/clearance.hpp"

int main() {
  char kind;
  while (std::scanf(" %c", &kind) == 1) {
    if (kind == 's') {
      double qa, qb;
      int sub;
      if (std::scanf("%la %la %d", &qa, &qb, &sub) != 3) return 1;
      for (int i = 1; i <= sub; ++i) std::printf("%a%c", drc_amd::clearance_sample(qa, qb, i, sub), i == sub ? '\n' : ' ');
    } else if (kind == 'f') {
      double d_stop;
      int n;
      if (std::scanf("%la %d", &d_stop, &n) != 2) return 1;
      std::vector<double> d(static_cast<size_t>(n));
      for (int k = 0; k < n; ++k)
        if (std::scanf("%la", &d[static_cast<size_t>(k)]) != 1) return 1;
      drc_amd::ClearFold f;
      int seen = 0;
      for (int k = 0; k < n; ++k) {
        ++seen;
        if (drc_amd::clearance_step(&f, k, d[static_cast<size_t>(k)], 100 + k, d_stop)) break;
      }
      std::printf("%d %d %a %d %d %d\n", f.result, f.sample_stop, f.d_min, f.sample_min, f.pair_min, seen);
    } else {
      return 1;
    }
  }
  return 0;
}
