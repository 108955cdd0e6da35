// Host-side harness for the dense core of the polish's small EQP
// (csrc/eqp_small.hpp, compiled for the CPU: no GPU needed).  Reads systems on
// stdin, one per line:
//   NS nF nR delta refine  K0 (N x N, row-major, N = nF + nR)  rhs (N)
// pads each to the tier NS exactly as the kernel does (zero K0 rows, zero
// right-hand side, identity regularisation: eqp_small_reg) and prints
//   ok sol[0] .. sol[NS-1]
// Used by tests/test_eqp_small_host.py.
#include <cstdio>
#include <hip/hip_runtime.h>
#include "../dyros_robot_controller_amd/csrc/eqp_small.hpp"
using namespace drc_amd;

template <int NS>
static void run(int nF, int nR, double delta, int refine, const double* K, const double* b) {
  const int N = nF + nR;
  double K0[NS * (NS + 1) / 2], reg[NS], rhs[NS], sol[NS];
  for (int i = 0; i < NS; ++i) {
    rhs[i] = i < N ? b[i] : 0.0;
    reg[i] = eqp_small_reg(i, nF, N, delta);
    for (int j = 0; j <= i; ++j) K0[eqp_pk(i, j)] = i < N ? K[i * N + j] : 0.0;
    sol[i] = 0.0;
  }
  const bool ok = eqp_small_core<NS>(K0, reg, rhs, refine, sol);
  printf("%d", ok ? 1 : 0);
  for (int i = 0; i < NS; ++i) printf(" %.17g", sol[i]);
  printf("\n");
}

int main() {
  int ns, nF, nR, refine;
  double delta;
  while (scanf("%d %d %d %lf %d", &ns, &nF, &nR, &delta, &refine) == 5) {
    const int N = nF + nR;
    double K[64], b[8];
    if (N < 0 || N > 8 || N > ns) return 2;
    for (int i = 0; i < N * N; ++i)
      if (scanf("%lf", &K[i]) != 1) return 2;
    for (int i = 0; i < N; ++i)
      if (scanf("%lf", &b[i]) != 1) return 2;
    if (ns == 2) run<2>(nF, nR, delta, refine, K, b);
    else if (ns == 4) run<4>(nF, nR, delta, refine, K, b);
    else if (ns == 8) run<8>(nF, nR, delta, refine, K, b);
    else return 2;
  }
  return 0;
}
