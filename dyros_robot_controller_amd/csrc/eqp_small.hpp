// Dense core of the polish's small reduced-KKT solve (qp_solver.hpp:
// eqp_small): an NS x NS quasi-definite system, NS a compile-time cap, held
// whole by the caller (on the device every lane of the wave holds the same
// copy and factors it redundantly in its own registers: no cross-lane traffic,
// no LDS round trip per pivot).  Plain host / device code with no wave
// intrinsics, so tools/eqp_small_host_test.hip runs it on the CPU
// (tests/test_eqp_small_host.py).
#pragma once

#ifndef DRC_HD
#define DRC_HD __host__ __device__
#endif

namespace drc_amd {

// packed lower triangle: entry (i, j), i >= j
DRC_HD constexpr int eqp_pk(int i, int j) { return i * (i + 1) / 2 + j; }

// Diagonal regularisation of row j of a reduced KKT with nF free variables
// and N - nF active rows, padded to the cap: [P_FF + dI, G^T; G, -dI], and the
// identity on the padding (rows j >= N: K0 row zero, right-hand side zero, so
// their solution entries stay exact zeros and touch nothing else)
DRC_HD __forceinline__ double eqp_small_reg(int j, int nF, int N, double delta) {
  return j < nF ? delta : (j < N ? -delta : 1.0);
}

// (L D L^T) b = b in place; L unit lower (packed, strict part), di = 1 / D
template <int NS>
DRC_HD __forceinline__ void eqp_small_ldl_solve(const double (&L)[NS * (NS + 1) / 2], const double (&di)[NS],
                                                double (&b)[NS]) {
#pragma unroll
  for (int j = 0; j < NS; ++j) {
#pragma unroll
    for (int i = j + 1; i < NS; ++i) b[i] -= L[eqp_pk(i, j)] * b[j];
  }
#pragma unroll
  for (int i = 0; i < NS; ++i) b[i] *= di[i];
#pragma unroll
  for (int j = NS - 1; j > 0; --j) {
#pragma unroll
    for (int i = 0; i < j; ++i) b[i] -= L[eqp_pk(j, i)] * b[j];
  }
}

// Solves K0 sol = rhs: LDL^T (natural order, no pivoting: quasi-definite) of
// K0 + diag(reg), then `refine` steps of iterative refinement against the
// unregularised K0 (packed lower triangle of the symmetric matrix).  One
// division per pivot (its reciprocal, formed once).  A zero pivot returns
// false.  Straight-line: every loop bound is NS.
template <int NS>
DRC_HD __forceinline__ bool eqp_small_core(const double (&K0)[NS * (NS + 1) / 2], const double (&reg)[NS],
                                           const double (&rhs)[NS], int refine, double (&sol)[NS]) {
  double L[NS * (NS + 1) / 2], d[NS], di[NS];
#pragma unroll
  for (int j = 0; j < NS; ++j) {
    double v[NS];  // L_jk d_k, k < j
    double dj = K0[eqp_pk(j, j)] + reg[j];
#pragma unroll
    for (int k = 0; k < j; ++k) {
      v[k] = L[eqp_pk(j, k)] * d[k];
      dj -= L[eqp_pk(j, k)] * v[k];
    }
    if (dj == 0.0) return false;
    d[j] = dj;
    di[j] = 1.0 / dj;
    L[eqp_pk(j, j)] = 1.0;
#pragma unroll
    for (int i = j + 1; i < NS; ++i) {
      double t = K0[eqp_pk(i, j)];
#pragma unroll
      for (int k = 0; k < j; ++k) t -= L[eqp_pk(i, k)] * v[k];
      L[eqp_pk(i, j)] = t * di[j];
    }
  }
#pragma unroll
  for (int i = 0; i < NS; ++i) sol[i] = rhs[i];
  eqp_small_ldl_solve<NS>(L, di, sol);
  for (int it = 0; it < refine; ++it) {
    double res[NS];
#pragma unroll
    for (int i = 0; i < NS; ++i) {
      double r = rhs[i];
#pragma unroll
      for (int j = 0; j < NS; ++j) r -= K0[i >= j ? eqp_pk(i, j) : eqp_pk(j, i)] * sol[j];
      res[i] = r;
    }
    eqp_small_ldl_solve<NS>(L, di, res);
#pragma unroll
    for (int i = 0; i < NS; ++i) sol[i] += res[i];
  }
  return true;
}

}  // namespace drc_amd
