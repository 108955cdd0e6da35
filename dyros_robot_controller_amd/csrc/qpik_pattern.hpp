// The fixed sparsity of the manipulator QP-IK constraint matrix G (qp_assemble,
// QP_IK.cpp:99-131), for N joints: ng = 2 N + 2 rows over nx = N + ng columns
// (N q-dot columns, then one slack column per row).
//   row r < 2 N : +-1 at column r mod N, and its slack column N + r
//   row 2 N     : the manipulability gradient (columns 0 .. N-1), slack 3 N
//   row 2 N + 1 : the distance gradient       (columns 0 .. N-1), slack 3 N + 1
// so q-dot column c sits in rows {c, N + c, 2 N, 2 N + 1} and slack column
// N + r in row r alone.  Ruiz scaling multiplies entries, so the pattern
// survives it.  Every list below is in ascending order: the solver's sums keep
// the order and grouping of the dense loops' nonzero terms (the skipped terms
// are exact zeros), so they return the dense results bit for bit.
// Host and device (tools/qpik_pattern_host_test.cpp runs it on the CPU).
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DRC_PAT_HD __host__ __device__ __forceinline__
#else
#define DRC_PAT_HD inline
#endif

namespace drc_amd {

template <int N>
struct QpikPattern {
  static constexpr int n = N, ng = 2 * N + 2, nx = 3 * N + 2;
  static constexpr int kMan = 2 * N, kDist = 2 * N + 1;  // the two gradient rows
  // rows of column c, ascending
  static DRC_PAT_HD constexpr int col_count(int c) { return c < N ? 4 : 1; }
  static DRC_PAT_HD constexpr int col_row(int c, int k) {
    return c < N ? (k == 0 ? c : (k == 1 ? N + c : 2 * N + (k - 2))) : c - N;
  }
  // columns of row r, ascending (the slack column last)
  static DRC_PAT_HD constexpr int row_count(int r) { return r < 2 * N ? 2 : N + 1; }
  static DRC_PAT_HD constexpr int row_col(int r, int k) {
    return r < 2 * N ? (k == 0 ? (r < N ? r : r - N) : N + r) : (k < N ? k : N + r);
  }
  static DRC_PAT_HD constexpr int slack_col(int r) { return N + r; }

  // The dense column passes (ADMM rhs, the polish's Jacobi constant) split
  // their sum over the rows by row parity: r0 takes the even rows, r1 the odd
  // ones, each in ascending order.  Of q-dot column c's rows, 2 N is even and
  // 2 N + 1 odd; c and N + c differ in parity when N is odd and agree when N
  // is even.  pair_a / pair_b name those two rows in the order parity_sums
  // takes them: (even row, odd row) for odd N, (c, N + c) for even N.
  static DRC_PAT_HD constexpr int pair_a(int c) { return (N & 1) && (c & 1) ? N + c : c; }
  static DRC_PAT_HD constexpr int pair_b(int c) { return (N & 1) && (c & 1) ? c : N + c; }
  // r0 += sum over even rows, r1 += sum over odd rows of g_r u_r for column
  // c's four rows: (ga, ua) / (gb, ub) rows pair_a / pair_b, (gm, um) row 2 N,
  // (gd, ud) row 2 N + 1.  One multiply-add per term, as in the dense loops.
  static DRC_PAT_HD void parity_sums(int c, double ga, double ua, double gb, double ub, double gm, double um,
                                     double gd, double ud, double& r0, double& r1) {
    if constexpr (N & 1) {
      r0 += ga * ua;
      r0 += gm * um;
      r1 += gb * ub;
      r1 += gd * ud;
    } else {
      const bool odd = c & 1;  // rows c and N + c both go to this accumulator, c first
      double a = odd ? r1 : r0;
      a += ga * ua;
      a += gb * ub;
      double e = odd ? r0 : a, o = odd ? a : r1;
      e += gm * um;
      o += gd * ud;
      r0 = e;
      r1 = o;
    }
  }
};

}  // namespace drc_amd
