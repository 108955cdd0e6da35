// Host check of csrc/qpik_pattern.hpp (tests/test_qpik_pattern_host.py): for
// N = 6 and N = 7 joints, G built densely by qp_assemble's rule (QP_IK.cpp:99-131)
// with random nonzero gradient rows and random positive row / column factors
// (what Ruiz scaling does to it), then
//   pattern : col_row / row_col / slack_col enumerate exactly the nonzero
//             positions of every column and row, in ascending order
//   colsum  : parity_sums over a column's four rows == the dense column pass
//             (even rows into r0, odd rows into r1, ascending), bit for bit,
//             from r0 = r1 = 0 (ADMM) and from r0 = q (the polish's guess)
//   rowsum  : a row's sum over row_col == the dense row sum, bit for bit
// Prints one "ok <check> <N> <cases>" line per check; any mismatch prints
// "FAIL ..." and the exit status is 1.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../dyros_robot_controller_amd/csrc/qpik_pattern.hpp"

using drc_amd::QpikPattern;

static int g_fail = 0;

static bool same_bits(double a, double b) {
  uint64_t x, y;
  std::memcpy(&x, &a, 8);
  std::memcpy(&y, &b, 8);
  return x == y;
}

template <int N>
static std::vector<double> build_g(std::mt19937_64& rng, bool scaled) {
  using Pat = QpikPattern<N>;
  constexpr int ng = Pat::ng, nx = Pat::nx;
  std::uniform_real_distribution<double> u(0.05, 3.0), sgn(-1.0, 1.0);
  std::vector<double> G(ng * nx, 0.0);
  for (int l = 0; l < ng; ++l) {
    if (l < N) {
      G[l * nx + l] = 1.0;
      G[l * nx + N + l] = 1.0;
    } else if (l < 2 * N) {
      G[l * nx + (l - N)] = -1.0;
      G[l * nx + 2 * N + (l - N)] = 1.0;
    } else if (l == 2 * N) {
      for (int c = 0; c < N; ++c) G[l * nx + c] = (sgn(rng) < 0 ? -1.0 : 1.0) * u(rng);
      G[l * nx + 3 * N] = 1.0;
    } else {
      for (int c = 0; c < N; ++c) G[l * nx + c] = (sgn(rng) < 0 ? -1.0 : 1.0) * u(rng);
      G[l * nx + 3 * N + 1] = 1.0;
    }
  }
  if (scaled) {
    std::vector<double> D(nx), E(ng);
    for (double& d : D) d = u(rng);
    for (double& e : E) e = u(rng);
    for (int r = 0; r < ng; ++r)
      for (int c = 0; c < nx; ++c) G[r * nx + c] *= E[r] * D[c];
  }
  return G;
}

template <int N>
static void check(int cases) {
  using Pat = QpikPattern<N>;
  constexpr int ng = Pat::ng, nx = Pat::nx;
  static_assert(Pat::slack_col(0) == N && Pat::kDist == ng - 1, "layout");
  std::mt19937_64 rng(1000 + N);
  std::uniform_real_distribution<double> val(-4.0, 4.0);
  int npat = 0, ncol = 0, nrow = 0;
  for (int t = 0; t < cases; ++t) {
    const std::vector<double> G = build_g<N>(rng, t & 1);
    // ---- pattern --------------------------------------------------------
    for (int c = 0; c < nx; ++c) {
      std::vector<int> nz;
      for (int r = 0; r < ng; ++r)
        if (G[r * nx + c] != 0.0) nz.push_back(r);
      bool ok = static_cast<int>(nz.size()) == Pat::col_count(c);
      for (int k = 0; ok && k < Pat::col_count(c); ++k) ok = nz[k] == Pat::col_row(c, k);
      for (int k = 1; ok && k < Pat::col_count(c); ++k) ok = Pat::col_row(c, k) > Pat::col_row(c, k - 1);
      if (!ok) { std::printf("FAIL pattern N=%d column %d\n", N, c); ++g_fail; }
      ++npat;
    }
    for (int r = 0; r < ng; ++r) {
      std::vector<int> nz;
      for (int c = 0; c < nx; ++c)
        if (G[r * nx + c] != 0.0) nz.push_back(c);
      bool ok = static_cast<int>(nz.size()) == Pat::row_count(r);
      for (int k = 0; ok && k < Pat::row_count(r); ++k) ok = nz[k] == Pat::row_col(r, k);
      for (int k = 1; ok && k < Pat::row_count(r); ++k) ok = Pat::row_col(r, k) > Pat::row_col(r, k - 1);
      ok = ok && nz.back() == Pat::slack_col(r) && Pat::slack_col(r) >= N;  // the one entry past the q-dot block
      for (int c = N; ok && c < nx; ++c) ok = (G[r * nx + c] != 0.0) == (c == Pat::slack_col(r));
      if (!ok) { std::printf("FAIL pattern N=%d row %d\n", N, r); ++g_fail; }
      ++npat;
    }
    // ---- column sums with the parity split ---------------------------------
    std::vector<double> u(ng), x(nx), q(nx);
    for (double& v : u) v = val(rng);
    for (double& v : x) v = val(rng);
    for (double& v : q) v = val(rng);
    if (t % 5 == 0) u[(t / 5) % ng] = 0.0;  // zeros and negative zeros among the data
    if (t % 7 == 0) u[(t / 7) % ng] = -0.0;
    if (t % 3 == 0) q[(t / 3) % N] = 0.0;
    for (int c = 0; c < N; ++c) {
      for (int start = 0; start < 2; ++start) {
        double d0 = start ? q[c] : 0.0, d1 = 0.0;
        for (int i = 0; i < ng; ++i) {
          if (i & 1) d1 += G[i * nx + c] * u[i];
          else d0 += G[i * nx + c] * u[i];
        }
        double s0 = start ? q[c] : 0.0, s1 = 0.0;
        const int ra = Pat::pair_a(c), rb = Pat::pair_b(c);
        Pat::parity_sums(c, G[ra * nx + c], u[ra], G[rb * nx + c], u[rb], G[Pat::kMan * nx + c], u[Pat::kMan],
                         G[Pat::kDist * nx + c], u[Pat::kDist], s0, s1);
        // (the two partial sums never start at -0 here; the kernels' one start that can be -0, the polish
        // guess's q_l, is read only through d0 + d1, where a zero's sign is lost: checked below)
        if (!same_bits(d0, s0) || !same_bits(d1, s1) || !same_bits(d0 + d1, s0 + s1)) {
          std::printf("FAIL colsum N=%d column %d start %d: dense %.17g %.17g sparse %.17g %.17g\n", N, c, start, d0, d1,
                      s0, s1);
          ++g_fail;
        }
        ++ncol;
      }
      {  // from -0, all four data zero: the dense sum turns +0 or stays -0 with the signs, c0 + c1 does not care
        double d0 = -0.0, d1 = 0.0, s0 = -0.0, s1 = 0.0;
        std::vector<double> z(ng, (t & 1) ? -0.0 : 0.0);
        for (int i = 0; i < ng; ++i) {
          if (i & 1) d1 += G[i * nx + c] * z[i];
          else d0 += G[i * nx + c] * z[i];
        }
        const int ra = Pat::pair_a(c), rb = Pat::pair_b(c);
        Pat::parity_sums(c, G[ra * nx + c], z[ra], G[rb * nx + c], z[rb], G[Pat::kMan * nx + c], z[Pat::kMan],
                         G[Pat::kDist * nx + c], z[Pat::kDist], s0, s1);
        if (!same_bits(d0 + d1, s0 + s1)) {
          std::printf("FAIL colsum N=%d column %d from -0\n", N, c);
          ++g_fail;
        }
      }
    }
    // ---- row sums -----------------------------------------------------------
    for (int r = 0; r < ng; ++r) {
      double d = 0.0, s = 0.0;
      for (int j = 0; j < nx; ++j) d += G[r * nx + j] * x[j];
      for (int k = 0; k < Pat::row_count(r); ++k) s += G[r * nx + Pat::row_col(r, k)] * x[Pat::row_col(r, k)];
      if (!same_bits(d, s)) {
        std::printf("FAIL rowsum N=%d row %d: dense %.17g sparse %.17g\n", N, r, d, s);
        ++g_fail;
      }
      ++nrow;
    }
  }
  std::printf("ok pattern %d %d\nok colsum %d %d\nok rowsum %d %d\n", N, npat, N, ncol, N, nrow);
}

int main() {
  check<6>(200);
  check<7>(200);
  return g_fail ? 1 : 0;
}
