// Host-side harness for the serial PinvCOD routines (csrc/pinv_cod.hpp,
// compiled for the CPU: no GPU needed).  Reads matrices on stdin, one per line:
//   S n st  A (n x n, row-major)     pinv_cod_serial, element (i,j) at [(i*n+j)*st]
//   R m n   A (m x n, row-major)     pinv_cod_rect (m == 6: also in the LDS
//                                    layout of closed_form_stage, task_stage.hpp)
// and prints the pseudo-inverse row-major on one line (n x n / n x m).
// Every array is its own heap block of exactly the documented size (the
// strided ones end at their last element), so that the build with
// -fsanitize=address,undefined reports any access outside them.
// Used by tests/test_pinv_cod_host.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <hip/hip_runtime.h>
#include "../dyros_robot_controller_amd/csrc/pinv_cod.hpp"
using namespace drc_amd;

static double* alloc(int n) {
  double* p = static_cast<double*>(malloc(sizeof(double) * (n > 0 ? n : 1)));
  for (int i = 0; i < n; ++i) p[i] = -7.25;  // stale contents, as LDS holds on the device
  return p;
}

// pinv_cod_serial's documented work size (pinv_cod.hpp) and pinv_cod_rect's
static int serial_work(int n) { return 3 * n * n + 3 * n; }
static int rect_work(int m, int n) { return m * n + m * m + n * m + 3 * m + 2 * n; }
// closed_form_stage (task_stage.hpp): X follows the COD work inside `ws`;
// api.cpp's LDS plan reserves max(160, cf_plan_ws(nv)) doubles for `ws`
static int cf_x_offset(int nv) { return 6 * nv + 36 + 6 * nv + 18 + 2 * nv; }
static int cf_plan_ws(int nv) { return 6 * nv + 36 + 6 * nv + 18 + 2 * nv + 6 * nv; }

static int run_serial(int n, int st, const double* a) {
  const int len = n > 0 ? (n * n - 1) * st + 1 : 0;
  double *A = alloc(len), *X = alloc(len), *w = alloc(serial_work(n));
  for (int i = 0; i < n * n; ++i) A[i * st] = a[i];
  pinv_cod_serial(A, n, st, X, w);
  for (int i = 0; i < n * n; ++i) printf("%s%.17g", i ? " " : "", X[i * st]);
  printf("\n");
  // the gaps of a strided array belong to other robots of the block: untouched
  for (int i = 0; i < len; ++i)
    if (i % st && (A[i] != -7.25 || X[i] != -7.25)) return 3;
  free(A); free(X); free(w);
  return 0;
}

static int run_rect(int m, int n, const double* a) {
  double *A = alloc(m * n), *X = alloc(n * m), *w = alloc(rect_work(m, n));
  memcpy(A, a, sizeof(double) * m * n);
  pinv_cod_rect(A, m, n, X, w);
  if (m == 6) {
    // the stage's layout: one block of the size the LDS plan reserves, X at
    // the offset closed_form_stage computes; same bits as the separate arrays
    if (cf_x_offset(n) < rect_work(6, n) || cf_x_offset(n) + 6 * n > cf_plan_ws(n)) return 4;
    double* ws = alloc(cf_plan_ws(n));
    double* X2 = ws + cf_x_offset(n);
    pinv_cod_rect(A, 6, n, X2, ws);
    if (memcmp(X, X2, sizeof(double) * 6 * n) != 0) return 5;
    free(ws);
  }
  for (int i = 0; i < n * m; ++i) printf("%s%.17g", i ? " " : "", X[i]);
  printf("\n");
  free(A); free(X); free(w);
  return 0;
}

int main() {
  char kind;
  int a, b;
  while (scanf(" %c %d %d", &kind, &a, &b) == 3) {
    int rows, cols;
    if (kind == 'S') {
      if (a < 0 || a > kMaxJoints || b < 1) return 2;
      rows = cols = a;
    } else if (kind == 'R') {
      if (a < 1 || a > 6 || b < 1 || b > kMaxJoints) return 2;
      rows = a, cols = b;
    } else {
      return 2;
    }
    double* v = alloc(rows * cols);
    for (int i = 0; i < rows * cols; ++i)
      if (scanf("%lf", &v[i]) != 1) return 2;
    const int rc = kind == 'S' ? run_serial(a, b, v) : run_rect(a, b, v);
    free(v);
    if (rc) return rc;
  }
  return 0;
}
