// TEST INFRASTRUCTURE ONLY (tests/test_gpu_mesh_narrow.py): the hull narrow
// phase of the task kernel -- gjk_wave, epa_run_wave with the cooperative hull
// support, sphere_hull_witness, refine_witness_hull: the functions task_stage.hpp calls for a pair
// with a hull, in the same order -- on one wavefront per shape pair, so it can
// be checked pair by pair against a scipy restatement.  Built by build.sh into
// tests/_mesh_narrow_gpu.so.
#include <hip/hip_runtime.h>

#include "../dyros_robot_controller_amd/csrc/qpik_device.hpp"

using namespace drc_amd;

using HullW = ShapeMT<const double*, true>;

// in: per pair 2 x 18 doubles (type, T[12], prm[3], first vertex, vertex count);
// verts: [nverts][3]; out: d, pA, pB, intersect (GJK's flag), d of the lane-serial GJK
__global__ void __launch_bounds__(64) mesh_narrow_kernel(const double* __restrict__ in, const double* __restrict__ verts,
                                                         int n, double* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  EpaPoly* E = reinterpret_cast<EpaPoly*>(lds);
  const int i = blockIdx.x, l = threadIdx.x;
  if (i >= n) return;
  const double* p = in + 36 * i;
  const HullW A{int(p[0]), p + 1, p[13], p[14], p[15], verts + 3 * int(p[16]), int(p[17])};
  const HullW B{int(p[18]), p + 19, p[31], p[32], p[33], verts + 3 * int(p[34]), int(p[35])};
  const double rs = A.type == kSphere ? A.p0 : (B.type == kSphere ? B.p0 : 0.0);
  const bool poly = A.type != kCylinder && B.type != kCylinder;
  const double tol = poly ? 0.0 : kGjkTol;
  if (l == 0) E->nv = 0;  // the stash counter, as the task stage zeroes it
  wsync();
  const GjkDist g = gjk_wave(A, B, 1e300, tol, E, i);
  double d = g.dist;
  V3 pA = g.pA, pB = g.pB;
  double dser = 0;
  if (g.intersect) {  // wave-uniform
    const int sn = static_cast<int>(E->out[1]);  // stashed simplex 0
    wsync();
    d = epa_run_wave(A, B, E, 0, 0, sn);
    wsync();
    pA = ld3(E->out);
    pB = ld3(E->out + 3);
  } else if (l == 0) {  // the same GJK with one lane scanning every vertex
    GjkState gs;
    gjk_run(serial_shape(A), serial_shape(B), gs, 1e300, tol);
    dser = sqrt(dot(gs.v, gs.v));
  }
  if (rs > 0) sphere_hull_witness(A.type == kSphere, rs, &d, &pA, &pB);
  // the winner's exact finish, on one lane as in the task stage
  if (l == 0) refine_witness_hull(serial_shape(A), serial_shape(B), &d, &pA, &pB);
  if (l == 0) {
    double* o = out + 9 * i;
    o[0] = d;
    o[1] = pA.x; o[2] = pA.y; o[3] = pA.z;
    o[4] = pB.x; o[5] = pB.y; o[6] = pB.z;
    o[7] = g.intersect;
    o[8] = dser;
  }
}

extern "C" int drc_test_mesh_narrow(const double* h_in, int n, const double* h_verts, int nverts, double* h_out) {
  double *din = nullptr, *dv = nullptr, *dout = nullptr;
  if (hipMalloc(&din, sizeof(double) * 36 * n) != hipSuccess) return 1;
  if (hipMalloc(&dv, sizeof(double) * 3 * (nverts > 0 ? nverts : 1)) != hipSuccess) return 1;
  if (hipMalloc(&dout, sizeof(double) * 9 * n) != hipSuccess) return 1;
  (void)hipMemcpy(din, h_in, sizeof(double) * 36 * n, hipMemcpyHostToDevice);
  (void)hipMemcpy(dv, h_verts, sizeof(double) * 3 * nverts, hipMemcpyHostToDevice);
  hipLaunchKernelGGL(mesh_narrow_kernel, dim3(n), dim3(64), sizeof(EpaPoly), 0, din, dv, n, dout);
  int rc = hipGetLastError() != hipSuccess;
  rc |= hipMemcpy(h_out, dout, sizeof(double) * 9 * n, hipMemcpyDeviceToHost) != hipSuccess;
  (void)hipFree(din);
  (void)hipFree(dv);
  (void)hipFree(dout);
  return rc;
}
