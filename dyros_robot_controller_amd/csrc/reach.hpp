// The stopping rule of drc_qpik_reach_batch: the error of a pose against the
// target as two trig-free numbers, and the thresholds they are compared with.
// Reference: no counterpart (its loop runs until the caller stops it).
//
//   e_p = |p_t - p|^2
//   e_R = |R - R_t|_F^2 = 8 sin^2(theta / 2), theta the angle between R and R_t
// so "within pos_tol metres and rot_tol radians" is e_p <= pos_tol^2 and
// e_R <= 8 sin^2(rot_tol / 2) without a square root, an acos or a logarithm of
// a rotation.  Both sums are formed in a fixed order with contraction off, so
// the persistent kernels (reach_kernel.hip, reach_path_kernel.hip), the
// stepwise path's update kernel (reach_path_kernel.hip),
// the host compiler (tools/reach_host_test.cpp, tests/test_reach_host.py) and
// numpy on the same doubles give the same bits.
//
// Plain host / device code without wave intrinsics, like halfspace.hpp.
#pragma once

#include <cmath>

#ifndef DRC_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define DRC_HD __host__ __device__
#else
#define DRC_HD
#endif
#endif

namespace drc_amd {

// pose, target: 12 values each in the API's layout (R column-major, then p;
// any pointer-like type).  err[0] = e_p = (dx dx + dy dy) + dz dz with
// d = target - pose; err[1] = e_R = sum over i = 0 .. 8, from 0 upward, of
// (pose[i] - target[i])^2.  Every product and every sum is rounded (no fma).
template <class PP, class PT>
DRC_HD inline void reach_error(PP pose, PT target, double* err) {
#pragma clang fp contract(off)
  const double dx = target[9] - pose[9], dy = target[10] - pose[10], dz = target[11] - pose[11];
  const double xx = dx * dx, yy = dy * dy, zz = dz * dz;
  const double xy = xx + yy;
  err[0] = xy + zz;
  double s = 0.0;
  for (int i = 0; i < 9; ++i) {
    const double d = pose[i] - target[i];
    const double dd = d * d;
    s = s + dd;
  }
  err[1] = s;
}

// The verdict: both errors within their thresholds.  A NaN fails both
// comparisons (the instance goes on to the QP, whose status then speaks).
DRC_HD inline bool reach_within(const double* err, double tau_p, double tau_r) {
  return err[0] <= tau_p && err[1] <= tau_r;
}

// tau[0] = pos_tol^2, tau[1] = 8 (s s) with s = sin(rot_tol / 2).  Host only
// (drc_reach_thresholds): the device takes the two numbers as arguments, so
// the host's sine is the only one involved.
inline void reach_thresholds(double pos_tol, double rot_tol, double* tau) {
#pragma clang fp contract(off)
  tau[0] = pos_tol * pos_tol;
  const double s = std::sin(0.5 * rot_tol);
  const double ss = s * s;
  tau[1] = 8.0 * ss;
}

}  // namespace drc_amd
