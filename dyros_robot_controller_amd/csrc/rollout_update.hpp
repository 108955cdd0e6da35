// The arithmetic of a closed-loop step's state update, shared by the rollout
// and the reach kernels through closed_loop.hpp: every path calls
// rollout_velocity / rollout_advance, so they return identical bits.
#pragma once

#include "kernel_common.hpp"

namespace drc_amd {

// v_{k+1} of joint row r.  Manipulator: eta.  Mobile manipulator: S(q_k) eta
// with the selection matrix of mobile_manipulator/robot_data.cpp:22-25,115-120
// -- identity on the arm and wheel rows, Rz(yaw) J_mobile on the virtual rows
// (the products qp_assemble forms for J~ = J S).  eta(a): actuated entry a.
template <class Eta>
__device__ __forceinline__ double rollout_velocity(const DevModel* M, int r, double cy, double sy,
                                                   const double (*Jm)[kMaxWheels], Eta eta) {
  if (M->kind == 0) return eta(r);
  const int a = r - M->mani_start, w = r - M->mobi_start, v = r - M->virtual_start;
  if (a >= 0 && a < M->n_arm) return eta(M->act_mani_start + a);
  if (w >= 0 && w < M->n_wheel) return eta(M->act_mobi_start + w);
  if (v < 0 || v > 2) return 0.0;
  double s = 0;
  for (int c = 0; c < M->n_wheel; ++c) {
    double sv;
    if (v == 0) sv = cy * Jm[0][c] - sy * Jm[1][c];
    else if (v == 1) sv = sy * Jm[0][c] + cy * Jm[1][c];
    else sv = Jm[2][c];
    s += sv * eta(M->act_mobi_start + c);
  }
  return s;
}

// q_{k+1} = q_k + dt v_{k+1}: a rounded product, then a rounded sum (never an
// fma), so numpy's q + dt * v reproduces it bit for bit
__device__ __forceinline__ double rollout_advance(double q, double dt, double v) {
#pragma clang fp contract(off)
  const double d = dt * v;
  return q + d;
}
// t_k = t + k dt, rounded the same way: the persistent kernel's step time and,
// on the host, the stepwise path's (api.cpp) are this one function
__host__ __device__ __forceinline__ double rollout_time(double t, int k, double dt) {
#pragma clang fp contract(off)
  const double d = static_cast<double>(k) * dt;
  return t + d;
}

// (LDS of the state update, at the start of the plan: lds_plan.hpp rollout_state_doubles)

// Orders this wave's global stores before its later loads of the same
// addresses: the stores have completed when the wait returns, and a CU's
// vector L1 is write-through, so the wave's own reload sees them.  (The IO
// pointers are not __restrict__, so the compiler keeps the program order too.)
__device__ __forceinline__ void state_visible() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

}  // namespace drc_amd
