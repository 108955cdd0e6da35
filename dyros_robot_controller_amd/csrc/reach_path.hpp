// drc_qpik_reach_path_batch (reach_path_kernel.hip,
// reach_path_obstacle_kernel.hip): what its kernels need beyond IO and
// ReachArgs, and their host-side launchers (called by api.cpp; each returns
// the hipError_t of its launch).  A header of its own, so that launch.hpp and
// the units that include it stay what they are.
#pragma once

#include "launch.hpp"

namespace drc_amd {

// re: as for drc_qpik_reach_batch, with max_steps the budget of one segment
// and steps_used the total step count.  W waypoints x_path [W][12][B] /
// xdot_path [W][6][B]; waypoints_reached [B]; dist_min [B] and steps_at [W][B]
// may be NULL.  Stepwise path only: cur_xt [12][B] / cur_xdt [6][B], every
// instance's current target, and seg [B], its segment step count
struct ReachPathArgs {
  ReachArgs re;
  int W;
  const double *x_path, *xdot_path;
  int32_t* waypoints_reached;
  double* dist_min;
  int32_t* steps_at;
  double *cur_xt, *cur_xdt;
  int32_t* seg;
};

// persistent kernel (compiled QPIK shapes in the Plain and Obst builds,
// hipErrorInvalidValue otherwise): per instance task stage, verdict / waypoint
// advance, QP and state update until it stops.  io as for launch_fused_kernel,
// with out / status / iters one step's scratch (all three required); its xt /
// xdt unused (the kernel points them at the current waypoint's block).  The
// LDS size follows from kt and kq
int launch_reach_path_kernel(unsigned grid, hipStream_t st, const DevModel* m, const KParams& kt, const KParams& kq,
                             const IO& io, const ReachPathArgs& rp, const StageIn& si);
// one round of the stepwise path: verdict, waypoint advance (gathering the new
// target into cur_xt / cur_xdt) or state update of every instance still
// active, from the stage outputs pose [12][B] / dist [1+dof][B] at the state
// in re.qf / re.vf and the round's eta [na][B] / status / iters.  first: the
// call's first round (dist_min starts at +inf); last: no QP ran
int launch_reach_path_update_kernel(int64_t B, hipStream_t st, const DevModel* m, int first, int last,
                                    const ReachPathArgs& rp, const double* pose, const double* dist,
                                    const double* eta, const int32_t* status, const int32_t* iters);

}  // namespace drc_amd
