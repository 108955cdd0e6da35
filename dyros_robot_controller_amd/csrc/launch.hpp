// Host-side launchers of the kernel translation units, called by the C-ABI in
// api.cpp: the task stage (task_kernel.hip), the QP kernels (qp_kernel.hip,
// qp_dense_kernel.hip, qpid_kernel.hip), the fused kernel (fused_kernel.hip),
// the rollout and reach kernels (rollout_kernel.hip, reach_kernel.hip), the
// path-clearance kernel (clearance_kernel.hip) and the
// order kernel (order_kernel.hip); reach_path.hpp and reach_seeds.hpp declare
// those of their entries.  A family that contains the task stage has one
// launcher, which takes the call's StageIn and launches that build, from the
// family's own or a sibling unit (*_mesh_kernel.hip, *_obstacle_kernel.hip,
// *_rate_kernel.hip; call_plan.hpp has_build: which family has which).  Each
// returns the hipError_t of its launch (0 = hipSuccess).
#pragma once

#include <hip/hip_runtime.h>

#include "call_plan.hpp"
#include "kernel_common.hpp"

namespace drc_amd {

// What a launch of the task stage needs beyond IO: the build, and what the
// Obst and Rate builds' kernels take as arguments of their own
// (kernel_common.hpp) -- ob the call's poses, rt its twists
struct StageIn {
  StageBuild build = StageBuild::Plain;
  ObstIn ob;
  RateIn rt;
  // step k of a per-step set of nobst slots: poses [steps][nobst][12][ld] and
  // twists [steps][nobst][6][ld] (ld = 0: [steps][nobst][12 | 6])
  StageIn at_step(int k, int nobst) const {
    StageIn s = *this;
    if (ob.pose) s.ob.pose += int64_t(k) * nobst * 12 * (ob.ld ? ob.ld : 1);
    if (rt.twist) s.rt.twist += int64_t(k) * nobst * 6 * (rt.ld ? rt.ld : 1);
    return s;
  }
  // the same poses without their twists: the Obst build where this is the Rate build
  StageIn without_twists() const { return {build == StageBuild::Rate ? StageBuild::Obst : build, ob, RateIn()}; }
};

// task_kernel<problem>: 0 QPIK stage, 1 QPID stage, 2 closed-form CLIK / OSF;
// hipErrorInvalidValue for a build the problem does not have
int launch_task_kernel(int problem, unsigned grid, size_t lds, hipStream_t st, const DevModel* m, const KParams& kp,
                       const IO& io, const StageIn& si);
// register-budget waves per SIMD of the task build launch_task_kernel picks
// for a plan of `lds` bytes per wave, and of the QP kernel
int task_waves_per_simd(int problem, size_t lds);
int qp_waves_per_simd();
// lane-per-instance task stage (nv = 6 or 7)
int launch_lane_task_kernel(int nv, unsigned grid, hipStream_t st, const DevModel* m, const KParams& kp,
                            const IO& io);
// The QPIK shapes with compile-time instantiations (register Schur ADMM), once:
// calls f with the shape's Dims tag, or returns
// hipErrorInvalidValue for any other shape without calling it.  Every launcher
// of a compiled kernel dispatches through it, and qp_compiled() asks it
template <class F>
int with_compiled_shape(int nx, int ng, int np, F&& f) {
  if (nx == 23 && ng == 16 && np == 7)  // FR3
    f(Dims<23, 16, 7, true, true>{});
  else if (nx == 20 && ng == 14 && np == 6)  // UR5e
    f(Dims<20, 14, 6, true, true>{});
  else if (nx == 9 && ng == 16 && np == 9)  // Husky-FR3
    f(Dims<9, 16, 9, true, true>{});
  else if (nx == 11 && ng == 16 && np == 11)  // XLS-FR3
    f(Dims<11, 16, 11, true, true>{});
  else
    return hipErrorInvalidValue;
  return hipSuccess;
}
bool qp_compiled(int nx, int ng, int np);
// qp_kernel for kp's shape; lds = the QP plan
int launch_qp_kernel(unsigned grid, size_t lds, hipStream_t st, const DevModel* m, const KParams& kp, const IO& io);
// the two manipulator shapes' dense reference build (qp_dense_kernel.hip;
// hipErrorInvalidValue for any other shape)
int launch_qp_dense_kernel(unsigned grid, size_t lds, hipStream_t st, const DevModel* m, const KParams& kp,
                           const IO& io);
int launch_qpid_kernel(unsigned grid, size_t lds, hipStream_t st, const DevModel* m, const KParams& kp, const IO& io);
// fused task + QP kernel (compiled QPIK shapes; hipErrorInvalidValue otherwise);
// lds = both plans' maximum plus the record slot
int launch_fused_kernel(unsigned grid, size_t lds, hipStream_t st, const DevModel* m, const KParams& kt,
                        const KParams& kq, const IO& io, const StageIn& si);

// persistent rollout kernel (rollout_kernel.hip; compiled QPIK shapes in the
// Plain and Mesh builds, hipErrorInvalidValue otherwise): per instance `steps`
// times task stage, QP and state update.  io as for launch_fused_kernel, with out / status / iters
// the [steps][...] trajectories (out_step doubles between two steps' io.out);
// qf / vf [dof][B] hold the state between steps; q_traj, pose_traj, dist_traj
// may be NULL.  The LDS size follows from kt and kq
int launch_rollout_kernel(unsigned grid, hipStream_t st, const DevModel* m, const KParams& kt, const KParams& kq,
                          const IO& io, int steps, int per_step, double dt, double* qf, double* vf, double* q_traj,
                          double* pose_traj, double* dist_traj, int64_t out_step, const StageIn& si);
// one rollout step's state update for the stepwise path: v = S(q_in) eta,
// qf = q_in + dt v (q_in may be qf), also into q_traj unless NULL
int launch_rollout_integrate_kernel(int64_t B, hipStream_t st, const DevModel* m, double dt, const double* q_in,
                                    const double* eta, double* qf, double* vf, double* q_traj);

// The reach entries (drc_qpik_reach_batch and its kin; reach_path.hpp and
// reach_seeds.hpp have the others' launchers): what their kernels need beyond IO.
// tau_p, tau_r: the thresholds of reach.hpp; qf / vf [dof][B] hold the state;
// result / steps_used [B]; status_last, iters_total [B], err_final [2][B] and
// dist_final [1+dof][B] may be NULL
struct ReachArgs {
  int max_steps;
  double dt, tau_p, tau_r;
  double *qf, *vf;
  int32_t *result, *steps_used, *status_last, *iters_total;
  double *err_final, *dist_final;
};
// `result` of an instance that has not stopped yet (stepwise path; every byte 0xff)
constexpr int32_t kReachActive = -1;
// drc_qpik_reach_batch's persistent kernel (reach_kernel.hip; compiled QPIK
// shapes in the Plain build -- no hulls, no obstacle slots --
// hipErrorInvalidValue otherwise): per instance task stage, verdict, QP and
// state update until it stops.  io as for launch_fused_kernel, with out /
// status / iters one step's scratch (all three required) and xt the target.
// The LDS size follows from kt and kq
int launch_reach_kernel(unsigned grid, hipStream_t st, const DevModel* m, const KParams& kt, const KParams& kq,
                        const IO& io, const ReachArgs& re, const StageIn& si);
// (not called any more: reach_kernel.hip says why reach_update_kernel is still in its unit)
int launch_reach_update_kernel(int64_t B, hipStream_t st, const DevModel* m, int k, int last, const ReachArgs& re,
                               const double* xt, const double* pose, const double* dist, const double* eta,
                               const int32_t* status, const int32_t* iters);

// drc_clearance_path_batch (clearance_kernel.hip): what its kernel takes beyond
// IO, as an argument of its own (IO and KParams keep their size: DESIGN.md
// "Obstacle slots").  q_path [waypoints][dof][ld]; result, sample_stop, d_min,
// sample_min, pair_min [B]; dist_traj [N][ld] or NULL
struct ClearArgs {
  int waypoints, substeps;
  double d_stop;
  const double* q_path;
  int32_t *result, *sample_stop;
  double* d_min;
  int32_t *sample_min, *pair_min;
  double* dist_traj;
};
// persistent clearance kernel (the Plain, Mesh and Obst builds; any model, no
// QP shape involved; hipErrorInvalidValue for Rate): one path per wave from the
// work queue io.queue, the distance stage sample after sample until the rule
// of clearance.hpp stops the walk.  kp: the task plan (lds its bytes); of io it
// reads B, b0, ld and queue
int launch_clearance_kernel(unsigned grid, size_t lds, hipStream_t st, const DevModel* m, const KParams& kp,
                            const IO& io, const ClearArgs& ca, const StageIn& si);

// drc_clearance_certify_batch (certify_kernel.hip): what its kernel takes beyond
// IO, as an argument of its own, as ClearArgs is.  q_path [waypoints][dof][ld];
// every output [B]; motion_bound [waypoints - 1][ld] or NULL
struct CertArgs {
  int waypoints, max_depth;
  double d_stop;
  const double* q_path;
  int32_t *result, *seg_stop;
  double *t_stop, *d_min;
  int32_t* seg_min;
  double* t_min;
  int32_t* pair_min;
  double* d_lower;
  int32_t* samples_used;
  double* motion_bound;
};
// persistent certify kernel (the Plain, Mesh and Obst builds, as the clearance
// kernel's; hipErrorInvalidValue for Rate): one path per wave from the work
// queue io.queue, the distance stage on the states that the fold of
// clearance_certify.hpp asks for.  kp: the task plan (lds its bytes); of io it
// reads B, b0, ld and queue; the model's motion_wt must be uploaded
int launch_certify_kernel(unsigned grid, size_t lds, hipStream_t st, const DevModel* m, const KParams& kp,
                          const IO& io, const CertArgs& ca, const StageIn& si);

// queue order of one sub-batch (order_kernel.hip): penetration-prone
// instances first (*hot_n zeroed; hot_list [B], hot_flag [B] scratch), then the
// others in index order, into order[b0 .. b0 + B)
int launch_order_kernel(int64_t B, hipStream_t st, const DevModel* m, const IO& io, int* hot_n, int32_t* hot_list,
                        uint8_t* hot_flag, int32_t* order);

#ifdef DRC_PHASE_TIMING
// diagnostic build: add each unit's phase slots to out[96]
int phase_cycles_task(unsigned long long* out, int reset);
int phase_cycles_qp(unsigned long long* out, int reset);
int phase_cycles_qp_dense(unsigned long long* out, int reset);
int phase_cycles_qpid(unsigned long long* out, int reset);
int phase_cycles_fused(unsigned long long* out, int reset);
// ... and the QP kernels' histogram of polish reduced-KKT sizes to out[16]
int phase_cycles_qp_hist(unsigned long long* out, int reset);
int phase_cycles_qp_dense_hist(unsigned long long* out, int reset);
int phase_cycles_fused_hist(unsigned long long* out, int reset);
#endif

}  // namespace drc_amd
