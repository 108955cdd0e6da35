// Host-side launchers of the kernel translation units (task_kernel.hip,
// qp_kernel.hip, qpid_kernel.hip), called by the C-ABI in api.cpp.  Each
// returns the hipError_t of its launch (0 = hipSuccess).
#pragma once

#include <hip/hip_runtime.h>

#include "kernel_common.hpp"

namespace drc_amd {

// task_kernel<problem>: 0 QPIK stage, 1 QPID stage, 2 closed-form CLIK / OSF
// mesh: the model has convex-hull geometry (problems 0 and 1 then run the
// build with the hull narrow phase; 2 has no distance stage)
int launch_task_kernel(int problem, unsigned grid, size_t lds, hipStream_t st, const DevModel* m, const KParams& kp,
                       const IO& io, bool mesh = false);
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
// mesh: the build with the hull narrow phase, as for launch_task_kernel
int launch_fused_kernel(unsigned grid, size_t lds, hipStream_t st, const DevModel* m, const KParams& kt,
                        const KParams& kq, const IO& io, bool mesh = false);
// the builds for models with obstacle slots (task_obstacle_kernel.hip,
// fused_obstacle_kernel.hip): the QPIK stage and the fused kernel with
// task_instance<0, false, OBST = true>, ob the call's poses
int launch_task_obstacle_kernel(unsigned grid, size_t lds, hipStream_t st, const DevModel* m, const KParams& kp,
                                const IO& io, const ObstIn& ob);
int launch_fused_obstacle_kernel(unsigned grid, size_t lds, hipStream_t st, const DevModel* m, const KParams& kt,
                                 const KParams& kq, const IO& io, const ObstIn& ob);
// ... and for moving slots (task_rate_kernel.hip, fused_rate_kernel.hip):
// task_instance<0, false, OBST = true, RATE = true>, rt the call's twists
int launch_task_rate_kernel(unsigned grid, size_t lds, hipStream_t st, const DevModel* m, const KParams& kp,
                            const IO& io, const ObstIn& ob, const RateIn& rt);
int launch_fused_rate_kernel(unsigned grid, size_t lds, hipStream_t st, const DevModel* m, const KParams& kt,
                             const KParams& kq, const IO& io, const ObstIn& ob, const RateIn& rt);

// persistent rollout kernel (rollout_kernel.hip; compiled QPIK shapes,
// hipErrorInvalidValue otherwise): per instance `steps` times task stage, QP
// and state update.  io as for launch_fused_kernel, with out / status / iters
// the [steps][...] trajectories (out_step doubles between two steps' io.out);
// qf / vf [dof][B] hold the state between steps; q_traj, pose_traj, dist_traj
// may be NULL.  The LDS size follows from kt and kq
int launch_rollout_kernel(unsigned grid, hipStream_t st, const DevModel* m, const KParams& kt, const KParams& kq,
                          const IO& io, int steps, int per_step, double dt, double* qf, double* vf, double* q_traj,
                          double* pose_traj, double* dist_traj, int64_t out_step, bool mesh);
// one rollout step's state update for the stepwise path: v = S(q_in) eta,
// qf = q_in + dt v (q_in may be qf), also into q_traj unless NULL
int launch_rollout_integrate_kernel(int64_t B, hipStream_t st, const DevModel* m, double dt, const double* q_in,
                                    const double* eta, double* qf, double* vf, double* q_traj);

// drc_qpik_reach_batch (reach_kernel.hip): what its kernels need beyond IO.
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
// persistent reach kernel (compiled QPIK shapes without hulls or obstacle
// slots, hipErrorInvalidValue otherwise): per instance task stage, verdict, QP
// and state update until it stops.  io as for launch_fused_kernel, with out /
// status / iters one step's scratch (all three required) and xt the target.
// The LDS size follows from kt and kq
int launch_reach_kernel(unsigned grid, hipStream_t st, const DevModel* m, const KParams& kt, const KParams& kq,
                        const IO& io, const ReachArgs& re);
// step k of the stepwise path: the verdict of every instance still active from
// the stage outputs pose [12][B] / dist [1+dof][B] at the state in re.qf /
// re.vf, then (last = 0) the step's status and the state update from eta
// [na][B]; last = 1: k = max_steps, no QP ran (eta, status, iters unused)
int launch_reach_update_kernel(int64_t B, hipStream_t st, const DevModel* m, int k, int last, const ReachArgs& re,
                               const double* xt, const double* pose, const double* dist, const double* eta,
                               const int32_t* status, const int32_t* iters);

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
