// The QPIK task stage for models with obstacle slots whose slots move
// (drc_qpik_*moving_obstacles_batch with a twist): task_obstacle_kernel.hip's
// kernel with task_instance<0, false, OBST = true, RATE = true>, whose obstacle
// lanes also load their slot's twist and whose distance for the QP carries the
// winner's dd/dt (task_stage.hpp).  A translation unit of its own, so that
// task_obstacle_kernel.hip compiles to what it was without it.  Both register
// budgets, as there.  Reference: no counterpart.
#include "task_stage.hpp"
#include "launch.hpp"

namespace drc_amd {

#ifndef DRC_TASK_WAVES
#define DRC_TASK_WAVES 2
#endif
template <int WAVES>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(WAVES, 8)))
task_rate_kernel(const DevModel* __restrict__ M0, const KParams kp, const IO io, const ObstIn ob, const RateIn rt) {
  extern __shared__ __attribute__((aligned(16))) double S[];
  PH_KSCOPE();
  const int64_t B = io.B;
  const InstSeq seq(B, kp.xcd_map, io.queue);
  for (int64_t j = seq.first(); j < seq.n; j = seq.next(j)) {
    const int64_t jj = seq.at(j);
    if (jj >= B) continue;
    const int64_t b = io.ordered(jj);
    stage_stamp(io, ST_TASK0, io.b0 + b);
    stage_where(io, ST_WTASK, io.b0 + b);
    task_instance<0, false, true, true>(M0, kp, io, S, b, ob, rt);
    stage_stamp(io, ST_TASK1, io.b0 + b);
  }
}

int launch_task_rate_kernel(unsigned grid, size_t lds, hipStream_t st, const DevModel* m, const KParams& kp,
                            const IO& io, const ObstIn& ob, const RateIn& rt) {
  if (task_waves_per_simd(0, lds) == 3 && DRC_TASK_WAVES != 3)
    hipLaunchKernelGGL(task_rate_kernel<3>, dim3(grid), dim3(64), lds, st, m, kp, io, ob, rt);
  else
    hipLaunchKernelGGL(task_rate_kernel<DRC_TASK_WAVES>, dim3(grid), dim3(64), lds, st, m, kp, io, ob, rt);
  return hipGetLastError();
}

}  // namespace drc_amd
