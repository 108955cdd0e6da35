// The QPIK task stage for models with obstacle slots (drc_model_set_obstacles):
// task_kernel.hip's wave-per-instance kernel with task_instance<0, false,
// OBST = true>, whose obstacle lanes load their geometry's pose from the call's
// array and whose pass 1 decides half-space pairs in closed form
// (task_stage.hpp, halfspace.hpp) -- and, with DRC_TASK_RATE defined
// (task_rate_kernel.hip), with RATE = true as well: the slots move.  Translation
// units of their own, so that task_kernel.hip and each other compile to what
// they were.  Both register budgets of the plain QPIK stage: two and three
// waves per SIMD (task_waves_per_simd).  Reference: no counterpart.
#include "task_stage.hpp"
#include "launch.hpp"

namespace drc_amd {

#ifndef DRC_TASK_WAVES
#define DRC_TASK_WAVES 2
#endif
// OB: one ObstIn, the call's poses (task_stage.hpp OBST), or that and one
// RateIn, the slots' twists (RATE) -- a pack, as fused_kernel's
template <int WAVES, class... OB>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(WAVES, 8)))
task_obstacle_kernel(const DevModel* __restrict__ M0, const KParams kp, const IO io, const OB... ob) {
  extern __shared__ __attribute__((aligned(16))) double S[];
  PH_KSCOPE();
  static_assert(sizeof...(OB) == 1 || sizeof...(OB) == 2, "one set of obstacle poses, at most one of twists");
  const int64_t B = io.B;
  const InstSeq seq(B, kp.xcd_map, io.queue);
  for (int64_t j = seq.first(); j < seq.n; j = seq.next(j)) {
    const int64_t jj = seq.at(j);
    if (jj >= B) continue;
    const int64_t b = io.ordered(jj);
    stage_stamp(io, ST_TASK0, io.b0 + b);
    stage_where(io, ST_WTASK, io.b0 + b);
    task_instance<0, false, true, sizeof...(OB) == 2>(M0, kp, io, S, b, ob...);
    stage_stamp(io, ST_TASK1, io.b0 + b);
  }
}

template <class... OB>
static int launch_slots(unsigned grid, size_t lds, hipStream_t st, const DevModel* m, const KParams& kp, const IO& io,
                        const OB&... ob) {
  if (task_waves_per_simd(0, lds) == 3 && DRC_TASK_WAVES != 3)
    hipLaunchKernelGGL((task_obstacle_kernel<3, OB...>), dim3(grid), dim3(64), lds, st, m, kp, io, ob...);
  else
    hipLaunchKernelGGL((task_obstacle_kernel<DRC_TASK_WAVES, OB...>), dim3(grid), dim3(64), lds, st, m, kp, io, ob...);
  return hipGetLastError();
}

// (task_kernel.hip's launch_task_kernel declares and calls them)
#if defined(DRC_TASK_RATE)
int launch_task_rate_kernel(unsigned grid, size_t lds, hipStream_t st, const DevModel* m, const KParams& kp,
                            const IO& io, const ObstIn& ob, const RateIn& rt) {
  return launch_slots(grid, lds, st, m, kp, io, ob, rt);
}
#else
int launch_task_obstacle_kernel(unsigned grid, size_t lds, hipStream_t st, const DevModel* m, const KParams& kp,
                                const IO& io, const ObstIn& ob) {
  return launch_slots(grid, lds, st, m, kp, io, ob);
}
#endif

}  // namespace drc_amd
