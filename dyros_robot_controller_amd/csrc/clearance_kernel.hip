// Path clearance (drc_clearance_path_batch): the minimum distance along
// joint-space paths, with a stop at the first sample below a threshold.
// Reference: no counterpart (its getMinDistance answers one state).
//
// clearance_kernel: a persistent grid with the work queue, one path per wave.
// The wave walks the path's samples (clearance.hpp) in order and runs the
// distance stage alone on each -- task_instance<3> (task_stage.hpp): FK chain,
// geometry poses, pass 1, candidate passes, EPA, the winner's refinement; d and
// pair are bit for bit dist[0] and pair of drc_qpik_stages_batch at that state.
// Lane l < nv holds coordinate l of the segment's two ends and writes the
// sample's into the plan's kq, so a sample costs no global round trip; the next
// waypoint's load is issued before the segment's last sample, whose stage
// hides it.  The rule's state is the same in every lane (all read d and pair
// from the plan), the verdict goes through readfirstlane, and the three stops
// -- INVALID, BLOCKED, the path's end -- are uniform branches that leave the
// sample loop; the wave then takes the next path from the queue.  A path costs
// the samples up to its stop, not N.
//
// This unit holds the Plain build; clearance_mesh_kernel.hip and
// clearance_obstacle_kernel.hip include it with DRC_CLEAR_MESH /
// DRC_CLEAR_OBST defined and hold the other two.
#include "task_stage.hpp"
#include "clearance.hpp"
#include "launch.hpp"

namespace drc_amd {

template <int WAVES, bool MESH, class... OB>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(WAVES, 8)))
clearance_kernel(const DevModel* __restrict__ M0, const KParams kp, const IO io, const ClearArgs ca, const OB... ob) {
  extern __shared__ __attribute__((aligned(16))) double S[];
  PH_KSCOPE();
  static_assert(sizeof...(OB) <= 1 && !(MESH && sizeof...(OB)), "at most one set of obstacle poses, not with hulls");
  const int l = lane_id();
  const int64_t B = io.B, LD = io.ld;
  const int nv = kp.nv, W = ca.waypoints, sub = ca.substeps;
  const int32_t n_last = static_cast<int32_t>(clearance_samples(W, sub) - 1);
  const int64_t wp = static_cast<int64_t>(nv) * LD;  // one waypoint of q_path
  const int npairs = M0->npairs;
  double* qv = S + kp.kq;
  const InstSeq seq(B, kp.xcd_map, io.queue);
  for (int64_t j = seq.first(); j < seq.n; j = seq.next(j)) {
    const int64_t b = seq.at(j);
    if (b >= B) continue;
    const int64_t gb = io.b0 + b;
    // this lane's coordinate of the path (lanes past nv read coordinate 0 and drop it)
    const double* qp = ca.q_path + static_cast<int64_t>(l < nv ? l : 0) * LD + gb;
    double qa = qp[0], qb = W > 1 ? qp[wp] : qa, qn = qb;
    ClearFold f;
    int seg = 0, i = 0;  // sample n = seg sub + i; i = 0 only at n = 0
    for (int32_t n = 0;; ++n) {
      const bool seg_end = i == sub;
      if (seg_end && seg + 2 < W) qn = qp[static_cast<int64_t>(seg + 2) * wp];  // in flight during the stage
      if (l < nv) qv[l] = n == 0 ? qa : clearance_sample(qa, qb, i, sub);
      task_instance<3, MESH, sizeof...(OB) != 0>(M0, kp, io, S, b, ob...);
      // (the stage ends on a wave barrier: its result is in the plan)
      const double d = S[kp.oSc + SC_DIST];
      const int pr = static_cast<int>(S[kp.oSc + SC_PAIR]);
      if (ca.dist_traj && l == 0) ca.dist_traj[static_cast<int64_t>(n) * LD + gb] = d;
      const bool stop = clearance_step(&f, n, d, pr < npairs ? pr : -1, ca.d_stop);
      if (__builtin_amdgcn_readfirstlane(stop ? 1 : 0) || n == n_last) break;
      if (seg_end) {
        qa = qb;
        qb = qn;
        ++seg;
        i = 1;
      } else {
        ++i;
      }
      wsync();  // every lane has read d and pair before the next sample's stage writes them
    }
    if (l == 0) {
      ca.result[gb] = f.result;
      ca.sample_stop[gb] = f.sample_stop;
      ca.d_min[gb] = f.d_min;
      ca.sample_min[gb] = f.sample_min;
      ca.pair_min[gb] = f.pair_min;
    }
    wsync();
  }
}

// Register budget: three waves per SIMD (the QPIK stage's 168-VGPR budget) for
// the Plain and Obst builds.  Budget and grid were swept together on FR3,
// B = 65 536, substeps 8, no stop (tools/bench_clearance.py --sweep on this
// library and a -DDRC_CLEAR_WAVES=2 one, profiles/clearance_grid.json, the
// numbers in DESIGN.md "Path clearance"): on 1 024 and 2 048 waves the
// two-wave build is 6 % faster, but three waves per SIMD are what lets a CU
// hold the waves of a 3 072-wave grid, and that pair is about 10 % faster than
// the best two-wave configuration and the fastest of the six.  Hull models
// keep two waves, as everywhere
#ifndef DRC_CLEAR_WAVES
#define DRC_CLEAR_WAVES 3
#endif

#if defined(DRC_CLEAR_MESH)
int launch_clearance_mesh_kernel(unsigned grid, size_t lds, hipStream_t st, const DevModel* m, const KParams& kp,
                                 const IO& io, const ClearArgs& ca) {
  hipLaunchKernelGGL((clearance_kernel<2, true>), dim3(grid), dim3(64), lds, st, m, kp, io, ca);
  return hipGetLastError();
}
#elif defined(DRC_CLEAR_OBST)
int launch_clearance_obstacle_kernel(unsigned grid, size_t lds, hipStream_t st, const DevModel* m, const KParams& kp,
                                     const IO& io, const ClearArgs& ca, const ObstIn& ob) {
  hipLaunchKernelGGL((clearance_kernel<DRC_CLEAR_WAVES, false, ObstIn>), dim3(grid), dim3(64), lds, st, m, kp, io, ca,
                     ob);
  return hipGetLastError();
}
#else
int launch_clearance_mesh_kernel(unsigned grid, size_t lds, hipStream_t st, const DevModel* m, const KParams& kp,
                                 const IO& io, const ClearArgs& ca);
int launch_clearance_obstacle_kernel(unsigned grid, size_t lds, hipStream_t st, const DevModel* m, const KParams& kp,
                                     const IO& io, const ClearArgs& ca, const ObstIn& ob);

int launch_clearance_kernel(unsigned grid, size_t lds, hipStream_t st, const DevModel* m, const KParams& kp,
                            const IO& io, const ClearArgs& ca, const StageIn& si) {
  if (!has_build(StageFamily::Clearance, si.build)) return hipErrorInvalidValue;  // (Rate: the slots are static)
  switch (si.build) {
    case StageBuild::Mesh: return launch_clearance_mesh_kernel(grid, lds, st, m, kp, io, ca);
    case StageBuild::Obst: return launch_clearance_obstacle_kernel(grid, lds, st, m, kp, io, ca, si.ob);
    case StageBuild::Plain:
      hipLaunchKernelGGL((clearance_kernel<DRC_CLEAR_WAVES, false>), dim3(grid), dim3(64), lds, st, m, kp, io, ca);
      return hipGetLastError();
    default: return hipErrorInvalidValue;
  }
}
#endif

}  // namespace drc_amd
