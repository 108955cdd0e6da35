// Certified path clearance (drc_clearance_certify_batch): the continuous check
// of joint-space paths by adaptive bisection (clearance_certify.hpp).
// Reference: no counterpart.
//
// certify_kernel: clearance_kernel's shape -- a persistent grid with the work
// queue, one path per wave, the distance stage alone (task_instance<3>) on every
// state that is evaluated, d and pair read from the plan (SC_DIST, SC_PAIR)
// between two wave barriers.  What differs is which states: the fold of
// clearance_certify.hpp asks for them, one after the other, and a segment costs
// the evaluations its certificate needs, not a fixed number.
//   - Lane l < nv holds coordinate l of the segment's two ends and writes the
//     evaluated state's into the plan's kq.  The waypoint after the segment is
//     loaded when the segment starts, ahead of all its evaluations.
//   - The segment's motion bound M is formed once, at its start: the lanes
//     stride the pairs, |dq_i| comes from lane i by a uniform-index lane read,
//     the sum runs in ascending i with every product and sum rounded, and a wave
//     max reduces it (exact).  A few dozen FP64 operations per lane.
//   - The right ends that wait for their turn (the depth-first stack) live in
//     one register, lane e holding depth e: a push is a predicated move, a pop a
//     lane read with a uniform index.  No LDS: the plan is the task stage's.
//   - The fold's state is the same in every lane; what it answers goes through
//     readfirstlane, and every stop is a uniform branch that leaves the walk.
//
// This unit holds the Plain build; certify_mesh_kernel.hip and
// certify_obstacle_kernel.hip include it with DRC_CERT_MESH / DRC_CERT_OBST
// defined and hold the other two.
#include "task_stage.hpp"
#include "clearance_certify.hpp"
#include "launch.hpp"

namespace drc_amd {

// the fold's stack in the lanes of one register (depth <= kCertMaxDepth < 64)
struct CertStackLanes {
  int l;
  double v;
  __device__ __forceinline__ void push(int32_t level, double x) {
    if (l == level) v = x;
  }
  __device__ __forceinline__ double pop(int32_t level) const { return rd_lane(v, __builtin_amdgcn_readfirstlane(level)); }
};

template <int WAVES, bool MESH, class... OB>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(WAVES, 8)))
certify_kernel(const DevModel* __restrict__ M0, const KParams kp, const IO io, const CertArgs ca, const OB... ob) {
  extern __shared__ __attribute__((aligned(16))) double S[];
  PH_KSCOPE();
  static_assert(sizeof...(OB) <= 1 && !(MESH && sizeof...(OB)), "at most one set of obstacle poses, not with hulls");
  const int l = lane_id();
  const int64_t B = io.B, LD = io.ld;
  const int nv = kp.nv, W = ca.waypoints;
  const int64_t wp = static_cast<int64_t>(nv) * LD;  // one waypoint of q_path
  const int npairs = M0->npairs, wld = M0->motion_ld;
  const double* __restrict__ wt = M0->motion_wt;
  // this lane's coordinate: is it one whose travel the weights assume, and how far
  const bool bounded = l < nv && (M0->travel_mask >> l & 1u) != 0;
  const double travel = l < nv ? fmax(fabs(M0->lower[l]), fabs(M0->upper[l])) : 0.0;
  double* qv = S + kp.kq;
  const InstSeq seq(B, kp.xcd_map, io.queue);
  for (int64_t j = seq.first(); j < seq.n; j = seq.next(j)) {
    const int64_t b = seq.at(j);
    if (b >= B) continue;
    const int64_t gb = io.b0 + b;
    // this lane's coordinate of the path (lanes past nv read coordinate 0 and drop it)
    const double* qp = ca.q_path + static_cast<int64_t>(l < nv ? l : 0) * LD + gb;
    double qa = qp[0], qb = W > 1 ? qp[wp] : qa, qn = qb;
    CertFold f;
    CertStackLanes stack{l, 0.0};
    double Mseg = 0.0;
    int seg = 0;  // the segment that starts next
    for (;;) {
      if (l < nv) qv[l] = f.ev_k == 0 ? qa : clearance_sample(qa, qb, f.ev_k, 1 << f.ev_e);
      task_instance<3, MESH, sizeof...(OB) != 0>(M0, kp, io, S, b, ob...);
      // (the stage ends on a wave barrier: its result is in the plan)
      const double d = S[kp.oSc + SC_DIST];
      const int pr = static_cast<int>(S[kp.oSc + SC_PAIR]);
      int next = __builtin_amdgcn_readfirstlane(
          cert_step(&f, stack, d, pr < npairs ? pr : -1, ca.d_stop, Mseg, ca.max_depth));
      if (next == kCertStop) break;
      if (next == kCertSegEnd) {
        if (seg + 1 >= W) break;  // the last segment, or a path of one waypoint: FREE
        if (seg > 0) {
          qa = qb;
          qb = qn;
        }
        if (seg + 2 < W) qn = qp[static_cast<int64_t>(seg + 2) * wp];  // in flight during the segment's stages
        const bool ok = !bounded || cert_travel_ok(qa, qb, travel);
        const bool travel_ok = __builtin_amdgcn_ballot_w64(!ok) == 0;
        const double adq = l < nv ? fabs(qb - qa) : 0.0;
        double m = 0.0;
        for (int p = l; p < npairs; p += 64) {
          double s = 0.0;
          for (int i = 0; i < nv; ++i) s = cert_motion_term(s, wt[i * wld + p], rd_lane(adq, i));
          m = s > m ? s : m;
        }
        Mseg = wave_max(m);
        if (ca.motion_bound && l == 0) ca.motion_bound[static_cast<int64_t>(seg) * LD + gb] = Mseg;
        next = __builtin_amdgcn_readfirstlane(cert_segment(&f, seg, travel_ok));
        if (next == kCertStop) break;
        ++seg;
      }
      wsync();  // every lane has read d and pair before the next stage writes them
    }
    if (l == 0) {
      ca.result[gb] = f.result;
      ca.seg_stop[gb] = f.seg_stop;
      ca.t_stop[gb] = f.t_stop;
      ca.d_min[gb] = f.d_min;
      ca.seg_min[gb] = f.seg_min;
      ca.t_min[gb] = f.t_min;
      ca.pair_min[gb] = f.pair_min;
      ca.d_lower[gb] = f.d_lower;
      ca.samples_used[gb] = f.samples;
    }
    wsync();
  }
}

// Register budget and grid: clearance_kernel's (DRC_CLEAR_WAVES, three waves
// per SIMD for the Plain and Obst builds, two for hulls; the grid is
// call_plan.hpp clearance_grid) -- the same stage on the same shape of work
#ifndef DRC_CLEAR_WAVES
#define DRC_CLEAR_WAVES 3
#endif

#if defined(DRC_CERT_MESH)
int launch_certify_mesh_kernel(unsigned grid, size_t lds, hipStream_t st, const DevModel* m, const KParams& kp,
                               const IO& io, const CertArgs& ca) {
  hipLaunchKernelGGL((certify_kernel<2, true>), dim3(grid), dim3(64), lds, st, m, kp, io, ca);
  return hipGetLastError();
}
#elif defined(DRC_CERT_OBST)
int launch_certify_obstacle_kernel(unsigned grid, size_t lds, hipStream_t st, const DevModel* m, const KParams& kp,
                                   const IO& io, const CertArgs& ca, const ObstIn& ob) {
  hipLaunchKernelGGL((certify_kernel<DRC_CLEAR_WAVES, false, ObstIn>), dim3(grid), dim3(64), lds, st, m, kp, io, ca, ob);
  return hipGetLastError();
}
#else
int launch_certify_mesh_kernel(unsigned grid, size_t lds, hipStream_t st, const DevModel* m, const KParams& kp,
                               const IO& io, const CertArgs& ca);
int launch_certify_obstacle_kernel(unsigned grid, size_t lds, hipStream_t st, const DevModel* m, const KParams& kp,
                                   const IO& io, const CertArgs& ca, const ObstIn& ob);

int launch_certify_kernel(unsigned grid, size_t lds, hipStream_t st, const DevModel* m, const KParams& kp,
                          const IO& io, const CertArgs& ca, const StageIn& si) {
  if (!has_build(StageFamily::Clearance, si.build)) return hipErrorInvalidValue;  // (Rate: the slots are static)
  switch (si.build) {
    case StageBuild::Mesh: return launch_certify_mesh_kernel(grid, lds, st, m, kp, io, ca);
    case StageBuild::Obst: return launch_certify_obstacle_kernel(grid, lds, st, m, kp, io, ca, si.ob);
    case StageBuild::Plain:
      hipLaunchKernelGGL((certify_kernel<DRC_CLEAR_WAVES, false>), dim3(grid), dim3(64), lds, st, m, kp, io, ca);
      return hipGetLastError();
    default: return hipErrorInvalidValue;
  }
}
#endif

}  // namespace drc_amd
