// Goal-reaching rollouts with per-instance stopping, through waypoints
// (drc_qpik_reach_path_batch; drc_qpik_reach_batch is the path of one
// waypoint): the closed loop of drc_qpik_rollout_batch in mode QPIKStep
// towards waypoint w of x_path [W][12][B], where every instance stops on its
// own -- the step budget of the segment is spent, or its QP is not solved
// (eta = 0: it would stay where it is) -- and an instance that comes within
// the tolerances of waypoint w (reach.hpp) goes on to waypoint w + 1 from the
// same state, with a fresh step budget, and stops once it has passed the last
// one.  Bit for bit W chained drc_qpik_reach_batch calls, without the call
// boundaries: a wave leaves an instance the moment it stops.  Reference: no
// counterpart.
//
// reach_path_kernel: the persistent form for the compiled QP shapes: one
// instance per wave from the work queue, the task record in LDS, the state in
// the caller's q_final / qdot_final arrays, the update scratch at the start of
// the plan.  The waypoint index, both step counters and the verdict are
// wave-uniform, so the stops and the waypoint advance are uniform branches.
// The kernel body is written out in full, the blocks of closed_loop.hpp
// included (the same text as there): through the header's functions, with
// equal registers, scratch and spills, the FR3 build measured 1.3 to 1.8 %
// slower than it was (profiles/closed_loop_refactor_ab.jsonl), so this kernel
// keeps the text it had.  OB: empty, or one ObstIn -- the build for models with
// obstacle slots (reach_path_obstacle_kernel.hip), as fused_kernel's.
//
// reach_path_update_kernel: verdict, advance and state update alone, one
// thread per instance, for the stepwise path (api.cpp).  Both forms go through
// the same functions of closed_loop.hpp (reach.hpp's and rollout_update.hpp's
// arithmetic) on the same values, so the two paths return identical bits
// (tests/test_gpu_reach_path.py).
#include "task_stage.hpp"
#include "qp_solver.hpp"
#include "reach_path.hpp"
#include "closed_loop.hpp"

namespace drc_amd {

template <class QD, class... OB>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(DRC_FUSED_WAVES, 8)))
reach_path_kernel(const DevModel* __restrict__ M0, const KParams kt, const KParams kq, const IO io,
                  const ReachPathArgs rp, const OB... ob) {
  extern __shared__ __attribute__((aligned(16))) double S[];
  PH_KSCOPE();
  __shared__ KParams kpl;  // LDS copy of the QP parameters for the out-of-line ADMM blocks
  {
    static_assert(sizeof(KParams) % 8 == 0, "KParams copied as 8-byte words");
    const uint64_t* src = reinterpret_cast<const uint64_t*>(&kq);
    uint64_t* dst = reinterpret_cast<uint64_t*>(&kpl);
    for (int e = lane_id(); e < static_cast<int>(sizeof(KParams) / 8); e += 64) dst[e] = src[e];
    wsync();
  }
  static_assert(sizeof...(OB) <= 1, "at most one set of obstacle poses");
  const ReachArgs& re = rp.re;
  const int l = lane_id();
  const int64_t B = io.B, LD = io.ld;
  const int nv = kt.nv, na = kq.na, W = rp.W;
  IO iol = io;  // the record lives in LDS, as in fused_kernel
  iol.rec = S + fused_rec_offset(kt, kq);
  iol.rec_stride = 0;
  double* qs = S;  // (rollout_state_doubles: dead plan space)
  double* es = qs + ((nv + 1) & ~1);
  double(*Jm)[kMaxWheels] = reinterpret_cast<double(*)[kMaxWheels]>(es + ((na + 1) & ~1));
  const InstSeq seq(B, kq.xcd_map, io.queue);
  for (int64_t j = seq.first(); j < seq.n; j = seq.next(j)) {
    const int64_t b = seq.at(j);
    if (b >= B) continue;
    const int64_t gb = io.b0 + b;
    // k: steps of the whole call, s: of this segment, w: the waypoint ahead
    int k = 0, s = 0, w = 0, res = DRC_REACH_BUDGET, st_last = 0, it_total = 0;
    double dmin = __builtin_inf();
    for (;;) {
      IO is = iol;
      is.xt = rp.x_path + int64_t(w) * 12 * LD;
      is.xdt = rp.xdot_path + int64_t(w) * 6 * LD;
      if (k > 0) {
        is.q = re.qf;
        is.qdot = re.vf;
      }
      task_instance<0, false, sizeof...(OB) != 0>(M0, kt, is, S, b, ob...);
      wsync();
      {
        const double d = iol.rec[kt.rDist];  // (a NaN is never taken)
        if (d < dmin) dmin = d;
      }
      // the pose at q_k from the task plan (the pure copies of the stage entry's
      // pose output) against waypoint w and,
      // while it is within, against the next ones: every lane forms the same
      // numbers.  The record was formed against the waypoint the stage started
      // with, so an advance runs the stage again before the QP reads it
      const int w0 = w;
      double err[2];
      {
        const double* Te = S + kt.kTe;
        double ps[12], tg[12];
        for (int i = 0; i < 12; ++i) ps[i] = i < 9 ? Te[(i % 3) * 3 + i / 3] : Te[i];
        for (;;) {
          const double* xw = rp.x_path + int64_t(w) * 12 * LD + gb;
          for (int i = 0; i < 12; ++i) tg[i] = xw[i * LD];
          reach_error(ps, tg, err);
          if (!__builtin_amdgcn_readfirstlane(reach_within(err, re.tau_p, re.tau_r) ? 1 : 0)) break;
          if (rp.steps_at && l == 0) rp.steps_at[int64_t(w) * LD + gb] = k;
          ++w;
          s = 0;
          if (w == W) break;
        }
      }
      // what stands there when the instance stops is the value at q_final (a
      // QP that fails leaves the state where this stage ran)
      if (re.err_final && l < 2) re.err_final[l * LD + gb] = l ? err[1] : err[0];
      if (re.dist_final && l <= nv) re.dist_final[l * LD + gb] = iol.rec[kt.rDist + l];
      if (w == W) {
        res = DRC_REACH_REACHED;
        break;
      }
      if (w != w0) {  // the same state, the new target
        wsync();
        continue;
      }
      if (s == re.max_steps) {
        res = DRC_REACH_BUDGET;
        break;
      }
      wsync();
      qp_instance<QD>(M0, kq, kpl, is, S, b);
      // ---------------- this step's status, wave-uniform ----------------------
      state_visible();
      st_last = __builtin_amdgcn_readfirstlane(
          __hip_atomic_load(is.status + gb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
      it_total += __builtin_amdgcn_readfirstlane(
          __hip_atomic_load(is.iters + gb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
      if (st_last != DRC_STATUS_SOLVED) {
        res = DRC_REACH_QP_FAILED;
        break;
      }
      // ---------------- state update (as rollout_kernel) ----------------------
      const double qk = l < nv ? is.q[l * LD + gb] : 0.0;  // step 0: the caller's q0 (q_final may alias it)
      if (l < nv) qs[l] = qk;
      if (l < na) es[l] = is.out[l * LD + gb];
      wsync();
      const DevModel* M = opaque_model(M0);
      double cy = 1, sy = 0;
      if (M->kind == 1) {
        if (l == 0) mobile_fk(M, qs + M->mobi_start, Jm);
        const double yaw = qs[M->virtual_start + 2];
        cy = cos(yaw);
        sy = sin(yaw);
        wsync();
      }
      if (l < nv) {
        const double v = rollout_velocity(M, l, cy, sy, Jm, [&](int a) { return es[a]; });
        const double qn = rollout_advance(qk, re.dt, v);
        re.vf[l * LD + gb] = v;
        re.qf[l * LD + gb] = qn;
      }
      state_visible();
      wsync();
      ++k;
      ++s;
    }
    // stopped at (q_k, v_k): from step 1 on the finals hold it
    if (k == 0 && l < nv) {
      const double q0 = io.q[l * LD + gb], v0 = io.qdot[l * LD + gb];
      re.qf[l * LD + gb] = q0;
      re.vf[l * LD + gb] = v0;
    }
    if (rp.steps_at)  // the waypoints never reached
      for (int i = w + l; i < W; i += 64) rp.steps_at[int64_t(i) * LD + gb] = -1;
    if (l == 0) {
      re.result[gb] = res;
      re.steps_used[gb] = k;
      rp.waypoints_reached[gb] = w;
      if (re.status_last) re.status_last[gb] = st_last;
      if (re.iters_total) re.iters_total[gb] = it_total;
      if (rp.dist_min) rp.dist_min[gb] = dmin;
    }
    wsync();
  }
}

template <class... OB>
static int launch_shapes(unsigned grid, hipStream_t st, const DevModel* m, const KParams& kt, const KParams& kq,
                         const IO& io, const ReachPathArgs& rp, const OB&... ob) {
  const size_t lds = closed_loop_lds_bytes(kt, kq);
  const dim3 g(grid), blk(64);
  if (int r = with_compiled_shape(kq.nx, kq.ng, kq.np, [&](auto qd) {
        hipLaunchKernelGGL((reach_path_kernel<decltype(qd), OB...>), g, blk, lds, st, m, kt, kq, io, rp, ob...);
      }))
    return r;  // not a compiled shape: the stepwise path runs it
  return hipGetLastError();
}

// The builds for models with obstacle slots are a translation unit of their
// own (reach_path_obstacle_kernel.hip includes this file with
// DRC_REACH_PATH_OBST defined), as fused_obstacle_kernel.hip's.
#if defined(DRC_REACH_PATH_OBST)
int launch_reach_path_obstacle_kernel(unsigned grid, hipStream_t st, const DevModel* m, const KParams& kt,
                                      const KParams& kq, const IO& io, const ReachPathArgs& rp, const ObstIn& ob) {
  return launch_shapes(grid, st, m, kt, kq, io, rp, ob);
}
#else
int launch_reach_path_obstacle_kernel(unsigned grid, hipStream_t st, const DevModel* m, const KParams& kt,
                                      const KParams& kq, const IO& io, const ReachPathArgs& rp, const ObstIn& ob);
int launch_reach_path_kernel(unsigned grid, hipStream_t st, const DevModel* m, const KParams& kt, const KParams& kq,
                             const IO& io, const ReachPathArgs& rp, const StageIn& si) {
  switch (si.build) {
    case StageBuild::Plain: return launch_shapes(grid, st, m, kt, kq, io, rp);
    case StageBuild::Obst: return launch_reach_path_obstacle_kernel(grid, st, m, kt, kq, io, rp, si.ob);
    default: return hipErrorInvalidValue;  // (no build for hulls or twists)
  }
}

// Stepwise path, one round.  Instances that have stopped (result !=
// kReachActive) are skipped.  An active one takes its verdict from the stage
// outputs at its state -- pose [12][B], dist [1+nv][B] -- with steps_used,
// waypoints_reached and seg as its counters k, w and s.  If it advances without
// passing the last waypoint, it gathers waypoint w's target into cur_xt /
// cur_xdt and ignores the round's QP, which was formed against the old one.
// Otherwise, unless it stops, it takes the update from the round's eta /
// status / iters.  last: no QP ran (an instance still active by then has used
// its W max_steps steps and W - 1 advances, one per round: it stands before the
// last waypoint with seg == max_steps, and its verdict is REACHED or BUDGET).
// The state is updated in place (thread_state_update).
__global__ void __launch_bounds__(256)
reach_path_update_kernel(const DevModel* __restrict__ M, int64_t B, int first, int last, const ReachPathArgs rp,
                         const double* pose, const double* dist, const double* eta, const int32_t* status,
                         const int32_t* iters) {
  const int64_t b = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (b >= B) return;
  const ReachArgs& re = rp.re;
  if (re.result[b] != kReachActive) return;
  const int W = rp.W;
  if (rp.dist_min) {
    const double d = dist[b], m = first ? __builtin_inf() : rp.dist_min[b];
    rp.dist_min[b] = d < m ? d : m;
  }
  const int k = re.steps_used[b];
  int w = rp.waypoints_reached[b];
  const int w0 = w;
  double ps[12], tg[12], err[2];
  for (int i = 0; i < 12; ++i) ps[i] = pose[i * B + b];
  for (;;) {
    const double* xw = rp.x_path + int64_t(w) * 12 * B + b;
    for (int i = 0; i < 12; ++i) tg[i] = xw[i * B];
    reach_error(ps, tg, err);
    if (!reach_within(err, re.tau_p, re.tau_r)) break;
    if (rp.steps_at) rp.steps_at[int64_t(w) * B + b] = k;
    if (++w == W) break;
  }
  if (w != w0) {
    rp.waypoints_reached[b] = w;
    rp.seg[b] = 0;
  }
  int res = kReachActive;
  if (w == W) {
    res = DRC_REACH_REACHED;
  } else if (w != w0) {
    for (int i = 0; i < 12; ++i) rp.cur_xt[i * B + b] = rp.x_path[(int64_t(w) * 12 + i) * B + b];
    for (int i = 0; i < 6; ++i) rp.cur_xdt[i * B + b] = rp.xdot_path[(int64_t(w) * 6 + i) * B + b];
    return;
  } else if (rp.seg[b] == re.max_steps || last) {
    res = DRC_REACH_BUDGET;
  } else if (thread_step_status(re, b, status, iters) != DRC_STATUS_SOLVED) {
    res = DRC_REACH_QP_FAILED;
  }
  if (res != kReachActive) {  // stopped at (q_k, v_k); steps_used holds k
    re.result[b] = res;
    thread_store_at_state(M, re, B, b, err, dist);
    return;
  }
  thread_state_update(M, B, b, re.dt, re.qf, eta, re.qf, re.vf);
  re.steps_used[b] = k + 1;
  rp.seg[b] += 1;
}

int launch_reach_path_update_kernel(int64_t B, hipStream_t st, const DevModel* m, int first, int last,
                                    const ReachPathArgs& rp, const double* pose, const double* dist,
                                    const double* eta, const int32_t* status, const int32_t* iters) {
  hipLaunchKernelGGL(reach_path_update_kernel, dim3(static_cast<unsigned>((B + 255) / 256)), dim3(256), 0, st, m, B,
                     first, last, rp, pose, dist, eta, status, iters);
  return hipGetLastError();
}
#endif

}  // namespace drc_amd
