// drc_qpik_reach_batch's persistent kernel.  The entry runs as a reach path of
// one waypoint (api.cpp reach_path_locked; reach_path_kernel.hip has the loop's
// description and the stepwise path's update kernel) and keeps this kernel for
// its persistent launch: with W = 1 reach_path_kernel makes the same stops in
// the same order from the same values, but under the same host code it
// measured 0.6 to 1.1 % slower on FR3 (DESIGN.md "Reach entries unified").
//
// reach_kernel: one instance per wave from the work queue, the task record in
// LDS, the state in the caller's q_final / qdot_final arrays.  The verdict is
// wave-uniform, so the three stops are uniform branches that leave the step
// loop, and the wave takes the next instance from the queue: an instance costs
// the steps it needs, not the horizon.  Its own here: the step loop with the
// three stops; the blocks between them -- LDS views, the stores at the state,
// status read-back, state update, epilogue -- are closed_loop.hpp's, which
// reach_seeds_kernel calls too (rollout_kernel and reach_path_kernel keep the
// same blocks as their own text).  The same functions of closed_loop.hpp as
// reach_path_update_kernel (reach.hpp's and rollout_update.hpp's arithmetic)
// on the same values, so the two paths return identical bits
// (tests/test_gpu_reach.py).
//
// reach_update_kernel: the stepwise update of one target, which nothing
// launches any more (reach_path_update_kernel with W = 1 took its place).  Its
// text stays for one measured reason: without it every function of this unit
// moves up in the code object, and reach_kernel, its instructions unchanged,
// ran 0.4 to 1.0 % slower on FR3; aligning the kernels to 1 or 4 KiB did not
// bring it back (DESIGN.md "Reach entries unified").  It goes with
// reach_kernel, or once the placement is understood.
#include "task_stage.hpp"
#include "qp_solver.hpp"
#include "closed_loop.hpp"

namespace drc_amd {

// (ReachArgs: launch.hpp.  io.out / io.status / io.iters of the persistent
// kernel are one step's scratch: eta [na][B], status [B], iters [B])

// Stepwise path.  Instances that have stopped (result != kReachActive) are
// skipped; an active one takes step k's verdict from the stage outputs at
// (q_k, v_k) -- pose [12][B], dist [1+nv][B] -- and, unless it stops, the
// update from that step's eta / status / iters.  last: k = max_steps, no QP ran.
// The state is updated in place (thread_state_update).
__global__ void __launch_bounds__(256)
reach_update_kernel(const DevModel* __restrict__ M, int64_t B, int k, int last, const ReachArgs re, const double* xt,
                    const double* pose, const double* dist, const double* eta, const int32_t* status,
                    const int32_t* iters) {
  const int64_t b = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (b >= B) return;
  if (re.result[b] != kReachActive) return;
  double ps[12], tg[12], err[2];
  for (int i = 0; i < 12; ++i) {
    ps[i] = pose[i * B + b];
    tg[i] = xt[i * B + b];
  }
  reach_error(ps, tg, err);
  int res = kReachActive;
  if (reach_within(err, re.tau_p, re.tau_r)) {
    res = DRC_REACH_REACHED;
  } else if (last) {
    res = DRC_REACH_BUDGET;
  } else if (thread_step_status(re, b, status, iters) != DRC_STATUS_SOLVED) {
    res = DRC_REACH_QP_FAILED;
  }
  if (res != kReachActive) {  // stopped at (q_k, v_k)
    re.result[b] = res;
    re.steps_used[b] = k;
    thread_store_at_state(M, re, B, b, err, dist);
    return;
  }
  thread_state_update(M, B, b, re.dt, re.qf, eta, re.qf, re.vf);
}

template <class QD>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(DRC_FUSED_WAVES, 8)))
reach_kernel(const DevModel* __restrict__ M0, const KParams kt, const KParams kq, const IO io, const ReachArgs re) {
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
  const int l = lane_id();
  const int64_t B = io.B, LD = io.ld;
  const int nv = kt.nv, na = kq.na;
  const ClosedLoopLds cl(io, S, kt, kq);
  const InstSeq seq(B, kq.xcd_map, io.queue);
  for (int64_t j = seq.first(); j < seq.n; j = seq.next(j)) {
    const int64_t b = seq.at(j);
    if (b >= B) continue;
    const int64_t gb = io.b0 + b;
    int k = 0, res = DRC_REACH_BUDGET, st_last = 0, it_total = 0;
    for (;;) {
      IO is = step_io(cl.io, k, re.qf, re.vf);
      task_instance<0, false>(M0, kt, is, S, b);
      wsync();
      // the pose at q_k from the task plan (the pure copies of the stage entry's
      // pose output) against the target: every lane forms the same two numbers
      double err[2];
      {
        const double* Te = S + kt.kTe;
        double ps[12], tg[12];
        for (int i = 0; i < 12; ++i) {
          ps[i] = plan_pose(Te, i);
          tg[i] = io.xt[i * LD + gb];
        }
        reach_error(ps, tg, err);
      }
      store_at_state(re, cl.io.rec + kt.rDist, gb, LD, l, nv, err);
      const int within = __builtin_amdgcn_readfirstlane(reach_within(err, re.tau_p, re.tau_r) ? 1 : 0);
      if (within) {
        res = DRC_REACH_REACHED;
        break;
      }
      if (k == re.max_steps) {
        res = DRC_REACH_BUDGET;
        break;
      }
      wsync();
      qp_instance<QD>(M0, kq, kpl, is, S, b);
      step_status(is, gb, st_last, it_total);
      if (st_last != DRC_STATUS_SOLVED) {
        res = DRC_REACH_QP_FAILED;
        break;
      }
      wave_state_update(M0, is, gb, LD, l, nv, na, re.dt, re.qf, re.vf, cl);
      ++k;
    }
    reach_finals(io, re, gb, LD, l, nv, k);
    if (l == 0) reach_outcome(re, gb, k, res, st_last, it_total);
    wsync();
  }
}

int launch_reach_kernel(unsigned grid, hipStream_t st, const DevModel* m, const KParams& kt, const KParams& kq,
                        const IO& io, const ReachArgs& re, const StageIn& si) {
  if (!has_build(StageFamily::Reach, si.build)) return hipErrorInvalidValue;  // (the plain build only)
  const size_t lds = closed_loop_lds_bytes(kt, kq);
  const dim3 g(grid), blk(64);
  if (int r = with_compiled_shape(kq.nx, kq.ng, kq.np, [&](auto qd) {
        hipLaunchKernelGGL((reach_kernel<decltype(qd)>), g, blk, lds, st, m, kt, kq, io, re);
      }))
    return r;  // not a compiled shape: the stepwise path runs it
  return hipGetLastError();
}

int launch_reach_update_kernel(int64_t B, hipStream_t st, const DevModel* m, int k, int last, const ReachArgs& re,
                               const double* xt, const double* pose, const double* dist, const double* eta,
                               const int32_t* status, const int32_t* iters) {
  hipLaunchKernelGGL(reach_update_kernel, dim3(static_cast<unsigned>((B + 255) / 256)), dim3(256), 0, st, m, B, k,
                     last, re, xt, pose, dist, eta, status, iters);
  return hipGetLastError();
}

}  // namespace drc_amd
