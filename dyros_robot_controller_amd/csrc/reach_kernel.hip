// Goal-reaching rollouts with per-instance stopping (drc_qpik_reach_batch):
// the closed loop of drc_qpik_rollout_batch in mode QPIKStep, where every
// instance stops on its own -- the pose is within the tolerances of the target
// (reach.hpp), the step budget is spent, or its QP is not solved (eta = 0: it
// would stay where it is for the rest of a fixed horizon).  Reference: no
// counterpart.
//
// reach_kernel: the persistent form for the compiled QP shapes, shaped like
// rollout_kernel (rollout_kernel.hip): one instance per wave from the work
// queue, the task record in LDS, the state in the caller's q_final /
// qdot_final arrays.  The verdict is wave-uniform, so the three stops are
// uniform branches that leave the step loop, and the wave takes the next
// instance from the queue: an instance costs the steps it needs, not the
// horizon.
//
// reach_update_kernel: verdict and state update alone, one thread per
// instance, for the stepwise path (api.cpp: the stage launch and
// drc_qpik_batch's launch sequence per step, then this kernel).  Both forms
// call reach_error / reach_within (reach.hpp) and rollout_velocity /
// rollout_advance (rollout_update.hpp) on the same values, so the two paths
// return identical bits (tests/test_gpu_reach.py).
#include "task_stage.hpp"
#include "qp_solver.hpp"
#include "launch.hpp"
#include "reach.hpp"
#include "rollout_update.hpp"

namespace drc_amd {

// (ReachArgs: launch.hpp.  io.out / io.status / io.iters of the persistent
// kernel are one step's scratch: eta [na][B], status [B], iters [B])

// Stepwise path.  Instances that have stopped (result != kReachActive) are
// skipped; an active one takes step k's verdict from the stage outputs at
// (q_k, v_k) -- pose [12][B], dist [1+nv][B] -- and, unless it stops, the
// update from that step's eta / status / iters.  last: k = max_steps, no QP ran.
// The state is updated in place: the yaw and the wheel positions are read
// before any row is written, and row r is read before it is written.
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
  } else {
    const int st = status[b];
    if (re.status_last) re.status_last[b] = st;
    if (re.iters_total) re.iters_total[b] += iters[b];
    if (st != DRC_STATUS_SOLVED) res = DRC_REACH_QP_FAILED;
  }
  if (res != kReachActive) {  // stopped at (q_k, v_k): the finals hold it
    re.result[b] = res;
    re.steps_used[b] = k;
    if (re.err_final) {
      re.err_final[b] = err[0];
      re.err_final[B + b] = err[1];
    }
    if (re.dist_final)
      for (int i = 0; i <= M->nv; ++i) re.dist_final[i * B + b] = dist[i * B + b];
    return;
  }
  double Jm[3][kMaxWheels];
  double cy = 1, sy = 0;
  if (M->kind == 1) {
    double wp[kMaxWheels];
    for (int w = 0; w < kMaxWheels; ++w) wp[w] = w < M->n_wheel ? re.qf[(M->mobi_start + w) * B + b] : 0.0;
    mobile_fk(M, wp, Jm);
    const double yaw = re.qf[(M->virtual_start + 2) * B + b];
    cy = cos(yaw);
    sy = sin(yaw);
  }
  const auto e = [&](int a) { return eta[a * B + b]; };
  for (int r = 0; r < M->nv; ++r) {
    const double q = re.qf[r * B + b];
    const double v = rollout_velocity(M, r, cy, sy, Jm, e);
    const double qn = rollout_advance(q, re.dt, v);
    re.vf[r * B + b] = v;
    re.qf[r * B + b] = qn;
  }
}

#ifndef DRC_FUSED_WAVES
#define DRC_FUSED_WAVES 2
#endif
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
  static_assert(QD::gs == 64, "the reach kernel runs one instance per wave");
  const int l = lane_id();
  const int64_t B = io.B, LD = io.ld;
  const int nv = kt.nv, na = kq.na;
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
    int k = 0, res = DRC_REACH_BUDGET, st_last = 0, it_total = 0;
    for (;;) {
      IO is = iol;
      if (k > 0) {
        is.q = re.qf;
        is.qdot = re.vf;
      }
      task_instance<0, false>(M0, kt, is, S, b);
      wsync();
      // the pose at q_k from the task plan (the pure copies of the stage entry's
      // pose output) against the target: every lane forms the same two numbers
      double err[2];
      {
        const double* Te = S + kt.kTe;
        double ps[12], tg[12];
        for (int i = 0; i < 12; ++i) {
          ps[i] = i < 9 ? Te[(i % 3) * 3 + i / 3] : Te[i];
          tg[i] = io.xt[i * LD + gb];
        }
        reach_error(ps, tg, err);
      }
      // what stands there when the instance stops is the value at q_final (a
      // QP that fails leaves the state where this stage ran)
      if (re.err_final && l < 2) re.err_final[l * LD + gb] = l ? err[1] : err[0];
      if (re.dist_final && l <= nv) re.dist_final[l * LD + gb] = iol.rec[kt.rDist + l];
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
    }
    // stopped at (q_k, v_k): from step 1 on the finals hold it
    if (k == 0 && l < nv) {
      const double q0 = io.q[l * LD + gb], v0 = io.qdot[l * LD + gb];
      re.qf[l * LD + gb] = q0;
      re.vf[l * LD + gb] = v0;
    }
    if (l == 0) {
      re.result[gb] = res;
      re.steps_used[gb] = k;
      if (re.status_last) re.status_last[gb] = st_last;
      if (re.iters_total) re.iters_total[gb] = it_total;
    }
    wsync();
  }
}

int launch_reach_kernel(unsigned grid, hipStream_t st, const DevModel* m, const KParams& kt, const KParams& kq,
                        const IO& io, const ReachArgs& re) {
  const int plan = fused_lds_doubles(kt, kq), state = rollout_state_doubles(kt, kq);
  const size_t lds = static_cast<size_t>(plan > state ? plan : state) * sizeof(double);
  const dim3 g(grid), blk(64);
  if (kq.nx == 23 && kq.ng == 16 && kq.np == 7)  // FR3
    hipLaunchKernelGGL((reach_kernel<Dims<23, 16, 7, true, true, 64>>), g, blk, lds, st, m, kt, kq, io, re);
  else if (kq.nx == 20 && kq.ng == 14 && kq.np == 6)  // UR5e
    hipLaunchKernelGGL((reach_kernel<Dims<20, 14, 6, true, true, 64>>), g, blk, lds, st, m, kt, kq, io, re);
  else if (kq.nx == 9 && kq.ng == 16 && kq.np == 9)  // Husky-FR3
    hipLaunchKernelGGL((reach_kernel<Dims<9, 16, 9, true, true, 64>>), g, blk, lds, st, m, kt, kq, io, re);
  else if (kq.nx == 11 && kq.ng == 16 && kq.np == 11)  // XLS-FR3
    hipLaunchKernelGGL((reach_kernel<Dims<11, 16, 11, true, true, 64>>), g, blk, lds, st, m, kt, kq, io, re);
  else
    return hipErrorInvalidValue;  // not a compiled shape: the stepwise path runs it
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
