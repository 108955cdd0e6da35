// Closed-loop QPIK rollouts (drc_qpik_rollout_batch): the reference's control
// loop -- QPIK*, then q_desired = q + qdot_desired * dt
// (examples/C++/src/fr3_controller.cpp:123-134) -- over a horizon of `steps`
// cycles on the device.
//
// rollout_kernel: the persistent form for the compiled QP shapes.  Each wave
// takes an instance from the work queue (as fused_kernel.hip's kernel) and runs
// all its steps before the next: task stage (task_stage.hpp), QP
// (qp_solver.hpp), state update.  The task record stays in LDS as in the fused
// kernel; the state (q, v) lives in the caller's q_final / qdot_final arrays,
// which task_instance reads through IO::q / IO::qdot from step 1 on: lane l
// reads back the element lane l stored one step earlier (state_visible()).
// Same device functions on the same values as drc_qpik_batch step by step, so
// every step's result is bit-identical to it (tests/test_gpu_rollout.py).
// The kernel body is written out in full, the blocks of closed_loop.hpp
// included (LDS views, step IO, state update -- the same text as
// wave_state_update): through the header's functions the hull build's FR3
// instantiation came out with one more VGPR spill (56 to 57; UR5e's with one
// fewer), in every form tried, so this kernel keeps the text it had
// (profiles/closed_loop_refactor_resources.txt).
//
// rollout_integrate_kernel: the state update alone, one thread per instance,
// for the stepwise path (api.cpp: drc_qpik_batch's launch sequence per step,
// then this kernel): closed_loop.hpp's thread_state_update, on the arithmetic
// of wave_state_update (rollout_update.hpp), so the two paths return identical
// bits.
#include "task_stage.hpp"
#include "qp_solver.hpp"
#include "closed_loop.hpp"

namespace drc_amd {

#ifndef DRC_ROLLOUT_MESH
// Stepwise path: one thread per instance.  q_in may be qf (in place)
__global__ void __launch_bounds__(256)
rollout_integrate_kernel(const DevModel* __restrict__ M, int64_t B, double dt, const double* q_in, const double* eta,
                         double* qf, double* vf, double* q_traj) {
  const int64_t b = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (b >= B) return;
  thread_state_update(M, B, b, dt, q_in, eta, qf, vf, q_traj);
}
#endif

// What the persistent kernel needs beyond IO
struct Rollout {
  int steps, per_step;  // per_step: targets are [steps][12 | 6][B]
  double dt;
  double *qf, *vf;  // q_final, qdot_final [dof][B]: the state between steps
  double *q_traj, *pose_traj, *dist_traj;
  int64_t out_step;  // doubles between two steps' eta in io.out (0: one scratch slot, no qdot_traj)
};

template <class QD, bool MESH = false>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(DRC_FUSED_WAVES, 8)))
rollout_kernel(const DevModel* __restrict__ M0, const KParams kt, const KParams kq, const IO io, const Rollout ro) {
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
    for (int k = 0; k < ro.steps; ++k) {
      IO is = iol;
      if (k > 0) {
        is.q = ro.qf;
        is.qdot = ro.vf;
      }
      if (ro.per_step) {
        if (is.xt) is.xt = io.xt + static_cast<int64_t>(k) * 12 * LD;
        is.xdt = io.xdt + static_cast<int64_t>(k) * 6 * LD;
      }
      is.out = io.out + k * ro.out_step;
      is.status = io.status + k * LD;
      if (io.iters) is.iters = io.iters + k * LD;
      KParams ktl = kt;  // this step's task parameters
      ktl.t = rollout_time(kt.t, k, ro.dt);
      task_instance<0, MESH>(M0, ktl, is, S, b);
      wsync();
      // stage outputs at q_k, in drc_qpik_stages_batch's layouts: the pose from
      // the task plan (not overlaid before the QP starts), the distance from
      // the record
      if (ro.pose_traj && l < 12) {
        const double* Te = S + kt.kTe;
        ro.pose_traj[(static_cast<int64_t>(k) * 12 + l) * LD + gb] = l < 9 ? Te[(l % 3) * 3 + l / 3] : Te[l];
      }
      if (ro.dist_traj && l <= nv)
        ro.dist_traj[(static_cast<int64_t>(k) * (1 + nv) + l) * LD + gb] = iol.rec[kt.rDist + l];
      wsync();
      qp_instance<QD>(M0, kq, kpl, is, S, b);
      // ---------------- state update ----------------------------------------
      state_visible();
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
        const double qn = rollout_advance(qk, ro.dt, v);
        ro.vf[l * LD + gb] = v;
        ro.qf[l * LD + gb] = qn;
        if (ro.q_traj) ro.q_traj[(static_cast<int64_t>(k) * nv + l) * LD + gb] = qn;
      }
      state_visible();
      wsync();
    }
  }
}

template <bool MESH>
static int launch_rollout(unsigned grid, size_t lds, hipStream_t st, const DevModel* m, const KParams& kt,
                          const KParams& kq, const IO& io, const Rollout& ro) {
  const dim3 g(grid), blk(64);
  if (int r = with_compiled_shape(kq.nx, kq.ng, kq.np, [&](auto qd) {
        hipLaunchKernelGGL((rollout_kernel<decltype(qd), MESH>), g, blk, lds, st, m, kt, kq, io, ro);
      }))
    return r;  // not a compiled shape: the stepwise path runs it
  return hipGetLastError();
}

// The builds for models with hulls are a translation unit of their own
// (rollout_mesh_kernel.hip includes this file with DRC_ROLLOUT_MESH defined),
// as fused_mesh_kernel.hip is for the fused kernel.
#ifdef DRC_ROLLOUT_MESH
int launch_rollout_mesh_kernel(unsigned grid, size_t lds, hipStream_t st, const DevModel* m, const KParams& kt,
                               const KParams& kq, const IO& io, const Rollout& ro) {
  return launch_rollout<true>(grid, lds, st, m, kt, kq, io, ro);
}
#else
int launch_rollout_mesh_kernel(unsigned grid, size_t lds, hipStream_t st, const DevModel* m, const KParams& kt,
                               const KParams& kq, const IO& io, const Rollout& ro);
int launch_rollout_kernel(unsigned grid, hipStream_t st, const DevModel* m, const KParams& kt, const KParams& kq,
                          const IO& io, int steps, int per_step, double dt, double* qf, double* vf, double* q_traj,
                          double* pose_traj, double* dist_traj, int64_t out_step, const StageIn& si) {
  const Rollout ro{steps, per_step, dt, qf, vf, q_traj, pose_traj, dist_traj, out_step};
  const size_t lds = closed_loop_lds_bytes(kt, kq);
  switch (si.build) {
    case StageBuild::Plain: return launch_rollout<false>(grid, lds, st, m, kt, kq, io, ro);
    case StageBuild::Mesh: return launch_rollout_mesh_kernel(grid, lds, st, m, kt, kq, io, ro);
    default: return hipErrorInvalidValue;  // (no build takes poses: the stepwise path runs models with slots)
  }
}

int launch_rollout_integrate_kernel(int64_t B, hipStream_t st, const DevModel* m, double dt, const double* q_in,
                                    const double* eta, double* qf, double* vf, double* q_traj) {
  hipLaunchKernelGGL(rollout_integrate_kernel, dim3(static_cast<unsigned>((B + 255) / 256)), dim3(256), 0, st, m, B,
                     dt, q_in, eta, qf, vf, q_traj);
  return hipGetLastError();
}
#endif

}  // namespace drc_amd
