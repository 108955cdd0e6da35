// The parts of a closed-loop step that the persistent kernels reach_kernel and
// reach_seeds_kernel and the stepwise path's update kernels
// (rollout_integrate_kernel, reach_path_update_kernel)
// have in common, as plain functions: every kernel
// keeps its own step loop -- stage, verdict, QP, status, update -- with its stop
// rules in place, and calls these for the blocks that are the same everywhere.
// The arithmetic itself is rollout_update.hpp's and reach.hpp's; both forms of
// an entry point go through the same functions here, so the persistent and the
// stepwise path return identical bits.
//
// No function here calls lane_id(): the kernel passes its own l (the opaque asm
// of lane_id() inside a helper changes the register allocation of the whole
// kernel), and IO comes by const reference.
//
// Two blocks stay written out in the persistent kernels: the word-wise copy of
// KParams into LDS (fused_kernel.hip and qp_kernel.hip have it too) and the
// loop that reads the pose and the target column before reach_error.  These
// kernels spill at their register budget, and with either block behind a
// function -- simplified on its own before it is inlined -- the allocation of
// the whole kernel comes out differently, with more VGPR spills in some
// instantiations and thousands of other instructions in fused_kernel and
// qp_kernel, whose assembly is to stay what it was.  With the functions below
// every kernel keeps its VGPRs, scratch and VGPR spill count
// (profiles/closed_loop_refactor_resources.txt).  rollout_kernel and
// reach_path_kernel are the exceptions: their bodies keep the text of all these
// blocks (each file says why), so a change to wave_state_update is made there
// too; their stepwise kernels and launchers use this header.
#pragma once

#include "launch.hpp"
#include "reach.hpp"
#include "rollout_update.hpp"

// Occupancy target of the persistent kernels (waves per SIMD), fused_kernel's
#ifndef DRC_FUSED_WAVES
#define DRC_FUSED_WAVES 2
#endif

namespace drc_amd {

// A persistent kernel's view of its LDS S: the call's IO with the task record
// in LDS (one slot, as in fused_kernel), and the state update's scratch -- q_k
// [nv], eta_k [na], J_mobile -- at the start of the plan, dead once the QP has
// stored its outputs (rollout_state_doubles)
struct ClosedLoopLds {
  IO io;
  double *qs, *es;
  double (*Jm)[kMaxWheels];
  __device__ __forceinline__ ClosedLoopLds(const IO& io0, double* S, const KParams& kt, const KParams& kq) : io(io0) {
    io.rec = S + fused_rec_offset(kt, kq);
    io.rec_stride = 0;
    qs = S;
    es = qs + ((kt.nv + 1) & ~1);
    Jm = reinterpret_cast<double(*)[kMaxWheels]>(es + ((kq.na + 1) & ~1));
  }
};
// ... and its size in bytes: the fused kernel's for every compiled shape
inline size_t closed_loop_lds_bytes(const KParams& kt, const KParams& kq) {
  const int plan = fused_lds_doubles(kt, kq), state = rollout_state_doubles(kt, kq);
  return static_cast<size_t>(plan > state ? plan : state) * sizeof(double);
}

// IO of step k: from step 1 on the stages read the state from the finals,
// where lane l reads back the element it stored one step earlier
__device__ __forceinline__ IO step_io(const IO& iol, int k, const double* qf, const double* vf) {
  IO is = iol;
  if (k > 0) {
    is.q = qf;
    is.qdot = vf;
  }
  return is;
}

// State update of instance gb by its wave, after the QP of step `is` (whose
// stores the caller has made visible: state_visible()).  Lane l reloads q_k[l]
// from is.q -- step 0: the caller's q0, which q_final may alias -- and stores
// v_{k+1}[l], q_{k+1}[l] to vf / qf [dof][LD]; the wave's own next stage reads
// them back (state_visible)
__device__ __forceinline__ void wave_state_update(const DevModel* M0, const IO& is, int64_t gb, int64_t LD, int l, int nv,
                                                  int na, double dt, double* qf, double* vf, const ClosedLoopLds& cl) {
  const double qk = l < nv ? is.q[l * LD + gb] : 0.0;
  if (l < nv) cl.qs[l] = qk;
  if (l < na) cl.es[l] = is.out[l * LD + gb];
  wsync();
  const DevModel* M = opaque_model(M0);
  double cy = 1, sy = 0;
  if (M->kind == 1) {
    if (l == 0) mobile_fk(M, cl.qs + M->mobi_start, cl.Jm);
    const double yaw = cl.qs[M->virtual_start + 2];
    cy = cos(yaw);
    sy = sin(yaw);
    wsync();
  }
  if (l < nv) {
    const double v = rollout_velocity(M, l, cy, sy, cl.Jm, [&](int a) { return cl.es[a]; });
    const double qn = rollout_advance(qk, dt, v);
    vf[l * LD + gb] = v;
    qf[l * LD + gb] = qn;
  }
  state_visible();
  wsync();
}

// The same update by one thread, instance b of B.  q_in may be qf (in place):
// the yaw and the wheel positions are read before any row is written, and row
// r is read before it is written
__device__ __forceinline__ void thread_state_update(const DevModel* M, int64_t B, int64_t b, double dt, const double* q_in,
                                                    const double* eta, double* qf, double* vf,
                                                    double* q_traj = nullptr) {
  double Jm[3][kMaxWheels];
  double cy = 1, sy = 0;
  if (M->kind == 1) {
    double wp[kMaxWheels];
    for (int w = 0; w < kMaxWheels; ++w) wp[w] = w < M->n_wheel ? q_in[(M->mobi_start + w) * B + b] : 0.0;
    mobile_fk(M, wp, Jm);
    const double yaw = q_in[(M->virtual_start + 2) * B + b];
    cy = cos(yaw);
    sy = sin(yaw);
  }
  const auto e = [&](int a) { return eta[a * B + b]; };
  for (int r = 0; r < M->nv; ++r) {
    const double q = q_in[r * B + b];
    const double v = rollout_velocity(M, r, cy, sy, Jm, e);
    const double qn = rollout_advance(q, dt, v);
    vf[r * B + b] = v;
    qf[r * B + b] = qn;
    if (q_traj) q_traj[r * B + b] = qn;
  }
}

// Entry i of the pose at q_k in the API's layout (R column-major, then p) from
// the task plan's Te = S + kt.kTe (R row-major, then p): the pure copies of the
// stage entry's pose output
__device__ __forceinline__ double plan_pose(const double* Te, int i) { return i < 9 ? Te[(i % 3) * 3 + i / 3] : Te[i]; }

// The verdict's errors and the record's distances [1+nv] at q_k, by the wave:
// what stands there when the instance stops is the value at q_final (a QP that
// fails leaves the state where this stage ran)
__device__ __forceinline__ void store_at_state(const ReachArgs& re, const double* rec_dist, int64_t gb, int64_t LD, int l,
                                               int nv, const double* err) {
  if (re.err_final && l < 2) re.err_final[l * LD + gb] = l ? err[1] : err[0];
  if (re.dist_final && l <= nv) re.dist_final[l * LD + gb] = rec_dist[l];
}

// This step's status and iteration count of instance gb, wave-uniform, once the
// QP's stores are visible to the wave
__device__ __forceinline__ void step_status(const IO& is, int64_t gb, int& st_last, int& it_total) {
  state_visible();
  st_last = __builtin_amdgcn_readfirstlane(
      __hip_atomic_load(is.status + gb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
  it_total += __builtin_amdgcn_readfirstlane(
      __hip_atomic_load(is.iters + gb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}

// ... and by the thread of the stepwise path, into status_last / iters_total
__device__ __forceinline__ int thread_step_status(const ReachArgs& re, int64_t b, const int32_t* status,
                                                  const int32_t* iters) {
  const int st = status[b];
  if (re.status_last) re.status_last[b] = st;
  if (re.iters_total) re.iters_total[b] += iters[b];
  return st;
}

// An instance of a persistent reach kernel has stopped at (q_k, v_k) after k
// steps: from step 1 on the finals hold it, at k = 0 they take the inputs ...
__device__ __forceinline__ void reach_finals(const IO& io, const ReachArgs& re, int64_t gb, int64_t LD, int l, int nv,
                                             int k) {
  if (k == 0 && l < nv) {
    const double q0 = io.q[l * LD + gb], v0 = io.qdot[l * LD + gb];
    re.qf[l * LD + gb] = q0;
    re.vf[l * LD + gb] = v0;
  }
}
// ... and one lane (the kernel's `if (l == 0)`) writes the outcome
__device__ __forceinline__ void reach_outcome(const ReachArgs& re, int64_t gb, int k, int res, int st_last, int it_total) {
  re.result[gb] = res;
  re.steps_used[gb] = k;
  if (re.status_last) re.status_last[gb] = st_last;
  if (re.iters_total) re.iters_total[gb] = it_total;
}
// ... and of the stepwise path, whose finals hold the state: the verdict's
// errors and the stage's distances are those at q_final (store_at_state)
__device__ __forceinline__ void thread_store_at_state(const DevModel* M, const ReachArgs& re, int64_t B, int64_t b,
                                                      const double* err, const double* dist) {
  if (re.err_final) {
    re.err_final[b] = err[0];
    re.err_final[B + b] = err[1];
  }
  if (re.dist_final)
    for (int i = 0; i <= M->nv; ++i) re.dist_final[i * B + b] = dist[i * B + b];
}

}  // namespace drc_amd
