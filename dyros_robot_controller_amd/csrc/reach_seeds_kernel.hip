// Reach from several seeds per target (drc_qpik_reach_seeds_batch): S T
// instances of drc_qpik_reach_batch's loop (reach_kernel.hip), instance (s, t)
// at column s T + t, of which the select kernel returns one per target by the
// rule of reach_seeds.hpp.  Reference: no counterpart.
//
// reach_seeds_kernel: the persistent form for the compiled QP shapes: one
// instance per wave from the work queue, the task record in LDS, the state in
// the (scratch) q_final / qdot_final arrays, the update scratch at the start of
// the plan; the blocks it has in common with reach_kernel are closed_loop.hpp's.
// Its own here is the step loop with one 32-bit word per group.  A wave
// whose instance is REACHED publishes its key with an atomic min (lane 0); a
// wave whose verdict failed loads the word (relaxed, agent scope, made uniform)
// and leaves the instance on a uniform branch if seeds_cancelled says so.  No
// spin, no fence and no payload behind the flag: the word is the whole message,
// a stale value only delays a stop, and no output depends on it (reach_seeds.hpp
// has the argument).  The per-XCD L2s are not coherent for plain accesses, so
// the word is touched by these two atomics alone.  OB: empty, or one ObstIn --
// the build for models with obstacle slots (reach_seeds_obstacle_kernel.hip).
//
// reach_seeds_expand_kernel: targets (and per-target poses) [..][T] to
// [..][S T], since task_instance indexes them with the state's stride.
// reach_seeds_select_kernel: one thread per group, the winner and the gather.
// Both serve the stepwise path too (api.cpp), which runs the existing stepwise
// reach on the expanded arrays: the same bits as the persistent kernel
// (tests/test_gpu_reach_seeds.py).
#include "task_stage.hpp"
#include "qp_solver.hpp"
#include "reach_seeds.hpp"
#include "closed_loop.hpp"

namespace drc_amd {

template <class QD, class... OB>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(DRC_FUSED_WAVES, 8)))
reach_seeds_kernel(const DevModel* __restrict__ M0, const KParams kt, const KParams kq, const IO io,
                   const ReachSeedsArgs rs, const OB... ob) {
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
  const ReachArgs& re = rs.re;
  const int l = lane_id();
  const int64_t B = io.B, LD = io.ld;
  const int nv = kt.nv, na = kq.na;
  const ClosedLoopLds cl(io, S, kt, kq);
  const InstSeq seq(B, kq.xcd_map, io.queue);
  for (int64_t j = seq.first(); j < seq.n; j = seq.next(j)) {
    const int64_t b = seq.at(j);
    if (b >= B) continue;
    const int64_t gb = io.b0 + b;
    const int sd = static_cast<int>(gb / rs.T);  // the seed and its group
    uint32_t* word = rs.word + (gb - sd * rs.T);
    int k = 0, res = DRC_REACH_BUDGET, st_last = 0, it_total = 0;
    for (;;) {
      IO is = step_io(cl.io, k, re.qf, re.vf);
      task_instance<0, false, sizeof...(OB) != 0>(M0, kt, is, S, b, ob...);
      wsync();
      // the pose at q_k from the task plan against the target (reach_kernel)
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
      store_at_state(re, cl.io.rec + kt.rDist, gb, LD, l, nv, err);  // (err_final: scratch, the select kernel needs it)
      const int within = __builtin_amdgcn_readfirstlane(reach_within(err, re.tau_p, re.tau_r) ? 1 : 0);
      if (within) {
        if (rs.cancel && l == 0)
          __hip_atomic_fetch_min(word, seeds_key(rs.rule, rs.S, k, sd), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        res = DRC_REACH_REACHED;
        break;
      }
      if (k == re.max_steps) {
        res = DRC_REACH_BUDGET;
        break;
      }
      if (rs.cancel) {  // has a seed of this group made this one a loser?
        const uint32_t w = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(
            static_cast<int>(__hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))));
        if (seeds_cancelled(rs.rule, rs.S, w, k, sd)) {
          res = DRC_REACH_CANCELLED;
          break;
        }
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

template <class... OB>
static int launch_shapes(unsigned grid, hipStream_t st, const DevModel* m, const KParams& kt, const KParams& kq,
                         const IO& io, const ReachSeedsArgs& rs, const OB&... ob) {
  // the update scratch lies in the plan: fused_lds_doubles for every compiled shape
  const size_t lds = closed_loop_lds_bytes(kt, kq);
  const dim3 g(grid), blk(64);
  if (int r = with_compiled_shape(kq.nx, kq.ng, kq.np, [&](auto qd) {
        hipLaunchKernelGGL((reach_seeds_kernel<decltype(qd), OB...>), g, blk, lds, st, m, kt, kq, io, rs, ob...);
      }))
    return r;  // not a compiled shape: the stepwise path runs it
  return hipGetLastError();
}

// The builds for models with obstacle slots are a translation unit of their
// own (reach_seeds_obstacle_kernel.hip includes this file with
// DRC_REACH_SEEDS_OBST defined), as reach_path_obstacle_kernel.hip's.
#if defined(DRC_REACH_SEEDS_OBST)
int launch_reach_seeds_obstacle_kernel(unsigned grid, hipStream_t st, const DevModel* m, const KParams& kt,
                                       const KParams& kq, const IO& io, const ReachSeedsArgs& rs, const ObstIn& ob) {
  return launch_shapes(grid, st, m, kt, kq, io, rs, ob);
}
#else
int launch_reach_seeds_obstacle_kernel(unsigned grid, hipStream_t st, const DevModel* m, const KParams& kt,
                                       const KParams& kq, const IO& io, const ReachSeedsArgs& rs, const ObstIn& ob);
int launch_reach_seeds_kernel(unsigned grid, hipStream_t st, const DevModel* m, const KParams& kt, const KParams& kq,
                              const IO& io, const ReachSeedsArgs& rs, const StageIn& si) {
  switch (si.build) {
    case StageBuild::Plain: return launch_shapes(grid, st, m, kt, kq, io, rs);
    case StageBuild::Obst: return launch_reach_seeds_obstacle_kernel(grid, st, m, kt, kq, io, rs, si.ob);
    default: return hipErrorInvalidValue;  // (no build for hulls or twists)
  }
}

// dst [rows][S T] from src [rows][ld]: one thread per element of dst
__global__ void __launch_bounds__(256)
reach_seeds_expand_kernel(int64_t n, int64_t T, int64_t B, const double* __restrict__ src, int64_t ld,
                          double* __restrict__ dst) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= n) return;
  const int64_t r = i / B, c = i - r * B;
  dst[i] = src[r * ld + c % T];
}

int launch_reach_seeds_expand_kernel(hipStream_t st, int rows, int64_t T, int S, const double* src, int64_t ld,
                                     double* dst) {
  const int64_t B = T * S, n = B * rows;
  hipLaunchKernelGGL(reach_seeds_expand_kernel, dim3(static_cast<unsigned>((n + 255) / 256)), dim3(256), 0, st, n, T, B,
                     src, ld, dst);
  return hipGetLastError();
}

// One thread per group.  The instances' outcomes are those of this call -- with
// cancellation the losers' may be cut short, which leaves the winner what it is
// (reach_seeds.hpp)
__global__ void __launch_bounds__(256)
reach_seeds_select_kernel(int nv, const ReachSeedsArgs rs, const ReachSeedsOut out) {
  const int64_t t = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  const int64_t T = rs.T, B = T * rs.S;
  if (t >= T) return;
  const ReachArgs& re = rs.re;
  const int s = seeds_winner(rs.rule, rs.S, re.result + t, re.steps_used + t, re.err_final + t, re.err_final + B + t, T);
  const int64_t b = s * T + t;
  out.seed[t] = s;
  out.result[t] = re.result[b];
  out.steps_used[t] = re.steps_used[b];
  for (int r = 0; r < nv; ++r) {
    out.q_sol[r * T + t] = re.qf[r * B + b];
    out.qdot_sol[r * T + t] = re.vf[r * B + b];
  }
  if (out.status_last) out.status_last[t] = re.status_last[b];
  if (out.iters_total) out.iters_total[t] = re.iters_total[b];
  if (out.err_final) {
    out.err_final[t] = re.err_final[b];
    out.err_final[T + t] = re.err_final[B + b];
  }
  if (out.dist_final)
    for (int r = 0; r <= nv; ++r) out.dist_final[r * T + t] = re.dist_final[r * B + b];
}

int launch_reach_seeds_select_kernel(hipStream_t st, int nv, const ReachSeedsArgs& rs, const ReachSeedsOut& out) {
  hipLaunchKernelGGL(reach_seeds_select_kernel, dim3(static_cast<unsigned>((rs.T + 255) / 256)), dim3(256), 0, st, nv,
                     rs, out);
  return hipGetLastError();
}
#endif

}  // namespace drc_amd
