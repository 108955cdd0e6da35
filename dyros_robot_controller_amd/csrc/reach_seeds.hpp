// drc_qpik_reach_seeds_batch (reach_seeds_kernel.hip,
// reach_seeds_obstacle_kernel.hip): S seeds per target, one answer per target.
// The rule that picks a group's winner, the key a seed that has reached
// publishes to its group's word and the predicate by which another seed of the
// group stops early -- and, for the device compiler, what the kernels need
// beyond IO and ReachArgs and their host-side launchers (called by api.cpp;
// each returns the hipError_t of its launch).  A header of its own, so that
// launch.hpp and the units that include it stay what they are.  Reference: no
// counterpart.
//
// The rule part is plain host / device code without wave intrinsics, like
// reach.hpp: the select kernel, the host compiler
// (tools/reach_seeds_host_test.cpp, tests/test_reach_seeds_host.py) and numpy
// state the same winner.
//
// Why cancellation cannot change an output.  The winner is defined on the
// outcomes every seed would have without cancellation.  A seed publishes only
// when it is REACHED, at its step k, and an instance reads the word only after
// a failed verdict at its own step k:
//   FIRST         key = s.  s stops if word < s: a lower seed has reached, so s
//                 is not the lowest seed that reaches.
//   FEWEST_STEPS  key = k S + s.  s stops at step k if word / S <= k: some seed
//                 reached in k steps or fewer, while s needs more than k.
// The winner never meets its own condition, whatever the order and whenever (or
// whether) a key becomes visible; a seed that stops early is REACHED for fewer
// seeds, never for more, and with the same step count.  So the winner among the
// outcomes of a cancelling call is the winner among the uncancelled ones
// (seeds_winner works on either), and its values are its uncancelled ones.  If
// no seed reaches, no key is published and nothing is cancelled.
#pragma once

#include <cstdint>

#ifndef DRC_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define DRC_HD __host__ __device__
#else
#define DRC_HD
#endif
#endif

namespace drc_amd {

// the values of include/drc_amd.h (api.cpp asserts that they agree)
constexpr int kSeedsFirst = 0, kSeedsFewestSteps = 1;
constexpr int kSeedsReached = 0, kSeedsCancelled = 3;
// a group's word before any seed has published: above every key, as (max_steps
// + 1) S < 2^31 (every byte 0xff)
constexpr uint32_t kSeedsNoKey = 0xffffffffu;

// what seed s of S publishes with an atomic min when it is REACHED at step k
DRC_HD inline uint32_t seeds_key(int rule, int S, int k, int s) {
  return rule == kSeedsFewestSteps ? static_cast<uint32_t>(k) * static_cast<uint32_t>(S) + static_cast<uint32_t>(s)
                                   : static_cast<uint32_t>(s);
}

// whether seed s, outside the tolerances at step k, stops on the value it read
// from its group's word (any value the word has held, or kSeedsNoKey)
DRC_HD inline bool seeds_cancelled(int rule, int S, uint32_t word, int k, int s) {
  if (word == kSeedsNoKey) return false;
  return rule == kSeedsFewestSteps ? word / static_cast<uint32_t>(S) <= static_cast<uint32_t>(k)
                                   : word < static_cast<uint32_t>(s);
}

// no seed reached: a is strictly closer than b -- the least e_p, then the least
// e_R; a NaN counts as +inf (equal errors: the caller keeps the lower index)
DRC_HD inline bool seeds_closer(double ep_a, double er_a, double ep_b, double er_b) {
  const double inf = __builtin_inf();
  if (ep_a != ep_a) ep_a = inf;
  if (er_a != er_a) er_a = inf;
  if (ep_b != ep_b) ep_b = inf;
  if (er_b != er_b) er_b = inf;
  if (ep_a != ep_b) return ep_a < ep_b;
  return er_a < er_b;
}

// The winner of one group: seed s has result[s * ld], steps[s * ld], e_p
// ep[s * ld] and e_R er[s * ld].  Some seed REACHED: the lowest such index
// (FIRST) or the one with the fewest steps, ties to the lowest index
// (FEWEST_STEPS).  None: the closest by seeds_closer, ties to the lowest index.
DRC_HD inline int seeds_winner(int rule, int S, const int32_t* result, const int32_t* steps, const double* ep,
                               const double* er, int64_t ld) {
  int win = -1;
  for (int s = 0; s < S; ++s) {
    if (result[s * ld] != kSeedsReached) continue;
    if (win < 0) {
      win = s;
      if (rule != kSeedsFewestSteps) return win;
    } else if (steps[s * ld] < steps[win * ld]) {
      win = s;
    }
  }
  if (win >= 0) return win;
  win = 0;
  for (int s = 1; s < S; ++s)
    if (seeds_closer(ep[s * ld], er[s * ld], ep[win * ld], er[win * ld])) win = s;
  return win;
}

}  // namespace drc_amd

#if defined(__HIPCC__)
#include "launch.hpp"

namespace drc_amd {

// re: as for drc_qpik_reach_batch on the S T instances, instance (s, t) at
// column s T + t, every array in stream scratch (result / steps_used may be the
// caller's inst_result / inst_steps).  word [T]: the groups' words, every byte
// 0xff before the launch, touched by agent-scope atomics only
struct ReachSeedsArgs {
  ReachArgs re;
  int64_t T;
  int S, rule, cancel;
  uint32_t* word;
};

// the [T] outputs of a call, gathered from re's arrays by the select kernel;
// status_last, iters_total, err_final [2][T], dist_final [1+dof][T] may be NULL
struct ReachSeedsOut {
  int32_t *seed, *result, *steps_used;
  double *q_sol, *qdot_sol;
  int32_t *status_last, *iters_total;
  double *err_final, *dist_final;
};

// persistent kernel (compiled QPIK shapes in the Plain and Obst builds,
// hipErrorInvalidValue otherwise): reach_kernel's loop per instance, with the
// publish and the cancel check of its group's word.  io as for
// launch_reach_kernel, xt / xdt the targets expanded to [..][S T]; si.ob the
// call's poses (ld 0, or expanded to [n][12][S T])
int launch_reach_seeds_kernel(unsigned grid, hipStream_t st, const DevModel* m, const KParams& kt, const KParams& kq,
                              const IO& io, const ReachSeedsArgs& rs, const StageIn& si);
// dst [rows][S T] from src [rows][ld], ld >= T: column s T + t is column t
int launch_reach_seeds_expand_kernel(hipStream_t st, int rows, int64_t T, int S, const double* src, int64_t ld,
                                     double* dst);
// one thread per group: the winner by seeds_winner over rs.re's result,
// steps_used and err_final (required here), then the gather into out
int launch_reach_seeds_select_kernel(hipStream_t st, int nv, const ReachSeedsArgs& rs, const ReachSeedsOut& out);

}  // namespace drc_amd
#endif
