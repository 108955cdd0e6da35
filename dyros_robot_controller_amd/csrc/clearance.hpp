// Path clearance (drc_clearance_path_batch): the sample states of a joint-space
// path and the rule that folds the distances at those states into a verdict.
// Reference: no counterpart.
//
// A path is `waypoints` states; consecutive ones bound a segment, which is
// walked in `substeps` equal steps of the parameter:
//   sample 0                 waypoint 0
//   sample j substeps + i    on segment j (waypoint j -> j + 1), 1 <= i <= substeps:
//                            waypoint j + 1 itself for i == substeps, otherwise
//                            qa + t (qb - qa) with t = double(i) / double(substeps)
// N = (waypoints - 1) substeps + 1 samples in all.  The quotient, the
// difference, the product and the sum are each rounded once (contraction off),
// so the persistent kernel (clearance_kernel.hip), the host compiler
// (tools/clearance_host_test.cpp, tests/test_clearance_host.py) and numpy's
// qa + (i / substeps) * (qb - qa) on the same doubles give the same bits.
//
// Plain host / device code without wave intrinsics, like reach.hpp.
#pragma once

#include <cmath>
#include <cstdint>

#ifndef DRC_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define DRC_HD __host__ __device__
#else
#define DRC_HD
#endif
#endif

namespace drc_amd {

// (the values of DRC_CLEAR_* in include/drc_amd.h; api.cpp asserts it)
constexpr int32_t kClearFree = 0, kClearBlocked = 1, kClearInvalid = 2;

// N, in 64 bits: the caller checks it against 2^31
DRC_HD inline int64_t clearance_samples(int64_t waypoints, int64_t substeps) { return (waypoints - 1) * substeps + 1; }

// One coordinate of sample i (1 <= i <= substeps) of the segment qa -> qb
DRC_HD inline double clearance_sample(double qa, double qb, int i, int substeps) {
#pragma clang fp contract(off)
  if (i == substeps) return qb;
  const double t = static_cast<double>(i) / static_cast<double>(substeps);
  const double d = qb - qa;
  const double td = t * d;
  return qa + td;
}

// The running state of one path's walk, as it starts
struct ClearFold {
  double d_min = INFINITY;
  int32_t sample_min = -1, pair_min = -1;
  int32_t result = kClearFree, sample_stop = -1;
};

// The rule: takes (d, pair) of the distance stage at sample n -- the samples
// come in order, from 0 -- and returns true when the walk stops there.
//   d NaN        INVALID at n (the minimum keeps what it held)
//   d < d_min    the minimum becomes (d, n, pair); strict, so the lowest sample wins a tie
//   d < d_stop   BLOCKED at n (after the minimum took the sample)
// A walk that never stops ends FREE with sample_stop = -1, as it began.
// d_stop = -inf never blocks; +inf blocks at sample 0 unless d is +inf itself.
DRC_HD inline bool clearance_step(ClearFold* f, int32_t n, double d, int32_t pair, double d_stop) {
  if (d != d) {
    f->result = kClearInvalid;
    f->sample_stop = n;
    return true;
  }
  if (d < f->d_min) {
    f->d_min = d;
    f->sample_min = n;
    f->pair_min = pair;
  }
  if (d < d_stop) {
    f->result = kClearBlocked;
    f->sample_stop = n;
    return true;
  }
  return false;
}

}  // namespace drc_amd
