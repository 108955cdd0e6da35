// Certified path clearance (drc_clearance_certify_batch): the continuous check
// of a joint-space path by adaptive bisection, after Schwarzer, Saha and
// Latombe.  Reference: no counterpart.
//
// Along the straight segment qa -> qb every pair's relative motion is at most
// M = max_p sum_i Wt[i][p] |qb_i - qa_i| (the motion weights of model.cpp
// build_motion_tables), and the signed distance of two convex bodies is
// 1-Lipschitz in that motion.  On an interval of length tau of the segment's
// parameter whose ends have the distances d0 and d1, therefore
//     d(t) >= (d0 + d1) / 2 - tau M / 2.
// Where that is at least d_stop the interval is certified (a leaf); where not,
// its midpoint is evaluated and the two halves are treated alike, left first,
// down to max_depth.  Positions are the dyadic t = k / 2^e; the state there is
// clearance_sample(qa, qb, k, 2^e) of clearance.hpp (exact at both ends).
//
// The walk of one path is one CertFold, stepped by the three functions below:
// the caller evaluates the sample the fold asks for (ev_k / 2^ev_e on segment
// seg) and hands (d, pair) to cert_step.  The right ends of the intervals that
// wait for their turn live in a stack that the caller owns, one distance per
// depth 1 .. max_depth (the persistent kernel keeps it in the lanes of one
// register, the host in an array): anything with push(level, v) / pop(level).
//
// Every operation is rounded once (contraction off), so certify_kernel.hip,
// the host compiler (tools/clearance_certify_host_test.cpp) and the Python
// restatement of tests/test_clearance_certify_host.py give the same bits.
// Plain host / device code without wave intrinsics, like clearance.hpp.
#pragma once

#include "clearance.hpp"

namespace drc_amd {

// (DRC_CLEAR_UNDECIDED in include/drc_amd.h; api.cpp asserts it)
constexpr int32_t kClearUndecided = 3;
constexpr int kCertMaxDepth = 20;

// what the caller does after a call of cert_segment / cert_step
enum CertNext : int32_t {
  kCertEval = 0,     // evaluate the sample (seg, ev_k / 2^ev_e), then cert_step
  kCertSegEnd = 1,   // the segment is certified: cert_segment on the next one; after the last the walk ends FREE
  kCertStop = 2,     // the walk is over: result, seg_stop and t_stop say why and where
};

// most evaluations a path can take, in 64 bits: the caller checks it against 2^31
DRC_HD inline int64_t certify_max_samples(int64_t waypoints, int max_depth) {
  return (waypoints - 1) * (int64_t(1) << max_depth) + 1;
}

// t = k / 2^e, exact
DRC_HD inline double cert_t(int32_t k, int32_t e) {
  return static_cast<double>(k) / static_cast<double>(int64_t(1) << e);
}

// One term of the motion bound: s + w |dq|, the product and the sum rounded
DRC_HD inline double cert_motion_term(double s, double w, double adq) {
#pragma clang fp contract(off)
  const double t = w * adq;
  return s + t;
}

// The running state of one path's walk, as it starts: the first sample asked
// for is waypoint 0 (segment 0, t = 0)
struct CertFold {
  double d_min = INFINITY, t_min = -1.0;
  double d_lower = INFINITY, t_stop = -1.0;
  int32_t seg_min = -1, pair_min = -1;
  int32_t result = kClearFree, seg_stop = -1;
  int32_t samples = 0;
  // the walk: the current interval [k, k + 1] / 2^e of segment seg, its end
  // distances, and the sample that is asked for
  int32_t seg = 0, e = 0, k = 0;
  int32_t ev_k = 0, ev_e = 0;
  double d0 = INFINITY, d1 = INFINITY;
};

DRC_HD inline int32_t cert_stop(CertFold* f, int32_t result, int32_t k, int32_t e) {
  f->result = result;
  f->seg_stop = f->seg;
  f->t_stop = cert_t(k, e);
  return kCertStop;
}

// Start of segment seg (waypoint seg -> seg + 1).  travel_ok: every coordinate
// of the model's travel_mask has max(|qa|, |qb|) <= travel (cert_travel_ok).
// Segment 0 has waypoint 0 evaluated by then (d0); a later one starts where
// the previous one ended.  Asks for t = 1
DRC_HD inline int32_t cert_segment(CertFold* f, int32_t seg, bool travel_ok) {
  f->seg = seg;
  f->e = 0;
  f->k = 0;
  if (!travel_ok) return cert_stop(f, kClearUndecided, 0, 0);
  f->ev_k = 1;
  f->ev_e = 0;
  return kCertEval;
}

// One coordinate's part of travel_ok (NaN fails)
DRC_HD inline bool cert_travel_ok(double qa, double qb, double travel) {
  const double a = qa < 0 ? -qa : qa, b = qb < 0 ? -qb : qb;
  return (a > b ? a : b) <= travel && a == a && b == b;
}

// (d, pair) of the sample that was asked for.
//   d NaN        INVALID at the sample (the minimum keeps what it held)
//   d < d_min    the minimum becomes (d, seg, t, pair); strict: the first evaluated wins a tie
//   d < d_stop   BLOCKED at the sample
// Then the intervals, until one needs its midpoint or the segment is done:
//   lb = 0.5 (d0 + d1) - (0.5 (t1 - t0)) M;  lb >= d_stop: a leaf, d_lower = min(d_lower, lb), on to
//   the next pending interval; otherwise UNDECIDED at (seg, t0) if e == max_depth, else the midpoint.
// Waypoint 0 answers kCertSegEnd: the caller starts segment 0, or ends a path of one waypoint
template <class Stack>
DRC_HD inline int32_t cert_step(CertFold* f, Stack& stack, double d, int32_t pair, double d_stop, double M,
                                int32_t max_depth) {
#pragma clang fp contract(off)
  const int32_t sk = f->ev_k, se = f->ev_e;
  f->samples += 1;
  if (d != d) return cert_stop(f, kClearInvalid, sk, se);
  if (d < f->d_min) {
    f->d_min = d;
    f->seg_min = f->seg;
    f->t_min = cert_t(sk, se);
    f->pair_min = pair;
  }
  if (d < d_stop) return cert_stop(f, kClearBlocked, sk, se);
  if (se == 0 && sk == 0) {  // waypoint 0
    f->d0 = d;
    return kCertSegEnd;
  }
  if (se == 0) {  // t = 1: the whole segment
    f->d1 = d;
  } else {  // the midpoint of [k, k + 1] / 2^e: the right half waits, the left half is next
    stack.push(f->e + 1, f->d1);
    f->e += 1;
    f->k *= 2;
    f->d1 = d;
  }
  for (;;) {
    const double half = 0.5 / static_cast<double>(int64_t(1) << f->e);  // 0.5 (t1 - t0), exact
    const double sum = f->d0 + f->d1;
    const double mid = 0.5 * sum;
    const double slack = half * M;
    const double lb = mid - slack;
    if (lb >= d_stop) {
      if (lb < f->d_lower) f->d_lower = lb;
      f->d0 = f->d1;
      while (f->e > 0 && (f->k & 1)) {  // a right half ends its parent too
        f->e -= 1;
        f->k >>= 1;
      }
      if (f->e == 0) return kCertSegEnd;
      f->k += 1;
      f->d1 = stack.pop(f->e);
      continue;
    }
    if (f->e == max_depth) return cert_stop(f, kClearUndecided, f->k, f->e);
    f->ev_k = 2 * f->k + 1;
    f->ev_e = f->e + 1;
    return kCertEval;
  }
}

// The host's stack: one distance per depth
struct CertStackArray {
  double v[kCertMaxDepth + 1];
  DRC_HD void push(int32_t level, double x) { v[level] = x; }
  DRC_HD double pop(int32_t level) const { return v[level]; }
};

}  // namespace drc_amd
