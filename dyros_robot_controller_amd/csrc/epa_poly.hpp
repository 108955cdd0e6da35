// The EPA polytope of the task stage as it lies in LDS: plain data, no HIP.
// qpik_device.hpp has the functions that grow it; lds_plan.hpp lays the
// candidate list and the geometry poses over some of its fields, and the
// asserts below are what that overlay relies on.
#pragma once

#include <cstddef>
#include <cstdint>

#include "model.hpp"

namespace drc_amd {

// caps: hpp-fcl's GJKSolver defaults (epa_max_vertex_num 64,
// epa_max_face_num 128, epa_max_iterations 255), mirrored by the oracle
constexpr int kEpaMaxV = 64, kEpaMaxF = 128;
static_assert(kEpaMaxF == 128, "face bit masks are two 64-bit words");
static_assert(kEpaMaxF <= 256 && kEpaMaxV <= 127, "EpaPoly's 8-bit face and horizon fields");
struct EpaPoly {
  double vw[kEpaMaxV][3], va[kEpaMaxV][3];
  double fn[kEpaMaxF][3], fd[kEpaMaxF];
  // narrow index types (faces < 128, edges < 3, vertices and horizon positions
  // < 64): the polytope is most of the task kernel's per-wave LDS
  // From fn to alive: written only once EPA runs, after the last GJK candidate
  // is consumed.  The task plan lays the candidate list and the geometry poses
  // over these fields (lds_plan.hpp plan_kinematics); what the candidate GJKs
  // write (epa_stash: vertex slots, out[], nv) lies outside them.
  int16_t adj[kEpaMaxF][3];  // neighbour across edge e: face | (its edge << 8)
  int16_t hl[kEpaMaxV];      // a step's horizon edges: face | (edge << 8)
  uint8_t fv[kEpaMaxF][3];
  uint8_t freel[kEpaMaxF];  // recycled slots, last freed first
  int8_t vout[kEpaMaxV], vin[kEpaMaxV];  // horizon edge leaving / entering each vertex (-1: none)
  int8_t alive[kEpaMaxF];
  double out[6];
  int nv, nf, fail, stop, nfree;
};

// The polytope in the task plan, in doubles: its footprint (kEpaWideDoubles:
// the footprint before its index fields were narrowed, which the wide plan
// keeps so that it has the former size and residency: A/B runs), and where the
// face planes and out[] begin.
constexpr int kEpaDoubles = (static_cast<int>((sizeof(EpaPoly) + 7) / 8) + 1) & ~1, kEpaWideDoubles = 1178;
constexpr int kEpaFnDoubles = static_cast<int>(offsetof(EpaPoly, fn) / 8);
constexpr int kEpaOutDoubles = static_cast<int>(offsetof(EpaPoly, out) / 8);
static_assert(sizeof(EpaPoly) <= kEpaWideDoubles * 8, "the wide plan's polytope footprint");
// The int list of the GJK candidates lies in the face planes (fn, fd): the
// candidate GJKs write the EPA seed stash (epa_stash: vertex slots
// kEpaStashV0.., out[], nv) while later candidates are still being read, so the
// list must not overlap those; the face planes are only written once EPA
// starts, after the last candidate is consumed
static_assert(offsetof(EpaPoly, fn) % 8 == 0 && offsetof(EpaPoly, fd) == offsetof(EpaPoly, fn) + sizeof(EpaPoly::fn),
              "face planes: one contiguous double-aligned region");
static_assert(sizeof(EpaPoly::fn) + sizeof(EpaPoly::fd) >= kMaxPairs * sizeof(int),
              "the face planes hold a candidate list of kMaxPairs ints");
static_assert(offsetof(EpaPoly, fn) >= sizeof(EpaPoly::vw) + sizeof(EpaPoly::va) &&
                  offsetof(EpaPoly, out) >= offsetof(EpaPoly, fd) + sizeof(EpaPoly::fd) &&
                  offsetof(EpaPoly, nv) > offsetof(EpaPoly, out),
              "stash (vw / va slots, out[], nv) outside the candidate list");
// ... and with the geometry poses under the polytope, poses and list may share
// bytes only with fields EPA writes later, [fn, out)
static_assert(offsetof(EpaPoly, out) % 8 == 0 && offsetof(EpaPoly, out) > offsetof(EpaPoly, alive) &&
                  offsetof(EpaPoly, alive) > offsetof(EpaPoly, adj) && offsetof(EpaPoly, hl) > offsetof(EpaPoly, fd) &&
                  offsetof(EpaPoly, fv) > offsetof(EpaPoly, fd) && offsetof(EpaPoly, freel) > offsetof(EpaPoly, fd) &&
                  offsetof(EpaPoly, vout) > offsetof(EpaPoly, fd) && offsetof(EpaPoly, vin) > offsetof(EpaPoly, fd) &&
                  offsetof(EpaPoly, adj) == offsetof(EpaPoly, fd) + sizeof(EpaPoly::fd),
              "fn .. alive: the fields EPA writes after the last candidate, then out[] and the counters");

}  // namespace drc_amd
