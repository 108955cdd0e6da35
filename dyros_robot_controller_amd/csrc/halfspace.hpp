// Distance between a primitive (sphere, cylinder, box) and a half-space, in
// closed form.  Reference: no counterpart (the reference's getMinDistance is a
// self-collision query; obstacle slots are this project's).
//
// The half-space of a pose (R, p) is the solid {x : (x - p) . n <= 0} with
// n = R e_z.  For a convex shape with centre c, rotation R_g and support
// function h,
//   d = n . (c - p) - h(-n)
//     sphere   h = r
//     cylinder h = (h/2) |n . a| + r sqrt(1 - (n . a)^2),   a = R_g e_z
//     box      h = sum_i e_i |n . R_g e_i|
// positive when separated, negative by the penetration depth otherwise: exact
// on both sides, no iteration.  The shape's witness is its support point
// towards -n -- the centre of the support set where that is a cap, a face or an
// edge -- and the half-space's witness its projection onto the plane, so the
// two differ by d n and the task stage's dist_grad (which normalises their
// difference and flips the sign under penetration) yields n^T J(witness) on
// both sides of the plane.
//
// Plain host / device code without wave intrinsics: the task stage's obstacle
// build calls it in pass 1 (task_stage.hpp), tools/halfspace_host_test.cpp
// compiles it with the host compiler (tests/test_halfspace_host.py).
#pragma once

#include <cmath>

#ifndef DRC_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define DRC_HD __host__ __device__
#else
#define DRC_HD
#endif
#endif

namespace drc_amd {

// type: 0 sphere (p0 = r), 1 cylinder (p0 = r, p1 = h/2, axis z), 2 box (half
// extents p0..p2).  T, P: poses of the shape and of the half-space, 12 values
// each: the rotation row-major, then the origin (any pointer-like type).
// Returns d; ps[3] the shape's witness, pp[3] the half-space's.
template <class PT, class PP>
DRC_HD inline double halfspace_distance(int type, PT T, double p0, double p1, double p2, PP P, double* ps,
                                        double* pp) {
  const double n[3] = {P[2], P[5], P[8]};  // R e_z
  // -n in the shape's frame: component i is -n . R_g e_i
  double dl[3];
  for (int i = 0; i < 3; ++i) dl[i] = -(T[i] * n[0] + T[3 + i] * n[1] + T[6 + i] * n[2]);
  double loc[3] = {0.0, 0.0, 0.0};  // support point towards -n, shape frame
  double h = 0.0;
  if (type == 0) {
    h = p0;
    for (int i = 0; i < 3; ++i) loc[i] = p0 * dl[i];
  } else if (type == 1) {
    const double rho = sqrt(dl[0] * dl[0] + dl[1] * dl[1]);  // sqrt(1 - (n . a)^2)
    h = p1 * fabs(dl[2]) + p0 * rho;
    const double f = rho > 0.0 ? p0 / rho : 0.0;  // n along the axis: the cap's centre
    loc[0] = f * dl[0];
    loc[1] = f * dl[1];
    loc[2] = dl[2] > 0.0 ? p1 : (dl[2] < 0.0 ? -p1 : 0.0);  // n across the axis: the side line's centre
  } else {
    const double e[3] = {p0, p1, p2};
    for (int i = 0; i < 3; ++i) {
      h += e[i] * fabs(dl[i]);
      loc[i] = dl[i] > 0.0 ? e[i] : (dl[i] < 0.0 ? -e[i] : 0.0);  // a zero component: the face's / edge's centre
    }
  }
  const double d = n[0] * (T[9] - P[9]) + n[1] * (T[10] - P[10]) + n[2] * (T[11] - P[11]) - h;
  for (int r = 0; r < 3; ++r) {
    ps[r] = T[3 * r] * loc[0] + T[3 * r + 1] * loc[1] + T[3 * r + 2] * loc[2] + T[9 + r];
    pp[r] = ps[r] - d * n[r];
  }
  return d;
}

}  // namespace drc_amd
