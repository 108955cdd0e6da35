// Task stage of one instance (one wavefront): FK, frame Jacobian, task
// velocity, manipulability + gradient, self-collision distance + gradient
// (and the QPID / closed-form extras), ending in the task record or the
// stage outputs.  Used by task_kernel (task_kernel.hip) and the fused
// task + QP kernel (fused_kernel.hip).
//   FK / LWA frame Jacobian        robot_data.cpp:101-107,392-402
//   task error (+ cubic profile)   math_type_define.h:633-687, robot_controller.cpp:292-317
//   manipulability + gradient      robot_data.cpp:519-553 (MoMa :439-475)
//   min self-distance + gradient   robot_data.cpp:424-494 (hpp-fcl GJK/EPA semantics)
//   QPID stage data, CLIK / OSF    robot_data.cpp:109,476-512, robot_controller.cpp:150-260
#pragma once

#include "halfspace.hpp"
#include "kernel_common.hpp"

namespace drc_amd {

// ------------------------------------------------------------------------
// QPID stage data.  Pinocchio's LOCAL_WORLD_ALIGNED
// Jacobian time variation is d/dt of the LWA Jacobian (robot_data.cpp:109,
// 414, 476-477).  Column c of the Jacobian of a point p carried by a body,
// differentiated with the joint velocities restricted to `mask`:
//   revolute c:  [zd x (p - o_c) + z_c x (pdot - od_c); zd],  zd = w_par(c) x z_c
//   prismatic c: [zd; 0]
// with w_par(c) the angular velocity of c's parent body and od_c the velocity
// of c's origin.  One lane per column, O(nv) per lane.
// ------------------------------------------------------------------------
__device__ __forceinline__ void col_dot(const DevModel* M, const double* T, const double* Zw, const double* qd, int nv,
                                        int c, V3 p, V3 pdot, uint32_t mask, V3* lin, V3* ang) {
  const V3 oc = v3(T[12 * c + 9], T[12 * c + 10], T[12 * c + 11]), zc = ld3(Zw + 3 * c);
  V3 w = v3(0, 0, 0), od = v3(0, 0, 0);
  const uint32_t ac = M->anc[c] & mask;
  for (int a = 1; a <= nv; ++a) {
    if (!(ac & (1u << (a - 1)))) continue;
    const V3 za = ld3(Zw + 3 * a);
    if (M->jtype[a] == kRevolute) {
      if (a != c) w = w + qd[a - 1] * za;
      od = od + qd[a - 1] * cross(za, oc - v3(T[12 * a + 9], T[12 * a + 10], T[12 * a + 11]));
    } else {
      od = od + qd[a - 1] * za;
    }
  }
  const V3 zd = cross(w, zc);
  if (M->jtype[c] == kRevolute) {
    *lin = cross(zd, p - oc) + cross(zc, pdot - od);
    *ang = zd;
  } else {
    *lin = zd;
    *ang = v3(0, 0, 0);
  }
}

// velocity and angular velocity of the body of joint X (point p on it)
__device__ __forceinline__ void body_velocity(const DevModel* M, const double* T, const double* Zw, const double* qd,
                                              int nv, int X, V3 p, V3* v, V3* w) {
  *v = v3(0, 0, 0);
  *w = v3(0, 0, 0);
  if (X <= 0) return;
  const uint32_t ax = M->anc[X];
  for (int a = 1; a <= nv; ++a) {
    if (!(ax & (1u << (a - 1)))) continue;
    const V3 za = ld3(Zw + 3 * a);
    if (M->jtype[a] == kRevolute) {
      *w = *w + qd[a - 1] * za;
      *v = *v + qd[a - 1] * cross(za, p - v3(T[12 * a + 9], T[12 * a + 10], T[12 * a + 11]));
    } else {
      *v = *v + qd[a - 1] * za;
    }
  }
}

// Fills kBias = [Jdot v (6), man_gd, dist_gd] and kJd (6 x nv frame Jdot):
//   v = qdot (manipulator) or S eta (MoMa, getJacobianActuatedTimeVariation *
//       eta, mobile_manipulator/robot_data.cpp:412-415, Sdot neglected);
//   man_gd  = getManipulability(true,true).grad_dot . qdot_arm, contracted:
//       sum_i qdot_i dJ_i = Da (arm-only Jdot), so with W = Ja^T Ai
//       man_gd = mdot tr(Da W) + m [tr(Da Jda^T Ai) - 2 tr((Da W)(Jda W))],
//       mdot = m tr(Jda W)           (robot_data.cpp:555-569, MoMa :477-492);
//   dist_gd = getMinDistance(..,true,..).grad_dot . qdot_arm
//       = sum_{c in arm} qdot_c n.(JB_dot - JA_dot)[:, c]   (robot_data.cpp:496-512).
// full: also the reference's grad_dot VECTORS (stage outputs) into kGdv =
//   [getManipulability grad_dot (narm) | getMinDistance grad_dot (nv)].

__device__ __noinline__ void qpid_task_extras(const DevModel* M, const KParams& kp, double* S, double bestd,
                                              int besti, bool full) {
  const int l = lane_id(), nv = kp.nv, narm = kp.narm, c0 = kp.c0;
  const double *T = S + kp.kT, *Zw = S + kp.kZ, *J = S + kp.kJ, *qd = S + kp.kqd, *Te = S + kp.kTe,
               *red = S + kp.oRed, *W = S + kp.kW, *Ai = S + kp.kAi, *qv = S + kp.kq;
  double *Jd = S + kp.kJd, *Da = S + kp.kDa, *vf = S + kp.kVf, *X = S + kp.kX6, *out = S + kp.kBias;
  const uint32_t all = 0xffffffffu, arm = ((1u << narm) - 1) << c0;
  const uint32_t anc_e = M->anc[kp.frame_joint];
  const V3 pe = v3(Te[9], Te[10], Te[11]);
  V3 ve = v3(0, 0, 0), va = v3(0, 0, 0);  // frame-point velocity: full / arm joints only
  for (int c = 0; c < nv; ++c) {
    const V3 jc = v3(J[c], J[nv + c], J[2 * nv + c]);
    ve = ve + qd[c] * jc;
    if (arm & (1u << c)) va = va + qd[c] * jc;
  }
  double dsum = 0;
  const double(*Jm)[kMaxWheels] = mobile_jac(M, kp, S, qv);  // read for mobile manipulators only
  if (l < nv) {
    const int j = l + 1;
    V3 lin = v3(0, 0, 0), ang = v3(0, 0, 0), lina = v3(0, 0, 0), anga = v3(0, 0, 0);
    if (anc_e & (1u << l)) {
      col_dot(M, T, Zw, qd, nv, j, pe, ve, all, &lin, &ang);
      if (arm & (1u << l)) col_dot(M, T, Zw, qd, nv, j, pe, va, arm, &lina, &anga);
    }
    Jd[0 * nv + l] = lin.x; Jd[1 * nv + l] = lin.y; Jd[2 * nv + l] = lin.z;
    Jd[3 * nv + l] = ang.x; Jd[4 * nv + l] = ang.y; Jd[5 * nv + l] = ang.z;
    if (arm & (1u << l)) {
      const int c = l - c0;
      Da[0 * narm + c] = lina.x; Da[1 * narm + c] = lina.y; Da[2 * narm + c] = lina.z;
      Da[3 * narm + c] = anga.x; Da[4 * narm + c] = anga.y; Da[5 * narm + c] = anga.z;
    }
    // actuated velocity mapped to the joints: S eta (MoMa robot_data.cpp:115-120)
    double v = qd[l];
    if (M->kind == 1 && l >= M->virtual_start && l < M->virtual_start + 3) {
      const int r = l - M->virtual_start;
      const double yaw = qv[M->virtual_start + 2], cy = cos(yaw), sy = sin(yaw);
      v = 0;
      for (int w = 0; w < M->n_wheel; ++w) {
        const double j0 = Jm[0][w], j1 = Jm[1][w], j2 = Jm[2][w];
        const double sw = r == 0 ? cy * j0 - sy * j1 : (r == 1 ? sy * j0 + cy * j1 : j2);
        v += sw * qd[M->mobi_start + w];
      }
    }
    vf[l] = v;
    // self-collision grad_dot of this column (robot_data.cpp:496-512)
    double gcol = 0;
    if (besti < M->npairs && (full || (arm & (1u << l)))) {
      const V3 pA = ld3(red), pB = ld3(red + 3);
      V3 n = pB - pA;
      n = (1.0 / sqrt(dot(n, n))) * n;
      V3 jdx[2];
      for (int s_ = 0; s_ < 2; ++s_) {
        const int jX = M->gparent[s_ == 0 ? M->pair_a[besti] : M->pair_b[besti]];
        jdx[s_] = v3(0, 0, 0);
        if (jX <= 0 || !(M->anc[jX] & (1u << l))) continue;
        const V3 oX = v3(T[12 * jX + 9], T[12 * jX + 10], T[12 * jX + 11]);
        const V3 pX = s_ == 0 ? pA : pB, zj = ld3(Zw + 3 * j);
        V3 cl, ca;  // column of the joint Jacobian of jX at oX
        if (M->jtype[j] == kRevolute) {
          cl = cross(zj, oX - v3(T[12 * j + 9], T[12 * j + 10], T[12 * j + 11]));
          ca = zj;
        } else {
          cl = zj;
          ca = v3(0, 0, 0);
        }
        V3 vX, wX, ld, ad;
        body_velocity(M, T, Zw, qd, nv, jX, oX, &vX, &wX);
        col_dot(M, T, Zw, qd, nv, j, oX, vX, all, &ld, &ad);
        const V3 r = pX - oX, rd = cross(wX, r);
        jdx[s_] = ld - (cross(rd, ca) + cross(r, ad));
      }
      gcol = dot(n, jdx[1] - jdx[0]);
      if (arm & (1u << l)) dsum = qd[l] * gcol;
    }
    if (full) S[kp.kGdv + narm + l] = gcol;
  }
  const double dist_gd = wave_sum(dsum);
  (void)bestd;
  wsync();
  // 6x6 products for the manipulability term (lanes (a, b))
  double t1 = 0, t2 = 0, t3 = 0;
  if (l < 36) {
    const int a = l / 6, b = l % 6;
    double x1 = 0, x2 = 0, x3 = 0;
    for (int c = 0; c < narm; ++c) {
      const double dac = Da[a * narm + c], jac = Jd[a * nv + c0 + c];
      x1 += dac * W[c * 6 + b];
      x2 += jac * W[c * 6 + b];
      x3 += dac * Jd[b * nv + c0 + c];
    }
    X[l] = x1;
    X[36 + l] = x2;
    if (a == b) {
      t1 = x2;
      t2 = x1;
    }
    t3 = x3 * Ai[b * 6 + a];
  }
  wsync();
  double t4 = 0;
  if (l < 36) t4 = X[l] * X[36 + (l % 6) * 6 + l / 6];
  t1 = wave_sum(t1);
  t2 = wave_sum(t2);
  t3 = wave_sum(t3);
  t4 = wave_sum(t4);
  const double m = S[kp.oSc + SC_MAN], mdot = m * t1;
  if (l < 6) {
    double s = 0;
    for (int c = 0; c < nv; ++c) s += Jd[l * nv + c] * vf[c];
    out[l] = s;
  }
  if (l == 0) {
    out[6] = mdot * t2 + m * (t3 - 2.0 * t4);
    out[7] = dist_gd;
  }
  if (full) {
    // grad_dot_k = mdot tr(dJ_k Ja^T Ai) + m tr(dJ_k (Jda^T Ai + Ja^T Ai_dot)),
    // Ja^T Ai_dot = -2 W (Jda W) = -2 W X2; lane per (k, c) builds dJ_k[:, c]
    // (the manipulability gradient's closed form) and dots it with the rows.
    double* Y = X + 72;  // narm x 6: Jda^T Ai - 2 W X2
    for (int e = l; e < narm * 6; e += 64) {
      const int c = e / 6, a = e % 6;
      double y = 0;
      for (int b_ = 0; b_ < 6; ++b_) y += Jd[b_ * nv + c0 + c] * Ai[b_ * 6 + a] - 2.0 * W[c * 6 + b_] * X[36 + b_ * 6 + a];
      Y[e] = y;
    }
    wsync();
    double* part = X + 72 + 6 * narm;  // narm x narm x 2
    for (int e = l; e < narm * narm; e += 64) {
      const int kk = e / narm, c = e % narm, jk = c0 + kk + 1, ji = c0 + c + 1;
      double p1 = 0, p2 = 0;
      if ((anc_e & (1u << (jk - 1))) && (anc_e & (1u << (ji - 1)))) {
        const V3 zk = ld3(Zw + 3 * jk), zi = ld3(Zw + 3 * ji);
        const V3 pk_ = v3(T[12 * jk + 9], T[12 * jk + 10], T[12 * jk + 11]);
        const V3 pi_ = v3(T[12 * ji + 9], T[12 * ji + 10], T[12 * ji + 11]);
        const bool krev = M->jtype[jk] == kRevolute;
        const V3 dpe = krev ? cross(zk, pe - pk_) : zk;
        const bool moves_i = jk != ji && (M->anc[ji] & (1u << (jk - 1)));
        const V3 dzi = (moves_i && krev) ? cross(zk, zi) : v3(0, 0, 0);
        const V3 dpi = moves_i ? (krev ? cross(zk, pi_ - pk_) : zk) : v3(0, 0, 0);
        V3 lin, ang;
        if (M->jtype[ji] == kRevolute) {
          lin = cross(dzi, pe - pi_) + cross(zi, dpe - dpi);
          ang = dzi;
        } else {
          lin = dzi;
          ang = v3(0, 0, 0);
        }
        const double *w = W + c * 6, *y = Y + c * 6;
        p1 = lin.x * w[0] + lin.y * w[1] + lin.z * w[2] + ang.x * w[3] + ang.y * w[4] + ang.z * w[5];
        p2 = lin.x * y[0] + lin.y * y[1] + lin.z * y[2] + ang.x * y[3] + ang.y * y[4] + ang.z * y[5];
      }
      part[2 * e] = p1;
      part[2 * e + 1] = p2;
    }
    wsync();
    if (l < narm) {
      double s1 = 0, s2 = 0;
      for (int c = 0; c < narm; ++c) {
        s1 += part[2 * (l * narm + c)];
        s2 += part[2 * (l * narm + c) + 1];
      }
      S[kp.kGdv + l] = mdot * s1 + m * s2;
    }
  }
  wsync();
}

// ------------------------------------------------------------------------
// Closed-form controllers, Manipulator::RobotController
// (robot_controller.cpp:156-275), on the task stage's J and task vector
// (xdd: CLIK Kp e + xdot_target; OSF Kp e + Kv edot, or xddot_target):
//   CLIK: qdot = J^+ xdd + (I - J^+ J) nu,              J^+ = PinvCOD(J)
//   OSF:  Lambda = PinvCOD(J M^-1 J^T), tau = J^T Lambda xdd + (I - J^T Lambda J M^-1) nu + g
// Small dense products are lane-parallel; a 6x6 SPD inverse goes through six
// lane-parallel Jordan exchanges when the Frobenius condition estimate
// certifies that PinvCOD keeps every mode (< 1e5), otherwise one lane runs the
// serial COD (PinvCOD's rank cut).
// ------------------------------------------------------------------------
__device__ __forceinline__ bool inv6_certified(const double* A, double* Ai) {
  const int l = lane_id(), ii = l / 6, jj = l % 6;
  if (l < 36) Ai[l] = A[l];
  wsync();
  double piv_min = 1e300;
  for (int k = 0; k < 6; ++k) {
    const double akk = Ai[k * 6 + k];
    double nv_ = 0;
    if (l < 36) {
      const double aij = Ai[l], aik = Ai[ii * 6 + k], akj = Ai[k * 6 + jj];
      if (ii == k && jj == k) nv_ = 1.0 / akk;
      else if (ii == k) nv_ = akj / akk;
      else if (jj == k) nv_ = -aik / akk;
      else nv_ = aij - aik * akj / akk;
    }
    piv_min = fmin(piv_min, akk);
    wsync();
    if (l < 36) Ai[l] = nv_;
    wsync();
  }
  const double fa = wave_sum(l < 36 ? A[l] * A[l] : 0.0), fi = wave_sum(l < 36 ? Ai[l] * Ai[l] : 0.0);
  return piv_min > 0 && fa * fi < 1e10;
}

__device__ __noinline__ void closed_form_stage(const DevModel* M, const KParams& kp, double* S, const IO& io,
                                               int64_t gb, int64_t LD) {
  const int l = lane_id(), nv = kp.nv;
  const double *J = S + kp.kJ, *xdd = S + kp.kxdd;
  double* A6 = S + kp.kA6;
  double* Ai = S + kp.kAi;
  double* W = S + kp.kCf;           // 6 x nv: J^+ ^T (CLIK) / J M^-1 (OSF)
  double* W2 = W + 6 * nv;          // 6 x nv: Lambda J M^-1 (OSF)
  double* Mi = W2 + 6 * nv;         // nv x nv
  double* nu = Mi + nv * nv;        // nv
  double* gv = nu + nv;             // nv
  double* vec = gv + 2 * nv;        // 48: task vectors
  double* ws = vec + 48;            // serial COD work
  if (l < nv) {
    nu[l] = io.cf_null ? io.cf_null[(int64_t)l * LD + gb] : 0.0;
    if (kp.cf == 2) gv[l] = io.dG[(int64_t)l * LD + gb];
  }
  if (kp.cf == 2)
    for (int e = l; e < nv * nv; e += 64) Mi[e] = io.dM[(int64_t)e * LD + gb];
  wsync();
  double out = 0;
  if (kp.cf == 1) {  // CLIK (robot_controller.cpp:156-172)
    if (l < 36) {
      const int a = l / 6, b = l % 6;
      double s = 0;
      for (int c = 0; c < nv; ++c) s += J[a * nv + c] * J[b * nv + c];
      A6[l] = s;
    }
    wsync();
    if (inv6_certified(A6, Ai)) {  // J^+ = J^T (J J^T)^-1, stored transposed: W[i][c] = J^+[c][i]
      for (int e = l; e < 6 * nv; e += 64) {
        const int i = e / nv, c = e % nv;
        double s = 0;
        for (int r = 0; r < 6; ++r) s += J[r * nv + c] * Ai[r * 6 + i];
        W[e] = s;
      }
    } else if (l == 0) {
      double* X = ws + 6 * nv + 36 + 6 * nv + 18 + 2 * nv;  // nv x 6 after the COD work
      pinv_cod_rect(J, 6, nv, X, ws);
      for (int c = 0; c < nv; ++c)
        for (int i = 0; i < 6; ++i) W[i * nv + c] = X[c * 6 + i];
    }
    wsync();
    if (l < 6) {
      double s = 0;
      for (int c = 0; c < nv; ++c) s += J[l * nv + c] * nu[c];
      vec[l] = xdd[l] - s;  // xdd - J nu
    }
    wsync();
    if (l < nv) {
      double s = nu[l];
      for (int i = 0; i < 6; ++i) s += W[i * nv + l] * vec[i];
      out = s;
    }
  } else {  // OSF (robot_controller.cpp:216-230)
    for (int e = l; e < 6 * nv; e += 64) {
      const int i = e / nv, c = e % nv;
      double s = 0;
      for (int a = 0; a < nv; ++a) s += J[i * nv + a] * Mi[a * nv + c];
      W[e] = s;
    }
    wsync();
    if (l < 36) {
      const int a = l / 6, b = l % 6;
      double s = 0;
      for (int c = 0; c < nv; ++c) s += W[a * nv + c] * J[b * nv + c];
      A6[l] = s;
    }
    wsync();
    if (!inv6_certified(A6, Ai)) pinv_cod6_wave(A6, Ai, ws);
    for (int e = l; e < 6 * nv; e += 64) {
      const int i = e / nv, c = e % nv;
      double s = 0;
      for (int j = 0; j < 6; ++j) s += Ai[i * 6 + j] * W[j * nv + c];
      W2[e] = s;
    }
    if (l < 6) {
      double s = 0;
      for (int j = 0; j < 6; ++j) s += Ai[l * 6 + j] * xdd[j];
      vec[l] = s;  // F = Lambda xdd
    }
    wsync();
    if (l < 6) {
      double s = 0;
      for (int c = 0; c < nv; ++c) s += W2[l * nv + c] * nu[c];
      vec[6 + l] = vec[l] - s;  // F - J_T_pinv nu
    }
    wsync();
    if (l < nv) {
      double s = gv[l] + nu[l];
      for (int i = 0; i < 6; ++i) s += J[i * nv + l] * vec[6 + i];
      out = s;
    }
  }
  if (l < nv) io.out[(int64_t)l * LD + gb] = out;
  wsync();
}

// Model tables of the wave task stage (model.cpp build_stage_tables): what the
// stages would otherwise gather per instance through dependent loads
// (pair_order -> slot_a / slot_b -> gtype / gparam -> gbound; jtype / anc by a
// lane's joint index, each feeding a branch).
#ifdef __HIP_DEVICE_COMPILE__
typedef __attribute__((address_space(1))) const double glb_cdouble;
#else
typedef const double glb_cdouble;
#endif
struct PairTab {
  glb_cdouble* t;
  int ld;
};
__device__ __forceinline__ PairTab pair_tab(const DevModel* M) { return PairTab{(glb_cdouble*)M->pair_tab, M->pair_ld}; }
struct PairRec {
  int p, ga, gb, ta, tb;
  double pa[3], pb[3], ba, bb;
};
// record of slot sl of pair_order: nine independent loads, consecutive lanes
// on consecutive addresses
__device__ __forceinline__ PairRec pair_rec(const PairTab& pt, int i) {
  glb_cdouble* t = pt.t + i;
  PairRec r;
  const unsigned long long m = static_cast<unsigned long long>(__double_as_longlong(t[kPairMeta * pt.ld]));
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    r.pa[k] = t[(kPairParamA + k) * pt.ld];
    r.pb[k] = t[(kPairParamB + k) * pt.ld];
  }
  r.ba = t[kPairBoundA * pt.ld];
  r.bb = t[kPairBoundB * pt.ld];
  r.p = static_cast<int>(m & 0xffffu);
  r.ga = static_cast<int>((m >> 16) & 0xffu);
  r.gb = static_cast<int>((m >> 24) & 0xffu);
  r.ta = static_cast<int>((m >> 32) & 0xfu);
  r.tb = static_cast<int>((m >> 36) & 0xfu);
  return r;
}
// joint k supports joint j (anc[j] bit k - 1), from DevModel::anc_bits held in SGPRs
struct AncBits {
  uint64_t w[4];
};
__device__ __forceinline__ AncBits anc_bits(const DevModel* M) {
  return AncBits{{M->anc_bits[0], M->anc_bits[1], M->anc_bits[2], M->anc_bits[3]}};
}
__device__ __forceinline__ bool supports(const AncBits& ab, int k, int j) {
  const int bit = 16 * (j - 1) + (k - 1), w = bit >> 6;
  const uint64_t x = w == 0 ? ab.w[0] : (w == 1 ? ab.w[1] : (w == 2 ? ab.w[2] : ab.w[3]));
  return (x >> (bit & 63)) & 1u;
}
__device__ __forceinline__ bool revolute(uint32_t rev_mask, int j) { return (rev_mask >> (j - 1)) & 1u; }

// Pose of a geometry (R row-major | p): a link's geometry rides on its joint's
// frame; an obstacle slot's is the call's pose (R column-major there, no
// product).  The geometry-pose stage and the pose pairs that EPA and the
// winner's refinement form again go through these, so that both have the
// same bits from one source expression.
__device__ __forceinline__ void link_geom_pose(const double* T, int gpar, const double* gpl, double* dst) {
  double out[12];
  tmul(T + 12 * gpar, gpl, out);
  for (int i = 0; i < 12; ++i) dst[i] = out[i];
}
__device__ __forceinline__ void slot_geom_pose(const double* opl, double* dst) {
#pragma unroll
  for (int i = 0; i < 9; ++i) dst[i] = opl[(i % 3) * 3 + i / 3];
#pragma unroll
  for (int i = 9; i < 12; ++i) dst[i] = opl[i];
}

// The poses of geometries g0 and g1 into d0 and d1 (12 each), by the calling
// lane (gb: the instance's position in the call's arrays).  Out of line: it is
// called only in the branch of an instance that runs EPA, and the stage's
// register allocation should not see it.
template <bool OBST>
__device__ __noinline__ void pose_pair(const DevModel* M, const double* T, double* d0, double* d1, int g0, int g1,
                                       [[maybe_unused]] const ObstIn ob, [[maybe_unused]] int obst0,
                                       [[maybe_unused]] int64_t gb) {
  for (int s_ = 0; s_ < 2; ++s_) {
    const int g = s_ == 0 ? g0 : g1;
    double* dst = s_ == 0 ? d0 : d1;
    bool slot = false;
    if constexpr (OBST) {
      if (g >= obst0) {  // the call's pose again, as the state-in loads read it
        slot = true;
        const int64_t os = ob.ld ? ob.ld : 1;
        const double* op = ob.pose + (int64_t)(g - obst0) * 12 * os + (ob.ld ? gb : 0);
        double o[12];
        for (int i = 0; i < 12; ++i) o[i] = op[i * os];
        slot_geom_pose(o, dst);
      }
    }
    if (!slot) {
      double gp[12];
      for (int i = 0; i < 12; ++i) gp[i] = M->gplace[g][i];
      link_geom_pose(T, M->gparent[g], gp, dst);
    }
  }
}

// One instance b of the task stage on this wave (S: the wave's LDS plan kp).
// PROBLEM 0: QPIK stage data; 1: also the QPID extras; 2: closed-form CLIK / OSF;
// 3: the distance stage alone (clearance_kernel.hip): FK chain, geometry poses,
// pass 1, the candidate passes, EPA and the winner's refinement -- no targets,
// frame Jacobian, task velocity, manipulability, grad d or record.  Its state
// is what the caller left in the plan's kq (io.q is not read), and its result
// stays in the plan: SC_DIST and SC_PAIR hold what the QPIK stage returns as
// dist[0] and pair.  What it skips is switched off by the compile-time kTask
// inside the statements' own conditions, never by a scope around them: the
// other instantiations see the same scopes, hence the same lifetimes, and
// compile to what they were (DESIGN.md "Path clearance").
// MESH: the model has convex-hull geometry (GeomType kMesh).  A build of its
// own, chosen at launch, so the kernels of mesh-free models carry none of it.
// OBST: the model has obstacle slots (DevModel::nobst): geometries whose pose is
// an input of the call (ob), among them half-spaces, which pass 1 decides
// in closed form (halfspace.hpp).  A build of its own again; not with MESH.
// RATE (with OBST, QPIK only): the slots move with the call's twists (rt), and
// the distance the QP reads carries the winner's dd/dt: the record's distance
// slot holds d + (dd/dt) / alpha_cbf, so that the QP's row -alpha (d - dist_min)
// becomes -alpha (d - dist_min) - dd/dt without a change to the QP.  The
// stage outputs keep the geometric d; dd/dt is an output of its own (rt.rate).
template <int PROBLEM, bool MESH = false, bool OBST = false, bool RATE = false>
__device__ __forceinline__ void task_instance(const DevModel* __restrict__ M0, const KParams& kp, const IO& io, double* S,
                                              int64_t b, [[maybe_unused]] const ObstIn ob = ObstIn(),
                                              [[maybe_unused]] const RateIn rt = RateIn()) {
  constexpr bool kTask = PROBLEM != 3;  // the task data around the distance stage
  const int l = lane_id();
  const int nv = kp.nv;
  EpaPoly* ews = reinterpret_cast<EpaPoly*>(S + kp.kEpa);  // LDS-resident polytope
  PH_DECL
  const int64_t gb = io.b0 + b, LD = io.ld;  // position in the caller's [field][B] arrays
  PH_ONLY(const unsigned long long inst_t0 = __builtin_amdgcn_s_memtime(); unsigned long long ph_snap[8];
          for (int k_ = 0; k_ < 8; ++k_) ph_snap[k_] = ph_acc[k_];
          unsigned long long epa_calls = 0, epa_steps = 0, epa_maxsteps = 0, epa_t[8] = {0, 0, 0, 0, 0, 0, 0, 0};)
  // re-derive the model pointer each instance: keeps LICM from hoisting
  // model-constant loads out of the instance loop into spilled registers
  const DevModel* M = opaque_model(M0);
  // ---------------- state in ----------------
  double* qv = S + kp.kq;
  double* qd = S + kp.kqd;
  if (kTask && l < nv) {
    qv[l] = io.q[l * LD + gb];
    qd[l] = io.qdot[l * LD + gb];
  }
  // task targets, one value per lane (lanes 0-11 x_target, 12-17 xdot_target,
  // 18-29 x_init, 30-35 xdot_init): issued here so their latency overlaps the
  // FK; the task-velocity stage reads them by v_readlane
  // model constants of this lane's joint (and, before the chain, of its
  // geometry: kMaxGeoms = 64, one per lane), issued with the state loads so
  // that one memory latency covers them; lane 0 and the lanes past nv / ngeom
  // read entry 0 and drop it
  const uint32_t rev_mask = M->rev_mask;
  const int jm = l <= nv ? l : 0, gm = l < M->ngeom ? l : 0;
  double jpl[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) jpl[i] = M->jplace[jm][i];
  const V3 axl = ld3(M->axis[jm]);
  double tgt = 0.0;
  if (!kTask || (PROBLEM == 2 && kp.cf == 3)) {
    // kinematics only (drc_kinematics_batch), the distance stage alone: no task targets
  } else if (l < 12) {
    if (kp.mode != DRC_MODE_QPIK) tgt = io.xt[l * LD + gb];
  } else if (l < 18) {
    tgt = io.xdt[(l - 12) * LD + gb];
  } else if (l < 36 && kp.mode == DRC_MODE_QPIK_CUBIC) {
    tgt = l < 30 ? io.xi[(l - 18) * LD + gb] : io.xdi[(l - 30) * LD + gb];
  }
  // (OBST) the lane of an obstacle geometry: its pose's 12 values, issued with
  // the loads above so that the FK chain hides them.  Field-major like
  // x_target (consecutive instances on consecutive addresses); ld = 0 is
  // one pose set for the whole batch
  static_assert(!(MESH && OBST), "no obstacle build for hull models");
  static_assert(!RATE || (OBST && PROBLEM == 0), "obstacle twists: the QPIK stage of a model with slots");
  [[maybe_unused]] double opl[12];
  [[maybe_unused]] double otw[6];  // (RATE) the slot's twist: v of the pose origin, then omega
  [[maybe_unused]] const int obst0 = OBST ? M->obst0 : 0;
  if constexpr (OBST) {
    if (l >= obst0 && l < M->ngeom) {
      const int64_t os = ob.ld ? ob.ld : 1;
      const double* op = ob.pose + (int64_t)(l - obst0) * 12 * os + (ob.ld ? gb : 0);
#pragma unroll
      for (int i = 0; i < 12; ++i) opl[i] = op[i * os];
      if constexpr (RATE) {
        const int64_t ts = rt.ld ? rt.ld : 1;
        const double* tp = rt.twist + (int64_t)(l - obst0) * 6 * ts + (rt.ld ? gb : 0);
#pragma unroll
        for (int i = 0; i < 6; ++i) otw[i] = tp[i * ts];
      }
    }
  }
  wsync();
  // ---------------- FK: local joint transforms, then the chain ------------
  double* T = S + kp.kT;  // (nv+1) x 12
  double* Zw = S + kp.kZ;  // (nv+1) x 3
  if (l < 12) T[l] = (l == 0 || l == 4 || l == 8) ? 1.0 : 0.0;
  double* loc = S + kp.kTg;  // scratch: local transforms nv x 12 (before geometry poses)
  if (l >= 1 && l <= nv) {
    const int j = l;
    double Mj[12];
    const double ax[3] = {axl.x, axl.y, axl.z};
    const double qq = qv[j - 1];
    if (revolute(rev_mask, j)) {
      double c, s;
      sincos(qq, &s, &c);
      double C = 1 - c, x = ax[0], y = ax[1], z = ax[2];
      Mj[0] = c + x * x * C; Mj[1] = x * y * C - z * s; Mj[2] = x * z * C + y * s;
      Mj[3] = y * x * C + z * s; Mj[4] = c + y * y * C; Mj[5] = y * z * C - x * s;
      Mj[6] = z * x * C - y * s; Mj[7] = z * y * C + x * s; Mj[8] = c + z * z * C;
      Mj[9] = Mj[10] = Mj[11] = 0;
    } else {
      Mj[0] = Mj[4] = Mj[8] = 1;
      Mj[1] = Mj[2] = Mj[3] = Mj[5] = Mj[6] = Mj[7] = 0;
      Mj[9] = ax[0] * qq; Mj[10] = ax[1] * qq; Mj[11] = ax[2] * qq;
    }
    double Lj[12];
    tmul(jpl, Mj, Lj);
    for (int i = 0; i < 12; ++i) loc[(j - 1) * 12 + i] = Lj[i];
  }
  wsync();
  // this lane's geometry placement: in flight while the chain below runs
  double gpl[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) gpl[i] = M->gplace[gm][i];
  const int gpar = M->gparent[gm];
  for (int j = 1; j <= nv; ++j) {  // oMi[j] = oMi[parent] * local[j]; 12 lanes
    const double* a = T + M->parent[j] * 12;
    const double* bb = loc + (j - 1) * 12;
    double v = 0;
    if (l < 9) {
      int r = l / 3, c = l % 3;
      v = a[3 * r] * bb[c] + a[3 * r + 1] * bb[3 + c] + a[3 * r + 2] * bb[6 + c];
    } else if (l < 12) {
      int r = l - 9;
      v = a[3 * r] * bb[9] + a[3 * r + 1] * bb[10] + a[3 * r + 2] * bb[11] + a[9 + r];
    }
    wsync();
    if (l < 12) T[j * 12 + l] = v;
    wsync();
  }
  double* Te = S + kp.kTe;
  if (kTask && l >= 1 && l <= nv) st3(Zw + 3 * l, rot(T + 12 * l, axl));
  if (kTask && l == 0) tmul(T + 12 * kp.frame_joint, kp.frame_place, Te);
  wsync();
  // geometry poses
  double* Tg = S + kp.kTg;
  if (l < M->ngeom) {
    bool slot = false;
    if constexpr (OBST) {
      if (l >= obst0) {  // the call's pose is the geometry's row (R column-major -> row-major): no tmul
        slot = true;
        slot_geom_pose(opl, Tg + l * 12);
      }
    }
    if (!slot) link_geom_pose(T, gpar, gpl, Tg + l * 12);
  }
  PH(0);
  // ---------------- frame Jacobian (LWA), 6 x nv row-major -------------
  double* J = S + kp.kJ;
  // (PROBLEM 3 never writes Te and uses neither pe nor anc_e: dead there, not inputs of the distance stage)
  const V3 pe = v3(Te[9], Te[10], Te[11]);
  const uint32_t anc_e = M->anc[kp.frame_joint];
  if (kTask && l < nv) {
    const int j = l + 1;
    V3 lin = v3(0, 0, 0), ang = v3(0, 0, 0);
    if (anc_e & (1u << l)) {
      V3 z = ld3(Zw + 3 * j);
      if (revolute(rev_mask, j)) {
        lin = cross(z, pe - v3(T[12 * j + 9], T[12 * j + 10], T[12 * j + 11]));
        ang = z;
      } else {
        lin = z;
      }
    }
    J[0 * nv + l] = lin.x; J[1 * nv + l] = lin.y; J[2 * nv + l] = lin.z;
    J[3 * nv + l] = ang.x; J[4 * nv + l] = ang.y; J[5 * nv + l] = ang.z;
  }
  wsync();
  // ---------------- task velocity ---------------------------------------
  double* xdd = S + kp.kxdd;
  // getVelocity = J qdot (robot_data.cpp:419-422), row r on lane r
  double jq = 0.0;
  if (kTask && l < 6)
    for (int c = 0; c < nv; ++c) jq += J[l * nv + c] * qd[c];
  if (kTask && l == 0) {
    if (kp.mode == DRC_MODE_QPIK) {
      for (int i = 0; i < 6; ++i) xdd[i] = rd_lane(tgt, 12 + i);
    } else {
      double xt[12], xdt[6];
      for (int i = 0; i < 12; ++i) xt[i] = rd_lane(tgt, i);
      for (int i = 0; i < 6; ++i) xdt[i] = rd_lane(tgt, 12 + i);
      if (kp.mode == DRC_MODE_QPIK_CUBIC) {  // getTaskSpaceCubic (math_type_define.h:647)
        double xi[12], xdi[6], Rt[9], Ri[9];
        for (int i = 0; i < 12; ++i) xi[i] = rd_lane(tgt, 18 + i);
        for (int i = 0; i < 6; ++i) xdi[i] = rd_lane(tgt, 30 + i);
        for (int r = 0; r < 3; ++r)
          for (int c = 0; c < 3; ++c) {
            Rt[3 * r + c] = xt[3 * c + r];
            Ri[3 * r + c] = xi[3 * c + r];
          }
        const double t = kp.t, t0 = kp.t0, tf = kp.t0 + kp.duration;
        double pd[3], vd[3];
        for (int i = 0; i < 3; ++i) {
          pd[i] = cubic(t, t0, tf, xi[9 + i], xt[9 + i], xdi[i], xdt[i]);
          vd[i] = cubic_dot(t, t0, tf, xi[9 + i], xt[9 + i], xdi[i], xdt[i]);
        }
        double RiT_Rt[9], Rd[9];
        for (int a = 0; a < 3; ++a)
          for (int c = 0; c < 3; ++c)
            RiT_Rt[3 * a + c] = Ri[a] * Rt[c] + Ri[3 + a] * Rt[3 + c] + Ri[6 + a] * Rt[6 + c];
        V3 r = so3_log(RiT_Rt);
        if (t >= tf) {
          for (int i = 0; i < 9; ++i) Rd[i] = Rt[i];
        } else if (t < t0) {
          for (int i = 0; i < 9; ++i) Rd[i] = Ri[i];
        } else {
          double E3[9];
          so3_exp(cubic(t, t0, tf, 0, 1, 0, 0) * r, E3);
          for (int a = 0; a < 3; ++a)
            for (int c = 0; c < 3; ++c)
              Rd[3 * a + c] = Ri[3 * a] * E3[c] + Ri[3 * a + 1] * E3[3 + c] + Ri[3 * a + 2] * E3[6 + c];
        }
        V3 rd = v3(cubic_dot(t, t0, tf, 0, r.x, 0, 0), cubic_dot(t, t0, tf, 0, r.y, 0, 0),
                   cubic_dot(t, t0, tf, 0, r.z, 0, 0));
        rd = v3(Ri[0] * rd.x + Ri[1] * rd.y + Ri[2] * rd.z, Ri[3] * rd.x + Ri[4] * rd.y + Ri[5] * rd.z,
                Ri[6] * rd.x + Ri[7] * rd.y + Ri[8] * rd.z);
        double tau = (t - t0) / (tf - t0);
        if (tau < 0 || tau > 1) rd = v3(0, 0, 0);
        for (int r0 = 0; r0 < 3; ++r0)
          for (int c = 0; c < 3; ++c) xt[3 * c + r0] = Rd[3 * r0 + c];
        for (int i = 0; i < 3; ++i) {
          xt[9 + i] = pd[i];
          xdt[i] = vd[i];
        }
        xdt[3] = rd.x; xdt[4] = rd.y; xdt[5] = rd.z;
      }
      // getTaskSpaceError (math_type_define.h:633) with getPhi (:283)
      double e[6], xdot[6];
      for (int i = 0; i < 3; ++i) e[i] = xt[9 + i] - Te[9 + i];
      V3 phi = v3(0, 0, 0);
      for (int i = 0; i < 3; ++i)
        phi = phi + cross(v3(xt[3 * i], xt[3 * i + 1], xt[3 * i + 2]), v3(Te[i], Te[3 + i], Te[6 + i]));
      e[3] = -0.5 * phi.x; e[4] = -0.5 * phi.y; e[5] = -0.5 * phi.z;
      for (int r = 0; r < 6; ++r) xdot[r] = rd_lane(jq, r);
      for (int i = 0; i < 6; ++i)
        xdd[i] = kp.kp[i] * e[i] + kp.kv[i] * (xdt[i] - xdot[i]) + kp.ff * xdt[i];
    }
  }
  PH(1);
  if constexpr (PROBLEM == 2) {  // closed-form controllers: no CBF stages
    if (kp.cf == 3) {  // kinematics only: getPose / getJacobian / getVelocity (robot_data.cpp:378-422)
      if (io.st_pose && l < 12) io.st_pose[l * LD + gb] = l < 9 ? Te[(l % 3) * 3 + l / 3] : Te[l];
      if (io.st_jac)
        for (int e = l; e < 6 * nv; e += 64) io.st_jac[(int64_t)e * LD + gb] = J[e];
      if (io.st_xdd && l < 6) io.st_xdd[l * LD + gb] = jq;  // J qdot, row r on lane r
      wsync();
      return;
    }
    closed_form_stage(M, kp, S, io, gb, LD);
    PH_FLUSH(0);
    return;
  }
  // ---------------- manipulability (arm columns c0..c0+narm) -------------
  const int narm = kp.narm, c0 = kp.c0;
  double* A6 = S + kp.kA6;
  double* Ai = S + kp.kAi;
  if (kTask && l < 36) {
    int a = l / 6, bb = l % 6;
    double s = 0;
    for (int c = 0; c < narm; ++c) s += J[a * nv + c0 + c] * J[bb * nv + c0 + c];
    A6[l] = s;
  }
  wsync();
  if constexpr (kTask) {
    // JJ^T (SPD) inverted by six lane-parallel Jordan exchanges (36 lanes),
    // det = product of the pivots.  Ill-conditioned JJ^T (Frobenius
    // condition estimate >= 1e5) takes the serial COD path (rank by pivoted
    // QR, Moore-Penrose on the kept modes), matching DyrosMath::PinvCOD's
    // threshold semantics (math_type_define.h:563).
    // lane i < 6 holds row i in registers; the pivot row moves by
    // v_readlane (same element formulas as the LDS form it replaced)
    double piv_min = 1e300, det = 1;
    const int lr = l < 6 ? l : 0;
    double r6[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) r6[j] = A6[lr * 6 + j];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      const double akk = bcast(r6[k], k), aik = r6[k], ia = 1.0 / akk;  // one FP64 divide per pivot
      double pk6[6];
#pragma unroll
      for (int j = 0; j < 6; ++j) pk6[j] = bcast(r6[j], k);
#pragma unroll
      for (int j = 0; j < 6; ++j) {
        double v;
        if (l == k && j == k) v = ia;
        else if (l == k) v = pk6[j] * ia;
        else if (j == k) v = -aik * ia;
        else v = r6[j] - aik * (pk6[j] * ia);
        r6[j] = v;
      }
      piv_min = fmin(piv_min, akk);
      det *= akk;
    }
    if (l < 6)
#pragma unroll
      for (int j = 0; j < 6; ++j) Ai[l * 6 + j] = r6[j];
    wsync();
    // kappa_2 <= |A|_F |A^-1|_F; below 1e5 the pivoted QR of PinvCOD keeps
    // every mode (|R_55|/|R_00| >= 1/kappa_2 > COD_THRESHOLD 1e-6)
    const double fa = wave_sum(l < 36 ? A6[l] * A6[l] : 0.0), fi = wave_sum(l < 36 ? Ai[l] * Ai[l] : 0.0);
    if (!(piv_min > 0) || !(fa * fi < 1e10)) {  // uniform
      const double dt = det_lu6_wave(A6);
      pinv_cod6_wave(A6, Ai, S + kp.kScr);
      // at a singularity det(JJ^T) is rounding noise of either sign: a negative
      // one is zero, not NaN (a NaN input stays NaN); DESIGN.md "Manipulability at a singularity"
      if (l == 0) S[kp.oSc + SC_MAN] = dt < 0 ? 0.0 : sqrt(dt);
    } else if (l == 0) {
      S[kp.oSc + SC_MAN] = sqrt(det);
    }
    wsync();
  }
  double* W = S + kp.kW;  // narm x 6 = Jr^T Ai
  for (int e = l; kTask && e < narm * 6; e += 64) {
    int c = e / 6, a = e % 6;
    double s = 0;
    for (int i = 0; i < 6; ++i) s += J[i * nv + c0 + c] * Ai[i * 6 + a];
    W[e] = s;
  }
  wsync();
  double* part = S + kp.kPart;
  const AncBits ancb = anc_bits(M);
  for (int e = l; kTask && e < narm * narm; e += 64) {
    const int kk = e / narm, c = e % narm;
    const int jk = c0 + kk + 1, ji = c0 + c + 1;  // joint ids of q_k and column i
    double acc = 0;
    if ((anc_e & (1u << (jk - 1))) && (anc_e & (1u << (ji - 1)))) {
      V3 zk = ld3(Zw + 3 * jk), zi = ld3(Zw + 3 * ji);
      V3 pk_ = v3(T[12 * jk + 9], T[12 * jk + 10], T[12 * jk + 11]);
      V3 pi_ = v3(T[12 * ji + 9], T[12 * ji + 10], T[12 * ji + 11]);
      const bool krev = revolute(rev_mask, jk);
      V3 dpe = krev ? cross(zk, pe - pk_) : zk;
      const bool moves_i = jk != ji && supports(ancb, jk, ji);
      V3 dzi = (moves_i && krev) ? cross(zk, zi) : v3(0, 0, 0);
      V3 dpi = moves_i ? (krev ? cross(zk, pi_ - pk_) : zk) : v3(0, 0, 0);
      V3 lin, ang;
      if (revolute(rev_mask, ji)) {
        lin = cross(dzi, pe - pi_) + cross(zi, dpe - dpi);
        ang = dzi;
      } else {
        lin = dzi;
        ang = v3(0, 0, 0);
      }
      const double* w = W + c * 6;
      acc = lin.x * w[0] + lin.y * w[1] + lin.z * w[2] + ang.x * w[3] + ang.y * w[4] + ang.z * w[5];
    }
    part[e] = acc;
  }
  wsync();
  double* mg = S + kp.kmg;
  if (kTask && l < narm) {
    double s = 0;
    for (int c = 0; c < narm; ++c) s += part[l * narm + c];
    mg[l] = S[kp.oSc + SC_MAN] * s;
  }
  PH(2);
  // ---------------- self-collision distance (broad + narrow phase) -------
  // Each lane owns pairs p = l, l+64, ... and keeps its running minimum with
  // witness points in registers (ties -> lowest pair index, the oracle's
  // first-strict-min rule), so the winner's witnesses never get recomputed.
  double* pd = S + kp.kPd;
  int8_t* pf = reinterpret_cast<int8_t*>(S + kp.kPf);  // 0 open, 1 done, 2 penetrating (EPA)
  double bestd = 1.7976931348623157e308;
  int besti = 0x7fffffff;
  int bhow = 0;  // how the running best was found: 0 closed form, 1 GJK, 2 EPA
  V3 bpA = v3(0, 0, 0), bpB = v3(0, 0, 0);
  double ub = 1e300;
  // slots in type-class order (model.cpp pair_order): each round of 64 lanes
  // runs one or two pair types instead of all of them
  // (MESH) a hull with its pose, for the whole wave; the broad phase takes a
  // hull for its bounding box (gparam: a lower bound on the box holds for the
  // hull inside it, penetration included)
  [[maybe_unused]] auto hull_shape = [&](int g, const double* pose) {
    return ShapeMT<lds_pose*, true>{M->gtype[g], (lds_pose*)pose, M->gparam[g][0], M->gparam[g][1],
                                    M->gparam[g][2], M->mesh_verts + 3 * M->gmesh_first[g], M->gmesh_count[g]};
  };
  const PairTab ptab = pair_tab(M);
  for (int sl = l; sl < M->npairs; sl += 64) {
    const PairRec pr = pair_rec(ptab, sl);  // the slot's record: one level of loads
    const int p = pr.p;
    ShapeL A{pr.ta, (lds_pose*)(Tg + 12 * pr.ga), pr.pa[0], pr.pa[1], pr.pa[2]};
    ShapeL Bs{pr.tb, (lds_pose*)(Tg + 12 * pr.gb), pr.pb[0], pr.pb[1], pr.pb[2]};
    V3 pA, pB;
    double d;
    if constexpr (MESH) {
      if (A.type == kMesh || Bs.type == kMesh) {  // bound on the bounding box(es); the narrow phase is gjk_wave
        if (A.type == kMesh) A.type = kBox;
        if (Bs.type == kMesh) Bs.type = kBox;
        pd[p] = (A.type == kSphere || Bs.type == kSphere) ? sphere_pair(A, Bs, &pA, &pB)
                                                          : pair_lower_bound(A, Bs, pr.ba, pr.bb);
        pf[p] = 0;
        continue;
      }
    }
    bool hs = false;
    if constexpr (OBST) {
      if (Bs.type == kHalfSpace) {  // exact by closed form: never a GJK candidate (an obstacle is a pair's b)
        double ws[3], wp[3];
        d = halfspace_distance(A.type, A.T, A.p0, A.p1, A.p2, Bs.T, ws, wp);
        pA = ld3(ws);
        pB = ld3(wp);
        hs = true;
      }
    }
    const bool closed = hs || ((A.type == kSphere || Bs.type == kSphere)
                                   ? (d = sphere_pair(A, Bs, &pA, &pB), true)
                                   : (A.type == kCylinder && Bs.type == kCylinder && cyl_cyl_side(A, Bs, &d, &pA, &pB)));
    if (closed) {
      pf[p] = 1;
      ub = fmin(ub, d);
      if (d < bestd || (d == bestd && p < besti)) {  // ties -> lowest pair index
        bestd = d;
        besti = p;
        bhow = 0;
        bpA = pA;
        bpB = pB;
      }
    } else {  // swept-core / separating-axis lower bound
      pd[p] = pair_lower_bound(A, Bs, pr.ba, pr.bb);
      pf[p] = 0;
    }
  }
  ub = -wave_max(-ub);
  PH(3);
  // exact GJK only where the swept-core bound can still win.  The candidates
  // are compacted into a list first, so a wave runs them in ceil(n / 64)
  // rounds instead of one round per 64 pair slots.
  bool pen = false;  // some candidate intersects: the EPA search below has work
  {
    int* cand = reinterpret_cast<int*>(S + kp.kCand);
    int ncand = 0;
    [[maybe_unused]] int nhull = 0;  // (MESH) pairs with a hull: a second list, from the buffer's end down
    for (int p0 = 0; p0 < M->npairs; p0 += 64) {
      const int p = p0 + l;
      bool c = p < M->npairs && pf[p] == 0 && pd[p] - 1e-9 <= ub;
      if constexpr (MESH) {
        const bool h = c && (M->gtype[M->pair_a[p]] == kMesh || M->gtype[M->pair_b[p]] == kMesh);
        const unsigned long long mh = __ballot(h);
        if (h) cand[M->npairs - 1 - (nhull + __popcll(mh & ((1ull << l) - 1)))] = p;
        nhull += __popcll(mh);
        c = c && !h;
      }
      const unsigned long long m = __ballot(c);
      if (c) cand[ncand + __popcll(m & ((1ull << l) - 1))] = p;
      ncand += __popcll(m);
    }
    if (l == 0) ews->nv = 0;  // EPA seed stash counter (epa_stash)
    wsync();
    for (int c = l; c < ncand; c += 64) {
      const int p = cand[c];
      const int ga = M->pair_a[p], gb = M->pair_b[p];
      ShapeL A{M->gtype[ga], (lds_pose*)(Tg + 12 * ga), M->gparam[ga][0], M->gparam[ga][1], M->gparam[ga][2]};
      ShapeL Bs{M->gtype[gb], (lds_pose*)(Tg + 12 * gb), M->gparam[gb][0], M->gparam[gb][1], M->gparam[gb][2]};
      // early exit once GJK's lower bound shows the pair cannot reach ub
      const GjkDist g = gjk(A, Bs, ub + 1e-9, ews, p);
      if (g.pruned) {
        pf[p] = 1;
      } else if (g.intersect) {
        pf[p] = 2;  // penetrating: EPA below
        pen = true;
      } else {
        pf[p] = 1;
        if (g.dist < bestd || (g.dist == bestd && p < besti)) {
          bestd = g.dist;
          besti = p;
          bhow = 1;
          bpA = g.pA;
          bpB = g.pB;
        }
      }
    }
    if constexpr (MESH) {
      // pairs with a hull, one at a time on the whole wave (gjk_wave), in
      // pair order.  Every distance found so far tightens the cut.  Lane
      // p & 63 keeps the pair's result, as it does for EPA below.  A sphere
      // is its centre here, with the radius taken off afterwards; a centre
      // inside the hull goes to EPA like any overlap.  Two polytopes (hull,
      // box, a sphere's centre) end exactly, with the repeated support point
      // (tol 0); a hull against a cylinder stops like the primitives and is
      // refined if it wins (refine_witness_hull).
      ub = fmin(ub, -wave_max(-bestd));
      for (int c = 0; c < nhull; ++c) {
        const int p = cand[M->npairs - 1 - c];
        const int ga = M->pair_a[p], gb = M->pair_b[p];
        const auto A = hull_shape(ga, Tg + 12 * ga), Bs = hull_shape(gb, Tg + 12 * gb);
        const double rs = A.type == kSphere ? A.p0 : (Bs.type == kSphere ? Bs.p0 : 0.0);
        const bool poly = A.type != kCylinder && Bs.type != kCylinder;
        const GjkDist g = gjk_wave(A, Bs, ub + 1e-9 + rs, poly ? 0.0 : kGjkTol, ews, p);
        if (g.intersect) {
          pen = true;
          if (l == 0) pf[p] = 2;
          continue;
        }
        if (l == 0) pf[p] = 1;
        if (g.pruned) continue;
        double d = g.dist;
        V3 pA = g.pA, pB = g.pB;
        if (rs > 0) sphere_hull_witness(A.type == kSphere, rs, &d, &pA, &pB);
        ub = fmin(ub, d);
        if (l == (p & 63) && (d < bestd || (d == bestd && p < besti))) {
          bestd = d;
          besti = p;
          bhow = 1;
          bpA = pA;
          bpB = pB;
        }
      }
    }
  }
  wsync();
  PH(4);
  // EPA, best-first with bounds: the lower bound pd[p] <= d(p) also
  // caps the penetration depth, so pairs are expanded in increasing pd and
  // the search stops once no remaining pair can undercut the running
  // minimum (same argmin and tie rule as computing every pair).  The owning
  // lane expands the polytope, the whole wave scans for the closest face.
  // (Only pairs whose GJK intersected are searched: none, no search.)
  if (__any(pen)) {
    // The task plan may lay the polytope over Tg (lds_plan.hpp plan_kinematics): from
    // here on the poses in Tg are gone.  EPA works on the poses of its pair,
    // formed again in Pp; after the search the winner's two poses go back to
    // their places in Tg, where the refinement (and dist_rate) read them as
    // they do for an instance without EPA.
    double* Pp = S + kp.kPp;
#ifdef DRC_EPA_PRIO  // A/B variant: an EPA wave takes issue priority on its SIMD
    __builtin_amdgcn_s_setprio(DRC_EPA_PRIO);
#endif
    double gbd = bestd;
    int gbi = besti;
    wave_argmin(gbd, gbi);
    // stashed GJK simplices of intersecting pairs (epa_stash): pair and size
    // per slot, valid until a polytope grows into the stash's vertex slots
    const int nst = ews->nv < kEpaStash ? ews->nv : kEpaStash;
    int sp0 = nst > 0 ? static_cast<int>(ews->out[0]) : -1, sp1 = nst > 1 ? static_cast<int>(ews->out[2]) : -1;
    const int sn0 = nst > 0 ? static_cast<int>(ews->out[1]) : 0, sn1 = nst > 1 ? static_cast<int>(ews->out[3]) : 0;
    wsync();  // stash metadata read before the first EPA overwrites out[]
    for (;;) {
      double cpd = 1.7976931348623157e308;
      int cp = 0x7fffffff;
      for (int p = l; p < M->npairs; p += 64)
        if (pf[p] == 2 && pd[p] < cpd) {
          cpd = pd[p];
          cp = p;
        }
      wave_argmin(cpd, cp);
      if (cp == 0x7fffffff || cpd > gbd || (cpd == gbd && cp > gbi)) break;
      const int p = cp, ln = p & 63, ga = M->pair_a[p], gb = M->pair_b[p];
      if (l == 0) pose_pair<OBST>(M, T, Pp, Pp + 12, ga, gb, ob, obst0, io.b0 + b);  // (the loop's closing barrier: the last pair's readers are done)
      wsync();
      const ShapeL A{M->gtype[ga], (lds_pose*)Pp, M->gparam[ga][0], M->gparam[ga][1], M->gparam[ga][2]};
      const ShapeL Bs{M->gtype[gb], (lds_pose*)(Pp + 12), M->gparam[gb][0], M->gparam[gb][1], M->gparam[gb][2]};
      PH_ONLY(epa_calls++; unsigned long long est[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};)
      const int sk = p == sp0 ? 0 : (p == sp1 ? 1 : -1);
      double dall_;
      if constexpr (MESH) {  // the same EPA with the hulls' cooperative support
        dall_ = epa_run_wave(hull_shape(ga, Pp), hull_shape(gb, Pp + 12), ews, ln, sk, sk == 0 ? sn0 : sn1 PH_ONLY(, est));
        const double rs = A.type == kSphere ? A.p0 : (Bs.type == kSphere ? Bs.p0 : 0.0);
        if (rs > 0) {  // sphere centre inside a hull: the radius comes off, the sphere's witness moves out
          wsync();
          V3 wA = ld3(ews->out), wB = ld3(ews->out + 3);
          sphere_hull_witness(A.type == kSphere, rs, &dall_, &wA, &wB);
          wsync();
          if (l == ln) {
            st3(ews->out, wA);
            st3(ews->out + 3, wB);
          }
          wsync();
        }
      } else {
        dall_ = epa_run_wave(A, Bs, ews, ln, sk, sk == 0 ? sn0 : sn1 PH_ONLY(, est));
      }
      const double dall = dall_;
      if (ews->nv > kEpaStashV0) sp0 = sp1 = -1;  // grown into the stash slots
      PH_ONLY(epa_steps += est[0]; if (est[0] > epa_maxsteps) epa_maxsteps = est[0];
              epa_t[0] += est[1]; epa_t[1] += est[2]; epa_t[2] += est[3];
              for (int k_ = 0; k_ < 5; ++k_) epa_t[3 + k_] += est[4 + k_];)
      if (l == ln && (dall < bestd || (dall == bestd && p < besti))) {
        bestd = dall;
        besti = p;
        bhow = 2;
        bpA = ld3(ews->out);
        bpB = ld3(ews->out + 3);
      }
      if (dall < gbd || (dall == gbd && p < gbi)) {
        gbd = dall;
        gbi = p;
      }
      if (l == ln) pf[p] = 1;
      wsync();
    }
    {  // the polytope is dead: the winner's poses back into Tg (the argmin of the lines below)
      double wd = bestd;
      int wi = besti;
      wave_argmin(wd, wi);
      if (l == 0 && wi < M->npairs) {
        const int wa = M->pair_a[wi], wb = M->pair_b[wi];
        pose_pair<OBST>(M, T, Tg + 12 * wa, Tg + 12 * wb, wa, wb, ob, obst0, io.b0 + b);
      }
      wsync();
    }
#ifdef DRC_EPA_PRIO
    __builtin_amdgcn_s_setprio(0);
#endif
  }
  PH(5);
  const double myd = bestd;
  const int myi = besti;
  wave_argmin(bestd, besti);
  double* dgv = S + kp.kdg;
  double* red = S + kp.oRed;
  // The winning pair's GJK / EPA witnesses are refined to the exact critical
  // point (D17).  The QPIK stage does it after the task data are written,
  // where little is live across the call (in place, the call's register
  // saves and frame slowed every instance: measured); QPID's extras read
  // the witnesses, so QPID refines here.
  auto refine_winner = [&]() {
    const int ga = M->pair_a[besti], gb = M->pair_b[besti];
    const ShapeL A{M->gtype[ga], (lds_pose*)(Tg + 12 * ga), M->gparam[ga][0], M->gparam[ga][1], M->gparam[ga][2]};
    const ShapeL Bs{M->gtype[gb], (lds_pose*)(Tg + 12 * gb), M->gparam[gb][0], M->gparam[gb][1], M->gparam[gb][2]};
    double dref = S[kp.oSc + SC_DIST];
    V3 rA = ld3(red), rB = ld3(red + 3);
    if constexpr (MESH) {
      if (A.type == kMesh || Bs.type == kMesh) {  // a pair with a hull (refine_witness_hull)
        if (refine_witness_hull(serial_shape(hull_shape(ga, Tg + 12 * ga)), serial_shape(hull_shape(gb, Tg + 12 * gb)), &dref, &rA, &rB)) {
          st3(red, rA);
          st3(red + 3, rB);
          S[kp.oSc + SC_DIST] = dref;
        }
        return;
      }
    }
#ifdef DRC_NO_REFINE  // diagnostic build: the raw GJK / EPA witnesses
    if (false && refine_witness(A, Bs, &dref, &rA, &rB)) {
#else
    if (refine_witness(A, Bs, &dref, &rA, &rB)) {
#endif
      st3(red, rA);
      st3(red + 3, rB);
      S[kp.oSc + SC_DIST] = dref;
    }
  };
  // grad d = n^T (J_B(pB) - J_A(pA)) for joint l + 1, sign flipped when penetrating
  auto dist_grad = [&](double dd) {
    double g = 0;
    if (besti < M->npairs) {
      const int jA = M->gparent[M->pair_a[besti]], jB = M->gparent[M->pair_b[besti]];
      V3 pA = ld3(red), pB = ld3(red + 3), n = pB - pA;
      n = (1.0 / sqrt(dot(n, n))) * n;
      const int j = l + 1;
      V3 z = ld3(Zw + 3 * j), pj = v3(T[12 * j + 9], T[12 * j + 10], T[12 * j + 11]);
      const bool rev = revolute(rev_mask, j);
      V3 cA = v3(0, 0, 0), cB = v3(0, 0, 0);
      if (jA > 0 && (M->anc[jA] & (1u << l))) cA = rev ? cross(z, pA - pj) : z;
      if (jB > 0 && (M->anc[jB] & (1u << l))) cB = rev ? cross(z, pB - pj) : z;
      g = dot(n, cB - cA);
      if (dd < 0) g = -g;
    }
    return g;
  };
  // (RATE) dd/dt of the winning pair while the joints rest: the B-term of
  // dist_grad with the slot's rigid motion in place of a joint's column,
  // s n . (v + omega x (pB - p)), p the slot pose's origin.  Formed by the lane
  // of the obstacle geometry, which holds the twist, and broadcast; 0 for a
  // self pair (an obstacle is a pair's b)
  [[maybe_unused]] auto dist_rate = [&](double dd) {
    double r = 0;
    if constexpr (RATE) {
      const int gB = besti < M->npairs ? M->pair_b[besti] : 0;
      if (gB >= obst0 && besti < M->npairs) {
        if (l == gB) {
          const V3 pA = ld3(red), pB = ld3(red + 3), po = v3(Tg[12 * gB + 9], Tg[12 * gB + 10], Tg[12 * gB + 11]);
          V3 n = pB - pA;
          n = (1.0 / sqrt(dot(n, n))) * n;
          r = dot(n, v3(otw[0], otw[1], otw[2]) + cross(v3(otw[3], otw[4], otw[5]), pB - po));
          if (dd < 0) r = -r;
        }
        r = bcast(r, __builtin_amdgcn_readfirstlane(gB));
      }
    }
    return r;
  };
  if (myi == besti && myi < M->npairs) {  // the winning lane publishes its witnesses
    st3(red, bpA);
    st3(red + 3, bpB);
    S[kp.oSc + SC_DIST] = myd;
    S[kp.oSc + SC_HOW] = bhow;
  }
  if (l == 0) {
    if (besti >= M->npairs) {
      S[kp.oSc + SC_DIST] = bestd;
      S[kp.oSc + SC_HOW] = 0;
    }
    S[kp.oSc + SC_PAIR] = besti;
  }
  wsync();
  if constexpr (PROBLEM == 1 || PROBLEM == 3) {
    if (l == 0 && S[kp.oSc + SC_HOW] != 0) refine_winner();
    wsync();
  }
  if constexpr (PROBLEM == 3) {  // SC_DIST, SC_PAIR: the caller reads them (clearance_kernel.hip)
    PH_FLUSH(0);
    return;
  }
  bestd = S[kp.oSc + SC_DIST];
  PH(6);
  if (l < nv) dgv[l] = dist_grad(bestd);
  [[maybe_unused]] const double drate = dist_rate(bestd);
  wsync();
  if constexpr (PROBLEM == 1) qpid_task_extras(M, kp, S, bestd, besti, io.st_gdv != nullptr);
  PH(7);
  PH_ONLY(if (l == 0) {  // straggler census: max instance cycles, count above 400 k (~7x FR3's mean)
    const unsigned long long dt = __builtin_amdgcn_s_memtime() - inst_t0;
    atomicMax(&g_phase_cycles[30], dt);
    if (dt > 400000ull) {
      atomicAdd(&g_phase_cycles[31], 1ull);
      atomicAdd(&g_phase_cycles[29], dt);
      for (int k_ = 0; k_ < 8; ++k_) atomicAdd(&g_phase_cycles[8 + k_], ph_acc[k_] - ph_snap[k_]);
    }
    if (epa_calls) {  // EPA census over every instance
      atomicAdd(&g_phase_cycles[22], epa_calls);
      atomicAdd(&g_phase_cycles[23], epa_steps);
      atomicMax(&g_phase_cycles[28], epa_maxsteps);
      atomicAdd(&g_phase_cycles[18], epa_t[0] + epa_t[1]);  // (qp kernel leaves 18, 20 free)
      atomicAdd(&g_phase_cycles[20], epa_t[2]);
      // growth split (slots no other stage of a QPIK call writes)
      atomicAdd(&g_phase_cycles[59], epa_t[3]);
      atomicAdd(&g_phase_cycles[61], epa_t[4]);
      atomicAdd(&g_phase_cycles[62], epa_t[5]);
      atomicAdd(&g_phase_cycles[63], epa_t[6]);
      atomicAdd(&g_phase_cycles[60], epa_t[7]);  // seed polytope (slot 60: the lane stage's, not run here)
    }
  })
  // ---------------- task data out -----------------------------------------
  if (io.rec) {  // product path: one coalesced record per instance
    double* rec = io.rec + b * io.rec_stride;
    for (int e = l; e < kp.rLen; e += 64) {
      double v;
      if (e < kp.rMan) v = J[e];
      else if (e == kp.rMan) v = S[kp.oSc + SC_MAN];
      else if (e < kp.rDist) v = mg[e - kp.rMan - 1];
      else if (e == kp.rDist) v = RATE ? bestd + drate / kp.alpha_cbf : bestd;
      else if (e < kp.rXdd) v = dgv[e - kp.rDist - 1];
      else if (e < kp.rQ) v = xdd[e - kp.rXdd];
      else if (PROBLEM == 0 || e < kp.rQd) v = qv[e - kp.rQ];
      else if (e < kp.rBias) v = qd[e - kp.rQd];
      else v = S[kp.kBias + e - kp.rBias];  // QPID: Jdot v (6), man_gd, dist_gd
      rec[e] = v;
    }
  } else {  // stage outputs, [field][B]
    if (io.st_pose && l < 12) {
      // R row-major -> column-major storage, then p
      double v = l < 9 ? Te[(l % 3) * 3 + l / 3] : Te[l];
      io.st_pose[l * LD + gb] = v;
    }
    if (io.st_jac)
      for (int e = l; e < 6 * nv; e += 64) io.st_jac[(int64_t)e * LD + gb] = J[e];
    if (io.st_man) {
      if (l == 0) io.st_man[gb] = S[kp.oSc + SC_MAN];
      if (l < narm) io.st_man[(int64_t)(1 + l) * LD + gb] = mg[l];
    }
    if (io.st_dist) {
      if (l == 0) io.st_dist[gb] = bestd;
      if (l < nv) io.st_dist[(int64_t)(1 + l) * LD + gb] = dgv[l];
    }
    if constexpr (RATE)
      if (rt.rate && l == 0) rt.rate[gb] = drate;
    if (io.st_pair && l == 0) io.st_pair[gb] = besti < M->npairs ? besti : -1;
    if (io.st_xdd && l < 6) io.st_xdd[l * LD + gb] = xdd[l];
    if constexpr (PROBLEM == 1) {
      if (io.st_jdot)
        for (int e = l; e < 6 * nv; e += 64) io.st_jdot[(int64_t)e * LD + gb] = S[kp.kJd + e];
      if (io.st_qpid && l < 8) io.st_qpid[l * LD + gb] = S[kp.kBias + l];
      if (io.st_gdv)
        for (int e = l; e < narm + nv; e += 64) io.st_gdv[(int64_t)e * LD + gb] = S[kp.kGdv + e];
    }
  }
  wsync();
  if constexpr (PROBLEM == 0) {  // late refinement of the winner (D17): patch d and grad d
    if (S[kp.oSc + SC_HOW] != 0) {
      if (l == 0) refine_winner();
      wsync();
      const double dd = S[kp.oSc + SC_DIST];
      const double g = l < nv ? dist_grad(dd) : 0.0;
      [[maybe_unused]] const double dr = dist_rate(dd);  // (RATE) from the refined witnesses, patched like d
      if (io.rec) {
        double* rec = io.rec + b * io.rec_stride;
        if (l == 0) rec[kp.rDist] = RATE ? dd + dr / kp.alpha_cbf : dd;
        if (l < nv) rec[kp.rDist + 1 + l] = g;
      } else if (io.st_dist) {
        if (l == 0) io.st_dist[gb] = dd;
        if (l < nv) io.st_dist[(int64_t)(1 + l) * LD + gb] = g;
      }
      if constexpr (RATE)
        if (!io.rec && rt.rate && l == 0) rt.rate[gb] = dr;
      wsync();
    }
  }
  PH_FLUSH(0);
}

}  // namespace drc_amd
