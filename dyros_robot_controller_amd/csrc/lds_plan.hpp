// The per-wave LDS plan: the kernel parameters that carry it (KParams), the
// functions that lay it out from the model's dimensions, and the three small
// layout functions the host and the kernels share (where the fused kernels'
// record and the closed-loop kernels' state lie).  Every kernel takes its
// offsets from here, and the plans are unions: regions of different stages
// share bytes by the rules written at each place below.
// No HIP include: api.cpp lays out every call's plans with these functions,
// and the host compiler checks the rules on their output
// (tools/lds_plan_host_test.cpp, tests/test_lds_plan_host.py).
//
// One plan per wave: every QP kernel runs one instance on the 64 lanes of a
// wave (DESIGN.md "Out of scope" has the two-instances-per-wave build that was
// tried and removed).
#pragma once

#include "../../include/drc_amd.h"
#include "epa_poly.hpp"
#include "model.hpp"

#ifndef DRC_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define DRC_HD __host__ __device__
#else
#define DRC_HD
#endif
#endif
#if defined(__HIPCC__) || defined(__CUDACC__)
#define DRC_PLAN_FN DRC_HD __forceinline__
#else
#define DRC_PLAN_FN DRC_HD inline
#endif

namespace drc_amd {

// Kernel parameters, passed by value.  LDS offsets (in doubles) are laid out
// by the host from the model dimensions (plan_dims, plan_task, plan_qp below).
struct KParams {
  double kp[6], kv[6], ff, alpha_cbf, w_reg, slack_w, man_min, dist_min;
  double t, t0, duration;
  double frame_place[12];
  int frame_joint, mode, stages;
  int nv, nx, ng, np, na, m, narm, c0;
  int xcd_map;                         // XCD-aware instance order (grid % 8 == 0)
  int rJac, rMan, rDist, rXdd, rQ, rLen;  // per-instance task record (doubles)
  int problem;                         // 0 QPIK, 1 QPID (torque-level QP)
  int rQd, rBias, rMgd, rDgd;          // QPID extras of the task record
  int nbuf;                            // polish work-vector stride (>= ncap)
  int ncap;                            // largest polish KKT the LDS plan holds (nx + ng, or 48 for QPID)
  int eqp_small;                       // polish: reduced KKTs of up to this many rows take the small EQP (<= kEqpSmallCap; 0 = never)
  drc_solver_settings s;
  // persistent QP region
  int oP, oG, oQ, oAB, oL, oU, oD, oE, oRho, oX, oZ, oY, oDY, oXT, oZT, oT1, oT2, oRed, oSc;
  int oDi, oEi;  // D^-1 and E^-1 beside the scaling (OSQP scaling.c keeps Dinv / Einv)
  int oBc;  // max(32, nx + ng) doubles: vectors broadcast through LDS (ADMM passes, polish KKT sweeps)
  // union region (kinematics | K^-1 | polish)
  int oU0;
  int oHi;  // whole-body polish: cached rows of (P + delta I)^-1 (persistent, nx * nx), -1 if unused
  int kT, kZ, kTe, kJ, kTg, kq, kqd, kA6, kAi, kW, kPart, kPd, kPf, kCand, kxdd, kmg, kdg, kJt, kSv, kScr, kEpa;
  int kPp;   // pose pair (2 x 12) of the pair EPA expands (task_stage.hpp)
  int kOvl;  // first offset of the task plan's overlay that nothing reads once the task record is written
  int kJd, kDa, kVf, kX6, kBias, kMq, kGq;  // QPID: Jdot, arm-only Jdot, S eta, 6x6 scratch, bias | M, g
  int kGdv;                                 // QPID stage: grad_dot vectors
  int cf;                                   // closed-form controller: 1 CLIK, 2 OSF (task_kernel<2>)
  int kCf;                                  // its LDS work area
  int lds_doubles;
};

// Register EQP of the polish (eqp_regs): reduced KKTs of up to this many rows
// are solved lane-per-row in registers; the LDS plan sizes follow it.
constexpr int kEqpRegCap = 16;

// The fused kernel's LDS: the task plan (kt) and the QP plan (kq) overlay each
// other from offset 0, and the task record sits where neither stage touches it
// while the other reads it: in the task plan's overlay region (from kOvl: EPA
// polytope, GJK candidates, manipulability scratch -- dead once the record is
// written, task_stage.hpp "task data out") when that region lies past the QP
// plan and holds the record, else past both plans.  Whole-body plans then need
// no extra space for the record: 8 instead of 7 fused waves per CU (r06).
// Offsets in doubles; same function on the host (launch size) and the device.
DRC_PLAN_FN int fused_rec_offset(const KParams& kt, const KParams& kq) {
  const int rec = (kt.rLen + 1) & ~1;
  const int plans = kt.lds_doubles > kq.lds_doubles ? kt.lds_doubles : kq.lds_doubles;
  const int inside = kt.kOvl > kq.lds_doubles ? kt.kOvl : kq.lds_doubles;
  return kt.kEpa > 0 && inside + rec <= kt.lds_doubles ? inside : plans;
}
DRC_PLAN_FN int fused_lds_doubles(const KParams& kt, const KParams& kq) {
  const int plans = kt.lds_doubles > kq.lds_doubles ? kt.lds_doubles : kq.lds_doubles;
  const int end = fused_rec_offset(kt, kq) + ((kt.rLen + 1) & ~1);
  return end > plans ? end : plans;
}
// LDS of the closed-loop kernels' state update: q_k [nv], eta_k [na], J_mobile
// [3][kMaxWheels].  It lies at the start of the plan, not past it: once the QP
// has stored its outputs nothing in the plan is live (the next task stage
// rewrites it from the state arrays), so the kernel needs no more LDS than the
// fused kernel and keeps its waves per CU (fused_rec_offset's comment).
DRC_PLAN_FN int rollout_state_doubles(const KParams& kt, const KParams& kq) {
  return ((kt.nv + 1) & ~1) + ((kq.na + 1) & ~1) + 3 * kMaxWheels;
}

// ---------------------------------------------------------------- the plan
enum LdsPlanResult { kPlanOk = 0, kPlanQpTooLarge, kPlanModelTooLarge };

// What a test may ask a plan function for: every region it hands out, with the
// rule of the comments below that the region falls under.  (kPlanRecord: the
// fused kernels' record, which fused_rec_offset places; the test adds it.)
enum PlanGroup { kPlanPersistent, kPlanLive, kPlanManip, kPlanPolytope, kPlanPoses, kPlanCand, kPlanRecord };
struct PlanTrace {
  struct Region {
    const char* name;
    int off, len, group;
  };
  static constexpr int kCap = 96;
  Region r[kCap];
  int n = 0;
};
// Hands out the regions of a plan one after the other, each rounded up to an
// even number of doubles (16-byte alignment)
struct PlanCursor {
  int off;
  PlanTrace* tr;  // null on the product path
  void note(const char* name, int o, int n, int group) const {
    if (tr && tr->n < PlanTrace::kCap) tr->r[tr->n++] = {name, o, n, group};
  }
  int take(const char* name, int n, int group) {
    const int o = off;
    off += (n + 1) & ~1;
    note(name, o, n, group);
    return o;
  }
};
// k->field = the next n doubles, of group g (rows of these read as a table; the order is the layout)
#define DRC_TAKE(field, n) k->field = c.take(#field, n, g)

// The QP dimensions and the task record's offsets of a model (k->problem set)
inline LdsPlanResult plan_dims(const DevModel& M, KParams* k) {
  k->nv = M.nv;
  if (M.kind == 0) {
    k->narm = M.nv;
    k->c0 = 0;
    k->np = M.nv;
    k->nx = 3 * M.nv + 2;  // QP_IK.cpp:24-28
    k->na = M.nv;
  } else {
    k->narm = M.n_arm;
    k->c0 = M.mani_start;
    k->np = M.n_arm + M.n_wheel;
    k->nx = k->np;  // MoMa QP_IK.cpp:20
    k->na = k->np;
  }
  k->ng = 2 * k->narm + 2;
  if (k->problem == 1) {  // QPID: QP_ID.cpp:11-63 / MoMa QP_ID.cpp:11-33
    k->nx = M.kind == 0 ? 6 * M.nv + 2 : 2 * k->na;
    k->ng = 4 * k->narm + 2 + k->na;
  }
  k->m = k->nx + k->ng;
  k->rJac = 0;
  k->rMan = 6 * M.nv;
  k->rDist = k->rMan + 1 + k->narm;
  k->rXdd = k->rDist + 1 + M.nv;
  k->rQ = k->rXdd + 6;
  k->rQd = k->rQ + M.nv;
  k->rBias = k->rQd + M.nv;
  k->rMgd = k->rBias + 6;
  k->rDgd = k->rMgd + 1;
  k->rLen = k->problem == 1 ? k->rDgd + 1 : k->rQd;
  // larger than one wavefront's row mapping
  return k->nx > 64 || k->ng > 64 || k->narm > 8 || k->m > 128 ? kPlanQpTooLarge : kPlanOk;
}

inline LdsPlanResult plan_end(KParams* k, int end) {
  k->lds_doubles = end;
  return end * 8 > 160 * 1024 ? kPlanModelTooLarge : kPlanOk;
}
inline int plan_max(int a, int b) { return a > b ? a : b; }

// The persistent QP region of the QP kernels; the union starts at oU0
// (compiled: the QP shape has a compile-time instantiation, qp_compiled())
inline void plan_qp_persistent(const DevModel& M, KParams* k, bool compiled, PlanCursor& c) {
  const int nx = k->nx, ng = k->ng, np = k->np, m = k->m, g = kPlanPersistent;
  DRC_TAKE(oP, np * np), DRC_TAKE(oG, ng * nx), DRC_TAKE(oQ, nx), DRC_TAKE(oAB, nx), DRC_TAKE(oL, m), DRC_TAKE(oU, m);
  DRC_TAKE(oD, nx), DRC_TAKE(oE, m), DRC_TAKE(oDi, nx), DRC_TAKE(oEi, m), DRC_TAKE(oRho, m);
  DRC_TAKE(oX, nx), DRC_TAKE(oZ, m), DRC_TAKE(oY, m), DRC_TAKE(oDY, m), DRC_TAKE(oXT, nx), DRC_TAKE(oZT, m);
  DRC_TAKE(oT1, plan_max(m, nx)), DRC_TAKE(oT2, plan_max(m, nx)), DRC_TAKE(oRed, 64), DRC_TAKE(oSc, 32);
  DRC_TAKE(oBc, plan_max(nx + ng, 32));  // Ruiz factors (nx + ng), ADMM passes (ng + np), EQP (<= kEqpRegCap)
  k->oHi = -1;
  if (k->problem == 0 && M.kind == 1 && compiled) DRC_TAKE(oHi, nx * nx);
  k->oU0 = c.off;
}

// QPIK QP kernel: the union holds only what it uses -- the task record
// view (q, J, xdd, grad m, grad d, the mobile Jacobian, the task
// Jacobian), the factor (Schur blocks for the compiled shapes, K^-1
// otherwise) and the polish (index lists, x / y candidates; the LDS
// EQP only where a KKT can exceed the register EQP's kEqpRegCap).
// FR3: ~10 KB per wave instead of ~20.
inline LdsPlanResult plan_qpik_qp(const DevModel& M, KParams* k, bool compiled, PlanTrace* tr) {
  PlanCursor c{0, tr};
  plan_qp_persistent(M, k, compiled, c);
  const int nx = k->nx, ng = k->ng, np = k->np, m = k->m, nv = M.nv, g = kPlanLive;
  DRC_TAKE(kq, nv), DRC_TAKE(kJ, 6 * nv), DRC_TAKE(kxdd, 6), DRC_TAKE(kmg, k->narm), DRC_TAKE(kdg, nv);
  DRC_TAKE(kSv, 3 * kMaxWheels), DRC_TAKE(kJt, 6 * np);
  const int fac_end = k->oU0 + (compiled ? np * np + ng * np + 4 * ng : nx * nx + nx * ng);
  // manipulator QPs: the register EQP's size; a larger reduced KKT fails
  // that polish attempt and ADMM continues (the oracle applies the same
  // cap).  Whole-body QPs have no variable bounds, so every variable is free
  // in the reduced KKT (N = nx + active rows): capped at 16 their polish
  // fails whenever 6 (XLS-FR3) / 8 (Husky-FR3) rows are active and the
  // instance runs to the tight ADMM fallback (up to ~3 000 iterations);
  // they get the LDS EQP for N > 16
  const int N = M.kind == 1 ? nx + ng : (nx + ng < kEqpRegCap ? nx + ng : kEqpRegCap);
  k->ncap = N;
  k->nbuf = (N + 7) & ~7;
  const int reg_pol = k->oU0 + 128 + m;  // Fidx/Ridx | xx | yy
  // (compiled whole-body shapes solve every polish KKT in range-space form,
  // eqp_range: its H^-1 g_a buffer instead of the LDS LDL^T's)
  const int lds_pol = k->oHi >= 0 ? k->oU0 + 256 + kEqpRegCap * nx
                      : (compiled && N <= kEqpRegCap) ? 0
                      : k->oU0 + 64 + 64 + 128 + k->nbuf * 5 + N * (N + 1) / 2;
  const int end = plan_max(plan_max(c.off, fac_end), plan_max(reg_pol, lds_pol));
  return plan_end(k, (end + 1) & ~1);  // 16-byte aligned
}

// The kinematics view of the union from c.off on, of the task kernel (epa:
// with the EPA polytope overlay) and of the QPID QP kernel; c.off ends past it.
// wide: the polytope's former footprint and the geometry poses beside it;
// poses_beside: the poses beside it although the plan is narrow.  Returns false
// when the poses were to lie under the polytope and do not fit there: the
// caller lays the view out again with poses_beside.
inline bool plan_kinematics(const DevModel& M, KParams* k, bool epa, bool wide, bool poses_beside, PlanCursor& c) {
  const int nv = M.nv, np = k->np, narm = k->narm, na = k->na, ncand = (M.npairs + 1) / 2;
  const bool qpid = k->problem == 1;
  int g = kPlanLive;
  DRC_TAKE(kT, (nv + 1) * 12), DRC_TAKE(kZ, (nv + 1) * 3), DRC_TAKE(kTe, 12), DRC_TAKE(kJ, 6 * nv);
  const int ng_ = M.ngeom > nv ? M.ngeom : nv;  // (nv: the FK's local transforms, loc, use the poses' space first)
  // The geometry poses are read by the broad phase and the candidate GJKs;
  // after those only EPA and the winner's refinement want the poses of one
  // pair: EPA forms its pair's again in kPp and puts the winner's back in
  // place when it is done.  So with EPA the poses go into the overlay below,
  // under polytope fields that are written only once EPA runs.
  const bool tg_over = epa && !wide && !poses_beside;
  if (!tg_over) k->kTg = c.take("kTg", ng_ * 12, kPlanPoses);
  DRC_TAKE(kq, nv), DRC_TAKE(kqd, nv), DRC_TAKE(kPd, M.npairs), DRC_TAKE(kPf, (M.npairs + 7) / 8);  // kPf: one byte per pair
  DRC_TAKE(kxdd, 6), DRC_TAKE(kmg, narm), DRC_TAKE(kdg, nv), DRC_TAKE(kSv, 3 * kMaxWheels);
  // the pose pair of the pair EPA expands (2 x 12).  The QPIK task
  // stage never stages the mobile Jacobian (QPID's extras and the QP kernels do),
  // so there the pair takes kSv's place
  static_assert(3 * kMaxWheels >= 24, "kSv holds the pose pair");
  k->kPp = k->kSv;
  if (epa && qpid) DRC_TAKE(kPp, 24);
  // QPID's task extras read Ai and W after the collision stage
  if (!epa || qpid) DRC_TAKE(kAi, 36), DRC_TAKE(kW, narm * 6);
  if (qpid) {  // QPID stage data (task kernel) and dynamics (QP kernel)
    DRC_TAKE(kJd, 6 * nv), DRC_TAKE(kDa, 6 * narm), DRC_TAKE(kVf, nv), DRC_TAKE(kX6, 72 + 6 * narm + 2 * narm * narm);
    DRC_TAKE(kGdv, narm + nv), DRC_TAKE(kBias, 8), DRC_TAKE(kMq, na * na), DRC_TAKE(kGq, na);
  }
  if (k->cf && k->cf != 3) {  // W, W2 (6 x nv), M^-1, nu, g, task vectors, then the serial COD work (+ its nv x 6 result)
    const int ws = 6 * nv + 36 + 6 * nv + 18 + 2 * nv + 6 * nv;
    DRC_TAKE(kCf, 2 * 6 * nv + nv * nv + 3 * nv + 48 + plan_max(ws, 160));
  }
  // Regions dead once the collision stage starts (manipulability work, the
  // QP kernel's task Jacobian), then the EPA polytope laid over them: they
  // share LDS, which keeps the QPIK task kernel within 20 KB per wave
  // (8 waves per CU).  The GJK candidate list lives in the polytope's space
  // too (it is consumed before EPA starts).
  const int scr0 = c.off;
  g = kPlanManip;
  if (epa && !qpid) DRC_TAKE(kAi, 36), DRC_TAKE(kW, narm * 6);
  DRC_TAKE(kA6, 36), DRC_TAKE(kPart, narm * narm), DRC_TAKE(kJt, 6 * np);
  DRC_TAKE(kScr, 160);  // serial 6x6 COD work (pinv_cod_serial: 3n^2 + 3n)
  k->kOvl = k->kEpa = 0;
  if (!epa) {
    k->kCand = c.take("kCand", ncand, kPlanCand);
    return true;
  }
  k->kEpa = k->kOvl = scr0;
  const int ep = scr0 + (wide ? kEpaWideDoubles : kEpaDoubles);
  c.note("kEpa", scr0, ep - scr0, kPlanPolytope);
  k->kCand = scr0 + kEpaFnDoubles;  // the list lies in the polytope's face planes (epa_poly.hpp)
  if (tg_over) {
    // The poses, then the candidate list, from the face planes on.  While the
    // candidate GJKs read the poses, the stage writes the list (before),
    // the stash and pd / pf (live region): poses and list may share bytes
    // only with fields EPA writes later, [fn, out); and the poses start past
    // the manipulability scratch (kAi .. kScr, written after the poses).
    k->kTg = plan_max(k->kCand, k->kScr + 160);
    c.note("kTg", k->kTg, ng_ * 12, kPlanPoses);
    // the fused kernels' record must leave the poses alone (an instance that
    // ran no EPA refines its winner on them after the record is written);
    // the list is dead by then
    k->kOvl = k->kCand = k->kTg + ng_ * 12;
  }
  c.note("kCand", k->kCand, ncand, kPlanCand);
  if (tg_over && k->kCand + ncand > scr0 + kEpaOutDoubles) return false;  // a model with many geometries
  c.off = plan_max(c.off, plan_max(ep, k->kCand + ncand));
  return true;
}

// task_kernel: scalars + kinematics only (oRed: the winner's two witness
// points), with the EPA polytope unless the call is a closed-form controller's
inline LdsPlanResult plan_task(const DevModel& M, KParams* k, bool wide, PlanTrace* tr = nullptr) {
  PlanCursor c{0, tr};
  const int g = kPlanPersistent;
  DRC_TAKE(oRed, wide ? 64 : 8), DRC_TAKE(oSc, 32);
  k->oHi = -1;
  k->oU0 = c.off;
  const int mark = tr ? tr->n : 0;
  PlanCursor u = c;
  if (!plan_kinematics(M, k, !k->cf, wide, false, u)) {  // the poses do not fit under the polytope: beside it
    if (tr) tr->n = mark;
    u = c;
    plan_kinematics(M, k, !k->cf, wide, true, u);
  }
  return plan_end(k, u.off);
}

// QPID QP kernel: the persistent region, then the union of the kinematics
// view, K^-1 (nx * nx) and the polish
inline LdsPlanResult plan_qpid_qp(const DevModel& M, KParams* k, PlanTrace* tr) {
  PlanCursor c{0, tr};
  plan_qp_persistent(M, k, false, c);
  plan_kinematics(M, k, false, false, false, c);
  // polish KKT: free variables + active G rows.  QPID's (<= 81) is capped at 48 —
  // typically 7 qdd + 7 tau + 7 equality rows + the few active CBF rows and free
  // slacks — which halves the per-wave LDS; a larger guess fails that polish try
  constexpr int N = 48;
  k->ncap = N;
  k->nbuf = 64;
  const int kinv_end = k->oU0 + k->nx * k->nx, pol_end = k->oU0 + 64 + 64 + 128 + k->nbuf * 5 + N * (N + 1) / 2;
  return plan_end(k, plan_max(c.off, plan_max(kinv_end, pol_end)));
}

inline LdsPlanResult plan_qp(const DevModel& M, KParams* k, bool compiled, PlanTrace* tr = nullptr) {
  return k->problem == 0 ? plan_qpik_qp(M, k, compiled, tr) : plan_qpid_qp(M, k, tr);
}
#undef DRC_TAKE

}  // namespace drc_amd
