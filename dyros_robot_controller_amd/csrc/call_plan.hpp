// The dispatch plan of a QPIK call: which task stage runs, whether the call is
// one fused kernel or the task -> QP pipeline, in which order the instances
// are handed out, into how many concurrent sub-batches the batch is cut and
// how large each sub-batch's persistent grids are -- then which build of the
// task stage a model and a call need and which kernel family has it, and with
// that the rule by which the closed-loop entries pick their persistent kernel.
// Pure integer logic on the batch size, a few model facts and the DRC_* knobs
// (api.cpp reads the environment and fills PlanIn;
// tools/call_plan_host_test.cpp runs the rules with the host compiler).  Every
// threshold stands here with the measurement that set it.
#pragma once
#include <cstdint>

namespace drc_amd {

// The tuning knobs, with their defaults (api.cpp: env_int)
struct PlanKnobs {
  int64_t fuse_max = 16384;     // DRC_FUSE_MAX
  int64_t order_min = 2049;     // DRC_ORDER_MIN
  int64_t order_max = 8192;     // DRC_ORDER_MAX
  int64_t min_subbatch = 4096;  // DRC_MIN_SUBBATCH (>= 1)
  int64_t grid_task = 1024;     // DRC_GRID_TASK (>= 8)
  int64_t grid_qp = 4096;       // DRC_GRID_QP (>= 8)
  int64_t grid_fused = 2048;    // DRC_GRID_FUSED (>= 8)
  int64_t grid_clear = 3072;    // DRC_GRID_CLEAR (>= 8)
};

struct PlanIn {
  int64_t B = 0;              // instances of the call
  int stages = 0;             // a stage call (the task stage's outputs, no QP)
  int fused = 1;              // drc_set_fusion
  int lane_stage = 0;         // drc_debug_lane_stage: 0 off, 1 / 2 the lane stage, 3 auto (stage calls only)
  int chunks = 4;             // drc_set_concurrency
  bool caller_order = false;  // drc_debug_instance_order holds an order of exactly B instances
  int kind = 0;               // 0 manipulator, 1 whole-body
  int nv = 0;
  int ncand_slots = 0;
  bool has_mesh = false;     // collision hulls
  bool slots = false;        // obstacle slots (nobst > 0)
  bool twists = false;       // the call carries the slots' twists
  bool qp_compiled = false;  // the QP shape has a compile-time instantiation (qp_compiled())
  int qp_group = 64;         // kQpGroup: lanes per QP instance
  int max_cand_slots = 0;    // kMaxCandSlots
  PlanKnobs knobs;
};

// One contiguous range of the batch and its launches
struct SubBatch {
  int64_t b0 = 0, Bc = 0;
  int xcd_map = 0;
  int64_t grid_task = 0, grid_qp = 0, grid_fused = 0;
};

struct CallPlan {
  bool lane = false;              // lane-per-instance task stage (lane_task.hpp)
  bool fuse = false;              // one fused task + QP kernel per sub-batch
  bool auto_order = false;        // order_kernel.hip: penetration-prone instances first
  bool use_caller_order = false;  // the order of drc_debug_instance_order
  int S = 1;                      // concurrent sub-batches
};

// A launch of >= 16 Ki instances keeps the XCD-aware order; smaller ones run
// grid-stride order
inline int xcd_map_for(int64_t B) { return B >= 16384 ? 1 : 0; }

// A persistent grid (work queues hand out the instances): one wave per
// instance up to the cap.  The cap is a multiple of 8 (the knobs are clamped
// to >= 8): with the XCD-aware order every residue class blockIdx & 7 needs
// waves to drain its queue
inline int64_t persistent_grid(int64_t B, int64_t cap) {
  cap &= ~int64_t(7);
  return B < cap ? B : cap;
}

// What the fused kernel and the closed-loop entries' persistent kernels need
// alike: fusion switched on and a compiled QP shape on 64-lane groups
inline bool fusable_shape(const PlanIn& in) { return in.fused && in.qp_group == 64 && in.qp_compiled; }

inline CallPlan plan_call(const PlanIn& in) {
  CallPlan p;
  const int64_t B = in.B;
  const bool stages = in.stages != 0;
  // lane-per-instance task stage (lane_task.hpp) for the compiled joint counts
  // (3, auto: stage-only calls, where nothing overlaps the task stage.  The
  // default is 0: a full QPIK call is faster with the wave-per-instance
  // kernel, which shares the CUs with the QP kernels of the other sub-batches
  // (DESIGN.md), and stage and QPIK calls then see the same GJK witnesses)
  const int ls = in.lane_stage;
  p.lane = (ls == 1 || ls == 2 || (ls == 3 && stages)) && (in.nv == 6 || in.nv == 7) &&
           in.ncand_slots <= in.max_cand_slots && !in.has_mesh && !in.slots;
  // fused up to 16 Ki instances: there a call is a few instances per wave, its
  // makespan the tail the fused kernel and the EPA-first order below shorten;
  // at full batch the overlapped sub-batch pipeline wins.  Measured at
  // B = 16 384 (fused / pipeline): FR3 +10.5 % (+33 % with the order), UR5e
  // +10 % with the order (-4.1 % without), XLS-FR3 +4.3 %, Husky-FR3 +5.9 %;
  // B = 32 768: FR3 +3.7 %, UR5e -13 %, XLS-FR3 -12 %; B = 65 536: FR3 -13 %,
  // UR5e -21 % (profiles/r06t_envab_fuse_*.jsonl, r06x_*, r06y_*).
  // DRC_FUSE_MAX overrides
  p.fuse = fusable_shape(in) && !stages && !p.lane && B <= in.knobs.fuse_max;
  // penetration-prone instances first (order_kernel.hip) for calls whose
  // makespan is the EPA tail: manipulator calls of 2 049 .. 8 192 instances
  // (DRC_ORDER_MIN / _MAX), and every fused manipulator call above that (FR3
  // fused at B = 12 288 +38 %, 16 384 +20 %, profiles/r06v_envab_order*.jsonl).
  // Fewer: the 2 048-wave fused grid starts every instance at once anyway.
  // Pipeline calls above 8 192: the order gains less than it costs
  // (profiles/r06f_envab_order_*.jsonl).  Whole-body robots: their predictor
  // flags ~60 % of the instances, which orders nothing (XLS-FR3 B = 4 096
  // -2.6 %, profiles/r06j_envab_order_b4096.jsonl; FR3 +15.7 %, UR5e +7.7 %).
  // A caller's explicit order (drc_debug_instance_order) wins
  // (not with obstacle slots: the order kernel's predictor knows no poses)
  p.auto_order = !stages && !p.lane && !in.caller_order && !in.slots && B >= in.knobs.order_min &&
                 (B <= in.knobs.order_max || p.fuse) && in.kind == 0 && in.ncand_slots > 0 &&
                 in.ncand_slots <= in.max_cand_slots;
  p.use_caller_order = !stages && !p.lane && in.caller_order;
  // sub-batches of >= 4 Ki instances (a chunk of >= 16 Ki keeps the XCD-aware
  // order; smaller ones run grid-stride order): with one sub-batch the QP
  // kernel waits for the whole task kernel, with several they overlap
  // (Husky-FR3's 16 Ki batch)
  if (!stages && !p.fuse)
    for (int c = in.chunks; c > 1; --c)
      // four sub-batches only of >= 16 Ki instances each (Husky-FR3, B = 16 384:
      // 4 x 4 Ki 10.49 M against 3 x 5.5 Ki 11.14 M solves/s, r04z)
      if (B / c >= in.knobs.min_subbatch && (c < 4 || B / c >= 16384)) {
        p.S = c;
        break;
      }
  return p;
}

// Sub-batch c of the plan's S: a contiguous range and its persistent grids,
// 1 024 task and 4 096 QP waves per sub-batch.  Re-swept on the r06 kernels
// (the QP kernel's instances are now cheaper than the task kernel's): against
// 2 048 / 2 048, FR3 +2.8 %, UR5e +2.0 %, XLS-FR3 +1.4 %
// (profiles/r06ae_envab_grid.jsonl, r06af_envab_grid2.jsonl); DRC_GRID_TASK
// / _QP / _FUSED override for such experiments
inline SubBatch plan_sub_batch(const PlanIn& in, const CallPlan& p, int c) {
  SubBatch s;
  s.b0 = in.B * c / p.S;
  s.Bc = in.B * (c + 1) / p.S - s.b0;
  s.xcd_map = xcd_map_for(s.Bc);
  s.grid_task = persistent_grid(s.Bc, in.knobs.grid_task);
  s.grid_qp = persistent_grid(s.Bc, in.knobs.grid_qp);
  s.grid_fused = persistent_grid(s.Bc, in.knobs.grid_fused);
  return s;
}

// The persistent grid of a path-clearance call (drc_clearance_path_batch,
// clearance_kernel.hip): one launch for the whole batch, one path per wave.
// No QP kernel shares the CUs with it, so the pipeline's 1 024 task waves were
// no evidence for it.  Swept with the register budget on FR3, B = 65 536,
// substeps 8, no stop (tools/bench_clearance.py --sweep,
// profiles/clearance_grid.json; the numbers in DESIGN.md "Path clearance"):
// 1 024 waves leave half of the wave slots empty and cost 1.6 to 1.9 times
// the call of 2 048 or 3 072 waves; with the three-wave build 3 072 is the
// fastest.  At B = 4 096 (two-wave build, profiles/clearance_grid_b4096.json)
// 2 048 and 3 072 are equal and 7 % ahead of 1 024.  DRC_GRID_CLEAR overrides
inline int64_t clearance_grid(int64_t B, const PlanKnobs& knobs) { return persistent_grid(B, knobs.grid_clear); }

// The builds of the task stage, task_instance<PROBLEM, MESH, OBST, RATE>
// (task_stage.hpp): plain, with the hull narrow phase, with obstacle slots
// whose poses the call carries, and with the slots' twists as well
enum class StageBuild { Plain, Mesh, Obst, Rate };
constexpr int kStageBuilds = 4;

// Hulls together with slots have no build: drc_model_set_obstacles refuses
// slots on a hull model (model.cpp), so no model asks for one
constexpr bool stage_build_exists(bool has_mesh, bool slots) { return !(has_mesh && slots); }
// The build a model and a call need -- the one place that decides it.  twists:
// the call carries obstacle twists (they count with slots only)
constexpr StageBuild stage_build(bool has_mesh, bool slots, bool twists) {
  return slots ? (twists ? StageBuild::Rate : StageBuild::Obst) : has_mesh ? StageBuild::Mesh : StageBuild::Plain;
}
// the builds whose calls carry the slots' poses
constexpr bool takes_poses(StageBuild b) { return b == StageBuild::Obst || b == StageBuild::Rate; }

// The kernel families that contain the stage: task_kernel's three problems
// (the QPIK stage, the QPID stage, closed-form CLIK / OSF), the fused kernel
// and the closed-loop entries' persistent kernels; Clearance is the distance
// stage alone along a path (clearance_kernel.hip)
enum class StageFamily { Task0, Task1, Task2, Fused, Rollout, Reach, ReachPath, ReachSeeds, Clearance };
constexpr int kStageFamilies = 9;

// Which family is compiled in which build (its launcher returns
// hipErrorInvalidValue for any other).  Task2 has no distance stage, so hull
// models run its plain build
constexpr bool has_build(StageFamily f, StageBuild b) {
  switch (f) {
    case StageFamily::Task0:
    case StageFamily::Fused: return true;
    case StageFamily::Task1:
    case StageFamily::Rollout: return b == StageBuild::Plain || b == StageBuild::Mesh;
    case StageFamily::Task2:
    case StageFamily::Reach: return b == StageBuild::Plain;
    case StageFamily::ReachPath:
    case StageFamily::ReachSeeds: return b == StageBuild::Plain || b == StageBuild::Obst;
    case StageFamily::Clearance: return b != StageBuild::Rate;  // (static slots: no twists)
  }
  return false;
}

// The fusion rule selects a closed-loop entry's persistent kernel (rollout,
// reach, reach_path, reach_seeds): the compiled QP shapes up to max_b
// instances, where the entry's family has the build that the model and the
// call need.  It asks for lane_stage == 0 where plan_call asks for !lane:
// the persistent kernels have no lane stage, so any lane-stage mode that is
// set sends these entries down their stepwise path -- also where the stepwise
// calls then run without the lane stage themselves (mode 3 on a QP call, a
// joint count without a lane build, a model with hulls or slots)
inline bool persistent_path(const PlanIn& in, int64_t max_b, StageFamily family) {
  return fusable_shape(in) && in.lane_stage == 0 && in.B <= max_b && stage_build_exists(in.has_mesh, in.slots) &&
         has_build(family, stage_build(in.has_mesh, in.slots, in.twists));
}

}  // namespace drc_amd
