// Host side of the MI355X-native QP-IK: the C-ABI of include/drc_amd.h.
// Model build and upload, per-stream scratch, the launch sequences (task ->
// QP kernels on forked sub-batch streams, QPID, closed-form controllers), the
// synchronous host-buffer entries and the dynamics entries.  The kernels live
// in task_kernel.hip, qp_kernel.hip, qpid_kernel.hip and dynamics.hip.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <algorithm>
#include <vector>

#include "../../include/drc_amd.h"
#include "../../include/drc_amd_debug.h"
#include "call_plan.hpp"
#include "clearance.hpp"
#include "clearance_certify.hpp"
#include "dynamics.hpp"
#include "host_staging.hpp"
#include "kernel_common.hpp"
#include "launch.hpp"
#include "mesh.hpp"
#include "reach.hpp"
#include "reach_path.hpp"
#include "reach_seeds.hpp"
#include "rollout_update.hpp"
#include "scratch_layout.hpp"

// ==========================================================================
// host side: the C-ABI (include/drc_amd.h)
// ==========================================================================
namespace drc_amd {

// A block of device scratch: grown to what a call needs, never shrunk (grow)
struct Block {
  void* p = nullptr;
  int64_t bytes = 0;
};

// Per-stream scratch of a model: the work-queue counters and four blocks,
// each carved by the layouts of scratch_layout.hpp (DESIGN.md "Stream
// scratch").  There are several because calls nest: a stepwise closed-loop
// call holds `roll` while each of its steps uses `pool`, and a stepwise seeds
// call holds `seeds` around a reach that uses `roll`.  Calls on one stream
// are ordered by that stream, so they may share it; calls on two streams get
// disjoint contexts (the
// C-ABI's "reentrant per stream", include/drc_amd.h).  At most kMaxStreamCtx
// contexts are kept: a new stream beyond that evicts the least recently used
// one (once the last call that used it has finished: `done`, an event recorded
// on the caller's stream after each call's launches), and
// drc_model_release_stream frees a stream's context at once, so a caller
// cycling through streams holds a bounded amount of device memory.
struct StreamCtx {
  hipStream_t stream = nullptr;
  hipEvent_t done = nullptr;  // recorded on `stream` after every call's launches
  uint64_t last_use = 0;
  Block pool;  // task records, hard and order lists / QPID records and dynamics / OSF M^-1, g
  // work-queue counters, one slot of kSlotInts per launch sequence: slots
  // 0..15 the QPIK sub-batches, 16 QPID, 17 the closed-form controllers.  In a
  // slot: the task (or fused) kernel's queue and the QP kernel's, one counter
  // per XCD class each, then the lane stage's hard count and the order
  // kernel's hot count
  static constexpr int kSlotInts = 32, kXcdClasses = 8;
  static constexpr int kSlotTask = 0, kSlotQp = 8, kSlotHard = 16, kSlotHot = 24;
  static_assert(kSlotQp >= kSlotTask + kXcdClasses && kSlotHard >= kSlotQp + kXcdClasses && kSlotHot > kSlotHard &&
                    kSlotHot < kSlotInts,
                "the users of a queue slot do not overlap and fit it");
  static constexpr int kQueueSlotQpid = 16, kQueueSlotCf = 17, kQueueInts = 18 * kSlotInts;
  int* d_queue = nullptr;
  Block dyn_list;  // instances whose M_inv needs the serial COD
  Block roll;      // rollout / reach / reach path scratch: one step's eta, stage outputs, status, counters
  Block seeds;     // drc_qpik_reach_seeds_batch: per-instance results, expanded targets, group words
};
constexpr size_t kMaxStreamCtx = 8;

// Fork/join streams of the concurrent sub-batches, shared by every caller
// stream of a model: a process gets 4 hardware queues (GPU_MAX_HW_QUEUES), so
// the internal streams do not multiply with the caller's streams.  Calls are
// enqueued under the model's launch mutex, so an event is recorded and waited
// on by one call before the next re-records it; work of two caller streams on
// one lane runs in order (each call on its own context's scratch).
struct Lanes {
  std::vector<hipStream_t> lanes;  // concurrent sub-batches (drc_set_concurrency)
  std::vector<hipEvent_t> joins;
  // per sub-batch: the lane stage's hard instances run their task kernel on a
  // side stream while the QP of the other instances runs
  std::vector<hipStream_t> sides;
  std::vector<hipEvent_t> side_fork, side_join;
  hipEvent_t fork = nullptr;
};

struct drc_model_impl {
  HostModel hm;
  DevModel* d_model = nullptr;
  double* d_mesh = nullptr;  // hull vertices of the collision meshes (DevModel::mesh_verts)
  double* d_pair_tab = nullptr;  // per-pair records of the task stage (DevModel::pair_tab)
  double* d_motion_wt = nullptr;  // motion weights of the certified clearance (DevModel::motion_wt)
  int device = 0;
  drc_kinematic_param kparam{};
  drc_joint_index jidx{};
  drc_actuator_index aidx{};
  std::vector<std::unique_ptr<StreamCtx>> ctxs;  // one per caller stream seen (at most kMaxStreamCtx)
  uint64_t ctx_tick = 0;
  Lanes ln;
  int timing = 0;  // drc_debug_kernel_timing: HIP events around each launch
  int lane_stage = 0;  // drc_debug_lane_stage: 0 off, 1 lane stage + side-stream hard path, 2 + serial hard path, 3 auto
  bool task_plan_wide = false;  // drc_debug_task_plan_wide: geometry poses outside the polytope overlay
  int eqp_small_cap = -1;  // drc_debug_eqp_small_cap: -1 the compiled tiers, 0 general EQP only, k small EQP for N <= k
  bool qp_dense = false;   // drc_debug_qp_dense: the manipulator shapes' QP kernel with dense G loops
  int64_t qp_dense_launches = 0;
  int64_t clearance_grid_last = 0;  // drc_debug_clearance_grid: waves of the last clearance launch
  // timed calls: the events and the call's sub-batch count S.  S > 1: {call
  // start, call end, then per sub-batch task start, task end, QP end}; S = 1:
  // {task start, last, task start, task end, last} (last: the QP's end, or the
  // fused kernel's)
  std::vector<std::pair<std::vector<hipEvent_t>, int>> events;
  std::vector<hipEvent_t> evpool;  // timing events returned by drc_debug_kernel_times, reused
  // concurrent sub-batches: the batch is cut into `chunks` contiguous ranges,
  // the last on the caller's stream and the others on internal streams forked
  // from / joined to it, so one range's task kernel overlaps another's QP
  // kernel and the straggler tails of the kernels interleave.  4 streams fit
  // the 4 hardware queues a process gets by default; measured on MI355X
  // (r04u, B = 65 536): 4 sub-batches FR3 23.6 M / UR5e 20.3 M / XLS-FR3 17.9 M
  // against 22.6 / 19.1 / 17.7 M at 3 (then on 3 internal streams + the
  // caller's); 6 sub-batches, with 8 hardware queues or 4, were slower
  int chunks = 4;
  // fused task + QP kernel for the compiled QPIK shapes and small batches
  // (fused_kernel.hip; drc_set_fusion): one launch per call, the record in LDS
  int fused = 1;
  // drc_debug_instance_order: a scheduling order for calls of exactly
  // order_n instances (device copy), or none
  int32_t* d_order = nullptr;
  int64_t order_n = 0;
  // host-buffer entry points: device staging + an internal stream
  std::mutex host_mu;
  void* stage = nullptr;
  int64_t stage_bytes = 0;
  // pinned host mirror of the staging buffer: every synchronous *_host entry
  // packs its inputs into it and copies them over in one transfer, and brings
  // the outputs back in one (HostStage; both grow together, ensure_staging)
  double* pinned = nullptr;
  int64_t pinned_bytes = 0;
  hipStream_t hstream = nullptr;
  hipEvent_t hdone = nullptr;  // recorded after a synchronous entry's copy back
  // drc_debug_host_timeline: per synchronous call, steady-clock ns at entry,
  // inputs packed, H2D + launches + D2H enqueued, completion seen, exit
  int tl_on = 0;
  std::vector<int64_t> tl;
  std::mutex mu;         // the context list, timing events, concurrency
  std::mutex launch_mu;  // one call's launch sequence is enqueued as a unit, so
                         // two host threads sharing a stream cannot interleave
                         // their kernels on its scratch
};

static thread_local std::string g_last_error;
static int set_err(int code, const std::string& msg) {
  g_last_error = msg;
  return code;
}
#define HIP_TRY(expr)                                                                   \
  do {                                                                                  \
    hipError_t e_ = (expr);                                                             \
    if (e_ != hipSuccess) return set_err(DRC_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)

// Widths of a model's vectors: the actuated joints (arm + wheels of a
// whole-body robot; q-dot*, qddot and tau of the QP entries) and the arm
static int actuated_width(const DevModel& d) { return d.kind == 1 ? d.n_arm + d.n_wheel : d.nv; }
static int arm_width(const DevModel& d) { return d.kind == 1 ? d.n_arm : d.nv; }

static void free_ctx(StreamCtx* c) {
  // the event outlives a destroyed stream: waiting on it orders the frees
  // after this context's last use without draining any other stream
  if (c->done) (void)hipEventSynchronize(c->done), (void)hipEventDestroy(c->done);
  c->done = nullptr;
  if (c->d_queue) (void)hipFree(c->d_queue);
  c->d_queue = nullptr;
  for (Block* b : {&c->pool, &c->dyn_list, &c->roll, &c->seeds}) {
    if (b->p) (void)hipFree(b->p);
    *b = Block();
  }
}

// A tuning knob from the environment: its integer value when set and
// parsable, clamped to >= lo; otherwise the default.
static int64_t env_int(const char* name, int64_t def, int64_t lo) {
  const char* v = getenv(name);
  if (!v || !*v) return def;
  char* end = nullptr;
  const long long x = strtoll(v, &end, 10);
  if (end == v) return def;
  return x < lo ? lo : x;
}

// The scratch context of `st` (created on first use; the caller holds
// m->launch_mu and m->mu, so no launch still being enqueued uses an evicted
// context).  Beyond kMaxStreamCtx streams the least recently used context is
// freed once its `done` event has completed (its stream may already be
// destroyed; the event stays valid, and no other stream is waited for).
static int stream_ctx(drc_model_impl* m, hipStream_t st, StreamCtx** out) {
  for (auto& c : m->ctxs)
    if (c->stream == st) {
      c->last_use = ++m->ctx_tick;
      *out = c.get();
      return DRC_OK;
    }
  if (m->ctxs.size() >= kMaxStreamCtx) {
    size_t lru = 0;
    for (size_t i = 1; i < m->ctxs.size(); ++i)
      if (m->ctxs[i]->last_use < m->ctxs[lru]->last_use) lru = i;
    free_ctx(m->ctxs[lru].get());
    m->ctxs.erase(m->ctxs.begin() + static_cast<std::ptrdiff_t>(lru));
  }
  std::unique_ptr<StreamCtx> c(new StreamCtx());
  c->stream = st;
  c->last_use = ++m->ctx_tick;
  HIP_TRY(hipEventCreateWithFlags(&c->done, hipEventDisableTiming));
  HIP_TRY(hipMalloc(&c->d_queue, StreamCtx::kQueueInts * sizeof(int)));
  *out = c.get();
  m->ctxs.push_back(std::move(c));
  return DRC_OK;
}
// Grows a block to exactly `bytes` (no head-room: tests/test_gpu_streams.py
// bounds what a model holds); the caller holds m->mu
static int grow(Block* b, int64_t bytes) {
  if (b->bytes >= bytes) return DRC_OK;
  if (b->p) HIP_TRY(hipFree(b->p));  // synchronises: no launch still uses it
  *b = Block();
  HIP_TRY(hipMalloc(&b->p, bytes));
  b->bytes = bytes;
  return DRC_OK;
}

// The start and the end of every launch path: selects the model's device,
// takes the caller stream's context, grows and carves the blocks the path
// names, and records the context's `done` event on every exit once the context
// is in use, so eviction (free_ctx) never frees scratch that kernels of this
// call still use.  Every launch path enqueues on the caller's stream only,
// except the QPIK path's concurrent sub-batches: a call that fails after
// forking may have left kernels on the model's internal fork / side streams
// that `done` on the caller's stream does not follow, so that path (forks set)
// waits for those streams -- the model's own, never the device: other streams
// and models in the process are not stalled, and a failure before anything was
// forked costs no synchronisation at all.
// (the caller holds m->launch_mu, from before the Launch is made until after
// it is gone: `done` is recorded on a context that nobody can have evicted)
struct Launch {
  drc_model_impl* m;
  hipStream_t st;
  StreamCtx* cx = nullptr;
  const Lanes* forks = nullptr;  // set once a sub-batch may run on a fork stream
  bool ok = false;
  Launch(drc_model_impl* model, void* stream) : m(model), st(reinterpret_cast<hipStream_t>(stream)) {}
  Launch(const Launch&) = delete;
  ~Launch() {
    if (!cx || !cx->done) return;
    if (!ok && forks) {
      for (hipStream_t s : forks->lanes) (void)hipStreamSynchronize(s);
      for (hipStream_t s : forks->sides) (void)hipStreamSynchronize(s);
    }
    (void)hipEventRecord(cx->done, st);
  }
  int context() {
    std::lock_guard<std::mutex> g(m->mu);
    return stream_ctx(m, st, &cx);
  }
  int begin() {
    HIP_TRY(hipSetDevice(m->device));
    return context();
  }
  // One block of the context by its layout (scratch_layout.hpp): measured
  // without a base, grown to the layout's bytes, carved
  template <class F, class L>
  int carve(Block StreamCtx::*block, F layout, L* out) {
    std::lock_guard<std::mutex> g(m->mu);
    Block* b = &(cx->*block);
    if (int r = grow(b, layout(nullptr).bytes)) return r;
    *out = layout(b->p);
    return DRC_OK;
  }
  int done() {
    ok = true;
    return DRC_OK;
  }
};
static void free_lanes(Lanes* c) {
  for (hipStream_t ls : c->lanes) (void)hipStreamSynchronize(ls);
  for (hipStream_t ls : c->sides) (void)hipStreamSynchronize(ls);
  for (hipStream_t ls : c->lanes) (void)hipStreamDestroy(ls);
  for (hipEvent_t e : c->joins) (void)hipEventDestroy(e);
  for (hipStream_t ls : c->sides) (void)hipStreamDestroy(ls);
  for (hipEvent_t e : c->side_fork) (void)hipEventDestroy(e);
  for (hipEvent_t e : c->side_join) (void)hipEventDestroy(e);
  if (c->fork) (void)hipEventDestroy(c->fork);
}

// DyrosMath::PinvCOD on a small dense matrix (host, model build only):
// Moore-Penrose inverse via the normal equations' symmetric eigen-system,
// rank cut at 1e-6 relative (math_type_define.h:7,563-570).
static void pinv_small(const double* A, int r, int c, double* X /* c x r */) {
  // X = (A^T A)^+ A^T with (A^T A) symmetric c x c (c <= 3 here)
  double N[9] = {0}, V[9], w[3];
  for (int i = 0; i < c; ++i)
    for (int j = 0; j < c; ++j)
      for (int k = 0; k < r; ++k) N[i * c + j] += A[k * c + i] * A[k * c + j];
  for (int i = 0; i < c * c; ++i) V[i] = (i % (c + 1) == 0) ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 60; ++sweep) {
    double off = 0;
    for (int i = 0; i < c; ++i)
      for (int j = i + 1; j < c; ++j) off += N[i * c + j] * N[i * c + j];
    if (off < 1e-300) break;
    for (int p = 0; p < c; ++p)
      for (int q = p + 1; q < c; ++q) {
        if (std::fabs(N[p * c + q]) < 1e-300) continue;
        double th = (N[q * c + q] - N[p * c + p]) / (2 * N[p * c + q]);
        double t = (th >= 0 ? 1 : -1) / (std::fabs(th) + std::sqrt(th * th + 1));
        double cs = 1 / std::sqrt(t * t + 1), sn = t * cs;
        for (int k = 0; k < c; ++k) {
          double a = N[k * c + p], b = N[k * c + q];
          N[k * c + p] = cs * a - sn * b;
          N[k * c + q] = sn * a + cs * b;
        }
        for (int k = 0; k < c; ++k) {
          double a = N[p * c + k], b = N[q * c + k];
          N[p * c + k] = cs * a - sn * b;
          N[q * c + k] = sn * a + cs * b;
        }
        for (int k = 0; k < c; ++k) {
          double a = V[k * c + p], b = V[k * c + q];
          V[k * c + p] = cs * a - sn * b;
          V[k * c + q] = sn * a + cs * b;
        }
      }
  }
  double wmax = 0;
  for (int i = 0; i < c; ++i) {
    w[i] = N[i * c + i];
    wmax = std::fmax(wmax, std::fabs(w[i]));
  }
  double Ni[9] = {0};
  for (int e = 0; e < c; ++e) {
    if (std::sqrt(std::fabs(w[e])) <= 1e-6 * std::sqrt(wmax)) continue;
    for (int i = 0; i < c; ++i)
      for (int j = 0; j < c; ++j) Ni[i * c + j] += V[i * c + e] * V[j * c + e] / w[e];
  }
  for (int i = 0; i < c; ++i)
    for (int k = 0; k < r; ++k) {
      double s = 0;
      for (int j = 0; j < c; ++j) s += Ni[i * c + j] * A[k * c + j];
      X[i * r + k] = s;
    }
}

// Mobile::RobotData::computeFKJacobian (src/mobile/robot_data.cpp:123-204) at
// the wheel positions `wheel_pos` (used by the caster drive only; may be NULL
// for the configuration-independent drives, then zero steer angles).
static int mobile_fk_jacobian(const drc_kinematic_param& p, int* W, double out[3][kMaxWheels],
                              const double* wheel_pos = nullptr) {
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < kMaxWheels; ++c) out[r][c] = 0;
  if (p.type == DRC_DRIVE_DIFFERENTIAL) {
    *W = 2;
    out[0][0] = p.wheel_radius / 2.;
    out[0][1] = p.wheel_radius / 2.;
    out[2][0] = -p.wheel_radius / p.base_width;
    out[2][1] = p.wheel_radius / p.base_width;
    return DRC_OK;
  }
  if (p.type == DRC_DRIVE_MECANUM) {
    const int n = p.n_wheels;
    if (n < 1 || n > kMaxWheels) return set_err(DRC_ERR_INVALID_ARGUMENT, "mecanum wheel count out of range");
    double Jinv[kMaxWheels * 3], X[3 * kMaxWheels];
    for (int i = 0; i < n; ++i) {
      const double r = p.wheel_radius, g = p.roller_angles[i], px = p.base2wheel_positions[i][0],
                   py = p.base2wheel_positions[i][1], pt = p.base2wheel_angles[i];
      // (1/r) [1 tan g] [[cos pt, sin pt], [-sin pt, cos pt]] [[1 0 -py], [0 1 px]]
      const double a0 = std::cos(pt) - std::tan(g) * std::sin(pt), a1 = std::sin(pt) + std::tan(g) * std::cos(pt);
      Jinv[i * 3 + 0] = a0 / r;
      Jinv[i * 3 + 1] = a1 / r;
      Jinv[i * 3 + 2] = (-a0 * py + a1 * px) / r;
    }
    pinv_small(Jinv, n, 3, X);
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < n; ++c) out[r][c] = X[r * n + c];
    *W = n;
    return DRC_OK;
  }
  if (p.type == DRC_DRIVE_CASTER) {  // CasterFKJacobian (:179-204): W = 2 x casters
    const int C = p.n_wheels;
    if (C < 1 || 2 * C > kMaxWheels) return set_err(DRC_ERR_INVALID_ARGUMENT, "caster count out of range");
    double zero[kMaxWheels] = {0};
    caster_fk_jacobian(C, p.wheel_radius, p.wheel_offset, p.base2wheel_positions, wheel_pos ? wheel_pos : zero, out);
    *W = 2 * C;
    return DRC_OK;
  }
  return set_err(DRC_ERR_INVALID_ARGUMENT, "unknown drive type");
}

// Mobile::RobotController::computeIKJacobian (src/mobile/robot_controller.cpp:55-125):
// wheel velocities = J_ik (W x 3, row-major) * base twist.
static int mobile_ik_jacobian(const drc_kinematic_param& p, const double* wheel_pos, double* J, int* W) {
  const double r = p.wheel_radius;
  if (p.type == DRC_DRIVE_DIFFERENTIAL) {  // DifferentialIKJacobian (:76-84)
    *W = 2;
    const double e[6] = {1 / r, 0, -p.base_width / (2 * r), 1 / r, 0, p.base_width / (2 * r)};
    for (int i = 0; i < 6; ++i) J[i] = e[i];
    return DRC_OK;
  }
  if (p.type == DRC_DRIVE_MECANUM) {  // MecanumIKJacobian (:86-107)
    const int n = p.n_wheels;
    if (n < 1 || n > kMaxWheels) return set_err(DRC_ERR_INVALID_ARGUMENT, "mecanum wheel count out of range");
    for (int i = 0; i < n; ++i) {
      const double g = p.roller_angles[i], px = p.base2wheel_positions[i][0], py = p.base2wheel_positions[i][1],
                   pt = p.base2wheel_angles[i];
      const double a0 = std::cos(pt) - std::tan(g) * std::sin(pt), a1 = std::sin(pt) + std::tan(g) * std::cos(pt);
      J[i * 3 + 0] = a0 / r;
      J[i * 3 + 1] = a1 / r;
      J[i * 3 + 2] = (-a0 * py + a1 * px) / r;
    }
    *W = n;
    return DRC_OK;
  }
  if (p.type == DRC_DRIVE_CASTER) {  // CasterIKJacobian (:109-125), steer angle = wheel_pos(2i)
    const int C = p.n_wheels;
    if (C < 1 || 2 * C > kMaxWheels) return set_err(DRC_ERR_INVALID_ARGUMENT, "caster count out of range");
    const double b = p.wheel_offset;
    for (int i = 0; i < C; ++i) {
      const double phi = wheel_pos ? wheel_pos[2 * i] : 0.0, sp = std::sin(phi), cp = std::cos(phi);
      const double px = p.base2wheel_positions[i][0], py = p.base2wheel_positions[i][1];
      double* r0 = J + (2 * i) * 3;
      double* r1 = J + (2 * i + 1) * 3;
      r0[0] = -sp / b;
      r0[1] = cp / b;
      r0[2] = (px * cp + py * sp) / b - 1;
      r1[0] = cp / r;
      r1[1] = sp / r;
      r1[2] = (px * sp - py * cp) / r;
    }
    *W = 2 * C;
    return DRC_OK;
  }
  return set_err(DRC_ERR_INVALID_ARGUMENT, "unknown drive type");
}

// lane_task.hpp (the off-by-default debug stage) knows the primitives only
static const char kMeshStageMsg[] =
    "the model has collision meshes: the lane-per-instance debug stage handles sphere, cylinder and box geometry only";

// What a call carries for the task stage's build (launch.hpp StageIn), as its
// entry states it: nothing (the plain entries: the Plain build), or the obstacle
// poses (drc_qpik_*obstacles_batch: [n][12][ld] in x_target's layout, ld = 0 one
// set shared by the batch), or those and their twists
// (drc_qpik_*moving_obstacles_batch: [n][6][ld] with the poses' ld, and the
// stage output dist_rate; NULL twists: the obstacle entry itself).
// check_slots() then holds it against the model
static StageIn stage_in(const double* obstacle_pose, int64_t obstacle_ld, const double* obstacle_twist = nullptr,
                        double* dist_rate = nullptr) {
  if (!obstacle_twist) return {StageBuild::Obst, {obstacle_pose, obstacle_ld}, {}};
  return {StageBuild::Rate, {obstacle_pose, obstacle_ld}, {obstacle_twist, obstacle_ld, dist_rate}};
}
// The twists against the call: the rate reaches the QP as d + (dd/dt) / alpha_cbf
// (task_stage.hpp RATE), so a call with twists needs alpha_cbf > 0
static int check_rate(const StageIn& si, const drc_qpik_params* params) {
  if (si.build == StageBuild::Rate && !(params->alpha_cbf > 0))
    return set_err(DRC_ERR_INVALID_ARGUMENT, "obstacle_twist needs alpha_cbf > 0: the rate enters the QP as d + rate / alpha_cbf");
  return DRC_OK;
}
static const char kSlotsPlainMsg[] =
    "the model has obstacle slots: pass their poses through drc_qpik_obstacles_batch, "
    "drc_qpik_stages_obstacles_batch or drc_qpik_rollout_obstacles_batch";
static const char kSlotsUnsupportedMsg[] =
    "the model has obstacle slots: only the drc_qpik_*obstacles_batch entries take their poses "
    "(drc_model_set_obstacles with n = 0 removes the slots)";
// The call's build against the model: slots need poses (slots_msg: the entry's
// own "pass their poses through ..."), poses need slots (plain_entry: the entry
// that runs a model without them, where the text names one).  Then the build
// is the model's and the call's together (call_plan.hpp stage_build): a plain
// call on a hull model runs the Mesh build
static int check_slots(const drc_model_impl* m, StageIn* si, const char* slots_msg, const char* plain_entry = nullptr) {
  const DevModel& dm = m->hm.dev;
  const bool slots = dm.nobst > 0, poses = takes_poses(si->build);
  if (slots && !poses) return set_err(DRC_ERR_INVALID_ARGUMENT, slots_msg);
  if (!slots && poses)
    return set_err(DRC_ERR_INVALID_ARGUMENT,
                   std::string("the model has no obstacle slots (drc_model_set_obstacles declares them)") +
                       (plain_entry ? std::string(": ") + plain_entry + " runs it" : std::string()));
  si->build = stage_build(dm.has_mesh != 0, slots, si->build == StageBuild::Rate);
  return DRC_OK;
}
// ... and the poses themselves: [nobst][12][ld] with ld = 0 or at least `cols` columns
static int check_obstacle_pose(const StageIn& si, int64_t cols, const char* cols_name) {
  if (takes_poses(si.build) && cols > 0 && (!si.ob.pose || (si.ob.ld != 0 && si.ob.ld < cols)))
    return set_err(DRC_ERR_INVALID_ARGUMENT,
                   std::string("obstacle_pose is required, obstacle_ld is 0 (shared) or at least ") + cols_name);
  return DRC_OK;
}

static int upload(drc_model_impl* m) {
  HIP_TRY(hipSetDevice(m->device));
  if (m->hm.has_mesh() && !m->d_mesh) {  // the hulls' vertices: one model-owned buffer
    const size_t bytes = m->hm.mesh_verts.size() * sizeof(double);
    HIP_TRY(hipMalloc(&m->d_mesh, bytes));
    HIP_TRY(hipMemcpy(m->d_mesh, m->hm.mesh_verts.data(), bytes, hipMemcpyHostToDevice));
    m->hm.dev.mesh_verts = m->d_mesh;
  }
  {  // the task stage's per-pair records (model.cpp build_stage_tables)
    const size_t bytes = m->hm.pair_tab.size() * sizeof(double);
    if (m->d_pair_tab) HIP_TRY(hipFree(m->d_pair_tab));  // a re-upload (drc_model_set_obstacles)
    m->d_pair_tab = nullptr;
    HIP_TRY(hipMalloc(&m->d_pair_tab, bytes));
    HIP_TRY(hipMemcpy(m->d_pair_tab, m->hm.pair_tab.data(), bytes, hipMemcpyHostToDevice));
    m->hm.dev.pair_tab = m->d_pair_tab;
  }
  {  // the certified clearance's motion weights (model.cpp build_motion_tables)
    const size_t bytes = m->hm.motion_wt.size() * sizeof(double);
    if (m->d_motion_wt) HIP_TRY(hipFree(m->d_motion_wt));  // a re-upload (drc_model_set_obstacles)
    m->d_motion_wt = nullptr;
    HIP_TRY(hipMalloc(&m->d_motion_wt, bytes));
    HIP_TRY(hipMemcpy(m->d_motion_wt, m->hm.motion_wt.data(), bytes, hipMemcpyHostToDevice));
    m->hm.dev.motion_wt = m->d_motion_wt;
  }
  if (!m->d_model) HIP_TRY(hipMalloc(&m->d_model, sizeof(DevModel)));
  HIP_TRY(hipMemcpy(m->d_model, &m->hm.dev, sizeof(DevModel), hipMemcpyHostToDevice));
  return DRC_OK;
}

static int make_kparams(const drc_model_impl* mm, const drc_qpik_params* p, int stages, KParams* k,
                        int problem = 0, int cf = 0) {
  const DevModel& M = mm->hm.dev;
  std::memset(k, 0, sizeof(*k));
  k->problem = problem;
  k->cf = cf;
  for (int i = 0; i < 6; ++i) {
    k->kp[i] = p->kp[i];
    k->kv[i] = p->kv[i];
  }
  k->ff = p->feedforward;
  k->alpha_cbf = p->alpha_cbf;
  k->w_reg = p->w_reg;
  k->slack_w = p->slack_w;
  k->man_min = p->man_min;
  k->dist_min = p->dist_min;
  k->t = p->t;
  k->t0 = p->t0;
  k->duration = p->duration;
  if (stages && p->frame_id == -1) {  // stage outputs without a task frame: last joint
    k->frame_joint = M.nv;
    static const double eye[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
    std::memcpy(k->frame_place, eye, sizeof(k->frame_place));
  } else {
    if (p->frame_id < 0 || p->frame_id >= M.nframes)
      return set_err(DRC_ERR_UNKNOWN_LINK, "params.frame_id does not name a link of the model");
    if (M.frame_joint[p->frame_id] == 0)
      return set_err(DRC_ERR_UNKNOWN_LINK, "task frame is attached to the universe (no joint moves it)");
    k->frame_joint = M.frame_joint[p->frame_id];
    std::memcpy(k->frame_place, M.frame_place[p->frame_id], sizeof(k->frame_place));
  }
  if (p->mode < DRC_MODE_QPIK || p->mode > DRC_MODE_QPIK_CUBIC) return set_err(DRC_ERR_INVALID_ARGUMENT, "bad mode");
  k->mode = p->mode;
  k->stages = stages;
  k->s = p->solver;
  k->eqp_small = mm->eqp_small_cap < 0 || mm->eqp_small_cap > kEqpSmallCap ? kEqpSmallCap : mm->eqp_small_cap;
  if (plan_dims(M, k)) return set_err(DRC_ERR_UNSUPPORTED, "QP larger than one wavefront's row mapping");
  if (k->s.max_iter < 1 || k->s.check_termination < 0) return set_err(DRC_ERR_INVALID_ARGUMENT, "bad solver settings");
  // the LDS plan (lds_plan.hpp): the task kernel's, or the QP kernel's
  if (stages ? plan_task(M, k, mm->task_plan_wide) : plan_qp(M, k, qp_compiled(k->nx, k->ng, k->np)))
    return set_err(DRC_ERR_UNSUPPORTED, "model too large for the per-wave LDS plan");
  return DRC_OK;
}

// The record of a call: kernel_common.hpp's IO, filled by field name.  The
// entries set the caller's arrays; the launch functions add the scratch, the
// queue and the order of each launch
static IO make_io(int64_t B) {
  IO io{};
  io.B = B;
  io.b0 = 0;
  io.ld = B;
  return io;
}
// ... with the six task inputs that every controller entry of the C ABI
// takes, in the ABI's order.  Everything else is assigned by name
static IO task_io(int64_t B, const double* q, const double* qdot, const double* xt, const double* xdt,
                  const double* xi, const double* xdi) {
  IO io = make_io(B);
  io.q = q;
  io.qdot = qdot;
  io.xt = xt;
  io.xdt = xdt;
  io.xi = xi;
  io.xdi = xdi;
  return io;
}

// The inputs a mode needs: the state and xdot_target (state_msg names them as
// the entry does), x_target for Step / Cubic, x_init / xdot_init for Cubic
// (family: QPIK or QPID)
static int check_mode_inputs(const IO& io, int mode, const char* state_msg, const char* family) {
  if (!io.q || !io.qdot || !io.xdt) return set_err(DRC_ERR_INVALID_ARGUMENT, state_msg);
  if (mode != DRC_MODE_QPIK && !io.xt)
    return set_err(DRC_ERR_INVALID_ARGUMENT,
                   std::string("x_target required for ") + family + "Step/" + family + "Cubic");
  if (mode == DRC_MODE_QPIK_CUBIC && (!io.xi || !io.xdi))
    return set_err(DRC_ERR_INVALID_ARGUMENT, std::string("x_init/xdot_init required for ") + family + "Cubic");
  return DRC_OK;
}

// The knobs of the dispatch plan (call_plan.hpp), read once
static const PlanKnobs& plan_knobs() {
  static const PlanKnobs k = [] {
    PlanKnobs v;
    v.fuse_max = env_int("DRC_FUSE_MAX", v.fuse_max, 0);
    v.order_min = env_int("DRC_ORDER_MIN", v.order_min, 0);
    v.order_max = env_int("DRC_ORDER_MAX", v.order_max, 0);
    v.min_subbatch = env_int("DRC_MIN_SUBBATCH", v.min_subbatch, 1);
    v.grid_task = env_int("DRC_GRID_TASK", v.grid_task, 8);
    v.grid_qp = env_int("DRC_GRID_QP", v.grid_qp, 8);
    v.grid_fused = env_int("DRC_GRID_FUSED", v.grid_fused, 8);
    v.grid_clear = env_int("DRC_GRID_CLEAR", v.grid_clear, 8);
    return v;
  }();
  return k;
}
// ... and its view of a call of B instances on the model (kq: the QP's
// parameters, none for a stage call; si: what the call carries)
static PlanIn plan_in(const drc_model_impl* m, int64_t B, int stages, const KParams* kq, const StageIn& si) {
  const DevModel& dm = m->hm.dev;
  PlanIn in;
  in.B = B;
  in.stages = stages;
  in.fused = m->fused;
  in.lane_stage = m->lane_stage;
  in.chunks = m->chunks;
  in.caller_order = m->d_order && m->order_n == B;
  in.kind = dm.kind;
  in.nv = dm.nv;
  in.ncand_slots = dm.ncand_slots;
  in.has_mesh = dm.has_mesh != 0;
  in.slots = dm.nobst > 0;
  in.twists = si.build == StageBuild::Rate;
  in.qp_compiled = kq && qp_compiled(kq->nx, kq->ng, kq->np);
  in.qp_group = 64;
  in.max_cand_slots = kMaxCandSlots;
  in.knobs = plan_knobs();
  return in;
}

// One QPIK call (stages: the task stage's outputs only) of call.B instances:
// the checks, the plan (call_plan.hpp), scratch and streams, then one pass
// that enqueues each sub-batch.
// (the caller holds m->launch_mu: launch() for one call, the stepwise rollout
// for its whole sequence of steps)
static int launch_locked(drc_model_impl* m, const drc_qpik_params* params, int stages, const IO& call, void* stream,
                         StageIn si = {}) {
  const int64_t B = call.B;
  if (B < 0) return set_err(DRC_ERR_INVALID_ARGUMENT, "negative batch");
  if (int r = check_slots(m, &si, kSlotsPlainMsg)) return r;
  if (int r = check_obstacle_pose(si, B, "the batch")) return r;
  if (int r = check_rate(si, params)) return r;
  if (B == 0) return DRC_OK;
  if (B > 0x7ffffff0) return set_err(DRC_ERR_INVALID_ARGUMENT, "batch too large");  // 32-bit work-queue counters
  if (int r = check_mode_inputs(call, params->mode, "q, qdot and xdot_target are required", "QPIK")) return r;
  if (!stages && (!call.out || !call.status))
    return set_err(DRC_ERR_INVALID_ARGUMENT, "qdot_out and status are required");
  KParams kt, kq;
  int rc = make_kparams(m, params, 1, &kt);
  if (rc) return rc;
  if (!stages) {
    rc = make_kparams(m, params, 0, &kq);
    if (rc) return rc;
  }
  Launch L(m, stream);
  if (int r = L.begin()) return r;
  hipStream_t st = L.st;
  StreamCtx* const cx = L.cx;
  // product path: per-instance task records in the stream's pool; the stage
  // API writes [field][B]
  const int64_t stride = record_stride(kt.rLen);
  const DevModel& dm = m->hm.dev;
  const PlanIn pin = plan_in(m, B, stages, stages ? nullptr : &kq, si);
  const CallPlan plan = plan_call(pin);
  const bool lane = plan.lane, fuse = plan.fuse, auto_order = plan.auto_order;
  const int ls = m->lane_stage, S = plan.S;
  QpikPool pool{};
  if (!stages || lane)
    if (int r = L.carve(&StreamCtx::pool, [&](void* p) { return qpik_pool(p, stride, B, stages != 0, auto_order); },
                        &pool))
      return r;
  const bool timed = m->timing && !stages;
  std::vector<hipEvent_t> tev;
  // (timing events come from the model's pool: creating five to fourteen
  // events per call cost host time inside the bench's timed region)
  auto mkev = [&](hipEvent_t* e) -> int {
    {
      std::lock_guard<std::mutex> g(m->mu);
      if (!m->evpool.empty()) {
        *e = m->evpool.back();
        m->evpool.pop_back();
      } else {
        *e = nullptr;
      }
    }
    if (!*e) HIP_TRY(hipEventCreate(e));
    tev.push_back(*e);
    return DRC_OK;
  };
  {
    std::lock_guard<std::mutex> g(m->mu);
    while (static_cast<int>(m->ln.lanes.size()) < S) {
      hipStream_t ls;
      hipEvent_t je;
      HIP_TRY(hipStreamCreateWithFlags(&ls, hipStreamNonBlocking));
      HIP_TRY(hipEventCreateWithFlags(&je, hipEventDisableTiming));
      m->ln.lanes.push_back(ls);
      m->ln.joins.push_back(je);
    }
    while (lane && !stages && ls == 1 && static_cast<int>(m->ln.sides.size()) < S) {
      hipStream_t ss;
      hipEvent_t f, j;
      HIP_TRY(hipStreamCreateWithFlags(&ss, hipStreamNonBlocking));
      HIP_TRY(hipEventCreateWithFlags(&f, hipEventDisableTiming));
      HIP_TRY(hipEventCreateWithFlags(&j, hipEventDisableTiming));
      m->ln.sides.push_back(ss);
      m->ln.side_fork.push_back(f);
      m->ln.side_join.push_back(j);
    }
    if (!m->ln.fork) HIP_TRY(hipEventCreateWithFlags(&m->ln.fork, hipEventDisableTiming));
  }
  // (one sub-batch: its own task-start / last events bracket the call, no
  // separate call events)
  hipEvent_t e_start = nullptr, e_end = nullptr, t0e = nullptr, t1e = nullptr, t2e = nullptr;
  if (timed && S > 1) {
    if (int r = mkev(&e_start)) return r;
    if (int r = mkev(&e_end)) return r;
    HIP_TRY(hipEventRecord(e_start, st));
  }
  L.forks = &m->ln;  // (launch_mu held: the stream lists do not change under it)
  if (S > 1) HIP_TRY(hipEventRecord(m->ln.fork, st));
  for (int c = 0; c < S; ++c) {
    const SubBatch sb = plan_sub_batch(pin, plan, c);
    const int64_t b0 = sb.b0, Bc = sb.Bc;
    // the last sub-batch runs on the caller's stream itself: S sub-batches take
    // S streams, so S = 4 still fits HIP's default 4 hardware queues per process
    const bool own = S > 1 && c < S - 1;
    hipStream_t cs = own ? m->ln.lanes[c] : st;
    if (own) HIP_TRY(hipStreamWaitEvent(cs, m->ln.fork, 0));
    KParams kt_c = kt, kq_c = kq;
    kt_c.xcd_map = kq_c.xcd_map = sb.xcd_map;
    const int64_t gq = sb.grid_qp;
    const unsigned gt = static_cast<unsigned>(sb.grid_task);
    // this sub-batch's record: the caller's arrays, its range, its scratch
    IO io = call;
    io.B = Bc;
    io.b0 = b0;
    io.rec = pool.rec ? pool.rec + b0 * stride : nullptr;
    io.rec_stride = stride;
    if (stages) io.stamps = nullptr;
    io.order = plan.use_caller_order ? m->d_order : nullptr;
    int* qc = cx->d_queue + c * StreamCtx::kSlotInts;  // c < 16 (drc_set_concurrency)
    // the whole slot (128 B, one aligned fill; 17 ints took two fill kernels)
    HIP_TRY(hipMemsetAsync(qc, 0, StreamCtx::kSlotInts * sizeof(int), cs));
    io.queue = qc + StreamCtx::kSlotTask;
    hipEvent_t e0 = nullptr, e1 = nullptr, e2 = nullptr;
    // kernel timing: every sub-batch's task and QP launches (each marker is a
    // queue packet between two kernels; a call of one sub-batch records two or
    // three: the five of r05 cost 6 % at FR3 B = 4 096.  Timing only the
    // caller-stream sub-batch of a four-sub-batch call saved 1.5 % but its
    // events then disagreed with rocprofv3's kernel averages by ~40 %, r05fin)
    if (timed) {
      if (int r = mkev(&e0)) return r;
      if (int r = mkev(&e1)) return r;
      if (!fuse)  // the fused kernel has no QP launch of its own: its end is e1
        if (int r = mkev(&e2)) return r;
      HIP_TRY(hipEventRecord(e0, cs));
      t0e = e0;
      t1e = e1;
      t2e = fuse ? e1 : e2;
    }
    const size_t lds_t = static_cast<size_t>(kt_c.lds_doubles) * sizeof(double);
    const size_t lds_q = stages ? 0 : static_cast<size_t>(kq_c.lds_doubles) * sizeof(double);
    auto launch_qp = [&]() -> int {
      io.queue = qc + StreamCtx::kSlotQp;
      // compile-time QP shapes of the bundled robots; anything else runs the
      // runtime-sized instantiation
      if (m->qp_dense && dm.kind == 0 && qp_compiled(kq_c.nx, kq_c.ng, kq_c.np)) {  // the dense reference build
        HIP_TRY(static_cast<hipError_t>(
            launch_qp_dense_kernel(static_cast<unsigned>(gq), lds_q, cs, m->d_model, kq_c, io)));
        ++m->qp_dense_launches;
        return DRC_OK;
      }
      HIP_TRY(static_cast<hipError_t>(launch_qp_kernel(static_cast<unsigned>(gq), lds_q, cs, m->d_model, kq_c, io)));
      return DRC_OK;
    };
    if (pool.order) {  // this sub-batch's order (hot count in the zeroed queue slot; hot list / flags after it)
      HIP_TRY(static_cast<hipError_t>(launch_order_kernel(Bc, cs, m->d_model, io, qc + StreamCtx::kSlotHot,
                                                          pool.hot + b0, pool.hot_flag + b0, pool.order)));
      io.order = pool.order;
    }
    if (fuse) {  // one fused task + QP kernel, the record in LDS
      const int64_t gf = sb.grid_fused;
      const size_t lds_f = static_cast<size_t>(fused_lds_doubles(kt_c, kq_c)) * sizeof(double);
      io.queue = qc + StreamCtx::kSlotTask;
      HIP_TRY(static_cast<hipError_t>(
          launch_fused_kernel(static_cast<unsigned>(gf), lds_f, cs, m->d_model, kt_c, kq_c, io, si)));
      if (timed) HIP_TRY(hipEventRecord(e1, cs));
    } else if (!lane) {  // wave-per-instance task kernel on every instance, then the QP
      HIP_TRY(static_cast<hipError_t>(launch_task_kernel(0, gt, lds_t, cs, m->d_model, kt_c, io, si)));
      if (timed) HIP_TRY(hipEventRecord(e1, cs));
      if (!stages)
        if (int r = launch_qp()) return r;
    } else {
      // lane stage for every instance; the wave-per-instance task kernel only
      // for the instances it hands back (hard list)
      io.hard_list = pool.hard + b0;
      io.hard_n = qc + StreamCtx::kSlotHard;
      io.hard_flag = stages ? nullptr : pool.hard_flag + b0;
      const unsigned gl = static_cast<unsigned>((Bc + 63) / 64);  // one lane per instance
      HIP_TRY(static_cast<hipError_t>(launch_lane_task_kernel(dm.nv, gl, cs, m->d_model, kt_c, io)));
      if (timed) HIP_TRY(hipEventRecord(e1, cs));
      io.hard_mode = 1;
      if (stages || ls != 1) {  // hard task kernel, then one QP pass over every instance
        HIP_TRY(static_cast<hipError_t>(launch_task_kernel(0, gt, lds_t, cs, m->d_model, kt_c, io, si)));
        io.hard_mode = 0;
        if (!stages)
          if (int r = launch_qp()) return r;
      } else {
        // hard task kernel on the side stream, overlapped with the QP of the
        // other instances; then the QP of the hard ones
        hipStream_t ss = m->ln.sides[c];
        HIP_TRY(hipEventRecord(m->ln.side_fork[c], cs));
        HIP_TRY(hipStreamWaitEvent(ss, m->ln.side_fork[c], 0));
        HIP_TRY(static_cast<hipError_t>(launch_task_kernel(0, gt, lds_t, ss, m->d_model, kt_c, io, si)));
        HIP_TRY(hipEventRecord(m->ln.side_join[c], ss));
        io.hard_mode = 2;
        if (int r = launch_qp()) return r;
        HIP_TRY(hipStreamWaitEvent(cs, m->ln.side_join[c], 0));
        io.hard_mode = 1;
        if (int r = launch_qp()) return r;
      }
      io.hard_mode = 0;
    }
    if (timed && !fuse) HIP_TRY(hipEventRecord(e2, cs));
    if (own) HIP_TRY(hipEventRecord(m->ln.joins[c], cs));
  }
  for (int c = 0; c < S - 1; ++c) HIP_TRY(hipStreamWaitEvent(st, m->ln.joins[c], 0));
  if (timed) {
    if (S > 1) HIP_TRY(hipEventRecord(e_end, st));
    std::vector<hipEvent_t> ev = S > 1 ? tev : std::vector<hipEvent_t>{t0e, t2e, t0e, t1e, t2e};
    std::lock_guard<std::mutex> g(m->mu);
    m->events.push_back({ev, S});
  }
  return L.done();
}

static int launch(const drc_model_impl* cm, const drc_qpik_params* params, int stages, const IO& call, void* stream,
                  const StageIn& si = {}) {
  drc_model_impl* m = const_cast<drc_model_impl*>(cm);
  if (!m || !params) return set_err(DRC_ERR_INVALID_ARGUMENT, "null model/params");
  std::lock_guard<std::mutex> launch_lock(m->launch_mu);
  return launch_locked(m, params, stages, call, stream, si);
}

// --------------------------------------------------------------------------
// The closed-loop entries (rollout, reach, reach_path, reach_seeds): what their
// host sides have in common
// --------------------------------------------------------------------------
static bool finite_positive(double x) { return std::isfinite(x) && x > 0; }

static int check_dt(double dt) {
  if (!finite_positive(dt)) return set_err(DRC_ERR_INVALID_ARGUMENT, "dt must be finite and positive");
  return DRC_OK;
}
static int check_dt_tolerances(double dt, double pos_tol, double rot_tol) {
  if (int rc = check_dt(dt)) return rc;
  if (!finite_positive(pos_tol) || !finite_positive(rot_tol))
    return set_err(DRC_ERR_INVALID_ARGUMENT, "pos_tol and rot_tol must be finite and positive");
  return DRC_OK;
}
static int check_batch(int64_t B) {
  if (B < 0) return set_err(DRC_ERR_INVALID_ARGUMENT, "negative batch");
  if (B > 0x7ffffff0) return set_err(DRC_ERR_INVALID_ARGUMENT, "batch too large");  // 32-bit work-queue counters
  return DRC_OK;
}
// the task stage's and the QP's parameters of a QPIK call
static int make_kparams_pair(const drc_model_impl* m, const drc_qpik_params* params, KParams* kt, KParams* kq) {
  if (int rc = make_kparams(m, params, 1, kt)) return rc;
  return make_kparams(m, params, 0, kq);
}

// What a persistent closed-loop launch needs first: the grid, the placement
// and the zeroed work queue of io, the caller's IO of the whole batch (q, qdot,
// the targets, eta / status / iters -- one step's scratch or the trajectories;
// every other member null)
static int persistent_setup(StreamCtx* cx, hipStream_t st, KParams* kt, KParams* kq, IO* io, unsigned* grid) {
  *grid = static_cast<unsigned>(persistent_grid(io->B, plan_knobs().grid_fused));
  kt->xcd_map = kq->xcd_map = xcd_map_for(io->B);
  HIP_TRY(hipMemsetAsync(cx->d_queue, 0, StreamCtx::kSlotInts * sizeof(int), st));
  io->queue = cx->d_queue + StreamCtx::kSlotTask;  // slot 0, as a fused call's single sub-batch
  return DRC_OK;
}

// Start of a stepwise reach: the finals carry the state from the start, every
// instance active, the counters zero
static int stepwise_reach_init(hipStream_t st, int64_t B, int nv, const double* q0, const double* qdot0,
                               const ReachArgs& re) {
  const size_t state_bytes = size_t(nv) * B * 8;
  if (re.qf != q0) HIP_TRY(hipMemcpyAsync(re.qf, q0, state_bytes, hipMemcpyDeviceToDevice, st));
  if (re.vf != qdot0) HIP_TRY(hipMemcpyAsync(re.vf, qdot0, state_bytes, hipMemcpyDeviceToDevice, st));
  HIP_TRY(hipMemsetAsync(re.result, 0xff, size_t(B) * 4, st));  // kReachActive
  if (re.status_last) HIP_TRY(hipMemsetAsync(re.status_last, 0, size_t(B) * 4, st));
  if (re.iters_total) HIP_TRY(hipMemsetAsync(re.iters_total, 0, size_t(B) * 4, st));
  return DRC_OK;
}

// Whether a reach entry of `family` runs its persistent kernel: the rollout's
// rule, up to the largest batch at which the persistent kernel was measured to
// beat the stepwise path -- every size measured, through 65 536: one waypoint
// of 32 steps (FR3 556 against 1 674 ms, Husky-FR3 43.9 against 151.7 ms;
// profiles/reach_bench.json, DESIGN.md "Reach"), 3 waypoints of 32 steps (FR3
// 1 191 against 8 654 ms, Husky-FR3 129 against 570 ms) and four slots with
// one waypoint (FR3 565 against 1 786 ms; profiles/reach_path_bench.json,
// DESIGN.md "Reach paths").  Unlike a rollout's, a reach call's stepwise path
// pays the horizon for every instance.  DRC_REACH_MAX overrides (read per
// call, so that one process can measure both paths).  No persistent build has
// the hull narrow phase
static bool reach_persistent(const drc_model_impl* m, int64_t B, const KParams& kq, const StageIn& si,
                             StageFamily family) {
  return persistent_path(plan_in(m, B, 0, &kq, si), env_int("DRC_REACH_MAX", 65536, 0), family);
}

// drc_qpik_rollout_batch: `steps` control cycles (QPIK*, then the state
// update) enqueued on the caller's stream.  The compiled QP shapes up to
// rollout_max instances run the persistent kernel (rollout_kernel.hip: one
// launch, every instance's whole horizon on one wave); everything else runs
// step by step: drc_qpik_batch's launch sequence (and, for pose_traj /
// dist_traj, the stage launch) followed by the integrate kernel, q_final /
// qdot_final carrying the state.  Same device functions either way: identical
// bits (tests/test_gpu_rollout.py).
static int rollout(const drc_model_impl* cm, const drc_qpik_params* params, int64_t B, int steps, double dt,
                   const double* q0, const double* qdot0, const double* xt, const double* xdt, const double* xi,
                   const double* xdi, int per_step, double* qf, double* vf, double* qdot_traj, int32_t* status_traj,
                   int32_t* iters_traj, double* q_traj, double* pose_traj, double* dist_traj, void* stream,
                   StageIn si = {}, int ob_per_step = 0) {
  drc_model_impl* m = const_cast<drc_model_impl*>(cm);
  if (!m || !params) return set_err(DRC_ERR_INVALID_ARGUMENT, "null model/params");
  std::lock_guard<std::mutex> launch_lock(m->launch_mu);
  if (int rc = check_slots(m, &si, kSlotsPlainMsg)) return rc;
  if (ob_per_step != 0 && ob_per_step != 1)
    return set_err(DRC_ERR_INVALID_ARGUMENT, "obstacles_per_step must be 0 or 1");
  if (int rc = check_obstacle_pose(si, B, "the batch")) return rc;
  if (int rc = check_rate(si, params)) return rc;
  if (steps < 1) return set_err(DRC_ERR_INVALID_ARGUMENT, "steps must be at least 1");
  if (int rc = check_dt(dt)) return rc;
  if (per_step != 0 && per_step != 1) return set_err(DRC_ERR_INVALID_ARGUMENT, "targets_per_step must be 0 or 1");
  if (per_step && params->mode == DRC_MODE_QPIK_CUBIC)
    return set_err(DRC_ERR_INVALID_ARGUMENT, "per-step targets with QPIKCubic: the time already moves the target");
  if (!qf || !vf || !status_traj)
    return set_err(DRC_ERR_INVALID_ARGUMENT, "q_final, qdot_final and status_traj are required");
  if (int rc = check_batch(B)) return rc;
  // the inputs at step 0: the persistent kernel's record, the template of a step's
  const IO in = task_io(B, q0, qdot0, xt, xdt, xi, xdi);
  if (B > 0)
    if (int rc = check_mode_inputs(in, params->mode, "q0, qdot0 and xdot_target are required", "QPIK")) return rc;
  KParams kt, kq;
  if (int rc = make_kparams_pair(m, params, &kt, &kq)) return rc;
  if (B == 0) return DRC_OK;
  Launch L(m, stream);
  if (int r = L.begin()) return r;
  hipStream_t st = L.st;
  StreamCtx* const cx = L.cx;
  const DevModel& dm = m->hm.dev;
  const int nv = dm.nv, na = kq.na;
  // The persistent kernel up to the batch size where it was measured to beat
  // the stepwise path at 32 steps (profiles/rollout_bench.json, DESIGN.md
  // "Rollouts"): manipulators (FR3) through 4 096 instances -- from 8 192 on
  // the stepwise path's fused calls with their EPA-first order win, 10.8
  // against 12.4 ms -- and whole-body robots (Husky-FR3) at every size
  // measured, through 65 536 (92.8 against 133.2 ms).  DRC_ROLLOUT_MAX
  // overrides (read per call, so that one process can measure both paths)
  const int64_t rollout_max = env_int("DRC_ROLLOUT_MAX", dm.kind == 0 ? 4096 : 65536, 0);
  // (models with obstacle slots: the stepwise path; no persistent build takes poses)
  const bool persistent = persistent_path(plan_in(m, B, 0, &kq, si), rollout_max, StageFamily::Rollout);
  RolloutScratch sc;
  if (int r = L.carve(&StreamCtx::roll, [&](void* p) { return rollout_scratch(p, na, B, qdot_traj != nullptr); }, &sc))
    return r;
  double* eta = qdot_traj ? qdot_traj : sc.eta;  // without qdot_traj: one step's eta in stream scratch
  const int64_t out_step = qdot_traj ? int64_t(na) * B : 0;
  if (persistent) {
    IO io = in;
    io.out = eta;
    io.status = status_traj;
    io.iters = iters_traj;
    unsigned grid;
    if (int r = persistent_setup(cx, st, &kt, &kq, &io, &grid)) return r;
    HIP_TRY(static_cast<hipError_t>(launch_rollout_kernel(grid, st, m->d_model, kt, kq, io, steps, per_step, dt, qf, vf,
                                                          q_traj, pose_traj, dist_traj, out_step, si)));
    return L.done();
  }
  for (int k = 0; k < steps; ++k) {
    drc_qpik_params pk = *params;
    pk.t = rollout_time(params->t, k, dt);
    const double *qk = k ? qf : q0, *vk = k ? vf : qdot0;
    const double* xt_k = per_step && xt ? xt + int64_t(k) * 12 * B : xt;
    const double* xdt_k = per_step ? xdt + int64_t(k) * 6 * B : xdt;
    double* eta_k = eta + k * out_step;
    // this step's pose set and twists, or the shared ones
    const StageIn si_k = ob_per_step ? si.at_step(k, dm.nobst) : si;
    IO step = in;
    step.q = qk;
    step.qdot = vk;
    step.xt = xt_k;
    step.xdt = xdt_k;
    // (pose_traj / dist_traj: the stage launch without twists -- the geometric d)
    if (pose_traj || dist_traj) {
      IO sg = step;
      sg.st_pose = pose_traj ? pose_traj + int64_t(k) * 12 * B : nullptr;
      sg.st_dist = dist_traj ? dist_traj + int64_t(k) * (1 + nv) * B : nullptr;
      if (int rc = launch_locked(m, &pk, 1, sg, stream, si_k.without_twists())) return rc;
    }
    step.out = eta_k;
    step.status = status_traj + int64_t(k) * B;
    step.iters = iters_traj ? iters_traj + int64_t(k) * B : nullptr;
    if (int rc = launch_locked(m, &pk, 0, step, stream, si_k)) return rc;
    HIP_TRY(static_cast<hipError_t>(launch_rollout_integrate_kernel(
        B, st, m->d_model, dt, qk, eta_k, qf, vf, q_traj ? q_traj + int64_t(k) * nv * B : nullptr)));
  }
  return L.done();
}

// The reach entries' core: the QPIKStep loop through W waypoints with
// per-instance stopping (include/drc_amd.h), enqueued on the caller's stream;
// drc_qpik_reach_batch is the path of one waypoint.  The caller holds
// m->launch_mu and has made its entry's checks.  family: the entry's row of
// has_build (call_plan.hpp).  The compiled QP shapes in a build that the
// family has, up to reach_max instances, run the persistent kernel
// (reach_path_kernel.hip, reach_path_obstacle_kernel.hip: a wave leaves an
// instance when it stops and takes the next).  Everything else runs in rounds
// of the stage launch at every instance's current target (stream scratch,
// gathered by the update kernel when the instance advances), drc_qpik_batch's
// launch sequence and the update kernel, which skips the instances that have
// stopped.  That path cannot end early -- no host synchronisation, so the host
// does not know who is still active -- and enqueues the most rounds an instance
// can need.  An active instance has exactly one event per round, a step or an
// advance to the next waypoint; it has at most W max_steps steps and W - 1
// advances that do not finish it.  So one that is still active after
// R0 = W max_steps + W - 1 rounds stands before waypoint W - 1 with its
// segment's budget spent: its next verdict is REACHED or BUDGET, and no QP is
// needed.  R0 rounds with a QP are enqueued, then one stage launch and update
// that settle whoever is left.  Same device functions either way: identical
// bits (tests/test_gpu_reach.py, tests/test_gpu_reach_path.py).
// waypoints_reached: NULL for an entry without one (stream scratch holds it)
static int reach_path_locked(drc_model_impl* m, const drc_qpik_params* params, StageFamily family, int64_t B, int W,
                             int max_steps, double dt, double pos_tol, double rot_tol, const double* q0,
                             const double* qdot0, const double* x_path, const double* xdot_path, double* qf,
                             double* vf, int32_t* result, int32_t* waypoints_reached, int32_t* steps_used,
                             int32_t* status_last, int32_t* iters_total, double* err_final, double* dist_final,
                             double* dist_min, int32_t* steps_at, void* stream, const StageIn& si) {
  KParams kt, kq;
  if (int rc = make_kparams_pair(m, params, &kt, &kq)) return rc;
  if (B == 0) return DRC_OK;
  Launch L(m, stream);
  if (int r = L.begin()) return r;
  hipStream_t st = L.st;
  StreamCtx* const cx = L.cx;
  const DevModel& dm = m->hm.dev;
  const int nv = dm.nv, na = kq.na;
  double tau[2];
  reach_thresholds(pos_tol, rot_tol, tau);
  const bool persistent = reach_persistent(m, B, kq, si, family);
  ReachScratch sc;  // one step's eta, stage outputs, status and iters, the current targets, the segment counters
  if (int r = L.carve(
          &StreamCtx::roll,
          [&](void* p) {
            if (!waypoints_reached) return reach_scratch(p, na, nv, B, persistent);
            return ReachScratch{reach_path_scratch(p, na, nv, B, persistent), nullptr};
          },
          &sc))
    return r;
  if (!waypoints_reached) waypoints_reached = sc.wp;
  const ReachPathArgs rp{{max_steps, dt, tau[0], tau[1], qf, vf, result, steps_used, status_last, iters_total,
                          err_final, dist_final},
                         W, x_path, xdot_path, waypoints_reached, dist_min, steps_at, sc.xt, sc.xdt, sc.seg};
  if (persistent) {
    IO io = task_io(B, q0, qdot0, x_path, xdot_path, nullptr, nullptr);
    io.out = sc.eta;
    io.status = sc.status;
    io.iters = sc.iters;
    unsigned grid;
    if (int r = persistent_setup(cx, st, &kt, &kq, &io, &grid)) return r;
    // The one family-specific step: the reach entry keeps its own kernel, the
    // same loop without the waypoint advance: under this same host code
    // reach_path_kernel with W = 1 measured 0.6 to 1.1 % slower on FR3
    // (DESIGN.md "Reach entries unified")
    if (family == StageFamily::Reach)
      HIP_TRY(static_cast<hipError_t>(launch_reach_kernel(grid, st, m->d_model, kt, kq, io, rp.re, si)));
    else
      HIP_TRY(static_cast<hipError_t>(launch_reach_path_kernel(grid, st, m->d_model, kt, kq, io, rp, si)));
    return L.done();
  }
  // the finals carry the state from the start, every instance active at
  // waypoint 0 with no step taken
  if (int r = stepwise_reach_init(st, B, nv, q0, qdot0, rp.re)) return r;
  HIP_TRY(hipMemcpyAsync(sc.xt, x_path, size_t(12) * B * 8, hipMemcpyDeviceToDevice, st));
  HIP_TRY(hipMemcpyAsync(sc.xdt, xdot_path, size_t(6) * B * 8, hipMemcpyDeviceToDevice, st));
  HIP_TRY(hipMemsetAsync(waypoints_reached, 0, size_t(B) * 4, st));
  HIP_TRY(hipMemsetAsync(steps_used, 0, size_t(B) * 4, st));
  HIP_TRY(hipMemsetAsync(sc.seg, 0, size_t(B) * 4, st));
  if (steps_at) HIP_TRY(hipMemsetAsync(steps_at, 0xff, size_t(W) * B * 4, st));  // -1: never reached
  const int64_t rounds = int64_t(W) * max_steps + W - 1;  // R0
  IO qp = task_io(B, qf, vf, sc.xt, sc.xdt, nullptr, nullptr);  // a step's QPIK call on the finals, and its stage launch
  IO sg = qp;
  sg.st_pose = sc.pose;
  sg.st_dist = sc.dist;
  qp.out = sc.eta;
  qp.status = sc.status;
  qp.iters = sc.iters;
  for (int64_t r = 0; r <= rounds; ++r) {
    const int last = r == rounds;
    if (int rc = launch_locked(m, params, 1, sg, stream, si)) return rc;
    if (!last)
      if (int rc = launch_locked(m, params, 0, qp, stream, si)) return rc;
    HIP_TRY(static_cast<hipError_t>(launch_reach_path_update_kernel(B, st, m->d_model, r == 0, last, rp, sc.pose,
                                                                    sc.dist, sc.eta, sc.status, sc.iters)));
  }
  return L.done();
}

static const char kSlotsReachMsg[] =
    "the model has obstacle slots: pass their poses through drc_qpik_reach_obstacles_batch";

// drc_qpik_reach_batch: its own checks, then the core with x_target as a path
// of one waypoint.  Its family is Reach, whose one build is the plain one: a
// model with hulls or slots runs stepwise.
// (reach_locked: the caller holds m->launch_mu -- reach() for one call,
// reach_seeds() for its stepwise path)
static int reach_locked(drc_model_impl* m, const drc_qpik_params* params, int64_t B, int max_steps, double dt,
                        double pos_tol, double rot_tol, const double* q0, const double* qdot0, const double* xt,
                        const double* xdt, double* qf, double* vf, int32_t* result, int32_t* steps_used,
                        int32_t* status_last, int32_t* iters_total, double* err_final, double* dist_final,
                        void* stream, StageIn si) {
  if (int rc = check_slots(m, &si, kSlotsReachMsg)) return rc;
  if (int rc = check_obstacle_pose(si, B, "the batch")) return rc;
  if (params->mode != DRC_MODE_QPIK_STEP)
    return set_err(DRC_ERR_INVALID_ARGUMENT, "drc_qpik_reach_batch runs DRC_MODE_QPIK_STEP only");
  if (max_steps < 0) return set_err(DRC_ERR_INVALID_ARGUMENT, "max_steps must not be negative");
  if (int rc = check_dt_tolerances(dt, pos_tol, rot_tol)) return rc;
  if (!qf || !vf || !result || !steps_used)
    return set_err(DRC_ERR_INVALID_ARGUMENT, "q_final, qdot_final, result and steps_used are required");
  if (int rc = check_batch(B)) return rc;
  if (B > 0 && (!q0 || !qdot0 || !xt || !xdt))
    return set_err(DRC_ERR_INVALID_ARGUMENT, "q0, qdot0, x_target and xdot_target are required");
  return reach_path_locked(m, params, StageFamily::Reach, B, 1, max_steps, dt, pos_tol, rot_tol, q0, qdot0, xt, xdt, qf,
                           vf, result, nullptr, steps_used, status_last, iters_total, err_final, dist_final, nullptr,
                           nullptr, stream, si);
}

static int reach(const drc_model_impl* cm, const drc_qpik_params* params, int64_t B, int max_steps, double dt,
                 double pos_tol, double rot_tol, const double* q0, const double* qdot0, const double* xt,
                 const double* xdt, double* qf, double* vf, int32_t* result, int32_t* steps_used,
                 int32_t* status_last, int32_t* iters_total, double* err_final, double* dist_final, void* stream,
                 const StageIn& si = {}) {
  drc_model_impl* m = const_cast<drc_model_impl*>(cm);
  if (!m || !params) return set_err(DRC_ERR_INVALID_ARGUMENT, "null model/params");
  std::lock_guard<std::mutex> launch_lock(m->launch_mu);
  return reach_locked(m, params, B, max_steps, dt, pos_tol, rot_tol, q0, qdot0, xt, xdt, qf, vf, result, steps_used,
                      status_last, iters_total, err_final, dist_final, stream, si);
}

static const char kSlotsReachPathMsg[] =
    "the model has obstacle slots: pass their poses through drc_qpik_reach_path_obstacles_batch";

// drc_qpik_reach_path_batch: its own checks, then the core.  Its family has
// the builds that take the slots' poses, so models with slots run the
// persistent kernel too
static int reach_path(const drc_model_impl* cm, const drc_qpik_params* params, int64_t B, int W, int max_steps,
                      double dt, double pos_tol, double rot_tol, const double* q0, const double* qdot0,
                      const double* x_path, const double* xdot_path, double* qf, double* vf, int32_t* result,
                      int32_t* waypoints_reached, int32_t* steps_used, int32_t* status_last, int32_t* iters_total,
                      double* err_final, double* dist_final, double* dist_min, int32_t* steps_at, void* stream,
                      StageIn si = {}) {
  drc_model_impl* m = const_cast<drc_model_impl*>(cm);
  if (!m || !params) return set_err(DRC_ERR_INVALID_ARGUMENT, "null model/params");
  std::lock_guard<std::mutex> launch_lock(m->launch_mu);
  if (int rc = check_slots(m, &si, kSlotsReachPathMsg, "drc_qpik_reach_path_batch")) return rc;
  if (int rc = check_obstacle_pose(si, B, "the batch")) return rc;
  if (params->mode != DRC_MODE_QPIK_STEP)
    return set_err(DRC_ERR_INVALID_ARGUMENT, "drc_qpik_reach_path_batch runs DRC_MODE_QPIK_STEP only");
  if (W < 1) return set_err(DRC_ERR_INVALID_ARGUMENT, "waypoints must be at least 1");
  if (max_steps < 0) return set_err(DRC_ERR_INVALID_ARGUMENT, "max_steps must not be negative");
  if (int64_t(W) * (int64_t(max_steps) + 1) > 0x7ffffff0)
    return set_err(DRC_ERR_INVALID_ARGUMENT, "waypoints * (max_steps + 1) too large");  // 32-bit step counters
  if (int rc = check_dt_tolerances(dt, pos_tol, rot_tol)) return rc;
  if (!qf || !vf || !result || !waypoints_reached || !steps_used)
    return set_err(DRC_ERR_INVALID_ARGUMENT,
                   "q_final, qdot_final, result, waypoints_reached and steps_used are required");
  if (int rc = check_batch(B)) return rc;
  if (B > 0 && (!q0 || !qdot0 || !x_path || !xdot_path))
    return set_err(DRC_ERR_INVALID_ARGUMENT, "q0, qdot0, x_path and xdot_path are required");
  return reach_path_locked(m, params, StageFamily::ReachPath, B, W, max_steps, dt, pos_tol, rot_tol, q0, qdot0, x_path,
                           xdot_path, qf, vf, result, waypoints_reached, steps_used, status_last, iters_total,
                           err_final, dist_final, dist_min, steps_at, stream, si);
}

static const char kSlotsReachSeedsMsg[] =
    "the model has obstacle slots: pass their poses through drc_qpik_reach_seeds_obstacles_batch";

static_assert(kSeedsFirst == DRC_SEEDS_FIRST && kSeedsFewestSteps == DRC_SEEDS_FEWEST_STEPS &&
                  kSeedsReached == DRC_REACH_REACHED && kSeedsCancelled == DRC_REACH_CANCELLED,
              "reach_seeds.hpp restates include/drc_amd.h");

// drc_qpik_reach_seeds_batch: S seeds for each of T targets, the S T instances
// of reach() with instance (s, t) at column s T + t, and one answer per target
// by the rule of reach_seeds.hpp (include/drc_amd.h), enqueued on the caller's
// stream.  Per-instance finals and outcomes go to stream scratch, from which
// the select kernel gathers the winners.  task_instance indexes targets and
// poses with the state's stride, so the targets (and per-target poses) are
// expanded to [..][S T] in scratch first.  reach_path()'s dispatch rule applied
// to S T: the persistent kernel (reach_seeds_kernel.hip, with its ObstIn builds
// for models with slots), where seeds of a group tell each other through the
// group's word that the answer is there; everything else runs reach()'s
// stepwise path on the expanded arrays, without cancellation.  Same device
// functions either way: identical bits (tests/test_gpu_reach_seeds.py).
static int reach_seeds(const drc_model_impl* cm, const drc_qpik_params* params, int64_t T, int S, int rule, int cancel,
                       int max_steps, double dt, double pos_tol, double rot_tol, const double* q0,
                       const double* qdot0, const double* xt, const double* xdt, int32_t* seed, int32_t* result,
                       int32_t* steps_used, double* q_sol, double* qdot_sol, int32_t* status_last,
                       int32_t* iters_total, double* err_final, double* dist_final, int32_t* inst_result,
                       int32_t* inst_steps, void* stream, StageIn si = {}) {
  drc_model_impl* m = const_cast<drc_model_impl*>(cm);
  if (!m || !params) return set_err(DRC_ERR_INVALID_ARGUMENT, "null model/params");
  std::lock_guard<std::mutex> launch_lock(m->launch_mu);
  if (int rc = check_slots(m, &si, kSlotsReachSeedsMsg, "drc_qpik_reach_seeds_batch")) return rc;
  if (S < 1) return set_err(DRC_ERR_INVALID_ARGUMENT, "seeds must be at least 1");
  if (T < 0) return set_err(DRC_ERR_INVALID_ARGUMENT, "negative number of targets");
  if (rule != DRC_SEEDS_FIRST && rule != DRC_SEEDS_FEWEST_STEPS)
    return set_err(DRC_ERR_INVALID_ARGUMENT, "rule is DRC_SEEDS_FIRST or DRC_SEEDS_FEWEST_STEPS");
  if (int rc = check_obstacle_pose(si, T, "the number of targets")) return rc;
  if (params->mode != DRC_MODE_QPIK_STEP)
    return set_err(DRC_ERR_INVALID_ARGUMENT, "drc_qpik_reach_seeds_batch runs DRC_MODE_QPIK_STEP only");
  if (max_steps < 0) return set_err(DRC_ERR_INVALID_ARGUMENT, "max_steps must not be negative");
  if ((int64_t(max_steps) + 1) * S >= (int64_t(1) << 31))
    return set_err(DRC_ERR_INVALID_ARGUMENT, "(max_steps + 1) * seeds must be below 2^31");  // the 32-bit keys
  if (T > 0x7ffffff0 / S)  // 32-bit work-queue counters
    return set_err(DRC_ERR_INVALID_ARGUMENT, "seeds * targets too large");
  if (int rc = check_dt_tolerances(dt, pos_tol, rot_tol)) return rc;
  if (!seed || !result || !steps_used || !q_sol || !qdot_sol)
    return set_err(DRC_ERR_INVALID_ARGUMENT, "seed, result, steps_used, q_sol and qdot_sol are required");
  if (T > 0 && (!q0 || !qdot0 || !xt || !xdt))
    return set_err(DRC_ERR_INVALID_ARGUMENT, "q0, qdot0, x_target and xdot_target are required");
  KParams kt, kq;
  if (int rc = make_kparams_pair(m, params, &kt, &kq)) return rc;
  if (T == 0) return DRC_OK;
  Launch L(m, stream);
  if (int r = L.begin()) return r;
  hipStream_t st = L.st;
  StreamCtx* const cx = L.cx;
  const DevModel& dm = m->hm.dev;
  const int nv = dm.nv, na = kq.na;
  const int64_t B = T * S;
  double tau[2];
  reach_thresholds(pos_tol, rot_tol, tau);
  const bool persistent = reach_persistent(m, B, kq, si, StageFamily::ReachSeeds);
  const bool ob_expand = si.ob.ld != 0;
  // the expanded targets and poses, the instances' finals and outcomes, one step's scratch, the groups' words
  SeedsScratch sc;
  if (int r = L.carve(&StreamCtx::seeds,
                      [&](void* p) { return seeds_scratch(p, na, nv, dm.nobst, T, S, persistent, ob_expand); }, &sc))
    return r;
  HIP_TRY(static_cast<hipError_t>(launch_reach_seeds_expand_kernel(st, 12, T, S, xt, T, sc.xt)));
  HIP_TRY(static_cast<hipError_t>(launch_reach_seeds_expand_kernel(st, 6, T, S, xdt, T, sc.xdt)));
  if (ob_expand) {  // from here on si carries the expanded poses
    HIP_TRY(static_cast<hipError_t>(
        launch_reach_seeds_expand_kernel(st, dm.nobst * 12, T, S, si.ob.pose, si.ob.ld, sc.pose)));
    si.ob = ObstIn{sc.pose, B};
  }
  // the diagnostics are the instances' own result / steps_used
  const ReachSeedsArgs rs{{max_steps, dt, tau[0], tau[1], sc.qf, sc.vf, inst_result ? inst_result : sc.result,
                           inst_steps ? inst_steps : sc.steps, status_last ? sc.status_last : nullptr,
                           iters_total ? sc.iters_total : nullptr, sc.err, dist_final ? sc.dist : nullptr},
                          T, S, rule, persistent && cancel ? 1 : 0, sc.word};
  const ReachArgs& re = rs.re;
  if (persistent) {
    IO io = task_io(B, q0, qdot0, sc.xt, sc.xdt, nullptr, nullptr);
    io.out = sc.eta;
    io.status = sc.status;
    io.iters = sc.iters;
    unsigned grid;
    if (int r = persistent_setup(cx, st, &kt, &kq, &io, &grid)) return r;
    HIP_TRY(hipMemsetAsync(sc.word, 0xff, size_t(T) * 4, st));  // kSeedsNoKey
    HIP_TRY(static_cast<hipError_t>(launch_reach_seeds_kernel(grid, st, m->d_model, kt, kq, io, rs, si)));
  } else {
    if (int rc = reach_locked(m, params, B, max_steps, dt, pos_tol, rot_tol, q0, qdot0, sc.xt, sc.xdt, re.qf, re.vf,
                              re.result, re.steps_used, re.status_last, re.iters_total, re.err_final, re.dist_final,
                              stream, si))
      return rc;
  }
  const ReachSeedsOut out{seed, result, steps_used, q_sol, qdot_sol, status_last, iters_total, err_final, dist_final};
  HIP_TRY(static_cast<hipError_t>(launch_reach_seeds_select_kernel(st, nv, rs, out)));
  return L.done();
}

// --------------------------------------------------------------------------
// Path clearance (drc_clearance_path_batch): one launch of the persistent
// clearance kernel (clearance_kernel.hip) on the caller's stream -- every model
// runs it, there is no stepwise form.  params: defaults (the distance stage
// reads none of them; they size the task plan).  The queue is slot 0's, as a
// closed-loop entry's single launch
// --------------------------------------------------------------------------
static_assert(kClearFree == DRC_CLEAR_FREE && kClearBlocked == DRC_CLEAR_BLOCKED && kClearInvalid == DRC_CLEAR_INVALID,
              "clearance.hpp and drc_amd.h agree on the verdicts");
static const char kSlotsClearanceMsg[] =
    "the model has obstacle slots: pass their poses through drc_clearance_path_obstacles_batch";

static int clearance(const drc_model_impl* cm, const drc_qpik_params* params, int64_t B, int waypoints, int substeps,
                     double d_stop, const double* q_path, int32_t* result, int32_t* sample_stop, double* d_min,
                     int32_t* sample_min, int32_t* pair_min, double* dist_traj, void* stream, StageIn si = {}) {
  drc_model_impl* m = const_cast<drc_model_impl*>(cm);
  if (!m || !params) return set_err(DRC_ERR_INVALID_ARGUMENT, "null model/params");
  std::lock_guard<std::mutex> launch_lock(m->launch_mu);
  if (int rc = check_batch(B)) return rc;
  if (int r = check_slots(m, &si, kSlotsClearanceMsg, "drc_clearance_path_batch")) return r;
  if (int r = check_obstacle_pose(si, B, "the batch")) return r;
  if (waypoints < 1 || substeps < 1) return set_err(DRC_ERR_INVALID_ARGUMENT, "waypoints and substeps must be at least 1");
  if (d_stop != d_stop) return set_err(DRC_ERR_INVALID_ARGUMENT, "d_stop is NaN (-INFINITY never blocks)");
  if (clearance_samples(waypoints, substeps) > 0x7fffffff)
    return set_err(DRC_ERR_INVALID_ARGUMENT, "(waypoints - 1) substeps + 1 samples do not fit 31 bits");
  if (B == 0) return DRC_OK;
  if (!q_path || !result || !sample_stop || !d_min || !sample_min || !pair_min)
    return set_err(DRC_ERR_INVALID_ARGUMENT, "q_path, result, sample_stop, d_min, sample_min and pair_min are required");
  KParams kt;
  if (int rc = make_kparams(m, params, 1, &kt)) return rc;
  Launch L(m, stream);
  if (int r = L.begin()) return r;
  hipStream_t st = L.st;
  IO io = make_io(B);
  kt.xcd_map = xcd_map_for(B);
  HIP_TRY(hipMemsetAsync(L.cx->d_queue, 0, StreamCtx::kSlotInts * sizeof(int), st));
  io.queue = L.cx->d_queue + StreamCtx::kSlotTask;
  const ClearArgs ca{waypoints, substeps, d_stop, q_path, result, sample_stop, d_min, sample_min, pair_min, dist_traj};
  const unsigned grid = static_cast<unsigned>(clearance_grid(B, plan_knobs()));
  HIP_TRY(static_cast<hipError_t>(launch_clearance_kernel(
      grid, static_cast<size_t>(kt.lds_doubles) * sizeof(double), st, m->d_model, kt, io, ca, si)));
  m->clearance_grid_last = grid;
  return L.done();
}

// --------------------------------------------------------------------------
// Certified path clearance (drc_clearance_certify_batch): one launch of the
// persistent certify kernel (certify_kernel.hip), prepared as clearance() is;
// the grid is the clearance kernel's
// --------------------------------------------------------------------------
static_assert(kClearUndecided == DRC_CLEAR_UNDECIDED, "clearance_certify.hpp and drc_amd.h agree on the verdict");
static_assert(kCertMaxDepth == DRC_CERTIFY_MAX_DEPTH, "clearance_certify.hpp and drc_amd.h agree on the depth");
static const char kSlotsCertifyMsg[] =
    "the model has obstacle slots: pass their poses through drc_clearance_certify_obstacles_batch";

static int certify(const drc_model_impl* cm, const drc_qpik_params* params, int64_t B, int waypoints, double d_stop,
                   int max_depth, const double* q_path, int32_t* result, int32_t* seg_stop, double* t_stop,
                   double* d_min, int32_t* seg_min, double* t_min, int32_t* pair_min, double* d_lower,
                   int32_t* samples_used, double* motion_bound, void* stream, StageIn si = {}) {
  drc_model_impl* m = const_cast<drc_model_impl*>(cm);
  if (!m || !params) return set_err(DRC_ERR_INVALID_ARGUMENT, "null model/params");
  std::lock_guard<std::mutex> launch_lock(m->launch_mu);
  if (int rc = check_batch(B)) return rc;
  if (int r = check_slots(m, &si, kSlotsCertifyMsg, "drc_clearance_certify_batch")) return r;
  if (int r = check_obstacle_pose(si, B, "the batch")) return r;
  if (waypoints < 1) return set_err(DRC_ERR_INVALID_ARGUMENT, "waypoints must be at least 1");
  if (max_depth < 0 || max_depth > kCertMaxDepth)
    return set_err(DRC_ERR_INVALID_ARGUMENT, "max_depth must be in 0 .. " + std::to_string(kCertMaxDepth));
  if (d_stop != d_stop) return set_err(DRC_ERR_INVALID_ARGUMENT, "d_stop is NaN (-INFINITY certifies every segment at depth 0)");
  if (certify_max_samples(waypoints, max_depth) > 0x7fffffff)
    return set_err(DRC_ERR_INVALID_ARGUMENT, "(waypoints - 1) 2^max_depth + 1 evaluations do not fit 31 bits");
  if (m->hm.motion_unbounded)
    return set_err(DRC_ERR_UNSUPPORTED,
                   "a prismatic joint below a revolute one has no finite limit: the motion weights are unbounded");
  if (B == 0) return DRC_OK;
  if (!q_path || !result || !seg_stop || !t_stop || !d_min || !seg_min || !t_min || !pair_min || !d_lower ||
      !samples_used)
    return set_err(DRC_ERR_INVALID_ARGUMENT,
                   "q_path, result, seg_stop, t_stop, d_min, seg_min, t_min, pair_min, d_lower and samples_used are required");
  KParams kt;
  if (int rc = make_kparams(m, params, 1, &kt)) return rc;
  Launch L(m, stream);
  if (int r = L.begin()) return r;
  hipStream_t st = L.st;
  IO io = make_io(B);
  kt.xcd_map = xcd_map_for(B);
  HIP_TRY(hipMemsetAsync(L.cx->d_queue, 0, StreamCtx::kSlotInts * sizeof(int), st));
  io.queue = L.cx->d_queue + StreamCtx::kSlotTask;
  const CertArgs ca{waypoints, max_depth, d_stop,   q_path,  result,       seg_stop,    t_stop, d_min,
                    seg_min,   t_min,     pair_min, d_lower, samples_used, motion_bound};
  const unsigned grid = static_cast<unsigned>(clearance_grid(B, plan_knobs()));
  HIP_TRY(static_cast<hipError_t>(launch_certify_kernel(
      grid, static_cast<size_t>(kt.lds_doubles) * sizeof(double), st, m->d_model, kt, io, ca, si)));
  m->clearance_grid_last = grid;
  return L.done();
}

// QPID pipeline for one call: dynamics launch(es) -> task kernel (QPID stage
// data into the records) -> QPID kernel; or, with stages, the task kernel
// writing the stage outputs.  Model-owned scratch holds the records and the
// dynamics ([na*na][B] M, [na][B] g, MoMa also [nv][B] joint-order g).
// (call: out = qddot, out2 = tau; the stage outputs with st_jdot, st_qpid, st_gdv)
static int launch_qpid(const drc_model_impl* cm, const drc_qpik_params* params, int stages, const IO& call,
                       void* stream) {
  drc_model_impl* m = const_cast<drc_model_impl*>(cm);
  const int64_t B = call.B;
  const double *q = call.q, *qdot = call.qdot;
  if (!m || !params) return set_err(DRC_ERR_INVALID_ARGUMENT, "null model/params");
  std::lock_guard<std::mutex> launch_lock(m->launch_mu);
  if (m->hm.dev.nobst > 0) return set_err(DRC_ERR_UNSUPPORTED, kSlotsUnsupportedMsg);
  if (int rc = check_batch(B)) return rc;
  if (B == 0) return DRC_OK;
  if (int r = check_mode_inputs(call, params->mode, "q, qdot and xdot_target are required", "QPID")) return r;
  if (!stages && (!call.out || !call.out2 || !call.status))
    return set_err(DRC_ERR_INVALID_ARGUMENT, "qddot_out, tau_out and status are required");
  KParams kt, kq;
  int rc = make_kparams(m, params, 1, &kt, 1);
  if (rc) return rc;
  if (!stages) {
    rc = make_kparams(m, params, 0, &kq, 1);
    if (rc) return rc;
  }
  const DevModel& d = m->hm.dev;
  Launch L(m, stream);
  if (int r = L.begin()) return r;
  hipStream_t st = L.st;
  StreamCtx* const cx = L.cx;
  const int64_t stride = record_stride(kt.rLen);
  QpidPool pool;  // (a stage call: nothing)
  if (int r = L.carve(&StreamCtx::pool,
                      [&](void* p) { return qpid_pool(p, stride, kt.na, d.nv, B, stages != 0, d.kind == 1); }, &pool))
    return r;
  if (!stages) {
    // getMassMatrix / getGravity (or the *Actuated getters) the equality rows use
    rc = launch_dynamics(m->d_model, d, d.kind == 1, B, q, qdot, pool.M, nullptr, pool.g, nullptr, nullptr, nullptr, st);
    if (!rc && d.kind == 1)
      rc = launch_dynamics(m->d_model, d, false, B, q, qdot, nullptr, nullptr, pool.g_joint, nullptr, nullptr, nullptr, st);
    if (rc) return set_err(DRC_ERR_HIP, std::string("dynamics launch: ") + hipGetErrorString(hipGetLastError()));
  }
  const int64_t grid = B < 8192 ? B : 8192;
  KParams kt_c = kt, kq_c = kq;
  kt_c.xcd_map = kq_c.xcd_map = xcd_map_for(B);
  IO io = call;
  io.rec = pool.rec;
  io.rec_stride = stride;
  io.dM = pool.M;
  io.dG = pool.g;
  io.dGf = pool.g_joint;
  int* qc = cx->d_queue + StreamCtx::kQueueSlotQpid * StreamCtx::kSlotInts;
  // the task and the QP queue
  HIP_TRY(hipMemsetAsync(qc, 0, (StreamCtx::kSlotQp + StreamCtx::kXcdClasses) * sizeof(int), st));
  io.queue = qc + StreamCtx::kSlotTask;
  const StageIn si{stage_build(d.has_mesh != 0, false, false)};  // (no slots here: the hulls alone decide)
  HIP_TRY(static_cast<hipError_t>(launch_task_kernel(1, static_cast<unsigned>(grid),
                                                     static_cast<size_t>(kt_c.lds_doubles) * sizeof(double), st,
                                                     m->d_model, kt_c, io, si)));
  if (!stages) {
    io.queue = qc + StreamCtx::kSlotQp;
    const size_t lds = static_cast<size_t>(kq_c.lds_doubles) * sizeof(double);
    HIP_TRY(static_cast<hipError_t>(launch_qpid_kernel(static_cast<unsigned>(grid), lds, st, m->d_model, kq_c, io)));
  }
  return L.done();
}

// Closed-form controllers: [dynamics (OSF: M^-1, g)] -> task_kernel<2>.
// (call: cf 1, 2 the targets, cf_null and out; cf 3 the state and st_pose,
// st_jac, st_xdd = xdot)
static int launch_closed_form(const drc_model_impl* cm, const drc_qpik_params* params, int cf, const IO& call,
                              void* stream) {
  drc_model_impl* m = const_cast<drc_model_impl*>(cm);
  const int64_t B = call.B;
  const double *q = call.q, *qdot = call.qdot;
  if (!m || !params) return set_err(DRC_ERR_INVALID_ARGUMENT, "null model/params");
  std::lock_guard<std::mutex> launch_lock(m->launch_mu);
  if (cf != 3 && m->hm.dev.nobst > 0) return set_err(DRC_ERR_UNSUPPORTED, kSlotsUnsupportedMsg);
  if (cf == 3) {  // kinematics only (drc_kinematics_batch): any model kind, no task targets
    if (int rc = check_batch(B)) return rc;
    if (B == 0) return DRC_OK;
    if (!q || (call.st_xdd && !qdot)) return set_err(DRC_ERR_INVALID_ARGUMENT, "q (and qdot for xdot) required");
    KParams kt;
    drc_qpik_params pp = *params;
    pp.mode = DRC_MODE_QPIK;
    int rc = make_kparams(m, &pp, 1, &kt, 2, 3);
    if (rc) return rc;
    Launch L(m, stream);
    if (int r = L.begin()) return r;
    hipStream_t st = L.st;
    StreamCtx* const cx = L.cx;
    const int64_t grid = B < 8192 ? B : 8192;
    kt.xcd_map = xcd_map_for(B);
    // qdot may be NULL when xdot is not requested.  The stage still loads a
    // qdot vector (its J qdot product is then discarded, never stored), so q
    // stands in as a readable buffer of the same shape; with xdot requested
    // the caller's qdot is required (checked above)
    IO io = call;
    if (!qdot) io.qdot = q;
    // fixed assignment when every wave has one instance: no counter reset to enqueue
    io.queue = B > grid ? cx->d_queue + StreamCtx::kQueueSlotCf * StreamCtx::kSlotInts + StreamCtx::kSlotTask : nullptr;
    if (io.queue) HIP_TRY(hipMemsetAsync(io.queue, 0, StreamCtx::kXcdClasses * sizeof(int), st));
    // (no distance stage: hull models run the Plain build too)
    HIP_TRY(static_cast<hipError_t>(launch_task_kernel(2, static_cast<unsigned>(grid),
                                                       static_cast<size_t>(kt.lds_doubles) * sizeof(double), st,
                                                       m->d_model, kt, io, StageIn())));
    return L.done();
  }
  if (m->hm.dev.kind != 0) return set_err(DRC_ERR_INVALID_ARGUMENT, "CLIK / OSF are Manipulator::RobotController entries");
  if (int rc = check_batch(B)) return rc;
  if (B == 0) return DRC_OK;
  if (!q || !qdot || !call.xdt || !call.out)
    return set_err(DRC_ERR_INVALID_ARGUMENT, "q, qdot, xdot_target and out are required");
  if (cf == 1 && params->mode == DRC_MODE_QPIK) return set_err(DRC_ERR_INVALID_ARGUMENT, "CLIK has Step and Cubic forms only");
  if (params->mode != DRC_MODE_QPIK && !call.xt) return set_err(DRC_ERR_INVALID_ARGUMENT, "x_target required");
  if (params->mode == DRC_MODE_QPIK_CUBIC && (!call.xi || !call.xdi))
    return set_err(DRC_ERR_INVALID_ARGUMENT, "x_init/xdot_init required");
  drc_qpik_params pp = *params;
  for (int i = 0; i < 6; ++i) pp.kv[i] = cf == 1 ? 0.0 : params->kv[i];  // CLIK: Kp e + xdot_target (:168)
  pp.feedforward = cf == 1 ? 1.0 : 0.0;                                 // OSF: Kp e + Kv edot (:243)
  KParams kt;
  int rc = make_kparams(m, &pp, 1, &kt, 2, cf);
  if (rc) return rc;
  const DevModel& d = m->hm.dev;
  Launch L(m, stream);
  if (int r = L.begin()) return r;
  hipStream_t st = L.st;
  StreamCtx* const cx = L.cx;
  OsfPool pool{};
  if (cf == 2) {  // getMassMatrixInv (PinvCOD(M)) and getGravity (robot_data.cpp:111-118)
    DynList cod;
    if (int r = L.carve(&StreamCtx::pool, [&](void* p) { return osf_pool(p, d.nv, B); }, &pool)) return r;
    if (int r = L.carve(&StreamCtx::dyn_list, [&](void* p) { return dyn_list(p, B); }, &cod)) return r;
    rc = launch_dynamics(m->d_model, d, false, B, q, qdot, nullptr, pool.Minv, pool.g, nullptr, nullptr, cod.list, st);
    if (rc) return set_err(DRC_ERR_HIP, std::string("dynamics launch: ") + hipGetErrorString(hipGetLastError()));
  }
  const int64_t grid = B < 8192 ? B : 8192;
  kt.xcd_map = xcd_map_for(B);
  IO io = call;
  io.dM = pool.Minv;
  io.dG = pool.g;
  io.queue = cx->d_queue + StreamCtx::kQueueSlotCf * StreamCtx::kSlotInts + StreamCtx::kSlotTask;
  HIP_TRY(hipMemsetAsync(io.queue, 0, StreamCtx::kXcdClasses * sizeof(int), st));
  HIP_TRY(static_cast<hipError_t>(launch_task_kernel(2, static_cast<unsigned>(grid),
                                                     static_cast<size_t>(kt.lds_doubles) * sizeof(double), st,
                                                     m->d_model, kt, io, StageIn())));
  return L.done();
}

}  // namespace drc_amd

using drc_amd::drc_model_impl;
struct drc_model : drc_model_impl {};

extern "C" {

const char* drc_error_string(int code) {
  switch (code) {
    case DRC_OK: return "ok";
    case DRC_ERR_INVALID_ARGUMENT: return "invalid argument";
    case DRC_ERR_FILE: return "file does not exist";
    case DRC_ERR_PARSE: return "parse error";
    case DRC_ERR_UNSUPPORTED: return "unsupported model";
    case DRC_ERR_UNKNOWN_LINK: return "link name not found in URDF";
    case DRC_ERR_HIP: return "HIP runtime error";
    case DRC_ERR_SIZE_MISMATCH: return "size mismatch";
    default: return "unknown error";
  }
}
const char* drc_last_error(void) { return drc_amd::g_last_error.c_str(); }

#ifndef DRC_BUILD_ID
#define DRC_BUILD_ID "unknown"
#endif
const char* drc_build_id(void) { return DRC_BUILD_ID; }

int drc_debug_lds_plan(drc_model* m, const drc_qpik_params* params, int problem, int* task_bytes, int* qp_bytes,
                       int* fused_bytes) {
  if (!m || !params || !task_bytes || !qp_bytes || !fused_bytes) return drc_amd::set_err(DRC_ERR_INVALID_ARGUMENT, "null argument");
  if (problem != 0 && problem != 1) return drc_amd::set_err(DRC_ERR_INVALID_ARGUMENT, "problem must be 0 (QPIK) or 1 (QPID)");
  drc_amd::KParams kt, kq;
  if (int rc = drc_amd::make_kparams(m, params, 1, &kt, problem)) return rc;
  if (int rc = drc_amd::make_kparams(m, params, 0, &kq, problem)) return rc;
  *task_bytes = kt.lds_doubles * 8;
  *qp_bytes = kq.lds_doubles * 8;
  // the fused kernel (QPIK only): the larger plan plus the task record
  *fused_bytes = problem == 0 ? drc_amd::fused_lds_doubles(kt, kq) * 8 : 0;
  return DRC_OK;
}

int drc_debug_waves(drc_model* m, const drc_qpik_params* params, int* task_waves, int* qp_waves) {
  if (!m || !params || !task_waves || !qp_waves) return drc_amd::set_err(DRC_ERR_INVALID_ARGUMENT, "null argument");
  drc_amd::KParams kt;
  if (int rc = drc_amd::make_kparams(m, params, 1, &kt, 0)) return rc;
  *task_waves = drc_amd::task_waves_per_simd(0, static_cast<size_t>(kt.lds_doubles) * 8);
  *qp_waves = drc_amd::qp_waves_per_simd();
  return DRC_OK;
}

int drc_debug_host_timeline(drc_model* m, int enable, int64_t* out, int64_t cap, int64_t* n) {
  if (!m) return drc_amd::set_err(DRC_ERR_INVALID_ARGUMENT, "null model");
  std::lock_guard<std::mutex> g(m->host_mu);
  const int64_t rows = static_cast<int64_t>(m->tl.size() / 5);
  if (n) *n = rows;
  if (out)
    for (int64_t i = 0; i < rows * 5 && i < cap * 5; ++i) out[i] = m->tl[static_cast<size_t>(i)];
  m->tl.clear();
  m->tl_on = enable != 0;
  return DRC_OK;
}

int drc_debug_kernel_timing(drc_model* m, int enable) {
  if (!m) return drc_amd::set_err(DRC_ERR_INVALID_ARGUMENT, "null model");
  m->timing = enable != 0;
  return DRC_OK;
}

int drc_debug_kernel_times(drc_model* m, double* wall_ms, double* task_ms, double* qp_ms, int* calls) {
  if (!m || !wall_ms || !task_ms || !qp_ms || !calls) return drc_amd::set_err(DRC_ERR_INVALID_ARGUMENT, "null argument");
  std::lock_guard<std::mutex> g(m->mu);
  double tw = 0, t0 = 0, t1 = 0;
  for (auto& evs : m->events) {  // {start, end, task start, task end, qp end}, sub-batches
    const std::vector<hipEvent_t>& ev = evs.first;
    float a = 0;
    if (hipEventSynchronize(ev[1]) != hipSuccess) return drc_amd::set_err(DRC_ERR_HIP, "hipEventSynchronize");
    if (hipEventElapsedTime(&a, ev[0], ev[1]) != hipSuccess) return drc_amd::set_err(DRC_ERR_HIP, "hipEventElapsedTime");
    tw += a;
    for (size_t c = 2; c + 2 < ev.size(); c += 3) {
      float x = 0, y = 0;
      if (hipEventElapsedTime(&x, ev[c], ev[c + 1]) != hipSuccess ||
          hipEventElapsedTime(&y, ev[c + 1], ev[c + 2]) != hipSuccess)
        return drc_amd::set_err(DRC_ERR_HIP, "hipEventElapsedTime");
      t0 += x;
      t1 += y;
    }
  }
  *calls = static_cast<int>(m->events.size());
  for (auto& evs : m->events) {  // completed: reusable (each event once: a call's list may name one twice)
    std::vector<hipEvent_t> u = evs.first;
    std::sort(u.begin(), u.end());
    u.erase(std::unique(u.begin(), u.end()), u.end());
    for (hipEvent_t e : u) m->evpool.push_back(e);
  }
  m->events.clear();
  *wall_ms = tw;
  *task_ms = t0;
  *qp_ms = t1;
  return DRC_OK;
}

int drc_set_fusion(drc_model* m, int enable) {
  if (!m) return drc_amd::set_err(DRC_ERR_INVALID_ARGUMENT, "null model");
  std::lock_guard<std::mutex> g(m->launch_mu);
  m->fused = enable != 0;
  return DRC_OK;
}

int drc_set_concurrency(drc_model* m, int chunks) {
  if (!m || chunks < 1 || chunks > 16) return drc_amd::set_err(DRC_ERR_INVALID_ARGUMENT, "chunks must be 1..16");
  std::lock_guard<std::mutex> g(m->mu);
  m->chunks = chunks;
  return DRC_OK;
}

int drc_debug_lane_stage(drc_model* m, int enable) {
  if (!m) return drc_amd::set_err(DRC_ERR_INVALID_ARGUMENT, "null model");
  if (enable && m->hm.has_mesh()) return drc_amd::set_err(DRC_ERR_UNSUPPORTED, drc_amd::kMeshStageMsg);
  std::lock_guard<std::mutex> g(m->launch_mu);
  if (m->hm.dev.nobst > 0) return drc_amd::set_err(DRC_ERR_UNSUPPORTED, drc_amd::kSlotsUnsupportedMsg);
  m->lane_stage = enable < 0 ? 0 : (enable > 3 ? 3 : enable);
  return DRC_OK;
}

int drc_debug_instance_order(drc_model* m, const int32_t* order, int64_t n) {
  using drc_amd::set_err;
  if (!m) return set_err(DRC_ERR_INVALID_ARGUMENT, "null model");
  std::lock_guard<std::mutex> g(m->launch_mu);
  HIP_TRY(hipSetDevice(m->device));
  if (m->d_order) {
    HIP_TRY(hipDeviceSynchronize());  // calls in flight may still read it
    HIP_TRY(hipFree(m->d_order));
  }
  m->d_order = nullptr;
  m->order_n = 0;
  if (!order || n <= 0) return DRC_OK;
  std::vector<char> seen(n, 0);
  for (int64_t i = 0; i < n; ++i) {
    if (order[i] < 0 || order[i] >= n || seen[order[i]]) return drc_amd::set_err(DRC_ERR_INVALID_ARGUMENT, "not a permutation");
    seen[order[i]] = 1;
  }
  HIP_TRY(hipMalloc(&m->d_order, n * sizeof(int32_t)));
  HIP_TRY(hipMemcpy(m->d_order, order, n * sizeof(int32_t), hipMemcpyHostToDevice));
  m->order_n = n;
  return DRC_OK;
}

#ifdef DRC_PHASE_TIMING
// diagnostic build only: accumulated per-phase s_memtime cycles, slots 0 .. 63
static int phase_cycles_all(unsigned long long* all, int reset) {
  for (int i = 0; i < 96; ++i) all[i] = 0;
  if (drc_amd::phase_cycles_task(all, reset) || drc_amd::phase_cycles_qp(all, reset) ||
      drc_amd::phase_cycles_qp_dense(all, reset) ||
      drc_amd::phase_cycles_qpid(all, reset) || drc_amd::phase_cycles_fused(all, reset))
    return DRC_ERR_HIP;
  return DRC_OK;
}
int drc_debug_phase_cycles(unsigned long long* out, int reset) {
  unsigned long long all[96];
  if (int rc = phase_cycles_all(all, reset)) return rc;
  for (int i = 0; i < 64; ++i) out[i] = all[i];
  return DRC_OK;
}
// ... and slots 64 .. 95 into out[32]: the QP kernel's front end split finer
// (Ruiz scaling: checks, V load, passes, write-back; schur_setup: weights, S
// entries, Gauss-Jordan, G_c S^-1; qp_assemble after the record load: J~ and
// P, G / q / bounds).  Never resets: drc_debug_phase_cycles does.
int drc_debug_phase_cycles_fine(unsigned long long* out) {
  unsigned long long all[96];
  if (int rc = phase_cycles_all(all, 0)) return rc;
  for (int i = 0; i < 32; ++i) out[i] = all[64 + i];
  return DRC_OK;
}
// diagnostic build only: polish EQPs by reduced-KKT size N (bins 0 .. 14, then N >= 15)
int drc_debug_eqp_hist(unsigned long long* out, int reset) {
  for (int i = 0; i < 16; ++i) out[i] = 0;
  if (drc_amd::phase_cycles_qp_hist(out, reset) || drc_amd::phase_cycles_qp_dense_hist(out, reset) ||
      drc_amd::phase_cycles_fused_hist(out, reset))
    return DRC_ERR_HIP;
  return DRC_OK;
}
#endif

int drc_debug_eqp_small_cap(drc_model* m, int cap) {
  if (!m) return drc_amd::set_err(DRC_ERR_INVALID_ARGUMENT, "null model");
  std::lock_guard<std::mutex> g(m->launch_mu);
  m->eqp_small_cap = cap < 0 ? -1 : cap;
  return DRC_OK;
}

int drc_debug_task_plan_wide(drc_model* m, int on) {
  if (!m) return drc_amd::set_err(DRC_ERR_INVALID_ARGUMENT, "null model");
  std::lock_guard<std::mutex> g(m->launch_mu);
  m->task_plan_wide = on != 0;
  return DRC_OK;
}

int drc_debug_qp_dense(drc_model* m, int on) {
  if (!m) return drc_amd::set_err(DRC_ERR_INVALID_ARGUMENT, "null model");
  std::lock_guard<std::mutex> g(m->launch_mu);
  m->qp_dense = on != 0;
  return DRC_OK;
}

int drc_debug_clearance_grid(drc_model* m, int64_t* grid) {
  if (!m || !grid) return drc_amd::set_err(DRC_ERR_INVALID_ARGUMENT, "null argument");
  std::lock_guard<std::mutex> launch_lock(m->launch_mu);
  *grid = m->clearance_grid_last;
  return DRC_OK;
}

int drc_debug_qp_dense_launches(drc_model* m, int64_t* count) {
  if (!m || !count) return drc_amd::set_err(DRC_ERR_INVALID_ARGUMENT, "null argument");
  std::lock_guard<std::mutex> g(m->launch_mu);
  *count = m->qp_dense_launches;
  return DRC_OK;
}

int drc_model_create_manipulator(const char* urdf, const char* srdf, const char* packages, int device,
                                 drc_model** out) {
  if (!urdf || !out) return drc_amd::set_err(DRC_ERR_INVALID_ARGUMENT, "null argument");
  auto* m = new drc_model();
  std::string err;
  int rc = drc_amd::build_model_from_urdf(urdf, srdf ? srdf : "", packages ? packages : "", &m->hm, &err);
  if (rc) {
    delete m;
    return drc_amd::set_err(rc, err);
  }
  m->hm.dev.kind = 0;
  m->device = device;
  rc = drc_amd::upload(m);
  if (rc) {
    delete m;
    return rc;
  }
  *out = m;
  return DRC_OK;
}

int drc_model_create_mobile_manipulator(const drc_kinematic_param* param, const drc_joint_index* ji,
                                        const drc_actuator_index* ai, const char* urdf, const char* srdf,
                                        const char* packages, int device, drc_model** out) {
  if (!param || !ji || !ai || !urdf || !out) return drc_amd::set_err(DRC_ERR_INVALID_ARGUMENT, "null argument");
  auto* m = new drc_model();
  std::string err;
  int rc = drc_amd::build_model_from_urdf(urdf, srdf ? srdf : "", packages ? packages : "", &m->hm, &err);
  if (rc) {
    delete m;
    return drc_amd::set_err(rc, err);
  }
  drc_amd::DevModel& d = m->hm.dev;
  int W = 0;
  rc = drc_amd::mobile_fk_jacobian(*param, &W, d.J_mobile);
  if (rc) {
    delete m;
    return rc;
  }
  d.drive = param->type;
  d.wheel_radius = param->wheel_radius;
  d.wheel_offset = param->wheel_offset;
  for (int i = 0; i < drc_amd::kMaxWheels / 2; ++i)
    for (int k = 0; k < 2; ++k) d.caster_pos[i][k] = param->base2wheel_positions[i][k];
  if (param->type == DRC_DRIVE_CASTER && !(param->wheel_offset != 0)) {
    delete m;
    return drc_amd::set_err(DRC_ERR_INVALID_ARGUMENT, "caster drive needs a nonzero wheel_offset");
  }
  // MobileManipulator::RobotData ctor (mobile_manipulator/robot_data.cpp:18-25)
  const int virtual_dof = 3;
  d.kind = 1;
  d.n_wheel = W;
  d.n_arm = d.nv - (virtual_dof + W);  // every joint 1-DoF, no extra joints
  d.virtual_start = ji->virtual_start;
  d.mani_start = ji->mani_start;
  d.mobi_start = ji->mobi_start;
  d.act_mani_start = ai->mani_start;
  d.act_mobi_start = ai->mobi_start;
  d.dyn_origin = ji->virtual_start + 3;  // the base (yaw joint) origin: keeps spatial moments small
  if (d.n_arm < 1 || d.n_arm > 8 || ji->virtual_start + 3 > d.nv || ji->mani_start + d.n_arm > d.nv ||
      ji->mobi_start + W > d.nv || ai->mani_start + d.n_arm > d.n_arm + W || ai->mobi_start + W > d.n_arm + W) {
    delete m;
    return drc_amd::set_err(DRC_ERR_INVALID_ARGUMENT, "JointIndex/ActuatorIndex inconsistent with the URDF dof");
  }
  m->kparam = *param;
  m->jidx = *ji;
  m->aidx = *ai;
  m->device = device;
  rc = drc_amd::upload(m);
  if (rc) {
    delete m;
    return rc;
  }
  *out = m;
  return DRC_OK;
}

int drc_model_release_stream(drc_model* m, void* stream) {
  using drc_amd::set_err;
  if (!m) return drc_amd::set_err(DRC_ERR_INVALID_ARGUMENT, "null model");
  std::lock_guard<std::mutex> launch_lock(m->launch_mu);
  std::lock_guard<std::mutex> g(m->mu);
  HIP_TRY(hipSetDevice(m->device));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  for (size_t i = 0; i < m->ctxs.size(); ++i)
    if (m->ctxs[i]->stream == st) {
      HIP_TRY(hipStreamSynchronize(st));  // the stream is still valid: its work on the context drains first
      drc_amd::free_ctx(m->ctxs[i].get());
      m->ctxs.erase(m->ctxs.begin() + static_cast<std::ptrdiff_t>(i));
      break;
    }
  return DRC_OK;
}

void drc_model_destroy(drc_model* m) {
  if (!m) return;
  (void)hipSetDevice(m->device);
  (void)hipDeviceSynchronize();
  for (auto& c : m->ctxs) drc_amd::free_ctx(c.get());
  drc_amd::free_lanes(&m->ln);
  if (m->d_model) (void)hipFree(m->d_model);
  if (m->d_mesh) (void)hipFree(m->d_mesh);
  if (m->d_pair_tab) (void)hipFree(m->d_pair_tab);
  if (m->d_motion_wt) (void)hipFree(m->d_motion_wt);
  if (m->d_order) (void)hipFree(m->d_order);
  if (m->hstream) (void)hipStreamSynchronize(m->hstream), (void)hipStreamDestroy(m->hstream);
  if (m->stage) (void)hipFree(m->stage);
  if (m->pinned) (void)hipHostFree(m->pinned);
  if (m->hdone) (void)hipEventDestroy(m->hdone);
  for (auto& evs : m->events) {
    std::vector<hipEvent_t> u = evs.first;
    std::sort(u.begin(), u.end());
    u.erase(std::unique(u.begin(), u.end()), u.end());
    for (hipEvent_t e : u) (void)hipEventDestroy(e);
  }
  for (hipEvent_t e : m->evpool) (void)hipEventDestroy(e);
  delete m;
}

int drc_model_info(const drc_model* m, int* dof, int* act, int* mani, int* mobi, int* ngeom, int* npairs) {
  if (!m) return drc_amd::set_err(DRC_ERR_INVALID_ARGUMENT, "null model");
  const drc_amd::DevModel& d = m->hm.dev;
  if (dof) *dof = d.nv;
  if (act) *act = drc_amd::actuated_width(d);
  if (mani) *mani = drc_amd::arm_width(d);
  if (mobi) *mobi = d.kind == 1 ? d.n_wheel : 0;
  if (ngeom) *ngeom = d.ngeom;
  if (npairs) *npairs = d.npairs;
  return DRC_OK;
}

int drc_model_geom_info(const drc_model* m, int geom, int* type, double param[3], int* n_vertices,
                        double* hull_residual) {
  if (!m) return drc_amd::set_err(DRC_ERR_INVALID_ARGUMENT, "null model");
  const drc_amd::DevModel& d = m->hm.dev;
  if (geom < 0 || geom >= d.ngeom) return drc_amd::set_err(DRC_ERR_INVALID_ARGUMENT, "geometry index out of range");
  if (type) *type = d.gtype[geom];
  if (param)
    for (int i = 0; i < 3; ++i) param[i] = d.gparam[geom][i];
  const bool urdf_geom = geom < static_cast<int>(m->hm.mesh_count.size());  // (obstacle slots: primitives)
  if (n_vertices) *n_vertices = urdf_geom ? m->hm.mesh_count[geom] : 0;
  if (hull_residual) *hull_residual = urdf_geom ? m->hm.mesh_residual[geom] : 0.0;
  return DRC_OK;
}

int drc_model_motion_weights(const drc_model* m, double* rho, double* wt, uint32_t* travel_mask) {
  if (!m) return drc_amd::set_err(DRC_ERR_INVALID_ARGUMENT, "null model");
  const drc_amd::DevModel& d = m->hm.dev;
  if (rho)
    for (int i = 0; i < d.nv * d.ngeom; ++i) rho[i] = m->hm.motion_rho[i];
  if (wt)
    for (int j = 0; j < d.nv; ++j)
      for (int p = 0; p < d.npairs; ++p)
        wt[static_cast<size_t>(j) * d.npairs + p] = m->hm.motion_wt[static_cast<size_t>(j) * d.motion_ld + p];
  if (travel_mask) *travel_mask = d.travel_mask;
  return DRC_OK;
}

int drc_mesh_convex_hull(const char* path, const double scale[3], int max_vertices, double* verts_out, int cap,
                         int* n_out, double* residual_out) {
  if (!path || !n_out) return drc_amd::set_err(DRC_ERR_INVALID_ARGUMENT, "null argument");
  *n_out = 0;
  drc_amd::MeshHull hull;
  std::string err;
  const int rc = drc_amd::mesh_convex_hull(path, scale, max_vertices > 0 ? max_vertices : drc_amd::kMaxMeshVerts,
                                           &hull, &err);
  if (rc) return drc_amd::set_err(rc, err);
  const int n = static_cast<int>(hull.verts.size());
  *n_out = n;
  if (residual_out) *residual_out = hull.residual;
  if (n > cap || (n > 0 && !verts_out))
    return drc_amd::set_err(DRC_ERR_SIZE_MISMATCH, "verts_out holds " + std::to_string(cap < 0 ? 0 : cap) +
                                                       " vertices, the hull has " + std::to_string(n));
  for (int i = 0; i < n; ++i)
    for (int k = 0; k < 3; ++k) verts_out[3 * i + k] = hull.verts[i][k];
  return DRC_OK;
}

int drc_model_limits(const drc_model* m, double* q_lb, double* q_ub, double* qd_lb, double* qd_ub) {
  if (!m) return drc_amd::set_err(DRC_ERR_INVALID_ARGUMENT, "null model");
  const drc_amd::DevModel& d = m->hm.dev;
  for (int i = 0; i < d.nv; ++i) {
    if (q_lb) q_lb[i] = d.lower[i];
    if (q_ub) q_ub[i] = d.upper[i];
    if (qd_lb) qd_lb[i] = -d.vel[i];
    if (qd_ub) qd_ub[i] = d.vel[i];
  }
  return DRC_OK;
}

int drc_model_find_frame(const drc_model* m, const char* name, int* id) {
  if (!m || !name || !id) return drc_amd::set_err(DRC_ERR_INVALID_ARGUMENT, "null argument");
  const auto& names = m->hm.frame_names;
  for (size_t i = 0; i < names.size(); ++i)
    if (names[i] == name) {
      *id = static_cast<int>(i);
      return DRC_OK;
    }
  *id = -1;
  return drc_amd::set_err(DRC_ERR_UNKNOWN_LINK, std::string("Link name ") + name + " not found in URDF.");
}

int drc_model_mobile_fk_jacobian(const drc_model* m, double* J) {
  if (!m || !J) return drc_amd::set_err(DRC_ERR_INVALID_ARGUMENT, "null argument");
  const drc_amd::DevModel& d = m->hm.dev;
  if (d.kind != 1) return drc_amd::set_err(DRC_ERR_INVALID_ARGUMENT, "not a mobile manipulator");
  if (d.drive == drc_amd::kDriveCaster)
    return drc_amd::set_err(DRC_ERR_INVALID_ARGUMENT,
                            "caster drive: J_mobile depends on the steer angles (drc_mobile_fk_jacobian)");
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < d.n_wheel; ++c) J[r * d.n_wheel + c] = d.J_mobile[r][c];
  return DRC_OK;
}

int drc_mobile_fk_jacobian(const drc_kinematic_param* p, const double* wheel_pos, double* J, int* n_wheels) {
  if (!p || !J || !n_wheels) return drc_amd::set_err(DRC_ERR_INVALID_ARGUMENT, "null argument");
  if (p->type == DRC_DRIVE_CASTER && !wheel_pos)
    return drc_amd::set_err(DRC_ERR_INVALID_ARGUMENT, "caster drive: wheel positions required");
  double Jm[3][drc_amd::kMaxWheels];
  int W = 0;
  if (int rc = drc_amd::mobile_fk_jacobian(*p, &W, Jm, wheel_pos)) return rc;
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < W; ++c) J[r * W + c] = Jm[r][c];
  *n_wheels = W;
  return DRC_OK;
}

int drc_mobile_ik_jacobian(const drc_kinematic_param* p, const double* wheel_pos, double* J, int* n_wheels) {
  if (!p || !J || !n_wheels) return drc_amd::set_err(DRC_ERR_INVALID_ARGUMENT, "null argument");
  if (p->type == DRC_DRIVE_CASTER && !wheel_pos)
    return drc_amd::set_err(DRC_ERR_INVALID_ARGUMENT, "caster drive: wheel positions required");
  return drc_amd::mobile_ik_jacobian(*p, wheel_pos, J, n_wheels);
}

int drc_default_qpik_params(const drc_model* m, int exact, drc_qpik_params* p) {
  if (!m || !p) return drc_amd::set_err(DRC_ERR_INVALID_ARGUMENT, "null argument");
  std::memset(p, 0, sizeof(*p));
  const bool moma = m->hm.dev.kind == 1;
  for (int i = 0; i < 6; ++i) {
    p->kp[i] = moma ? 400 : 100;  // robot_controller.cpp:12 ; MoMa :15
    p->kv[i] = moma ? 0 : 20;     // MoMa QPIKStep: Kp*e + xdot_target (:177)
  }
  p->feedforward = moma ? 1.0 : 0.0;
  p->alpha_cbf = 50;
  p->w_reg = moma ? 0.01 : 1.0;
  p->slack_w = 1000;
  p->man_min = 0.01;
  p->dist_min = 0.05;
  p->mode = DRC_MODE_QPIK_STEP;
  p->frame_id = -1;
  drc_solver_settings& s = p->solver;
  s.rho = 0.1;
  s.sigma = 1e-6;
  s.alpha = 1.6;
  s.eps_abs = 1e-3;
  s.eps_rel = 1e-3;
  s.eps_prim_inf = 1e-4;
  s.max_iter = 4000;
  s.check_termination = 25;
  s.scaling = 10;
  s.adaptive_rho = 1;
  s.adaptive_rho_interval = 25;
  s.adaptive_rho_tolerance = 5;
  s.polish = exact ? 1 : 0;
  s.polish_refine_iter = 3;
  s.delta = 1e-6;
  s.exact = exact ? 1 : 0;
  s.eps_exact = 1e-9;
  s.eps_fallback = 1e-7;
  // exact mode: the ADMM iterate only seeds the certified polish's first
  // active-set guess, so how often it is tried is a speed choice.  With the
  // projected-Jacobi guess the first polish paid off at iteration 20 (+1-2.5 %
  // against 25, profiles/r05h_envab_check20.jsonl); with the infeasible-phase
  // drop rule it pays off far earlier: manipulators at 8 (FR3 +7 %, UR5e +4 %;
  // below 8 UR5e loses), the whole-body QPs at 2 (XLS-FR3 +12 %, Husky-FR3
  // +6 %; profiles/r05ae-ag_envab_check*.jsonl).  The oracle's exact mode uses
  // the same intervals.  DRC_EXACT_CHECK overrides both (A/B experiments)
  static const int64_t exact_check_env = drc_amd::env_int("DRC_EXACT_CHECK", 0, 0);
  const int64_t exact_check = exact_check_env > 0 ? exact_check_env : (moma ? 2 : 8);
  // OSQP's 3 refinement steps.  2 certify the same attempts at eps_exact
  // (tools/polish_census.py --refine; 1 fails half) and measured UR5e +1.1 %,
  // FR3 +0.1 % (profiles/r05b_envab.jsonl), but leave ~2e-9 in q-dot on some
  // instances (a golden fixture moved by 2.5e-9): not taken for that
  static const int64_t exact_refine = drc_amd::env_int("DRC_EXACT_REFINE", 3, 0);
  // Ruiz passes in exact mode: 1 (manipulators) / 2 (whole-body) instead of
  // OSQP's 10.  The ADMM only seeds the certified polish there (8 / 2
  // iterations), and the certified point is the QP's unique optimum whatever
  // the scaling; a pass or two equilibrate enough for the polish to certify at
  // its first attempt, the rest cost (whole-body QPs run all 10: a balanced
  // row's factor converges geometrically and never reaches exactly 1).
  // Measured, one box, 2 against 10: FR3 +2.6 %, UR5e +2.1 %, Husky-FR3
  // +2.9 %, XLS-FR3 +9.9 %, Caster-FR3 +10.5 %; one pass leaves the whole-body
  // polish failing (3.6 M solves/s), none fails everywhere
  // (profiles/r06f_envab_exact_scaling.jsonl, r06g_envab_exact_scaling.jsonl);
  // 1 against 2 on the manipulators: FR3 +0.6 %, UR5e +1.8 %, FR3 B = 4 096
  // +1.2 % (profiles/r06al_envab_scal1*.jsonl).  The oracle's exact mode uses
  // the same counts.  DRC_EXACT_SCALING overrides both kinds (A/B experiments)
  static const int64_t exact_scaling_env = drc_amd::env_int("DRC_EXACT_SCALING", 0, 0);
  const int64_t exact_scaling = exact_scaling_env > 0 ? exact_scaling_env : (moma ? 2 : 1);
  if (exact) {
    s.check_termination = static_cast<int>(exact_check);
    s.polish_refine_iter = static_cast<int>(exact_refine);
    s.scaling = static_cast<int>(exact_scaling);
  }
  return DRC_OK;
}

int drc_qpik_batch(const drc_model* m, const drc_qpik_params* p, int64_t B, const double* q, const double* qdot,
                   const double* xt, const double* xdt, const double* xi, const double* xdi, double* out,
                   int32_t* status, int32_t* iters, void* stream) {
  drc_amd::IO io = drc_amd::task_io(B, q, qdot, xt, xdt, xi, xdi);
  io.out = out;
  io.status = status;
  io.iters = iters;
  return drc_amd::launch(m, p, 0, io, stream);
}

int drc_qpik_rollout_batch(const drc_model* m, const drc_qpik_params* p, int64_t B, int steps, double dt,
                           const double* q0, const double* qdot0, const double* xt, const double* xdt,
                           const double* xi, const double* xdi, int targets_per_step, double* q_final,
                           double* qdot_final, double* qdot_traj, int32_t* status_traj, int32_t* iters_traj,
                           double* q_traj, double* pose_traj, double* dist_traj, void* stream) {
  return drc_amd::rollout(m, p, B, steps, dt, q0, qdot0, xt, xdt, xi, xdi, targets_per_step, q_final, qdot_final,
                          qdot_traj, status_traj, iters_traj, q_traj, pose_traj, dist_traj, stream);
}

int drc_qpik_stages_batch(const drc_model* m, const drc_qpik_params* p, int64_t B, const double* q,
                          const double* qdot, const double* xt, const double* xdt, const double* xi,
                          const double* xdi, double* pose, double* jac, double* man, double* dist, int32_t* pair,
                          double* xdd, void* stream) {
  drc_amd::IO io = drc_amd::task_io(B, q, qdot, xt, xdt, xi, xdi);
  io.st_pose = pose;
  io.st_jac = jac;
  io.st_man = man;
  io.st_dist = dist;
  io.st_pair = pair;
  io.st_xdd = xdd;
  return drc_amd::launch(m, p, 1, io, stream);
}

// ---- obstacle slots ------------------------------------------------------------
int drc_model_set_obstacles(drc_model* m, int n, const int* type, const double* param, const char* const* links,
                            int n_links) {
  using drc_amd::set_err;
  if (!m) return set_err(DRC_ERR_INVALID_ARGUMENT, "null model");
  std::lock_guard<std::mutex> launch_lock(m->launch_mu);
  std::string err;
  drc_amd::HostModel hm = m->hm;  // built aside: a refused call leaves the model as it was
  if (int rc = drc_amd::set_obstacles(&hm, n, type, param, links, n_links, &err)) return set_err(rc, err);
  HIP_TRY(hipSetDevice(m->device));
  // the model's outstanding work (every stream that ran it) reads the old tables
  HIP_TRY(hipDeviceSynchronize());
  const drc_amd::HostModel old = m->hm;
  m->hm = hm;
  drc_qpik_params pp;
  int rc = drc_default_qpik_params(m, 1, &pp);
  if (!rc) {  // the task stage's LDS plan with the new geometry and pair counts
    drc_amd::KParams kt;
    pp.frame_id = -1;
    rc = drc_amd::make_kparams(m, &pp, 1, &kt);
  }
  if (rc) {
    m->hm = old;
    return rc;
  }
  return drc_amd::upload(m);
}

int drc_qpik_obstacles_batch(const drc_model* m, const drc_qpik_params* p, int64_t B, const double* q,
                             const double* qdot, const double* xt, const double* xdt, const double* xi,
                             const double* xdi, const double* obstacle_pose, int64_t obstacle_ld, double* out,
                             int32_t* status, int32_t* iters, void* stream) {
  return drc_qpik_moving_obstacles_batch(m, p, B, q, qdot, xt, xdt, xi, xdi, obstacle_pose, nullptr, obstacle_ld, out,
                                         status, iters, stream);
}

int drc_qpik_stages_obstacles_batch(const drc_model* m, const drc_qpik_params* p, int64_t B, const double* q,
                                    const double* qdot, const double* xt, const double* xdt, const double* xi,
                                    const double* xdi, const double* obstacle_pose, int64_t obstacle_ld,
                                    double* pose, double* jac, double* man, double* dist, int32_t* pair, double* xdd,
                                    void* stream) {
  return drc_qpik_stages_moving_obstacles_batch(m, p, B, q, qdot, xt, xdt, xi, xdi, obstacle_pose, nullptr, obstacle_ld,
                                                pose, jac, man, dist, pair, xdd, nullptr, stream);
}

int drc_qpik_rollout_obstacles_batch(const drc_model* m, const drc_qpik_params* p, int64_t B, int steps, double dt,
                                     const double* q0, const double* qdot0, const double* xt, const double* xdt,
                                     const double* xi, const double* xdi, int targets_per_step,
                                     const double* obstacle_pose, int64_t obstacle_ld, int obstacles_per_step,
                                     double* q_final, double* qdot_final, double* qdot_traj, int32_t* status_traj,
                                     int32_t* iters_traj, double* q_traj, double* pose_traj, double* dist_traj,
                                     void* stream) {
  return drc_qpik_rollout_moving_obstacles_batch(m, p, B, steps, dt, q0, qdot0, xt, xdt, xi, xdi, targets_per_step,
                                                 obstacle_pose, nullptr, obstacle_ld, obstacles_per_step, q_final,
                                                 qdot_final, qdot_traj, status_traj, iters_traj, q_traj, pose_traj,
                                                 dist_traj, stream);
}

// ---- moving obstacles: a twist per slot (task_stage.hpp RATE) ------------------------
// obstacle_twist = NULL: the obstacle entry itself
int drc_qpik_moving_obstacles_batch(const drc_model* m, const drc_qpik_params* p, int64_t B, const double* q,
                                    const double* qdot, const double* xt, const double* xdt, const double* xi,
                                    const double* xdi, const double* obstacle_pose, const double* obstacle_twist,
                                    int64_t obstacle_ld, double* out, int32_t* status, int32_t* iters, void* stream) {
  drc_amd::IO io = drc_amd::task_io(B, q, qdot, xt, xdt, xi, xdi);
  io.out = out;
  io.status = status;
  io.iters = iters;
  return drc_amd::launch(m, p, 0, io, stream, drc_amd::stage_in(obstacle_pose, obstacle_ld, obstacle_twist));
}

int drc_qpik_stages_moving_obstacles_batch(const drc_model* m, const drc_qpik_params* p, int64_t B, const double* q,
                                           const double* qdot, const double* xt, const double* xdt, const double* xi,
                                           const double* xdi, const double* obstacle_pose,
                                           const double* obstacle_twist, int64_t obstacle_ld, double* pose, double* jac,
                                           double* man, double* dist, int32_t* pair, double* xdd, double* dist_rate,
                                           void* stream) {
  drc_amd::IO io = drc_amd::task_io(B, q, qdot, xt, xdt, xi, xdi);
  io.st_pose = pose;
  io.st_jac = jac;
  io.st_man = man;
  io.st_dist = dist;
  io.st_pair = pair;
  io.st_xdd = xdd;
  if (int rc = drc_amd::launch(m, p, 1, io, stream,
                               drc_amd::stage_in(obstacle_pose, obstacle_ld, obstacle_twist, dist_rate)))
    return rc;
  if (!obstacle_twist && dist_rate && B > 0) {  // no twist: nothing but the robot moves
    using drc_amd::set_err;
    HIP_TRY(hipSetDevice(m->device));
    HIP_TRY(hipMemsetAsync(dist_rate, 0, size_t(B) * 8, reinterpret_cast<hipStream_t>(stream)));
  }
  return DRC_OK;
}

int drc_qpik_rollout_moving_obstacles_batch(const drc_model* m, const drc_qpik_params* p, int64_t B, int steps,
                                            double dt, const double* q0, const double* qdot0, const double* xt,
                                            const double* xdt, const double* xi, const double* xdi,
                                            int targets_per_step, const double* obstacle_pose,
                                            const double* obstacle_twist, int64_t obstacle_ld, int obstacles_per_step,
                                            double* q_final, double* qdot_final, double* qdot_traj,
                                            int32_t* status_traj, int32_t* iters_traj, double* q_traj,
                                            double* pose_traj, double* dist_traj, void* stream) {
  return drc_amd::rollout(m, p, B, steps, dt, q0, qdot0, xt, xdt, xi, xdi, targets_per_step, q_final, qdot_final,
                          qdot_traj, status_traj, iters_traj, q_traj, pose_traj, dist_traj, stream,
                          drc_amd::stage_in(obstacle_pose, obstacle_ld, obstacle_twist), obstacles_per_step);
}

// ---- goal-reaching rollouts ------------------------------------------------------
int drc_qpik_reach_batch(const drc_model* m, const drc_qpik_params* p, int64_t B, int max_steps, double dt,
                         double pos_tol, double rot_tol, const double* q0, const double* qdot0, const double* xt,
                         const double* xdt, double* q_final, double* qdot_final, int32_t* result,
                         int32_t* steps_used, int32_t* status_last, int32_t* iters_total, double* err_final,
                         double* dist_final, void* stream) {
  return drc_amd::reach(m, p, B, max_steps, dt, pos_tol, rot_tol, q0, qdot0, xt, xdt, q_final, qdot_final, result,
                        steps_used, status_last, iters_total, err_final, dist_final, stream);
}

int drc_qpik_reach_obstacles_batch(const drc_model* m, const drc_qpik_params* p, int64_t B, int max_steps, double dt,
                                   double pos_tol, double rot_tol, const double* q0, const double* qdot0,
                                   const double* xt, const double* xdt, const double* obstacle_pose,
                                   int64_t obstacle_ld, double* q_final, double* qdot_final, int32_t* result,
                                   int32_t* steps_used, int32_t* status_last, int32_t* iters_total,
                                   double* err_final, double* dist_final, void* stream) {
  return drc_amd::reach(m, p, B, max_steps, dt, pos_tol, rot_tol, q0, qdot0, xt, xdt, q_final, qdot_final, result,
                        steps_used, status_last, iters_total, err_final, dist_final, stream,
                        drc_amd::stage_in(obstacle_pose, obstacle_ld));
}

int drc_qpik_reach_path_batch(const drc_model* m, const drc_qpik_params* p, int64_t B, int waypoints, int max_steps,
                              double dt, double pos_tol, double rot_tol, const double* q0, const double* qdot0,
                              const double* x_path, const double* xdot_path, double* q_final, double* qdot_final,
                              int32_t* result, int32_t* waypoints_reached, int32_t* steps_used, int32_t* status_last,
                              int32_t* iters_total, double* err_final, double* dist_final, double* dist_min,
                              int32_t* steps_at, void* stream) {
  return drc_amd::reach_path(m, p, B, waypoints, max_steps, dt, pos_tol, rot_tol, q0, qdot0, x_path, xdot_path,
                             q_final, qdot_final, result, waypoints_reached, steps_used, status_last, iters_total,
                             err_final, dist_final, dist_min, steps_at, stream);
}

int drc_qpik_reach_path_obstacles_batch(const drc_model* m, const drc_qpik_params* p, int64_t B, int waypoints,
                                        int max_steps, double dt, double pos_tol, double rot_tol, const double* q0,
                                        const double* qdot0, const double* x_path, const double* xdot_path,
                                        const double* obstacle_pose, int64_t obstacle_ld, double* q_final,
                                        double* qdot_final, int32_t* result, int32_t* waypoints_reached,
                                        int32_t* steps_used, int32_t* status_last, int32_t* iters_total,
                                        double* err_final, double* dist_final, double* dist_min, int32_t* steps_at,
                                        void* stream) {
  return drc_amd::reach_path(m, p, B, waypoints, max_steps, dt, pos_tol, rot_tol, q0, qdot0, x_path, xdot_path,
                             q_final, qdot_final, result, waypoints_reached, steps_used, status_last, iters_total,
                             err_final, dist_final, dist_min, steps_at, stream,
                             drc_amd::stage_in(obstacle_pose, obstacle_ld));
}

int drc_qpik_reach_seeds_batch(const drc_model* m, const drc_qpik_params* p, int64_t targets, int seeds, int rule,
                               int cancel, int max_steps, double dt, double pos_tol, double rot_tol, const double* q0,
                               const double* qdot0, const double* xt, const double* xdt, int32_t* seed,
                               int32_t* result, int32_t* steps_used, double* q_sol, double* qdot_sol,
                               int32_t* status_last, int32_t* iters_total, double* err_final, double* dist_final,
                               int32_t* inst_result, int32_t* inst_steps, void* stream) {
  return drc_amd::reach_seeds(m, p, targets, seeds, rule, cancel, max_steps, dt, pos_tol, rot_tol, q0, qdot0, xt, xdt,
                              seed, result, steps_used, q_sol, qdot_sol, status_last, iters_total, err_final,
                              dist_final, inst_result, inst_steps, stream);
}

int drc_qpik_reach_seeds_obstacles_batch(const drc_model* m, const drc_qpik_params* p, int64_t targets, int seeds,
                                         int rule, int cancel, int max_steps, double dt, double pos_tol,
                                         double rot_tol, const double* q0, const double* qdot0, const double* xt,
                                         const double* xdt, const double* obstacle_pose, int64_t obstacle_ld,
                                         int32_t* seed, int32_t* result, int32_t* steps_used, double* q_sol,
                                         double* qdot_sol, int32_t* status_last, int32_t* iters_total,
                                         double* err_final, double* dist_final, int32_t* inst_result,
                                         int32_t* inst_steps, void* stream) {
  return drc_amd::reach_seeds(m, p, targets, seeds, rule, cancel, max_steps, dt, pos_tol, rot_tol, q0, qdot0, xt, xdt,
                              seed, result, steps_used, q_sol, qdot_sol, status_last, iters_total, err_final,
                              dist_final, inst_result, inst_steps, stream, drc_amd::stage_in(obstacle_pose, obstacle_ld));
}

int drc_reach_thresholds(double pos_tol, double rot_tol, double out[2]) {
  using drc_amd::set_err;
  if (!out) return set_err(DRC_ERR_INVALID_ARGUMENT, "out is required");
  if (!drc_amd::finite_positive(pos_tol) || !drc_amd::finite_positive(rot_tol))
    return set_err(DRC_ERR_INVALID_ARGUMENT, "pos_tol and rot_tol must be finite and positive");
  drc_amd::reach_thresholds(pos_tol, rot_tol, out);
  return DRC_OK;
}

// ---- path clearance ------------------------------------------------------------
// (the distance stage reads no drc_qpik_params field: the defaults size its plan)
static int clearance_params(const drc_model* m, drc_qpik_params* pp) {
  if (!m) return drc_amd::set_err(DRC_ERR_INVALID_ARGUMENT, "null model");
  if (int rc = drc_default_qpik_params(m, 1, pp)) return rc;
  pp->mode = DRC_MODE_QPIK;
  pp->frame_id = -1;
  return DRC_OK;
}

int drc_clearance_path_batch(const drc_model* m, int64_t B, int waypoints, int substeps, double d_stop,
                             const double* q_path, int32_t* result, int32_t* sample_stop, double* d_min,
                             int32_t* sample_min, int32_t* pair_min, double* dist_traj, void* stream) {
  drc_qpik_params pp;
  if (int rc = clearance_params(m, &pp)) return rc;
  return drc_amd::clearance(m, &pp, B, waypoints, substeps, d_stop, q_path, result, sample_stop, d_min, sample_min,
                            pair_min, dist_traj, stream);
}

int drc_clearance_path_obstacles_batch(const drc_model* m, int64_t B, int waypoints, int substeps, double d_stop,
                                       const double* q_path, const double* obstacle_pose, int64_t obstacle_ld,
                                       int32_t* result, int32_t* sample_stop, double* d_min, int32_t* sample_min,
                                       int32_t* pair_min, double* dist_traj, void* stream) {
  drc_qpik_params pp;
  if (int rc = clearance_params(m, &pp)) return rc;
  return drc_amd::clearance(m, &pp, B, waypoints, substeps, d_stop, q_path, result, sample_stop, d_min, sample_min,
                            pair_min, dist_traj, stream, drc_amd::stage_in(obstacle_pose, obstacle_ld));
}

int drc_clearance_certify_batch(const drc_model* m, int64_t B, int waypoints, double d_stop, int max_depth,
                                const double* q_path, int32_t* result, int32_t* seg_stop, double* t_stop,
                                double* d_min, int32_t* seg_min, double* t_min, int32_t* pair_min, double* d_lower,
                                int32_t* samples_used, double* motion_bound, void* stream) {
  drc_qpik_params pp;
  if (int rc = clearance_params(m, &pp)) return rc;
  return drc_amd::certify(m, &pp, B, waypoints, d_stop, max_depth, q_path, result, seg_stop, t_stop, d_min, seg_min,
                          t_min, pair_min, d_lower, samples_used, motion_bound, stream);
}

int drc_clearance_certify_obstacles_batch(const drc_model* m, int64_t B, int waypoints, double d_stop, int max_depth,
                                          const double* q_path, const double* obstacle_pose, int64_t obstacle_ld,
                                          int32_t* result, int32_t* seg_stop, double* t_stop, double* d_min,
                                          int32_t* seg_min, double* t_min, int32_t* pair_min, double* d_lower,
                                          int32_t* samples_used, double* motion_bound, void* stream) {
  drc_qpik_params pp;
  if (int rc = clearance_params(m, &pp)) return rc;
  return drc_amd::certify(m, &pp, B, waypoints, d_stop, max_depth, q_path, result, seg_stop, t_stop, d_min, seg_min,
                          t_min, pair_min, d_lower, samples_used, motion_bound, stream,
                          drc_amd::stage_in(obstacle_pose, obstacle_ld));
}

// ---- QPID -------------------------------------------------
int drc_default_qpid_params(const drc_model* m, int exact, drc_qpik_params* p) {
  int rc = drc_default_qpik_params(m, exact, p);
  if (rc) return rc;
  const bool moma = m->hm.dev.kind == 1;
  for (int i = 0; i < 6; ++i) {
    p->kp[i] = moma ? 400 : 100;  // robot_controller.cpp:12-13; MoMa :15-16
    p->kv[i] = moma ? 40 : 20;    // QPIDStep: Kp e + Kv (xdot_target - xdot) (:347; MoMa :230)
  }
  p->feedforward = 0;
  p->w_reg = 0;  // QP_ID.cpp:102: the regulariser is commented out
  // P is singular on null(J); OSQP's polish delta 1e-6 cannot certify at
  // eps_exact there, so parity mode regularises the polish with 1e-10
  if (exact) p->solver.delta = 1e-10;
  p->solver.check_termination = 25;  // QPID keeps OSQP's check interval,
  p->solver.polish_refine_iter = 3;   // refinement count and Ruiz passes in every mode
  p->solver.scaling = 10;             // (its optimum is a face: the scaling picks the point on it)
  return DRC_OK;
}

int drc_qpid_batch(const drc_model* m, const drc_qpik_params* p, int64_t B, const double* q, const double* qdot,
                   const double* xt, const double* xdt, const double* xi, const double* xdi, double* qddot_out,
                   double* tau_out, int32_t* status, int32_t* iters, void* stream) {
  drc_amd::IO io = drc_amd::task_io(B, q, qdot, xt, xdt, xi, xdi);
  io.out = qddot_out;
  io.out2 = tau_out;
  io.status = status;
  io.iters = iters;
  return drc_amd::launch_qpid(m, p, 0, io, stream);
}

int drc_qpid_stages_batch(const drc_model* m, const drc_qpik_params* p, int64_t B, const double* q,
                          const double* qdot, const double* xt, const double* xdt, const double* xi,
                          const double* xdi, double* pose, double* jac, double* man, double* dist, int32_t* pair,
                          double* xddot_des, double* jdot, double* qpid_terms, double* graddot, void* stream) {
  drc_amd::IO io = drc_amd::task_io(B, q, qdot, xt, xdt, xi, xdi);
  io.st_pose = pose;
  io.st_jac = jac;
  io.st_man = man;
  io.st_dist = dist;
  io.st_pair = pair;
  io.st_xdd = xddot_des;
  io.st_jdot = jdot;
  io.st_qpid = qpid_terms;
  io.st_gdv = graddot;
  return drc_amd::launch_qpid(m, p, 1, io, stream);
}

}  // extern "C"

// ---- host-buffer entry points (synchronous; staged through device memory) --
namespace drc_amd {
// Device staging buffer and its pinned host mirror, both >= `words` doubles
// (the caller holds m->host_mu).
static int ensure_staging(drc_model* m, int64_t words) {
  const int64_t bytes = words * 8;
  if (m->stage_bytes < bytes) {
    if (m->stage) (void)hipFree(m->stage);
    m->stage = nullptr;
    m->stage_bytes = 0;
    if (hipMalloc(&m->stage, bytes) != hipSuccess) return drc_amd::set_err(DRC_ERR_HIP, "hipMalloc (staging)");
    m->stage_bytes = bytes;
  }
  if (m->pinned_bytes < bytes) {
    if (m->pinned) (void)hipHostFree(m->pinned);
    m->pinned = nullptr;
    m->pinned_bytes = 0;
    if (hipHostMalloc(reinterpret_cast<void**>(&m->pinned), bytes, hipHostMallocDefault) != hipSuccess)
      return drc_amd::set_err(DRC_ERR_HIP, "hipHostMalloc (staging)");
    m->pinned_bytes = bytes;
  }
  if (!m->hdone && hipEventCreateWithFlags(&m->hdone, hipEventDisableTiming) != hipSuccess)
    return drc_amd::set_err(DRC_ERR_HIP, "hipEventCreate (host entries)");
  if (!m->hstream && hipStreamCreateWithFlags(&m->hstream, hipStreamNonBlocking) != hipSuccess)
    return drc_amd::set_err(DRC_ERR_HIP, "hipStreamCreate");
  return DRC_OK;
}

static inline int64_t now_ns() {
  return std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch())
      .count();
}
// How a synchronous entry waits for its copy back (DRC_HOST_WAIT, in us): it
// polls the completion event for up to that long (default 300 us: one B = 1
// cycle is ~100 us, polling keeps the thread on its core instead of handing
// it to the scheduler and waking it up again), with a pause between polls,
// then blocks in hipEventSynchronize -- a long call (large B) does not hold a
// core busy for its whole GPU time.  0: block at once.
static int wait_done(drc_model* m) {
  static const int64_t spin_ns = 1000 * env_int("DRC_HOST_WAIT", 300, 0);
  if (hipEventRecord(m->hdone, m->hstream) != hipSuccess) return drc_amd::set_err(DRC_ERR_HIP, "hipEventRecord");
  if (spin_ns > 0) {
    const int64_t t_end = now_ns() + spin_ns;
    do {
      const hipError_t e = hipEventQuery(m->hdone);
      if (e == hipSuccess) return DRC_OK;
      if (e != hipErrorNotReady) return drc_amd::set_err(DRC_ERR_HIP, "hipEventQuery");
      for (int k = 0; k < 16; ++k) __builtin_ia32_pause();
    } while (now_ns() < t_end);
  }
  if (hipEventSynchronize(m->hdone) != hipSuccess) return drc_amd::set_err(DRC_ERR_HIP, "hipEventSynchronize");
  return DRC_OK;
}

// A synchronous host-buffer call in one round trip.  The entry registers each
// of its host arrays once, with its element count and where the array's device
// pointer goes (a NULL array gets a NULL device pointer and no space): in()
// arrays are packed into the pinned mirror and sent in one transfer, out()
// arrays lie after the inputs (host_staging.hpp) and come back in one
// transfer.  run() sets the device pointers, sends the inputs, calls
// `launches` (which enqueues on m->hstream), fetches the outputs, waits and
// copies them to the caller.  The staging buffers are the model's: the object
// holds m->host_mu from its construction to the entry's return.
class HostStage {
 public:
  explicit HostStage(drc_model* m) : m_(m), lock_(m->host_mu) {}
  template <class T>
  void in(const T* host, int64_t count, const T** dev) {
    add(host, nullptr, count, sizeof(T), dev,
        [](void* to, void* p) { *static_cast<const T**>(to) = static_cast<const T*>(p); });
  }
  template <class T>
  void out(T* host, int64_t count, T** dev) {
    add(nullptr, host, count, sizeof(T), dev, [](void* to, void* p) { *static_cast<T**>(to) = static_cast<T*>(p); });
  }
  template <class Launches>
  int run(Launches launches) {
    drc_model* const m = m_;
    if (full_) return set_err(DRC_ERR_INVALID_ARGUMENT, "too many host arrays in one call");
    if (hipSetDevice(m->device) != hipSuccess) return set_err(DRC_ERR_HIP, "hipSetDevice");
    const int64_t t0 = m->tl_on ? now_ns() : 0;
    const int64_t wi = lay_.in_words, wo = lay_.out_words;
    if (int rc = ensure_staging(m, wi + wo)) return rc;
    double* dev = reinterpret_cast<double*>(m->stage);
    for (int i = 0; i < lay_.n; ++i) {
      arr_[i].set(arr_[i].dev, dev + lay_.offset(i));
      if (arr_[i].src) std::memcpy(m->pinned + lay_.offset(i), arr_[i].src, lay_.r[i].bytes);
    }
    const int64_t t1 = m->tl_on ? now_ns() : 0;
    if (wi && hipMemcpyAsync(dev, m->pinned, wi * 8, hipMemcpyHostToDevice, m->hstream) != hipSuccess)
      return set_err(DRC_ERR_HIP, "hipMemcpyAsync H2D");
    if (int rc = launches()) return rc;
    if (wo && hipMemcpyAsync(m->pinned + wi, dev + wi, wo * 8, hipMemcpyDeviceToHost, m->hstream) != hipSuccess)
      return set_err(DRC_ERR_HIP, "hipMemcpyAsync D2H");
    const int64_t t2 = m->tl_on ? now_ns() : 0;
    if (int rc = wait_done(m)) return rc;
    const int64_t t3 = m->tl_on ? now_ns() : 0;
    for (int i = 0; i < lay_.n; ++i)
      if (arr_[i].dst) std::memcpy(arr_[i].dst, m->pinned + lay_.offset(i), lay_.r[i].bytes);
    if (m->tl_on) {
      const int64_t t4 = now_ns();
      for (int64_t v : {t0, t1, t2, t3, t4}) m->tl.push_back(v);
    }
    return DRC_OK;
  }

 private:
  struct Arr {
    const void* src;  // the caller's input array, or
    void* dst;        // the caller's output array
    void* dev;        // the entry's device pointer of this array, set through
    void (*set)(void* to, void* p);
  };
  void add(const void* src, void* dst, int64_t count, int elem_bytes, void* dev, void (*set)(void*, void*)) {
    set(dev, nullptr);
    const int i = lay_.add(src || dst, dst != nullptr, count, elem_bytes);
    if (i == StagingLayout::kFull) full_ = true;
    if (i >= 0) arr_[i] = {src, dst, dev, set};
  }
  drc_model* m_;
  std::lock_guard<std::mutex> lock_;
  StagingLayout lay_;
  Arr arr_[StagingLayout::kMaxArrays];
  bool full_ = false;
};

// The six task inputs of a controller entry, into the call record
static void stage_task_inputs(HostStage& st, IO& io, int64_t nv, const double* q, const double* qdot,
                              const double* xt, const double* xdt, const double* xi, const double* xdi) {
  st.in(q, nv * io.B, &io.q);
  st.in(qdot, nv * io.B, &io.qdot);
  st.in(xt, 12 * io.B, &io.xt);
  st.in(xdt, 6 * io.B, &io.xdt);
  st.in(xi, 12 * io.B, &io.xi);
  st.in(xdi, 6 * io.B, &io.xdi);
}

// drc_qpik_host; with `stamps` (host [kStamps][B]) its two variants that also
// return the kernels' stage stamps
static int qpik_host(drc_model* m, const drc_qpik_params* p, int64_t B, const double* q, const double* qdot,
                     const double* xt, const double* xdt, const double* xi, const double* xdi, double* out,
                     int32_t* status, int32_t* iters, uint64_t* stamps) {
  if (!m || !p) return set_err(DRC_ERR_INVALID_ARGUMENT, "null model/params");
  if (B <= 0) return B == 0 ? DRC_OK : set_err(DRC_ERR_INVALID_ARGUMENT, "negative batch");
  HostStage st(m);
  IO io = make_io(B);
  stage_task_inputs(st, io, m->hm.dev.nv, q, qdot, xt, xdt, xi, xdi);
  st.out(out, actuated_width(m->hm.dev) * B, &io.out);
  st.out(status, B, &io.status);
  st.out(iters, B, &io.iters);
  st.out(stamps, kStamps * B, &io.stamps);
  return st.run([&]() -> int {
    if (io.stamps && hipMemsetAsync(io.stamps, 0, sizeof(uint64_t) * kStamps * B, m->hstream) != hipSuccess)
      return set_err(DRC_ERR_HIP, "hipMemsetAsync(stamps)");
    return launch(m, p, 0, io, m->hstream);
  });
}
}  // namespace drc_amd

extern "C" {
using drc_amd::HostStage;
using drc_amd::IO;

int drc_qpik_host(drc_model* m, const drc_qpik_params* p, int64_t B, const double* q, const double* qdot,
                  const double* xt, const double* xdt, const double* xi, const double* xdi, double* out,
                  int32_t* status, int32_t* iters) {
  if (!m) return drc_amd::set_err(DRC_ERR_INVALID_ARGUMENT, "null model");
  if (!out || !status) return drc_amd::set_err(DRC_ERR_INVALID_ARGUMENT, "qdot_out and status are required");
  return drc_amd::qpik_host(m, p, B, q, qdot, xt, xdt, xi, xdi, out, status, iters, nullptr);
}

int drc_qpik_host_timed(drc_model* m, const drc_qpik_params* p, int64_t B, const double* q, const double* qdot,
                        const double* xt, const double* xdt, const double* xi, const double* xdi, double* out,
                        int32_t* status, int32_t* iters, drc_time_duration* ts) {
  if (!m) return drc_amd::set_err(DRC_ERR_INVALID_ARGUMENT, "null model");
  if (!out || !status || !ts) return drc_amd::set_err(DRC_ERR_INVALID_ARGUMENT, "qdot_out, status and time_status are required");
  std::memset(ts, 0, sizeof(*ts));
  if (B <= 0) return B == 0 ? DRC_OK : drc_amd::set_err(DRC_ERR_INVALID_ARGUMENT, "negative batch");
  std::vector<uint64_t> st(static_cast<size_t>(drc_amd::kStamps * B));
  const auto t0 = std::chrono::steady_clock::now();
  const int rc = drc_amd::qpik_host(m, p, B, q, qdot, xt, xdt, xi, xdi, out, status, iters, st.data());
  const double wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  if (rc) return rc;
  // stamps are s_memrealtime ticks (100 MHz); per-instance stage durations, averaged
  // (the region was cleared before the launch: an instance whose stamps are
  // missing -- a debug task stage that does not stamp -- or out of order is
  // left out of the averages)
  const double tick = 1e-8;
  double task = 0, asmb = 0, solve = 0, store = 0, span = 0;
  int64_t valid = 0;
  for (int64_t b = 0; b < B; ++b) {
    auto at = [&](int k) { return st[static_cast<size_t>(k * B + b)]; };
    bool ok = at(0) != 0;
    for (int k = 1; k < drc_amd::kTimeStamps && ok; ++k) ok = at(k) >= at(k - 1);
    if (!ok) continue;
    auto dt = [&](int k1, int k0) { return static_cast<double>(at(k1) - at(k0)) * tick; };
    task += dt(drc_amd::ST_TASK1, drc_amd::ST_TASK0);
    asmb += dt(drc_amd::ST_ASM, drc_amd::ST_QP0);
    solve += dt(drc_amd::ST_SOLVED, drc_amd::ST_ASM);
    store += dt(drc_amd::ST_OUT, drc_amd::ST_SOLVED);
    span += dt(drc_amd::ST_OUT, drc_amd::ST_TASK0);
    ++valid;
  }
  if (valid == 0) {  // no stamps (a debug stage): the whole call counts as getSolution's place
    ts->solve_qp = wall;
    return DRC_OK;
  }
  const double inv = 1.0 / static_cast<double>(valid);
  ts->set_ineq = task * inv;         // FK, J, manipulability + gradient, min distance + gradient
  ts->set_constraint = asmb * inv;   // P, q, bounds, CBF rows stacked (QP_base.h:202-227)
  ts->set_qp = ts->set_ineq + ts->set_constraint;
  ts->set_solver = solve * inv;      // Ruiz scaling, factorisation, ADMM, certified polish
  // output store plus what the call spends outside the instance (launch,
  // transfers, synchronisation): getSolution's place in the reference
  ts->solve_qp = store * inv + (wall - span * inv > 0 ? wall - span * inv : 0.0);
  return DRC_OK;
}

int drc_debug_qpik_stamps(drc_model* m, const drc_qpik_params* p, int64_t B, const double* q, const double* qdot,
                          const double* xt, const double* xdt, const double* xi, const double* xdi, double* out,
                          int32_t* status, int32_t* iters, uint64_t* stamps) {
  if (!m) return drc_amd::set_err(DRC_ERR_INVALID_ARGUMENT, "null model");
  if (!out || !status || !stamps) return drc_amd::set_err(DRC_ERR_INVALID_ARGUMENT, "qdot_out, status and stamps are required");
  return drc_amd::qpik_host(m, p, B, q, qdot, xt, xdt, xi, xdi, out, status, iters, stamps);
}

int drc_qpik_stages_host(drc_model* m, const drc_qpik_params* p, int64_t B, const double* q, const double* qdot,
                         const double* xt, const double* xdt, const double* xi, const double* xdi, double* pose,
                         double* jac, double* man, double* dist, int32_t* pair, double* xdd) {
  using drc_amd::set_err;
  if (!m) return set_err(DRC_ERR_INVALID_ARGUMENT, "null model");
  if (!p) return set_err(DRC_ERR_INVALID_ARGUMENT, "null model/params");
  if (B <= 0) return B == 0 ? DRC_OK : set_err(DRC_ERR_INVALID_ARGUMENT, "negative batch");
  const int64_t n = m->hm.dev.nv, na = drc_amd::arm_width(m->hm.dev);
  HostStage st(m);
  IO io = drc_amd::make_io(B);
  drc_amd::stage_task_inputs(st, io, n, q, qdot, xt, xdt, xi, xdi);
  st.out(pose, 12 * B, &io.st_pose);
  st.out(jac, 6 * n * B, &io.st_jac);
  st.out(man, (1 + na) * B, &io.st_man);
  st.out(dist, (1 + n) * B, &io.st_dist);
  st.out(xdd, 6 * B, &io.st_xdd);
  st.out(pair, B, &io.st_pair);
  return st.run([&] { return drc_amd::launch(m, p, 1, io, m->hstream); });
}

// dist_traj goes both ways: the entries the walk does not reach keep what the
// caller's array held, so its content is staged in and copied under the
// kernel's stores before the launch
int drc_clearance_path_host(drc_model* m, int64_t B, int waypoints, int substeps, double d_stop, const double* q_path,
                            int32_t* result, int32_t* sample_stop, double* d_min, int32_t* sample_min,
                            int32_t* pair_min, double* dist_traj) {
  using drc_amd::set_err;
  if (!m) return set_err(DRC_ERR_INVALID_ARGUMENT, "null model");
  if (B < 0) return set_err(DRC_ERR_INVALID_ARGUMENT, "negative batch");
  if (waypoints < 1 || substeps < 1) return set_err(DRC_ERR_INVALID_ARGUMENT, "waypoints and substeps must be at least 1");
  const int64_t N = drc_amd::clearance_samples(waypoints, substeps);
  if (N > 0x7fffffff) return set_err(DRC_ERR_INVALID_ARGUMENT, "(waypoints - 1) substeps + 1 samples do not fit 31 bits");
  if (B == 0) return DRC_OK;
  HostStage st(m);
  const double *dq, *dprev;
  int32_t *dres, *dstop, *dsmin, *dpmin;
  double *ddmin, *dtraj;
  st.in(q_path, int64_t(waypoints) * m->hm.dev.nv * B, &dq);
  st.in(static_cast<const double*>(dist_traj), N * B, &dprev);
  st.out(result, B, &dres);
  st.out(sample_stop, B, &dstop);
  st.out(d_min, B, &ddmin);
  st.out(sample_min, B, &dsmin);
  st.out(pair_min, B, &dpmin);
  st.out(dist_traj, N * B, &dtraj);
  return st.run([&]() -> int {
    if (dtraj && hipMemcpyAsync(dtraj, dprev, size_t(N) * B * 8, hipMemcpyDeviceToDevice, m->hstream) != hipSuccess)
      return set_err(DRC_ERR_HIP, "hipMemcpyAsync(dist_traj)");
    return drc_clearance_path_batch(m, B, waypoints, substeps, d_stop, dq, dres, dstop, ddmin, dsmin, dpmin, dtraj,
                                    m->hstream);
  });
}


// ---- per-cycle kinematics and state ----------------------
int drc_kinematics_batch(const drc_model* m, int frame_id, int64_t B, const double* q, const double* qdot,
                         double* pose, double* jac, double* xdot, void* stream) {
  if (!m) return drc_amd::set_err(DRC_ERR_INVALID_ARGUMENT, "null model");
  drc_qpik_params p;
  if (int rc = drc_default_qpik_params(m, 1, &p)) return rc;
  p.frame_id = frame_id;
  drc_amd::IO io = drc_amd::make_io(B);
  io.q = q;
  io.qdot = qdot;
  io.st_pose = pose;
  io.st_jac = jac;
  io.st_xdd = xdot;
  return drc_amd::launch_closed_form(m, &p, 3, io, stream);
}

int drc_state_host(drc_model* m, int frame_id, int64_t B, const double* q, const double* qdot, double* pose,
                   double* jac, double* xdot, double* M, double* M_inv, double* g, double* nle, double* c) {
  using drc_amd::set_err;
  if (!m) return set_err(DRC_ERR_INVALID_ARGUMENT, "null model");
  if (B <= 0) return B == 0 ? DRC_OK : set_err(DRC_ERR_INVALID_ARGUMENT, "negative batch");
  if (!q) return set_err(DRC_ERR_INVALID_ARGUMENT, "q is required");
  if ((xdot || nle || c) && !qdot) return set_err(DRC_ERR_INVALID_ARGUMENT, "qdot is required for xdot / nle / c");
  const int64_t n = m->hm.dev.nv;
  HostStage st(m);
  const double *dq, *dqd;
  double *dpose, *djac, *dxdot, *dM, *dMinv, *dg, *dnle, *dc;
  st.in(q, n * B, &dq);
  st.in(qdot, n * B, &dqd);
  st.out(pose, 12 * B, &dpose);
  st.out(jac, 6 * n * B, &djac);
  st.out(xdot, 6 * B, &dxdot);
  st.out(M, n * n * B, &dM);
  st.out(M_inv, n * n * B, &dMinv);
  st.out(g, n * B, &dg);
  st.out(nle, n * B, &dnle);
  st.out(c, n * B, &dc);
  return st.run([&]() -> int {
    if (pose || jac || xdot)
      if (int rc = drc_kinematics_batch(m, frame_id, B, dq, dqd, dpose, djac, dxdot, m->hstream)) return rc;
    if (M || M_inv || g || nle || c)
      if (int rc = drc_dynamics_batch(m, 0, B, dq, dqd, dM, dMinv, dg, dnle, dc, m->hstream)) return rc;
    return DRC_OK;
  });
}

// ---- closed-form controllers ------------------------------
int drc_clik_batch(const drc_model* m, const drc_qpik_params* p, int64_t B, const double* q, const double* qdot,
                   const double* xt, const double* xdt, const double* xi, const double* xdi, const double* null_qdot,
                   double* qdot_out, void* stream) {
  drc_amd::IO io = drc_amd::task_io(B, q, qdot, xt, xdt, xi, xdi);
  io.cf_null = null_qdot;
  io.out = qdot_out;
  return drc_amd::launch_closed_form(m, p, 1, io, stream);
}

int drc_osf_batch(const drc_model* m, const drc_qpik_params* p, int64_t B, const double* q, const double* qdot,
                  const double* xt, const double* xdt, const double* xi, const double* xdi, const double* null_torque,
                  double* tau_out, void* stream) {
  drc_amd::IO io = drc_amd::task_io(B, q, qdot, xt, xdt, xi, xdi);
  io.cf_null = null_torque;
  io.out = tau_out;
  return drc_amd::launch_closed_form(m, p, 2, io, stream);
}

int drc_closed_form_host(drc_model* m, const drc_qpik_params* p, int kind, int64_t B, const double* q,
                         const double* qdot, const double* xt, const double* xdt, const double* xi, const double* xdi,
                         const double* nullv, double* out) {
  using drc_amd::set_err;
  if (!m || !p) return set_err(DRC_ERR_INVALID_ARGUMENT, "null model/params");
  if (kind != 1 && kind != 2) return set_err(DRC_ERR_INVALID_ARGUMENT, "kind must be 1 (CLIK) or 2 (OSF)");
  if (B <= 0) return B == 0 ? DRC_OK : set_err(DRC_ERR_INVALID_ARGUMENT, "negative batch");
  if (!out) return set_err(DRC_ERR_INVALID_ARGUMENT, "out is required");
  const int64_t n = m->hm.dev.nv;
  HostStage st(m);
  IO io = drc_amd::make_io(B);
  drc_amd::stage_task_inputs(st, io, n, q, qdot, xt, xdt, xi, xdi);
  st.in(nullv, n * B, &io.cf_null);
  st.out(out, n * B, &io.out);
  return st.run([&] { return drc_amd::launch_closed_form(m, p, kind, io, m->hstream); });
}

int drc_qpid_host(drc_model* m, const drc_qpik_params* p, int64_t B, const double* q, const double* qdot,
                  const double* xt, const double* xdt, const double* xi, const double* xdi, double* qdd, double* tau,
                  int32_t* status, int32_t* iters) {
  using drc_amd::set_err;
  if (!m || !p) return set_err(DRC_ERR_INVALID_ARGUMENT, "null model/params");
  if (B <= 0) return B == 0 ? DRC_OK : set_err(DRC_ERR_INVALID_ARGUMENT, "negative batch");
  if (!qdd || !tau || !status) return set_err(DRC_ERR_INVALID_ARGUMENT, "qddot_out, tau_out and status are required");
  const int64_t na = drc_amd::actuated_width(m->hm.dev);
  HostStage st(m);
  IO io = drc_amd::make_io(B);
  drc_amd::stage_task_inputs(st, io, m->hm.dev.nv, q, qdot, xt, xdt, xi, xdi);
  st.out(qdd, na * B, &io.out);
  st.out(tau, na * B, &io.out2);
  st.out(status, B, &io.status);
  st.out(iters, B, &io.iters);
  return st.run([&] { return drc_amd::launch_qpid(m, p, 0, io, m->hstream); });
}

int drc_qpid_stages_host(drc_model* m, const drc_qpik_params* p, int64_t B, const double* q, const double* qdot,
                         const double* xt, const double* xdt, const double* xi, const double* xdi, double* pose,
                         double* jac, double* man, double* dist, int32_t* pair, double* xddot_des, double* jdot,
                         double* qpid_terms, double* graddot) {
  using drc_amd::set_err;
  if (!m || !p) return set_err(DRC_ERR_INVALID_ARGUMENT, "null model/params");
  if (B <= 0) return B == 0 ? DRC_OK : set_err(DRC_ERR_INVALID_ARGUMENT, "negative batch");
  const int64_t n = m->hm.dev.nv, na = drc_amd::arm_width(m->hm.dev);
  HostStage st(m);
  IO io = drc_amd::make_io(B);
  drc_amd::stage_task_inputs(st, io, n, q, qdot, xt, xdt, xi, xdi);
  st.out(pose, 12 * B, &io.st_pose);
  st.out(jac, 6 * n * B, &io.st_jac);
  st.out(man, (1 + na) * B, &io.st_man);
  st.out(dist, (1 + n) * B, &io.st_dist);
  st.out(pair, B, &io.st_pair);
  st.out(xddot_des, 6 * B, &io.st_xdd);
  st.out(jdot, 6 * n * B, &io.st_jdot);
  st.out(qpid_terms, 8 * B, &io.st_qpid);
  st.out(graddot, (na + n) * B, &io.st_gdv);
  return st.run([&] { return drc_amd::launch_qpid(m, p, 1, io, m->hstream); });
}

// ---- joint-space dynamics ------------------------------
int drc_dynamics_batch(drc_model* m, int actuated, int64_t B, const double* q, const double* qdot, double* M,
                       double* M_inv, double* g, double* nle, double* c, void* stream) {
  using drc_amd::set_err;
  if (!m) return drc_amd::set_err(DRC_ERR_INVALID_ARGUMENT, "null model");
  if (B < 0) return drc_amd::set_err(DRC_ERR_INVALID_ARGUMENT, "negative batch");
  if (B == 0) return DRC_OK;
  if (!q) return drc_amd::set_err(DRC_ERR_INVALID_ARGUMENT, "q is required");
  if ((nle || c) && !qdot) return drc_amd::set_err(DRC_ERR_INVALID_ARGUMENT, "qdot is required for nle / c");
  if (actuated && m->hm.dev.kind != 1)
    return drc_amd::set_err(DRC_ERR_INVALID_ARGUMENT, "actuated dynamics need a mobile-manipulator model");
  if (B > 0x7ffffff0) return drc_amd::set_err(DRC_ERR_INVALID_ARGUMENT, "batch too large");
  HIP_TRY(hipSetDevice(m->device));
  std::lock_guard<std::mutex> launch_lock(m->launch_mu);
  drc_amd::Launch L(m, stream);
  drc_amd::DynList cod{};  // (a context, and the COD list in it, only for M_inv)
  if (M_inv) {
    if (int r = L.context()) return r;
    if (int r = L.carve(&drc_amd::StreamCtx::dyn_list, [&](void* p) { return drc_amd::dyn_list(p, B); }, &cod)) return r;
  }
  const int rc = drc_amd::launch_dynamics(m->d_model, m->hm.dev, actuated != 0, B, q, qdot, M, M_inv, g, nle, c,
                                          cod.list, L.st);
  if (rc == 1) return drc_amd::set_err(DRC_ERR_INVALID_ARGUMENT, "batch too large");
  if (rc) return drc_amd::set_err(DRC_ERR_HIP, std::string("dynamics launch: ") + hipGetErrorString(hipGetLastError()));
  return L.done();
}

int drc_dynamics_host(drc_model* m, int actuated, int64_t B, const double* q, const double* qdot, double* M,
                      double* M_inv, double* g, double* nle, double* c) {
  using drc_amd::set_err;
  if (!m) return set_err(DRC_ERR_INVALID_ARGUMENT, "null model");
  if (B <= 0) return B == 0 ? DRC_OK : set_err(DRC_ERR_INVALID_ARGUMENT, "negative batch");
  if (!q) return set_err(DRC_ERR_INVALID_ARGUMENT, "q is required");
  const int64_t n = m->hm.dev.nv, no = actuated ? drc_amd::actuated_width(m->hm.dev) : n;
  HostStage st(m);
  const double *dq, *dqd;
  double *dM, *dMinv, *dg, *dnle, *dc;
  st.in(q, n * B, &dq);
  st.in(qdot, n * B, &dqd);
  st.out(M, no * no * B, &dM);
  st.out(M_inv, no * no * B, &dMinv);
  st.out(g, no * B, &dg);
  st.out(nle, no * B, &dnle);
  st.out(c, no * B, &dc);
  // (a missing qdot, or `actuated` on a manipulator: the batch entry's errors)
  return st.run([&] { return drc_dynamics_batch(m, actuated, B, dq, dqd, dM, dMinv, dg, dnle, dc, m->hstream); });
}

// ---- joint torque step ---------------------------------
int drc_joint_torque_step_batch(drc_model* m, int64_t B, const double* q, const double* qdot, const double* q_target,
                                const double* qdot_target, const double* qddot_target, double dt, const double* kp,
                                const double* kv, double* tau, void* stream) {
  using drc_amd::set_err;
  if (!m) return set_err(DRC_ERR_INVALID_ARGUMENT, "null model");
  if (m->hm.dev.nobst > 0) return set_err(DRC_ERR_UNSUPPORTED, drc_amd::kSlotsUnsupportedMsg);
  if (B < 0) return set_err(DRC_ERR_INVALID_ARGUMENT, "negative batch");
  if (B == 0) return DRC_OK;
  if (!q || !tau) return set_err(DRC_ERR_INVALID_ARGUMENT, "q and tau are required");
  if (!qddot_target && (!qdot || !qdot_target))
    return set_err(DRC_ERR_INVALID_ARGUMENT, "qdot and qdot_target are required without qddot_target");
  const drc_amd::DevModel& d = m->hm.dev;
  const int nb = d.kind == 1 ? d.n_arm : d.nv;
  double kpv[drc_amd::kMaxJoints], kvv[drc_amd::kMaxJoints];
  for (int i = 0; i < nb; ++i) {  // robot_controller.cpp:14-15 (MoMa :17-18): 400 / 40
    kpv[i] = kp ? kp[i] : 400.0;
    kvv[i] = kv ? kv[i] : 40.0;
  }
  HIP_TRY(hipSetDevice(m->device));
  const int rc = drc_amd::launch_torque_step(m->d_model, d, B, q, qdot, q_target, qdot_target, qddot_target, dt, kpv,
                                             kvv, tau, reinterpret_cast<hipStream_t>(stream));
  if (rc == 1) return set_err(DRC_ERR_INVALID_ARGUMENT, "batch too large");
  if (rc) return set_err(DRC_ERR_HIP, std::string("torque step launch: ") + hipGetErrorString(hipGetLastError()));
  return DRC_OK;
}

int drc_joint_torque_step_host(drc_model* m, int64_t B, const double* q, const double* qdot, const double* q_target,
                               const double* qdot_target, const double* qddot_target, double dt, const double* kp,
                               const double* kv, double* tau) {
  using drc_amd::set_err;
  if (!m) return set_err(DRC_ERR_INVALID_ARGUMENT, "null model");
  if (m->hm.dev.nobst > 0) return set_err(DRC_ERR_UNSUPPORTED, drc_amd::kSlotsUnsupportedMsg);
  if (B <= 0) return B == 0 ? DRC_OK : set_err(DRC_ERR_INVALID_ARGUMENT, "negative batch");
  if (!q || !tau) return set_err(DRC_ERR_INVALID_ARGUMENT, "q and tau are required");
  const int64_t n = m->hm.dev.nv, nb = drc_amd::arm_width(m->hm.dev);
  HostStage st(m);
  const double *dq, *dqd, *dqt, *dqdt, *dqddt;
  double* dtau;
  st.in(q, n * B, &dq);
  st.in(qdot, n * B, &dqd);
  st.in(q_target, nb * B, &dqt);
  st.in(qdot_target, nb * B, &dqdt);
  st.in(qddot_target, nb * B, &dqddt);
  st.out(tau, nb * B, &dtau);
  return st.run(
      [&] { return drc_joint_torque_step_batch(m, B, dq, dqd, dqt, dqdt, dqddt, dt, kp, kv, dtau, m->hstream); });
}

}  // extern "C"

