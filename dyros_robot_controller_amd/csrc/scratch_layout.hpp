// Layouts of the per-stream device scratch (api.cpp StreamCtx: pool, roll,
// seeds, dyn_list).  Each layout is one sequence of "take n elements of T"
// steps that yields the named regions and the byte count together: a launch
// path calls it on a null base to measure, grows the block to `bytes`, and
// calls it again on the block.  The size passed to the allocator and the
// addresses passed to the kernels come from the same steps, so they cannot
// disagree.  No HIP here: tools/scratch_layout_host_test.cpp checks the rules
// on the CPU (DESIGN.md "Stream scratch").
#pragma once
#include <cstddef>
#include <cstdint>

namespace drc_amd {

// What a Carver took, for the host test: a region's name, element size,
// offset, element count and the address it handed out
struct RegionLog {
  struct Region {
    const char* name;
    int elem;
    int64_t off, n;
    void* p;
  };
  static constexpr int kMax = 16;
  int count = 0;
  Region r[kMax];
};

// Carves arrays off a block one after the other.  Every region starts aligned
// to its element (or to `align`, a power of two, where a layout asks for
// more); an empty region has no address; without a base only the offsets count
struct Carver {
  char* base;
  RegionLog* log = nullptr;
  int64_t off = 0;
  template <class T>
  T* take(const char* name, int64_t n, int64_t align = int64_t(sizeof(T))) {
    off = (off + align - 1) & ~(align - 1);
    T* p = base && n > 0 ? reinterpret_cast<T*>(base + off) : nullptr;
    if (log && log->count < RegionLog::kMax) log->r[log->count++] = {name, int(sizeof(T)), off, n, p};
    off += n * int64_t(sizeof(T));
    return p;
  }
};

// Task records are padded to whole 128-B lines
inline int64_t record_stride(int rLen) { return (int64_t(rLen) + 15) & ~int64_t(15); }

// pool, drc_qpik_batch and the stage call with the lane stage: the task
// records [B][stride] (none for a stage call), the lane stage's hard list and
// flags, then -- on an 8-byte boundary, which the byte count includes either
// way -- the order kernel's order, hot list and hot flags (auto_order only)
struct QpikPool {
  double* rec;
  int32_t* hard;
  uint8_t* hard_flag;
  int32_t *order, *hot;
  uint8_t* hot_flag;
  int64_t bytes;
};
inline QpikPool qpik_pool(void* base, int64_t stride, int64_t B, bool stages, bool auto_order,
                          RegionLog* log = nullptr) {
  Carver c{static_cast<char*>(base), log};
  QpikPool L;
  L.rec = c.take<double>("rec", stages ? 0 : stride * B);
  L.hard = c.take<int32_t>("hard", B);
  L.hard_flag = c.take<uint8_t>("hard_flag", B);
  L.order = c.take<int32_t>("order", auto_order ? B : 0, 8);
  L.hot = c.take<int32_t>("hot", auto_order ? B : 0);
  L.hot_flag = c.take<uint8_t>("hot_flag", auto_order ? B : 0);
  L.bytes = c.off;
  return L;
}

// pool, drc_qpid_batch: the records, M [na*na][B], g [na][B] and, whole-body
// robots, the joint-order g [nv][B].  A stage call takes nothing
struct QpidPool {
  double *rec, *M, *g, *g_joint;
  int64_t bytes;
};
inline QpidPool qpid_pool(void* base, int64_t stride, int na, int nv, int64_t B, bool stages, bool whole_body,
                          RegionLog* log = nullptr) {
  Carver c{static_cast<char*>(base), log};
  QpidPool L;
  L.rec = c.take<double>("rec", stages ? 0 : stride * B);
  L.M = c.take<double>("M", stages ? 0 : int64_t(na) * na * B);
  L.g = c.take<double>("g", stages ? 0 : int64_t(na) * B);
  L.g_joint = c.take<double>("g_joint", !stages && whole_body ? int64_t(nv) * B : 0);
  L.bytes = c.off;
  return L;
}

// pool, drc_osf_batch: M^-1 [nv*nv][B] and g [nv][B]
struct OsfPool {
  double *Minv, *g;
  int64_t bytes;
};
inline OsfPool osf_pool(void* base, int nv, int64_t B, RegionLog* log = nullptr) {
  Carver c{static_cast<char*>(base), log};
  OsfPool L;
  L.Minv = c.take<double>("Minv", int64_t(nv) * nv * B);
  L.g = c.take<double>("g", int64_t(nv) * B);
  L.bytes = c.off;
  return L;
}

// dyn_list, the dynamics launches with M^-1: the instances that need the
// serial COD, and their count
struct DynList {
  int32_t* list;
  int64_t bytes;
};
inline DynList dyn_list(void* base, int64_t B, RegionLog* log = nullptr) {
  Carver c{static_cast<char*>(base), log};
  DynList L;
  L.list = c.take<int32_t>("list", B + 1);
  L.bytes = c.off;
  return L;
}

// roll, drc_qpik_rollout_batch: one step's eta [na][B], unless the caller's
// qdot_traj takes it
struct RolloutScratch {
  double* eta;
  int64_t bytes;
};
inline RolloutScratch rollout_scratch(void* base, int na, int64_t B, bool qdot_traj, RegionLog* log = nullptr) {
  Carver c{static_cast<char*>(base), log};
  RolloutScratch L;
  L.eta = c.take<double>("eta", qdot_traj ? 0 : int64_t(na) * B);
  L.bytes = c.off;
  return L;
}

// roll, drc_qpik_reach_path_batch: one step's eta [na][B], then (stepwise) the
// stage outputs pose [12][B] and dist [1+nv][B] and the current targets
// [12][B], [6][B], then status [B], iters [B] and the segment counters [B]
struct ReachPathScratch {
  double *eta, *pose, *dist, *xt, *xdt;
  int32_t *status, *iters, *seg;
  int64_t bytes;
};
// (the regions, for the two layouts that hold them)
inline void take_reach_path(Carver& c, ReachPathScratch& L, int na, int nv, int64_t B, bool persistent) {
  L.eta = c.take<double>("eta", int64_t(na) * B);
  L.pose = c.take<double>("pose", persistent ? 0 : 12 * B);
  L.dist = c.take<double>("dist", persistent ? 0 : int64_t(1 + nv) * B);
  L.xt = c.take<double>("xt", persistent ? 0 : 12 * B);
  L.xdt = c.take<double>("xdt", persistent ? 0 : 6 * B);
  L.status = c.take<int32_t>("status", B);
  L.iters = c.take<int32_t>("iters", B);
  L.seg = c.take<int32_t>("seg", B);
  L.bytes = c.off;
}
inline ReachPathScratch reach_path_scratch(void* base, int na, int nv, int64_t B, bool persistent,
                                           RegionLog* log = nullptr) {
  Carver c{static_cast<char*>(base), log};
  ReachPathScratch L;
  take_reach_path(c, L, na, nv, B, persistent);
  return L;
}

// roll, drc_qpik_reach_batch, a reach path of one waypoint: reach path's, then
// wp [B], the waypoints_reached that the reach entry's caller does not have
struct ReachScratch : ReachPathScratch {
  int32_t* wp;
};
inline ReachScratch reach_scratch(void* base, int na, int nv, int64_t B, bool persistent, RegionLog* log = nullptr) {
  Carver c{static_cast<char*>(base), log};
  ReachScratch L;
  take_reach_path(c, L, na, nv, B, persistent);
  L.wp = c.take<int32_t>("wp", B);
  L.bytes = c.off;
  return L;
}

// seeds, drc_qpik_reach_seeds_batch, B = S T instances: the expanded targets
// [12][B], [6][B], the instances' finals [nv][B] twice, err [2][B], dist
// [1+nv][B], the per-target poses expanded [nobst][12][B] (ob_expand),
// (persistent) one step's eta [na][B]; then result, steps, status_last,
// iters_total [B], one step's status and iters [B] and the groups' words [T]
struct SeedsScratch {
  double *xt, *xdt, *qf, *vf, *err, *dist, *pose, *eta;
  int32_t *result, *steps, *status_last, *iters_total, *status, *iters;
  uint32_t* word;
  int64_t bytes;
};
inline SeedsScratch seeds_scratch(void* base, int na, int nv, int nobst, int64_t T, int S, bool persistent,
                                  bool ob_expand, RegionLog* log = nullptr) {
  Carver c{static_cast<char*>(base), log};
  const int64_t B = T * S;
  SeedsScratch L;
  L.xt = c.take<double>("xt", 12 * B);
  L.xdt = c.take<double>("xdt", 6 * B);
  L.qf = c.take<double>("qf", int64_t(nv) * B);
  L.vf = c.take<double>("vf", int64_t(nv) * B);
  L.err = c.take<double>("err", 2 * B);
  L.dist = c.take<double>("dist", int64_t(1 + nv) * B);
  L.pose = c.take<double>("pose", ob_expand ? int64_t(nobst) * 12 * B : 0);
  L.eta = c.take<double>("eta", persistent ? int64_t(na) * B : 0);
  L.result = c.take<int32_t>("result", B);
  L.steps = c.take<int32_t>("steps", B);
  L.status_last = c.take<int32_t>("status_last", B);
  L.iters_total = c.take<int32_t>("iters_total", B);
  L.status = c.take<int32_t>("status", B);
  L.iters = c.take<int32_t>("iters", B);
  L.word = c.take<uint32_t>("word", T);
  L.bytes = c.off;
  return L;
}

}  // namespace drc_amd
