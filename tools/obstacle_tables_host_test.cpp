// Host check of the obstacle slots' bookkeeping (model.cpp set_obstacles):
// counts, every pair record against the plain gather, the type-class order,
// n = 0 restoring the tables byte for byte, the limits and the refusals.
// Stand-alone: compiled with model.cpp and mesh.cpp, no GPU
// (tests/test_obstacle_tables_host.py).
//   usage: obstacle_tables_host_test URDF SRDF|- LINKS|-   (triples of arguments;
//          LINKS: comma-separated link names, "-" for every moving link)
// Prints one line per model,
//   "ok <ngeom0> <npairs0> <ngeom> <npairs> <paired geometries>",
// "ok-hull" for a model with collision meshes (obstacles refused), or the
// first mismatch; exit status 1 on any failure.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../dyros_robot_controller_amd/csrc/model.hpp"
#include "../include/drc_amd.h"

using namespace drc_amd;

static int fail(const char* what, int a, int b) {
  std::printf("MISMATCH %s at %d %d\n", what, a, b);
  return 1;
}

static int check_record(const HostModel& hm, int rec, int p) {
  const DevModel& m = hm.dev;
  const double* t = hm.pair_tab.data() + rec;
  const int ld = m.pair_ld, ga = m.pair_a[p], gb = m.pair_b[p];
  uint64_t meta;
  std::memcpy(&meta, t + kPairMeta * ld, sizeof(meta));
  if (static_cast<int>(meta & 0xffff) != p) return fail("pair index", rec, p);
  if (static_cast<int>((meta >> 16) & 0xff) != ga || static_cast<int>((meta >> 24) & 0xff) != gb)
    return fail("geometry ids", rec, p);
  if (static_cast<int>((meta >> 32) & 0xf) != m.gtype[ga] || static_cast<int>((meta >> 36) & 0xf) != m.gtype[gb])
    return fail("geometry types", rec, p);
  if (meta >> 40) return fail("meta high bits", rec, p);
  for (int k = 0; k < 3; ++k)
    if (t[(kPairParamA + k) * ld] != m.gparam[ga][k] || t[(kPairParamB + k) * ld] != m.gparam[gb][k])
      return fail("gparam", rec, k);
  if (t[kPairBoundA * ld] != m.gbound[ga] || t[kPairBoundB * ld] != m.gbound[gb]) return fail("gbound", rec, p);
  return 0;
}

static int pair_class(const DevModel& m, int p) {
  int ta = m.gtype[m.pair_a[p]], tb = m.gtype[m.pair_b[p]];
  if (ta > tb) std::swap(ta, tb);
  return tb == kHalfSpace ? 7 : (tb == kMesh ? 6 : (ta == 0 ? tb : (ta == 1 ? 2 + tb : 5)));
}

static bool same(const HostModel& a, const HostModel& b) {
  return std::memcmp(&a.dev, &b.dev, sizeof(DevModel)) == 0 && a.pair_tab == b.pair_tab &&
         a.geom_names == b.geom_names && a.geom_link == b.geom_link && a.base_pairs == b.base_pairs;
}

static int check_model(HostModel& hm, const std::vector<std::string>& links) {
  const HostModel fresh = hm;
  const int g0 = hm.dev.ngeom, p0 = hm.dev.npairs;
  std::string err;
  std::vector<const char*> lk;
  for (const std::string& s : links) lk.push_back(s.c_str());
  const char* const* lp = lk.empty() ? nullptr : lk.data();
  const int nl = static_cast<int>(lk.size());
  const int type[4] = {kSphere, kBox, kCylinder, kHalfSpace};
  const double prm[12] = {0.08, 0, 0, 0.15, 0.2, 0.01, 0.05, 0.25, 0, 7, 7, 7 /* ignored */};
  if (hm.has_mesh()) {  // hull models refuse obstacles, and n = 0 is a no-op
    if (set_obstacles(&hm, 4, type, prm, lp, nl, &err) != DRC_ERR_UNSUPPORTED || err.empty())
      return fail("hull model not refused", 0, 0);
    if (!same(hm, fresh)) return fail("refusal changed the hull model", 0, 0);
    if (set_obstacles(&hm, 0, nullptr, nullptr, nullptr, 0, &err) != DRC_OK) return fail("n = 0 on a hull model", 0, 0);
    if (!same(hm, fresh)) return fail("n = 0 changed the hull model", 0, 0);
    std::printf("ok-hull\n");
    return 0;
  }
  // the geometries the links own
  std::vector<int> with;
  for (int g = 0; g < g0; ++g) {
    bool in = links.empty() ? hm.dev.gparent[g] > 0 : false;
    for (const std::string& s : links) in = in || hm.geom_link[g] == s;
    if (in) with.push_back(g);
  }
  const int nw = static_cast<int>(with.size());
  if (int rc = set_obstacles(&hm, 4, type, prm, lp, nl, &err)) {
    std::printf("set_obstacles failed %d %s\n", rc, err.c_str());
    return 1;
  }
  const DevModel& m = hm.dev;
  if (m.ngeom != g0 + 4 || m.nobst != 4 || m.obst0 != g0) return fail("geometry count", m.ngeom, g0 + 4);
  if (m.npairs != p0 + 4 * nw) return fail("pair count", m.npairs, p0 + 4 * nw);
  if (static_cast<int>(hm.geom_names.size()) != m.ngeom) return fail("geom_names", m.ngeom, 0);
  for (int p = 0; p < p0; ++p)
    if (m.pair_a[p] != fresh.dev.pair_a[p] || m.pair_b[p] != fresh.dev.pair_b[p]) return fail("self pair moved", p, 0);
  for (int i = 0; i < 4; ++i) {
    const int g = g0 + i;
    static const double eye[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
    if (m.gparent[g] != 0 || m.gtype[g] != type[i] || std::memcmp(m.gplace[g], eye, sizeof(eye)))
      return fail("slot geometry", g, 0);
    for (int k = 0; k < 3; ++k) {
      const int np = type[i] == kSphere ? 1 : (type[i] == kCylinder ? 2 : (type[i] == kBox ? 3 : 0));
      if (m.gparam[g][k] != (k < np ? prm[3 * i + k] : 0.0)) return fail("slot parameters", g, k);
    }
    for (int k = 0; k < nw; ++k) {  // obstacle-major, the link geometries in index order
      const int p = p0 + i * nw + k;
      if (m.pair_a[p] != with[k] || m.pair_b[p] != g) return fail("obstacle pair", p, g);
    }
  }
  // pair_order: a permutation, classes ascending (half-space pairs last), every record the plain gather
  if (m.pair_ld % 64 || m.pair_ld < m.npairs) return fail("pair_ld", m.pair_ld, m.npairs);
  if (hm.pair_tab.size() < static_cast<size_t>(kPairFields) * m.pair_ld) return fail("pair_tab size", 0, 0);
  std::vector<int> seen(m.npairs, 0);
  int ncand = 0;
  for (int sl = 0; sl < m.npairs; ++sl) {
    const int p = m.pair_order[sl];
    if (p < 0 || p >= m.npairs || seen[p]++) return fail("pair_order not a permutation", sl, p);
    if (sl && pair_class(m, m.pair_order[sl - 1]) > pair_class(m, p)) return fail("class order", sl, p);
    if (sl && pair_class(m, m.pair_order[sl - 1]) == pair_class(m, p) && m.pair_order[sl - 1] > p)
      return fail("pair order within a class", sl, p);
    if (m.slot_a[sl] != m.pair_a[p] || m.slot_b[sl] != m.pair_b[p]) return fail("slot_a / slot_b", sl, 0);
    if (check_record(hm, sl, p)) return 1;
  }
  for (int p = 0; p < m.npairs; ++p) {
    const bool gjk = m.gtype[m.pair_a[p]] != kSphere && m.gtype[m.pair_b[p]] != kSphere && pair_class(m, p) != 7;
    if (gjk != (m.cand_slot[p] >= 0 || (gjk && ncand >= kMaxCandSlots))) return fail("cand_slot", p, m.cand_slot[p]);
    ncand += gjk;
  }
  if (ncand != m.ncand_slots) return fail("ncand_slots", ncand, m.ncand_slots);
  const int ngeom = m.ngeom, npairs = m.npairs;
  // refusals leave the model as it is
  const HostModel with4 = hm;
  const int mesh_type[1] = {kMesh}, bad_type[1] = {9};
  const double one[3] = {0.1, 0.1, 0.1}, neg[3] = {-0.1, 0, 0};
  const char* unknown[1] = {"no_such_link"};
  if (set_obstacles(&hm, 1, mesh_type, one, lp, nl, &err) != DRC_ERR_UNSUPPORTED) return fail("mesh obstacle", 0, 0);
  if (set_obstacles(&hm, 1, bad_type, one, lp, nl, &err) != DRC_ERR_INVALID_ARGUMENT) return fail("bad type", 0, 0);
  if (set_obstacles(&hm, 1, type, neg, lp, nl, &err) != DRC_ERR_INVALID_ARGUMENT) return fail("bad radius", 0, 0);
  if (set_obstacles(&hm, 1, type, one, unknown, 1, &err) != DRC_ERR_UNKNOWN_LINK) return fail("unknown link", 0, 0);
  if (set_obstacles(&hm, -1, type, one, lp, nl, &err) != DRC_ERR_INVALID_ARGUMENT) return fail("negative n", 0, 0);
  {
    std::vector<int> ty(kMaxGeoms + 1, kSphere);
    std::vector<double> pr(3 * (kMaxGeoms + 1), 0.05);
    const int over = kMaxGeoms - g0 + 1;  // one geometry too many
    if (set_obstacles(&hm, over, ty.data(), pr.data(), lp, nl, &err) != DRC_ERR_UNSUPPORTED)
      return fail("geometry limit", over, 0);
    // the most slots that fit the geometry limit: refused exactly when the pairs exceed theirs
    const int most = kMaxGeoms - g0;
    const int rc = set_obstacles(&hm, most, ty.data(), pr.data(), lp, nl, &err);
    const bool fits = p0 + most * nw <= kMaxPairs;
    if (rc != (fits ? DRC_OK : DRC_ERR_UNSUPPORTED)) return fail("pair limit", rc, p0 + most * nw);
    if (fits) {
      if (hm.dev.ngeom != kMaxGeoms || hm.dev.npairs != p0 + most * nw) return fail("full model counts", 0, 0);
      for (int sl = 0; sl < hm.dev.npairs; ++sl)
        if (check_record(hm, sl, hm.dev.pair_order[sl])) return 1;
      if (set_obstacles(&hm, 4, type, prm, lp, nl, &err)) return fail("replacing the slots", 0, 0);
    }
  }
  if (err.empty()) return fail("refusal without a message", 0, 0);
  if (!same(hm, with4)) return fail("refusal / replacement changed the model", 0, 0);
  // n = 0: byte for byte the fresh build
  if (set_obstacles(&hm, 0, nullptr, nullptr, nullptr, 0, &err) != DRC_OK) return fail("n = 0", 0, 0);
  if (!same(hm, fresh)) return fail("n = 0 does not restore the model", 0, 0);
  std::printf("ok %d %d %d %d %d\n", g0, p0, ngeom, npairs, nw);
  return 0;
}

int main(int argc, char** argv) {
  int rc = 0;
  for (int i = 1; i + 2 < argc; i += 3) {
    HostModel hm;
    std::string err;
    const std::string srdf = std::strcmp(argv[i + 1], "-") ? argv[i + 1] : "";
    const int r = build_model_from_urdf(argv[i], srdf, "", &hm, &err);
    if (r) {
      std::printf("BUILD FAILED %d %s\n", r, err.c_str());
      rc = 1;
      continue;
    }
    std::vector<std::string> links;
    if (std::strcmp(argv[i + 2], "-")) {
      std::string s = argv[i + 2];
      size_t a = 0;
      while (a <= s.size()) {
        const size_t b = s.find(',', a);
        links.push_back(s.substr(a, b == std::string::npos ? std::string::npos : b - a));
        if (b == std::string::npos) break;
        a = b + 1;
      }
    }
    rc |= check_model(hm, links);
  }
  return rc;
}
