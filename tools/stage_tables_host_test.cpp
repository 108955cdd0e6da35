// Host check of the task stage's model tables (model.cpp build_stage_tables):
// every per-slot record against the gather it replaces
// (pair_order -> pair_a / pair_b -> gtype / gparam / gbound), the joint masks
// against jtype / anc.  Stand-alone: compiled with model.cpp and
// mesh.cpp, no GPU (tests/test_stage_tables_host.py).
//   usage: stage_tables_host_test URDF [SRDF|-] ...   (pairs of arguments)
// Prints one line per model, "ok <nv> <ngeom> <npairs>", or the first
// mismatch; exit status 1 on any failure.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>

#include "../dyros_robot_controller_amd/csrc/model.hpp"

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

static int check_model(const HostModel& hm) {
  const DevModel& m = hm.dev;
  // masks
  for (int j = 1; j <= m.nv; ++j)
    if (((m.rev_mask >> (j - 1)) & 1u) != (m.jtype[j] == kRevolute ? 1u : 0u)) return fail("rev_mask", j, 0);
  if (m.nv < 32 && (m.rev_mask >> m.nv)) return fail("rev_mask beyond nv", m.nv, 0);
  for (int j = 1; j <= kMaxJoints; ++j)
    for (int k = 1; k <= kMaxJoints; ++k) {
      const int bit = 16 * (j - 1) + (k - 1);
      const bool got = (m.anc_bits[bit >> 6] >> (bit & 63)) & 1u;
      const bool want = j <= m.nv && k <= m.nv && (m.anc[j] & (1u << (k - 1)));
      if (got != want) return fail("anc_bits", j, k);
    }
  // records
  if (m.pair_ld % 64 || m.pair_ld < m.npairs) return fail("pair_ld", m.pair_ld, m.npairs);
  if (hm.pair_tab.size() < static_cast<size_t>(kPairFields) * m.pair_ld) return fail("pair_tab size", 0, 0);
  for (int sl = 0; sl < m.npairs; ++sl) {
    if (m.slot_a[sl] != m.pair_a[m.pair_order[sl]] || m.slot_b[sl] != m.pair_b[m.pair_order[sl]])
      return fail("slot_a / slot_b", sl, 0);
    if (check_record(hm, sl, m.pair_order[sl])) return 1;
  }
  std::printf("ok %d %d %d\n", m.nv, m.ngeom, m.npairs);
  return 0;
}

int main(int argc, char** argv) {
  int rc = 0;
  for (int i = 1; i + 1 < argc; i += 2) {
    HostModel hm;
    std::string err;
    const std::string srdf = std::strcmp(argv[i + 1], "-") ? argv[i + 1] : "";
    const int r = build_model_from_urdf(argv[i], srdf, "", &hm, &err);
    if (r) {
      std::printf("BUILD FAILED %d %s\n", r, err.c_str());
      rc = 1;
      continue;
    }
    rc |= check_model(hm);
  }
  return rc;
}
