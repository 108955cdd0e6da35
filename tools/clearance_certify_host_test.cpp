// Host harness of the certified path clearance: the fold of
// csrc/clearance_certify.hpp and the motion weights of model.cpp
// (build_motion_tables), compiled with the host compiler alone together with
// model.cpp and mesh.cpp (tests/test_clearance_certify_host.py).
//
//   <exe> model <urdf> <srdf or -> <n_slots> [k]
//       builds the model (k > 0: with the upper limit of joint k set to +inf
//       and the motion tables rebuilt), declares n_slots sphere slots (r = 0.1,
//       every moving link) when n_slots > 0, and prints
//         "nv ngeom npairs pair_ld motion_ld travel_mask unbounded"
//         ngeom lines "g parent type"
//         npairs lines "p a b"
//         nv lines of rho[j][0 .. ngeom), %a
//         nv lines of wt[j][0 .. npairs), %a
//       then, for n_slots > 0, "restored 1" if n = 0 gives the fresh model back
//       byte for byte (device image, pair table, motion tables), else "restored 0".
//
//   <exe> fold        (stdin, one walk per line; doubles as %la hex floats)
//       d_stop max_depth waypoints depth, then per segment
//       "travel_ok M d[0] .. d[2^depth]": the distances on the segment's grid of
//       2^depth steps (d[0] is used on segment 0 only); the sample k / 2^e is
//       entry k << (depth - e) and its pair is 1000 seg + that index.  A path
//       of one waypoint gives one pseudo-segment whose d[0] is its state.
//       stdout per walk: "result seg_stop t_stop d_min seg_min t_min pair_min
//       d_lower samples" (%a for doubles), then the evaluated samples
//       "seg:k/e" in order.
//
//   <exe> motion      (stdin, one case per line)
//       nv npairs |dq_0| .. |dq_{nv-1}| then wt [nv][npairs] row by row:
//       prints M = max_p sum_i wt[i][p] |dq_i| by cert_motion_term, %a.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../dyros_robot_controller_amd/csrc/clearance_certify.hpp"
#include "../dyros_robot_controller_amd/csrc/model.hpp"

using namespace drc_amd;

static bool same(const HostModel& a, const HostModel& b) {
  return std::memcmp(&a.dev, &b.dev, sizeof(DevModel)) == 0 && a.pair_tab == b.pair_tab &&
         a.motion_rho == b.motion_rho && a.motion_wt == b.motion_wt && a.motion_unbounded == b.motion_unbounded &&
         a.geom_names == b.geom_names;
}

static int model_main(int argc, char** argv) {
  if (argc < 5) return 2;
  HostModel hm;
  std::string err;
  const std::string srdf = std::strcmp(argv[3], "-") ? argv[3] : "";
  if (int rc = build_model_from_urdf(argv[2], srdf, "", &hm, &err)) {
    std::fprintf(stderr, "%s\n", err.c_str());
    return rc;
  }
  if (const int k = argc > 5 ? std::atoi(argv[5]) : 0) {  // (the URDF reader takes finite numbers only)
    if (k < 1 || k > hm.dev.nv) return 2;
    hm.dev.upper[k - 1] = INFINITY;
    build_motion_tables(&hm);
  }
  const HostModel fresh = hm;
  const int n_slots = std::atoi(argv[4]);
  if (n_slots > 0) {
    std::vector<int> type(static_cast<size_t>(n_slots), static_cast<int>(kSphere));
    std::vector<double> param(static_cast<size_t>(3 * n_slots), 0.1);
    if (int rc = set_obstacles(&hm, n_slots, type.data(), param.data(), nullptr, 0, &err)) {
      std::fprintf(stderr, "%s\n", err.c_str());
      return rc;
    }
  }
  const DevModel& m = hm.dev;
  std::printf("%d %d %d %d %d %u %d\n", m.nv, m.ngeom, m.npairs, m.pair_ld, m.motion_ld, m.travel_mask,
              hm.motion_unbounded ? 1 : 0);
  for (int g = 0; g < m.ngeom; ++g) std::printf("%d %d %d\n", g, m.gparent[g], m.gtype[g]);
  for (int p = 0; p < m.npairs; ++p) std::printf("%d %d %d\n", p, m.pair_a[p], m.pair_b[p]);
  for (int j = 0; j < m.nv; ++j) {
    for (int g = 0; g < m.ngeom; ++g) std::printf("%a ", hm.motion_rho[static_cast<size_t>(j) * m.ngeom + g]);
    std::printf("\n");
  }
  for (int j = 0; j < m.nv; ++j) {
    for (int p = 0; p < m.npairs; ++p) std::printf("%a ", hm.motion_wt[static_cast<size_t>(j) * m.motion_ld + p]);
    std::printf("\n");
  }
  if (n_slots > 0) {
    if (int rc = set_obstacles(&hm, 0, nullptr, nullptr, nullptr, 0, &err)) return rc;
    std::printf("restored %d\n", same(hm, fresh) ? 1 : 0);
  }
  return 0;
}

static int fold_main() {
  double d_stop;
  int max_depth, W, depth;
  while (std::scanf("%la %d %d %d", &d_stop, &max_depth, &W, &depth) == 4) {
    const int nseg = W > 1 ? W - 1 : 1, n = (1 << depth) + 1;
    std::vector<int> ok(static_cast<size_t>(nseg));
    std::vector<double> M(static_cast<size_t>(nseg)), d(static_cast<size_t>(nseg) * n);
    for (int s = 0; s < nseg; ++s) {
      if (std::scanf("%d %la", &ok[s], &M[s]) != 2) return 1;
      for (int i = 0; i < n; ++i)
        if (std::scanf("%la", &d[static_cast<size_t>(s) * n + i]) != 1) return 1;
    }
    CertFold f;
    CertStackArray stack{};
    std::string trace;
    int seg = 0;  // the segment that starts next
    double Mseg = 0.0;
    for (;;) {
      if (f.ev_e > depth) return 1;  // (the case's grid is coarser than its max_depth)
      const int sseg = f.seg, idx = f.ev_k << (depth - f.ev_e);
      trace += " " + std::to_string(sseg) + ":" + std::to_string(f.ev_k) + "/" + std::to_string(f.ev_e);
      int next = cert_step(&f, stack, d[static_cast<size_t>(sseg) * n + idx], 1000 * sseg + idx, d_stop, Mseg, max_depth);
      if (next == kCertStop) break;
      if (next == kCertSegEnd) {
        if (seg + 1 >= W) break;
        Mseg = M[seg];
        next = cert_segment(&f, seg, ok[seg] != 0);
        if (next == kCertStop) break;
        ++seg;
      }
    }
    std::printf("%d %d %a %a %d %a %d %a %d%s\n", f.result, f.seg_stop, f.t_stop, f.d_min, f.seg_min, f.t_min, f.pair_min,
                f.d_lower, f.samples, trace.c_str());
  }
  return 0;
}

static int motion_main() {
  int nv, np;
  while (std::scanf("%d %d", &nv, &np) == 2) {
    std::vector<double> adq(static_cast<size_t>(nv)), wt(static_cast<size_t>(nv) * np);
    for (double& x : adq)
      if (std::scanf("%la", &x) != 1) return 1;
    for (double& x : wt)
      if (std::scanf("%la", &x) != 1) return 1;
    double m = 0.0;
    for (int p = 0; p < np; ++p) {
      double s = 0.0;
      for (int i = 0; i < nv; ++i) s = cert_motion_term(s, wt[static_cast<size_t>(i) * np + p], adq[i]);
      m = s > m ? s : m;
    }
    std::printf("%a\n", m);
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc >= 2 && !std::strcmp(argv[1], "model")) return model_main(argc, argv);
  if (argc >= 2 && !std::strcmp(argv[1], "fold")) return fold_main();
  if (argc >= 2 && !std::strcmp(argv[1], "motion")) return motion_main();
  return 2;
}
