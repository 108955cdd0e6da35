// csrc/call_plan.hpp with the host compiler: answers the queries that
// tests/test_call_plan_host.py writes to standard input, one per line, with one
// line each; the expected values stand in the test.  A query is
//   [knob=value ...] plan|sub|pers B stages fused lane_stage chunks caller_order
//                    kind nv ncand_slots has_mesh slots qp_compiled [...]
//   plan               -> "plan lane fuse auto_order use_caller_order S"
//   sub  ... c         -> "sub b0 Bc xcd_map grid_task grid_qp grid_fused"
//   pers ... max_b family -> "pers 0|1"
//   pers ... max_b serves_hulls serves_slots -> the same, asked as before the
//                      families had names: of the closed-loop family that has
//                      exactly the Mesh build and the Obst build so stated
// and, on the stage builds alone,
//   build has_mesh slots twists -> "build plain|mesh|obst|rate", or "build none"
//   has family build            -> "has 0|1"
// and, on the path-clearance grid (clearance_grid),
//   [grid_clear=value] clear B  -> "clear grid"
// family: problem0 problem1 problem2 fused rollout reach reach_path reach_seeds
// clearance.
// Knobs: fuse_max, order_min, order_max, min_subbatch, grid_task, grid_qp,
// grid_fused, grid_clear (default: PlanKnobs'), qp_group (64), max_cand (16) and twists (0:
// the call carries obstacle twists).
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../dyros_robot_controller_amd/csrc/call_plan.hpp"

using namespace drc_amd;

static const char* const kBuildName[kStageBuilds] = {"plain", "mesh", "obst", "rate"};
static const char* const kFamilyName[kStageFamilies] = {"problem0", "problem1",   "problem2",    "fused",    "rollout",
                                                        "reach",    "reach_path", "reach_seeds", "clearance"};
static int index_of(const char* const* names, int n, const std::string& s) {
  for (int i = 0; i < n; ++i)
    if (s == names[i]) return i;
  return -1;
}

static bool answer(const std::string& line, std::ostream& out) {
  std::istringstream is(line);
  std::vector<std::string> tok;
  for (std::string t; is >> t;) tok.push_back(t);
  PlanIn in;
  in.qp_group = 64;
  in.max_cand_slots = 16;
  size_t a = 0;
  for (; a < tok.size() && tok[a].find('=') != std::string::npos; ++a) {
    const std::string k = tok[a].substr(0, tok[a].find('='));
    const long long v = std::stoll(tok[a].substr(tok[a].find('=') + 1));
    if (k == "fuse_max") in.knobs.fuse_max = v;
    else if (k == "order_min") in.knobs.order_min = v;
    else if (k == "order_max") in.knobs.order_max = v;
    else if (k == "min_subbatch") in.knobs.min_subbatch = v;
    else if (k == "grid_task") in.knobs.grid_task = v;
    else if (k == "grid_qp") in.knobs.grid_qp = v;
    else if (k == "grid_fused") in.knobs.grid_fused = v;
    else if (k == "grid_clear") in.knobs.grid_clear = v;
    else if (k == "qp_group") in.qp_group = static_cast<int>(v);
    else if (k == "max_cand") in.max_cand_slots = static_cast<int>(v);
    else if (k == "twists") in.twists = v != 0;
    else return false;
  }
  if (a < tok.size() && tok[a] == "build" && tok.size() == a + 4) {
    const bool mesh = tok[a + 1] != "0", slots = tok[a + 2] != "0", twists = tok[a + 3] != "0";
    out << "build "
        << (stage_build_exists(mesh, slots) ? kBuildName[static_cast<int>(stage_build(mesh, slots, twists))] : "none")
        << '\n';
    return true;
  }
  if (a < tok.size() && tok[a] == "has" && tok.size() == a + 3) {
    const int f = index_of(kFamilyName, kStageFamilies, tok[a + 1]), b = index_of(kBuildName, kStageBuilds, tok[a + 2]);
    if (f < 0 || b < 0) return false;
    out << "has " << (has_build(static_cast<StageFamily>(f), static_cast<StageBuild>(b)) ? 1 : 0) << '\n';
    return true;
  }
  if (a < tok.size() && tok[a] == "clear" && tok.size() == a + 2) {
    out << "clear " << clearance_grid(std::stoll(tok[a + 1]), in.knobs) << '\n';
    return true;
  }
  if (tok.size() < a + 13) return false;
  const std::string what = tok[a++];
  int family = -1;
  if (what == "pers" && index_of(kFamilyName, kStageFamilies, tok.back()) >= 0) {  // the last token names the family
    family = index_of(kFamilyName, kStageFamilies, tok.back());
    tok.pop_back();
  }
  std::vector<long long> v;
  for (; a < tok.size(); ++a) v.push_back(std::stoll(tok[a]));
  in.B = v[0];
  in.stages = static_cast<int>(v[1]);
  in.fused = static_cast<int>(v[2]);
  in.lane_stage = static_cast<int>(v[3]);
  in.chunks = static_cast<int>(v[4]);
  in.caller_order = v[5] != 0;
  in.kind = static_cast<int>(v[6]);
  in.nv = static_cast<int>(v[7]);
  in.ncand_slots = static_cast<int>(v[8]);
  in.has_mesh = v[9] != 0;
  in.slots = v[10] != 0;
  in.qp_compiled = v[11] != 0;
  const CallPlan p = plan_call(in);
  if (what == "plan" && v.size() == 12) {
    out << "plan " << p.lane << ' ' << p.fuse << ' ' << p.auto_order << ' ' << p.use_caller_order << ' ' << p.S << '\n';
  } else if (what == "sub" && v.size() == 13 && v[12] >= 0 && v[12] < p.S) {
    const SubBatch s = plan_sub_batch(in, p, static_cast<int>(v[12]));
    out << "sub " << s.b0 << ' ' << s.Bc << ' ' << s.xcd_map << ' ' << s.grid_task << ' ' << s.grid_qp << ' '
        << s.grid_fused << '\n';
  } else if (what == "pers" && family < 0 && v.size() == 15) {
    for (int f = static_cast<int>(StageFamily::Rollout); f <= static_cast<int>(StageFamily::ReachSeeds) && family < 0; ++f)
      if (has_build(static_cast<StageFamily>(f), StageBuild::Mesh) == (v[13] != 0) &&
          has_build(static_cast<StageFamily>(f), StageBuild::Obst) == (v[14] != 0))
        family = f;
    if (family < 0) return false;
    out << "pers " << (persistent_path(in, v[12], static_cast<StageFamily>(family)) ? 1 : 0) << '\n';
  } else if (what == "pers" && family >= 0 && v.size() == 13) {
    out << "pers " << (persistent_path(in, v[12], static_cast<StageFamily>(family)) ? 1 : 0) << '\n';
  } else {
    return false;
  }
  return true;
}

int main() {
  for (std::string line; std::getline(std::cin, line);)
    if (!answer(line, std::cout)) {
      std::cout << "BAD QUERY " << line << '\n';
      return 2;
    }
  return 0;
}
