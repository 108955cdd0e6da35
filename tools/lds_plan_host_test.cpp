// csrc/lds_plan.hpp with the host compiler: lays out every LDS plan the
// library can ask for on the given models and prints the offsets, the regions
// with their groups (the plan functions' trace) and the three small layout
// functions; tests/test_lds_plan_host.py checks the sharing rules on the
// output.  Stand-alone: compiled with model.cpp and mesh.cpp, no GPU.
//   usage: lds_plan_host_test NAME URDF SRDF|- MOBILE|- COMPILED ...   (five arguments per model)
//          URDF "@bounds": no file, a model at the bounds (nv 16, 64 geometries, 1024 pairs)
//          MOBILE: n_wheel,virtual_start,mani_start,mobi_start,act_mani_start,act_mobi_start
//                  (what drc_model_create_mobile_manipulator sets), "-" for a manipulator
//          COMPILED: 1 when the QPIK QP shape has a compile-time instantiation (qp_compiled())
// Prints, per model,
//   "model NAME nv ngeom npairs kind"
//   "epa fn out nv_field narrow wide"   (EpaPoly: offsets of fn, out[] and nv, the two footprints; doubles)
// per plan
//   "plan NAME/VARIANT result=R field=value ..."   (R: LdsPlanResult; VARIANT: task_narrow_qpik, qp_qpid, ...)
//   "region NAME/VARIANT name offset length group" for every region taken
// and per QPIK task plan, with the QPIK QP plan,
//   "fused NAME/VARIANT rec_offset=.. rec_len=.. fused_lds=.. state=.."
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../dyros_robot_controller_amd/csrc/lds_plan.hpp"
#include "../dyros_robot_controller_amd/csrc/model.hpp"

using namespace drc_amd;

// One plan as api.cpp's make_kparams asks for it (task: a stage call)
static int lay(const DevModel& M, int problem, int cf, bool task, bool wide, bool compiled, KParams* k, PlanTrace* tr) {
  std::memset(k, 0, sizeof(*k));
  k->problem = problem;
  k->cf = cf;
  if (int r = plan_dims(M, k)) return r;
  return task ? plan_task(M, k, wide, tr) : plan_qp(M, k, compiled, tr);
}

static void print_plan(const std::string& name, int rc, const KParams& k, bool task, const PlanTrace& tr) {
  std::printf("plan %s result=%d", name.c_str(), rc);
#define F(f) std::printf(" " #f "=%d", k.f)
  F(nv); F(nx); F(ng); F(np); F(na); F(m); F(narm); F(c0);
  F(rJac); F(rMan); F(rDist); F(rXdd); F(rQ); F(rLen); F(rQd); F(rBias); F(rMgd); F(rDgd);
  if (!task) {  // the polish caps belong to the QP plans (qp_solver.hpp reads them from the QP kernel's parameters)
    F(nbuf); F(ncap);
  }
  F(oP); F(oG); F(oQ); F(oAB); F(oL); F(oU); F(oD); F(oE); F(oRho); F(oX); F(oZ); F(oY); F(oDY); F(oXT); F(oZT);
  F(oT1); F(oT2); F(oRed); F(oSc); F(oDi); F(oEi); F(oBc); F(oU0); F(oHi);
  F(kT); F(kZ); F(kTe); F(kJ); F(kTg); F(kq); F(kqd); F(kA6); F(kAi); F(kW); F(kPart); F(kPd); F(kPf); F(kCand);
  F(kxdd); F(kmg); F(kdg); F(kJt); F(kSv); F(kScr); F(kEpa); F(kPp); F(kOvl);
  F(kJd); F(kDa); F(kVf); F(kX6); F(kBias); F(kMq); F(kGq); F(kGdv); F(cf); F(kCf); F(lds_doubles);
#undef F
  std::printf("\n");
  for (int i = 0; i < tr.n; ++i)
    std::printf("region %s %s %d %d %d\n", name.c_str(), tr.r[i].name, tr.r[i].off, tr.r[i].len, tr.r[i].group);
}

static void run_model(const std::string& name, const DevModel& M, bool compiled) {
  std::printf("model %s %d %d %d %d\n", name.c_str(), M.nv, M.ngeom, M.npairs, M.kind);
  std::printf("epa %d %d %d %d %d\n", kEpaFnDoubles, kEpaOutDoubles, static_cast<int>(offsetof(EpaPoly, nv) / 8),
              kEpaDoubles, kEpaWideDoubles);
  static const struct { const char* tag; int problem, cf; } kinds[5] = {
      {"qpik", 0, 0}, {"qpid", 1, 0}, {"cf1", 2, 1}, {"cf2", 2, 2}, {"cf3", 2, 3}};
  KParams kq[2];
  int rq[2];
  for (int p = 0; p < 2; ++p) {
    PlanTrace tr;
    rq[p] = lay(M, p, 0, false, false, compiled, &kq[p], &tr);
    print_plan(name + "/qp_" + kinds[p].tag, rq[p], kq[p], false, tr);
  }
  for (int wide = 0; wide < 2; ++wide)
    for (const auto& kd : kinds) {
      PlanTrace tr;
      KParams kt;
      const std::string v = name + "/task_" + (wide ? "wide_" : "narrow_") + kd.tag;
      const int rc = lay(M, kd.problem, kd.cf, true, wide != 0, compiled, &kt, &tr);
      print_plan(v, rc, kt, true, tr);
      if (kd.problem == 0 && rc == kPlanOk && rq[0] == kPlanOk)
        std::printf("fused %s rec_offset=%d rec_len=%d fused_lds=%d state=%d\n", v.c_str(), fused_rec_offset(kt, kq[0]),
                    (kt.rLen + 1) & ~1, fused_lds_doubles(kt, kq[0]), rollout_state_doubles(kt, kq[0]));
    }
}

int main(int argc, char** argv) {
  if ((argc - 1) % 5) {
    std::printf("BAD ARGUMENTS\n");
    return 2;
  }
  for (int i = 1; i + 4 < argc; i += 5) {
    HostModel hm;
    DevModel& d = hm.dev;
    if (!std::strcmp(argv[i + 1], "@bounds")) {
      d.nv = kMaxJoints;
      d.ngeom = kMaxGeoms;
      d.npairs = kMaxPairs;
    } else {
      std::string err;
      const std::string srdf = std::strcmp(argv[i + 2], "-") ? argv[i + 2] : "";
      if (int r = build_model_from_urdf(argv[i + 1], srdf, "", &hm, &err)) {
        std::printf("BUILD FAILED %s %d %s\n", argv[i], r, err.c_str());
        return 1;
      }
    }
    if (std::strcmp(argv[i + 3], "-")) {  // drc_model_create_mobile_manipulator
      int W, vs, ms, ws, am, aw;
      if (std::sscanf(argv[i + 3], "%d,%d,%d,%d,%d,%d", &W, &vs, &ms, &ws, &am, &aw) != 6) {
        std::printf("BAD MOBILE %s\n", argv[i + 3]);
        return 2;
      }
      d.kind = 1;
      d.n_wheel = W;
      d.n_arm = d.nv - (3 + W);
      d.virtual_start = vs;
      d.mani_start = ms;
      d.mobi_start = ws;
      d.act_mani_start = am;
      d.act_mobi_start = aw;
    }
    run_model(argv[i], d, std::atoi(argv[i + 4]) != 0);
  }
  return 0;
}
