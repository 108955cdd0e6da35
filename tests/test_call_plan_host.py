"""csrc/call_plan.hpp -- the dispatch plan of a QPIK call and the rule that
picks a closed-loop entry's persistent kernel from the table of stage builds
-- compiled with the host
compiler (tools/call_plan_host_test.cpp).  The expected values below are
written out from the rules as api.cpp documented them before the plan had a
header of its own (thresholds: DRC_FUSE_MAX 16 384, DRC_ORDER_MIN / _MAX 2 049
/ 8 192, DRC_MIN_SUBBATCH 4 096, four sub-batches only of >= 16 384 instances
each, DRC_GRID_TASK / _QP / _FUSED 1 024 / 4 096 / 2 048, the XCD-aware order
from 16 384 instances on); nothing here computes them from a second copy of
the code."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.environ.get("CXX", "g++")

FIELDS = ("B", "stages", "fused", "lane_stage", "chunks", "caller_order", "kind", "nv", "ncand", "has_mesh", "slots",
          "compiled")
# an FR3-like manipulator, fusion off, the default concurrency
BASE = dict(B=0, stages=0, fused=0, lane_stage=0, chunks=4, caller_order=0, kind=0, nv=7, ncand=8, has_mesh=0,
            slots=0, compiled=1)
PLAN_OUT = ("lane", "fuse", "auto_order", "use_caller_order", "S")
SUB_OUT = ("b0", "Bc", "xcd_map", "grid_task", "grid_qp", "grid_fused")

CASES = {}


def case(name, what, expect, extra=(), knobs=(), **kw):
    assert name not in CASES and set(kw) <= set(BASE), name
    f = dict(BASE, **kw)
    line = " ".join(list(knobs) + [what] + [str(f[k]) for k in FIELDS] + [str(x) for x in extra])
    CASES[name] = (line, what, expect)


def raw(name, line, what, expect):
    """A query on the stage builds alone: no call behind it."""
    assert name not in CASES, name
    CASES[name] = (line, what, expect)


# ---- sub-batch count: chunks = 4, default knobs, not fused
for B, S in ((8191, 1), (8192, 2), (12287, 2), (12288, 3), (16384, 3), (65535, 3), (65536, 4)):
    case("count_%d" % B, "plan", dict(S=S, fuse=0), B=B)
case("count_six_chunks", "plan", dict(S=6), B=98304, chunks=6)
case("count_six_chunks_below", "plan", dict(S=5), B=98303, chunks=6)   # 98 303 / 6 < 16 384; / 5 = 19 660
case("count_one_chunk", "plan", dict(S=1), B=65536, chunks=1)
case("count_stage_call", "plan", dict(S=1), B=65536, stages=1)
case("count_fused_call", "plan", dict(S=1, fuse=1), B=16384, fused=1)
case("count_min_subbatch_knob", "plan", dict(S=3), B=3000, knobs=["min_subbatch=1000"])

# ---- fusion
case("fuse_at_max", "plan", dict(fuse=1, S=1), B=16384, fused=1)
case("fuse_above_max", "plan", dict(fuse=0, S=3), B=16385, fused=1)
case("fuse_uncompiled", "plan", dict(fuse=0), B=4096, fused=1, compiled=0)
case("fuse_switched_off", "plan", dict(fuse=0), B=4096, fused=0)
case("fuse_lane_stage", "plan", dict(fuse=0, lane=1), B=4096, fused=1, lane_stage=1)
case("fuse_stage_call", "plan", dict(fuse=0), B=4096, fused=1, stages=1)
case("fuse_group_32", "plan", dict(fuse=0), B=4096, fused=1, knobs=["qp_group=32"])
case("fuse_max_knob_at", "plan", dict(fuse=1), B=100, fused=1, knobs=["fuse_max=100"])
case("fuse_max_knob_above", "plan", dict(fuse=0), B=101, fused=1, knobs=["fuse_max=100"])

# ---- automatic order: manipulator, 0 < ncand_slots <= kMaxCandSlots (16 here)
case("order_2048", "plan", dict(auto_order=0), B=2048)
case("order_2049", "plan", dict(auto_order=1, use_caller_order=0), B=2049)
case("order_8192_unfused", "plan", dict(auto_order=1, fuse=0), B=8192)
case("order_8193_unfused", "plan", dict(auto_order=0, fuse=0), B=8193)
case("order_16384_fused", "plan", dict(auto_order=1, fuse=1), B=16384, fused=1)
case("order_2048_fused", "plan", dict(auto_order=0, fuse=1), B=2048, fused=1)
case("order_obstacle_slots", "plan", dict(auto_order=0), B=4096, slots=1)
case("order_whole_body", "plan", dict(auto_order=0), B=4096, kind=1)
case("order_callers", "plan", dict(auto_order=0, use_caller_order=1), B=4096, caller_order=1)
case("order_stage_call", "plan", dict(auto_order=0, use_caller_order=0), B=4096, stages=1, caller_order=1)
case("order_no_cand_slots", "plan", dict(auto_order=0), B=4096, ncand=0)
case("order_cand_slots_at_max", "plan", dict(auto_order=1), B=4096, ncand=16)
case("order_cand_slots_above_max", "plan", dict(auto_order=0), B=4096, ncand=17)
case("order_lane_stage", "plan", dict(lane=1, auto_order=0, use_caller_order=0), B=4096, lane_stage=2, caller_order=1)
case("order_knobs", "plan", dict(auto_order=1), B=100, knobs=["order_min=100", "order_max=100"])
case("order_knobs_above", "plan", dict(auto_order=0), B=101, knobs=["order_min=100", "order_max=100"])

# ---- lane stage: modes 1 and 2 need nv in {6, 7}, no hulls, no obstacle slots; mode 3 only for stage calls
for mode in (1, 2):
    for nv in (6, 7):
        case("lane_mode%d_nv%d" % (mode, nv), "plan", dict(lane=1), B=256, lane_stage=mode, nv=nv)
        case("lane_mode%d_nv%d_stages" % (mode, nv), "plan", dict(lane=1), B=256, lane_stage=mode, nv=nv, stages=1)
    case("lane_mode%d_nv8" % mode, "plan", dict(lane=0), B=256, lane_stage=mode, nv=8)
    case("lane_mode%d_nv5" % mode, "plan", dict(lane=0), B=256, lane_stage=mode, nv=5)
    case("lane_mode%d_hulls" % mode, "plan", dict(lane=0), B=256, lane_stage=mode, has_mesh=1)
    case("lane_mode%d_slots" % mode, "plan", dict(lane=0), B=256, lane_stage=mode, slots=1)
    case("lane_mode%d_cand_above_max" % mode, "plan", dict(lane=0), B=256, lane_stage=mode, ncand=17)
case("lane_mode0", "plan", dict(lane=0), B=256, lane_stage=0)
case("lane_mode3_qp_call", "plan", dict(lane=0, fuse=1), B=256, lane_stage=3, fused=1)
case("lane_mode3_stage_call", "plan", dict(lane=1), B=256, lane_stage=3, stages=1)
case("lane_mode3_stage_call_hulls", "plan", dict(lane=0), B=256, lane_stage=3, stages=1, has_mesh=1)

# ---- sub-batch ranges B c / S .. B (c + 1) / S, xcd_map from Bc >= 16 384, grids min(Bc, cap)
for c in range(4):
    case("sub_65536_%d" % c, "sub", dict(b0=16384 * c, Bc=16384, xcd_map=1, grid_task=1024, grid_qp=4096,
                                          grid_fused=2048), extra=[c], B=65536)
for c, (b0, Bc) in enumerate(((0, 16384), (16384, 16385), (32769, 16385), (49154, 16385))):
    case("sub_65539_%d" % c, "sub", dict(b0=b0, Bc=Bc, xcd_map=1), extra=[c], B=65539)
for c, (b0, Bc) in enumerate(((0, 4096), (4096, 4096), (8192, 4097))):
    case("sub_12289_%d" % c, "sub", dict(b0=b0, Bc=Bc, xcd_map=0, grid_task=1024, grid_qp=4096, grid_fused=2048),
         extra=[c], B=12289)
for c, (b0, Bc, xcd) in enumerate(((0, 16383, 0), (16383, 16384, 1), (32767, 16384, 1))):
    case("sub_49151_%d" % c, "sub", dict(b0=b0, Bc=Bc, xcd_map=xcd), extra=[c], B=49151)
case("sub_fused_100", "sub", dict(b0=0, Bc=100, xcd_map=0, grid_task=100, grid_qp=100, grid_fused=100), extra=[0],
     B=100, fused=1)
case("sub_fused_16384", "sub", dict(b0=0, Bc=16384, xcd_map=1, grid_fused=2048), extra=[0], B=16384, fused=1)
case("sub_one_3000", "sub", dict(b0=0, Bc=3000, xcd_map=0, grid_task=1024, grid_qp=3000, grid_fused=2048), extra=[0],
     B=3000)
# caps are multiples of 8
case("sub_grid_knobs", "sub", dict(b0=0, Bc=5000, grid_task=1024, grid_qp=8, grid_fused=2048), extra=[0], B=5000,
     knobs=["grid_task=1030", "grid_qp=8", "grid_fused=2055"])
case("sub_grid_knobs_small", "sub", dict(grid_task=17, grid_qp=17, grid_fused=17), extra=[0], B=17,
     knobs=["grid_task=24", "grid_qp=31", "grid_fused=4000"])

# ---- the stage builds (DESIGN.md "Stage builds"): the build a model and a call need ...
for mesh, slots, twists, name in ((0, 0, 0, "plain"), (0, 0, 1, "plain"), (1, 0, 0, "mesh"), (1, 0, 1, "mesh"),
                                  (0, 1, 0, "obst"), (0, 1, 1, "rate"), (1, 1, 0, "none"), (1, 1, 1, "none")):
    raw("build_%d%d%d" % (mesh, slots, twists), "build %d %d %d" % (mesh, slots, twists), "build", name)
# ... and the whole table of which kernel family is compiled in which
BUILDS = ("plain", "mesh", "obst", "rate")
HAS = {
    "problem0": ("plain", "mesh", "obst", "rate"),   # the QPIK task stage
    "problem1": ("plain", "mesh"),                   # the QPID stage
    "problem2": ("plain",),                          # closed-form (hull models run it too: no distance stage)
    "fused": ("plain", "mesh", "obst", "rate"),
    "rollout": ("plain", "mesh"),
    "reach": ("plain",),
    "reach_path": ("plain", "obst"),
    "reach_seeds": ("plain", "obst"),
}
for fam, have in HAS.items():
    for b in BUILDS:
        raw("has_%s_%s" % (fam, b), "has %s %s" % (fam, b), "has", int(b in have))

# ---- the persistent-path predicate, as its four users ask: (max_b, family), against the table above
ROLLOUT_MAX = 4096      # manipulators; whole-body robots 65 536
REACH_MAX = 65536
for who, mx in (("rollout", ROLLOUT_MAX), ("reach", REACH_MAX), ("reach_path", REACH_MAX), ("reach_seeds", REACH_MAX)):
    args = [mx, who]
    case("pers_%s_plain" % who, "pers", 1, extra=args, B=mx, fused=1)
    case("pers_%s_above_max" % who, "pers", 0, extra=args, B=mx + 1, fused=1)
    case("pers_%s_hulls" % who, "pers", int("mesh" in HAS[who]), extra=args, B=256, fused=1, has_mesh=1)
    case("pers_%s_slots" % who, "pers", int("obst" in HAS[who]), extra=args, B=256, fused=1, slots=1)
    case("pers_%s_moving_slots" % who, "pers", int("rate" in HAS[who]), extra=args, B=256, fused=1, slots=1,
         knobs=["twists=1"])
    case("pers_%s_twists_no_slots" % who, "pers", 1, extra=args, B=256, fused=1, knobs=["twists=1"])
    case("pers_%s_fusion_off" % who, "pers", 0, extra=args, B=256, fused=0)
    case("pers_%s_uncompiled" % who, "pers", 0, extra=args, B=256, fused=1, compiled=0)
    case("pers_%s_group_32" % who, "pers", 0, extra=args, B=256, fused=1, knobs=["qp_group=32"])
    # any lane-stage mode, also where the plan itself ends without the lane stage
    case("pers_%s_lane_mode1" % who, "pers", 0, extra=args, B=256, fused=1, lane_stage=1)
    case("pers_%s_lane_mode3" % who, "pers", 0, extra=args, B=256, fused=1, lane_stage=3)
    case("pers_%s_lane_mode1_nv8" % who, "pers", 0, extra=args, B=256, fused=1, lane_stage=1, nv=8)
case("pers_rollout_whole_body", "pers", 1, extra=[65536, "rollout"], B=65536, fused=1, kind=1, nv=9)
case("pers_hulls_and_slots", "pers", 0, extra=[65536, "rollout"], B=256, fused=1, has_mesh=1, slots=1)
# ... where plan_call, asked for the same model, runs without the lane stage and fuses
case("plan_lane_mode3_fuses", "plan", dict(lane=0, fuse=1), B=256, fused=1, lane_stage=3)
case("plan_lane_mode1_nv8_fuses", "plan", dict(lane=0, fuse=1), B=256, fused=1, lane_stage=1, nv=8)


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    assert shutil.which(CXX), "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("call_plan") / "call_plan")
    subprocess.check_call([CXX, "-O1", "-std=c++17", "-Wall", "-Werror",
                           os.path.join(ROOT, "tools", "call_plan_host_test.cpp"), "-o", exe])
    names = list(CASES)
    r = subprocess.run([exe], input="".join(CASES[n][0] + "\n" for n in names), capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-500:])
    lines = r.stdout.splitlines()
    assert len(lines) == len(names)
    return dict(zip(names, lines))


@pytest.mark.parametrize("name", list(CASES))
def test_plan(answers, name):
    line, what, expect = CASES[name]
    tok = answers[name].split()
    assert tok[0] == what, (line, answers[name])
    if what == "build":
        assert tok[1:] == [expect], (line, answers[name])
        return
    got = [int(t) for t in tok[1:]]
    if what in ("pers", "has"):
        assert got == [expect], (line, answers[name])
        return
    out = dict(zip(PLAN_OUT if what == "plan" else SUB_OUT, got))
    assert len(got) == len(out)
    assert {k: out[k] for k in expect} == expect, (line, answers[name])
