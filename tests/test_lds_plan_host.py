"""csrc/lds_plan.hpp -- where every region of the per-wave LDS plans lies and
which regions share bytes -- compiled with the host compiler
(tools/lds_plan_host_test.cpp, with model.cpp and mesh.cpp) and checked
against the rules the header's comments state.

Models: the five bundled robots (the three mobile ones with the indices the
tests create them with) and three synthetic ones: a single link (no collision
pairs), 48 boxes on 8 links (1008 pairs: the geometry poses do not fit under
the EPA polytope, so the task plan is laid out a second time with the poses
beside it) and a model at the bounds of model.hpp (nv 16, 64 geometries, 1024
pairs; whole-body with 8 arm joints, the widest QP one wavefront maps).
Plans, per model: the task plan narrow and wide for QPIK, QPID and the
closed-form kinds 1, 2, 3; the QP plan for QPIK and QPID.

The offsets of the bundled robots are pinned in tests/golden/lds_plan_bundled.txt,
recorded from the layout code before it had a header of its own."""
import os
import shutil
import subprocess

import pytest

from dyros_robot_controller_amd import robot_path
from test_gpu_many_candidates import tangle_urdf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.environ.get("CXX", "g++")
CSRC = os.path.join(ROOT, "dyros_robot_controller_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "lds_plan_bundled.txt")

# n_wheel, virtual_start, mani_start, mobi_start, act_mani_start, act_mobi_start (oracle.ROBOTS)
BUNDLED = {"fr3": None, "ur5e": None, "husky_fr3": "2,0,3,10,0,7", "xls_fr3": "4,0,3,10,0,7",
           "caster_fr3": "4,0,3,10,0,7"}
SYNTHETIC = ("nopairs", "crowded", "bounds")
KINDS = ("qpik", "qpid", "cf1", "cf2", "cf3")
TASK = ["task_%s_%s" % (w, k) for w in ("narrow", "wide") for k in KINDS]
VARIANTS = ["qp_qpik", "qp_qpid"] + TASK
CASES = ["%s/%s" % (m, v) for m in list(BUNDLED) + list(SYNTHETIC) for v in VARIANTS]
PERSISTENT, LIVE, MANIP, POLYTOPE, POSES, CAND = range(6)   # lds_plan.hpp PlanGroup
OK, QP_TOO_LARGE, MODEL_TOO_LARGE = range(3)                # lds_plan.hpp LdsPlanResult
LDS_BYTES = 160 * 1024

NOPAIRS_URDF = """<robot name="nopairs">
  <link name="base"/>
  <link name="arm"><collision><geometry><box size="0.1 0.1 0.1"/></geometry></collision></link>
  <joint name="j1" type="revolute"><parent link="base"/><child link="arm"/><axis xyz="0 0 1"/>
    <limit lower="-1" upper="1" velocity="1" effort="1"/></joint>
</robot>
"""


def model_args(tmp):
    """The program's arguments: NAME URDF SRDF MOBILE COMPILED per model."""
    args = []
    for name, mobile in BUNDLED.items():   # every bundled robot's QPIK shape is compiled (launch.hpp)
        args += [name, robot_path(name), robot_path(name, "srdf"), mobile or "-", "1"]
    nopairs = os.path.join(tmp, "nopairs.urdf")
    with open(nopairs, "w") as fh:
        fh.write(NOPAIRS_URDF)
    crowded = os.path.join(tmp, "crowded.urdf")
    tangle_urdf(crowded, n_joints=8, boxes=6)
    args += ["nopairs", nopairs, "-", "-", "0", "crowded", crowded, "-", "-", "0",
             "bounds", "@bounds", "-", "5,0,3,11,0,8", "0"]
    return args


def parse(text):
    out = dict(model={}, epa=None, plan={}, region={}, fused={}, lines={})
    for ln in text.splitlines():
        t = ln.split()
        if t[0] == "model":
            out["model"][t[1]] = dict(zip(("nv", "ngeom", "npairs", "kind"), map(int, t[2:])))
        elif t[0] == "epa":
            out["epa"] = dict(zip(("fn", "out", "nv", "narrow", "wide"), map(int, t[1:])))
        elif t[0] in ("plan", "fused"):
            out[t[0]][t[1]] = {k: int(v) for k, v in (x.split("=") for x in t[2:])}
            out["lines"][(t[0], t[1])] = ln
        elif t[0] == "region":
            out["region"].setdefault(t[1], []).append((t[2], int(t[3]), int(t[4]), int(t[5])))
        else:
            raise AssertionError(ln)
    return out


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    assert shutil.which(CXX), "no host C++ compiler"
    tmp = str(tmp_path_factory.mktemp("lds_plan"))
    exe = os.path.join(tmp, "lds_plan_host")
    subprocess.check_call([CXX, "-O1", "-std=c++17", "-Wall", "-Werror", os.path.join(ROOT, "tools", "lds_plan_host_test.cpp"),
                           os.path.join(CSRC, "model.cpp"), os.path.join(CSRC, "mesh.cpp"), "-o", exe])
    r = subprocess.run([exe] + model_args(tmp), capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-500:])
    p = parse(r.stdout)
    assert sorted(p["plan"]) == sorted(CASES)
    return p


def overlap(a, b):
    """Doubles that [a0, a0 + an) and [b0, b0 + bn) share."""
    return max(0, min(a[0] + a[1], b[0] + b[1]) - max(a[0], b[0]))


def inside(a, lo, hi):
    return a[1] == 0 or (lo <= a[0] and a[0] + a[1] <= hi)


def test_models(plans):
    m = plans["model"]
    assert (m["fr3"]["ngeom"], m["fr3"]["npairs"]) == (35, 180)
    assert m["nopairs"]["npairs"] == 0
    assert (m["crowded"]["nv"], m["crowded"]["ngeom"], m["crowded"]["npairs"]) == (8, 48, 1008)
    assert (m["bounds"]["nv"], m["bounds"]["ngeom"], m["bounds"]["npairs"]) == (16, 64, 1024)


@pytest.mark.parametrize("case", CASES)
def test_plan_rules(plans, case):
    k, regions, epa = plans["plan"][case], plans["region"].get(case, []), plans["epa"]
    model, variant = case.split("/")
    if model == "bounds":   # laid out within the LDS or refused as too large for it, never as anything else
        assert k["result"] in (OK, MODEL_TOO_LARGE), k
    else:
        assert k["result"] == OK, k
    if k["result"] != OK:
        return
    lds = k["lds_doubles"]
    assert 0 < lds * 8 <= LDS_BYTES
    # every region 16-byte aligned and inside the plan
    for name, off, n, group in regions:
        assert off % 2 == 0 and off >= 0 and off + n <= lds, (name, off, n, lds)
    for f, v in k.items():
        if f[0] in "ok" and not (f == "oHi" and v == -1):   # the offsets: o.. and k..
            assert v % 2 == 0 and 0 <= v <= lds, (f, v)
    # persistent, live kinematics and manipulability scratch: pairwise disjoint (and the poses, which are
    # read while the manipulability scratch is written, share nothing with any of them)
    solid = [r for r in regions if r[3] in (PERSISTENT, LIVE, MANIP, POSES)]
    for i, a in enumerate(solid):
        for b in solid[i + 1:]:
            assert overlap(a[1:3], b[1:3]) == 0, (a, b)
    by = {g: [r for r in regions if r[3] == g] for g in range(6)}
    task = variant.startswith("task_")
    with_epa = task and variant.split("_")[2] in ("qpik", "qpid")
    assert (k["kEpa"] > 0) == with_epa and len(by[POLYTOPE]) == with_epa
    assert len(by[POSES]) == (0 if variant == "qp_qpik" else 1) and len(by[CAND]) == len(by[POSES])
    if variant == "qp_qpik":
        return
    poses, cand = by[POSES][0][1:3], by[CAND][0][1:3]
    assert poses[0] == k["kTg"] and cand[0] == k["kCand"]
    n_pairs, n_geom = plans["model"][model]["npairs"], max(plans["model"][model]["ngeom"], plans["model"][model]["nv"])
    assert poses[1] == 12 * n_geom and cand[1] == (n_pairs + 1) // 2
    if not with_epa:
        # no polytope: the list has a region of its own, and no pose pair is formed (kPp names kSv, unused:
        # DESIGN.md "LDS plan: a header of its own", findings)
        assert all(overlap(cand, r[1:3]) == 0 for r in solid)
        assert k["kOvl"] == 0 and k["kPp"] == k["kSv"]
        return
    poly = by[POLYTOPE][0][1:3]
    assert poly[0] == k["kEpa"] and poly[1] == (epa["wide"] if "wide" in variant else epa["narrow"])
    fn, out = poly[0] + epa["fn"], poly[0] + epa["out"]
    # the candidate list: in the face planes (clear of the stash's vertex slots before fn, of out[] and of nv)
    assert fn <= cand[0] and cand[0] + cand[1] <= out and poly[0] + epa["nv"] >= out
    live = [r for r in regions if r[3] in (PERSISTENT, LIVE)]
    assert all(overlap(cand, r[1:3]) == 0 for r in live) and overlap(cand, poses) == 0
    # the polytope lies over the manipulability scratch only
    assert all(overlap(poly, r[1:3]) == 0 for r in live)
    under = overlap(poses, poly) > 0
    # (crowded, bounds: poses and list are longer than [fn, out), the second layout)
    assert under == ("narrow" in variant and model not in ("crowded", "bounds")), (poses, poly)
    if under:
        assert poses[0] >= k["kScr"] + 160 and inside(poses, fn, out)
        assert k["kOvl"] == k["kCand"] == poses[0] + poses[1]
    else:
        assert k["kOvl"] == k["kEpa"]
    # the pose pair: over kSv for the QPIK stage only (which never stages the mobile Jacobian)
    if variant.endswith("qpik"):
        assert k["kPp"] == k["kSv"]
    else:
        pp = [r for r in by[LIVE] if r[0] == "kPp"]
        assert len(pp) == 1 and pp[0][1] == k["kPp"] and pp[0][2] == 24


@pytest.mark.parametrize("case", ["%s/task_%s_qpik" % (m, w) for m in list(BUNDLED) + list(SYNTHETIC)
                                  for w in ("narrow", "wide")])
def test_fused_record_and_state(plans, case):
    kt, kq, f = plans["plan"][case], plans["plan"][case.split("/")[0] + "/qp_qpik"], plans["fused"][case]
    rec, n = f["rec_offset"], f["rec_len"]
    assert n % 2 == 0 and kt["rLen"] <= n <= kt["rLen"] + 1 and rec % 2 == 0
    assert rec >= kt["kOvl"] and rec >= kq["lds_doubles"] and rec + n <= f["fused_lds"]
    assert f["fused_lds"] >= max(kt["lds_doubles"], kq["lds_doubles"]) and f["fused_lds"] * 8 <= LDS_BYTES
    if rec < kt["lds_doubles"]:   # inside the task plan: past the poses, inside the plan
        poses = [r for r in plans["region"][case] if r[3] == POSES][0]
        assert rec >= poses[1] + poses[2] and rec + n <= kt["lds_doubles"]
        live = [r for r in plans["region"][case] if r[3] in (PERSISTENT, LIVE)]
        assert all(overlap((rec, n), r[1:3]) == 0 for r in live)
    assert f["state"] <= rec


def test_sizes_the_suite_pins(plans):
    size = lambda case: plans["plan"][case]["lds_doubles"] * 8
    # tests/test_gpu_task_plan.py
    for robot in ("fr3", "ur5e"):
        assert size(robot + "/task_narrow_qpik") <= 12800
    assert size("fr3/task_wide_qpik") == 17072
    # DESIGN.md "Occupancy, spills and traffic", the task kernel's two-wave build, KB per wave
    table = {"task_narrow_qpik": (12.8, 11.5, 14.7, 15.3, 14.8), "task_wide_qpik": (17.1, 14.0, 19.4, 20.1, 19.4)}
    for variant, row in table.items():
        for robot, kb in zip(BUNDLED, row):
            assert round(size("%s/%s" % (robot, variant)) / 1000, 1) == kb, (robot, variant)
    for robot in BUNDLED:
        assert size(robot + "/task_wide_qpik") > size(robot + "/task_narrow_qpik")
        for w in ("narrow", "wide"):   # fused: the task plan, the record inside its overlay
            case = "%s/task_%s_qpik" % (robot, w)
            assert plans["fused"][case]["fused_lds"] * 8 == size(case)


def test_bundled_offsets_unchanged(plans):
    with open(GOLDEN) as fh:
        want = [ln.rstrip("\n") for ln in fh if ln.startswith(("plan ", "fused "))]
    got = [ln for (what, case), ln in plans["lines"].items() if case.split("/")[0] in BUNDLED]
    assert len(want) == len(BUNDLED) * (len(VARIANTS) + 2) and sorted(got) == sorted(want)
