"""Certified path clearance on the CPU: the motion weights of model.cpp
(build_motion_tables) and the fold of csrc/clearance_certify.hpp, compiled with
the host compiler (tools/clearance_certify_host_test.cpp, -ffp-contract=off),
against numbers worked out by hand here, the oracle's forward kinematics, and
the rule of include/drc_amd.h restated in plain Python (tests/_certify.py), bit
for bit."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import _certify as CF
import oracle as O
import pyref as R
from dyros_robot_controller_amd import robot_path

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dyros_robot_controller_amd", "csrc")
CXX = os.environ.get("CXX", "g++")
INF, NAN = math.inf, math.nan
FREE, BLOCKED, INVALID, UNDECIDED = CF.FREE, CF.BLOCKED, CF.INVALID, CF.UNDECIDED

# revolute (z) -> prismatic (z, travel 0.4) -> revolute (y); a box on the fixed
# base, a sphere, a cylinder and a box on the three moving links
URDF = """<?xml version="1.0"?>
<robot name="rpr">
  <link name="base"><collision><origin xyz="0 0 0.05"/><geometry><box size="0.2 0.2 0.1"/></geometry></collision></link>
  <link name="l1"><collision><origin xyz="0.1 0 0"/><geometry><sphere radius="0.05"/></geometry></collision></link>
  <link name="l2"><collision><origin xyz="0 0.3 0.4"/><geometry><cylinder radius="0.03" length="0.08"/></geometry></collision></link>
  <link name="l3"><collision><origin xyz="0 0 0.12"/><geometry><box size="0.06 0.08 0.24"/></geometry></collision></link>
  <joint name="j1" type="revolute"><parent link="base"/><child link="l1"/><origin xyz="0 0 0.3"/><axis xyz="0 0 1"/>
    <limit lower="-2" upper="2" velocity="1" effort="1"/></joint>
  <joint name="j2" type="prismatic"><parent link="l1"/><child link="l2"/><origin xyz="0 0 0.2"/><axis xyz="0 0 1"/>
    <limit lower="-0.1" upper="0.4" velocity="1" effort="1"/></joint>
  <joint name="j3" type="revolute"><parent link="l2"/><child link="l3"/><origin xyz="0.3 0 0.4"/><axis xyz="0 1 0"/>
    <limit lower="-2" upper="2" velocity="1" effort="1"/></joint>
</robot>
"""
# by hand: |p| of the placements, the bounding radii, the prismatic travel
P_G1, RAD_G1 = 0.1, 0.05                              # sphere r
P_G2, RAD_G2 = 0.5, math.sqrt(0.03 ** 2 + 0.04 ** 2)  # (0, 0.3, 0.4); cylinder sqrt(r^2 + (h/2)^2) = 0.05
P_G3, RAD_G3 = 0.12, 0.13                             # box half extents (0.03, 0.04, 0.12)
P_J2, TRAVEL_J2, P_J3 = 0.2, 0.4, 0.5                 # j3 at (0.3, 0, 0.4)
RHO = np.array([
    # base, sphere (on j1), cylinder (on j2), box (on j3)
    [0.0, P_G1 + RAD_G1, (P_J2 + TRAVEL_J2) + P_G2 + RAD_G2, P_J3 + (P_J2 + TRAVEL_J2) + P_G3 + RAD_G3],   # about j1
    [0.0, 0.0, P_G2 + RAD_G2, P_J3 + P_G3 + RAD_G3],                                                     # about j2
    [0.0, 0.0, 0.0, P_G3 + RAD_G3],                                                                      # about j3
])
PAIRS = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
WT = np.array([
    [0.15, 1.15, 1.35, 0.0, 0.0, 0.0],   # j1 revolute: rho of the supported side; supports both of (1,2) (1,3) (2,3)
    [0.0, 1.0, 1.0, 1.0, 1.0, 0.0],      # j2 prismatic: 1; neither of (0,1), both of (2,3)
    [0.0, 0.0, 0.25, 0.0, 0.25, 0.25],   # j3 revolute: the box only
])


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    assert shutil.which(CXX), "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("certify") / "certify")
    subprocess.check_call([CXX, "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-Wno-unknown-pragmas",
                           os.path.join(ROOT, "tools", "clearance_certify_host_test.cpp"),
                           os.path.join(CSRC, "model.cpp"), os.path.join(CSRC, "mesh.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def rpr(tmp_path_factory):
    p = tmp_path_factory.mktemp("rpr") / "rpr.urdf"
    p.write_text(URDF)
    return str(p)


def fx(t):
    return float.fromhex(t) if "x" in t else float(t)


def model_tables(tool, urdf, srdf="-", slots=0, inf_joint=0):
    out = subprocess.run([tool, "model", urdf, srdf, str(slots), str(inf_joint)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-300:]
    lines = out.stdout.strip().splitlines()
    nv, ngeom, npairs, pair_ld, motion_ld, mask, unbounded = (int(t) for t in lines[0].split())
    geoms = [tuple(int(t) for t in ln.split()[1:]) for ln in lines[1:1 + ngeom]]
    pairs = [tuple(int(t) for t in ln.split()[1:]) for ln in lines[1 + ngeom:1 + ngeom + npairs]]
    k = 1 + ngeom + npairs
    rho = np.array([[fx(t) for t in ln.split()] for ln in lines[k:k + nv]]).reshape(nv, ngeom)
    wt = np.array([[fx(t) for t in ln.split()] for ln in lines[k + nv:k + 2 * nv]]).reshape(nv, npairs)
    restored = int(lines[k + 2 * nv].split()[1]) if slots else None
    return dict(nv=nv, ngeom=ngeom, npairs=npairs, pair_ld=pair_ld, motion_ld=motion_ld, mask=mask,
                unbounded=unbounded, geoms=geoms, pairs=pairs, rho=rho, wt=wt, restored=restored)


# ---- the motion weights -------------------------------------------------------
def test_weights_of_a_written_out_tree(tool, rpr):
    m = model_tables(tool, rpr)
    assert (m["nv"], m["ngeom"]) == (3, 4) and m["pairs"] == PAIRS
    assert [g[0] for g in m["geoms"]] == [0, 1, 2, 3] and [g[1] for g in m["geoms"]] == [2, 0, 1, 2]
    np.testing.assert_allclose(m["rho"], RHO, rtol=0, atol=1e-15)
    np.testing.assert_allclose(m["wt"], WT, rtol=0, atol=1e-15)
    assert m["motion_ld"] == m["pair_ld"] >= m["npairs"]
    assert (m["rho"][:, 0] == 0).all(), "a fixed-link geometry moves with no joint"


def test_a_joint_that_supports_both_geometries_weighs_nothing(tool, rpr):
    m = model_tables(tool, rpr)
    for p, (a, b) in enumerate(PAIRS):
        for j in range(3):
            both = a >= j + 1 and b >= j + 1      # the chain: joint j+1 supports geometry g iff g's joint >= j+1
            neither = a < j + 1 and b < j + 1
            assert (m["wt"][j, p] == 0.0) == (both or neither), (j, p)
    assert m["wt"][0, PAIRS.index((1, 3))] == 0.0 and m["rho"][0, 1] > 0 and m["rho"][0, 3] > 0


def test_a_slot_pair_weighs_the_robot_side_only(tool, rpr):
    m = model_tables(tool, rpr, slots=1)
    assert m["ngeom"] == 5 and m["pairs"] == PAIRS + [(1, 4), (2, 4), (3, 4)]
    assert m["geoms"][4] == (0, 0) and (m["rho"][:, 4] == 0).all()
    np.testing.assert_allclose(m["rho"][:, :4], RHO, rtol=0, atol=1e-15)
    np.testing.assert_allclose(m["wt"][:, :6], WT, rtol=0, atol=1e-15)
    np.testing.assert_allclose(m["wt"][:, 6:], RHO[:, 1:] * [[1], [0], [1]] + [[0] * 3, [0, 1, 1], [0] * 3],
                               rtol=0, atol=1e-15)   # revolute rows: rho of the link geometry; prismatic row: 1
    assert m["restored"] == 1, "n = 0 does not give the fresh model back byte for byte"


def test_travel_mask_and_the_unsupported_case(tool, rpr):
    m = model_tables(tool, rpr)
    assert m["mask"] == 0b010 and m["unbounded"] == 0     # j2: prismatic, a revolute joint above, geometry below
    inf = model_tables(tool, rpr, inf_joint=2)
    assert inf["mask"] == 0b010 and inf["unbounded"] == 1
    assert np.isinf(inf["rho"][0, 2]) and np.isinf(inf["wt"][0, 1]) and inf["rho"][1, 2] == RHO[1, 2]
    for robot in ("fr3", "ur5e"):
        assert model_tables(tool, robot_path(robot), robot_path(robot, "srdf"))["mask"] == 0
    # the mobile bases' virtual x, y: prismatic, but no revolute joint above them
    husky = model_tables(tool, robot_path("husky_fr3"), robot_path("husky_fr3", "srdf"), slots=2)
    assert husky["mask"] == 0 and husky["unbounded"] == 0 and husky["restored"] == 1
    assert np.isfinite(husky["wt"]).all() and (husky["wt"] >= 0).all()


def test_fr3_the_bound_is_a_bound(tool):
    """Between the ends of a segment the centre of every geometry of every
    pair moves at most sum_j rho[j][g] |dq_j| (the oracle's FK; the weights
    bound every point of the geometry, the centre among them)."""
    m = model_tables(tool, robot_path("fr3"), robot_path("fr3", "srdf"))
    pm, _, _ = O.load("fr3")
    assert m["ngeom"] == len(pm.geoms) and m["pairs"] == [tuple(p) for p in pm.pairs]
    assert [g[0] for g in m["geoms"]] == [g["parent_joint"] for g in pm.geoms]
    used = sorted({g for p in m["pairs"] for g in p})
    rng = np.random.default_rng(3)
    lo, hi = np.asarray(pm.lower), np.asarray(pm.upper)
    tight = 0.0
    for _ in range(200):
        qa, qb = rng.uniform(lo, hi), rng.uniform(lo, hi)
        ca = [T[:3, 3] for T in R.geom_poses(pm, R.fk(pm, qa))]
        cb = [T[:3, 3] for T in R.geom_poses(pm, R.fk(pm, qb))]
        bound = np.abs(qb - qa) @ m["rho"]
        for g in used:
            moved = np.linalg.norm(cb[g] - ca[g])
            assert moved <= bound[g], (g, moved, bound[g])
            tight = max(tight, moved / bound[g]) if bound[g] > 0 else tight
    print("FR3: largest centre displacement / bound over 200 segments: %.3f" % tight)
    assert 0.05 < tight <= 1.0, tight


# ---- the fold -------------------------------------------------------------------
def run_folds(tool, cases):
    """cases: (d_stop, max_depth, W, depth, [(travel_ok, M, [d ...]) per segment])."""
    lines = []
    for d_stop, max_depth, W, depth, segs in cases:
        t = [hexf(d_stop), str(max_depth), str(W), str(depth)]
        for ok, M, d in segs:
            assert len(d) == 2 ** depth + 1
            t += [str(int(ok)), hexf(M)] + [hexf(x) for x in d]
        lines.append(" ".join(t))
    res = subprocess.run([tool, "fold"], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-300:]
    out = res.stdout.strip().splitlines()
    assert len(out) == len(cases)
    got = []
    for ln in out:
        t = ln.split()
        r = dict(result=int(t[0]), seg_stop=int(t[1]), t_stop=fx(t[2]), d_min=fx(t[3]), seg_min=int(t[4]),
                 t_min=fx(t[5]), pair_min=int(t[6]), d_lower=fx(t[7]), samples_used=int(t[8]))
        seen = [(int(a), int(b), int(c)) for a, b, c in (s.replace(":", "/").split("/") for s in t[9:])]
        got.append((r, seen))
    return got


def hexf(x):
    return "nan" if x != x else ("inf" if x == INF else ("-inf" if x == -INF else float(x).hex()))


def restate(case):
    d_stop, max_depth, W, depth, segs = case

    def dist(j, k, e):
        idx = k << (depth - e)
        return segs[j][2][idx], 1000 * j + idx
    return CF.fold(dist, W, d_stop, max_depth, [s[1] for s in segs], [s[0] for s in segs])


def same(a, b):
    (ra, sa), (rb, sb) = a, b
    assert sa == sb, (sa, sb)
    for k in CF.FIELDS:
        x, y = ra[k], rb[k]
        if isinstance(x, float) or isinstance(y, float):
            assert np.float64(x).view(np.uint64) == np.float64(y).view(np.uint64), (k, x, y)
        else:
            assert x == y, (k, x, y)


X = 9.0   # a grid entry the walk must not read
# name: (case, what the rule gives: result, seg_stop, t_stop, d_min, seg_min, t_min, pair_min, d_lower, samples)
FOLD_CASES = {
    # lb = 0.5 (0.5 + 0.7) - 0.5 * 0.4 = 0.4 >= 0.1
    "certified_at_depth_0": ((0.1, 3, 2, 1, [(1, 0.4, [0.5, X, 0.7])]),
                             (FREE, -1, -1.0, 0.5, 0, 0.0, 0, 0.5 * (0.5 + 0.7) - 0.5 * 0.4, 2)),
    # depth 0: 0.6 - 0.5 = 0.1 < 0.3; halves: 0.5 (0.5 + 0.6) - 0.25 = 0.3 and 0.5 (0.6 + 0.7) - 0.25 = 0.4
    "one_bisection": ((0.3, 3, 2, 1, [(1, 1.0, [0.5, 0.6, 0.7])]),
                      (FREE, -1, -1.0, 0.5, 0, 0.0, 0, 0.5 * (0.5 + 0.6) - 0.25 * 1.0, 3)),
    "blocked_at_a_midpoint": ((0.3, 3, 2, 1, [(1, 1.0, [0.5, 0.2, 0.7])]),
                              (BLOCKED, 0, 0.5, 0.2, 0, 0.5, 1, INF, 3)),
    "blocked_at_waypoint_0": ((0.3, 3, 2, 0, [(1, 1.0, [0.1, 0.7])]), (BLOCKED, 0, 0.0, 0.1, 0, 0.0, 0, INF, 1)),
    "blocked_at_t_1_of_segment_1": ((0.3, 3, 3, 0, [(1, 0.1, [0.5, 0.7]), (1, 0.1, [X, 0.2])]),
                                    (BLOCKED, 1, 1.0, 0.2, 1, 1.0, 1001, 0.5 * (0.5 + 0.7) - 0.5 * 0.1, 3)),
    "undecided_at_max_depth_0": ((0.3, 0, 2, 0, [(1, 1.0, [0.5, 0.7])]), (UNDECIDED, 0, 0.0, 0.5, 0, 0.0, 0, INF, 2)),
    # M = 8: at depth 3 lb = mid - 0.5 still below 0.3 on the first interval [0, 1/8]
    "undecided_at_max_depth_3": ((0.3, 3, 2, 3, [(1, 8.0, [0.5, 0.5, 0.5, X, 0.5, X, X, X, 0.5])]),
                                 (UNDECIDED, 0, 0.0, 0.5, 0, 0.0, 0, INF, 5)),
    "nan_at_a_midpoint": ((0.3, 3, 2, 1, [(1, 1.0, [0.5, NAN, 0.7])]), (INVALID, 0, 0.5, 0.5, 0, 0.0, 0, INF, 3)),
    "nan_at_waypoint_0": ((0.3, 3, 2, 0, [(1, 1.0, [NAN, 0.7])]), (INVALID, 0, 0.0, INF, -1, -1.0, -1, INF, 1)),
    "d_stop_minus_inf_is_a_leaf_at_depth_0": ((-INF, 0, 3, 0, [(1, 50.0, [0.5, -0.2]), (1, 70.0, [X, 0.1])]),
                                              (FREE, -1, -1.0, -0.2, 0, 1.0, 1, 0.5 * (-0.2 + 0.1) - 0.5 * 70.0, 3)),
    "d_stop_plus_inf_blocks_at_once": ((INF, 3, 2, 0, [(1, 1.0, [5.0, 6.0])]), (BLOCKED, 0, 0.0, 5.0, 0, 0.0, 0, INF, 1)),
    "d_stop_plus_inf_d_inf": ((INF, 3, 2, 0, [(1, 0.0, [INF, INF])]), (FREE, -1, -1.0, INF, -1, -1.0, -1, INF, 2)),
    "travel_violation_on_segment_1": ((0.1, 3, 3, 0, [(1, 0.4, [0.5, 0.7]), (0, 0.4, [X, 0.7])]),
                                      (UNDECIDED, 1, 0.0, 0.5, 0, 0.0, 0, 0.5 * (0.5 + 0.7) - 0.5 * 0.4, 2)),
    "travel_violation_on_segment_0": ((0.1, 3, 2, 0, [(0, 0.4, [0.5, 0.7])]), (UNDECIDED, 0, 0.0, 0.5, 0, 0.0, 0, INF, 1)),
    "one_waypoint": ((0.1, 3, 1, 0, [(1, 0.0, [0.5, X])]), (FREE, -1, -1.0, 0.5, 0, 0.0, 0, INF, 1)),
    "one_waypoint_blocked": ((0.6, 3, 1, 0, [(1, 0.0, [0.5, X])]), (BLOCKED, 0, 0.0, 0.5, 0, 0.0, 0, INF, 1)),
    # evaluated in the order t = 0, 1, 1/2: the first evaluated of equal distances keeps the minimum
    "tie_first_evaluated_wins": ((0.25, 3, 2, 1, [(1, 1.0, [0.7, 0.5, 0.5])]),
                                 (FREE, -1, -1.0, 0.5, 0, 1.0, 2, 0.5 * (0.5 + 0.5) - 0.25 * 1.0, 3)),
    "tie_across_segments": ((0.1, 3, 3, 0, [(1, 0.1, [0.5, 0.5]), (1, 0.1, [X, 0.5])]),
                            (FREE, -1, -1.0, 0.5, 0, 0.0, 0, 0.5 * (0.5 + 0.5) - 0.5 * 0.1, 3)),
    "lb_equal_to_d_stop_is_a_leaf": ((0.25, 0, 2, 0, [(1, 0.5, [0.5, 0.5])]),
                                     (FREE, -1, -1.0, 0.5, 0, 0.0, 0, 0.25, 2)),
}


@pytest.mark.parametrize("name", sorted(FOLD_CASES))
def test_fold_written_out(tool, name):
    case, want = FOLD_CASES[name]
    got = run_folds(tool, [case])[0]
    ref = restate(case)
    same(got, ref)
    assert all(case[4][j][2][k << (case[3] - e)] != X for j, k, e in got[1]), "the walk read an entry it must not"
    w = dict(zip(CF.FIELDS, want))
    for k in CF.FIELDS:
        assert got[0][k] == w[k], (name, k, got[0][k], w[k])


def test_fold_walks_left_to_right_depth_first(tool):
    """A segment that needs depth 2 on its left half only: the order of the evaluations."""
    d = [0.30, 0.30, 0.30, X, 0.60, X, X, X, 0.9]   # grid of 8 steps; M = 1, d_stop = 0.19
    case = (0.19, 3, 2, 3, [(1, 1.0, d)])
    got = run_folds(tool, [case])[0]
    same(got, restate(case))
    # [0,1]: 0.6 - 0.5 < 0.19 -> 1/2; [0,1/2]: 0.45 - 0.25 leaf; [1/2,1]: 0.75 - 0.25 leaf
    assert got[1] == [(0, 0, 0), (0, 1, 0), (0, 1, 1)] and got[0]["result"] == FREE
    d = [0.30, 0.26, 0.30, X, 0.40, X, 0.5, X, 0.6]
    case = (0.19, 3, 2, 3, [(1, 1.0, d)])
    got = run_folds(tool, [case])[0]
    same(got, restate(case))
    # [0,1]: 0.45 - 0.5; [0,1/2]: 0.35 - 0.25 -> 1/4; [0,1/4]: 0.3 - 0.125 -> 1/8; [0,1/8], [1/8,1/4]: 0.28 - 0.0625,
    # [1/4,1/2]: 0.35 - 0.125, [1/2,1]: 0.5 - 0.25: leaves
    assert got[1] == [(0, 0, 0), (0, 1, 0), (0, 1, 1), (0, 1, 2), (0, 1, 3)] and got[0]["result"] == FREE
    assert got[0]["samples_used"] == 5


def test_fold_random_sequences(tool):
    rng = np.random.default_rng(17)
    cases = []
    for n in range(400):
        depth = int(rng.integers(0, 5))
        max_depth = int(rng.integers(0, depth + 1))
        W = int(rng.integers(1, 5))
        base = rng.uniform(0.0, 0.4)
        d_stop = float(rng.choice([0.0, 0.05, 0.1, 0.2, -INF, INF], p=[.2, .25, .25, .2, .05, .05]))
        segs = []
        for j in range(max(W - 1, 1)):
            # a smooth profile plus noise, sometimes dipping below d_stop; a NaN now and then
            t = np.linspace(0, 1, 2 ** depth + 1)
            d = base + 0.3 * np.sin(rng.uniform(0, 6) + rng.uniform(1, 5) * t) + rng.normal(0, 0.02, t.size) + 0.25
            if rng.random() < 0.1:
                d[rng.integers(0, t.size)] = NAN
            if rng.random() < 0.15:
                d = np.round(d, 1)   # ties
            segs.append((int(rng.random() > 0.05), float(rng.uniform(0.0, 2.0)), [float(x) for x in d]))
        cases.append((d_stop, max_depth, W, depth, segs))
    got = run_folds(tool, cases)
    seen = np.zeros(4, int)
    for c, g in zip(cases, got):
        same(g, restate(c))
        seen[g[0]["result"]] += 1
    print("random folds: FREE %d, BLOCKED %d, INVALID %d, UNDECIDED %d" % tuple(seen))
    assert (seen >= 20).all(), seen


def test_motion_bound_sum_in_ascending_order(tool):
    rng = np.random.default_rng(23)
    lines, want = [], []
    for _ in range(50):
        nv, npairs = int(rng.integers(1, 15)), int(rng.integers(1, 90))
        wt = rng.uniform(0, 2, (nv, npairs)) * (rng.random((nv, npairs)) < 0.6)
        dq = np.abs(rng.uniform(-3, 3, nv))
        lines.append("%d %d %s %s" % (nv, npairs, " ".join(hexf(x) for x in dq), " ".join(hexf(x) for x in wt.ravel())))
        want.append(CF.motion_bound(wt, dq))
    res = subprocess.run([tool, "motion"], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert res.returncode == 0
    got = [fx(t) for t in res.stdout.split()]
    assert [float(x).hex() for x in got] == [float(x).hex() for x in want]
