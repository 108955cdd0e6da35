"""The task plan with the geometry poses under the EPA polytope (lds_plan.hpp
plan_kinematics) against the wide plan that keeps them beside it
(drc_debug_task_plan_wide), on the same build and the same inputs.

The device code is the same for both layouts; only where data lie in LDS
differs.  Once EPA runs on an instance the narrow plan's poses are gone: EPA
forms the poses of its pair again and, when the search is over, puts the
winner's back for the refinement (task_stage.hpp pose_pair).  So every output must agree BIT FOR BIT: q-dot*,
status and iteration counts, and the stage outputs (pose, Jacobian,
manipulability and gradient, distance and gradient, pair, task velocity; the
QPID and rate extras where a case has them).

The comparison proves something only where EPA ran, so each case asserts its
coverage, computed on the CPU by the oracle's pruned distance search (the
restatement of the device's: same candidates, same best-first EPA order) with
its EPA census: per instance the number of EPA calls and whether the final
winner is a pair EPA expanded.  An instance where EPA ran and another pair
wins is the one that catches a stale read of the poses.  The seeds below were
picked on the CPU with the oracle alone, for these counts.  Across the file
the cases' own assertions add up to: EPA on well over 8 instances, instances
with several EPA calls and instances won by an EPA pair (the tangled model
alone: 8 and 32), and instances where EPA ran and another pair wins (the
obstacle and the bench cases).
"""
import ctypes as C

import numpy as np
import pytest

import oracle as O
import _obstacles as OB
from _common import LINK, make_manipulator, make_moma, moma_step_inputs, step_inputs
from dyros_robot_controller_amd import _batch, _capi, manipulator, mobile_manipulator, robot_path
from test_gpu_many_candidates import tangle_urdf

pytestmark = pytest.mark.gpu

MOMA = ("husky_fr3",)
# 12 task waves per CU on an MI355X (160 KB of LDS, one wave per workgroup): the
# plan must fit 12 times whether LDS is handed out in granules of 512 B
# (13 312 B) or of 1 280 B (12 800 B)
RUNG_BYTES = 12800
WIDE_BYTES = {"fr3": 17072}    # the plan before the poses moved under the polytope

_CACHE = {}


# ---------------------------------------------------------------- helpers
def census(om, q, prepare=None):
    """Per instance (EPA calls, winner is an EPA pair, winning pair) of the
    oracle's pruned distance search."""
    L = O.lib()
    L.oracle_epa_census.argtypes = [C.POINTER(C.c_longlong), C.c_int]
    L.oracle_epa_census.restype = None
    out = (C.c_longlong * 8)()
    rows = []
    O.set_pruned_narrow_phase(True)
    try:
        for b in range(q.shape[1]):
            if prepare:
                prepare(b)
            L.oracle_epa_census(None, 1)
            _, _, pair = O.min_distance(om, q[:, b])
            L.oracle_epa_census(out, 0)
            rows.append((int(out[0]), out[0] > 0 and out[2] == out[0] - 1, int(pair)))
    finally:
        L.oracle_epa_census(None, 0)
        O.set_pruned_narrow_phase(False)
    return rows


def cover(name, rows, ran=1, multi=0, other=0, won=0):
    """Asserts the counts a case's seed was picked for."""
    got = coverage_counts(rows)
    print("%s: EPA ran on %d of %d instances, %d with several calls, %d where another pair wins, %d where an EPA "
          "pair wins" % ((name, got[0], len(rows)) + got[1:]))
    assert got[0] >= ran and got[1] >= multi and got[2] >= other and got[3] >= won, (name, got)


def coverage_counts(rows):
    return (sum(r[0] > 0 for r in rows), sum(r[0] >= 2 for r in rows), sum(r[0] > 0 and not r[1] for r in rows),
            sum(bool(r[1]) for r in rows))


def both_layouts(rd, fn):
    """fn() under the narrow (default) and the wide plan."""
    lib, res = _capi.lib(), []
    try:
        for wide in (0, 1):
            _capi.check(lib.drc_debug_task_plan_wide(rd.model.handle, C.c_int(wide)))
            res.append(fn())
    finally:
        _capi.check(lib.drc_debug_task_plan_wide(rd.model.handle, C.c_int(0)))
    return res


def assert_same_bits(narrow, wide):
    assert narrow.keys() == wide.keys()
    for k in narrow:
        a, b = np.ascontiguousarray(narrow[k]), np.ascontiguousarray(wide[k])
        assert a.dtype == b.dtype and a.shape == b.shape, k
        if a.tobytes() != b.tobytes():
            bad = np.flatnonzero((a != b).reshape(a.shape[0], -1).any(axis=0) if a.ndim > 1 else a != b)
            raise AssertionError("%s differs between the layouts, instances %s" % (k, bad[:16].tolist()))


def _sync():
    import torch
    torch.cuda.synchronize()


def _fusion(rd, on):
    _capi.check(_capi.lib().drc_set_fusion(rd.model.handle, C.c_int(on)))


def _solve(ctrl, rd, fused, q, qd, xt, xdt, link, tag, **kw):
    import torch
    _fusion(rd, fused)
    try:
        it = torch.zeros(q.shape[1], dtype=torch.int32, device=rd.device)
        out, st = ctrl.QPIK_step_batch(q, qd, xt, xdt, link, iters=it, **kw)
        _sync()
    finally:
        _fusion(rd, 1)
    return {tag + "qdot": out.cpu().numpy(), tag + "status": st.cpu().numpy(), tag + "iters": it.cpu().numpy()}


def _stages(rd, q, qd, xt, xdt, link, **kw):
    p = manipulator.QPIKParamsBuilder(rd.model, exact=True).params(link, _capi.MODE_QPIK_STEP)
    a = lambda v: _batch.as_device(v, rd.device)
    st = _batch.stages_batch(rd.model, p, a(q), a(qd), a(xt), a(xdt), **kw)
    _sync()
    return {"stage_" + k: v.cpu().numpy() for k, v in st.items()}


def _robot(robot, cuda):
    if robot not in _CACHE:
        moma = robot in MOMA
        rd = make_moma(robot, cuda) if moma else make_manipulator(robot, cuda)
        ctrl = (mobile_manipulator if moma else manipulator).RobotController(0.001, rd, solver_mode="exact")
        _CACHE[robot] = (rd, ctrl, O.load(robot)[1])
    return _CACHE[robot]


def _plan_bytes(rd, problem=0):
    p = manipulator.QPIKParamsBuilder(rd.model, exact=True).params(LINK["fr3"] if rd.model.dof == 7 else LINK["ur5e"],
                                                                    _capi.MODE_QPIK_STEP)
    t, q, f = C.c_int(), C.c_int(), C.c_int()
    _capi.check(_capi.lib().drc_debug_lds_plan(rd.model.handle, C.byref(p), problem, C.byref(t), C.byref(q), C.byref(f)))
    return t.value


# ---------------------------------------------------------------- the plan's size
@pytest.mark.parametrize("robot", ["fr3", "ur5e"])
def test_plan_fits_twelve_waves_per_cu(cuda, robot):
    """(Creating a model needs a device, so this is a GPU test although it launches nothing.)"""
    rd, _, _ = _robot(robot, cuda)
    narrow, wide = both_layouts(rd, lambda: _plan_bytes(rd))
    print("%s task plan: %d B, wide %d B" % (robot, narrow, wide))
    assert narrow <= RUNG_BYTES, narrow
    assert wide > narrow
    if robot in WIDE_BYTES:
        assert wide == WIDE_BYTES[robot], wide


# ---------------------------------------------------------------- bench stress workload
# (robot, B) -> seed, and the coverage the oracle finds for it (ran, several calls, another pair wins, EPA pair wins)
BENCH = {
    ("fr3", 1): (45, (1, 0, 1, 0)), ("fr3", 65): (16, (3, 0, 1, 2)), ("fr3", 512): (1, (3, 1, 1, 2)),
    ("ur5e", 1): (2, (1, 0, 0, 1)), ("ur5e", 65): (1, (8, 1, 1, 6)), ("ur5e", 512): (1, (48, 4, 2, 48)),
    ("husky_fr3", 1): (7, (1, 1, 0, 1)), ("husky_fr3", 65): (1, (8, 6, 2, 6)), ("husky_fr3", 512): (1, (40, 24, 12, 24)),
}


@pytest.mark.parametrize("B", [1, 65, 512])
@pytest.mark.parametrize("robot", ["fr3", "ur5e", "husky_fr3"])
def test_bench_stress_workload(cuda, robot, B):
    rd, ctrl, om = _robot(robot, cuda)
    seed, want = BENCH[(robot, B)]
    q, qd, xt, xdt = (moma_step_inputs if robot in MOMA else step_inputs)(rd, robot, seed, B, cuda, stress=True)
    cover("bench %s B=%d" % (robot, B), census(om, q), *want)

    def run():
        r = _solve(ctrl, rd, 0, q, qd, xt, xdt, LINK[robot], "pipeline_")
        if B == 65:
            r.update(_solve(ctrl, rd, 1, q, qd, xt, xdt, LINK[robot], "fused_"))
        r.update(_stages(rd, q, qd, xt, xdt, LINK[robot]))
        return r
    assert_same_bits(*both_layouts(rd, run))


# ---------------------------------------------------------------- the tangled model
def test_tangled_model_several_epa_pairs(cuda, tmp_path):
    """36 boxes, 540 pairs, no closed form: several pairs of one instance reach EPA."""
    urdf = str(tmp_path / "tangle.urdf")
    tangle_urdf(urdf)
    rd = manipulator.RobotData(urdf, "", device=cuda)
    ctrl = manipulator.RobotController(0.001, rd, solver_mode="exact")
    _, om, _ = O.load_paths(urdf, None, dict(ee="link6", kind=0))
    B = 64
    q = np.random.default_rng(11).uniform(-2.4, 2.4, (6, B))
    qd = np.zeros((6, B))
    xt = np.tile(np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0.1, 0.1, 0.2], float)[:, None], (1, B))
    xdt = np.zeros((6, B))
    cover("tangle", census(om, q), ran=32, multi=8, other=0, won=32)

    def run():
        r = _solve(ctrl, rd, 0, q, qd, xt, xdt, "link6", "pipeline_")
        r.update(_stages(rd, q, qd, xt, xdt, "link6"))
        return r
    assert_same_bits(*both_layouts(rd, run))


# ---------------------------------------------------------------- obstacle slots, with and without twists
def _slot_scene(cuda, B):
    """The four slots of tests/test_gpu_obstacles.py, the sphere, box and cylinder
    posed on the arm's links so that they penetrate them, the half-space far
    below (the oracle's twin holds it as a box: kept out of every search)."""
    rd0 = make_manipulator("fr3", cuda)
    q, qd, xt, xdt = step_inputs(rd0, "fr3", 5, B, cuda)
    pm, om, spec, g0 = OB.twin("fr3", OB.FOUR_TYPES, OB.FOUR_PARAMS, OB.FR3_ARM_LINKS)
    rng = np.random.default_rng(23)
    poses = OB.fr3_scene(11, B)
    for b in range(B):
        for i, joint in ((0, 4), (1, 5), (2, 6)):   # centred near a joint frame of the arm: inside its links
            T = O.joint_placement(om, q[:, b], joint)
            poses[b, i, 9:12] = np.asarray(T)[:3, 3] + rng.uniform(-0.05, 0.05, 3)
        poses[b, 3, :9] = np.eye(3).reshape(-1)
        poses[b, 3, 9:12] = (0.0, 0.0, -5.0)
    return q, qd, xt, xdt, poses, om, g0, len(pm.pairs)


@pytest.mark.parametrize("rate", [False, True], ids=["obst", "rate"])
def test_obstacle_slots_penetrating_links(cuda, rate):
    B = 64
    if "slots" not in _CACHE:
        rd = make_manipulator("fr3", cuda)
        rd.set_obstacles(OB.FOUR_TYPES, OB.FOUR_PARAMS, OB.FR3_ARM_LINKS)
        ctrl = manipulator.RobotController(0.001, rd, solver_mode="exact")
        q, qd, xt, xdt, poses, om, g0, p0 = _slot_scene(cuda, B)
        rows = census(om, q, lambda b: OB.set_poses(om, g0, OB.FOUR_TYPES, poses[b]))
        _CACHE["slots"] = (rd, ctrl, q, qd, xt, xdt, poses, rows, p0)
    rd, ctrl, q, qd, xt, xdt, poses, rows, p0 = _CACHE["slots"]
    cover("slots rate=%d" % rate, rows, ran=32, multi=8, other=16, won=1)
    # the rate build's own read of the poses after EPA: EPA ran and a slot pair wins
    assert sum(r[0] > 0 and r[2] >= p0 for r in rows) >= 4
    kw = dict(obstacle_pose=OB.to_field_major(poses))
    if rate:
        kw["obstacle_twist"] = OB.to_field_major(np.random.default_rng(77).uniform(-1, 1, (B, 4, 6)))

    def run():
        r = _solve(ctrl, rd, 0, q, qd, xt, xdt, LINK["fr3"], "pipeline_", **kw)
        r.update(_solve(ctrl, rd, 1, q, qd, xt, xdt, LINK["fr3"], "fused_", **kw))
        r.update(_stages(rd, q, qd, xt, xdt, LINK["fr3"], **kw))
        return r
    assert_same_bits(*both_layouts(rd, run))


# ---------------------------------------------------------------- hull build
@pytest.mark.parametrize("case", ["another pair wins", "hull pair wins"])
def test_hull_model(cuda, tmp_path, case):
    """FR3 with the box of its collision model (on fr3_link7) as a convex hull
    (the hull build of the task stage) on stress-tier states: the oracle's
    census of the primitive twin says where links overlap (a hull of a box is
    that box).  One seed has an instance where EPA ran and another pair wins;
    the other one where the hull overlaps a link, reaches EPA and wins."""
    from test_gpu_mesh_model import _box_as_mesh_urdf
    B = 32
    rd0, _, om = _robot("fr3", cuda)
    seed, want, hull_wins = HULL[case]
    q, qd, xt, xdt = step_inputs(rd0, "fr3", seed, B, cuda, stress=True)
    rows = census(om, q)
    cover("hull, " + case, rows, *want)
    box = [g for g in range(om.ngeom) if om.gtype[g] == OB.BOX]
    assert len(box) == 1   # the geometry _box_as_mesh_urdf turns into the hull
    assert sum(bool(r[1]) and box[0] in (om.pair_a[r[2]], om.pair_b[r[2]]) for r in rows) >= hull_wins
    urdf, _ = _box_as_mesh_urdf(tmp_path, "fr3", "package://pkg/meshes/box.stl")
    rd = manipulator.RobotData(urdf, robot_path("fr3", "srdf"), str(tmp_path), device=cuda)
    ctrl = manipulator.RobotController(0.001, rd, solver_mode="exact")

    def run():
        r = _solve(ctrl, rd, 0, q, qd, xt, xdt, LINK["fr3"], "pipeline_")
        r.update(_solve(ctrl, rd, 1, q, qd, xt, xdt, LINK["fr3"], "fused_"))
        r.update(_stages(rd, q, qd, xt, xdt, LINK["fr3"]))
        return r
    assert_same_bits(*both_layouts(rd, run))


# case -> seed, coverage, instances won by an EPA pair that holds the hull
HULL = {"another pair wins": (19, (2, 0, 1, 1), 0), "hull pair wins": (17, (1, 0, 0, 1), 1)}


# ---------------------------------------------------------------- other users of the plan
QPID = (16, (3, 0, 1, 2))
ROLLOUT = (16, (3, 0, 1, 2))


def test_qpid_stage(cuda):
    """task_kernel<1>: the QPID extras read the winner's witnesses after the refinement."""
    B = 65
    rd, ctrl, om = _robot("fr3", cuda)
    seed, want = QPID
    q, qd, xt, xdt = step_inputs(rd, "fr3", seed, B, cuda, stress=True)
    cover("qpid", census(om, q), *want)
    p = ctrl._pbd.params(LINK["fr3"], _capi.MODE_QPID_STEP, ctrl.Kp_task_, ctrl.Kv_task_)
    a = lambda v: _batch.as_device(v, cuda)

    def run():
        r = {"qpid_%d" % i: v.cpu().numpy() for i, v in enumerate(ctrl.QPID_step_batch(q, qd, xt, xdt, LINK["fr3"]))}
        st = _batch.qpid_stages_batch(rd.model, p, a(q), a(qd), a(xt), a(xdt))
        _sync()
        r.update({"stage_" + k: v.cpu().numpy() for k, v in st.items()})
        return r
    assert_same_bits(*both_layouts(rd, run))


def test_rollout_of_four_steps(cuda):
    """The closed-loop kernel lays the task record into the task plan's overlay."""
    import torch
    B = 64
    rd, ctrl, om = _robot("fr3", cuda)
    seed, want = ROLLOUT
    q, qd, xt, xdt = step_inputs(rd, "fr3", seed, B, cuda, stress=True)
    cover("rollout (first step)", census(om, q), *want)
    want_fields = _batch.ROLLOUT_FIELDS

    def run():
        res = ctrl.QPIK_rollout_batch(q, qd, xt, xdt, LINK["fr3"], 4, mode="step", want=want_fields)
        torch.cuda.synchronize()
        return {k: getattr(res, k).cpu().numpy() for k in ("q_final", "qdot_final", "status_traj") + want_fields}
    assert_same_bits(*both_layouts(rd, run))
