"""Goal-reaching rollouts through waypoints (drc_qpik_reach_path_batch,
QPIK_reach_path_batch) against W chained drc_qpik_reach_batch calls and against
the caller's own loop over the existing entries.

The contract is bitwise.  The chain (_chain) is what a caller does today: one
reach call per waypoint, each from the previous finals, numpy masks keeping
the instances whose previous result is REACHED; every field of the
ReachPathResult except dist_min (a reach call reports d only where it stops)
must equal it (test 1; with obstacle slots 4; a hull model 5).  The loop
(_loop) does per step what include/drc_amd.h states, with the stage entry, the
single-step entry and a one-step rollout, and gives dist_min too (test 2).  The
persistent kernel (reach_path_kernel.hip), the stepwise path (drc_set_fusion 0)
and every batch size return the same bits (tests 3, 4).

Inputs: gains, dt, tolerances and the 40 steps per segment are those of
tests/test_gpu_reach.py; waypoint 0's goal is its census goal, goal w >= 1 is
goal w - 1 plus numpy.random.default_rng(100000 + i).uniform(-0.15, 0.15, nv),
drawn consecutively; the targets are the device's stage poses at the goals.
On the CPU oracle, W = 3 and 64 instances: FR3 reaches all three with 43
(waypoints_reached 0/1/2/3: 11/6/4/43; 20 QP failed, 1 out of budget), UR5e
with 28 of 64 (23/9/4/28; 16, 20).  The mobile manipulators' shares, from the
chained reach calls on the device with the three by-hand instances of test 1:
Husky-FR3 62 of 64 (0/2/0/62; none failed, 2 out of budget), XLS-FR3 28 of 32
(1/1/2/28; none, 4), Caster-FR3 22 of 32 (3/4/3/22; none, 10); there FR3 gives
42 of 64 (11/7/4/42; 20, 2) and UR5e 12 of its first 32 (9/7/4/12; 12, 8)."""
import ctypes as C
import re

import numpy as np
import pytest

import _reach as RC
import test_gpu_reach as TR
from _common import LINK
from _mesh_io import box_triangles, write_stl_ascii
from dyros_robot_controller_amd import _batch, _capi, manipulator, robot_path

pytestmark = pytest.mark.gpu

POS_TOL, ROT_TOL, MAX_STEPS = TR.POS_TOL, TR.ROT_TOL, TR.MAX_STEPS
REQUIRED = ("q_final", "qdot_final", "result", "waypoints_reached", "steps_used")
FIELDS = REQUIRED + _batch.REACH_PATH_FIELDS
CHAIN_FIELDS = tuple(k for k in FIELDS if k != "dist_min")
_PATHS = {}


def _path_inputs(S, B, W, obstacle_pose=None):
    """(q0, v0, x_path [W][12][B], xdot_path [W][6][B]) of the first B instances."""
    rd = S["rd"]
    lo, hi = rd.get_joint_position_limit() if S["moma"] else rd.getJointPositionLimit()
    q0, goal = RC.census_states(lo, hi, B)
    rng = [np.random.default_rng(100000 + i) for i in range(B)]
    z, xdt = np.zeros_like(q0), np.zeros((6, B))
    x_path = []
    for w in range(W):
        if w:
            goal = goal + np.stack([r.uniform(-0.15, 0.15, q0.shape[0]) for r in rng], axis=1)
        x_path.append(TR._stage(S, goal, z, np.zeros((12, B)), xdt, obstacle_pose)[0])
    return q0, z, np.stack(x_path), np.zeros((W, 6, B))


def _setup(robot, cuda, B, W=3):
    """test_gpu_reach's model and parameters with path inputs (shared, never modified)."""
    key = (robot, B, W)
    if key not in _PATHS:
        S = dict(TR._setup(robot, cuda, B))
        S["q"], S["v"], S["xp"], S["xdp"] = _path_inputs(S, B, W)
        _PATHS[key] = S
    return _PATHS[key]


def _np(res):
    TR._sync()
    return {k: (None if getattr(res, k) is None else getattr(res, k).cpu().numpy()) for k in FIELDS}


def _path(S, q=None, v=None, xp=None, xdp=None, max_steps=MAX_STEPS, p=None, obstacle_pose=None, **kw):
    a = lambda t: _batch.as_device(np.array(t), S["dev"])
    q, v = (S["q"] if q is None else q), (S["v"] if v is None else v)
    xp, xdp = (S["xp"] if xp is None else xp), (S["xdp"] if xdp is None else xdp)
    res = _batch.qpik_reach_path_batch(S["rd"].model, S["p"] if p is None else p, a(q), a(v), a(xp), a(xdp), max_steps,
                                       S["dt"], POS_TOL, ROT_TOL, obstacle_pose=obstacle_pose, **kw)
    assert res.thresholds == RC.thresholds(POS_TOL, ROT_TOL)
    return _np(res)


def _empty(B, nv, W):
    return dict(result=np.full(B, -1, np.int32), waypoints_reached=np.zeros(B, np.int32),
                steps_used=np.zeros(B, np.int32), status_last=np.zeros(B, np.int32), iters_total=np.zeros(B, np.int32),
                err_final=np.zeros((2, B)), dist_final=np.zeros((1 + nv, B)), dist_min=np.full(B, np.inf),
                steps_at=np.full((W, B), -1, np.int32))


def _chain(S, q0, v0, xp, xdp, max_steps=MAX_STEPS, p=None, obstacle_pose=None):
    """W chained reach calls on the whole batch, numpy masks carrying the state
    of the instances that reached the previous waypoint (module docstring)."""
    W, B, nv = xp.shape[0], q0.shape[1], q0.shape[0]
    q, v = q0.copy(), v0.copy()
    out = _empty(B, nv, W)
    del out["dist_min"]
    alive = np.ones(B, bool)
    for w in range(W):
        r = TR._reach(S, q=q, v=v, xt=xp[w], xdt=xdp[w], max_steps=max_steps, p=p, obstacle_pose=obstacle_pose)
        q[:, alive], v[:, alive] = r["q_final"][:, alive], r["qdot_final"][:, alive]
        out["result"][alive] = r["result"][alive]
        out["steps_used"][alive] += r["steps_used"][alive]
        ran = alive & (r["status_last"] != 0)   # (a call in which no QP ran leaves the last status)
        out["status_last"][ran] = r["status_last"][ran]
        out["iters_total"][alive] += r["iters_total"][alive]
        out["err_final"][:, alive] = r["err_final"][:, alive]
        out["dist_final"][:, alive] = r["dist_final"][:, alive]
        alive = alive & (r["result"] == RC.REACHED)
        out["steps_at"][w, alive] = out["steps_used"][alive]
        out["waypoints_reached"][alive] += 1
    out["q_final"], out["qdot_final"] = q, v
    return out


def _loop(S, q0, v0, xp, xdp, max_steps=MAX_STEPS):
    """The caller's own loop over the stage entry, the single-step entry and a
    one-step rollout: _loop of test_gpu_reach.py with the waypoint rule."""
    import torch
    p, model, dev = S["p"], S["rd"].model, S["dev"]
    a = lambda t: _batch.as_device(t, dev)
    tau_p, tau_r = RC.thresholds(POS_TOL, ROT_TOL)
    W, B, nv = xp.shape[0], q0.shape[1], q0.shape[0]
    ar = np.arange(B)
    q, v = q0.copy(), v0.copy()
    out = _empty(B, nv, W)
    w, s, k = out["waypoints_reached"], np.zeros(B, np.int32), out["steps_used"]
    active = np.ones(B, bool)
    target = lambda path: np.ascontiguousarray(path[np.minimum(w, W - 1), :, ar].T)

    def stop(mask, code, err, dist):
        out["result"][mask] = code
        out["err_final"][:, mask] = err[:, mask]
        out["dist_final"][:, mask] = dist[:, mask]

    while active.any():
        xt, xdt = target(xp), target(xdp)
        pose, dist = TR._stage(S, q, v, xt, xdt)
        lower = active & (dist[0] < out["dist_min"])
        out["dist_min"][lower] = dist[0][lower]
        err, todo = np.zeros((2, B)), active.copy()
        while todo.any():   # waypoint w and, while the pose is within, the next ones
            e = np.stack(RC.reach_error(pose, target(xp)))
            err[:, todo] = e[:, todo]
            within = todo & (e[0] <= tau_p) & (e[1] <= tau_r)
            out["steps_at"][w[within], ar[within]] = k[within]
            w[within] += 1
            s[within] = 0
            done = within & (w == W)
            stop(done, RC.REACHED, err, dist)
            active &= ~done
            todo = within & ~done
        spent = active & (s == max_steps)
        stop(spent, RC.BUDGET, err, dist)
        active &= ~spent
        if not active.any():
            break
        xt, xdt = target(xp), target(xdp)
        it = torch.zeros(B, dtype=torch.int32, device=dev)
        _, st = _batch.qpik_batch(model, p, a(q), a(v), a(xt), a(xdt), iters=it)
        TR._sync()
        st, it = st.cpu().numpy(), it.cpu().numpy()
        out["status_last"][active] = st[active]
        out["iters_total"][active] += it[active]
        failed = active & (st != _capi.STATUS_SOLVED)
        stop(failed, RC.QP_FAILED, err, dist)
        active &= ~failed
        r = _batch.qpik_rollout_batch(model, p, a(q), a(v), 1, S["dt"], a(xt), a(xdt), want=())
        TR._sync()
        q[:, active] = r.q_final.cpu().numpy()[:, active]
        v[:, active] = r.qdot_final.cpu().numpy()[:, active]
        k[active] += 1
        s[active] += 1
    out["q_final"], out["qdot_final"] = q, v
    return out


def _assert_same(a, b, fields=FIELDS, msg=""):
    for k in fields:
        np.testing.assert_array_equal(a[k], b[k], err_msg="%s %s" % (k, msg))


def _assert_consistent(r, W):
    """err_final lies under the thresholds exactly for the REACHED instances,
    who passed every waypoint; steps_at counts up and ends with the -1s."""
    tau_p, tau_r = RC.thresholds(POS_TOL, ROT_TOL)
    under = (r["err_final"][0] <= tau_p) & (r["err_final"][1] <= tau_r)
    reached = r["result"] == RC.REACHED
    np.testing.assert_array_equal(under, reached)
    np.testing.assert_array_equal(r["waypoints_reached"] == W, reached)
    assert set(np.unique(r["result"])) <= {RC.REACHED, RC.BUDGET, RC.QP_FAILED}
    np.testing.assert_array_equal((r["steps_at"] >= 0).sum(axis=0), r["waypoints_reached"])
    at = np.where(r["steps_at"] >= 0, r["steps_at"], r["steps_used"][None])
    assert np.all(np.diff(at, axis=0) >= 0) and np.all(at[-1] <= r["steps_used"])
    assert np.all(r["dist_min"] <= r["dist_final"][0])


# 1 ------------------------------------------------------------------------
@pytest.mark.parametrize("robot,B", [("fr3", 64), ("husky_fr3", 64), ("ur5e", 32), ("xls_fr3", 32),
                                     ("caster_fr3", 32)])
def test_against_chained_reach_calls(cuda, robot, B):
    W = 3
    S = _setup(robot, cuda, B)
    q0, v0, xp, xdp = S["q"], S["v"], S["xp"].copy(), S["xdp"]
    # by hand: instance 0 starts on waypoint 0; instance 1's waypoint 1 is a copy of its waypoint 0;
    # instance 2's waypoint 1 lies five metres below the floor
    xp[0][:, 0] = TR._stage(S, q0, v0, xp[0], xdp[0])[0][:, 0]
    xp[1][:, 1] = xp[0][:, 1]
    xp[1][11, 2] = -5.0
    got = _path(S, xp=xp)
    ref = _chain(S, q0, v0, xp, xdp)
    ok = got["result"] == RC.REACHED
    print("%s: reached all %d of %d, waypoints_reached 0/1/2/3 %s, QP failed %d, budget %d, steps per segment %s" % (
        robot, ok.sum(), B, np.bincount(got["waypoints_reached"], minlength=W + 1).tolist(),
        (got["result"] == RC.QP_FAILED).sum(), (got["result"] == RC.BUDGET).sum(),
        sorted(set(np.diff(got["steps_at"][:, ok], axis=0, prepend=0).ravel().tolist()))))
    _assert_same(got, ref, CHAIN_FIELDS)
    _assert_consistent(got, W)
    assert got["steps_at"][0, 0] == 0
    assert got["steps_at"][1, 1] == got["steps_at"][0, 1]
    assert got["result"][2] == RC.BUDGET and got["waypoints_reached"][2] == 1, (got["result"][2], got["steps_at"][:, 2])
    assert got["steps_used"][2] == got["steps_at"][0, 2] + MAX_STEPS
    if robot == "fr3":
        assert ok.sum() >= 32, got["waypoints_reached"]
        assert set(got["waypoints_reached"]) == {0, 1, 2, 3}
    moved = got["steps_used"] > 0
    assert np.abs(got["q_final"][:, moved] - q0[:, moved]).max() > 0
    # W = 1 is drc_qpik_reach_batch itself
    one, reach = _path(S, xp=xp[:1], xdp=xdp[:1]), TR._reach(S, xt=xp[0], xdt=xdp[0])
    _assert_same(one, reach, TR.FIELDS, "W = 1")
    np.testing.assert_array_equal(one["waypoints_reached"], reach["result"] == RC.REACHED)
    np.testing.assert_array_equal(one["steps_at"][0], np.where(reach["result"] == RC.REACHED, reach["steps_used"], -1))
    # without the optional outputs: the same required ones
    none = _path(S, xp=xp, want=())
    assert all(none[k] is None for k in _batch.REACH_PATH_FIELDS)
    _assert_same(got, none, REQUIRED)
    # max_steps = 0 moves nothing: it walks through the waypoints already satisfied
    zero = _path(S, xp=xp, max_steps=0)
    _assert_same(zero, _chain(S, q0, v0, xp, xdp, max_steps=0), CHAIN_FIELDS, "max_steps = 0")
    assert zero["waypoints_reached"][0] >= 1 and not zero["waypoints_reached"][1:].any()
    assert not zero["steps_used"].any() and not zero["status_last"].any() and not zero["iters_total"].any()
    np.testing.assert_array_equal(zero["q_final"], q0)
    np.testing.assert_array_equal(zero["qdot_final"], v0)


# 2 ------------------------------------------------------------------------
def test_against_the_callers_own_loop(cuda):
    S = _setup("fr3", cuda, 64)
    got = _path(S)
    _assert_same(got, _loop(S, S["q"], S["v"], S["xp"], S["xdp"]))
    _assert_consistent(got, 3)
    assert np.all(np.isfinite(got["dist_min"])) and (got["dist_min"] < got["dist_final"][0]).any()


# 3 ------------------------------------------------------------------------
@pytest.mark.parametrize("robot", ["fr3", "xls_fr3"])
def test_path_and_batch_size_independence(cuda, robot):
    """B = 2 100: the smallest batch at which a wave of the 2 048-wave grid
    takes a second instance (state carried over between instances would show)."""
    S = _setup(robot, cuda, 2100)
    K, W = 12, 3
    full = {}
    try:
        for fused in (1, 0):
            TR._set_fusion(S, fused)
            full[fused] = _path(S, max_steps=K)
        _assert_same(full[1], full[0])
        for B in (1, 70):
            cut = lambda t: np.ascontiguousarray(t[..., :B])
            for fused in (1, 0):
                TR._set_fusion(S, fused)
                r = _path(S, q=cut(S["q"]), v=cut(S["v"]), xp=cut(S["xp"]), xdp=cut(S["xdp"]), max_steps=K)
                for k in FIELDS:
                    np.testing.assert_array_equal(r[k], full[1][k][..., :B], err_msg="%s B=%d fused=%d" % (k, B, fused))
        # in place: q_final / qdot_final are the inputs themselves
        for fused in (1, 0):
            TR._set_fusion(S, fused)
            a = lambda t: _batch.as_device(np.array(t), cuda)
            q, v, xp, xdp = a(S["q"]), a(S["v"]), a(S["xp"]), a(S["xdp"])
            res = _batch.qpik_reach_path_batch(S["rd"].model, S["p"], q, v, xp, xdp, K, S["dt"], POS_TOL, ROT_TOL,
                                               q_final=q, qdot_final=v)
            assert res.q_final.data_ptr() == q.data_ptr() and res.qdot_final.data_ptr() == v.data_ptr()
            _assert_same(full[1], _np(res), msg="in place, fused=%d" % fused)
            np.testing.assert_array_equal(xp.cpu().numpy(), S["xp"])  # the other inputs are never written
            np.testing.assert_array_equal(xdp.cpu().numpy(), S["xdp"])
    finally:
        TR._set_fusion(S, 1)
    r = full[1]
    _assert_consistent(r, W)
    budget = r["result"] == RC.BUDGET
    assert budget.any()
    seg0 = np.where(r["waypoints_reached"] > 0, r["steps_at"][np.maximum(r["waypoints_reached"] - 1, 0), np.arange(2100)], 0)
    np.testing.assert_array_equal((r["steps_used"] - seg0)[budget], K)   # the budget is per segment
    if robot == "fr3":   # (FR3 needs 9 steps and more per segment; the mobile manipulators more than 12)
        assert (r["waypoints_reached"] > 1).any() and (r["steps_used"] > K).any()


def test_the_last_round_settles_the_worst_case(cuda):
    """The stepwise path enqueues R0 = W max_steps + W - 1 rounds with a QP and
    one that settles (api.cpp reach_path_locked).  W = 2, max_steps = 1: an
    instance that steps (round 0), comes within waypoint 0 (round 1), steps
    towards waypoint 1 (round 2) and is out of budget uses all R0 = 3 rounds, one
    event in each, and takes its verdict from the settling round."""
    B, W = 4, 2
    S = TR._setup("fr3", cuda, 70)
    q, v, xt, xdt = (np.ascontiguousarray(S[k][:, :B]) for k in ("q", "v", "xt", "xdt"))
    # every instance's errors at the start and after one step towards its census target
    e0 = TR._reach(S, q=q, v=v, xt=xt, xdt=xdt, max_steps=0)["err_final"]
    e1 = TR._reach(S, q=q, v=v, xt=xt, xdt=xdt, max_steps=1)["err_final"]
    fell = np.all(e1 < e0, axis=0)
    # one tolerance pair with the start outside and the state after one step inside: the pair between the two
    # states of an instance (geometric means of its errors), that of the instance it separates the most for
    best, tol = np.zeros(B, bool), None
    for i in np.flatnonzero(fell):
        pos_tol = float(np.sqrt(np.sqrt(e0[0, i] * e1[0, i])))
        rot_tol = float(2.0 * np.arcsin(np.sqrt(np.sqrt(e0[1, i] * e1[1, i]) / 8.0)))
        tau_p, tau_r = RC.thresholds(pos_tol, rot_tol)
        sep = fell & ~((e0[0] <= tau_p) & (e0[1] <= tau_r)) & (e1[0] <= tau_p) & (e1[1] <= tau_r)
        if sep.sum() > best.sum():
            best, tol = sep, (pos_tol, rot_tol)
    print("errors at the start %s, after one step %s, separated %s by %s" % (e0.tolist(), e1.tolist(), best, tol))
    assert best.any()
    xp = np.stack([xt, xt])
    xp[1][11] -= 5.0   # five metres below the floor
    xdp = np.zeros((W, 6, B))
    a = lambda t: _batch.as_device(np.array(t), cuda)
    got = {}
    try:
        for fused in (1, 0):
            TR._set_fusion(S, fused)
            got[fused] = _np(_batch.qpik_reach_path_batch(S["rd"].model, S["p"], a(q), a(v), a(xp), a(xdp), 1, S["dt"],
                                                          *tol))
    finally:
        TR._set_fusion(S, 1)
    r = got[0]
    assert set(np.unique(r["result"])) <= {RC.REACHED, RC.BUDGET, RC.QP_FAILED}, r["result"]   # none left at -1
    np.testing.assert_array_equal(r["waypoints_reached"][best], 1)
    np.testing.assert_array_equal(r["steps_used"][best], 2)
    np.testing.assert_array_equal(r["result"][best], RC.BUDGET)
    np.testing.assert_array_equal(r["steps_at"][:, best], np.repeat([[1], [-1]], best.sum(), axis=1))
    _assert_same(r, got[1])


# 4 ------------------------------------------------------------------------
def _fr3_obstacles(cuda):
    if "obst" not in _PATHS:
        S = dict(TR._fr3_obstacles(cuda))
        S["q"], S["v"], S["xp"], S["xdp"] = _path_inputs(S, 32, 2, S["poses"])
        _PATHS["obst"] = S
    return _PATHS["obst"]


@pytest.mark.parametrize("shared", [False, True])
def test_obstacle_slots(cuda, shared):
    S = _fr3_obstacles(cuda)
    pose = np.ascontiguousarray(S["poses"][:, :, 5]) if shared else S["poses"]
    got = {}
    try:
        for fused in (1, 0):
            TR._set_fusion(S, fused)
            got[fused] = _path(S, obstacle_pose=pose)
    finally:
        TR._set_fusion(S, 1)
    _assert_same(got[1], got[0])
    got = got[1]
    _assert_same(got, _chain(S, S["q"], S["v"], S["xp"], S["xdp"], obstacle_pose=pose), CHAIN_FIELDS)
    _assert_consistent(got, 2)
    assert (got["steps_used"] > 0).any()
    if shared:   # passed shared or replicated per instance: the same bits
        repl = _path(S, obstacle_pose=np.ascontiguousarray(np.repeat(pose[:, :, None], 32, axis=2)))
        _assert_same(got, repl)
    else:        # (the poses matter: the slot-free model's distance stage differs)
        free = _path(TR._setup("fr3", cuda, 70), q=S["q"], v=S["v"], xp=S["xp"], xdp=S["xdp"])
        assert not np.array_equal(free["dist_min"], got["dist_min"])


# 5 ------------------------------------------------------------------------
def test_urdf_with_a_collision_mesh(cuda, tmp_path):
    """The hull model of test_gpu_reach.py: the stepwise dispatch."""
    text = open(robot_path("fr3")).read()
    m = re.search(r'<box size="([^"]+)"/>', text)
    size = np.array([float(x) for x in m.group(1).split()])
    (tmp_path / "pkg" / "meshes").mkdir(parents=True)
    write_stl_ascii(tmp_path / "pkg" / "meshes" / "box.stl", box_triangles(0.5 * size).reshape(-1, 3))
    (tmp_path / "pkg" / "urdf").mkdir()
    urdf = tmp_path / "pkg" / "urdf" / "fr3_mesh.urdf"
    urdf.write_text(text[:m.start()] + '<mesh filename="package://pkg/meshes/box.stl"/>' + text[m.end():])
    rd = manipulator.RobotData(str(urdf), robot_path("fr3", "srdf"), str(tmp_path), device=cuda)
    ctrl = manipulator.RobotController(0.001, rd, solver_mode="exact")
    p, dt = TR._params(ctrl, LINK["fr3"], False)
    S = dict(robot="fr3", rd=rd, ctrl=ctrl, p=p, dt=dt, moma=False, dev=cuda)
    S["q"], S["v"], S["xp"], S["xdp"] = _path_inputs(S, 8, 2)
    got = _path(S)
    _assert_same(got, _chain(S, S["q"], S["v"], S["xp"], S["xdp"]), CHAIN_FIELDS)
    _assert_consistent(got, 2)
    assert (got["waypoints_reached"] == 2).any()


@pytest.mark.parametrize("robot", ["fr3", "caster_fr3"])
def test_qp_failed(cuda, robot):
    """The reference's solver settings cut to one ADMM iteration (test_qp_failed
    of test_gpu_reach.py): every instance fails at its first QP."""
    import torch
    B = 32
    S = _setup(robot, cuda, B)
    pb = manipulator.QPIKParamsBuilder(S["rd"].model, exact=False)
    p = pb.params(LINK[robot], _capi.MODE_QPIK_STEP, *(() if S["moma"] else (np.full(6, 100.0), np.zeros(6))))
    if S["moma"]:
        for i in range(6):
            p.kv[i] = 0.0
    p.solver.max_iter = 1
    a = lambda t: _batch.as_device(t, cuda)
    it = torch.zeros(B, dtype=torch.int32, device=cuda)
    _, st = _batch.qpik_batch(S["rd"].model, p, a(S["q"]), a(S["v"]), a(S["xp"][0]), a(S["xdp"][0]), iters=it)
    TR._sync()
    st = st.cpu().numpy()
    assert np.all(st != _capi.STATUS_SOLVED), st
    for fused in (1, 0):
        TR._set_fusion(S, fused)
        try:
            r = _path(S, p=p)
        finally:
            TR._set_fusion(S, 1)
        np.testing.assert_array_equal(r["result"], np.full(B, RC.QP_FAILED))
        assert not r["steps_used"].any() and not r["waypoints_reached"].any()
        np.testing.assert_array_equal(r["steps_at"], np.full((3, B), -1))
        np.testing.assert_array_equal(r["status_last"], st)
        np.testing.assert_array_equal(r["iters_total"], it.cpu().numpy())
        np.testing.assert_array_equal(r["q_final"], S["q"])
        np.testing.assert_array_equal(r["qdot_final"], S["v"])
        np.testing.assert_array_equal(r["dist_min"], r["dist_final"][0])


def test_error_codes(cuda):
    import torch
    S = _setup("fr3", cuda, 64)
    O = _fr3_obstacles(cuda)
    B, W = 4, 2
    a = lambda t: _batch.as_device(np.ascontiguousarray(t[..., :B]), cuda)
    q, v, xp, xdp = a(S["q"]), a(S["v"]), a(S["xp"][:W]), a(S["xdp"][:W])
    qf, vf = torch.empty_like(q), torch.empty_like(v)
    res, wr, steps = (torch.empty(B, dtype=torch.int32, device=cuda) for _ in range(3))
    op = _batch.as_device(np.ascontiguousarray(O["poses"][:, :, :B]), cuda)
    stream = C.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    lib = _capi.lib()

    def call(model=S, obstacles=False, mode=_capi.MODE_QPIK_STEP, B=B, W=W, max_steps=2, dt=0.005, pos_tol=POS_TOL,
             rot_tol=ROT_TOL, q=q, v=v, xp=xp, xdp=xdp, qf=qf, vf=vf, res=res, wr=wr, steps=steps, op=op, ld=B):
        p = model["ctrl"]._pb.params(LINK["fr3"], mode, np.full(6, 100.0), np.zeros(6))
        head = (model["rd"].model.handle, C.byref(p), C.c_int64(B), C.c_int(W), C.c_int(max_steps), C.c_double(dt),
                C.c_double(pos_tol), C.c_double(rot_tol), ptr(q), ptr(v), ptr(xp), ptr(xdp))
        tail = (ptr(qf), ptr(vf), ptr(res), ptr(wr), ptr(steps), None, None, None, None, None, None, stream)
        if obstacles:
            return lib.drc_qpik_reach_path_obstacles_batch(*head, ptr(op), C.c_int64(ld), *tail)
        return lib.drc_qpik_reach_path_batch(*head, *tail)

    ok, bad = _capi.DRC_OK, _capi.DRC_ERR_INVALID_ARGUMENT
    assert call() == ok
    assert call(model=O, obstacles=True) == ok
    assert call(model=O, obstacles=True, ld=0) == ok
    assert call(W=0) == bad and call(W=-1) == bad and call(W=1) == ok
    assert call(mode=_capi.MODE_QPIK) == bad and call(mode=_capi.MODE_QPIK_CUBIC) == bad
    assert "DRC_MODE_QPIK_STEP" in lib.drc_last_error().decode()
    assert call(max_steps=-1) == bad and call(max_steps=0) == ok
    for x in (0.0, -1e-3, float("nan"), float("inf")):
        assert call(dt=x) == bad, x
        assert call(pos_tol=x) == bad, x
        assert call(rot_tol=x) == bad, x
    for k in ("q", "v", "xp", "xdp", "qf", "vf", "res", "wr", "steps"):
        assert call(**{k: None}) == bad, k
    assert call(model=O) == bad   # the plain entry on a model with slots
    assert "drc_qpik_reach_path_obstacles_batch" in lib.drc_last_error().decode()
    assert call(obstacles=True) == bad   # the obstacle entry on a model without
    assert "drc_qpik_reach_path_batch" in lib.drc_last_error().decode()
    assert call(model=O, obstacles=True, op=None) == bad and call(model=O, obstacles=True, ld=B - 1) == bad
    assert call(B=-1) == bad
    assert call(B=0) == ok and call(B=0, q=None, xp=None) == ok
    with pytest.raises(ValueError):
        S["ctrl"].QPIK_reach_path_batch(S["q"], S["v"], S["xp"], LINK["fr3"], 2, want=("q_traj",))
    with pytest.raises(ValueError):
        S["ctrl"].QPIK_reach_path_batch(S["q"], S["v"], S["xp"][0], LINK["fr3"], 2)
    TR._sync()


@pytest.mark.parametrize("robot", ["fr3", "husky_fr3"])
def test_controller_entry(cuda, robot):
    """QPIK_reach_path_batch of both controllers: xdot_path None is zeros, w_reg
    None the default, and the gains are the controller's."""
    S = _setup(robot, cuda, 64)
    c = S["ctrl"]
    kp, kv = c.Kp_task_.copy(), c.Kv_task_.copy()
    try:
        if not S["moma"]:
            c.setTaskGain(np.full(6, 100.0), np.zeros(6))
        res = c.QPIK_reach_path_batch(S["q"], S["v"], S["xp"], LINK[robot], MAX_STEPS, dt=S["dt"],
                                      w_reg=None if S["moma"] else 0.01)
    finally:
        c.Kp_task_, c.Kv_task_ = kp, kv
    assert (res.REACHED, res.BUDGET, res.QP_FAILED) == (0, 1, 2)
    assert res.thresholds == RC.thresholds(POS_TOL, ROT_TOL)
    _assert_same(_np(res), _path(S))
