"""Goal-reaching rollouts with per-instance stopping (drc_qpik_reach_batch,
QPIK_reach_batch) against the caller's own loop over the existing entries.

The contract is bitwise.  The reference loop (_loop) does per step what
include/drc_amd.h states: the stage entry for the pose and the distance at
(q_k, v_k), the error and the verdict in numpy (tests/_reach.py), the
single-step entry for (eta, status, iters), and a one-step rollout for the
state update, whose finals are taken for the instances still active.  Every
field of the ReachResult must equal it (test 1; with obstacle slots 4; a hull
model, which runs step by step, 5), and the persistent kernel
(reach_kernel.hip), the stepwise path (drc_set_fusion 0) and every batch size
return the same bits (test 3).  The entry's host side is the reach path's with
one waypoint (test 8).

Census inputs: instance i draws from numpy.random.default_rng(i) a start in
the middle 40 % of the position limits (clipped to +-3) and a goal within 0.15
per joint of it; v0 = 0; the target is the device's stage pose at the goal;
1e-4 m, 1e-3 rad, 40 steps.  Manipulators: Kp 100, Kv 0, w_reg 0.01, dt 5 ms;
mobile manipulators: the defaults (Kp 400, w_reg 0.01) at dt 1 ms.  On the CPU
oracle these reach 53 / 41 / 64 / 60 / 57 of 64 (FR3, UR5e, Husky-, XLS-,
Caster-FR3); the device's share is asserted to be at least a half."""
import ctypes as C
import re

import numpy as np
import pytest

import _obstacles as OB
import _reach as RC
from _common import LINK, make_manipulator, make_moma
from _mesh_io import box_triangles, write_stl_ascii
from dyros_robot_controller_amd import _batch, _capi, manipulator, mobile_manipulator, robot_path

pytestmark = pytest.mark.gpu

MOMA = ("husky_fr3", "xls_fr3", "caster_fr3")
POS_TOL, ROT_TOL, MAX_STEPS = 1e-4, 1e-3, 40
FIELDS = ("q_final", "qdot_final", "result", "steps_used") + _batch.REACH_FIELDS
_CACHE = {}


def _sync():
    import torch
    torch.cuda.synchronize()


def _params(ctrl, link, moma):
    """The census' gains: QPIKStep parameters and dt."""
    if moma:
        return ctrl._pb.params(link, _capi.MODE_QPIK_STEP, ctrl.Kp_task_, np.zeros(6)), 0.001
    p = ctrl._pb.params(link, _capi.MODE_QPIK_STEP, np.full(6, 100.0), np.zeros(6))
    p.w_reg = 0.01
    return p, 0.005


def _stage(S, q, v, xt, xdt, obstacle_pose=None):
    a = lambda t: _batch.as_device(t, S["dev"])
    st = _batch.stages_batch(S["rd"].model, S["p"], a(q), a(v), a(xt), a(xdt), obstacle_pose=obstacle_pose)
    _sync()
    return st["pose"].cpu().numpy(), st["dist"].cpu().numpy()


def _inputs(S, B, obstacle_pose=None):
    """Census inputs (q0, v0, x_target, xdot_target) of the first B instances."""
    rd = S["rd"]
    lo, hi = rd.get_joint_position_limit() if S["moma"] else rd.getJointPositionLimit()
    q0, qg = RC.census_states(lo, hi, B)
    z = np.zeros_like(q0)
    xdt = np.zeros((6, B))
    xt, _ = _stage(S, qg, z, np.zeros((12, B)), xdt, obstacle_pose)
    return q0, z, xt, xdt


def _setup(robot, cuda, B):
    """Model, controller, parameters and census inputs (shared, never modified)."""
    key = (robot, B)
    if key not in _CACHE:
        moma = robot in MOMA
        base = next((v for (r, _), v in _CACHE.items() if r == robot), None)
        if base is None:
            rd = make_moma(robot, cuda) if moma else make_manipulator(robot, cuda)
            ctrl = (mobile_manipulator if moma else manipulator).RobotController(0.001, rd, solver_mode="exact")
        else:
            rd, ctrl = base["rd"], base["ctrl"]
        p, dt = _params(ctrl, LINK[robot], moma)
        S = dict(robot=robot, rd=rd, ctrl=ctrl, p=p, dt=dt, moma=moma, dev=cuda)
        S["q"], S["v"], S["xt"], S["xdt"] = _inputs(S, B)
        _CACHE[key] = S
    return _CACHE[key]


def _np(res):
    _sync()
    return {k: (None if getattr(res, k) is None else getattr(res, k).cpu().numpy()) for k in FIELDS}


def _reach(S, q=None, v=None, xt=None, xdt=None, max_steps=MAX_STEPS, p=None, obstacle_pose=None, **kw):
    a = lambda t: _batch.as_device(np.array(t), S["dev"])
    q, v = (S["q"] if q is None else q), (S["v"] if v is None else v)
    xt, xdt = (S["xt"] if xt is None else xt), (S["xdt"] if xdt is None else xdt)
    res = _batch.qpik_reach_batch(S["rd"].model, S["p"] if p is None else p, a(q), a(v), a(xt), a(xdt), max_steps,
                                  S["dt"], POS_TOL, ROT_TOL, obstacle_pose=obstacle_pose, **kw)
    assert res.thresholds == RC.thresholds(POS_TOL, ROT_TOL)
    return _np(res)


def _loop(S, q0, v0, xt, xdt, max_steps=MAX_STEPS, p=None, obstacle_pose=None):
    """The caller's own loop over the existing entries (module docstring)."""
    import torch
    p = S["p"] if p is None else p
    model, dev = S["rd"].model, S["dev"]
    a = lambda t: _batch.as_device(t, dev)
    tau_p, tau_r = RC.thresholds(POS_TOL, ROT_TOL)
    B, nv = q0.shape[1], q0.shape[0]
    q, v = q0.copy(), v0.copy()
    out = dict(result=np.full(B, -1, np.int32), steps_used=np.zeros(B, np.int32), status_last=np.zeros(B, np.int32),
               iters_total=np.zeros(B, np.int32), err_final=np.zeros((2, B)), dist_final=np.zeros((1 + nv, B)))
    active = np.ones(B, bool)

    def stop(mask, code, k, err, dist):
        out["result"][mask], out["steps_used"][mask] = code, k
        out["err_final"][:, mask] = np.stack(err)[:, mask]
        out["dist_final"][:, mask] = dist[:, mask]

    for k in range(max_steps + 1):
        pose, dist = _stage(dict(S, p=p), q, v, xt, xdt, obstacle_pose)
        err = RC.reach_error(pose, xt)
        within = (err[0] <= tau_p) & (err[1] <= tau_r)
        stop(active & within, RC.REACHED, k, err, dist)
        active &= ~within
        if k == max_steps:
            stop(active, RC.BUDGET, k, err, dist)
            break
        if not active.any():
            break
        it = torch.zeros(B, dtype=torch.int32, device=dev)
        eta, st = _batch.qpik_batch(model, p, a(q), a(v), a(xt), a(xdt), iters=it, obstacle_pose=obstacle_pose)
        _sync()
        st, it = st.cpu().numpy(), it.cpu().numpy()
        out["status_last"][active] = st[active]
        out["iters_total"][active] += it[active]
        failed = active & (st != _capi.STATUS_SOLVED)
        stop(failed, RC.QP_FAILED, k, err, dist)
        active &= ~failed
        r = _batch.qpik_rollout_batch(model, p, a(q), a(v), 1, S["dt"], a(xt), a(xdt), want=(),
                                      obstacle_pose=obstacle_pose)
        _sync()
        q[:, active] = r.q_final.cpu().numpy()[:, active]
        v[:, active] = r.qdot_final.cpu().numpy()[:, active]
    out["q_final"], out["qdot_final"] = q, v
    return out


def _assert_same(a, b, fields=FIELDS, msg=""):
    for k in fields:
        np.testing.assert_array_equal(a[k], b[k], err_msg="%s %s" % (k, msg))


def _assert_consistent(r):
    """err_final lies under the thresholds exactly for the REACHED instances."""
    tau_p, tau_r = RC.thresholds(POS_TOL, ROT_TOL)
    under = (r["err_final"][0] <= tau_p) & (r["err_final"][1] <= tau_r)
    np.testing.assert_array_equal(under, r["result"] == RC.REACHED)
    assert set(np.unique(r["result"])) <= {RC.REACHED, RC.BUDGET, RC.QP_FAILED}


def _set_fusion(S, on):
    _capi.check(_capi.lib().drc_set_fusion(S["rd"].model.handle, C.c_int(on)))


# 1 ------------------------------------------------------------------------
@pytest.mark.parametrize("robot,B", [("fr3", 70), ("husky_fr3", 70), ("ur5e", 32), ("xls_fr3", 32),
                                     ("caster_fr3", 32)])
def test_against_the_callers_own_loop(cuda, robot, B):
    S = _setup(robot, cuda, B)
    q0, v0, xt, xdt = S["q"], S["v"], S["xt"].copy(), S["xdt"]
    # by hand: instance 0 starts at its target; instances 1 and 2 have it 5 m away and 4 to 5 m below the
    # floor, where no base drives and no arm reaches.  (Along the floor Kp dt = 0.4 takes a mobile base 5 m in
    # 21 steps; 5 m straight up, Caster-FR3's instance 1 meets the ADMM iteration limit at step 20 and
    # stops as QP_FAILED, as it does in the caller's loop.)
    xt[:, 0] = _stage(S, q0, v0, xt, xdt)[0][:, 0]
    xt[11, 1] -= 5.0
    xt[9, 2] += 3.0
    xt[11, 2] -= 4.0
    got = _reach(S, xt=xt)
    ref = _loop(S, q0, v0, xt, xdt)
    print("%s: reached %d of %d, steps %s, budget %d, QP failed %d" % (
        robot, (got["result"] == RC.REACHED).sum(), B,
        sorted(set(got["steps_used"][got["result"] == RC.REACHED]))[::max(1, B // 8)],
        (got["result"] == RC.BUDGET).sum(), (got["result"] == RC.QP_FAILED).sum()))
    _assert_same(got, ref)
    _assert_consistent(got)
    assert got["result"][0] == RC.REACHED and got["steps_used"][0] == 0
    assert got["status_last"][0] == 0 and got["iters_total"][0] == 0
    np.testing.assert_array_equal(got["q_final"][:, 0], q0[:, 0])
    np.testing.assert_array_equal(got["qdot_final"][:, 0], v0[:, 0])
    for b in (1, 2):
        assert got["result"][b] == RC.BUDGET and got["steps_used"][b] == MAX_STEPS, (b, got["result"][b])
    assert 2 * (got["result"] == RC.REACHED).sum() >= B, got["result"]
    moved = got["steps_used"] > 0
    assert np.abs(got["q_final"][:, moved] - q0[:, moved]).max() > 0
    # without the optional outputs: the same required ones
    none = _reach(S, xt=xt, want=())
    assert all(none[k] is None for k in _batch.REACH_FIELDS)
    _assert_same(got, none, ("q_final", "qdot_final", "result", "steps_used"))
    # max_steps = 0 only checks the error
    zero = _reach(S, xt=xt, max_steps=0)
    np.testing.assert_array_equal(zero["result"], np.where(np.arange(B) == 0, RC.REACHED, RC.BUDGET))
    assert not zero["steps_used"].any() and not zero["status_last"].any() and not zero["iters_total"].any()
    np.testing.assert_array_equal(zero["q_final"], q0)
    np.testing.assert_array_equal(zero["qdot_final"], v0)


# 2 ------------------------------------------------------------------------
@pytest.mark.parametrize("robot", ["fr3", "caster_fr3"])
def test_qp_failed(cuda, robot):
    """The reference's solver settings cut to one ADMM iteration: the
    single-step entry reports a non-solved status for every instance."""
    import torch
    S = _setup(robot, cuda, 32)
    B = 32
    pb = manipulator.QPIKParamsBuilder(S["rd"].model, exact=False)
    p = pb.params(LINK[robot], _capi.MODE_QPIK_STEP, *(() if S["moma"] else (np.full(6, 100.0), np.zeros(6))))
    if S["moma"]:
        for i in range(6):
            p.kv[i] = 0.0
    p.solver.max_iter = 1
    a = lambda t: _batch.as_device(t, cuda)
    it = torch.zeros(B, dtype=torch.int32, device=cuda)
    eta, st = _batch.qpik_batch(S["rd"].model, p, a(S["q"]), a(S["v"]), a(S["xt"]), a(S["xdt"]), iters=it)
    _sync()
    st = st.cpu().numpy()
    assert np.all(st != _capi.STATUS_SOLVED), st
    assert not eta.cpu().numpy().any()
    for fused in (1, 0):
        _set_fusion(S, fused)
        try:
            r = _reach(S, p=p)
        finally:
            _set_fusion(S, 1)
        np.testing.assert_array_equal(r["result"], np.full(B, RC.QP_FAILED))
        assert not r["steps_used"].any()
        np.testing.assert_array_equal(r["status_last"], st)
        np.testing.assert_array_equal(r["iters_total"], it.cpu().numpy())
        np.testing.assert_array_equal(r["q_final"], S["q"])
        np.testing.assert_array_equal(r["qdot_final"], S["v"])
        _assert_consistent(r)


# 3 ------------------------------------------------------------------------
@pytest.mark.parametrize("robot", ["fr3", "xls_fr3"])
def test_path_and_batch_size_independence(cuda, robot):
    """B = 2 100: the smallest batch at which a wave of the 2 048-wave grid
    takes a second instance (state carried over between instances would show)."""
    S = _setup(robot, cuda, 2100)
    K = 12
    full = {}
    try:
        for fused in (1, 0):
            _set_fusion(S, fused)
            full[fused] = _reach(S, max_steps=K)
        _assert_same(full[1], full[0])
        for B in (1, 70):
            cut = lambda t: np.ascontiguousarray(t[:, :B])
            for fused in (1, 0):
                _set_fusion(S, fused)
                r = _reach(S, q=cut(S["q"]), v=cut(S["v"]), xt=cut(S["xt"]), xdt=cut(S["xdt"]), max_steps=K)
                for k in FIELDS:
                    np.testing.assert_array_equal(r[k], full[1][k][..., :B], err_msg="%s B=%d fused=%d" % (k, B, fused))
        # in place: q_final / qdot_final are the inputs themselves
        for fused in (1, 0):
            _set_fusion(S, fused)
            a = lambda t: _batch.as_device(np.array(t), cuda)
            q, v, xt, xdt = a(S["q"]), a(S["v"]), a(S["xt"]), a(S["xdt"])
            res = _batch.qpik_reach_batch(S["rd"].model, S["p"], q, v, xt, xdt, K, S["dt"], POS_TOL, ROT_TOL,
                                          q_final=q, qdot_final=v)
            assert res.q_final.data_ptr() == q.data_ptr() and res.qdot_final.data_ptr() == v.data_ptr()
            _assert_same(full[1], _np(res), msg="in place, fused=%d" % fused)
            np.testing.assert_array_equal(xt.cpu().numpy(), S["xt"])  # the other inputs are never written
            np.testing.assert_array_equal(xdt.cpu().numpy(), S["xdt"])
    finally:
        _set_fusion(S, 1)
    r = full[1]
    _assert_consistent(r)
    assert (r["result"] == RC.BUDGET).any() and np.all(r["steps_used"][r["result"] == RC.BUDGET] == K)
    if robot == "fr3":   # (FR3 needs 9 steps and more; the mobile manipulators more than 12)
        assert ((r["result"] == RC.REACHED) & (r["steps_used"] < K)).any()


# 4 ------------------------------------------------------------------------
def _fr3_obstacles(cuda):
    if "obst" not in _CACHE:
        B = 32
        rd = make_manipulator("fr3", cuda)
        rd.set_obstacles(OB.FOUR_TYPES, OB.FOUR_PARAMS, OB.FR3_ARM_LINKS)
        ctrl = manipulator.RobotController(0.001, rd, solver_mode="exact")
        p, dt = _params(ctrl, LINK["fr3"], False)
        S = dict(robot="fr3", rd=rd, ctrl=ctrl, p=p, dt=dt, moma=False, dev=cuda)
        S["poses"] = OB.to_field_major(OB.fr3_scene(11, B))
        S["q"], S["v"], S["xt"], S["xdt"] = _inputs(S, B, S["poses"])
        _CACHE["obst"] = S
    return _CACHE["obst"]


@pytest.mark.parametrize("shared", [False, True])
def test_obstacle_slots(cuda, shared):
    S = _fr3_obstacles(cuda)
    pose = np.ascontiguousarray(S["poses"][:, :, 5]) if shared else S["poses"]
    got = _reach(S, obstacle_pose=pose)
    ref = _loop(S, S["q"], S["v"], S["xt"], S["xdt"], obstacle_pose=pose)
    _assert_same(got, ref)
    _assert_consistent(got)
    assert (got["steps_used"] > 0).any()
    if shared:   # passed shared or replicated per instance: the same bits
        repl = _reach(S, obstacle_pose=np.ascontiguousarray(np.repeat(pose[:, :, None], 32, axis=2)))
        _assert_same(got, repl)
    else:        # (the poses matter: the slot-free model's distance stage differs)
        free = _reach(_setup("fr3", cuda, 70), q=S["q"], v=S["v"], xt=S["xt"], xdt=S["xdt"])
        assert not np.array_equal(free["dist_final"], got["dist_final"])


# 5 ------------------------------------------------------------------------
def test_urdf_with_a_collision_mesh(cuda, tmp_path):
    """FR3 with its box primitive as a 12-triangle STL of the same size (the
    fixture of tests/test_gpu_rollout.py): a hull model, the stepwise dispatch."""
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
    p, dt = _params(ctrl, LINK["fr3"], False)
    S = dict(robot="fr3", rd=rd, ctrl=ctrl, p=p, dt=dt, moma=False, dev=cuda)
    S["q"], S["v"], S["xt"], S["xdt"] = _inputs(S, 8)
    got = _reach(S)
    _assert_same(got, _loop(S, S["q"], S["v"], S["xt"], S["xdt"]))
    _assert_consistent(got)
    assert (got["steps_used"] > 0).any()


# 6 ------------------------------------------------------------------------
def test_error_codes(cuda):
    import torch
    S = _setup("fr3", cuda, 70)
    O = _fr3_obstacles(cuda)
    B = 4
    a = lambda t: _batch.as_device(np.ascontiguousarray(t[:, :B]), cuda)
    q, v, xt, xdt = (a(S[k]) for k in ("q", "v", "xt", "xdt"))
    qf, vf = torch.empty_like(q), torch.empty_like(v)
    res, steps = (torch.empty(B, dtype=torch.int32, device=cuda) for _ in range(2))
    op = _batch.as_device(np.ascontiguousarray(O["poses"][:, :, :B]), cuda)
    stream = C.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    lib = _capi.lib()

    def call(model=S, obstacles=False, mode=_capi.MODE_QPIK_STEP, B=B, max_steps=2, dt=0.005, pos_tol=POS_TOL,
             rot_tol=ROT_TOL, q=q, v=v, xt=xt, xdt=xdt, qf=qf, vf=vf, res=res, steps=steps, op=op, ld=B):
        p = model["ctrl"]._pb.params(LINK["fr3"], mode, np.full(6, 100.0), np.zeros(6))
        head = (model["rd"].model.handle, C.byref(p), C.c_int64(B), C.c_int(max_steps), C.c_double(dt),
                C.c_double(pos_tol), C.c_double(rot_tol), ptr(q), ptr(v), ptr(xt), ptr(xdt))
        tail = (ptr(qf), ptr(vf), ptr(res), ptr(steps), None, None, None, None, stream)
        if obstacles:
            return lib.drc_qpik_reach_obstacles_batch(*head, ptr(op), C.c_int64(ld), *tail)
        return lib.drc_qpik_reach_batch(*head, *tail)

    ok, bad = _capi.DRC_OK, _capi.DRC_ERR_INVALID_ARGUMENT
    assert call() == ok
    assert call(model=O, obstacles=True) == ok
    assert call(model=O, obstacles=True, ld=0) == ok
    assert call(mode=_capi.MODE_QPIK) == bad and call(mode=_capi.MODE_QPIK_CUBIC) == bad
    assert "DRC_MODE_QPIK_STEP" in lib.drc_last_error().decode()
    assert call(max_steps=-1) == bad and call(max_steps=0) == ok
    for x in (0.0, -1e-3, float("nan"), float("inf")):
        assert call(dt=x) == bad, x
        assert call(pos_tol=x) == bad, x
        assert call(rot_tol=x) == bad, x
    for k in ("q", "v", "xt", "xdt", "qf", "vf", "res", "steps"):
        assert call(**{k: None}) == bad, k
    assert call(model=O) == bad   # the plain entry on a model with slots
    assert "drc_qpik_reach_obstacles_batch" in lib.drc_last_error().decode()
    assert call(obstacles=True) == bad   # the obstacle entry on a model without
    assert call(model=O, obstacles=True, op=None) == bad and call(model=O, obstacles=True, ld=B - 1) == bad
    assert call(B=-1) == bad
    assert call(B=0) == ok and call(B=0, q=None, xt=None) == ok
    with pytest.raises(ValueError):
        S["ctrl"].QPIK_reach_batch(S["q"], S["v"], S["xt"], LINK["fr3"], 2, want=("q_traj",))
    _sync()


# 7 ------------------------------------------------------------------------
@pytest.mark.parametrize("robot", ["fr3", "husky_fr3"])
def test_controller_entry(cuda, robot):
    """QPIK_reach_batch of both controllers: xdot_target None is zeros, w_reg
    None the default, and the gains are the controller's."""
    S = _setup(robot, cuda, 70)
    c = S["ctrl"]
    kp, kv = c.Kp_task_.copy(), c.Kv_task_.copy()
    try:
        if not S["moma"]:
            c.setTaskGain(np.full(6, 100.0), np.zeros(6))
        res = c.QPIK_reach_batch(S["q"], S["v"], S["xt"], LINK[robot], MAX_STEPS, dt=S["dt"],
                                 w_reg=None if S["moma"] else 0.01)
    finally:
        c.Kp_task_, c.Kv_task_ = kp, kv
    assert (res.REACHED, res.BUDGET, res.QP_FAILED) == (0, 1, 2)
    assert res.thresholds == RC.thresholds(POS_TOL, ROT_TOL)
    _assert_same(_np(res), _reach(S))


# 8 ------------------------------------------------------------------------
@pytest.mark.parametrize("robot", ["fr3", "husky_fr3"])
def test_is_a_reach_path_of_one_waypoint(cuda, robot):
    """drc_qpik_reach_batch hands its arguments to the reach-path code with
    W = 1: every field the two results share, bit for bit, on both dispatch
    paths."""
    S = _setup(robot, cuda, 70)
    a = lambda t: _batch.as_device(np.array(t), cuda)
    try:
        for fused in (1, 0):
            _set_fusion(S, fused)
            path = _batch.qpik_reach_path_batch(S["rd"].model, S["p"], a(S["q"]), a(S["v"]), a(S["xt"][None]),
                                                a(S["xdt"][None]), MAX_STEPS, S["dt"], POS_TOL, ROT_TOL)
            _assert_same(_reach(S), _np(path), msg="fused=%d" % fused)
    finally:
        _set_fusion(S, 1)
