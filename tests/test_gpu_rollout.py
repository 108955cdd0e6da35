"""Closed-loop rollouts on the device (drc_qpik_rollout_batch,
QPIK_rollout_batch): `steps` cycles of QPIK* with q += dt * qdot_desired
between them (examples/C++/src/fr3_controller.cpp:123-134), against the
single-step entry applied step by step.

The contract is bitwise: one step equals drc_qpik_batch and numpy's
q + dt * eta (test 1), a K-step call equals K one-step calls fed with the
previous finals (test 2) -- which pins the whole loop by induction -- and the
persistent kernel (rollout_kernel.hip), the stepwise path (drc_set_fusion 0)
and every batch size return the same bits (test 3).  Stress-tier inputs,
dt = 0.001, every instance compared.

The virtual joints of a mobile manipulator follow v = Rz(yaw) J_mobile eta, a
sum of n_wheel products formed with the device's sin / cos.  Against numpy
(oracle/pyref.selection_matrix, libm sin / cos) q_final's virtual rows are
held to 64 eps (|q| + dt sum |S| |eta|): the rounding of the short sum.
qdot_final's are held to 64 eps sum_w (|cos| |J_0w| + |sin| |J_1w|) |eta_w|
(row yaw: |J_2w| |eta_w|): each entry of S is itself a difference of two
rounded products, whose rounding does not shrink when they cancel, so the
bound uses the products' magnitudes (with at most 8 wheels, a few eps each for
sin / cos, the two products, the difference and the fused sum: 64 eps covers
it with room).  q_final is also bit-equal to numpy's q0 + dt * qdot_final."""
import ctypes as C

import numpy as np
import pytest

import oracle as O
import pyref as R
from _common import LINK, make_manipulator, make_moma, moma_step_inputs, oracle_batch, stage_step, step_inputs
from _mesh_io import box_triangles, write_stl_ascii
from dyros_robot_controller_amd import _batch, _capi, manipulator, mobile_manipulator, robot_path

pytestmark = pytest.mark.gpu

MOMA = ("husky_fr3", "xls_fr3", "caster_fr3")
ROBOTS = ("fr3", "ur5e", "husky_fr3", "xls_fr3", "caster_fr3")
DT = 0.001
ALL = _batch.ROLLOUT_FIELDS
FIELDS = ("q_final", "qdot_final", "status_traj") + ALL
EPS = np.finfo(np.float64).eps
_CACHE = {}


def _setup(robot, cuda, B=70, seed=31):
    """Model, controller and one stress-tier batch (shared by the tests, never modified)."""
    key = (robot, B, seed)
    if key not in _CACHE:
        moma = robot in MOMA
        rd = make_moma(robot, cuda) if moma else make_manipulator(robot, cuda)
        ctrl = (mobile_manipulator if moma else manipulator).RobotController(DT, rd, solver_mode="exact")
        q, qd, xt, xdt = (moma_step_inputs if moma else step_inputs)(rd, robot, seed, B, cuda, stress=True)
        xi = xt.copy()
        xi[9:] -= 0.01
        _CACHE[key] = dict(rd=rd, ctrl=ctrl, q=q, qd=qd, xt=xt, xdt=xdt, xi=xi, xdi=np.zeros_like(xdt))
    return _CACHE[key]


def _np(res):
    import torch
    torch.cuda.synchronize()
    return {k: (None if getattr(res, k) is None else getattr(res, k).cpu().numpy()) for k in FIELDS}


def _roll(S, mode, steps, q=None, qd=None, xt=None, xdt=None, t=0.4, want=ALL, per_step=False, link=None):
    """One QPIK_rollout_batch call (cubic: from x_init over [0, 1] s at time t)."""
    link = link or LINK[S.get("robot", "fr3")]
    q, qd = (S["q"] if q is None else q), (S["qd"] if qd is None else qd)
    xt, xdt = (S["xt"] if xt is None else xt), (S["xdt"] if xdt is None else xdt)
    cubic = mode == "cubic"
    return _np(S["ctrl"].QPIK_rollout_batch(q, qd, xt, xdt, link, steps, mode=mode,
                                            x_init=S["xi"] if cubic else None, xdot_init=S["xdi"] if cubic else None,
                                            current_time=t if cubic else 0, init_time=0, duration=1,
                                            targets_per_step=per_step, want=want))


def _single(S, mode, q, qd, xt, xdt, link, t=0.4):
    """The existing single-step entry: (eta, status, iters)."""
    import torch
    c = S["ctrl"]
    it = torch.zeros(q.shape[1], dtype=torch.int32, device=torch.device("cuda", 0))
    if mode == "cubic":
        p = c._pb.params(link, _capi.MODE_QPIK_CUBIC, c.Kp_task_, _kv(c), t, 0, 1)
    else:
        p = c._pb.params(link, _capi.MODE_QPIK if mode == "qpik" else _capi.MODE_QPIK_STEP, c.Kp_task_, _kv(c))
    dev = c.robot_data_.device
    a = lambda v: _batch.as_device(v, dev)
    cubic = mode == "cubic"
    out, st = _batch.qpik_batch(c.robot_data_.model, p, a(q), a(qd), None if mode == "qpik" else a(xt), a(xdt),
                                a(S["xi"]) if cubic else None, a(S["xdi"]) if cubic else None, iters=it)
    torch.cuda.synchronize()
    return out.cpu().numpy(), st.cpu().numpy(), it.cpu().numpy()


def _kv(ctrl):
    return np.zeros(6) if isinstance(ctrl, mobile_manipulator.RobotController) else ctrl.Kv_task_


def _assert_same(a, b, fields=FIELDS):
    for k in fields:
        assert (a[k] is None) == (b[k] is None), k
        if a[k] is not None:
            np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def _set_fusion(S, on):
    _capi.check(_capi.lib().drc_set_fusion(S["rd"].model.handle, C.c_int(on)))


def _chain(S, mode, steps, link, t=0.4):
    """`steps` one-step rollouts, each fed with the previous finals (cubic: at t + k dt)."""
    q, qd = S["q"], S["qd"]
    parts = []
    for k in range(steps):
        r = _roll(S, mode, 1, q=q, qd=qd, t=t + k * DT, link=link)
        parts.append(r)
        q, qd = r["q_final"], r["qdot_final"]
    out = {k: np.concatenate([p[k] for p in parts]) for k in ("status_traj",) + ALL}
    out["q_final"], out["qdot_final"] = q, qd
    return out


# 1 ------------------------------------------------------------------------
@pytest.mark.parametrize("robot", ROBOTS)
def test_one_step_is_the_existing_entry(cuda, robot):
    S = _setup(robot, cuda)
    link = LINK[robot]
    r = _roll(S, "step", 1, link=link)
    eta, st, it = _single(S, "step", S["q"], S["qd"], S["xt"], S["xdt"], link)
    np.testing.assert_array_equal(r["status_traj"][0], st)
    np.testing.assert_array_equal(r["qdot_traj"][0], eta)
    np.testing.assert_array_equal(r["iters_traj"][0], it)
    assert (st == 1).sum() >= 1, st  # not a comparison of zeros
    assert np.abs(eta[:, st == 1]).max() > 0
    assert np.all(eta[:, st != 1] == 0.0)
    q0 = S["q"]
    np.testing.assert_array_equal(r["q_traj"][0], r["q_final"])
    if robot not in MOMA:
        np.testing.assert_array_equal(r["qdot_final"], eta)
        np.testing.assert_array_equal(r["q_final"], q0 + DT * eta)
        return
    spec = O.ROBOTS[robot]
    vs, ms, ws = spec["joint_index"]
    am, aw = spec["actuator_index"]
    na, nw, nv = spec["n_arm"], spec["n_wheel"], q0.shape[0]
    v, qf = r["qdot_final"], r["q_final"]
    np.testing.assert_array_equal(v[ms:ms + na], eta[am:am + na])
    np.testing.assert_array_equal(v[ws:ws + nw], eta[aw:aw + nw])
    np.testing.assert_array_equal(qf, q0 + DT * v)  # every row, the virtual ones included
    worst_q = worst_v = 0.0
    for b in range(q0.shape[1]):
        Jm = spec["J_mobile"](q0[ws:ws + nw, b]) if spec.get("drive") == 2 else spec["J_mobile"]()
        yaw = q0[vs + 2, b]
        Sm = R.selection_matrix(nv, na, nw, spec["joint_index"], spec["actuator_index"], Jm, yaw)
        absS = np.abs(Sm) @ np.abs(eta[:, b])
        qref = q0[:, b] + DT * (Sm @ eta[:, b])
        bound_q = 64 * EPS * (np.abs(q0[:, b]) + DT * absS)
        c, s = abs(np.cos(yaw)), abs(np.sin(yaw))
        aJ, ae = np.abs(np.asarray(Jm, float)[:, :nw]), np.abs(eta[aw:aw + nw, b])
        bound_v = 64 * EPS * np.array([(c * aJ[0] + s * aJ[1]) @ ae, (s * aJ[0] + c * aJ[1]) @ ae, aJ[2] @ ae])
        for i in range(3):
            dq, dv = abs(qf[vs + i, b] - qref[vs + i]), abs(v[vs + i, b] - (Sm @ eta[:, b])[vs + i])
            worst_q, worst_v = max(worst_q, dq / max(bound_q[vs + i], 1e-300)), max(worst_v, dv / max(bound_v[i], 1e-300))
            assert dq <= bound_q[vs + i], (b, i, dq, bound_q[vs + i])
            assert dv <= bound_v[i], (b, i, dv, bound_v[i])
    print("%s: virtual rows at %.3f (q) / %.3f (v) of their bounds" % (robot, worst_q, worst_v))


# 2 ------------------------------------------------------------------------
CHAIN = [(r, m) for r in ("fr3", "husky_fr3") for m in ("step", "qpik", "cubic")] + \
        [(r, "step") for r in ("ur5e", "xls_fr3", "caster_fr3")]


@pytest.mark.parametrize("robot,mode", CHAIN)
def test_chaining(cuda, robot, mode):
    S = _setup(robot, cuda)
    whole = _roll(S, mode, 9, link=LINK[robot])
    _assert_same(whole, _chain(S, mode, 9, LINK[robot]))
    assert (whole["status_traj"] == 1).any()
    assert np.abs(whole["q_final"] - S["q"]).max() > 0


# 3 ------------------------------------------------------------------------
@pytest.mark.parametrize("robot", ["fr3", "xls_fr3"])
def test_path_and_batch_size_independence(cuda, robot):
    """B = 2 100: the smallest batch at which a wave of the 2 048-wave grid
    takes a second instance (state carried over between instances would show)."""
    S = _setup(robot, cuda, B=2100, seed=32)
    full = {}
    try:
        for fused in (1, 0):
            _set_fusion(S, fused)
            full[fused] = _roll(S, "step", 3, link=LINK[robot])
        _assert_same(full[1], full[0])
        for B in (1, 70):
            cut = lambda a: np.ascontiguousarray(a[:, :B])
            for fused in (1, 0):
                _set_fusion(S, fused)
                r = _roll(S, "step", 3, q=cut(S["q"]), qd=cut(S["qd"]), xt=cut(S["xt"]), xdt=cut(S["xdt"]),
                          link=LINK[robot])
                for k in FIELDS:
                    np.testing.assert_array_equal(r[k], full[1][k][..., :B], err_msg="%s B=%d fused=%d" % (k, B, fused))
    finally:
        _set_fusion(S, 1)
    assert (full[1]["status_traj"] == 1).any()


# 4 ------------------------------------------------------------------------
def test_per_step_targets_and_stage_outputs(cuda):
    import torch
    S = _setup("fr3", cuda)
    link, K = LINK["fr3"], 4
    xt = np.stack([S["xt"] + np.r_[np.zeros(9), 1e-3 * k * np.ones(3)][:, None] for k in range(K)])
    xdt = np.stack([S["xdt"] * (1 + 0.1 * k) for k in range(K)])
    r = _roll(S, "step", K, xt=xt, xdt=xdt, per_step=True, link=link)
    assert np.abs(r["qdot_traj"][1] - r["qdot_traj"][0]).max() > 0
    c = S["ctrl"]
    p = c._pb.params(link, _capi.MODE_QPIK_STEP, c.Kp_task_, c.Kv_task_)
    a = lambda v: _batch.as_device(v, cuda)
    for k in range(K):
        qk = S["q"] if k == 0 else r["q_traj"][k - 1]
        vk = S["qd"] if k == 0 else r["qdot_traj"][k - 1]
        eta, st, it = _single(S, "step", qk, vk, xt[k], xdt[k], link)
        np.testing.assert_array_equal(r["status_traj"][k], st)
        np.testing.assert_array_equal(r["qdot_traj"][k], eta)
        np.testing.assert_array_equal(r["iters_traj"][k], it)
        np.testing.assert_array_equal(r["q_traj"][k], qk + DT * eta)
        sg = _batch.stages_batch(c.robot_data_.model, p, a(qk), a(vk), a(xt[k]), a(xdt[k]))
        torch.cuda.synchronize()
        pose, dist = sg["pose"].cpu().numpy(), sg["dist"].cpu().numpy()
        # tests/test_gpu_golden.py: kinematic stage data 1e-9 relative, the distance 1e-9 separated / 1e-6
        # penetrating; its gradient 1e-6 (tests/_common.py narrow_phase_close)
        assert np.abs(r["pose_traj"][k] - pose).max() <= 1e-9 * max(1.0, np.abs(pose).max())
        dd = np.abs(r["dist_traj"][k][0] - dist[0])
        assert np.all(dd <= np.where(dist[0] > 0, 1e-9, 1e-6)), (k, dd.max())
        assert np.abs(r["dist_traj"][k][1:] - dist[1:]).max() <= 1e-6


# 5 ------------------------------------------------------------------------
@pytest.mark.parametrize("robot", ["fr3", "husky_fr3", "caster_fr3"])
def test_aliasing_and_optional_outputs(cuda, robot):
    import torch
    S = _setup(robot, cuda)
    c, link = S["ctrl"], LINK[robot]
    ref = _roll(S, "step", 3, link=link)
    none = _roll(S, "step", 3, link=link, want=())
    assert all(none[k] is None for k in ALL)
    _assert_same(ref, none, ("q_final", "qdot_final", "status_traj"))
    p = c._pb.params(link, _capi.MODE_QPIK_STEP, c.Kp_task_, _kv(c))
    a = lambda v: _batch.as_device(np.array(v), cuda)
    q, qd, xt, xdt = a(S["q"]), a(S["qd"]), a(S["xt"]), a(S["xdt"])
    res = _batch.qpik_rollout_batch(c.robot_data_.model, p, q, qd, 3, DT, xt, xdt, want=ALL, q_final=q, qdot_final=qd)
    assert res.q_final.data_ptr() == q.data_ptr() and res.qdot_final.data_ptr() == qd.data_ptr()
    _assert_same(ref, _np(res))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(xt.cpu().numpy(), S["xt"])  # the other inputs are never written
    np.testing.assert_array_equal(xdt.cpu().numpy(), S["xdt"])


# 6 ------------------------------------------------------------------------
def _hull_fr3(cuda, tmp_path):
    """FR3 with its box primitive as a 12-triangle STL of the same size (the
    fixture of tests/test_gpu_mesh_model.py)."""
    import re
    text = open(robot_path("fr3")).read()
    m = re.search(r'<box size="([^"]+)"/>', text)
    size = np.array([float(x) for x in m.group(1).split()])
    (tmp_path / "pkg" / "meshes").mkdir(parents=True)
    write_stl_ascii(tmp_path / "pkg" / "meshes" / "box.stl", box_triangles(0.5 * size).reshape(-1, 3))
    (tmp_path / "pkg" / "urdf").mkdir()
    urdf = tmp_path / "pkg" / "urdf" / "fr3_mesh.urdf"
    urdf.write_text(text[:m.start()] + '<mesh filename="package://pkg/meshes/box.stl"/>' + text[m.end():])
    return manipulator.RobotData(str(urdf), robot_path("fr3", "srdf"), str(tmp_path), device=cuda)


def test_urdf_with_a_collision_mesh(cuda, tmp_path):
    """The hull FR3: the MESH build of the kernel."""
    rd = _hull_fr3(cuda, tmp_path)
    S = dict(_setup("fr3", cuda), rd=rd, ctrl=manipulator.RobotController(DT, rd, solver_mode="exact"))
    whole = _roll(S, "step", 2, link=LINK["fr3"])
    _assert_same(whole, _chain(S, "step", 2, LINK["fr3"]))
    assert (whole["status_traj"] == 1).any()


def test_hull_decides_the_distance(cuda, tmp_path):
    """The hull FR3 at three states whose closest pair is one of the hull's:
    the persistent kernel against the stepwise path (the task kernel's and the
    fused kernel's hull builds, which tests/test_gpu_mesh_model.py holds
    against the primitive twin), bit for bit, and step 0 against the oracle on
    the primitive twin within the end-to-end bound of tests/test_gpu_parity.py.
    A persistent kernel without the hull narrow phase forms another distance
    row at these states."""
    rd = _hull_fr3(cuda, tmp_path)
    _, om, _ = O.load("fr3")
    box = [g for g in range(om.ngeom) if om.gtype[g] == 2]
    box_pairs = [p for p in range(om.npairs) if box[0] in (om.pair_a[p], om.pair_b[p])]
    q, qd, xt, xdt = step_inputs(rd, "fr3", 42, 2048, cuda)
    pick = np.flatnonzero(np.isin(stage_step(rd.model, cuda, q, qd, xt, xdt, LINK["fr3"])["pair"], box_pairs))[:3]
    assert len(pick) == 3
    q, qd, xt, xdt = (np.ascontiguousarray(v[:, pick]) for v in (q, qd, xt, xdt))
    S = dict(rd=rd, ctrl=manipulator.RobotController(DT, rd, solver_mode="exact"), q=q, qd=qd, xt=xt, xdt=xdt)
    got = {}
    try:
        for fused in (1, 0):
            _set_fusion(S, fused)
            got[fused] = _roll(S, "step", 2, link=LINK["fr3"])
    finally:
        _set_fusion(S, 1)
    _assert_same(got[1], got[0])
    st = stage_step(rd.model, cuda, q, qd, xt, xdt, LINK["fr3"])
    assert np.isin(st["pair"], box_pairs).all()   # a hull pair is the closest at step 0 ...
    np.testing.assert_array_equal(got[1]["dist_traj"][0], st["dist"])   # ... and that is the row the kernel formed
    ref, rstat, _, _ = oracle_batch("fr3", q, qd, xt, xdt, exact=True)
    np.testing.assert_array_equal(got[1]["status_traj"][0], rstat)
    err = np.abs(got[1]["qdot_traj"][0] - ref).max(axis=0)
    print("hull pairs %s, d %s; step 0 against the oracle: max %.3e" % (st["pair"].tolist(), st["dist"][0].tolist(),
                                                                         err.max()))
    assert (rstat == 1).any() and err.max() <= 1e-4, err


# 7 ------------------------------------------------------------------------
def test_argument_errors(cuda):
    import torch
    S = _setup("fr3", cuda)
    c, link = S["ctrl"], LINK["fr3"]
    B = 4
    a = lambda v: _batch.as_device(np.ascontiguousarray(v[:, :B]), cuda)
    q, qd, xt, xdt, xi, xdi = (a(S[k]) for k in ("q", "qd", "xt", "xdt", "xi", "xdi"))
    qf, vf = torch.empty_like(q), torch.empty_like(qd)
    st = torch.empty((2, B), dtype=torch.int32, device=cuda)
    stream = C.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())

    def call(mode=_capi.MODE_QPIK_STEP, B=B, steps=2, dt=DT, per_step=0, qf=qf, vf=vf, st=st, q=q):
        p = c._pb.params(link, mode, c.Kp_task_, c.Kv_task_, 0.4, 0, 1)
        return _capi.lib().drc_qpik_rollout_batch(
            c.robot_data_.model.handle, C.byref(p), C.c_int64(B), C.c_int(steps), C.c_double(dt), ptr(q), ptr(qd),
            ptr(xt), ptr(xdt), ptr(xi), ptr(xdi), C.c_int(per_step), ptr(qf), ptr(vf), None, ptr(st), None, None,
            None, None, stream)

    bad = _capi.DRC_ERR_INVALID_ARGUMENT
    assert call() == _capi.DRC_OK
    assert call(mode=_capi.MODE_QPIK_CUBIC) == _capi.DRC_OK
    assert call(steps=0) == bad and call(steps=-3) == bad
    for dt in (0.0, -DT, float("nan"), float("inf")):
        assert call(dt=dt) == bad, dt
    assert call(qf=None) == bad and call(vf=None) == bad and call(st=None) == bad and call(q=None) == bad
    assert call(mode=_capi.MODE_QPIK_CUBIC, per_step=1) == bad
    assert "QPIKCubic" in _capi.lib().drc_last_error().decode()
    assert call(B=-1) == bad
    assert call(B=0) == _capi.DRC_OK
    with pytest.raises(ValueError):
        c.QPIK_rollout_batch(S["q"], S["qd"], S["xt"], S["xdt"], link, 2, mode="spline")
    torch.cuda.synchronize()
