"""GPU parity of the batched QPID path against the oracle
restatement (oracle/drc_oracle.c: oracle_qpid_one), through the C-ABI.

Reference: Manipulator::QPID (src/manipulator/QP_ID.cpp:7-193) via
RobotController::QPID/QPIDStep/QPIDCubic (robot_controller.cpp:319-361), and
MobileManipulator::QPID (src/mobile_manipulator/QP_ID.cpp:7-184, controller
:199-250).

Tolerances (FP64):
  * stage data: Jdot 1e-10 abs; Jdot v and the manipulability grad_dot term
    1e-7 relative; the distance grad_dot term 1e-5 (1e-3 penetrating), the
    witness-point tolerance of the distance gradient;
  * exact mode: P = 2 J^T J is singular on null(J), so the optimum is a
    face and (qddot, tau) are fixed only up to a null(J) component that the
    certified polish's regularised solve picks (any point of the face is
    KKT-exact; the reference's OSQP returns an ADMM-path-dependent point of it).
    Contract: status identical; the task acceleration J qddot (unique on the
    face) within 1e-9 relative except where the self-collision row's data
    differs between device and oracle (witness points agree to the
    narrow-phase tolerance; UR5e's near-contact workload and parallel axes,
    SURVEY H2): there the device's task acceleration must be the optimum
    (1e-7) of the QP built from its own stage data, with <= 10 % beyond 1e-6
    and all within 1e-2; the
    dynamics rows M qddot + g = tau within 1e-8 relative; qddot/tau themselves
    within 1e-6 relative at the median and 1e-4 on >= 95 % (the null(J)
    spread, measured 1e-9 .. 1e-6 — tools/qpid_parity_stats.py);
  * non-solved instances: qddot = 0, tau = gravity (robot_controller.cpp:
    333-336; MoMa: joint-order gravity at actuator offsets, :211,218).
The oracle's M, g come from the numpy restatement (pyref.dynamics), pinned in
tests/test_oracle_dynamics.py; the device computes its own."""
import numpy as np
import pytest

import oracle as O
from _common import LINK, make_manipulator, make_moma, moma_step_inputs, step_inputs
from dyros_robot_controller_amd import _batch, _capi, manipulator
from dyros_robot_controller_amd import mobile_manipulator as MM

pytestmark = pytest.mark.gpu


def _inputs(robot, cuda, seed, B):
    if robot in ("husky_fr3", "xls_fr3"):
        rd = make_moma(robot, cuda)
        q, qd, xt, xdt = moma_step_inputs(rd, robot, seed, B, cuda)
        ctrl = MM.RobotController(0.001, rd, solver_mode="exact")
    else:
        rd = make_manipulator(robot, cuda)
        q, qd, xt, xdt = step_inputs(rd, robot, seed, B, cuda)
        ctrl = manipulator.RobotController(0.001, rd, solver_mode="exact")
    return rd, ctrl, q, qd, xt, xdt


def _oracle(robot, q, qd, xt, xdt, exact=True, mode=1, xi=None, xdi=None, t=0.0, t0=0.0, T=1.0):
    pm, om, spec = O.load(robot)
    par = O.default_qpid_params(om.kind, exact=exact)
    par.mode, par.t, par.t0, par.duration = mode, t, t0, T
    B = q.shape[1]
    na = om.nv if om.kind == 0 else om.n_arm + om.n_wheel
    qdd, tau, st, diags, dyn = np.zeros((na, B)), np.zeros((na, B)), np.zeros(B, int), [], []
    for b in range(B):
        M, g, gf = O.qpid_dynamics(pm, om, spec, q[:, b], qd[:, b])
        dyn.append((M, g))
        s, a, t_, dg = O.qpid_one(om, par, q[:, b], qd[:, b], M, g, gf, xt[:, b] if xt is not None else None,
                                  xdt[:, b], None if xi is None else xi[:, b], None if xdi is None else xdi[:, b])
        qdd[:, b], tau[:, b], st[b] = a, t_, s
        diags.append(dg)
    return qdd, tau, st, diags, om, spec, dyn


def _task_matrix(om, spec, q, dg):
    import pyref as R
    J = np.array(dg.J[:6 * om.nv]).reshape(6, om.nv)
    if om.kind == 0:
        return J
    Jm = np.array([[om.J_mobile[r][c] for c in range(om.n_wheel)] for r in range(3)])
    S = R.selection_matrix(om.nv, om.n_arm, om.n_wheel, spec["joint_index"], spec["actuator_index"], Jm,
                           q[om.virtual_start + 2])
    return J @ S


@pytest.mark.parametrize("robot", ["fr3", "xls_fr3"])
def test_qpid_stages_match_oracle(cuda, robot):
    rd, ctrl, q, qd, xt, xdt = _inputs(robot, cuda, 31, 96)
    p = ctrl._pbd.params(LINK[robot], _capi.MODE_QPID_STEP, ctrl.Kp_task_, ctrl.Kv_task_)
    a = lambda v: _batch.as_device(v, cuda)
    st = _batch.qpid_stages_batch(rd.model, p, a(q), a(qd), a(xt), a(xdt))
    st = {k: v.cpu().numpy() for k, v in st.items()}
    # pose, J, manipulability and min distance are the QPIK stage's (drc_qpik_stages_batch, which
    # tests/test_gpu_task_fixed_stages.py holds against the oracle): the same device functions on the same state,
    # with contraction fixed per source expression (build.sh), hence the same bits
    ik = _batch.stages_batch(rd.model, p, a(q), a(qd), a(xt), a(xdt))
    for k in ("pose", "jac", "man", "dist", "pair"):
        v = ik[k].cpu().numpy()
        print("%s %s: max |QPID stage - QPIK stage| %.3e" % (robot, k, np.abs(st[k].astype(float) - v).max()))
        np.testing.assert_array_equal(st[k], v, err_msg=k)
    _, _, _, diags, om, spec, _ = _oracle(robot, q, qd, xt, xdt)
    nv = om.nv
    for b, dg in enumerate(diags):
        np.testing.assert_allclose(st["jdot"][:, b].reshape(6, nv), np.array(dg.Jdot[:6 * nv]).reshape(6, nv),
                                   atol=1e-10)
        np.testing.assert_allclose(st["xddot_des"][:, b], np.array(dg.xdot_des), rtol=1e-9, atol=1e-9)
        terms = st["qpid_terms"][:, b]
        np.testing.assert_allclose(terms[:6], np.array(dg.jdot_v), rtol=1e-8, atol=1e-9)
        assert abs(terms[6] - dg.man_gd) <= 1e-7 * max(1.0, abs(dg.man_gd)), (b, terms[6], dg.man_gd)
        if st["pair"][b] == dg.pair:   # witness-point tolerance, as the distance gradient (test_gpu_parity.py)
            tol = 1e-5 if dg.dist > 0 else 1e-3
            assert abs(terms[7] - dg.dist_gd) <= tol * max(1.0, abs(dg.dist_gd)), (b, terms[7], dg.dist_gd)


def _check_parity(om, spec, q, qdd, tau, status, rq, rt, rs, diags, dyn):
    assert np.array_equal(status, rs), [(int(i), int(status[i]), int(rs[i])) for i in np.flatnonzero(status != rs)]
    ok = rs == O.SOLVED
    scale = np.maximum(1.0, np.maximum(np.abs(rq).max(axis=0), np.abs(rt).max(axis=0)))
    rel = np.maximum(np.abs(qdd - rq).max(axis=0), np.abs(tau - rt).max(axis=0)) / scale
    if ok.any():
        assert np.median(rel[ok]) <= 1e-6, np.median(rel[ok])
        assert np.mean(rel[ok] > 1e-4) <= 0.05, np.sort(rel[ok])[-10:]
    tacc = []
    for b in np.nonzero(ok)[0]:
        Jt = _task_matrix(om, spec, q[:, b], diags[b])
        tr = Jt @ rq[:, b]
        tacc.append(np.max(np.abs(Jt @ qdd[:, b] - tr)) / (1 + np.max(np.abs(tr))))
        M, g = dyn[b]
        res = M @ qdd[:, b] + g - tau[:, b]
        assert np.max(np.abs(res)) <= 1e-8 * (1 + np.max(np.abs(tau[:, b]))), (b, res)
    tacc = np.array(tacc)
    if len(tacc):
        assert np.mean(tacc > 1e-6) <= 0.10, np.sort(tacc)[-10:]
        assert np.all(tacc <= 1e-2), np.sort(tacc)[-5:]
    return np.nonzero(ok)[0][tacc > 1e-9] if len(tacc) else np.zeros(0, int)
    # non-solved: qddot = 0 and tau = gravity (compared with the oracle's through rel, exact up to M/g rounding)
    assert np.all(qdd[:, ~ok] == 0)
    assert np.all(rel[~ok] <= 1e-9)


@pytest.mark.parametrize("robot", ["fr3", "ur5e"])
def test_qpid_step_exact_matches_oracle(cuda, robot):
    rd, ctrl, q, qd, xt, xdt = _inputs(robot, cuda, 32, 192)
    qdd, tau, status = ctrl.QPID_step_batch(q, qd, xt, xdt, LINK[robot])
    qdd, tau, status = qdd.cpu().numpy(), tau.cpu().numpy(), status.cpu().numpy()
    rq, rt, rs, diags, om, spec, dyn = _oracle(robot, q, qd, xt, xdt)
    assert np.all(rs == O.SOLVED)   # slacks keep the manipulator QP feasible
    off = _check_parity(om, spec, q, qdd, tau, status, rq, rt, rs, diags, dyn)
    _narrow_phase_explains(rd, ctrl, robot, cuda, q, qd, xt, xdt, off, diags, om)


def _narrow_phase_explains(rd, ctrl, robot, cuda, q, qd, xt, xdt, off, diags, om):
    """Instances whose task acceleration differs beyond 1e-9 relative: the
    self-collision row's data (gradient, grad_dot term) must differ between
    the device and the oracle — witness points agree only to the narrow-phase
    tolerance, and UR5e's parallel joint axes make them non-unique
    — or the min distance is non-smooth there."""
    if len(off) == 0:
        return
    from _common import nonsmooth_min_distance
    p = ctrl._pbd.params(LINK[robot], _capi.MODE_QPID_STEP, ctrl.Kp_task_, ctrl.Kv_task_)
    a = lambda v: _batch.as_device(v, cuda)
    st = _batch.qpid_stages_batch(rd.model, p, a(q[:, off]), a(qd[:, off]), a(xt[:, off]), a(xdt[:, off]))
    st = {k: v.cpu().numpy() for k, v in st.items()}
    import pyref as R
    pm, _, spec = O.load(robot)
    arm = np.arange(om.nv)
    for i, b in enumerate(off):
        dg = diags[b]
        gd = np.max(np.abs(st["dist"][1:, i] - np.array(dg.dist_grad[:om.nv])))
        gdd = abs(st["qpid_terms"][7, i] - dg.dist_gd)
        assert gd > 1e-12 or gdd > 1e-12 or nonsmooth_min_distance(om, q[:, b]), (b, gd, gdd)
        # the device's answer is the optimum of the QP built from its own stage data
        J = st["jac"][:, i].reshape(6, om.nv)
        M, g, _ = O.qpid_dynamics(pm, om, spec, q[:, b], qd[:, b])
        man = (st["man"][0, i], st["man"][1:, i], st["qpid_terms"][6, i])
        dist = (st["dist"][0, i], st["dist"][1:, i], st["qpid_terms"][7, i])
        P, qv, A, l, u = R.build_qp_qpid(pm, q[:, b], qd[:, b], J, st["xddot_des"][:, i], st["qpid_terms"][:6, i],
                                         M, g, man, dist, arm, 0, slacks=True)
        x, y, s2 = R.solve_qp_exact(P, qv, A, l, u)
        if s2 == 1 and max(R.kkt_residuals(P, qv, A, l, u, x, y)) < 1e-6:
            qdd_dev = ctrl.QPID_step_batch(q[:, b:b + 1], qd[:, b:b + 1], xt[:, b:b + 1], xdt[:, b:b + 1],
                                           LINK[robot])[0].cpu().numpy()[:, 0]
            tr = J @ x[:om.nv]
            assert np.max(np.abs(J @ qdd_dev - tr)) <= 1e-7 * (1 + np.max(np.abs(tr))), b
    print("%s: %d/%d instances with task acceleration beyond 1e-9 (narrow-phase data differs)" % (
        robot, len(off), q.shape[1]))


@pytest.mark.parametrize("robot", ["husky_fr3", "xls_fr3"])
def test_moma_qpid_step_exact_matches_oracle(cuda, robot):
    rd, ctrl, q, qd, xt, xdt = _inputs(robot, cuda, 33, 192)
    qdd, tau, status = ctrl.QPID_step_batch(q, qd, xt, xdt, LINK[robot])
    qdd, tau, status = qdd.cpu().numpy(), tau.cpu().numpy(), status.cpu().numpy()
    rq, rt, rs, diags, om, spec, dyn = _oracle(robot, q, qd, xt, xdt)
    _check_parity(om, spec, q, qdd, tau, status, rq, rt, rs, diags, dyn)
    # no slacks: some instances are infeasible; their torque is the joint-order gravity at actuator offsets
    bad = rs != O.SOLVED
    pm = O.load(robot)[0]
    for b in np.nonzero(bad)[0][:8]:
        gf = O.qpid_dynamics(pm, om, spec, q[:, b], qd[:, b])[2]
        np.testing.assert_allclose(tau[:, b], gf[:qdd.shape[0]], atol=1e-9)


def test_qpid_modes_and_single_instance(cuda):
    """QPID(xddot_target) and QPIDCubic batches, and the reference-signature
    single-instance QPIDStep (returns tau)."""
    robot = "fr3"
    rd, ctrl, q, qd, xt, xdt = _inputs(robot, cuda, 34, 64)
    rng = np.random.default_rng(5)
    xdd = rng.normal(0, 0.5, (6, 64))
    qdd, tau, status = [v.cpu().numpy() for v in ctrl.QPID_batch(q, qd, xdd, LINK[robot])]
    rq, rt, rs, diags, om, spec, dyn = _oracle(robot, q, qd, None, xdd, mode=0)
    _check_parity(om, spec, q, qdd, tau, status, rq, rt, rs, diags, dyn)
    xi, xdi = xt.copy(), np.zeros((6, 64))
    xi[9:] -= 0.05
    qdd, tau, status = [v.cpu().numpy() for v in ctrl.QPID_cubic_batch(q, qd, xt, xdt, xi, xdi, 0.4, 0.0, 1.0,
                                                                       LINK[robot])]
    rq, rt, rs, diags, om, spec, dyn = _oracle(robot, q, qd, xt, xdt, mode=2, xi=xi, xdi=xdi, t=0.4, t0=0.0, T=1.0)
    _check_parity(om, spec, q, qdd, tau, status, rq, rt, rs, diags, dyn)
    rd.updateState(q[:, 0], qd[:, 0])
    T = manipulator.pose_from12(xt[:, 0])
    t1 = ctrl.QPIDStep(T, xdt[:, 0], LINK[robot])
    rq, rt, rs, _, _, _, _ = _oracle(robot, q[:, :1], qd[:, :1], xt[:, :1], xdt[:, :1])
    np.testing.assert_allclose(t1, rt[:, 0], rtol=1e-5, atol=1e-6)


def test_qpid_reference_settings_match_oracle(cuda):
    """osqp_default mode (the reference's OSQP settings): the same ADMM path
    on both sides, so the early-stopped point agrees too."""
    robot = "fr3"
    rd = make_manipulator(robot, cuda)
    ctrl = manipulator.RobotController(0.001, rd, solver_mode="osqp_default")
    q, qd, xt, xdt = step_inputs(rd, robot, 35, 96, cuda)
    qdd, tau, status = [v.cpu().numpy() for v in ctrl.QPID_step_batch(q, qd, xt, xdt, LINK[robot])]
    rq, rt, rs, diags, om, spec, dyn = _oracle(robot, q, qd, xt, xdt, exact=False)
    assert np.mean(status == rs) >= 0.95
    both = (status == rs) & (rs == O.SOLVED)
    err = np.abs(tau - rt).max(axis=0)[both]
    assert np.median(err) <= 1e-6, np.median(err)


@pytest.mark.parametrize("robot", ["fr3", "husky_fr3"])
def test_graddot_vectors_and_jdot_getters(cuda, robot):
    """getManipulability(true, true).grad_dot, getMinDistance(true, true).grad_dot
    and getJacobianTimeVariation through the Python mirrors (QPID stage
    outputs) vs the oracle's literal restatement of robot_data.cpp:496-512,
    555-569 (MoMa :477-492)."""
    rd, ctrl, q, qd, xt, xdt = _inputs(robot, cuda, 36, 6)
    pm, om, spec = O.load(robot)
    for b in range(q.shape[1]):
        Jd, mgd, dgd = O.qpid_stages(om, q[:, b], qd[:, b])
        if om.kind == 0:
            rd.updateState(q[:, b], qd[:, b])
            man = rd.getManipulability(True, True, LINK[robot])
            dist = rd.getMinDistance(True, True, False)
            np.testing.assert_allclose(rd.getJacobianTimeVariation(LINK[robot]), Jd, atol=1e-10)
        else:
            rd.q_, rd.qdot_ = q[:, b].copy(), qd[:, b].copy()
            man = rd.get_manipulability(True, True, LINK[robot])
            dist = rd.get_min_distance(True, True)
            np.testing.assert_allclose(rd.get_jacobian_time_variation(LINK[robot]), Jd, atol=1e-10)
        np.testing.assert_allclose(man.grad_dot, mgd, rtol=1e-7, atol=1e-8)
        d = O.min_distance(om, q[:, b])[0]
        np.testing.assert_allclose(dist.grad_dot, dgd, atol=1e-5 if d > 0 else 1e-3)
