"""The pseudo-inverse rank decisions of the device at kinematic singularities.

Four device sites pair a certified fast inverse with a PinvCOD fallback
(tests/_singular.py names them).  Every input here carries a class decided on
the CPU from the reference decomposition alone: K (certified path), F
(fallback, every mode kept), T (fallback, modes dropped), each a factor >= 3
from the decision, so the kernel and the oracle cannot decide differently and
no instance is exempt from the tolerance.  Every test first asserts, from the
classifier, that each class it claims has >= 16 instances and that no input is
ambiguous.  Inputs: UR5e with the wrist (q[4]) or elbow (q[2]) joint at eps
from an exact singularity, the workload's stress tiers, and, for FR3 and the
Husky-FR3 arm, states descended to a singularity inside the joint limits.

The figures in the docstrings below were measured on an MI355X with the seeds
of this file; every test prints its own."""
import ctypes as C

import mpmath as mp
import numpy as np
import pytest

import oracle as O
import pyref as R
import _singular as SG
from _common import LINK, assert_qpik_parity, make_manipulator, make_moma, stage_pose
from dyros_robot_controller_amd import _capi, manipulator, workload

pytestmark = pytest.mark.gpu

PER = 20          # instances per class and test
_CACHE = {}


def _pool(robot):
    if ("pool", robot) not in _CACHE:
        _CACHE["pool", robot] = SG.pool(robot)
    return _CACHE["pool", robot]


def _classes(robot, site):
    """Class of every pool state at one site ("" where it was not computed:
    OSF needs the dynamics of each state, so only part of the pool is classified)."""
    if (site, robot) not in _CACHE:
        pm, om, _ = O.load(robot)
        q, qd = _pool(robot)
        N = q.shape[1]
        if site == "manip":
            cls = SG.classify_batch(lambda x: SG.classify_manip(robot, om, x), q)
        elif site == "clik":
            cls = SG.classify_batch(lambda x: SG.classify_clik(om, x), q)
        else:
            cls = np.array([""] * N, dtype=object)
            sub = np.r_[0:600] if robot == "ur5e" else np.r_[0:400, N - 48:N]
            for b in sub:
                cls[b] = SG.classify_osf(om, q[:, b], R.dynamics(pm, q[:, b], qd[:, b])["Minv"])
        _CACHE[site, robot] = cls
    return _CACHE[site, robot]


def _pick(robot, site, want):
    """States of the classes in `want`, PER each, interleaved; asserts the
    coverage the test claims."""
    cls = _classes(robot, site)
    idx = SG.select(cls, want, PER)
    q, qd = _pool(robot)
    got = SG.counts(cls[idx])
    assert all(got[c] >= 16 for c in want) and got[SG.AMBIGUOUS] == 0 and sum(got.values()) == len(idx), got
    return q[:, idx].copy(), qd[:, idx].copy(), cls[idx]


def _targets(model, cuda, q, qd, link, seed):
    st = stage_pose(model, cuda, q, qd, link)
    return workload.perturb_targets(st["pose"], seed, q.shape[1])


def _rel(a, b):
    return np.abs(a - b).max(axis=0) / np.maximum(1.0, np.abs(b).max(axis=0))


def _det_mp(Jr):
    """det(Jr Jr^T) at 50 digits, of the double-precision Jr as given."""
    with mp.workdps(50):
        A = mp.matrix(Jr.tolist())
        return mp.det(A * A.T)


@pytest.mark.parametrize("robot", ["ur5e", "fr3", "husky_fr3"])
def test_manipulability_by_class(cuda, robot):
    """Manipulability stage (stage_pose) against the C oracle, 20 instances of
    each of K, F, T (Husky-FR3: the arm block).  K and F: m to 1e-10 relative
    to max(1, m), grad m to 1e-8, every instance.  T: m is noise (delta m ~
    sqrt(delta det)), so m^2 is compared with det(J J^T) at 50 digits, within
    10x the larger of the C oracle's and numpy's worst error against it on the
    same inputs; m finite and >= 0; grad m finite and within 1e-8 of the
    oracle's.

    Measured, 20 / 20 / 20 instances, none ambiguous (m, grad m against the
    C oracle; |m^2 - det| against mpmath: device / C oracle / numpy):
      ur5e       K 2.1e-16, 1.8e-14   F 3.6e-15, 1.0e-12   T grad 1.3e-09
                 T |m^2 - det| 6.5e-18 / 4.9e-18 / 5.5e-18  (bound 5.5e-17)
      fr3        K 1.8e-15, 4.8e-15   F 7.8e-15, 4.6e-13   T grad 5.2e-10
                 T |m^2 - det| 5.5e-17 / 2.5e-17 / 7.1e-18  (bound 2.5e-16)
      husky_fr3  K 3.5e-16, 2.8e-15   F 5.6e-15, 1.9e-13   T grad 4.9e-11
                 T |m^2 - det| 2.4e-17 / 2.7e-17 / 5.0e-17  (bound 5.0e-16)
    In class T the oracle and pyref differ by up to 2.5e-9 in m and in grad m
    (UR5e), which is why m itself is not compared there."""
    moma = O.ROBOTS[robot]["kind"] == 1
    rd = make_moma(robot, cuda) if moma else make_manipulator(robot, cuda)
    q, qd, cls = _pick(robot, "manip", (SG.K, SG.F, SG.T))
    pm, om, _ = O.load(robot)
    st = stage_pose(rd.model, cuda, q, qd, LINK[robot])
    B = q.shape[1]
    ref = [O.manipulability(om, q[:, b]) for b in range(B)]
    m_ref, g_ref = np.array([r[0] for r in ref]), np.stack([r[1] for r in ref], axis=1)
    m, g = st["man"][0], st["man"][1:]
    assert np.all(np.isfinite(m_ref)) and np.all(np.isfinite(g_ref))
    assert np.all(np.isfinite(m)) and np.all(m >= 0) and np.all(np.isfinite(g))
    em = np.abs(m - m_ref) / np.maximum(1.0, m_ref)
    eg = np.abs(g - g_ref).max(axis=0)
    for c in (SG.K, SG.F, SG.T):
        print("%s %s: %d instances, m %.2e, grad %.2e" % (robot, c, np.sum(cls == c), em[cls == c].max(), eg[cls == c].max()))
    t = cls == SG.T
    cols = SG.arm_cols(robot)
    e_or, e_np, e_dev = [], [], []
    for b in np.nonzero(t)[0]:
        J = SG.jacobian(om, q[:, b])
        Jr = J if cols is None else J[:, cols]
        det = _det_mp(Jr)
        e_or.append(float(abs(mp.mpf(m_ref[b]) ** 2 - det)))
        e_np.append(float(abs(mp.mpf(np.linalg.det(Jr @ Jr.T)) - det)))
        e_dev.append(float(abs(mp.mpf(m[b]) ** 2 - det)))
    tol = 10 * max(max(e_or), max(e_np))
    print("%s T: |m^2 - det| device %.2e, oracle %.2e, numpy %.2e" % (robot, max(e_dev), max(e_or), max(e_np)))
    assert np.all(em[~t] <= 1e-10), em[~t].max()
    assert np.all(eg <= 1e-8), eg.max()
    assert max(e_dev) <= tol, (max(e_dev), tol)


def _clik_cases(nu):
    # (cubic, null-space term)
    return [(False, None), (False, nu), (True, None), (True, nu)]


@pytest.mark.parametrize("robot", ["ur5e", "fr3"])
def test_clik_by_class(cuda, robot):
    """CLIKStep and CLIKCubic, with and without the null-space velocity,
    against oracle_clik_one on 20 instances of each of K, F, T: 1e-8 relative
    to max(1, |out|_inf) on every instance.  T runs the rank < 6 branch of
    pinv_cod_rect (UR5e: 6 x 6; FR3: 6 x 7).  With the rank decision of
    pinv_cod_rect ignored (r = 6, a scratch build) class T misses by up to
    2e16 (UR5e) and 3e8 (FR3); the worst instances are all in T.

    Measured worst relative error against the C oracle over the four forms,
    20 / 20 / 20 instances, none ambiguous:
      ur5e  K 2.1e-13   F 1.1e-12   T 2.0e-14
      fr3   K 5.3e-13   F 1.7e-13   T 4.6e-15
    so 1e-8 holds in class F as well, where J^+ is largest."""
    rd = make_manipulator(robot, cuda)
    ctrl = manipulator.RobotController(0.001, rd)
    q, qd, cls = _pick(robot, "clik", (SG.K, SG.F, SG.T))
    B, link = q.shape[1], LINK[robot]
    xt, xdt = _targets(rd.model, cuda, q, qd, link, 71)
    nu = np.random.default_rng(4).normal(size=q.shape)
    xi, xdi = xt.copy(), np.zeros((6, B))
    xi[9:] += 0.03
    _, om, _ = O.load(robot)
    par = O.default_params(0)
    worst = {c: 0.0 for c in (SG.K, SG.F, SG.T)}
    for cubic, nv_ in _clik_cases(nu):
        if cubic:
            out = ctrl.CLIK_cubic_batch(q, qd, xt, xdt, xi, xdi, 0.3, 0.0, 1.0, link, null_qdot=nv_)
            par.mode, par.t, par.t0, par.duration = 2, 0.3, 0.0, 1.0
        else:
            out = ctrl.CLIK_step_batch(q, qd, xt, xdt, link, null_qdot=nv_)
            par.mode = 1
        out = out.cpu().numpy()
        ref = np.stack([O.clik_one(om, par, q[:, b], qd[:, b], xt[:, b], xdt[:, b], xi[:, b] if cubic else None,
                                   xdi[:, b] if cubic else None, null_qdot=None if nv_ is None else nv_[:, b])
                        for b in range(B)], axis=1)
        assert np.all(np.isfinite(out))
        rel = _rel(out, ref)
        for c in worst:
            worst[c] = max(worst[c], rel[cls == c].max())
        assert np.all(rel <= 1e-8), (cubic, nv_ is not None, np.sort(rel)[-5:], cls[np.argsort(rel)[-5:]])
    print(robot, "CLIK worst relative error by class:", {c: "%.2e" % v for c, v in worst.items()})


@pytest.mark.parametrize("robot", ["ur5e", "fr3"])
def test_osf_by_class(cuda, robot):
    """OSF, OSFStep and OSFCubic, with and without the null-space torque,
    against oracle_osf_one (M^-1, g from pyref) on 20 instances per class:
    1e-8 relative to max(1, |out|_inf) on every instance.  UR5e: K, F, T.
    FR3: F and T only; J M^-1 J^T of FR3 never passes the certificate (0 of
    448 classified states are in K), so its certified path has no input.

    Measured worst relative error against the C oracle over the six forms,
    20 instances per class, none ambiguous:
      ur5e  K 8.5e-14   F 4.8e-12   T 1.7e-12
      fr3   F 4.1e-13   T 1.6e-12"""
    rd = make_manipulator(robot, cuda)
    ctrl = manipulator.RobotController(0.001, rd)
    want = (SG.K, SG.F, SG.T) if robot == "ur5e" else (SG.F, SG.T)
    q, qd, cls = _pick(robot, "osf", want)
    B, link = q.shape[1], LINK[robot]
    xt, xdt = _targets(rd.model, cuda, q, qd, link, 72)
    rng = np.random.default_rng(5)
    nu, xdd = rng.normal(size=q.shape), rng.normal(size=(6, B))
    xi, xdi = xt.copy(), np.zeros((6, B))
    xi[9:] += 0.03
    pm, om, _ = O.load(robot)
    dyn = [R.dynamics(pm, q[:, b], qd[:, b]) for b in range(B)]
    par = O.default_params(0)
    worst = {c: 0.0 for c in want}
    for mode in (0, 1, 2):
        for nv_ in (None, nu):
            if mode == 0:
                out = ctrl.OSF_batch(q, qd, xdd, link, null_torque=nv_)
            elif mode == 1:
                out = ctrl.OSF_step_batch(q, qd, xt, xdt, link, null_torque=nv_)
            else:
                out = ctrl.OSF_cubic_batch(q, qd, xt, xdt, xi, xdi, 0.3, 0.0, 1.0, link, null_torque=nv_)
            out = out.cpu().numpy()
            par.mode, par.t, par.t0, par.duration = mode, 0.3, 0.0, 1.0
            ref = np.stack([O.osf_one(om, par, q[:, b], qd[:, b], dyn[b]["Minv"], dyn[b]["g"],
                                      None if mode == 0 else xt[:, b], xdd[:, b] if mode == 0 else xdt[:, b],
                                      xi[:, b] if mode == 2 else None, xdi[:, b] if mode == 2 else None,
                                      null_torque=None if nv_ is None else nv_[:, b]) for b in range(B)], axis=1)
            assert np.all(np.isfinite(out))
            rel = _rel(out, ref)
            for c in worst:
                worst[c] = max(worst[c], rel[cls == c].max())
            assert np.all(rel <= 1e-8), (mode, nv_ is not None, np.sort(rel)[-5:], cls[np.argsort(rel)[-5:]])
    print(robot, "OSF worst relative error by class:", {c: "%.2e" % v for c, v in worst.items()})


@pytest.mark.parametrize("eps", [0.0, 1e-9, 1e-7])
def test_qpik_at_singularity(cuda, eps):
    """QPIKStep of UR5e with the wrist (32 states) or the elbow (32 states) at
    eps from the exact singularity: all 64 in class T of the manipulability
    stage.  The full parity contract (assert_qpik_parity, no instance beyond
    1e-4), and no instance ends non-finite: det(J J^T) is rounding noise of
    either sign there, and its square root used to be NaN on about half of
    such states ("Manipulability at a singularity").

    Measured: 64 of 64 in class T at each eps; every status SOLVED, no instance
    beyond 1e-4 (expected_off = 0).  Without the clamp in the kernel (a scratch
    build) the stage's m is NaN on some of the 64 states at each of the three
    eps (on about half of them at eps = 0), and all three cases fail."""
    robot = "ur5e"
    rd = make_manipulator(robot, cuda)
    ctrl = manipulator.RobotController(0.001, rd, solver_mode="exact")
    parts = [SG.ur5e_states(j, eps, 32, 80 + j) for j in (SG.UR5E_WRIST, SG.UR5E_ELBOW)]
    q, qd = (np.concatenate([p[i] for p in parts], axis=1) for i in (0, 1))
    _, om, _ = O.load(robot)
    got = SG.counts(SG.classify_batch(lambda x: SG.classify_manip(robot, om, x), q))
    assert got[SG.T] == 64, got
    xt, xdt = _targets(rd.model, cuda, q, qd, LINK[robot], 73)
    assert all(np.all(np.isfinite(a)) for a in (q, qd, xt, xdt))
    out, status = ctrl.QPIK_step_batch(q, qd, xt, xdt, LINK[robot])
    out, status = out.cpu().numpy(), status.cpu().numpy()
    st = stage_pose(rd.model, cuda, q, qd, LINK[robot])
    assert np.all(np.isfinite(st["man"])) and np.all(st["man"][0] >= 0)
    assert not np.any(status == O.NONFINITE), np.nonzero(status == O.NONFINITE)
    assert np.all(np.isfinite(out))
    assert_qpik_parity(robot, rd.model, q, qd, xt, xdt, out, status, 0)


@pytest.mark.parametrize("robot", ["fr3", "ur5e"])
def test_results_do_not_depend_on_instance_order(cuda, robot):
    """B = 4 096 instances tiled K F T K F T ... from 20 states per class, so
    that every persistent wave takes several instances and runs a certified one
    after a fallback one.  The stage outputs, q-dot*, status and iteration
    counts of the run in index order and of a permuted run are bit-equal after
    un-permuting, on the fused and on the two-kernel path (and equal between
    the two).  No oracle."""
    import torch
    rd = make_manipulator(robot, cuda)
    ctrl = manipulator.RobotController(0.001, rd, solver_mode="exact")
    q0, qd0, _ = _pick(robot, "manip", (SG.K, SG.F, SG.T))
    B = 4096
    tile = np.resize(np.arange(q0.shape[1]), B)
    q, qd = np.ascontiguousarray(q0[:, tile]), np.ascontiguousarray(qd0[:, tile])
    xt, xdt = _targets(rd.model, cuda, q, qd, LINK[robot], 74)
    perm = np.random.default_rng(6).permutation(B)
    inv = np.argsort(perm)
    P = lambda a: np.ascontiguousarray(a[:, perm])

    def run(q_, qd_, xt_, xdt_):
        it = torch.zeros(B, dtype=torch.int32, device=cuda)
        out, status = ctrl.QPIK_step_batch(q_, qd_, xt_, xdt_, LINK[robot], iters=it)
        torch.cuda.synchronize()
        return out.cpu().numpy(), status.cpu().numpy(), it.cpu().numpy()

    s_a = stage_pose(rd.model, cuda, q, qd, LINK[robot])
    s_b = stage_pose(rd.model, cuda, P(q), P(qd), LINK[robot])
    for k in s_a:
        np.testing.assert_array_equal(s_a[k], s_b[k][..., inv], err_msg=k)
    res = {}
    try:
        for fused in (1, 0):
            _capi.check(_capi.lib().drc_set_fusion(rd.model.handle, C.c_int(fused)))
            a = run(q, qd, xt, xdt)
            b = run(P(q), P(qd), P(xt), P(xdt))
            for x, y in zip(a, b):
                np.testing.assert_array_equal(x, y[..., inv])
            res[fused] = a
    finally:
        _capi.check(_capi.lib().drc_set_fusion(rd.model.handle, C.c_int(1)))
    for x, y in zip(res[1], res[0]):
        np.testing.assert_array_equal(x, y)
