"""Moving obstacles on the GPU: obstacle twists in the QPIK distance row
(drc_qpik_moving_obstacles_batch, drc_qpik_stages_moving_obstacles_batch,
drc_qpik_rollout_moving_obstacles_batch, the ``obstacle_twist`` keyword).

Reference: the C oracle on the twin of the model (tests/_obstacles.py).  The
rate dd/dt = s n . (v + omega x (pB - p)) is formed from O.pair_distance's
witnesses (tests/_moving.py; its conventions are pinned on the oracle alone in
tests/test_obstacle_rate_oracle.py), and the oracle's QP is fed d + rate /
alpha_cbf in place of d (oracle.qpik_batch_dist).

Tolerances: dist_rate 1e-6 max(1, |v| + |omega| |pB - p|) where the device and
the oracle pick the same pair and the oracle's min distance is smooth -- the
existing 1e-6 on grad d, the same expression for unit joint rates, scaled by
the speed bound of the witness point.  Smooth means smooth in q
(_common.nonsmooth_min_distance, as for grad d) and a unique closest point
(_moving.halfspace_witness_not_unique): Husky-FR3's base box has vertical
edges, the wall of husky_scene is vertical, and no motion of the planar base
tilts one against the other, so the joint-space test cannot see that every
point of such an edge is a closest point -- the rate then depends on which one
is reported (the device reports the edge's centre, halfspace.hpp; the oracle's
GJK / EPA some point of it; the 9 instances of that scene where this pair wins).
At least 16 obstacle pairs must pass the comparison; q-dot* 1e-6 against the oracle's QP on the
device's own stage data with identical statuses; end to end a median of 1e-9
with every instance within 1e-4.  Everything else is bit for bit."""
import ctypes as C

import numpy as np
import pytest

import oracle as O
import _moving as MV
import _obstacles as OB
from _common import LINK, make_manipulator, make_moma, moma_step_inputs, nonsmooth_min_distance, step_inputs
from dyros_robot_controller_amd import _batch, _capi, manipulator, mobile_manipulator

pytestmark = pytest.mark.gpu

_CACHE = {}


def _sync():
    import torch
    torch.cuda.synchronize()


def _stages(rd, q, qd, xt, xdt, link, pose, twist=None):
    """Stage outputs of QPIKStep (with ``twist``: through drc_qpik_stages_moving_obstacles_batch)."""
    p = manipulator.QPIKParamsBuilder(rd.model, exact=True).params(link, _capi.MODE_QPIK_STEP)
    a = lambda v: _batch.as_device(v, rd.device)
    st = _batch.stages_batch(rd.model, p, a(q), a(qd), a(xt), a(xdt), obstacle_pose=pose, obstacle_twist=twist)
    _sync()
    return {k: v.cpu().numpy() for k, v in st.items()}


def _solve(ctrl, q, qd, xt, xdt, link, pose, twist=None):
    import torch
    it = torch.zeros(q.shape[1], dtype=torch.int32, device=ctrl.robot_data_.device)
    out, st = ctrl.QPIK_step_batch(q, qd, xt, xdt, link, iters=it, obstacle_pose=pose, obstacle_twist=twist)
    _sync()
    return out.cpu().numpy(), st.cpu().numpy(), it.cpu().numpy()


def _solve_c(rd, p, q, qd, xt, xdt, pose, twist, ld, xi=None, xdi=None):
    """drc_qpik_moving_obstacles_batch itself (twist None: a NULL pointer)."""
    import torch
    dev = rd.device
    B = q.shape[1]
    a = lambda v: _batch.as_device(v, dev)
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    t = [a(v) for v in (q, qd, xt, xdt, xi, xdi, pose, twist)]
    out = torch.zeros((rd.model.actuated_dof, B), dtype=torch.float64, device=dev)
    status = torch.zeros(B, dtype=torch.int32, device=dev)
    iters = torch.zeros(B, dtype=torch.int32, device=dev)
    _capi.check(_capi.lib().drc_qpik_moving_obstacles_batch(
        rd.model.handle, C.byref(p), C.c_int64(B), *[ptr(v) for v in t[:6]], ptr(t[6]), ptr(t[7]), C.c_int64(ld),
        ptr(out), ptr(status), ptr(iters), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    _sync()
    return out.cpu().numpy(), status.cpu().numpy(), iters.cpu().numpy()


def _fr3(cuda):
    """FR3 with the four obstacles of tests/test_gpu_obstacles.py, 256 workload
    instances with per-instance poses and twists, and the oracle's distance
    stage and rates on the twin (computed once, never modified)."""
    if "fr3" not in _CACHE:
        B = 256
        rd0 = make_manipulator("fr3", cuda)
        q, qd, xt, xdt = step_inputs(rd0, "fr3", 3, B, cuda)
        rd = make_manipulator("fr3", cuda)
        rd.set_obstacles(OB.FOUR_TYPES, OB.FOUR_PARAMS, OB.FR3_ARM_LINKS)
        poses = OB.fr3_scene(11, B)
        twists = np.random.default_rng(77).uniform(-1, 1, (B, 4, 6))
        pm, om, spec, g0 = OB.twin("fr3", OB.FOUR_TYPES, OB.FOUR_PARAMS, OB.FR3_ARM_LINKS)
        d, g, pr = OB.oracle_distance(om, g0, OB.FOUR_TYPES, q, poses)
        rate, scale, _, _, ob = MV.oracle_rates(om, g0, OB.FOUR_TYPES, q, poses, twists)
        _CACHE["fr3"] = dict(rd=rd, rd0=rd0, ctrl=manipulator.RobotController(0.001, rd, solver_mode="exact"),
                             q=q, qd=qd, xt=xt, xdt=xdt, poses=poses, pose_fm=OB.to_field_major(poses),
                             twists=twists, twist_fm=OB.to_field_major(twists), om=om, g0=g0, p0=len(pm.pairs),
                             ref=(d, g, pr), rate=rate, scale=scale, ob=ob)
    return _CACHE["fr3"]


def _assert_rate(om, g0, types, p0, q, poses, twists, st, st_plain, ref_pair, what):
    """Test 1 of the module docstring: dist_rate against the formula on the
    oracle's witnesses, exactly 0 for self pairs, dist and pair those of the
    twist-free stage entry."""
    np.testing.assert_array_equal(st["dist"], st_plain["dist"])
    np.testing.assert_array_equal(st["pair"], st_plain["pair"])
    for k in ("pose", "jac", "man", "xdot_des"):
        np.testing.assert_array_equal(st[k], st_plain[k], err_msg=k)
    rate, scale, _, _, _ = MV.oracle_rates(om, g0, types, q, poses, twists, pairs=st["pair"])
    same = st["pair"] == ref_pair
    err = np.abs(st["dist_rate"] - rate)
    tol = 1e-6 * np.maximum(1.0, scale)
    self_pair = st["pair"] < p0
    print("%s dist_rate: obstacle pair wins %d of %d, same pair as the oracle %d; max |rate - oracle| %.3e "
          "(max |rate| %.3f)" % (what, (~self_pair).sum(), len(err), same.sum(), err[same].max(),
                                 np.abs(st["dist_rate"]).max()))
    assert np.all(st["dist_rate"][self_pair] == 0.0)
    assert (same & ~self_pair).sum() >= 16
    off = np.flatnonzero(same & (err > tol))
    for b in off:   # only where the reference is ill-defined: d without a derivative in q or along the twist
        OB.set_poses(om, g0, types, poses[b])
        slot = om.pair_b[int(ref_pair[b])] - g0
        assert nonsmooth_min_distance(om, q[:, b]) or (types[slot] == OB.HALFSPACE and MV.halfspace_witness_not_unique(
            om, q[:, b], int(ref_pair[b]), poses[b, slot])), (int(b), err[b], tol[b])
    print("%s dist_rate: beyond the tolerance where the oracle's distance is non-smooth: %s" % (what, off.tolist()))
    assert (same & ~self_pair & (err <= tol)).sum() >= 16   # (enough obstacle pairs are compared)


def _assert_qp(om, g0, types, kind, q, qd, xt, xdt, poses, twists, out, status, st, what, min_changed):
    """Test 2 of the module docstring.  Returns the number of instances whose
    oracle answer the twists change by more than 1e-3."""
    par = O.default_params(kind, exact=True)
    par.mode = 1
    fed = st["dist"].copy()
    fed[0] += st["dist_rate"] / par.alpha_cbf
    ref_d, rstat_d, _ = O.qpik_batch_dist(om, par, q, qd, xt, xdt, fed, nthreads=8)
    err_d = np.abs(out - ref_d).max(axis=0)
    # end to end: the oracle's own d, grad d and witnesses
    rate, _, _, _, _ = MV.oracle_rates(om, g0, types, q, poses, twists)
    d, g, _ = OB.oracle_distance(om, g0, types, q, poses)
    ref, rstat, _ = O.qpik_batch_dist(om, par, q, qd, xt, xdt, np.vstack([d + rate / par.alpha_cbf, g]), nthreads=8)
    ref0, rstat0, _ = O.qpik_batch_dist(om, par, q, qd, xt, xdt, np.vstack([d, g]), nthreads=8)
    err = np.abs(out - ref).max(axis=0)
    changed = int((np.abs(ref - ref0).max(axis=0) > 1e-3).sum())
    print("%s: q-dot* on the device's stage data max %.3e; end to end median %.3e, max %.3e; non-solved %d; "
          "the twists change the oracle's answer by more than 1e-3 in %d instances (the device's in %d)"
          % (what, err_d.max(), np.median(err), err.max(), (status != 1).sum(), changed,
             (np.abs(out - ref0).max(axis=0) > 1e-3).sum()))
    assert changed >= min_changed, changed   # (a condition on the inputs, from the oracle alone)
    np.testing.assert_array_equal(status, rstat_d)
    assert err_d.max() <= 1e-6, (err_d.max(), int(err_d.argmax()))
    np.testing.assert_array_equal(status, rstat)
    assert np.median(err) <= 1e-9 and err.max() <= 1e-4, (np.median(err), err.max(), int(err.argmax()))
    assert np.all(out[:, status != 1] == 0.0)
    return changed


# ---------------------------------------------------------------- 1. dist_rate
def test_fr3_dist_rate_matches_oracle_witnesses(cuda):
    """Measured on an MI355X: an obstacle pair wins 202 of the 256 instances, the oracle's pair everywhere;
    max |dist_rate - oracle| 2.3e-12 (max |dist_rate| 2.27); none beyond the tolerance."""
    S = _fr3(cuda)
    link = LINK["fr3"]
    st = _stages(S["rd"], S["q"], S["qd"], S["xt"], S["xdt"], link, S["pose_fm"], S["twist_fm"])
    st0 = _stages(S["rd"], S["q"], S["qd"], S["xt"], S["xdt"], link, S["pose_fm"])
    assert "dist_rate" in st and "dist_rate" not in st0
    # Pose, J, manipulability and the task velocity do not depend on the slots.  The two obstacle entries share
    # their host path, so they are held against drc_qpik_stages_batch on the model without slots (which
    # tests/test_gpu_task_fixed_stages.py holds against the oracle): the same device functions with contraction
    # fixed per source expression (build.sh), hence the same bits
    free = _stages(S["rd0"], S["q"], S["qd"], S["xt"], S["xdt"], link, None)
    for k in ("pose", "jac", "man", "xdot_des"):
        print("FR3 %s: max |with slots - without| %.3e" % (k, np.abs(st[k] - free[k]).max()))
        np.testing.assert_array_equal(st[k], free[k], err_msg=k)
    _assert_rate(S["om"], S["g0"], OB.FOUR_TYPES, S["p0"], S["q"], S["poses"], S["twists"], st, st0, S["ref"][2], "FR3")


# ---------------------------------------------------------------- 2. QP parity
def test_fr3_qpik_step_parity_with_twists(cuda):
    """Measured on an MI355X: q-dot* against the oracle's QP on the device's stage data max 1.2e-11; end to end
    median 2.2e-15, max 1.2e-11; every instance solved; the twists change q-dot* by more than 1e-3 in 23 instances."""
    S = _fr3(cuda)
    q, qd, xt, xdt, link = S["q"], S["qd"], S["xt"], S["xdt"], LINK["fr3"]
    out, status, _ = _solve(S["ctrl"], q, qd, xt, xdt, link, S["pose_fm"], S["twist_fm"])
    st = _stages(S["rd"], q, qd, xt, xdt, link, S["pose_fm"], S["twist_fm"])
    _assert_qp(S["om"], S["g0"], OB.FOUR_TYPES, 0, q, qd, xt, xdt, S["poses"], S["twists"], out, status, st, "FR3", 16)
    plain = _solve(S["ctrl"], q, qd, xt, xdt, link, S["pose_fm"])
    assert (np.abs(out - plain[0]).max(axis=0) > 1e-3).sum() >= 16


# ---------------------------------------------------------------- 3. bit-for-bit properties
def _set_fusion(rd, on):
    _capi.check(_capi.lib().drc_set_fusion(rd.model.handle, C.c_int(on)))


def _same(a, b, what):
    for x, y, name in zip(a, b, ("qdot", "status", "iters")):
        np.testing.assert_array_equal(x, y, err_msg="%s: %s" % (what, name))


def test_fr3_null_and_zero_twist_equal_the_obstacle_entry(cuda):
    S = _fr3(cuda)
    B = 64
    q, qd, xt, xdt = (np.ascontiguousarray(S[k][:, :B]) for k in ("q", "qd", "xt", "xdt"))
    pose = np.ascontiguousarray(S["pose_fm"][:, :, :B])
    link = LINK["fr3"]
    p = S["ctrl"]._pb.params(link, _capi.MODE_QPIK_STEP, S["ctrl"].Kp_task_, S["ctrl"].Kv_task_, 0.0, 0.0, 1.0)
    base = _solve(S["ctrl"], q, qd, xt, xdt, link, pose)           # drc_qpik_obstacles_batch
    _same(_solve_c(S["rd"], p, q, qd, xt, xdt, pose, None, B), base, "twist NULL")
    _same(_solve_c(S["rd"], p, q, qd, xt, xdt, pose, np.zeros((4, 6, B)), B), base, "zero twist")
    _same(_solve(S["ctrl"], q, qd, xt, xdt, link, pose, np.zeros((4, 6))), base, "zero twist, shared")
    st0 = _stages(S["rd"], q, qd, xt, xdt, link, pose)
    stz = _stages(S["rd"], q, qd, xt, xdt, link, pose, np.zeros((4, 6, B)))
    assert np.all(stz["dist_rate"] == 0.0)
    for k in st0:
        np.testing.assert_array_equal(stz[k], st0[k], err_msg=k)


def test_fr3_bitwise_properties(cuda):
    S = _fr3(cuda)
    B = 64
    q, qd, xt, xdt = (np.ascontiguousarray(S[k][:, :B]) for k in ("q", "qd", "xt", "xdt"))
    pose = np.ascontiguousarray(S["pose_fm"][:, :, :B])
    twist = np.ascontiguousarray(S["twist_fm"][:, :, :B])
    link = LINK["fr3"]
    base = _solve(S["ctrl"], q, qd, xt, xdt, link, pose, twist)
    assert not np.array_equal(base[0], _solve(S["ctrl"], q, qd, xt, xdt, link, pose)[0])   # (the twists matter)
    _set_fusion(S["rd"], 0)
    try:
        off = _solve(S["ctrl"], q, qd, xt, xdt, link, pose, twist)
    finally:
        _set_fusion(S["rd"], 1)
    _same(base, off, "fusion off")
    # one shared set (obstacle_ld = 0) and the same set replicated per instance
    one_p, one_t = np.ascontiguousarray(pose[:, :, 5]), np.ascontiguousarray(twist[:, :, 5])
    shared = _solve(S["ctrl"], q, qd, xt, xdt, link, one_p, one_t)
    repl = _solve(S["ctrl"], q, qd, xt, xdt, link, np.ascontiguousarray(np.repeat(one_p[:, :, None], B, axis=2)),
                  np.ascontiguousarray(np.repeat(one_t[:, :, None], B, axis=2)))
    _same(shared, repl, "shared / replicated")
    st_s = _stages(S["rd"], q, qd, xt, xdt, link, one_p, one_t)
    st_r = _stages(S["rd"], q, qd, xt, xdt, link, np.ascontiguousarray(np.repeat(one_p[:, :, None], B, axis=2)),
                   np.ascontiguousarray(np.repeat(one_t[:, :, None], B, axis=2)))
    for k in st_s:
        np.testing.assert_array_equal(st_s[k], st_r[k], err_msg=k)
    assert np.any(st_s["dist_rate"] != 0.0)


def test_fr3_batch_of_2100_agrees_with_its_prefixes(cuda):
    S = _fr3(cuda)
    B = 2100
    rd0 = make_manipulator("fr3", cuda)
    q, qd, xt, xdt = step_inputs(rd0, "fr3", 5, B, cuda)
    pose = OB.to_field_major(OB.fr3_scene(13, B))
    twist = OB.to_field_major(np.random.default_rng(78).uniform(-1, 1, (B, 4, 6)))
    link = LINK["fr3"]
    full = _solve(S["ctrl"], q, qd, xt, xdt, link, pose, twist)
    for n in (1, 64, 1000):
        part = _solve(S["ctrl"], *(np.ascontiguousarray(v[:, :n]) for v in (q, qd, xt, xdt)), link,
                      np.ascontiguousarray(pose[:, :, :n]), np.ascontiguousarray(twist[:, :, :n]))
        _same([v[..., :n] for v in full], part, "prefix %d" % n)
    _set_fusion(S["rd"], 0)
    try:
        off = _solve(S["ctrl"], q, qd, xt, xdt, link, pose, twist)
    finally:
        _set_fusion(S["rd"], 1)
    _same(full, off, "B = 2100, fusion off")


def test_fr3_controller_entries_agree_with_the_c_entry(cuda):
    S = _fr3(cuda)
    B = 64
    q, qd, xt, xdt = (np.ascontiguousarray(S[k][:, :B]) for k in ("q", "qd", "xt", "xdt"))
    pose = np.ascontiguousarray(S["pose_fm"][:, :, :B])
    twist = np.ascontiguousarray(S["twist_fm"][:, :, :B])
    link, ctrl, rd = LINK["fr3"], S["ctrl"], S["rd"]
    par = lambda mode, t=0.0, t0=0.0, T=1.0: ctrl._pb.params(link, mode, ctrl.Kp_task_, ctrl.Kv_task_, t, t0, T)
    host = lambda r: (r[0].cpu().numpy(), r[1].cpu().numpy())
    got = host(ctrl.QPIK_batch(q, qd, xdt, link, obstacle_pose=pose, obstacle_twist=twist))
    want = _solve_c(rd, par(_capi.MODE_QPIK), q, qd, None, xdt, pose, twist, B)
    _same(got, want[:2], "QPIK_batch")
    got = host(ctrl.QPIK_step_batch(q, qd, xt, xdt, link, obstacle_pose=pose, obstacle_twist=twist))
    want = _solve_c(rd, par(_capi.MODE_QPIK_STEP), q, qd, xt, xdt, pose, twist, B)
    _same(got, want[:2], "QPIK_step_batch")
    st = _stages(rd, q, qd, xt, xdt, link, pose)
    xi, xdi = st["pose"], np.zeros((6, B))
    got = host(ctrl.QPIK_cubic_batch(q, qd, xt, xdt, xi, xdi, 0.3, 0.0, 1.0, link, obstacle_pose=pose,
                                     obstacle_twist=twist))
    want = _solve_c(rd, par(_capi.MODE_QPIK_CUBIC, 0.3, 0.0, 1.0), q, qd, xt, xdt, pose, twist, B, xi, xdi)
    _same(got, want[:2], "QPIK_cubic_batch")
    with pytest.raises(ValueError):
        ctrl.QPIK_step_batch(q, qd, xt, xdt, link, obstacle_twist=twist)
    with pytest.raises(ValueError):
        ctrl.QPIK_rollout_batch(q, qd, xt, xdt, link, 2, obstacle_twist=twist)


# ---------------------------------------------------------------- 4. mobile manipulator
def test_husky_fr3_world_frame_twists(cuda):
    """Measured on an MI355X: an obstacle pair wins 34 of 64 instances, the oracle's pair everywhere; dist_rate
    beyond the tolerance in the 9 instances where the wall wins against the base box's vertical edge (module
    docstring; up to 9.4e-2, half the edge's height times the tilt rate), 25 obstacle pairs compared; q-dot* on the
    device's stage data max 1.3e-11, end to end median 5.8e-13, max 1.3e-11; 20 PrimalInfeasible on both sides."""
    robot, B = "husky_fr3", 64
    rd0 = make_moma(robot, cuda)
    q, qd, xt, xdt = moma_step_inputs(rd0, robot, 17, B, cuda)
    rd = make_moma(robot, cuda)
    rd.set_obstacles(OB.HUSKY_TYPES, OB.HUSKY_PARAMS, OB.HUSKY_LINKS)
    pm, om, spec, g0 = OB.twin(robot, OB.HUSKY_TYPES, OB.HUSKY_PARAMS, OB.HUSKY_LINKS)
    poses = OB.husky_scene(51, q, spec["joint_index"][0])
    twists = np.random.default_rng(79).uniform(-1, 1, (B, 2, 6))   # world frame, like the poses
    ref = OB.oracle_distance(om, g0, OB.HUSKY_TYPES, q, poses)
    pose_fm, twist_fm = OB.to_field_major(poses), OB.to_field_major(twists)
    link = LINK[robot]
    st = _stages(rd, q, qd, xt, xdt, link, pose_fm, twist_fm)
    st0 = _stages(rd, q, qd, xt, xdt, link, pose_fm)
    _assert_rate(om, g0, OB.HUSKY_TYPES, len(pm.pairs), q, poses, twists, st, st0, ref[2], "Husky-FR3")
    ctrl = mobile_manipulator.RobotController(0.001, rd, solver_mode="exact")
    out, status, _ = _solve(ctrl, q, qd, xt, xdt, link, pose_fm, twist_fm)
    _assert_qp(om, g0, OB.HUSKY_TYPES, 1, q, qd, xt, xdt, poses, twists, out, status, st, "Husky-FR3", 0)


# ---------------------------------------------------------------- 5. rollout
@pytest.mark.parametrize("twist_per_step", [False, True])
def test_fr3_rollout_equals_single_steps(cuda, twist_per_step):
    S = _fr3(cuda)
    B, steps, dt = 64, 4, 0.001
    q, qd, xt, xdt = (np.ascontiguousarray(S[k][:, :B]) for k in ("q", "qd", "xt", "xdt"))
    link = LINK["fr3"]
    pose0 = np.ascontiguousarray(S["pose_fm"][:, :, :B])
    twist0 = np.ascontiguousarray(S["twist_fm"][:, :, :B])
    pose = _batch.obstacle_trajectory(pose0, twist0, dt, steps).numpy()
    np.testing.assert_array_equal(pose[0], pose0)
    # (per step: another twist each step with the same poses -- the entry takes what it is given)
    twist = np.stack([twist0 * (1.0 - 0.25 * k) for k in range(steps)]) if twist_per_step else twist0
    want = ("qdot_traj", "q_traj", "dist_traj", "iters_traj")
    res = S["ctrl"].QPIK_rollout_batch(q, qd, xt, xdt, link, steps, dt=dt, want=want, obstacle_pose=pose,
                                       obstacle_twist=twist)
    free = S["ctrl"].QPIK_rollout_batch(q, qd, xt, xdt, link, steps, dt=dt, want=want, obstacle_pose=pose)
    _sync()
    np.testing.assert_array_equal(res.dist_traj[0].cpu().numpy(), free.dist_traj[0].cpu().numpy())
    assert not np.array_equal(res.qdot_traj[0].cpu().numpy(), free.qdot_traj[0].cpu().numpy())
    qk, vk = q.copy(), qd.copy()
    for k in range(steps):
        pk = np.ascontiguousarray(pose[k])
        tk = np.ascontiguousarray(twist[k]) if twist_per_step else twist
        eta, status, iters = _solve(S["ctrl"], qk, vk, xt, xdt, link, pk, tk)
        st = _stages(S["rd"], qk, vk, xt, xdt, link, pk, tk)
        np.testing.assert_array_equal(res.qdot_traj[k].cpu().numpy(), eta, err_msg="qdot_traj %d" % k)
        np.testing.assert_array_equal(res.status_traj[k].cpu().numpy(), status, err_msg="status_traj %d" % k)
        np.testing.assert_array_equal(res.iters_traj[k].cpu().numpy(), iters, err_msg="iters_traj %d" % k)
        np.testing.assert_array_equal(res.dist_traj[k].cpu().numpy(), st["dist"], err_msg="dist_traj %d" % k)
        vk = eta
        qk = qk + dt * vk
        np.testing.assert_array_equal(res.q_traj[k].cpu().numpy(), qk, err_msg="q_traj %d" % k)
    np.testing.assert_array_equal(res.q_final.cpu().numpy(), qk)
    np.testing.assert_array_equal(res.qdot_final.cpu().numpy(), vk)


# ---------------------------------------------------------------- 6. the effect
# instances of the seed-3 workload states on which the oracle's loop shows the effect (chosen from the oracle
# alone; on most of the others the arm's softened row does not react to a sphere coming in from this side at all)
EFFECT_INSTANCES = (0, 2, 10, 11, 13, 25, 27, 28)
SPHERE_R = 0.08


def _place_sphere(om, g0, p0, qb, clearance):
    """Centre of the sphere slot with ``clearance`` to the closest paired arm
    geometry, on that geometry's outward normal, and the unit approach direction."""
    c = np.array([0.6, 0.3, 0.6])
    for _ in range(20):
        OB.set_poses(om, g0, (OB.SPHERE,), OB.pack_poses(np.eye(3)[None], c[None]))
        d, pA, _ = min((O.pair_distance(om, qb, p) for p in range(p0, om.npairs)), key=lambda r: r[0])
        n = (c - pA) / np.linalg.norm(c - pA)
        if abs(d - clearance) <= 1e-12:
            return c, -n
        c = pA + n * (clearance + SPHERE_R)
    raise AssertionError("no placement with the clearance asked for")


def _oracle_loop(om, g0, q0, xt, traj, twists, steps, dt, with_term):
    """The closed loop of the rollout on the CPU oracle (QPIKStep, v = q-dot*,
    q += dt v): the minimum over the steps of the distance, per instance."""
    B = q0.shape[1]
    par = O.default_params(0, exact=True)
    par.mode = 1
    qk, vk, xdt = q0.copy(), np.zeros_like(q0), np.zeros((6, B))
    dmin = np.full(B, np.inf)
    for k in range(steps):
        dist = np.zeros((1 + om.nv, B))
        for b in range(B):
            OB.set_poses(om, g0, (OB.SPHERE,), traj[k, :, :, b])
            d, g, pr = O.min_distance(om, qk[:, b])
            dmin[b] = min(dmin[b], d)
            rate = 0.0
            if with_term and om.pair_b[pr] >= g0:
                dd, pA, pB = O.pair_distance(om, qk[:, b], pr)
                rate = MV.rate_formula(dd, pA, pB, traj[k, 0, 9:12, b], twists[b, 0])
            dist[0, b], dist[1:, b] = d + rate / par.alpha_cbf, g
        vk, status, _ = O.qpik_batch_dist(om, par, qk, vk, xt, xdt, dist, nthreads=8)
        assert np.all(status == 1), (k, status)
        qk = qk + dt * vk
    return dmin


def test_fr3_approaching_sphere_keeps_more_clearance_with_the_term(cuda):
    """A sphere 0.08 m from the resting arm comes in at 0.5 m/s (steady-state deficit v / alpha = 10 mm without the
    term).  Measured: the oracle's minimum clearance with the term is 3.2 to 9.8 mm above the one without; on an MI355X
    the device's figures equal the oracle's to the five digits printed."""
    B, steps, dt, speed = len(EFFECT_INSTANCES), 150, 0.001, 0.5
    pm, om, spec, g0 = OB.twin("fr3", (OB.SPHERE,), ((SPHERE_R, 0, 0),), OB.FR3_ARM_LINKS)
    p0 = len(pm.pairs)
    q0 = np.ascontiguousarray(OB.fr3_states(om, 3, 32)[0][:, list(EFFECT_INSTANCES)])
    xt = np.stack([O.fk_pose(om, q0[:, b])[0] for b in range(B)], axis=1)   # the target: the pose the arm has
    pose0, twists = np.zeros((B, 1, 12)), np.zeros((B, 1, 6))
    for b in range(B):
        c, u = _place_sphere(om, g0, p0, q0[:, b], 0.08)
        pose0[b, 0], twists[b, 0, :3] = OB.pack_poses(np.eye(3), c), speed * u
    pose_fm, twist_fm = OB.to_field_major(pose0), OB.to_field_major(twists)
    traj = _batch.obstacle_trajectory(pose_fm, twist_fm, dt, steps).numpy()   # [steps][1][12][B]
    o_with = _oracle_loop(om, g0, q0, xt, traj, twists, steps, dt, True)
    o_without = _oracle_loop(om, g0, q0, xt, traj, twists, steps, dt, False)
    print("oracle: min clearance with the term    %s" % np.array2string(o_with, precision=5))
    print("oracle: min clearance without the term %s" % np.array2string(o_without, precision=5))
    assert np.all(o_with - o_without >= 1e-3), o_with - o_without   # (a condition on the inputs, from the oracle alone)
    rd = make_manipulator("fr3", cuda)
    rd.set_obstacles((OB.SPHERE,), ((SPHERE_R, 0, 0),), OB.FR3_ARM_LINKS)
    ctrl = manipulator.RobotController(dt, rd, solver_mode="exact")
    run = lambda tw: ctrl.QPIK_rollout_batch(q0, np.zeros_like(q0), xt, np.zeros((6, B)), LINK["fr3"], steps, dt=dt,
                                             want=("dist_traj",), obstacle_pose=traj, obstacle_twist=tw)
    r_with, r_without = run(twist_fm), run(None)
    _sync()
    assert np.all(r_with.status_traj.cpu().numpy() == 1) and np.all(r_without.status_traj.cpu().numpy() == 1)
    d_with = r_with.dist_traj[:, 0].cpu().numpy().min(axis=0)
    d_without = r_without.dist_traj[:, 0].cpu().numpy().min(axis=0)
    print("device: min clearance with the term    %s" % np.array2string(d_with, precision=5))
    print("device: min clearance without the term %s" % np.array2string(d_without, precision=5))
    assert np.all(d_with - d_without >= 0.5 * (o_with - o_without)), (d_with - d_without, o_with - o_without)


# ---------------------------------------------------------------- 7. errors
def _rc(fn, *args):
    rc = fn(*args)
    return rc, _capi.lib().drc_last_error().decode()


def test_error_codes(cuda):
    import torch
    S = _fr3(cuda)
    lib = _capi.lib()
    rd = make_manipulator("fr3", cuda)   # no slots yet
    h = rd.model.handle
    B, steps = 8, 2
    dev = lambda v: _batch.as_device(np.ascontiguousarray(v), cuda)
    q, qd, xt, xdt = (dev(S[k][:, :B]) for k in ("q", "qd", "xt", "xdt"))
    pose, twist = dev(S["pose_fm"][:, :, :B]), dev(S["twist_fm"][:, :, :B])
    mark = 7.25
    out = torch.full((steps * 8, B), mark, dtype=torch.float64, device=cuda)   # (room for any one output: dist_traj)
    rate = torch.full((B,), mark, dtype=torch.float64, device=cuda)
    status = torch.full((steps, B), 77, dtype=torch.int32, device=cuda)
    qf, vf = torch.full((7, B), mark, dtype=torch.float64, device=cuda), torch.full((7, B), mark, dtype=torch.float64, device=cuda)
    p = manipulator.QPIKParamsBuilder(rd.model, exact=True).params(LINK["fr3"], _capi.MODE_QPIK_STEP)
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    stream = C.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)

    def calls(par, tw, ld):
        """The three new entries with these params, twist and obstacle_ld: their return codes and messages."""
        plain = (h, C.byref(par), C.c_int64(B), ptr(q), ptr(qd), ptr(xt), ptr(xdt), None, None)
        roll = (h, C.byref(par), C.c_int64(B), C.c_int(steps), C.c_double(0.001), ptr(q), ptr(qd), ptr(xt), ptr(xdt),
                None, None, C.c_int(0))
        return (_rc(lib.drc_qpik_moving_obstacles_batch, *plain, ptr(pose), ptr(tw), C.c_int64(ld), ptr(out),
                    ptr(status), None, stream),
                _rc(lib.drc_qpik_stages_moving_obstacles_batch, *plain, ptr(pose), ptr(tw), C.c_int64(ld), None, None,
                    None, ptr(out), None, None, ptr(rate), stream),
                _rc(lib.drc_qpik_rollout_moving_obstacles_batch, *roll, ptr(pose), ptr(tw), C.c_int64(ld), C.c_int(0),
                    ptr(qf), ptr(vf), None, ptr(status), None, None, None, ptr(out), stream))

    def refused(res):
        for rc, msg in res:
            assert rc == _capi.DRC_ERR_INVALID_ARGUMENT and msg, (rc, msg)
        _sync()
        for t in (out, rate, qf, vf):
            assert torch.all(t == mark)
        assert torch.all(status == 77)

    refused(calls(p, twist, B))          # a model without slots
    refused(calls(p, None, B))
    rd.set_obstacles(OB.FOUR_TYPES, OB.FOUR_PARAMS, OB.FR3_ARM_LINKS)
    p = manipulator.QPIKParamsBuilder(rd.model, exact=True).params(LINK["fr3"], _capi.MODE_QPIK_STEP)
    refused(calls(p, twist, B - 1))      # a bad obstacle_ld
    bad = manipulator.QPIKParamsBuilder(rd.model, exact=True).params(LINK["fr3"], _capi.MODE_QPIK_STEP)
    for alpha in (0.0, -1.0, float("nan")):
        bad.alpha_cbf = alpha
        refused(calls(bad, twist, B))    # the rate enters as d + rate / alpha_cbf
    bad.alpha_cbf = 0.0
    # (without a twist alpha_cbf = 0 stays what it was: the obstacle entry's answer)
    rc, msg = calls(bad, None, B)[0]
    assert rc == _capi.DRC_OK, (rc, msg)
    # the plain and the obstacle entries behave as before on the same model
    plain = (h, C.byref(p), C.c_int64(B), ptr(q), ptr(qd), ptr(xt), ptr(xdt), None, None)
    rc, msg = _rc(lib.drc_qpik_batch, *plain, ptr(out), ptr(status), None, stream)
    assert rc == _capi.DRC_ERR_INVALID_ARGUMENT and "drc_qpik_obstacles_batch" in msg, (rc, msg)
    rc, msg = _rc(lib.drc_qpik_obstacles_batch, *plain, ptr(pose), C.c_int64(B), ptr(out), ptr(status), None, stream)
    assert rc == _capi.DRC_OK, (rc, msg)
    for res in calls(p, twist, B) + calls(p, None, B):
        assert res[0] == _capi.DRC_OK, res
    _sync()
    assert torch.all(rate == 0.0)        # the last stages call had no twist: nothing but the robot moves
