"""Obstacle slots in the QPIK distance stage (drc_model_set_obstacles, the
drc_qpik_*obstacles_batch entries, RobotData.set_obstacles and the
``obstacle_pose`` keyword) on the GPU.

Reference: the C oracle on the twin of the model (tests/_obstacles.py): the
slots appended to oracle.OracleModel as geometries of joint 0, their pose
written into gplace per instance, a half-space standing as a box of 20 m half
extents with its +z face in the plane.

Tolerances are the project's existing ones: the distance stage's 1e-9
separated / 1e-6 penetrating, 1e-6 on its gradient where the same pair wins
and the oracle's min distance is smooth (tests/_common.py
nonsmooth_min_distance), q-dot* 1e-6 against the oracle's QP fed the device's
own distance stage (oracle.qpik_batch_dist) with identical statuses, and end to
end (the oracle's own narrow phase) a median of 1e-9 with every instance within
1e-4.  Everything else is bit for bit."""
import ctypes as C

import numpy as np
import pytest

import oracle as O
import _obstacles as OB
from _common import LINK, make_manipulator, make_moma, moma_step_inputs, nonsmooth_min_distance, step_inputs
from dyros_robot_controller_amd import _batch, _capi, manipulator, mobile_manipulator

pytestmark = pytest.mark.gpu

_CACHE = {}


def _sync():
    import torch
    torch.cuda.synchronize()


def _stages(rd, q, qd, xt, xdt, link, pose):
    """Stage outputs of QPIKStep through drc_qpik_stages_obstacles_batch."""
    p = manipulator.QPIKParamsBuilder(rd.model, exact=True).params(link, _capi.MODE_QPIK_STEP)
    a = lambda v: _batch.as_device(v, rd.device)
    st = _batch.stages_batch(rd.model, p, a(q), a(qd), a(xt), a(xdt), obstacle_pose=pose)
    _sync()
    return {k: v.cpu().numpy() for k, v in st.items()}


def _solve(ctrl, q, qd, xt, xdt, link, pose=None):
    import torch
    it = torch.zeros(q.shape[1], dtype=torch.int32, device=ctrl.robot_data_.device)
    out, st = ctrl.QPIK_step_batch(q, qd, xt, xdt, link, iters=it, obstacle_pose=pose)
    _sync()
    return out.cpu().numpy(), st.cpu().numpy(), it.cpu().numpy()


def _fr3(cuda):
    """FR3 with the four obstacles on the links moved by joint 3 and beyond, a
    slot-free FR3, 256 workload instances with per-instance poses, and the
    oracle's distance stage on the twin (computed once, never modified)."""
    if "fr3" not in _CACHE:
        rd0 = make_manipulator("fr3", cuda)
        q, qd, xt, xdt = step_inputs(rd0, "fr3", 3, 256, cuda)
        rd = make_manipulator("fr3", cuda)
        rd.set_obstacles(OB.FOUR_TYPES, OB.FOUR_PARAMS, OB.FR3_ARM_LINKS)
        poses = OB.fr3_scene(11, 256)
        pm, om, spec, g0 = OB.twin("fr3", OB.FOUR_TYPES, OB.FOUR_PARAMS, OB.FR3_ARM_LINKS)
        d, g, pr = OB.oracle_distance(om, g0, OB.FOUR_TYPES, q, poses)
        _CACHE["fr3"] = dict(rd0=rd0, rd=rd, ctrl=manipulator.RobotController(0.001, rd, solver_mode="exact"),
                             ctrl0=manipulator.RobotController(0.001, rd0, solver_mode="exact"),
                             q=q, qd=qd, xt=xt, xdt=xdt, poses=poses, pose_fm=OB.to_field_major(poses),
                             om=om, g0=g0, p0=len(pm.pairs), nw=(om.npairs - len(pm.pairs)) // 4,
                             ref=(d, g, pr))
    return _CACHE["fr3"]


def _assert_distance_stage(om, g0, types, q, poses, st, ref, max_pair_ties=2):
    """d, grad d and the pair against the oracle (module docstring)."""
    d, g, pr = ref
    dd = np.abs(st["dist"][0] - d)
    same = st["pair"] == pr
    dg = np.abs(st["dist"][1:] - g).max(axis=0)
    print("distance stage: max |d dist| separated %.3e, penetrating %.3e; pair differs in %d; max |d grad| %.3e" %
          (dd[d > 0].max() if (d > 0).any() else 0, dd[d <= 0].max() if (d <= 0).any() else 0, (~same).sum(),
           dg[same].max()))
    assert np.all(dd <= np.where(d > 0, 1e-9, 1e-6)), (dd.max(), int(dd.argmax()))
    # another closest pair only where two candidates tie within the tolerance (then d agrees, checked above)
    assert (~same).sum() <= max_pair_ties, np.flatnonzero(~same)
    for b in np.flatnonzero(same & (dg > 1e-6)):
        OB.set_poses(om, g0, types, poses[b])
        assert nonsmooth_min_distance(om, q[:, b]), (int(b), dg[b])


# ---------------------------------------------------------------- 1. distance stage
def test_fr3_distance_stage_matches_oracle(cuda):
    """Measured on an MI355X: closest pair sphere 16 (13 separated / 3 penetrating), box 34 (21 / 13), cylinder
    15 (9 / 6), half-space 137 (34 / 103), a self pair 54 of the 256 instances; max |d dist| 1.5e-14 separated,
    2.3e-14 penetrating, the pair differs nowhere, max |d grad| 3.8e-12."""
    S = _fr3(cuda)
    d, g, pr = S["ref"]
    # the inputs exercise every obstacle type, separated and penetrating (from the oracle alone)
    for i, name in enumerate(("sphere", "box", "cylinder", "half-space")):
        win = (pr >= S["p0"] + i * S["nw"]) & (pr < S["p0"] + (i + 1) * S["nw"])
        assert win.sum() >= 8 and (win & (d > 0)).any() and (win & (d < 0)).any(), \
            (name, win.sum(), (win & (d > 0)).sum(), (win & (d < 0)).sum())
    assert (S["rd"].model.n_geoms, S["rd"].model.n_pairs) == (35 + 4, 180 + 4 * 23)
    st = _stages(S["rd"], S["q"], S["qd"], S["xt"], S["xdt"], LINK["fr3"], S["pose_fm"])
    _assert_distance_stage(S["om"], S["g0"], OB.FOUR_TYPES, S["q"], S["poses"], st, S["ref"])


def test_fr3_halfspace_matches_numpy_closed_form(cuda):
    """Where a half-space pair wins, d equals the numpy closed form evaluated
    on the oracle's pose of the winning geometry."""
    S = _fr3(cuda)
    om, d, pr = S["om"], S["ref"][0], S["ref"][2]
    st = _stages(S["rd"], S["q"], S["qd"], S["xt"], S["xdt"], LINK["fr3"], S["pose_fm"])
    first = S["p0"] + 3 * S["nw"]
    wins = np.flatnonzero((pr >= first) & (st["pair"] == pr))
    assert len(wins) >= 8
    worst = 0.0
    for b in wins:
        ga = om.pair_a[int(pr[b])]
        Tj = O.joint_placement(om, S["q"][:, b], om.gparent[ga])
        gp = np.array([om.gplace[ga][i] for i in range(12)])
        Rg, c = Tj[:3, :3] @ gp[:9].reshape(3, 3), Tj[:3, :3] @ gp[9:] + Tj[:3, 3]
        pose = S["poses"][b, 3]
        dn, _, _ = OB.halfspace_closed_form(om.gtype[ga], [om.gparam[ga][i] for i in range(3)], Rg, c,
                                            pose[:9].reshape(3, 3).T, pose[9:])
        worst = max(worst, abs(st["dist"][0, b] - dn))
    print("half-space winners %d: max |d - closed form| %.3e" % (len(wins), worst))
    assert worst <= 1e-12, worst   # a few products of O(1) values on either side (tests/test_halfspace_host.py)


# ---------------------------------------------------------------- 2. end to end
def test_fr3_qpik_step_parity(cuda):
    """Measured on an MI355X: q-dot* against the oracle's QP on the device's distance stage max 1.1e-11; end to end
    median 2.3e-15, max 1.1e-11; every instance solved."""
    S = _fr3(cuda)
    q, qd, xt, xdt, om = S["q"], S["qd"], S["xt"], S["xdt"], S["om"]
    out, status, _ = _solve(S["ctrl"], q, qd, xt, xdt, LINK["fr3"], S["pose_fm"])
    st = _stages(S["rd"], q, qd, xt, xdt, LINK["fr3"], S["pose_fm"])
    par = O.default_params(0, exact=True)
    par.mode = 1
    ref_d, rstat_d, _ = O.qpik_batch_dist(om, par, q, qd, xt, xdt, st["dist"], nthreads=8)
    err_d = np.abs(out - ref_d).max(axis=0)
    print("q-dot* against the oracle's QP on the device's distance stage: max %.3e; non-solved %d" %
          (err_d.max(), (status != 1).sum()))
    np.testing.assert_array_equal(status, rstat_d)
    assert err_d.max() <= 1e-6, (err_d.max(), int(err_d.argmax()))
    ref, rstat = np.zeros_like(out), np.zeros_like(status)
    for b in range(q.shape[1]):
        OB.set_poses(om, S["g0"], OB.FOUR_TYPES, S["poses"][b])
        rstat[b], ref[:, b], _ = O.qpik_one(om, par, q[:, b], qd[:, b], xt[:, b], xdt[:, b])
    err = np.abs(out - ref).max(axis=0)
    print("end to end: median %.3e, max %.3e, beyond 1e-4: %d" % (np.median(err), err.max(), (err > 1e-4).sum()))
    np.testing.assert_array_equal(status, rstat)
    assert np.median(err) <= 1e-9 and err.max() <= 1e-4, (np.median(err), err.max(), int(err.argmax()))
    assert np.all(out[:, status != 1] == 0.0)
    active = st["dist"][0] < 0.05 + 0.2   # the CBF row can bind: d near dist_min
    assert active.sum() >= 32, active.sum()


# ---------------------------------------------------------------- 3. bit-for-bit properties
def _set_fusion(rd, on):
    _capi.check(_capi.lib().drc_set_fusion(rd.model.handle, C.c_int(on)))


def test_fr3_bitwise_properties(cuda):
    S = _fr3(cuda)
    B = 64
    q, qd, xt, xdt = (np.ascontiguousarray(S[k][:, :B]) for k in ("q", "qd", "xt", "xdt"))
    pose = np.ascontiguousarray(S["pose_fm"][:, :, :B])
    link = LINK["fr3"]
    base = _solve(S["ctrl"], q, qd, xt, xdt, link, pose)
    # fusion on / off
    _set_fusion(S["rd"], 0)
    try:
        off = _solve(S["ctrl"], q, qd, xt, xdt, link, pose)
    finally:
        _set_fusion(S["rd"], 1)
    for a, b in zip(base, off):
        np.testing.assert_array_equal(a, b)
    # a batch and its two halves
    for lo, hi in ((0, B // 2), (B // 2, B)):
        half = _solve(S["ctrl"], *(np.ascontiguousarray(v[:, lo:hi]) for v in (q, qd, xt, xdt)), link,
                      np.ascontiguousarray(pose[:, :, lo:hi]))
        for a, b in zip(base, half):
            np.testing.assert_array_equal(a[..., lo:hi], b)
    # shared poses (ld = 0) and the same poses replicated per instance
    one = np.ascontiguousarray(pose[:, :, 5])
    shared = _solve(S["ctrl"], q, qd, xt, xdt, link, one)
    repl = _solve(S["ctrl"], q, qd, xt, xdt, link, np.ascontiguousarray(np.repeat(one[:, :, None], B, axis=2)))
    for a, b in zip(shared, repl):
        np.testing.assert_array_equal(a, b)
    assert not np.array_equal(shared[0], base[0])   # (the poses matter)
    st_s = _stages(S["rd"], q, qd, xt, xdt, link, one)
    st_r = _stages(S["rd"], q, qd, xt, xdt, link, np.ascontiguousarray(np.repeat(one[:, :, None], B, axis=2)))
    for k in st_s:
        np.testing.assert_array_equal(st_s[k], st_r[k], err_msg=k)


def test_fr3_far_obstacles_equal_slot_free_model(cuda):
    S = _fr3(cuda)
    B = 64
    q, qd, xt, xdt = (np.ascontiguousarray(S[k][:, :B]) for k in ("q", "qd", "xt", "xdt"))
    link = LINK["fr3"]
    eye = np.eye(3)
    far = OB.pack_poses(np.stack([eye] * 4), np.array([[1000.0, 0, 0], [0, 1000.0, 0], [-1000.0, 0, 0],
                                                       [0, 0, -1000.0]]))   # the half-space: everything below z = -1000
    st = _stages(S["rd"], q, qd, xt, xdt, link, far)
    assert np.all((st["pair"] >= 0) & (st["pair"] < S["p0"]))   # a self pair wins every instance
    got = _solve(S["ctrl"], q, qd, xt, xdt, link, far)
    want = _solve(S["ctrl0"], q, qd, xt, xdt, link)
    for a, b in zip(got, want):
        np.testing.assert_array_equal(a, b)
    a = lambda v: _batch.as_device(v, cuda)
    p = manipulator.QPIKParamsBuilder(S["rd0"].model, exact=True).params(link, _capi.MODE_QPIK_STEP)
    st0 = {k: v.cpu().numpy() for k, v in _batch.stages_batch(S["rd0"].model, p, a(q), a(qd), a(xt), a(xdt)).items()}
    for k in st0:
        np.testing.assert_array_equal(st[k], st0[k], err_msg=k)


def test_fr3_removing_the_slots_restores_the_model(cuda):
    S = _fr3(cuda)
    B = 64
    q, qd, xt, xdt = (np.ascontiguousarray(S[k][:, :B]) for k in ("q", "qd", "xt", "xdt"))
    rd = make_manipulator("fr3", cuda)
    ctrl = manipulator.RobotController(0.001, rd, solver_mode="exact")
    rd.set_obstacles(OB.FOUR_TYPES, OB.FOUR_PARAMS, OB.FR3_ARM_LINKS)
    with_slots = _solve(ctrl, q, qd, xt, xdt, LINK["fr3"], np.ascontiguousarray(S["pose_fm"][:, :, :B]))
    rd.set_obstacles([])
    assert (rd.model.n_geoms, rd.model.n_pairs, rd.model.n_obstacles) == (35, 180, 0)
    got = _solve(ctrl, q, qd, xt, xdt, LINK["fr3"])
    want = _solve(S["ctrl0"], q, qd, xt, xdt, LINK["fr3"])
    for a, b in zip(got, want):
        np.testing.assert_array_equal(a, b)
    assert not np.array_equal(with_slots[0], want[0])


# ---------------------------------------------------------------- 4. full wave, long candidate list
def _distance_case(cuda, types, params, links, poses, seed, B):
    rd0 = _fr3(cuda)["rd0"]
    q, qd, xt, xdt = step_inputs(rd0, "fr3", seed, B, cuda)
    rd = make_manipulator("fr3", cuda)
    rd.set_obstacles(types, params, links)
    pm, om, spec, g0 = OB.twin("fr3", types, params, links)
    assert (rd.model.n_geoms, rd.model.n_pairs) == (om.ngeom, om.npairs)
    ref = OB.oracle_distance(om, g0, types, q, poses)
    st = _stages(rd, q, qd, xt, xdt, LINK["fr3"], OB.to_field_major(poses))
    _assert_distance_stage(om, g0, types, q, poses, st, ref)
    return rd, ref, len(pm.pairs)


def test_fr3_sixty_four_geometries(cuda):
    """FR3 plus 29 spheres on the last two links' geometries: exactly 64
    geometries, every lane of the geometry-pose stage busy."""
    B = 32
    types, params = (OB.SPHERE,) * 29, ((0.05, 0, 0),) * 29
    rd, (d, g, pr), p0 = _distance_case(cuda, types, params, ("fr3_link6", "fr3_link7"), OB.spheres_scene(41, B), 9, B)
    assert rd.model.n_geoms == 64 and rd.model.n_pairs == 180 + 29 * 9
    assert (pr >= p0).sum() >= 8 and ((pr >= p0) & (d < 0)).any() and ((pr >= p0) & (d > 0)).any()


def test_fr3_candidate_list_beyond_the_epa_stash(cuda):
    """FR3 plus 27 plates on every moving link: 405 plate pairs without a
    closed form, of which 348 .. 405 per instance stay GJK candidates after the
    broad phase (counted on the CPU with tools/narrow_host_test.hip's lower
    bounds for these inputs, the plate pairs alone) -- beyond the 336 entries
    at which the candidate list once met the EPA seed stash
    (tests/test_gpu_many_candidates.py); 19 .. 91 of them intersect."""
    B = 32
    types, params = (OB.BOX,) * 27, (OB.PLATE,) * 27
    rd, (d, g, pr), p0 = _distance_case(cuda, types, params, None, OB.plates_scene(31, B), 7, B)
    assert rd.model.n_pairs == 180 + 27 * 31
    assert (d < 0).sum() >= B // 2


# ---------------------------------------------------------------- 5. mobile manipulator
def test_husky_fr3_world_obstacles(cuda):
    """Husky-FR3, a box and a wall in the world frame, the base's geometry among the paired links.  Measured on an
    MI355X: the box wins 18, the wall 16 of 64 instances; max |d dist| 3.5e-15, max |d grad| 1.3e-13; q-dot* on the
    device's distance stage max 6.8e-12, end to end median 5.7e-13, max 7.2e-12; 21 PrimalInfeasible on both sides."""
    robot, B = "husky_fr3", 64
    rd0 = make_moma(robot, cuda)
    q, qd, xt, xdt = moma_step_inputs(rd0, robot, 17, B, cuda)
    rd = make_moma(robot, cuda)
    rd.set_obstacles(OB.HUSKY_TYPES, OB.HUSKY_PARAMS, OB.HUSKY_LINKS)
    pm, om, spec, g0 = OB.twin(robot, OB.HUSKY_TYPES, OB.HUSKY_PARAMS, OB.HUSKY_LINKS)
    assert (rd.model.n_geoms, rd.model.n_pairs) == (om.ngeom, om.npairs) == (41, 288 + 2 * 25)
    poses = OB.husky_scene(51, q, spec["joint_index"][0])
    ref = OB.oracle_distance(om, g0, OB.HUSKY_TYPES, q, poses)
    p0, nw = len(pm.pairs), 25
    box, wall = (ref[2] >= p0) & (ref[2] < p0 + nw), ref[2] >= p0 + nw
    assert box.sum() >= 8 and wall.sum() >= 8, (box.sum(), wall.sum())
    pose_fm = OB.to_field_major(poses)
    st = _stages(rd, q, qd, xt, xdt, LINK[robot], pose_fm)
    _assert_distance_stage(om, g0, OB.HUSKY_TYPES, q, poses, st, ref)
    ctrl = mobile_manipulator.RobotController(0.001, rd, solver_mode="exact")
    out, status, _ = _solve(ctrl, q, qd, xt, xdt, LINK[robot], pose_fm)
    par = O.default_params(1, exact=True)
    par.mode = 1
    ref_d, rstat_d, _ = O.qpik_batch_dist(om, par, q, qd, xt, xdt, st["dist"], nthreads=8)
    err_d = np.abs(out - ref_d).max(axis=0)
    rstat = np.zeros_like(status)
    ref_e = np.zeros_like(out)
    for b in range(B):
        OB.set_poses(om, g0, OB.HUSKY_TYPES, poses[b])
        rstat[b], ref_e[:, b], _ = O.qpik_one(om, par, q[:, b], qd[:, b], xt[:, b], xdt[:, b])
    err = np.abs(out - ref_e).max(axis=0)
    print("Husky-FR3: q-dot* on the device's distance stage max %.3e; end to end median %.3e max %.3e; "
          "primal infeasible %d" % (err_d.max(), np.median(err), err.max(), (status == O.PRIMAL_INFEASIBLE).sum()))
    np.testing.assert_array_equal(status, rstat_d)
    np.testing.assert_array_equal(status, rstat)   # PrimalInfeasible included
    assert err_d.max() <= 1e-6, (err_d.max(), int(err_d.argmax()))
    assert np.median(err) <= 1e-9 and err.max() <= 1e-4, (np.median(err), err.max(), int(err.argmax()))
    assert np.all(out[:, status != 1] == 0.0)


# ---------------------------------------------------------------- 6. rollout
@pytest.mark.parametrize("per_step", [False, True])
def test_fr3_rollout_equals_single_steps(cuda, per_step):
    S = _fr3(cuda)
    B, steps, dt = 32, 8, 0.001
    q, qd, xt, xdt = (np.ascontiguousarray(S[k][:, :B]) for k in ("q", "qd", "xt", "xdt"))
    link = LINK["fr3"]
    pose0 = np.ascontiguousarray(S["pose_fm"][:, :, :B])
    if per_step:   # every obstacle drifts 5 mm per step along x
        pose = np.stack([pose0] * steps)
        pose[:, :, 9, :] += 0.005 * np.arange(steps)[:, None, None]
    else:
        pose = pose0
    res = S["ctrl"].QPIK_rollout_batch(q, qd, xt, xdt, link, steps, dt=dt, want=("qdot_traj", "q_traj", "dist_traj"),
                                       obstacle_pose=pose)
    _sync()
    qk, vk = q.copy(), qd.copy()
    for k in range(steps):
        pk = pose[k] if per_step else pose
        eta, status, _ = _solve(S["ctrl"], qk, vk, xt, xdt, link, np.ascontiguousarray(pk))
        st = _stages(S["rd"], qk, vk, xt, xdt, link, np.ascontiguousarray(pk))
        np.testing.assert_array_equal(res.qdot_traj[k].cpu().numpy(), eta, err_msg="qdot_traj %d" % k)
        np.testing.assert_array_equal(res.status_traj[k].cpu().numpy(), status, err_msg="status_traj %d" % k)
        np.testing.assert_array_equal(res.dist_traj[k].cpu().numpy(), st["dist"], err_msg="dist_traj %d" % k)
        vk = eta
        qk = qk + dt * vk
        np.testing.assert_array_equal(res.q_traj[k].cpu().numpy(), qk, err_msg="q_traj %d" % k)
    np.testing.assert_array_equal(res.q_final.cpu().numpy(), qk)
    np.testing.assert_array_equal(res.qdot_final.cpu().numpy(), vk)


# ---------------------------------------------------------------- 7. errors
def _rc(fn, *args):
    rc = fn(*args)
    msg = _capi.lib().drc_last_error().decode()
    return rc, msg


def test_error_codes(cuda, tmp_path):
    import torch
    S = _fr3(cuda)
    lib = _capi.lib()
    rd = make_manipulator("fr3", cuda)
    h = rd.model.handle
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)

    def set_obst(types, params, links=()):
        n = len(types)
        prm = np.ascontiguousarray(params, dtype=np.float64).reshape(-1)
        names = [s.encode() for s in links]
        return _rc(lib.drc_model_set_obstacles, h, C.c_int(n), (C.c_int * max(n, 1))(*types),
                   prm.ctypes.data_as(dp), (C.c_char_p * max(len(names), 1))(*names) if names else None,
                   C.c_int(len(names)))

    def expect(res, code):
        rc, msg = res
        assert rc == code and msg, (rc, code, msg)

    one = [[0.1, 0.1, 0.1]]
    expect(set_obst([3], one), _capi.DRC_ERR_UNSUPPORTED)                       # mesh obstacle
    expect(set_obst([0], one, ["no_such_link"]), _capi.DRC_ERR_UNKNOWN_LINK)
    expect(set_obst([0] * 30, one * 30), _capi.DRC_ERR_UNSUPPORTED)             # 65 geometries
    expect(set_obst([0] * 29, one * 29), _capi.DRC_ERR_UNSUPPORTED)             # 180 + 29 * 31 pairs > 1024
    rd.model._read_info()
    assert (rd.model.n_geoms, rd.model.n_pairs) == (35, 180)   # the refusals left the model alone
    B = 8
    q, qd, xt, xdt = (_batch.as_device(np.ascontiguousarray(S[k][:, :B]), cuda) for k in ("q", "qd", "xt", "xdt"))
    pose = _batch.as_device(np.ascontiguousarray(S["pose_fm"][:, :, :B]), cuda)
    out = torch.zeros((8, B), dtype=torch.float64, device=cuda)   # (room for any one output of the refused calls)
    status = torch.zeros(B, dtype=torch.int32, device=cuda)
    p = manipulator.QPIKParamsBuilder(rd.model, exact=True).params(LINK["fr3"], _capi.MODE_QPIK_STEP)
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    stream = C.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)
    plain = (h, C.byref(p), C.c_int64(B), ptr(q), ptr(qd), ptr(xt), ptr(xdt), None, None)
    # an obstacle entry on a model without slots
    expect(_rc(lib.drc_qpik_obstacles_batch, *plain, ptr(pose), C.c_int64(B), ptr(out), ptr(status), None, stream),
           _capi.DRC_ERR_INVALID_ARGUMENT)
    expect(_rc(lib.drc_qpik_stages_obstacles_batch, *plain, ptr(pose), C.c_int64(B), None, None, None, ptr(out), None,
               None, stream), _capi.DRC_ERR_INVALID_ARGUMENT)
    rd.set_obstacles(OB.FOUR_TYPES, OB.FOUR_PARAMS, OB.FR3_ARM_LINKS)
    # the plain entries on a model with slots: the message names the obstacle entry
    rc, msg = _rc(lib.drc_qpik_batch, *plain, ptr(out), ptr(status), None, stream)
    assert rc == _capi.DRC_ERR_INVALID_ARGUMENT and "drc_qpik_obstacles_batch" in msg, (rc, msg)
    rc, msg = _rc(lib.drc_qpik_stages_batch, *plain, None, None, None, ptr(out), None, None, stream)
    assert rc == _capi.DRC_ERR_INVALID_ARGUMENT and "drc_qpik_stages_obstacles_batch" in msg, (rc, msg)
    st_traj = torch.zeros((2, B), dtype=torch.int32, device=cuda)
    qf, vf = torch.zeros((7, B), dtype=torch.float64, device=cuda), torch.zeros((7, B), dtype=torch.float64, device=cuda)
    roll = (h, C.byref(p), C.c_int64(B), C.c_int(2), C.c_double(0.001), ptr(q), ptr(qd), ptr(xt), ptr(xdt), None, None,
            C.c_int(0))
    tail = (ptr(qf), ptr(vf), None, ptr(st_traj), None, None, None, None, stream)
    rc, msg = _rc(lib.drc_qpik_rollout_batch, *roll, *tail)
    assert rc == _capi.DRC_ERR_INVALID_ARGUMENT and "drc_qpik_rollout_obstacles_batch" in msg, (rc, msg)
    # bad pose arguments
    expect(_rc(lib.drc_qpik_obstacles_batch, *plain, None, C.c_int64(B), ptr(out), ptr(status), None, stream),
           _capi.DRC_ERR_INVALID_ARGUMENT)
    expect(_rc(lib.drc_qpik_obstacles_batch, *plain, ptr(pose), C.c_int64(B - 1), ptr(out), ptr(status), None, stream),
           _capi.DRC_ERR_INVALID_ARGUMENT)
    expect(_rc(lib.drc_qpik_rollout_obstacles_batch, *roll, ptr(pose), C.c_int64(B), C.c_int(2), *tail),
           _capi.DRC_ERR_INVALID_ARGUMENT)
    # entries whose task-stage builds take no obstacles
    unsupported = _capi.DRC_ERR_UNSUPPORTED
    expect(_rc(lib.drc_qpid_batch, *plain, ptr(out), ptr(out), ptr(status), None, stream), unsupported)
    expect(_rc(lib.drc_qpid_stages_batch, *plain, None, None, None, ptr(out), None, None, None, None, None, stream),
           unsupported)
    expect(_rc(lib.drc_clik_batch, *plain, None, ptr(out), stream), unsupported)
    expect(_rc(lib.drc_osf_batch, *plain, None, ptr(out), stream), unsupported)
    expect(_rc(lib.drc_joint_torque_step_batch, h, C.c_int64(B), ptr(q), ptr(qd), ptr(q), ptr(qd), None,
               C.c_double(0.001), None, None, ptr(out), stream), unsupported)
    expect(_rc(lib.drc_debug_lane_stage, h, C.c_int(1)), unsupported)
    # the model reports its slots
    t, n, res, prm = C.c_int(-1), C.c_int(-1), C.c_double(-1), (C.c_double * 3)()
    for i, (ty, pr_) in enumerate(zip(OB.FOUR_TYPES, OB.FOUR_PARAMS)):
        _capi.check(lib.drc_model_geom_info(h, C.c_int(35 + i), C.byref(t), prm, C.byref(n), C.byref(res)))
        assert (t.value, n.value, res.value) == (ty, 0, 0.0) and list(prm) == [float(x) for x in pr_]
    # a model with hulls takes no obstacles
    (tmp_path / "tet.obj").write_text("v 0 0 0\nv 0.1 0 0\nv 0 0.1 0\nv 0 0 0.1\nf 1 2 3\n")
    urdf = tmp_path / "hull.urdf"
    urdf.write_text('<robot name="hull"><link name="base"/>'
                    '<link name="arm"><collision><geometry><mesh filename="tet.obj"/></geometry></collision></link>'
                    '<joint name="j1" type="revolute"><parent link="base"/><child link="arm"/><axis xyz="0 0 1"/>'
                    '<limit lower="-1" upper="1" velocity="1" effort="1"/></joint></robot>')
    hull = manipulator.RobotData(str(urdf), "", device=cuda)
    with pytest.raises(_capi.DrcError) as e:
        hull.set_obstacles([0], one)
    assert e.value.code == unsupported
    _sync()
