"""Collision meshes through the public API on the GPU: URDFs whose <collision>
geometry is a <mesh> (written into tmp_path by the tests) against their
primitive twins and against a scipy restatement of the hull distance.

Tolerances are the existing ones: the distance stage's 1e-9 separated / 1e-6
penetrating and 1e-6 on its gradient (tests/_common.py narrow_phase_close,
tests/test_gpu_golden.py), q-dot* end to end median 1e-9 / every instance
1e-4, and 1e-6 against the exact optimum of the QP built on the device's own
stage data (tests/_common.py qp_from_stages)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
from scipy.spatial import ConvexHull

import oracle as O
from _common import LINK, moma_kinematic_param, moma_step_inputs, qp_from_stages, stage_pose, stage_step, step_inputs
from _mesh_io import all_mesh_fr3, box_triangles, point_hull_distance, write_obj, write_stl_ascii
from dyros_robot_controller_amd import _capi, manipulator, mobile_manipulator, robot_path

pytestmark = pytest.mark.gpu

BOX_RE = re.compile(r'<box size="([^"]+)"/>')


def _box_as_mesh_urdf(tmp_path, robot, uri, which=0):
    """The robot's URDF with its `which`-th box primitive as a 12-triangle STL
    of the same size, referenced by `uri` (package:// or relative)."""
    text = open(robot_path(robot)).read()
    m = list(BOX_RE.finditer(text))[which]
    size = np.array([float(x) for x in m.group(1).split()])
    (tmp_path / "pkg" / "meshes").mkdir(parents=True, exist_ok=True)
    # (ASCII: a binary STL's floats would round the half extents by ~1e-9, more than the distance tolerance)
    write_stl_ascii(tmp_path / "pkg" / "meshes" / "box.stl", box_triangles(0.5 * size).reshape(-1, 3))
    (tmp_path / "pkg" / "urdf").mkdir(exist_ok=True)
    urdf = tmp_path / "pkg" / "urdf" / (robot + "_mesh.urdf")
    urdf.write_text(text[:m.start()] + '<mesh filename="%s"/>' % uri + text[m.end():])
    return str(urdf), 0.5 * size


def _geom_info(model, g):
    t, n, res, prm = C.c_int(-1), C.c_int(-1), C.c_double(-1), (C.c_double * 3)()
    _capi.check(_capi.lib().drc_model_geom_info(model.handle, C.c_int(g), C.byref(t), prm, C.byref(n), C.byref(res)))
    return t.value, np.array(prm[:]), n.value, res.value


def _dist_close(d, ref):
    return np.abs(d - ref) <= np.where(ref > 0, 1e-9, 1e-6)


@pytest.fixture(scope="module")
def fr3_primitive(cuda):
    """The primitive FR3, 256 stress-tier workload instances plus states where
    one of the box's pairs is the closest, and its results."""
    rd = manipulator.RobotData(robot_path("fr3"), robot_path("fr3", "srdf"), device=cuda)
    _, om, _ = O.load("fr3")
    box = [g for g in range(om.ngeom) if om.gtype[g] == 2]
    assert len(box) == 1
    box_pairs = [p for p in range(om.npairs) if box[0] in (om.pair_a[p], om.pair_b[p])]
    q, qd, xt, xdt = step_inputs(rd, "fr3", 41, 256, cuda, stress=True)
    # targeted states: of 8 192 more draws, up to 64 whose closest pair is one of the box's
    q2, qd2, xt2, xdt2 = step_inputs(rd, "fr3", 42, 8192, cuda)
    s2 = stage_step(rd.model, cuda, q2, qd2, xt2, xdt2, LINK["fr3"])
    pick = np.flatnonzero(np.isin(s2["pair"], box_pairs))[:64]
    q, qd, xt, xdt = (np.ascontiguousarray(np.hstack([a, b[:, pick]])) for a, b in
                      ((q, q2), (qd, qd2), (xt, xt2), (xdt, xdt2)))
    st = stage_step(rd.model, cuda, q, qd, xt, xdt, LINK["fr3"])
    ctrl = manipulator.RobotController(0.001, rd, solver_mode="exact")
    out, status = ctrl.QPIK_step_batch(q, qd, xt, xdt, LINK["fr3"])
    return dict(rd=rd, box=box[0], box_pairs=box_pairs, q=q, qd=qd, xt=xt, xdt=xdt, st=st,
                out=out.cpu().numpy(), status=status.cpu().numpy())


@pytest.mark.parametrize("variant", ["package", "relative"])
def test_fr3_box_as_mesh_matches_primitive(cuda, tmp_path, fr3_primitive, variant):
    """Measured on an MI355X: the box's pairs win 69 of the 320 instances (56 separated, 13 penetrating); against
    the primitive twin max |d dist| 8.3e-17, max |d grad| 2.8e-16, max |d q-dot*| 1.1e-13."""
    P = fr3_primitive
    uri = "package://pkg/meshes/box.stl" if variant == "package" else "../meshes/box.stl"
    urdf, half = _box_as_mesh_urdf(tmp_path, "fr3", uri)
    rd = manipulator.RobotData(urdf, robot_path("fr3", "srdf"), str(tmp_path) if variant == "package" else "",
                               device=cuda)
    assert (rd.model.n_geoms, rd.model.n_pairs) == (P["rd"].model.n_geoms, P["rd"].model.n_pairs)
    for g in range(rd.model.n_geoms):
        t, prm, n, res = _geom_info(rd.model, g)
        tp, prmp, np_, _ = _geom_info(P["rd"].model, g)
        if g == P["box"]:
            assert (t, n, res) == (3, 8, 0.0) and (tp, np_) == (2, 0)
            np.testing.assert_allclose(prm, half, rtol=0, atol=1e-15)
        else:
            assert (t, n, res) == (tp, 0, 0.0)
            np.testing.assert_array_equal(prm, prmp)
    q, qd, xt, xdt = P["q"], P["qd"], P["xt"], P["xdt"]
    st = stage_step(rd.model, cuda, q, qd, xt, xdt, LINK["fr3"])
    ref = P["st"]
    wins = np.isin(ref["pair"], P["box_pairs"])
    assert wins.sum() >= 5, wins.sum()  # the hull path decides these instances
    dd = np.abs(st["dist"][0] - ref["dist"][0])
    dg = np.abs(st["dist"][1:] - ref["dist"][1:]).max(axis=0)
    same = st["pair"] == ref["pair"]
    print("box pairs win %d of %d; max |d dist| %.3e (box %.3e), max |d grad| %.3e (box %.3e), pair differs in %d" %
          (wins.sum(), len(wins), dd.max(), dd[wins].max(), dg.max(), dg[wins].max(), (~same).sum()))
    sepw, penw = wins & (ref["dist"][0] > 0), wins & (ref["dist"][0] <= 0)
    print("box pairs win: separated %d, |d dist| > 1e-9 in %d (max %.3e), |d grad| > 1e-6 in %d (max %.3e); "
          "penetrating %d, max |d dist| %.3e, |d grad| > 1e-6 in %d (max %.3e)" %
          (sepw.sum(), (dd[sepw] > 1e-9).sum(), dd[sepw].max(), (dg[sepw] > 1e-6).sum(), dg[sepw].max(), penw.sum(),
           dd[penw].max() if penw.any() else 0, (dg[penw] > 1e-6).sum(), dg[penw].max() if penw.any() else 0))
    assert np.all(_dist_close(st["dist"][0], ref["dist"][0])), (dd.max(), int(np.argmax(dd)))
    # another closest pair only where two candidates tie within the tolerance (then d agrees, checked above)
    assert (~same).sum() <= 2, np.flatnonzero(~same)
    assert dg[same].max() <= 1e-6, (dg[same].max(), int(np.argmax(np.where(same, dg, 0))))
    np.testing.assert_array_equal(st["pair"][~wins & same], ref["pair"][~wins & same])
    ctrl = manipulator.RobotController(0.001, rd, solver_mode="exact")
    out, status = ctrl.QPIK_step_batch(q, qd, xt, xdt, LINK["fr3"])
    out, status = out.cpu().numpy(), status.cpu().numpy()
    np.testing.assert_array_equal(status, P["status"])
    err = np.abs(out - P["out"]).max(axis=0)
    print("q-dot*: median |d| %.3e, max %.3e" % (np.median(err), err.max()))
    assert np.median(err) <= 1e-9 and err.max() <= 1e-4, (np.median(err), err.max())
    assert np.all(out[:, status != 1] == 0.0)


def test_fr3_box_as_mesh_fused_and_qpid(cuda, tmp_path, fr3_primitive):
    """drc_set_fusion on and off return the same bits, and one QPID call
    equals the primitive twin's within the QPIK tolerances."""
    import torch
    P = fr3_primitive
    urdf, _ = _box_as_mesh_urdf(tmp_path, "fr3", "package://pkg/meshes/box.stl")
    rd = manipulator.RobotData(urdf, robot_path("fr3", "srdf"), str(tmp_path), device=cuda)
    ctrl = manipulator.RobotController(0.001, rd, solver_mode="exact")
    q, qd, xt, xdt = (np.ascontiguousarray(P[k][:, -64:]) for k in ("q", "qd", "xt", "xdt"))
    res = []
    for fused in (1, 0):
        _capi.check(_capi.lib().drc_set_fusion(rd.model.handle, C.c_int(fused)))
        out, status = ctrl.QPIK_step_batch(q, qd, xt, xdt, LINK["fr3"])
        torch.cuda.synchronize()
        res.append((out.cpu().numpy(), status.cpu().numpy()))
    _capi.check(_capi.lib().drc_set_fusion(rd.model.handle, C.c_int(1)))
    np.testing.assert_array_equal(res[0][0], res[1][0])
    np.testing.assert_array_equal(res[0][1], res[1][1])
    np.testing.assert_array_equal(res[0][1], P["status"][-64:])
    assert np.abs(res[0][0] - P["out"][:, -64:]).max() <= 1e-4
    # the lane-per-instance debug stage is not extended to hulls: refused
    assert _capi.lib().drc_debug_lane_stage(rd.model.handle, C.c_int(1)) == _capi.DRC_ERR_UNSUPPORTED
    assert "mesh" in _capi.lib().drc_last_error().decode()
    both = []
    for r in (rd, P["rd"]):
        c = manipulator.RobotController(0.001, r, solver_mode="exact")
        both.append([v.cpu().numpy() for v in c.QPID_step_batch(q, qd, xt, xdt, LINK["fr3"])])
    np.testing.assert_array_equal(both[0][2], both[1][2])
    e = np.maximum(*(np.abs(both[0][k] - both[1][k]).max(axis=0) for k in (0, 1)))
    print("QPID: median |d| %.3e, max %.3e" % (np.median(e), e.max()))
    assert np.median(e) <= 1e-9 and e.max() <= 1e-4 * max(1.0, np.abs(both[1][1]).max())


def test_fr3_box_as_mesh_qpid_stage(cuda, tmp_path, fr3_primitive):
    """The QPID stage's hull build at three states whose closest pair is one of
    the hull's: its distance row equals the QPIK stage's bit for bit
    (tests/test_gpu_qpid.py holds that for the primitives) and the oracle's on
    the primitive twin within the distance tolerances above.  A QPID stage
    without the hull narrow phase forms another row at these states."""
    from dyros_robot_controller_amd import _batch
    P = fr3_primitive
    urdf, _ = _box_as_mesh_urdf(tmp_path, "fr3", "package://pkg/meshes/box.stl")
    rd = manipulator.RobotData(urdf, robot_path("fr3", "srdf"), str(tmp_path), device=cuda)
    ctrl = manipulator.RobotController(0.001, rd, solver_mode="exact")
    q, qd, xt, xdt = (np.ascontiguousarray(P[k][:, -3:]) for k in ("q", "qd", "xt", "xdt"))
    p = ctrl._pbd.params(LINK["fr3"], _capi.MODE_QPID_STEP, ctrl.Kp_task_, ctrl.Kv_task_)
    a = lambda v: _batch.as_device(v, cuda)
    st = {k: v.cpu().numpy() for k, v in _batch.qpid_stages_batch(rd.model, p, a(q), a(qd), a(xt), a(xdt)).items()}
    ik = {k: v.cpu().numpy() for k, v in _batch.stages_batch(rd.model, p, a(q), a(qd), a(xt), a(xdt)).items()}
    assert np.isin(st["pair"], P["box_pairs"]).all()   # the hull decides the distance row
    for k in ("pose", "jac", "man", "dist", "pair"):
        np.testing.assert_array_equal(st[k], ik[k], err_msg=k)
    _, om, _ = O.load("fr3")
    for b in range(3):
        d, dg, pr = O.min_distance(om, q[:, b])
        print("instance %d: pair %d (oracle %d), d %.6f, |d - oracle| %.3e, max |grad - oracle| %.3e" %
              (b, st["pair"][b], pr, d, abs(st["dist"][0, b] - d), np.abs(st["dist"][1:, b] - dg).max()))
        assert _dist_close(st["dist"][0, b], d), (b, st["dist"][0, b], d)


def test_husky_fr3_chassis_as_mesh(cuda, tmp_path):
    MM = mobile_manipulator
    spec = O.ROBOTS["husky_fr3"]
    vs, ms, ws = spec["joint_index"]
    am, aw = spec["actuator_index"]
    urdf, half = _box_as_mesh_urdf(tmp_path, "husky_fr3", "package://pkg/meshes/box.stl", which=0)
    rds = [MM.RobotData(moma_kinematic_param("husky_fr3"), MM.JointIndex(vs, ms, ws), MM.ActuatorIndex(am, aw), u,
                        robot_path("husky_fr3", "srdf"), pk, device=cuda)
           for u, pk in ((urdf, str(tmp_path)), (robot_path("husky_fr3"), ""))]
    kinds = [_geom_info(rds[0].model, g)[0] for g in range(rds[0].model.n_geoms)]
    assert kinds.count(3) == 1 and _geom_info(rds[0].model, kinds.index(3))[2:] == (8, 0.0)
    q, qd, xt, xdt = moma_step_inputs(rds[1], "husky_fr3", 9, 64, cuda, stress=True)
    outs = []
    for rd in rds:
        ctrl = MM.RobotController(0.001, rd, solver_mode="exact")
        out, status = ctrl.QPIK_step_batch(q, qd, xt, xdt, LINK["husky_fr3"])
        outs.append((out.cpu().numpy(), status.cpu().numpy()))
    np.testing.assert_array_equal(outs[0][1], outs[1][1])
    err = np.abs(outs[0][0] - outs[1][0]).max(axis=0)
    print("Husky-FR3: median |d| %.3e, max %.3e, %d solved" % (np.median(err), err.max(), (outs[0][1] == 1).sum()))
    assert np.median(err) <= 1e-9 and err.max() <= 1e-4


# ---------------------------------------------------------------- all-mesh FR3
def _link_poses(model, cuda, q, link):
    import torch
    B = q.shape[1]
    if link == "fr3_link0":  # the root link: fixed to the world at the origin (no joint moves it: not a task frame)
        return np.tile(np.eye(3), (B, 1, 1)), np.zeros((B, 3))
    dq = torch.as_tensor(q, device=cuda).contiguous()
    pose = torch.zeros((12, B), dtype=torch.float64, device=cuda)
    _capi.check(_capi.lib().drc_kinematics_batch(model.handle, C.c_int(model.frame_id(link)), C.c_int64(B),
                                                 C.c_void_p(dq.data_ptr()), None, C.c_void_p(pose.data_ptr()), None,
                                                 None, C.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)))
    torch.cuda.synchronize()
    p = pose.cpu().numpy()
    return p[:9].T.reshape(B, 3, 3).transpose(0, 2, 1), p[9:].T  # (column-major R), p


def _hull_distance(PA, PB):
    diff = (PA[:, None, :] - PB[None, :, :]).reshape(-1, 3)
    h = ConvexHull(diff)
    if np.all(h.equations[:, 3] <= 0):
        return -np.min(-h.equations[:, 3])
    return point_hull_distance(np.zeros(3), diff, h.simplices)


def test_fr3_all_mesh_against_scipy(cuda, tmp_path):
    urdf, hulls, pairs = all_mesh_fr3(tmp_path)
    rd = manipulator.RobotData(urdf, robot_path("fr3", "srdf"), device=cuda)
    assert rd.model.n_geoms == len(hulls) and rd.model.n_pairs == len(pairs), (rd.model.n_pairs, len(pairs))
    for g, name in enumerate(hulls):
        assert _geom_info(rd.model, g)[2:] == (len(hulls[name]), 0.0) and len(hulls[name]) <= 64
    prim = manipulator.RobotData(robot_path("fr3"), robot_path("fr3", "srdf"), device=cuda)
    B = 64
    q, qd, xt, xdt = step_inputs(prim, "fr3", 51, B, cuda, stress=True)
    st = stage_step(rd.model, cuda, q, qd, xt, xdt, LINK["fr3"])
    world = {}
    for name, pts in hulls.items():
        R, p = _link_poses(rd.model, cuda, q, name)
        world[name] = np.einsum("bij,nj->bni", R, pts) + p[:, None, :]
    ref = np.array([min(_hull_distance(world[a][b], world[c][b]) for a, c in pairs) for b in range(B)])
    err = np.abs(st["dist"][0] - ref)
    print("all-mesh FR3: %d pairs, %d of %d penetrating, max |d - scipy| separated %.3e penetrating %.3e" %
          (len(pairs), (ref < 0).sum(), B, err[ref > 0].max(), err[ref <= 0].max() if (ref <= 0).any() else 0.0))
    assert np.all(_dist_close(st["dist"][0], ref)), (err.max(), int(np.argmax(err)))
    ctrl = manipulator.RobotController(0.001, rd, solver_mode="exact")
    out, status = ctrl.QPIK_step_batch(q, qd, xt, xdt, LINK["fr3"])
    out, status = out.cpu().numpy(), status.cpu().numpy()
    assert set(np.unique(status)) <= {1, -2, -3}, np.unique(status)  # solved, max iterations, primal infeasible
    assert np.all(out[:, status != 1] == 0.0)
    pm, _, _ = O.load("fr3")
    worst = 0.0
    for b in np.flatnonzero(status == 1):  # the exact optimum of the QP built on the device's stage data
        x = qp_from_stages(pm, q, st, b, LINK["fr3"])
        assert x is not None
        worst = max(worst, np.abs(x - out[:, b]).max())
    print("all-mesh FR3: max |q-dot* - stage-fed optimum| %.3e" % worst)
    assert worst <= 1e-6, worst


# ------------------------------------------------------ gradient consistency
_TWO_TET = """<robot name="two_tet">
  <link name="base"><collision><geometry><mesh filename="a.obj"/></geometry></collision></link>
  <link name="l1"/>
  <link name="l2"><collision><origin xyz="0.25 0 0"/><geometry><mesh filename="b.obj"/></geometry></collision></link>
  <joint name="j1" type="revolute"><parent link="base"/><child link="l1"/><origin xyz="0 0 0.1"/><axis xyz="0 0 1"/>
    <limit lower="-3" upper="3" velocity="1" effort="1"/></joint>
  <joint name="j2" type="revolute"><parent link="l1"/><child link="l2"/><origin xyz="0.2 0 0"/><axis xyz="0 1 0"/>
    <limit lower="-3" upper="3" velocity="1" effort="1"/></joint>
</robot>
"""


def test_two_tetrahedra_gradient_is_consistent(cuda, tmp_path):
    """Central difference of the device's own distance over q against its
    gradient, h = 1e-5, on separated states (d >= 0.05 by the scipy
    restatement).  Margin: the truncation error h^2/6 |d'''|.  Every point of
    link 2's tetrahedron moves on circles of radius <= L = 0.2 + 0.25 + 0.08
    (link offsets plus the tetrahedron's size), so along a joint coordinate
    r = x_B(q) - x_A has |r'|, |r''|, |r'''| <= L, and for d = |r| >= d0
    (vertex / edge features; a face feature has only the last term)
      |d'''| <= 3 L^3 / d0^2 + 3 L^2 / d0 + L  = 113 at d0 = 0.05,
    which gives 1.9e-9; 1e-10 more covers the rounding of the two distances
    (2 * 1e-16 / 2h).  Instances whose closest features change between q - h
    and q + h are excluded: without a switch the two one-sided differences differ
    by h |d''| <= h (2 L^2 / d0 + L) = 1.2e-4; twice that counts as a switch."""
    rng = np.random.default_rng(4)
    ta = rng.normal(size=(4, 3))
    ta = 0.08 * ta / np.linalg.norm(ta, axis=1)[:, None]
    tb = rng.normal(size=(4, 3))
    tb = 0.08 * tb / np.linalg.norm(tb, axis=1)[:, None]
    write_obj(tmp_path / "a.obj", ta)
    write_obj(tmp_path / "b.obj", tb)
    (tmp_path / "r.urdf").write_text(_TWO_TET)
    rd = manipulator.RobotData(str(tmp_path / "r.urdf"), "", device=cuda)
    assert rd.model.n_pairs == 1
    L, d0, h = 0.2 + 0.25 + 0.08, 0.05, 1e-5
    margin = h * h / 6 * (3 * L ** 3 / d0 ** 2 + 3 * L ** 2 / d0 + L) + 1e-10

    def rz(a):
        return np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])

    def ry(a):
        return np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])

    # (the hulls are stored about their bounding-box centres; the restatement uses the files' vertices)
    qs = []
    while len(qs) < 128:
        q = rng.uniform(-3, 3, size=2)
        R1 = rz(q[0])
        R2 = R1 @ ry(q[1])
        PB = (tb + [0.25, 0, 0]) @ R2.T + R1 @ [0.2, 0, 0] + [0, 0, 0.1]
        if _hull_distance(ta, PB) >= d0:
            qs.append(q)
    q = np.ascontiguousarray(np.array(qs).T)

    def dist(qq):
        return stage_pose(rd.model, cuda, np.ascontiguousarray(qq), np.zeros_like(qq), "l2")["dist"]

    s0 = dist(q)
    assert np.all(s0[0] >= d0 - 1e-9)
    bad = np.zeros(q.shape[1], dtype=bool)
    worst = 0.0
    for k in range(2):
        e = np.zeros((2, 1))
        e[k] = h
        dp, dm = dist(q + e)[0], dist(q - e)[0]
        cd = (dp - dm) / (2 * h)
        # one-sided differences disagree beyond the second-order term: the closest features switched
        switch = np.abs((dp - s0[0]) / h - (s0[0] - dm) / h) > 2 * h * (2 * L * L / d0 + L)
        bad |= switch
        worst = max(worst, np.abs(cd - s0[1 + k])[~switch].max())
        assert np.all(np.abs(cd - s0[1 + k])[~switch] <= margin), (np.abs(cd - s0[1 + k])[~switch].max(), margin)
    print("gradient: max |central difference - grad| %.3e (margin %.3e), %d of %d excluded" %
          (worst, margin, bad.sum(), len(bad)))
    assert bad.mean() <= 0.10, bad.mean()
