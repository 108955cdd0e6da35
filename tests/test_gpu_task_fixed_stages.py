"""Fixed-cost stages of the wave task stage (csrc/task_stage.hpp: FK from the
preloaded joint and geometry placements, the joint masks in the Jacobian and
the manipulability gradient, the per-slot pair records of the broad phase)
against the oracle, through the stage outputs of drc_qpik_stages_batch.

Tolerances are those of test_gpu_golden.py / test_gpu_many_candidates.py:
pose and J 1e-12, manipulability 1e-10 (relative to max(1, m)), its gradient
1e-8, min distance 1e-9 separated / 2e-6 penetrating (EPA).  The oracle's
getMinDistance runs every pair (not the pruned search).  The argmin pair must
be the oracle's unless the oracle's own distance of the device's pair lies
within 1e-9 of its minimum (a tie at the distance tolerance).

Synthetic models (a 5-joint tree with a prismatic joint, written to tmp_path):
at most three joints lie on the path to the task frame, so J J^T is singular
by construction and sqrt(det) is rounding noise on both sides; manipulability
and its gradient are compared on the bundled robots only.

The zero-pair model (one geometry): device and oracle both report pair -1,
the largest double as distance and a zero gradient."""
import numpy as np
import pytest

import oracle as O
from _common import LINK, make_manipulator, make_moma, moma_step_inputs, stage_pose, step_inputs
from dyros_robot_controller_amd import manipulator

pytestmark = pytest.mark.gpu

MOMA = ("husky_fr3", "xls_fr3", "caster_fr3")
B_ROBOT = 257


def check_against_oracle(om, q, st, manip=True):
    B = q.shape[1]
    nv = q.shape[0]
    worst = dict(pose=0.0, jac=0.0, man=0.0, mgrad=0.0, sep=0.0, pen=0.0)
    for b in range(B):
        pose, J = O.fk_pose(om, q[:, b])
        dev_pose = np.concatenate([st["pose"][:9, b].reshape(3, 3).T.ravel(), st["pose"][9:, b]])  # col-major R -> row-major
        worst["pose"] = max(worst["pose"], np.abs(dev_pose - pose).max())
        worst["jac"] = max(worst["jac"], np.abs(st["jac"][:, b].reshape(6, nv) - J).max())
        if manip:
            m, mg = O.manipulability(om, q[:, b])
            worst["man"] = max(worst["man"], abs(st["man"][0, b] - m) / max(1.0, m))
            worst["mgrad"] = max(worst["mgrad"], np.abs(st["man"][1:, b] - mg).max())
        if om.npairs == 0:
            continue
        d, _, pair = O.min_distance(om, q[:, b])
        e = abs(st["dist"][0, b] - d)
        worst["pen" if d < 0 else "sep"] = max(worst["pen" if d < 0 else "sep"], e)
        dp = int(st["pair"][b])
        if dp != pair:  # allowed only as a tie: the oracle's distance of the device's pair within 1e-9 of its minimum
            assert 0 <= dp < om.npairs, (b, dp)
            d2 = O.pair_distance(om, q[:, b], dp)[0]
            assert d2 - d <= 1e-9, (b, dp, pair, d2, d)
    print("worst errors:", {k: "%.2e" % v for k, v in worst.items()})
    assert worst["pose"] <= 1e-12 and worst["jac"] <= 1e-12, worst
    assert worst["man"] <= 1e-10 and worst["mgrad"] <= 1e-8, worst
    assert worst["sep"] <= 1e-9 and worst["pen"] <= 2e-6, worst


@pytest.mark.parametrize("robot", ["fr3", "ur5e", "husky_fr3", "xls_fr3", "caster_fr3"])
def test_bundled_robots(cuda, robot):
    """Chains (FR3, UR5e) and trees (the whole-body robots), stress tiers on."""
    if robot in MOMA:
        rd = make_moma(robot, cuda)
        q, qd, _, _ = moma_step_inputs(rd, robot, 31, B_ROBOT, cuda, stress=True)
    else:
        rd = make_manipulator(robot, cuda)
        q, qd, _, _ = step_inputs(rd, robot, 31, B_ROBOT, cuda, stress=True)
    st = stage_pose(rd.model, cuda, q, qd, LINK[robot])
    _, om, _ = O.load(robot)
    check_against_oracle(om, q, st)


# geometry per link of the synthetic tree: (type, size, xyz); "far" links carry
# geometry metres away from the rest
def tree_urdf(path, geoms):
    """base -j1(rev z)-> l1 -j2(rev y)-> l2 -j3(prismatic x)-> tip
                         l1 -j4(rev x)-> l4 -j5(rev y)-> l5
    l2 and l4 are both children of l1; the task frame `tip` is on the l2
    branch.  geoms: {link: [(tag, attrs, xyz), ...]}."""
    out = ['<?xml version="1.0"?>', '<robot name="tree">']
    for link in ("base", "l1", "l2", "tip", "l4", "l5"):
        out.append('  <link name="%s">' % link)
        if link != "base":
            out.append('    <inertial><origin xyz="0 0 0.05"/><mass value="1.0"/>'
                       '<inertia ixx="0.01" iyy="0.01" izz="0.01" ixy="0" ixz="0" iyz="0"/></inertial>')
        for tag, attrs, xyz in geoms.get(link, []):
            out.append('    <collision><origin xyz="%s" rpy="0.3 -0.2 0.5"/><geometry><%s %s/></geometry></collision>'
                       % (xyz, tag, attrs))
        out.append('  </link>')
    joints = [("j1", "revolute", "base", "l1", "0 0 0.1", "0 0 1"), ("j2", "revolute", "l1", "l2", "0 0.1 0.2", "0 1 0"),
              ("j3", "prismatic", "l2", "tip", "0.1 0 0.2", "1 0 0"), ("j4", "revolute", "l1", "l4", "0 -0.1 0.2", "1 0 0"),
              ("j5", "revolute", "l4", "l5", "0 0 0.25", "0 1 0")]
    for name, jt, par, child, xyz, axis in joints:
        lim = '-0.3" upper="0.3' if jt == "prismatic" else '-2.5" upper="2.5'
        out.append('  <joint name="%s" type="%s"><parent link="%s"/><child link="%s"/><origin xyz="%s" rpy="0.1 0 -0.2"/>'
                   '<axis xyz="%s"/><limit lower="%s" velocity="2.0" effort="50"/></joint>' % (name, jt, par, child, xyz, axis, lim))
    out.append('</robot>')
    with open(path, "w") as fh:
        fh.write("\n".join(out) + "\n")


SPH = lambda r, xyz: ("sphere", 'radius="%g"' % r, xyz)
CYL = lambda r, h, xyz: ("cylinder", 'radius="%g" length="%g"' % (r, h), xyz)
BOX = lambda a, b, c, xyz: ("box", 'size="%g %g %g"' % (a, b, c), xyz)
# 13 geometries: 78 pairs less the 8 within a link = 70 (a full round of 64 lanes and six more slots)
GEOMS_70 = {
    "base": [BOX(0.2, 0.2, 0.05, "0 0 0"), SPH(0.3, "4 3 0")],                       # the sphere: metres away
    "l1": [CYL(0.04, 0.2, "0 0 0.1"), SPH(0.05, "0 0 0.22"), BOX(0.06, 0.05, 0.04, "0.05 0 0.1")],
    "l2": [CYL(0.035, 0.18, "0 0 0.1"), SPH(0.045, "0.05 0 0.2")],
    "tip": [BOX(0.05, 0.04, 0.06, "0.05 0 0"), CYL(0.2, 0.5, "3 -4 2")],             # the cylinder: metres away
    "l4": [CYL(0.035, 0.2, "0 0 0.12"), BOX(0.05, 0.05, 0.05, "0 0.04 0.2")],
    "l5": [SPH(0.05, "0 0 0.1"), CYL(0.03, 0.15, "0 0 0.2")],
}
GEOMS_3 = {"l1": [CYL(0.04, 0.2, "0 0 0.1")], "tip": [BOX(0.05, 0.04, 0.06, "0.05 0 0")], "l5": [SPH(0.05, "0 0 0.1")]}
GEOMS_1 = {"l5": [SPH(0.05, "0 0 0.1")]}


@pytest.mark.parametrize("name,geoms,npairs", [("pairs70", GEOMS_70, 70), ("pairs3", GEOMS_3, 3), ("pairs0", GEOMS_1, 0)])
def test_synthetic_tree(cuda, tmp_path, name, geoms, npairs):
    """A branch, a prismatic joint, mixed sphere / cylinder / box geometry;
    70 pairs (a full round and a nearly empty one), fewer than 64, none."""
    urdf = str(tmp_path / (name + ".urdf"))
    tree_urdf(urdf, geoms)
    rd = manipulator.RobotData(urdf, "", device=cuda)
    _, om, _ = O.load_paths(urdf, None, dict(ee="tip", kind=0))
    assert rd.model.n_pairs == npairs and om.npairs == npairs and om.nv == 5
    assert sorted(om.jtype[j] for j in range(1, 6)) == [0, 0, 0, 0, 1] and om.parent[2] == om.parent[4] == 1
    B = 130
    rng = np.random.default_rng(7)
    lo = np.array([om.lower[j] for j in range(5)])
    hi = np.array([om.upper[j] for j in range(5)])
    q = lo[:, None] + (hi - lo)[:, None] * rng.uniform(0.02, 0.98, (5, B))
    st = stage_pose(rd.model, cuda, q, np.zeros((5, B)), "tip")
    check_against_oracle(om, q, st, manip=False)
    if npairs == 0:
        d, g, pair = O.min_distance(om, q[:, 0])  # no pair: the largest double, a zero gradient, pair -1
        assert pair == -1 and np.all(st["pair"] == -1)
        assert np.all(st["dist"][0] == d) and np.all(st["dist"][1:] == g[:, None])


def test_batch_edges_fr3(cuda):
    """Results do not depend on the batch size: B = 1, 65 and 1025 (one more
    than the task grid: a wave takes a second instance) against the same
    instances of a B = 2048 call, bit for bit."""
    rd = make_manipulator("fr3", cuda)
    q, qd, _, _ = step_inputs(rd, "fr3", 5, 2048, cuda, stress=True)
    ref = stage_pose(rd.model, cuda, q, qd, LINK["fr3"])
    for B in (1, 65, 1025):
        st = stage_pose(rd.model, cuda, np.ascontiguousarray(q[:, :B]), np.ascontiguousarray(qd[:, :B]), LINK["fr3"])
        for k in ("pose", "jac", "man", "dist", "pair"):
            np.testing.assert_array_equal(st[k], ref[k][..., :B], err_msg="%s at B=%d" % (k, B))
