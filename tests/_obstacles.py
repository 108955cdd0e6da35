"""Shared helpers of the obstacle-slot tests (test infrastructure): the C
oracle's twin of a model with obstacle slots, pose generators, and the
half-space closed form in numpy.

The oracle twin.  ``oracle.OracleModel`` has room for 96 geometries; the slots
are appended to it as geometries with parent joint 0, paired like
``drc_model_set_obstacles`` pairs them (after the model's own pairs, slot by
slot, the link geometries in index order), and their pose is written into
``gplace`` per instance (the oracle's R is row-major, the API's pose
column-major).  A half-space is represented by a box of 20 m half extents whose
+z face lies in the plane, the face centre at the pose's origin."""
import numpy as np

import oracle as O
from dyros_robot_controller_amd import workload

SPHERE, CYLINDER, BOX, HALFSPACE = 0, 1, 2, 4
BIG = 20.0   # half extents of the box that stands for a half-space

# the four obstacles of the FR3 distance-stage test: a sphere r 0.08, a box
# 0.3 x 0.4 x 0.02, a cylinder r 0.05 h/2 0.25, a half-space
FOUR_TYPES = (SPHERE, BOX, CYLINDER, HALFSPACE)
FOUR_PARAMS = ((0.08, 0, 0), (0.15, 0.2, 0.01), (0.05, 0.25, 0), (0, 0, 0))
FR3_ARM_LINKS = ("fr3_link3", "fr3_link4", "fr3_link5", "fr3_link6", "fr3_link7")   # moved by joint 3 and beyond


def twin(robot, types, params, links=None):
    """(pm, om, spec, first): the oracle model of ``robot`` with the obstacle
    slots appended; ``first`` is the index of the first slot geometry."""
    pm, om, spec = O.load(robot)
    g0, p0 = om.ngeom, om.npairs
    if links is None:
        with_ = [g for g in range(g0) if om.gparent[g] > 0]
    else:
        with_ = [g for g in range(g0) if pm.geoms[g]["link"] in links]
    assert g0 + len(types) <= O.MAXG and p0 + len(types) * len(with_) <= O.MAXP
    p = p0
    for i, (t, prm) in enumerate(zip(types, params)):
        g = g0 + i
        om.gparent[g] = 0
        om.gtype[g] = BOX if t == HALFSPACE else t
        for k in range(3):
            om.gparam[g][k] = BIG if t == HALFSPACE else float(prm[k])
        for a in with_:
            om.pair_a[p], om.pair_b[p] = a, g
            p += 1
    om.ngeom, om.npairs = g0 + len(types), p
    return pm, om, spec, g0


def set_poses(om, first, types, pose12):
    """Writes one instance's slot poses (pose12 [n][12]: R column-major, p)
    into the twin's gplace."""
    for i, t in enumerate(types):
        R = np.asarray(pose12[i][:9]).reshape(3, 3).T
        p = np.asarray(pose12[i][9:12], dtype=float)
        if t == HALFSPACE:
            p = p - BIG * R[:, 2]
        row = np.concatenate([R.reshape(-1), p])
        for k in range(12):
            om.gplace[first + i][k] = row[k]


def random_rotations(rng, n):
    """n rotation matrices, uniform (normalised quaternions)."""
    qn = rng.normal(size=(n, 4))
    qn /= np.linalg.norm(qn, axis=1)[:, None]
    w, x, y, z = qn.T
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], -1),
                     np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], -1),
                     np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1)], 1)


def pack_poses(R, p):
    """R [..., 3, 3], p [..., 3] -> [..., 12] in the API's layout."""
    return np.concatenate([np.swapaxes(R, -1, -2).reshape(R.shape[:-2] + (9,)), p], axis=-1)


WORKSPACE = ((0.1, 0.8), (-0.6, 0.6), (0.0, 1.0))


def fr3_scene(seed, B, types=FOUR_TYPES, box=WORKSPACE, back=(0.2, 0.6)):
    """Per-instance poses [B][n][12]: rotations uniform, positions uniform in
    ``box``; a half-space's plane passes through such a point pushed back
    ``back`` metres along its normal."""
    rng = np.random.default_rng(seed)
    n = len(types)
    R = random_rotations(rng, B * n).reshape(B, n, 3, 3)
    lo = np.array([b[0] for b in box])
    hi = np.array([b[1] for b in box])
    p = lo + (hi - lo) * rng.uniform(size=(B, n, 3))
    s = rng.uniform(back[0], back[1], size=(B, n))
    for i, t in enumerate(types):
        if t == HALFSPACE:
            p[:, i] -= s[:, i, None] * R[:, i, :, 2]
    return pack_poses(R, p)


FR3_MOVING_LINKS = ("fr3_link1", "fr3_link2") + FR3_ARM_LINKS
PLATE = (1.3, 1.3, 0.005)   # half extents of the plates of plates_scene


def plates_scene(seed, B, n=27):
    """Per-instance poses [B][n][12] of n thin plates (boxes of half extents
    PLATE) through the arm's workspace: tilted up to ~30 degrees from the
    horizontal, centres 0.5 .. 0.9 m off the base axis, heights 0 .. 0.9 m.
    A plate's broad-phase bound (its bounding sphere about the centre, raised
    along the one axis towards the other geometry) is weak when that axis lies
    in the plate, so nearly every plate pair stays a GJK candidate, and the
    arm crosses several plates."""
    rng = np.random.default_rng(seed)
    R = np.zeros((B, n, 3, 3))
    tilt = rng.uniform(-0.5, 0.5, size=(B, n, 2))
    yaw = rng.uniform(-np.pi, np.pi, size=(B, n))
    for b in range(B):
        for i in range(n):
            cx, sx, cy, sy = np.cos(tilt[b, i, 0]), np.sin(tilt[b, i, 0]), np.cos(tilt[b, i, 1]), np.sin(tilt[b, i, 1])
            cz, sz = np.cos(yaw[b, i]), np.sin(yaw[b, i])
            Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
            Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
            Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
            R[b, i] = Rz @ Ry @ Rx
    rad, az = rng.uniform(0.5, 0.9, size=(B, n)), rng.uniform(-np.pi, np.pi, size=(B, n))
    p = np.stack([rad * np.cos(az), rad * np.sin(az), rng.uniform(0.0, 0.9, size=(B, n))], axis=-1)
    return pack_poses(R, p)


def spheres_scene(seed, B, n=29, box=WORKSPACE):
    """Per-instance poses [B][n][12] of n spheres with centres uniform in ``box``."""
    rng = np.random.default_rng(seed)
    lo = np.array([b[0] for b in box])
    hi = np.array([b[1] for b in box])
    R = np.broadcast_to(np.eye(3), (B, n, 3, 3))
    return pack_poses(R, lo + (hi - lo) * rng.uniform(size=(B, n, 3)))


HUSKY_LINKS = ("base_link",) + FR3_ARM_LINKS
HUSKY_TYPES = (BOX, HALFSPACE)
HUSKY_PARAMS = ((0.2, 0.3, 0.15), (0, 0, 0))


def husky_scene(seed, q, virtual_start=0):
    """World-frame poses [B][2][12] for the mobile manipulator at the base
    positions q[virtual_start : +2]: a randomly turned box within 1 m of the
    base, 0.2 .. 1.2 m up, and a wall (a half-space with a horizontal normal)
    whose plane stands 0.3 .. 1.5 m from the base's origin, the robot on its
    free side."""
    rng = np.random.default_rng(seed)
    B = q.shape[1]
    base = np.stack([q[virtual_start], q[virtual_start + 1], np.zeros(B)], axis=-1)
    R = random_rotations(rng, B * 2).reshape(B, 2, 3, 3)
    p = np.zeros((B, 2, 3))
    p[:, 0] = base + np.stack([rng.uniform(-1, 1, B), rng.uniform(-1, 1, B), rng.uniform(0.2, 1.2, B)], axis=-1)
    az = rng.uniform(-np.pi, np.pi, B)
    n = np.stack([np.cos(az), np.sin(az), np.zeros(B)], axis=-1)
    ez = np.broadcast_to(np.array([0.0, 0.0, 1.0]), (B, 3))
    R[:, 1] = np.stack([np.cross(ez, n), ez, n], axis=-1)   # columns (e_z x n, e_z, n): right-handed, R e_z = n
    p[:, 1] = base - rng.uniform(0.3, 1.5, B)[:, None] * n + np.array([0, 0, 0.5])
    return pack_poses(R, p)


def to_field_major(poses):
    """[B][n][12] -> the entries' [n][12][B]."""
    return np.ascontiguousarray(np.transpose(poses, (1, 2, 0)))


def fr3_states(om, seed, B):
    """The benchmark workload's joint states from the oracle model's limits."""
    nv = om.nv
    lo = np.array([om.lower[i] for i in range(nv)])
    hi = np.array([om.upper[i] for i in range(nv)])
    vmax = np.array([om.vel[i] for i in range(nv)])
    return workload.joint_states(lo, hi, vmax, seed, B)


def oracle_distance(om, first, types, q, poses):
    """The oracle's distance stage per instance: (d [B], grad [nv][B], pair [B])."""
    B = q.shape[1]
    d, g, pr = np.zeros(B), np.zeros((om.nv, B)), np.zeros(B, np.int64)
    for b in range(B):
        set_poses(om, first, types, poses[b])
        d[b], g[:, b], pr[b] = O.min_distance(om, q[:, b])
    return d, g, pr


def halfspace_closed_form(gtype, prm, Rg, c, Rp, p):
    """(d, shape witness, plane witness) of a primitive (centre c, rotation Rg)
    against the half-space {x : (x - p) . Rp e_z <= 0}."""
    n = Rp[:, 2]
    if gtype == SPHERE:
        h, loc = prm[0], -prm[0] * (Rg.T @ n)
    elif gtype == CYLINDER:
        s = float(n @ Rg[:, 2])
        h = prm[1] * abs(s) + prm[0] * np.sqrt(max(0.0, 1.0 - s * s))
        dl = -(Rg.T @ n)
        rho = np.hypot(dl[0], dl[1])
        loc = np.array([prm[0] * dl[0] / rho, prm[0] * dl[1] / rho, np.sign(dl[2]) * prm[1]])
    else:
        e = np.asarray(prm[:3], dtype=float)
        dl = -(Rg.T @ n)
        h, loc = float(e @ np.abs(dl)), np.sign(dl) * e
    d = float(n @ (c - p)) - h
    ps = Rg @ loc + c
    return d, ps, ps - float(n @ (ps - p)) * n
