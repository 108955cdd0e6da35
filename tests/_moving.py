"""Shared helpers of the moving-obstacle tests (test infrastructure): the
rate of the closest distance under a slot's rigid motion, from the C oracle's
witnesses on the twin of tests/_obstacles.py, and the twin's poses displaced
along a twist.

Convention (include/drc_amd.h): a twist is (v, omega) in the world frame, v the
velocity of the slot pose's origin p.  With the closest pair's witnesses pA
(robot) and pB (obstacle), n = (pB - pA) / |pB - pA| and s = +1 (d >= 0) or -1
(d < 0):  dd/dt = s n . (v + omega x (pB - p))."""
import numpy as np

import oracle as O
import _obstacles as OB


def rate_formula(d, pA, pB, origin, twist):
    n = (pB - pA) / np.linalg.norm(pB - pA)
    r = float(n @ (twist[:3] + np.cross(twist[3:], pB - origin)))
    return r if d >= 0 else -r


def rodrigues(phi):
    """exp(phi^) of a rotation vector."""
    th = np.linalg.norm(phi)
    if th == 0:
        return np.eye(3)
    u = phi / th
    K = np.array([[0, -u[2], u[1]], [u[2], 0, -u[0]], [-u[1], u[0], 0]])
    return np.eye(3) + np.sin(th) * K + 2 * np.sin(th / 2) ** 2 * (K @ K)


def displaced(pose12, twist, h):
    """[n][12] poses moved for a time h along their twists [n][6]:
    R -> exp(h omega^) R, p -> p + h v."""
    out = np.array(pose12, dtype=float)
    for i in range(out.shape[0]):
        R = out[i, :9].reshape(3, 3).T
        out[i, :9] = (rodrigues(h * twist[i, 3:]) @ R).T.reshape(-1)
        out[i, 9:] += h * twist[i, :3]
    return out


def oracle_rates(om, g0, types, q, poses, twists, pairs=None):
    """Per instance, from the oracle alone: (rate [B], scale [B], d [B], pair [B],
    obstacle [B]) with rate the formula on O.pair_distance's witnesses of the
    closest pair (``pairs``: of these pairs instead), 0 where a self pair wins;
    scale = |v| + |omega| |pB - p|, the speed bound of the witness point that
    the tolerances scale with; obstacle: the pair is an obstacle pair."""
    B = q.shape[1]
    rate, scale, dd = np.zeros(B), np.zeros(B), np.zeros(B)
    pr, ob = np.zeros(B, np.int64), np.zeros(B, bool)
    for b in range(B):
        OB.set_poses(om, g0, types, poses[b])
        dd[b], _, pr[b] = O.min_distance(om, q[:, b])
        p = int(pr[b] if pairs is None else pairs[b])
        if p < 0:
            continue
        gb = om.pair_b[p]
        if gb < g0:
            continue
        ob[b] = True
        i = gb - g0
        d, pA, pB = O.pair_distance(om, q[:, b], p)
        origin = poses[b, i, 9:12]
        rate[b] = rate_formula(d, pA, pB, origin, twists[b, i])
        scale[b] = np.linalg.norm(twists[b, i, :3]) + np.linalg.norm(twists[b, i, 3:]) * np.linalg.norm(pB - origin)
    return rate, scale, dd, pr, ob


def central_difference(om, g0, types, q, pose12, twist, h=1e-5):
    """d/dt of the oracle's min distance with the joints at rest and the slots
    moving along their twists."""
    OB.set_poses(om, g0, types, displaced(pose12, twist, h))
    dp = O.min_distance(om, q)[0]
    OB.set_poses(om, g0, types, displaced(pose12, twist, -h))
    dm = O.min_distance(om, q)[0]
    return (dp - dm) / (2 * h)


def halfspace_witness_not_unique(om, q, pair, pose12, eps=1e-9):
    """True where every point of an edge, a face or a side line of the robot
    geometry of ``pair`` is a closest point to the half-space of pose ``pose12``
    (its support set towards the plane is not a point: a box axis, the
    cylinder's axis or its cap lies in the plane's direction within eps).  The
    distance then has no derivative along a motion that tilts the plane -- the
    distances of the edge's ends split -- and dd/dt depends on which closest
    point a narrow phase reports (halfspace.hpp: the support set's centre; the
    oracle's GJK / EPA on the twin's box: some point of it), as grad d does where
    the distance is non-smooth in q.  No joint motion reveals it where the
    geometry cannot tilt against the plane: a mobile base's box, whose edges
    are vertical, against a vertical wall."""
    ga = om.pair_a[pair]
    Tj = O.joint_placement(om, q, om.gparent[ga])
    gp = np.array([om.gplace[ga][i] for i in range(12)])
    Rg = Tj[:3, :3] @ gp[:9].reshape(3, 3)
    dl = -(Rg.T @ np.asarray(pose12[:9]).reshape(3, 3).T[:, 2])
    if om.gtype[ga] == OB.BOX:
        return bool(np.any(np.abs(dl) < eps))
    if om.gtype[ga] == OB.CYLINDER:
        return bool(abs(dl[2]) < eps or np.hypot(dl[0], dl[1]) < eps)
    return False
