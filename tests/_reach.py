"""Shared helpers of the reach tests (test infrastructure): the error of a pose
against the target and its thresholds in numpy, as include/drc_amd.h states
them for drc_qpik_reach_batch, and the census inputs."""
import math

import numpy as np

REACHED, BUDGET, QP_FAILED = 0, 1, 2


def reach_error(pose, target):
    """(e_p, e_R) of poses [12][...] (R column-major, then p): numpy rounds every
    product and every sum, in the order written."""
    pose, target = np.asarray(pose, dtype=np.float64), np.asarray(target, dtype=np.float64)
    dx, dy, dz = target[9] - pose[9], target[10] - pose[10], target[11] - pose[11]
    e_p = (dx * dx + dy * dy) + dz * dz
    e_r = np.zeros_like(e_p)
    for i in range(9):
        d = pose[i] - target[i]
        e_r = e_r + d * d
    return e_p, e_r


def thresholds(pos_tol, rot_tol):
    s = math.sin(0.5 * rot_tol)
    return pos_tol * pos_tol, 8.0 * (s * s)


def census_states(lo, hi, B, first=0):
    """(q0, qg) [nv][B]: instance i draws from numpy.random.default_rng(i) a
    start in the middle 40 % of the position limits (clipped to +-3) and a goal
    within 0.15 of it per joint."""
    lo, hi = np.clip(np.asarray(lo, float), -3, 3), np.clip(np.asarray(hi, float), -3, 3)
    nv = len(lo)
    q0, qg = np.zeros((nv, B)), np.zeros((nv, B))
    for i in range(B):
        r = np.random.default_rng(first + i)
        q0[:, i] = lo + (hi - lo) * (0.3 + 0.4 * r.random(nv))
        qg[:, i] = q0[:, i] + r.uniform(-0.15, 0.15, nv)
    return q0, qg
