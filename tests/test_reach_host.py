"""The reach error and thresholds (csrc/reach.hpp) compiled with the host
compiler (tools/reach_host_test.cpp) against the formulas that
include/drc_amd.h states for drc_qpik_reach_batch, written in numpy
(tests/_reach.py):

    e_p = (dx*dx + dy*dy) + dz*dz,  d = x_target[9..11] - pose[9..11]
    e_R = sum_{i = 0..8}, from 0 upward, of (pose[i] - x_target[i])^2
    tau_p = pos_tol*pos_tol,  tau_R = 8*(s*s),  s = sin(0.5*rot_tol)

Bit-equal: every product and every sum is rounded once in the same order on
both sides (contraction off), and the sine is libm's on both sides.  1 000
random pose pairs, from far apart down to a few ulp apart, where the verdict
against the thresholds flips."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import _obstacles as OB
import _reach as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.environ.get("CXX", "g++")
N = 1000
TOLS = [(1e-4, 1e-3), (1e-3, 1e-2), (0.05, 0.3), (1e-6, 3.0), (2.5, 1e-7)]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    assert shutil.which(CXX), "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("reach") / "reach_host")
    subprocess.check_call([CXX, "-O2", "-std=c++17", "-ffp-contract=off",
                           os.path.join(ROOT, "tools", "reach_host_test.cpp"), "-o", exe])
    return exe


def run(exe, lines):
    res = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True)
    return [[float(x) for x in ln.split()] for ln in res.stdout.strip().splitlines()]


def pose_pairs():
    """[12][N] poses and targets: random rotations and positions; the target is
    the pose moved by 10^-u metres and turned by 10^-w radians, u, w uniform in
    0 .. 9, so that the pairs straddle the thresholds of 1e-4 m / 1e-3 rad."""
    rng = np.random.default_rng(7)
    R = OB.random_rotations(rng, N)
    p = rng.uniform(-2, 2, size=(N, 3))
    axis = rng.normal(size=(N, 3))
    axis /= np.linalg.norm(axis, axis=1)[:, None]
    ang = 10.0 ** -rng.uniform(0, 9, N)
    K = np.zeros((N, 3, 3))
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0] = -axis[:, 2], axis[:, 1], axis[:, 2]
    K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -axis[:, 0], -axis[:, 1], axis[:, 0]
    E = np.eye(3) + np.sin(ang)[:, None, None] * K + (1 - np.cos(ang))[:, None, None] * (K @ K)
    step = rng.normal(size=(N, 3))
    step *= (10.0 ** -rng.uniform(0, 9, N) / np.linalg.norm(step, axis=1))[:, None]
    return OB.pack_poses(R, p).T.copy(), OB.pack_poses(E @ R, p + step).T.copy()


def test_error_is_bit_equal_to_numpy(harness):
    pose, target = pose_pairs()
    tau = RC.thresholds(1e-4, 1e-3)
    lines = ["t %.17g %.17g" % (1e-4, 1e-3)]
    for b in range(N):
        lines.append("e " + " ".join("%.17g" % v for v in np.r_[pose[:, b], target[:, b]]))
    rows = np.array(run(harness, lines)[1:])
    assert rows.shape == (N, 3)
    e_p, e_r = RC.reach_error(pose, target)
    np.testing.assert_array_equal(rows[:, 0], e_p)
    np.testing.assert_array_equal(rows[:, 1], e_r)
    within = (e_p <= tau[0]) & (e_r <= tau[1])
    np.testing.assert_array_equal(rows[:, 2], within.astype(float))
    # the set exercises both verdicts and both reasons for the negative one
    assert within.sum() >= 50 and ((e_p > tau[0]) & (e_r <= tau[1])).sum() >= 50
    assert ((e_p <= tau[0]) & (e_r > tau[1])).sum() >= 50


def test_identical_poses_and_nan(harness):
    pose, _ = pose_pairs()
    lines = ["t 1e-4 1e-3", "e " + " ".join("%.17g" % v for v in np.r_[pose[:, 0], pose[:, 0]])]
    bad = pose[:, 1].copy()
    bad[10] = np.nan
    lines.append("e " + " ".join("%.17g" % v for v in np.r_[bad, pose[:, 1]]))
    bad = pose[:, 2].copy()
    bad[4] = np.nan
    lines.append("e " + " ".join("%.17g" % v for v in np.r_[bad, pose[:, 2]]))
    rows = run(harness, lines)
    assert rows[1] == [0.0, 0.0, 1.0]
    assert np.isnan(rows[2][0]) and rows[2][1] == 0.0 and rows[2][2] == 0.0   # a NaN fails the comparison
    assert rows[3][0] == 0.0 and np.isnan(rows[3][1]) and rows[3][2] == 0.0


@pytest.mark.parametrize("pos_tol,rot_tol", TOLS)
def test_thresholds(harness, pos_tol, rot_tol):
    (tp, tr), = run(harness, ["t %.17g %.17g" % (pos_tol, rot_tol)])
    assert (tp, tr) == RC.thresholds(pos_tol, rot_tol)
    assert tp == pos_tol * pos_tol
    s = np.sin(0.5 * rot_tol)
    assert tr == 8.0 * (s * s)
    # tau_R is the e_R of a turn by exactly rot_tol: 8 sin^2(rot_tol / 2) = 4 (1 - cos rot_tol)
    assert abs(tr - 4 * (1 - np.cos(rot_tol))) <= 1e-15 + 1e-9 * tr


def test_library_thresholds_are_the_same_numbers():
    """drc_reach_thresholds (host only: no device is touched)."""
    import ctypes as C

    from dyros_robot_controller_amd import _batch, _capi
    for pos_tol, rot_tol in TOLS:
        assert _batch.reach_thresholds(pos_tol, rot_tol) == RC.thresholds(pos_tol, rot_tol)
    out = (C.c_double * 2)()
    bad = _capi.DRC_ERR_INVALID_ARGUMENT
    for pos_tol, rot_tol in ((0.0, 1e-3), (-1e-4, 1e-3), (1e-4, 0.0), (float("nan"), 1e-3), (1e-4, float("inf"))):
        assert _capi.lib().drc_reach_thresholds(C.c_double(pos_tol), C.c_double(rot_tol), out) == bad
    assert _capi.lib().drc_reach_thresholds(C.c_double(1e-4), C.c_double(1e-3), None) == bad
