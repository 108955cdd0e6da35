"""Moving obstacles on the CPU: the conventions of the obstacle twist, pinned
on the C oracle alone (no device code can influence them), and
_batch.obstacle_trajectory.

1. dd/dt = s n . (v + omega x (pB - p)) on O.pair_distance's witnesses of the
   twin (tests/_obstacles.py) against a central difference (h = 1e-5) of
   O.min_distance over the poses displaced by exp(+-h omega^) R, p +- h v.
   Tolerance 1e-6, the project's gradient tolerance (the expression is grad d's
   B-term with the slot's rigid motion for a joint's column).
2. obstacle_trajectory against scipy.linalg.expm: 1e-13 on R and p for
   |omega| k dt <= 3 (Rodrigues' formula in float64: a handful of roundings of
   O(1) values), R^T R - I <= 1e-14, the shapes, and zero twist bit for bit."""
import numpy as np
import pytest

import _moving as MV
import _obstacles as OB
from dyros_robot_controller_amd import _batch


def test_rate_formula_matches_central_difference_of_the_oracle():
    """Measured: an obstacle pair is the closest in 202 of the 256 instances (sphere 16, box 34, cylinder 15,
    half-space 137; 77 separated, 125 penetrating); max |formula - central difference| 7.6e-9, nothing excluded."""
    B = 256
    pm, om, spec, g0 = OB.twin("fr3", OB.FOUR_TYPES, OB.FOUR_PARAMS, OB.FR3_ARM_LINKS)
    q, _ = OB.fr3_states(om, 3, B)
    poses = OB.fr3_scene(11, B)
    twists = np.random.default_rng(77).uniform(-1, 1, (B, 4, 6))
    rate, scale, d, pr, ob = MV.oracle_rates(om, g0, OB.FOUR_TYPES, q, poses, twists)
    p0, nw = len(pm.pairs), (om.npairs - len(pm.pairs)) // 4
    for i, name in enumerate(("sphere", "box", "cylinder", "half-space")):
        win = (pr >= p0 + i * nw) & (pr < p0 + (i + 1) * nw)
        assert win.sum() >= 8 and (win & (d > 0)).any() and (win & (d < 0)).any(), \
            (name, win.sum(), (win & (d > 0)).sum(), (win & (d < 0)).sum())
    assert np.array_equal(ob, pr >= p0) and np.all(rate[~ob] == 0.0)
    worst = 0.0
    for b in np.flatnonzero(ob):
        fd = MV.central_difference(om, g0, OB.FOUR_TYPES, q[:, b], poses[b], twists[b])
        worst = max(worst, abs(rate[b] - fd))
        assert abs(rate[b] - fd) <= 1e-6, (int(b), rate[b], fd, int(pr[b]), d[b])
    print("obstacle pairs win %d (separated %d, penetrating %d); max |formula - central difference| %.3e"
          % (ob.sum(), (ob & (d > 0)).sum(), (ob & (d < 0)).sum(), worst))


def _expm_reference(pose0, twist, dt, steps):
    from scipy.linalg import expm
    out = np.zeros((steps,) + pose0.shape)
    for k in range(steps):
        for i in range(pose0.shape[0]):
            w = twist[i, 3:]
            E = expm(k * dt * np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]))
            out[k, i, :9] = (E @ pose0[i, :9].reshape(3, 3).T).T.reshape(-1)
            out[k, i, 9:] = pose0[i, 9:] + k * dt * twist[i, :3]
    return out


def test_obstacle_trajectory_matches_expm():
    rng = np.random.default_rng(5)
    n, steps, dt = 6, 16, 0.02
    pose0 = OB.pack_poses(OB.random_rotations(rng, n), rng.uniform(-1, 1, (n, 3)))
    twist = rng.uniform(-1, 1, (n, 6))
    twist[:, 3:] *= rng.uniform(0.01, 3.0 / ((steps - 1) * dt), (n, 1)) / np.linalg.norm(twist[:, 3:], axis=1)[:, None]
    twist[0, 3:] *= 1e-9 / np.linalg.norm(twist[0, 3:])      # a tiny rotation
    assert np.linalg.norm(twist[:, 3:], axis=1).max() * (steps - 1) * dt <= 3.0
    got = _batch.obstacle_trajectory(pose0, twist, dt, steps).numpy()
    ref = _expm_reference(pose0, twist, dt, steps)
    assert got.shape == (steps, n, 12)
    err = np.abs(got - ref).max()
    R = np.swapaxes(got[..., :9].reshape(steps, n, 3, 3), -1, -2)
    orth = np.abs(np.swapaxes(R, -1, -2) @ R - np.eye(3)).max()
    print("obstacle_trajectory: max |pose - expm| %.3e, max |R^T R - I| %.3e" % (err, orth))
    assert err <= 1e-13, err
    assert orth <= 1e-14, orth
    assert np.array_equal(got[0], pose0)     # k = 0: the start, bit for bit


def test_obstacle_trajectory_shapes_and_zero_twist():
    rng = np.random.default_rng(6)
    n, B, steps, dt = 3, 5, 4, 0.001
    pose0 = OB.pack_poses(OB.random_rotations(rng, n), rng.uniform(-1, 1, (n, 3)))
    pose0[1, 9] = -0.0                        # (a negative zero stays one)
    poseB = OB.to_field_major(OB.pack_poses(OB.random_rotations(rng, B * n).reshape(B, n, 3, 3),
                                            rng.uniform(-1, 1, (B, n, 3))))
    twist, twistB = rng.uniform(-1, 1, (n, 6)), rng.uniform(-1, 1, (n, 6, B))
    assert tuple(_batch.obstacle_trajectory(pose0, twist, dt, steps).shape) == (steps, n, 12)
    assert tuple(_batch.obstacle_trajectory(poseB, twist, dt, steps).shape) == (steps, n, 12, B)
    assert tuple(_batch.obstacle_trajectory(pose0, twistB, dt, steps).shape) == (steps, n, 12, B)
    full = _batch.obstacle_trajectory(poseB, twistB, dt, steps).numpy()
    assert full.shape == (steps, n, 12, B)
    for b in range(B):   # the [B] axis is a batch of independent trajectories
        one = _batch.obstacle_trajectory(np.ascontiguousarray(poseB[:, :, b]), np.ascontiguousarray(twistB[:, :, b]),
                                         dt, steps).numpy()
        np.testing.assert_array_equal(full[..., b], one)
    for p0, z in ((pose0, np.zeros((n, 6))), (poseB, np.zeros((n, 6, B))), (poseB, np.zeros((n, 6)))):
        still = _batch.obstacle_trajectory(p0, z, dt, steps).numpy()
        for k in range(steps):
            assert still[k].tobytes() == np.ascontiguousarray(p0).tobytes()
    with pytest.raises(ValueError):
        _batch.obstacle_trajectory(pose0[:, :11], twist, dt, steps)
