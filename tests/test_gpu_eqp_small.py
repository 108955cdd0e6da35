"""The polish's small EQP (csrc/qp_solver.hpp: eqp_small + polish_pass_small,
reduced KKTs of N <= kEqpSmallCap = 4 rows) against the general register EQP
on identical inputs, through drc_debug_eqp_small_cap: FR3 and UR5e QPIKStep,
exact mode, stress-tier inputs, B = 512 (every N from 0 to 8 occurs).

The two paths solve the same system with another rounding (LDL^T instead of
Gauss-Jordan, P x and G^T y summed once for the multipliers and the
residuals), so they are not bit-identical: the contract is identical status,
q-dot within the stage-fed parity tolerance of tests/_common.py (1e-6) on
every instance, and identical ADMM iteration counts on at least 99 % of the
instances (a certification that sits at the eps_exact threshold may tip).
The fused kernel and the two-kernel pipeline inline the same device functions
and stay bit-identical to each other on the small path."""
import ctypes as C

import numpy as np
import pytest

from _common import LINK, assert_qpik_parity, make_manipulator, step_inputs
from dyros_robot_controller_amd import _capi, manipulator

pytestmark = pytest.mark.gpu

CAPS = (0, 1, 2, 3, 4, 8, -1)  # 8 and -1 resolve to the largest compiled tier
B = 512
_cache = {}


def _solve(ctrl, rd, robot, cap, fused, q, qd, xt, xdt):
    import torch
    lib = _capi.lib()
    _capi.check(lib.drc_debug_eqp_small_cap(rd.model.handle, C.c_int(cap)))
    _capi.check(lib.drc_set_fusion(rd.model.handle, C.c_int(fused)))
    try:
        it = torch.zeros(q.shape[1], dtype=torch.int32, device=torch.device("cuda", 0))
        out, st = ctrl.QPIK_step_batch(q, qd, xt, xdt, LINK[robot], iters=it)
        torch.cuda.synchronize()
        return out.cpu().numpy(), st.cpu().numpy(), it.cpu().numpy()
    finally:
        _capi.check(lib.drc_debug_eqp_small_cap(rd.model.handle, C.c_int(-1)))
        _capi.check(lib.drc_set_fusion(rd.model.handle, C.c_int(1)))


def _batch(cuda, robot):
    """Inputs and the result at every cap, computed once per robot."""
    if robot not in _cache:
        rd = make_manipulator(robot, cuda)
        ctrl = manipulator.RobotController(0.001, rd, solver_mode="exact")
        inp = step_inputs(rd, robot, 2, B, cuda, stress=True)
        res = {cap: _solve(ctrl, rd, robot, cap, 1, *inp) for cap in CAPS}
        _cache[robot] = (rd, ctrl, inp, res)
    return _cache[robot]


@pytest.mark.parametrize("robot", ["fr3", "ur5e"])
def test_small_path_matches_oracle(cuda, robot):
    rd, _, inp, res = _batch(cuda, robot)
    out, status, _ = res[-1]
    assert_qpik_parity(robot, rd.model, *inp, out, status, 0)


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("robot", ["fr3", "ur5e"])
def test_cap_matches_general_path(cuda, robot, cap):
    _, _, _, res = _batch(cuda, robot)
    (o0, s0, i0), (o, s, i) = res[0], res[cap]
    dq = np.abs(o - o0).max(axis=0)
    differ = np.nonzero(i != i0)[0]
    print("%s cap %d: max |dq| %.3e, iteration counts differ on %d of %d instances %s"
          % (robot, cap, dq.max(), differ.size, B, differ[:8].tolist()))
    np.testing.assert_array_equal(s, s0)
    assert dq.max() <= 1e-6, (dq.max(), int(np.argmax(dq)))
    assert differ.size <= B // 100, differ
    if cap == 0:  # the general path twice: deterministic
        np.testing.assert_array_equal(o, o0)
        np.testing.assert_array_equal(i, i0)


def test_caps_take_different_paths(cuda):
    """The switch does select: some q-dot changes in its last bits between the
    general path and the compiled tiers, and caps beyond the largest tier are
    that tier (bit-identical)."""
    _, _, _, res = _batch(cuda, "fr3")
    assert np.any(res[-1][0] != res[0][0])
    for k in (4, 8):
        np.testing.assert_array_equal(res[k][0], res[-1][0])
        np.testing.assert_array_equal(res[k][2], res[-1][2])


@pytest.mark.parametrize("robot", ["fr3", "ur5e"])
@pytest.mark.parametrize("nb", [1, 65])
def test_fused_and_two_kernel_bit_identical(cuda, robot, nb):
    """One wave, and a partial second grid row: the fused kernel and the
    two-kernel pipeline on the small path, bit for bit."""
    rd, ctrl, inp, _ = _batch(cuda, robot)
    sub = tuple(a[:, :nb].copy() for a in inp)
    (o1, s1, i1), (o0, s0, i0) = (_solve(ctrl, rd, robot, -1, f, *sub) for f in (1, 0))
    np.testing.assert_array_equal(s1, s0)
    np.testing.assert_array_equal(o1, o0)
    np.testing.assert_array_equal(i1, i0)
