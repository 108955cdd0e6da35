"""The manipulator QP kernels' sparse G loops (csrc/qp_solver.hpp:
kQpikSparse -- schur_setup, the Schur ADMM's G-column pass, qp_scale_roles,
the polish's Jacobi guess, all following csrc/qpik_pattern.hpp) against the
same kernel built with every G loop dense (qp_dense_kernel.hip, selected by
drc_debug_qp_dense on the two-kernel pipeline), on identical inputs: FR3 and
UR5e QPIKStep, stress-tier inputs.

Only exact zeros leave the sums and the order and grouping of the remaining
terms are kept, so the contract is bit-identity of q-dot, status and ADMM
iteration counts: at B = 1 (one wave), B = 65 (a partial second grid row) and
B = 512 (every active-set size occurs), in exact mode and in osqp_default mode
(adaptive rho with refactorisation -- schur_setup at changed rho -- about 120
iterations per instance).  The fused kernel inlines the same device functions
and stays bit-identical to the sparse pipeline; the rollout, reach, path and
seeds kernels are compared with the stepwise pipeline by their own tests."""
import ctypes as C

import numpy as np
import pytest

from _common import LINK, assert_qpik_parity, make_manipulator, step_inputs
from dyros_robot_controller_amd import _capi, manipulator

pytestmark = pytest.mark.gpu

B = 512
SIZES = (1, 65, 512)
MODES = ("exact", "osqp_default")
_cache = {}


def _dense_launches(rd):
    n = C.c_int64(0)
    _capi.check(_capi.lib().drc_debug_qp_dense_launches(rd.model.handle, C.byref(n)))
    return n.value


def _solve(ctrl, rd, robot, dense, fused, q, qd, xt, xdt):
    import torch
    lib = _capi.lib()
    _capi.check(lib.drc_debug_qp_dense(rd.model.handle, C.c_int(dense)))
    _capi.check(lib.drc_set_fusion(rd.model.handle, C.c_int(fused)))
    try:
        it = torch.zeros(q.shape[1], dtype=torch.int32, device=torch.device("cuda", 0))
        out, st = ctrl.QPIK_step_batch(q, qd, xt, xdt, LINK[robot], iters=it)
        torch.cuda.synchronize()
        return out.cpu().numpy(), st.cpu().numpy(), it.cpu().numpy()
    finally:
        _capi.check(lib.drc_debug_qp_dense(rd.model.handle, C.c_int(0)))
        _capi.check(lib.drc_set_fusion(rd.model.handle, C.c_int(1)))


def _robot(cuda, robot):
    """The model, one controller per solver mode and the B = 512 inputs, once per robot."""
    if robot not in _cache:
        rd = make_manipulator(robot, cuda)
        ctrls = {m: manipulator.RobotController(0.001, rd, solver_mode=m) for m in MODES}
        inp = step_inputs(rd, robot, 2, B, cuda, stress=True)
        _cache[robot] = (rd, ctrls, inp, {})
    return _cache[robot]


def _pair(cuda, robot, mode, nb):
    """(sparse, dense) results of the two-kernel pipeline on the first nb instances, computed once."""
    rd, ctrls, inp, res = _robot(cuda, robot)
    if (mode, nb) not in res:
        sub = tuple(a[:, :nb].copy() for a in inp)
        n0 = _dense_launches(rd)
        sparse = _solve(ctrls[mode], rd, robot, 0, 0, *sub)
        n1 = _dense_launches(rd)
        dense = _solve(ctrls[mode], rd, robot, 1, 0, *sub)
        n2 = _dense_launches(rd)
        res[(mode, nb)] = (sparse, dense, (n1 - n0, n2 - n1))
    return res[(mode, nb)]


@pytest.mark.parametrize("nb", SIZES)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("robot", ["fr3", "ur5e"])
def test_sparse_matches_dense_bit_for_bit(cuda, robot, mode, nb):
    (o, s, i), (od, sd, idn), _ = _pair(cuda, robot, mode, nb)
    print("%s %s B=%d: %d solved, mean iterations %.1f, max %d; q-dot differs on %d instances, iterations on %d"
          % (robot, mode, nb, int((s == _capi.STATUS_SOLVED).sum()), i.mean(), i.max(),
             int(np.any(o != od, axis=0).sum()), int((i != idn).sum())))
    np.testing.assert_array_equal(s, sd)
    np.testing.assert_array_equal(i, idn)
    np.testing.assert_array_equal(o, od)
    assert np.isfinite(o).all()


@pytest.mark.parametrize("robot", ["fr3", "ur5e"])
def test_switch_selects_the_dense_build(cuda, robot):
    """The outputs cannot show which instantiation ran (they are equal): the
    model's count of dense QP launches moves with the switch on and only then."""
    _, _, (off, on) = _pair(cuda, robot, "exact", 65)
    assert off == 0 and on >= 1


@pytest.mark.parametrize("nb", [1, 65])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("robot", ["fr3", "ur5e"])
def test_fused_matches_sparse_pipeline(cuda, robot, mode, nb):
    rd, ctrls, inp, _ = _robot(cuda, robot)
    (o0, s0, i0), _, _ = _pair(cuda, robot, mode, nb)
    sub = tuple(a[:, :nb].copy() for a in inp)
    o1, s1, i1 = _solve(ctrls[mode], rd, robot, 0, 1, *sub)
    np.testing.assert_array_equal(s1, s0)
    np.testing.assert_array_equal(o1, o0)
    np.testing.assert_array_equal(i1, i0)


@pytest.mark.parametrize("robot", ["fr3", "ur5e"])
def test_parity_with_the_oracle(cuda, robot):
    rd, _, inp, _ = _robot(cuda, robot)
    (out, status, _), _, _ = _pair(cuda, robot, "exact", B)
    assert_qpik_parity(robot, rd.model, *inp, out, status, 0)
