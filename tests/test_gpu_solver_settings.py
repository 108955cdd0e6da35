"""The ADMM loop's control flow under solver settings the bench never uses.

Since r06 the ADMM iterations run as a call-free loop between termination
checks / adaptive-rho steps (qp_solver.hpp: qp_admm drives admm_iters_schur
and admm_check), so the loop bounds are computed from max_iter,
check_termination and adaptive_rho_interval instead of tested per iteration.
These cases exercise every boundary of that computation against the oracle
(oracle/drc_oracle.c runs OSQP's per-iteration loop, QP_base.h:143-177):

  * max_iter below the first check (5 < 25 in reference mode, 5 < 8 in exact
    mode): MaxIter after exactly 5 iterations, zero output (QP_IK.cpp:56-61);
  * max_iter not a multiple of the check interval (60 with checks every 25);
  * no termination checks (check_termination = 0): MaxIter at max_iter;
  * adaptive rho off, and checks / adaptive-rho steps on interleaved intervals
    (10 / 7: steps that fall on one iteration and on different ones);
  * exact mode with a short check interval (3).

Device against the oracle on identical settings (FR3 and XLS-FR3 on the Schur
loop, Caster-FR3 on the runtime-sized LDS loop, which tests the intervals at
every iteration; stress-tier inputs): iteration counts and statuses identical
and q-dot within the
reference census bound (1e-7 relative up to 150 iterations, x10 per 250
beyond; 1e-6 in exact mode, the parity contract's QP bound) on every instance
except where both sides ran >= 500 ADMM iterations (the reference-settings
contract's exemption, tests/test_gpu_reference_settings.py: the interleaved
adaptive-rho case has two such FR3 runs of ~1 000+ iterations); exact zeros
where not Solved.
"""
import numpy as np
import pytest

import oracle as O
from _common import LINK, make_manipulator, make_moma, moma_step_inputs, oracle_params, step_inputs
from dyros_robot_controller_amd import manipulator, mobile_manipulator

pytestmark = pytest.mark.gpu

B = 256
LONG_RUN = 500


def run_length_tol(k):
    """The reference census envelope (tests/test_gpu_reference_settings.py):
    1e-7 relative up to 150 iterations, x10 per 250 beyond."""
    return 1e-7 * 10.0 ** (np.maximum(k - 150, 0) / 250.0)
CASES = [
    ("osqp_default", {"max_iter": 5}),
    ("osqp_default", {"max_iter": 60}),
    ("osqp_default", {"max_iter": 60, "check_termination": 0}),
    ("osqp_default", {"adaptive_rho": 0}),
    ("osqp_default", {"check_termination": 10, "adaptive_rho_interval": 7}),
    ("exact", {"max_iter": 5}),
    ("exact", {"check_termination": 3, "max_iter": 100}),
]


# Caster-FR3 runs the runtime-sized QP kernel (no compiled shape), so its loop
# bounds and checks face the oracle too.  It leaves out {"adaptive_rho": 0}
# alone: there the oracle itself runs >= LONG_RUN iterations on 230 of the 256
# instances, so the test's floor on compared instances (B // 4) cannot hold.
_ids = [f"{m}-{'-'.join(f'{k}{v}' for k, v in o.items())}" for m, o in CASES]
ROBOT_CASES = [pytest.param(r, m, o, id=f"{i}-{r}") for r in ("fr3", "xls_fr3", "caster_fr3")
               for (m, o), i in zip(CASES, _ids) if not (r == "caster_fr3" and o == {"adaptive_rho": 0})]


@pytest.mark.parametrize("robot,mode,over", ROBOT_CASES)
def test_admm_loop_bounds_match_oracle(cuda, robot, mode, over):
    import torch
    moma = robot in ("xls_fr3", "caster_fr3")
    rd = make_moma(robot, cuda) if moma else make_manipulator(robot, cuda)
    ctrl = (mobile_manipulator if moma else manipulator).RobotController(0.001, rd, solver_mode=mode)
    for k, v in over.items():
        setattr(ctrl._pb.base.solver, k, v)
    args = (moma_step_inputs if moma else step_inputs)(rd, robot, 7, B, cuda, stress=True)
    args = [a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a) for a in args]
    it = torch.zeros(B, dtype=torch.int32, device=cuda)
    out, st = ctrl.QPIK_step_batch(*[torch.as_tensor(a, device=cuda) for a in args], LINK[robot], iters=it)
    torch.cuda.synchronize()
    out, st, it = out.cpu().numpy(), st.cpu().numpy(), it.cpu().numpy()

    par, om = oracle_params(robot, exact=(mode == "exact"))
    for k, v in over.items():
        setattr(par.solver, k, v)
    ref, rst, rit = O.qpik_batch(om, par, *args, nthreads=16)

    assert np.all(np.isfinite(out))
    bad = st != 1
    assert np.all(out[:, bad] == 0.0), "non-Solved instances must return zeros"
    max_iter = over.get("max_iter", int(par.solver.max_iter))
    assert np.all(it <= max_iter)
    if max_iter < (int(par.solver.check_termination) or max_iter + 1):
        assert np.all(st != 1) and np.all(it == max_iter), "stops before the first check: MaxIter at max_iter"
    if over.get("check_termination") == 0:
        assert np.all(it == max_iter)
    # the reference-settings contract's exemption: two ADMM trajectories that
    # both ran >= LONG_RUN iterations may separate (rounding, amplified by the
    # run length; the census of tests/test_gpu_reference_settings.py)
    long_run = (it >= LONG_RUN) & (rit >= LONG_RUN)
    agree = ~long_run
    np.testing.assert_array_equal(it[agree], rit[agree])
    np.testing.assert_array_equal(st[agree], rst[agree])
    assert agree.sum() >= B // 4   # (XLS-FR3 without adaptive rho: two thirds of its runs exceed 500 iterations)
    scale = np.maximum(1.0, np.abs(ref).max(axis=0))
    err = (np.abs(out - ref).max(axis=0) / scale)[agree]
    tol = 1e-6 if mode == "exact" else run_length_tol(it[agree])
    assert np.all(err <= tol), (float(err.max()), int(it[agree][err.argmax()]))
