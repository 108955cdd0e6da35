"""The synchronous host-buffer entries that stage their arrays through the
model's device buffer -- drc_qpid_host, drc_qpid_stages_host,
drc_closed_form_host, drc_dynamics_host, drc_joint_torque_step_host -- against
the *_batch entry each one wraps, run on device tensors with the same inputs:
the kernels and their launches are the same, so every output is the same bits
(assert_array_equal, no tolerance).

FR3 (nv = actuated = arm = 7) and XLS-FR3 (whole-body: nv, the actuated width
and the arm width all differ); B = 1 and B = 3 (an odd batch leaves the last
8-byte word of an int32 array half filled); B = 0 touches no output, B < 0 is
an error; the optional pointers NULL and given; one error that the host entry
leaves to its batch entry; and a sequence of entries on one model, whose
staging buffer is shared and regrown between calls, against fresh models."""
import ctypes as C

import numpy as np
import pytest

from _common import LINK, make_manipulator, make_moma, moma_step_inputs, step_inputs
from dyros_robot_controller_amd import _batch, _capi, manipulator

pytestmark = pytest.mark.gpu
ROBOTS = ("fr3", "xls_fr3")
POISON = {np.float64: -7.25, np.int32: -77}
F, I = np.float64, np.int32


def _make(robot, cuda):
    return make_moma(robot, cuda) if robot == "xls_fr3" else make_manipulator(robot, cuda)


@pytest.fixture(scope="module")
def world(cuda):
    """Per robot: the model and one B = 3 input set (B = 1 takes its first column)."""
    w = {}
    rng = np.random.default_rng(7)
    for robot in ROBOTS:
        rd = _make(robot, cuda)
        q, qd, xt, xdt = (moma_step_inputs if robot == "xls_fr3" else step_inputs)(rd, robot, 41, 3, cuda)
        n, nb = rd.model.dof, rd.model.mani_dof
        ins = dict(q=q, qd=qd, xt=xt, xdt=xdt, nullv=rng.uniform(-0.1, 0.1, (n, 3)),
                   q_target=rng.uniform(-1, 1, (nb, 3)), qd_target=rng.uniform(-1, 1, (nb, 3)),
                   qdd_target=rng.uniform(-1, 1, (nb, 3)))
        w[robot] = (rd, ins)
    return w


def _hptr(a):
    if a is None:
        return None
    return a.ctypes.data_as(C.POINTER(C.c_double if a.dtype == F else C.c_int))


def _dptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


# ---- the five entries: (host entry, batch entry, argument list, outputs {name: (rows or 0 for [B], dtype)})
def qpid_entry(model, p):
    lib, na = _capi.lib(), model.actuated_dof
    args = lambda B, i, o: (model.handle, C.byref(p), B, i("q"), i("qd"), i("xt"), i("xdt"), i("xi"), i("xdi"),
                            o("qdd"), o("tau"), o("status"), o("iters"))
    return lib.drc_qpid_host, lib.drc_qpid_batch, args, dict(qdd=(na, F), tau=(na, F), status=(0, I), iters=(0, I))


def qpid_stages_entry(model, p):
    lib, n, na = _capi.lib(), model.dof, model.mani_dof
    args = lambda B, i, o: (model.handle, C.byref(p), B, i("q"), i("qd"), i("xt"), i("xdt"), i("xi"), i("xdi"),
                            o("pose"), o("jac"), o("man"), o("dist"), o("pair"), o("xddot_des"), o("jdot"),
                            o("qpid_terms"), o("graddot"))
    spec = dict(pose=(12, F), jac=(6 * n, F), man=(1 + na, F), dist=(1 + n, F), pair=(0, I), xddot_des=(6, F),
                jdot=(6 * n, F), qpid_terms=(8, F), graddot=(na + n, F))
    return lib.drc_qpid_stages_host, lib.drc_qpid_stages_batch, args, spec


def closed_form_entry(model, p, kind):
    lib = _capi.lib()
    tail = lambda B, i, o: (B, i("q"), i("qd"), i("xt"), i("xdt"), i("xi"), i("xdi"), i("nullv"), o("out"))
    host = lambda *a: lib.drc_closed_form_host(model.handle, C.byref(p), kind, *a)
    batch = lambda *a: (lib.drc_clik_batch if kind == 1 else lib.drc_osf_batch)(model.handle, C.byref(p), *a)
    return host, batch, tail, dict(out=(model.dof, F))


def dynamics_entry(model, actuated):
    lib = _capi.lib()
    no = model.actuated_dof if actuated else model.dof
    args = lambda B, i, o: (model.handle, actuated, B, i("q"), i("qd"), o("M"), o("Minv"), o("g"), o("nle"), o("c"))
    spec = dict(M=(no * no, F), Minv=(no * no, F), g=(no, F), nle=(no, F), c=(no, F))
    return lib.drc_dynamics_host, lib.drc_dynamics_batch, args, spec


def torque_step_entry(model, kp, kv):
    lib = _capi.lib()
    args = lambda B, i, o: (model.handle, B, i("q"), i("qd"), i("q_target"), i("qd_target"), i("qdd_target"),
                            C.c_double(0.001), _hptr(kp), _hptr(kv), o("tau"))
    return lib.drc_joint_torque_step_host, lib.drc_joint_torque_step_batch, args, dict(tau=(model.mani_dof, F))


def _host_outputs(spec, B):
    return {k: np.full((r, B) if r else (B,), POISON[dt], dt) for k, (r, dt) in spec.items()}


def run_host(entry, B, ins, use, want, cols=None):
    """The host entry on the first `cols` (default B) columns of the inputs
    named in `use` (the others NULL); outputs outside `want` are passed as
    NULL.  Returns (rc, {name: array}) with every output array of the entry,
    poisoned before the call."""
    host, _, args, spec = entry
    nb = B if cols is None else cols
    hin = {k: np.ascontiguousarray(ins[k][:, :nb]) for k in use}
    out = _host_outputs(spec, nb)
    rc = host(*args(C.c_int64(B), lambda k: _hptr(hin.get(k)), lambda k: _hptr(out[k]) if k in want else None))
    return rc, out


def run_batch(cuda, entry, B, ins, use, want):
    import torch
    _, batch, args, spec = entry
    din = {k: _batch.as_device(np.ascontiguousarray(ins[k][:, :B]), cuda) for k in use}
    dout = {k: torch.zeros((spec[k][0], B) if spec[k][0] else (B,),
                           dtype=torch.float64 if spec[k][1] == F else torch.int32, device=cuda) for k in want}
    rc = batch(*args(C.c_int64(B), lambda k: _dptr(din.get(k)), lambda k: _dptr(dout.get(k))),
               C.c_void_p(torch.cuda.current_stream(cuda).cuda_stream))
    torch.cuda.synchronize()
    return rc, {k: v.cpu().numpy() for k, v in dout.items()}


def check_same(cuda, entry, B, ins, use, want):
    """Host entry == batch entry, bit for bit, on the outputs asked for; the
    host arrays that were not passed keep their poison."""
    rc, out = run_host(entry, B, ins, use, want)
    _capi.check(rc)
    rc, ref = run_batch(cuda, entry, B, ins, use, want)
    _capi.check(rc)
    for k in entry[3]:
        if k in want:
            np.testing.assert_array_equal(out[k], ref[k], err_msg=k)
        else:
            assert np.all(out[k] == POISON[entry[3][k][1]]), k


def check_edges(entry, ins, use):
    """B = 0: DRC_OK and no output touched; B = -1: DRC_ERR_INVALID_ARGUMENT
    (and no output touched).  Every pointer is given, with room for 3."""
    for B, code in ((0, _capi.DRC_OK), (-1, _capi.DRC_ERR_INVALID_ARGUMENT)):
        rc, out = run_host(entry, B, ins, use, tuple(entry[3]), cols=3)
        assert rc == code, (B, rc)
        for k, (_, dt) in entry[3].items():
            assert np.all(out[k] == POISON[dt]), (B, k)


TASK = ("q", "qd", "xt", "xdt")


def _qpid_params(model, robot):
    return manipulator.QPIKParamsBuilder(model, exact=True, qpid=True).params(LINK[robot], _capi.MODE_QPID_STEP)


def _qpik_params(model, robot):
    return manipulator.QPIKParamsBuilder(model, exact=True).params(LINK[robot], _capi.MODE_QPIK_STEP)


@pytest.mark.parametrize("robot", ROBOTS)
def test_qpid_host(cuda, world, robot):
    rd, ins = world[robot]
    e = qpid_entry(rd.model, _qpid_params(rd.model, robot))
    for B in (1, 3):
        check_same(cuda, e, B, ins, TASK, ("qdd", "tau", "status", "iters"))
        check_same(cuda, e, B, ins, TASK, ("qdd", "tau", "status"))          # iters NULL
    check_edges(e, ins, TASK)


@pytest.mark.parametrize("robot", ROBOTS)
def test_qpid_stages_host(cuda, world, robot):
    rd, ins = world[robot]
    e = qpid_stages_entry(rd.model, _qpid_params(rd.model, robot))
    every = tuple(e[3])
    for B in (1, 3):
        check_same(cuda, e, B, ins, TASK, every)
        check_same(cuda, e, B, ins, TASK, ("pair",))                         # the others keep their poison
        check_same(cuda, e, B, ins, TASK, tuple(k for k in every if k != "pair"))
    check_edges(e, ins, TASK)


@pytest.mark.parametrize("kind", [1, 2])
def test_closed_form_host(cuda, world, kind):
    rd, ins = world["fr3"]
    e = closed_form_entry(rd.model, _qpik_params(rd.model, "fr3"), kind)
    for B in (1, 3):
        check_same(cuda, e, B, ins, TASK, ("out",))                          # nullv NULL
        check_same(cuda, e, B, ins, TASK + ("nullv",), ("out",))
    check_edges(e, ins, TASK + ("nullv",))


@pytest.mark.parametrize("kind", [1, 2])
def test_closed_form_host_whole_body_is_the_batch_entrys_error(cuda, world, kind):
    """CLIK / OSF serve manipulators only: on XLS-FR3 the host entry returns
    what the batch entry returns, and writes nothing."""
    rd, ins = world["xls_fr3"]
    e = closed_form_entry(rd.model, _qpik_params(rd.model, "xls_fr3"), kind)
    lib = _capi.lib()
    rc_b, _ = run_batch(cuda, e, 3, ins, TASK, ("out",))
    text_b = lib.drc_last_error().decode()
    rc_h, out = run_host(e, 3, ins, TASK, ("out",))
    assert (rc_h, lib.drc_last_error().decode()) == (rc_b, text_b)
    assert rc_h == _capi.DRC_ERR_INVALID_ARGUMENT and text_b == "CLIK / OSF are Manipulator::RobotController entries"
    assert np.all(out["out"] == POISON[F])


@pytest.mark.parametrize("robot,actuated", [("fr3", 0), ("xls_fr3", 0), ("xls_fr3", 1)])
def test_dynamics_host(cuda, world, robot, actuated):
    rd, ins = world[robot]
    e = dynamics_entry(rd.model, actuated)
    for B in (1, 3):
        check_same(cuda, e, B, ins, ("q", "qd"), tuple(e[3]))
        check_same(cuda, e, B, ins, ("q",), ("g",))                          # qdot NULL, only g
    check_edges(e, ins, ("q", "qd"))


@pytest.mark.parametrize("robot", ROBOTS)
def test_dynamics_host_leaves_missing_qdot_to_the_batch_entry(world, robot):
    """nle without qdot: drc_dynamics_host does not check it, drc_dynamics_batch
    reports it; code and text as they were before the host entries shared one
    staging helper."""
    rd, ins = world[robot]
    rc, out = run_host(dynamics_entry(rd.model, 0), 3, ins, ("q",), ("g", "nle"))
    assert rc == _capi.DRC_ERR_INVALID_ARGUMENT
    assert _capi.lib().drc_last_error().decode() == "qdot is required for nle / c"
    assert np.all(out["g"] == POISON[F]) and np.all(out["nle"] == POISON[F])


@pytest.mark.parametrize("robot", ROBOTS)
def test_joint_torque_step_host(cuda, world, robot):
    rd, ins = world[robot]
    nb = rd.model.mani_dof
    gains = (np.linspace(300.0, 500.0, nb), np.linspace(30.0, 50.0, nb))
    state = ("q", "qd", "q_target", "qd_target")
    for kp, kv in ((None, None), gains):
        e = torque_step_entry(rd.model, kp, kv)
        for B in (1, 3):
            check_same(cuda, e, B, ins, state, ("tau",))                     # qddot_target NULL
            check_same(cuda, e, B, ins, state + ("qdd_target",), ("tau",))
    check_edges(torque_step_entry(rd.model, *gains), ins, state + ("qdd_target",))


def test_shared_staging_sequence(cuda, world):
    """Four entries in a row on one model -- dynamics at B = 3, QPID at B = 1,
    a closed form at B = 3, QPIK at B = 1: the staging buffer and its pinned
    mirror are shared, regrown and reused between them -- each against the
    same call on a model of its own."""
    _, ins = world["fr3"]
    lib = _capi.lib()

    def qpik_entry(model):
        p = _qpik_params(model, "fr3")
        args = lambda B, i, o: (model.handle, C.byref(p), B, i("q"), i("qd"), i("xt"), i("xdt"), None, None,
                                o("out"), o("status"), o("iters"))
        return lib.drc_qpik_host, None, args, dict(out=(model.actuated_dof, F), status=(0, I), iters=(0, I))

    steps = ((lambda m: dynamics_entry(m, 0), 3, ("q", "qd")),
             (lambda m: qpid_entry(m, _qpid_params(m, "fr3")), 1, TASK),
             (lambda m: closed_form_entry(m, _qpik_params(m, "fr3"), 1), 3, TASK),
             (qpik_entry, 1, TASK))
    shared = make_manipulator("fr3", cuda)
    for make, B, use in steps:
        e = make(shared.model)
        rc, out = run_host(e, B, ins, use, tuple(e[3]))
        _capi.check(rc)
        fresh = make_manipulator("fr3", cuda)
        e = make(fresh.model)
        rc, ref = run_host(e, B, ins, use, tuple(e[3]))
        _capi.check(rc)
        for k in ref:
            np.testing.assert_array_equal(out[k], ref[k], err_msg=k)
