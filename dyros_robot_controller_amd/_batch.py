"""Batched device-side entry: torch tensors in HBM -> C-ABI -> HIP kernel.

torch is used as plumbing only (device allocations and the current HIP
stream); the arithmetic happens in ``libdrc_amd.so``.
"""
import ctypes as C

import numpy as np

from . import _capi

_FIELD_SHAPES = {"q": "dof", "qdot": "dof", "x_target": 12, "xdot_target": 6, "x_init": 12, "xdot_init": 6}


def _torch():
    import torch
    return torch


def as_device(a, device):
    """float64, contiguous, on ``device`` (a torch.device)."""
    torch = _torch()
    if a is None:
        return None
    if not isinstance(a, torch.Tensor):
        a = torch.as_tensor(np.asarray(a, dtype=np.float64))
    return a.to(device=device, dtype=torch.float64).contiguous()


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def check_shapes(dof, B, **fields):
    for k, v in fields.items():
        if v is None:
            continue
        rows = dof if _FIELD_SHAPES[k] == "dof" else _FIELD_SHAPES[k]
        if tuple(v.shape) != (rows, B):
            raise ValueError("%s must be [%d][B=%d] (field-major SoA), got %s" % (k, rows, B, tuple(v.shape)))


def obstacle_poses(model, obstacle_pose, B, device, steps=None):
    """The obstacle-pose argument of the ``*_obstacles_batch`` entries:
    (device tensor, obstacle_ld, per_step).  Accepts [n][12] (one set shared by
    the batch, ld 0) or [n][12][B] (a set per instance), n the model's obstacle
    slots, each pose R column-major then p as ``x_target``; with ``steps`` also
    a leading [steps] axis (per_step True)."""
    n = model.n_obstacles
    t = as_device(obstacle_pose, device)
    shape = tuple(t.shape)
    cores = ((n, 12), (n, 12, B))
    per_step = shape not in cores and steps is not None and shape[:1] == (steps,) and shape[1:] in cores
    core = shape[1:] if per_step else shape
    if core in cores:
        return t, (0 if len(core) == 2 else B), per_step
    raise ValueError("obstacle_pose must be [n=%d][12] or [n=%d][12][B=%d]%s, got %s"
                     % (n, n, B, "" if steps is None else ", optionally with a leading [steps=%d]" % steps, shape))


def obstacle_twists(model, obstacle_twist, B, device, steps=None):
    """The obstacle-twist argument of the ``*_moving_obstacles_batch`` entries,
    obstacle_poses' sibling: (device tensor, obstacle_ld, per_step) for [n][6]
    or [n][6][B] (optionally with a leading [steps] axis), each twist the
    world-frame velocity v of the slot pose's origin, then the angular velocity."""
    n = model.n_obstacles
    t = as_device(obstacle_twist, device)
    shape = tuple(t.shape)
    cores = ((n, 6), (n, 6, B))
    per_step = shape not in cores and steps is not None and shape[:1] == (steps,) and shape[1:] in cores
    core = shape[1:] if per_step else shape
    if core in cores:
        return t, (0 if len(core) == 2 else B), per_step
    raise ValueError("obstacle_twist must be [n=%d][6] or [n=%d][6][B=%d]%s, got %s"
                     % (n, n, B, "" if steps is None else ", optionally with a leading [steps=%d]" % steps, shape))


def _pose_and_twist(model, obstacle_pose, obstacle_twist, B, device, steps=None):
    """(pose, twist, obstacle_ld, per_step) of a call with twists: the C entries
    take one obstacle_ld and one obstacles_per_step for both arrays, so a twist
    laid out otherwise than the poses is brought to their layout."""
    if obstacle_pose is None:
        raise ValueError("obstacle_twist without obstacle_pose")
    op, ld, per_step = obstacle_poses(model, obstacle_pose, B, device, steps=steps)
    tw, tld, tps = obstacle_twists(model, obstacle_twist, B, device, steps=steps)
    n = model.n_obstacles
    if tps and not per_step:
        raise ValueError("per-step obstacle_twist needs per-step obstacle_pose")
    if tld and not ld:
        raise ValueError("per-instance obstacle_twist needs per-instance obstacle_pose")
    if ld and not tld:
        tw = tw.unsqueeze(-1).expand(*tw.shape, B)
    if per_step and not tps:
        tw = tw.unsqueeze(0).expand(steps, *tw.shape)
    return op, tw.contiguous(), ld, per_step


def obstacle_trajectory(pose0, twist, dt, steps):
    """Poses of obstacle slots that move with a constant twist: [steps][n][12]
    (or [steps][n][12][B] when ``pose0`` or ``twist`` carries the [B] axis) with
    R_k = exp(k dt omega^) R_0 and p_k = p_0 + k dt v, k = 0 .. steps - 1, from
    ``pose0`` [n][12]([B]) (R column-major, then p) and ``twist`` [n][6]([B])
    (v, then omega; world frame, v taken at the pose origin).  Rodrigues'
    formula in float64 torch, on ``pose0``'s device.  The per-step
    ``obstacle_pose`` that is consistent with an ``obstacle_twist``."""
    torch = _torch()
    p0 = pose0 if isinstance(pose0, torch.Tensor) else torch.as_tensor(np.asarray(pose0, dtype=np.float64))
    p0 = p0.to(torch.float64)
    tw = twist if isinstance(twist, torch.Tensor) else torch.as_tensor(np.asarray(twist, dtype=np.float64))
    tw = tw.to(device=p0.device, dtype=torch.float64)
    batched = p0.dim() == 3 or tw.dim() == 3
    shapes = (tuple(p0.shape), tuple(tw.shape))
    if p0.dim() == 2:
        p0 = p0.unsqueeze(-1)
    if tw.dim() == 2:
        tw = tw.unsqueeze(-1)
    n = p0.shape[0]
    if p0.dim() != 3 or tw.dim() != 3 or p0.shape[1] != 12 or tuple(tw.shape[:2]) != (n, 6):
        raise ValueError("pose0 must be [n][12]([B]) and twist [n][6]([B]), got %s and %s"
                         % shapes)
    nb = max(p0.shape[2], tw.shape[2])
    p0 = p0.expand(n, 12, nb)
    tw = tw.expand(n, 6, nb)
    steps = int(steps)
    k = torch.arange(steps, dtype=torch.float64, device=p0.device).view(steps, 1, 1, 1) * float(dt)
    phi = k * tw[None, :, 3:6]                      # rotation vector k dt omega: [steps][n][3][nb]
    th = torch.sqrt((phi * phi).sum(dim=2))         # [steps][n][nb]
    u = phi / torch.where(th > 0, th, torch.ones_like(th)).unsqueeze(2)
    s, c2 = torch.sin(th), 2.0 * torch.sin(0.5 * th) ** 2   # sin, 1 - cos
    ux, uy, uz = u[:, :, 0], u[:, :, 1], u[:, :, 2]
    zero = torch.zeros_like(ux)
    K = torch.stack((torch.stack((zero, -uz, uy), 2), torch.stack((uz, zero, -ux), 2),
                     torch.stack((-uy, ux, zero), 2)), 2)   # [steps][n][3][3][nb]
    eye = torch.eye(3, dtype=torch.float64, device=p0.device).view(1, 1, 3, 3, 1)
    uu = u.unsqueeze(3) * u.unsqueeze(2)
    E = eye + s[:, :, None, None] * K + c2[:, :, None, None] * (uu - eye)   # unit u: K^2 = u u^T - I
    C0 = p0[:, :9].reshape(n, 3, 3, nb)             # [n][column j][row i][nb]
    Ck = torch.einsum("snimb,njmb->snjib", E, C0)
    Ck = torch.where((th > 0)[:, :, None, None], Ck, C0.unsqueeze(0).expand(steps, n, 3, 3, nb))
    kv = k * tw[None, :, 0:3]
    P0 = p0[None, :, 9:12].expand(steps, n, 3, nb)
    Pk = torch.where(kv != 0, P0 + kv, P0)
    out = torch.cat((Ck.reshape(steps, n, 9, nb), Pk), dim=2).contiguous()
    return out if batched else out[..., 0].contiguous()


def qpik_batch(model, params, q, qdot, x_target=None, xdot_target=None, x_init=None, xdot_init=None,
               out=None, status=None, iters=None, stream=None, obstacle_pose=None, obstacle_twist=None):
    """Launch ``drc_qpik_batch`` on device tensors laid out [field][B]
    (``drc_qpik_obstacles_batch`` with ``obstacle_pose``, see obstacle_poses;
    ``drc_qpik_moving_obstacles_batch`` with ``obstacle_twist`` too, see
    obstacle_twists)."""
    torch = _torch()
    dev = q.device
    B = q.shape[1]
    check_shapes(model.dof, B, q=q, qdot=qdot, x_target=x_target, xdot_target=xdot_target,
                 x_init=x_init, xdot_init=xdot_init)
    if out is None:
        out = torch.empty((model.actuated_dof, B), dtype=torch.float64, device=dev)
    if status is None:
        status = torch.empty(B, dtype=torch.int32, device=dev)
    if stream is None:
        stream = torch.cuda.current_stream(dev).cuda_stream
    if obstacle_twist is not None:
        op, tw, ld, _ = _pose_and_twist(model, obstacle_pose, obstacle_twist, B, dev)
        _capi.check(_capi.lib().drc_qpik_moving_obstacles_batch(
            model.handle, C.byref(params), C.c_int64(B), _ptr(q), _ptr(qdot), _ptr(x_target), _ptr(xdot_target),
            _ptr(x_init), _ptr(xdot_init), _ptr(op), _ptr(tw), C.c_int64(ld), _ptr(out), _ptr(status), _ptr(iters),
            C.c_void_p(stream)))
        return out, status
    if obstacle_pose is not None:
        op, ld, _ = obstacle_poses(model, obstacle_pose, B, dev)
        _capi.check(_capi.lib().drc_qpik_obstacles_batch(
            model.handle, C.byref(params), C.c_int64(B), _ptr(q), _ptr(qdot), _ptr(x_target), _ptr(xdot_target),
            _ptr(x_init), _ptr(xdot_init), _ptr(op), C.c_int64(ld), _ptr(out), _ptr(status), _ptr(iters),
            C.c_void_p(stream)))
        return out, status
    _capi.check(_capi.lib().drc_qpik_batch(
        model.handle, C.byref(params), C.c_int64(B), _ptr(q), _ptr(qdot), _ptr(x_target), _ptr(xdot_target),
        _ptr(x_init), _ptr(xdot_init), _ptr(out), _ptr(status), _ptr(iters), C.c_void_p(stream)))
    return out, status


ROLLOUT_FIELDS = ("qdot_traj", "iters_traj", "q_traj", "pose_traj", "dist_traj")


class RolloutResult:
    """Device tensors of one ``drc_qpik_rollout_batch`` call: ``q_final``,
    ``qdot_final`` [dof][B], ``status_traj`` [steps][B], and those of
    ``qdot_traj`` [steps][na][B], ``iters_traj`` [steps][B], ``q_traj``
    [steps][dof][B], ``pose_traj`` [steps][12][B], ``dist_traj``
    [steps][1+dof][B] that were asked for (None otherwise)."""

    def __init__(self, **fields):
        self.__dict__.update(fields)


def qpik_rollout_batch(model, params, q, qdot, steps, dt, x_target=None, xdot_target=None, x_init=None,
                       xdot_init=None, targets_per_step=False, want=("qdot_traj", "q_traj"), q_final=None,
                       qdot_final=None, stream=None, obstacle_pose=None, obstacle_twist=None):
    """Launch ``drc_qpik_rollout_batch`` on device tensors laid out [field][B]
    (per-step targets: [steps][field][B]); with ``obstacle_pose`` (see
    obstacle_poses; a leading [steps] axis moves the obstacles)
    ``drc_qpik_rollout_obstacles_batch``, with ``obstacle_twist`` too (see
    obstacle_twists; obstacle_trajectory makes the poses that go with a
    constant twist) ``drc_qpik_rollout_moving_obstacles_batch``.  ``want``: the optional
    trajectories to allocate and fill (ROLLOUT_FIELDS); ``q_final`` /
    ``qdot_final`` may be given (``q`` / ``qdot`` themselves: in place)."""
    torch = _torch()
    dev = q.device
    B = q.shape[1]
    steps = int(steps)
    nv, na = model.dof, model.actuated_dof
    check_shapes(nv, B, q=q, qdot=qdot, x_init=x_init, xdot_init=xdot_init)
    unknown = set(want) - set(ROLLOUT_FIELDS)
    if unknown:
        raise ValueError("unknown rollout outputs %s (know %s)" % (sorted(unknown), ROLLOUT_FIELDS))
    if targets_per_step:
        for name, t, rows in (("x_target", x_target, 12), ("xdot_target", xdot_target, 6)):
            if t is not None and tuple(t.shape) != (steps, rows, B):
                raise ValueError("%s must be [steps=%d][%d][B=%d], got %s" % (name, steps, rows, B, tuple(t.shape)))
    else:
        check_shapes(nv, B, x_target=x_target, xdot_target=xdot_target)
    for name, t in (("q_final", q_final), ("qdot_final", qdot_final)):
        if t is not None and (tuple(t.shape) != (nv, B) or t.dtype != torch.float64 or not t.is_contiguous()):
            raise ValueError("%s must be a contiguous float64 [%d][B=%d] tensor" % (name, nv, B))
    n = max(steps, 0)
    f = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)
    i = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)
    res = RolloutResult(
        q_final=f(nv, B) if q_final is None else q_final,
        qdot_final=f(nv, B) if qdot_final is None else qdot_final,
        status_traj=i(n, B),
        qdot_traj=f(n, na, B) if "qdot_traj" in want else None,
        iters_traj=i(n, B) if "iters_traj" in want else None,
        q_traj=f(n, nv, B) if "q_traj" in want else None,
        pose_traj=f(n, 12, B) if "pose_traj" in want else None,
        dist_traj=f(n, 1 + nv, B) if "dist_traj" in want else None)
    if stream is None:
        stream = torch.cuda.current_stream(dev).cuda_stream
    if obstacle_twist is not None:
        op, tw, ld, per_step = _pose_and_twist(model, obstacle_pose, obstacle_twist, B, dev, steps=steps)
        _capi.check(_capi.lib().drc_qpik_rollout_moving_obstacles_batch(
            model.handle, C.byref(params), C.c_int64(B), C.c_int(steps), C.c_double(dt), _ptr(q), _ptr(qdot),
            _ptr(x_target), _ptr(xdot_target), _ptr(x_init), _ptr(xdot_init), C.c_int(1 if targets_per_step else 0),
            _ptr(op), _ptr(tw), C.c_int64(ld), C.c_int(1 if per_step else 0),
            _ptr(res.q_final), _ptr(res.qdot_final), _ptr(res.qdot_traj), _ptr(res.status_traj),
            _ptr(res.iters_traj), _ptr(res.q_traj), _ptr(res.pose_traj), _ptr(res.dist_traj), C.c_void_p(stream)))
        return res
    if obstacle_pose is not None:
        op, ld, per_step = obstacle_poses(model, obstacle_pose, B, dev, steps=steps)
        _capi.check(_capi.lib().drc_qpik_rollout_obstacles_batch(
            model.handle, C.byref(params), C.c_int64(B), C.c_int(steps), C.c_double(dt), _ptr(q), _ptr(qdot),
            _ptr(x_target), _ptr(xdot_target), _ptr(x_init), _ptr(xdot_init), C.c_int(1 if targets_per_step else 0),
            _ptr(op), C.c_int64(ld), C.c_int(1 if per_step else 0),
            _ptr(res.q_final), _ptr(res.qdot_final), _ptr(res.qdot_traj), _ptr(res.status_traj),
            _ptr(res.iters_traj), _ptr(res.q_traj), _ptr(res.pose_traj), _ptr(res.dist_traj), C.c_void_p(stream)))
        return res
    _capi.check(_capi.lib().drc_qpik_rollout_batch(
        model.handle, C.byref(params), C.c_int64(B), C.c_int(steps), C.c_double(dt), _ptr(q), _ptr(qdot),
        _ptr(x_target), _ptr(xdot_target), _ptr(x_init), _ptr(xdot_init), C.c_int(1 if targets_per_step else 0),
        _ptr(res.q_final), _ptr(res.qdot_final), _ptr(res.qdot_traj), _ptr(res.status_traj), _ptr(res.iters_traj),
        _ptr(res.q_traj), _ptr(res.pose_traj), _ptr(res.dist_traj), C.c_void_p(stream)))
    return res


REACH_FIELDS = ("status_last", "iters_total", "err_final", "dist_final")


def reach_thresholds(pos_tol, rot_tol):
    """``drc_reach_thresholds``: (tau_p, tau_R), the numbers ``drc_qpik_reach_batch``
    compares ``err_final``'s two rows with."""
    out = (C.c_double * 2)()
    _capi.check(_capi.lib().drc_reach_thresholds(C.c_double(pos_tol), C.c_double(rot_tol), out))
    return float(out[0]), float(out[1])


class ReachResult:
    """Device tensors of one ``drc_qpik_reach_batch`` call: ``q_final``,
    ``qdot_final`` [dof][B], ``result`` [B] (REACHED, BUDGET or QP_FAILED),
    ``steps_used`` [B], and those of ``status_last`` [B], ``iters_total`` [B],
    ``err_final`` [2][B] (e_p, e_R), ``dist_final`` [1+dof][B] that were asked
    for (None otherwise); ``thresholds``: (tau_p, tau_R) on the host."""
    REACHED, BUDGET, QP_FAILED = _capi.REACH_REACHED, _capi.REACH_BUDGET, _capi.REACH_QP_FAILED

    def __init__(self, **fields):
        self.__dict__.update(fields)


def qpik_reach_batch(model, params, q, qdot, x_target, xdot_target, max_steps, dt, pos_tol=1e-4, rot_tol=1e-3,
                     want=REACH_FIELDS, q_final=None, qdot_final=None, stream=None, obstacle_pose=None):
    """Launch ``drc_qpik_reach_batch`` on device tensors laid out [field][B]
    (``drc_qpik_reach_obstacles_batch`` with ``obstacle_pose``, see
    obstacle_poses: one pose set for the horizon).  ``want``: the optional
    outputs to allocate and fill (REACH_FIELDS); ``q_final`` / ``qdot_final``
    may be given (``q`` / ``qdot`` themselves: in place)."""
    torch = _torch()
    dev = q.device
    B = q.shape[1]
    nv = model.dof
    check_shapes(nv, B, q=q, qdot=qdot, x_target=x_target, xdot_target=xdot_target)
    unknown = set(want) - set(REACH_FIELDS)
    if unknown:
        raise ValueError("unknown reach outputs %s (know %s)" % (sorted(unknown), REACH_FIELDS))
    for name, t in (("q_final", q_final), ("qdot_final", qdot_final)):
        if t is not None and (tuple(t.shape) != (nv, B) or t.dtype != torch.float64 or not t.is_contiguous()):
            raise ValueError("%s must be a contiguous float64 [%d][B=%d] tensor" % (name, nv, B))
    f = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)
    i = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)
    res = ReachResult(
        q_final=f(nv, B) if q_final is None else q_final,
        qdot_final=f(nv, B) if qdot_final is None else qdot_final,
        result=i(B), steps_used=i(B),
        status_last=i(B) if "status_last" in want else None,
        iters_total=i(B) if "iters_total" in want else None,
        err_final=f(2, B) if "err_final" in want else None,
        dist_final=f(1 + nv, B) if "dist_final" in want else None,
        thresholds=None)
    if stream is None:
        stream = torch.cuda.current_stream(dev).cuda_stream
    head = (model.handle, C.byref(params), C.c_int64(B), C.c_int(int(max_steps)), C.c_double(dt),
            C.c_double(pos_tol), C.c_double(rot_tol), _ptr(q), _ptr(qdot), _ptr(x_target), _ptr(xdot_target))
    tail = (_ptr(res.q_final), _ptr(res.qdot_final), _ptr(res.result), _ptr(res.steps_used), _ptr(res.status_last),
            _ptr(res.iters_total), _ptr(res.err_final), _ptr(res.dist_final), C.c_void_p(stream))
    if obstacle_pose is not None:
        op, ld, _ = obstacle_poses(model, obstacle_pose, B, dev)
        _capi.check(_capi.lib().drc_qpik_reach_obstacles_batch(*head, _ptr(op), C.c_int64(ld), *tail))
    else:
        _capi.check(_capi.lib().drc_qpik_reach_batch(*head, *tail))
    res.thresholds = reach_thresholds(pos_tol, rot_tol)
    return res


REACH_PATH_FIELDS = REACH_FIELDS + ("dist_min", "steps_at")


class ReachPathResult(ReachResult):
    """Device tensors of one ``drc_qpik_reach_path_batch`` call: those of a
    ReachResult (``steps_used`` the total over the call, ``err_final`` against
    the waypoint the instance stopped at), ``waypoints_reached`` [B] (0 .. W),
    and those of ``dist_min`` [B], ``steps_at`` [W][B] (-1: never reached) that
    were asked for (None otherwise)."""


def qpik_reach_path_batch(model, params, q, qdot, x_path, xdot_path, max_steps, dt, pos_tol=1e-4, rot_tol=1e-3,
                          want=REACH_PATH_FIELDS, q_final=None, qdot_final=None, stream=None, obstacle_pose=None):
    """Launch ``drc_qpik_reach_path_batch`` on device tensors: ``q`` / ``qdot``
    [dof][B], ``x_path`` [W][12][B], ``xdot_path`` [W][6][B]
    (``drc_qpik_reach_path_obstacles_batch`` with ``obstacle_pose``, see
    obstacle_poses: one pose set for the call).  ``max_steps`` is the budget of
    one segment.  ``want``: the optional outputs to allocate and fill
    (REACH_PATH_FIELDS); ``q_final`` / ``qdot_final`` may be given (``q`` /
    ``qdot`` themselves: in place)."""
    torch = _torch()
    dev = q.device
    B = q.shape[1]
    nv = model.dof
    check_shapes(nv, B, q=q, qdot=qdot)
    W = x_path.shape[0] if x_path.dim() == 3 else -1
    for name, t, rows in (("x_path", x_path, 12), ("xdot_path", xdot_path, 6)):
        if t.dim() != 3 or tuple(t.shape) != (W, rows, B):
            raise ValueError("%s must be [W][%d][B=%d], got %s" % (name, rows, B, tuple(t.shape)))
    unknown = set(want) - set(REACH_PATH_FIELDS)
    if unknown:
        raise ValueError("unknown reach path outputs %s (know %s)" % (sorted(unknown), REACH_PATH_FIELDS))
    for name, t in (("q_final", q_final), ("qdot_final", qdot_final)):
        if t is not None and (tuple(t.shape) != (nv, B) or t.dtype != torch.float64 or not t.is_contiguous()):
            raise ValueError("%s must be a contiguous float64 [%d][B=%d] tensor" % (name, nv, B))
    f = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)
    i = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)
    res = ReachPathResult(
        q_final=f(nv, B) if q_final is None else q_final,
        qdot_final=f(nv, B) if qdot_final is None else qdot_final,
        result=i(B), waypoints_reached=i(B), steps_used=i(B),
        status_last=i(B) if "status_last" in want else None,
        iters_total=i(B) if "iters_total" in want else None,
        err_final=f(2, B) if "err_final" in want else None,
        dist_final=f(1 + nv, B) if "dist_final" in want else None,
        dist_min=f(B) if "dist_min" in want else None,
        steps_at=i(W, B) if "steps_at" in want else None,
        thresholds=None)
    if stream is None:
        stream = torch.cuda.current_stream(dev).cuda_stream
    head = (model.handle, C.byref(params), C.c_int64(B), C.c_int(W), C.c_int(int(max_steps)), C.c_double(dt),
            C.c_double(pos_tol), C.c_double(rot_tol), _ptr(q), _ptr(qdot), _ptr(x_path), _ptr(xdot_path))
    tail = (_ptr(res.q_final), _ptr(res.qdot_final), _ptr(res.result), _ptr(res.waypoints_reached),
            _ptr(res.steps_used), _ptr(res.status_last), _ptr(res.iters_total), _ptr(res.err_final),
            _ptr(res.dist_final), _ptr(res.dist_min), _ptr(res.steps_at), C.c_void_p(stream))
    if obstacle_pose is not None:
        op, ld, _ = obstacle_poses(model, obstacle_pose, B, dev)
        _capi.check(_capi.lib().drc_qpik_reach_path_obstacles_batch(*head, _ptr(op), C.c_int64(ld), *tail))
    else:
        _capi.check(_capi.lib().drc_qpik_reach_path_batch(*head, *tail))
    res.thresholds = reach_thresholds(pos_tol, rot_tol)
    return res


REACH_SEEDS_FIELDS = REACH_FIELDS + ("inst_result", "inst_steps")
SEEDS_RULES = {"first": _capi.SEEDS_FIRST, "fewest_steps": _capi.SEEDS_FEWEST_STEPS}


class ReachSeedsResult:
    """Device tensors of one ``drc_qpik_reach_seeds_batch`` call, one entry per
    target: ``seed`` [T] (the winner's index), ``result`` [T], ``steps_used``
    [T], ``q_sol``, ``qdot_sol`` [dof][T], and those of ``status_last`` [T],
    ``iters_total`` [T], ``err_final`` [2][T], ``dist_final`` [1+dof][T] and the
    per-instance diagnostics ``inst_result``, ``inst_steps`` [S][T] that were
    asked for (None otherwise); ``thresholds``: (tau_p, tau_R) on the host."""
    REACHED, BUDGET, QP_FAILED, CANCELLED = (_capi.REACH_REACHED, _capi.REACH_BUDGET, _capi.REACH_QP_FAILED,
                                             _capi.REACH_CANCELLED)

    def __init__(self, **fields):
        self.__dict__.update(fields)


def qpik_reach_seeds_batch(model, params, q, qdot, x_target, xdot_target, max_steps, dt, pos_tol=1e-4, rot_tol=1e-3,
                           seeds=None, rule="first", cancel=True, want=REACH_FIELDS, stream=None, obstacle_pose=None):
    """Launch ``drc_qpik_reach_seeds_batch`` on device tensors: ``q`` / ``qdot``
    [dof][S][T], or [dof][S*T] with ``seeds`` = S (seed s of target t at column
    s*T + t); ``x_target`` [12][T], ``xdot_target`` [6][T]
    (``drc_qpik_reach_seeds_obstacles_batch`` with ``obstacle_pose`` [n][12]
    for one scene or [n][12][T] for one per target).  ``rule``: "first" or
    "fewest_steps" (or the DRC_SEEDS_* value); ``cancel``: losers stop once
    their group has its answer, which never changes an output.  ``want``: the
    optional outputs to allocate and fill (REACH_SEEDS_FIELDS)."""
    torch = _torch()
    dev = q.device
    nv = model.dof
    T = x_target.shape[1] if x_target.dim() == 2 else -1
    if q.dim() == 3:
        S = q.shape[1]
        if seeds is not None and int(seeds) != S:
            raise ValueError("q is [dof][S=%d][T] but seeds = %s" % (S, seeds))
    else:
        if seeds is None:
            raise ValueError("q laid out [dof][S*T] needs seeds = S")
        S = int(seeds)
    for name, t in (("q", q), ("qdot", qdot)):
        if tuple(t.shape) not in ((nv, S, T), (nv, S * T)) or t.dtype != torch.float64 or not t.is_contiguous():
            raise ValueError("%s must be a contiguous float64 [%d][S=%d][T=%d] or [%d][S*T] tensor, got %s"
                             % (name, nv, S, T, nv, tuple(t.shape)))
    check_shapes(nv, T, x_target=x_target, xdot_target=xdot_target)
    unknown = set(want) - set(REACH_SEEDS_FIELDS)
    if unknown:
        raise ValueError("unknown reach seeds outputs %s (know %s)" % (sorted(unknown), REACH_SEEDS_FIELDS))
    f = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)
    i = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)
    res = ReachSeedsResult(
        seed=i(T), result=i(T), steps_used=i(T), q_sol=f(nv, T), qdot_sol=f(nv, T),
        status_last=i(T) if "status_last" in want else None,
        iters_total=i(T) if "iters_total" in want else None,
        err_final=f(2, T) if "err_final" in want else None,
        dist_final=f(1 + nv, T) if "dist_final" in want else None,
        inst_result=i(S, T) if "inst_result" in want else None,
        inst_steps=i(S, T) if "inst_steps" in want else None,
        thresholds=None)
    if stream is None:
        stream = torch.cuda.current_stream(dev).cuda_stream
    head = (model.handle, C.byref(params), C.c_int64(T), C.c_int(S), C.c_int(SEEDS_RULES.get(rule, rule)),
            C.c_int(1 if cancel else 0), C.c_int(int(max_steps)), C.c_double(dt), C.c_double(pos_tol),
            C.c_double(rot_tol), _ptr(q), _ptr(qdot), _ptr(x_target), _ptr(xdot_target))
    tail = (_ptr(res.seed), _ptr(res.result), _ptr(res.steps_used), _ptr(res.q_sol), _ptr(res.qdot_sol),
            _ptr(res.status_last), _ptr(res.iters_total), _ptr(res.err_final), _ptr(res.dist_final),
            _ptr(res.inst_result), _ptr(res.inst_steps), C.c_void_p(stream))
    if obstacle_pose is not None:
        op, ld, _ = obstacle_poses(model, obstacle_pose, T, dev)
        _capi.check(_capi.lib().drc_qpik_reach_seeds_obstacles_batch(*head, _ptr(op), C.c_int64(ld), *tail))
    else:
        _capi.check(_capi.lib().drc_qpik_reach_seeds_batch(*head, *tail))
    res.thresholds = reach_thresholds(pos_tol, rot_tol)
    return res


class ClearanceResult:
    """Device tensors of one ``drc_clearance_path_batch`` call, one entry per
    path: ``result`` [B] (FREE / BLOCKED / INVALID), ``sample_stop`` [B] (-1
    when FREE), ``d_min`` [B], ``sample_min`` [B], ``pair_min`` [B], and
    ``dist_traj`` [N][B] when asked for (None otherwise; entries past a stop
    hold what the tensor held before the call)."""
    FREE, BLOCKED, INVALID = _capi.CLEAR_FREE, _capi.CLEAR_BLOCKED, _capi.CLEAR_INVALID

    def __init__(self, **fields):
        self.__dict__.update(fields)


def clearance_path_batch(model, q_path, substeps=1, d_stop=None, obstacle_pose=None, dist_traj=False, stream=None):
    """Launch ``drc_clearance_path_batch`` on a device tensor ``q_path``
    [waypoints][dof][B] (a rollout's ``q_traj`` fits): the minimum distance over
    the N = (waypoints - 1) substeps + 1 samples of each path, stopping at the
    first sample below ``d_stop`` (None: -inf, the whole profile).
    ``obstacle_pose`` [n][12] or [n][12][B] (see obstacle_poses):
    ``drc_clearance_path_obstacles_batch``.  ``dist_traj``: True allocates the
    [N][B] profile (zeros), a tensor of that shape is filled in place."""
    torch = _torch()
    dev = q_path.device
    nv = model.dof
    if q_path.dim() != 3 or q_path.shape[1] != nv or q_path.dtype != torch.float64 or not q_path.is_contiguous():
        raise ValueError("q_path must be a contiguous float64 [waypoints][%d][B] tensor, got %s"
                         % (nv, tuple(q_path.shape)))
    W, B = int(q_path.shape[0]), int(q_path.shape[2])
    substeps = int(substeps)
    N = (W - 1) * substeps + 1
    if isinstance(dist_traj, torch.Tensor):
        if tuple(dist_traj.shape) != (N, B) or dist_traj.dtype != torch.float64 or not dist_traj.is_contiguous():
            raise ValueError("dist_traj must be a contiguous float64 [N=%d][B=%d] tensor, got %s"
                             % (N, B, tuple(dist_traj.shape)))
        traj = dist_traj
    else:
        traj = torch.zeros((max(N, 0), B), dtype=torch.float64, device=dev) if dist_traj else None
    i = lambda: torch.empty(B, dtype=torch.int32, device=dev)
    res = ClearanceResult(result=i(), sample_stop=i(), d_min=torch.empty(B, dtype=torch.float64, device=dev),
                          sample_min=i(), pair_min=i(), dist_traj=traj)
    if stream is None:
        stream = torch.cuda.current_stream(dev).cuda_stream
    head = (model.handle, C.c_int64(B), C.c_int(W), C.c_int(substeps),
            C.c_double(-np.inf if d_stop is None else d_stop), _ptr(q_path))
    tail = (_ptr(res.result), _ptr(res.sample_stop), _ptr(res.d_min), _ptr(res.sample_min), _ptr(res.pair_min),
            _ptr(res.dist_traj), C.c_void_p(stream))
    if obstacle_pose is not None:
        op, ld, _ = obstacle_poses(model, obstacle_pose, B, dev)
        _capi.check(_capi.lib().drc_clearance_path_obstacles_batch(*head, _ptr(op), C.c_int64(ld), *tail))
    else:
        _capi.check(_capi.lib().drc_clearance_path_batch(*head, *tail))
    return res


class CertifyResult:
    """Device tensors of one ``drc_clearance_certify_batch`` call, one entry per
    path: ``result`` [B] (FREE / BLOCKED / INVALID / UNDECIDED), ``seg_stop``,
    ``t_stop`` [B] (-1 when FREE), ``d_min``, ``seg_min``, ``t_min``,
    ``pair_min`` [B], ``d_lower`` [B] (the certified lower bound of the
    continuous path when FREE), ``samples_used`` [B], and ``motion_bound``
    [waypoints - 1][B] when asked for (None otherwise; segments that were not
    started hold what the tensor held before the call)."""
    FREE, BLOCKED, INVALID, UNDECIDED = _capi.CLEAR_FREE, _capi.CLEAR_BLOCKED, _capi.CLEAR_INVALID, _capi.CLEAR_UNDECIDED

    def __init__(self, **fields):
        self.__dict__.update(fields)


def clearance_certify_batch(model, q_path, d_stop=0.0, max_depth=8, obstacle_pose=None, motion_bound=False,
                            stream=None):
    """Launch ``drc_clearance_certify_batch`` on a device tensor ``q_path``
    [waypoints][dof][B]: the continuous check of each path against ``d_stop``
    by adaptive bisection down to ``max_depth`` (include/drc_amd.h states the
    rule).  ``obstacle_pose`` [n][12] or [n][12][B] (see obstacle_poses):
    ``drc_clearance_certify_obstacles_batch``.  ``motion_bound``: True allocates
    the [waypoints - 1][B] bounds (zeros), a tensor of that shape is filled in
    place."""
    torch = _torch()
    dev = q_path.device
    nv = model.dof
    if q_path.dim() != 3 or q_path.shape[1] != nv or q_path.dtype != torch.float64 or not q_path.is_contiguous():
        raise ValueError("q_path must be a contiguous float64 [waypoints][%d][B] tensor, got %s"
                         % (nv, tuple(q_path.shape)))
    W, B = int(q_path.shape[0]), int(q_path.shape[2])
    if isinstance(motion_bound, torch.Tensor):
        if tuple(motion_bound.shape) != (W - 1, B) or motion_bound.dtype != torch.float64 \
                or not motion_bound.is_contiguous():
            raise ValueError("motion_bound must be a contiguous float64 [waypoints - 1 = %d][B = %d] tensor, got %s"
                             % (W - 1, B, tuple(motion_bound.shape)))
        mb = motion_bound
    else:
        mb = torch.zeros((max(W - 1, 0), B), dtype=torch.float64, device=dev) if motion_bound else None
    i = lambda: torch.empty(B, dtype=torch.int32, device=dev)
    d = lambda: torch.empty(B, dtype=torch.float64, device=dev)
    res = CertifyResult(result=i(), seg_stop=i(), t_stop=d(), d_min=d(), seg_min=i(), t_min=d(), pair_min=i(),
                        d_lower=d(), samples_used=i(), motion_bound=mb)
    if stream is None:
        stream = torch.cuda.current_stream(dev).cuda_stream
    head = (model.handle, C.c_int64(B), C.c_int(W), C.c_double(d_stop), C.c_int(int(max_depth)), _ptr(q_path))
    tail = (_ptr(res.result), _ptr(res.seg_stop), _ptr(res.t_stop), _ptr(res.d_min), _ptr(res.seg_min),
            _ptr(res.t_min), _ptr(res.pair_min), _ptr(res.d_lower), _ptr(res.samples_used), _ptr(res.motion_bound),
            C.c_void_p(stream))
    if obstacle_pose is not None:
        op, ld, _ = obstacle_poses(model, obstacle_pose, B, dev)
        _capi.check(_capi.lib().drc_clearance_certify_obstacles_batch(*head, _ptr(op), C.c_int64(ld), *tail))
    else:
        _capi.check(_capi.lib().drc_clearance_certify_batch(*head, *tail))
    return res


def motion_weights(model):
    """``drc_model_motion_weights``: (rho [dof][n_geoms], wt [dof][n_pairs],
    travel_mask) of the model as it stands (obstacle slots included), numpy."""
    dof, ngeom, npairs = C.c_int(), C.c_int(), C.c_int()
    _capi.check(_capi.lib().drc_model_info(model.handle, C.byref(dof), None, None, None, C.byref(ngeom),
                                           C.byref(npairs)))
    rho = np.zeros((dof.value, ngeom.value), dtype=np.float64)
    wt = np.zeros((dof.value, npairs.value), dtype=np.float64)
    mask = C.c_uint32()
    dp = C.POINTER(C.c_double)
    _capi.check(_capi.lib().drc_model_motion_weights(model.handle, rho.ctypes.data_as(dp), wt.ctypes.data_as(dp),
                                                     C.byref(mask)))
    return rho, wt, mask.value


def clearance_grid(model):
    """``drc_debug_clearance_grid``: the waves of the model's last clearance launch (0: none yet)."""
    g = C.c_int64()
    _capi.check(_capi.lib().drc_debug_clearance_grid(model.handle, C.byref(g)))
    return g.value


def qpid_batch(model, params, q, qdot, x_target=None, xdot_target=None, x_init=None, xdot_init=None,
               qddot=None, tau=None, status=None, iters=None, stream=None):
    """Launch ``drc_qpid_batch``: returns (qddot [na][B],
    tau [na][B], status [B]) device tensors."""
    torch = _torch()
    dev = q.device
    B = q.shape[1]
    check_shapes(model.dof, B, q=q, qdot=qdot, x_target=x_target, xdot_target=xdot_target,
                 x_init=x_init, xdot_init=xdot_init)
    na = model.actuated_dof
    if qddot is None:
        qddot = torch.empty((na, B), dtype=torch.float64, device=dev)
    if tau is None:
        tau = torch.empty((na, B), dtype=torch.float64, device=dev)
    if status is None:
        status = torch.empty(B, dtype=torch.int32, device=dev)
    if stream is None:
        stream = torch.cuda.current_stream(dev).cuda_stream
    _capi.check(_capi.lib().drc_qpid_batch(
        model.handle, C.byref(params), C.c_int64(B), _ptr(q), _ptr(qdot), _ptr(x_target), _ptr(xdot_target),
        _ptr(x_init), _ptr(xdot_init), _ptr(qddot), _ptr(tau), _ptr(status), _ptr(iters), C.c_void_p(stream)))
    return qddot, tau, status


def qpid_stages_batch(model, params, q, qdot, x_target=None, xdot_target=None, x_init=None, xdot_init=None):
    """QPID stage outputs: the QPIK stage fields plus jdot [6*nv][B] and
    qpid_terms [8][B] = (Jdot v, man grad_dot . qdot_arm, dist grad_dot . qdot_arm)."""
    torch = _torch()
    dev = q.device
    B = q.shape[1]
    nv = model.dof
    f = lambda r: torch.zeros((r, B), dtype=torch.float64, device=dev)
    pose, jac, man, dist, xdd, jdot, terms = f(12), f(6 * nv), f(1 + model.mani_dof), f(1 + nv), f(6), f(6 * nv), f(8)
    gdv = f(model.mani_dof + nv)
    pair = torch.zeros(B, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    _capi.check(_capi.lib().drc_qpid_stages_batch(
        model.handle, C.byref(params), C.c_int64(B), _ptr(q), _ptr(qdot), _ptr(x_target), _ptr(xdot_target),
        _ptr(x_init), _ptr(xdot_init), _ptr(pose), _ptr(jac), _ptr(man), _ptr(dist), _ptr(pair), _ptr(xdd),
        _ptr(jdot), _ptr(terms), _ptr(gdv), C.c_void_p(stream)))
    return dict(pose=pose, jac=jac, man=man, dist=dist, pair=pair, xddot_des=xdd, jdot=jdot, qpid_terms=terms,
                man_graddot=gdv[:model.mani_dof], dist_graddot=gdv[model.mani_dof:])


def stages_batch(model, params, q, qdot, x_target=None, xdot_target=None, x_init=None, xdot_init=None,
                 obstacle_pose=None, obstacle_twist=None):
    """Stage outputs (pose, J, manipulability, min distance, task velocity);
    with ``obstacle_pose`` (see obstacle_poses) ``drc_qpik_stages_obstacles_batch``;
    with ``obstacle_twist`` too ``drc_qpik_stages_moving_obstacles_batch``, which
    adds ``dist_rate`` [B], the closest pair's dd/dt from the slot's motion."""
    torch = _torch()
    dev = q.device
    B = q.shape[1]
    nv = model.dof
    mani = model.mani_dof
    f = lambda r: torch.zeros((r, B), dtype=torch.float64, device=dev)
    pose, jac, man, dist, xdd = f(12), f(6 * nv), f(1 + mani), f(1 + nv), f(6)
    pair = torch.zeros(B, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    if obstacle_twist is not None:
        op, tw, ld, _ = _pose_and_twist(model, obstacle_pose, obstacle_twist, B, dev)
        rate = torch.zeros(B, dtype=torch.float64, device=dev)
        _capi.check(_capi.lib().drc_qpik_stages_moving_obstacles_batch(
            model.handle, C.byref(params), C.c_int64(B), _ptr(q), _ptr(qdot), _ptr(x_target), _ptr(xdot_target),
            _ptr(x_init), _ptr(xdot_init), _ptr(op), _ptr(tw), C.c_int64(ld), _ptr(pose), _ptr(jac), _ptr(man),
            _ptr(dist), _ptr(pair), _ptr(xdd), _ptr(rate), C.c_void_p(stream)))
        return dict(pose=pose, jac=jac, man=man, dist=dist, pair=pair, xdot_des=xdd, dist_rate=rate)
    if obstacle_pose is not None:
        op, ld, _ = obstacle_poses(model, obstacle_pose, B, dev)
        _capi.check(_capi.lib().drc_qpik_stages_obstacles_batch(
            model.handle, C.byref(params), C.c_int64(B), _ptr(q), _ptr(qdot), _ptr(x_target), _ptr(xdot_target),
            _ptr(x_init), _ptr(xdot_init), _ptr(op), C.c_int64(ld), _ptr(pose), _ptr(jac), _ptr(man), _ptr(dist),
            _ptr(pair), _ptr(xdd), C.c_void_p(stream)))
        return dict(pose=pose, jac=jac, man=man, dist=dist, pair=pair, xdot_des=xdd)
    _capi.check(_capi.lib().drc_qpik_stages_batch(
        model.handle, C.byref(params), C.c_int64(B), _ptr(q), _ptr(qdot), _ptr(x_target), _ptr(xdot_target),
        _ptr(x_init), _ptr(xdot_init), _ptr(pose), _ptr(jac), _ptr(man), _ptr(dist), _ptr(pair), _ptr(xdd),
        C.c_void_p(stream)))
    return dict(pose=pose, jac=jac, man=man, dist=dist, pair=pair, xdot_des=xdd)


DYN_FIELDS = ("M", "Minv", "g", "nle", "c")


def dynamics_batch(model, q, qdot=None, actuated=False, fields=DYN_FIELDS, stream=None):
    """Launch ``drc_dynamics_batch`` on device tensors
    [dof][B]; returns {name: tensor} with M, Minv as [n][n][B] and the vectors
    as [n][B] (n = actuated dof when ``actuated``)."""
    torch = _torch()
    dev = q.device
    B = q.shape[1]
    check_shapes(model.dof, B, q=q, qdot=qdot)
    n = model.actuated_dof if actuated else model.dof
    out = {}
    for k in fields:
        rows = n * n if k in ("M", "Minv") else n
        out[k] = torch.empty((rows, B), dtype=torch.float64, device=dev)
    if stream is None:
        stream = torch.cuda.current_stream(dev).cuda_stream
    _capi.check(_capi.lib().drc_dynamics_batch(
        model.handle, C.c_int(1 if actuated else 0), C.c_int64(B), _ptr(q), _ptr(qdot),
        _ptr(out.get("M")), _ptr(out.get("Minv")), _ptr(out.get("g")), _ptr(out.get("nle")), _ptr(out.get("c")),
        C.c_void_p(stream)))
    for k in ("M", "Minv"):
        if k in out:
            out[k] = out[k].view(n, n, B)
    return out


def dynamics_host(model, q, qdot=None, actuated=False):
    """``drc_dynamics_host`` on numpy arrays [dof][B] (synchronous)."""
    q = np.ascontiguousarray(q, dtype=np.float64)
    B = q.shape[1]
    qd = None if qdot is None else np.ascontiguousarray(qdot, dtype=np.float64)
    n = model.actuated_dof if actuated else model.dof
    M, Mi = np.zeros((n, n, B)), np.zeros((n, n, B))
    g = np.zeros((n, B))
    nle = np.zeros((n, B)) if qd is not None else None
    c = np.zeros((n, B)) if qd is not None else None
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double)) if a is not None else None
    _capi.check(_capi.lib().drc_dynamics_host(model.handle, C.c_int(1 if actuated else 0), C.c_int64(B), dp(q),
                                              dp(qd), dp(M), dp(Mi), dp(g), dp(nle), dp(c)))
    return dict(M=M, Minv=Mi, g=g, nle=nle, c=c)


def joint_torque_step_batch(model, q, qdot=None, q_target=None, qdot_target=None, qddot_target=None, dt=0.0,
                            kp=None, kv=None, stream=None):
    """``drc_joint_torque_step_batch`` on device tensors: tau [nb][B] for the
    controlled block (all joints, or the arm of a mobile manipulator)."""
    torch = _torch()
    dev = q.device
    B = q.shape[1]
    check_shapes(model.dof, B, q=q, qdot=qdot)
    nb = model.mani_dof
    for name, t in (("q_target", q_target), ("qdot_target", qdot_target), ("qddot_target", qddot_target)):
        if t is not None and tuple(t.shape) != (nb, B):
            raise ValueError("%s must be [%d][B=%d], got %s" % (name, nb, B, tuple(t.shape)))
    tau = torch.empty((nb, B), dtype=torch.float64, device=dev)
    gain = lambda g: None if g is None else np.ascontiguousarray(np.broadcast_to(np.asarray(g, float), (nb,)))
    kp, kv = gain(kp), gain(kv)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double)) if a is not None else None
    if stream is None:
        stream = torch.cuda.current_stream(dev).cuda_stream
    _capi.check(_capi.lib().drc_joint_torque_step_batch(
        model.handle, C.c_int64(B), _ptr(q), _ptr(qdot), _ptr(q_target), _ptr(qdot_target), _ptr(qddot_target),
        C.c_double(dt), dp(kp), dp(kv), _ptr(tau), C.c_void_p(stream)))
    return tau


def closed_form_batch(model, params, kind, q, qdot, x_target=None, xdot_target=None, x_init=None, xdot_init=None,
                      null=None, out=None, stream=None):
    """``drc_clik_batch`` (kind "clik") / ``drc_osf_batch`` (kind "osf") on
    device tensors [field][B]; returns qdot / tau [dof][B]."""
    torch = _torch()
    dev = q.device
    B = q.shape[1]
    check_shapes(model.dof, B, q=q, qdot=qdot, x_target=x_target, xdot_target=xdot_target,
                 x_init=x_init, xdot_init=xdot_init)
    if null is not None and tuple(null.shape) != (model.dof, B):
        raise ValueError("null vector must be [%d][B=%d]" % (model.dof, B))
    if out is None:
        out = torch.empty((model.dof, B), dtype=torch.float64, device=dev)
    if stream is None:
        stream = torch.cuda.current_stream(dev).cuda_stream
    fn = _capi.lib().drc_clik_batch if kind == "clik" else _capi.lib().drc_osf_batch
    _capi.check(fn(model.handle, C.byref(params), C.c_int64(B), _ptr(q), _ptr(qdot), _ptr(x_target),
                   _ptr(xdot_target), _ptr(x_init), _ptr(xdot_init), _ptr(null), _ptr(out), C.c_void_p(stream)))
    return out
