"""A call's outputs do not depend on what its stream's scratch held before.

A model keeps four device blocks per caller stream (DESIGN.md "Stream
scratch"): the pool, the closed-loop scratch, the seeds scratch and the COD
list.  Every entry carves its block by its own layout, so a block last carved
by one entry is carved next by another, grows when a call needs more and is
reused, larger than needed, by the next smaller call.  Here one model per robot
runs a sequence of calls on one stream, passing through the entry kinds at a
small batch (3), then a large one (67; 2 049 for drc_qpik_batch, the smallest
batch at which the default knobs switch the order arrays on), then the small
one again, first on the stepwise paths (drc_set_fusion 0), then on the
persistent ones.  Every output tensor of every call is compared bit for bit
with the same call on a model created for that call alone.

The sizes are the smallest at which the host-side layout can go wrong; the
kernels' own wave-boundary cases are covered by the entries' own tests."""
import ctypes as C

import numpy as np
import pytest

import _obstacles as OB
from _common import LINK, make_manipulator, make_moma, moma_step_inputs, step_inputs
from dyros_robot_controller_amd import _batch, _capi, manipulator, mobile_manipulator

pytestmark = pytest.mark.gpu

SMALL, LARGE, ORDER_ON = 3, 67, 2049
DT, POS_TOL, ROT_TOL = 0.005, 1e-4, 1e-3
SEEDS = ((3, 2), (23, 3), (3, 2))   # (T, S)
TWO_TYPES, TWO_PARAMS = OB.FOUR_TYPES[:2], OB.FOUR_PARAMS[:2]


def _tensors(res):
    """The output tensors of a call, by name."""
    import torch
    if isinstance(res, dict):
        items = res.items()
    elif isinstance(res, tuple):
        items = enumerate(res)
    elif torch.is_tensor(res):
        items = [("out", res)]
    else:
        items = vars(res).items()
    return {str(k): v for k, v in items if torch.is_tensor(v)}


def _set_fusion(rd, on):
    _capi.check(_capi.lib().drc_set_fusion(rd.model.handle, C.c_int(on)))


def _fr3_inputs(cuda):
    rd = make_manipulator("fr3", cuda)
    ctrl = manipulator.RobotController(0.001, rd, solver_mode="exact")
    q, v, xt, xdt = step_inputs(rd, "fr3", 71, ORDER_ON, cuda)
    ik = ctrl._pb.params(LINK["fr3"], _capi.MODE_QPIK_STEP, np.full(6, 100.0), np.zeros(6))
    ik.w_reg = 0.01
    return dict(q=q, v=v, xt=xt, xdt=xdt, ik=ik,
                id=ctrl._pbd.params(LINK["fr3"], _capi.MODE_QPID_STEP, ctrl.Kp_task_, ctrl.Kv_task_),
                cf=ctrl._pb.params(LINK["fr3"], _capi.MODE_QPIK_STEP, ctrl.Kp_task_, ctrl.Kv_task_))


def _husky_inputs(cuda):
    rd = make_moma("husky_fr3", cuda)
    ctrl = mobile_manipulator.RobotController(0.001, rd, solver_mode="exact")
    q, v, xt, xdt = moma_step_inputs(rd, "husky_fr3", 72, LARGE, cuda)
    return dict(q=q, v=v, xt=xt, xdt=xdt,
                id=ctrl._pbd.params(LINK["husky_fr3"], _capi.MODE_QPID_STEP, ctrl.Kp_task_, ctrl.Kv_task_))


def _slotted_fr3(cuda):
    rd = make_manipulator("fr3", cuda)
    rd.set_obstacles(TWO_TYPES, TWO_PARAMS, OB.FR3_ARM_LINKS)
    return rd


class _Calls:
    """The entries as (name, fusion, call) with call(model) -> output tensors; every call
    takes the first columns of one input set, so the same call has the same inputs on any model."""

    def __init__(self, I, cuda, poses=None):
        self.I, self.dev, self.poses = I, cuda, poses

    def cols(self, B, *names):
        return [_batch.as_device(np.ascontiguousarray(self.I[k][:, :B]), self.dev) for k in names]

    def pose(self, B):
        return None if self.poses is None else np.ascontiguousarray(self.poses[:, :, :B])

    def qpik(self, m, B):
        return _batch.qpik_batch(m, self.I["ik"], *self.cols(B, "q", "v", "xt", "xdt"), obstacle_pose=self.pose(B))

    def stages(self, m, B):
        return _batch.stages_batch(m, self.I["ik"], *self.cols(B, "q", "v", "xt", "xdt"))

    def qpid(self, m, B):
        return _batch.qpid_batch(m, self.I["id"], *self.cols(B, "q", "v", "xt", "xdt"))

    def osf(self, m, B):
        return _batch.closed_form_batch(m, self.I["cf"], "osf", *self.cols(B, "q", "v", "xt", "xdt"))

    def minv(self, m, B):
        return _batch.dynamics_batch(m, *self.cols(B, "q", "v"), fields=("Minv",))

    def rollout(self, m, B):
        return _batch.qpik_rollout_batch(m, self.I["ik"], *self.cols(B, "q", "v"), 3, DT, *self.cols(B, "xt", "xdt"),
                                         want=())

    def reach(self, m, B):
        return _batch.qpik_reach_batch(m, self.I["ik"], *self.cols(B, "q", "v", "xt", "xdt"), 3, DT, POS_TOL, ROT_TOL,
                                       obstacle_pose=self.pose(B))

    def reach_path(self, m, B):
        import torch
        q, v, xt, xdt = self.cols(B, "q", "v", "xt", "xdt")
        xt2, xdt2 = self.cols(2 * B, "xt", "xdt")
        path = torch.stack((xt, xt2[:, B:])).contiguous()      # W = 2: the instance's target, then another's
        return _batch.qpik_reach_path_batch(m, self.I["ik"], q, v, path, torch.stack((xdt, xdt2[:, B:])).contiguous(),
                                            2, DT, POS_TOL, ROT_TOL)

    def seeds(self, m, TS):
        T, S = TS
        q, v = self.cols(S * T, "q", "v")
        xt, xdt = self.cols(T, "xt", "xdt")
        nv = q.shape[0]
        return _batch.qpik_reach_seeds_batch(m, self.I["ik"], q.view(nv, S, T), v.view(nv, S, T), xt, xdt, 3, DT,
                                             POS_TOL, ROT_TOL, want=_batch.REACH_SEEDS_FIELDS,
                                             obstacle_pose=self.pose(T))

    def passes(self, fusion, kinds):
        """Size by size through the kinds: consecutive calls on a block are of different kinds."""
        out = []
        for i, B in enumerate((SMALL, LARGE, SMALL)):
            for kind in kinds:
                n = {"qpik": {LARGE: ORDER_ON}.get(B, B), "seeds": SEEDS[i]}.get(kind, B)
                out.append(("%s %s fusion %d" % (kind, n, fusion), fusion, lambda m, f=getattr(self, kind), n=n: f(m, n)))
        return out


CLOSED_LOOP = ("rollout", "reach", "reach_path", "seeds")


def _sequences(cuda):
    """(robot, model factory, calls) of the three shared models."""
    fr3 = _Calls(_fr3_inputs(cuda), cuda)
    husky = _Calls(_husky_inputs(cuda), cuda)
    slotted = _Calls(fr3.I, cuda, OB.to_field_major(OB.fr3_scene(11, LARGE + SMALL, types=TWO_TYPES)))
    return [
        ("fr3", lambda: make_manipulator("fr3", cuda),
         fr3.passes(0, ("qpik", "stages", "qpid", "osf", "minv") + CLOSED_LOOP) + fr3.passes(1, CLOSED_LOOP + ("qpik",))),
        ("husky_fr3", lambda: make_moma("husky_fr3", cuda), husky.passes(1, ("qpid",))),
        ("fr3 with two slots", lambda: _slotted_fr3(cuda),
         slotted.passes(0, ("seeds", "reach")) + slotted.passes(1, ("seeds", "reach"))),
    ]


def test_outputs_do_not_depend_on_earlier_calls(cuda):
    import torch
    ncalls = 0
    for robot, make, calls in _sequences(cuda):
        shared = make()
        got = []
        for name, fusion, call in calls:
            _set_fusion(shared, fusion)
            got.append(_tensors(call(shared.model)))
        torch.cuda.synchronize()
        for (name, fusion, call), mine in zip(calls, got):
            alone = make()
            _set_fusion(alone, fusion)
            ref = _tensors(call(alone.model))
            torch.cuda.synchronize()
            assert mine.keys() == ref.keys() and len(ref) > 0, (robot, name)
            for k in ref:
                assert torch.equal(mine[k], ref[k]), "%s, %s: %s differs from the call on a fresh model" % (robot, name, k)
            ncalls += 1
    print("%d calls compared" % ncalls)
