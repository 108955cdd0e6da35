"""Reach from several seeds per target (drc_qpik_reach_seeds_batch,
QPIK_reach_seeds_batch) against the caller's composition: drc_qpik_reach_batch
on the S T instances with the targets replicated, plus the rule of
include/drc_amd.h in numpy (tests/_reach_seeds.py).  Every comparison is
bitwise, for both rules and with and without cancellation: cancellation changes
how much work the losers do, never an output.

Inputs: the gains, dt and tolerances of tests/test_gpu_reach.py; target t is
the stage pose at the census goal t; seed (s, t) = clip(goal + default_rng(
200000 + 1000 s + t).uniform(-0.3, 0.3, nv)) to the position limits clipped to
+-3; v0 = 0; 60 steps.  On the CPU oracle, FR3 with T = 64 and S = 4: 45 to 49
instances per seed reach, 59 groups have a reached seed (1, 14, 30, 44 and 60
do not), FIRST picks seed 0 in 49 groups and a later seed in 10, FEWEST_STEPS
spreads the winners 17 / 14 / 14 / 14 with 3 step ties.

Placed by hand in every configuration (_place), so that every case occurs
whatever the device's sample holds: group 0 has its target 5 m below the
floor (none reaches); one group has every seed a bitwise copy of its seed 0 (a
tie); for every j one group has seed j sitting on the target (REACHED at step
0: the FEWEST_STEPS winner), with the seeds below j bitwise copies of a seed of
that group that did not reach in the unplaced sample, where the group has one
(the FIRST winner is then j too).  Whether a seed fails is up to the device's
sample; FR3's has such groups (the oracle's has 15), and the FIRST winners of
every index are asserted there."""
import ctypes as C
import re

import numpy as np
import pytest

import _reach as RC
import _reach_seeds as RS
import test_gpu_reach as TR
from _common import LINK
from _mesh_io import box_triangles, write_stl_ascii
from dyros_robot_controller_amd import _batch, _capi, manipulator, robot_path

pytestmark = pytest.mark.gpu

POS_TOL, ROT_TOL, MAX_STEPS = TR.POS_TOL, TR.ROT_TOL, 60
GROUP = ("result", "steps_used", "q_sol", "qdot_sol") + _batch.REACH_FIELDS
OUT = ("seed",) + GROUP
INST = {"result": "result", "steps_used": "steps_used", "q_sol": "q_final", "qdot_sol": "qdot_final",
        "status_last": "status_last", "iters_total": "iters_total", "err_final": "err_final",
        "dist_final": "dist_final"}
RULES = (RS.FIRST, RS.FEWEST_STEPS)
_CACHE = {}


def _goals(S, T):
    rd = S["rd"]
    lo, hi = rd.get_joint_position_limit() if S["moma"] else rd.getJointPositionLimit()
    return RC.census_states(lo, hi, T)[1], lo, hi


def _composition(S, q3, xt, xdt, obstacle_pose=None):
    """drc_qpik_reach_batch on the S T instances, targets (and per-target poses) replicated."""
    nv, Sd, T = q3.shape
    rep = lambda t: np.ascontiguousarray(np.tile(t, (1,) * (t.ndim - 1) + (Sd,)))
    op = obstacle_pose if obstacle_pose is None or obstacle_pose.ndim == 2 else rep(obstacle_pose)
    q = np.ascontiguousarray(q3.reshape(nv, Sd * T))
    return TR._reach(S, q=q, v=np.zeros_like(q), xt=rep(xt), xdt=rep(xdt), max_steps=MAX_STEPS, obstacle_pose=op)


def _winner(comp, rule, Sd, T):
    g = lambda k: comp[k].reshape(Sd, T)
    return RS.winner(rule, g("result"), g("steps_used"), comp["err_final"][0].reshape(Sd, T),
                     comp["err_final"][1].reshape(Sd, T))


def _gather(comp, rule, Sd, T):
    """The composition's per-group outputs: its instances gathered by the numpy rule."""
    win = _winner(comp, rule, Sd, T)
    b = win.astype(np.int64) * T + np.arange(T)
    out = {k: comp[src][..., b] for k, src in INST.items()}
    out["seed"] = win
    return out


def _seeds(S, q3, xt, xdt, rule, cancel, want=_batch.REACH_SEEDS_FIELDS, obstacle_pose=None, flat=False):
    import torch
    a = lambda t: _batch.as_device(np.array(t), S["dev"])
    nv, Sd, T = q3.shape
    q = a(q3.reshape(nv, Sd * T) if flat else q3)
    res = _batch.qpik_reach_seeds_batch(S["rd"].model, S["p"], q, torch.zeros_like(q), a(xt), a(xdt), MAX_STEPS,
                                        S["dt"], POS_TOL, ROT_TOL, seeds=Sd if flat else None, rule=rule,
                                        cancel=cancel, want=want, obstacle_pose=obstacle_pose)
    assert res.thresholds == RC.thresholds(POS_TOL, ROT_TOL)
    TR._sync()
    return {k: (None if getattr(res, k) is None else getattr(res, k).cpu().numpy())
            for k in OUT + ("inst_result", "inst_steps")}


def _assert_same(got, ref, fields=OUT, msg=""):
    for k in fields:
        np.testing.assert_array_equal(got[k], ref[k], err_msg="%s %s" % (k, msg))


def _place(q3, xt, goal, comp0):
    """The cases placed by hand (module docstring): (q3, xt, first_ok), first_ok
    the seed indices j > 0 whose group got failing copies below seed j."""
    nv, Sd, T = q3.shape
    q3, xt = q3.copy(), xt.copy()
    reached0 = comp0["result"].reshape(Sd, T) == RC.REACHED
    xt[11, 0] -= 5.0
    free = list(range(1, T))
    tie = next((t for t in free if reached0[0, t] and comp0["steps_used"][t] > 0), free[0])
    free.remove(tie)
    q3[:, :, tie] = q3[:, :1, tie]
    first_ok = []
    for j in range(Sd - 1, -1, -1):   # (the groups with a failing seed go to the highest j first)
        t = next((t for t in free if not reached0[:, t].all()), free[0]) if j else free[0]
        free.remove(t)
        if j and not reached0[:, t].all():
            q3[:, :j, t] = q3[:, [int(np.argmin(reached0[:, t]))], t]
            first_ok.append(j)
        q3[:, j, t] = goal[:, t]
    return q3, xt, first_ok


def _case(robot, cuda, T, Sd=4):
    """Inputs with the placed cases and the composition's results (shared, never modified)."""
    key = (robot, T, Sd)
    if key not in _CACHE:
        S = TR._setup(robot, cuda, T)
        goal, lo, hi = _goals(S, T)
        q3 = RS.seeds(goal, lo, hi, Sd)
        comp0 = _composition(S, q3, S["xt"], S["xdt"])
        q3, xt, first_ok = _place(q3, S["xt"], goal, comp0)
        comp = _composition(S, q3, xt, S["xdt"])
        for v in (q3, xt, *comp.values()):
            v.setflags(write=False)
        _CACHE[key] = dict(S=S, q3=q3, xt=xt, xdt=S["xdt"], comp=comp, first_ok=first_ok, natural=comp0)
    return _CACHE[key]


def _coverage(K, Sd, T, robot):
    """Every case occurs: a winner of every index, a group with none reached, a tie."""
    comp = K["comp"]
    res, steps = comp["result"].reshape(Sd, T), comp["steps_used"].reshape(Sd, T)
    reached = res == RC.REACHED
    assert set(np.unique(res)) <= {RC.REACHED, RC.BUDGET, RC.QP_FAILED}
    assert (~reached.any(axis=0)).any() and not reached[:, 0].any()
    fewest = np.where(reached, steps, MAX_STEPS + 1)
    ties = ((fewest == fewest.min(axis=0)).sum(axis=0) > 1) & reached.any(axis=0)
    assert ties.any()
    some = reached.any(axis=0)
    assert set(_winner(comp, RS.FEWEST_STEPS, Sd, T)[some]) == set(range(Sd))
    first = set(_winner(comp, RS.FIRST, Sd, T)[some])
    assert first >= {0} | set(K["first_ok"])
    if robot == "fr3":
        assert first == set(range(Sd)), (first, K["first_ok"])
    assert (steps[reached] == 0).any() and (steps[reached] > 0).any()
    nat = K["natural"]["result"].reshape(Sd, T) == RC.REACHED
    print("%s T=%d S=%d: per seed %s reach, %d groups with a reached seed (unplaced sample: %s, %d); FIRST winners %s, "
          "FEWEST_STEPS winners %s, %d step ties" % (
              robot, T, Sd, reached.sum(axis=1), some.sum(), nat.sum(axis=1), nat.any(axis=0).sum(),
              np.bincount(_winner(comp, RS.FIRST, Sd, T)[some], minlength=Sd),
              np.bincount(_winner(comp, RS.FEWEST_STEPS, Sd, T)[some], minlength=Sd), ties.sum()))


# 1 ------------------------------------------------------------------------
@pytest.mark.parametrize("robot,T", [("fr3", 64), ("ur5e", 16), ("husky_fr3", 16), ("xls_fr3", 16),
                                     ("caster_fr3", 8)])
def test_against_the_composition(cuda, robot, T):
    """(Caster-FR3's QP shape is not compiled: the stepwise path.)"""
    Sd = 4
    K = _case(robot, cuda, T, Sd)
    _coverage(K, Sd, T, robot)
    for rule in RULES:
        ref = _gather(K["comp"], rule, Sd, T)
        for cancel in (0, 1):
            got = _seeds(K["S"], K["q3"], K["xt"], K["xdt"], rule, cancel)
            _assert_same(got, ref, msg="rule %d cancel %d" % (rule, cancel))
    # q laid out [dof][S T]; without the optional outputs: the same required ones
    ref = _gather(K["comp"], RS.FIRST, Sd, T)
    none = _seeds(K["S"], K["q3"], K["xt"], K["xdt"], "first", True, want=(), flat=True)
    assert all(none[k] is None for k in _batch.REACH_SEEDS_FIELDS)
    _assert_same(none, ref, ("seed", "result", "steps_used", "q_sol", "qdot_sol"))


# 2 ------------------------------------------------------------------------
def test_scheduling_independence(cuda):
    """T = 700, S = 3: 2 100 instances, more than the 2 048-wave grid, so waves
    take a second instance while seeds of its group are still running."""
    T, Sd = 700, 3
    S = TR._setup("fr3", cuda, T)
    goal, lo, hi = _goals(S, T)
    q3 = RS.seeds(goal, lo, hi, Sd)
    run = lambda rule, cancel: _seeds(S, q3, S["xt"], S["xdt"], rule, cancel)
    for rule in RULES:
        plain = run(rule, 0)
        again = run(rule, 1), run(rule, 1)   # two consecutive calls
        for r in again:
            _assert_same(r, plain, msg="rule %d, cancel 1 against 0" % rule)
        TR._set_fusion(S, 0)
        try:
            step = run(rule, 1)
        finally:
            TR._set_fusion(S, 1)
        _assert_same(step, plain, OUT + ("inst_result", "inst_steps"), msg="rule %d, stepwise" % rule)
        saved = plain["inst_steps"].sum() - again[0]["inst_steps"].sum()
        print("rule %d: %d of %d instances cancelled, %d of %d steps saved" % (
            rule, (again[0]["inst_result"] == RS.CANCELLED).sum(), Sd * T, saved, plain["inst_steps"].sum()))
        assert (plain["result"] == RC.REACHED).sum() > T // 2 and (plain["seed"] > 0).any()
        assert not (plain["inst_result"] == RS.CANCELLED).any()


# 3 ------------------------------------------------------------------------
def test_diagnostics(cuda):
    T, Sd = 64, 4
    K = _case("fr3", cuda, T, Sd)
    comp = K["comp"]
    res0, steps0 = comp["result"].reshape(Sd, T), comp["steps_used"].reshape(Sd, T)
    cols = np.arange(T)
    for rule in RULES:
        plain = _seeds(K["S"], K["q3"], K["xt"], K["xdt"], rule, 0)
        np.testing.assert_array_equal(plain["inst_result"], res0)
        np.testing.assert_array_equal(plain["inst_steps"], steps0)
        got = _seeds(K["S"], K["q3"], K["xt"], K["xdt"], rule, 1)
        win = _winner(comp, rule, Sd, T)
        np.testing.assert_array_equal(got["seed"], win)
        np.testing.assert_array_equal(got["inst_result"][win, cols], res0[win, cols])
        np.testing.assert_array_equal(got["inst_steps"][win, cols], steps0[win, cols])
        assert np.all(got["inst_steps"] <= steps0)
        gone = got["inst_result"] == RS.CANCELLED
        # whoever was not cancelled did what it does without cancellation
        np.testing.assert_array_equal(got["inst_result"][~gone], res0[~gone])
        np.testing.assert_array_equal(got["inst_steps"][~gone], steps0[~gone])
        s, t = np.nonzero(gone)
        assert np.all(res0[win[t], t] == RC.REACHED)   # only in groups that have their answer
        if rule == RS.FIRST:
            assert np.all(s > win[t])
        else:
            assert np.all(got["inst_steps"][s, t] >= steps0[win[t], t])
        print("rule %d: %d cancelled, steps %d against %d" % (rule, gone.sum(), got["inst_steps"].sum(), steps0.sum()))


# 4 ------------------------------------------------------------------------
@pytest.mark.parametrize("shared", [False, True])
def test_obstacle_slots(cuda, shared):
    """The four-slot scene of tests/_obstacles.py, one scene per target or one for the call."""
    O = TR._fr3_obstacles(cuda)
    T, Sd = 16, 3
    goal, lo, hi = _goals(O, T)
    q3 = RS.seeds(goal, lo, hi, Sd)
    q3[:, 1, 3] = q3[:, 0, 3]   # a tie, if the seed reaches
    xt, xdt = np.ascontiguousarray(O["xt"][:, :T]), np.ascontiguousarray(O["xdt"][:, :T])
    pose = np.ascontiguousarray(O["poses"][:, :, 5] if shared else O["poses"][:, :, :T])
    comp = _composition(O, q3, xt, xdt, obstacle_pose=pose)
    assert (comp["steps_used"] > 0).any() and (comp["result"] == RC.REACHED).any()
    for rule in RULES:
        ref = _gather(comp, rule, Sd, T)
        for cancel in (0, 1):
            got = _seeds(O, q3, xt, xdt, rule, cancel, obstacle_pose=pose)
            _assert_same(got, ref, msg="rule %d cancel %d" % (rule, cancel))
        TR._set_fusion(O, 0)
        try:
            _assert_same(_seeds(O, q3, xt, xdt, rule, 1, obstacle_pose=pose), ref, msg="stepwise, rule %d" % rule)
        finally:
            TR._set_fusion(O, 1)
    if not shared:   # (the poses matter: the slot-free model's distance stage differs)
        free = _seeds(TR._setup("fr3", cuda, 70), q3, xt, xdt, RS.FEWEST_STEPS, 1)
        assert not np.array_equal(free["dist_final"], ref["dist_final"])


# 5 ------------------------------------------------------------------------
def test_urdf_with_a_collision_mesh(cuda, tmp_path):
    """FR3 with its box primitive as a 12-triangle STL of the same size (the
    fixture of tests/test_gpu_reach.py): a hull model, the stepwise dispatch."""
    text = open(robot_path("fr3")).read()
    m = re.search(r'<box size="([^"]+)"/>', text)
    size = np.array([float(x) for x in m.group(1).split()])
    (tmp_path / "pkg" / "meshes").mkdir(parents=True)
    write_stl_ascii(tmp_path / "pkg" / "meshes" / "box.stl", box_triangles(0.5 * size).reshape(-1, 3))
    (tmp_path / "pkg" / "urdf").mkdir()
    urdf = tmp_path / "pkg" / "urdf" / "fr3_mesh.urdf"
    urdf.write_text(text[:m.start()] + '<mesh filename="package://pkg/meshes/box.stl"/>' + text[m.end():])
    rd = manipulator.RobotData(str(urdf), robot_path("fr3", "srdf"), str(tmp_path), device=cuda)
    ctrl = manipulator.RobotController(0.001, rd, solver_mode="exact")
    p, dt = TR._params(ctrl, LINK["fr3"], False)
    S = dict(robot="fr3", rd=rd, ctrl=ctrl, p=p, dt=dt, moma=False, dev=cuda)
    T, Sd = 6, 2
    _, _, xt, xdt = TR._inputs(S, T)
    goal, lo, hi = _goals(S, T)
    q3 = RS.seeds(goal, lo, hi, Sd)
    q3[:, 1, 2] = goal[:, 2]
    comp = _composition(S, q3, xt, xdt)
    assert (comp["steps_used"] > 0).any() and (comp["result"] == RC.REACHED).any()
    for rule in RULES:
        _assert_same(_seeds(S, q3, xt, xdt, rule, 1), _gather(comp, rule, Sd, T), msg="rule %d" % rule)


# 6 ------------------------------------------------------------------------
def test_one_seed_is_the_reach_entry(cuda):
    T = 64
    K = _case("fr3", cuda, T)
    q3 = np.ascontiguousarray(K["q3"][:, :1])
    ref = _composition(K["S"], q3, K["xt"], K["xdt"])
    for rule in RULES:
        for cancel in (0, 1):
            got = _seeds(K["S"], q3, K["xt"], K["xdt"], rule, cancel)
            assert not got["seed"].any()
            for k, src in INST.items():
                np.testing.assert_array_equal(got[k], ref[src], err_msg=k)
            np.testing.assert_array_equal(got["inst_result"][0], ref["result"])
            np.testing.assert_array_equal(got["inst_steps"][0], ref["steps_used"])


# 7 ------------------------------------------------------------------------
def test_error_codes(cuda):
    import torch
    S = TR._setup("fr3", cuda, 70)
    O = TR._fr3_obstacles(cuda)
    T, Sd, nv = 4, 2, 7
    a = lambda t: _batch.as_device(np.ascontiguousarray(t), cuda)
    q = a(np.tile(S["q"][:, :T], (1, Sd)))
    v = torch.zeros_like(q)
    xt, xdt = a(S["xt"][:, :T]), a(S["xdt"][:, :T])
    op = a(O["poses"][:, :, :T])
    i32 = lambda *shape: torch.full(shape, -77, dtype=torch.int32, device=cuda)
    f64 = lambda *shape: torch.full(shape, -77.0, dtype=torch.float64, device=cuda)
    outs = dict(seed=i32(T), res=i32(T), steps=i32(T), qs=f64(nv, T), vs=f64(nv, T), stl=i32(T), its=i32(T),
                err=f64(2, T), dist=f64(1 + nv, T), ires=i32(Sd * T), isteps=i32(Sd * T))
    stream = C.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    lib = _capi.lib()

    def call(model=S, obstacles=False, mode=_capi.MODE_QPIK_STEP, T=T, Sd=Sd, rule=0, cancel=1, max_steps=2, dt=0.005,
             pos_tol=POS_TOL, rot_tol=ROT_TOL, q=q, v=v, xt=xt, xdt=xdt, op=op, ld=T, **kw):
        o = dict(outs, **kw)
        p = model["ctrl"]._pb.params(LINK["fr3"], mode, np.full(6, 100.0), np.zeros(6))
        head = (model["rd"].model.handle, C.byref(p), C.c_int64(T), C.c_int(Sd), C.c_int(rule), C.c_int(cancel),
                C.c_int(max_steps), C.c_double(dt), C.c_double(pos_tol), C.c_double(rot_tol), ptr(q), ptr(v), ptr(xt),
                ptr(xdt))
        tail = tuple(ptr(o[k]) for k in ("seed", "res", "steps", "qs", "vs", "stl", "its", "err", "dist", "ires",
                                         "isteps")) + (stream,)
        if obstacles:
            return lib.drc_qpik_reach_seeds_obstacles_batch(*head, ptr(op), C.c_int64(ld), *tail)
        return lib.drc_qpik_reach_seeds_batch(*head, *tail)

    ok, bad = _capi.DRC_OK, _capi.DRC_ERR_INVALID_ARGUMENT
    assert call(Sd=0) == bad and call(Sd=-1) == bad and call(T=-1) == bad
    assert call(rule=2) == bad and call(rule=-1) == bad
    assert "DRC_SEEDS_FIRST" in lib.drc_last_error().decode()
    assert call(max_steps=2 ** 30 - 1) == bad   # (max_steps + 1) S = 2^31
    assert "2^31" in lib.drc_last_error().decode()
    assert call(T=2 ** 30, Sd=2) == bad and call(T=0x7ffffff1, Sd=1) == bad   # above the work-queue limit
    assert call(mode=_capi.MODE_QPIK) == bad and call(mode=_capi.MODE_QPIK_CUBIC) == bad
    assert "DRC_MODE_QPIK_STEP" in lib.drc_last_error().decode()
    assert call(max_steps=-1) == bad
    for x in (0.0, -1e-3, float("nan"), float("inf")):
        assert call(dt=x) == bad, x
        assert call(pos_tol=x) == bad, x
        assert call(rot_tol=x) == bad, x
    for k in ("q", "v", "xt", "xdt", "seed", "res", "steps", "qs", "vs"):
        assert call(**{k: None}) == bad, k
    assert call(model=O) == bad   # the plain entry on a model with slots
    assert "drc_qpik_reach_seeds_obstacles_batch" in lib.drc_last_error().decode()
    assert call(obstacles=True) == bad   # the obstacle entry on a model without
    assert call(model=O, obstacles=True, op=None) == bad and call(model=O, obstacles=True, ld=T - 1) == bad
    assert call(T=0) == ok and call(T=0, q=None, xt=None) == ok
    TR._sync()
    for k, t in outs.items():   # refusals (and T = 0) write nothing
        assert bool((t == -77).all()), k
    assert call() == ok and call(rule=1, cancel=0) == ok and call(max_steps=0) == ok
    assert call(**{k: None for k in ("stl", "its", "err", "dist", "ires", "isteps")}) == ok
    assert call(model=O, obstacles=True) == ok and call(model=O, obstacles=True, ld=0) == ok
    TR._sync()
    assert not bool((outs["seed"] == -77).any()) and not bool((outs["ires"] == -77).any())
    with pytest.raises(ValueError):
        S["ctrl"].QPIK_reach_seeds_batch(S["q"][:, :8], S["v"][:, :8], S["xt"][:, :T], LINK["fr3"], 2)   # no seeds
    with pytest.raises(ValueError):
        S["ctrl"].QPIK_reach_seeds_batch(S["q"][:, :8], S["v"][:, :8], S["xt"][:, :T], LINK["fr3"], 2, seeds=2,
                                         want=("q_traj",))
    TR._sync()


# 8 ------------------------------------------------------------------------
@pytest.mark.parametrize("robot,T", [("fr3", 64), ("husky_fr3", 16)])
def test_controller_entry(cuda, robot, T):
    """QPIK_reach_seeds_batch of both controllers: xdot_target None is zeros,
    w_reg None the default, and the gains are the controller's."""
    K = _case(robot, cuda, T)
    S, Sd = K["S"], 4
    c = S["ctrl"]
    kp, kv = c.Kp_task_.copy(), c.Kv_task_.copy()
    try:
        if not S["moma"]:
            c.setTaskGain(np.full(6, 100.0), np.zeros(6))
        res = c.QPIK_reach_seeds_batch(K["q3"].copy(), np.zeros_like(K["q3"]), K["xt"].copy(), LINK[robot], MAX_STEPS,
                                       dt=S["dt"],
                                       w_reg=None if S["moma"] else 0.01, rule="fewest_steps")
    finally:
        c.Kp_task_, c.Kv_task_ = kp, kv
    assert (res.REACHED, res.BUDGET, res.QP_FAILED, res.CANCELLED) == (0, 1, 2, 3)
    assert res.inst_result is None and res.inst_steps is None
    TR._sync()
    ref = _gather(K["comp"], RS.FEWEST_STEPS, Sd, T)
    for k in OUT:
        np.testing.assert_array_equal(getattr(res, k).cpu().numpy(), ref[k], err_msg=k)
