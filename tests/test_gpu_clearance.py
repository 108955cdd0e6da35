"""Path clearance on the device (drc_clearance_path_batch,
min_distance_path_batch) against the stage entry and the rule of
include/drc_amd.h in numpy.

The reference of every test is _batch.stages_batch in mode QPIK with qdot = 0,
run once on the sample states that numpy forms
(qa + (i / substeps) * (qb - qa); the waypoint itself for i == substeps), and
the fold of its dist[0] / pair by the rule as the header states it (_fold).  The
contract is bitwise: profile, minimum, argmin, pair, verdict and stop.  The
per-sample pair is read back through one-sample paths (waypoints = 1, where
pair_min is the sample's pair).  A stop is checked two ways: the outputs equal
the fold of the full profile, and the entries of dist_traj past the stop still
hold the sentinel they were filled with -- a build that evaluates past a stop,
or folds in another order, fails.

Figures of the device run that the conditions on the three classes (never
below d_stop / below at sample 0 / first below at a later sample) rest on are
printed by the tests; on the C oracle and on the device alike: FR3 d_stop 0.08:
48 / 8 / 8, UR5e d_stop 0.02: 36 / 19 / 9."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import _obstacles as OB
import oracle as O
from _common import LINK, make_manipulator, make_moma, moma_step_inputs
from _mesh_io import all_mesh_fr3
from dyros_robot_controller_amd import _batch, _capi, manipulator, robot_path, workload

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FREE, BLOCKED, INVALID = 0, 1, 2
SENTINEL = -777.25
FIELDS = ("result", "sample_stop", "d_min", "sample_min", "pair_min")
_CACHE = {}


def _sync():
    import torch
    torch.cuda.synchronize()


# ---- numpy: the sample states and the rule ---------------------------------------
def _samples(path, sub):
    """path [W][dof][B] -> the sample states [N][dof][B]."""
    out = [path[0]]
    for j in range(path.shape[0] - 1):
        qa, qb = path[j], path[j + 1]
        for i in range(1, sub + 1):
            out.append(qb if i == sub else qa + (i / sub) * (qb - qa))
    return np.stack(out)


def _fold(d, pair, d_stop):
    """The rule on a profile d, pair [N][B]: the five outputs and evaluated [N][B]."""
    N, B = d.shape
    r = dict(result=np.zeros(B, np.int32), sample_stop=np.full(B, -1, np.int32), d_min=np.full(B, np.inf),
             sample_min=np.full(B, -1, np.int32), pair_min=np.full(B, -1, np.int32))
    seen = np.zeros((N, B), bool)
    for b in range(B):
        for n in range(N):
            seen[n, b] = True
            x = d[n, b]
            if x != x:
                r["result"][b], r["sample_stop"][b] = INVALID, n
                break
            if x < r["d_min"][b]:
                r["d_min"][b], r["sample_min"][b], r["pair_min"][b] = x, n, pair[n, b]
            if x < d_stop:
                r["result"][b], r["sample_stop"][b] = BLOCKED, n
                break
    return r, seen


def _classes(d, d_stop):
    """(never below, below at sample 0, first below at a later sample) per path."""
    below = d < d_stop
    never = ~below.any(axis=0)
    at0 = below[0]
    return never, at0, ~never & ~at0


# ---- device -----------------------------------------------------------------
def _stage(model, dev, states, obstacle_pose=None):
    """The stage entry on states [N][dof][B] (mode QPIK, qdot = 0): dist[0] and pair, [N][B].
    obstacle_pose [n][12] or [n][12][B]: the same scene at every sample of a path."""
    N, nv, B = states.shape
    q = np.ascontiguousarray(np.transpose(states, (1, 0, 2)).reshape(nv, N * B))
    p = manipulator.QPIKParamsBuilder(model, exact=True).params_no_frame(_capi.MODE_QPIK)
    a = lambda t: _batch.as_device(t, dev)
    if obstacle_pose is not None and obstacle_pose.ndim == 3:
        obstacle_pose = np.ascontiguousarray(np.tile(obstacle_pose, (1, 1, N)))
    st = _batch.stages_batch(model, p, a(q), a(np.zeros_like(q)), None, a(np.zeros((6, N * B))),
                             obstacle_pose=obstacle_pose)
    _sync()
    return st["dist"][0].cpu().numpy().reshape(N, B), st["pair"].cpu().numpy().reshape(N, B)


def _clear(model, dev, path, sub=1, d_stop=None, obstacle_pose=None, traj=True, sentinel=None):
    """The entry on path [W][dof][B]: its outputs as numpy arrays (dist_traj prefilled with `sentinel`)."""
    import torch
    W, nv, B = path.shape
    N = (W - 1) * sub + 1
    t = traj
    if traj and sentinel is not None:
        t = torch.full((N, B), sentinel, dtype=torch.float64, device=dev)
    res = _batch.clearance_path_batch(model, _batch.as_device(np.ascontiguousarray(path), dev), substeps=sub,
                                      d_stop=d_stop, obstacle_pose=obstacle_pose, dist_traj=t)
    _sync()
    out = {k: getattr(res, k).cpu().numpy() for k in FIELDS}
    out["dist_traj"] = None if res.dist_traj is None else res.dist_traj.cpu().numpy()
    return out


def _pairs(model, dev, states, obstacle_pose=None):
    """Per-sample (d, pair) [N][B] through one-sample paths."""
    N, nv, B = states.shape
    if obstacle_pose is not None and obstacle_pose.ndim == 3:
        obstacle_pose = np.ascontiguousarray(np.tile(obstacle_pose, (1, 1, N)))
    flat = np.ascontiguousarray(np.transpose(states, (1, 0, 2)).reshape(1, nv, N * B))
    r = _clear(model, dev, flat, obstacle_pose=obstacle_pose, traj=False)
    assert not r["result"].any() and not r["sample_min"].any() and (r["sample_stop"] == -1).all()
    return r["d_min"].reshape(N, B), r["pair_min"].reshape(N, B)


def _assert_fold(got, ref, msg=""):
    for k in FIELDS:
        np.testing.assert_array_equal(got[k], ref[k], err_msg="%s %s" % (k, msg))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _model(robot, cuda):
    """The robot's RobotData (shared, never modified)."""
    if robot not in _CACHE:
        moma = robot in ("husky_fr3", "xls_fr3", "caster_fr3")
        _CACHE[robot] = make_moma(robot, cuda) if moma else make_manipulator(robot, cuda)
    return _CACHE[robot]


def _edges(robot, cuda, amp, B=64):
    """The edges of a manipulator: qa the workload's states (seed 7), qb = clip(qa + U(-amp, amp))."""
    rd = _model(robot, cuda)
    lo, hi = rd.getJointPositionLimit()
    _, vel = rd.getJointVelocityLimit()
    qa = workload.joint_states(lo, hi, vel, 7, B)[0]
    qb = np.clip(qa + np.random.default_rng(11).uniform(-amp, amp, qa.shape), lo[:, None], hi[:, None])
    return np.stack([qa, qb])


def _profile(robot, cuda, amp, sub=8):
    """(path, states, d, pair) of the edges: the stage's profile, computed once."""
    key = ("profile", robot)
    if key not in _CACHE:
        path = _edges(robot, cuda, amp)
        states = _samples(path, sub)
        d, pair = _stage(_model(robot, cuda).model, cuda, states)
        _CACHE[key] = (path, states, d, pair)
    return _CACHE[key]


def _check_profile(model, cuda, path, sub, d, pair, obstacle_pose=None, free=True):
    """Test 1's checks: the whole profile, per-sample pairs and the fold, no stop."""
    states = _samples(path, sub)
    got = _clear(model, cuda, path, sub, obstacle_pose=obstacle_pose, sentinel=SENTINEL)
    np.testing.assert_array_equal(_bits(got["dist_traj"]), _bits(d))
    dd, pp = _pairs(model, cuda, states, obstacle_pose)
    np.testing.assert_array_equal(_bits(dd), _bits(d))
    np.testing.assert_array_equal(pp, pair)
    ref, seen = _fold(d, pair, -np.inf)
    assert seen.all()
    _assert_fold(got, ref)
    if free:
        assert (got["result"] == FREE).all() and (got["sample_stop"] == -1).all()
    return got


def _check_stops(model, cuda, path, sub, d, pair, d_stop, obstacle_pose=None, need=4, what=""):
    """Test 2's checks: every output equals the fold of the full profile, the
    entries past a stop keep the sentinel, and each class holds `need` paths."""
    got = _clear(model, cuda, path, sub, d_stop=d_stop, obstacle_pose=obstacle_pose, sentinel=SENTINEL)
    ref, seen = _fold(d, pair, d_stop)
    _assert_fold(got, ref, what)
    np.testing.assert_array_equal(_bits(got["dist_traj"][seen]), _bits(d[seen]))
    assert (got["dist_traj"][~seen] == SENTINEL).all(), "a sample past a stop was evaluated"
    never, at0, later = _classes(d, d_stop)
    print("%s d_stop %g: never below %d, below at sample 0 %d, first below later %d; samples evaluated %d of %d" % (
        what, d_stop, never.sum(), at0.sum(), later.sum(), seen.sum(), seen.size))
    assert min(never.sum(), at0.sum(), later.sum()) >= need, (never.sum(), at0.sum(), later.sum())
    assert (got["result"][never] == FREE).all() and (got["result"][~never] == BLOCKED).all()
    assert (got["sample_stop"][at0] == 0).all() and (got["sample_stop"][later] > 0).all()
    return got


# 1 ------------------------------------------------------------------------
def test_fr3_profile(cuda):
    path, states, d, pair = _profile("fr3", cuda, 1.5)
    assert states.shape == (9, 7, 64)
    _check_profile(_model("fr3", cuda).model, cuda, path, 8, d, pair)


# 2 ------------------------------------------------------------------------
def test_fr3_early_stop(cuda):
    path, states, d, pair = _profile("fr3", cuda, 1.5)
    _check_stops(_model("fr3", cuda).model, cuda, path, 8, d, pair, 0.08, what="FR3")


# 3 ------------------------------------------------------------------------
def test_ur5e_early_stop(cuda):
    path, states, d, pair = _profile("ur5e", cuda, 0.6)
    _check_stops(_model("ur5e", cuda).model, cuda, path, 8, d, pair, 0.02, what="UR5e")


# 4 ------------------------------------------------------------------------
@pytest.mark.parametrize("robot", ["husky_fr3", "caster_fr3"])
def test_whole_body(cuda, robot):
    """The full state -- virtual joints, wheels, arm -- interpolated coordinate by
    coordinate; Caster-FR3's QP shape is not compiled, and no QP is involved."""
    rd = _model(robot, cuda)
    B = 32
    qa = moma_step_inputs(rd, robot, 3, B, cuda)[0]
    qb = qa + np.random.default_rng(11).uniform(-0.3, 0.3, qa.shape)
    path = np.stack([qa, qb])
    d, pair = _stage(rd.model, cuda, _samples(path, 8))
    got = _check_profile(rd.model, cuda, path, 8, d, pair, free=False)
    assert np.isfinite(got["d_min"]).all() and (got["pair_min"] >= 0).all()
    res = rd.min_distance_path_batch(path, substeps=8, dist_traj=True)   # the RobotData entry
    _sync()
    np.testing.assert_array_equal(_bits(res.dist_traj.cpu().numpy()), _bits(d))
    assert (res.FREE, res.BLOCKED, res.INVALID) == (0, 1, 2)


# 5 ------------------------------------------------------------------------
def test_several_waypoints(cuda):
    rd = _model("fr3", cuda)
    model = rd.model
    lo, hi = rd.getJointPositionLimit()
    _, vel = rd.getJointVelocityLimit()
    B, W, sub = 70, 4, 3
    rng = np.random.default_rng(12)
    way = [workload.joint_states(lo, hi, vel, 7, B)[0]]
    for _ in range(W - 1):
        way.append(np.clip(way[-1] + rng.uniform(-0.8, 0.8, way[0].shape), lo[:, None], hi[:, None]))
    path = np.stack(way)
    # the three edge calls' profiles, the shared waypoints counted once
    prof = []
    for j in range(W - 1):
        e = _clear(model, cuda, path[j:j + 2], sub)
        prof.append(e["dist_traj"] if j == 0 else e["dist_traj"][1:])
    prof = np.concatenate(prof)
    assert prof.shape == ((W - 1) * sub + 1, B)
    d, pair = _stage(model, cuda, _samples(path, sub))
    np.testing.assert_array_equal(_bits(prof), _bits(d))
    for d_stop in (None, 0.08):
        got = _clear(model, cuda, path, sub, d_stop=d_stop, sentinel=SENTINEL)
        ref, seen = _fold(d, pair, -np.inf if d_stop is None else d_stop)
        _assert_fold(got, ref, "d_stop %s" % d_stop)
        np.testing.assert_array_equal(_bits(got["dist_traj"][seen]), _bits(d[seen]))
        assert (got["dist_traj"][~seen] == SENTINEL).all()
    assert (got["sample_stop"] > sub).any(), "no stop beyond the first segment"
    # waypoints = 1: one sample
    one = _clear(model, cuda, path[:1], sub, d_stop=0.08)
    assert one["dist_traj"].shape == (1, B)
    _assert_fold(one, _fold(d[:1], pair[:1], 0.08)[0])
    # substeps = 1: the waypoints themselves
    ws = _clear(model, cuda, path, 1)
    np.testing.assert_array_equal(_bits(ws["dist_traj"]), _bits(d[::sub]))
    _assert_fold(ws, _fold(d[::sub], pair[::sub], -np.inf)[0])


def test_rollout_trajectory(cuda):
    """A rollout's q_traj passed straight in: q_traj[k] = q_{k+1} and dist_traj[k]
    is taken at q_k, so the path q_traj[:-1] has the profile dist_traj[1:, 0]."""
    rd = _model("fr3", cuda)
    ctrl = manipulator.RobotController(0.001, rd, solver_mode="exact")
    B, steps = 64, 6
    lo, hi = rd.getJointPositionLimit()
    _, vel = rd.getJointVelocityLimit()
    q, qd = workload.joint_states(lo, hi, vel, 7, B)
    p = ctrl._pb.params(LINK["fr3"], _capi.MODE_QPIK, np.full(6, 100.0), np.zeros(6))
    a = lambda t: _batch.as_device(t, cuda)
    xdt = np.zeros((6, B))
    xdt[0] = 0.1
    ro = _batch.qpik_rollout_batch(rd.model, p, a(q), a(np.zeros_like(q)), steps, 0.005, None, a(xdt),
                                   want=("q_traj", "dist_traj"))
    res = _batch.clearance_path_batch(rd.model, ro.q_traj[:steps - 1].contiguous(), dist_traj=True)
    _sync()
    want = ro.dist_traj[1:, 0].cpu().numpy()
    np.testing.assert_array_equal(_bits(res.dist_traj.cpu().numpy()), _bits(want))
    np.testing.assert_array_equal(_bits(res.d_min.cpu().numpy()), _bits(want.min(axis=0)))
    np.testing.assert_array_equal(res.sample_min.cpu().numpy(), want.argmin(axis=0))
    assert (ro.q_traj[0] != ro.q_traj[steps - 1]).any().item(), "the rollout did not move"


# 6 ------------------------------------------------------------------------
@pytest.mark.parametrize("robot,amp", [("fr3", 1.5), ("ur5e", 0.6)])
def test_independent_of_the_stage(cuda, robot, amp):
    """d_min against the C oracle's min distance at the state of sample_min, at
    the stage tolerances of tests/test_gpu_parity.py: 1e-9 separated, 1e-6 penetrating."""
    path, states, d, pair = _profile(robot, cuda, amp)
    got = _clear(_model(robot, cuda).model, cuda, path, 8, traj=False)
    _, om, _ = O.load(robot)
    worst = [0.0, 0.0]
    for b in range(path.shape[2]):
        ref = O.min_distance(om, np.ascontiguousarray(states[got["sample_min"][b], :, b]))[0]
        err = abs(got["d_min"][b] - ref)
        worst[ref <= 0] = max(worst[ref <= 0], err)
        assert err <= (1e-9 if ref > 0 else 1e-6), (b, got["d_min"][b], ref)
    print("%s: max |d_min - oracle| separated %.3e, penetrating %.3e" % (robot, worst[0], worst[1]))


# 7 ------------------------------------------------------------------------
def _fr3_obstacles(cuda):
    if "obst" not in _CACHE:
        rd = make_manipulator("fr3", cuda)
        rd.set_obstacles(OB.FOUR_TYPES, OB.FOUR_PARAMS, OB.FR3_ARM_LINKS)
        _CACHE["obst"] = (rd, OB.to_field_major(OB.fr3_scene(11, 64)))
    return _CACHE["obst"]


@pytest.mark.parametrize("shared", [False, True])
def test_obstacle_slots(cuda, shared):
    path = _profile("fr3", cuda, 1.5)[0]
    rd, poses = _fr3_obstacles(cuda)
    pose = np.ascontiguousarray(poses[:, :, 5]) if shared else poses
    d, pair = _stage(rd.model, cuda, _samples(path, 8), pose)
    _check_profile(rd.model, cuda, path, 8, d, pair, obstacle_pose=pose, free=False)
    if not shared:
        assert (pair >= _model("fr3", cuda).model.n_pairs).any(), "no obstacle pair ever the closest"
    _check_stops(rd.model, cuda, path, 8, d, pair, 0.05, obstacle_pose=pose, need=1,
                 what="FR3 + four obstacles, %s" % ("one scene" if shared else "a scene per path"))


def test_obstacle_entries_against_the_model(cuda):
    import torch
    rd, poses = _fr3_obstacles(cuda)
    plain = _model("fr3", cuda)
    path = _batch.as_device(np.ascontiguousarray(_profile("fr3", cuda, 1.5)[0]), cuda)
    with pytest.raises(_capi.DrcError) as e:
        _batch.clearance_path_batch(rd.model, path)   # the plain entry on a model with slots
    assert e.value.code == _capi.DRC_ERR_INVALID_ARGUMENT and "drc_clearance_path_obstacles_batch" in str(e.value)
    B = path.shape[2]
    out = [torch.empty(B, dtype=torch.int32, device=cuda) for _ in range(2)]
    dm = torch.empty(B, dtype=torch.float64, device=cuda)
    out2 = [torch.empty(B, dtype=torch.int32, device=cuda) for _ in range(2)]
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    op = _batch.as_device(poses, cuda)

    def call(op=op, ld=B, model=rd.model):
        return _capi.lib().drc_clearance_path_obstacles_batch(
            model.handle, C.c_int64(B), C.c_int(2), C.c_int(2), C.c_double(0.05), ptr(path), ptr(op),
            C.c_int64(ld), ptr(out[0]), ptr(out[1]), ptr(dm), ptr(out2[0]), ptr(out2[1]), None,
            C.c_void_p(torch.cuda.current_stream(cuda).cuda_stream))
    bad = _capi.DRC_ERR_INVALID_ARGUMENT
    assert call() == _capi.DRC_OK and call(ld=B + 3) == _capi.DRC_OK
    assert call(op=None) == bad and call(ld=B - 1) == bad   # poses need to be there, a column per path
    assert call(model=plain.model) == bad                   # the obstacle entry on a model without slots
    assert "drc_clearance_path_batch runs it" in _capi.lib().drc_last_error().decode()
    _sync()


# 8 ------------------------------------------------------------------------
def test_hull_model(cuda, tmp_path):
    urdf, hulls, pairs = all_mesh_fr3(tmp_path)
    rd = manipulator.RobotData(urdf, robot_path("fr3", "srdf"), device=cuda)
    path = np.ascontiguousarray(_profile("fr3", cuda, 1.5)[0][:, :, :32])
    d, pair = _stage(rd.model, cuda, _samples(path, 8))
    _check_profile(rd.model, cuda, path, 8, d, pair, free=False)
    stop = float(np.median(d.min(axis=0)))   # half of the paths stop somewhere
    got = _clear(rd.model, cuda, path, 8, d_stop=stop, sentinel=SENTINEL)
    ref, seen = _fold(d, pair, stop)
    _assert_fold(got, ref)
    assert (got["dist_traj"][~seen] == SENTINEL).all() and (~seen).any() and (got["result"] == FREE).any()


# 9 ------------------------------------------------------------------------
def _queue_paths(cuda, B):
    rd = _model("fr3", cuda)
    lo, hi = rd.getJointPositionLimit()
    _, vel = rd.getJointVelocityLimit()
    qa = workload.joint_states(lo, hi, vel, 21, B)[0]
    qb = np.clip(qa + np.random.default_rng(22).uniform(-1.5, 1.5, qa.shape), lo[:, None], hi[:, None])
    return np.stack([qa, qb])


def test_one_path(cuda):
    path = np.ascontiguousarray(_profile("fr3", cuda, 1.5)[0][:, :, 9:10])
    d, pair = _stage(_model("fr3", cuda).model, cuda, _samples(path, 8))
    _check_profile(_model("fr3", cuda).model, cuda, path, 8, d, pair)


_CHILD = """
import sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1])
from dyros_robot_controller_amd import _batch, manipulator, robot_path
dev = torch.device("cuda", 0)
rd = manipulator.RobotData(robot_path("fr3"), robot_path("fr3", "srdf"), device=dev)
path = np.load(sys.argv[2])
traj = torch.full((3, path.shape[2]), -777.25, dtype=torch.float64, device=dev)
res = _batch.clearance_path_batch(rd.model, _batch.as_device(path, dev), substeps=2, d_stop=0.08, dist_traj=traj)
torch.cuda.synchronize()
np.savez(sys.argv[3], grid=_batch.clearance_grid(rd.model), **{k: getattr(res, k).cpu().numpy() for k in
                         ("result", "sample_stop", "d_min", "sample_min", "pair_min", "dist_traj")})
"""


def test_queue_and_grid(cuda, tmp_path):
    """B = 2 100 paths on the default grid (a wave per path) and on 8 waves,
    where the work queue hands each wave some 260 paths (DRC_GRID_CLEAR=8, read
    once per process: a child process, which reports the grid it launched):
    identical outputs, equal to the fold."""
    B = 2100
    path = _queue_paths(cuda, B)
    model = _model("fr3", cuda).model
    got = _clear(model, cuda, path, 2, d_stop=0.08, sentinel=SENTINEL)
    assert _batch.clearance_grid(model) == min(B, 3072), "the default grid: one wave per path up to 3 072"
    d, pair = _stage(model, cuda, _samples(path, 2))
    ref, seen = _fold(d, pair, 0.08)
    _assert_fold(got, ref)
    assert (got["dist_traj"][~seen] == SENTINEL).all() and (~seen).any()
    np.save(tmp_path / "path.npy", path)
    (tmp_path / "child.py").write_text(_CHILD)
    env = dict(os.environ, DRC_GRID_CLEAR="8")
    subprocess.run([sys.executable, str(tmp_path / "child.py"), ROOT, str(tmp_path / "path.npy"),
                    str(tmp_path / "out.npz")], check=True, env=env, timeout=300)
    small = np.load(tmp_path / "out.npz")
    assert int(small["grid"]) == 8, "the child did not launch 8 waves: DRC_GRID_CLEAR is not read"
    for k in FIELDS:
        np.testing.assert_array_equal(small[k], got[k], err_msg=k)
    np.testing.assert_array_equal(_bits(small["dist_traj"]), _bits(got["dist_traj"]))


def test_host_form(cuda):
    path = np.ascontiguousarray(_profile("fr3", cuda, 1.5)[0])
    model = _model("fr3", cuda).model
    W, nv, B = path.shape
    N = 9
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    for d_stop in (-np.inf, 0.08):
        dev = _clear(model, cuda, path, 8, d_stop=d_stop, sentinel=SENTINEL)
        ints = {k: np.full(B, -5, np.int32) for k in ("result", "sample_stop", "sample_min", "pair_min")}
        d_min = np.zeros(B)
        traj = np.full((N, B), SENTINEL)
        rc = _capi.lib().drc_clearance_path_host(
            model.handle, C.c_int64(B), C.c_int(W), C.c_int(8), C.c_double(d_stop), path.ctypes.data_as(dp),
            ints["result"].ctypes.data_as(ip), ints["sample_stop"].ctypes.data_as(ip), d_min.ctypes.data_as(dp),
            ints["sample_min"].ctypes.data_as(ip), ints["pair_min"].ctypes.data_as(ip), traj.ctypes.data_as(dp))
        assert rc == _capi.DRC_OK, _capi.lib().drc_last_error()
        for k in ints:
            np.testing.assert_array_equal(ints[k], dev[k], err_msg=k)
        np.testing.assert_array_equal(_bits(d_min), _bits(dev["d_min"]))
        np.testing.assert_array_equal(_bits(traj), _bits(dev["dist_traj"]))   # the sentinel past a stop included
    # without dist_traj
    rc = _capi.lib().drc_clearance_path_host(
        model.handle, C.c_int64(B), C.c_int(W), C.c_int(8), C.c_double(0.08), path.ctypes.data_as(dp),
        ints["result"].ctypes.data_as(ip), ints["sample_stop"].ctypes.data_as(ip), d_min.ctypes.data_as(dp),
        ints["sample_min"].ctypes.data_as(ip), ints["pair_min"].ctypes.data_as(ip), None)
    assert rc == _capi.DRC_OK
    np.testing.assert_array_equal(ints["sample_stop"], dev["sample_stop"])


# 10 -----------------------------------------------------------------------
def test_argument_errors(cuda):
    import torch
    model = _model("fr3", cuda).model
    B = 4
    path = _batch.as_device(np.ascontiguousarray(_profile("fr3", cuda, 1.5)[0][:, :, :B]), cuda)
    i32 = lambda: torch.empty(B, dtype=torch.int32, device=cuda)
    res, stop, smin, pmin = i32(), i32(), i32(), i32()
    dmin = torch.empty(B, dtype=torch.float64, device=cuda)
    traj = torch.empty((3, B), dtype=torch.float64, device=cuda)
    stream = C.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    lib = _capi.lib()

    def call(B=B, W=2, sub=2, d_stop=0.05, path=path, res=res, stop=stop, dmin=dmin, smin=smin, pmin=pmin, traj=traj,
             model=model.handle):
        return lib.drc_clearance_path_batch(model, C.c_int64(B), C.c_int(W), C.c_int(sub), C.c_double(d_stop),
                                            ptr(path), ptr(res), ptr(stop), ptr(dmin), ptr(smin), ptr(pmin),
                                            ptr(traj), stream)
    ok, bad = _capi.DRC_OK, _capi.DRC_ERR_INVALID_ARGUMENT
    assert call() == ok and call(traj=None) == ok
    assert call(W=0) == bad and call(W=-1) == bad and call(W=1) == ok
    assert call(sub=0) == bad and call(sub=-3) == bad
    assert call(d_stop=float("nan")) == bad
    assert "NaN" in lib.drc_last_error().decode()
    assert call(d_stop=float("inf")) == ok and call(d_stop=-float("inf")) == ok
    assert call(W=2, sub=2 ** 31 - 1) == bad          # N = 2^31
    assert call(W=3, sub=2 ** 30) == bad              # N = 2^31 + 1
    assert "31 bits" in lib.drc_last_error().decode()
    assert call(B=0x7ffffff1) == bad and call(B=2 ** 40) == bad   # above the work-queue limit
    assert "batch too large" in lib.drc_last_error().decode()
    assert call(B=-1) == bad
    for k in ("path", "res", "stop", "dmin", "smin", "pmin"):
        assert call(**{k: None}) == bad, k
    assert call(model=None) == bad
    assert call(B=0) == ok and call(B=0, path=None, res=None) == ok
    _sync()
    with pytest.raises(ValueError):
        _batch.clearance_path_batch(model, path[0])                       # not [waypoints][dof][B]
    with pytest.raises(ValueError):
        _batch.clearance_path_batch(model, path, substeps=2, dist_traj=traj[:2])   # dist_traj is [N = 3][B]
