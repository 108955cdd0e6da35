"""Certified path clearance on the device (drc_clearance_certify_batch,
certify_path_batch) against the stage entry and the rule of include/drc_amd.h
in plain Python (tests/_certify.py).

The reference of the bitwise tests is _batch.stages_batch in mode QPIK with
qdot = 0, run once on every dyadic state of the paths that numpy forms
(qa + (k / 2^D) * (qb - qa), the waypoints themselves at the ends), and the
Python fold of its dist[0] / pair with M_j taken from the entry's motion_bound
(which test 2 holds against the model's weights).  The guarantee is checked
against drc_clearance_path_batch at 256 substeps.

Figures that the class conditions of test 1 rest on, from the C oracle's
distances on the CPU (FR3, three waypoints, amplitudes 0.15 / 0.4 / 1.2 / 2.0,
d_stop 0.04, max_depth 5): FREE 49 (39 of them with an evaluation at depth >=
2), BLOCKED 10, UNDECIDED 5; the test prints the device's."""
import ctypes as C

import numpy as np
import pytest

import _certify as CF
import _obstacles as OB
import oracle as O
import pyref as R
from _common import make_manipulator, make_moma, moma_step_inputs
from _mesh_io import all_mesh_fr3
from dyros_robot_controller_amd import _batch, _capi, manipulator, robot_path, workload

pytestmark = pytest.mark.gpu

FREE, BLOCKED, INVALID, UNDECIDED = CF.FREE, CF.BLOCKED, CF.INVALID, CF.UNDECIDED
FLOATS = ("t_stop", "d_min", "t_min", "d_lower")
_CACHE = {}


def _sync():
    import torch
    torch.cuda.synchronize()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _model(robot, cuda):
    """The robot's RobotData (shared, never modified)."""
    if robot not in _CACHE:
        moma = robot in ("husky_fr3", "xls_fr3", "caster_fr3")
        _CACHE[robot] = make_moma(robot, cuda) if moma else make_manipulator(robot, cuda)
    return _CACHE[robot]


# ---- numpy: the dyadic states -------------------------------------------------
def _grid(path, depth):
    """path [W][dof][B] -> [W - 1][2^depth + 1][dof][B]: the states k / 2^depth of every segment."""
    n = 2 ** depth
    out = []
    for j in range(path.shape[0] - 1):
        qa, qb = path[j], path[j + 1]
        out.append(np.stack([qa if k == 0 else (qb if k == n else qa + (k / n) * (qb - qa)) for k in range(n + 1)]))
    return np.stack(out)


# ---- device -----------------------------------------------------------------
def _stage(model, dev, states, obstacle_pose=None):
    """The stage entry on states [N][dof][B] (mode QPIK, qdot = 0): dist[0] and pair, [N][B]."""
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


def _certify(model, dev, path, d_stop, max_depth, obstacle_pose=None, motion_bound=True):
    res = _batch.clearance_certify_batch(model, _batch.as_device(np.ascontiguousarray(path), dev), d_stop=d_stop,
                                         max_depth=max_depth, obstacle_pose=obstacle_pose, motion_bound=motion_bound)
    _sync()
    out = {k: getattr(res, k).cpu().numpy() for k in CF.FIELDS}
    out["motion_bound"] = None if res.motion_bound is None else res.motion_bound.cpu().numpy()
    return out


def _dense_min(model, dev, path, obstacle_pose=None):
    res = _batch.clearance_path_batch(model, _batch.as_device(np.ascontiguousarray(path), dev), substeps=256,
                                      obstacle_pose=obstacle_pose)
    _sync()
    assert (res.result.cpu().numpy() == FREE).all()
    return res.d_min.cpu().numpy()


def _reference(model, dev, path, d_stop, max_depth, M, obstacle_pose=None):
    """The Python fold per path on one stage call over the depth-max_depth grid: (outputs, deepest evaluation)."""
    W, nv, B = path.shape
    n = 2 ** max_depth + 1
    if W > 1:
        states = _grid(path, max_depth).reshape((W - 1) * n, nv, B)
    else:
        states = path
    d, pair = _stage(model, dev, states, obstacle_pose)
    ref = {k: [] for k in CF.FIELDS}
    deepest = []
    for b in range(B):
        def dist(j, k, e):
            i = j * n + (k << (max_depth - e)) if W > 1 else 0
            return float(d[i, b]), int(pair[i, b])
        r, seen = CF.fold(dist, W, d_stop, max_depth, None if M is None else M[:, b])
        for k in CF.FIELDS:
            ref[k].append(r[k])
        deepest.append(max(e for _, _, e in seen))
    return {k: np.array(v) for k, v in ref.items()}, np.array(deepest)


def _assert_same(got, ref, msg=""):
    for k in CF.FIELDS:
        if k in FLOATS:
            np.testing.assert_array_equal(_bits(got[k]), _bits(ref[k]), err_msg="%s %s" % (k, msg))
        else:
            np.testing.assert_array_equal(got[k], ref[k], err_msg="%s %s" % (k, msg))


def _check(model, dev, path, d_stop, max_depth, obstacle_pose=None, msg=""):
    got = _certify(model, dev, path, d_stop, max_depth, obstacle_pose)
    ref, deepest = _reference(model, dev, path, d_stop, max_depth, got["motion_bound"], obstacle_pose)
    _assert_same(got, ref, msg)
    return got, deepest


# ---- the paths of tests 1 to 3 --------------------------------------------------
D_STOP, MAX_DEPTH, AMPS = 0.04, 5, (0.15, 0.4, 1.2, 2.0)


def _fr3_paths(cuda, B=64, seed=12, base_seed=7):
    rd = _model("fr3", cuda)
    lo, hi = rd.getJointPositionLimit()
    _, vel = rd.getJointVelocityLimit()
    rng = np.random.default_rng(seed)
    way = [workload.joint_states(lo, hi, vel, base_seed, B)[0]]
    amp = np.array([AMPS[b % len(AMPS)] for b in range(B)])
    for _ in range(2):
        way.append(np.clip(way[-1] + rng.uniform(-1, 1, way[0].shape) * amp, lo[:, None], hi[:, None]))
    return np.stack(way)


def _fr3_case(cuda):
    if "case" not in _CACHE:
        path = _fr3_paths(cuda)
        got, deepest = _check(_model("fr3", cuda).model, cuda, path, D_STOP, MAX_DEPTH)
        _CACHE["case"] = (path, got, deepest)
    return _CACHE["case"]


# 1 ------------------------------------------------------------------------
def test_fr3_bitwise_against_the_composition(cuda):
    path, got, deepest = _fr3_case(cuda)   # (the comparison itself is in _check)
    assert path.shape == (3, 7, 64)
    r = got["result"]
    free_deep = ((r == FREE) & (deepest >= 2)).sum()
    print("FR3 d_stop %g max_depth %d: FREE %d (%d with an evaluation at depth >= 2), BLOCKED %d, INVALID %d, "
          "UNDECIDED %d; evaluations %d, at most %d per path" % (
              D_STOP, MAX_DEPTH, (r == FREE).sum(), free_deep, (r == BLOCKED).sum(), (r == INVALID).sum(),
              (r == UNDECIDED).sum(), got["samples_used"].sum(), 2 * 2 ** MAX_DEPTH + 1))
    assert free_deep >= 8 and (r == BLOCKED).sum() >= 8 and (r == UNDECIDED).sum() >= 1
    f = r == FREE
    assert (got["seg_stop"][f] == -1).all() and (got["t_stop"][f] == -1.0).all()
    assert (got["d_lower"][f] >= D_STOP).all() and (got["d_lower"][f] <= got["d_min"][f]).all()
    assert (got["samples_used"] <= 2 * 2 ** MAX_DEPTH + 1).all() and (got["samples_used"] >= 1).all()
    u = r == UNDECIDED
    assert (got["d_min"][u] >= D_STOP).all(), "an UNDECIDED path saw no sample below d_stop"
    res = _model("fr3", cuda).certify_path_batch(path, d_stop=D_STOP, max_depth=MAX_DEPTH)   # the RobotData entry
    _sync()
    np.testing.assert_array_equal(res.result.cpu().numpy(), r)
    np.testing.assert_array_equal(_bits(res.d_lower.cpu().numpy()), _bits(got["d_lower"]))
    assert (res.FREE, res.BLOCKED, res.INVALID, res.UNDECIDED) == (0, 1, 2, 3) and res.motion_bound is None


# 2 ------------------------------------------------------------------------
@pytest.mark.parametrize("robot", ["fr3", "husky_fr3"])
def test_motion_bound_bitwise(cuda, robot):
    rd = _model(robot, cuda)
    if robot == "fr3":
        path = _fr3_paths(cuda)
    else:
        qa = moma_step_inputs(rd, robot, 3, 64, cuda)[0]
        path = np.stack([qa, qa + np.random.default_rng(11).uniform(-0.3, 0.3, qa.shape)])
    rho, wt, mask = _batch.motion_weights(rd.model)
    assert wt.shape == (path.shape[1], rd.model.n_pairs) and rho.shape == (path.shape[1], rd.model.n_geoms) and mask == 0
    got = _certify(rd.model, cuda, path, -np.inf, 0)    # every segment is started and certified at depth 0
    assert (got["result"] == FREE).all() and (got["samples_used"] == path.shape[0]).all()
    want = np.array([[CF.motion_bound(wt, np.abs(path[j + 1, :, b] - path[j, :, b])) for b in range(path.shape[2])]
                     for j in range(path.shape[0] - 1)])
    np.testing.assert_array_equal(_bits(got["motion_bound"]), _bits(want))
    assert (want > 0).all()


# 3 ------------------------------------------------------------------------
def test_guarantee_fr3(cuda):
    path, got, _ = _fr3_case(cuda)
    f = got["result"] == FREE
    dense = _dense_min(_model("fr3", cuda).model, cuda, path)
    print("FR3: %d FREE paths, min over them of (dense minimum - d_lower) %.3e" % (f.sum(), (dense - got["d_lower"])[f].min()))
    assert (got["d_lower"][f] <= dense[f] + 1e-9).all()
    assert (dense[f] >= D_STOP).all()


@pytest.mark.parametrize("robot", ["husky_fr3", "caster_fr3"])
def test_guarantee_whole_body(cuda, robot):
    """The full state: virtual joints (prismatic x, y: weight 1; yaw: the reach
    of the whole robot about the base), wheels and arm."""
    rd = _model(robot, cuda)
    B, d_stop = 64, 0.0
    qa = moma_step_inputs(rd, robot, 3, B, cuda)[0]
    path = np.stack([qa, qa + np.random.default_rng(11).uniform(-0.1, 0.1, qa.shape)])
    got, _ = _check(rd.model, cuda, path, d_stop, 6)
    f = got["result"] == FREE
    dense = _dense_min(rd.model, cuda, path)
    print("%s: FREE %d, BLOCKED %d, UNDECIDED %d of %d; min (dense minimum - d_lower) %.3e; mean evaluations %.1f" % (
        robot, f.sum(), (got["result"] == BLOCKED).sum(), (got["result"] == UNDECIDED).sum(), B,
        (dense - got["d_lower"])[f].min() if f.any() else np.nan, got["samples_used"].mean()))
    assert f.sum() >= 8
    assert (got["d_lower"][f] <= dense[f] + 1e-9).all()
    assert (dense[f] >= d_stop).all()


# 4 ------------------------------------------------------------------------
PLATE_TYPES, PLATE_PARAMS = (OB.BOX,), ((0.15, 0.15, 0.002),)


def _tunnel_edges(want=8, delta=0.3, trials=400):
    """Edges qa -> qb of the FR3 and a thin plate each, chosen with the oracle
    twin: the plate stands in the way of one of the last three geometries, its
    normal along that geometry's displacement, so the ends lie on either side;
    the midpoint state penetrates it and both ends are more than 0.02 away."""
    pm, om, _, first = OB.twin("fr3", PLATE_TYPES, PLATE_PARAMS)
    om0 = O.load("fr3")[1]
    lo, hi, vel = np.asarray(pm.lower), np.asarray(pm.upper), np.asarray(pm.vel)
    rng = np.random.default_rng(5)
    q0 = workload.joint_states(lo, hi, vel, 7, trials)[0]
    edges = []
    for n in range(trials):
        qm = q0[:, n]
        u = rng.normal(size=7)
        u /= np.linalg.norm(u)
        qa, qb = qm - delta * u, qm + delta * u
        if (qa < lo).any() or (qa > hi).any() or (qb < lo).any() or (qb > hi).any():
            continue
        g = len(pm.geoms) - 1 - int(rng.integers(0, 3))
        ca, cm, cb = (R.geom_poses(pm, R.fk(pm, q))[g][:3, 3] for q in (qa, qm, qb))
        nz = (cb - ca) / np.linalg.norm(cb - ca)
        ex = np.cross(nz, [0.3, 0.5, 0.8])
        ex /= np.linalg.norm(ex)
        pose = OB.pack_poses(np.stack([ex, np.cross(nz, ex), nz], axis=1), cm)
        if O.min_distance(om0, np.ascontiguousarray(qm))[0] < 0.02:
            continue   # (the robot's own pairs are not what is tested)
        if not (nz @ (ca - cm) < -0.02 and nz @ (cb - cm) > 0.02):
            continue
        OB.set_poses(om, first, PLATE_TYPES, [pose])
        d = [O.min_distance(om, np.ascontiguousarray(q))[0] for q in (qa, qm, qb)]
        if d[1] < 0 and d[0] > 0.02 and d[2] > 0.02:
            edges.append((qa, qb, pose))
            if len(edges) == want:
                break
    return edges


def test_tunnelling(cuda):
    edges = _tunnel_edges()
    assert len(edges) == 8
    rd = make_manipulator("fr3", cuda)
    rd.set_obstacles(PLATE_TYPES, PLATE_PARAMS)
    path = np.ascontiguousarray(np.stack([np.stack([e[0] for e in edges], axis=1), np.stack([e[1] for e in edges], axis=1)]))
    pose = OB.to_field_major(np.stack([e[2][None] for e in edges]))
    sampled = _batch.clearance_path_batch(rd.model, _batch.as_device(path, cuda), substeps=1, d_stop=0.0,
                                          obstacle_pose=pose)
    _sync()
    assert (sampled.result.cpu().numpy() == FREE).all() and (sampled.d_min.cpu().numpy() > 0.02 - 1e-6).all()
    got, _ = _check(rd.model, cuda, path, 0.0, 8, obstacle_pose=pose)
    assert (got["result"] == BLOCKED).all() and (got["seg_stop"] == 0).all()
    assert ((got["t_stop"] > 0) & (got["t_stop"] < 1)).all() and (got["d_min"] < 0).all()
    # the stage entry at the stop state
    t = got["t_stop"]
    stop = path[0] + t * (path[1] - path[0])
    d, pair = _stage(rd.model, cuda, stop[None], pose)
    np.testing.assert_array_equal(_bits(d[0]), _bits(got["d_min"]))
    assert (d[0] < 0).all() and (pair[0] >= _model("fr3", cuda).model.n_pairs).all(), "not the plate's pair"
    print("tunnelling: stops at t = %s after %s evaluations" % (t, got["samples_used"]))


# 5 ------------------------------------------------------------------------
def _fr3_obstacles(cuda):
    if "obst" not in _CACHE:
        rd = make_manipulator("fr3", cuda)
        rd.set_obstacles(OB.FOUR_TYPES, OB.FOUR_PARAMS, OB.FR3_ARM_LINKS)
        _CACHE["obst"] = (rd, OB.to_field_major(OB.fr3_scene(11, 64)))
    return _CACHE["obst"]


@pytest.mark.parametrize("shared", [False, True])
def test_obstacle_slots(cuda, shared):
    path = _fr3_paths(cuda)
    rd, poses = _fr3_obstacles(cuda)
    pose = np.ascontiguousarray(poses[:, :, 5]) if shared else poses
    got, _ = _check(rd.model, cuda, path, D_STOP, 4, obstacle_pose=pose,
                    msg="one scene" if shared else "a scene per path")
    r = got["result"]
    print("FR3 + four obstacles, %s: FREE %d, BLOCKED %d, UNDECIDED %d" % (
        "one scene" if shared else "a scene per path", (r == FREE).sum(), (r == BLOCKED).sum(), (r == UNDECIDED).sum()))
    assert (r == FREE).any() and (r == BLOCKED).any()
    if not shared:
        assert (got["pair_min"] >= _model("fr3", cuda).model.n_pairs).any(), "no obstacle pair ever the closest"
    f = r == FREE
    dense = _dense_min(rd.model, cuda, path, pose)
    assert (got["d_lower"][f] <= dense[f] + 1e-9).all() and (dense[f] >= D_STOP).all()


def test_hull_model(cuda, tmp_path):
    urdf, hulls, pairs = all_mesh_fr3(tmp_path)
    rd = manipulator.RobotData(urdf, robot_path("fr3", "srdf"), device=cuda)
    path = np.ascontiguousarray(_fr3_paths(cuda)[:, :, :32])
    got, _ = _check(rd.model, cuda, path, 0.0, 4)
    r = got["result"]
    print("all-hull FR3: FREE %d, BLOCKED %d, UNDECIDED %d" % ((r == FREE).sum(), (r == BLOCKED).sum(), (r == UNDECIDED).sum()))
    assert (r == FREE).any() and (r != FREE).any()


def test_one_waypoint_depth_0_and_one_path(cuda):
    model = _model("fr3", cuda).model
    path = _fr3_paths(cuda)
    # one waypoint: its one state, no segment
    got = _certify(model, cuda, path[:1], D_STOP, MAX_DEPTH, motion_bound=False)
    d, pair = _stage(model, cuda, path[:1])
    below = d[0] < D_STOP
    assert below.any() and (~below).any()
    np.testing.assert_array_equal(got["result"], np.where(below, BLOCKED, FREE))
    np.testing.assert_array_equal(_bits(got["d_min"]), _bits(d[0]))
    np.testing.assert_array_equal(got["pair_min"], pair[0])
    assert (got["samples_used"] == 1).all() and np.isinf(got["d_lower"]).all()
    assert (got["seg_stop"] == np.where(below, 0, -1)).all() and (got["t_stop"] == np.where(below, 0.0, -1.0)).all()
    ref, _ = _reference(model, cuda, path[:1], D_STOP, MAX_DEPTH, None)
    _assert_same(got, ref, "one waypoint")
    # max_depth 0: a segment is certified whole or not at all
    got, deepest = _check(model, cuda, path, D_STOP, 0)
    assert (deepest == 0).all() and (got["samples_used"] <= 3).all()
    assert (got["result"] == UNDECIDED).any() and (got["result"] == FREE).any()
    # B = 1
    whole = _fr3_case(cuda)[1]
    for b in (3, 9):
        one, _ = _check(model, cuda, np.ascontiguousarray(path[:, :, b:b + 1]), D_STOP, MAX_DEPTH)
        for k in CF.FIELDS:
            assert _bits(one[k].astype(np.float64))[0] == _bits(whole[k].astype(np.float64))[b], (k, b)


def test_queue_of_2100_paths(cuda):
    """More paths than one round of the grid's waves on some machines, and no multiple of anything."""
    B = 2100
    path = _fr3_paths(cuda, B=B, seed=22, base_seed=21)
    got, _ = _check(_model("fr3", cuda).model, cuda, path, D_STOP, 3)
    r = got["result"]
    assert min((r == FREE).sum(), (r == BLOCKED).sum(), (r == UNDECIDED).sum()) >= 20


def test_entries_against_the_wrong_model(cuda):
    import torch
    rd, poses = _fr3_obstacles(cuda)
    plain = _model("fr3", cuda)
    path = _batch.as_device(np.ascontiguousarray(_fr3_paths(cuda)), cuda)
    with pytest.raises(_capi.DrcError) as e:
        _batch.clearance_certify_batch(rd.model, path)   # the plain entry on a model with slots
    assert e.value.code == _capi.DRC_ERR_INVALID_ARGUMENT and "drc_clearance_certify_obstacles_batch" in str(e.value)
    B = path.shape[2]
    i32 = lambda: torch.empty(B, dtype=torch.int32, device=cuda)
    f64 = lambda: torch.empty(B, dtype=torch.float64, device=cuda)
    out = (i32(), i32(), f64(), f64(), i32(), f64(), i32(), f64(), i32())
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    op = _batch.as_device(poses, cuda)

    def call(op=op, ld=B, model=rd.model):
        return _capi.lib().drc_clearance_certify_obstacles_batch(
            model.handle, C.c_int64(B), C.c_int(3), C.c_double(0.05), C.c_int(2), ptr(path), ptr(op), C.c_int64(ld),
            *[ptr(t) for t in out], None, C.c_void_p(torch.cuda.current_stream(cuda).cuda_stream))
    bad = _capi.DRC_ERR_INVALID_ARGUMENT
    assert call() == _capi.DRC_OK and call(ld=B + 3) == _capi.DRC_OK
    assert call(op=None) == bad and call(ld=B - 1) == bad   # poses need to be there, a column per path
    assert call(model=plain.model) == bad                   # the obstacle entry on a model without slots
    assert "drc_clearance_certify_batch runs it" in _capi.lib().drc_last_error().decode()
    _sync()


def test_argument_errors(cuda):
    import torch
    model = _model("fr3", cuda).model
    B = 4
    path = _batch.as_device(np.ascontiguousarray(_fr3_paths(cuda)[:, :, :B]), cuda)
    i32 = lambda: torch.empty(B, dtype=torch.int32, device=cuda)
    f64 = lambda: torch.empty(B, dtype=torch.float64, device=cuda)
    names = ("res", "sstop", "tstop", "dmin", "smin", "tmin", "pmin", "dlow", "used")
    outs = dict(zip(names, (i32(), i32(), f64(), f64(), i32(), f64(), i32(), f64(), i32())))
    mb = torch.empty((2, B), dtype=torch.float64, device=cuda)
    stream = C.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    lib = _capi.lib()

    def call(B=B, W=3, d_stop=0.05, depth=2, path=path, mb=mb, model=model.handle, **kw):
        o = dict(outs, **kw)
        return lib.drc_clearance_certify_batch(model, C.c_int64(B), C.c_int(W), C.c_double(d_stop), C.c_int(depth),
                                               ptr(path), *[ptr(o[k]) for k in names], ptr(mb), stream)
    ok, bad = _capi.DRC_OK, _capi.DRC_ERR_INVALID_ARGUMENT
    assert call() == ok and call(mb=None) == ok
    assert call(W=0) == bad and call(W=-1) == bad and call(W=1) == ok
    assert call(depth=-1) == bad and call(depth=21) == bad
    assert "max_depth" in lib.drc_last_error().decode()
    assert call(depth=0) == ok and call(depth=20, W=1) == ok
    assert call(d_stop=float("nan")) == bad
    assert "NaN" in lib.drc_last_error().decode()
    assert call(d_stop=float("inf")) == ok and call(d_stop=-float("inf")) == ok
    assert call(W=2049, depth=20) == bad         # 2048 * 2^20 + 1 = 2^31 + 1 evaluations
    assert "31 bits" in lib.drc_last_error().decode()
    assert call(B=0x7ffffff1) == bad and call(B=2 ** 40) == bad   # above the work-queue limit
    assert "batch too large" in lib.drc_last_error().decode()
    assert call(B=-1) == bad
    assert call(path=None) == bad
    for k in names:
        assert call(**{k: None}) == bad, k
    assert call(model=None) == bad
    assert call(B=0) == ok and call(B=0, path=None, res=None) == ok
    _sync()
    with pytest.raises(ValueError):
        _batch.clearance_certify_batch(model, path[0])                      # not [waypoints][dof][B]
    with pytest.raises(ValueError):
        _batch.clearance_certify_batch(model, path, motion_bound=mb[:1])    # motion_bound is [waypoints - 1 = 2][B]
    assert lib.drc_model_motion_weights(None, None, None, None) == bad
    assert lib.drc_model_motion_weights(model.handle, None, None, None) == ok
