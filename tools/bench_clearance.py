#!/usr/bin/env python3
"""Path clearance (drc_clearance_path_batch), ms per call on FR3 and Husky-FR3
against what a caller could do before it existed:
  compose    drc_qpik_stages_batch on the N B materialised sample states -- only
             dist and pair asked for, outputs allocated once, the states formed
             outside the timed region -- then the fold in torch (first sample
             below d_stop, minimum and argmin up to it, the pair gathered);
  clearance  one drc_clearance_path_batch call on the [2][dof][B] edges.
Edges: FR3 from the benchmark's joint states (seed 7) to clip(qa + U(-1.5, 1.5));
Husky-FR3 from its whole-body states to qa + U(-0.3, 0.3) on every coordinate;
`substeps` 8, d_stop -inf (the whole profile) and 0.08.  The two alternate for
--rounds rounds, the median round is reported (tools/bench_reach.py's method),
with the mean number of samples the entry evaluated.

--sweep: the kernel's grid (DRC_GRID_CLEAR 1 024 / 2 048 / 3 072) on FR3, --B
paths (65 536), substeps 8, no stop, for every library of --libs: the register
budget is a build (-DDRC_CLEAR_WAVES=3), so its A/B is this sweep on two
libraries.  The knob is read once per process, so every measurement is a child
process of this tool; the configurations alternate.  A row is kept only if the
library reports (drc_debug_clearance_grid) that it launched the grid asked for.

Information for DESIGN.md "Path clearance" and the defaults in call_plan.hpp /
clearance_kernel.hip, not a gate.  Prints one JSON line.

  python tools/bench_clearance.py [--sweep [--libs a.so,b.so] [--B 65536]] [--batches 4096,65536] [--reps 5] [--warmup 2] [--rounds 3]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

SUB = 8
D_STOPS = (("none", float("-inf")), ("0.08", 0.08))


def setup(robot, B, dev):
    """(rd, path [2][dof][B] on the device)."""
    import numpy as np
    from _common import make_manipulator, make_moma
    from dyros_robot_controller_amd import _batch, workload
    if robot == "fr3":
        rd = make_manipulator(robot, dev)
        lo, hi = rd.getJointPositionLimit()
        _, vel = rd.getJointVelocityLimit()
        qa = workload.joint_states(lo, hi, vel, 7, B)[0]
        qb = np.clip(qa + np.random.default_rng(11).uniform(-1.5, 1.5, qa.shape), lo[:, None], hi[:, None])
    else:
        rd = make_moma(robot, dev)
        lo, hi = rd.get_joint_position_limit()
        _, vel = rd.get_joint_velocity_limit()
        ji = rd.get_joint_index()
        qa = workload.mobile_states(lo, hi, vel, (ji.virtual_start, ji.mani_start, ji.mobi_start),
                                    rd.get_manipulator_dof(), rd.get_mobile_dof(), 7, B)[0]
        qb = qa + np.random.default_rng(11).uniform(-0.3, 0.3, qa.shape)
    return rd, _batch.as_device(np.ascontiguousarray(np.stack([qa, qb])), dev)


def child(args):
    """One measurement in this process: ms per clearance call."""
    import torch
    from bench import timed_steps
    from dyros_robot_controller_amd import _batch, _capi
    dev = torch.device("cuda", 0)
    rd, path = setup(args.robot, args.B, dev)
    fn = lambda: _batch.clearance_path_batch(rd.model, path, substeps=SUB, d_stop=None)
    ms = 1e3 * timed_steps(torch, fn, args.reps, args.warmup)
    print(json.dumps({"ms": ms, "grid": _batch.clearance_grid(rd.model), "build": _capi.build_id()}))


def sweep(args):
    """(library, grid) configurations, alternating; every row carries the grid
    and the build id that the child's library reported."""
    libs = args.libs.split(",")
    configs = [(lib, grid) for lib in libs for grid in (1024, 2048, 3072)]
    runs = {c: [] for c in configs}
    seen = {}
    for _ in range(args.rounds):   # the configurations alternate, so drift of the box hits all alike
        for lib, grid in configs:
            env = dict(os.environ, DRC_GRID_CLEAR=str(grid), DRC_AMD_LIB=lib)
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--robot", "fr3", "--B",
                                  str(args.B), "--reps", str(args.reps), "--warmup", str(args.warmup)], env=env,
                                 check=True, capture_output=True, text=True, timeout=600).stdout
            r = json.loads(out.strip().splitlines()[-1])
            if r["grid"] != min(grid, args.B):
                raise SystemExit("%s launched %d waves with DRC_GRID_CLEAR=%d" % (lib, r["grid"], grid))
            runs[(lib, grid)].append(r["ms"])
            seen[lib] = r["build"]
    rows = [{"library": lib, "build": seen[lib], "grid": min(grid, args.B), "ms": sorted(t)[len(t) // 2],
             "runs": [round(x, 4) for x in t]} for (lib, grid), t in runs.items()]
    print(json.dumps({"metric": "ms per clearance call", "robot": "fr3", "B": args.B, "substeps": SUB, "d_stop": "none",
                      "reps": args.reps, "rounds": args.rounds, "sweep": rows}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--libs", default=os.environ.get("DRC_AMD_LIB", "libdrc_amd.so"),
                    help="--sweep: the libraries to sweep, comma-separated (names under the package)")
    ap.add_argument("--robot", default="fr3")
    ap.add_argument("--B", type=int, default=65536)
    ap.add_argument("--batches", default="4096,65536")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    if args.child:
        return child(args)
    if args.sweep:
        return sweep(args)
    import ctypes as C
    import torch
    from bench import timed_steps
    from dyros_robot_controller_amd import _batch, _capi, manipulator

    dev = torch.device("cuda", 0)
    N = SUB + 1
    line = {"metric": "ms per call", "substeps": SUB, "samples": N, "reps": args.reps, "rounds": args.rounds,
            "build": _capi.build_id(), "robots": {}}
    for robot in ("fr3", "husky_fr3"):
        rows = {}
        for B in (int(b) for b in args.batches.split(",")):
            rd, path = setup(robot, B, dev)
            model, nv = rd.model, rd.model.dof
            p = manipulator.QPIKParamsBuilder(model, exact=True).params_no_frame(_capi.MODE_QPIK)
            t = (torch.arange(N, device=dev, dtype=torch.float64) / SUB).view(N, 1, 1)
            states = path[0] + t * (path[1] - path[0])
            states[N - 1] = path[1]
            q = states.permute(1, 0, 2).reshape(nv, N * B).contiguous()   # column n B + b
            qd, xdt = torch.zeros_like(q), torch.zeros((6, N * B), dtype=torch.float64, device=dev)
            dist = torch.empty((1 + nv, N * B), dtype=torch.float64, device=dev)
            pair = torch.empty(N * B, dtype=torch.int32, device=dev)
            ptr = lambda x: C.c_void_p(x.data_ptr())
            idx = torch.arange(N, device=dev).view(N, 1)
            row = {}
            for name, d_stop in D_STOPS:
                def compose():
                    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
                    _capi.check(_capi.lib().drc_qpik_stages_batch(
                        model.handle, C.byref(p), C.c_int64(N * B), ptr(q), ptr(qd), None, ptr(xdt), None, None,
                        None, None, None, ptr(dist), ptr(pair), None, stream))
                    d = dist[0].view(N, B)
                    below = d < d_stop
                    blocked = below.any(dim=0)
                    stop = torch.where(blocked, below.to(torch.int8).argmax(dim=0), torch.full_like(blocked, -1, dtype=torch.int64))
                    last = torch.where(blocked, stop, torch.full_like(stop, N - 1))
                    d_min, s_min = d.masked_fill(idx > last, float("inf")).min(dim=0)
                    return blocked, stop, d_min, s_min, pair.view(N, B).gather(0, s_min.view(1, B))
                clear = lambda: _batch.clearance_path_batch(model, path, substeps=SUB, d_stop=d_stop)
                runs = {"compose": [], "clearance": []}
                for _ in range(args.rounds):
                    for k, fn in (("compose", compose), ("clearance", clear)):
                        runs[k].append(1e3 * timed_steps(torch, fn, args.reps, args.warmup))
                res = clear()
                grid = _batch.clearance_grid(model)   # what the library launched
                blocked, stop, d_min, _, _ = compose()
                torch.cuda.synchronize()
                assert torch.equal(res.d_min, d_min) and torch.equal(res.sample_stop.long(), stop), "the two disagree"
                ev = torch.where(res.sample_stop < 0, torch.full_like(res.sample_stop, N), res.sample_stop + 1)
                row[name] = {k: sorted(v)[len(v) // 2] for k, v in runs.items()}
                row[name]["runs"] = {k: [round(x, 4) for x in v] for k, v in runs.items()}
                row[name]["mean_samples_evaluated"] = float(ev.double().mean())
                row[name]["blocked_share"] = float(blocked.double().mean())
                row[name]["grid"] = grid
            rows[str(B)] = row
        line["robots"][robot] = rows
    print(json.dumps(line))


if __name__ == "__main__":
    main()
