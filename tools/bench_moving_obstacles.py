#!/usr/bin/env python3
"""Cost of the obstacle twists (drc_qpik_moving_obstacles_batch), ms per call
on FR3 with the four obstacle slots of tests/_obstacles.py, exact mode,
QPIKStep on the workload inputs with per-instance poses (fr3_scene) and twists
(uniform in [-1, 1]):
  obstacles  drc_qpik_obstacles_batch: the obstacle builds, no twist;
  moving     drc_qpik_moving_obstacles_batch with a twist per slot and instance:
             the rate builds (task_stage.hpp RATE).
The two alternate within each round; the figure is the median of the rounds.
Information for DESIGN.md "Moving obstacles", not a gate.  Prints one JSON line.

  python tools/bench_moving_obstacles.py [--batches 4096,65536] [--reps 20] [--warmup 5] [--rounds 3]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="4096,65536")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    import numpy as np
    import torch
    from bench import timed_steps  # the benchmark's own timing helper
    import _obstacles as OB
    from _common import LINK, make_manipulator, step_inputs
    from dyros_robot_controller_amd import _batch, _capi, manipulator

    dev = torch.device("cuda", 0)
    a = lambda t: _batch.as_device(t, dev)
    rd0 = make_manipulator("fr3", dev)
    rd = make_manipulator("fr3", dev)
    rd.set_obstacles(OB.FOUR_TYPES, OB.FOUR_PARAMS, OB.FR3_ARM_LINKS)
    ctrl = manipulator.RobotController(0.001, rd, solver_mode="exact")
    p = ctrl._pb.params(LINK["fr3"], _capi.MODE_QPIK_STEP, ctrl.Kp_task_, ctrl.Kv_task_, 0.0, 0.0, 1.0)
    line = {"metric": "ms per call, FR3 with four obstacle slots, exact mode", "reps": args.reps, "warmup": args.warmup,
            "rounds": args.rounds, "build": _capi.build_id(), "batches": {}}
    for B in (int(b) for b in args.batches.split(",")):
        q, qd, xt, xdt = (a(v) for v in step_inputs(rd0, "fr3", 3, B, dev))
        pose = a(OB.to_field_major(OB.fr3_scene(11, B)))
        twist = a(OB.to_field_major(np.random.default_rng(77).uniform(-1, 1, (B, 4, 6))))
        out = torch.empty((7, B), dtype=torch.float64, device=dev)
        status = torch.empty(B, dtype=torch.int32, device=dev)
        paths = (("obstacles", lambda: _batch.qpik_batch(rd.model, p, q, qd, xt, xdt, out=out, status=status,
                                                         obstacle_pose=pose)),
                 ("moving", lambda: _batch.qpik_batch(rd.model, p, q, qd, xt, xdt, out=out, status=status,
                                                      obstacle_pose=pose, obstacle_twist=twist)))
        runs = {name: [] for name, _ in paths}
        for _ in range(args.rounds):
            for name, fn in paths:
                runs[name].append(1e3 * timed_steps(torch, fn, args.reps, args.warmup))
        row = {name: sorted(t)[len(t) // 2] for name, t in runs.items()}
        row["runs"] = {name: [round(x, 4) for x in t] for name, t in runs.items()}
        line["batches"][str(B)] = row
        print("B=%d %s" % (B, row["runs"]), file=sys.stderr)
    print(json.dumps(line))


if __name__ == "__main__":
    main()
