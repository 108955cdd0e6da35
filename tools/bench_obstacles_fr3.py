#!/usr/bin/env python3
"""QPIKStep throughput of FR3 with four obstacle slots (a sphere, a box, a
cylinder and a half-space on the links moved by joint 3 and beyond; the
scene of tests/test_gpu_obstacles.py) next to the slot-free FR3 on the same
stress-tier inputs: once with a pose set per instance, once with one set
shared by the batch.  Information for DESIGN.md "Measured", not a gate.
Prints one JSON line per batch size.

  python tools/bench_obstacles_fr3.py [--batch 16384 65536] [--steps 20] [--warmup 5]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[16384, 65536])   # fused, pipeline
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    import numpy as np
    import torch
    from bench import make_inputs, timed_steps  # the benchmark's own inputs and timing helper
    import _obstacles as OB
    from dyros_robot_controller_amd import _batch, manipulator, robot_path

    dev = torch.device("cuda", 0)
    plain = manipulator.RobotData(robot_path("fr3"), robot_path("fr3", "srdf"), device=dev)
    slots = manipulator.RobotData(robot_path("fr3"), robot_path("fr3", "srdf"), device=dev)
    slots.set_obstacles(OB.FOUR_TYPES, OB.FOUR_PARAMS, OB.FR3_ARM_LINKS)
    c0 = manipulator.RobotController(0.001, plain, solver_mode="exact")
    c1 = manipulator.RobotController(0.001, slots, solver_mode="exact")
    for B in args.batch:
        _, (dq, dqd, dxt, dxdt), _ = make_inputs(plain, "fr3", B, 12345, 0, dev)
        poses = OB.fr3_scene(11, B)
        per = _batch.as_device(OB.to_field_major(poses), dev)
        shared = _batch.as_device(np.ascontiguousarray(poses[0]), dev)
        line = {"metric": "QPIKStep solves/s, FR3 with four obstacle slots", "batch": B,
                "geoms": slots.model.n_geoms, "pairs": slots.model.n_pairs}
        runs = (("slot_free", lambda: c0.QPIK_step_batch(dq, dqd, dxt, dxdt, "fr3_link8")),
                ("per_instance_poses", lambda: c1.QPIK_step_batch(dq, dqd, dxt, dxdt, "fr3_link8", obstacle_pose=per)),
                ("shared_poses", lambda: c1.QPIK_step_batch(dq, dqd, dxt, dxdt, "fr3_link8", obstacle_pose=shared)))
        for name, fn in runs:
            s = timed_steps(torch, fn, args.steps, args.warmup)
            line[name + "_solves_per_s"] = B / s
            line[name + "_ms_per_call"] = 1e3 * s
            out, status = fn()
            torch.cuda.synchronize()
            line[name + "_non_solved"] = int((status != 1).sum().item())
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
