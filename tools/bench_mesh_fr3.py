#!/usr/bin/env python3
"""QPIKStep throughput of an all-mesh FR3 (every link's collision primitives
replaced by one convex hull of <= 24 vertices, tests/_mesh_io.py
all_mesh_fr3), next to the primitive FR3 on the same inputs.  Information for
DESIGN.md "Measured", not a gate.  Prints one JSON line.

  python tools/bench_mesh_fr3.py [--batch 16384] [--steps 20] [--warmup 5]"""
import argparse
import json
import os
import pathlib
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16384)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    import torch
    from bench import make_inputs, timed_steps  # the benchmark's own inputs and timing helper
    from _mesh_io import all_mesh_fr3
    from dyros_robot_controller_amd import manipulator, robot_path

    dev = torch.device("cuda", 0)
    prim = manipulator.RobotData(robot_path("fr3"), robot_path("fr3", "srdf"), device=dev)
    with tempfile.TemporaryDirectory() as tmp:
        urdf, hulls, pairs = all_mesh_fr3(pathlib.Path(tmp))
        mesh = manipulator.RobotData(urdf, robot_path("fr3", "srdf"), device=dev)
    _, (dq, dqd, dxt, dxdt), _ = make_inputs(prim, "fr3", args.batch, 12345, 0, dev)
    line = {"metric": "QPIKStep solves/s, FR3 with convex-hull collision geometry", "batch": args.batch,
            "hulls": len(hulls), "vertices": sum(len(h) for h in hulls.values()), "pairs": len(pairs)}
    for name, rd in (("primitive", prim), ("all_mesh", mesh)):
        ctrl = manipulator.RobotController(0.001, rd, solver_mode="exact")
        s = timed_steps(torch, lambda: ctrl.QPIK_step_batch(dq, dqd, dxt, dxdt, "fr3_link8"), args.steps, args.warmup)
        line[name + "_solves_per_s"] = args.batch / s
        line[name + "_ms_per_call"] = 1e3 * s
    print(json.dumps(line))


if __name__ == "__main__":
    main()
