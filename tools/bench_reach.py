#!/usr/bin/env python3
"""Goal-reaching rollouts (QPIK_reach_batch / drc_qpik_reach_batch), ms per
call on FR3 and Husky-FR3 for three ways to bring a link to a pose, on the
same census-style inputs (tests/_reach.py: a goal within 0.15 per joint of
the start, the target the stage pose at the goal; 1e-4 m, 1e-3 rad):
  rollout     the fixed horizon a caller had before: drc_qpik_rollout_batch
              with steps = max_steps, every instance pays the whole horizon;
  stepwise    drc_qpik_reach_batch's stepwise path (DRC_REACH_MAX = 0);
  persistent  its persistent kernel (DRC_REACH_MAX raised past the batch).
Manipulator: Kp 100, Kv 0, w_reg 0.01, dt 5 ms; mobile manipulator: the
defaults at dt 1 ms.  Reports the mean steps_used and the shares of the three
results next to the times.  Information for DESIGN.md "Reach" and the
persistent kernel's batch-size threshold, not a gate.  Prints one JSON line.

  python tools/bench_reach.py [--steps 32] [--batches 256,4096,16384,65536] [--reps 5] [--warmup 2] [--rounds 3]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--batches", default="256,4096,16384,65536")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    import numpy as np
    import torch
    from bench import timed_steps  # the benchmark's own timing helper
    import _reach as RC
    from _common import make_manipulator, make_moma, stage_pose
    from dyros_robot_controller_amd import _batch, _capi, manipulator, mobile_manipulator

    dev = torch.device("cuda", 0)
    K, pos_tol, rot_tol = args.steps, 1e-4, 1e-3
    batches = [int(b) for b in args.batches.split(",")]
    line = {"metric": "ms per goal-reaching call", "max_steps": K, "pos_tol": pos_tol, "rot_tol": rot_tol,
            "reps": args.reps, "rounds": args.rounds, "build": _capi.build_id(), "robots": {}}
    for robot in ("fr3", "husky_fr3"):
        moma = robot == "husky_fr3"
        rd = make_moma(robot, dev) if moma else make_manipulator(robot, dev)
        ctrl = (mobile_manipulator if moma else manipulator).RobotController(0.001, rd, solver_mode="exact")
        link = "fr3_link8"
        if moma:
            p, dt = ctrl._pb.params(link, _capi.MODE_QPIK_STEP, ctrl.Kp_task_, np.zeros(6)), 0.001
        else:
            p, dt = ctrl._pb.params(link, _capi.MODE_QPIK_STEP, np.full(6, 100.0), np.zeros(6)), 0.005
            p.w_reg = 0.01
        lo, hi = rd.get_joint_position_limit() if moma else rd.getJointPositionLimit()
        q0_all, qg_all = RC.census_states(lo, hi, max(batches))
        rows = {}
        for B in batches:
            q0, qg = np.ascontiguousarray(q0_all[:, :B]), np.ascontiguousarray(qg_all[:, :B])
            a = lambda t: _batch.as_device(t, dev)
            xt = a(stage_pose(rd.model, dev, qg, np.zeros_like(qg), link)["pose"])
            q, v, xdt = a(q0), a(np.zeros_like(q0)), a(np.zeros((6, B)))
            roll = lambda: _batch.qpik_rollout_batch(rd.model, p, q, v, K, dt, xt, xdt, want=())
            reach = lambda: _batch.qpik_reach_batch(rd.model, p, q, v, xt, xdt, K, dt, pos_tol, rot_tol, want=())
            paths = (("rollout", None, roll), ("stepwise", "0", reach), ("persistent", str(1 << 30), reach))
            runs = {name: [] for name, _, _ in paths}
            for _ in range(args.rounds):  # the paths alternate, so drift of the box hits all three alike
                for name, cap, fn in paths:
                    if cap is not None:
                        os.environ["DRC_REACH_MAX"] = cap
                    runs[name].append(1e3 * timed_steps(torch, fn, args.reps, args.warmup))
                    os.environ.pop("DRC_REACH_MAX", None)
            row = {name: sorted(t)[len(t) // 2] for name, t in runs.items()}  # median of the rounds
            row["runs"] = {name: [round(x, 4) for x in t] for name, t in runs.items()}
            res = reach()
            torch.cuda.synchronize()
            result, steps = res.result.cpu().numpy(), res.steps_used.cpu().numpy()
            row["mean_steps_used"] = float(steps.mean())
            row["share"] = {"reached": float((result == res.REACHED).mean()), "budget": float((result == res.BUDGET).mean()),
                            "qp_failed": float((result == res.QP_FAILED).mean())}
            rows[str(B)] = row
        line["robots"][robot] = rows
    print(json.dumps(line))


if __name__ == "__main__":
    main()
