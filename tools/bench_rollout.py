#!/usr/bin/env python3
"""Closed-loop QPIKStep rollouts of K steps (QPIK_rollout_batch), ms per
rollout on FR3 and Husky-FR3 for three paths on the same inputs:
  user        what a caller wrote before the entry existed: K x QPIK_step_batch
              plus the torch state update q + dt * qdot (mobile manipulator:
              qdot = S(q) eta in torch), one stream, one final synchronisation;
  stepwise    drc_qpik_rollout_batch's stepwise path (DRC_ROLLOUT_MAX = 0);
  persistent  its persistent kernel (DRC_ROLLOUT_MAX raised past the batch).
Information for DESIGN.md "Rollouts" and the persistent kernel's batch-size
threshold, not a gate.  Prints one JSON line.

  python tools/bench_rollout.py [--steps 32] [--batches 1,256,4096,16384,65536] [--reps 5] [--warmup 2] [--rounds 3]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)


def user_loop(torch, ctrl, rd, moma, link, K, dt, q0, qd0, xt, xdt):
    """K single-step calls and the state update in torch."""
    if moma:
        ji, ai = rd.get_joint_index(), rd.get_actuator_index()
        n, W = rd.get_manipulator_dof(), rd.get_mobile_dof()
        Jm = torch.as_tensor(rd.compute_mobile_FK_jacobian([0.0] * W), device=q0.device)  # differential: constant

    def run():
        q, qd = q0, qd0
        for _ in range(K):
            eta, _ = ctrl.QPIK_step_batch(q, qd, xt, xdt, link)
            if moma:
                qd = torch.empty_like(q)
                qd[ji.mani_start:ji.mani_start + n] = eta[ai.mani_start:ai.mani_start + n]
                w = eta[ai.mobi_start:ai.mobi_start + W]
                qd[ji.mobi_start:ji.mobi_start + W] = w
                tw = Jm @ w
                c, s = torch.cos(q[ji.virtual_start + 2]), torch.sin(q[ji.virtual_start + 2])
                qd[ji.virtual_start] = c * tw[0] - s * tw[1]
                qd[ji.virtual_start + 1] = s * tw[0] + c * tw[1]
                qd[ji.virtual_start + 2] = tw[2]
            else:
                qd = eta
            q = q + dt * qd
        return q
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--batches", default="1,256,4096,16384,65536")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    import torch
    from bench import make_inputs, timed_steps  # the benchmark's own inputs and timing helper
    from _common import make_manipulator, make_moma
    from dyros_robot_controller_amd import _capi, manipulator, mobile_manipulator

    dev = torch.device("cuda", 0)
    K, dt = args.steps, 0.001
    batches = [int(b) for b in args.batches.split(",")]
    line = {"metric": "ms per closed-loop QPIKStep rollout", "steps": K, "dt": dt, "reps": args.reps, "rounds": args.rounds,
            "build": _capi.build_id(), "robots": {}}
    for robot in ("fr3", "husky_fr3"):
        moma = robot == "husky_fr3"
        rd = make_moma(robot, dev) if moma else make_manipulator(robot, dev)
        ctrl = (mobile_manipulator if moma else manipulator).RobotController(dt, rd, solver_mode="exact")
        link = "fr3_link8"
        rows = {}
        for B in batches:
            _, (dq, dqd, dxt, dxdt), _ = make_inputs(rd, robot, B, 12345, 0, dev)
            roll = lambda: ctrl.QPIK_rollout_batch(dq, dqd, dxt, dxdt, link, K, want=("qdot_traj", "q_traj"))
            paths = (("user", None, user_loop(torch, ctrl, rd, moma, link, K, dt, dq, dqd, dxt, dxdt)),
                     ("stepwise", "0", roll), ("persistent", str(1 << 30), roll))
            runs = {name: [] for name, _, _ in paths}
            for _ in range(args.rounds):  # the paths alternate, so drift of the box hits all three alike
                for name, cap, fn in paths:
                    if cap is not None:
                        os.environ["DRC_ROLLOUT_MAX"] = cap
                    runs[name].append(1e3 * timed_steps(torch, fn, args.reps, args.warmup))
                    os.environ.pop("DRC_ROLLOUT_MAX", None)
            row = {name: sorted(v)[len(v) // 2] for name, v in runs.items()}  # median of the rounds
            row["runs"] = {name: [round(x, 4) for x in v] for name, v in runs.items()}
            row["solved_fraction_last_step"] = float((roll().status_traj[-1] == 1).float().mean().item())
            rows[str(B)] = row
        line["robots"][robot] = rows
    print(json.dumps(line))


if __name__ == "__main__":
    main()
