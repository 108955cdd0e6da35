#!/usr/bin/env python3
"""Goal-reaching rollouts through waypoints (QPIK_reach_path_batch /
drc_qpik_reach_path_batch), ms per call on FR3 and Husky-FR3 for three ways to
take a link through W poses, on the inputs of tests/test_gpu_reach_path.py
(the census goal of tests/_reach.py, then W - 1 further goals within 0.15 per
joint of the previous one; 1e-4 m, 1e-3 rad):
  chain       what a caller had before: W drc_qpik_reach_batch calls, the state
              of the instances that reached the previous pose carried over with
              torch masks;
  stepwise    drc_qpik_reach_path_batch's stepwise path (DRC_REACH_MAX = 0);
  persistent  its persistent kernel (DRC_REACH_MAX raised past the batch).
Then FR3 with four obstacle slots (tests/_obstacles.py, one shared pose set)
and one waypoint: drc_qpik_reach_obstacles_batch, which runs step by step,
against the new entry's two paths.  Manipulator: Kp 100, Kv 0, w_reg 0.01, dt
5 ms; mobile manipulator: the defaults at dt 1 ms.  Reports the mean
steps_used next to the times.  Information for DESIGN.md "Reach paths" and the
persistent kernel's batch-size threshold, not a gate.  Prints one JSON line.

  python tools/bench_reach_path.py [--steps 32] [--waypoints 3] [--batches 256,4096,16384,65536]
                                   [--reps 5] [--warmup 2] [--rounds 3]"""
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
    ap.add_argument("--waypoints", type=int, default=3)
    ap.add_argument("--batches", default="256,4096,16384,65536")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    import numpy as np
    import torch
    from bench import timed_steps  # the benchmark's own timing helper
    import _obstacles as OB
    import _reach as RC
    from _common import make_manipulator, make_moma
    from dyros_robot_controller_amd import _batch, _capi, manipulator, mobile_manipulator

    dev = torch.device("cuda", 0)
    K, pos_tol, rot_tol = args.steps, 1e-4, 1e-3
    batches = [int(b) for b in args.batches.split(",")]
    line = {"metric": "ms per call through the waypoints", "max_steps": K, "pos_tol": pos_tol, "rot_tol": rot_tol,
            "reps": args.reps, "warmup": args.warmup, "rounds": args.rounds, "build": _capi.build_id(), "robots": {}}
    a = lambda t: _batch.as_device(t, dev)

    def measure(paths):
        """Median over the rounds of each path's ms per call; the paths alternate,
        so drift of the machine hits all of them alike."""
        runs = {name: [] for name, _, _ in paths}
        for _ in range(args.rounds):
            for name, cap, fn in paths:
                if cap is not None:
                    os.environ["DRC_REACH_MAX"] = cap
                runs[name].append(1e3 * timed_steps(torch, fn, args.reps, args.warmup))
                os.environ.pop("DRC_REACH_MAX", None)
        row = {name: sorted(t)[len(t) // 2] for name, t in runs.items()}
        row["runs"] = {name: [round(x, 4) for x in t] for name, t in runs.items()}
        return row

    for robot, slots, W in (("fr3", False, args.waypoints), ("husky_fr3", False, args.waypoints), ("fr3", True, 1)):
        moma = robot == "husky_fr3"
        rd = make_moma(robot, dev) if moma else make_manipulator(robot, dev)
        pose = None
        if slots:
            rd.set_obstacles(OB.FOUR_TYPES, OB.FOUR_PARAMS, OB.FR3_ARM_LINKS)
            pose = a(np.ascontiguousarray(OB.to_field_major(OB.fr3_scene(11, 32))[:, :, 5]))
        ctrl = (mobile_manipulator if moma else manipulator).RobotController(0.001, rd, solver_mode="exact")
        link = "fr3_link8"
        if moma:
            p, dt = ctrl._pb.params(link, _capi.MODE_QPIK_STEP, ctrl.Kp_task_, np.zeros(6)), 0.001
        else:
            p, dt = ctrl._pb.params(link, _capi.MODE_QPIK_STEP, np.full(6, 100.0), np.zeros(6)), 0.005
            p.w_reg = 0.01
        lo, hi = rd.get_joint_position_limit() if moma else rd.getJointPositionLimit()
        Bmax = max(batches)
        q0_all, goal = RC.census_states(lo, hi, Bmax)
        rng = np.random.default_rng(100000)  # (one stream for the batch: the tests draw per instance)
        xp_all = []
        for w in range(W):
            if w:
                goal = goal + rng.uniform(-0.15, 0.15, goal.shape)
            st = _batch.stages_batch(rd.model, p, a(goal), a(np.zeros_like(goal)), a(np.zeros((12, Bmax))),
                                     a(np.zeros((6, Bmax))), obstacle_pose=pose)
            xp_all.append(st["pose"])
        xp_all = torch.stack(xp_all)
        rows = {}
        for B in batches:
            q, v = a(np.ascontiguousarray(q0_all[:, :B])), a(np.zeros((q0_all.shape[0], B)))
            xp, xdp = xp_all[:, :, :B].contiguous(), a(np.zeros((W, 6, B)))
            reach = lambda qq, vv, w: _batch.qpik_reach_batch(rd.model, p, qq, vv, xp[w], xdp[w], K, dt, pos_tol,
                                                              rot_tol, want=(), obstacle_pose=pose)
            path = lambda: _batch.qpik_reach_path_batch(rd.model, p, q, v, xp, xdp, K, dt, pos_tol, rot_tol, want=(),
                                                        obstacle_pose=pose)

            def chain():
                qc, vc, alive = q, v, None
                for w in range(W):
                    r = reach(qc, vc, w)
                    if alive is None:
                        qc, vc, alive = r.q_final, r.qdot_final, r.result == r.REACHED
                    else:
                        qc, vc = torch.where(alive, r.q_final, qc), torch.where(alive, r.qdot_final, vc)
                        alive = alive & (r.result == r.REACHED)
                return qc, vc, alive

            # (with slots the existing entry runs step by step whatever DRC_REACH_MAX says)
            row = measure(((("reach_obstacles" if slots else "chain"), None, chain), ("stepwise", "0", path),
                           ("persistent", str(1 << 30), path)))
            res = path()
            torch.cuda.synchronize()
            row["mean_steps_used"] = float(res.steps_used.double().mean())
            row["share_reached_all"] = float((res.result == res.REACHED).double().mean())
            rows[str(B)] = row
            print("%s%s B=%d %s" % (robot, " slots" if slots else "", B,
                                    {k: round(x, 3) for k, x in row.items() if isinstance(x, float)}), file=sys.stderr)
        line["robots"][robot + ("_slots" if slots else "")] = {"waypoints": W, "batches": rows}
    print(json.dumps(line))


if __name__ == "__main__":
    main()
