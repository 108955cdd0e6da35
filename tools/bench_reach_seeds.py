#!/usr/bin/env python3
"""Reach from several seeds per target (QPIK_reach_seeds_batch /
drc_qpik_reach_seeds_batch), ms per call on FR3 and Husky-FR3 for the ways to
get one answer per target out of S start states, on the inputs of
tests/test_gpu_reach_seeds.py (target t the stage pose at the census goal of
tests/_reach.py, seed (s, t) within 0.3 rad per joint of the goal; 1e-4 m,
1e-3 rad, 60 steps):
  composition   what a caller had before: drc_qpik_reach_batch on the S T
                instances with the targets replicated, then a torch gather by
                the FIRST rule;
  cancel0       drc_qpik_reach_seeds_batch, every instance run to its own stop;
  first         ... with cancellation, rule DRC_SEEDS_FIRST;
  fewest        ... with cancellation, rule DRC_SEEDS_FEWEST_STEPS.
Then one far-seed case: seeds uniform in the middle 80 % of the position
limits, 200 steps.  Manipulator: Kp 100, Kv 0, w_reg 0.01, dt 5 ms; mobile
manipulator: the defaults at dt 1 ms.  Reports the share of groups reached and
the mean steps per instance with cancellation next to the uncancelled mean.
Information for DESIGN.md "Reach seeds" and the default of ``cancel``, not a
gate.  Prints one JSON line.

  python tools/bench_reach_seeds.py [--configs 64x4,1024x4,4096x4,16384x4,4096x16] [--far 1024x8]
                                    [--reps 3] [--warmup 1] [--rounds 3]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="64x4,1024x4,4096x4,16384x4,4096x16")
    ap.add_argument("--far", default="1024x8")
    ap.add_argument("--robots", default="fr3,husky_fr3")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    import numpy as np
    import torch
    from bench import timed_steps  # the benchmark's own timing helper
    import _reach as RC
    import _reach_seeds as RS
    from _common import make_manipulator, make_moma
    from dyros_robot_controller_amd import _batch, _capi, manipulator, mobile_manipulator

    dev = torch.device("cuda", 0)
    pos_tol, rot_tol = 1e-4, 1e-3
    parse = lambda s: [tuple(int(x) for x in c.split("x")) for c in s.split(",") if c]
    line = {"metric": "ms per call, one answer per target from S seeds", "pos_tol": pos_tol, "rot_tol": rot_tol,
            "reps": args.reps, "warmup": args.warmup, "rounds": args.rounds, "build": _capi.build_id(), "robots": {}}
    a = lambda t: _batch.as_device(t, dev)

    def measure(paths):
        """Median over the rounds of each path's ms per call; the paths alternate,
        so drift of the machine hits all of them alike."""
        runs = {name: [] for name, _ in paths}
        for _ in range(args.rounds):
            for name, fn in paths:
                runs[name].append(1e3 * timed_steps(torch, fn, args.reps, args.warmup))
        row = {name: sorted(t)[len(t) // 2] for name, t in runs.items()}
        row["runs"] = {name: [round(x, 4) for x in t] for name, t in runs.items()}
        return row

    for robot in args.robots.split(","):
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
        lo3, hi3 = np.clip(np.asarray(lo, float), -3, 3), np.clip(np.asarray(hi, float), -3, 3)
        near, far = parse(args.configs), parse(args.far)
        Tmax = max(T for T, _ in near + far)
        goal_all = RC.census_states(lo, hi, Tmax)[1]
        xt_all = _batch.stages_batch(rd.model, p, a(goal_all), a(np.zeros_like(goal_all)), a(np.zeros((12, Tmax))),
                                     a(np.zeros((6, Tmax))))["pose"]
        rows = {}
        for (T, S), K, is_far in [(c, 60, False) for c in near] + [(c, 200, True) for c in far]:
            goal = goal_all[:, :T]
            if is_far:  # (one stream for the call: the near seeds draw per instance, as the tests do)
                q3 = lo3[:, None, None] + (hi3 - lo3)[:, None, None] * (
                    0.1 + 0.8 * np.random.default_rng(300000).random((len(lo3), S, T)))
            else:
                q3 = RS.seeds(goal, lo, hi, S)
            q = a(np.ascontiguousarray(q3.reshape(len(lo3), S * T)))
            v = torch.zeros_like(q)
            xt, xdt = xt_all[:, :T].contiguous(), a(np.zeros((6, T)))
            cols = torch.arange(T, device=dev)
            sidx = torch.arange(S, device=dev)[:, None]

            def composition():
                r = _batch.qpik_reach_batch(rd.model, p, q, v, xt.repeat(1, S), xdt.repeat(1, S), K, dt, pos_tol,
                                            rot_tol, want=("err_final",))
                reached = r.result.view(S, T) == r.REACHED
                first = torch.where(reached, sidx, S).min(dim=0).values
                closest = torch.nan_to_num(r.err_final[0].view(S, T), nan=float("inf")).argmin(dim=0)
                b = torch.where(first < S, first, closest) * T + cols
                return r.q_final[:, b], r.qdot_final[:, b], r.result[b], r.steps_used[b]

            seeds = lambda rule, cancel, want=(): _batch.qpik_reach_seeds_batch(
                rd.model, p, q, v, xt, xdt, K, dt, pos_tol, rot_tol, seeds=S, rule=rule, cancel=cancel, want=want)
            row = measure((("composition", composition), ("cancel0", lambda: seeds("first", False)),
                           ("first", lambda: seeds("first", True)), ("fewest", lambda: seeds("fewest_steps", True))))
            row["max_steps"] = K
            plain = seeds("first", False, ("inst_steps",))
            torch.cuda.synchronize()
            row["share_groups_reached"] = float((plain.result == plain.REACHED).double().mean())
            row["mean_inst_steps"] = {"cancel0": float(plain.inst_steps.double().mean())}
            for rule in ("first", "fewest_steps"):
                r = seeds(rule, True, ("inst_steps", "inst_result"))
                torch.cuda.synchronize()
                row["mean_inst_steps"][rule] = float(r.inst_steps.double().mean())
                row.setdefault("share_cancelled", {})[rule] = float((r.inst_result == r.CANCELLED).double().mean())
            rows["%dx%d%s" % (T, S, "_far" if is_far else "")] = row
            print("%s T=%d S=%d%s %s steps %s" % (robot, T, S, " far" if is_far else "",
                                                 {k: round(x, 3) for k, x in row.items() if isinstance(x, float)},
                                                 {k: round(x, 2) for k, x in row["mean_inst_steps"].items()}),
                  file=sys.stderr)
        line["robots"][robot] = rows
    print(json.dumps(line))


if __name__ == "__main__":
    main()
