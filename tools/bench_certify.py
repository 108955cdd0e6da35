#!/usr/bin/env python3
"""Certified path clearance (drc_clearance_certify_batch), ms per call on FR3 and
Husky-FR3 on the edges of tools/bench_clearance.py, against the way to the same
guarantee without it:
  certify    one drc_clearance_certify_batch call at max_depth 8;
  dense      drc_clearance_path_batch at the uniform substeps = 2^D with its
             profile, D the deepest level the certified call needed on that
             batch (the smallest max_depth whose verdicts equal max_depth 8's),
             then the bound in torch: M from the model's weights, lb over
             adjacent samples, its minimum and the verdict.
d_stop 0.0 and 0.05.  The two alternate for --rounds rounds and the median round
is reported, with the mean samples_used, the verdict shares at max_depth 8 and D.

Information for DESIGN.md "Certified clearance", not a gate.  Prints one JSON line.

  python tools/bench_certify.py [--batches 4096,65536] [--reps 3] [--warmup 1] [--rounds 3]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)

MAX_DEPTH = 8
D_STOPS = (0.0, 0.05)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="4096,65536")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    import torch
    from bench import timed_steps
    from bench_clearance import setup
    from dyros_robot_controller_amd import _batch, _capi

    dev = torch.device("cuda", 0)
    line = {"metric": "ms per call", "max_depth": MAX_DEPTH, "reps": args.reps, "rounds": args.rounds,
            "build": _capi.build_id(), "robots": {}}
    for robot in ("fr3", "husky_fr3"):
        rows = {}
        for B in (int(b) for b in args.batches.split(",")):
            rd, path = setup(robot, B, dev)
            model = rd.model
            wt = torch.from_numpy(_batch.motion_weights(model)[1]).to(dev)   # [nv][npairs]
            row = {}
            for d_stop in D_STOPS:
                cert = lambda depth=MAX_DEPTH: _batch.clearance_certify_batch(model, path, d_stop=d_stop, max_depth=depth)
                full = cert()
                torch.cuda.synchronize()
                D = MAX_DEPTH
                for depth in range(MAX_DEPTH):
                    if torch.equal(cert(depth).result, full.result):
                        D = depth
                        break
                sub = 2 ** D
                traj = torch.zeros((sub + 1, B), dtype=torch.float64, device=dev)

                def dense():
                    res = _batch.clearance_path_batch(model, path, substeps=sub, d_stop=d_stop, dist_traj=traj)
                    M = ((path[1] - path[0]).abs().t() @ wt).max(dim=1).values
                    lb = 0.5 * (traj[:-1] + traj[1:]) - (0.5 / sub) * M
                    d_lower = lb.min(dim=0).values
                    return res.result, (res.result == 0) & (d_lower >= d_stop), d_lower
                runs = {"certify": [], "dense": []}
                for _ in range(args.rounds):
                    for k, fn in (("certify", cert), ("dense", dense)):
                        runs[k].append(1e3 * timed_steps(torch, fn, args.reps, args.warmup))
                blocked, free, _ = dense()
                torch.cuda.synchronize()
                r = full.result
                # the dense walk sees every state the certified one does, so what one blocks the other cannot certify
                assert not (free & (r == 1)).any() and not ((blocked == 1) & (r == 0)).any(), "the two disagree"
                row[str(d_stop)] = {k: sorted(v)[len(v) // 2] for k, v in runs.items()}
                row[str(d_stop)].update({
                    "ratio_dense_over_certify": row[str(d_stop)]["dense"] / row[str(d_stop)]["certify"],
                    "runs": {k: [round(x, 4) for x in v] for k, v in runs.items()},
                    "D": D, "dense_samples": sub + 1,
                    "mean_samples_used": float(full.samples_used.double().mean()),
                    "max_samples_used": int(full.samples_used.max()),
                    "share": {name: float((r == code).double().mean())
                              for code, name in enumerate(("free", "blocked", "invalid", "undecided"))},
                    "dense_free_share": float(free.double().mean()),
                    "grid": _batch.clearance_grid(model)})
            rows[str(B)] = row
        line["robots"][robot] = rows
    print(json.dumps(line))


if __name__ == "__main__":
    main()
