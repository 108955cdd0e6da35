"""Host wall time of the synchronous host-buffer entries drc_qpid_host,
drc_qpid_stages_host, drc_closed_form_host (CLIK), drc_dynamics_host and
drc_joint_torque_step_host on the FR3 (GPU box): B = 1 (20 warm-up calls, 400
timed) and B = 4096 (5 warm-up calls, 40 timed), p50 / p99 in us, one JSON line.
DRC_AMD_LIB selects the library, so two builds can be run in alternation as
fresh processes:

    DRC_AMD_LIB=libdrc_amd_parent.so python tools/host_entry_latency.py >> ab.jsonl
    python tools/host_entry_latency.py >> ab.jsonl
    python tools/host_entry_latency.py --summarise ab.jsonl libdrc_amd_parent.so

--summarise: per entry and size the p50 of every round, and whether the other
build's median round stays at or below the named build's highest round.
"""
import argparse
import ctypes as C
import gc
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIZES = ((1, 20, 400), (4096, 5, 40))


def measure():
    import torch
    import bench
    from dyros_robot_controller_amd import BUNDLED, _capi, make_robot, manipulator
    dev = torch.device("cuda", 0)
    rd = make_robot("fr3", dev)
    link = BUNDLED["fr3"]["link"]
    (q, qd, xt, xdt), _, _ = bench.make_inputs(rd, "fr3", SIZES[-1][0], 12345, 0, dev)
    pid = manipulator.QPIKParamsBuilder(rd.model, exact=True, qpid=True).params(link, _capi.MODE_QPID_STEP)
    pik = manipulator.QPIKParamsBuilder(rd.model, exact=True).params(link, _capi.MODE_QPIK_STEP)
    lib, h, n = _capi.lib(), rd.model.handle, rd.model.dof
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    res = {"lib": os.path.basename(_capi.LIB_PATH), "build_id": _capi.build_id(), "robot": "fr3", "entries": {}}
    for B, warmup, calls in SIZES:
        col = lambda a: np.ascontiguousarray(a[:, :B])
        task = [dp(col(a)) for a in (q, qd, xt, xdt)] + [None, None]
        f = lambda rows: dp(np.zeros((rows, B)))
        i32 = lambda: ip(np.zeros(B, np.int32))
        Bc = C.c_int64(B)
        entries = {
            "drc_qpid_host": (lib.drc_qpid_host, (h, C.byref(pid), Bc, *task, f(n), f(n), i32(), i32())),
            "drc_qpid_stages_host": (lib.drc_qpid_stages_host,
                                     (h, C.byref(pid), Bc, *task, f(12), f(6 * n), f(1 + n), f(1 + n), i32(), f(6),
                                      f(6 * n), f(8), f(2 * n))),
            "drc_closed_form_host": (lib.drc_closed_form_host, (h, C.byref(pik), 1, Bc, *task, None, f(n))),
            "drc_dynamics_host": (lib.drc_dynamics_host,
                                  (h, 0, Bc, task[0], task[1], f(n * n), f(n * n), f(n), f(n), f(n))),
            "drc_joint_torque_step_host": (lib.drc_joint_torque_step_host,
                                           (h, Bc, task[0], task[1], task[0], task[1], None, C.c_double(0.001), None,
                                            None, f(n))),
        }
        for name, (fn, args) in entries.items():
            ts = []
            gc_was = gc.isenabled()
            gc.disable()
            for k in range(warmup + calls):
                t0 = time.perf_counter()
                rc = fn(*args)
                t1 = time.perf_counter()
                _capi.check(rc)
                if k >= warmup:
                    ts.append(t1 - t0)
            if gc_was:
                gc.enable()
            ts = np.array(ts) * 1e6
            res["entries"].setdefault(name, {})["b%d" % B] = {
                "p50_us": float(np.percentile(ts, 50)), "p99_us": float(np.percentile(ts, 99)), "calls": calls}
    print(json.dumps(res), flush=True)


def summarise(path, base):
    rows = [json.loads(l) for l in open(path) if l.strip()]
    ids = sorted({r["lib"] for r in rows})
    assert base in ids and len(ids) == 2, ids
    other = [i for i in ids if i != base][0]
    ok = True
    for name in rows[0]["entries"]:
        for size in rows[0]["entries"][name]:
            p50 = {i: [r["entries"][name][size]["p50_us"] for r in rows if r["lib"] == i] for i in ids}
            bound, value = max(p50[base]), float(np.median(p50[other]))
            ok &= value <= bound
            print(json.dumps({"entry": name, "size": size, "base": base, "base_round_p50_us": p50[base],
                              "other": other, "other_round_p50_us": p50[other], "other_median_us": value,
                              "base_max_us": bound, "within": bool(value <= bound)}))
    return 0 if ok else 1


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--summarise", nargs=2, metavar=("JSONL", "BASE_LIB"))
    a = ap.parse_args()
    sys.exit(summarise(*a.summarise) if a.summarise else measure())
