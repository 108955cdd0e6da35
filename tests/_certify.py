"""The rule of drc_clearance_certify_batch as include/drc_amd.h states it, in
plain Python (every operation on Python floats, hence rounded once): what
tests/test_clearance_certify_host.py holds against csrc/clearance_certify.hpp
compiled with the host compiler and tests/test_gpu_clearance_certify.py against
the kernel, bit for bit."""
import math

FREE, BLOCKED, INVALID, UNDECIDED = 0, 1, 2, 3
FIELDS = ("result", "seg_stop", "t_stop", "d_min", "seg_min", "t_min", "pair_min", "d_lower", "samples_used")


class _Stop(Exception):
    pass


def fold(dist, waypoints, d_stop, max_depth, M, travel_ok=None):
    """One path.  dist(j, k, e) -> (d, pair) at t = k / 2^e of segment j; M[j]
    the segment's motion bound; travel_ok[j] (None: all True).  Returns the
    entry's nine outputs as a dict and the list of evaluated (j, k, e)."""
    r = dict(result=FREE, seg_stop=-1, t_stop=-1.0, d_min=math.inf, seg_min=-1, t_min=-1.0, pair_min=-1,
             d_lower=math.inf, samples_used=0)
    seen = []

    def stop(result, j, t):
        r["result"], r["seg_stop"], r["t_stop"] = result, j, t
        raise _Stop()

    def evaluate(j, k, e):
        d, pair = dist(j, k, e)
        seen.append((j, k, e))
        r["samples_used"] += 1
        t = k / 2 ** e
        if d != d:
            stop(INVALID, j, t)
        if d < r["d_min"]:
            r["d_min"], r["seg_min"], r["t_min"], r["pair_min"] = d, j, t, pair
        if d < d_stop:
            stop(BLOCKED, j, t)
        return d

    def interval(j, k, e, d0, d1):
        t0, t1 = k / 2 ** e, (k + 1) / 2 ** e
        lb = 0.5 * (d0 + d1) - (0.5 * (t1 - t0)) * M[j]
        if lb >= d_stop:
            r["d_lower"] = min(r["d_lower"], lb)
            return
        if e == max_depth:
            stop(UNDECIDED, j, t0)
        dm = evaluate(j, 2 * k + 1, e + 1)
        interval(j, 2 * k, e + 1, d0, dm)
        interval(j, 2 * k + 1, e + 1, dm, d1)

    try:
        d_end = evaluate(0, 0, 0)
        for j in range(waypoints - 1):
            if travel_ok is not None and not travel_ok[j]:
                stop(UNDECIDED, j, 0.0)
            d1 = evaluate(j, 1, 0)
            interval(j, 0, 0, d_end, d1)
            d_end = d1
    except _Stop:
        pass
    return r, seen


def motion_bound(wt, dq_abs):
    """M = max_p sum_i wt[i][p] |dq_i|: the sum in ascending i from 0.0, the max
    exact and starting from 0.0.  wt [nv][npairs], dq_abs [nv] (numpy or lists)."""
    m = 0.0
    for p in range(len(wt[0])):
        s = 0.0
        for i in range(len(dq_abs)):
            s = s + float(wt[i][p]) * float(dq_abs[i])
        if s > m:
            m = s
    return m
