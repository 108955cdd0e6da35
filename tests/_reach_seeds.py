"""Shared helpers of the reach seeds tests (test infrastructure): the rule of
drc_qpik_reach_seeds_batch in numpy, as include/drc_amd.h states it, and the
seeds of the GPU tests."""
import numpy as np

REACHED, BUDGET, QP_FAILED, CANCELLED = 0, 1, 2, 3
FIRST, FEWEST_STEPS = 0, 1
NO_KEY = 0xffffffff


def winner(rule, result, steps, e_p, e_r):
    """The winning seed of every group, from [S][T] arrays of (uncancelled)
    outcomes.  Some seed REACHED: the lowest such index (FIRST) or the least
    steps, ties to the lowest index (FEWEST_STEPS).  None: the least e_p, then
    the least e_R, then the lowest index, a NaN counting as +inf."""
    result, steps = np.asarray(result), np.asarray(steps)
    reached = result == REACHED
    if rule == FIRST:
        win = np.argmax(reached, axis=0)
    else:
        win = np.argmin(np.where(reached, steps.astype(np.int64), np.iinfo(np.int64).max), axis=0)
    e_p = np.where(np.isnan(e_p), np.inf, e_p)
    e_r = np.where(np.isnan(e_r), np.inf, e_r)
    least_p = e_p == e_p.min(axis=0)
    least = least_p & (e_r == np.where(least_p, e_r, np.inf).min(axis=0))
    return np.where(reached.any(axis=0), win, np.argmax(least, axis=0)).astype(np.int32)


def key(rule, S, k, s):
    return k * S + s if rule == FEWEST_STEPS else s


def cancelled(rule, S, word, k, s):
    if word == NO_KEY:
        return False
    return word // S <= k if rule == FEWEST_STEPS else word < s


def seeds(goal, lo, hi, S):
    """q0 [nv][S][T]: seed (s, t) = clip(goal_t + default_rng(200000 + 1000 s +
    t).uniform(-0.3, 0.3, nv)) to the position limits clipped to +-3."""
    lo, hi = np.clip(np.asarray(lo, float), -3, 3), np.clip(np.asarray(hi, float), -3, 3)
    nv, T = goal.shape
    q = np.zeros((nv, S, T))
    for s in range(S):
        for t in range(T):
            r = np.random.default_rng(200000 + 1000 * s + t)
            q[:, s, t] = np.clip(goal[:, t] + r.uniform(-0.3, 0.3, nv), lo, hi)
    return q
