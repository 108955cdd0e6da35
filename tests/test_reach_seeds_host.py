"""The rule of drc_qpik_reach_seeds_batch (csrc/reach_seeds.hpp) compiled with
the host compiler (tools/reach_seeds_host_test.cpp) against its statement in
numpy (tests/_reach_seeds.py, after include/drc_amd.h):

    some seed REACHED: FIRST the lowest such index; FEWEST_STEPS the least
        steps_used, ties to the lowest index
    none: the least e_p, then the least e_R, then the lowest index; NaN = +inf
    key: s (FIRST), k S + s (FEWEST_STEPS), published by a REACHED seed at step k
    stop at step k after a failed verdict: word < s (FIRST), word // S <= k
        (FEWEST_STEPS); never on the initial word

and the invariant that makes cancellation safe, by brute force over every
interleaving of the seeds' steps and every (stale) value a read may return:
the true winner is never cancelled, and the outcomes of a cancelling call give
the same winner with the same result and step count."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import _reach_seeds as RS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.environ.get("CXX", "g++")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    assert shutil.which(CXX), "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("reach_seeds") / "reach_seeds_host")
    subprocess.check_call([CXX, "-O2", "-std=c++17", "-Wall", "-Werror",
                           os.path.join(ROOT, "tools", "reach_seeds_host_test.cpp"), "-o", exe])
    return exe


def run(exe, lines):
    res = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True)
    return [[int(x) for x in ln.split()] for ln in res.stdout.strip().splitlines()]


def groups(S, G, rng):
    """[S][G] outcomes with many ties: few distinct step counts and errors, NaN
    and inf errors, every fifth group without a REACHED seed."""
    result = rng.integers(0, 3, size=(S, G))
    result[:, ::5] = rng.integers(1, 3, size=(S, len(range(0, G, 5))))
    steps = rng.integers(0, 4, size=(S, G))
    vals = np.array([0.0, 1e-9, 1e-9 * (1 + 2 ** -52), 0.25, 3.0, np.inf, np.nan])
    e_p = vals[rng.integers(0, len(vals), size=(S, G))]
    e_r = vals[rng.integers(0, len(vals), size=(S, G))]
    e_p[:, ::7] = e_p[0, ::7]   # equal e_p: e_R decides
    e_r[:, ::35] = e_r[0, ::35]   # and equal e_R: the index decides
    return result, steps, e_p, e_r


@pytest.mark.parametrize("rule", [RS.FIRST, RS.FEWEST_STEPS])
def test_winner_is_numpys(harness, rule):
    rng = np.random.default_rng(11 + rule)
    lines, want, seen = [], [], dict(none=0, tie=0, nan=0, later=0)
    for S, G in ((1, 200), (2, 700), (3, 700), (4, 1400), (7, 700), (16, 350)):
        result, steps, e_p, e_r = groups(S, G, rng)
        win = RS.winner(rule, result, steps, e_p, e_r)
        for g in range(G):
            lines.append("w %d %d " % (rule, S) + " ".join(
                "%d %d %r %r" % (result[s, g], steps[s, g], float(e_p[s, g]), float(e_r[s, g])) for s in range(S)))
        want += list(win)
        reached = result == RS.REACHED
        none = ~reached.any(axis=0)
        seen["none"] += none.sum()
        seen["nan"] += (none & np.isnan(e_p).any(axis=0)).sum()
        seen["later"] += (win > 0).sum()
        best = np.where(reached, steps, 99).min(axis=0)
        seen["tie"] += ((np.where(reached, steps, 99) == best).sum(axis=0)[~none] > 1).sum()
    got = [r[0] for r in run(harness, lines)]
    assert len(got) == len(want) >= 4000
    np.testing.assert_array_equal(got, want)
    assert all(v >= 100 for v in seen.values()), seen


def test_winner_by_hand(harness):
    R, B, Q = RS.REACHED, RS.BUDGET, RS.QP_FAILED
    nan, inf = float("nan"), float("inf")
    cases = [
        # (rule, [(result, steps, e_p, e_R)], winner)
        (RS.FIRST, [(B, 9, 1, 1), (R, 7, 0, 0), (R, 2, 0, 0)], 1),
        (RS.FEWEST_STEPS, [(B, 9, 1, 1), (R, 7, 0, 0), (R, 2, 0, 0)], 2),
        (RS.FEWEST_STEPS, [(Q, 0, 1, 1), (R, 5, 0, 0), (R, 5, 0, 0), (R, 6, 0, 0)], 1),   # a step tie
        (RS.FEWEST_STEPS, [(RS.CANCELLED, 1, 1, 1), (R, 5, 0, 0)], 1),   # a cancelled seed is never REACHED
        (RS.FIRST, [(B, 9, 2.0, 0.1), (Q, 3, 1.0, 0.7), (B, 9, 1.0, 0.2)], 2),   # none: e_p, then e_R
        (RS.FIRST, [(B, 9, 1.0, 0.2), (Q, 3, 1.0, 0.2)], 0),   # ... then the index
        (RS.FEWEST_STEPS, [(B, 9, nan, 0.0), (B, 9, inf, 0.5), (B, 9, inf, nan)], 0),   # NaN = +inf: e_R 0 wins
        (RS.FIRST, [(B, 9, nan, nan), (B, 9, nan, nan)], 0),
        (RS.FIRST, [(B, 9, nan, 0.0), (B, 9, 5.0, nan)], 1),
        (RS.FIRST, [(B, 4, 3.0, 3.0)], 0), (RS.FEWEST_STEPS, [(R, 4, 0, 0)], 0),   # S = 1
    ]
    lines = ["w %d %d " % (rule, len(seeds)) + " ".join("%d %d %r %r" % (r, k, float(a), float(b))
                                                         for r, k, a, b in seeds) for rule, seeds, _ in cases]
    assert [r[0] for r in run(harness, lines)] == [w for _, _, w in cases]


def test_key_and_cancel_predicate(harness):
    rng = np.random.default_rng(5)
    lines, want = [], []
    # the key bound: (max_steps + 1) S just below 2^31, so that the largest key is 2^31 - 2 or so
    bound = [(1, 2 ** 31 - 2), (2, 2 ** 30 - 2), (4, 2 ** 29 - 2), (60, (2 ** 31 - 1) // 60 - 1),
             (2 ** 30, 0), (2 ** 31 - 1, 0)]
    for rule in (RS.FIRST, RS.FEWEST_STEPS):
        for S, kmax in bound:
            assert (kmax + 1) * S < 2 ** 31
            for k, s in ((kmax, S - 1), (kmax, 0), (0, S - 1), (kmax // 2, S // 2)):
                lines.append("k %d %d %d %d" % (rule, S, k, s))
                want.append(RS.key(rule, S, k, s))
                assert want[-1] < 2 ** 31 < RS.NO_KEY
                for word in (RS.NO_KEY, RS.key(rule, S, kmax, S - 1), RS.key(rule, S, k, s), 0):
                    lines.append("c %d %d %d %d %d" % (rule, S, word, k, s))
                    want.append(int(RS.cancelled(rule, S, word, k, s)))
        for _ in range(1000):
            S = int(rng.integers(1, 9))
            k, s, kw, sw = int(rng.integers(0, 6)), int(rng.integers(0, S)), int(rng.integers(0, 6)), int(rng.integers(0, S))
            word = RS.key(rule, S, kw, sw) if rng.random() < 0.9 else RS.NO_KEY
            lines.append("c %d %d %d %d %d" % (rule, S, word, k, s))
            want.append(int(RS.cancelled(rule, S, word, k, s)))
    got = [r[0] for r in run(harness, lines)]
    assert got == want
    assert 200 < sum(w == 1 for w in want) and 200 < sum(w == 0 for w in want)
    # the initial word never cancels, even where floor(word / S) <= k would hold
    assert run(harness, ["c 1 %d %d 3 0" % (2 ** 30, RS.NO_KEY), "c 0 4 %d 5 3" % RS.NO_KEY]) == [[0], [0]]


@pytest.mark.parametrize("rule", [RS.FIRST, RS.FEWEST_STEPS])
@pytest.mark.parametrize("S,K", [(1, 3), (2, 3), (3, 2), (4, 1)])
def test_no_interleaving_cancels_the_winner(harness, rule, S, K):
    """Every assignment of outcomes (REACHED or not, at step 0 .. K) to S seeds,
    every order of their steps, every stale read."""
    (leaves, cancels, bad), = run(harness, ["i %d %d %d" % (rule, S, K)])
    print("rule %d S %d K %d: %d schedules, %d with a cancelled seed" % (rule, S, K, leaves, cancels))
    assert bad == 0
    assert leaves >= (2 * (K + 1)) ** S
    assert (cancels > 0) == (S > 1)   # the check is not vacuous: seeds do get cancelled
