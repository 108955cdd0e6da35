"""Path clearance on the CPU: the sample states and the fold rule of
csrc/clearance.hpp compiled with the host compiler
(tools/clearance_host_test.cpp) against what include/drc_amd.h states for
drc_clearance_path_batch, written in numpy and plain Python:

    sample i of a segment, 1 <= i <= substeps:  qb itself for i == substeps,
        otherwise qa + (i / substeps) * (qb - qa)
    d_min = +inf, sample_min = pair_min = -1; for n = 0 .. N - 1 in order:
        d_n NaN      -> INVALID at n, stop
        d_n < d_min  -> (d_min, sample_min, pair_min) = (d_n, n, pair_n)
        d_n < d_stop -> BLOCKED at n, stop
    otherwise FREE, sample_stop = -1

Bit-equal: the quotient, the difference, the product and the sum are each
rounded once on both sides (contraction off).  The new kernel family's cells in
the table of stage builds and the clamp of its grid knob are asked of
csrc/call_plan.hpp through tools/call_plan_host_test.cpp."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.environ.get("CXX", "g++")
FREE, BLOCKED, INVALID = 0, 1, 2
INF, NAN = math.inf, math.nan


def compile_tool(tmp_path_factory, name, flags):
    assert shutil.which(CXX), "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp(name) / name)
    subprocess.check_call([CXX, "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas"] + flags +
                          [os.path.join(ROOT, "tools", name + "_host_test.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return compile_tool(tmp_path_factory, "clearance", ["-O2", "-ffp-contract=off"])


@pytest.fixture(scope="module")
def plan_tool(tmp_path_factory):
    return compile_tool(tmp_path_factory, "call_plan", ["-O1"])


def run(exe, lines):
    res = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert res.returncode == 0, (res.stdout[-300:], res.stderr[-300:])
    out = res.stdout.strip().splitlines()
    assert len(out) == len(lines)
    return out


def hexf(x):
    return "nan" if x != x else float(x).hex()


def bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64)


# ---- the sample states ------------------------------------------------------
def test_samples_equal_numpy_bit_for_bit(harness):
    rng = np.random.default_rng(5)
    n = 1000
    qa = rng.uniform(-3.2, 3.2, n)
    qb = np.where(rng.random(n) < 0.1, qa, qa + rng.uniform(-3, 3, n) * 10.0 ** -rng.integers(0, 12, n))
    sub = rng.integers(1, 17, n)
    out = run(harness, ["s %s %s %d" % (hexf(a), hexf(b), s) for a, b, s in zip(qa, qb, sub)])
    for k in range(n):
        got = np.array([float.fromhex(t) for t in out[k].split()])
        assert got.shape == (sub[k],)
        i = np.arange(1, sub[k] + 1)
        want = qa[k] + (i / sub[k]) * (qb[k] - qa[k])   # rounded: quotient, difference, product, sum
        want[-1] = qb[k]                                # i == substeps: the waypoint itself
        assert np.array_equal(bits(got), bits(want)), (k, qa[k], qb[k], sub[k])


def test_last_sample_is_the_waypoint_where_the_formula_is_not(harness):
    """qa + 1.0 * (qb - qa) is not qb for every pair of doubles: the rule for
    i == substeps is what makes consecutive segments meet in the waypoint."""
    rng = np.random.default_rng(6)
    qa, qb = rng.uniform(-3, 3, 4000), rng.uniform(-3, 3, 4000)
    off = np.nonzero(qa + 1.0 * (qb - qa) != qb)[0]
    assert off.size > 0
    out = run(harness, ["s %s %s 3" % (hexf(qa[k]), hexf(qb[k])) for k in off[:50]])
    for k, line in zip(off[:50], out):
        assert float.fromhex(line.split()[-1]) == qb[k]


# ---- the fold ---------------------------------------------------------------
def fold(d, d_stop):
    """(result, sample_stop, d_min, sample_min, pair_min, seen) with pair_n = 100 + n."""
    d_min, s_min, p_min = INF, -1, -1
    for n, x in enumerate(d):
        if x != x:
            return INVALID, n, d_min, s_min, p_min, n + 1
        if x < d_min:
            d_min, s_min, p_min = x, n, 100 + n
        if x < d_stop:
            return BLOCKED, n, d_min, s_min, p_min, n + 1
    return FREE, -1, d_min, s_min, p_min, len(d)


FOLD_CASES = {
    "free": ([0.3, 0.2, 0.25, 0.4], 0.1, (FREE, -1, 0.2, 1, 101, 4)),
    "tie_lowest_sample_wins": ([0.3, 0.2, 0.2, 0.2, 0.5], 0.1, (FREE, -1, 0.2, 1, 101, 5)),
    "tie_at_the_start": ([0.2, 0.2], -INF, (FREE, -1, 0.2, 0, 100, 2)),
    "stop_at_0": ([0.05, 0.5, 0.01], 0.1, (BLOCKED, 0, 0.05, 0, 100, 1)),
    "stop_at_last": ([0.5, 0.4, 0.3, 0.05], 0.1, (BLOCKED, 3, 0.05, 3, 103, 4)),
    "stop_in_the_middle_lower_later": ([0.5, 0.09, 0.01, 0.5], 0.1, (BLOCKED, 1, 0.09, 1, 101, 2)),
    "equal_to_d_stop_is_clear": ([0.5, 0.1, 0.3], 0.1, (FREE, -1, 0.1, 1, 101, 3)),
    "penetrating_no_stop": ([0.1, -0.02, -0.01], -INF, (FREE, -1, -0.02, 1, 101, 3)),
    "d_stop_minus_inf_never_blocks": ([-1e300, -INF, 3.0], -INF, (FREE, -1, -INF, 1, 101, 3)),
    "d_stop_plus_inf_blocks_at_0": ([5.0, 1.0], INF, (BLOCKED, 0, 5.0, 0, 100, 1)),
    "d_stop_plus_inf_d_inf": ([INF, 1.0], INF, (BLOCKED, 1, 1.0, 1, 101, 2)),
    "all_inf": ([INF, INF], 0.1, (FREE, -1, INF, -1, -1, 2)),
    "nan_at_0": ([NAN, 0.5], 0.1, (INVALID, 0, INF, -1, -1, 1)),
    "nan_in_the_middle": ([0.5, 0.3, NAN, 0.01], 0.1, (INVALID, 2, 0.3, 1, 101, 3)),
    "nan_at_0_no_stop": ([NAN], -INF, (INVALID, 0, INF, -1, -1, 1)),
    "nan_after_a_stop_is_never_seen": ([0.5, 0.05, NAN, NAN], 0.1, (BLOCKED, 1, 0.05, 1, 101, 2)),
    "one_sample": ([0.7], 0.1, (FREE, -1, 0.7, 0, 100, 1)),
    "one_sample_blocked": ([0.07], 0.1, (BLOCKED, 0, 0.07, 0, 100, 1)),
}


def parse_fold(line):
    t = line.split()
    return int(t[0]), int(t[1]), float.fromhex(t[2]) if "x" in t[2] else float(t[2]), int(t[3]), int(t[4]), int(t[5])


@pytest.mark.parametrize("name", list(FOLD_CASES))
def test_fold_cases(harness, name):
    d, d_stop, want = FOLD_CASES[name]
    assert fold(d, d_stop) == want, "the restatement itself"
    got = parse_fold(run(harness, ["f %s %d %s" % (hexf(d_stop), len(d), " ".join(hexf(x) for x in d))])[0])
    assert got == want


def test_fold_random_sequences(harness):
    """Random profiles on a coarse grid (ties are common), NaNs sprinkled in,
    every kind of d_stop."""
    rng = np.random.default_rng(8)
    seqs = []
    for _ in range(400):
        n = int(rng.integers(1, 20))
        d = np.round(rng.uniform(-0.05, 0.4, n), 2)
        d[rng.random(n) < 0.04] = NAN
        d_stop = [-INF, INF, 0.0, 0.08, 0.2, float(np.round(rng.uniform(-0.05, 0.4), 2))][int(rng.integers(0, 6))]
        seqs.append((list(map(float, d)), d_stop))
    out = run(harness, ["f %s %d %s" % (hexf(s), len(d), " ".join(hexf(x) for x in d)) for d, s in seqs])
    kinds = set()
    for (d, s), line in zip(seqs, out):
        want = fold(d, s)
        assert parse_fold(line) == want, (d, s)
        kinds.add(want[0])
    assert kinds == {FREE, BLOCKED, INVALID}


# ---- the dispatch plan: the family's builds and the grid knob ------------------
def test_clearance_family_builds(plan_tool):
    out = run(plan_tool, ["has clearance %s" % b for b in ("plain", "mesh", "obst", "rate")])
    assert out == ["has 1", "has 1", "has 1", "has 0"]


@pytest.mark.parametrize("query,grid", [
    ("clear 1", 1), ("clear 100", 100), ("clear 3072", 3072), ("clear 65536", 3072),   # the default: 3 072 waves
    ("grid_clear=2048 clear 65536", 2048), ("grid_clear=3072 clear 2100", 2100),
    ("grid_clear=8 clear 2100", 8), ("grid_clear=15 clear 2100", 8),                    # a multiple of 8 ...
    ("grid_clear=1030 clear 5000", 1024), ("grid_clear=2055 clear 5000", 2048),
    ("grid_clear=24 clear 17", 17),                                                     # ... or one wave per path
])
def test_clearance_grid_clamp(plan_tool, query, grid):
    assert run(plan_tool, [query]) == ["clear %d" % grid]
