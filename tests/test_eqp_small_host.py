"""Dense core of the polish's small EQP (csrc/eqp_small.hpp: LDL^T of the
regularised reduced KKT, solve, iterative refinement against the unregularised
one) compiled for the host and checked against numpy.linalg.solve on random
quasi-definite systems [P_FF, G^T; G, 0] of every size the tier takes.

Runs on the CPU: hipcc compiles the DRC_HD functions as plain host code
(tools/eqp_small_host_test.hip, which pads each system to the tier exactly as
the kernel does).

Tolerance.  The method (regularise by delta, factor without pivoting, refine
three times against K0) has an error of its own, far above one rounding when
delta meets the slack-like pivots.  It is measured, not guessed: the same
inputs go through a plain double-precision restatement of the method written
in numpy below, and the harness must stay within 10x the worst relative error
of that restatement.  Attained (delta 1e-6, 3 refinements, seeds below):
NS = 4: restatement worst 4.2e-11, harness worst 4.2e-11 over 192 systems;
NS = 8: both 1.2e-3 over 528 systems (a nearly singular square G, nF = nR = 3:
the method's own limit); medians 1.5e-16 to 2.4e-16.  The worst cases coincide:
the two differ only in the order of a few sums."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
DELTA, REFINE = 1e-6, 3  # drc_default_qpik_params: OSQP's polish delta and refinement count
TIERS = (4, 8)           # 4: the tier the kernels compile (kEqpSmallCap); 8: the template's next size
SEEDS = 24


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if not shutil.which(HIPCC) and not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    exe = str(tmp_path_factory.mktemp("es") / "eqp_small_host")
    subprocess.check_call([HIPCC, "-O2", "-std=c++17", "-ffp-contract=on", "--offload-arch=gfx950", "--cuda-host-only",
                           os.path.join(ROOT, "tools", "eqp_small_host_test.hip"), "-o", exe])
    return exe


def make_system(rng, nF, nR):
    """K0 = [P_FF, G^T; G, 0]: P_FF the leading block of 2 J^T J + I for a
    random 6 x 7 J (the QPIK cost), nR random G rows; a random right-hand side."""
    J = rng.normal(size=(6, 7))
    P = (2 * J.T @ J + np.eye(7))[:nF, :nF]
    G = rng.normal(size=(nR, nF))
    N = nF + nR
    K0 = np.zeros((N, N))
    K0[:nF, :nF] = P
    K0[nF:, :nF] = G
    K0[:nF, nF:] = G.T
    return K0, rng.normal(size=N)


def run_harness(exe, ns, systems, delta=DELTA, refine=REFINE):
    lines = []
    for nF, nR, K0, b in systems:
        lines.append(" ".join(["%d %d %d %.17g %d" % (ns, nF, nR, delta, refine)] +
                              ["%.17g" % v for v in K0.reshape(-1)] + ["%.17g" % v for v in b]))
    res = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True)
    rows = [ln.split() for ln in res.stdout.strip().splitlines()]
    assert len(rows) == len(systems)
    return [(int(r[0]), np.array([float(x) for x in r[1:]])) for r in rows]


def ldl_restated(K0, b, nF, delta=DELTA, refine=REFINE):
    """The method in plain numpy: LDL^T (natural order) of K0 + diag(+delta on
    the free block, -delta on the rows), solve, `refine` refinement steps
    against K0.  None on a zero pivot."""
    N = len(b)
    K = K0 + np.diag([delta] * nF + [-delta] * (N - nF))
    L, d = np.eye(N), np.zeros(N)
    for j in range(N):
        d[j] = K[j, j] - np.sum(L[j, :j] ** 2 * d[:j])
        if d[j] == 0.0:
            return None
        for i in range(j + 1, N):
            L[i, j] = (K[i, j] - np.sum(L[i, :j] * L[j, :j] * d[:j])) / d[j]

    def solve(r):
        y = r.copy()
        for j in range(N):
            y[j + 1:] -= L[j + 1:, j] * y[j]
        y /= d
        for j in range(N - 1, -1, -1):
            y[:j] -= L[j, :j] * y[j]
        return y
    sol = solve(b)
    for _ in range(refine):
        sol = sol + solve(b - K0 @ sol)
    return sol


def relerr(a, ref):
    return np.abs(a - ref).max() / max(np.abs(ref).max(), 1e-300)


@pytest.mark.parametrize("ns", TIERS)
def test_matches_numpy_solve(harness, ns):
    """N = 1 .. NS, every split into free variables and 0 - 3 active rows with a
    nonsingular K0 (nR <= nF): relative error against numpy.linalg.solve on K0
    within 10x what the numpy restatement of the method attains."""
    rng = np.random.default_rng(100 + ns)
    systems = []
    for N in range(1, ns + 1):
        for nR in range(max(0, N - 7), min(3, N // 2) + 1):  # nR = 0: the degenerate case without rows (P_FF is at most 7 x 7)
            for _ in range(SEEDS):
                K0, b = make_system(rng, N - nR, nR)
                systems.append((N - nR, nR, K0, b))
    assert {nF + nR for nF, nR, _, _ in systems} == set(range(1, ns + 1))
    out = run_harness(harness, ns, systems)
    e_dev, e_ref = [], []
    for (nF, nR, K0, b), (ok, sol) in zip(systems, out):
        N = nF + nR
        exact = np.linalg.solve(K0, b)
        assert ok == 1
        assert np.all(sol[N:] == 0.0)  # the padding is inert
        e_dev.append(relerr(sol[:N], exact))
        e_ref.append(relerr(ldl_restated(K0, b, nF), exact))
    e_dev, e_ref = np.array(e_dev), np.array(e_ref)
    print("NS=%d: %d systems, restatement worst %.3e, harness worst %.3e (median %.1e / %.1e)"
          % (ns, len(systems), e_ref.max(), e_dev.max(), np.median(e_ref), np.median(e_dev)))
    assert e_dev.max() <= 10 * e_ref.max(), (e_dev.max(), e_ref.max())


@pytest.mark.parametrize("ns", TIERS)
def test_degenerate_blocks(harness, ns):
    """N = 0 (nothing to solve: all zeros, success), and active rows without a
    free variable (nF = 0): K0 is the zero matrix there, so numpy.linalg.solve
    has no answer; the regularised system -delta I does, and every refinement
    step adds the same -rhs / delta.  Compared with the numpy restatement and
    with that closed form."""
    rng = np.random.default_rng(200 + ns)
    ok, sol = run_harness(harness, ns, [(0, 0, np.zeros((0, 0)), np.zeros(0))])[0]
    assert ok == 1 and np.all(sol == 0.0)
    systems = [(0, nR, *make_system(rng, 0, nR)) for nR in range(1, min(3, ns) + 1)]
    for (nF, nR, K0, b), (ok, sol) in zip(systems, run_harness(harness, ns, systems)):
        assert ok == 1 and np.all(sol[nR:] == 0.0)
        ref = ldl_restated(K0, b, 0)
        assert relerr(sol[:nR], ref) <= 1e-15
        assert relerr(sol[:nR], -b * (1 + REFINE) / DELTA) <= 1e-15


@pytest.mark.parametrize("ns", TIERS)
def test_zero_pivot_fails(harness, ns):
    """An exactly singular regularised system returns failure: a zero first
    pivot, and a zero second pivot (delta = 2^-20 keeps every value exact)."""
    d = 2.0 ** -20
    first = (1, 0, np.array([[-d]]), np.array([1.0]))
    second = (2, 0, np.array([[1 - d, 1.0], [1.0, 1 - d]]), np.array([1.0, 2.0]))
    assert ldl_restated(first[2], first[3], 1, delta=d) is None
    assert ldl_restated(second[2], second[3], 2, delta=d) is None
    for ok, _ in run_harness(harness, ns, [first, second], delta=d):
        assert ok == 0
    # ... and the same blocks at the solver's delta are regular
    for ok, _ in run_harness(harness, ns, [first, second]):
        assert ok == 1
