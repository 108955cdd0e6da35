"""The serial PinvCOD routines of csrc/pinv_cod.hpp (pinv_cod_serial: the
dynamics' M and the 6 x 6 J J^T; pinv_cod_rect: CLIK's J) compiled for the host
and checked against a 50-digit mpmath restatement of DyrosMath::PinvCOD:
column-pivoted QR, rank = pivots above 1e-6 of the largest, Moore-Penrose
inverse of the QR-truncated matrix.

Runs on the CPU: hipcc compiles the DRC_HD functions as plain host code
(tools/pinv_cod_host_test.hip).  A second build of the same program with
-fsanitize=address,undefined runs the same inputs with every array in its own
heap block of exactly the documented size (3n^2 + 3n; m n + m m + n m + 3m +
2n), and, for m = 6, once more in the layout closed_form_stage uses inside the
block its LDS plan reserves; its output must equal the plain build's bit for
bit.

Inputs.  Symmetric n x n, n = 2 .. 12, element strides 1 and 16 (the dynamics
kernel's), and 6 x n, n = 2 .. 9.  Per size: full rank (class K of
tests/_singular.py), graded spectra drawn until they land in class F (every
pivot kept, certificate refused) and class T (modes dropped, each a factor
>= 3 from the cut), and exact deficiency: U U^T / a rank-3 product, columns
repeated at another scale, a zero column, the zero matrix.  Column norms are
never tied, so the pivot order is unique; no input is ambiguous.

Tolerance.  Measured, not guessed: the same inputs go through pyref.pinv_cod
(LAPACK's pivoted QR), and per class the harness's worst relative error
against mpmath must stay within 10x pyref's worst.  Attained (seeds below;
relative to max|X|; harness / pyref, number of inputs):
  symmetric  K 3.5e-15 / 2.5e-15 (33)   F 1.5e-11 / 3.6e-11 (33)
             T 7.5e-14 / 3.4e-14 (33)   deficient 5.6e-14 / 4.5e-14 (44)
  6 x n      K 1.2e-14 / 1.0e-14 (30)   F 1.2e-11 / 3.6e-12 (24)
             T 1.8e-14 / 2.7e-14 (24)   deficient 2.7e-15 / 1.8e-15 (26)
(both strides give the same figures).  Class F is the method's own limit:
forming W W^T squares a condition number of 3e5 on both sides.  With the rank
decision of pinv_cod_rect ignored (r = 6, a scratch copy) the 6 x n class T
misses by 5e9."""
import os
import shutil
import subprocess

import mpmath as mp
import numpy as np
import pytest

import pyref as R
import _singular as SG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SRC = os.path.join(ROOT, "tools", "pinv_cod_host_test.hip")
SYM_N, RECT_N, STRIDES = range(2, 13), range(2, 10), (1, 16)
PER_SIZE = 3
DIGITS = 50


def _build(path, extra):
    subprocess.check_call([HIPCC, "-O2", "-std=c++17", "-ffp-contract=on", "--offload-arch=gfx950", "--cuda-host-only",
                           *extra, SRC, "-o", path])
    return path


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if not shutil.which(HIPCC) and not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    return _build(str(tmp_path_factory.mktemp("pc") / "pinv_cod_host"), [])


@pytest.fixture(scope="module")
def harness_san(tmp_path_factory):
    if not shutil.which(HIPCC) and not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    return _build(str(tmp_path_factory.mktemp("pcs") / "pinv_cod_host_san"),
                  ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])


# -- the 50-digit reference ---------------------------------------------------
def pinv_cod_mp(A, thr=1e-6):
    """PinvCOD at 50 digits: pivoted QR (modified Gram-Schmidt, which at this
    precision is as good as Householder), rank by |R_kk| > thr |R_00|, then
    P W^T (W W^T)^-1 Q_r^T with W = R[:r, :]."""
    with mp.workdps(DIGITS):
        m, n = A.shape
        a = [[mp.mpf(float(A[i, j])) for i in range(m)] for j in range(n)]  # columns
        perm = list(range(n))
        kmax = min(m, n)
        Q, Rm = [], [[mp.mpf(0)] * n for _ in range(kmax)]
        for k in range(kmax):
            nrm = [mp.sqrt(sum(x * x for x in a[j])) for j in range(k, n)]
            p = k + max(range(len(nrm)), key=lambda i: nrm[i])
            a[k], a[p] = a[p], a[k]
            perm[k], perm[p] = perm[p], perm[k]
            for row in Rm:
                row[k], row[p] = row[p], row[k]
            d = nrm[p - k]
            if d == 0 or (k and d < mp.mpf(10) ** -40 * Rm[0][0]):
                break
            q = [x / d for x in a[k]]
            Q.append(q)
            Rm[k][k] = d
            for j in range(k + 1, n):
                c = sum(x * y for x, y in zip(q, a[j]))
                Rm[k][j] = c
                a[j] = [y - c * x for x, y in zip(q, a[j])]
        X = np.zeros((n, m))
        if not Q:
            return X, 0
        r = sum(1 for k in range(len(Q)) if Rm[k][k] > mp.mpf(thr) * Rm[0][0])
        W = mp.matrix([[Rm[i][j] for j in range(n)] for i in range(r)])
        Qr = mp.matrix([[Q[i][j] for j in range(m)] for i in range(r)])   # Q_r^T
        Z = W.T * (mp.inverse(W * W.T) * Qr)
        for c in range(n):
            for j in range(m):
                X[perm[c], j] = float(Z[c, j])
        return X, r


# -- inputs -------------------------------------------------------------------
def _orth(rng, n):
    return np.linalg.qr(rng.normal(size=(n, n)))[0]


def _untie(A):
    """Scales column j (and row j of a square matrix, which keeps it symmetric)
    by its own factor, so that equal columns of a construction do not tie."""
    s = 1.0 + 0.03 * np.arange(A.shape[1])
    return (A * s) * (s[:, None] if A.shape[0] == A.shape[1] else 1.0)


def _graded(rng, m, n, want):
    """A = U diag(s) V^T (V = U for the square PSD case) with a log-uniform
    spectrum, redrawn until tests/_singular.py puts it in class `want`."""
    k = min(m, n)
    for _ in range(4000):
        if want == SG.F:   # smallest mode just above the cut: certificate refused, nothing dropped
            lo = rng.uniform(3.5e-6, 6e-6) if m == n else rng.uniform(1e-5, 1e-3)
            s = np.concatenate([[1.0], np.exp(rng.uniform(np.log(lo), 0, k - 2)), [lo]]) if k > 1 else np.ones(1)
        else:              # some modes far below the cut
            nd = int(rng.integers(1, k))
            s = np.concatenate([np.exp(rng.uniform(np.log(1e-3), 0, k - nd)), np.exp(rng.uniform(np.log(1e-10), np.log(1e-8), nd))])
        U = _orth(rng, m)
        V = U if m == n else _orth(rng, n)
        A = (U[:, :k] * s) @ V[:, :k].T
        A = (A + A.T) / 2 if m == n else A
        if _class(A) == want:
            return A
    raise AssertionError("no %s input for %d x %d" % (want, m, n))


def _class(A):
    m, n = A.shape
    return SG.classify(A) if m == n else SG.classify(A, A @ A.T)


def _deficient(rng, m, n):
    """Exactly rank-deficient inputs: a low-rank product, a column repeated at
    another scale, a zero column, the zero matrix."""
    out = []
    if m == n:
        U = rng.normal(size=(n, max(1, n // 2)))
        out.append(_untie(U @ U.T))
        B = rng.normal(size=(n, n))
        B[1] = 0.5 * B[0]                 # row (and column) 1 of B B^T is half of row 0
        out.append(B @ B.T)
        C = rng.normal(size=(n, n))
        C[n - 1] = 0
        out.append(_untie(C @ C.T))       # a zero row and column
    else:
        out.append(_untie(rng.normal(size=(m, 1)) @ rng.normal(size=(1, n)) if n < 4 else
                          rng.normal(size=(m, 3)) @ rng.normal(size=(3, n))))
        A = _untie(rng.normal(size=(m, n)))
        A[:, 1] = 0.5 * A[:, 0]
        out.append(A)
        A = _untie(rng.normal(size=(m, n)))
        A[:, n - 1] = 0
        out.append(A)
    out.append(np.zeros((m, n)))
    return out


def _inputs(kind):
    """[(label, A)]: label K / F / T from the classifier, or "deficient"."""
    rng = np.random.default_rng(20 if kind == "S" else 21)
    cases = []
    for n in (SYM_N if kind == "S" else RECT_N):
        m = n if kind == "S" else 6
        # 6 x n, n < 6: J J^T is singular, so no such input is in class K
        for _ in range(PER_SIZE if kind == "S" else (2 * PER_SIZE if n >= 6 else 0)):
            if kind == "S":
                B = rng.normal(size=(n, n + 2))
                cases.append((SG.K, _untie(B @ B.T + 0.5 * np.eye(n))))
            else:
                cases.append((SG.K, _untie(rng.normal(size=(m, n)) + 2 * np.eye(m, n))))
        for _ in range(PER_SIZE):
            cases.append((SG.F, _graded(rng, m, n, SG.F)))
            cases.append((SG.T, _graded(rng, m, n, SG.T)))
        # (a 6 x n input with n > 6 survives a repeated or zero column at full rank: it
        # then carries its own class, still with a column the pivoting must pass over)
        for A in _deficient(rng, m, n):
            cases.append(("deficient" if not A.any() or _class(A) == SG.T else _class(A), A))
    return cases


def _run(exe, kind, mats, st=1):
    lines = []
    for A in mats:
        m, n = A.shape
        lines.append(" ".join(["%s %d %d" % (kind, n if kind == "S" else m, st if kind == "S" else n)] +
                              ["%.17g" % v for v in A.reshape(-1)]))
    res = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert res.returncode == 0, (res.returncode, res.stderr[-2000:])
    rows = res.stdout.strip().splitlines()
    assert len(rows) == len(mats)
    return [np.array([float(x) for x in r.split()]).reshape(A.shape[1], A.shape[0]) for r, A in zip(rows, mats)], \
        res.stdout


def _relerr(X, ref):
    return np.abs(X - ref).max() / max(np.abs(ref).max(), 1e-300)


_REF = {}


def _reference(kind):
    """Inputs, mpmath answers and pyref's errors, computed once per kind."""
    if kind not in _REF:
        cases = _inputs(kind)
        for label, A in cases:   # the labels are the classifier's, from the reference decomposition alone
            assert label in (SG.K, SG.F, SG.T, "deficient"), (label, A.shape)
            if A.any():
                assert _class(A) == (SG.T if label == "deficient" else label), (label, _class(A), A.shape)
            nrm = np.sort(np.linalg.norm(A, axis=0))
            assert not A.any() or np.all(np.diff(nrm) > 1e-9 * nrm[-1]), "tied column norms"
        exact = [pinv_cod_mp(A) for _, A in cases]
        e_py = np.array([_relerr(R.pinv_cod(A), X) for (_, A), (X, _) in zip(cases, exact)])
        _REF[kind] = (cases, exact, e_py)
    return _REF[kind]


def _check(kind, outs):
    cases, exact, e_py = _reference(kind)
    labels = np.array([c[0] for c in cases])
    e_dev = np.array([_relerr(X, ref) for X, (ref, _) in zip(outs, exact)])
    for (label, A), X, (ref, r) in zip(cases, outs, exact):
        if r == 0:
            assert np.all(X == 0.0)
    for c in (SG.K, SG.F, SG.T, "deficient"):
        sel = labels == c
        assert sel.sum() >= 16, (c, sel.sum())
        print("%s %s: %d inputs, harness worst %.2e, pyref worst %.2e" % (kind, c, sel.sum(), e_dev[sel].max(),
                                                                          e_py[sel].max()))
        assert e_dev[sel].max() <= 10 * max(e_py[sel].max(), np.finfo(float).eps), (c, e_dev[sel].max(), e_py[sel].max())


def test_reference_truncates_where_claimed():
    """The mpmath rank equals the number of pivot ratios above the cut that
    scipy's QR reports, on every input: classes F and K keep all modes, T and
    the deficient inputs drop at least one."""
    for kind in ("S", "R"):
        cases, exact, _ = _reference(kind)
        for (label, A), (_, r) in zip(cases, exact):
            full = min(A.shape)
            assert r == int(np.sum(SG.pivot_ratios(A) > SG.COD_THRESHOLD)), (label, A.shape)
            assert (r == full) == (label in (SG.K, SG.F)), (label, r, A.shape)


@pytest.mark.parametrize("st", STRIDES)
def test_symmetric_matches_mpmath(harness, st):
    cases, _, _ = _reference("S")
    outs, _ = _run(harness, "S", [A for _, A in cases], st)
    _check("S", outs)


def test_rect_matches_mpmath(harness):
    cases, _, _ = _reference("R")
    outs, _ = _run(harness, "R", [A for _, A in cases])
    _check("R", outs)


def test_sanitizer_build_runs_clean(harness, harness_san):
    """The address / undefined-behaviour build of the same stand-alone program:
    exit status 0 (no report; the stage-layout and stride-gap checks of the
    harness pass) and the plain build's output bit for bit."""
    for kind, strides in (("S", STRIDES), ("R", (1,))):
        mats = [A for _, A in _reference(kind)[0]]
        for st in strides:
            assert _run(harness_san, kind, mats, st)[1] == _run(harness, kind, mats, st)[1]
