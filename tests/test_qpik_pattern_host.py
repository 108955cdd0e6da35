"""csrc/qpik_pattern.hpp -- the fixed sparsity of the manipulator QP-IK
constraint matrix that the QP kernels' sparse G loops follow -- compiled with
the host compiler (tools/qpik_pattern_host_test.cpp).  For N = 6 (UR5e) and
N = 7 (FR3), on G built densely by qp_assemble's rule with random nonzero
gradient rows, unscaled and with random row / column factors:

  * the helper enumerates exactly the nonzero positions of every column and
    every row, in ascending order, and the right slack column;
  * a column's sum over its four rows, split by row parity as the dense passes
    split it, and a row's sum over its listed columns equal the dense sums bit
    for bit on random finite data (zeros and negative zeros included).

Built with contraction off (every product and sum rounded once on both
sides); the device build's fused a += b * c drops the same exact zeros, which
tests/test_gpu_qp_sparse.py checks on the kernels themselves."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.environ.get("CXX", "g++")
CASES = 200


def _build(tmp, name, flags):
    exe = str(tmp / name)
    subprocess.check_call([CXX, "-O2", "-std=c++17"] + flags +
                          [os.path.join(ROOT, "tools", "qpik_pattern_host_test.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def outputs(tmp_path_factory):
    assert shutil.which(CXX), "no host C++ compiler"
    tmp = tmp_path_factory.mktemp("qpik_pattern")
    exes = [_build(tmp, "plain", ["-ffp-contract=off"])]
    res = []
    for exe in exes:
        r = subprocess.run([exe], capture_output=True, text=True)
        res.append((r.returncode, r.stdout))
    return res


@pytest.mark.parametrize("n", [6, 7])
@pytest.mark.parametrize("check", ["pattern", "colsum", "rowsum"])
def test_pattern_and_sums(outputs, check, n):
    ng, nx = 2 * n + 2, 3 * n + 2
    count = {"pattern": CASES * (nx + ng), "colsum": CASES * n * 2, "rowsum": CASES * ng}[check]
    for rc, out in outputs:
        assert "FAIL" not in out, out[:2000]
        assert rc == 0
        assert "ok %s %d %d" % (check, n, count) in out.splitlines(), out[:2000]
