"""Model tables of the wave task stage (csrc/model.cpp build_stage_tables),
checked on the CPU: tools/stage_tables_host_test.cpp builds each model with
model.cpp and compares every per-slot record with the gather it replaces
(pair_order -> pair_a / pair_b -> gtype / gparam / gbound) and the joint masks
(rev_mask, anc_bits) with jtype / anc.

Models: the five bundled robots (chains and trees) and the synthetic 5-joint
trees of tests/test_gpu_task_fixed_stages.py (a branch, a prismatic joint; 70,
3 and 0 pairs)."""
import os
import shutil
import subprocess

import pytest

from dyros_robot_controller_amd import robot_path
from test_gpu_task_fixed_stages import GEOMS_1, GEOMS_3, GEOMS_70, tree_urdf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.environ.get("CXX", "g++")
CSRC = os.path.join(ROOT, "dyros_robot_controller_amd", "csrc")
ROBOTS = ("fr3", "ur5e", "husky_fr3", "xls_fr3", "caster_fr3")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if not shutil.which(CXX):
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("st") / "stage_tables_host")
    subprocess.check_call([CXX, "-O1", "-std=c++17", os.path.join(ROOT, "tools", "stage_tables_host_test.cpp"),
                           os.path.join(CSRC, "model.cpp"), os.path.join(CSRC, "mesh.cpp"), "-o", exe])
    return exe


def run(exe, models):
    args = [exe]
    for urdf, srdf in models:
        args += [urdf, srdf or "-"]
    res = subprocess.run(args, capture_output=True, text=True)
    lines = res.stdout.strip().splitlines()
    assert res.returncode == 0 and len(lines) == len(models), (res.stdout, res.stderr)
    return [[int(x) for x in ln.split()[1:]] for ln in lines if ln.startswith("ok ")]


def test_bundled_robots(harness):
    out = run(harness, [(robot_path(r), robot_path(r, "srdf")) for r in ROBOTS])
    assert len(out) == len(ROBOTS)
    assert [o[0] for o in out] == [7, 6, 12, 14, 14], out
    assert all(o[2] > 0 for o in out)


def test_synthetic_trees(harness, tmp_path):
    models = []
    for name, geoms in (("pairs70", GEOMS_70), ("pairs3", GEOMS_3), ("pairs0", GEOMS_1)):
        urdf = str(tmp_path / (name + ".urdf"))
        tree_urdf(urdf, geoms)
        models.append((urdf, None))
    out = run(harness, models)
    assert out == [[5, 13, 70], [5, 3, 3], [5, 1, 0]], out
