"""Bookkeeping of the obstacle slots (csrc/model.cpp set_obstacles), checked
on the CPU: tools/obstacle_tables_host_test.cpp builds each model with
model.cpp, declares a sphere, a box, a cylinder and a half-space, and checks
the counts (geometries + n, pairs + n x geometries of the listed links), the
order of the new pairs, every pair's pair_tab record against the plain gather,
the type-class order (half-space pairs last), that n = 0 restores the tables
byte for byte, and that the limits (64 geometries, 1024 pairs) and the
refusals (mesh obstacle, unknown link, bad type or size, a model with hulls)
return their codes and leave the model alone.

Models: FR3 with the links moved by joint 3 and beyond, FR3 and Husky-FR3 with
every moving link, a synthetic 5-joint tree (70 pairs), and a one-hull model."""
import os
import shutil
import subprocess

import pytest

from dyros_robot_controller_amd import robot_path
from test_gpu_task_fixed_stages import GEOMS_70, tree_urdf
import _obstacles as OB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.environ.get("CXX", "g++")
CSRC = os.path.join(ROOT, "dyros_robot_controller_amd", "csrc")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if not shutil.which(CXX):
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("ob") / "obstacle_tables_host")
    subprocess.check_call([CXX, "-O1", "-std=c++17", os.path.join(ROOT, "tools", "obstacle_tables_host_test.cpp"),
                           os.path.join(CSRC, "model.cpp"), os.path.join(CSRC, "mesh.cpp"), "-o", exe])
    return exe


def run(exe, models):
    args = [exe]
    for urdf, srdf, links in models:
        args += [urdf, srdf or "-", ",".join(links) if links else "-"]
    res = subprocess.run(args, capture_output=True, text=True)
    lines = res.stdout.strip().splitlines()
    assert res.returncode == 0 and len(lines) == len(models), (res.stdout, res.stderr)
    return lines


def test_bundled_robots(harness):
    fr3 = (robot_path("fr3"), robot_path("fr3", "srdf"))
    husky = (robot_path("husky_fr3"), robot_path("husky_fr3", "srdf"))
    out = run(harness, [fr3 + (OB.FR3_ARM_LINKS,), fr3 + (None,), husky + (None,),
                        husky + (("base_link",) + OB.FR3_ARM_LINKS,)])
    rows = [[int(x) for x in ln.split()[1:]] for ln in out if ln.startswith("ok ")]
    # geometries, pairs, then with the four slots, and the geometries they are paired with
    assert rows == [[35, 180, 39, 180 + 4 * 23, 23], [35, 180, 39, 180 + 4 * 31, 31],
                    [39, 288, 43, 288 + 4 * 39, 39], [39, 288, 43, 288 + 4 * 25, 25]], out


def test_synthetic_tree(harness, tmp_path):
    urdf = str(tmp_path / "pairs70.urdf")
    tree_urdf(urdf, GEOMS_70)
    out = run(harness, [(urdf, None, None)])
    row = [int(x) for x in out[0].split()[1:]]
    assert out[0].startswith("ok ") and row[:2] == [13, 70] and row[2] == 17 and row[3] == 70 + 4 * row[4], out


def test_hull_model_refuses_obstacles(harness, tmp_path):
    (tmp_path / "tet.obj").write_text("v 0 0 0\nv 0.1 0 0\nv 0 0.1 0\nv 0 0 0.1\nf 1 2 3\n")
    urdf = tmp_path / "hull.urdf"
    urdf.write_text("""<robot name="hull">
  <link name="base"/>
  <link name="arm"><collision><geometry><mesh filename="tet.obj"/></geometry></collision></link>
  <joint name="j1" type="revolute"><parent link="base"/><child link="arm"/><axis xyz="0 0 1"/>
    <limit lower="-1" upper="1" velocity="1" effort="1"/></joint>
</robot>
""")
    assert run(harness, [(str(urdf), None, None)]) == ["ok-hull"]
