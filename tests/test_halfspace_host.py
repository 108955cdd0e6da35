"""The half-space closed form (csrc/halfspace.hpp) compiled with the host
compiler (tools/halfspace_host_test.cpp) against two independent references:

* the same closed form written in numpy (tests/_obstacles.py), distance and
  both witnesses;
* the C oracle's narrow phase on the twin of the half-space, a box of 20 m half
  extents with its +z face in the plane (GJK / EPA, then the exact witness
  refinement D17), distance.

200 random states of FR3 and plane poses x FR3's three primitive types (a
sphere, a cylinder and the box of link 7), separated and penetrating.

Tolerance 1e-12 on the distance, as the two references agree with each other
to 1.6e-14 on such cases: the values are O(1) sums of a few products, so each
side carries a few ulp (1e-16).  The witnesses of the closed form and of its
numpy restatement are the same few products as well: 1e-12."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import oracle as O
import _obstacles as OB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.environ.get("CXX", "g++")
N = 200
TOL = 1e-12


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if not shutil.which(CXX):
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("hs") / "halfspace_host")
    subprocess.check_call([CXX, "-O2", "-std=c++17", "-ffp-contract=off",
                           os.path.join(ROOT, "tools", "halfspace_host_test.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def cases():
    """Per case: (type, params, shape pose R, c, plane pose R, p, oracle d)."""
    pm, om, spec, g0 = OB.twin("fr3", (OB.HALFSPACE,), ((0, 0, 0),), OB.FR3_ARM_LINKS)
    p0 = len(pm.pairs)
    with_ = [g for g in range(g0) if pm.geoms[g]["link"] in OB.FR3_ARM_LINKS]
    pick = {}   # one geometry per primitive type
    for k, g in enumerate(with_):
        pick.setdefault(om.gtype[g], (k, g))
    assert sorted(pick) == [OB.SPHERE, OB.CYLINDER, OB.BOX]
    q, _ = OB.fr3_states(om, 5, N)
    poses = OB.fr3_scene(21, N, types=(OB.HALFSPACE,), back=(-0.2, 0.6))
    out = []
    for b in range(N):
        OB.set_poses(om, g0, (OB.HALFSPACE,), poses[b])
        Rp, p = poses[b, 0, :9].reshape(3, 3).T, poses[b, 0, 9:]
        for t, (k, g) in sorted(pick.items()):
            Tj = O.joint_placement(om, q[:, b], om.gparent[g])
            gp = np.array([om.gplace[g][i] for i in range(12)])
            Tg = np.eye(4)
            Tg[:3, :3], Tg[:3, 3] = gp[:9].reshape(3, 3), gp[9:]
            Tw = Tj @ Tg
            d_or, _, _ = O.pair_distance(om, q[:, b], p0 + k)
            prm = [om.gparam[g][i] for i in range(3)]
            out.append((t, prm, Tw[:3, :3].copy(), Tw[:3, 3].copy(), Rp, p, d_or))
    return out


def run_harness(exe, cases):
    lines = []
    for t, prm, Rg, c, Rp, p, _ in cases:
        vals = list(prm) + list(Rg.reshape(-1)) + list(c) + list(Rp.reshape(-1)) + list(p)
        lines.append("%d " % t + " ".join("%.17g" % v for v in vals))
    res = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True)
    rows = np.array([[float(x) for x in ln.split()] for ln in res.stdout.strip().splitlines()])
    assert rows.shape == (len(cases), 7)
    return rows


def test_cases_cover_both_sides(cases):
    for t in (OB.SPHERE, OB.CYLINDER, OB.BOX):
        d = np.array([c[6] for c in cases if c[0] == t])
        assert len(d) == N and (d > 0).sum() >= 20 and (d < 0).sum() >= 20, (t, (d > 0).sum(), (d < 0).sum())


def test_against_numpy_closed_form(harness, cases):
    rows = run_harness(harness, cases)
    worst = 0.0
    for r, (t, prm, Rg, c, Rp, p, _) in zip(rows, cases):
        d, ps, pp = OB.halfspace_closed_form(t, prm, Rg, c, Rp, p)
        worst = max(worst, abs(r[0] - d), np.abs(r[1:4] - ps).max(), np.abs(r[4:7] - pp).max())
        # the witnesses: one on the shape's side of d, one in the plane, d n apart
        n = Rp[:, 2]
        assert abs(n @ (r[4:7] - p)) <= TOL and np.abs(r[1:4] - r[4:7] - r[0] * n).max() <= TOL
    print("closed form vs numpy: worst %.3g" % worst)
    assert worst <= TOL, worst


def test_against_oracle_big_box(harness, cases):
    rows = run_harness(harness, cases)
    err = np.abs(rows[:, 0] - np.array([c[6] for c in cases]))
    print("closed form vs the oracle's big-box twin: worst %.3g" % err.max())
    assert err.max() <= TOL, (err.max(), int(err.argmax()))
