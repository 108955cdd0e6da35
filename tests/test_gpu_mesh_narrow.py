"""The hull narrow phase on the GPU, pair by pair (tests/gpu_mesh_narrow.hip:
gjk_wave, epa_run_wave with the cooperative hull support and
sphere_hull_witness, the functions task_stage.hpp runs for a pair with a hull,
one wavefront per pair), against a scipy restatement.

Reference for hull-hull, hull-box (the box as its 8 corners) and hull-sphere
(the centre as one point, the radius taken off afterwards): the convex hull of
all differences a_i - b_j.  The origin inside it (every facet offset <= 0):
the penetration depth is the smallest -offset; otherwise the distance is the
smallest closed-form point-triangle distance from the origin over the facets.

Tolerances: separated polytope pairs end exactly (GJK runs until the support
point repeats), so the distance stage's 1e-9 of tests/test_gpu_golden.py
applies unchanged; penetrating pairs get test_gpu_narrow.py's EPA bound, 2e-6
(EPA stops at a 1e-6 support gap).  Hull-cylinder has no polytope reference:
each pair runs with a box primitive and with the same box as an 8-vertex hull,
which pins the hull path to the path the oracle already verifies."""
import ctypes as C
import os

import numpy as np
import pytest
from scipy.spatial import ConvexHull

from _mesh_io import point_hull_distance

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

SPHERE, CYL, BOX, MESH = 0, 1, 2, 3
VCOUNTS = (4, 5, 63, 64, 65, 256)  # smallest solid; around the lane stride; the cap


def _rot(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def _pose(R, t):
    return np.concatenate([R.reshape(-1), t])


def _ellipsoid_hull(rng, n):
    """n points on an ellipsoid: every one is a vertex of their hull."""
    while True:
        p = rng.normal(size=(n, 3))
        p = p / np.linalg.norm(p, axis=1)[:, None] * rng.uniform(0.05, 0.12, size=3)
        if n > 5 or abs(np.linalg.det(p[1:4] - p[0])) > 1e-5:
            return p


def _box_corners(h):
    return np.array([[sx * h[0], sy * h[1], sz * h[2]] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)])


class Cases:
    """Shape pairs for the harness: 36 doubles a pair, one vertex buffer."""

    def __init__(self):
        self.rows, self.verts, self.nv = [], [], 0
        self.world = []  # per pair: (points of A, points of B, sphere radius) in the world, for the reference

    def hull(self, pts):
        first = self.nv
        self.verts.append(np.asarray(pts, dtype=float))
        self.nv += len(pts)
        lo, hi = pts.min(axis=0), pts.max(axis=0)
        return (MESH, 0.5 * (hi - lo), first, len(pts), pts)

    @staticmethod
    def prim(kind, prm):
        pts = _box_corners(prm) if kind == BOX else np.zeros((1, 3))
        return (kind, np.asarray(prm, dtype=float), 0, 0, pts)

    def add(self, a, Ra, ta, b, Rb, tb):
        self.rows.append(np.concatenate([[a[0]], _pose(Ra, ta), a[1], [a[2], a[3]],
                                         [b[0]], _pose(Rb, tb), b[1], [b[2], b[3]]]))
        rs = a[1][0] if a[0] == SPHERE else (b[1][0] if b[0] == SPHERE else 0.0)
        self.world.append((a[4] @ Ra.T + ta, b[4] @ Rb.T + tb, rs))

    def run(self):
        so = os.path.join(ROOT, "tests", "_mesh_narrow_gpu.so")
        if not os.path.exists(so):
            raise RuntimeError("tests/_mesh_narrow_gpu.so missing: run build.sh")
        lib = C.CDLL(so)
        buf = np.ascontiguousarray(np.array(self.rows))
        verts = np.ascontiguousarray(np.vstack(self.verts))
        out = np.zeros((len(buf), 9))
        dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        assert lib.drc_test_mesh_narrow(dp(buf), C.c_int(len(buf)), dp(verts), C.c_int(len(verts)), dp(out)) == 0
        return out


def reference_distance(PA, PB, rs):
    """Signed distance of conv(PA) and conv(PB) (minus the sphere radius rs)."""
    diff = (PA[:, None, :] - PB[None, :, :]).reshape(-1, 3)
    h = ConvexHull(diff)
    if np.all(h.equations[:, 3] <= 0):
        d = -np.min(-h.equations[:, 3])
    else:
        d = point_hull_distance(np.zeros(3), diff, h.simplices)
    return d - rs


def polytope_cases(seed=5):
    rng = np.random.default_rng(seed)
    cs = Cases()
    hulls = {v: [cs.hull(_ellipsoid_hull(rng, v)) for _ in range(3)] for v in VCOUNTS}
    for v in VCOUNTS:
        for k in range(75):
            a = hulls[v][k % 3]
            kind = k % 3
            if kind == 0:  # another hull (two 256-vertex hulls meet a few times only: 65 536 differences each)
                w = VCOUNTS[(k // 3) % len(VCOUNTS)]
                if v == 256 and w == 256 and k >= 40:
                    w = 64
                b = hulls[w][(k // 3) % 3]
            elif kind == 1:
                b = Cases.prim(BOX, rng.uniform(0.03, 0.1, size=3))
            else:
                b = Cases.prim(SPHERE, [rng.uniform(0.02, 0.08), 0, 0])
            ta = rng.uniform(-0.5, 0.5, size=3)
            t = rng.normal(size=3)
            tb = ta + t * rng.uniform(0.0, 0.26) / np.linalg.norm(t)
            Ra, Rb = _rot(rng), _rot(rng)
            if k % 2:  # either order
                cs.add(b, Rb, tb, a, Ra, ta)
            else:
                cs.add(a, Ra, ta, b, Rb, tb)
    return cs


@pytest.fixture(scope="module")
def polytope_results(cuda):
    cs = polytope_cases()
    ref = np.array([reference_distance(*w) for w in cs.world])
    return cs, cs.run(), ref


def test_hull_pairs_match_scipy(polytope_results):
    cs, dev, ref = polytope_results
    rows = np.array(cs.rows)
    sphere = (rows[:, 0] == SPHERE) | (rows[:, 18] == SPHERE)
    pen = ref < 0
    assert len(ref) >= 440 and pen.sum() >= 100 and (~pen).sum() >= 100, (len(ref), pen.sum())
    # penetration flags: GJK's own for two polytopes; a sphere overlaps once its radius reaches the hull
    assert np.array_equal(dev[~sphere, 7] == 1, pen[~sphere])
    assert np.array_equal(dev[:, 0] < 0, pen)
    err = np.abs(dev[:, 0] - ref)
    print("separated: max |d - ref| %.3e; penetrating: max %.3e, median %.3e" %
          (err[~pen].max(), err[pen].max(), np.median(err[pen])))
    assert err[~pen].max() <= 1e-9, (err[~pen].max(), int(np.argmax(np.where(pen, 0, err))))
    assert err[pen].max() <= 2e-6, (err[pen].max(), int(np.argmax(np.where(pen, err, 0))))
    # the witnesses realise the distance
    gap = np.linalg.norm(dev[:, 4:7] - dev[:, 1:4], axis=1)
    assert np.max(np.abs(gap - np.abs(dev[:, 0]))) <= 1e-9
    # the cooperative and the lane-serial support scan run the same GJK: same bits
    sep = ~sphere & (dev[:, 7] == 0)
    assert np.array_equal(dev[sep, 0], dev[sep, 8])


def test_hull_cylinder_matches_box_primitive(cuda):
    rng = np.random.default_rng(11)
    prim, mesh = Cases(), Cases()
    mesh.hull(np.zeros((1, 3)))  # (vertex 0 unused: the hulls below do not start at offset 0)
    for k in range(120):
        h = rng.uniform(0.03, 0.1, size=3)
        cyl = Cases.prim(CYL, [rng.uniform(0.03, 0.08), rng.uniform(0.03, 0.12), 0])
        Ra, Rb, ta = _rot(rng), _rot(rng), rng.uniform(-0.5, 0.5, size=3)
        t = rng.normal(size=3)
        tb = ta + t * rng.uniform(0.0, 0.24) / np.linalg.norm(t)
        box_h = mesh.hull(_box_corners(h)[rng.permutation(8)])
        if k % 2:
            prim.add(cyl, Rb, tb, Cases.prim(BOX, h), Ra, ta)
            mesh.add(cyl, Rb, tb, box_h, Ra, ta)
        else:
            prim.add(Cases.prim(BOX, h), Ra, ta, cyl, Rb, tb)
            mesh.add(box_h, Ra, ta, cyl, Rb, tb)
    prim.verts.append(np.zeros((1, 3)))
    a, b = prim.run(), mesh.run()
    pen = a[:, 7] == 1
    assert pen.sum() >= 30 and (~pen).sum() >= 30, pen.sum()
    assert np.array_equal(a[:, 7], b[:, 7])
    err = np.abs(a[:, :7] - b[:, :7]).max(axis=1)
    print("box primitive vs 8-vertex hull against cylinders: separated max %.3e, penetrating max %.3e" %
          (err[~pen].max(), err[pen].max()))
    assert err[~pen].max() <= 1e-9, err[~pen].max()
    assert err[pen].max() <= 1e-6, err[pen].max()


def _cyl_support(R, t, r, hh, u):
    """Support value of the cylinder (axis R[:, 2], radius r, half height hh) in direction u."""
    ul = R.T @ u
    return u @ t + r * np.hypot(ul[0], ul[1]) + hh * abs(ul[2])


def test_general_hull_against_cylinder_is_a_critical_point(cuda):
    """40-vertex ellipsoid hulls (triangular faces, no two coplanar) against
    cylinders, either order: the exact finish on vertex, edge and general face
    features, which the box twins above do not reach.  No closed reference
    exists, so the result is held to the optimality conditions: with
    n = (pB - pA) / d, pA lies in A and is A's support point along n, pB lies in
    B and is B's support point along -n.  Then -(h_A(n) + h_B(-n)) = d, a lower
    bound on the signed distance that equals it only at the solution, so
    gap = d - lower bound >= 0 is the distance error: 1e-9 for separated pairs
    (the distance stage's bound), 2e-6 for penetrating ones (EPA's, as in
    test_gpu_narrow.py; a refined pair reaches 1e-9 there too)."""
    rng = np.random.default_rng(17)
    cs = Cases()
    meta = []
    for k in range(96):
        pts = _ellipsoid_hull(rng, 40)
        hull = cs.hull(pts)
        r, hh = rng.uniform(0.03, 0.08), rng.uniform(0.03, 0.12)
        cyl = Cases.prim(CYL, [r, hh, 0])
        Rh, Rc, th = _rot(rng), _rot(rng), rng.uniform(-0.5, 0.5, size=3)
        t = rng.normal(size=3)
        tc = th + t * rng.uniform(0.0, 0.26) / np.linalg.norm(t)
        if k % 2:
            cs.add(cyl, Rc, tc, hull, Rh, th)
        else:
            cs.add(hull, Rh, th, cyl, Rc, tc)
        meta.append((k % 2 == 0, pts @ Rh.T + th, Rc, tc, r, hh))
    out = cs.run()
    gaps, pen = [], out[:, 7] == 1
    for (hull_is_a, W, Rc, tc, r, hh), o in zip(meta, out):
        d, pA, pB = o[0], o[1:4], o[4:7]
        n = (pB - pA) / d
        pH, pC, nH = (pA, pB, n) if hull_is_a else (pB, pA, -n)
        eq = ConvexHull(W).equations
        assert (eq[:, :3] @ pH + eq[:, 3]).max() <= 1e-9          # the hull's witness lies in the hull
        cl = Rc.T @ (pC - tc)
        assert np.hypot(cl[0], cl[1]) <= r + 1e-9 and abs(cl[2]) <= hh + 1e-9   # and the cylinder's in the cylinder
        assert abs(np.linalg.norm(pB - pA) - abs(d)) <= 1e-12
        gaps.append(d + (W @ nH).max() + _cyl_support(Rc, tc, r, hh, -nH))
    gaps = np.array(gaps)
    print("general hull vs cylinder: %d separated, max gap %.3e; %d penetrating, max gap %.3e, %d of them <= 1e-9" %
          ((~pen).sum(), gaps[~pen].max(), pen.sum(), gaps[pen].max(), (gaps[pen] <= 1e-9).sum()))
    assert pen.sum() >= 25 and (~pen).sum() >= 25, pen.sum()
    assert gaps.min() >= -1e-12
    assert gaps[~pen].max() <= 1e-9, (gaps[~pen].max(), int(np.argmax(np.where(pen, 0, gaps))))
    assert gaps[pen].max() <= 2e-6, (gaps[pen].max(), int(np.argmax(np.where(pen, gaps, 0))))


def test_support_ties_do_not_depend_on_vertex_order(cuda):
    """Two axis-aligned cubes face to face: every support direction ties four
    vertices.  The same cubes with their vertices permuted, and padded with
    interior points beyond one lane stride (the scan then deals the tied
    vertices to other lanes), give the same bits."""
    rng = np.random.default_rng(2)
    cube = _box_corners([0.1, 0.1, 0.1])
    pad = np.vstack([cube, rng.uniform(-0.05, 0.05, size=(70, 3))])
    cs = Cases()
    eye = np.eye(3)
    for pts in (cube, cube[rng.permutation(8)], pad, pad[rng.permutation(78)], pad[::-1]):
        for t in ([0.3, 0, 0], [0, -0.35, 0], [0, 0, 0.25]):
            cs.add(cs.hull(pts), eye, np.zeros(3), cs.hull(pts[::-1]), eye, np.array(t, dtype=float))
    out = cs.run()[:, 0].reshape(5, 3)
    np.testing.assert_array_equal(out, np.tile(out[0], (5, 1)))
    np.testing.assert_allclose(out[0], [0.1, 0.15, 0.05], rtol=0, atol=1e-15)
