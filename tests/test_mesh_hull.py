"""Collision meshes on the host (csrc/mesh.cpp) through drc_mesh_convex_hull,
the function the model build calls: the file formats, the hull's vertex set
against scipy.spatial.ConvexHull, degenerate and bad inputs, the reduction to
a vertex cap with its residual, and the mesh errors of the model build (which
fail before a device is touched).  No GPU needed."""
import ctypes as C
import os

import numpy as np
import pytest
from scipy.spatial import ConvexHull

from _mesh_io import convex_hull, point_hull_distance, write_obj, write_stl_ascii, write_stl_binary
from dyros_robot_controller_amd import _capi


def _f32(a):
    """Values a binary STL holds exactly."""
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def _rows(a):
    return sorted(map(tuple, np.asarray(a).tolist()))


def _ball(rng, n, r=1.0):
    p = rng.normal(size=(n, 3))
    p *= (r * rng.uniform(0, 1, size=(n, 1)) ** (1 / 3)) / np.linalg.norm(p, axis=1)[:, None]
    return p


def _last_error():
    return _capi.lib().drc_last_error().decode()


def test_formats_agree(tmp_path):
    pts = _f32(_ball(np.random.default_rng(0), 61) + [0.3, -0.2, 0.1])
    write_stl_binary(tmp_path / "c.stl", pts)
    write_stl_ascii(tmp_path / "a.stl", pts)
    write_obj(tmp_path / "c.obj", pts)
    hulls = []
    for name in ("c.stl", "a.stl", "c.obj"):
        rc, v, res = convex_hull(tmp_path / name)
        assert rc == _capi.DRC_OK, _last_error()
        assert res == 0.0
        hulls.append(v)
    want = pts[ConvexHull(pts).vertices]
    for v in hulls:
        assert _rows(v) == _rows(want)
    # the vertices come in the order of their first occurrence in the file
    first = [int(np.flatnonzero((pts == v).all(axis=1))[0]) for v in hulls[0]]
    assert first == sorted(first)
    for v in hulls[1:]:
        np.testing.assert_array_equal(v, hulls[0])


def _clouds():
    rng = np.random.default_rng(1)
    corners = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], dtype=float)
    ball = _ball(rng, 200)
    yield "ball200", ball, None, None
    yield "cube_interior", np.vstack([rng.uniform(-0.999, 0.999, size=(1000, 3)), corners]) * [1, 2, 0.5], None, 8
    b100 = _ball(rng, 100, 0.4)
    yield "duplicates", np.vstack([b100, b100[::-1], b100[::3]]), None, None
    # nearly coplanar facets: a point 1e-6 above each face's centre is a
    # vertex (six shallow pyramids), one 1e-6 below is not
    bumps = np.vstack([s * (1 + e) * np.eye(3)[k] for k in range(3) for s in (-1, 1) for e in (1e-6,)])
    dents = np.vstack([s * (1 - 1e-6) * np.eye(3)[k] + 0.3 * np.eye(3)[(k + 1) % 3] for k in range(3) for s in (-1, 1)])
    yield "near_coplanar", np.vstack([dents, corners, bumps]), None, 14
    yield "scaled", ball, (2.0, 0.5, 3.0), None
    yield "mirrored", ball[:80], (-1.0, 1.0, 0.001), None


@pytest.mark.parametrize("name,pts,scale,count", list(_clouds()), ids=[c[0] for c in _clouds()])
def test_hull_matches_scipy(tmp_path, name, pts, scale, count):
    write_obj(tmp_path / "m.obj", pts)
    rc, v, res = convex_hull(tmp_path / "m.obj", scale=scale)
    assert rc == _capi.DRC_OK, _last_error()
    scaled = pts * (np.ones(3) if scale is None else np.array(scale))
    want = np.unique(scaled[ConvexHull(scaled).vertices], axis=0)
    if count is not None:
        assert len(want) == count  # what the cloud was built to give
    assert _rows(v) == _rows(want)
    assert res == 0.0


def test_degenerate_and_bad_inputs(tmp_path):
    rng = np.random.default_rng(2)
    u, w = np.array([1.0, 2.0, -0.5]), np.array([0.3, -1.0, 2.0])
    ab = rng.uniform(-1, 1, size=(50, 2))
    write_obj(tmp_path / "plane.obj", ab[:, :1] * u + ab[:, 1:] * w + 0.7)
    write_obj(tmp_path / "line.obj", ab[:, :1] * u + 0.1)
    write_obj(tmp_path / "three.obj", np.eye(3))
    (tmp_path / "robot.dae").write_text("<COLLADA/>")
    for name, code in (("plane.obj", _capi.DRC_ERR_UNSUPPORTED), ("line.obj", _capi.DRC_ERR_UNSUPPORTED),
                       ("three.obj", _capi.DRC_ERR_UNSUPPORTED), ("robot.dae", _capi.DRC_ERR_UNSUPPORTED),
                       ("absent.stl", _capi.DRC_ERR_FILE)):
        rc, v, _ = convex_hull(tmp_path / name)
        assert rc == code, (name, rc, _last_error())
        assert len(v) == 0
        assert name in _last_error(), _last_error()
    # a buffer that is too small is reported with the count it needs
    write_obj(tmp_path / "tet.obj", np.vstack([np.eye(3), np.zeros(3), [0.1, 0.1, 0.1]]))
    rc, v, _ = convex_hull(tmp_path / "tet.obj", cap=3)
    assert rc == _capi.DRC_ERR_SIZE_MISMATCH
    rc, v, _ = convex_hull(tmp_path / "tet.obj")
    assert rc == _capi.DRC_OK and len(v) == 4


def test_reduction_and_residual(tmp_path):
    rng = np.random.default_rng(3)
    pts = rng.normal(size=(1000, 3))
    pts = _f32(0.25 * pts / np.linalg.norm(pts, axis=1)[:, None])
    write_stl_binary(tmp_path / "sphere.stl", pts)
    full = _rows(pts[ConvexHull(pts).vertices])
    rc, v, res = convex_hull(tmp_path / "sphere.stl", max_vertices=64)
    assert rc == _capi.DRC_OK, _last_error()
    assert len(v) == 64
    assert set(_rows(v)) <= set(full)  # a subset of the hull's vertices: an inner approximation
    h = ConvexHull(v)
    outside = pts[(pts @ h.equations[:, :3].T + h.equations[:, 3]).max(axis=1) > 0]
    want = max(point_hull_distance(p, v, h.simplices) for p in outside)
    print("residual %.17g, scipy restatement %.17g" % (res, want))
    assert want > 1e-3  # 64 of ~1000 vertices on a 0.25 m sphere leave millimetres out
    assert abs(res - want) <= 1e-12 * want
    # the cap above the hull's size: the full hull, nothing left out
    rc, v, res = convex_hull(tmp_path / "sphere.stl", max_vertices=2000)
    assert rc == _capi.DRC_OK and _rows(v) == full and res == 0.0


REF_LINK0 = "/root/reference/examples/robots/fr3/assets/link0.stl"


@pytest.mark.skipif(not os.path.exists(REF_LINK0), reason="reference tree absent")
def test_reference_fr3_link0():
    """A real collision mesh (the reference tree's FR3 link0, a binary STL):
    the hull's vertex set equals scipy's for the file's points (102)."""
    raw = open(REF_LINK0, "rb").read()
    ntri = int(np.frombuffer(raw[80:84], dtype="<u4")[0])
    assert len(raw) == 84 + 50 * ntri
    rec = np.frombuffer(raw[84:], dtype=np.dtype([("n", "<f4", 3), ("v", "<f4", (3, 3)), ("a", "<u2")]))
    pts = np.unique(rec["v"].reshape(-1, 3).astype(np.float64), axis=0)
    want = pts[ConvexHull(pts).vertices]
    rc, v, res = convex_hull(REF_LINK0)
    assert rc == _capi.DRC_OK, _last_error()
    print("link0.stl: %d triangles, %d distinct points, %d hull vertices" % (ntri, len(pts), len(v)))
    assert len(v) == len(want) == 102
    assert _rows(v) == _rows(want)
    assert res == 0.0


def test_ascii_stl_keyword_is_a_whole_word(tmp_path):
    """A solid named after the keyword does not count as a vertex line."""
    pts = _f32(_ball(np.random.default_rng(7), 30))
    write_stl_ascii(tmp_path / "a.stl", pts)
    text = (tmp_path / "a.stl").read_text().replace("solid cloud", "solid vertex_cloud of vertex data")
    (tmp_path / "b.stl").write_text(text)
    (rc, va, _), (rc2, vb, _) = convex_hull(tmp_path / "a.stl"), convex_hull(tmp_path / "b.stl")
    assert rc == rc2 == _capi.DRC_OK, _last_error()
    np.testing.assert_array_equal(va, vb)


_URDF = """<robot name="r">
  <link name="base"><collision><geometry><sphere radius="0.1"/></geometry></collision></link>
  <link name="arm"><collision><origin xyz="0 0 0.2"/><geometry><mesh filename="%s"/></geometry></collision></link>
  <joint name="j1" type="revolute"><parent link="base"/><child link="arm"/><axis xyz="0 0 1"/>
    <limit lower="-1" upper="1" velocity="1" effort="1"/></joint>
</robot>
"""


@pytest.mark.parametrize("filename,packages,code", [
    ("meshes/absent.stl", None, _capi.DRC_ERR_FILE),
    ("package://pkg/meshes/absent.stl", "PKG", _capi.DRC_ERR_FILE),
    ("package://pkg/meshes/absent.stl", None, _capi.DRC_ERR_FILE),  # no packages_path to look in
    ("meshes/arm.dae", None, _capi.DRC_ERR_UNSUPPORTED),
    ("meshes/flat.obj", None, _capi.DRC_ERR_UNSUPPORTED),
])
def test_model_build_mesh_errors(tmp_path, filename, packages, code):
    """The mesh errors of the model build name the link and the file, and come
    before anything is uploaded (so this needs no device)."""
    (tmp_path / "meshes").mkdir()
    (tmp_path / "meshes" / "arm.dae").write_text("<COLLADA/>")
    write_obj(tmp_path / "meshes" / "flat.obj", [[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]])
    urdf = tmp_path / "r.urdf"
    urdf.write_text(_URDF % filename)
    h = C.c_void_p()
    pk = None if packages is None else str(tmp_path).encode()
    rc = _capi.lib().drc_model_create_manipulator(str(urdf).encode(), b"", pk, C.c_int(0), C.byref(h))
    assert rc == code, (rc, _last_error())
    assert not h.value
    assert "arm" in _last_error() and os.path.basename(filename) in _last_error(), _last_error()

