"""Mesh writers and the scipy restatement of the hull for the mesh tests (test
infrastructure).  The tests write their meshes into tmp_path: none is
committed."""
import ctypes as C
import struct
import xml.etree.ElementTree as ET

import numpy as np

from scipy.spatial import ConvexHull

from dyros_robot_controller_amd import _capi, robot_path


def _triangles(points):
    """Every point in some triangle: consecutive triples, the last one padded."""
    p = np.asarray(points, dtype=np.float64)
    pad = (-len(p)) % 3
    if pad:
        p = np.vstack([p, np.repeat(p[-1:], pad, axis=0)])
    return p.reshape(-1, 3, 3)


def write_stl_binary(path, points, triangles=None):
    tri = _triangles(points) if triangles is None else np.asarray(triangles, dtype=np.float64)
    with open(path, "wb") as f:
        f.write(b"binary stl".ljust(80, b" "))
        f.write(struct.pack("<I", len(tri)))
        for t in tri:
            f.write(struct.pack("<12fH", 0.0, 0.0, 0.0, *t.reshape(-1), 0))


def write_stl_ascii(path, points):
    with open(path, "w") as f:
        f.write("solid cloud\n")
        for t in _triangles(points):
            f.write(" facet normal 0 0 0\n  outer loop\n")
            for v in t:
                f.write("   vertex %.17g %.17g %.17g\n" % tuple(v))
            f.write("  endloop\n endfacet\n")
        f.write("endsolid cloud\n")


def write_obj(path, points):
    with open(path, "w") as f:
        f.write("# cloud\no cloud\n")
        for v in np.asarray(points, dtype=np.float64):
            f.write("v %.17g %.17g %.17g\n" % tuple(v))
        f.write("f 1 2 3\n")


def box_triangles(half):
    """The 12 triangles of an axis-aligned box with the given half extents."""
    hx, hy, hz = half
    c = np.array([[sx * hx, sy * hy, sz * hz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)])
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    tri = []
    for a, b, cc, d in quads:
        tri.append([c[a], c[b], c[cc]])
        tri.append([c[a], c[cc], c[d]])
    return np.array(tri)


def convex_hull(path, scale=None, max_vertices=0, cap=4096):
    """drc_mesh_convex_hull -> (rc, vertices [n, 3], residual)."""
    lib = _capi.lib()
    out = np.zeros((cap, 3))
    n = C.c_int(0)
    res = C.c_double(-1.0)
    sc = None if scale is None else (C.c_double * 3)(*scale)
    rc = lib.drc_mesh_convex_hull(str(path).encode(), sc, C.c_int(max_vertices),
                                  out.ctypes.data_as(C.POINTER(C.c_double)), C.c_int(cap), C.byref(n), C.byref(res))
    return rc, out[:n.value].copy(), res.value


def point_hull_distance(p, verts, simplices):
    """Distance of the point p from the surface triangles verts[simplices]
    (closed form: the face where p projects inside it, else its edges)."""
    a, b, c = (verts[simplices[:, k]] for k in range(3))
    best = np.inf
    n = np.cross(b - a, c - a)
    n /= np.linalg.norm(n, axis=1)[:, None]
    h = np.einsum("ij,ij->i", p - a, n)
    q = p - h[:, None] * n
    inside = np.ones(len(a), dtype=bool)
    for u, v in ((a, b), (b, c), (c, a)):
        inside &= np.einsum("ij,ij->i", np.cross(v - u, q - u), n) >= 0
        e = v - u
        t = np.clip(np.einsum("ij,ij->i", p - u, e) / np.einsum("ij,ij->i", e, e), 0.0, 1.0)
        best = min(best, np.linalg.norm(p - (u + t[:, None] * e), axis=1).min())
    if inside.any():
        best = min(best, np.abs(h[inside]).min())
    return best


# ---------------------------------------------------------------- all-mesh FR3
def _rpy(r, p, y):
    cr, sr, cp, sp, cy, sy = np.cos(r), np.sin(r), np.cos(p), np.sin(p), np.cos(y), np.sin(y)
    return np.array([[cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr],
                     [sy * cp, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr], [-sp, cp * sr, cp * cr]])


def _surface_points(geom):
    s = geom[0]
    if s.tag == "sphere":
        r, k = float(s.get("radius")), np.arange(16) + 0.5
        phi, th = np.arccos(1 - 2 * k / 16), np.pi * (1 + 5 ** 0.5) * k
        return r * np.stack([np.cos(th) * np.sin(phi), np.sin(th) * np.sin(phi), np.cos(phi)], axis=1)
    if s.tag == "cylinder":
        r, h, a = float(s.get("radius")), 0.5 * float(s.get("length")), np.arange(8) * np.pi / 4
        ring = np.stack([r * np.cos(a), r * np.sin(a), np.zeros(8)], axis=1)
        return np.vstack([ring + [0, 0, h], ring - [0, 0, h]])
    h = 0.5 * np.array([float(x) for x in s.get("size").split()])
    return np.array([[sx * h[0], sy * h[1], sz * h[2]] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)])


def all_mesh_fr3(tmp_path, cap=24):
    """FR3 with each link's primitives replaced by one hull (<= cap vertices)
    of points sampled on them.  Returns the URDF path, {link: hull points in
    the link frame} and the link pairs the model checks."""
    tree = ET.parse(robot_path("fr3"))
    root = tree.getroot()
    hulls = {}
    (tmp_path / "m").mkdir()
    for link in root.findall("link"):
        cols = link.findall("collision")
        if not cols:
            continue
        pts = []
        for c in cols:
            o = c.find("origin")
            xyz = np.array([float(x) for x in (o.get("xyz") if o is not None and o.get("xyz") else "0 0 0").split()])
            rpy = [float(x) for x in (o.get("rpy") if o is not None and o.get("rpy") else "0 0 0").split()]
            pts.append(_surface_points(c.find("geometry")) @ _rpy(*rpy).T + xyz)
            link.remove(c)
        pts = np.vstack(pts)
        pts = pts[ConvexHull(pts).vertices]
        if len(pts) > cap:  # thin out, then keep what is still a vertex
            pts = pts[np.linspace(0, len(pts) - 1, cap).astype(int)]
            pts = pts[ConvexHull(pts).vertices]
        hulls[link.get("name")] = pts
        write_obj(tmp_path / "m" / (link.get("name") + ".obj"), pts)
        g = ET.SubElement(ET.SubElement(link, "collision"), "geometry")
        ET.SubElement(g, "mesh", filename="m/%s.obj" % link.get("name"))
    # the moving joint each link hangs on (fixed joints merge into the parent)
    parent = {}
    joints = root.findall("joint")
    children = {j.find("child").get("link") for j in joints}
    todo = [(l.get("name"), 0) for l in root.findall("link") if l.get("name") not in children]
    nid = 0
    while todo:
        name, jid = todo.pop()
        parent[name] = jid
        for j in sorted((j for j in joints if j.find("parent").get("link") == name), key=lambda j: j.get("name")):
            if j.get("type") == "fixed":
                todo.append((j.find("child").get("link"), jid))
            else:
                nid += 1
                todo.append((j.find("child").get("link"), 1000 + nid))
    off = {frozenset((d.get("link1"), d.get("link2")))
           for d in ET.parse(robot_path("fr3", "srdf")).getroot().findall("disable_collisions")}
    names = [l.get("name") for l in root.findall("link") if l.get("name") in hulls]
    pairs = [(a, b) for i, a in enumerate(names) for b in names[i + 1:]
             if parent[a] != parent[b] and frozenset((a, b)) not in off]
    urdf = tmp_path / "fr3_all_mesh.urdf"
    tree.write(urdf)
    return str(urdf), hulls, pairs
