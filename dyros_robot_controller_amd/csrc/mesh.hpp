// Collision meshes: file loader (binary / ASCII STL, Wavefront OBJ), URDF mesh
// URI resolution and the 3-D quickhull that turns a mesh into the convex hull
// of its vertices (DESIGN.md "Collision meshes").  Host code only.
#pragma once

#include <array>
#include <string>
#include <vector>

namespace drc_amd {

constexpr int kMaxMeshVerts = 256;        // hull vertices kept per mesh
constexpr int kMaxMeshVertsModel = 2048;  // and per model (one buffer of double[3], 48 KB)

using P3 = std::array<double, 3>;

struct MeshHull {
  std::vector<P3> verts;  // hull vertices, in the order of their first occurrence in the file
  double residual = 0;    // largest distance of a left-out vertex from the kept hull (0: full hull)
};

// Vertices of a mesh file, duplicates included, in file order.  The format
// follows the extension (.stl, .obj; anything else: DRC_ERR_UNSUPPORTED).
int load_mesh_vertices(const std::string& path, std::vector<P3>* pts, std::string* err);

// Convex hull of pts: indices of the hull vertices (ascending).  More than
// max_vertices hull vertices: the farthest-point insertion stops there (an
// inner approximation) and *residual gets the largest distance of a left-out
// point from the kept hull.  Fewer than four non-coplanar points:
// DRC_ERR_UNSUPPORTED.
int convex_hull(const std::vector<P3>& pts, int max_vertices, std::vector<int>* hull, double* residual,
                std::string* err);

// load, scale, hull
int mesh_convex_hull(const std::string& path, const double scale[3], int max_vertices, MeshHull* out,
                     std::string* err);

// URDF mesh filename -> path: package://a/b -> <packages>/a/b (Pinocchio's
// package-dir rule), file://, absolute paths as given, relative paths against
// the URDF's directory.
int resolve_mesh_uri(const std::string& uri, const std::string& packages, const std::string& urdf_dir,
                     std::string* path, std::string* err);

}  // namespace drc_amd
