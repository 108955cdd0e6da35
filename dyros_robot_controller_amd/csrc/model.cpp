// URDF/SRDF subset reader and Pinocchio-convention model build.
//
// Restates (reference src/manipulator/robot_data.cpp:21-62):
//   pinocchio::urdf::buildModel    urdfdom orders a link's children by joint
//                                  name (std::map); Pinocchio walks the tree
//                                  depth first in that order; fixed joints
//                                  are merged into the moving parent.
//   pinocchio::urdf::buildGeom     COLLISION elements, file order per link,
//                                  placement = body placement * origin.
//   GeometryModel::addAllCollisionPairs   all (i<j) with different parent joints.
//   pinocchio::srdf::removeCollisionPairs drop pairs between disabled links.
//   lowerPositionLimit / velocityLimit    from <limit>.
#include "model.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <map>
#include <memory>
#include <set>
#include <sstream>

#include "../../include/drc_amd.h"
#include "call_plan.hpp"
#include "mesh.hpp"

namespace drc_amd {
namespace {

// ---------------------------------------------------------------- tiny XML
struct XmlNode {
  std::string tag;
  std::map<std::string, std::string> attr;
  std::vector<std::unique_ptr<XmlNode>> kids;
  const XmlNode* child(const char* t) const {
    for (auto& k : kids)
      if (k->tag == t) return k.get();
    return nullptr;
  }
  std::vector<const XmlNode*> children(const char* t) const {
    std::vector<const XmlNode*> r;
    for (auto& k : kids)
      if (k->tag == t) r.push_back(k.get());
    return r;
  }
  const char* get(const char* k, const char* def = nullptr) const {
    auto it = attr.find(k);
    return it == attr.end() ? def : it->second.c_str();
  }
};

class XmlParser {
 public:
  explicit XmlParser(const std::string& s) : s_(s) {}
  std::unique_ptr<XmlNode> parse(std::string* err) {
    std::unique_ptr<XmlNode> root;
    while (skip_misc()) {
      if (root) break;
      root = element(err);
      if (!root) return nullptr;
    }
    if (!root) *err = "no root element";
    return root;
  }

 private:
  const std::string& s_;
  size_t i_ = 0;
  bool at(const char* p) const { return s_.compare(i_, std::strlen(p), p) == 0; }
  void ws() {
    while (i_ < s_.size() && std::isspace(static_cast<unsigned char>(s_[i_]))) ++i_;
  }
  // skips whitespace, comments, <? ?> and <! > ; true if a '<' element follows
  bool skip_misc() {
    for (;;) {
      ws();
      if (i_ >= s_.size()) return false;
      if (at("<!--")) {
        size_t e = s_.find("-->", i_ + 4);
        i_ = e == std::string::npos ? s_.size() : e + 3;
      } else if (at("<?")) {
        size_t e = s_.find("?>", i_ + 2);
        i_ = e == std::string::npos ? s_.size() : e + 2;
      } else if (at("<!")) {
        size_t e = s_.find('>', i_ + 2);
        i_ = e == std::string::npos ? s_.size() : e + 1;
      } else if (s_[i_] == '<') {
        return true;
      } else {
        size_t e = s_.find('<', i_);  // text content: ignored
        i_ = e == std::string::npos ? s_.size() : e;
      }
    }
  }
  std::string name() {
    size_t b = i_;
    while (i_ < s_.size() && (std::isalnum(static_cast<unsigned char>(s_[i_])) || s_[i_] == '_' ||
                              s_[i_] == ':' || s_[i_] == '-' || s_[i_] == '.'))
      ++i_;
    return s_.substr(b, i_ - b);
  }
  std::unique_ptr<XmlNode> element(std::string* err) {
    auto n = std::make_unique<XmlNode>();
    ++i_;  // '<'
    n->tag = name();
    if (n->tag.empty()) {
      *err = "malformed tag at byte " + std::to_string(i_);
      return nullptr;
    }
    for (;;) {
      ws();
      if (i_ >= s_.size()) {
        *err = "unterminated tag <" + n->tag + ">";
        return nullptr;
      }
      if (at("/>")) {
        i_ += 2;
        return n;
      }
      if (s_[i_] == '>') {
        ++i_;
        break;
      }
      std::string k = name();
      ws();
      if (k.empty() || i_ >= s_.size() || s_[i_] != '=') {
        *err = "malformed attribute in <" + n->tag + ">";
        return nullptr;
      }
      ++i_;
      ws();
      char q = s_[i_];
      if (q != '"' && q != '\'') {
        *err = "unquoted attribute in <" + n->tag + ">";
        return nullptr;
      }
      size_t e = s_.find(q, i_ + 1);
      if (e == std::string::npos) {
        *err = "unterminated attribute in <" + n->tag + ">";
        return nullptr;
      }
      n->attr[k] = s_.substr(i_ + 1, e - i_ - 1);
      i_ = e + 1;
    }
    for (;;) {
      if (!skip_misc()) {
        *err = "missing </" + n->tag + ">";
        return nullptr;
      }
      if (at("</")) {
        i_ += 2;
        std::string t = name();
        ws();
        if (t != n->tag || i_ >= s_.size() || s_[i_] != '>') {
          *err = "mismatched </" + t + "> for <" + n->tag + ">";
          return nullptr;
        }
        ++i_;
        return n;
      }
      auto k = element(err);
      if (!k) return nullptr;
      n->kids.push_back(std::move(k));
    }
  }
};

// ----------------------------------------------------------- SE(3) helpers
struct SE3 {
  double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  double p[3] = {0, 0, 0};
};
SE3 mul(const SE3& a, const SE3& b) {
  SE3 c;
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j)
      c.R[3 * i + j] = a.R[3 * i] * b.R[j] + a.R[3 * i + 1] * b.R[3 + j] + a.R[3 * i + 2] * b.R[6 + j];
    c.p[i] = a.R[3 * i] * b.p[0] + a.R[3 * i + 1] * b.p[1] + a.R[3 * i + 2] * b.p[2] + a.p[i];
  }
  return c;
}
bool parse_vec(const char* s, int n, double* out) {
  if (!s) return false;
  std::istringstream is(s);
  for (int i = 0; i < n; ++i)
    if (!(is >> out[i])) return false;
  return true;
}
// rpy -> Rz(y) Ry(p) Rx(r)
SE3 origin_of(const XmlNode* el) {
  SE3 T;
  const XmlNode* o = el ? el->child("origin") : nullptr;
  if (!o) return T;
  double xyz[3] = {0, 0, 0}, rpy[3] = {0, 0, 0};
  if (o->get("xyz")) parse_vec(o->get("xyz"), 3, xyz);
  if (o->get("rpy")) parse_vec(o->get("rpy"), 3, rpy);
  const double cr = std::cos(rpy[0]), sr = std::sin(rpy[0]), cp = std::cos(rpy[1]),
               sp = std::sin(rpy[1]), cy = std::cos(rpy[2]), sy = std::sin(rpy[2]);
  const double R[9] = {cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr,
                       sy * cp, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr,
                       -sp,     cp * sr,                cp * cr};
  std::memcpy(T.R, R, sizeof(R));
  std::memcpy(T.p, xyz, sizeof(xyz));
  return T;
}
void put12(const SE3& T, double* out) {
  std::memcpy(out, T.R, 9 * sizeof(double));
  std::memcpy(out + 9, T.p, 3 * sizeof(double));
}
bool read_file(const std::string& path, std::string* out) {
  std::ifstream f(path, std::ios::binary);
  if (!f) return false;
  std::stringstream ss;
  ss << f.rdbuf();
  *out = ss.str();
  return true;
}

struct Builder {
  const XmlNode* robot;
  std::map<std::string, const XmlNode*> links, joints;
  std::map<std::string, std::vector<std::string>> children;  // link -> joint names (sorted)
  HostModel* hm;
  std::vector<std::string> geom_link;
  std::map<std::string, int> frame_of_link;
  std::string packages, urdf_dir;  // where mesh URIs are looked up
  std::string err;
  int err_code = DRC_ERR_UNSUPPORTED;

  bool add_link(const std::string& lname, int jid, const SE3& place) {
    DevModel& m = hm->dev;
    if (m.nframes >= kMaxFrames) return fail("too many links");
    frame_of_link[lname] = m.nframes;
    hm->frame_names.push_back(lname);
    m.frame_joint[m.nframes] = jid;
    put12(place, m.frame_place[m.nframes]);
    ++m.nframes;
    const XmlNode* ln = links[lname];
    int k = 0;
    for (const XmlNode* c : ln->children("collision")) {
      const XmlNode* g = c->child("geometry");
      if (!g || g->kids.empty()) return fail("collision without geometry in link " + lname);
      const XmlNode* s = g->kids[0].get();
      if (m.ngeom >= kMaxGeoms) return fail("too many collision geometries");
      int gi = m.ngeom;
      double prm[3] = {0, 0, 0};
      SE3 centre;  // mesh: from the file's frame to the bounding box's centre
      if (s->tag == "sphere") {
        m.gtype[gi] = kSphere;
        if (!parse_vec(s->get("radius"), 1, prm)) return fail("bad sphere radius");
        m.gbound[gi] = prm[0];
      } else if (s->tag == "cylinder") {
        m.gtype[gi] = kCylinder;
        double rl[2];
        if (!parse_vec(s->get("radius"), 1, rl) || !parse_vec(s->get("length"), 1, rl + 1))
          return fail("bad cylinder");
        prm[0] = rl[0];
        prm[1] = 0.5 * rl[1];
        m.gbound[gi] = rl[0];  // capsule core = axis segment
      } else if (s->tag == "box") {
        m.gtype[gi] = kBox;
        double sz[3];
        if (!parse_vec(s->get("size"), 3, sz)) return fail("bad box size");
        for (int i = 0; i < 3; ++i) prm[i] = 0.5 * sz[i];
        m.gbound[gi] = std::sqrt(prm[0] * prm[0] + prm[1] * prm[1] + prm[2] * prm[2]);
      } else if (s->tag == "mesh") {
        // the convex hull of the file's vertices, centred on its bounding box:
        // gparam / gbound describe that box, which the broad phase takes for
        // the mesh (a lower bound on the box holds for the hull inside it)
        m.gtype[gi] = kMesh;
        const char* fn = s->get("filename");
        if (!fn) return fail("mesh without filename in link " + lname);
        double sc[3] = {1, 1, 1};
        if (s->get("scale") && !parse_vec(s->get("scale"), 3, sc)) return fail("bad mesh scale in link " + lname);
        std::string path, e;
        MeshHull hull;
        int rc = resolve_mesh_uri(fn, packages, urdf_dir, &path, &e);
        if (!rc) rc = mesh_convex_hull(path, sc, kMaxMeshVerts, &hull, &e);
        if (rc) return fail("collision mesh of link " + lname + ": " + e, rc);
        const int first = static_cast<int>(hm->mesh_verts.size() / 3), nvx = static_cast<int>(hull.verts.size());
        if (first + nvx > kMaxMeshVertsModel)
          return fail("collision meshes exceed " + std::to_string(kMaxMeshVertsModel) +
                      " hull vertices per model (link " + lname + ", " + path + ")");
        double lo[3], hi[3];
        for (int i = 0; i < 3; ++i) lo[i] = hi[i] = hull.verts[0][i];
        for (const P3& v : hull.verts)
          for (int i = 0; i < 3; ++i) {
            lo[i] = std::min(lo[i], v[i]);
            hi[i] = std::max(hi[i], v[i]);
          }
        for (int i = 0; i < 3; ++i) {
          centre.p[i] = 0.5 * (lo[i] + hi[i]);
          prm[i] = 0.5 * (hi[i] - lo[i]);
        }
        for (const P3& v : hull.verts)
          for (int i = 0; i < 3; ++i) hm->mesh_verts.push_back(v[i] - centre.p[i]);
        m.gbound[gi] = std::sqrt(prm[0] * prm[0] + prm[1] * prm[1] + prm[2] * prm[2]);
        hm->mesh_first.resize(gi + 1, 0);
        hm->mesh_count.resize(gi + 1, 0);
        hm->mesh_residual.resize(gi + 1, 0.0);
        hm->mesh_files.resize(gi + 1);
        hm->mesh_first[gi] = first;
        hm->mesh_count[gi] = nvx;
        hm->mesh_residual[gi] = hull.residual;
        hm->mesh_files[gi] = path;
      } else {
        return fail("unsupported collision geometry <" + s->tag + "> in link " + lname);
      }
      std::memcpy(m.gparam[gi], prm, sizeof(prm));
      m.gparent[gi] = jid;
      put12(mul(mul(place, origin_of(c)), centre), m.gplace[gi]);
      hm->geom_names.push_back(lname + "_" + std::to_string(k++));
      geom_link.push_back(lname);
      ++m.ngeom;
    }
    if (const XmlNode* ie = ln->child("inertial")) {
      // URDF <inertial>: mass, com origin, inertia about the com in the origin's
      // rotated frame; rotate into the joint frame and merge (parallel axis)
      const XmlNode* ms = ie->child("mass");
      const XmlNode* it = ie->child("inertia");
      double mass = 0;
      if (ms && ms->get("value") && !parse_vec(ms->get("value"), 1, &mass)) return fail("bad mass in link " + lname);
      double Il[6] = {0, 0, 0, 0, 0, 0};  // xx yy zz xy xz yz
      static const char* kI[6] = {"ixx", "iyy", "izz", "ixy", "ixz", "iyz"};
      for (int k2 = 0; k2 < 6; ++k2)
        if (it && it->get(kI[k2]) && !parse_vec(it->get(kI[k2]), 1, &Il[k2])) return fail("bad inertia in link " + lname);
      const SE3 T = mul(place, origin_of(ie));
      const double L[9] = {Il[0], Il[3], Il[4], Il[3], Il[1], Il[5], Il[4], Il[5], Il[2]};
      double RI[9], I[9];
      for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) RI[3 * r + c] = T.R[3 * r] * L[c] + T.R[3 * r + 1] * L[3 + c] + T.R[3 * r + 2] * L[6 + c];
      for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) I[3 * r + c] = RI[3 * r] * T.R[3 * c] + RI[3 * r + 1] * T.R[3 * c + 1] + RI[3 * r + 2] * T.R[3 * c + 2];
      double* b = m.inertia[jid];
      const double m0 = b[0], m1 = m0 + mass;
      double c0[3] = {b[1], b[2], b[3]}, c1[3];
      for (int i = 0; i < 3; ++i) c1[i] = m1 > 0 ? (m0 * c0[i] + mass * T.p[i]) / m1 : 0.0;
      // I_new(about c1) = I0 + m0 (|d0|^2 E - d0 d0^T) + I + mass (|d|^2 E - d d^T)
      double Inew[9];
      for (int i = 0; i < 9; ++i) Inew[i] = 0;
      const double I0[9] = {b[4], b[7], b[8], b[7], b[5], b[9], b[8], b[9], b[6]};
      auto add = [&](const double* Ib, double mb, const double* cb) {
        const double d[3] = {cb[0] - c1[0], cb[1] - c1[1], cb[2] - c1[2]};
        const double dd = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
        for (int r = 0; r < 3; ++r)
          for (int c = 0; c < 3; ++c) Inew[3 * r + c] += Ib[3 * r + c] + mb * ((r == c ? dd : 0.0) - d[r] * d[c]);
      };
      add(I0, m0, c0);
      add(I, mass, T.p);
      b[0] = m1;
      for (int i = 0; i < 3; ++i) b[1 + i] = c1[i];
      b[4] = Inew[0]; b[5] = Inew[4]; b[6] = Inew[8];
      b[7] = Inew[1]; b[8] = Inew[2]; b[9] = Inew[5];
    }
    return true;
  }

  bool walk(const std::string& lname, int jid, const SE3& place) {
    if (!add_link(lname, jid, place)) return false;
    for (const std::string& jn : children[lname]) {
      const XmlNode* j = joints[jn];
      const std::string child = j->child("child")->get("link");
      SE3 jp = mul(place, origin_of(j));
      std::string type = j->get("type", "");
      if (type == "fixed") {
        if (!walk(child, jid, jp)) return false;
        continue;
      }
      if (type != "revolute" && type != "prismatic")
        return fail("unsupported joint type '" + type + "' (" + jn + "); continuous/floating/planar joints change nq (SURVEY H4b)");
      DevModel& m = hm->dev;
      if (m.nv >= kMaxJoints) return fail("too many joints");
      int id = ++m.nv;
      m.parent[id] = jid;
      m.jtype[id] = type == "revolute" ? kRevolute : kPrismatic;
      put12(jp, m.jplace[id]);
      double ax[3] = {1, 0, 0};
      if (const XmlNode* a = j->child("axis")) parse_vec(a->get("xyz"), 3, ax);
      double n = std::sqrt(ax[0] * ax[0] + ax[1] * ax[1] + ax[2] * ax[2]);
      for (int i = 0; i < 3; ++i) m.axis[id][i] = ax[i] / n;
      double lo = 0, hi = 0, vel = 0, eff = 0;
      if (const XmlNode* l = j->child("limit")) {
        if (l->get("lower")) parse_vec(l->get("lower"), 1, &lo);
        if (l->get("upper")) parse_vec(l->get("upper"), 1, &hi);
        if (l->get("velocity")) parse_vec(l->get("velocity"), 1, &vel);
        if (l->get("effort")) parse_vec(l->get("effort"), 1, &eff);
      }
      m.lower[id - 1] = lo;
      m.upper[id - 1] = hi;
      m.vel[id - 1] = vel;
      hm->effort.push_back(eff);
      hm->joint_names.push_back(jn);
      m.anc[id] = (jid > 0 ? m.anc[jid] : 0u) | (1u << (id - 1));
      if (!walk(child, id, SE3())) return false;
    }
    return true;
  }
  bool fail(const std::string& e, int code = DRC_ERR_UNSUPPORTED) {
    err = e;
    err_code = code;
    return false;
  }
};

}  // namespace

int build_model_from_urdf(const std::string& urdf_path, const std::string& srdf_path,
                          const std::string& packages_path, HostModel* out, std::string* err) {
  std::string text;
  if (!read_file(urdf_path, &text)) {
    *err = "URDF file does not exist: " + urdf_path;
    return DRC_ERR_FILE;
  }
  XmlParser xp(text);
  auto root = xp.parse(err);
  if (!root) return DRC_ERR_PARSE;
  if (root->tag != "robot") {
    *err = "URDF root element is <" + root->tag + ">, expected <robot>";
    return DRC_ERR_PARSE;
  }
  *out = HostModel();
  Builder b;
  b.robot = root.get();
  b.hm = out;
  b.packages = packages_path;
  {
    const size_t sep = urdf_path.find_last_of('/');
    b.urdf_dir = sep == std::string::npos ? "" : (sep == 0 ? "/" : urdf_path.substr(0, sep));
  }
  std::set<std::string> child_links;
  for (auto& k : root->kids) {
    if (k->tag == "link") b.links[k->get("name", "")] = k.get();
    if (k->tag == "joint") b.joints[k->get("name", "")] = k.get();
  }
  for (auto& kv : b.joints) {  // std::map: joint-name order, as urdfdom
    const XmlNode* p = kv.second->child("parent");
    const XmlNode* c = kv.second->child("child");
    if (!p || !c || !p->get("link") || !c->get("link")) {
      *err = "joint " + kv.first + " lacks parent/child";
      return DRC_ERR_PARSE;
    }
    if (!b.links.count(p->get("link")) || !b.links.count(c->get("link"))) {
      *err = "joint " + kv.first + " references an unknown link";
      return DRC_ERR_PARSE;
    }
    b.children[p->get("link")].push_back(kv.first);
    child_links.insert(c->get("link"));
  }
  std::vector<std::string> roots;
  for (auto& kv : b.links)
    if (!child_links.count(kv.first)) roots.push_back(kv.first);
  if (roots.size() != 1) {
    *err = "URDF must have exactly one root link";
    return DRC_ERR_PARSE;
  }
  if (!b.walk(roots[0], 0, SE3())) {
    *err = b.err;
    return b.err_code;
  }
  DevModel& m = out->dev;
  out->mesh_first.resize(m.ngeom, 0);
  out->mesh_count.resize(m.ngeom, 0);
  out->mesh_residual.resize(m.ngeom, 0.0);
  out->mesh_files.resize(m.ngeom);
  m.has_mesh = out->has_mesh() ? 1 : 0;
  for (int g = 0; g < m.ngeom; ++g) {
    m.gmesh_first[g] = out->mesh_first[g];
    m.gmesh_count[g] = out->mesh_count[g];
  }
  // addAllCollisionPairs
  std::vector<std::pair<int, int>> pairs;
  for (int i = 0; i < m.ngeom; ++i)
    for (int j = i + 1; j < m.ngeom; ++j)
      if (m.gparent[i] != m.gparent[j]) pairs.emplace_back(i, j);
  // srdf::removeCollisionPairs
  if (!srdf_path.empty()) {
    std::string st;
    if (read_file(srdf_path, &st)) {
      XmlParser sp(st);
      std::string e2;
      auto sr = sp.parse(&e2);
      if (!sr) {
        *err = "SRDF: " + e2;
        return DRC_ERR_PARSE;
      }
      std::set<std::pair<int, int>> drop;
      for (const XmlNode* d : sr->children("disable_collisions")) {
        const char* l1 = d->get("link1");
        const char* l2 = d->get("link2");
        if (!l1 || !l2 || !b.frame_of_link.count(l1) || !b.frame_of_link.count(l2)) continue;
        if (std::string(l1) == l2) continue;
        for (int a = 0; a < m.ngeom; ++a) {
          if (b.geom_link[a] != l1) continue;
          for (int c = 0; c < m.ngeom; ++c)
            if (b.geom_link[c] == l2) drop.insert({std::min(a, c), std::max(a, c)});
        }
      }
      std::vector<std::pair<int, int>> kept;
      for (auto& p : pairs)
        if (!drop.count(p)) kept.push_back(p);
      pairs.swap(kept);
    }
    // a missing SRDF keeps every pair (reference robot_data.cpp:44-48)
  }
  if (static_cast<int>(pairs.size()) > kMaxPairs) {
    *err = "too many collision pairs";
    return DRC_ERR_UNSUPPORTED;
  }
  m.npairs = static_cast<int>(pairs.size());
  for (int p = 0; p < m.npairs; ++p) {
    m.pair_a[p] = static_cast<int16_t>(pairs[p].first);
    m.pair_b[p] = static_cast<int16_t>(pairs[p].second);
  }
  out->geom_link = b.geom_link;
  out->base_pairs = m.npairs;
  m.nobst = 0;
  m.obst0 = m.ngeom;
  build_pair_tables(out);
  build_motion_tables(out);
  return DRC_OK;
}

void build_pair_tables(HostModel* hm) {
  DevModel& m = hm->dev;
  // pair order of the wave kernel's closed-form / bound pass: by type class
  // (sphere-sphere, sphere-cylinder, sphere-box, cylinder-cylinder,
  // cylinder-box, box-box, then every pair with a mesh, then every pair with a
  // half-space), pair index order within a class
  {
    int n = 0;
    for (int cls = 0; cls < 8; ++cls)
      for (int p = 0; p < m.npairs; ++p) {
        int ta = m.gtype[m.pair_a[p]], tb = m.gtype[m.pair_b[p]];
        if (ta > tb) std::swap(ta, tb);
        // (0,0)0 (0,1)1 (0,2)2 (1,1)3 (1,2)4 (2,2)5 (*,mesh)6 (*,half-space)7
        const int c = tb == kHalfSpace ? 7 : (tb == kMesh ? 6 : (ta == 0 ? tb : (ta == 1 ? 2 + tb : 5)));
        if (c == cls) m.pair_order[n++] = static_cast<int16_t>(p);
      }
    for (int sl = 0; sl < m.npairs; ++sl) {
      m.slot_a[sl] = m.pair_a[m.pair_order[sl]];
      m.slot_b[sl] = m.pair_b[m.pair_order[sl]];
    }
  }
  // GJK candidate slots of the lane-per-instance task stage: the pairs with
  // no sphere and no half-space (no closed form), numbered in pair order
  m.ncand_slots = 0;
  for (int p = 0; p < m.npairs; ++p) {
    m.cand_slot[p] = -1;
    if (m.gtype[m.pair_a[p]] != kSphere && m.gtype[m.pair_b[p]] != kSphere && m.gtype[m.pair_b[p]] != kHalfSpace) {
      if (m.ncand_slots < kMaxCandSlots) m.cand_pair[m.ncand_slots] = static_cast<int16_t>(p);
      m.cand_slot[p] = static_cast<int16_t>(m.ncand_slots < kMaxCandSlots ? m.ncand_slots : -1);
      ++m.ncand_slots;
    }
  }
  build_stage_tables(hm);
}

int set_obstacles(HostModel* hm, int n, const int* type, const double* param, const char* const* links, int n_links,
                  std::string* err) {
  DevModel& m = hm->dev;
  const int g0 = m.obst0;  // geometries of the URDF
  if (n < 0 || n_links < 0 || (n > 0 && !type) || (n_links > 0 && !links)) {
    *err = "set_obstacles: negative count or missing array";
    return DRC_ERR_INVALID_ARGUMENT;
  }
  if (!stage_build_exists(hm->has_mesh(), n > 0)) {
    *err = "the model has collision meshes: obstacle slots are not built for hull models";
    return DRC_ERR_UNSUPPORTED;
  }
  for (int i = 0; i < n; ++i) {
    if (type[i] == kMesh) {
      *err = "obstacle " + std::to_string(i) + ": mesh obstacles are not supported";
      return DRC_ERR_UNSUPPORTED;
    }
    if (type[i] != kSphere && type[i] != kCylinder && type[i] != kBox && type[i] != kHalfSpace) {
      *err = "obstacle " + std::to_string(i) + ": unknown geometry type " + std::to_string(type[i]);
      return DRC_ERR_INVALID_ARGUMENT;
    }
    if (type[i] != kHalfSpace && !param) {
      *err = "set_obstacles: param is required for sphere, cylinder and box obstacles";
      return DRC_ERR_INVALID_ARGUMENT;
    }
    const int np = type[i] == kSphere ? 1 : (type[i] == kCylinder ? 2 : (type[i] == kBox ? 3 : 0));
    for (int k = 0; k < np; ++k)
      if (!(param[3 * i + k] > 0) || !std::isfinite(param[3 * i + k])) {
        *err = "obstacle " + std::to_string(i) + ": parameters must be finite and positive";
        return DRC_ERR_INVALID_ARGUMENT;
      }
  }
  // the geometries each obstacle is paired with
  std::vector<int> with;
  if (n_links == 0) {
    for (int g = 0; g < g0; ++g)
      if (m.gparent[g] > 0) with.push_back(g);
  } else {
    std::set<std::string> named;
    for (int k = 0; k < n_links; ++k) {
      if (!links[k] || std::find(hm->frame_names.begin(), hm->frame_names.end(), links[k]) == hm->frame_names.end()) {
        *err = std::string("set_obstacles: unknown link '") + (links[k] ? links[k] : "(null)") + "'";
        return DRC_ERR_UNKNOWN_LINK;
      }
      named.insert(links[k]);
    }
    for (int g = 0; g < g0; ++g)
      if (named.count(hm->geom_link[g])) with.push_back(g);
  }
  if (g0 + n > kMaxGeoms) {
    *err = "obstacle slots: more than " + std::to_string(kMaxGeoms) + " collision geometries";
    return DRC_ERR_UNSUPPORTED;
  }
  if (hm->base_pairs + static_cast<int64_t>(n) * static_cast<int64_t>(with.size()) > kMaxPairs) {
    *err = "obstacle slots: more than " + std::to_string(kMaxPairs) + " collision pairs";
    return DRC_ERR_UNSUPPORTED;
  }
  // back to the URDF's model: what a fresh build leaves past its geometries and pairs is zero
  for (int g = g0; g < kMaxGeoms; ++g) {
    m.gparent[g] = m.gtype[g] = 0;
    m.gbound[g] = 0;
    std::memset(m.gplace[g], 0, sizeof(m.gplace[g]));
    std::memset(m.gparam[g], 0, sizeof(m.gparam[g]));
  }
  for (int p = hm->base_pairs; p < kMaxPairs; ++p) m.pair_a[p] = m.pair_b[p] = 0;
  std::memset(m.pair_order, 0, sizeof(m.pair_order));
  std::memset(m.slot_a, 0, sizeof(m.slot_a));
  std::memset(m.slot_b, 0, sizeof(m.slot_b));
  std::memset(m.cand_slot, 0, sizeof(m.cand_slot));
  std::memset(m.cand_pair, 0, sizeof(m.cand_pair));
  hm->geom_names.resize(g0);
  m.ngeom = g0 + n;
  m.nobst = n;
  m.npairs = hm->base_pairs;
  for (int i = 0; i < n; ++i) {
    const int g = g0 + i;
    m.gparent[g] = 0;
    m.gtype[g] = type[i];
    const SE3 eye;
    put12(eye, m.gplace[g]);
    const double* pr = param + 3 * i;
    if (type[i] == kSphere) {
      m.gparam[g][0] = pr[0];
      m.gbound[g] = pr[0];
    } else if (type[i] == kCylinder) {
      m.gparam[g][0] = pr[0];
      m.gparam[g][1] = pr[1];
      m.gbound[g] = pr[0];  // capsule core = axis segment
    } else if (type[i] == kBox) {
      for (int k = 0; k < 3; ++k) m.gparam[g][k] = pr[k];
      m.gbound[g] = std::sqrt(pr[0] * pr[0] + pr[1] * pr[1] + pr[2] * pr[2]);
    }
    hm->geom_names.push_back("obstacle_" + std::to_string(i));
    for (int a : with) {  // obstacle-major, the link geometries in index order
      m.pair_a[m.npairs] = static_cast<int16_t>(a);
      m.pair_b[m.npairs] = static_cast<int16_t>(g);
      ++m.npairs;
    }
  }
  build_pair_tables(hm);
  build_motion_tables(hm);
  return DRC_OK;
}

void build_motion_tables(HostModel* hm) {
  DevModel& m = hm->dev;
  const int nv = m.nv;
  auto norm3 = [](const double* p) { return std::sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]); };
  auto travel = [&](int k) { return std::max(std::fabs(m.lower[k - 1]), std::fabs(m.upper[k - 1])); };
  hm->motion_rho.assign(static_cast<size_t>(std::max(nv * m.ngeom, 1)), 0.0);
  for (int g = 0; g < m.ngeom; ++g) {
    const int c = m.gparent[g];
    if (c <= 0) continue;  // fixed links and obstacle slots do not move with q
    const double* pr = m.gparam[g];
    double rad = 0.0;
    switch (m.gtype[g]) {
      case kSphere: rad = pr[0]; break;
      case kCylinder: rad = std::sqrt(pr[0] * pr[0] + pr[1] * pr[1]); break;
      default: rad = norm3(pr); break;  // box, hull: the half extents
    }
    // up the chain from c: `below` is the sum over the joints strictly below j
    double below = 0.0;
    for (int j = c; j > 0; j = m.parent[j]) {
      hm->motion_rho[static_cast<size_t>(j - 1) * m.ngeom + g] = below + norm3(m.gplace[g] + 9) + rad;
      below += norm3(m.jplace[j] + 9) + (m.jtype[j] == kPrismatic ? travel(j) : 0.0);
    }
  }
  m.travel_mask = 0;
  hm->motion_unbounded = false;
  for (int k = 1; k <= nv; ++k) {
    if (m.jtype[k] != kPrismatic) continue;
    bool rev_above = false, geom_below = false;
    for (int j = m.parent[k]; j > 0; j = m.parent[j]) rev_above |= m.jtype[j] == kRevolute;
    for (int g = 0; g < m.ngeom; ++g) geom_below |= m.gparent[g] > 0 && (m.anc[m.gparent[g]] >> (k - 1) & 1u) != 0;
    if (!rev_above || !geom_below) continue;
    m.travel_mask |= 1u << (k - 1);
    if (!std::isfinite(travel(k))) hm->motion_unbounded = true;
  }
  m.motion_ld = m.pair_ld;
  m.motion_wt = nullptr;  // (the device buffer: the caller uploads the table)
  hm->motion_wt.assign(static_cast<size_t>(std::max(nv, 1)) * std::max(m.motion_ld, 1), 0.0);
  for (int p = 0; p < m.npairs; ++p) {
    const int ga = m.pair_a[p], gb = m.pair_b[p];
    const uint32_t sa = m.gparent[ga] > 0 ? m.anc[m.gparent[ga]] : 0u, sb = m.gparent[gb] > 0 ? m.anc[m.gparent[gb]] : 0u;
    for (int j = 1; j <= nv; ++j) {
      const bool ia = (sa >> (j - 1) & 1u) != 0, ib = (sb >> (j - 1) & 1u) != 0;
      if (ia == ib) continue;  // moves both alike, or neither
      hm->motion_wt[static_cast<size_t>(j - 1) * m.motion_ld + p] =
          m.jtype[j] == kPrismatic ? 1.0 : hm->motion_rho[static_cast<size_t>(j - 1) * m.ngeom + (ia ? ga : gb)];
    }
  }
}

void build_stage_tables(HostModel* hm) {
  DevModel& m = hm->dev;
  m.rev_mask = 0;
  for (int w = 0; w < 4; ++w) m.anc_bits[w] = 0;
  for (int j = 1; j <= m.nv; ++j) {
    if (m.jtype[j] == kRevolute) m.rev_mask |= 1u << (j - 1);
    for (int k = 1; k <= m.nv; ++k)
      if (m.anc[j] & (1u << (k - 1))) {
        const int bit = 16 * (j - 1) + (k - 1);
        m.anc_bits[bit >> 6] |= 1ull << (bit & 63);
      }
  }
  // one record per broad-phase slot (see DevModel::pair_tab)
  m.pair_ld = (m.npairs + 63) / 64 * 64;  // whole rounds of 64 lanes
  hm->pair_tab.assign(static_cast<size_t>(kPairFields) * std::max(m.pair_ld, 1), 0.0);
  for (int sl = 0; sl < m.npairs; ++sl) {
    const int p = m.pair_order[sl], ga = m.pair_a[p], gb = m.pair_b[p];
    double* rec = hm->pair_tab.data() + sl;
    const uint64_t meta = static_cast<uint64_t>(p) | static_cast<uint64_t>(ga) << 16 | static_cast<uint64_t>(gb) << 24 |
                          static_cast<uint64_t>(m.gtype[ga]) << 32 | static_cast<uint64_t>(m.gtype[gb]) << 36;
    std::memcpy(rec + kPairMeta * m.pair_ld, &meta, sizeof(meta));
    for (int k = 0; k < 3; ++k) {
      rec[(kPairParamA + k) * m.pair_ld] = m.gparam[ga][k];
      rec[(kPairParamB + k) * m.pair_ld] = m.gparam[gb][k];
    }
    rec[kPairBoundA * m.pair_ld] = m.gbound[ga];
    rec[kPairBoundB * m.pair_ld] = m.gbound[gb];
  }
}

}  // namespace drc_amd
