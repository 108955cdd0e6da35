// Robot model: host-side URDF/SRDF build and the flat device image the
// kernels read.  Restates Pinocchio's model/geometry build as the reference
// uses it in Manipulator::RobotData::RobotData (src/manipulator/robot_data.cpp:7-70).
#pragma once

#include <cstdint>
#include <string>
#include <vector>

namespace drc_amd {

constexpr int kMaxJoints = 16;    // 1-DoF joints (XLS-FR3 needs 14)
constexpr int kMaxGeoms = 64;
constexpr int kMaxPairs = 1024;
constexpr int kMaxFrames = 64;
constexpr int kMaxWheels = 8;
constexpr int kMaxCandSlots = 128;  // non-sphere pairs the lane-per-instance task stage tracks

enum JointType : int { kRevolute = 0, kPrismatic = 1 };
enum GeomType : int { kSphere = 0, kCylinder = 1, kBox = 2, kMesh = 3, kHalfSpace = 4 };
// kMesh: convex hull of a mesh's vertices; kHalfSpace: obstacle slots only, the
// solid {x : (x - p) . R e_z <= 0} of the slot's pose (R, p) (halfspace.hpp)
enum DriveKind : int { kDriveDifferential = 0, kDriveMecanum = 1, kDriveCaster = 2 };  // DRC_DRIVE_*

// Flat, POD model image in HBM.  Transforms are 12 doubles: R row-major, p.
struct DevModel {
  int nv, ngeom, npairs, nframes;
  int kind;                        // 0 manipulator, 1 mobile manipulator
  int n_arm, n_wheel;
  int virtual_start, mani_start, mobi_start;
  int act_mani_start, act_mobi_start;
  int parent[kMaxJoints + 1];
  int jtype[kMaxJoints + 1];
  uint32_t anc[kMaxJoints + 1];    // bit (k-1) set iff joint k supports joint j (inclusive)
  double jplace[kMaxJoints + 1][12];
  double axis[kMaxJoints + 1][3];
  double lower[kMaxJoints], upper[kMaxJoints], vel[kMaxJoints];
  int frame_joint[kMaxFrames];
  double frame_place[kMaxFrames][12];
  int gparent[kMaxGeoms];
  int gtype[kMaxGeoms];
  double gplace[kMaxGeoms][12];
  double gparam[kMaxGeoms][3];     // sphere r | cylinder r, h/2 | box half extents | mesh: its bounding box's
  double gbound[kMaxGeoms];        // conservative core/bounding radius for the broad phase
  int16_t pair_a[kMaxPairs], pair_b[kMaxPairs];
  int16_t cand_slot[kMaxPairs];       // pair -> GJK candidate slot (pairs without a sphere), or -1
  int16_t cand_pair[kMaxCandSlots];   // slot -> pair
  int ncand_slots;                    // non-sphere pairs (> kMaxCandSlots: lane stage not used)
  int16_t pair_order[kMaxPairs];      // pairs grouped by shape-type class (pair index order within a class):
                                      // the wave kernel's lanes then take same-type pairs in each round
  int16_t slot_a[kMaxPairs], slot_b[kMaxPairs];  // pair_a / pair_b of pair_order[slot]: one load level less
  double J_mobile[3][kMaxWheels];  // base twist = J_mobile * wheel velocity (differential, mecanum)
  int drive;                       // DriveKind; caster: J_mobile depends on the steer angles (mobile_fk.hpp)
  double wheel_radius, wheel_offset;
  double caster_pos[kMaxWheels / 2][2];  // base2wheel_positions of the casters
  // rigid-body inertia carried by each joint (links behind fixed joints merged,
  // Pinocchio appendBodyToJoint), in the joint frame:
  // {mass, com x, y, z, Ixx, Iyy, Izz, Ixy, Ixz, Iyz} with I about the com
  double inertia[kMaxJoints + 1][10];
  int dyn_origin;                  // joint whose origin the dynamics kernel takes as spatial reference (0 = world)
  // convex hulls of the collision meshes (appended: the layout above is what
  // the kernels of mesh-free models were built against).  Geometry g of type
  // kMesh owns mesh_verts[3 * gmesh_first[g] ...], gmesh_count[g] vertices
  int has_mesh;
  int gmesh_first[kMaxGeoms], gmesh_count[kMaxGeoms];
  const double* mesh_verts;        // device buffer [n][3] (model-owned), null without meshes
  // tables of the wave task stage, built once with the model (build_stage_tables)
  // so that no stage gathers model constants through dependent loads per instance:
  uint32_t rev_mask;               // bit (j-1) set iff joint j is revolute
  uint64_t anc_bits[4];            // bit 16 (j-1) + (k-1) set iff joint k supports joint j: anc[] as one bit table
  // per-slot broad-phase records, field-major: field f of slot sl of
  // pair_order (the broad phase's lane order) at pair_tab[f * pair_ld + sl].
  // Fields: kPairMeta (pair | ga << 16 | gb << 24 | type a << 32 | type b << 36,
  // the double's bits), gparam of a (3), gparam of b (3), gbound of a, of b.
  const double* pair_tab;          // device buffer (model-owned)
  int pair_ld;
  // obstacle slots (set_obstacles; appended, as the hull fields were):
  // geometries [obst0, obst0 + nobst) have parent 0 and a pose that is an input
  // of each call, not gplace (which holds the identity)
  int nobst, obst0;
  // motion weights of the certified path clearance (build_motion_tables;
  // appended): weight of joint j (1-based) on pair p at
  // motion_wt[(j - 1) * motion_ld + p], the bound on the pair's relative motion
  // per unit of |dq_j| (clearance_certify.hpp); travel_mask: bit (k-1) set iff
  // the weights assume |q_k| <= max(|lower_k|, |upper_k|) of the prismatic joint k
  const double* motion_wt;         // device buffer [nv][motion_ld] (model-owned)
  int motion_ld;
  uint32_t travel_mask;
};
constexpr int kPairFields = 9;
constexpr int kPairMeta = 0, kPairParamA = 1, kPairParamB = 4, kPairBoundA = 7, kPairBoundB = 8;

struct HostModel {
  DevModel dev{};
  std::vector<std::string> joint_names;   // index j-1
  std::vector<std::string> frame_names;   // link (BODY) frames, index = frame id
  std::vector<std::string> geom_names;
  std::vector<double> effort;
  // convex hulls of the collision meshes (mesh.hpp), all in one buffer:
  // geometry g owns vertices [mesh_first[g], mesh_first[g] + mesh_count[g]),
  // relative to the centre of their bounding box (the offset is in gplace)
  std::vector<double> mesh_verts;         // [n][3]
  std::vector<int> mesh_first, mesh_count;  // per geometry (count 0: primitive)
  std::vector<double> mesh_residual;        // per geometry: what a reduced hull leaves out (mesh.hpp)
  std::vector<std::string> mesh_files;      // per geometry: the resolved file
  std::vector<double> pair_tab;             // DevModel::pair_tab, [kPairFields][dev.pair_ld]
  std::vector<std::string> geom_link;       // per geometry of the URDF: its link
  int base_pairs = 0;                       // pairs of the URDF / SRDF (the obstacle pairs follow them)
  std::vector<double> motion_rho;           // [nv][ngeom]: reach of geometry g about joint j's origin (build_motion_tables)
  std::vector<double> motion_wt;            // DevModel::motion_wt, [nv][dev.motion_ld]
  bool motion_unbounded = false;            // a joint of travel_mask has a non-finite limit: no certificate
  bool has_mesh() const { return !mesh_verts.empty(); }
};

// Returns 0 on success, DRC_ERR_* otherwise; err gets a readable reason.
// packages_path: where package://a/b mesh URIs are looked up (<packages_path>/a/b).
int build_model_from_urdf(const std::string& urdf_path, const std::string& srdf_path,
                          const std::string& packages_path, HostModel* out, std::string* err);
// Fills rev_mask / anc_bits and the per-slot pair records from the model's
// jtype / anc / pair / geometry arrays (called by build_model_from_urdf).
void build_stage_tables(HostModel* hm);
// Fills pair_order / slot_a / slot_b, the candidate slots and the stage tables
// from the geometry and pair arrays (called by build_model_from_urdf and
// set_obstacles).
void build_pair_tables(HostModel* hm);
// Fills motion_rho, motion_wt, motion_ld, travel_mask and motion_unbounded from
// the kinematic tree, the joint limits and the geometry and pair arrays (called
// where build_pair_tables is: by build_model_from_urdf and set_obstacles).
//   rad_g      bounding radius of geometry g about its frame origin, from gparam
//   travel_k   max(|lower_k|, |upper_k|) of a prismatic joint k
//   rho[j][g]  for j supporting g's parent joint c: the sum over the joints k of
//              the chain strictly below j down to c of |p(jplace[k])| (+ travel_k,
//              k prismatic), plus |p(gplace[g])| + rad_g; 0 otherwise
//   wt[j][p]   0 if j supports both or neither geometry of pair p; otherwise 1
//              (j prismatic) or rho[j][the supported one] (j revolute)
void build_motion_tables(HostModel* hm);
// Declares n obstacle slots (replacing any earlier ones; n = 0 removes them and
// leaves the model what build_model_from_urdf made): geometries ngeom .. with
// parent 0, identity placement, type[i] (kSphere, kCylinder, kBox, kHalfSpace)
// and param[i][3], each paired with every geometry of the named links
// (n_links = 0: of every link that a joint moves).  The host tables only: the
// caller uploads them.  Returns 0 or DRC_ERR_*, the model unchanged on error.
int set_obstacles(HostModel* hm, int n, const int* type, const double* param, const char* const* links, int n_links,
                  std::string* err);

}  // namespace drc_amd
