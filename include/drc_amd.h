/*
 * drc_amd.h — C-ABI of the MI355X-native batched QP-IK solver.
 *
 * This is the drop-in boundary for the per-control-cycle hot path of
 * YoungWook0533/dyros_robot_controller.  Plain C: opaque
 * handles, plain pointers and sizes, integer return codes, no C++ types and
 * no exceptions cross it.  Every entry point names the reference interface
 * it replaces (file:line in the reference tree).
 *
 * Conventions
 *  - Batched arrays are structure-of-arrays, field-major: element (f, b) of
 *    a [F][B] array is at ptr[f * B + b].  All batched pointers are DEVICE
 *    pointers owned by the caller (HBM resident); `stream` is a hipStream_t
 *    (NULL = default stream).  Calls are asynchronous on that stream.  A
 *    model keeps its per-call scratch (task records, work-queue counters)
 *    per caller stream (at most 8 streams; see drc_model_release_stream), so
 *    calls on one model from several streams never share scratch, and calls
 *    from several host threads are safe (each call's launches are enqueued as
 *    a unit).  The internal fork/join streams of the concurrent sub-batches
 *    are per model, shared by the caller streams.
 *  - Poses are 12 doubles: R column-major (9) then p (3) — Eigen::Affine3d
 *    `linear()` memory order followed by `translation()`.
 *  - Velocities / twists are [v(3); w(3)] in the world frame
 *    (Pinocchio LOCAL_WORLD_ALIGNED, robot_data.cpp:401).
 *
 * Diagnostic entries with no reference counterpart (kernel timing, stage
 * stamps, LDS / occupancy plans, the lane-stage switch) are declared in
 * drc_amd_debug.h; the product boundary is this header.
 */
#ifndef DRC_AMD_H
#define DRC_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- return codes ------------------------------------------------------ */
enum {
    DRC_OK = 0,
    DRC_ERR_INVALID_ARGUMENT = 1,
    DRC_ERR_FILE = 2,            /* URDF missing: reference std::exit()s (robot_data.cpp:17-18) */
    DRC_ERR_PARSE = 3,
    DRC_ERR_UNSUPPORTED = 4,     /* model outside the kernel's limits          */
    DRC_ERR_UNKNOWN_LINK = 5,    /* reference: stderr + zero result (:395-399) */
    DRC_ERR_HIP = 6,
    DRC_ERR_SIZE_MISMATCH = 7    /* reference: std::runtime_error (robot_controller.cpp:23-26) */
};

/* ---- per-instance solve status (mirrors OSQP status values) ------------ */
enum {
    DRC_STATUS_SOLVED = 1,
    DRC_STATUS_MAX_ITER = -2,
    DRC_STATUS_PRIMAL_INFEASIBLE = -3,
    DRC_STATUS_NONFINITE = -10
};

/* ---- controller entry points (robot_controller.h) ---------------------- */
enum {
    DRC_MODE_QPIK = 0,           /* QPIK(xdot_target)              manipulator/robot_controller.cpp:277 */
    DRC_MODE_QPIK_STEP = 1,      /* QPIKStep(x_target, xdot_target)                                :292 */
    DRC_MODE_QPIK_CUBIC = 2      /* QPIKCubic(x_t, xd_t, x_i, xd_i, t, t0, T)                     :303 */
};

/* ---- mobile base description (type_define.h:58-72 KinematicParam) ------ */
enum { DRC_DRIVE_DIFFERENTIAL = 0, DRC_DRIVE_MECANUM = 1, DRC_DRIVE_CASTER = 2 };
#define DRC_MAX_WHEELS 8
typedef struct drc_kinematic_param {
    int type;
    double wheel_radius;
    double max_lin_speed, max_ang_speed, max_lin_acc, max_ang_acc;
    double base_width;                              /* differential */
    int n_wheels;                                   /* mecanum wheels / casters (W = 2 per caster) */
    double roller_angles[DRC_MAX_WHEELS];
    double base2wheel_positions[DRC_MAX_WHEELS][2];
    double base2wheel_angles[DRC_MAX_WHEELS];
    double wheel_offset;                            /* caster */
} drc_kinematic_param;

/* type_define.h:151-156 / :167-171 */
typedef struct drc_joint_index { int virtual_start, mani_start, mobi_start; } drc_joint_index;
typedef struct drc_actuator_index { int mani_start, mobi_start; } drc_actuator_index;

/* ---- QP solver settings: OSQP's ADMM (QP_base.h:143-165) --------------- */
typedef struct drc_solver_settings {
    double rho, sigma, alpha;          /* 0.1, 1e-6, 1.6                    */
    double eps_abs, eps_rel;           /* 1e-3, 1e-3 (reference: defaults)  */
    double eps_prim_inf;               /* 1e-4                              */
    int max_iter;                      /* 4000                              */
    int check_termination;             /* 25                                */
    int scaling;                       /* 10 Ruiz iterations                */
    int adaptive_rho;                  /* 1                                 */
    int adaptive_rho_interval;         /* 25                                */
    double adaptive_rho_tolerance;     /* 5                                 */
    int polish;                        /* reference: 0                      */
    int polish_refine_iter;            /* 3                                 */
    double delta;                      /* 1e-6                              */
    int exact;                         /* 1: certified polish + tight fallback (parity mode) */
    double eps_exact;                  /* 1e-9 KKT acceptance of a polished point */
    double eps_fallback;               /* 1e-7 ADMM-only termination when polish keeps failing */
} drc_solver_settings;

/* ---- QPIK parameters (controller gains + QP constants) ----------------- */
typedef struct drc_qpik_params {
    double kp[6], kv[6];               /* manipulator: 100 / 20 (robot_controller.cpp:12-13)
                                          MoMa: 400 / 0 (mobile_manipulator/robot_controller.cpp:15) */
    double feedforward;                /* MoMa QPIKStep adds xdot_target (:177): 1; manipulator 0 */
    double alpha_cbf;                  /* 50      (QP_IK.cpp:101)           */
    double w_reg;                      /* 1.0 / 0.01 (QP_IK.cpp:81, MoMa :71) */
    double slack_w;                    /* 1000    (QP_IK.cpp:83-86)         */
    double man_min;                    /* 0.01    (QP_IK.cpp:122)           */
    double dist_min;                   /* 0.05    (QP_IK.cpp:130)           */
    int mode;                          /* DRC_MODE_*                        */
    int frame_id;                      /* from drc_model_find_frame         */
    double t, t0, duration;            /* QPIKCubic timing                  */
    drc_solver_settings solver;
} drc_qpik_params;

typedef struct drc_model drc_model;     /* opaque; owns its device copy */

/* Manipulator::RobotData(urdf, srdf, packages)  manipulator/robot_data.h:49,
 * robot_data.cpp:7-70 (model, collision pairs, limits).  `device` = HIP
 * device ordinal that receives the model constants.
 * Collision geometry: sphere, cylinder, box, and <mesh filename= scale=>
 * (binary / ASCII STL, OBJ), which becomes the convex hull of its vertices
 * (drc_mesh_convex_hull).  packages_path: package://a/b.stl is read from
 * <packages_path>/a/b.stl; file:// and absolute paths as given, relative
 * paths against the URDF's directory.  NULL or "" is fine unless a
 * package:// URI occurs.  A mesh file that is missing (DRC_ERR_FILE), of
 * another format or degenerate (DRC_ERR_UNSUPPORTED) fails the build with the
 * link and the file in drc_last_error(). */
int drc_model_create_manipulator(const char* urdf_path, const char* srdf_path,
                                 const char* packages_path, int device, drc_model** out);

/* MobileManipulator::RobotData(param, joint_idx, actuator_idx, urdf, srdf, packages)
 * mobile_manipulator/robot_data.h:55, robot_data.cpp:7-44. */
int drc_model_create_mobile_manipulator(const drc_kinematic_param* param,
                                        const drc_joint_index* joint_idx,
                                        const drc_actuator_index* actuator_idx,
                                        const char* urdf_path, const char* srdf_path,
                                        const char* packages_path, int device, drc_model** out);

void drc_model_destroy(drc_model* model);

/* getDof / getActuatordDof / getManipulatorDof / getMobileDof
 * (manipulator/robot_data.h, mobile_manipulator/robot_data.h) and the
 * collision model size (geometries, active pairs). */
int drc_model_info(const drc_model* model, int* dof, int* actuated_dof, int* mani_dof,
                   int* mobi_dof, int* n_geoms, int* n_pairs);

/* Collision geometry `geom` (0 .. n_geoms-1, the obstacle slots of
 * drc_model_set_obstacles last): *type 0 sphere, 1 cylinder, 2 box,
 * 3 mesh (convex hull), 4 half-space (an obstacle slot; param zero); param: sphere r | cylinder r, h/2 | box half extents |
 * mesh: half extents of the hull's bounding box; *n_vertices: hull vertices
 * (0 for primitives); *hull_residual: 0 for a full hull, else what the
 * 256-vertex cap left out (drc_mesh_convex_hull).  Outputs may be NULL. */
int drc_model_geom_info(const drc_model* model, int geom, int* type, double param[3],
                        int* n_vertices, double* hull_residual);

/* What a collision mesh file turns into (host only, no device is touched; the
 * model build calls the same code).  Reads a binary / ASCII STL or an OBJ
 * (`v` lines), multiplies by scale (NULL: 1 1 1) and returns the vertices of
 * the convex hull in file order: verts_out [cap][3], *n_out their number.
 * max_vertices (<= 0: 256, the model's per-mesh cap; else >= 4): a hull with
 * more vertices is cut short by stopping quickhull's farthest-point insertion
 * there -- a subset of the hull's vertices, hence an inner approximation --
 * and *residual_out is the largest distance of a left-out vertex from the
 * reduced hull (0 otherwise).  DRC_ERR_FILE: missing / unreadable file;
 * DRC_ERR_UNSUPPORTED: another format (Collada, ...) or fewer than four
 * non-coplanar vertices; DRC_ERR_SIZE_MISMATCH: cap too small (*n_out set). */
int drc_mesh_convex_hull(const char* path, const double scale[3], int max_vertices,
                         double* verts_out, int cap, int* n_out, double* residual_out);

/* getJointPositionLimit / getJointVelocityLimit (robot_data.h) — host arrays [dof] */
int drc_model_limits(const drc_model* model, double* q_lb, double* q_ub, double* qdot_lb,
                     double* qdot_ub);

/* pinocchio Model::getFrameId(link_name) as used by every getter
 * (robot_data.cpp:380,394): DRC_ERR_UNKNOWN_LINK when absent. */
int drc_model_find_frame(const drc_model* model, const char* link_name, int* frame_id);

/* Mobile FK Jacobian J_mobile (3 x W, row-major) of the base
 * (mobile/robot_data.cpp:123-176); host array.  Differential / mecanum only:
 * a caster base's J_mobile depends on the steer angles (drc_mobile_fk_jacobian). */
int drc_model_mobile_fk_jacobian(const drc_model* model, double* J3xW);

/* Mobile::RobotData::computeFKJacobian(wheel_pos) (mobile/robot_data.cpp:123-204)
 * for any drive, host arrays: J3xW [3][W] row-major; wheel_pos [W] (caster:
 * steer angle at 2i, drive angle at 2i+1; ignored otherwise, may be NULL);
 * *n_wheels receives W.  KinematicParam.n_wheels counts mecanum wheels or
 * casters (W = 2 x casters, :27-30). */
int drc_mobile_fk_jacobian(const drc_kinematic_param* param, const double* wheel_pos, double* J3xW, int* n_wheels);
/* Mobile::RobotController::computeIKJacobian (mobile/robot_controller.cpp:55-125):
 * wheel velocities = J [W][3] row-major * base twist; same arguments. */
int drc_mobile_ik_jacobian(const drc_kinematic_param* param, const double* wheel_pos, double* JWx3, int* n_wheels);

/* Reference defaults for the model kind (robot_controller ctor gains, QP
 * constants, OSQP defaults).  exact=0: the reference's OSQP settings
 * (eps 1e-3, no polish); exact=1: certified-optimal settings used for
 * parity. */
int drc_default_qpik_params(const drc_model* model, int exact, drc_qpik_params* params);

/* Batched QPIK / QPIKStep / QPIKCubic.
 *   Manipulator  (robot_controller.cpp:277-317): q, qdot [dof][B].
 *   Mobile manip (mobile_manipulator/robot_controller.cpp:147-197): q, qdot
 *       are the full joint vectors [dof][B] in JointIndex order
 *       (getJointVector, mobile_manipulator/robot_data.cpp:418-427).
 *   x_target [12][B] (modes STEP/CUBIC), xdot_target [6][B],
 *   x_init [12][B] / xdot_init [6][B] (mode CUBIC only, else NULL).
 *   qdot_out [na][B]: manipulator na = dof (QPIK returns qdot);
 *       MoMa na = actuated dof in ActuatorIndex order (eta, split into
 *       (qdot_mobile, qdot_arm) by ActuatorIndex, :161-164).
 *   status [B] (DRC_STATUS_*), iters [B] (may be NULL).
 * Non-solved instances get a zero output (QP_IK.cpp:56-61). */
int drc_qpik_batch(const drc_model* model, const drc_qpik_params* params, int64_t B,
                   const double* q, const double* qdot, const double* x_target,
                   const double* xdot_target, const double* x_init, const double* xdot_init,
                   double* qdot_out, int32_t* status, int32_t* iters, void* stream);

/* Closed-loop rollout: `steps` control cycles of drc_qpik_batch with the
 * reference loop's integration q_desired = q + qdot_desired * dt between them
 * (examples/C++/src/fr3_controller.cpp:123-134), enqueued on `stream` without
 * host synchronisation.  For step k = 0 .. steps-1 on the state (q_k, v_k),
 * (q_0, v_0) = (q0, qdot0) [dof][B]:
 *   (eta_k, status_k, iters_k) are exactly drc_qpik_batch's results for
 *       `params` with t = params->t + (double)k * dt (product rounded, then
 *       the sum) on (q_k, v_k) and step k's targets; non-solved instances give
 *       eta_k = 0 and stay where they are;
 *   v_{k+1} = eta_k (manipulator), or S(q_k) eta_k (mobile manipulator: the
 *       selection matrix of mobile_manipulator/robot_data.cpp:22-25,115-120,
 *       virtual block Rz(yaw_k) J_mobile(wheel positions); arm and wheel rows
 *       are eta's entries unchanged);
 *   q_{k+1} = q_k + dt * v_{k+1}, a rounded product then a rounded sum.
 * Targets as drc_qpik_batch; targets_per_step = 1: x_target [steps][12][B] and
 * xdot_target [steps][6][B], one set per step (not with DRC_MODE_QPIK_CUBIC,
 * where the time already moves the target); 0: one set for the horizon.
 * Outputs: q_final, qdot_final [dof][B] = (q_steps, v_steps), required;
 *   q_final may alias q0 and qdot_final qdot0 (no other input is written);
 *   status_traj [steps][B] required; the others may be NULL:
 *   qdot_traj [steps][na][B] = eta_k, iters_traj [steps][B],
 *   q_traj [steps][dof][B] = q_{k+1},
 *   pose_traj [steps][12][B], dist_traj [steps][1+dof][B] at q_k in the
 *   layouts of drc_qpik_stages_batch.
 * The QP shapes the library compiles (drc_set_fusion) run, up to 4 096
 * instances of a manipulator and 65 536 of a mobile manipulator (where it was
 * measured faster; DRC_ROLLOUT_MAX overrides), as one persistent kernel whose
 * waves take an instance through its whole horizon; other models, larger
 * batches and drc_set_fusion(model, 0) run step by step: drc_qpik_batch's
 * launches and a state-update kernel per step.  Results are bit-identical
 * either way, and to `steps` drc_qpik_batch calls with the update above.
 * DRC_ERR_INVALID_ARGUMENT: steps < 1, dt not finite or not positive, a NULL
 * required pointer, per-step targets with CUBIC; otherwise drc_qpik_batch's
 * codes.  B = 0 returns DRC_OK.  (Reference: no counterpart, one robot.) */
int drc_qpik_rollout_batch(const drc_model* model, const drc_qpik_params* params,
                           int64_t B, int steps, double dt,
                           const double* q0, const double* qdot0,
                           const double* x_target, const double* xdot_target,
                           const double* x_init, const double* xdot_init,
                           int targets_per_step,
                           double* q_final, double* qdot_final,
                           double* qdot_traj, int32_t* status_traj, int32_t* iters_traj,
                           double* q_traj, double* pose_traj, double* dist_traj,
                           void* stream);

/* Stage outputs of the same kernel for parity checks: per instance
 *   pose [12][B]  (getPose with the pose at the current q — SURVEY Q1),
 *   jac  [6*dof][B] row-major (getJacobian, LWA),
 *   man  [1+mani][B] (manipulability, grad)  (getManipulability(true,false)),
 *   dist [1+dof][B]  (distance, grad)        (getMinDistance(true,false,false)),
 *   pair [B] (argmin collision pair), xdot_des [6][B] (the QP's task velocity).
 * Any output pointer may be NULL.  params->frame_id == -1 selects no task
 * frame (pose/jac/man/xdot_des then refer to the last joint's frame), for
 * callers that only need the distance stage (getMinDistance). */
int drc_qpik_stages_batch(const drc_model* model, const drc_qpik_params* params, int64_t B,
                          const double* q, const double* qdot, const double* x_target,
                          const double* xdot_target, const double* x_init,
                          const double* xdot_init, double* pose, double* jac, double* man,
                          double* dist, int32_t* pair, double* xdot_des, void* stream);

/* Obstacle slots: world geometry in the distance stage of QPIK, with poses that
 * are inputs of each call (a table, a floor, a wall, a moving object; one
 * scene per instance if wanted).  Declares n slots, replacing any declared
 * before; they are the model's geometries n_geoms .. n_geoms + n - 1 (n_geoms of
 * the URDF), parent joint 0, identity placement.  A slot's shape is a model
 * constant:
 *   type [n]      0 sphere, 1 cylinder, 2 box as drc_model_geom_info, or
 *                 4 half-space: for a pose (R, p) the solid
 *                 {x : (x - p) . R e_z <= 0} (floor, table top, wall);
 *                 3 (mesh) is refused with DRC_ERR_UNSUPPORTED;
 *   param [n][3]  sphere r | cylinder r, h/2 | box half extents, finite and
 *                 positive; ignored for a half-space (may be NULL if all are).
 * Each slot is paired with every collision geometry of the links named in
 * links [n_links] (DRC_ERR_UNKNOWN_LINK for a name the URDF lacks); links =
 * NULL, n_links = 0: of every link that a joint moves.  The new pairs follow the
 * model's own, slot by slot, the geometries in index order, so pair indices
 * reported by the stage entries stay those of the URDF for the self pairs.
 * There are no obstacle-obstacle pairs.  Name the links: a floor under a
 * fixed-base arm is a constant few centimetres from the first link and would
 * win every minimum.
 * A half-space pair is decided exactly, in closed form on both sides of the
 * plane (d < 0: penetration depth); primitive obstacles go through the same
 * narrow phase as the robot's own geometry.
 * n = 0 removes the slots: the model is then bit for bit what its build made.
 * The call waits for the model's outstanding work and replaces its device
 * tables; it must not run concurrently with other calls on the model.
 * DRC_ERR_UNSUPPORTED: more than 64 geometries or 1024 pairs in all, a mesh
 * obstacle, or a model with collision meshes (hull models take no obstacles).
 * While a model has slots, the plain drc_qpik_batch / drc_qpik_stages_batch /
 * drc_qpik_rollout_batch / drc_qpik_reach_batch and their host forms return DRC_ERR_INVALID_ARGUMENT
 * (they have no poses to give), and drc_qpid_*, drc_clik_batch, drc_osf_batch,
 * drc_closed_form_host, drc_joint_torque_step_* and drc_debug_lane_stage return
 * DRC_ERR_UNSUPPORTED; kinematics and dynamics entries are unaffected.
 * (Reference: no counterpart; its getMinDistance is a self-collision query.) */
int drc_model_set_obstacles(drc_model* model, int n, const int* type, const double* param,
                            const char* const* links, int n_links);

/* drc_qpik_batch / drc_qpik_stages_batch on a model with obstacle slots.
 *   obstacle_pose [n][12][obstacle_ld]: slot k's pose in x_target's layout (R
 *       column-major, then p), world frame, field-major;
 *   obstacle_ld: the row stride, >= B: a pose set per instance; 0: one [n][12]
 *       set shared by the batch.
 * Everything else as the plain entries; results do not depend on fusion, on
 * the batch split, or on whether shared poses are passed shared or replicated.
 * DRC_ERR_INVALID_ARGUMENT on a model without slots.
 * (Reference: no counterpart.) */
int drc_qpik_obstacles_batch(const drc_model* model, const drc_qpik_params* params, int64_t B,
                             const double* q, const double* qdot, const double* x_target,
                             const double* xdot_target, const double* x_init,
                             const double* xdot_init, const double* obstacle_pose,
                             int64_t obstacle_ld, double* qdot_out, int32_t* status,
                             int32_t* iters, void* stream);
int drc_qpik_stages_obstacles_batch(const drc_model* model, const drc_qpik_params* params,
                                    int64_t B, const double* q, const double* qdot,
                                    const double* x_target, const double* xdot_target,
                                    const double* x_init, const double* xdot_init,
                                    const double* obstacle_pose, int64_t obstacle_ld,
                                    double* pose, double* jac, double* man, double* dist,
                                    int32_t* pair, double* xdot_des, void* stream);

/* drc_qpik_rollout_batch on a model with obstacle slots: obstacle_pose and
 * obstacle_ld as above; obstacles_per_step = 0: one pose set for the horizon,
 * 1: obstacle_pose [steps][n][12][obstacle_ld] (or [steps][n][12] with
 * obstacle_ld = 0), one set per step: moving obstacles, as targets_per_step
 * does for targets.  Runs step by step (no persistent kernel takes poses):
 * bit-identical to `steps` drc_qpik_obstacles_batch calls with the state update
 * of drc_qpik_rollout_batch.  (Reference: no counterpart.) */
int drc_qpik_rollout_obstacles_batch(const drc_model* model, const drc_qpik_params* params,
                                     int64_t B, int steps, double dt,
                                     const double* q0, const double* qdot0,
                                     const double* x_target, const double* xdot_target,
                                     const double* x_init, const double* xdot_init,
                                     int targets_per_step,
                                     const double* obstacle_pose, int64_t obstacle_ld,
                                     int obstacles_per_step,
                                     double* q_final, double* qdot_final,
                                     double* qdot_traj, int32_t* status_traj, int32_t* iters_traj,
                                     double* q_traj, double* pose_traj, double* dist_traj,
                                     void* stream);

/* Moving obstacles: the three obstacle entries with a twist per slot, so that
 * the distance constraint sees where an obstacle is going and not only where
 * it is.
 *   obstacle_twist [n][6][obstacle_ld] (or [n][6] with obstacle_ld = 0), laid
 *       out like obstacle_pose with 6 values in place of 12: v (3), the velocity
 *       of the slot pose's origin p, then omega (3), the angular velocity.
 * Frame: both are expressed in the world frame and v is taken at the pose's
 * origin -- world-aligned at the local origin, the convention of the frame
 * Jacobian (LOCAL_WORLD_ALIGNED).  For mobile manipulators it is the world
 * frame too, like the poses.
 * With the closest pair's witnesses pA (robot) and pB (obstacle), n = (pB - pA)
 * / |pB - pA| and s = +1 (d >= 0) or -1 (d < 0),
 *   dist_rate = dd/dt at rest = s n . (v + omega x (pB - p)),
 * exact for a half-space too (pB the projection onto the plane), and 0 when a
 * self pair is the closest.  The QP's distance row becomes
 *   grad d . qdot (+ slack) >= -alpha_cbf (d - dist_min) - dist_rate;
 * nothing else changes.  The term reaches the QP as the distance d + dist_rate
 * / alpha_cbf, so a call with twists needs alpha_cbf > 0
 * (DRC_ERR_INVALID_ARGUMENT otherwise).  Every distance a caller sees (dist,
 * dist_traj) stays the geometric d.
 * Mobile manipulators: the row keeps the reference's arm-only columns; the
 * base's own motion is not part of it, with or without twists.
 * obstacle_twist = NULL: the obstacle entry itself, bit for bit (dist_rate 0).
 * drc_qpik_stages_moving_obstacles_batch: dist_rate [B] (may be NULL) is the
 * one new output.  drc_qpik_rollout_moving_obstacles_batch: obstacle_twist
 * gets the leading [steps] axis with obstacles_per_step = 1, like the poses;
 * bit-identical to `steps` drc_qpik_moving_obstacles_batch calls with the state
 * update of drc_qpik_rollout_batch.  The poses are the caller's: nothing
 * integrates them on the device.
 * Error codes as the obstacle entries (a model without slots, a bad
 * obstacle_ld: DRC_ERR_INVALID_ARGUMENT); a refused call writes nothing.
 * The reach entries take one static scene per call and no twists.
 * (Reference: no counterpart.) */
int drc_qpik_moving_obstacles_batch(const drc_model* model, const drc_qpik_params* params,
                                    int64_t B, const double* q, const double* qdot,
                                    const double* x_target, const double* xdot_target,
                                    const double* x_init, const double* xdot_init,
                                    const double* obstacle_pose, const double* obstacle_twist,
                                    int64_t obstacle_ld, double* qdot_out, int32_t* status,
                                    int32_t* iters, void* stream);
int drc_qpik_stages_moving_obstacles_batch(const drc_model* model, const drc_qpik_params* params,
                                           int64_t B, const double* q, const double* qdot,
                                           const double* x_target, const double* xdot_target,
                                           const double* x_init, const double* xdot_init,
                                           const double* obstacle_pose,
                                           const double* obstacle_twist, int64_t obstacle_ld,
                                           double* pose, double* jac, double* man, double* dist,
                                           int32_t* pair, double* xdot_des, double* dist_rate,
                                           void* stream);
int drc_qpik_rollout_moving_obstacles_batch(const drc_model* model, const drc_qpik_params* params,
                                            int64_t B, int steps, double dt,
                                            const double* q0, const double* qdot0,
                                            const double* x_target, const double* xdot_target,
                                            const double* x_init, const double* xdot_init,
                                            int targets_per_step,
                                            const double* obstacle_pose,
                                            const double* obstacle_twist, int64_t obstacle_ld,
                                            int obstacles_per_step,
                                            double* q_final, double* qdot_final,
                                            double* qdot_traj, int32_t* status_traj,
                                            int32_t* iters_traj, double* q_traj, double* pose_traj,
                                            double* dist_traj, void* stream);

/* ---- goal-reaching rollouts: how an instance of drc_qpik_reach_batch stopped */
enum {
    DRC_REACH_REACHED = 0,       /* pose within pos_tol and rot_tol of x_target        */
    DRC_REACH_BUDGET = 1,        /* max_steps steps taken and still outside them       */
    DRC_REACH_QP_FAILED = 2      /* a step's QP was not solved; the state is unchanged */
};

/* Goal-reaching rollout: the closed loop of drc_qpik_rollout_batch in mode
 * DRC_MODE_QPIK_STEP towards one pose x_target [12][B], where every instance
 * stops on its own.  For each instance, with (q_0, v_0) = (q0, qdot0) and k = 0:
 *   1. the task stage of drc_qpik_batch at (q_k, v_k) gives the pose of the
 *      task frame (and d, grad d).  Its error against x_target is two numbers,
 *      every product and sum rounded (no fma), in this order:
 *        e_p = (dx*dx + dy*dy) + dz*dz, d = x_target[9..11] - pose[9..11];
 *        e_R = sum over i = 0 .. 8, from 0 upward, of (pose[i] - x_target[i])^2
 *            = |R - R_t|_F^2 = 8 sin^2(theta / 2);
 *   2. e_p <= tau_p and e_R <= tau_R: DRC_REACH_REACHED, stop (a NaN fails
 *      both comparisons and goes on to the QP);
 *   3. k == max_steps: DRC_REACH_BUDGET, stop;
 *   4. the step's QP gives (eta_k, status_k, iters_k), exactly drc_qpik_batch's
 *      results on (q_k, v_k).  status_k != DRC_STATUS_SOLVED:
 *      DRC_REACH_QP_FAILED, stop, the state unchanged (eta_k = 0: a fixed
 *      horizon would solve the same failing QP at every remaining step).
 *      Otherwise the state update of drc_qpik_rollout_batch (the same bits),
 *      k += 1, back to 1.
 * tau_p = pos_tol * pos_tol, tau_R = 8 * (s * s) with s = sin(0.5 * rot_tol),
 * computed once on the host: drc_reach_thresholds returns the very numbers.
 * params->t is not advanced (QPIKStep does not read it).
 * Outputs, [..][B] field-major:
 *   q_final, qdot_final [dof][B]: the state where the instance stopped, always
 *       written (k = 0: the inputs); may alias q0 / qdot0; required;
 *   result [B] (DRC_REACH_*), steps_used [B] (the k at the stop); required;
 *   status_last [B]: the status of the last QP that ran, 0 if none ran;
 *   iters_total [B]: the sum of the ADMM iterations;
 *   err_final [2][B]: e_p, e_R at q_final;
 *   dist_final [1+dof][B]: d, grad d at q_final, drc_qpik_stages_batch's layout;
 *       these four may be NULL.
 * A call takes at most max_steps QP solves and max_steps + 1 task stages per
 * instance; max_steps = 0 only checks the error.
 * The QP shapes the library compiles (drc_set_fusion), on a model without
 * collision meshes or obstacle slots and up to DRC_REACH_MAX instances
 * (default 65 536, the largest batch measured: the persistent kernel was
 * faster at every size, DESIGN.md "Reach"), run as one persistent kernel
 * whose waves leave an instance when it stops and take the next.  Everything
 * else runs step by step: per step the stage launch, drc_qpik_batch's launches
 * and an update kernel that skips the instances that have stopped.  That path
 * cannot end early: it enqueues max_steps steps for the whole batch, and the
 * stopped instances still run through the launches, their results ignored.
 * Results are bit-identical either way.
 * DRC_ERR_INVALID_ARGUMENT: a mode other than DRC_MODE_QPIK_STEP,
 * max_steps < 0, dt / pos_tol / rot_tol not finite or not positive, a NULL
 * required pointer, a model with obstacle slots (drc_qpik_reach_obstacles_batch
 * takes their poses).  B = 0 returns DRC_OK.  Asynchronous on `stream`, no host
 * synchronisation.  (Reference: no counterpart.) */
int drc_qpik_reach_batch(const drc_model* model, const drc_qpik_params* params,
                         int64_t B, int max_steps, double dt, double pos_tol, double rot_tol,
                         const double* q0, const double* qdot0,
                         const double* x_target, const double* xdot_target,
                         double* q_final, double* qdot_final,
                         int32_t* result, int32_t* steps_used,
                         int32_t* status_last, int32_t* iters_total,
                         double* err_final, double* dist_final, void* stream);

/* drc_qpik_reach_batch on a model with obstacle slots: obstacle_pose and
 * obstacle_ld as for drc_qpik_obstacles_batch, one pose set for the horizon.
 * Runs step by step (drc_qpik_reach_path_obstacles_batch with one waypoint
 * gives the same results from a persistent kernel).
 * DRC_ERR_INVALID_ARGUMENT on a model without slots. */
int drc_qpik_reach_obstacles_batch(const drc_model* model, const drc_qpik_params* params,
                                   int64_t B, int max_steps, double dt, double pos_tol,
                                   double rot_tol, const double* q0, const double* qdot0,
                                   const double* x_target, const double* xdot_target,
                                   const double* obstacle_pose, int64_t obstacle_ld,
                                   double* q_final, double* qdot_final,
                                   int32_t* result, int32_t* steps_used,
                                   int32_t* status_last, int32_t* iters_total,
                                   double* err_final, double* dist_final, void* stream);

/* Goal-reaching rollout through waypoints: the loop of drc_qpik_reach_batch
 * towards W = `waypoints` poses in turn.  x_path [W][12][B] and xdot_path
 * [W][6][B] are laid out as the per-step targets of drc_qpik_rollout_batch.
 * Mode DRC_MODE_QPIK_STEP only.  For each instance, with (q_0, v_0) =
 * (q0, qdot0), the total step count k = 0, the segment step count s = 0, the
 * waypoint index w = 0 and dist_min = +inf:
 *   1. the task stage of drc_qpik_batch at (q_k, v_k) with waypoint w as the
 *      target gives the pose, d and grad d.  d < dist_min: dist_min = d (a NaN
 *      is never taken);
 *   2. (e_p, e_R) against x_path[w], formed and compared exactly as in
 *      drc_qpik_reach_batch (drc_reach_thresholds).  Within: steps_at[w] = k,
 *      w += 1, s = 0; w == W: DRC_REACH_REACHED, stop; otherwise back to 1 at
 *      the same state with the new target (the pose and d do not depend on the
 *      target, the task record the QP reads does);
 *   3. s == max_steps: DRC_REACH_BUDGET, stop -- the budget is per segment;
 *   4. the step's QP, exactly drc_qpik_batch on (q_k, v_k) towards x_path[w] /
 *      xdot_path[w].  Not solved: DRC_REACH_QP_FAILED, stop, the state
 *      unchanged.  Otherwise the state update of drc_qpik_rollout_batch (the
 *      same bits), k += 1, s += 1, back to 1.
 * This is, bit for bit, W chained drc_qpik_reach_batch calls, each starting
 * from the previous q_final / qdot_final, where an instance goes on to the
 * next call only if its previous result is DRC_REACH_REACHED; W = 1 is
 * drc_qpik_reach_batch itself.
 * Outputs, [..][B] field-major:
 *   q_final, qdot_final [dof][B]: may alias q0 / qdot0; result [B]
 *       (DRC_REACH_*); waypoints_reached [B]: the w at the stop, 0 .. W;
 *       steps_used [B]: the total k; these five are required;
 *   status_last [B]: the status of the last QP that ran in the whole call, 0 if
 *       none ran; iters_total [B]: the sum of the ADMM iterations over the call;
 *   err_final [2][B]: the error against waypoint min(w, W - 1) at q_final;
 *   dist_final [1+dof][B]: d, grad d at q_final;
 *   dist_min [B]: the least d over every state at which the stage ran;
 *   steps_at [W][B]: the k at which waypoint w was found reached, -1 for those
 *       never reached; these six may be NULL.
 * A call takes at most W max_steps QP solves and W max_steps + W task stages
 * per instance; max_steps = 0 only walks through the waypoints that are
 * already satisfied.
 * The dispatch is drc_qpik_reach_batch's (compiled QP shape, no collision
 * meshes, drc_set_fusion, up to DRC_REACH_MAX instances: one persistent
 * kernel), except that a model with obstacle slots qualifies too, through
 * drc_qpik_reach_path_obstacles_batch.  Everything else runs in W (max_steps
 * + 1) rounds of the stage launch, drc_qpik_batch's launches and an update
 * kernel, every instance's current target held in stream scratch.  Results are
 * bit-identical either way.
 * DRC_ERR_INVALID_ARGUMENT: as drc_qpik_reach_batch, waypoints < 1, a model
 * with obstacle slots (drc_qpik_reach_path_obstacles_batch takes their poses).
 * B = 0 returns DRC_OK.  Asynchronous on `stream`, no host synchronisation.
 * (Reference: no counterpart.) */
int drc_qpik_reach_path_batch(const drc_model* model, const drc_qpik_params* params,
                              int64_t B, int waypoints, int max_steps, double dt,
                              double pos_tol, double rot_tol,
                              const double* q0, const double* qdot0,
                              const double* x_path, const double* xdot_path,
                              double* q_final, double* qdot_final,
                              int32_t* result, int32_t* waypoints_reached, int32_t* steps_used,
                              int32_t* status_last, int32_t* iters_total,
                              double* err_final, double* dist_final,
                              double* dist_min, int32_t* steps_at, void* stream);

/* drc_qpik_reach_path_batch on a model with obstacle slots: obstacle_pose and
 * obstacle_ld as for drc_qpik_reach_obstacles_batch, one pose set for the
 * call.  The persistent kernel where the dispatch above allows it.
 * DRC_ERR_INVALID_ARGUMENT on a model without slots (drc_qpik_reach_path_batch
 * runs it). */
int drc_qpik_reach_path_obstacles_batch(const drc_model* model, const drc_qpik_params* params,
                                        int64_t B, int waypoints, int max_steps, double dt,
                                        double pos_tol, double rot_tol,
                                        const double* q0, const double* qdot0,
                                        const double* x_path, const double* xdot_path,
                                        const double* obstacle_pose, int64_t obstacle_ld,
                                        double* q_final, double* qdot_final,
                                        int32_t* result, int32_t* waypoints_reached,
                                        int32_t* steps_used,
                                        int32_t* status_last, int32_t* iters_total,
                                        double* err_final, double* dist_final,
                                        double* dist_min, int32_t* steps_at, void* stream);

/* ---- reach from several seeds per target -------------------------------------- */
enum {
    DRC_REACH_CANCELLED = 3      /* drc_qpik_reach_seeds_batch, inst_result only: stopped
                                    because another seed of its group had won          */
};
enum {
    DRC_SEEDS_FIRST = 0,         /* the lowest seed index that reached                 */
    DRC_SEEDS_FEWEST_STEPS = 1   /* the least steps_used, ties to the lowest index     */
};

/* Reach from several seeds per target: for each of T = `targets` poses, S =
 * `seeds` start states are tried and one answer is returned.
 * There are T groups, S seeds per group and S T instances; instance (s, t) is
 * column s T + t of q0, qdot0 [dof][S T].  Targets are per group: x_target
 * [12][T], xdot_target [6][T].  Mode DRC_MODE_QPIK_STEP only.
 * Every instance runs the loop of drc_qpik_reach_batch unchanged.  Its
 * uncancelled outcome is what that entry returns for it: result, steps_used,
 * the finals, status_last, iters_total, err_final, dist_final.
 * The group's winner is defined on uncancelled outcomes alone.
 * If some seed is DRC_REACH_REACHED:
 *   rule = DRC_SEEDS_FIRST: the lowest seed index that reached (order the seeds
 *       by preference: warm start first, then perturbations, then random);
 *   rule = DRC_SEEDS_FEWEST_STEPS: the seed with the least steps_used, ties to
 *       the lowest seed index.
 * If no seed is DRC_REACH_REACHED: the seed with the least e_p at its final
 * state, ties to the least e_R, then to the lowest seed index; a NaN counts as
 * +inf.
 * Outputs per group, [..][T] field-major, each the winner's uncancelled value:
 *   seed [T], result [T], steps_used [T], q_sol, qdot_sol [dof][T]: required;
 *   status_last [T], iters_total [T], err_final [2][T], dist_final [1+dof][T]:
 *       may be NULL.
 * Together they are, bit for bit, what drc_qpik_reach_batch on the S T
 * instances with the targets replicated gives, gathered by the rule above.
 * Cancellation (cancel = 1): an instance that is REACHED at step k publishes a
 * key to its group's word with an atomic min: s under FIRST, k S + s under
 * FEWEST_STEPS.  An instance whose verdict at step k is "not within" (and that
 * has steps left) reads the word and stops as DRC_REACH_CANCELLED if word < s
 * (FIRST) or floor(word / S) <= k (FEWEST_STEPS).  The true winner can never
 * satisfy its own stop condition, so every per-group output is independent of
 * timing; a stale read only delays a stop, and nothing depends on when, or
 * whether, a published key becomes visible.  cancel = 0 runs every instance to
 * its own stop.  Cancellation only changes how much work the losers do.
 * Diagnostics inst_result, inst_steps [S T] (may be NULL): what each instance
 * did in this call.  cancel = 0: exactly drc_qpik_reach_batch's result /
 * steps_used.  cancel = 1: the winners' entries are their uncancelled ones, the
 * others' depend on timing (inst_steps never exceeds the uncancelled count).
 * The dispatch is drc_qpik_reach_path_batch's, applied to S T: compiled QP
 * shape, no collision meshes, drc_set_fusion, up to DRC_REACH_MAX instances run
 * one persistent kernel, models with obstacle slots too
 * (drc_qpik_reach_seeds_obstacles_batch).  Everything else runs the stepwise
 * path of drc_qpik_reach_batch on the S T instances; there is no cancellation
 * there (a lockstep path saves nothing by it).  The per-group outputs are
 * bit-identical either way.  Per-instance results, the replicated targets and
 * the groups' words live in stream scratch.
 * DRC_ERR_INVALID_ARGUMENT: seeds < 1, targets < 0, (max_steps + 1) seeds not
 * below 2^31, seeds targets above the work-queue limit (0x7ffffff0), an unknown
 * rule, any of drc_qpik_reach_batch's own conditions, a model with obstacle
 * slots (drc_qpik_reach_seeds_obstacles_batch takes their poses).  targets = 0
 * returns DRC_OK.  Asynchronous on `stream`, no host synchronisation.
 * (Reference: no counterpart.) */
int drc_qpik_reach_seeds_batch(const drc_model* model, const drc_qpik_params* params,
                               int64_t targets, int seeds, int rule, int cancel,
                               int max_steps, double dt, double pos_tol, double rot_tol,
                               const double* q0, const double* qdot0,
                               const double* x_target, const double* xdot_target,
                               int32_t* seed, int32_t* result, int32_t* steps_used,
                               double* q_sol, double* qdot_sol,
                               int32_t* status_last, int32_t* iters_total,
                               double* err_final, double* dist_final,
                               int32_t* inst_result, int32_t* inst_steps, void* stream);

/* drc_qpik_reach_seeds_batch on a model with obstacle slots: obstacle_pose
 * [n][12][obstacle_ld]; obstacle_ld = 0 is one scene for the whole call,
 * obstacle_ld >= targets one scene per target (column t; every seed of the
 * group meets it).  DRC_ERR_INVALID_ARGUMENT on a model without slots
 * (drc_qpik_reach_seeds_batch runs it). */
int drc_qpik_reach_seeds_obstacles_batch(const drc_model* model, const drc_qpik_params* params,
                                         int64_t targets, int seeds, int rule, int cancel,
                                         int max_steps, double dt, double pos_tol, double rot_tol,
                                         const double* q0, const double* qdot0,
                                         const double* x_target, const double* xdot_target,
                                         const double* obstacle_pose, int64_t obstacle_ld,
                                         int32_t* seed, int32_t* result, int32_t* steps_used,
                                         double* q_sol, double* qdot_sol,
                                         int32_t* status_last, int32_t* iters_total,
                                         double* err_final, double* dist_final,
                                         int32_t* inst_result, int32_t* inst_steps, void* stream);

/* The thresholds of drc_qpik_reach_batch (host only, no device is touched):
 * out[0] = tau_p, out[1] = tau_R.  DRC_ERR_INVALID_ARGUMENT: a tolerance that
 * is not finite and positive, out NULL. */
int drc_reach_thresholds(double pos_tol, double rot_tol, double out[2]);

/* ---- path clearance: the minimum distance along joint-space paths -----------
 * Is the joint-space motion collision-free, and if not, where does it stop
 * being so?  Each of the B instances is one path of `waypoints` full states
 * (q_path [waypoints][dof][B], the layout of a rollout's q_traj, which can be
 * passed straight in; dof is the full state: virtual joints and wheels
 * included, the base yaw interpolated like any coordinate).  A segment between
 * two waypoints is walked in `substeps` steps, N = (waypoints - 1) substeps + 1
 * samples per path:
 *   sample 0                waypoint 0
 *   sample j substeps + i   1 <= i <= substeps, on segment j: waypoint j + 1
 *                           itself for i == substeps, otherwise
 *                           qa + t (qb - qa), t = double(i) / double(substeps),
 *                           the difference, the product and the sum each
 *                           rounded once: numpy's qa + (i / substeps) * (qb - qa).
 * d_n, pair_n: the distance stage at sample n, bit for bit dist[0] and pair of
 * drc_qpik_stages_batch at that state (the refined distance; hulls and
 * obstacle slots included).  They depend on no drc_qpik_params field and not
 * on qdot, so the entry takes neither.  The rule:
 *   1. d_min = +inf, sample_min = pair_min = -1.
 *   2. For n = 0 .. N - 1 in order:
 *        d_n NaN:        result = DRC_CLEAR_INVALID, sample_stop = n, stop;
 *        d_n < d_min:    (d_min, sample_min, pair_min) = (d_n, n, pair_n) -- strict:
 *                        the lowest sample wins a tie;
 *        d_n < d_stop:   result = DRC_CLEAR_BLOCKED, sample_stop = n, stop.
 *   3. After the last sample: DRC_CLEAR_FREE, sample_stop = -1.
 * d_stop = -INFINITY never blocks and gives the whole profile.  dist_traj
 * [N][B] (may be NULL) receives d_n of the samples evaluated and is left
 * untouched after a stop; the last clear sample is sample_stop - 1.  Samples
 * past a stop are not evaluated: a path costs the samples it needs.
 * One persistent kernel, one path per wave, for every model (no QP shape is
 * involved); asynchronous on `stream`, no host synchronisation.
 * DRC_ERR_INVALID_ARGUMENT: waypoints < 1, substeps < 1, d_stop NaN, N not
 * below 2^31, B negative or above the work-queue limit, q_path or one of result
 * / sample_stop / d_min / sample_min / pair_min NULL, a model with obstacle
 * slots (drc_clearance_path_obstacles_batch takes their poses).  B = 0:
 * DRC_OK, nothing is touched. */
enum {
    DRC_CLEAR_FREE = 0,          /* no sample below d_stop                              */
    DRC_CLEAR_BLOCKED = 1,       /* sample_stop is the first sample with d < d_stop     */
    DRC_CLEAR_INVALID = 2        /* the distance at sample_stop is NaN                  */
};
int drc_clearance_path_batch(const drc_model* model, int64_t B, int waypoints, int substeps,
                             double d_stop, const double* q_path,
                             int32_t* result, int32_t* sample_stop,
                             double* d_min, int32_t* sample_min, int32_t* pair_min,
                             double* dist_traj, void* stream);

/* drc_clearance_path_batch on a model with obstacle slots.  The slots are
 * static for the call: obstacle_pose [n][12][obstacle_ld], obstacle_ld = 0 one
 * scene for every path, obstacle_ld >= B one scene per path (column b); in the
 * world frame for mobile manipulators.  DRC_ERR_INVALID_ARGUMENT on a model
 * without slots (drc_clearance_path_batch runs it). */
int drc_clearance_path_obstacles_batch(const drc_model* model, int64_t B, int waypoints,
                                       int substeps, double d_stop, const double* q_path,
                                       const double* obstacle_pose, int64_t obstacle_ld,
                                       int32_t* result, int32_t* sample_stop,
                                       double* d_min, int32_t* sample_min, int32_t* pair_min,
                                       double* dist_traj, void* stream);

/* Host-buffer form of drc_clearance_path_batch: every array is a HOST array,
 * staged in one round trip like drc_qpik_host.  dist_traj comes back whole: the
 * entries past a stop hold what the caller's array held. */
int drc_clearance_path_host(drc_model* model, int64_t B, int waypoints, int substeps,
                            double d_stop, const double* q_path,
                            int32_t* result, int32_t* sample_stop,
                            double* d_min, int32_t* sample_min, int32_t* pair_min,
                            double* dist_traj);

/* ---- certified path clearance: the continuous check of joint-space paths ------
 * drc_clearance_path_batch's FREE speaks of its samples.  This entry's FREE
 * speaks of the motion: every state of every straight segment between
 * consecutive waypoints of q_path [waypoints][dof][B] has d >= d_lower >=
 * d_stop.  It evaluates the distance stage where the path is close to
 * something and nowhere else (adaptive bisection, after Schwarzer, Saha and
 * Latombe); d and pair at a state are bit for bit dist[0] and pair of
 * drc_qpik_stages_batch, as for drc_clearance_path_batch.
 *
 * The model's motion weights (drc_model_motion_weights) bound how far a pair's
 * two geometries move against each other per unit of joint motion; the signed
 * distance of two convex bodies is 1-Lipschitz in that motion, on both sides of
 * contact.  Per segment j (waypoint j -> j + 1, ends qa, qb):
 *   M_j = max over the pairs p of  sum_{i = 1 .. dof} Wt[i][p] |qb_i - qa_i|,
 * the sum in ascending i, the difference, each product and each sum rounded
 * once, the max exact.  Positions on a segment are t = k / 2^e, e <= max_depth;
 * the state there is that of sample k of drc_clearance_path_batch with
 * substeps = 2^e (waypoint j + 1 itself at t = 1, waypoint j at t = 0).
 * The walk, left to right and depth first:
 *   1. d_min = d_lower = +inf, seg_min = pair_min = seg_stop = -1,
 *      t_min = t_stop = -1, samples_used = 0.  Waypoint 0 is evaluated
 *      (segment 0, t = 0).  A path of one waypoint ends here, FREE.
 *   2. Start of segment j: if a coordinate k of travel_mask has
 *      !(max(|qa_k|, |qb_k|) <= travel_k): DRC_CLEAR_UNDECIDED,
 *      (seg_stop, t_stop) = (j, 0), stop.  Then t = 1 is evaluated; t = 0 is
 *      the previous segment's end.
 *   3. Every evaluated sample (d, pair) at (j, t) counts in samples_used, then
 *        d NaN:       DRC_CLEAR_INVALID, (seg_stop, t_stop) = (j, t), stop;
 *        d < d_min:   (d_min, seg_min, t_min, pair_min) = (d, j, t, pair) --
 *                     strict: the first evaluated wins a tie;
 *        d < d_stop:  DRC_CLEAR_BLOCKED, (seg_stop, t_stop) = (j, t), stop.
 *   4. Interval [t0, t1] at depth e (t1 - t0 = 2^-e), end distances d0, d1:
 *        lb = 0.5 (d0 + d1) - (0.5 (t1 - t0)) M_j, each operation rounded;
 *        lb >= d_stop:    certified: d_lower = min(d_lower, lb), on to the
 *                         next pending interval;
 *        e == max_depth:  DRC_CLEAR_UNDECIDED, (seg_stop, t_stop) = (j, t0), stop;
 *        otherwise the midpoint is evaluated, then the left half is treated,
 *        then the right half.
 *   5. After the last segment: DRC_CLEAR_FREE.
 * d_stop = -INFINITY certifies every interval at depth 0; +INFINITY blocks at
 * the first sample that is not +inf.  max_depth is 0 .. DRC_CERTIFY_MAX_DEPTH;
 * a path takes at most (waypoints - 1) 2^max_depth + 1 evaluations, which must
 * stay below 2^31.  motion_bound [waypoints - 1][B] (may be NULL) receives M_j
 * of the segments that were started.
 * What is certified is the model the distance stage sees: hull models are
 * certified against their hulls, and the 256-vertex cap is an inner
 * approximation whose residual drc_model_geom_info reports.  A penetration
 * depth (d < 0) carries EPA's 1e-6; a separated distance the stage's 1e-9.
 * The bound uses the path's minimum distance with the largest pair weight,
 * which is conservative; obstacle slots are static for the call.
 * One persistent kernel, one path per wave, asynchronous on `stream`.
 * DRC_ERR_INVALID_ARGUMENT: as drc_clearance_path_batch (waypoints < 1, d_stop
 * NaN, B, a NULL among q_path and the outputs other than motion_bound, a model
 * with slots), max_depth outside its range, too many evaluations.
 * DRC_ERR_UNSUPPORTED: a prismatic joint of travel_mask has no finite limit.
 * B = 0: DRC_OK, nothing is touched. */
enum {
    DRC_CLEAR_UNDECIDED = 3,     /* not certified within max_depth, or out of the travel */
    DRC_CERTIFY_MAX_DEPTH = 20
};
int drc_clearance_certify_batch(const drc_model* model, int64_t B, int waypoints, double d_stop,
                                int max_depth, const double* q_path,
                                int32_t* result, int32_t* seg_stop, double* t_stop,
                                double* d_min, int32_t* seg_min, double* t_min, int32_t* pair_min,
                                double* d_lower, int32_t* samples_used, double* motion_bound,
                                void* stream);

/* drc_clearance_certify_batch on a model with obstacle slots: obstacle_pose and
 * obstacle_ld as for drc_clearance_path_obstacles_batch.  A pair with a slot
 * weighs the robot's side only.  DRC_ERR_INVALID_ARGUMENT on a model without
 * slots (drc_clearance_certify_batch runs it). */
int drc_clearance_certify_obstacles_batch(const drc_model* model, int64_t B, int waypoints,
                                          double d_stop, int max_depth, const double* q_path,
                                          const double* obstacle_pose, int64_t obstacle_ld,
                                          int32_t* result, int32_t* seg_stop, double* t_stop,
                                          double* d_min, int32_t* seg_min, double* t_min,
                                          int32_t* pair_min, double* d_lower,
                                          int32_t* samples_used, double* motion_bound,
                                          void* stream);

/* The motion weights behind drc_clearance_certify_batch (host only).
 *   rad_g      bounding radius of geometry g about its own frame origin:
 *              sphere r, cylinder sqrt(r^2 + (h/2)^2), box and hull the norm
 *              of the half extents
 *   travel_k   max(|lower_k|, |upper_k|) of a prismatic joint k
 *   rho [dof][n_geoms]   rho[j][g], for a joint j that supports the joint c
 *              carrying g: the sum of |p(placement of k)| (+ travel_k, k
 *              prismatic) over the joints k strictly below j down to c, plus
 *              |p(placement of g)| + rad_g -- no point of g is ever farther
 *              from the origin of j's frame; 0 for every other j, and for
 *              geometries that no joint moves (fixed links, obstacle slots)
 *   wt [dof][n_pairs]    wt[j][p] = 0 if j supports both geometries of pair p
 *              or neither; otherwise 1 (j prismatic) or rho[j][the supported
 *              geometry] (j revolute)
 *   *travel_mask  bit k - 1 set for each prismatic joint k that has a revolute
 *              joint above it and geometry below: the weights hold while
 *              |q_k| <= travel_k
 * Outputs may be NULL. */
int drc_model_motion_weights(const drc_model* model, double* rho, double* wt,
                             uint32_t* travel_mask);

/* Host-buffer forms of drc_qpik_batch / drc_qpik_stages_batch: same
 * arguments, but every array is a HOST array ([field][B], row stride B).  The
 * call stages them through model-owned device memory on an internal stream
 * and returns when the outputs are back on the host (PCIe-inclusive).  Calls
 * on one model are serialised.  Used by the C++ facade (include/drc_amd.hpp)
 * for the reference's single-robot signatures (B = 1). */
int drc_qpik_host(drc_model* model, const drc_qpik_params* params, int64_t B,
                  const double* q, const double* qdot, const double* x_target,
                  const double* xdot_target, const double* x_init, const double* xdot_init,
                  double* qdot_out, int32_t* status, int32_t* iters);
int drc_qpik_stages_host(drc_model* model, const drc_qpik_params* params, int64_t B,
                         const double* q, const double* qdot, const double* x_target,
                         const double* xdot_target, const double* x_init,
                         const double* xdot_init, double* pose, double* jac, double* man,
                         double* dist, int32_t* pair, double* xdot_des);

/* QP::TimeDuration (include/dyros_robot_controller/QP_base.h:19-43): seconds
 * per stage of one solve, as QPBase::solveQP fills it (:100-174). */
typedef struct drc_time_duration {
    double set_qp;          /* set_cost + set_bound + set_ineq + set_eq + set_constraint */
    double set_cost, set_bound, set_ineq, set_eq, set_constraint;
    double set_solver;      /* OSQP setup + solve (QP_base.h:143-170) */
    double solve_qp;        /* getSolution (:172-174) */
} drc_time_duration;

/* drc_qpik_host with QP::TimeDuration filled from per-instance stage stamps
 * the kernels write (s_memrealtime, averaged over the B instances):
 *   set_ineq       the task stage: FK, J, manipulability and its gradient, min
 *                  self-distance and its gradient (what setCost / setIneqConstraint
 *                  query, QP_IK.cpp:69-131, done in one pass);
 *   set_constraint assembly of P, q, bounds and the CBF rows (QP_base.h:202-227);
 *   set_cost, set_bound, set_eq  0 (assembled in the passes above);
 *   set_qp         set_ineq + set_constraint;
 *   set_solver     Ruiz scaling, factorisation, ADMM and the certified polish;
 *   solve_qp       the output store plus the call's launch / transfer /
 *                  synchronisation time outside the instance.
 * Reference behaviour on failure (QP_IK.cpp:56-61, time_status.setZero()) is
 * the caller's: the C++ facade's QPIK::getOptJointVel zeroes it. */
int drc_qpik_host_timed(drc_model* model, const drc_qpik_params* params, int64_t B,
                        const double* q, const double* qdot, const double* x_target,
                        const double* xdot_target, const double* x_init, const double* xdot_init,
                        double* qdot_out, int32_t* status, int32_t* iters, drc_time_duration* time_status);

/* ---- per-cycle kinematics and robot state -----------
 * drc_kinematics_batch: getPose / getJacobian / getVelocity of one frame for B
 * robots (Manipulator::RobotData, src/manipulator/robot_data.cpp:378-422; the
 * pose at the current q) without the manipulability and
 * self-collision stages the QPIK path adds: pose [12][B], jac [6*dof][B]
 * row-major, xdot [6][B] = J qdot.  Any output may be NULL; qdot may be NULL
 * when xdot is.  frame_id from drc_model_find_frame (-1: the last joint).
 * Asynchronous on `stream`. */
int drc_kinematics_batch(const drc_model* model, int frame_id, int64_t B, const double* q,
                         const double* qdot, double* pose, double* jac, double* xdot, void* stream);
/* One control cycle's robot state for host arrays in ONE round trip: the
 * frame's pose / J / J qdot (drc_kinematics_batch) and updateDynamics' M,
 * M_inv, g, nle, c ([n*n][B], [n][B] as drc_dynamics_batch, actuated = 0) --
 * what RobotData::updateState caches and the cycle's getPose / getVelocity /
 * getJacobian / moveJointTorqueStep read (robot_data.cpp:91-124,378-422,
 * robot_controller.cpp:115-125).  The inputs go over in one transfer and the
 * outputs come back in one; any output may be NULL.  Synchronous. */
int drc_state_host(drc_model* model, int frame_id, int64_t B, const double* q, const double* qdot,
                   double* pose, double* jac, double* xdot, double* M, double* M_inv, double* g,
                   double* nle, double* c);

/* Concurrency of drc_qpik_batch: the batch is split into up to `chunks`
 * contiguous sub-batches (each >= 4096 instances, >= 16384 when there are 4)
 * that run concurrently: the last on the caller's stream, the others on
 * internal streams forked from and joined back to it (default 4: 4 streams,
 * HIP's default hardware queues per process).  Results do not depend on it. */
int drc_set_concurrency(drc_model* model, int chunks);

/* Fused task + QP kernel for the QP shapes the library compiles (the bundled
 * FR3, UR5e, Husky-FR3, XLS-FR3 layouts) and batches of up to 16 384
 * instances (the DRC_FUSE_MAX environment variable overrides): 1 (default)
 * runs such a drc_qpik_batch call as one kernel whose
 * waves take an instance through the task stage and the QP before the next,
 * the task record kept in LDS; 0 always runs the task-kernel -> QP-kernel
 * pipeline (drc_set_concurrency sub-batches), as larger batches do.  Results
 * are bit-identical either way (the library is built with -ffp-contract=on:
 * every multiply-add rounds the same in both kernels), so an instance's
 * result depends neither on the batch size nor on this switch. */
int drc_set_fusion(drc_model* model, int enable);

/* Frees the per-stream scratch (task-record pool, work-queue counters) the
 * model keeps for `stream`, after the stream's queued work has finished; call
 * it before destroying a stream the model was used on.  A model keeps at most
 * 8 such contexts in any case (the least recently used one is freed when a
 * ninth stream appears), so a caller cycling through streams cannot grow it
 * without bound.  No-op for a stream the model has not seen.  (Reference: no
 * counterpart — the reference's OSQP solver object is per controller.) */
int drc_model_release_stream(drc_model* model, void* stream);

const char* drc_error_string(int code);
/* Identity of this library build: a hash of its sources and compile flags
 * (build.sh).  Profiles measured on a build carry its id, so a counter
 * summary is only ever attributed to the build it came from.  (Reference: no
 * counterpart.) */
const char* drc_build_id(void);
/* Thread-local detail of the last failing call (parse position, HIP error). */
const char* drc_last_error(void);

/* ---- joint-space dynamics --------------------
 * drc_dynamics_batch: for B robots, the quantities RobotData::updateState caches
 * after updateDynamics:
 *   actuated = 0:  Manipulator::RobotData::updateDynamics (src/manipulator/robot_data.cpp:109-124)
 *                  M = crba (symmetric), M_inv = DyrosMath::PinvCOD(M), g = computeGeneralizedGravity,
 *                  nle = nonLinearEffects, c = nle - g;  n = dof.  Getters getMassMatrix / getMassMatrixInv /
 *                  getGravity / getNonlinearEffects / getCoriolis (robot_data.h:176-198); computeMassMatrix /
 *                  computeGravity / computeCoriolis / computeNonlinearEffects (robot_data.h:70-92) are the
 *                  same call with the fields they return.
 *   actuated = 1:  MobileManipulator::RobotData::updateDynamics (src/mobile_manipulator/robot_data.cpp:126-144)
 *                  S^T M S, PinvCOD(S^T M S), S^T g, S^T nle, S^T (nle - g) with the selection matrix of
 *                  robot_data.cpp:22-25,115-120;  n = actuated dof.  (getMassMatrixActuated etc.,
 *                  mobile_manipulator/robot_data.h:425-445; compute*Actuated :151-187.)
 * q, qdot: [dof][B] full joint vectors (JointIndex order for mobile manipulators); qdot may be NULL when
 * nle and c are NULL (treated as zero).  Outputs, any of which may be NULL: M, M_inv [n*n][B] (entry (i,j) at
 * field i*n + j), g, nle, c [n][B].  Gravity is Pinocchio's default (0, 0, -9.81).  Asynchronous on `stream`;
 * a second, usually empty, launch re-solves M_inv by a serial COD where the kernel cannot certify full rank. */
int drc_dynamics_batch(drc_model* model, int actuated, int64_t B, const double* q, const double* qdot,
                       double* M, double* M_inv, double* g, double* nle, double* c, void* stream);
/* Same contract with HOST buffers; synchronous (PCIe-inclusive). */
int drc_dynamics_host(drc_model* model, int actuated, int64_t B, const double* q, const double* qdot,
                      double* M, double* M_inv, double* g, double* nle, double* c);

/* ---- joint torque step ------------------------
 * Manipulator::RobotController::moveJointTorqueStep (src/manipulator/robot_controller.cpp:115-125) for B
 * robots, computing M and g in the same launch (robot_data.cpp:111-112):
 *   tau = M qddot_target + g                                     when qddot_target != NULL
 *   tau = M (kp .* (q_target - q) + kv .* (qdot_target - qdot)) + g   otherwise,
 * with q_target == NULL meaning q + dt * qdot_target: the Euler step that follows QPIK in the reference's
 * FR3 control loop (examples/C++/src/fr3_controller.cpp:132-134), so
 *   drc_qpik_batch(...qdot_out...) ; drc_joint_torque_step_batch(..., NULL, qdot_out, NULL, dt, ...)
 * is that whole cycle on the device.  Mobile manipulators: the arm block, as
 * MobileManipulator::RobotController::moveManipulatorJointTorqueStep (mobile_manipulator/robot_controller.cpp:103-118).
 * q, qdot: [dof][B]; q_target, qdot_target, qddot_target, tau: [nb][B] with nb = dof (manipulator) or the arm
 * dof (mobile manipulator).  kp, kv: HOST arrays [nb] or NULL for the reference defaults 400 / 40
 * (robot_controller.cpp:14-15). */
int drc_joint_torque_step_batch(drc_model* model, int64_t B, const double* q, const double* qdot,
                                const double* q_target, const double* qdot_target, const double* qddot_target,
                                double dt, const double* kp, const double* kv, double* tau, void* stream);
/* Same contract with HOST buffers; synchronous. */
int drc_joint_torque_step_host(drc_model* model, int64_t B, const double* q, const double* qdot,
                               const double* q_target, const double* qdot_target, const double* qddot_target,
                               double dt, const double* kp, const double* kv, double* tau);

/* ---- QPID: the torque-level QP ----------------------
 * Manipulator::RobotController::QPID / QPIDStep / QPIDCubic (src/manipulator/robot_controller.cpp:319-361) over
 * Manipulator::QPID (src/manipulator/QP_ID.cpp:7-193), and the MobileManipulator twins
 * (src/mobile_manipulator/robot_controller.cpp:199-250, QP_ID.cpp:7-184), for B robots.  Same params struct
 * as QPIK: mode DRC_MODE_QPID* (0 = QPID(xddot_target) with the task acceleration in xdot_target,
 * 1 = QPIDStep, 2 = QPIDCubic), kp/kv the task gains (defaults 100/20, MoMa 400/40).  Per call: M and g of the
 * equality rows are computed on the device (drc_dynamics_batch's kernel), then the QPID stage data (frame
 * Jacobian time variation, grad_dot terms of the singularity and self-collision CBF rows) and the QP.
 *   qddot_out [na][B]: qddot (manipulator) / eta_dot in ActuatorIndex order (MoMa);
 *   tau_out   [na][B]: joint torques / actuated torques;
 *   status [B], iters [B] (may be NULL).
 * Non-Solved: qddot = 0, tau = getGravity() (robot_controller.cpp:333-336); MoMa: tau[i] = the joint-order
 * getGravity()[i] — the reference slices that vector at ActuatorIndex offsets (mobile_manipulator/
 * robot_controller.cpp:211,218), restated as written. */
enum { DRC_MODE_QPID = 0, DRC_MODE_QPID_STEP = 1, DRC_MODE_QPID_CUBIC = 2 };
int drc_default_qpid_params(const drc_model* model, int exact, drc_qpik_params* params);
int drc_qpid_batch(const drc_model* model, const drc_qpik_params* params, int64_t B,
                   const double* q, const double* qdot, const double* x_target,
                   const double* xdot_target, const double* x_init, const double* xdot_init,
                   double* qddot_out, double* tau_out, int32_t* status, int32_t* iters, void* stream);
/* Stage outputs of the QPID task stage: as drc_qpik_stages_batch (xddot_des = the QP's task
 * acceleration), plus jdot [6*dof][B] (getJacobianTimeVariation, LWA, robot_data.cpp:404-417),
 * qpid_terms [8][B] = (Jdot v (6) with v = qdot or S eta, grad_dot_m . qdot_arm, grad_dot_d . qdot_arm) and
 * graddot [mani + dof][B] = the grad_dot vectors of getManipulability(true, true) (robot_data.cpp:555-569;
 * MoMa :477-492) and getMinDistance(true, true) (:496-512).  Any output may be NULL. */
int drc_qpid_stages_batch(const drc_model* model, const drc_qpik_params* params, int64_t B,
                          const double* q, const double* qdot, const double* x_target,
                          const double* xdot_target, const double* x_init, const double* xdot_init,
                          double* pose, double* jac, double* man, double* dist, int32_t* pair,
                          double* xddot_des, double* jdot, double* qpid_terms, double* graddot, void* stream);
int drc_qpid_stages_host(drc_model* model, const drc_qpik_params* params, int64_t B,
                         const double* q, const double* qdot, const double* x_target,
                         const double* xdot_target, const double* x_init, const double* xdot_init,
                         double* pose, double* jac, double* man, double* dist, int32_t* pair,
                         double* xddot_des, double* jdot, double* qpid_terms, double* graddot);
/* Host-buffer form of drc_qpid_batch (synchronous, PCIe-inclusive). */
int drc_qpid_host(drc_model* model, const drc_qpik_params* params, int64_t B,
                  const double* q, const double* qdot, const double* x_target,
                  const double* xdot_target, const double* x_init, const double* xdot_init,
                  double* qddot_out, double* tau_out, int32_t* status, int32_t* iters);

/* ---- closed-form controllers -------------------------
 * Manipulator::RobotController::CLIKStep / CLIKCubic (src/manipulator/robot_controller.cpp:156-214):
 *   qdot = J^+ (Kp e + xdot_target) + (I - J^+ J) null_qdot,  J^+ = DyrosMath::PinvCOD(J);
 *   params->mode DRC_MODE_QPIK_STEP (1) or DRC_MODE_QPIK_CUBIC (2); kp = Kp_task_ (kv is not used).
 * Manipulator::RobotController::OSF / OSFStep / OSFCubic (:216-275):
 *   Lambda = PinvCOD(J M^-1 J^T), tau = J^T Lambda xddot + (I - J^T Lambda J M^-1) null_torque + g,
 *   xddot = xdot_target (mode 0, OSF(xddot_target)) or Kp e + Kv (xdot_target - J qdot) (modes 1, 2);
 *   M^-1 = getMassMatrixInv, g = getGravity computed on the device in the same call.
 * Manipulator models only.  q, qdot [dof][B]; x_target [12][B]; xdot_target [6][B]; x_init/xdot_init for the
 * cubic forms; null_qdot / null_torque [dof][B] or NULL (the overloads without them); out [dof][B].
 * Parameters: drc_default_qpik_params (Kp_task_ = 100, Kv_task_ = 20). */
int drc_clik_batch(const drc_model* model, const drc_qpik_params* params, int64_t B, const double* q,
                   const double* qdot, const double* x_target, const double* xdot_target, const double* x_init,
                   const double* xdot_init, const double* null_qdot, double* qdot_out, void* stream);
int drc_osf_batch(const drc_model* model, const drc_qpik_params* params, int64_t B, const double* q,
                  const double* qdot, const double* x_target, const double* xdot_target, const double* x_init,
                  const double* xdot_init, const double* null_torque, double* tau_out, void* stream);
/* Host-buffer form of both (kind 1 = CLIK, 2 = OSF); synchronous. */
int drc_closed_form_host(drc_model* model, const drc_qpik_params* params, int kind, int64_t B, const double* q,
                         const double* qdot, const double* x_target, const double* xdot_target,
                         const double* x_init, const double* xdot_init, const double* null_vec, double* out);

#ifdef __cplusplus
}
#endif
#endif /* DRC_AMD_H */
