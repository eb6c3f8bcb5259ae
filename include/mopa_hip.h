/*
 * mopa_hip.h -- C ABI of libmopa_hip.so, the MI355X (gfx950) implementation of
 * MoPA-RL's state-validity / motion-validation / RRT-Connect hot path.
 *
 * This is the drop-in boundary: each entry point below replaces one piece of
 * what the reference's Cython extension binds (reference
 * motion_planners/planner.pyx:9-52 -> motion_planners/include/KinematicPlanner.h:40-71).
 * Plain pointers and sizes only; no C++ types, no exceptions: every function
 * returns an int status (0 = MOPA_OK) and mopa_last_error() explains failures.
 *
 *   reference interface                              replaced by
 *   -----------------------------------------------  ----------------------------
 *   KinematicPlanner::KinematicPlanner(xml, algo,    mopa_scene_create()
 *     ..., passive_joint_idx, glue_bodies,           (the XML is compiled to the
 *     ignored_contacts, contact_threshold, ...)      flat MopaModel by the host
 *     KinematicPlanner.cpp:42-120                    shim: mopa_rl_amd/mjcf.py)
 *   KinematicPlanner::~KinematicPlanner              mopa_scene_destroy()
 *   KinematicPlanner::isValidState(vector<double>)   mopa_is_valid_state()      (1 state, host ptr)
 *     KinematicPlanner.cpp:253-286 ->                mopa_is_valid_batch()      (N states, device ptrs)
 *     MujocoStateValidityChecker::isValid
 *     mujoco_ompl_interface.cpp:909-978
 *   si->checkMotion (OMPL DiscreteMotionValidator,   mopa_check_motion_batch()
 *     resolution KinematicPlanner.cpp:87)
 *   ... its overload checkMotion(s1, s2, lastValid)  mopa_motion_report_batch() (N segments, device ptrs)
 *     (not called by the reference) + the blockers   mopa_motion_report()       (1 segment, host ptrs)
 *   KinematicPlanner::plan(start, goal, timelimit)   mopa_plan()                (1 query, host ptrs)
 *     KinematicPlanner.cpp:125-251 (RRTConnect)      mopa_plan_batch()          (E queries, device ptrs)
 *   invalid-target back-off of the rollout runner    mopa_pullback_batch()      (E targets, device ptrs)
 *     rl/mopa_rollouts.py:133-143
 *   KinematicPlanner::getPlannerStatus()             mopa_planner_status()
 *     KinematicPlanner.cpp:288-291
 *
 * Memory: "dev" pointers are HIP device pointers (e.g. torch tensor
 * data_ptr() on a ROCm device), "host" pointers are ordinary memory.  The
 * caller owns every buffer; the library never frees caller memory.  All
 * floating point data is IEEE double, C-contiguous.  `stream` is a
 * hipStream_t passed as void* (NULL = the default stream); batch calls are
 * asynchronous on that stream.  Streams: a scene keeps its launch scratch per
 * stream, so calls on DIFFERENT streams may be in flight at the same time (e.g.
 * validity on one stream while the planner runs on another); calls on the same
 * stream are ordered by the stream.  Host threads: one at a time per object for
 * the single-query forms (they share a staging buffer); the batch forms may be
 * called from several threads as long as each uses its own stream.  Devices:
 * every entry point runs on its object's device and restores the caller's
 * current device before returning.
 */
#ifndef MOPA_HIP_H
#define MOPA_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MOPA_OK 0
#define MOPA_ERR_INVALID_ARG 1
#define MOPA_ERR_UNSUPPORTED 2   /* e.g. ellipsoid / height-field geom, ball joint in the model */
#define MOPA_ERR_HIP 3           /* HIP runtime error (no device, launch failure...) */
#define MOPA_ERR_LIMIT 4         /* model exceeds a compile-time capacity */

/* planner result codes == the sentinel rows of KinematicPlanner.cpp:181-184,249-250 */
#define MOPA_PLAN_OK 0
#define MOPA_PLAN_NO_EXACT (-4)
#define MOPA_PLAN_INVALID_GOAL (-5)

/* "culled / ignored / no intersection found" value of mopa_debug_pair_dist outputs */
#define MOPA_FAR 1.0e10

/* geom / joint type codes (MuJoCo's mjtGeom / mjtJoint values) */
enum { MOPA_GEOM_PLANE = 0, MOPA_GEOM_SPHERE = 2, MOPA_GEOM_CAPSULE = 3, MOPA_GEOM_CYLINDER = 5, MOPA_GEOM_BOX = 6, MOPA_GEOM_MESH = 7 };
enum { MOPA_JNT_FREE = 0, MOPA_JNT_BALL = 1, MOPA_JNT_SLIDE = 2, MOPA_JNT_HINGE = 3 };

/* Flat compiled model (host pointers; copied by mopa_scene_create).
 * Same arrays as mopa_rl_amd.mjcf.CompiledModel.
 *
 * Preconditions -- what MuJoCo's compiler emits; every entry point that compiles a model (mopa_scene_create, _create_glued,
 * mopa_scene_k1_export, _export_glued; mopa_env_create, mopa_ik_create and their host halves mopa_env_tables_host, mopa_ik_tables_host,
 * mopa_dyn_tables_host: the body, joint and geom_body rules) checks them before anything indexes with these values and refuses a
 * model that breaks one:
 *   - body 0 is the world; 0 <= body_parent[b] < b for b >= 1                                    (MOPA_ERR_INVALID_ARG)
 *   - the bodies are in depth-first order: body_parent[b] is body b - 1 or one of its ancestors  (MOPA_ERR_UNSUPPORTED; a breadth-
 *     first numbering of a branching tree is refused, not compiled: the pose save slots of the FK program are numbered by depth)
 *   - body_jntnum[b] >= 0, and the joints body_jntadr[b] .. + body_jntnum[b] lie in [0, njnt)     (MOPA_ERR_INVALID_ARG)
 *   - jnt_type is one of MOPA_JNT_*; jnt_qposadr[j] and the slots behind it (7 of a free joint, 4 of a ball joint, 1 otherwise) lie
 *     in [0, nq)                                                                                  (MOPA_ERR_INVALID_ARG)
 *   - 0 <= geom_body[g] < nbody; the geoms are in body order; a mesh geom's geom_dataid names a mesh whose vertices lie in
 *     [0, nmeshvert)                                                                              (MOPA_ERR_INVALID_ARG / _UNSUPPORTED)
 *   - a candidate pair names two different geoms in [0, ngeom), at least one of them on a body that a joint moves
 *                                                                                                 (MOPA_ERR_INVALID_ARG)
 * Capacities (MOPA_ERR_LIMIT): 255 collidable geoms, 64 of them moving, 65535 candidate pairs.  Unit quaternions and unit joint axes are
 * the caller's responsibility. */
typedef struct MopaModel {
    int32_t nq, nbody, njnt, ngeom, npair;
    const int32_t *body_parent;   /* [nbody]            */
    const double  *body_pos;      /* [nbody,3]          */
    const double  *body_quat;     /* [nbody,4] wxyz, normalised */
    const int32_t *body_jntadr;   /* [nbody] first joint or -1 */
    const int32_t *body_jntnum;   /* [nbody]            */
    const int32_t *jnt_type;      /* [njnt]             */
    const int32_t *jnt_qposadr;   /* [njnt]             */
    const double  *jnt_axis;      /* [njnt,3] normalised */
    const double  *jnt_pos;       /* [njnt,3]           */
    const double  *jnt_ref;       /* [njnt] qpos0 of hinge/slide */
    const int32_t *jnt_limited;   /* [njnt]             */
    const double  *jnt_range;     /* [njnt,2]           */
    const int32_t *geom_type;     /* [ngeom] collidable geoms only */
    const int32_t *geom_body;     /* [ngeom]            */
    const int32_t *geom_mjid;     /* [ngeom] id among ALL geoms of the model (for ignored_contacts) */
    const double  *geom_size;     /* [ngeom,3]          */
    const double  *geom_pos;      /* [ngeom,3]          */
    const double  *geom_quat;     /* [ngeom,4]          */
    const int32_t *pair_geom;     /* [npair,2] candidate pairs after MuJoCo's static filters, type1<=type2 */
    /* convex hulls of mesh geoms (MuJoCo collides a mesh geom through the convex hull of its vertices):
     * vertices in the geom frame.  nmesh == 0 / NULL pointers for models without collidable meshes. */
    int32_t nmesh, nmeshvert;
    const int32_t *mesh_vertadr;  /* [nmesh] first vertex */
    const int32_t *mesh_vertnum;  /* [nmesh] */
    const double  *mesh_vert;     /* [nmeshvert,3] */
    const int32_t *geom_dataid;   /* [ngeom] mesh id of a MOPA_GEOM_MESH geom, -1 otherwise (may be NULL when nmesh == 0) */
} MopaModel;

/* Everything KinematicPlanner's constructor receives (KinematicPlanner.cpp:42-61). */
typedef struct MopaSceneDesc {
    MopaModel model;
    int32_t n_passive;
    const int32_t *passive_qpos_idx;   /* [n_passive] qpos addresses NOT planned over */
    int32_t n_ignored;
    const int32_t *ignored_pairs;      /* [n_ignored,2] ordered (lo,hi) MuJoCo geom ids */
    double contact_threshold;          /* state invalid iff some non-ignored dist <= this; must be <= 0 (negative in the
                                          reference); > 0 is rejected with MOPA_ERR_UNSUPPORTED: the broad phase culls at zero margin */
    double range;                      /* RRT-Connect maxDistance (KinematicPlanner.cpp:102-104) */
    double resolution;                 /* validity checking resolution; the reference hard-codes 0.005 (:87) */
    uint64_t seed;                     /* KinematicPlanner.cpp:95 */
    int32_t device;                    /* HIP device ordinal, -1 = current */
    const double *pair_cull_radius;    /* nullable, [model.npair]: > 0 = the pair can only reach contact_threshold while its two geom
                                          centres are within this distance (a compile-time bound, tools/prove_separated_pairs.py);
                                          the FP32 broad phase then culls with min(bounding-sphere sum, this).  0 = no bound */
} MopaSceneDesc;

typedef struct MopaScene MopaScene;

typedef struct MopaPlanParams {
    int32_t max_iters;     /* RRT-Connect iteration budget (replaces the wall-clock timelimit) */
    int32_t max_nodes;     /* per-tree node capacity */
    int32_t max_path;      /* rows available per env in `path` */
    uint64_t seed;         /* sample-stream seed; stream id = env_id_base + env index */
    uint64_t env_id_base;
    const uint64_t *env_ids_dev;   /* mopa_plan_batch only, nullable: explicit stream id per query (device pointer, [E]) --
                                      lets a caller plan for a compacted subset of its envs with the streams of the full set */
    const uint64_t *seeds_dev;     /* mopa_plan_batch only, nullable: explicit seed per query (device pointer, [E]) instead of
                                      `seed` -- queries of envs that are at different steps of their own rollouts in one launch */
    int32_t max_workgroups;        /* mopa_plan_batch only: persistent workgroups of the launch.  0 = one per CU (a lone launch ends
                                      with its slowest query, and two budget-exhausting queries on one SIMD slow each other down);
                                      < 0 = as many as the chip holds at once (two per CU: throughput, for launches that overlap
                                      others -- the iteration ladder); > 0 = an explicit cap (asynchronous rollouts leave the main
                                      stream's kernels room this way: a workgroup keeps ~70 KB of LDS while queries are left) */
    int32_t exclusive_cu;          /* mopa_plan_batch only: nonzero = the launch asks for more than half a CU's LDS, so that no other
                                      planner workgroup (of this or of an overlapping launch) shares its CUs -- for a burst of capped
                                      launches that together want one workgroup per CU.  Implied by max_workgroups == 0 */
    /* mopa_plan_batch only, all nullable (device pointers): continuing queries across launches.  A query's outcome is a
       function of its endpoints and sample stream only and the iteration budget merely ends the loop, so a launch with a
       small budget can leave its unsolved queries where a later launch with a larger budget picks them up -- the result is
       that of one launch with the larger budget, without retracing the first iterations (the iteration ladder).
       Saving: tree_q_dev [E][2][max_nodes][na] doubles (+ 8 of padding), tree_p_dev [E][2][max_nodes] int32 hold the trees
       instead of the library's scratch; state_dev [E][4] int64 receives (iterations done | -1 = "no exact solution"
       whatever the budget | -2 = settled: solved or invalid goal; start-tree size, goal-tree size, consumed checks).
       Continuing: resume_tree_q / resume_tree_p / resume_state = those buffers (rows gathered to this launch's query order,
       same max_nodes, same seeds / stream ids as the first launch); a query whose state says -2 is skipped, its outputs are
       not written -- so a launch's whole query list can be continued right behind it on the same stream, no host in between. */
    double *tree_q_dev;
    int32_t *tree_p_dev;
    int64_t *state_dev;
    const double *resume_tree_q;
    const int32_t *resume_tree_p;
    const int64_t *resume_state;
} MopaPlanParams;

const char *mopa_last_error(void);
const char *mopa_version(void);
/* number of visible HIP devices (0 when none); never fails */
int mopa_device_count(void);

int mopa_scene_create(const MopaSceneDesc *desc, MopaScene **out);
void mopa_scene_destroy(MopaScene *scene);

/* glue_bodies (KinematicPlanner's constructor argument; the reference: GlueTransformation, mujoco_ompl_interface.cpp:810-907): the
 * GLUED compile of the same description.  body_b (a model body id) carries exactly one free joint -- the manipulated object -- and is
 * posed as a jointless child of body_a, a body the active joints move (the gripper): for any active joint values
 *     p_b' = p_a' + R_a' t,   q_b' = normalize(q_a' * rq),
 * where the offset t = R(q_a)^T (p_b - p_a), rq = conj(q_a) * q_b is taken where forward kinematics leaves the two bodies at the
 * ATTACH row's own joint values.  This is the weld form of the reference's write-back form (it writes the world pose into the free
 * joint's qpos and runs FK again): the poses are equal up to rounding; on the CPU oracle the verdicts were equal on every state
 * compared, and min_dist equal except on 0.2 % of them, where the narrow phase's depth is not continuous in the pose (DESIGN.md
 * section 3).  The candidate pairs and ignored_pairs are the description's; the caller
 * ignores the object-gripper pairs, as with the reference.  desc->pair_cull_radius is not applied to pairs with a geom on body_b or
 * below it (the proofs behind it do not cover a carried object).  The FP32 broad phase's coordinate bound stays the caller's
 * responsibility for the offset, as it is for free-joint positions.
 * Which row attaches: mopa_is_valid_batch / mopa_check_motion_batch -- env row qpos_env[e], at its own active values, for every state
 * or segment of env e; mopa_plan_batch / mopa_plan -- the start row (the goal row's free-joint slots are not read), and in every row
 * of a solved path the 7 free-joint columns hold (p_b', q_b') at that waypoint; mopa_is_valid_state -- the state itself.  These
 * take ordinary qpos rows and attach internally, and so do mopa_debug_fk / mopa_debug_pair_dist (the state itself).  Every other
 * entry point that takes a scene and states (mopa_plan_star*, mopa_plan_race*, the K9 passes, mopa_pullback_batch, mopa_contacts_*,
 * mopa_interpolate_batch, the FK timing probe of the stats build) and the planner continuation of MopaPlanParams return
 * MOPA_ERR_UNSUPPORTED on a glued scene.  A glued scene runs the generic validity kernels (never a baked one).
 * Refused with MOPA_ERR_UNSUPPORTED: body_b without exactly one free joint (the reference's two-slide branch is not built), body_a
 * static, body_a >= body_b in body order, body_a inside body_b's subtree. */
int mopa_scene_create_glued(const MopaSceneDesc *desc, int32_t body_a, int32_t body_b, MopaScene **out);
/* out[0], out[1] = body_a, body_b of a glued scene; -1, -1 for an ordinary one */
int mopa_scene_glue(const MopaScene *scene, int32_t out[2]);
/* E qpos rows -> their ATTACHED rows: copies whose 7 free-joint slots of body_b hold the offset (t[3], rq[4]) at the row's own
 * joint values (k_glue_attach, one lane per row; not in place).  What the entry points above do internally. */
int mopa_glue_attach_batch(MopaScene *scene, const double *rows_dev /*[E,nq]*/, int64_t E, double *attached_dev /*[E,nq]*/, void *stream);
/* path rows in place: in rows r < min(path_len[e], max_path) of env e the 7 free-joint columns of body_b get (p_b', q_b') at the
 * row's active values, with the offset and the other passive values of attached_dev[e] (k_glue_rows, one lane per row) */
int mopa_glue_rows_batch(MopaScene *scene, double *path_dev /*[E,max_path,nq]*/, const int32_t *path_len_dev /*[E]*/,
                         const double *attached_dev /*[E,nq]*/, int64_t E, int32_t max_path, void *stream);
/* introspection used by the host shim and the tests */
int mopa_scene_num_active(const MopaScene *scene);
int mopa_scene_active_idx(const MopaScene *scene, int32_t *out /*[na]*/);
int mopa_scene_num_pairs(const MopaScene *scene);   /* non-ignored candidate pairs checked per state */
int mopa_scene_lds_bytes(const MopaScene *scene);
/* name of the validity kernel mopa_is_valid_batch dispatches for a batch of N states on this scene ("k_is_valid_v5",
 * "k_is_valid_v2" or "k_is_valid"); the benchmark labels its roofline line and selects profiler rows with it */
int mopa_scene_valid_kernel(const MopaScene *scene, int64_t N, char *out, int32_t cap /* >= 24 */);
/* the form mopa_check_motion_batch takes for N segments on this scene: "k_check_motion" (one wave per segment) or
 * "k_motion_expand" (the segments expanded into their states for the lane-per-state validity kernel) */
int mopa_scene_motion_kernel(const MopaScene *scene, int64_t N, char *out, int32_t cap /* >= 24 */);
/* k_is_valid_v5 on this scene: 0 = the generic instantiation, i > 0 = the i-th baked scene (mopa_valid_v5_baked.inc) */
int mopa_scene_k1_baked(const MopaScene *scene);
/* what the launch plan gives a batch of N states on the lane-per-state kernel k_is_valid_v5: *tiles_per_drain = 64-state tiles
 * a wave walks before one narrow-phase drain (1, or 2 for a pair-drain scene's verdict-only launch), *ent_cap = survivor entries
 * the wave's buffer holds (after the axis table and the second tile's words); both 0 when the batch goes to another kernel */
int mopa_scene_k1_drain_plan(const MopaScene *scene, int64_t N, int32_t want_min_dist, int32_t *tiles_per_drain, int32_t *ent_cap);
/* host-only export of what k_is_valid_v5 reads from a scene (no device needed; tools/bake_k1_scenes.py):
 * sizes[8] = n_dbl, n_int, n_tab, sizeof(SceneHdr), use_v5, centre table in LDS, mesh pairs, moving geoms;
 * dbl / ints / tab / hdr (nullable) receive the two blobs, the FP32 pair table and the header, *fingerprint (nullable)
 * the 64-bit FNV-1a hash over those bytes that selects a baked instantiation */
int mopa_scene_k1_export(const MopaSceneDesc *desc, int64_t *sizes /*[8]*/, double *dbl, int32_t *ints, int32_t *tab, void *hdr,
                         uint64_t *fingerprint);
/* byte offset of a field of the exported header (mopa_scene_k1_export's hdr) by name, -1 for an unknown name: the layout
 * tools/bake_k1_scenes.py reads the header with, taken from the compiler rather than restated */
int mopa_scene_hdr_offset(const char *field);
/* mopa_scene_k1_export of the glued compile (mopa_scene_create_glued's host half: its refusals are this call's status codes) */
int mopa_scene_k1_export_glued(const MopaSceneDesc *desc, int32_t body_a, int32_t body_b, int64_t *sizes /*[8]*/, double *dbl, int32_t *ints,
                               int32_t *tab, void *hdr, uint64_t *fingerprint);
/* host run of the forward kinematics compiled into the i-th baked scene (no device needed; tests): n states, state s =
 * q_active[s] (na values) over the env row qpos_env[s] (nq values); out[s][nmg][12] = each moving geom's world position
 * and row-major rotation matrix.  Returns MOPA_ERR_INVALID_ARG for an index that names no baked scene */
int mopa_k1_baked_fk_host(int index, int64_t n, const double *q_active, const double *qpos_env, double *out);
/* the kernel's walk is a sparse one (products with the scene's exact zeros and ones left out) guarded per state, with the dense walk
 * run over it when the guard's flag is up: mopa_k1_baked_fk_host is that production path.  mopa_k1_baked_fk_sparse_host: the sparse
 * walk alone, no re-run: out[s][nmg][7] = raw position and quaternion of each moving geom, tripped[s] = the guard's flag.
 * mopa_k1_baked_fk_pose_host: the same layout from the dense walk */
int mopa_k1_baked_fk_sparse_host(int index, int64_t n, const double *q_active, const double *qpos_env, double *out, uint8_t *tripped);
int mopa_k1_baked_fk_pose_host(int index, int64_t n, const double *q_active, const double *qpos_env, double *out);
/* the resident pairs of baked scene #index (pairs the baked walk evaluates in place), as the walk computes them on the host:
   out[n][n_res] distances in the order of the traits' list; *n_res (nullable) receives their number */
int mopa_k1_baked_resident_host(int index, int64_t n, const double *q_active, const double *qpos_env, double *out, int32_t *n_res);
/* the broad phase's test of the static non-plane partners of baked scene #index, per state, on the host: keep_new / keep_old
   [n][n_ent] (n_ent: entries of the FP32 pair table, returned through the nullable *n_ent) hold 1 / 0 for such an entry kept /
   culled under the built rule (per-axis reach of capsule and cylinder owners) and under the bounding-radius rule, 2 for every
   other entry; axis[n][nmg][3] (float): the |axis| magnitudes the kernel unpacks for those owners, -1 for the other geoms */
int mopa_k1_baked_static_host(int index, int64_t n, const double *q_active, const double *qpos_env, uint8_t *keep_new, uint8_t *keep_old,
                              float *axis, int32_t *n_ent);

/* N states: state i = qpos_env[i / samples_per_env] with its active entries replaced by q_active[i].
 * valid[i] = 1 iff no non-ignored pair has dist <= contact_threshold.
 * min_dist (nullable): deepest penetration = min(0, minimum signed distance over the non-ignored pairs), i.e. 0.0 for
 * a state in which nothing penetrates; requesting it disables the per-state early-out. */
int mopa_is_valid_batch(MopaScene *scene, const double *q_active_dev /*[N,na]*/, const double *qpos_env_dev /*[E,nq]*/,
                        int64_t N, int64_t samples_per_env, uint8_t *valid_dev /*[N]*/, double *min_dist_dev /*[N] or NULL*/,
                        void *stream);
/* The same with the number of states only known on the device: *n_dev <= N, N sizes the launch and the buffers; states from
 * *n_dev on are neither read nor written.  Needs a scene the lane-per-state kernel serves (MOPA_ERR_UNSUPPORTED otherwise). */
int mopa_is_valid_batch_counted(MopaScene *scene, const double *q_active_dev /*[N,na]*/, const double *qpos_env_dev /*[E,nq]*/,
                                int64_t N, int64_t samples_per_env, uint8_t *valid_dev /*[N]*/, double *min_dist_dev /*[N] or NULL*/,
                                const int64_t *n_dev, void *stream);

/* N segments qa[i] -> qb[i] (active coordinates), OMPL DiscreteMotionValidator semantics:
 * valid[i] = 1 iff qb[i] and every interior state interpolate(qa,qb,k/nd), k=1..nd-1, is valid,
 * nd = max_j ceil(|d_j| / (resolution * extent_j)).
 * Large batches are served by expanding every segment into its states (count, scan, expand), validating them with the
 * lane-per-state kernel and AND-ing per segment; that path reads the total state count back once, i.e. the call
 * synchronises `stream` before it returns (results are still produced asynchronously on the stream). */
int mopa_check_motion_batch(MopaScene *scene, const double *qa_dev /*[N,na]*/, const double *qb_dev /*[N,na]*/,
                            const double *qpos_env_dev /*[E,nq]*/, int64_t N, int64_t samples_per_env,
                            uint8_t *valid_dev /*[N]*/, void *stream);

/* E independent RRT-Connect queries (one per env).  path rows hold full qpos vectors with the passive
 * columns copied from start (KinematicPlanner.cpp:236-240; a glued scene: the carried body's free-joint columns hold its pose at
 * the waypoint, see mopa_scene_create_glued).  status[e] in {0,-4,-5}. */
int mopa_plan_batch(MopaScene *scene, const double *start_dev /*[E,nq]*/, const double *goal_dev /*[E,nq]*/, int64_t E,
                    const MopaPlanParams *params, double *path_dev /*[E,max_path,nq]*/, int32_t *path_len_dev /*[E]*/,
                    int32_t *status_dev /*[E]*/, int64_t *n_checks_dev /*[E] or NULL*/, void *stream);

/* K9: the two vertex-removing passes of OMPL's PathSimplifier (reduceVertices, collapseCloseVertices) over the rows
 * mopa_plan_batch wrote, in place, one wave per path, asynchronous on `stream` with no read-back.  Every surviving row is one of
 * the input rows (both endpoints are kept); the survivors are compacted to the front in order and path_len[e] is rewritten; rows
 * at and beyond the new length are unspecified.  The routines, their integer draws and the schedule are defined in DESIGN.md
 * ("K9 path simplification"); shortcutPath is mopa_shortcut_paths_batch below, the B-spline smoothing mopa_smooth_paths_batch;
 * checkAndRepair is NOT built.
 *   motion checks: mopa_check_motion_batch's rule between the rows' active entries, with the passive entries of row 0.
 *   draws:         the k-th draw of path e is the uniform of counter 2^63 + k of the stream (seed, id) that query e of
 *                  mopa_plan_batch samples from -- seed, env_id_base, env_ids_dev and seeds_dev as in MopaPlanParams.
 *   passes:        bit 0 = reduceVertices, bit 1 = collapseCloseVertices (a routine that is masked out returns false).
 *   skipped:       paths with status[e] != 0 (status_dev may be NULL: none) or path_len[e] < 3 (the unwritten rows of a
 *                  continuation launch among them) -- not one of their bytes is touched, info_dev's included.
 *   info_dev:      nullable, [E,2]: motion checks made, draws consumed.
 * Argument errors return before any launch: NULL scene / buffers, E < 0, max_path < 2, passes outside 1..3
 * (MOPA_ERR_INVALID_ARG); max_path beyond mopa_simplify_paths_max_path(scene), what the per-wave LDS lists hold -- at least 512
 * for the scenes of this project -- (MOPA_ERR_UNSUPPORTED). */
int mopa_simplify_paths_batch(MopaScene *scene, int64_t E, int32_t max_path, double *path_dev /*[E,max_path,nq] in/out*/,
                              int32_t *path_len_dev /*[E] in/out*/, const int32_t *status_dev /*[E] nullable*/, uint64_t seed,
                              uint64_t env_id_base, const uint64_t *env_ids_dev /*nullable*/, const uint64_t *seeds_dev /*nullable*/,
                              int32_t passes, int64_t *info_dev /*[E,2] nullable*/, void *stream);
int mopa_simplify_paths_max_path(const MopaScene *scene);

/* K9 with shortcutPath: OMPL's PathSimplifier::shortcutPath (passes bit 2) in front of the two vertex-removing passes (bits 0 and
 * 1, as above), in place, one wave per path, asynchronous on `stream` with no read-back.  shortcutPath connects points in the
 * interior of segments, so the result holds rows that are no input rows: a new row has the interpolated active entries and row
 * 0's passive entries.  Both endpoints are kept; the rows are put in order at the front and path_len[e] is rewritten (it can
 * grow, never beyond max_path); rows at and beyond the new length are unspecified.  The routine, every floating-point operation
 * of it, its two deviations from OMPL (a splice is accepted only if the stubs between a new interior point and its old
 * neighbours pass the motion check too; a splice that would need row max_path + 1 is skipped) and the schedule are defined in
 * DESIGN.md ("K9 path simplification: shortcutPath"); smoothBSpline is mopa_smooth_paths_batch below, checkAndRepair is NOT built.
 *   motion checks, draws, skipped paths: as for mopa_simplify_paths_batch (one draw counter runs through the whole call); a path
 *                  with path_len[e] > max_path is skipped too.
 *   passes:        1..7; with bit 2 clear the result is mopa_simplify_paths_batch's.
 *   max_rounds:    >= 1, bound on the rounds of the schedule (it stands in for OMPL's wall clock: a shortcut can add a vertex).
 *   info_dev:      nullable, [E,6]: motion checks, draws, rounds, accepted shortcut splices, capacity skips, largest vertex
 *                  count reached.
 * Argument errors return before any launch: NULL scene / buffers, E < 0, max_path < 2, passes outside 1..7, max_rounds < 1
 * (MOPA_ERR_INVALID_ARG); max_path beyond mopa_shortcut_paths_max_path(scene), what the per-wave LDS lists hold
 * (MOPA_ERR_UNSUPPORTED). */
int mopa_shortcut_paths_batch(MopaScene *scene, int64_t E, int32_t max_path, double *path_dev /*[E,max_path,nq] in/out*/,
                              int32_t *path_len_dev /*[E] in/out*/, const int32_t *status_dev /*[E] nullable*/, uint64_t seed,
                              uint64_t env_id_base, const uint64_t *env_ids_dev /*nullable*/, const uint64_t *seeds_dev /*nullable*/,
                              int32_t passes, int32_t max_rounds, int64_t *info_dev /*[E,6] nullable*/, void *stream);
int mopa_shortcut_paths_max_path(const MopaScene *scene);

/* K9 with smoothBSpline: per round of the schedule shortcutPath (passes bit 2), then OMPL's PathSimplifier::smoothBSpline (bit 3),
 * then the two vertex-removing passes (bits 0 and 1) -- PathSimplifier::simplify's schedule without its wall clock -- in place, one
 * wave per path, asynchronous on `stream` with no read-back.  A smoothing step (at most 3 per call of the routine) puts a vertex
 * into the middle of every segment and moves every old interior vertex to the middle of the middles towards its two new
 * neighbours when both motions pass and the vertex moves by more than 1/100 of the path's length at entry; so new rows appear
 * (interpolated active entries, row 0's passive ones) and input rows change their active entries.  Both endpoints are kept;
 * path_len[e] can grow, never beyond max_path; rows at and beyond the new length are unspecified.  The routine, every
 * floating-point operation of it and its three deviations from OMPL (a vertex moves only if the outer halves of its two old
 * segments pass the motion check too; a step in which nothing moves is undone; a midpoint between two vertices that stayed is
 * kept only if both its halves pass -- so every segment of a result has itself passed the motion check) are defined in DESIGN.md
 * ("K9 path simplification: smoothBSpline"); a step that would need more than max_path rows ends the smoothing and counts as a
 * capacity skip.  The routine draws nothing.  checkAndRepair is NOT built.
 *   motion checks, draws, skipped paths, max_rounds: as for mopa_shortcut_paths_batch.
 *   passes:        1..15; with bit 3 clear the result is mopa_shortcut_paths_batch's.
 *   info_dev:      nullable, [E,10]: columns 0-5 as for mopa_shortcut_paths_batch (the smoothing's capacity stops are added into
 *                  column 4), then smoothing steps subdivided, vertices moved, idle midpoints dropped, state checks.
 * Argument errors return before any launch: NULL scene / buffers, E < 0, max_path < 2, passes outside 1..15, max_rounds < 1
 * (MOPA_ERR_INVALID_ARG); max_path beyond mopa_smooth_paths_max_path(scene), what the per-wave LDS lists hold next to the slabs of
 * the four-state validity pass (MOPA_ERR_UNSUPPORTED). */
int mopa_smooth_paths_batch(MopaScene *scene, int64_t E, int32_t max_path, double *path_dev /*[E,max_path,nq] in/out*/,
                            int32_t *path_len_dev /*[E] in/out*/, const int32_t *status_dev /*[E] nullable*/, uint64_t seed,
                            uint64_t env_id_base, const uint64_t *env_ids_dev /*nullable*/, const uint64_t *seeds_dev /*nullable*/,
                            int32_t passes, int32_t max_rounds, int64_t *info_dev /*[E,10] nullable*/, void *stream);
int mopa_smooth_paths_max_path(const MopaScene *scene);

/* K3b: E independent RRT* queries (the reference's planner_type "rrt": OMPL geometric::RRTstar with k-nearest neighbourhoods and
 * the path-length objective), one wave per query, asynchronous on `stream` with no read-back.  A single tree that chooses every
 * new node's parent by cost among its k nearest nodes and rewires those neighbours through the new node; the planner is anytime
 * and always runs its whole iteration budget.  The routine, every floating-point operation of it and its deviations from OMPL (an
 * iteration budget for the wall clock, the counter sample stream, a node capacity) are defined in DESIGN.md ("K3b RRT*"); the
 * sequential form is tests/rrtstar_ref.py.
 *   draws:        iteration `it` of query e uses counters it * (na + 1) (goal bias) and it * (na + 1) + 1 + a (coordinate a) of the
 *                 stream (seed, id) -- seed, env_id_base, env_ids_dev, seeds_dev as in MopaPlanParams; K9's draws stay disjoint.
 *   neighbours:   k(n) = ceil(rewire_factor * (e + e / na) * ln(n + 1)) of the n nodes (mopa_plan_star_k), at most 64.
 *   motion checks: mopa_check_motion_batch's rule, with the passive entries of start[e].
 *   goal nodes:   new states within goal_threshold (L1, SO(2) the short way) of the goal; until one exists a sample is the goal
 *                 itself with probability goal_bias.
 *   results:      status[e] in {0, -4, -5}; path rows hold full qpos vectors with the passive columns of start (the chain of the
 *                 cheapest goal node; more than max_path rows: -4); path_len[e] = 0 and cost[e] = +inf unless status[e] = 0;
 *                 cost[e] = that node's cost, the chain's top-down sum of L1 segment lengths.
 *   info_dev:     nullable, [E,8]: iterations run, nodes, motion checks, rewires, goal nodes, first goal iteration (-1: none),
 *                 descendant cost updates, iterations that found the tree full.
 * The trees live in the library's scratch, one per resident wave (memory does not grow with E).
 * Argument errors return before any launch: NULL scene / params / buffers, E < 0, max_iters < 0, max_nodes < 2, max_path < 2,
 * goal_bias outside [0, 1], goal_threshold < 0, rewire_factor <= 0 (MOPA_ERR_INVALID_ARG); k(max_nodes) > 64 or trees the scratch
 * cannot hold (MOPA_ERR_UNSUPPORTED). */
typedef struct MopaStarParams {
    int32_t max_iters;     /* iteration budget: always spent */
    int32_t max_nodes;     /* node capacity of the tree; an iteration that finds it full does nothing */
    int32_t max_path;      /* rows available per query in `path` */
    uint64_t seed;
    uint64_t env_id_base;
    const uint64_t *env_ids_dev;   /* nullable, [E] */
    const uint64_t *seeds_dev;     /* nullable, [E] */
    double goal_bias;              /* OMPL's default: 0.05 */
    double goal_threshold;         /* the reference's `threshold` (0: the goal sample itself has to be reached) */
    double rewire_factor;          /* OMPL's default: 1.1 */
    int32_t max_workgroups;        /* > 0: cap on the persistent workgroups of the launch; otherwise two per CU */
} MopaStarParams;
int mopa_plan_star_batch(MopaScene *scene, const double *start_dev /*[E,nq]*/, const double *goal_dev /*[E,nq]*/, int64_t E,
                         const MopaStarParams *params, double *path_dev /*[E,max_path,nq]*/, int32_t *path_len_dev /*[E]*/,
                         int32_t *status_dev /*[E]*/, double *cost_dev /*[E] nullable*/, int64_t *info_dev /*[E,8] nullable*/,
                         void *stream);
/* the single-query host form of mopa_plan_star_batch (host pointers, stream id = env_id_base, synchronous) */
int mopa_plan_star(MopaScene *scene, const double *start_host, const double *goal_host, const MopaStarParams *params,
                   double *path_host /*[max_path,nq]*/, int32_t *path_len_out, int32_t *status_out, double *cost_out /*nullable*/,
                   int64_t *info_out /*[8] nullable*/);
/* k(n) of a scene with na active coordinates, computed on the host in double with libm's log (-1: na < 1 or n < 1) */
int mopa_plan_star_k(int32_t na, int64_t n, double rewire_factor);
int mopa_star_params_size(void);

/* K3b under the maximize-min-clearance objective, band-limited: RRT* that optimises the quantity mopa_path_clearance_batch measures.
 * Same shape as mopa_plan_star_batch (one wave per query, asynchronous on `stream`, no read-back, MopaStarParams unchanged); the
 * definition is the sequential form tests/star_clearance_ref.py ("K3b under the clearance objective").
 *   band:         finite, >= 0 and above the scene's contact_threshold; every clearance saturates at it.
 *   motion value: mc(a -> b) = mopa_motion_clearance_batch's `clearance` of the segment on the passive entries of start[e]; a motion
 *                 is valid iff mc > contact_threshold, which is mopa_check_motion_batch's verdict.
 *   key:          a chain's cost is the pair (C, L): C = min(the clearance of the start state, the values of its edges), L = its L1
 *                 length; (C1, L1) is better than (C2, L2) iff C1 > C2 or (C1 == C2 and L1 < L2).  LEXICOGRAPHIC ON PURPOSE: OMPL's
 *                 pure minimax cost ties wherever nothing is in band and never rewires there.  Where no evaluated motion is in band
 *                 the planner is mopa_plan_star_batch bit for bit.
 *   parent:       exact branch and bound over the neighbours' bounds (C[i], L[i] + dist), best first, starting from the nearest node;
 *   rewire:       pre-tested on the bound, then evaluated from the new state to the neighbour (no value is reused across directions).
 *   node set:     draws, nearest, steering, the full-tree rule, k(n) and the goal rules are mopa_plan_star_batch's, so for equal seed,
 *                 ids and parameters status (up to max_path), nodes, goal nodes and first goal iteration equal that planner's.
 *   results:      the chain of the goal node with the best key (the earliest among equals); clearance[e] = its C, which is the bits
 *                 of mopa_path_clearance_batch on the returned rows (vertex 0 counted), length[e] = its L.  Unless status[e] = 0:
 *                 path_len[e] = 0, clearance[e] = -inf, length[e] = +inf.
 *   info_dev:     nullable, [E,11]: columns 0-7 as mopa_plan_star_batch with column 2 counting motion evaluations (motions, never
 *                 states; an evaluation may stop at the first state at or below the threshold), 8 = evaluations of the parent walk,
 *                 9 = evaluations of the rewire step, 10 = rewires that strictly raised C.
 * Refused before any launch: everything mopa_plan_star_batch refuses; band negative, NaN or infinite, band <= contact_threshold
 * (MOPA_ERR_INVALID_ARG); a glued scene, a scene created with pair_cull_radius (MOPA_ERR_UNSUPPORTED); LDS (MOPA_ERR_LIMIT).
 * E == 0 returns MOPA_OK without a launch. */
int mopa_plan_star_clearance_batch(MopaScene *scene, const double *start_dev /*[E,nq]*/, const double *goal_dev /*[E,nq]*/, int64_t E,
                                   const MopaStarParams *params, double band, double *path_dev /*[E,max_path,nq]*/,
                                   int32_t *path_len_dev /*[E]*/, int32_t *status_dev /*[E]*/, double *clearance_dev /*[E]*/,
                                   double *length_dev /*[E] nullable*/, int64_t *info_dev /*[E,11] nullable*/, void *stream);
/* the single-query host form (host pointers, stream id = env_id_base, synchronous) */
int mopa_plan_star_clearance(MopaScene *scene, const double *start_host, const double *goal_host, const MopaStarParams *params, double band,
                             double *path_host /*[max_path,nq]*/, int32_t *path_len_out, int32_t *status_out, double *clearance_out,
                             double *length_out /*nullable*/, int64_t *info_out /*[11] nullable*/);

/* K3 race: E RRT-Connect queries, each run by `portfolio` = K members that share start, goal, env row and stream id and differ in
 * their seed only; asynchronous on `stream`, no read-back.  The result of a query is that of ONE member, chosen by a rule that does
 * not depend on timing (DESIGN.md "K3 race"; the sequential form is tests/race_ref.py):
 *   members:   member m of query g runs stream id env_ids_dev[g] (or env_id_base + g) with the seed (seed_g + m * 0x9E3779B97F4A7C15)
 *              mod 2^64, seed_g = seeds_dev[g] or seed, and the full budget.  Member 0 is exactly the query mopa_plan_batch runs, so
 *              portfolio = 1 gives mopa_plan_batch's status, rows, path_len and n_checks.
 *   winner:    the solved member (status 0; a solution of more than max_path rows is not solved) with the smallest (consumed checks,
 *              m).  A member stops early only when its count so far already exceeds a solved member's final count -- when it could no
 *              longer win --, so launch order, residency and placement cannot change a result.
 *   results:   the winner's rows (as mopa_plan_batch writes them), path_len, status 0, the winner's n_checks, winner = m, win_seed =
 *              its seed.  No solved member: status -5 if the goal is invalid (every member agrees), else -4; winner = -1, path_len =
 *              0, n_checks and win_seed are member 0's.
 *   info_dev:  nullable, [E,3]: members cut, checks spent by all members until they stopped, the winner's iterations (-1: none).
 *              Columns 0 and 1 DEPEND ON TIMING unless no_abort is set (then 0 and the sum of all members' full counts).
 *   memory:    the trees of all members live in the library's scratch: E * K * 2 * max_nodes * na doubles plus E * K * 2 * max_nodes
 *              int32 parents; MOPA_ERR_LIMIT, with the byte count in mopa_last_error(), when the device cannot hold them.
 *   launch:    mopa_plan_batch's policy over the E * K slots (slot v = member v / E of query v % E); max_workgroups as there.
 * Argument errors return before anything touches a device: NULL scene / params / buffers (info_dev alone is nullable), E < 0,
 * max_iters < 0, max_nodes < 2, max_path < 2, portfolio outside 1..256 (MOPA_ERR_INVALID_ARG). */
typedef struct MopaRaceParams {
    int32_t max_iters;     /* iteration budget of every member */
    int32_t max_nodes;     /* per-tree node capacity of every member */
    int32_t max_path;      /* rows available per query in `path` */
    int32_t portfolio;     /* K: members per query, 1..256 */
    uint64_t seed;
    uint64_t env_id_base;
    const uint64_t *env_ids_dev;   /* nullable, [E] */
    const uint64_t *seeds_dev;     /* nullable, [E] */
    int32_t max_workgroups;        /* as in MopaPlanParams */
    int32_t no_abort;              /* nonzero: no member is cut, every member runs to its own end (tests, measurements) */
} MopaRaceParams;
int mopa_plan_race_batch(MopaScene *scene, const double *start_dev /*[E,nq]*/, const double *goal_dev /*[E,nq]*/, int64_t E,
                         const MopaRaceParams *params, double *path_dev /*[E,max_path,nq]*/, int32_t *path_len_dev /*[E]*/,
                         int32_t *status_dev /*[E]*/, int64_t *n_checks_dev /*[E]*/, int32_t *winner_dev /*[E]*/,
                         uint64_t *win_seed_dev /*[E]*/, int64_t *info_dev /*[E,3] nullable*/, void *stream);
/* the single-query host form of mopa_plan_race_batch (host pointers, stream id = env_id_base, synchronous); sets the planner status
 * string as mopa_plan does.  n_checks_out, winner_out, win_seed_out and info_out [3] are nullable */
int mopa_plan_race(MopaScene *scene, const double *start_host, const double *goal_host, const MopaRaceParams *params,
                   double *path_host /*[max_path,nq]*/, int32_t *path_len_out, int32_t *status_out, int64_t *n_checks_out,
                   int32_t *winner_out, uint64_t *win_seed_out, int64_t *info_out);
int mopa_race_params_size(void);

/* The rollout's invalid-target back-off (rl/mopa_rollouts.py:133-143) for E envs, asynchronous (no read-back unless E * num_trials
 * rows would exceed 1 GiB of scratch; E < 256: one wave per env walks its trials, otherwise all candidate rows of all
 * invalid targets go through one validity launch -- same results): while target[e] (a full
 * qpos row, validated with its own passive entries) is invalid and fewer than num_trials steps were taken,
 *   target[e] += step_size * (cur[e] - target[e]) / ||cur[e] - target[e]||   (Euclidean norm over all nq entries, squares
 * summed left to right).  target is updated in place; n_trials[e] = steps taken, valid[e] = verdict of the final row. */
int mopa_pullback_batch(MopaScene *scene, const double *cur_dev /*[E,nq]*/, double *target_dev /*[E,nq] in/out*/, int64_t E,
                        double step_size, int32_t num_trials, int32_t *n_trials_dev /*[E]*/, uint8_t *valid_dev /*[E]*/,
                        void *stream);

/* ---- single-query convenience forms: what PyKinematicPlanner binds (host pointers, synchronous) ---- */
int mopa_is_valid_state(MopaScene *scene, const double *qpos_host /*[nq]*/, int32_t *valid_out, double *min_dist_out /*nullable*/);
int mopa_plan(MopaScene *scene, const double *start_host /*[nq]*/, const double *goal_host /*[nq]*/,
              const MopaPlanParams *params, double *path_host /*[max_path,nq]*/, int32_t *path_len_out, int32_t *status_out,
              int64_t *n_checks_out /*nullable*/);
/* OMPL-style status string of the last mopa_plan on this scene ("none" before the first). */
const char *mopa_planner_status(const MopaScene *scene);

/* debug / parity hooks: world pose of every collidable geom for one state (host pointers, synchronous) */
int mopa_debug_fk(MopaScene *scene, const double *qpos_host /*[nq]*/, double *geom_xpos_host /*[ngeom,3]*/,
                  double *geom_xmat_host /*[ngeom,9]*/);
/* per-candidate-pair distances (MOPA_FAR for culled / ignored pairs), in MopaModel.pair_geom order */
int mopa_debug_pair_dist(MopaScene *scene, const double *qpos_host /*[nq]*/, double *dist_host /*[npair]*/);

/* Contact report: WHICH pairs are in contact -- what a user of the reference reads off d->contact[i].geom1 / geom2 / dist
 * (mujoco_ompl_interface.cpp:917-978).  State i as in mopa_is_valid_batch.  One record per non-ignored candidate pair p with
 * dist_p <= cutoff: p = index into the pair list of the MopaSceneDesc the scene was created from, dist_p = the bits
 * mopa_debug_pair_dist reports.  The records of a state are sorted by ascending p; count[i] is their true number, even above
 * max_contacts (K) -- then the K records with the lowest p are kept.  Unused slots hold pair = -1, dist = MOPA_FAR.
 * cutoff must be finite and < 0 and K >= 1 (MOPA_ERR_INVALID_ARG): the broad phase culls at zero margin, so every pair at or
 * below a negative cutoff survives it and the report is exact.  A scene created with pair_cull_radius is proven down to its
 * contact_threshold only: cutoff > contact_threshold returns MOPA_ERR_UNSUPPORTED there.  cutoff = contact_threshold lists the
 * pairs that make a state invalid.  Two launches (the min-depth form of mopa_is_valid_batch, then one wave per state that has a
 * record), asynchronous on `stream`, deterministic: no atomics decide order or content. */
int mopa_contacts_batch(MopaScene *scene, const double *q_active_dev /*[N,na]*/, const double *qpos_env_dev /*[E,nq]*/,
                        int64_t N, int64_t samples_per_env, double cutoff, int32_t max_contacts /*K*/,
                        int32_t *count_dev /*[N]*/, int32_t *pair_dev /*[N,K]*/, double *dist_dev /*[N,K]*/, void *stream);
/* the same for one state (host pointers, synchronous) */
int mopa_contacts_state(MopaScene *scene, const double *qpos_host /*[nq]*/, double cutoff, int32_t max_contacts /*K*/,
                        int32_t *count /*[1]*/, int32_t *pair /*[K]*/, double *dist /*[K]*/);

/* Motion report: WHERE a segment is blocked and by which pairs -- OMPL's DiscreteMotionValidator::checkMotion(s1, s2, lastValid),
 * the overload mopa_check_motion_batch leaves out, plus the contact report of the first blocked state.
 * Segment i runs from qa[i] to qb[i] (active coordinates) on env row qpos_env[i / samples_per_env], as in mopa_check_motion_batch.
 *   nd = validSegmentCount(qa, qb) (mopa_check_motion_batch's), c = max(nd, 1)
 *   states s_k, k = 1 .. c: s_c = qb, its bits copied; for k < c, s_k[a] = interpolate(qa[a], qb[a], (double)k / (double)c) per
 *   coordinate (SO(2) coordinates the short way round) -- the expressions mopa_check_motion_batch evaluates.  qa is NOT tested
 *   (OMPL assumes s1 valid, and so does mopa_check_motion_batch).
 * Outputs per segment:
 *   valid         1 iff every s_k is valid: the byte mopa_check_motion_batch writes
 *   n_states      c
 *   first_bad     the smallest k with s_k invalid; 0 if the segment is valid
 *   last_valid_t  1.0 if valid, else (double)(first_bad - 1) / (double)c (one division; first_bad == 1 gives 0.0)
 *   last_valid_q  (nullable) qb if valid; the bits of qa if first_bad == 1; otherwise s_{first_bad - 1}, the very values that were
 *                 validated at that index
 *   first_bad_q   (nullable) s_{first_bad}; qb if the segment is valid, so that a contact report over these rows sees a valid
 *                 state and writes an empty row
 * Deviation: for nd == 0 (qa == qb) OMPL's (nd - 1) / nd is undefined; here c = 1, so an invalid qb gives first_bad = 1,
 * last_valid_t = 0.0, last_valid_q = qa.
 * Blockers (max_contacts = K >= 1; 0 with the three buffers NULL: off): block_count / block_pair / block_dist are, by definition,
 * what mopa_contacts_batch writes for the states first_bad_q with the same env mapping, cutoff = the scene's contact_threshold and
 * that K (it is called on them; first_bad_q lives in library scratch when the caller passed NULL).  A blocked segment has
 * block_count >= 1; a valid one the "unused" row: count 0, pair -1, MOPA_FAR.  Everything mopa_contacts_batch refuses is refused
 * here with its status, a scene whose contact_threshold is not negative included.  Frames and manifolds: pass first_bad_q to
 * mopa_contact_frames_batch / mopa_contact_manifolds_batch.
 * Two forms under mopa_check_motion_batch's dispatch rule (mopa_scene_motion_kernel names the form of both calls): one wave per
 * segment that walks k upwards and stops at the first invalid state (a segment blocked only at its end costs c passes here, one in
 * mopa_check_motion_batch), or the expansion into states with an ordered reduction; the latter reads the state count back once per
 * chunk, i.e. it synchronises `stream` before it returns.  Deterministic: every output word has one writer.
 * MOPA_ERR_INVALID_ARG: a NULL scene; with N > 0 a NULL qa / qb / qpos_env / valid / n_states / first_bad / last_valid_t; N < 0;
 * samples_per_env <= 0; max_contacts < 0; max_contacts == 0 with a blocker buffer given; max_contacts >= 1 with a NULL blocker
 * buffer (N > 0).  MOPA_ERR_UNSUPPORTED: a glued scene.  All of them before any launch; N == 0 returns MOPA_OK. */
int mopa_motion_report_batch(MopaScene *scene, const double *qa_dev /*[N,na]*/, const double *qb_dev /*[N,na]*/,
                             const double *qpos_env_dev /*[E,nq]*/, int64_t N, int64_t samples_per_env, uint8_t *valid_dev /*[N]*/,
                             int32_t *n_states_dev /*[N]*/, int32_t *first_bad_dev /*[N]*/, double *last_valid_t_dev /*[N]*/,
                             double *last_valid_q_dev /*[N,na] or NULL*/, double *first_bad_q_dev /*[N,na] or NULL*/,
                             int32_t max_contacts /*K, 0 = off*/, int32_t *block_count_dev /*[N]*/, int32_t *block_pair_dev /*[N,K]*/,
                             double *block_dist_dev /*[N,K]*/, void *stream);
/* the same for one segment (host pointers, synchronous): from the active entries of qpos_a to those of qpos_b; the passive
 * entries come from qpos_a, as in the path kernels.  The rows hold active coordinates. */
int mopa_motion_report(MopaScene *scene, const double *qpos_a_host /*[nq]*/, const double *qpos_b_host /*[nq]*/, int32_t *valid_out,
                       int32_t *n_states_out, int32_t *first_bad_out, double *last_valid_t_out, double *last_valid_q_out /*[na] or NULL*/,
                       double *first_bad_q_out /*[na] or NULL*/, int32_t max_contacts /*K, 0 = off*/, int32_t *block_count /*[1]*/,
                       int32_t *block_pair /*[K]*/, double *block_dist /*[K]*/);

/* Contact frames: the contact report plus, per record, what the reference reads off d->contact[i].frame / pos
 * (util/contact_info.py).  ONE frame per reported pair -- that of the deepest contact -- where MuJoCo may emit several contacts
 * (box-box, capsule-plane ...).  For record (state i, slot k) with geoms (g1, g2) as MopaModel.pair_geom orders them:
 *   normal[i,k,:]  unit vector from g1 towards g2: translating g2 by -dist * normal removes the overlap along it
 *   pos[i,k,:]     midpoint of two witness points, w1 on g1 and w2 on g2, with w2 - w1 = dist * normal
 * count / pair / dist are exactly mopa_contacts_batch's (same launches, same bytes); unused slots of normal / pos hold 0.0.
 * Same argument rules and status codes as mopa_contacts_batch, including the glued-scene and pair_cull_radius refusals.  One
 * more launch behind the report's two (a wave per state with a record), deterministic.  The definition per pair class is in
 * DESIGN.md section 4 ("Contact frames"; PARITY UNPINNED -- the points of a multi-point contact: mopa_contact_manifolds_batch). */
int mopa_contact_frames_batch(MopaScene *scene, const double *q_active_dev /*[N,na]*/, const double *qpos_env_dev /*[E,nq]*/,
                              int64_t N, int64_t samples_per_env, double cutoff, int32_t max_contacts /*K*/,
                              int32_t *count_dev /*[N]*/, int32_t *pair_dev /*[N,K]*/, double *dist_dev /*[N,K]*/,
                              double *normal_dev /*[N,K,3]*/, double *pos_dev /*[N,K,3]*/, void *stream);
/* the same for one state (host pointers, synchronous) */
int mopa_contact_frames_state(MopaScene *scene, const double *qpos_host /*[nq]*/, double cutoff, int32_t max_contacts /*K*/,
                              int32_t *count /*[1]*/, int32_t *pair /*[K]*/, double *dist /*[K]*/, double *normal /*[K,3]*/,
                              double *pos /*[K,3]*/);
/* Pair level: M posed primitive pairs, one lane each.  types [M,2] (MuJoCo geom type codes, either order: the pair is evaluated
 * in the narrow phase's canonical order and the normal negated on the way out when that is the reverse), recs [M,2,15] =
 * pos[3] mat[9] size[3] per geom, out [M,7] = dist, normal[3], pos[3]; dist = MOPA_FAR (and a zero frame) where the narrow phase
 * reports no overlap or the type pair is unsupported.  Meshes are not served at this level on the device. */
int mopa_geom_frames_batch(int32_t device, int64_t M, const int32_t *types_dev, const double *recs_dev, double *out_dev, void *stream);
/* The host compile of the same functions -- the sequential form the kernels match bit for bit.  Needs no GPU and makes no HIP
 * call.  A mesh as the second geom of every pair of type 7: its hull vertices mesh_verts [nvert,3] in the mesh frame (nullable
 * with nvert = 0). */
int mopa_geom_frames_host(int64_t M, const int32_t *types, const double *recs, const double *mesh_verts /*nullable*/, int32_t nvert,
                          double *out);

/* Contact manifolds: the contact report plus, per record, the frame's normal and UP TO max_points (P, 1..8) contact points --
 * what the reference reads off d->contact[i].pos / frame / dist per contact where MuJoCo emits several for a pair (box-plane 4,
 * capsule-plane 2, box-box up to 8).  [3P] The candidate points per pair class are restated from MuJoCo's documented behaviour,
 * PARITY UNPINNED; the table is in DESIGN.md section 4 ("Contact manifolds").  For record (state i, slot k):
 *   normal[i,k,:]        the bits mopa_contact_frames_batch reports: one normal per pair
 *   npoint[i,k]          the number of points with dist_j <= point_cutoff, at most 8, NOT capped by P; 0 in unused slots
 *   point_dist[i,k,j]    sorted ascending (deepest first, ties in generation order), the first P kept; MOPA_FAR in unused slots
 *   point_pos[i,k,j,:]   midpoint of the point's two witnesses, w1 on g1 and w2 on g2, w2 - w1 = dist_j * normal; 0.0 when unused
 * A class rule that yields no point under point_cutoff falls back to the single frame point (the bits of
 * mopa_contact_frames_batch's pos and of dist), as every single-point class does.  count / pair / dist are exactly
 * mopa_contacts_batch's (it is called first: same launches, same bytes, same argument rules and status codes, the glued-scene
 * and pair_cull_radius refusals included).  P outside 1..8, point_cutoff not finite or < cutoff, a null output:
 * MOPA_ERR_INVALID_ARG; a scene that does not fit LDS: MOPA_ERR_LIMIT.  One more launch behind the report's two, deterministic:
 * every output word has one writer, plain stores. */
int mopa_contact_manifolds_batch(MopaScene *scene, const double *q_active_dev /*[N,na]*/, const double *qpos_env_dev /*[E,nq]*/,
                                 int64_t N, int64_t samples_per_env, double cutoff, double point_cutoff, int32_t max_contacts /*K*/,
                                 int32_t max_points /*P*/, int32_t *count_dev /*[N]*/, int32_t *pair_dev /*[N,K]*/,
                                 double *dist_dev /*[N,K]*/, double *normal_dev /*[N,K,3]*/, int32_t *npoint_dev /*[N,K]*/,
                                 double *point_dist_dev /*[N,K,P]*/, double *point_pos_dev /*[N,K,P,3]*/, void *stream);
/* the same for one state (host pointers, synchronous) */
int mopa_contact_manifolds_state(MopaScene *scene, const double *qpos_host /*[nq]*/, double cutoff, double point_cutoff,
                                 int32_t max_contacts /*K*/, int32_t max_points /*P*/, int32_t *count /*[1]*/, int32_t *pair /*[K]*/,
                                 double *dist /*[K]*/, double *normal /*[K,3]*/, int32_t *npoint /*[K]*/, double *point_dist /*[K,P]*/,
                                 double *point_pos /*[K,P,3]*/);
/* Pair level: M posed primitive pairs, one lane each; types / recs as mopa_geom_frames_batch takes them.  normal_dist [M,4] =
 * normal[3], dist (the pair's, mopa_geom_frames_batch's bits); npoint [M]; points [M,P,4] = pos[3], dist_j.  No cutoff applies
 * to the pair itself at this level: only point_cutoff (finite) to its points.  Meshes are not served on the device. */
int mopa_geom_manifolds_batch(int32_t device, int64_t M, const int32_t *types_dev, const double *recs_dev, double point_cutoff,
                              int32_t max_points /*P*/, double *normal_dist_dev, int32_t *npoint_dev, double *points_dev, void *stream);
/* The host compile of the same functions -- the sequential form the kernels match bit for bit; no GPU, no HIP call.  mesh_verts
 * as in mopa_geom_frames_host. */
int mopa_geom_manifolds_host(int64_t M, const int32_t *types, const double *recs, const double *mesh_verts /*nullable*/, int32_t nvert,
                             double point_cutoff, int32_t max_points /*P*/, double *normal_dist, int32_t *npoint, double *points);

/* Proximity report: HOW FAR from collision a state is and which pairs are nearest, inside a band the caller gives (DESIGN.md
 * section 4, "Proximity report").  State i as in mopa_is_valid_batch.  Per non-ignored candidate pair p the band-limited distance
 * d_p: the bits of the contact report for shapes in overlap; for disjoint shapes the separation distance where the pair function
 * is one in closed form (plane-X, sphere-X, capsule-capsule, capsule-box, plane-mesh) and otherwise (box-box, cylinder pairs,
 * convex-mesh) MuJoCo's margin rule: the portal refinement on the shapes inflated by band / 2 each, band taken off its depth --
 * never more than 1e-6 above the true distance, below it by a shortfall that grows with band (measured per class in DESIGN.md).
 * Pairs with d_p > band are out of band.  Outputs per state:
 *   clearance[i]  min(band, min_p d_p): band when no pair is in band
 *   count[i]      the number of pairs in band, even above max_pairs (K)
 *   pair[i,:], dist[i,:]  the K nearest pairs (index into the pair list of the MopaSceneDesc) and their d_p, ascending by
 *                 (d_p, p); unused slots hold pair = -1, dist = MOPA_FAR
 * band must be finite and >= 0 and K >= 1 (MOPA_ERR_INVALID_ARG).  A glued scene and a scene created with pair_cull_radius (proven
 * down to its contact_threshold only) return MOPA_ERR_UNSUPPORTED; per-wave distance arrays beyond LDS MOPA_ERR_LIMIT; N == 0 is a
 * no-op.  One launch of its own (a wave per state, a broad phase widened by band), asynchronous on `stream`, deterministic: no
 * atomics decide order or content.  The validity, contact and motion entry points are untouched by it. */
int mopa_proximity_batch(MopaScene *scene, const double *q_active_dev /*[N,na]*/, const double *qpos_env_dev /*[E,nq]*/, int64_t N,
                         int64_t samples_per_env, double band, int32_t max_pairs /*K*/, double *clearance_dev /*[N]*/,
                         int32_t *count_dev /*[N]*/, int32_t *pair_dev /*[N,K]*/, double *dist_dev /*[N,K]*/, void *stream);
/* the same for one state (host pointers, synchronous) */
int mopa_proximity_state(MopaScene *scene, const double *qpos_host /*[nq]*/, double band, int32_t max_pairs /*K*/,
                         double *clearance /*[1]*/, int32_t *count /*[1]*/, int32_t *pair /*[K]*/, double *dist /*[K]*/);
/* Pair level: M posed pairs, one lane each; types / recs as mopa_geom_frames_batch takes them (either order: the value does not
 * depend on it), out [M] = d if d <= band, else MOPA_FAR.  A mesh (type 7) reads the hull mesh_verts_dev [nvert,3] in the mesh
 * frame (nullable with nvert = 0: mesh pairs then report MOPA_FAR). */
int mopa_geom_sep_batch(int32_t device, int64_t M, const int32_t *types_dev, const double *recs_dev, const double *mesh_verts_dev /*nullable*/,
                        int32_t nvert, double band, double *out_dev, void *stream);
/* The host compile of the same functions -- the sequential form the kernels match bit for bit; no GPU, no HIP call. */
int mopa_geom_sep_host(int64_t M, const int32_t *types, const double *recs, const double *mesh_verts /*nullable*/, int32_t nvert,
                       double band, double *out);
/* Exact route (opt-in; DESIGN.md section 4, "Proximity report", paragraph "Exact route").  The four entry points above with ONE
 * change: a disjoint pair of the inflated classes (box-box, cylinder pairs, convex-mesh) gets its separation distance from GJK on
 * the shapes as they are (gjk_distance, mopa_gjk.hpp) instead of the margin rule: true <= d <= true + 1e-6, the same bits at every
 * band that reports the pair and in either order of the pair.  Overlaps, the closed-form classes, band == 0, the culls, the
 * selection, the argument rules, the status codes and the messages are those of the entry point without `_exact`. */
int mopa_proximity_exact_batch(MopaScene *scene, const double *q_active_dev /*[N,na]*/, const double *qpos_env_dev /*[E,nq]*/, int64_t N,
                               int64_t samples_per_env, double band, int32_t max_pairs /*K*/, double *clearance_dev /*[N]*/,
                               int32_t *count_dev /*[N]*/, int32_t *pair_dev /*[N,K]*/, double *dist_dev /*[N,K]*/, void *stream);
int mopa_proximity_exact_state(MopaScene *scene, const double *qpos_host /*[nq]*/, double band, int32_t max_pairs /*K*/,
                               double *clearance /*[1]*/, int32_t *count /*[1]*/, int32_t *pair /*[K]*/, double *dist /*[K]*/);
int mopa_geom_sep_exact_batch(int32_t device, int64_t M, const int32_t *types_dev, const double *recs_dev,
                              const double *mesh_verts_dev /*nullable*/, int32_t nvert, double band, double *out_dev, void *stream);
/* iters_out [M] (nullable): the exact route's number of support evaluations for pair i; 0 where the route was not taken (overlap,
 * closed form, band == 0, culled); negative where the iteration cap ended it (the value is then a lower bound of the distance). */
int mopa_geom_sep_exact_host(int64_t M, const int32_t *types, const double *recs, const double *mesh_verts /*nullable*/, int32_t nvert,
                             double band, double *out, int32_t *iters_out /*[M] or NULL*/);
/* Witness points (opt-in; DESIGN.md section 4, "Proximity report", paragraph "Witness points"): the exact route's report with, for
 * every record, WHERE on the two shapes the distance is attained and in which direction.  mopa_proximity_exact_batch, then one
 * more launch behind it that reads the rows it wrote; clearance / count / pair / dist are its bytes.  Per record (slot < min(count,
 * K)) of pair (g1, g2) as the MopaSceneDesc lists it, world frame:
 *   p1[i,k,:], p2[i,k,:]  a point of g1 and a point of g2 with |p2 - p1| = dist for separated shapes (to 1e-6 for the GJK classes:
 *                 both are convex combinations of support points); for shapes in overlap the contact frame's two witness points,
 *                 pos -/+ (dist / 2) normal
 *   normal[i,k,:]  the unit vector from p1 towards p2 (separated) / the contact frame's normal (overlap): from g1 towards g2
 * Unused slots hold 0.0.  Argument rules, refusals and status codes are mopa_proximity_exact_batch's (a glued or pruned scene:
 * MOPA_ERR_UNSUPPORTED), a NULL among the three new buffers MOPA_ERR_INVALID_ARG; every refusal precedes the first launch; N == 0
 * is a no-op.  Deterministic: every output word has one writer. */
int mopa_proximity_witness_batch(MopaScene *scene, const double *q_active_dev /*[N,na]*/, const double *qpos_env_dev /*[E,nq]*/, int64_t N,
                                 int64_t samples_per_env, double band, int32_t max_pairs /*K*/, double *clearance_dev /*[N]*/,
                                 int32_t *count_dev /*[N]*/, int32_t *pair_dev /*[N,K]*/, double *dist_dev /*[N,K]*/,
                                 double *normal_dev /*[N,K,3]*/, double *p1_dev /*[N,K,3]*/, double *p2_dev /*[N,K,3]*/, void *stream);
/* the same for one state (host pointers, synchronous) */
int mopa_proximity_witness_state(MopaScene *scene, const double *qpos_host /*[nq]*/, double band, int32_t max_pairs /*K*/,
                                 double *clearance /*[1]*/, int32_t *count /*[1]*/, int32_t *pair /*[K]*/, double *dist /*[K]*/,
                                 double *normal /*[K,3]*/, double *p1 /*[K,3]*/, double *p2 /*[K,3]*/);
/* Pair level: types / recs / mesh_verts / band as mopa_geom_sep_exact_batch takes them; out [M,10] = d, n[3], p1[3], p2[3], d the
 * bits of mopa_geom_sep_exact_batch, p1 on the FIRST geom given: the other order returns p1 / p2 exchanged and n negated.
 * d == MOPA_FAR: the nine others are 0.0. */
int mopa_geom_witness_batch(int32_t device, int64_t M, const int32_t *types_dev, const double *recs_dev,
                            const double *mesh_verts_dev /*nullable*/, int32_t nvert, double band, double *out_dev /*[M,10]*/, void *stream);
/* The host compile of the same functions -- the sequential form the kernels match bit for bit; no GPU, no HIP call.  iters_out as
 * mopa_geom_sep_exact_host's. */
int mopa_geom_witness_host(int64_t M, const int32_t *types, const double *recs, const double *mesh_verts /*nullable*/, int32_t nvert,
                           double band, double *out /*[M,10]*/, int32_t *iters_out /*[M] or NULL*/);

/* Clearance report: HOW NEAR a motion comes to collision, where along it and to which pair -- OMPL's
 * MinimaxObjective::motionCost(s1, s2) under the maximize_min_clearance state cost ("Clearance report").
 * Segments and env rows as in mopa_check_motion_batch; segment i has c = max(validSegmentCount, 1) states s_k, k = 1 .. c, s_c = qb
 * (its bits), the states mopa_motion_report_batch walks; qa is not evaluated.  Per state d_k, p_k = what mopa_proximity_batch
 * writes to clearance and pair[.,0] for s_k at this band (d_k saturates at band; p_k = -1 when no pair is in band).  Per segment:
 *   clearance[i]      min_k d_k
 *   n_states[i]       c
 *   n_near[i]         the number of k with a pair in band
 *   k_min[i]          the smallest k with d_k == clearance and a pair in band; 0 when n_near == 0
 *   t_min[i]          (double)k_min / (double)c; 0.0 when k_min == 0, 1.0 when k_min == c
 *   pair_min[i]       p_{k_min} (index into the pair list of the MopaSceneDesc); -1 when k_min == 0
 *   end_clearance[i]  d_c
 *   q_min[i,:]        s_{k_min}; qb's bits when k_min == 0 (NULL: not written)
 * One form at every batch size: the segments are expanded into their states (mopa_check_motion_batch's large-batch pipeline), a
 * wave per state takes the minimum, a lane per segment reduces in order.  It reads the state count back once per chunk: `stream` is
 * synchronised in the MIDDLE of the call, behind the count and the scan, to size the launches that follow.  The per-state kernel, the
 * reduction and the row copy are still in flight when the call returns: the outputs are complete once `stream` has run them, as
 * with every other asynchronous entry point.  Deterministic: every output word has one writer.
 * Argument rules of mopa_proximity_batch: band finite and >= 0, N >= 0, samples_per_env > 0, no NULL among the required buffers
 * (MOPA_ERR_INVALID_ARG); a glued scene and a scene created with pair_cull_radius return MOPA_ERR_UNSUPPORTED; all of them before
 * any launch; N == 0 returns MOPA_OK.  It needs the scene's own LDS only: a scene whose per-wave distance arrays
 * mopa_proximity_batch refuses with MOPA_ERR_LIMIT is served here. */
int mopa_motion_clearance_batch(MopaScene *scene, const double *qa_dev /*[N,na]*/, const double *qb_dev /*[N,na]*/,
                                const double *qpos_env_dev /*[E,nq]*/, int64_t N, int64_t samples_per_env, double band,
                                double *clearance_dev /*[N]*/, int32_t *n_states_dev /*[N]*/, int32_t *n_near_dev /*[N]*/,
                                int32_t *k_min_dev /*[N]*/, double *t_min_dev /*[N]*/, int32_t *pair_min_dev /*[N]*/,
                                double *end_clearance_dev /*[N]*/, double *q_min_dev /*[N,na] or NULL*/, void *stream);
/* the same for one segment (host pointers, synchronous): from the active entries of qpos_a to those of qpos_b; the passive
 * entries come from qpos_a.  q_min holds active coordinates. */
int mopa_motion_clearance(MopaScene *scene, const double *qpos_a_host /*[nq]*/, const double *qpos_b_host /*[nq]*/, double band,
                          double *clearance_out, int32_t *n_states_out, int32_t *n_near_out, int32_t *k_min_out, double *t_min_out,
                          int32_t *pair_min_out, double *end_clearance_out, double *q_min_out /*[na] or NULL*/);
/* The same two with the per-state distances of mopa_proximity_exact_batch (the exact route above); everything else unchanged. */
int mopa_motion_clearance_exact_batch(MopaScene *scene, const double *qa_dev /*[N,na]*/, const double *qb_dev /*[N,na]*/,
                                      const double *qpos_env_dev /*[E,nq]*/, int64_t N, int64_t samples_per_env, double band,
                                      double *clearance_dev /*[N]*/, int32_t *n_states_dev /*[N]*/, int32_t *n_near_dev /*[N]*/,
                                      int32_t *k_min_dev /*[N]*/, double *t_min_dev /*[N]*/, int32_t *pair_min_dev /*[N]*/,
                                      double *end_clearance_dev /*[N]*/, double *q_min_dev /*[N,na] or NULL*/, void *stream);
int mopa_motion_clearance_exact(MopaScene *scene, const double *qpos_a_host /*[nq]*/, const double *qpos_b_host /*[nq]*/, double band,
                                double *clearance_out, int32_t *n_states_out, int32_t *n_near_out, int32_t *k_min_out, double *t_min_out,
                                int32_t *pair_min_out, double *end_clearance_out, double *q_min_out /*[na] or NULL*/);

/* ======================================================================================================
 * (BASELINE configs 3-5) batched KINEMATIC env.step for the three Sawyer obstacle envs --
 * the "env-steps/sec" half of the metric.  Restates what the reference envs compute around the physics:
 *   action scaling / desired joint state     `_step` of env/sawyer/sawyer_{push,lift,assembly}_obstacle.py
 *                                            (Lift: gripper target = gripper qpos + action[-1], sawyer.py:340-342)
 *   joint-limit clamp + episode bookkeeping  env/base.py:269-314
 *   reward / success                         sawyer_push_obstacle.py:71-104, sawyer_lift_obstacle.py:93-150,
 *                                            sawyer_assembly_obstacle.py:33-52
 *   observation (dict order)                 env/sawyer/sawyer.py:317-338 + the env's `_get_obs`
 * and REPLACES the physics (`_do_simulation`, 75 MuJoCo sub-steps of position servos) by its kinematic
 * limit: every actuated joint reaches its target clamped to the actuator's ctrlrange, velocities are zero,
 * nothing else moves (no contact forces: the manipulated object never moves).  NOT dynamics parity -- labelled as
 * such wherever it is reported.
 *
 * Frame / quat slots per kind (positions = world position of a point fixed in a body; quats = body orientations):
 *   all       frame 0 = site "grip_site";                           quat 0 = body "right_ee_attchment"
 *   PUSH      frames 1,2 = sites "right_eef","left_eef", 3 = body "cube", 4 = body "target";   quat 1 = "cube"
 *             obs[40]: common 25 + target_pos, cube_pos, cube_quat(xyzw), gripper_to_cube, cube_to_target
 *   LIFT      frames 1 = body "cube" (the can), 2 = body "bin1";                                 quat 1 = "cube"
 *             obs[35]: common 25 + cube_pos, cube_quat(xyzw), gripper_to_cube;  action[8] = 7 arm + gripper
 *             grasp test (`has_grasp`): touch geoms [can mesh, left-finger boxes..., right-finger boxes...]
 *   ASSEMBLY  frames 1..4 = sites "hole","hole_bottom","pegHead","pegEnd";                     quat 1 = "peg"
 *             obs[38]: common 25 + hole, pegHead, pegEnd, peg_quat(wxyz)
 *   common 25 = joint_pos 7, joint_vel 7 (0), gripper_qpos 2, gripper_qvel 2 (0), eef_pos 3, eef_quat 4 (xyzw)
 *   PUSHER    PusherObstacle-v0 (env/pusher/pusher_obstacle.py:183-274; BASELINE config 1's env, joint0 unlimited): four hinges under
 *             torque motors driven by the env's PID loop (env/base.py:200-209); kinematic limit: the joints reach
 *             desired_state = prev + action -- the action UNSCALED and UNCLIPPED, as the reference's `_step` leaves it (:262-266);
 *             the joint-limit clamp comes after reward / obs.  frames 0 = site "fingertip", 1 = body "fingertip", 2 = body "box",
 *             3 = body "target"; quats = "fingertip", "box" (unused); n_grip 0.
 *             obs[20]: cos(theta) 4, sin(theta) 4, box qpos 2 (= qpos[nq-2:]), joint vel 4 (0), box vel 2 (0), fingertip xy 2,
 *             goal 2 (= qpos[nq-4:nq-2]);  reward: 0.1 (1 - tanh 5 d_tip_box) [d < 0.1] + 0.3 (1 - tanh 5 d_box_target) [d < 0.1],
 *             success: d_box_target < distance_threshold (config/pusher.py: 0.05)
 * ====================================================================================================== */
#define MOPA_ENV_PUSH 0
#define MOPA_ENV_LIFT 1
#define MOPA_ENV_ASSEMBLY 2
#define MOPA_ENV_PUSHER 3
#define MOPA_ENV_OBS_DIM 40      /* largest observation (PUSH); see mopa_env_obs_dim */

typedef struct MopaEnvDesc {
    MopaModel model;                 /* body / joint arrays; LIFT also reads the touch geoms and the can's hull */
    int32_t kind;                    /* MOPA_ENV_* */
    int32_t n_arm;                   /* env.ref_joint_pos_indexes (7) */
    const int32_t *arm_qpos_idx;
    int32_t n_grip;                  /* env.ref_gripper_joint_pos_indexes (2) */
    const int32_t *grip_qpos_idx;
    int32_t n_act;                   /* position actuators written by `_do_simulation`, ctrl order: the arm's n_arm, then (LIFT) 2 gripper */
    const int32_t *act_qpos_idx;     /* [n_act] qpos address of the actuated joint */
    const double *act_ctrl_lo;       /* [n_act] ctrlrange (-inf / +inf when not ctrllimited) */
    const double *act_ctrl_hi;
    int32_t n_frames;                /* 5 (PUSH, ASSEMBLY), 3 (LIFT) or 4 (PUSHER), slots as listed above */
    const int32_t *frame_body;       /* [n_frames] */
    const double *frame_off;         /* [n_frames,3] offset in the body frame (site position; 0 for a body frame) */
    int32_t n_quats;                 /* 2 */
    const int32_t *quat_body;
    int32_t n_touch;                 /* LIFT: 1 + left + right collidable-geom indices (into model.geom_*), else 0 */
    const int32_t *touch_geom;
    int32_t n_touch_left;
    const double  *qpos_min;         /* [nq] per-qpos joint limits: _jnt_minimum[jnt_indices] (env/base.py:62-88) */
    const double  *qpos_max;         /* [nq] */
    const int32_t *qpos_limited;     /* [nq] */
    double ac_scale;                 /* config/sawyer.py (0.05) */
    double distance_threshold;       /* PUSH: 0.06 */
    double success_reward;           /* 150 */
    int32_t max_episode_steps;       /* 250 */
    int32_t device;                  /* HIP device ordinal, -1 = current */
} MopaEnvDesc;

typedef struct MopaEnv MopaEnv;

int mopa_env_create(const MopaEnvDesc *desc, MopaEnv **out);
void mopa_env_destroy(MopaEnv *env);
int mopa_env_obs_dim(const MopaEnv *env);      /* 40 / 35 / 38 / 20 */
int mopa_env_action_dim(const MopaEnv *env);   /* n_arm (+1 for LIFT) */

/* One step of E envs (all pointers device, f64 unless noted).  Per env e:
 *   prev = (is_planner && has_prev[e]) ? prev_state[e] : qpos[e, arm]
 *   desired = prev + clip(is_planner ? action[e, :n_arm] : action[e, :n_arm]*ac_scale, -ac_scale, +ac_scale)
 *   (PUSHER: desired = prev + action[e, :n_arm])
 *   LIFT: gripper targets = qpos[e, gripper] + action[e, n_arm]
 *   move_mask[e] (NULL = 1): bit 1 set -> env e sits this call out entirely (nothing read or written);
 *   bit 0 set -> every actuated joint = its target clamped to ctrlrange (kinematic servo); bit 0 clear -> the command is
 *   recorded but nothing moves
 *   prev_state[e] = desired, has_prev[e] = 1; limited qpos entries clipped to their range
 *   FK -> reward, success, obs; ep_len[e] += 1; done[e] = success || ep_len[e] == max_episode_steps
 * action == NULL: no step, only FK -> obs (reward/done/success untouched; used after a reset). */
int mopa_env_step_batch(MopaEnv *env, int64_t E, double *qpos_dev /*[E,nq] in/out*/, double *prev_state_dev /*[E,n_arm] in/out*/,
                        uint8_t *has_prev_dev /*[E] in/out*/, int32_t *ep_len_dev /*[E] in/out*/,
                        const double *action_dev /*[E,action_dim] or NULL*/, int32_t is_planner,
                        const uint8_t *move_mask_dev /*[E] or NULL*/, double *obs_dev /*[E,obs_dim]*/,
                        double *reward_dev /*[E]*/, uint8_t *done_dev /*[E]*/, uint8_t *success_dev /*[E]*/, void *stream);

/* Waypoint execution of the rollout runner (rl/mopa_rollouts.py:152-199) for E envs in ONE launch: env e steps through
 * traj[e, 0 .. path_len[e]-1] (full qpos rows; the action of step k is env.form_action(waypoint) = waypoint - current arm
 * state, is_planner semantics of mopa_env_step_batch) until its path ends or a step reports done, with
 *   smdp_rew[e] += disc_pow[k] * reward_k   (disc_pow[k] = discount_factor^k, supplied by the caller),
 *   smdp_done[e] = done_k, intra[e] = k for the last step taken.  Envs with path_len[e] == 0 are not touched.
 * last_extra (LIFT; NULL otherwise): the policy's gripper action, used as the gripper entry of the LAST waypoint's action
 * (:163-167); earlier waypoints use form_action's gripper difference.
 * rec_* (all four or none): per executed waypoint the obs after the step, the running return and the done flag, and
 * n_exec[e] = steps taken -- the reference's ob_list / meta_rew_list / done_list (input of its reuse_data relabelling).
 * obs / reward / done / success hold the env's last step afterwards, exactly as after that many mopa_env_step_batch calls. */
int mopa_env_exec_batch(MopaEnv *env, int64_t E, double *qpos_dev /*[E,nq] in/out*/, double *prev_state_dev /*[E,n_arm] in/out*/,
                        uint8_t *has_prev_dev /*[E] in/out*/, int32_t *ep_len_dev /*[E] in/out*/,
                        const double *traj_dev /*[E,L,nq]*/, const int64_t *path_len_dev /*[E]*/, int32_t L,
                        const double *disc_pow_dev /*[L]*/, const double *last_extra_dev /*[E] or NULL*/,
                        double *obs_dev /*[E,obs_dim]*/, double *reward_dev /*[E]*/,
                        uint8_t *done_dev /*[E]*/, uint8_t *success_dev /*[E]*/, double *smdp_rew_dev /*[E] in/out*/,
                        uint8_t *smdp_done_dev /*[E] in/out*/, int64_t *intra_dev /*[E] in/out*/,
                        double *rec_ob_dev /*[E,L,obs_dim] or NULL*/, double *rec_rew_dev /*[E,L] or NULL*/,
                        uint8_t *rec_done_dev /*[E,L] or NULL*/, int64_t *n_exec_dev /*[E] or NULL*/, void *stream);

/* ---- servo dynamics inside env.step (stage A: contact-free) ----------------------------------------
 * Replaces the kinematic limit of `_do_simulation` by what the reference runs when the robot touches nothing: nsub = 75
 * sub-steps of { qfrc_applied[arm] = qfrc_bias[arm]; ctrl = desired_state (+ LIFT gripper targets); mj_step } per env.step
 * (env/sawyer/sawyer_push_obstacle.py:186-203, sawyer_lift_obstacle.py:218-236, sawyer_assembly_obstacle.py:121-139,
 * env/base.py:388-392) on the arm's own tree, [3P] MuJoCo 2.0's pipeline restated: composite-rigid-body inertia + armature,
 * RNE bias (gravity included), joint damping integrated implicitly by the Euler step, position servos
 * force = clamp(kp ctrl - kp q, forcerange) (env/assets/xml/common/sawyer_joint_pos_act.xml, gripper_pick_pos_act.xml),
 * timestep 0.002 (sawyer_dependencies.xml:11).  NOT modelled: contacts (manipulated objects do not move), the solver's soft
 * joint-limit constraint (an inelastic stop at the range instead).  The tree is passed LUMPED -- one body per dof, bodies
 * welded to it folded into its inertial (mopa_rl_amd/dynamics.py) -- parents before children, at most 9 dofs. */
/* Stage B (Push): the manipulated object as a free rigid body with PENALTY contacts -- spring-damper normal force and
 * capped regularised Coulomb friction at the object's feature points found inside a collider (and a moving box collider's
 * vertices found inside the object); one-way coupling (the robot moves the object; its reaction on the arm is neglected).
 * NOT MuJoCo's solver (soft convex constraints + elliptic cones + noslip, sawyer_dependencies.xml:11): a labelled stand-in
 * so that env/sawyer/sawyer_push_obstacle.py's task has an object that can be pushed.  Colliders = the geoms MuJoCo pairs
 * with the object (candidate-pair list): static ones (body -1, pose in the world) first, then robot geoms sorted by their
 * dynamic body (pose in that body's frame).  With an object the qvel rows are [nd + 6]: the dofs, then (v, w) world. */
typedef struct MopaObjDesc {
    int32_t qadr;                     /* qpos address of the free joint (pos 3, quat 4); COM = body origin */
    double mass, inertia[3], damping; /* principal inertia in the body frame, free-joint damping */
    double half[3], rbound;           /* box half extents, bounding radius */
    int32_t nfeat; const double *feat;   /* [nfeat,3] feature points (body frame), the 8 vertices first */
    int32_t ncol;
    const int32_t *co_body, *co_type; /* [ncol] dynamic body (-1 static), mjtGeom type (plane / sphere / capsule / cylinder / box) */
    const double *co_size, *co_pos, *co_mat, *co_mu, *co_rbound;   /* [n,3] [n,3] [n,9] [n] [n] */
    double inv_mass, inv_inertia[3];  /* reciprocals (the integrator multiplies) */
    int32_t precull_every;            /* the full collider scan runs on every precull_every-th sub-step of a call (15) ... */
    double precull_margin;            /* ... with bounding spheres inflated by this much (0.15 m); other sub-steps visit its survivors */
    double kn, dn, eps_v, ct_max;     /* normal stiffness, normal damping, friction regularisation, cap of the friction's viscous coefficient */
} MopaObjDesc;

typedef struct MopaDynDesc {
    int32_t nd;
    const int32_t *parent;            /* [nd] parent dynamic body, -1 = fixed base */
    const int32_t *jtype;             /* [nd] 2 slide, 3 hinge */
    const int32_t *qadr;              /* [nd] qpos address of the dof */
    const double *rel_pos;            /* [nd,3] body frame in its parent dynamic body's frame (base: world) */
    const double *rel_quat;           /* [nd,4] wxyz */
    const double *axis, *jpos, *qref; /* [nd,3] [nd,3] [nd] joint axis / anchor (body frame), reference value */
    const double *mass, *ipos;        /* [nd] [nd,3] lumped mass, centre of mass (body frame) */
    const double *inertia;            /* [nd,6] about the COM, body axes: xx yy zz xy xz yz */
    const double *damping, *armature; /* [nd] */
    const int32_t *limited;           /* [nd] */
    const double *lo, *hi;            /* [nd] joint range */
    const int32_t *actuated;          /* [nd] must agree with the env's actuator list (MopaEnvDesc.act_qpos_idx) */
    const double *kp, *force_lo, *force_hi;   /* [nd] servo gain, force range (-inf / +inf when not forcelimited) */
    const int32_t *gravcomp;          /* [nd] the env copies qfrc_bias into qfrc_applied for this dof (the arm's joints) */
    double gravity[3];
    double timestep;                  /* 0.002 */
    int32_t nsub;                     /* int(frame_dt / timestep) = 75 */
    const MopaObjDesc *obj;           /* NULL: stage A (only the robot moves) */
} MopaDynDesc;
int mopa_env_attach_dynamics(MopaEnv *env, const MopaDynDesc *desc);
/* The dofs are listed parents first (MOPA_ERR_INVALID_ARG) and in depth-first order, as the bodies of a MopaModel are (MOPA_ERR_UNSUPPORTED).
 * A failed attach leaves the env as it was.
 *
 * The host halves of mopa_env_create and of mopa_env_create + mopa_env_attach_dynamics alone, no device needed: the status code the
 * creation would refuse the description with, and for an accepted one the FNV-1a fingerprint of the tables it would upload (header,
 * double table, int table / header, dof records, object table), the walk's body count and its pose save slots.  Outputs may be NULL. */
int mopa_env_tables_host(const MopaEnvDesc *desc, uint64_t *fingerprint, int32_t *nb, int32_t *n_save);
int mopa_dyn_tables_host(const MopaEnvDesc *env_desc, const MopaDynDesc *desc, uint64_t *fingerprint, int32_t *n_save);
/* (stage C) contacts of the arm, of the manipulated object (Push: cube, Lift: can, Assembly: furniture; a
 * free rigid body) and between the two, two-way coupled behind ONE soft-constraint solve per sub-step.  Replaces, inside
 * `sim.step()` of the reference's `_do_simulation` loop (env/sawyer/sawyer_push_obstacle.py:186-203, sawyer_lift_obstacle.py:
 * 218-236, sawyer_assembly_obstacle.py:121-139; options env/assets/xml/common/sawyer_dependencies.xml:11), [3P] MuJoCo 2.0's
 * mj_collision + mj_makeConstraint + the constraint solver + mj_Euler.  RESTATED FROM THE PUBLISHED SOLVER, PARITY UNPINNED:
 * soft constraints with solref / solimp impedance; the default pipeline (`solver` 2) is the XML's: ELLIPTIC friction cones
 * (`cone="elliptic"`, condim 3: MuJoCo's primal elliptic-cone cost) in the Newton solver (the XML names no solver = MuJoCo's
 * default) with `iterations="50"` / `tolerance="1e-10"`, then the noslip pass (`noslip_iterations="5"`: friction re-solved
 * without the regulariser inside the friction disc), joint limits as solver rows (`limit_rows`).  Selectable: Newton with
 * pyramidal cones (`solver` 1), projected Gauss-Seidel with pyramidal cones (`solver` 0).  Not restated: torsional / rolling
 * friction (condim 4 / 6 pairs are solved as condim 3), MuJoCo's own pair functions (see "Collision geometry").
 * obj_qadr < 0 (with np = 0, limit_rows = 0): NO contact stage and no object -- the contact-free servo dynamics of stage A in this
 * kernel's 16-lanes-per-env mapping (qvel rows stay [nd]).
 * Collision geometry: sampled feature points of one geom in the exact signed-distance function of the other (plane, sphere,
 * capsule, cylinder, box; the can as the bounding cylinder of its hull).
 * Bodies: 0 .. nd-1 the lumped dynamic bodies of the arm, nd the object, -1 the world.  Shapes are posed in the frame of
 * their body, features likewise.  A directed pair (F, S) tests the features of shape F in the distance function of shape S;
 * pr_par rows: mu, margin, K, B, d0, dmax, width, 0 (MuJoCo's per-pair mix of friction / margin / solref / solimp, formed on
 * the host).  Call after mopa_env_attach_dynamics (without MopaObjDesc); qvel rows become [nd + 6]: the dofs, then the
 * object's (velocity of its COM, angular velocity) in the world. */
#define MOPA_CT_MAXCON 16      /* contacts kept per env and sub-step: <= 16 (solver 0, 2: one contact per lane of an env's 16), <= 8 for solver 1 */
typedef struct MopaCtDesc {
    int32_t ns;
    const int32_t *sh_body, *sh_type;                       /* [ns] */
    const double *sh_size, *sh_pos, *sh_mat, *sh_rbound;    /* [ns,3] [ns,3] [ns,9] [ns] */
    const int32_t *sh_feat0;                                /* [ns + 1] */
    int32_t nf;
    const double *ft_pos, *ft_rad;                          /* [nf,3] [nf] */
    int32_t np;
    const int32_t *pr_f, *pr_s;                             /* [np] */
    const double *pr_par;                                   /* [np,12]: mu, margin, K, B, d0, dmax, width, -, condim (3 / 4 / 6), torsional friction,
                                                               rolling friction, - (solver 2 solves a pair with its condim; 0 / 1 as condim 3) */
    int32_t obj_qadr;                                       /* qpos address of the object's free joint */
    double obj_mass, obj_inertia[3], obj_ipos[3], obj_iquat[4], obj_damping;
    double obj_inv_mass, obj_inv_inertia[3], obj_inv_mass_d, obj_inv_inertia_d[3];
    int32_t maxcon, maxpair, iterations;
    double tolerance, inv_scale;
    int32_t precull_every;
    double precull_margin;
    int32_t near_every;              /* third culling level: active pairs within near_margin of contact, re-listed every near_every sub-steps */
    double near_margin;
    int32_t warmstart;
    int32_t solver;                  /* 2: Newton + elliptic cones (the XML's model; default of the Python host), 1: Newton + pyramidal cones,
                                        0: projected Gauss-Seidel + pyramidal cones */
    int32_t limit_rows;              /* joint limits as rows of the Newton solver (MuJoCo) instead of an inelastic stop (solver 1 / 2) */
    double lim_par[8];               /* their parameters in a pair record's layout: -, margin 0, K, B, d0, dmax, width, - */
    int32_t noslip_iterations;       /* sweeps of the noslip pass after the main solve (0 = none) */
    double noslip_tolerance;
    int32_t arena;                   /* solver 2: doubles of an env's LDS the (variable-size) contact records share; a contact whose record does not
                                        fit is dropped like one beyond maxcon.  0 = what keeps four waves on a CU (mopa_env_contact_arena tells) */
} MopaCtDesc;
int mopa_env_attach_contacts(MopaEnv *env, const MopaCtDesc *desc);
int mopa_ct_desc_size(void);           /* sizeof(MopaCtDesc) as the library was built (binding self-check) */
int mopa_env_contact_arena(const MopaEnv *env);   /* the arena (doubles per env) the attached contact stage runs with; -1 without one */
/* per-env counters of the last stepping launch: [E,4] int32 = contacts summed over the sub-steps, solver sweeps summed,
 * contacts dropped by the caps, largest contact count of a sub-step (NULL: not recorded) */
int mopa_env_set_contact_stats(MopaEnv *env, int32_t *stats_dev);
int mopa_env_dyn_dofs(const MopaEnv *env);      /* nd, or -1 without dynamics */
int mopa_env_dyn_qvel_width(const MopaEnv *env); /* nd (+ 6 with an object), or -1 */
/* waves that share 64 envs in a servo-dynamics launch of this env: 4 (the workgroup form), or 1 -- a tree in which two bodies park
 * their pose in one save slot (parent = -1 0 1 1 0 4 4), or MOPA_DYN_KERNEL=wave in the environment; -1 without dynamics */
int mopa_env_dyn_waves(const MopaEnv *env);
/* mj_forward at (qpos, qvel): bias [E,nd] <- qfrc_bias (what the env reads as gravity compensation before its next
 * sub-step; call after a reset / set_state with qvel = 0); M (optional) <- packed lower triangle of the joint-space
 * inertia [E, nd (nd + 1) / 2]; mask (optional): envs with bit 1 set are skipped. */
int mopa_env_dyn_forward_batch(MopaEnv *env, int64_t E, const double *qpos_dev /*[E,nq]*/, const double *qvel_dev /*[E,nd]*/,
                               double *bias_dev /*[E,nd]*/, double *M_dev /*or NULL*/, const uint8_t *mask_dev /*[E] or NULL*/,
                               void *stream);
/* n sub-steps towards explicit (ctrl-range clamped) servo targets ctrl [E,nd] (entries of unactuated dofs ignored) */
int mopa_env_dyn_substeps_batch(MopaEnv *env, int64_t E, double *qpos_dev /*[E,nq] in/out*/, double *qvel_dev /*[E,nd] in/out*/,
                                double *bias_lag_dev /*[E,nd] in/out*/, const double *ctrl_dev /*[E,nd]*/, int32_t n, void *stream);
/* mopa_env_step_batch with the servo dynamics as `_do_simulation`: same arguments and bookkeeping, plus the carried
 * qvel / bias_lag [E,nd]; move_mask bit 0 clear -> the command is recorded, no sub-step runs.  The obs reports joint_vel /
 * gripper_qvel, and -- as in the reference -- reward and obs are taken BEFORE the joint-limit clamp of env/base.py:269-290.
 * action == NULL: obs refresh only (qvel is read for the obs). */
int mopa_env_step_dyn_batch(MopaEnv *env, int64_t E, double *qpos_dev, double *qvel_dev, double *bias_lag_dev, double *prev_state_dev,
                            uint8_t *has_prev_dev, int32_t *ep_len_dev, const double *action_dev, int32_t is_planner,
                            const uint8_t *move_mask_dev, double *obs_dev, double *reward_dev, uint8_t *done_dev,
                            uint8_t *success_dev, void *stream);

/* ---- K8: PusherObstacle-v0 dynamics (mopa_pusher_dyn.inc) ----------------------------------------------------------------
 * `PusherObstacleEnv._step` (env/pusher/pusher_obstacle.py:245-279): the env's PID loop (env/base.py:200-209) sets the four
 * velocity actuators (pusher_gripper.xml:123-126) before each of nsub = int(frame_dt / timestep) sub-steps of MuJoCo 2.0's RK4
 * integrator (pusher_gripper.xml:7), restated in the plane: dofs joint0..3 (hinges about z) and box_x / box_y (slides); contacts
 * (planar capsule-box, capsule-capsule, box-box) and joint limits as soft-constraint rows solved by Newton with pyramidal cones.
 * PARITY UNPINNED.  qvel rows are [6] in dof order; i_term [E,4] is the PID's integral term, owned by
 * the caller (zeroed at reset).
 * Pair records: [npair, 20] doubles = class (0 capsule-box, 1 capsule-capsule, 2 box-box), body A, body B (-1 world, 0..3 arm
 * bodies, 4 the box), geom A [5], geom B [5] (capsule: end 0 xy, end 1 xy, radius; box: centre xy, half sizes xy, 0; in the
 * body's frame), mu, margin, K, B, d0, dmax, width. */
#define MOPA_PUSHER_MAXCON 16   /* contacts kept per env and forward pass at most */
typedef struct MopaPusherDynDesc {
    int32_t qadr[6];                  /* qpos addresses of joint0..3, box_x, box_y */
    int32_t limited[6];
    double lo[6], hi[6];
    double armature[6], damping[6];
    double base[2];                   /* joint0's anchor in the world (xy) */
    double rel[8];                    /* [4,2] anchor of arm body k in the frame of body k - 1 (entry 0 unused) */
    double mass[4], com[8], izz[4];   /* lumped arm bodies: mass, centre of mass [4,2] in the body frame, inertia about z at the COM */
    double box_mass, box_org[2], box_ref[2];
    double gear[4], kv[4], ctrl_lo[4], ctrl_hi[4];
    double kp, kd, ki, alpha;         /* PID gains (config/pusher.py:40-46) and the integral's decay 0.95 */
    double frame_dt, timestep;
    int32_t nsub;                     /* int(frame_dt / timestep) = 100 */
    int32_t iterations;               /* Newton iterations (MuJoCo's default 100) */
    double tolerance, inv_scale;      /* stop when (cost decrease) * inv_scale < tolerance (1e-8) */
    double lim_par[8];                /* joint-limit rows: -, margin, K, B, d0, dmax, width, - */
    int32_t maxcon;                   /* <= MOPA_PUSHER_MAXCON */
    int32_t npair;                    /* 0: no contact stage (the arm alone) */
    const double *pairs;              /* [npair, 20] */
} MopaPusherDynDesc;
int mopa_pusher_dyn_desc_size(void);  /* sizeof(MopaPusherDynDesc) as the library was built (binding self-check) */
int mopa_env_attach_pusher_dynamics(MopaEnv *env, const MopaPusherDynDesc *desc);
/* per-env counter of the stepping / sub-step launches that follow: [E] int32 = contacts dropped by the cap (NULL: off) */
int mopa_env_set_pusher_stats(MopaEnv *env, int32_t *stats_dev);
/* n raw sub-steps (PID + RK4) towards desired [E,4] with prev_state [E,4] as the PID's prev; qpos, qvel [E,6], i_term in/out */
int mopa_env_pusher_substeps_batch(MopaEnv *env, int64_t E, double *qpos_dev, double *qvel_dev, double *i_term_dev,
                                   const double *desired_dev, const double *prev_state_dev, int32_t n, void *stream);
/* mopa_env_step_batch with the Pusher dynamics as `_do_simulation`: same arguments and bookkeeping, plus qvel [E,6] and i_term
 * [E,4]; move_mask bit 0 clear -> the command is recorded, no sub-step runs.  action == NULL: obs refresh only. */
int mopa_env_step_pusher_batch(MopaEnv *env, int64_t E, double *qpos_dev, double *qvel_dev, double *i_term_dev, double *prev_state_dev,
                               uint8_t *has_prev_dev, int32_t *ep_len_dev, const double *action_dev, int32_t is_planner,
                               const uint8_t *move_mask_dev, double *obs_dev, double *reward_dev, uint8_t *done_dev,
                               uint8_t *success_dev, void *stream);

/* ---- contact-force readout of the solver-backed contact stages (K7: mopa_env_attach_contacts, K8: mopa_env_attach_pusher_dynamics) ----
 * `env.get_contact_force()` (env/base.py:568-581: sum over the contacts of sum_k |mj_contactForce(i)[k]|, read from the constraint forces
 * the last sub-step of `_do_simulation` left), for the launches that follow -- env.step and the raw sub-step entry points alike.  After the
 * last sub-step of a launch, for every env that ran a sub-step in it (the others keep their values):
 *   rows [E,K,8]  per contact of the launch's last constraint solve (K7: the solve of the last sub-step; K8: the 4th RK4 stage of the last
 *                 sub-step): pair (index into pr_f / pr_s resp. the Pusher pair records), key (K7: feature index, K8: signed distance),
 *                 f0 .. f5 = mj_contactForce in the contact frame (elliptic cones: the contact's dim solver forces, zero-padded; pyramidal
 *                 cones with edge forces p: f0 = (p0 + p1) + (p2 + p3), f1 = mu (p0 - p1), f2 = mu (p2 - p3)); joint-limit rows are no contacts
 *   force [E]     sum over the contacts, in contact order, of ((((|f0| + |f1|) + |f2|) + |f3|) + |f4|) + |f5| -- plain adds: the host
 *                 reproduces it from the rows bit for bit
 *   total [E]     += force (the caller's accumulator: a rollout's per-episode sum)
 *   count [E]     contacts
 * All pointers NULL: off.  MOPA_ERR_INVALID_ARG: rows with K below the stage's maxcon; an env without such a stage (kinematic, servo
 * dynamics alone, the penalty-contact object); force NULL with another pointer set.  The contact-free 16-lane form reports zeros.
 * PARITY UNPINNED against MuJoCo, like the solves it reads. */
int mopa_env_set_contact_force(MopaEnv *env, double *force_dev /*[E]*/, double *total_dev /*[E] in/out, or NULL*/,
                               double *rows_dev /*[E,K,8] or NULL*/, int32_t *count_dev /*[E] or NULL*/, int32_t K);

/* ---- bookkeeping of one batched rollout call (rl/mopa_rollouts.py:70-375 + rl/sac_agent.py:148-318 for E envs at once) -------------
 * The elementwise work of mopa_rl_amd/rollout.py::BatchMoPARollout.agent_step between the library's launches, as six
 * one-wave-per-env kernels (mopa_rollstep.inc names the stages).  All pointers are device buffers; bool buffers are bytes. */
typedef struct MopaRolloutStep {
    int64_t E;
    int32_t nq, n_arm, ac_dim, ac_stride, adim, obs_dim, K /* width of the straight-line pre-check: traj is [E, K+1, nq] */;
    int32_t discrete, normal_space;
    double omega, ac_scale, action_range, omega_over_scale, one_minus_omega, range_minus_scale;
    const double *lim_lo, *lim_hi, *lo_state, *hi_state, *lo_shrunk, *hi_shrunk, *safe_q;              /* [nq] */
    /* the env's buffers */
    const double *qpos, *obs, *reward;
    const uint8_t *done, *success;
    uint8_t *has_prev;
    /* the rollout's persistent state */
    uint8_t *busy, *pool_mask, *interp_overflow;
    int64_t *wait_since, *t_dev, *t_env, *pend_type;
    double *q_cur, *q_tgt, *pend_ob, *pend_ac;
    int64_t *c_rl, *c_interp, *c_mp_fail, *c_invalid;
    /* this call's inputs */
    const double *ac;                  /* [E, ac_stride] policy output */
    const int64_t *ac_type_in;         /* [E] (discrete) */
    const double *a_in;                /* [E, n_arm] joint displacement action from the IK (use_ik_target) or NULL */
    /* this call's buffers */
    double *prev_ob, *ac_tr, *a, *extra_ac, *target, *cur_m, *cur_v, *tgt_v, *traj;
    uint8_t *active, *is_pl, *pv, *plan_ok;
    int64_t *ac_type, *path_len;
    const uint8_t *tv, *ok;            /* target valid (after the pull-back); pre-check verdict */
    const int32_t *nst, *tlen;         /* pre-check: steps needed, trajectory length */
    const uint8_t *finished;           /* [E] envs whose planner query was picked up in this call, or NULL */
    double *act0;                      /* [E, adim] */
    uint8_t *flags, *sitting, *stepped, *is_pl_out;
    int64_t *plen_m;
    double *last_extra;                /* [E] or NULL */
    double *rew;
    uint8_t *done_out;
    int64_t *intra;
    double *ob_next;
    uint8_t *success_out;
    const uint8_t *retry_mask;         /* [E] envs waiting for a retry launch, or NULL */
    int64_t *pool_counts;              /* [2] <- number of set entries of pool_mask / retry_mask after the call, or NULL */
} MopaRolloutStep;
int mopa_rollout_stage(const MopaRolloutStep *step, int32_t stage /*0..5*/, void *stream);
int mopa_rollout_step_size(void);      /* sizeof(MopaRolloutStep) as the library was built (binding self-check) */
/* The planner's pick-up of the waiting envs (rl/mopa_rollouts.py:205-209 for E envs: the envs whose straight line is blocked get an RRT-Connect
 * query), one launch: out_count[0] <- number of set bytes of mask [E]; if min_n <= that <= cap: their indices ascending -> out_ids, rows of q_cur / q_tgt
 * [E,nq] -> out_cur / out_tgt [cap,nq], t_env[ids] -> out_steps, t_env[ids] + seed -> out_seeds, and the mask bytes are cleared; otherwise nothing
 * else is written (below min_n the pool waits; above cap the caller chooses which envs go first).  All buffers on the device; bool buffers are bytes. */
int mopa_rollout_pool_pick(int64_t E, int32_t nq, int64_t min_n, int64_t cap, uint8_t *mask_dev, const double *q_cur_dev, const double *q_tgt_dev,
                           const int64_t *t_env_dev, int64_t seed, int64_t *out_ids_dev, double *out_cur_dev, double *out_tgt_dev,
                           int64_t *out_steps_dev, int64_t *out_seeds_dev, int64_t *out_count_dev, void *stream);
/* The `reuse_data` relabelling (rl/mopa_rollouts.py:222-300; mopa_rl_amd/rollout.py::reuse_transitions is the host form and the reference
 * of this one) on the record of one agent step, for E envs, three launches on `stream`, no read-back: every env with n_exec > 3 (and
 * env_mask != 0, when a mask is given) turns up to R = max_reuse_data (1..64) (start, goal) waypoint pairs into transitions
 *     ob[start] -- displacement_to_action(waypoint[goal,:n_arm] - waypoint[start,:n_arm]) [, waypoint[goal,g] - waypoint[start,g]] --> ob[goal],
 *     rew = (meta_rew[goal] - meta_rew[start]) * inv_disc[start], done = done[goal], intra = goal - start - 1,
 * kept iff some arm entry of the action lies beyond +-omega and every entry inside [-1, 1]; a pair equal to an earlier pair of its env is skipped.
 *   record      ob [E,L,D], meta_rew [E,L], done [E,L] bytes, waypoint [E,L,nq], n_exec [E] int64 (values above L count as L);
 *               ac_type [E] or NULL; env_mask [E] bytes or NULL; grip_qpos_idx = g, or -1 (then dof = n_arm, else dof = n_arm + 1; dof <= 64)
 *   action map  ac_scale, omega, omega_over_scale = omega / ac_scale, c1 = (action_range - ac_scale) / (1 - ac_scale),
 *               c2 = (1 - ac_scale) / (1 - omega), action_range -- formed by the caller in doubles, used as they are; normal_space != 0:
 *               ac = displacement / action_range.  inv_disc [L]: discount_factor ** -(k + 1)
 *   pairs       [E,R,2] int32: draw i of env e is (start, goal); entries that are (-1,-1) or violate 0 <= start < goal < n_exec[e] emit nothing.
 *               NULL: draw i < min(n_exec[e], R) comes from the counter RNG, key (seed, stream 3 * env_id_total + env_id_base + e)
 *               (env_id_total 0: E), counters 2i and 2i + 1, through randint(low, high) = low + min(int(u * (high - low)), high - low - 1)
 *               as start = randint(0, n_exec - 1), goal = randint(start + 1, n_exec)
 *   outputs     count [1] <- transitions kept (the true number, also above cap); rows 0 .. min(count, cap) - 1, ordered by env, then draw:
 *               env, start, goal, intra [cap] int32, ac [cap,dof], rew [cap], done [cap] bytes, ob, ob_next [cap,D], ac_type [cap] (iff
 *               ac_type is given; cap = 0: the columns may be NULL).  Rows beyond them are not touched.  The order is computed (scan), not raced for: every run writes the same bytes.
 *   work        [2 * E] int64 scratch.
 * Argument errors (R outside 1..64, n_arm > dof, cap < 0, a NULL required buffer, inconsistent sizes) return MOPA_ERR_INVALID_ARG before
 * any launch. */
int mopa_reuse_batch(int64_t E, int32_t L, int32_t D, int32_t nq, int32_t n_arm, int32_t dof, int32_t grip_qpos_idx,
                     const double *ob_dev, const double *meta_rew_dev, const uint8_t *done_dev, const double *waypoint_dev,
                     const int64_t *n_exec_dev, const int32_t *ac_type_dev, const uint8_t *env_mask_dev,
                     double ac_scale, double omega, double omega_over_scale, double c1, double c2, double action_range, int32_t normal_space,
                     const double *inv_disc_dev, int32_t R, const int32_t *pairs_dev, uint64_t seed, int64_t env_id_base, int64_t env_id_total,
                     int64_t cap, int64_t *work_dev, int64_t *count_dev, int32_t *out_env_dev, int32_t *out_start_dev, int32_t *out_goal_dev,
                     double *out_ac_dev, double *out_rew_dev, uint8_t *out_done_dev, int32_t *out_intra_dev, double *out_ob_dev,
                     double *out_ob_next_dev, int32_t *out_ac_type_dev, void *stream);

/* The replay sink (the reference's rl/dataset.py as its trainer uses it: runner.run(every_steps=1), rl/trainer.py:280, so every stored rollout
 * holds ONE transition, the ring overwrites the oldest and RandomSampler, rl/dataset.py:51-84, draws uniformly over the stored transitions;
 * mopa_rl_amd/replay.py::DeviceReplayBuffer is the Python form).  All buffers on the device, nothing is read back.
 *   ring        [capacity, W] float32, W = 2 * D + A + 4; a row is  ob[D] | ac[A] | rew | done | intra_steps | ac_type | ob_next[D]  -- the width of a
 *               TransitionExchange record, with ac_type where that record has `stepped`.  Doubles are narrowed with (float)x (round to nearest
 *               even), integers and bytes converted exactly.
 *   state       [2] int64: state[0] = rows appended since creation, state[1] = min(state[0], capacity) = rows a sampler may draw.
 * mopa_replay_append selects rows of a source of n rows and writes them behind the ring's head, at most two launches on `stream` (n = 0: none):
 *   selection   mask [n] bytes: the rows with a non-zero byte, ascending; count [1] int64: rows 0 .. min(count, n) - 1 (a negative count keeps
 *               none); neither: all n rows; both: MOPA_ERR_INVALID_ARG.
 *   destination the k-th kept row goes to ring row (state[0] + k) % capacity; of m > capacity kept rows the first m - capacity are skipped, so no
 *               ring row is written twice in one call; then state[0] += m.  The order is computed (scan over the keep flags, 1024 at a time
 *               with a running carry), not raced for: every run writes the same bytes.
 *   source (a)  columns: ob [n,D], ac [n,ac_ld] (the first A entries of a row are taken; ac_ld >= A), rew [n] doubles, done [n] bytes, intra [n]
 *               int64 (intra_is_int64 != 0) or int32, ob_next [n,D], ac_type [n] int32 or NULL (stored as 0); packed = NULL
 *   source (b)  packed [n,W] float32 exchange records; column D + A + 3 (`stepped`) is the mask -- non-zero keeps the row --, the stored ac_type
 *               is 0; mask, count and every column pointer NULL
 *   work        [n + 2] int64 scratch.
 * mopa_replay_sample draws B * n_batches rows, one launch on `stream`: draw i takes u = uniform(key(seed, stream_id), counter draw_base + i) of the
 * counter RNG and the ring row min(int(u * size), size - 1) with size = state[1] read on the device -> out [B * n_batches, W], out_idx
 * [B * n_batches] int64.  size = 0: the rows are zero-filled and the indices are -1.  (draw_base by value: the caller keeps the counter.)
 * Argument errors (a NULL required buffer, capacity < 1, D < 1, A < 1, ac_ld < A, n < 0, B < 1, n_batches < 1, both a mask and a count, a
 * packed source next to a mask, a count or columns) return MOPA_ERR_INVALID_ARG before any launch. */
int mopa_replay_append(int64_t capacity, int32_t D, int32_t A, float *ring_dev, int64_t *state_dev, int64_t n,
                       const uint8_t *mask_dev, const int64_t *count_dev, const double *ob_dev, const double *ac_dev, int32_t ac_ld,
                       const double *rew_dev, const uint8_t *done_dev, const void *intra_dev, int32_t intra_is_int64,
                       const double *ob_next_dev, const int32_t *ac_type_dev, const float *packed_dev, int64_t *work_dev, void *stream);
int mopa_replay_sample(int64_t capacity, int32_t D, int32_t A, const float *ring_dev, const int64_t *state_dev, int64_t B, int64_t n_batches,
                       uint64_t seed, uint64_t stream_id, uint64_t draw_base, float *out_dev, int64_t *out_idx_dev, void *stream);

/* The arm state the NEXT mopa_env_step_batch call with the same arguments would reach (desired_state clamped to ctrlrange
 * and joint limits), without stepping: input of a collision gate (mopa_is_valid_batch with samples_per_env = 1 -> move_mask). */
int mopa_env_desired_batch(MopaEnv *env, int64_t E, const double *qpos_dev /*[E,nq]*/, const double *prev_state_dev /*[E,n_arm]*/,
                           const uint8_t *has_prev_dev /*[E]*/, const double *action_dev /*[E,action_dim]*/, int32_t is_planner,
                           double *desired_dev /*[E,n_arm]*/, void *stream);

/* ======================================================================================================
 *  batched damped-least-squares IK of a site pose: replaces
 * qpos_from_site_pose(env, site, target_pos, target_quat, joint_names=..., max_steps, tol, ...)   env/inverse_kinematics.py:18-135
 * with nullspace_method :274-281.  Per env and iteration:
 *   err_pos = target_pos - site_xpos;
 *   with an orientation target (:88-93): err_rot = mju_quat2Vel(target_quat * conj(mju_mat2Quat(site_xmat)), 1);
 *   err_norm = |err_pos| (+ rot_weight |err_rot|); success if err_norm < tol;
 *   J = [jacp; jacr] over the movable joints (hinge: axis x (p_site - anchor) / axis, slide: axis / 0) -- 3 x n for a
 *       position target, 6 x n with an orientation target (:38-44,101-105);
 *   dq = (J^T J + regularization_strength I)^-1 J^T err   (always regularised, as the reference calls it, :113-115);
 *   give up if err_norm / |dq| > progress_thresh; |dq| capped at max_update_norm; qpos[movable] += dq.
 * The reference's third mode (target_quat without target_pos) raises inside numpy (6-row Jacobian against a 3-vector)
 * and is not offered.  The linear solve is an unpivoted Cholesky factorisation (the reference uses LAPACK LU through
 * np.linalg.solve): equal to round-off (tests/golden/ref_py_ik.npz: 1e-12 on whole solves, equal step counts).
 * ====================================================================================================== */
typedef struct MopaIkDesc {
    MopaModel model;              /* body / joint arrays */
    int32_t n_joints;             /* movable joints, 1..8 */
    const int32_t *joint_ids;     /* [n_joints] model joint ids (hinge / slide, one per body), each at most once: a repeated id is
                                     refused with MOPA_ERR_INVALID_ARG (one of its two columns would stay zero) */
    int32_t site_body;            /* body carrying the site */
    double site_off[3];           /* site position in that body's frame */
    double site_quat[4];          /* site orientation in that body's frame, wxyz (all zero = identity) */
    int32_t device;               /* HIP device ordinal, -1 = current */
} MopaIkDesc;

typedef struct MopaIk MopaIk;

int mopa_ik_create(const MopaIkDesc *desc, MopaIk **out);
/* its host half alone (see mopa_env_tables_host): status, fingerprint of the tables, bodies on the site's chain */
int mopa_ik_tables_host(const MopaIkDesc *desc, uint64_t *fingerprint, int32_t *nb);
void mopa_ik_destroy(MopaIk *ik);
/* E independent IK problems; qpos rows are updated in place (IKResult.qpos); err_norm / steps / success as IKResult.
 * target_quat_dev NULL = position target only (rot_weight ignored). */
int mopa_ik_solve_batch(MopaIk *ik, int64_t E, double *qpos_dev /*[E,nq] in/out*/, const double *target_pos_dev /*[E,3]*/,
                        const double *target_quat_dev /*[E,4] wxyz or NULL*/, double rot_weight, int32_t max_steps, double tol,
                        double max_update_norm, double progress_thresh, double regularization_strength,
                        double *err_norm_dev /*[E]*/, int32_t *steps_dev /*[E]*/, uint8_t *success_dev /*[E]*/, void *stream);

/* World pose of the IK site for E states: site_pos [E,3], site_mat [E,9] row-major -- what the MoPA+IK rollouts read before
 * they pose the problem (env.sim.data.get_site_xpos / get_site_xmat(config.ik_target), rl/mopa_rollouts.py:91-99,692). */
int mopa_ik_site_pose_batch(MopaIk *ik, int64_t E, const double *qpos_dev /*[E,nq]*/, double *site_pos_dev /*[E,3]*/,
                            double *site_mat_dev /*[E,9]*/, void *stream);

/* The IK problem of the MoPA + IK action space for E envs (MoPARolloutRunner._cart2dispalcement, rl/mopa_rollouts.py:87-99,681-696):
 * target_cart = clip(site_pos + action_range * ac[:3], world box); target_quat (w, x, y, z) = mulQuat(q_site[(w, x, y, y)], ac[3:7] / |ac[3:7]|)
 * with q_site the quaternion of the float32-rounded site matrix (util/env.py:mat2quat, w >= 0).  ac rows are ac_stride (>= 7) doubles apart;
 * world_lo / world_hi: 3 HOST doubles each (env.min_world_size / max_world_size).  One launch, one lane per env. */
int mopa_ik_targets_batch(MopaIk *ik, int64_t E, const double *site_pos_dev /*[E,3]*/, const double *site_mat_dev /*[E,9]*/,
                          const double *ac_dev /*[E,ac_stride]*/, int64_t ac_stride, double action_range, const double *world_lo /*[3] host*/,
                          const double *world_hi /*[3] host*/, double *target_cart_dev /*[E,3]*/, double *target_quat_dev /*[E,4]*/, void *stream);

/* The position-only form of that problem: an env whose world box has n_cart = 2 or 3 entries and whose action carries no quaternion
 * (PusherObstacle-v0, scripts/2d/mopa_ik.sh; rl/trainer.py:93-110, rl/mopa_rollouts.py:91-98,684-690).  Components below n_cart:
 * clip(site_pos + action_range * ac, world box) -- a product, then a sum, then np.clip's comparisons; components at or above n_cart: the
 * site's own.  ac rows are ac_stride (>= n_cart) doubles apart; world_lo / world_hi: n_cart HOST doubles each.  One launch.
 * MOPA_ERR_INVALID_ARG before any launch: n_cart outside 2..3, a NULL buffer, E < 0, ac_stride < n_cart. */
int mopa_ik_targets_pos_batch(MopaIk *ik, int64_t E, const double *site_pos_dev /*[E,3]*/, const double *ac_dev /*[E,ac_stride]*/,
                              int64_t ac_stride, int32_t n_cart, double action_range, const double *world_lo /*[n_cart] host*/,
                              const double *world_hi /*[n_cart] host*/, double *target_cart_dev /*[E,3]*/, void *stream);

/* The whole pre-step of a position-only MoPA + IK rollout call (`_cart2dispalcement` with target_quat = None, rl/mopa_rollouts.py:683-728)
 * in ONE launch, one lane per env: site pose of qpos -> the target of mopa_ik_targets_pos_batch -> the position-only solve of
 * mopa_ik_solve_batch on the lane's own copy of the movable joints (qpos_dev is only read) -> clip of the movable joints to
 * jnt_lo / jnt_hi -> displacement = clipped - qpos[movable].  Bit for bit the composition of the separate launches
 * (site_pose, targets_pos, solve, elementwise maximum / minimum / subtraction).  err_norm_dev / steps_dev / success_dev (as IKResult)
 * may each be NULL.  Argument errors as above (plus max_steps <= 0), before any launch. */
int mopa_ik_displacement_pos_batch(MopaIk *ik, int64_t E, const double *qpos_dev /*[E,nq]*/, const double *ac_dev /*[E,ac_stride]*/,
                                   int64_t ac_stride, int32_t n_cart, double action_range, const double *world_lo /*[n_cart] host*/,
                                   const double *world_hi /*[n_cart] host*/, int32_t max_steps, double tol, double max_update_norm,
                                   double progress_thresh, double regularization_strength, const double *jnt_lo_dev /*[n_joints]*/,
                                   const double *jnt_hi_dev /*[n_joints]*/, double *displacement_dev /*[E,n_joints]*/,
                                   double *err_norm_dev /*[E] or NULL*/, int32_t *steps_dev /*[E] or NULL*/,
                                   uint8_t *success_dev /*[E] or NULL*/, void *stream);

/* The straight-line pre-check of SACAgent.plan / simple_interpolate (rl/sac_agent.py:198-204, 236-272) for E envs: the line
 * cur -> target is cut into int(s) equal steps, s = max(1, max_j |diff_j| / (0.8 ac_scale)) over the arm joints qpos[:n_arm]
 * (= the scene's active joints), each interior state a running sum from cur and validated (env row = cur); traj[e] = the
 * valid prefix of the walk followed by the exact target, traj_len[e] = its rows, ok[e] = 1 when no interior state was
 * invalid, n_steps[e] = int(s).  K (<= 64) is the fixed row capacity of the walk: callers pass an upper bound of int(s) and
 * check n_steps <= K.  cur must already be clipped (clip_qpos).  Three launches, no read-back. */
int mopa_interpolate_batch(MopaScene *scene, int64_t E, int32_t n_arm, int32_t K, const double *cur_dev /*[E,nq]*/,
                           const double *target_dev /*[E,nq]*/, double ac_scale, double *traj_dev /*[E,K+1,nq]*/,
                           int32_t *traj_len_dev /*[E]*/, uint8_t *ok_dev /*[E]*/, int32_t *n_steps_dev /*[E]*/, void *stream);

/* ===== planner paths -> executable trajectories (reference motion_planners/sampling_based_planner.py:71-99: un-wrap by
 * successive differences; rl/sac_agent.py:205-233: densification of long steps by simple_interpolate from the clipped
 * predecessor).  Three launches around one validity launch; no scene handle (pure arithmetic on caller buffers):
 *   mopa_paths_unwrap_batch    path rows [M, max_path, nq] as mopa_plan_batch wrote them are replaced IN PLACE by the
 *                              un-wrapped rows (row 0 = cur); seg_count[q, i] = interpolation steps of the segment
 *                              row i -> row i+1 (0 = no interpolation needed); n_walk[q] = sum of them; out_len[q] = rows of
 *                              the final trajectory (0 for queries with status != 0)
 *   mopa_paths_walk_batch      the interior states of all long segments, query after query at walk_off[q] (exclusive
 *                              prefix sum of n_walk) -> walk [sum n_walk, nq]; the caller validates them
 *                              (mopa_is_valid_batch on the rows' active columns, samples_per_env 1, rows as env rows)
 *   mopa_paths_assemble_batch  out [M, out_rows, nq]: per waypoint its interior states then the waypoint;
 *                              needs_fallback[q] = 1 when an interior state of q was invalid (the reference then plans
 *                              that segment with the simple / main planner, rl/sac_agent.py:300-306: left to the caller)
 * lo_state / hi_state / lo_shrunk / hi_shrunk [nq]: the agent's joint limits and limits +- joint_margin as the float32
 * arrays the reference holds them in (values widened to double; +-inf for unlimited coordinates) -- `clip_qpos`.
 * nq <= 64; arm coordinates are qpos[:n_arm]. */
int mopa_paths_unwrap_batch(int device, int64_t M, int32_t nq, int32_t n_arm, double *path_dev /*[M,max_path,nq] in/out*/,
                            int32_t max_path, const int32_t *path_len_dev /*[M]*/, const int32_t *status_dev /*[M]*/,
                            const double *cur_dev /*[M,nq]*/, double ac_scale, int32_t interpolate, const double *lo_state_dev,
                            const double *hi_state_dev, const double *lo_shrunk_dev, const double *hi_shrunk_dev,
                            int32_t *seg_count_dev /*[M,max_path]*/, int32_t *n_walk_dev /*[M]*/, int32_t *out_len_dev /*[M]*/,
                            void *stream);
/* the same with the seam rule of the reference's un-wrap loop for models with UNLIMITED joints (sampling_based_planner.py:79-97):
 * bit c of seam_mask marks qpos coordinate c as one of `non_limited_idx`; the planner's states live in (-3.14, 3.14) there
 * (SamplingBasedPlanner.convert_nonlimited -> util/env.py:joint_convert wraps start and goal before planning), and a step with
 * abs(state - pre_state) > 3.14 is taken the short way round: + (3.14 - pre + state + 3.14) when it left through +3.14,
 * - (3.14 - state + pre + 3.14) when through -3.14 (3.14, not pi; sums in this order).  seam_mask 0 == mopa_paths_unwrap_batch. */
int mopa_paths_unwrap_seam_batch(int device, int64_t M, int32_t nq, int32_t n_arm, double *path_dev /*[M,max_path,nq] in/out*/,
                                 int32_t max_path, const int32_t *path_len_dev /*[M]*/, const int32_t *status_dev /*[M]*/,
                                 const double *cur_dev /*[M,nq]*/, double ac_scale, int32_t interpolate, const double *lo_state_dev,
                                 const double *hi_state_dev, const double *lo_shrunk_dev, const double *hi_shrunk_dev,
                                 int32_t *seg_count_dev /*[M,max_path]*/, int32_t *n_walk_dev /*[M]*/, int32_t *out_len_dev /*[M]*/,
                                 uint64_t seam_mask, void *stream);
int mopa_paths_walk_batch(int device, int64_t M, int32_t nq, int32_t n_arm, const double *path_dev, int32_t max_path,
                          const int32_t *path_len_dev, const int32_t *out_len_dev, double ac_scale, const double *lo_state_dev,
                          const double *hi_state_dev, const double *lo_shrunk_dev, const double *hi_shrunk_dev,
                          const int32_t *seg_count_dev, const int64_t *walk_off_dev /*[M]*/, double *walk_dev /*[sum n_walk,nq]*/,
                          void *stream);
int mopa_paths_assemble_batch(int device, int64_t M, int32_t nq, const double *path_dev, int32_t max_path,
                              const int32_t *path_len_dev, const int32_t *out_len_dev, const int32_t *seg_count_dev,
                              const int64_t *walk_off_dev, const double *walk_dev /*nullable when no query has interior states*/,
                              const uint8_t *walk_valid_dev, double *out_dev /*[M,out_rows,nq]*/, int32_t out_rows,
                              uint8_t *needs_fallback_dev /*[M]*/, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MOPA_HIP_H */
