/*
 * tcmp.h -- C-ABI of the MI355X torque-constrained RRT* engine (libtcmp.so).
 *
 * Plain pointers and sizes only: every array argument is a HOST pointer owned by the caller,
 * row-major, fp64 configurations (7 per row), int32/int64 counts.  Every entry point returns
 * an int status (0 = ok, < 0 = error; tcmp_last_error() gives a thread-local message).
 * Calls are synchronous (the engine's stream is drained before return) unless noted.
 *
 * Each entry point names the reference interface it replaces
 * (HIRO-group/torque_constrained_motion_planning @ v0, src/...).
 */
#ifndef TCMP_H_
#define TCMP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct tcmp_handle tcmp_handle;
typedef struct tcmp_comm tcmp_comm;  /* multi-GPU communicator (tcmp_dist_init, below) */

/* torque_test modes, panda_primitives.py:228-236 */
#define TCMP_TORQUE_BASE 0 /* get_torque_limits_not_exceded_test_base   panda_primitives.py:13 */
#define TCMP_TORQUE_NOV 1  /* get_torque_limits_not_exceded_test_v3_nov panda_primitives.py:118 */
#define TCMP_TORQUE_RNE 2  /* get_torque_limits_not_exceded_test_v4     panda_primitives.py:155 */
#define TCMP_TORQUE_DYN 3  /* get_torque_limits_not_exceded_test_v2     panda_primitives.py:60
                              (M, C, g from rne.py's model: the reference's pdm is not shipped) */

/* plan status codes (tcmp_plan_result.status) */
#define TCMP_PLAN_OK 0            /* path found and validated (rrt_star.py:211) */
#define TCMP_PLAN_START_GOAL_COLLISION 1 /* rrt_star.py:152-154 */
#define TCMP_PLAN_NO_GOAL 2       /* rrt_star.py:199-201 */
#define TCMP_PLAN_VALIDATION_FAILED 3 /* rrt_star.py:208-210 */
#define TCMP_PLAN_MINJERK_ASSERT 4 /* min_jerk_v2.py:166 num_intervals == 0 */

/* ---- lifetime -------------------------------------------------------------------------- */
int tcmp_create(int device, tcmp_handle** out);
int tcmp_destroy(tcmp_handle* h);
const char* tcmp_last_error(void);
int tcmp_device_count(int* n);
int tcmp_version(void);
/* wait for all work queued on the handle's HIP stream */
int tcmp_synchronize(tcmp_handle* h);
/* profiling builds (-DTCMP_PROF) only: k_edges clock breakdown accumulated since create
 * (total, work fetch, collision, torque, bookkeeping, tier-4 exact, ...) and exact-test
 * outcome counts and mesh-stage clocks (12..35, then 44..51), the nearest scan's clocks and
 * visit counts (36..43), n <= 52; zeros otherwise. */
int tcmp_debug_counters(tcmp_handle* h, uint64_t* out, int32_t n);

/* Peak microbenchmarks on the handle's device (the spec peaks are re-measured
 * before use): out[0] fp64 vector FMA TFLOP/s, out[1] fp32 packed (v_pk_fma_f32) TFLOP/s,
 * out[2] HBM GB/s of a 1 GiB float4 device copy (read + write bytes), out[3] 0.  Best of five
 * launches each; allocates 2 GiB for the copy while it runs.  No reference counterpart. */
int tcmp_microbench(tcmp_handle* h, double* out);

/* Fixed obstacles (replaces Problem.fixed bodies + pybullet getClosestPoints,
 * utils.py:3165-3218 / 2833-2849).  n_obs oriented boxes, 15 doubles each:
 * centre(3), rotation R (9, row-major, columns = box axes, world frame), half extents(3). */
int tcmp_set_scene(tcmp_handle* h, const double* obb, int32_t n_obs);

/* Host only (no device): the interval tables the fused edge walk's first collision tier reads
 * for a scene of n_obs <= 32 boxes (as tcmp_set_scene takes them), viewed at `cells` = 64, 128
 * or 256 cells per axis.  tables [3][2][cells]: per axis, A[c] = bit mask of the boxes whose
 * shrunk world-AABB upper bound reaches cell c's lower edge, then B[c] = those whose lower bound
 * is at or below its upper edge.  bounds (may be NULL) [n_obs][8]: each box's fp32 bounds as the
 * tier compares them (hi x y z, 0, -lo x y z, 0).  grid (may be NULL) [4]: the first cell's lower
 * edge per axis, cells per metre.  No reference counterpart. */
int tcmp_tier0_tables(const double* obb, int32_t n_obs, int32_t cells, float* bounds,
                      uint32_t* tables, float* grid);

/* Host only: the obstacle mask of each of n link boxes [lo, hi] ([n][3] each, fp32) from
 * tcmp_tier0_tables' tables, computed as the device computes it. */
int tcmp_tier0_masks(const uint32_t* tables, int32_t cells, const float* lo, const float* hi,
                     int64_t n, uint32_t* masks);

/* Fixed convex-mesh obstacles (replaces pybullet GEOM_MESH bodies in Problem.fixed: Bullet
 * collides the convex hull of the mesh vertices, utils.py:2833-2880, closest points with
 * distance = -0.04).  All in the world frame; n_mesh hulls, rows of mesh m are
 * [off[m], off[m+1]) of each array (offsets start at 0):
 *   verts  V x 3            hull vertices
 *   planes F x 4            facet planes n.x <= d (unit outward n, d = max n.v)
 *   edges  E x 4 (int32)    hull edges: va vb (mesh-local vertex rows) f1 f2 (mesh-local
 *                           plane rows of the two adjacent facets)
 *   boxes  n_mesh x 18      outer box containing the hull: centre(3), R(9, columns = axes),
 *                           half(3); then the half extents (3) of a box with the same centre
 *                           and axes inside the hull (zeros = none)
 * Replaces the previous mesh set; boxes from tcmp_set_scene are kept (and vice versa).
 * Host-side hull construction: torque_constrained_motion_planning_amd/hull.py. */
int tcmp_set_meshes(tcmp_handle* h, const double* verts, const int32_t* vert_off,
                    const double* planes, const int32_t* plane_off, const int32_t* edges,
                    const int32_t* edge_off, const double* boxes, int32_t n_mesh);

/* A set of n hulls in tcmp_set_meshes' layout (world frame, rows [off[m], off[m+1])). */
typedef struct tcmp_hulls {
  const double* verts;        /* V x 3 */
  const int32_t* vert_off;    /* n + 1 */
  const double* planes;       /* F x 4: unit outward n, d */
  const int32_t* plane_off;
  const int32_t* edges;       /* E x 4: va vb f1 f2 (hull-local rows) */
  const int32_t* edge_off;
} tcmp_hulls;

/* Optional level-of-detail hulls for the current meshes (same count, call after
 * tcmp_set_meshes): inner[m] must lie inside mesh m's hull and outer[m] must contain it.
 * The kernels use them only as certificates before the exact test ("free" when the outer
 * hulls' depth is below 0.04 - 1e-4, "collision" when the inner hulls' depth exceeds
 * 0.04 + 1e-4), so results do not depend on them -- only speed.  hull.py builds them. */
int tcmp_set_mesh_lods(tcmp_handle* h, const tcmp_hulls* inner, const tcmp_hulls* outer,
                       int32_t n_mesh);

/* Optional inscribed spheres for the current meshes (call after tcmp_set_meshes; cleared by
 * it): spheres[n_mesh][k][4] = (cx, cy, cz, r), world frame, each ball inside mesh m's hull
 * (checked against the stored facet planes, n.c + r <= d + 1e-9; status -1 otherwise);
 * k must be 16.  Like the LODs they are certificates only (same reference semantics,
 * utils.py:2833 closest points at -0.04): a link sphere and a mesh sphere overlapping by
 * >= 0.04 + 1e-4 prove "collision", and the full hulls' projections on the direction between
 * the most-overlapping pair's centres overlapping by < 0.04 - 1e-4 prove "free".  Results do
 * not depend on them -- only speed.  spheres.py builds them. */
int tcmp_set_mesh_spheres(tcmp_handle* h, const double* spheres, int32_t n_mesh, int32_t k);

/* Self-collision (get_collision_fn(..., self_collisions=True), utils.py:3165-3191 with the
 * pairs of get_self_link_pairs, utils.py:3125-3149): enable != 0 adds the 33 link pairs of
 * the arm whose moving-ancestor joint sets differ and that are not parent/child (link0 is the
 * base, outside get_links; link8 has no geometry), same -0.04 closest-point threshold
 * (pairwise_link_collision -> get_closest_points default, utils.py:2781,2833,2851).  Every
 * later collision check (configs, edges, planning rounds, rewiring) includes them.  Off by
 * default, as in the reference planner (SELF_COLLISIONS = False, utils.py:56). */
int tcmp_set_self_collision(tcmp_handle* h, int32_t enable);

/* Bodies held by the gripper (get_collision_fn(..., attachments=[...]), utils.py:3165-3218: the
 * attached bodies are assigned to their parent link at every configuration and tested against
 * every obstacle; Grasp.get_attachment, utils.py:3363-3365, builds them).  n <= 4 convex hulls in
 * their own (child) frames, in tcmp_set_meshes' layout, each of at most 64 vertices (so at most
 * 124 facets and 186 edges).  parent_link: index into the ten moving collision links (0..6
 * panda_link1..7, 7 panda_hand, 8 / 9 the fingers).  parent_from_child: n x 12, R row-major then
 * p; the body's world pose at q is world_from_parent(q) * parent_from_child, world_from_parent
 * being the collision model's link frame.  The tool frame is no collision link: the caller folds
 * hand_from_tool = Trans(0, 0, 0.105) into parent_from_child.
 * Depth of a held body against an obstacle (a box of tcmp_set_scene or a mesh of
 * tcmp_set_meshes): the minimum overlap over the facet normals of both and the normalised cross
 * products of their unit edge directions (squared cross norm below 1e-12 skipped), fp64 -- the
 * definition tcmp_base_pd uses.  Held flag of a configuration: any depth >= 0.04.  No joint-limit
 * test of its own, no test against the robot's own links (utils.py:3191 is a TODO) or among held
 * bodies.
 * With attachments set, tcmp_check_configs ORs the held flag into its flags, and every edge walk
 * (tcmp_check_edges, tcmp_plan_round, tcmp_plan_run and its round graphs, tcmp_plan_shortcut,
 * tcmp_shortcut_path, tcmp_plan_connect, tcmp_connect_nodes) and the rewiring end an edge at
 * the first step whose held flag is set, as the sequential walk with that collision_fn does
 * (n_steps unchanged).  tcmp_plan_begin tests start and goal with it.
 * tcmp_plan_run_fused, tcmp_plan_run_group, tcmp_plan_run_shared, tcmp_plan_begin_many,
 * tcmp_plan_repair, tcmp_repair_traj and tcmp_goal_search do not check held bodies: with
 * attachments set they return -1 with a message naming the attachment and do nothing.
 * n = 0 clears.  Replaces the previous set; keeps boxes, meshes and the self-collision setting.
 * A set and a scene must fit a block's LDS together: the rewiring stages the arm's LDS (n x 160
 * + 76,280 B for a box scene of n obstacles, n x 32 + 71,496 B with meshes or self-collision) and behind it
 * 128 B per obstacle and 24 B per hull row (vertices, distinct facet normals and edge
 * directions) within 137,720 B -- about 210 boxes with one 8-vertex box held, about 88 with four
 * 64-vertex hulls.  tcmp_set_attachments, tcmp_set_scene, tcmp_set_meshes and
 * tcmp_set_self_collision refuse (-1, with the figures) a change that would not fit, and change
 * nothing then.
 * Refused (-1) while a plan is open, that is from its tcmp_plan_begin to its tcmp_plan_finish or
 * tcmp_plan_retrace (a finished plan's later stages take the set as it is then).  Validated (-1 otherwise): unit plane normals and every
 * vertex inside every plane within 1e-9, edge rows in range, R^T R = I within 1e-9, det R > 0,
 * parent_link in 0..9, the sizes above. */
int tcmp_set_attachments(tcmp_handle* h, const tcmp_hulls* hulls, int32_t n,
                         const int32_t* parent_link, const double* parent_from_child);

/* Probe (utils.py:3165-3218, the attachments' pairwise_collision): the depth of every held body
 * against every obstacle at n configurations, by the arithmetic the flags use and with no
 * certificate applied.  pd: n x n_att x (n_box + n_mesh), obstacles in tcmp_base_pd's order. */
int tcmp_attached_pd(tcmp_handle* h, const double* q, int64_t n, double* pd);

/* Instrumentation of the held bodies' edge post-pass (no reference counterpart).  counts[4]:
 * since the last tcmp_plan_begin (or tcmp_set_attachments), over every edge walk of the handle,
 * the edges whose arm walk accepted a prefix, those of them the held bodies shortened, those
 * they removed (n_safe' = 0); then the round graphs this handle has captured in its lifetime.
 * ms (may be NULL): the device time of the post-pass kernel alone since the last
 * tcmp_plan_begin, by events around its launches (0 with tcmp_set_timing off); it is part of
 * tcmp_plan_result.ms_edges. */
int tcmp_attach_stats(tcmp_handle* h, uint64_t* counts, double* ms);

/* per-kernel-family device timing of plans (tcmp_plan_result.ms_*: hipEvents recorded around
 * each family, event nodes inside captured round graphs).  On by default; off records no
 * events, so a round graph holds kernel nodes only and ms_* stay 0 (queries run concurrently
 * on several engines, whose event spans would include each other's kernels anyway).  No
 * reference counterpart (instrumentation). */
int tcmp_set_timing(tcmp_handle* h, int32_t enable);

/* ---- batched physics (host arrays in/out) ---------------------------------------------- */
/* rne(q, qd, qdd) with add_payload(r, m) state made explicit: payload iff payload_mass > 0
 * (rne.py:181-254).  q, qd, qdd, tau: n x 7. */
int tcmp_rne_batch(tcmp_handle* h, const double* q, const double* qd, const double* qdd,
                   int64_t n, double payload_mass, double* tau);

/* torque test on n configurations (panda_primitives.py:13-193); qd/qdd may be NULL (zeros,
 * the search-time call torque_fn(q)).  ok: n int32 (1 = within limits). */
int tcmp_torque_ok(tcmp_handle* h, const double* q, const double* qd, const double* qdd,
                   int64_t n, int32_t torque_mode, double payload_mass, int32_t* ok);

/* collision_fn(q) on n configurations (utils.py:3165-3218): joint limits then every moving
 * link hull vs every obstacle, penetration >= 0.04 m.  collides: n int32. */
int tcmp_check_configs(tcmp_handle* h, const double* q, int64_t n, int32_t* collides);

/* Body-level check any(pairwise_collision(robot, b) for b in obstacles) on n configurations
 * (franka_ik_fast.py:78, panda_primitives.py:260 -> utils.py:2872-2880 body_collision ->
 * get_closest_points(max_distance=-0.04), :2833): every link of the robot body, i.e. the moving
 * links AND the static base panda_link0, penetration >= 0.04 m, no joint-limit test.
 * The robot against the obstacles only: bodies set with tcmp_set_attachments are not part of it
 * (it is the grasp check, made before anything is held).  collides: n int32. */
int tcmp_check_body(tcmp_handle* h, const double* q, int64_t n, int32_t* collides);

/* Penetration depth of the static base panda_link0 (world = base frame) against each obstacle
 * of the scene: the tcmp_set_scene boxes, then the tcmp_set_meshes meshes (n must be their
 * sum).  The q-independent half of tcmp_check_body. */
int tcmp_base_pd(tcmp_handle* h, double* pd, int32_t n);

/* debug: one stage of the device's pair-depth chain on n given (link, pose, obstacle) pairs of
 * the scene set on the handle, one wave per pair, through the production device function with
 * the arguments the planner's kernels hand it.  No reference counterpart.
 * link: moving-link index 0..9; pose: n x 12, the link frame (R row-major, p) as tcmp_fk lays
 * it out; obstacle: box index, then n_box + mesh index (tcmp_base_pd's order).
 * stage -> pd (info is 0 unless stated):
 *   CHAIN       the whole chain (exact_pair); only pd >= 0.04 is meaningful
 *   BOX32/64    hull-vs-box in fp32 (NaN = "needs fp64") / fp64, on a box obstacle or on a
 *               mesh's outer box (flag INNER_BOX: its inner box)
 *   HULL32      fp32 hull-vs-hull on the full hulls, stop = 0.04 - 1e-4 (value, or NaN)
 *   HULL64      its fp64 restatement (returns early with an upper bound once below 0.04)
 *   LOD_IN/OUT  fp32 hull-vs-hull on the inner / outer level-of-detail hulls with their
 *               production stop (0.04 + 1e-4 / 0.04 - 1e-4); value or NaN
 *   FACET_AXES  the facet trial axes: an upper bound of the depth, or +inf
 *   SPHERE_CERT the inscribed-sphere certificate: pd 0, info 0 free / 1 collision / 2 undecided
 * An fp32 hull-vs-hull value below its stop is only an upper bound (early exit).
 * flag NO_PRUNE (HULL32, HULL64, LOD_IN, LOD_OUT): no Gauss-map cluster is skipped.
 * Returns -1 when the stage does not apply to a pair (a mesh stage on a box, a LOD stage on a
 * mesh without LODs, a sphere stage without spheres, INNER_BOX without an inner box) and
 * while self-collision pairs are on. */
enum {
  TCMP_PD_CHAIN = 0, TCMP_PD_BOX32 = 1, TCMP_PD_BOX64 = 2, TCMP_PD_HULL32 = 3, TCMP_PD_HULL64 = 4,
  TCMP_PD_LOD_IN = 5, TCMP_PD_LOD_OUT = 6, TCMP_PD_FACET_AXES = 7, TCMP_PD_SPHERE_CERT = 8
};
enum { TCMP_PD_NO_PRUNE = 1, TCMP_PD_INNER_BOX = 2 };
int tcmp_debug_pair_pd(tcmp_handle* h, const int32_t* link, const double* pose,
                       const int32_t* obstacle, int64_t n, int32_t stage, int32_t flags,
                       double* pd, int32_t* info);

/* debug: the device's fp32 wave reductions (the helpers of the exact tests and of the scan) on
 * n given waves, one wave per row, one launch; no scene or plan involved.  No reference
 * counterpart.  values: n x 64 x 6 floats (wave, lane, column), none NaN.  out: n x 9 --
 * the six results of the multi-value helper (minima of columns 0..2, maxima of columns 3..5),
 * then the single-value minimum, maximum and broadcast minimum of column 0. */
int tcmp_debug_wave_reduce(tcmp_handle* h, const float* values, int64_t n, float* out);

/* debug, host only (no device call): the Gauss-map edge records and cluster cones of n hulls,
 * exactly as tcmp_set_meshes / tcmp_set_mesh_lods upload them.  No reference counterpart.
 * records: E x 16 doubles (c = -n1, d = -n2, unit(d x c), edge vector, endpoint, 0), each
 * hull's rows sorted by arc direction; cones: C x 8 floats (axis, cos and sin of the
 * half-angle, first and end record row as int bits, 0), room for 128 per hull;
 * cluster_off: n + 1, hull m's cones are rows [cluster_off[m], cluster_off[m + 1]). */
int tcmp_gauss_clusters(const tcmp_hulls* H, int32_t n, double* records, float* cones,
                        int32_t* cluster_off);

/* safe_path_force_aware(extend(from, to), collision, torque) for n edges (rrt_star.py:90-98,
 * utils.py:3068-3077 with the given resolution vector (7, NULL = 0.1 as the planner uses)).
 * n_safe = len(safe prefix), n_steps = len(extend), last = prefix[-1] (valid if n_safe>0).
 * A resolution that is not finite or not positive: -1 ("resolutions and weights must be
 * positive"), nothing is launched. */
int tcmp_check_edges(tcmp_handle* h, const double* from, const double* to, int64_t n,
                     const double* resolutions, int32_t torque_mode, double payload_mass,
                     int32_t* n_safe, int32_t* n_steps, double* last);

/* Force-aware path shortcutting (no reference counterpart: the reference returns
 * goal_n.retrace() as it is).  One pass: anchors a_k = min(k s, n - 1) with s = 1 when
 * n <= max_anchors, else ceil((n - 1) / (max_anchors - 1)); every chord between two anchors at
 * least two waypoints apart goes through tcmp_check_edges' check and is valid when its whole
 * extend is safe and ends within 1e-6 of its target (the rewire acceptance, rrt_star.py:191);
 * a dynamic program over the anchors (original hops as they are, valid chords at their
 * distance fn length; the original hop wins ties, then the lowest anchor) picks the cheapest
 * subsequence; chosen chords are replaced by their extend points, ending in the target waypoint
 * itself.  Passes repeat on the new list until one uses no chord.  First and last waypoint are
 * kept bit for bit and cost_after <= cost_before.  Deterministic. */
typedef struct {
  int32_t max_anchors;       /* 2..1024, 0 = 512 */
  int32_t passes;            /* 1..8, 0 = 1 */
} tcmp_shortcut_cfg;

typedef struct {
  int32_t status;            /* 0, or TCMP_PLAN_NO_GOAL when the open plan has no goal node */
  int32_t passes_run;
  int64_t n_before, n_after; /* waypoints */
  double cost_before, cost_after; /* summed distance fn over consecutive waypoints */
  int64_t n_anchors;         /* first pass */
  uint64_t chords_tested, chords_valid, chords_used, chord_steps; /* over all passes */
  double ms;                 /* device time of the stage (0 with timing off) */
} tcmp_shortcut_result;

/* shortcut n_wp waypoints (n_wp x 7; 1 or 2 come back as they are) in the scene set on the
 * handle.  resolutions (7, NULL = 0.1), weights (7, NULL = 10): the extend and distance fns'.
 * out: cap_out x 7; too small: status -4 with res->n_after set.  Leaves an open plan alone. */
int tcmp_shortcut_path(tcmp_handle* h, const double* waypoints, int64_t n_wp,
                       const double* resolutions, const double* weights, int32_t torque_mode,
                       double payload_mass, const tcmp_shortcut_cfg* cfg, double* out,
                       int64_t cap_out, tcmp_shortcut_result* res);

/* Best-parent goal connection over the whole tree (no reference counterpart: the reference tries
 * the goal from the node nearest to it only, and never again once goal_n exists,
 * rrt_star.py:160-161, so goal_n.cost never improves).  Opt-in, between the rounds and the
 * shortcut or finish; it changes nothing unless called.
 *
 * Inputs: nodes i = 0 .. T-1 with configuration c_i and cost g_i >= 0, the target G, the weights
 * w and a bound B -- +inf without a goal node, else the current goal node's cost (the plan form
 * reads it from the tree row).
 *   key       key_i = g_i + distance(c_i, G, w), the distance fn summed in joint order
 *             (s += w_k * (d * d), sqrt, no contraction), then the one add
 *   eligible  key_i < B, strictly; a NaN key fails.  The goal node and everything below it are
 *             therefore never eligible; there is no other exclusion
 *   selected  M = min(n_eligible, K * passes); the M eligible nodes smallest by (key, i), in that
 *             order (ties to the lowest index); K = max_candidates
 *   pass p    tests ranks [p K, min(M, (p + 1) K)): each candidate's edge c_i -> G goes through
 *             tcmp_check_edges' check (safe_path_force_aware(extend(c_i, G)), the static torque
 *             test) with the call's resolutions, torque mode, payload mass and scene.  A
 *             candidate is valid iff n_safe > 0 and distance(last, G, w) < goal_tolerance (the
 *             test of a round's goal lane); its new cost is c = g_i + distance(c_i, last, w).
 *             The pass's winner is the valid candidate with c < B smallest by (c, rank).  The
 *             first pass with a winner ends the stage: later ranks are not tested
 *   outcome   OK with the winner; NONE when no pass had one (n_eligible == 0 included, then
 *             passes_run = 0); the plan form only: TREE_FULL when a winner exists but
 *             n_nodes == max_nodes.  NONE and TREE_FULL leave everything as it was, bit for bit
 * The ranking is by the straight-line key, so candidates behind one obstacle cluster together;
 * `passes` is the answer to that.  Deterministic: equal calls give equal bytes. */
#define TCMP_CONNECT_OK 0
#define TCMP_CONNECT_NONE 1
#define TCMP_CONNECT_TREE_FULL 2

typedef struct {
  int32_t max_candidates;    /* K: 1..65536, 0 = 1024 */
  int32_t passes;            /* 1..8, 0 = 1 */
} tcmp_connect_cfg;

typedef struct {
  int32_t status, passes_run;
  int64_t n_nodes, n_eligible, n_selected, n_tested, n_valid; /* tested, valid: the passes run */
  uint64_t edge_steps;       /* extend steps of the tested edges */
  int64_t goal_node_before, goal_node_after;  /* -1: none (the stand-alone form: both -1) */
  int64_t parent, rank;      /* the winner (TREE_FULL too), -1: none */
  double cost_before;        /* the goal node's cost; 0 without a goal (stand-alone: 0) */
  double cost_after;         /* OK: the new cost; else cost_before */
  double key_min;            /* smallest eligible key: no connection can beat it;
                                0 when n_eligible == 0 */
  double ms;                 /* device time of the stage (0 with timing off) */
} tcmp_connect_result;

/* the stage on n given nodes (nodes n x 7, cost n, 1 <= n <= INT_MAX, costs not negative) in
 * the scene set on the handle; bound = INFINITY: none.  resolutions (7, NULL = 0.1), weights (7,
 * NULL = 10).  ids_out, keys_out (cap_out each): the M selected, in rank order; nsafe_out,
 * nsteps_out (cap_out each): the verdicts of the tested ranks, -1 for ranks a stopped stage never
 * tested; cap_out < M with one of the four given: status -4 with res->n_selected set.  node_out
 * (8): on OK the winner's record, `last` (7 values) then c.  Any output pointer may be NULL.
 * Leaves an open plan alone. */
int tcmp_connect_nodes(tcmp_handle* h, const double* nodes, const double* cost, int64_t n,
                       const double* goal, double bound, const double* resolutions,
                       const double* weights, double goal_tolerance, int32_t torque_mode,
                       double payload_mass, const tcmp_connect_cfg* cfg, int32_t* ids_out,
                       double* keys_out, int32_t* nsafe_out, int32_t* nsteps_out, int64_t cap_out,
                       double* node_out, tcmp_connect_result* res);

/* Goal-set connection: the stage above with one change -- each node is tried toward the goal of
 * a given set that is nearest to it.  A grasp pose has a whole family of goal configurations
 * (joint 7 is free, up to 8 IK branches per value; tcmp_goal_search lists the feasible ones);
 * the rounds and tcmp_plan_connect aim at one.  Opt-in; nothing else changes.
 *
 * Inputs: the nodes (c_i, g_i), i = 0 .. T-1, goals G_0 .. G_{n-1} with 1 <= n <= 256, the
 * weights w and the bound B as for tcmp_connect_nodes.
 *   nearest   s_ij = sum_k w_k * (d * d) with d = G_jk - c_ik, k ascending, fp64, no contraction:
 *             the distance fn's sum before its square root.  j*(i) is the lowest j attaining
 *             min_j s_ij (a strict < scanning j ascending); a NaN s_ij never wins.  The rule is
 *             on s, not on the distance: a square root that maps two sums to one value cannot
 *             change j*.  Duplicate goals are allowed; the lowest index wins
 *   key       key_i = g_i + sqrt(s_{i j*}) = g_i + min_j distance(c_i, G_j, w) (sqrt is
 *             monotone); with n = 1 it is tcmp_connect_nodes' key bit for bit
 *   eligible, selected, pass, outcome: as tcmp_connect_nodes words them with G replaced per
 *             candidate by G_{j*(i)}: the edge tested is c_i -> G_{j*(i)}; the candidate is valid
 *             iff n_safe > 0 and distance(last, G_{j*(i)}, w) < goal_tolerance;
 *             c = g_i + distance(c_i, last, w); the winner is the valid candidate with c < B
 *             smallest by (c, rank); the first pass with a winner ends the stage.  B is the
 *             current goal node's cost, whichever goal it reached
 * Beyond tcmp_connect_result: goal_index of the winner (TREE_FULL too; -1: none), and per goal
 * three counts -- near (eligible nodes whose j* is that goal), tested and valid (over the passes
 * run): which of the goals the tree can reach.
 * A node is tried toward its nearest goal only: on a one-node tree exactly one goal is tried, and
 * a blocked goal shadows the others for the nodes nearest to it.  The counts show it (tested > 0,
 * valid == 0); the answer is a second call without that goal.  (Pairs (i, j) as candidates would
 * need T x n keys: this is why the rule is per node.)
 * Refused with -1 and nothing launched: n_goals outside 1..256, a goal value that is not finite,
 * and what tcmp_connect_nodes refuses.  Goals outside the joint limits, in collision or over the
 * torque limits are not refused: their edges fail. */
typedef struct {
  tcmp_connect_result r;
  int32_t n_goals, goal_index;
} tcmp_connect_set_result;

/* the stand-alone form: tcmp_connect_nodes' arguments with goals (n_goals x 7) for the goal.
 * goal_out (cap_out, counted in the -4 rule): j* of the selected ranks, -1 for ranks never tested,
 * as nsafe_out.  per_goal (3 x n_goals: the near, the tested, the valid counts; may be NULL). */
int tcmp_connect_goal_set(tcmp_handle* h, const double* nodes, const double* cost, int64_t n_nodes,
                          const double* goals, int32_t n_goals, double bound,
                          const double* resolutions, const double* weights, double goal_tolerance,
                          int32_t torque_mode, double payload_mass, const tcmp_connect_cfg* cfg,
                          int32_t* ids_out, double* keys_out, int32_t* goal_out,
                          int32_t* nsafe_out, int32_t* nsteps_out, int64_t cap_out,
                          double* node_out, int64_t* per_goal, tcmp_connect_set_result* res);

/* argmin over tree nodes of the weighted distance (rrt_star.py:9-14,171), first index wins
 * ties.  tree: T x 7, samples: n x 7, weights: 7 positive (NULL = 10 = 1/radius).  Runs the
 * planner's own nearest path: the radix-tree cell index of the tree and the pruned exact
 * scan k_nearest_wave32 (fp32 first pass, fp64 decision). */
int tcmp_nearest(tcmp_handle* h, const double* tree, int64_t T, const double* samples,
                 int64_t n, const double* weights, int32_t* idx);

/* dynam_fn min-jerk sampling (panda_primitives.py:299-316 -> min_jerk_v2.py:80-222):
 * n_wp waypoints (7 each), ni samples per segment; q/qd/qdd: (n_wp-1)*ni x 7. */
int tcmp_minjerk(tcmp_handle* h, const double* waypoints, int64_t n_wp, int64_t ni, double* q,
                 double* qd, double* qdd);

/* final validation loop (rrt_star.py:208-210) + Conf.torques (utils.py:3376-3377, rne
 * without payload).  first_fail = index of the first failing sample or -1.  tau may be NULL. */
int tcmp_validate_traj(tcmp_handle* h, const double* q, const double* qd, const double* qdd,
                       int64_t n, int32_t torque_mode, double payload_mass, int64_t* first_fail,
                       double* tau);

/* ---- goal IK ------------------------------------------------------------ */
/* ikfast get_ik (ikfast_panda_arm.cpp:12839 -> ComputeIk :12770, free joint = joint7 :398),
 * batched: poses n x 12 = panda_link8 in panda_link0 (rotation 9 row-major, then position 3,
 * the eerot/eetrans of :12854-12862), free_q7 n values.  sols: n x 8 x 7 (the count[i]
 * solutions of row i packed first, angles in (-pi, pi]); count: n.  Joint limits are NOT
 * applied (the reference filters afterwards, ikfast.py:166). */
int tcmp_ik(tcmp_handle* h, const double* poses, const double* free_q7, int64_t n, double* sols,
            int32_t* count);

/* ikfast get_fk (ikfast_panda_arm.cpp:12907 -> ComputeFk :307): q n x 7 -> poses n x 12. */
int tcmp_fk(tcmp_handle* h, const double* q, int64_t n, double* poses);

/* ---- the RRT* engine (rrt_star_force_aware, rrt_star.py:151-211) ------------------------ */
typedef struct {
  double start[7];
  double goal[7];
  double weights[7];      /* distance weights, 1/radius (panda_primitives.py:333-334) */
  double resolutions[7];  /* extend resolutions (panda_primitives.py:337: radius) */
  double radius;          /* rewire radius ([0.01], panda_primitives.py:346) */
  double goal_probability;/* 0.2 (rrt_star.py:151) */
  double goal_tolerance;  /* 1e-2 (rrt_star.py:178) */
  double payload_mass;    /* Problem.payload_mass (torque tests) */
  double execution_time;  /* Problem.execution_time (dynam_fn) */
  uint64_t seed;          /* Philox4x32-10 key for device sampling */
  int64_t max_nodes;      /* tree capacity (>= samples + 1) */
  int32_t max_batch;      /* largest round size that will be used */
  int32_t torque_mode;
} tcmp_plan_cfg;

typedef struct {
  int32_t status;         /* TCMP_PLAN_* */
  int32_t goal_found;
  int64_t n_nodes;
  int64_t n_samples;
  int64_t goal_node;
  int64_t n_waypoints;    /* len(goal_n.retrace()) */
  int64_t n_traj;         /* min-jerk samples */
  int64_t first_fail;
  uint64_t edge_steps;    /* extend steps checked (the new edges', then the rewire edges') */
  uint64_t pairs_tested;  /* link x obstacle pair classifications */
  uint64_t pairs_sat;     /* pairs reaching the OBB SAT tier */
  uint64_t pairs_exact;   /* exact hull tests */
  uint64_t nn_pairs;      /* (candidate, node) distance evaluations */
  double ms_nearest;      /* summed device time per kernel family (hipEvents) */
  double ms_edges;
  double ms_insert;
  double ms_rewire;
  double ms_finish;
  int64_t launches_nearest;
  uint64_t nn_box_tests;  /* (candidate, chunk-box) lower-bound tests of the pruned scan */
  double ms_nn_scan;      /* the k_nearest_wave32 launches alone (part of ms_nearest) */
  uint64_t snap_sum;      /* sum over rounds of the snapshot size T_r */
  uint64_t nn_full_pairs; /* sum over rounds of T_r * B_r: the brute-force scan's pair count */
  int64_t launches_nn_scan; /* k_nearest_wave32 launches (a one-node first round needs none) */
  uint64_t n_rewires;     /* new.rewire(n, d, path[:-1]) calls (rrt_star.py:187-192) on this
                             engine's lanes */
  uint64_t rewire_steps;  /* the rewire edges' extend steps (part of edge_steps, not k_edges') */
  int64_t graph_launches; /* tcmp_plan_run calls of this plan replayed as one captured graph */
  int64_t fused_plans;    /* plans of the fused rounds this plan grew in (tcmp_plan_run_fused;
                             0: its own rounds).  The fleet's kernel times (ms_*) are reported
                             on its first engine, every plan counts the fleet's rounds */
  double ms_edge_prep;    /* the edge order's sort and work records before k_edges (ms_edges
                             times k_edges alone) */
  double goal_cost;       /* goal_n.cost (rrt_star.py:25-27: the path's summed distance fn)
                             when a goal node exists, else 0 */
  int64_t goal_depth;     /* edges root -> goal node (len(retrace nodes) - 1), else 0 */
} tcmp_plan_result;

/* start a query: checks collision(start), collision(goal) (rrt_star.py:152), allocates the
 * tree and inserts the root.  result->status is set (0 or START_GOAL_COLLISION).  A weight or
 * resolution of cfg that is not finite or not positive: -1 ("resolutions and weights must be
 * positive"), nothing is launched and the handle's state is as before. */
int tcmp_plan_begin(tcmp_handle* h, const tcmp_plan_cfg* cfg, tcmp_plan_result* result);

/* one round of nb candidates.  samples == NULL: device Philox sampling (batched frontier,
 * at most one goal-biased lane per round).  Otherwise samples (nb x 7) and is_goal (nb) are
 * the host's draws (nb = 1 reproduces the reference loop exactly).  goal_found (nullable)
 * is written after a stream sync; pass NULL to keep rounds asynchronous. */
int tcmp_plan_round(tcmp_handle* h, const double* samples, const uint8_t* is_goal, int32_t nb,
                    int32_t* goal_found);

/* shared-tree rounds (SURVEY 8e's alternative to replica trees): every rank of `c` has the
 * same open plan (tcmp_plan_begin with identical cfg; max_nodes for the whole tree,
 * max_batch >= ceil(batch / world)) and calls this with the same n_samples / batch; rank r
 * takes lanes [r B / W, (r + 1) B / W) of each round of B and the ranks exchange, per round,
 * the goal lane and the accepted-edge counts (RCCL all-reduce / all-gather on the engine
 * stream) and then their new node records (one group of in-place ncclBroadcast calls), so
 * every rank holds the tree a single engine builds with tcmp_plan_run(h, n_samples, batch).
 * World 1 is tcmp_plan_run. */
int tcmp_plan_run_shared(tcmp_handle* h, tcmp_comm* c, int64_t n_samples, int32_t batch);

/* the same rounds driven by one process over n engines (devices may repeat), the exchanges
 * done through host copies and device-to-device copies: the single-process form of
 * tcmp_plan_run_shared (and its parity check on one GPU). */
int tcmp_plan_run_group(tcmp_handle* const* hs, int32_t n, int64_t n_samples, int32_t batch);

/* fused multi-plan rounds: n (1..31) engines on one device, each with its own open plan (its
 * own scene, start, goal, seed), all at the same round, grow their trees together -- one set
 * of kernel launches per round serves every plan's lanes (tcmp_fleet.h), on hs[0]'s stream;
 * the other engines' streams are ordered before and after it.  Every plan's tree is
 * bit-identical to what tcmp_plan_run(hs[q], n_samples, batch) grows alone; finish and fetch
 * each plan on its own engine as usual.  Box scenes may differ per plan; a fleet over convex
 * meshes or with self-collision pairs must be ONE scene (every plan's the lead's: replica trees
 * of one query), otherwise the call returns -1.  The plans must share the distance weights, at
 * most ~330 box obstacles over all plans (the fused edge kernel's LDS), and fewer than 2^31
 * node / lane slots over the fleet.  The multi-query form of tcmp_plan_run
 * (collect_data.py:74-85 plans several start/goal queries per scene step). */
int tcmp_plan_run_fused(tcmp_handle* const* hs, int32_t n, int64_t n_samples, int32_t batch);

/* tcmp_plan_begin / tcmp_plan_finish on n engines (cfgs[q], results[q] for hs[q]): every
 * engine's work is queued first, then the host waits once per engine -- a fleet's begins and
 * finishes cost about one device round trip instead of n.  Same results as the one-engine
 * calls; the first failing engine's error is reported (its index in the message).  Every cfg's
 * weights and resolutions are checked as tcmp_plan_begin's before the first engine's launch. */
int tcmp_plan_begin_many(tcmp_handle* const* hs, int32_t n, const tcmp_plan_cfg* cfgs,
                         tcmp_plan_result* results);
int tcmp_plan_finish_many(tcmp_handle* const* hs, int32_t n, tcmp_plan_result* results);

/* goal node of the open plan (-1 while none) and its cost -- goal_n.cost, the bound of the
 * informed rejection test (rrt_star.py:163-165); cost may be NULL. */
int tcmp_plan_goal(tcmp_handle* h, int64_t* node, double* cost);

/* device-sampled rounds of `batch` lanes until n_samples samples were drawn. */
int tcmp_plan_run(tcmp_handle* h, int64_t n_samples, int32_t batch);

/* retrace + dynam_fn min-jerk + final torque validation (rrt_star.py:199-211); fills result. */
int tcmp_plan_finish(tcmp_handle* h, tcmp_plan_result* result);

/* retrace only (rrt_star.py:199-200, goal_n.retrace()): the finish for a caller whose own
 * dynam_fn turns the waypoints into the trajectory (rrt_star.py:202 with a foreign dynam_fn).
 * No min-jerk, no validation: status is 0 (goal found) or TCMP_PLAN_NO_GOAL, n_traj 0,
 * first_fail -1; tcmp_plan_fetch then copies the waypoints. */
int tcmp_plan_retrace(tcmp_handle* h, tcmp_plan_result* result);

/* shortcut the open plan's path: retrace, then tcmp_shortcut_path's passes with the plan's own
 * weights, resolutions, torque mode and payload mass; the shortened list stays in the engine, and
 * the next tcmp_plan_finish / tcmp_plan_retrace / tcmp_plan_finish_many of this plan uses it
 * instead of retracing (until the next tcmp_plan_begin).  goal_cost / goal_depth stay the
 * tree's, and the plan's counters do not include the chords' (those are in `res`).  Without a
 * goal node: res->status = TCMP_PLAN_NO_GOAL and nothing changes. */
int tcmp_plan_shortcut(tcmp_handle* h, const tcmp_shortcut_cfg* cfg, tcmp_shortcut_result* res);

/* tcmp_connect_nodes' stage on the open plan's tree, with the plan's own goal, weights,
 * resolutions, goal tolerance, torque mode and payload mass.  On OK one node is appended at index
 * n_nodes with exactly the record a round's insertion writes (configuration = last, cost = c,
 * parent = i, extend target = G, its step counts), so the retrace regenerates the edge; n_nodes
 * grows by one and the new node is the goal node -- the old goal node stays as an ordinary node.
 * A stored shortcut list is dropped and the finished rows are invalidated, as by
 * tcmp_plan_shortcut (retime and repair are NOT_APPLICABLE until the next finish).  The plan's
 * counters are untouched (the edges' are in `res`).  No rewire pass runs around the new node.
 * Afterwards tcmp_plan_goal, tcmp_plan_digest, tcmp_plan_tree, the retrace, shortcut, finish and
 * further rounds see the new node; a plan meant to grow after a connection needs max_nodes one
 * above 1 + its samples.  A fleet member is connected on its own engine after
 * tcmp_plan_run_fused; the ranks of a shared tree must each call it (determinism keeps them
 * equal). */
int tcmp_plan_connect(tcmp_handle* h, const tcmp_connect_cfg* cfg, tcmp_connect_result* res);

/* tcmp_connect_goal_set's stage on the open plan's tree, with the plan's weights, resolutions,
 * goal tolerance, torque mode and payload mass, in tcmp_plan_connect's place and with its
 * effects: on OK one node is appended whose extend target is G_{j*}, the goal actually aimed at
 * (so the retrace regenerates the edge), and it becomes the goal node; NONE and TREE_FULL leave
 * every byte as it was.  The plan's own goal is not added to the set: the caller lists it if it
 * wants it.  A tree rooted at the start can so be connected to a new goal set without planning
 * again.  per_goal: 3 x n_goals, may be NULL. */
int tcmp_plan_connect_goal_set(tcmp_handle* h, const double* goals, int32_t n_goals,
                               const tcmp_connect_cfg* cfg, int64_t* per_goal,
                               tcmp_connect_set_result* res);

/* Torque-feasible retiming (no reference counterpart: the reference returns nothing when one
 * row of the trajectory fails the final torque test, rrt_star.py:208-210).  Playing the same rows
 * s times slower maps (q, v, a) to (q, v / s, a / s^2), and the rne and dyn torque models are
 * M a + C(q, v) v + g, so with x = 1 / s^2: tau(q, v sqrt(x), a x) = g(q) + x (tau(q, v, a) - g(q)).
 * Per row and tested joint j (limits L = 87 87 87 87 12 12, joint 7 untested), with
 * d = tau - g, sigma = sign(d) and the guard eps = 1e-9 N m:
 *   d != 0:  ub = ((L - eps) - sigma g) / |d|,  lb = (-(L - eps) - sigma g) / |d|
 *   d == 0:  ub = +inf, lb = 0 when |g| < L, else ub = -inf, lb = +inf
 * rne: g = rne(q, 0, 0, m), tau = rne(q, v, a, m), m = mass > 0.01 ? mass : 0; dyn: the same
 * without payload plus the static Jacobian force term on both; nov: d = 0 (the test ignores the
 * rates); base: no constraint.  x_hi = min ub, x_lo = max(0, max lb), x_max = 1 / min_scale^2,
 * x = min(x_max, x_hi), and x = 1.0 exactly when x >= 1 and min_scale == 1.
 * Status: INFEASIBLE when x <= 0 or x < x_lo; else OVER_CAP when max_scale > 0 and
 * x < 1 / max_scale^2; else OK, and then r = sqrt(x), s = 1 / r (host, fp64) and
 * qd' = qd r, qdd' = qdd x, psg' = psg s, one fp64 multiply each (x = 1 keeps every bit).
 * The scaled rows then go through the ordinary validation of the mode; a failing row there
 * gives UNVERIFIED and the rows stay as they were (the guard makes that unreachable in
 * practice).  Deterministic. */
#define TCMP_RETIME_OK 0
#define TCMP_RETIME_INFEASIBLE 1     /* no uniform retiming within [min_scale, inf) passes */
#define TCMP_RETIME_OVER_CAP 2       /* the slow-down needed exceeds max_scale */
#define TCMP_RETIME_UNVERIFIED 3     /* the scaled rows failed the validation pass */
#define TCMP_RETIME_NOT_APPLICABLE 4 /* tcmp_plan_retime: nothing to retime (see there) */

typedef struct {
  double min_scale;          /* (0, 1], 0 = 1; below 1 allows speeding up */
  double max_scale;          /* >= 1, 0 = no cap */
} tcmp_retime_cfg;

typedef struct {
  int32_t status;            /* TCMP_RETIME_* */
  int32_t bind_joint;        /* lowest joint attaining x_hi on bind_row; -1 when x_hi = +inf */
  int64_t n_rows;
  int64_t bind_row;          /* lowest row attaining x_hi; -1 when x_hi = +inf */
  int64_t n_static;          /* rows with some |g_j| >= L_j - eps */
  int64_t first_fail_before; /* the validation's first failing row as given, -1 = none */
  int64_t first_fail_after;  /* of the scaled rows (OK: -1); first_fail_before when not scaled */
  double x, r, s;            /* x = 1 / s^2, r = sqrt(x), s = 1 / r; 0 unless OK / UNVERIFIED */
  double x_hi, x_lo;
  double exec_time_after;    /* tcmp_plan_retime: s * execution_time; else 0 */
  double ms;                 /* device time of the stage (0 with timing off) */
} tcmp_retime_result;

/* retime n rows (q, qd, qdd: n x 7; psg: n or NULL) under torque_mode / payload_mass.
 * qd_out, qdd_out (n x 7) and psg_out (n, NULL iff psg is) are written when the status is OK
 * and left alone otherwise.  n = 0: OK with x = x_max.  cfg NULL = {1, 0}.  Leaves an open
 * plan alone. */
int tcmp_retime_traj(tcmp_handle* h, const double* q, const double* qd, const double* qdd,
                     const double* psg, int64_t n, int32_t torque_mode, double payload_mass,
                     const tcmp_retime_cfg* cfg, double* qd_out, double* qdd_out,
                     double* psg_out, tcmp_retime_result* res);

/* retime the trajectory of the open plan's last tcmp_plan_finish / tcmp_plan_finish_many, with
 * the plan's own torque mode and payload mass.  Applies when that finish's status was
 * TCMP_PLAN_OK or TCMP_PLAN_VALIDATION_FAILED; otherwise (no goal, a retrace-only finish, a
 * min-jerk assert, a shortcut or a retiming since that finish) res->status is
 * TCMP_RETIME_NOT_APPLICABLE and nothing changes.  On OK the engine's qd, qdd, psg and tau rows
 * are the scaled ones (tau recomputed from them), its stored status is TCMP_PLAN_OK and its
 * first_fail -1, so tcmp_plan_fetch returns the retimed trajectory; q and the waypoints are
 * untouched.  Any other status leaves every row as it was.  The next tcmp_plan_finish or
 * tcmp_plan_begin discards the retiming; the plan's counters are not touched. */
int tcmp_plan_retime(tcmp_handle* h, const tcmp_retime_cfg* cfg, tcmp_retime_result* res);

/* Collision repair of the min-jerk trajectory (no reference counterpart: the reference's final
 * validation tests torques only, rrt_star.py:208-210, and so does tcmp_plan_finish).  The edge
 * checks cover the chords between waypoints; the min-jerk rows leave them, because each joint of
 * an interior waypoint gets its own velocity (the mean of the adjacent slopes where they agree in
 * sign, else 0) and so its own time profile inside a segment.
 * Gated velocity: with a gate g[w] in {0, 1} per waypoint, the velocity of waypoint w is
 * g[w] ? (tcmp_minjerk's) : 0.0 for all seven joints, and everything else of tcmp_minjerk's
 * sampling is unchanged, operation for operation; the end waypoints' velocities are 0 whatever
 * their gates (which stay 1).  Every gate open gives tcmp_minjerk's rows bit for bit; between two
 * closed gates the rows lie on the chord, x = a + (b - a)(10 t^3 - 15 t^4 + 6 t^5).
 * A row fails when collision_fn(q_row) is true, as tcmp_check_configs decides it in the scene
 * set on the handle (joint limits, then boxes and meshes, and the self pairs when enabled).
 * Passes, from every interior gate open and every segment (rows [s ni, (s + 1) ni)) dirty:
 *   1. sample and check the ni rows of every dirty segment: hit (any failing row), the first
 *      failing row, the failing count; a clean segment keeps its last result (no hit);
 *   2. no segment hit: OK;
 *   3. a hit segment is stuck when each of its two waypoints is closed or a path end -- a
 *      rest-to-rest segment whose rows still fail (a collision between the edge check's
 *      resolution steps, or an end waypoint in collision): UNRESOLVED, with the lowest such
 *      segment and its first failing row;
 *   4. max_passes passes run: PASS_CAP;
 *   5. close g[s] and g[s + 1] of every hit segment s, all at once; the segments next to a gate
 *      that changed are the next pass's dirty set; again from 1.
 * Each continuing pass closes at least one gate: at most n_wp - 1 passes.  Two waypoints have no
 * gate, so any hit is UNRESOLVED.  The closure is greedy, not minimal.  Deterministic. */
#define TCMP_REPAIR_OK 0
#define TCMP_REPAIR_UNRESOLVED 1
#define TCMP_REPAIR_PASS_CAP 2
#define TCMP_REPAIR_COLLIDES 3        /* check_only: some row fails */
#define TCMP_REPAIR_NOT_APPLICABLE 4  /* tcmp_plan_repair: nothing to repair (see there) */

typedef struct {
  int32_t max_passes;        /* 0 = no cap */
  int32_t check_only;        /* != 0: the first pass only, OK or COLLIDES, nothing written */
} tcmp_repair_cfg;

typedef struct {
  int32_t status;            /* TCMP_REPAIR_* */
  int32_t passes_run;
  int64_t n_rows, n_segments;
  int64_t first_hit_before, rows_hit_before; /* rows as plain min-jerk gives them; -1, 0: none */
  int64_t first_hit_after, rows_hit_after;   /* of the last pass's gates (OK: -1, 0) */
  int64_t gates_closed, segments_resampled, rows_checked; /* summed over the passes */
  int64_t stuck_segment, stuck_row;          /* UNRESOLVED, else -1 */
  int64_t first_fail_before, first_fail_after; /* tcmp_plan_repair: the torque validation's first
                                                  failing row before / after; else -1 */
  double ms;                 /* device time of the stage (0 with timing off) */
} tcmp_repair_result;

/* repair the min-jerk rows of n_wp >= 2 waypoints (n_wp x 7), ni >= 1 samples per segment
 * (status -1 otherwise), in the scene set on the handle.  q, qd, qdd ((n_wp - 1) ni x 7) and
 * gates (n_wp) are written when the status is OK and left alone otherwise; with check_only they
 * may be NULL.  cfg NULL = {0, 0}.  Leaves an open plan alone.  Sized for a planner's paths
 * (tens to thousands of waypoints): the rows are checked across the whole device, but each pass's
 * bookkeeping over the segments runs in one workgroup, so a list of millions of waypoints is
 * accepted (n_wp and ni up to INT_MAX, 2^38 rows) and spends its passes' time there. */
int tcmp_repair_traj(tcmp_handle* h, const double* waypoints, int64_t n_wp, int64_t ni,
                     const tcmp_repair_cfg* cfg, double* q, double* qd, double* qdd, int32_t* gates,
                     tcmp_repair_result* res);

/* repair the trajectory of the open plan's last tcmp_plan_finish / tcmp_plan_finish_many, from
 * the waypoint list (a shortcut one if stored) and ni that finish used.  Applies when that
 * finish's status was TCMP_PLAN_OK or TCMP_PLAN_VALIDATION_FAILED and neither a repair that ended
 * OK nor a retiming that ended TCMP_RETIME_OK has run since; otherwise res->status is
 * TCMP_REPAIR_NOT_APPLICABLE and nothing changes.  A stage that left every row as it was does
 * not count: after a repair that ended UNRESOLVED or PASS_CAP, a check_only repair, or a
 * retiming that ended INFEASIBLE, OVER_CAP or UNVERIFIED, the repair still applies (and may be
 * repeated, for instance with another max_passes).  OK with no gate closed: the engine is untouched, bit for bit.  OK with gates
 * closed: the engine's q, qd and qdd rows are the repaired ones (psg and the waypoints are
 * untouched), the torque validation of the plan's mode and payload mass has run again on them,
 * tau is recomputed, and the stored status is TCMP_PLAN_OK or TCMP_PLAN_VALIDATION_FAILED with
 * the new first_fail (res->first_fail_after), so tcmp_plan_fetch returns the repaired trajectory
 * and tcmp_plan_retime afterwards works on it (rest-to-rest segments accelerate harder, so a
 * repaired trajectory may need it).  Any other status, and check_only, leave every row as it
 * was.  Repair then retime is allowed; retime then repair is NOT_APPLICABLE.  The next
 * tcmp_plan_finish or tcmp_plan_begin discards the repair; the plan's counters are not touched. */
int tcmp_plan_repair(tcmp_handle* h, const tcmp_repair_cfg* cfg, tcmp_repair_result* res);

/* Per-run torque-feasible retiming (no reference counterpart).  tcmp_retime_traj applies one
 * scale to every row, decided by the single worst row.  At a waypoint where the arm is at rest
 * -- all seven velocities 0 (a closed gate, or a natural reversal) and, as at every min-jerk
 * waypoint, zero acceleration -- the two sides are dynamically decoupled, so each stretch
 * between rest waypoints (a run) takes its own scale x_k; q is untouched (a repair's collision
 * verdict stays valid) and the retimed motion stays C^2.
 * Runs of a waypoint list: interior waypoint w (0 < w < n_wp - 1) is a rest waypoint when
 * gates != NULL && gates[w] == 0, or when all seven goal velocities of segment w - 1 are 0.0 as
 * tcmp_minjerk computes them (fp64, no contraction: v0 = (P[w] - P[w-1]) / 1.0,
 * v1 = (P[w+1] - P[w]) / 1.0, v0 v1 >= 1e-10 ? 0.5 (v0 + v1) : 0.0).  With rest waypoints
 * w_1 < ... < w_m the runs start at rows 0, w_1 ni, ..., w_m ni and end at (n_wp - 1) ni.
 * Per run k (rows [run_off[k], run_off[k+1])) everything is tcmp_retime_traj's definition
 * restricted to the run's rows (ub / lb, the guard, x_hi, x_lo, n_static, ties to the lowest
 * row, then the lowest joint; bind_row and first_fail are absolute rows): x_k = min(x_max,
 * x_hi_k), exactly 1.0 when x_k >= 1 and min_scale == 1; the run is INFEASIBLE or OVER_CAP by
 * the same tests; r_k = sqrt(x_k), s_k = 1 / r_k (host, fp64).  Overall: INFEASIBLE if any run
 * is, else OVER_CAP if any run is (fail_run: the lowest such run, else -1), and nothing is
 * written; else every row i of run k gets qd' = qd r_k, qdd' = qdd x_k (one fp64 multiply each:
 * x_k = 1 keeps every bit), and all scaled rows go through the mode's ordinary torque test (a
 * failing row: UNVERIFIED, first_fail_after set, outputs left alone).
 * Time warp (psg given): continuous, piecewise linear, knots at the boundary rows.  Origins
 * o_0 = psg[0], o_k = psg[run_off[k] - 1]; warped origins on the host in run order, O_0 = o_0,
 * O_k = O_{k-1} + (o_k - o_{k-1}) s_{k-1}; psg'[i] = O_k + (psg[i] - o_k) s_k (a subtract, a
 * multiply, an add, no contraction), and psg'[i] = psg[i] when s_k == 1.0 && O_k == o_k, so
 * leading unscaled runs keep their bits.  Deterministic. */
typedef struct {
  int64_t row_begin, row_end; /* the run's rows [row_begin, row_end) */
  int64_t bind_row;          /* lowest row of the run attaining x_hi; -1 when x_hi = +inf */
  int64_t first_fail;        /* the run's first row failing the test as given, -1 = none */
  int64_t n_static;          /* rows of the run with some |g_j| >= L_j - eps */
  int32_t status;            /* TCMP_RETIME_OK / INFEASIBLE / OVER_CAP, of this run alone */
  int32_t bind_joint;        /* lowest joint attaining x_hi on bind_row; -1 when x_hi = +inf */
  double x, r, s;            /* this run's scale; 0 unless the run's status is OK */
  double x_hi, x_lo;
  double t_begin;            /* O_k, the warped time at which the run begins; 0 without psg or
                                when the overall status is INFEASIBLE / OVER_CAP */
} tcmp_retime_run;

typedef struct {
  int32_t status;            /* TCMP_RETIME_* */
  int32_t n_scaled;          /* runs with x_k != 1 */
  int64_t n_rows, n_runs;
  int64_t fail_run;          /* lowest INFEASIBLE (else OVER_CAP) run, -1 = none */
  int64_t first_fail_before; /* the validation's first failing row as given, -1 = none */
  int64_t first_fail_after;  /* of the scaled rows (OK: -1); first_fail_before when not scaled */
  double x_min;              /* min x_k: 1 / sqrt(x_min) is tcmp_retime_traj's s at min_scale 1 */
  double time_ratio;         /* (sum_k s_k rows_k) / n_rows, summed in run order */
  double exec_time_after;    /* tcmp_plan_retime_runs: execution_time * time_ratio; else 0 */
  double ms;                 /* device time of the stage (0 with timing off) */
} tcmp_retime_runs_result;   /* n_scaled, x_min, time_ratio: 0 unless OK / UNVERIFIED; no runs
                                (n = 0): x_min = x_max, time_ratio = 1 */

/* the runs of n_wp >= 2 waypoints (n_wp x 7), ni >= 1 rows per segment (status -1 otherwise);
 * gates (n_wp) as tcmp_repair_traj returns them, or NULL = every gate open.  run_off receives
 * n_runs + 1 ascending row offsets, run_off[0] = 0, run_off[n_runs] = (n_wp - 1) ni.  cap (the
 * entries run_off holds) below n_runs + 1: status -4 with *n_runs set, run_off untouched.
 * Host only, no GPU. */
int tcmp_minjerk_runs(const double* waypoints, int64_t n_wp, int64_t ni, const int32_t* gates,
                      int64_t* run_off, int64_t cap, int64_t* n_runs);

/* retime n rows (q, qd, qdd: n x 7; psg: n or NULL) run by run.  run_off: n_runs + 1 strictly
 * ascending offsets with run_off[0] == 0 and run_off[n_runs] == n (status -1 otherwise; n == 0
 * needs n_runs == 0 and gives OK).  The caller vouches that the boundary rows run_off[k] - 1 are
 * at rest; the call does not test them (a sampled rest row carries rounding-level
 * accelerations).  qd_out, qdd_out (n x 7) and psg_out (n, NULL iff psg is) are written when the
 * status is OK and left alone otherwise; runs (n_runs entries, or NULL) receives the per-run
 * table whatever the status.  cfg NULL = {1, 0}.  Leaves an open plan alone.  The per-run
 * reduction gives each run to one wavefront: sized for a planner's runs (thousands of rows); a
 * single run of many millions of rows is reduced correctly but by 64 lanes. */
int tcmp_retime_runs_traj(tcmp_handle* h, const double* q, const double* qd, const double* qdd,
                          const double* psg, int64_t n, const int64_t* run_off, int64_t n_runs,
                          int32_t torque_mode, double payload_mass, const tcmp_retime_cfg* cfg,
                          double* qd_out, double* qdd_out, double* psg_out,
                          tcmp_retime_run* runs, tcmp_retime_runs_result* res);

/* per-run retiming of the open plan's last trajectory finish.  Applies exactly when
 * tcmp_plan_retime does (that finish ended TCMP_PLAN_OK or TCMP_PLAN_VALIDATION_FAILED and no
 * OK retiming, of either form, nor a shortcut has run since); otherwise res->status is
 * TCMP_RETIME_NOT_APPLICABLE and nothing changes.  The runs are tcmp_minjerk_runs of the
 * waypoint list and ni that finish used, with the gates of the last tcmp_plan_repair that ended
 * OK with gates closed (kept in a buffer of the plan's own; every gate open without one).
 * runs (cap_runs entries, or NULL: no table) receives the per-run table; cap_runs below n_runs:
 * status -4 with res->n_runs set and nothing changed.  On OK it acts as tcmp_plan_retime does:
 * the engine's qd, qdd and psg rows are the scaled ones, tau is recomputed, the stored status is
 * TCMP_PLAN_OK with first_fail -1, exec_time_after = execution_time * time_ratio, and
 * tcmp_plan_retime, tcmp_plan_retime_runs and tcmp_plan_repair are NOT_APPLICABLE until the next
 * finish.  Any other status leaves every row as it was. */
int tcmp_plan_retime_runs(tcmp_handle* h, const tcmp_retime_cfg* cfg, tcmp_retime_run* runs,
                          int64_t cap_runs, tcmp_retime_runs_result* res);

/* Torque-limited velocity-profile retiming (no reference counterpart).  Both retimings above play
 * the rows at a constant time scale, so the worst row sets the speed of its whole trajectory or
 * run.  Let the scale vary along the path instead: with the path parameter the original time
 * (psg), x = sd^2 and u = sdd, row (q, v, a) becomes (q, v sqrt(x), a x + v u) and its torque is
 *   tau = g(q) + u m + x d,   g = T(q, 0, 0), m = T(q, 0, v) - g, d = T(q, v, a) - g
 * (T: the six tested joints' torques as the mode's test sees them; the rates are read as
 * derivatives with respect to psg), affine in (u, x): the constant-scale identity is its u = 0
 * case.  The torque test of a row is 12 half-planes in (u, x), neighbouring rows are linked by
 * x_{i+1} = x_i + 2 D_i u_i, and the fastest profile comes from a backward pass over the
 * reachable sets and a forward greedy pass (time-optimal path parameterisation by reachability
 * analysis, discretised at the rows).
 * Per trajectory of rows i = 0 .. n-1: D_i = psg[i+1] - psg[i] > 0 (1 without psg),
 * L = 87 87 87 87 12 12, eps = 1e-9, Lg = L - eps, x_max = 1 / min_scale^2.
 * Coefficients: g, m, d from three passes of one instruction stream, so m = d = 0 exactly on a
 * row at rest and in nov mode; base: no constraint.
 * Uniform floor: x_u and the uniform status are tcmp_retime_traj's on these rows with the same
 * cfg (ub / lb from g and d).  Uniform OK: x_floor = x_u and the trajectory is anchored; else
 * x_floor = max_scale > 0 ? 1 / max_scale^2 : 1e-6, not anchored.
 * Lines of row i, each p - s x <= u <= P - S x:
 *   joint j, m_j != 0, A = |m_j|, sigma = sign(m_j):
 *     (P, S) = ((Lg_j - sigma g_j) / A, sigma d_j / A), (p, s) = ((-Lg_j - sigma g_j) / A, S);
 *   m_j == 0: the joint bounds x directly, by tcmp_retime_traj's ub / lb rules for d_j (d_j == 0
 *     included); a NaN among g_j, m_j, d_j: ub = -inf, lb = +inf;
 *   i < n-1, the link to row i+1's set: (P, S) = (hi_{i+1} / (2 D_i), 1 / (2 D_i)),
 *     (p, s) = (lo_{i+1} / (2 D_i), 1 / (2 D_i)).
 * Backward pass, i = n-1 .. 0 (u eliminated, so no vertex needs a tolerance): for every (upper k,
 * lower j) pair, at most 7 x 7, c = S_k - s_j, e = P_k - p_j: c > 0: x <= e / c; c < 0:
 * x >= e / c; c == 0 && e < 0: empty.  hi_i = min(x_max, direct ubs, pair ubs),
 * lo_i = max(x_floor, direct lbs, pair lbs).  Anchored: lo_i = x_floor, hi_i = max(hi_i, x_floor)
 * (the constant profile x_u lies in every set in exact arithmetic; only rounding can empty one,
 * which the guard and the validation cover).  Not anchored: !(lo_i <= hi_i) gives INFEASIBLE with
 * fail_row = i, the highest such row.
 * Forward pass: x_0 = hi_0; U = min over the row's joint upper lines of P - S x_i (+inf without
 * any), W = max over its joint lower lines (-inf); i < n-1: t = min(U, (hi_{i+1} - x_i) / (2 D_i)),
 * x_{i+1} = min(hi_{i+1}, max(lo_{i+1}, x_i + 2 D_i t)), u_i = (x_{i+1} - x_i) / (2 D_i); the last
 * row (and n = 1): u = min(U, max(0, W)).
 * Time: r_i = sqrt(x_i); psg'_0 = psg_0, psg'_{i+1} = psg'_i + 2 D_i / (r_i + r_{i+1}), summed in
 * row order; time_before = psg_{n-1} - psg_0, time_after = psg'_{n-1} - psg'_0, time_uniform the
 * same sum with x = x_u everywhere (0 when not anchored).
 * Rows: x_i == 1 && u_i == 0 copies the row; else qd' = qd r_i, qdd' = qdd x_i + qd u_i, each
 * product rounded before the add; q is untouched (a repair's collision verdict stays valid).
 * All of it fp64 without contraction.  The new rows go through the mode's ordinary torque test;
 * a failing row gives UNVERIFIED and the outputs are left alone.  Deterministic.
 * Consequences: a trajectory that passes at min_scale = 1 has x_u = 1 = x_max, so x = 1, u = 0 on
 * every row and every bit is kept.  Anchored: x_i >= x_u on every row and
 * time_after <= time_uniform, exactly -- never slower than tcmp_retime_traj.  Not anchored, it
 * also times rows the uniform retiming calls INFEASIBLE (rows that need acceleration to stay
 * inside a limit).  The acceleration is piecewise constant in the path parameter: the retimed
 * motion is C^1 with bounded jumps of qdd at the rows, where tcmp_plan_retime_runs stays C^2.
 * Velocity and jerk limits are not part of this. */
typedef struct {
  int32_t status;            /* TCMP_RETIME_OK / INFEASIBLE / UNVERIFIED (plan form: NOT_APPLICABLE) */
  int32_t anchored;          /* the uniform retiming is OK and its x is the floor of every set */
  int32_t uniform_status;    /* tcmp_retime_traj's status on these rows (OK / INFEASIBLE / OVER_CAP) */
  int32_t pad;
  int64_t n_rows;
  int64_t fail_row;          /* INFEASIBLE: the highest row whose set is empty, else -1 */
  int64_t first_fail_before; /* the validation's first failing row as given, -1 = none */
  int64_t first_fail_after;  /* of the new rows (OK: -1); first_fail_before when not written */
  int64_t n_at_floor, n_at_cap; /* rows with x_i == x_floor, x_i == x_max */
  double x_uniform;          /* tcmp_retime_traj's x; 0 unless uniform_status is OK */
  double x_floor;
  double x_min;              /* min x_i (n = 0: x_max); 0 when INFEASIBLE */
  double time_before, time_after, time_uniform; /* after, uniform: 0 when INFEASIBLE */
  double exec_time_after;    /* tcmp_plan_retime_profile; else 0 */
  double ms;                 /* device time of the whole call (0 with timing off) */
} tcmp_retime_profile_result; /* rows (fail_row, first_fail_*) count from the trajectory's start */

/* retime n_traj independent trajectories stored back to back: traj_off holds n_traj + 1 ascending
 * offsets from 0, trajectory t is rows [traj_off[t], traj_off[t+1]) of q, qd, qdd (n x 7,
 * n = traj_off[n_traj]) and psg (n, or NULL; strictly ascending inside a trajectory, status -1
 * otherwise).  qd_out, qdd_out (n x 7), psg_out (n, NULL iff psg is), x_out and u_out (n each, or
 * NULL) are written for the trajectories whose status is OK and left alone for the others;
 * coef_out (n x 18: g, m, d per row as the device computed them; debug; or NULL) is always
 * written.  results: n_traj records.  An empty trajectory gives OK.  ms (or NULL): the device
 * time of the call.  cfg NULL = {1, 0}.  One wavefront sweeps one trajectory, so the call is
 * sized for many trajectories of up to thousands of rows.  Leaves an open plan alone. */
int tcmp_retime_profile_traj(tcmp_handle* h, const double* q, const double* qd, const double* qdd,
                             const double* psg, const int64_t* traj_off, int64_t n_traj,
                             int32_t torque_mode, double payload_mass, const tcmp_retime_cfg* cfg,
                             double* qd_out, double* qdd_out, double* psg_out, double* x_out,
                             double* u_out, double* coef_out, tcmp_retime_profile_result* results,
                             double* ms);

/* velocity-profile retiming of the open plan's last trajectory finish.  Applies exactly when
 * tcmp_plan_retime does; otherwise res->status is TCMP_RETIME_NOT_APPLICABLE and nothing changes.
 * On OK it acts as tcmp_plan_retime does: the engine's qd, qdd and psg rows are the new ones, tau
 * is recomputed, the stored status is TCMP_PLAN_OK with first_fail -1,
 * exec_time_after = execution_time * time_after / time_before (execution_time when time_before
 * is 0), and every retiming form and tcmp_plan_repair are NOT_APPLICABLE until the next finish.
 * Any other status leaves every row as it was. */
int tcmp_plan_retime_profile(tcmp_handle* h, const tcmp_retime_cfg* cfg,
                             tcmp_retime_profile_result* res);

/* copy the finished plan: waypoints (n_waypoints x 7), trajectory q/qd/qdd (n_traj x 7),
 * psg (n_traj), tau = Conf.torques without payload (n_traj x 7).  Any pointer may be NULL. */
int tcmp_plan_fetch(tcmp_handle* h, double* waypoints, double* q, double* qd, double* qdd,
                    double* psg, double* tau);

/* digest of the open plan's tree, computed on the device: the sum over nodes i of a 64-bit
 * splitmix64 chain over (i, the node's 7 configuration and cost bits, its parent index), mod
 * 2^64 (torque_constrained_motion_planning_amd/shard.py tree_digest restates it).  Equal trees
 * give equal digests, so ranks of a shared-tree run (tcmp_plan_run_shared) can prove they hold
 * one tree by all-gathering it; n_nodes = the tree's node count. */
int tcmp_plan_digest(tcmp_handle* h, uint64_t* digest, int64_t* n_nodes);

/* debug: tree snapshot (cfg n x 7, cost n, parent n). */
int tcmp_plan_tree(tcmp_handle* h, int64_t cap, double* cfg, double* cost, int32_t* parent,
                   int64_t* n);
/* debug: the edge each node of the open plan's tree was inserted (or last rewired) on, rows as
 * tcmp_plan_tree's: tgt (cap x 7) the extend target the edge from the parent was walked toward,
 * meta (cap x 2) its (n_steps, n_safe) -- the node's configuration is the parent's after n_safe
 * refine steps of n_steps toward tgt (rrt_star.py:90-98, safe_path_force_aware(extend(...))).
 * The root's row is (its own configuration, 0, 0).  *n: the tree's node count. */
int tcmp_plan_tree_edges(tcmp_handle* h, int64_t cap, double* tgt, int32_t* meta, int64_t* n);

/* debug: the last round's nearest-neighbour step (rrt_star.py:171 for every lane): its nb
 * candidates (cand nb x 7), the chosen nearest node of each (nn, an index into the tree) and
 * the exact fp64 score of that node (sum_k (s_k - n_k)^2 when the weights are uniform, else
 * sum_k w_k (s_k - n_k)^2); snap = the snapshot size the round searched (nodes [0, snap)).
 * The first min(cap, nb) rows are copied; any array pointer may be NULL. */
int tcmp_plan_debug_round(tcmp_handle* h, int64_t cap, double* cand, int32_t* nn,
                          double* score, int64_t* snap, int32_t* nb);

/* ---- torque-aware goal search over the IK redundancy (opt-in) --------------------------- */
/* The reference turns a grasp pose into one goal configuration by taking the first free value
 * (joint 7) with any limit-valid IK solution, one of those at random, a body collision check and
 * up to 25 retries, and runs the static torque test once on what survived
 * (panda_primitives.py:240-265); tcmp_ik replays that.  tcmp_goal_search evaluates EVERY
 * candidate instead.  Candidate id = f * 8 + k of pose p is slot k of
 * tcmp_ik(poses[p], free_q7[f]), k < that call's count, and its configuration is tcmp_ik's bit
 * for bit (the same kernel runs), with one exception: tcmp_ik reports angles in (-pi, pi] and
 * joint 6's range reaches 3.7525, so a candidate whose q6 is below the lower limit while
 * q6 + 2 pi is at most the upper limit is taken at q6 + 2 pi (the only image that can be inside:
 * q6 <= -2.5307 never is), and the filters, the distance and q_out all use that image.  tcmp_ik
 * itself and the replay of the reference's choice keep the reported angle, as the reference does.
 * Filters, in order:
 *   limits     every joint within the limits, inclusive (collision_fn's test);
 *   torque     the six tested torques as the mode's test sees them at rest (zero rates): the
 *              candidate passes iff every !(|t_j| >= L_j), tcmp_torque_ok's comparison (a NaN
 *              fails); headroom = min_j (L_j - |t_j|) / L_j, 1.0 in TCMP_TORQUE_BASE;
 *   collision  the candidate collides iff tcmp_check_body or tcmp_check_configs says so in the
 *              scene on the handle: moving links against boxes and meshes, the self pairs when
 *              enabled, and the base link panda_link0, whose verdict is q-independent.
 * The feasible candidates of a pose are ordered by ascending (distance, id), distance =
 * sqrt(sum_k w_k (q_k - ref_k)^2) summed in joint order without contraction (the planner's
 * metric); the first n_out go to rows p * max_out + i of the outputs, the other rows are zeros
 * with id -1.  Headroom is reported, never a sort key: mirror branches (q1 + pi, -q2, q3 + pi)
 * have equal gravity torques up to rounding.  The result is deterministic (equal calls give equal
 * bytes), and the call leaves an open plan alone. */
typedef struct {
  int64_t n_solutions;   /* sum of tcmp_ik's counts over the free values */
  int64_t n_in_limits;   /* ... whose seven joints are within the limits */
  int64_t n_torque_ok;   /* ... and pass the mode's static torque test */
  int64_t n_feasible;    /* ... and are collision free */
  int32_t n_out;         /* min(n_feasible, max_out) */
  int32_t base_collides; /* panda_link0 collides with the scene: no candidate can be feasible */
} tcmp_goal_stats;

/* poses n_pose x 12 (as tcmp_ik takes them), free_q7 n_free values shared by all poses, ref 7,
 * weights 7 or NULL (10 each), max_out 1..256; n_pose >= 1, n_free >= 1 and
 * n_pose * n_free * 8 < 2^31, else status -1.  Outputs, each may be NULL: q_out
 * (n_pose * max_out x 7), dist_out, headroom_out, id_out (n_pose * max_out), stats (n_pose, one
 * per pose), ms (the device time of the stage).  One host wait. */
int tcmp_goal_search(tcmp_handle* h, const double* poses, int32_t n_pose,
                     const double* free_q7, int32_t n_free, const double* ref,
                     const double* weights, int32_t torque_mode, double payload_mass,
                     int32_t max_out, double* q_out, double* dist_out, double* headroom_out,
                     int32_t* id_out, tcmp_goal_stats* stats, double* ms);

/* ---- multi-GPU: query sharding + RCCL gather of solved paths -------------- */
/* One process per GPU; independent queries are dealt to ranks (collect_data.py:74-85 plans
 * them in a loop); the only collective is the gather of solved trajectories to rank 0.
 * A trajectory row is [q(7) qd(7) qdd(7) dt(1)] (Conf values / velocities / accelerations /
 * dt of create_trajectory, utils.py:3340-3347). */
#define TCMP_TRAJ_COLS 22
#define TCMP_REDUCE_SUM 0
#define TCMP_REDUCE_MAX 1

/* TCP rendezvous: rank 0 listens on addr:port; every other rank connects (retrying until
 * timeout_ms) and introduces itself with the job's identity (TCMP_JOB_ID, else the launcher's
 * TORCHELASTIC_RUN_ID, hashed with world and port: a stale or concurrent job is turned away).
 * Rank 0 sends its nbytes `blob` only after all world - 1 ranks have arrived; on a timeout it
 * closes every connection, so every rank fails together.  Host only, no GPU.  Used for the
 * ncclUniqueId; world == 1 returns at once. */
int tcmp_rendezvous(int32_t rank, int32_t world, const char* addr, int32_t port, void* blob,
                    int32_t nbytes, int32_t timeout_ms);

/* communicator of `world` ranks over RCCL on HIP device `device` (rank 0's unique id through
 * tcmp_rendezvous at addr:port).  world == 1: no RCCL communicator, no GPU touched. */
int tcmp_dist_init(int32_t rank, int32_t world, int32_t device, const char* addr, int32_t port,
                   tcmp_comm** out);
int tcmp_dist_destroy(tcmp_comm* c);
int tcmp_dist_rank(const tcmp_comm* c, int32_t* rank, int32_t* world);
/* ranks of the communicator's RCCL handle (ncclCommCount); 0 for a one-rank job, which has
 * no RCCL communicator.  Lets a multi-GPU run prove which collective world it ran in. */
int tcmp_dist_rccl_ranks(const tcmp_comm* c, int32_t* n);
/* device-synchronise this rank, then an RCCL all-reduce as the barrier */
int tcmp_dist_barrier(tcmp_comm* c);
/* in-place all-reduce of n doubles (op TCMP_REDUCE_SUM / TCMP_REDUCE_MAX) */
int tcmp_dist_allreduce(tcmp_comm* c, double* v, int32_t n, int32_t op);
/* all-gather of n int64 per rank: out = world x n, rank order */
int tcmp_dist_allgather_i64(tcmp_comm* c, const int64_t* in, int32_t n, int64_t* out);

/* gather every rank's solved paths to rank 0 (ncclGroupStart; ncclSend/ncclRecv;
 * ncclGroupEnd).  In: n_local paths, ids[i], rows[i], data = the paths' rows concatenated
 * (sum(rows) x TCMP_TRAJ_COLS); sizes = world x 2 int64 (queries, rows) of every rank when the
 * caller has all-gathered them already (tcmp_dist_allgather_i64), else NULL and the call does
 * the size all-gather itself.  Out, rank 0 only: n_queries paths in rank order (out_ids,
 * out_rows) with their rows concatenated in out_data, laid out by tcmp_gather_layout;
 * elsewhere n_queries = n_rows = 0.  Capacities too small: status -4 with n_queries / n_rows
 * set (the collective still completes on every rank).  Collective: every rank must call it.
 * Replaces the reference's host loop over queries (collect_data.py:74-85). */
int tcmp_gather_paths(tcmp_comm* c, int32_t n_local, const int64_t* ids, const int64_t* rows,
                      const double* data, const int64_t* sizes, int64_t cap_queries,
                      int64_t cap_rows, int64_t* out_ids, int64_t* out_rows, double* out_data,
                      int64_t* n_queries, int64_t* n_rows);

/* The two host-side halves of tcmp_gather_paths around its transport (RCCL send/recv on the
 * GPU; any byte transport works the same way).
 * tcmp_gather_pack: one rank's wire form -- hdr (2 n_local int64: id, rows of each path) and
 * body (sum(rows) x 22 doubles, the paths' rows concatenated; body may alias data).
 * tcmp_gather_unpack (rank 0): hdr_all / body_all hold every rank's wire form at the offsets of
 * tcmp_gather_layout(world, sizes); each rank's header rows are checked against the rows it
 * announced in sizes (status -6 otherwise: a transport that lost, duplicated or misplaced part
 * of a message), then the outputs are written as tcmp_gather_paths writes them (status -4
 * when the capacities are too small, n_queries / n_rows set).  Host only, no GPU. */
int tcmp_gather_pack(int32_t n_local, const int64_t* ids, const int64_t* rows, const double* data,
                     int64_t* hdr, double* body);
int tcmp_gather_unpack(int32_t world, const int64_t* sizes, const int64_t* hdr_all,
                       const double* body_all, int64_t cap_queries, int64_t cap_rows,
                       int64_t* out_ids, int64_t* out_rows, double* out_data, int64_t* n_queries,
                       int64_t* n_rows);

/* rank 0's receive layout of tcmp_gather_paths, host only: from sizes (world x 2: queries,
 * rows per rank) each rank's first header row q_off[k] and first trajectory row r_off[k] in
 * the rank-ordered output, and the totals.  Any output pointer may be NULL. */
int tcmp_gather_layout(int32_t world, const int64_t* sizes, int64_t* q_off, int64_t* r_off,
                       int64_t* total_q, int64_t* total_r);

#ifdef __cplusplus
}
#endif
#endif
