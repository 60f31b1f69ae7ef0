/*
 * include/nbk.h -- C-ABI of libnbk (numbotics_amd/csrc), the MI355X (gfx950) batched kinematics +
 * collision-validity engine.
 *
 * The reference (landonclark97/numbotics) has no FFI layer: its de-facto kernel ABI is the numba
 * signatures of the two batched kernels plus the Python methods that wrap PyBullet (SURVEY.md
 * section 8b).  Each entry point below names the reference interface it replaces; paths are relative
 * to the reference repository root.
 *
 * Conventions
 *   - plain pointers and sizes, no torch types; every array pointer that is not marked "host" is a
 *     DEVICE pointer (hipMalloc / torch.cuda tensor.data_ptr()) on the current device;
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); calls are asynchronous
 *     with respect to the host and capturable into a hipGraph (no allocation, no synchronisation).
 *     Two qualifications, both about the library's own scratch memory: nbk_validity_batch and
 *     nbk_edge_validity_batch keep one scratch set per (descriptor, stream), allocated on that
 *     stream's FIRST call (and regrown when a later batch needs more): such a call allocates and may
 *     wait for that stream's earlier work.  Captured before the scratch exists they return
 *     NBK_ERR_UNSUPPORTED (run the call once outside the capture, or use nbk_validity_batch_ws, whose
 *     scratch is the caller's); captured after, they are self-contained graph nodes: each replay
 *     prepares its own tables and clears its own counters in the stream's scratch, and direct calls
 *     made on that stream afterwards (in any order with the replays) do the same -- they no longer
 *     reuse tables between calls.  A graph holds the scratch's address: do not replay it after a
 *     direct call on the same stream with a LARGER batch has regrown the scratch (re-capture).  The *_host
 *     conveniences synchronise by definition, and so does nbk_spline_validity_batch (it reads its sample count back; it
 *     refuses a capturing stream; nbk_spline_continuous_batch does not).  Batches of 2^21 configurations or more (and edge batches of that many samples)
 *     run every other 2^20-configuration tile on a second, library-owned stream forked from and joined to `stream` with
 *     events -- the call still begins after, and completes before, its neighbours in `stream`'s order.  A captured call never
 *     uses the second stream.  A captured nbk_validity_batch that finds on `stream` the scratch a tiled direct call left there
 *     (sized for 2^20-configuration tiles, whatever that call's batch) runs such tiles one after the other on `stream`, so "once
 *     outside the capture" holds for these batches as for smaller ones; a captured edge batch runs its tiles without the second stream in its own
 *     scratch, which direct edge calls always size for that;
 *   - every compute call must be made with the descriptor's device current (hipSetDevice):
 *     NBK_ERR_INVALID otherwise;
 *   - float64 everywhere (the reference computes in float64); q is row-major (B, n_q);
 *   - return value: NBK_OK or a negative status; no exceptions cross the boundary;
 *   - a descriptor is immutable after creation and may be shared by streams and threads.  One made by nbk_model_create_movable
 *     is immutable except for its world poses (nbk_model_set_world_poses below).
 */
#ifndef NBK_H
#define NBK_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NBK_ABI_VERSION 2

enum {
    NBK_OK = 0,
    NBK_ERR_INVALID = -1,      /* bad argument (null pointer, negative size, bad index) */
    NBK_ERR_NO_DEVICE = -2,    /* no HIP device / not a gfx950 code object for this device */
    NBK_ERR_HIP = -3,          /* a HIP runtime call failed; see nbk_last_error() */
    NBK_ERR_UNSUPPORTED = -4,  /* descriptor exceeds a compiled-in limit (32 joints / DoF, 2^20 pairs, LDS capacity), or this
                                  entry point cannot serve this descriptor (per-pair distances of robots with 30+ primitives) */
    NBK_ERR_ALLOC = -5
};

/* shape / joint codes used inside descriptors */
enum { NBK_SPHERE = 0, NBK_CAPSULE = 1, NBK_BOX = 2, NBK_CYLINDER = 3, NBK_PLANE = 4, NBK_HULL = 5 };
enum { NBK_REVOLUTE = 0, NBK_PRISMATIC = 1 };
enum { NBK_CONNECT = 0, NBK_STEER = 1 };

#define NBK_MAX_JOINTS 32
#define NBK_MAX_DOF 32

/*
 * Flat robot + scene description ("compile the robot": replaces the per-frame flattening of
 * numbotics/robots/arm.py:17-71 and the per-query shape/pair bookkeeping of arm.py:190-250,555-580).
 * All pointers are HOST pointers; nbk_model_create copies everything to the device.
 */
typedef struct {
    int32_t n_q;                  /* degrees of freedom (columns of q) */
    int32_t n_joints;             /* movable joints = moving frames, parents first */
    const int32_t *joint_parent;  /* [J] parent moving frame, -1 = base */
    const int32_t *joint_type;    /* [J] NBK_REVOLUTE / NBK_PRISMATIC */
    const int32_t *joint_qidx;    /* [J] column of q */
    const double *joint_rot;      /* [J][27] M0 = R K, M1 = R (K - I), M2 = R [a]x (3x3 row-major each);
                                     local rotation = M0 - cos(q) M1 + sin(q) M2 (robots/helpers.py:43-55) */
    const double *joint_trans;    /* [J][3] translation of the (fixed-merged) joint offset */
    const double *joint_slide;    /* [J][3] R a for prismatic joints, 0 otherwise */
    const double *joint_axis;     /* [J][3] joint axis in the joint frame */
    const double *base_pose;      /* [12] 3x4 row-major */
    int32_t n_rshapes;            /* robot collision primitives */
    const int32_t *rshape_frame;  /* [S] moving frame carrying the shape, -1 = base */
    const int32_t *rshape_type;   /* [S] NBK_SPHERE / CAPSULE / BOX / CYLINDER / HULL */
    const double *rshape_local;   /* [S][12] pose of the primitive in its moving frame */
    const double *rshape_param;   /* [S][4] sphere r | capsule r,hl | cylinder r,hl | box hx,hy,hz | hull index ; [3] = margin */
    int32_t n_wshapes;            /* static world primitives (obstacles) */
    const int32_t *wshape_type;   /* [W] the above or NBK_PLANE (param[0..2] = unit normal) */
    const double *wshape_pose;    /* [W][12] world pose */
    const double *wshape_param;   /* [W][4] */
    int32_t n_pairs;              /* allowed (shape, shape) pairs, sorted by pair_a */
    const int32_t *pair_a;        /* [P] robot shape */
    const int32_t *pair_b;        /* [P] robot shape (< S) or S + world shape */
    /* Convex hulls of MESH collision shapes (numbotics/utils/shape.py:81-94 hands the file of numbotics/utils/mesh.py:18-37
     * to pybullet GEOM_MESH, i.e. one convex hull per mesh object; numbotics/physics/helpers.py:252-255 for URDF <mesh>).
     * A shape of type NBK_HULL names its hull in param[0]; vertices and face planes are in the primitive's local frame,
     * whose origin must be a point of the hull (the host uses the mean of the hull's vertices); margin inflates the hull. */
    int32_t n_hulls;
    const int32_t *hull_vert_begin;  /* [H+1] */
    const double *hull_verts;        /* [NV][3] */
    const int32_t *hull_face_begin;  /* [H+1]; a hull may have no planes (flat point set): distances stay exact; the
                                        penetration depth is EPA's either way, without planes its fallback (when EPA gives no
                                        answer) has only the other shape's axes and the centre line */
    const double *hull_planes;       /* [NF][4] unit outward normal n and offset d: inside n.x <= d.  nbk_model_create checks
                                        ||n|^2 - 1| <= 1e-9 and n.v <= d (+1e-9 relative) for every vertex of the hull and
                                        returns NBK_ERR_INVALID otherwise: the broadphase certifies collisions from the ball
                                        these planes inscribe */
} nbk_model_desc;

typedef struct nbk_model nbk_model;

int32_t nbk_abi_version(void);
const char *nbk_status_string(int32_t status);
const char *nbk_last_error(void);          /* text of the last HIP failure on this thread */
int32_t nbk_device_count(void);            /* 0 when no GPU is visible; never fails */

int32_t nbk_model_create(const nbk_model_desc *desc, nbk_model **out);
void nbk_model_destroy(nbk_model *m);
int32_t nbk_model_num_pairs(const nbk_model *m);

/*
 * Moving world bodies (the reference moves an obstacle with one resetBasePositionAndOrientation, numbotics/physics/object.py;
 * another chain's links move with its configuration).  Additive: nbk_model_create and descriptors made by it behave as before.
 *
 * nbk_model_create_movable makes the same descriptor as nbk_model_create -- same pairs, same kernels, accepted by every entry
 * point -- that is immutable EXCEPT FOR ITS WORLD POSES: the pose-dependent world tables (core frames, centres, the float32
 * copies of the broadphase, the static reach bounds) are rewritten on the device by an update.  world_radius (finite, >= 0) is the
 * caller's promise about how far from the origin the centre (pose translation) of a world shape will ever be: the slack of the
 * float32 broadphase is fixed at creation from max(robot reach, world_radius, the initial centres) and is compiled into the
 * per-robot broadphase, so poses beyond it are refused, not served.  A larger radius only makes the broadphase more conservative
 * (more narrowphase items); results stay bit-equal.  NBK_ERR_INVALID for a NaN / negative / infinite radius or an initial pose
 * that is not finite or lies beyond it.  The library's scratch of such a descriptor is sized for every pair (the host does not
 * know the poses), not for the pairs within reach.
 *
 * nbk_model_set_world_poses: poses (DEVICE) [W][12], 3x4 row-major world poses in the descriptor's world shape order (planes keep
 * the normal they were created with; only their point moves).  Asynchronous, no allocation, no host synchronisation, capturable:
 * one memset node and one kernel (k_world_update) in `stream`'s order -- calls issued to that stream afterwards see the new
 * poses, also the tables the validity path keeps between calls (they are prepared again on every stream of the descriptor).
 * Checks on OTHER streams are the caller's to order (events), in both directions: an update must not run while another stream
 * still checks against the descriptor.  The scalar host calls (private stream) wait for the last update issued outside a capture
 * by themselves; after replaying a graph that holds an update, synchronise before calling them.
 * Every pose is checked on the device: all 12 values finite and |centre| <= world_radius.  A pose that fails is not applied (its
 * shape keeps the previous pose) and sets the descriptor's world status; while it is set, EVERY configuration is reported
 * colliding, every edge and trajectory invalid (status NBK_CA_UNDECIDED unless NBK_CA_DEGENERATE, t_free NaN; a sampled spline
 * that would have been valid reports t_hit 0), and the distance-valued entry points (closest, pair distances, proximity rows,
 * records) return NaN everywhere and pair index -1 -- the rule for non-finite joint values, applied to the world, whatever the
 * geometry is.  The next update whose poses all pass clears it.  NBK_ERR_UNSUPPORTED on a descriptor made by nbk_model_create.
 *
 * nbk_model_set_world_poses_host: the same from HOST memory through pinned staging on the private stream of the scalar calls
 * (nbk_validity_scalar_host, nbk_edge_validity_scalar_host follow it without the caller's help); returns when the update is done.
 * nbk_model_world_status: synchronous read of the status: 0 ok, 1 a centre beyond world_radius, 2 a non-finite pose.  It waits
 * for the last update issued outside a capture (not for unrelated streams); after replaying a graph that holds an update,
 * synchronise that stream first.  Two updates are ordered by the library when one of them is the host entry (it follows the
 * last direct update); two direct updates on different streams are the caller's to order.
 * nbk_edge_continuous_batch and nbk_spline_continuous_batch certify against a world that stands still DURING the call.
 *
 * nbk_world_reach_bounds_host (no GPU needed): the static reach bounds the update computes, by the same routine on the host.
 * poses (host) [W][12]; bound (host) [P] in the caller's pair order: a lower bound, over all configurations, of the distance of
 * the two cores (margins not included) -- |c - b| - reach_a - (rho_a + rho_b), planes n.(b - c) - reach_a - rho_a, with b the base
 * origin, c the pose's translation, reach_a the sum of |joint_trans| on shape a's path + |its local translation| and rho the
 * bounding radii -- and -inf for robot-robot pairs and pairs with a prismatic joint on the shape's path.
 */
int32_t nbk_model_create_movable(const nbk_model_desc *desc, double world_radius, nbk_model **out);
int32_t nbk_model_set_world_poses(nbk_model *m, const double *poses /* DEVICE [W][12] */, void *stream);
int32_t nbk_model_set_world_poses_host(nbk_model *m, const double *poses /* host [W][12] */);
int32_t nbk_model_world_status(const nbk_model *m, int32_t *status);
int32_t nbk_world_reach_bounds_host(const nbk_model_desc *desc, const double *poses /* host [W][12] */, double *bound /* [P] */);

/*
 * The float32 broadphase compiled for one robot (hipRTC, on the first validity call of a descriptor with B >= 65536 plain q
 * rows; memoised per process).  Serial chains of at most 8 joints, at most 16 shapes and 2 world shapes with a pair take it;
 * every other descriptor, NBK_NO_JIT=1, a machine without hipRTC or a failed compile keep the generic kernel (same masks).
 *   nbk_broad_kernel_used   broadphase of the descriptor's last validity call: 0 none yet, 1 generic k_broad_f32,
 *                           2 the specialised kernel, 3 another broadphase (float64 / LDS forms)
 *   nbk_broad_spec_source   (no GPU needed) the complete source the specialised kernel is compiled from for `desc`: its
 *                           length + 1, 0 when the robot does not take it, < 0 an error; up to cap - 1 bytes + NUL to buf
 *   nbk_broad_spec_source_movable   the same for the descriptor nbk_model_create_movable(desc, world_radius) makes
 *   nbk_jit_compile         (no GPU needed) compile such a source for `arch` ("gfx950") the way the library does: the size of
 *                           the code object, or < 0 (nbk_last_error has the compiler's log)
 */
int32_t nbk_broad_kernel_used(const nbk_model *m);
int64_t nbk_broad_spec_source(const nbk_model_desc *desc, char *buf, int64_t cap);
int64_t nbk_broad_spec_source_movable(const nbk_model_desc *desc, double world_radius, char *buf, int64_t cap);
int64_t nbk_jit_compile(const char *src, const char *arch);

/*
 * Batched forward kinematics of one frame.
 * Replaces nb_compute_transformation + nb_joint_transform (numbotics/robots/helpers.py:33-113) as
 * called by Arm.forward_kinematics (numbotics/robots/arm.py:369-410).
 *   path  (host) [path_len] joint indices root -> frame;  local (host) [12] constant pose after the last
 *   joint (trailing fixed joints, COM offset, a single local_pose);  local_pose (device, optional)
 *   [B][16] per-configuration right factor;  T_out (device) [B][16] row-major 4x4.
 */
int32_t nbk_fk_batch(const nbk_model *m, const double *q, int64_t B, const int32_t *path, int32_t path_len,
                     const double *local, const double *local_pose, double *T_out, void *stream);

/*
 * FK of many frames of every configuration in one sweep (additive: the reference computes one frame per call,
 * numbotics/robots/arm.py:369-410; callers that need every link pose -- visualisation, proximity bookkeeping -- loop over
 * the link names).  A frame set names each frame by the moving frame (joint index, -1 = base) it hangs off and its constant
 * 3x4 local pose (trailing fixed joints, COM offset); host arrays, copied to the device once.
 *   T_out (device) [B][n_frames][16], frame order as given.  Poses are bit-identical to nbk_fk_batch on the same frame.
 */
typedef struct nbk_frameset nbk_frameset;
int32_t nbk_frameset_create(const nbk_model *m, int32_t n_frames, const int32_t *frame_joint, const double *frame_local,
                            nbk_frameset **out);
void nbk_frameset_destroy(nbk_frameset *fs);
int32_t nbk_fk_frames_batch(const nbk_model *m, const nbk_frameset *fs, const double *q, int64_t B, double *T_out,
                            void *stream);

/*
 * Batched geometric Jacobian [v; w] of one frame.
 * Replaces nb_compute_jacobian (numbotics/robots/helpers.py:117-187) as called by Arm.jacobian
 * (numbotics/robots/arm.py:413-461).  mode 0: end pose = T*local; 1: T*local*pose[b] (local_pose);
 * 2: end position = translation of pose[b] (global_pose).  J_out (device) [B][6][n_q].
 */
int32_t nbk_jacobian_batch(const nbk_model *m, const double *q, int64_t B, const int32_t *path,
                           int32_t path_len, const double *local, int32_t mode, const double *pose,
                           double *J_out, void *stream);

/*
 * Batched Arm.inverse_kinematics (numbotics/robots/arm.py:464-552): damped least squares
 *   q <- q + J^T (J J^T + lambda I)^-1 diff,  diff = [p* - p ; vee(0.5 (R - R^T))], R = R* R_ee^T
 * (numbotics/math/spatial.py:207-212), lambda_0 = 0.1, x1.2 / failures+1 when |diff| grew, x0.5 / failures = 0 otherwise;
 * an element iterates while |diff| > tol and failures < max_failures, at most max_iter times.
 *   pose [B][16] target poses, q0 [B][n_q] starts; path / local as for nbk_fk_batch (host);
 *   limits (host, optional) [n_q][2]: clip q to [lower, upper] after every step (use_limits=True);
 *   q_out [B][n_q]; success [B] uint8 = |diff| < tol; diff_norm (optional) [B]; iters (optional) [B] int32 steps taken.
 * The 6x6 damped system is solved by an unpivoted Cholesky (the reference calls LAPACK LU): equal to rounding.
 */
int32_t nbk_ik_batch(const nbk_model *m, const double *pose, const double *q0, int64_t B, const int32_t *path,
                     int32_t path_len, const double *local, const double *limits, double tol, int32_t max_iter,
                     int32_t max_failures, double *q_out, uint8_t *success, double *diff_norm, int32_t *iters,
                     void *stream);

/*
 * Batched Arm.in_collision (numbotics/robots/arm.py:603-604): bit b of mask_bits / mask_bytes[b] is 1
 * iff min over the allowed pairs of the signed distance is < threshold (strict).  Replaces the
 * per-configuration PyBullet round trip Arm.collisions -> Chain.distance_to -> getClosestPoints
 * (arm.py:555-580, numbotics/physics/chain.py:944-969).
 * A configuration with a NaN or infinite joint value is reported as colliding.
 *   mask_bits  (device, optional) [ceil(B/64)] uint64, bit (b % 64) of word (b / 64);
 *   mask_bytes (device, optional) [B] uint8.  At least one must be given.
 */
int32_t nbk_validity_batch(const nbk_model *m, const double *q, int64_t B, double threshold,
                           uint64_t *mask_bits, uint8_t *mask_bytes, void *stream);
/*
 * Same, with caller-owned scratch.  Every batch runs as a broadphase kernel that appends the surviving
 * (configuration, pair) items to a queue in `workspace`, followed by a dense narrowphase kernel.
 * nbk_validity_workspace_bytes(m, B) gives the size needed (0 only for B = 0 or a descriptor without pairs; a call that passes
 * no workspace runs the slower fused single-kernel path).  The queue is sized
 * for the worst case (every pair of every configuration of a tile survives): up to 1 GiB, up to 8 GiB for descriptors with
 * more than 512 pairs; larger batches are processed in tiles of that size.
 * nbk_validity_batch itself keeps one internal workspace per (descriptor, stream), grown with hipMalloc on demand: calls on
 * different streams share nothing and overlap; use this variant when the memory must be the caller's (allocator pools,
 * graphs that outlive a regrowth of the internal scratch).  `workspace` must be 64-byte aligned (hipMalloc / torch allocations
 * are): NBK_ERR_INVALID otherwise.
 */
int64_t nbk_validity_workspace_bytes(const nbk_model *m, int64_t B);
int32_t nbk_validity_batch_ws(const nbk_model *m, const double *q, int64_t B, double threshold,
                              uint64_t *mask_bits, uint8_t *mask_bytes, void *workspace,
                              int64_t workspace_bytes, void *stream);

/*
 * Batched Arm.closest_to (arm.py:599-600): min signed distance and the index of the pair attaining it
 * (first minimum in pair order; -1 / +inf when there are no pairs).
 */
int32_t nbk_closest_batch(const nbk_model *m, const double *q, int64_t B, double *min_dist,
                          int32_t *argmin, void *stream);

/*
 * Batched Arm.collisions (arm.py:555-580): signed distance of every allowed pair, dist [B][P], and
 * optionally the Proximity fields (numbotics/physics/collision.py:25-32) witness [B][P][9] =
 * position on subject, position on target, unit normal from target to subject.
 */
int32_t nbk_pair_distances_batch(const nbk_model *m, const double *q, int64_t B, double *dist,
                                 double *witness, void *stream);

/*
 * Batched Arm.jacobian_proximity (numbotics/robots/arm.py:620-632) over every allowed pair: besides dist [B][P] and
 * witness [B][P][9] (as above), jrows [B][P][n_q] with
 *   jrows[b][p] = n . Jv_subject(q_b; position_on_subject) - n . Jv_target(q_b; position_on_target),
 * n = normal_target_to_subject, Jv = the linear rows of Arm.jacobian(..., global_pose=trans_mat(pos=point))
 * (numbotics/robots/helpers.py:117-187); the target term is dropped for world targets (arm.py:628).
 * These are the gradient rows of the pair distances that IrisSolver's counter-example search consumes
 * (numbotics/planning/safe_sets.py:86-121).
 */
int32_t nbk_proximity_jacobian_batch(const nbk_model *m, const double *q, int64_t B, double *dist,
                                     double *witness, double *jrows, void *stream);

/*
 * Proximity records of chosen (configuration, pair) items: the entries of nbk_proximity_jacobian_batch one asks for, bit for bit.
 * IRIS' counter-example search asks about one body pair per evaluation -- distance_to(x, link, obj)[0].distance and
 * jacobian_proximity(x, link, obj) for SLSQP, closest_to(q) and its pair for the greedy search (numbotics/planning/safe_sets.py:86-152,
 * numbotics/robots/arm.py:607-632) -- where the all-pairs entries above compute every allowed pair of every configuration.
 *   q (device) [B][n_q]; items (device) [N][2] int32 = (configuration b, user pair index p);
 *   dist (device) [N]; witness (device, optional) [N][9]; jrows (device, optional) [N][n_q] -- the fields of
 *   nbk_proximity_jacobian_batch at [b][p].
 * Items outside [0,B) x [0,P) get NaN everywhere (q and the pair tables are not read for them).  One item per lane: items that
 * name the same pair in runs of 64 (pair-major order) are the fast case for hull shapes.  Unlike the all-pairs entries this one
 * parks nothing in LDS and serves every descriptor (robots with 30+ primitives included).
 * Asynchronous: no allocation, no host synchronisation.
 */
int32_t nbk_pair_records_items(const nbk_model *m, const double *q, int64_t B, const int32_t *items, int64_t N,
                               double *dist, double *witness, double *jrows, void *stream);

/*
 * Batched DiscreteConnector.connect / steer (numbotics/planning/sampling_based/connectors.py:57-100)
 * with the default linear trajectory (numbotics/planning/trajectories.py:6-22) and
 * validity_checker = not in_collision(q, threshold).
 *   starts, goals [E][n_q]; dist (optional) [E] = distance_func(start, goal), NULL = Euclidean norm;
 *   valid [E] uint8: 1 iff every sample T = arange(0, T_f, resolution/d) U {T_f} is collision free,
 *   0 also for d <= float32 eps (the reference returns None);
 *   end (optional) [E][n_q]: goal (connect) or traj(T_f) (steer), NaN for the degenerate edge;
 *   n_samples (optional) [E] int32 = len(T).
 * Asynchronous: the sample count is only known on the device, so the launches cover the CAPACITY of the stream's edge scratch
 * (at least E * (ceil(max_distance / resolution) + 2) samples, and 1.25 x what the previous call on the stream needed, which
 * the device reports through pinned memory) and blocks beyond the true count exit at once; edges that do not fit are walked
 * by one wave each -- same results.  (Robots whose primitives exceed the LDS-parked layout -- some 30+ -- size the scratch
 * with one read-back instead and cannot be captured.)
 */
int32_t nbk_edge_validity_batch(const nbk_model *m, const double *starts, const double *goals,
                                const double *dist, int64_t E, double resolution, double max_distance,
                                int32_t mode, double threshold, uint8_t *valid, double *end,
                                int32_t *n_samples, void *stream);

/*
 * Certified ContinuousConnector (numbotics/planning/sampling_based/connectors.py:108-185 searches each sub-interval with SciPy
 * SLSQP for a t where the checker is <= 0, a local search that can miss a contact): conservative advancement on the default
 * linear trajectory q(t) = (1-t)*s + t*g, t in [0, T_f].  One (edge, pair) item per lane; each item repeats, at most max_iter times,
 *   d = signed distance of the pair at q(t) (the bits of nbk_pair_records_items);
 *   d <= threshold: COLLISION at t;  gap = (d - threshold) - slack <= 0 (or NaN): UNDECIDED at t;  mu == 0: FREE at T_f;
 *   t' = t + gap / mu >= T_f: FREE at T_f;  else t = t'
 * and stops UNDECIDED at t when the iterations run out.  mu (nbk_edge_motion_bounds_host) bounds how fast any point of either
 * shape moves relative to the deepest common frame, so |d(t) - d(t')| <= mu |t - t'|: an edge reported FREE has no
 * configuration closer than threshold.  Per edge: t_free = the smallest stop point over the pairs; status = FREE when every pair
 * is FREE, else the status of the pair that stops at t_free (COLLISION before UNDECIDED on a tie); valid = status == FREE.
 *   starts, goals [E][n_q]; dist (optional) [E], NULL = Euclidean norm; T_f, the degenerate edge (d <= float32 eps: DEGENERATE,
 *   invalid, t_free and end NaN) and `end` (optional) [E][n_q] as nbk_edge_validity_batch; there is no resolution.
 *   valid [E] uint8; t_free [E] double (also the per-edge accumulator while the call runs); status [E] int32 NBK_CA_*.
 * A descriptor without pairs reports every non-degenerate edge FREE at T_f.  NBK_ERR_INVALID for max_iter < 1, slack < 0, a NaN
 * slack / threshold / max_distance, and null or size errors.  Asynchronous and capturable: no allocation, no host synchronisation,
 * three kernels on `stream`; nothing is parked in LDS, so every descriptor is served.
 */
enum { NBK_CA_FREE = 0, NBK_CA_COLLISION = 1, NBK_CA_UNDECIDED = 2, NBK_CA_DEGENERATE = 3 };
int32_t nbk_edge_continuous_batch(const nbk_model *m, const double *starts, const double *goals, const double *dist, int64_t E,
                                  double max_distance, int32_t mode, double threshold, int32_t max_iter, double slack,
                                  uint8_t *valid, double *end, double *t_free, int32_t *status, void *stream);
/*
 * The motion bounds mu [E][P] (user pair order) that nbk_edge_continuous_batch advances with, computed on the host by the same
 * routine from the descriptor alone (no GPU needed).  starts, goals (host) [E][n_q].  For pair p = (shape a, shape or world
 * shape b), Ja / Jb = the joints on a's / b's path and not on the other's; mu = sum over j in Ja, then Jb (joint index
 * ascending) of c_j |g - s|_qidx(j), with c_j = |joint_slide_j| for a prismatic joint and, for a revolute one, the bound
 * sum_{k below j on the path} (|joint_trans_k| + |joint_slide_k| max(|s|, |g|)_qidx(k) [prismatic k]) + |local translation| +
 * (rho + margin) on the distance from joint j's origin to the shape.
 */
int32_t nbk_edge_motion_bounds_host(const nbk_model_desc *desc, const double *starts, const double *goals, int64_t E, double *mu);

/*
 * Sampled collision check of clamped B-spline trajectories -- the smoothed references unit_bspline builds from a planner's
 * waypoints (numbotics/planning/trajectories.py:6-22; numbotics_amd.planning.unit_bspline / UnitBSpline).
 *   ctrl (device) [S][n_ctrl][n_q]: the control points of S trajectories; degree k, 1 <= k <= NBK_MAX_SPLINE_DEGREE, and
 *   k < n_ctrl <= 65536; knots (HOST) [n_ctrl + k + 1] = tau, shared by all S: finite, nondecreasing, tau[0..k] = 0 and
 *   tau[n_ctrl..n_ctrl+k] = 1 (clamped on [0, 1]); resolution > 0 and finite.  Anything else: NBK_ERR_INVALID.
 * Per trajectory, in float64, every operation in this order (the only fused multiply-add is the one named):
 *   1. speed bound: for i = 0 .. n-2 with den_i = tau[i+k+1] - tau[i+1] > 0 (others are skipped):
 *      acc = fma(df, df, acc) over the joints in order, df = ctrl[i+1][c] - ctrl[i][c] (the edge length's accumulation),
 *      v_i = ((double)k * sqrt(acc)) / den_i;  V = max v_i, NaN when any v_i is NaN.  |q'(t)| <= V.
 *   2. degenerate when !(V > 2^-23 && V <= DBL_MAX) (the edge rule with d := V): valid 0, n_samples 0, t_hit NaN.
 *   3. samples: step = resolution / V, m = ceil(1.0 / step), t_j = (double)j * step for j < m, t_m = 1.0; n_samples = m + 1
 *      (np.append(np.arange(0, 1, step), 1.0)).
 *   4. q_j = spline(t_j), one joint at a time as the general branch of UnitBSpline.__call__: span ell = (number of knots <= t) - 1
 *      clamped to [k, n-1]; r = 1..k, j = k down to r: den = tau[j+1+ell-r] - tau[j+ell-k], alpha = 0 when den == 0 else
 *      (t - tau[j+ell-k]) / den, d[j] = (1 - alpha) * d[j-1] + alpha * d[j] in four separately rounded operations.
 *   5. hit_j = the nbk_validity_batch verdict for q_j at `threshold` (a non-finite q_j collides); valid [S] uint8 = no hit_j;
 *      t_hit (optional) [S] = t_j of the smallest colliding j, NaN when valid; n_samples (optional) [S] int32.
 * With n_ctrl = 2, k = 1, tau = [0, 0, 1, 1] this is nbk_edge_validity_batch in connect mode with dist = NULL, bit for bit.
 * SYNCHRONOUS by design, an exception like the *_host conveniences: the sample total is read back (8 bytes) to size the mask
 * words and the tiles; the call returns after that read-back and the launches (plan, scan, then per tile of at most 2^20
 * samples: de Boor rows into the stream's scratch + the validity pipeline, then one reduction).  Scratch is the stream's own set
 * (grown as nbk_validity_batch's is); it holds one tile of q rows and one bit per sample.  On a capturing stream the call returns
 * NBK_ERR_UNSUPPORTED before any synchronisation or allocation (the capture stays usable); S = 0 returns NBK_OK at once; a total
 * of 2^31 samples or more, or S >= 2^26, returns NBK_ERR_UNSUPPORTED (split the batch).  Every descriptor is served.
 */
#define NBK_MAX_SPLINE_DEGREE 5
int32_t nbk_spline_validity_batch(const nbk_model *m, const double *ctrl, int64_t S, int32_t n_ctrl, int32_t degree,
                                  const double *knots /* host [n_ctrl + degree + 1] */, double resolution, double threshold,
                                  uint8_t *valid, double *t_hit /* optional */, int32_t *n_samples /* optional */, void *stream);

/*
 * Certified continuous check of clamped B-spline trajectories: the loop of nbk_edge_continuous_batch on the spline of
 * nbk_spline_validity_batch, so that a smoothed plan keeps the certificate its raw edges had.
 *   ctrl (device) [S][n_ctrl][n_q], degree k and the knots tau [n_ctrl + k + 1] as nbk_spline_validity_batch, except that the knots
 *   are a DEVICE array (the call reads nothing back).  One (trajectory, pair) item per lane, pair-major; each item starts at t = 0
 *   and makes at most max_iter distance evaluations:
 *     d = signed distance of the pair at q(t) (the bits of nbk_pair_records_items), q(t) by de Boor with the span rule and the
 *       operation order of nbk_spline_validity_batch step 4;
 *     d <= threshold: COLLISION at t;  gap = (d - threshold) - slack <= 0 (or NaN): UNDECIDED at t;
 *     else t advances across spans, spending gap: in span ell (the span of t) with hi = tau[ell + 1] and mu = mu[ell]
 *       (nbk_spline_motion_bounds_host): mu == 0: t = hi;  else tn = t + gap / mu; unless tn >= hi: t = tn and the advance ends;
 *       else gap = gap - mu * (hi - t) (two roundings) and t = hi.  Once t >= 1 the item stops FREE at 1; else when !(gap > 0) the
 *       advance ends; else it goes on in the span of the new t.  Crossing a span costs no distance evaluation;
 *   and stops UNDECIDED at t when the iterations run out.  An item also stops, without a say in the result, once its t passes the
 *   trajectory's current smallest stop point.  Per trajectory: t_free = the smallest stop point over the pairs; status NBK_CA_* =
 *   FREE when every pair is FREE, else the status of the pair that stops at t_free (COLLISION before UNDECIDED on a tie); valid =
 *   status == FREE.  valid [S] uint8; t_free [S] double (also the per-trajectory accumulator while the call runs); status [S] int32.
 * Degenerate (DEGENERATE, invalid, t_free NaN): V outside (2^-23, DBL_MAX] (nbk_spline_validity_batch steps 1-2), a non-finite
 * control point, or -- for every trajectory -- knots that are not finite, nondecreasing and clamped on [0, 1] (checked on the
 * device).  A descriptor without pairs reports every other trajectory FREE at 1.  With n_ctrl = 2, k = 1, tau = [0, 0, 1, 1] this
 * is nbk_edge_continuous_batch in connect mode with dist = NULL, bit for bit.  NBK_ERR_INVALID for max_iter < 1, slack < 0, a NaN
 * slack / threshold, degree outside 1 .. NBK_MAX_SPLINE_DEGREE, n_ctrl <= degree or > 65536, and null pointers; S = 0 returns
 * NBK_OK at once.  Asynchronous and capturable: no allocation, no host synchronisation, three kernels on `stream`; nothing is
 * parked in LDS, so every descriptor is served.
 */
int32_t nbk_spline_continuous_batch(const nbk_model *m, const double *ctrl, int64_t S, int32_t n_ctrl, int32_t degree,
                                    const double *knots /* DEVICE, n_ctrl + degree + 1 */, double threshold,
                                    int32_t max_iter, double slack, uint8_t *valid, double *t_free, int32_t *status,
                                    void *stream);
/*
 * The motion bounds mu [S][n_ctrl - degree][P] (span ell at index ell - degree, user pair order) that nbk_spline_continuous_batch
 * advances with, computed on the host by the same routine (no GPU needed).  ctrl, knots (host); the knots must pass the rules of
 * nbk_spline_validity_batch (NBK_ERR_INVALID otherwise).  On a non-empty span ell (tau[ell] < tau[ell+1]), with
 *   V_j = max_{i = ell-k .. ell-1} ((double)k * |c_{i+1} - c_i|_j) / (tau[i+k+1] - tau[i+1])   (three roundings per term)
 *   A_j = max_{i = ell-k .. ell} |c_i|_j,
 * mu is the formula of nbk_edge_motion_bounds_host with |g - s|_j replaced by V_j and the prismatic travel max(|s|, |g|)_j by A_j;
 * then |d_p(t) - d_p(t')| <= mu |t - t'| on the span.  Entries of empty spans are 0 (never used).
 */
int32_t nbk_spline_motion_bounds_host(const nbk_model_desc *desc, const double *ctrl /* host */, int64_t S, int32_t n_ctrl,
                                      int32_t degree, const double *knots /* host */, double *mu /* [S][n_ctrl-degree][P] */);

/*
 * Point-cloud obstacles (additive; the reference has no such obstacle: a depth camera's scan would be one sphere body per point).
 * A cloud is N points of ONE radius in a uniform grid on the device.  It belongs to no descriptor -- one cloud serves many robots --
 * and the entry points below look at the cloud ALONE: the descriptor's own pairs and world shapes play no part (full validity is
 * nbk_validity_batch, then nbk_cloud_validity_batch with accumulate on the same mask).
 *
 * nbk_cloud_create: the grid is lo[3], cell > 0 and dims[3] (each >= 1, product <= 2^22); the cell coordinate of x on an axis is
 * floor((x - lo) / cell) in float64 clamped to [0, dim - 1], so points outside the box land in border cells and none is dropped
 * (a box that is too small costs time, never a result).  It allocates everything the object will ever need, for up to `capacity`
 * points (1 .. 2^24).  NBK_ERR_INVALID -- before any device is looked for -- for a null pointer, a capacity out of range, a NaN or
 * non-positive cell, a non-finite lo, a dim below 1 or more than 2^22 cells.
 *
 * nbk_cloud_set_points: pts (DEVICE) [N][3].  Asynchronous, no allocation, no host synchronisation, capturable: a memset, then
 * count, scan and scatter kernels in `stream`'s order; queries issued to that stream afterwards see the new points and radius
 * (both live on the device: a replayed graph that holds an update sets them for the queries behind it).  Queries on OTHER streams
 * are the caller's to order, in both directions, as for nbk_model_set_world_poses.  N = 0 empties the cloud.  NBK_ERR_INVALID for
 * N > capacity, a NaN or negative radius, or null pts with N > 0.  A non-finite coordinate sets the cloud's status (2); while it is
 * set every configuration is reported colliding and the clearance outputs are NaN / -1 / -1, whatever the other points are; the
 * next update whose points are all finite clears it.  nbk_cloud_status: synchronous read (it waits for the last update issued outside a
 * capture, by an event of the cloud's own: that update's stream may be gone by then; after replaying a graph that holds an update, synchronise that stream first).
 *
 * nbk_cloud_validity_batch: bit b is the OR, over the selected robot shapes s and the points i, of the pair predicate of
 * nbk_validity_batch for (shape s, a sphere world shape of radius `radius` at p_i) -- bit for bit what a descriptor with those N
 * spheres as world shapes and those pairs reports.  A configuration with a non-finite joint value collides.
 *   shape_bits (HOST, optional) ceil(S / 64) words, bit s = robot shape s of the descriptor as it was given to nbk_model_create;
 *   NULL = every robot shape.  With a selection S must be at most 256 (NBK_ERR_UNSUPPORTED otherwise).
 *   accumulate != 0: OR into the caller's mask instead of overwriting it (bits beyond B in the last word: written 0 when
 *   overwriting, left alone when accumulating).  At least one of mask_bits / mask_bytes must be given.
 * nbk_cloud_clearance_batch: per configuration the minimum over the selected (s, i) of the signed distance of that pair (the bits of
 * nbk_pair_distances_batch for it), reported if and only if it is < d_max (finite: NBK_ERR_INVALID otherwise), with its shape
 * (the caller's index) and the point's index in the array given to the last update; on equal distances the smallest shape, then the
 * smallest point index.  Otherwise +inf, -1, -1 (an empty cloud, an empty selection).  A non-finite configuration or a set status:
 * NaN, -1, -1.  shape / point are optional.
 * Both are asynchronous and capturable (no allocation, no synchronisation, one kernel); nothing is parked in LDS beyond the staged
 * q rows, so every descriptor is served.  The descriptor's and the cloud's device must be current.
 *
 * nbk_cloud_cells_host (no GPU needed): the cell index ((z * dims[1] + y) * dims[0] + x) of each of N HOST points, by the routine
 * the device uses.
 */
typedef struct nbk_cloud nbk_cloud;
int32_t nbk_cloud_create(int64_t capacity, const double lo[3], double cell, const int32_t dims[3], nbk_cloud **out);
void nbk_cloud_destroy(nbk_cloud *c);
int32_t nbk_cloud_set_points(nbk_cloud *c, const double *pts /* DEVICE [N][3] */, int64_t N, double radius, void *stream);
int32_t nbk_cloud_status(const nbk_cloud *c, int32_t *status);   /* synchronous: 0 ok, 2 a non-finite point */
int32_t nbk_cloud_validity_batch(const nbk_model *m, const nbk_cloud *c, const double *q, int64_t B, double threshold,
                                 const uint64_t *shape_bits /* host, ceil(S/64) words, NULL = every robot shape */,
                                 int32_t accumulate, uint64_t *mask_bits, uint8_t *mask_bytes, void *stream);
int32_t nbk_cloud_clearance_batch(const nbk_model *m, const nbk_cloud *c, const double *q, int64_t B, double d_max,
                                  const uint64_t *shape_bits, double *min_dist /* [B] */, int32_t *shape /* [B] */,
                                  int32_t *point /* [B] */, void *stream);
int32_t nbk_cloud_cells_host(const double lo[3], double cell, const int32_t dims[3], const double *pts, int64_t N,
                             int32_t *cell_out);                 /* no GPU: the same routine, for tests */

/*
 * Depth frames to a cloud (additive): back-projection, the robot's own image taken out, and an update that honours the mask.  Three
 * stream-ordered steps in caller memory: no allocation, no host synchronisation, capturable; point i of a frame is pixel
 * i = v * W + u all the way, so the `point` of a clearance record names a pixel.  (Named nbk_frame_cloud_*, like the siblings over
 * edges, splines and records: the nbk_cloud_* names are the cloud object's own first set.)
 *
 * nbk_frame_cloud_backproject: depth (DEVICE) [H][W], depth_type 0 = float32, 1 = uint16 raw units; a pinhole fx, fy, cx, cy in the OPTICAL
 * frame (z forward, x right, y down) whose world pose is T (DEVICE, [3][4] row-major: read when the kernel runs, so a replayed graph
 * follows a pose rewritten in place).  Depth is metric along the view axis.  In float64, every operation rounded once, in this order:
 *     z  = (double)d * depth_scale;   xc = (((double)u - cx) * z) / fx;   yc = (((double)v - cy) * z) / fy;
 *     pts[i][e] = ((T[e][0] * xc + T[e][1] * yc) + T[e][2] * z) + T[e][3]
 * keep[i] = 1 iff z is finite, z > z_min and z <= z_max; otherwise keep[i] = 0 and pts[i] = (0, 0, 0) (a hole: 0, NaN, out of range).
 * NBK_ERR_INVALID -- before any device is looked for -- for H or W < 0, H * W > 2^24, an unknown depth_type, fx, fy or depth_scale
 * not positive (NaN included), a null T, or null depth / pts / keep with H * W > 0.  nbk_frame_cloud_backproject_host (no GPU needed): the
 * same routine on HOST arrays, T included.
 *
 * nbk_frame_cloud_self_filter: q0 (DEVICE) [n_q], pts (DEVICE) [N][3], keep (DEVICE) [N] read and written.  keep[i] stays 0 where it is 0;
 * else it becomes 0 iff for some selected robot shape s the predicate of nbk_cloud_validity_batch holds for (s, a sphere of `radius`
 * at pts[i]) at q0 with threshold = padding -- the same statements in the same order, so a cloud of the points kept reads free at
 * (q0, padding, the same selection), exactly.  A non-finite q0 removes nothing; a non-finite point is left as it is (the masked
 * update raises the status for it).  shape_bits as nbk_cloud_validity_batch.  One kernel: the selected shapes' cores at q0 are built
 * once per workgroup into LDS (168 bytes a shape); NBK_ERR_UNSUPPORTED when they do not fit 160 KB.  NBK_ERR_INVALID -- before any
 * device is looked for -- for a null m or q0, N < 0 or > 2^24, a NaN or negative radius, a NaN padding, null pts / keep with N > 0.
 * nbk_frame_cloud_self_filter_lds_bytes (no GPU needed): that kernel's LDS for n_shapes selected shapes, -1 when the entry refuses them.
 *
 * nbk_frame_cloud_set_points: nbk_cloud_set_points with keep (DEVICE) [N]; NULL = nbk_cloud_set_points, which is this call.  A
 * point with keep[i] == 0 is neither counted, nor stored, nor checked for finiteness; the cloud holds the others under their
 * ORIGINAL indices i (what nbk_cloud_clearance_batch reports).  `capacity` bounds N, the points submitted.
 * nbk_frame_cloud_count: the points the cloud holds (those kept); synchronous, as nbk_cloud_status.
 */
int32_t nbk_frame_cloud_backproject(const void *depth /* DEVICE [H][W] */, int32_t depth_type, int32_t H, int32_t W, double depth_scale,
                              double fx, double fy, double cx, double cy, const double *T /* DEVICE [3][4] */, double z_min,
                              double z_max, double *pts /* DEVICE [H*W][3] */, uint8_t *keep /* DEVICE [H*W] */, void *stream);
int32_t nbk_frame_cloud_backproject_host(const void *depth, int32_t depth_type, int32_t H, int32_t W, double depth_scale, double fx,
                                   double fy, double cx, double cy, const double *T, double z_min, double z_max, double *pts,
                                   uint8_t *keep);               /* no GPU: the same routine on host arrays */
int32_t nbk_frame_cloud_self_filter(const nbk_model *m, const double *q0 /* DEVICE [n_q] */, const double *pts /* DEVICE [N][3] */,
                              int64_t N, double radius, double padding, const uint64_t *shape_bits /* host */,
                              uint8_t *keep /* DEVICE [N], in and out */, void *stream);
int64_t nbk_frame_cloud_self_filter_lds_bytes(int32_t n_shapes);       /* no GPU */
int32_t nbk_frame_cloud_set_points(nbk_cloud *c, const double *pts /* DEVICE [N][3] */, const uint8_t *keep /* DEVICE [N] or NULL */,
                                    int64_t N, double radius, void *stream);
int32_t nbk_frame_cloud_count(const nbk_cloud *c, int64_t *n);         /* synchronous: the points held */

/*
 * Fused frames (additive): several depth frames in one cloud.  The caller keeps a STORE of M point slots in device memory -- store_pts
 * [M][3], store_keep [M]: slot j is held iff store_keep[j] != 0 -- and makes the cloud of it with nbk_frame_cloud_set_points at
 * N = M.  That update files a point under its index in the submitted array, so the `point` of every clearance or proximity record
 * is a SLOT, and a point keeps its slot for as long as it lives.  Three stream-ordered steps maintain the store; like the entries
 * above they allocate nothing, synchronise nothing and may be captured.  They write masks, indices and copies of doubles: every
 * result is exact.  One frame: backproject | self_filter on the frame | carve | (self_filter on the store) | novel | append | set_points.
 *
 * nbk_frame_cloud_carve: a held slot the new frame sees THROUGH is released.  The image and the camera as nbk_frame_cloud_backproject
 * takes them (T in DEVICE memory); store_pts (DEVICE) [M][3], store_keep (DEVICE) [M], the only thing written.  In float64, every
 * operation rounded once, in this order, for the point p of slot i:
 *     d[e] = p[e] - T[e][3]
 *     xc = (T[0][0] * d[0] + T[1][0] * d[1]) + T[2][0] * d[2];   yc, zc: the same with columns 1 and 2 of T   (R^T d: the rotation
 *                                                                 of T is taken to be orthonormal and is not checked)
 *     u = floor(((xc * fx) / zc + cx) + 0.5);   v = floor(((yc * fy) / zc + cy) + 0.5)                          (kept as doubles)
 * store_keep[i] becomes 0 iff it was not 0, and zc > z_min, and u - window >= 0, u + window <= W - 1, v - window >= 0,
 * v + window <= H - 1 (compared as doubles: NaN and huge values fall out), and EVERY pixel of the (2 window + 1)^2 window around
 * (u, v) is valid by the back-projection's test with (z_m - zc) > margin, z_m = (double)raw * depth_scale.  A hole anywhere in the
 * window is no evidence: the point stays; so does a point behind the surface, outside the image, or non-finite.  NBK_ERR_INVALID --
 * before any device is looked for -- by the image and camera rules of nbk_frame_cloud_backproject, for a NaN or infinite margin, window
 * < 0 or > 8, M < 0 or > 2^24, null store_pts / store_keep with M > 0.  nbk_frame_cloud_carve_host (no GPU needed): the same routine on
 * HOST arrays, T included.
 *
 * nbk_frame_cloud_novel: pts (DEVICE) [N][3], keep (DEVICE) [N] read and written: keep[i] becomes 0 iff it was not 0 and the cloud
 * holds a sorted point s with (held == NULL or held[original index of s] != 0) and
 *     ((dx * dx + dy * dy) + dz * dz) < merge * merge,   dx = pts[i][0] - cloud point s [0], ...      (strict; float64, rounded once each)
 * held (DEVICE, optional): one byte per point SUBMITTED to the cloud's last update -- the store's mask: the cloud as that update
 * left it, less the slots released since.  The cloud's N, status and grid are read on the device, so in a graph this step sees the
 * update before it; while the status is set or the cloud is empty nothing is read and keep stays.  merge <= 0 drops nothing; a
 * non-finite point keeps its 1 (the update raises the status for it).  Frame points are not thinned against each other.
 * NBK_ERR_INVALID for a null c, N < 0 or > 2^24, a NaN merge, null pts / keep with N > 0.
 *
 * nbk_frame_cloud_append: F = the ascending slots j < M with store_keep[j] == 0, A = the ascending i < N with new_keep[i] != 0; for
 * k < min(|F|, |A|): store_pts[F[k]] = new_pts[A[k]] (three doubles copied) and store_keep[F[k]] = 1.  counts (DEVICE) int64[3] =
 * (slots held afterwards, appended, dropped = |A| - appended); slot_of (DEVICE, optional) int32[N] = F[k] for A[k], -1 for a point
 * not kept or dropped; new_pts and new_keep are not modified; untouched slots keep their bytes.  Deterministic: ranks of a two-level
 * scan, no atomics; both lists' ranks are complete in the workspace before a slot is written.  workspace (DEVICE): at least
 * nbk_frame_cloud_append_workspace_bytes (no GPU needed; -1 for M < 1, N < 0 or either > 2^24) bytes at a 64-byte boundary.
 * NBK_ERR_INVALID for those sizes, a null store_pts / store_keep / counts / workspace, null new_pts / new_keep with N > 0, a workspace
 * too small or misaligned.
 */
int32_t nbk_frame_cloud_carve(const void *depth /* DEVICE [H][W] */, int32_t depth_type, int32_t H, int32_t W, double depth_scale,
                              double fx, double fy, double cx, double cy, const double *T /* DEVICE [3][4] */, double z_min,
                              double z_max, double margin, int32_t window, const double *store_pts /* DEVICE [M][3] */, int64_t M,
                              uint8_t *store_keep /* DEVICE [M], in and out */, void *stream);
int32_t nbk_frame_cloud_carve_host(const void *depth, int32_t depth_type, int32_t H, int32_t W, double depth_scale, double fx, double fy,
                                   double cx, double cy, const double *T, double z_min, double z_max, double margin, int32_t window,
                                   const double *store_pts, int64_t M, uint8_t *store_keep);     /* no GPU: the same routine */
int32_t nbk_frame_cloud_novel(const nbk_cloud *c, const double *pts /* DEVICE [N][3] */, int64_t N, double merge,
                              const uint8_t *held /* DEVICE or NULL */, uint8_t *keep /* DEVICE [N], in and out */, void *stream);
int64_t nbk_frame_cloud_append_workspace_bytes(int64_t M, int64_t N);  /* no GPU */
int32_t nbk_frame_cloud_append(double *store_pts /* DEVICE [M][3] */, uint8_t *store_keep /* DEVICE [M] */, int64_t M,
                               const double *new_pts /* DEVICE [N][3] */, const uint8_t *new_keep /* DEVICE [N] */, int64_t N,
                               int64_t *counts /* DEVICE [3] */, int32_t *slot_of /* DEVICE [N] or NULL */, void *workspace,
                               int64_t workspace_bytes, void *stream);

/*
 * Rendered frames (additive): depth frames of the device scene, ray-cast.  Replaces World.depth_image (numbotics/physics/world.py:
 * 363-398: computeViewMatrix, computeProjectionMatrixFOV, getCameraImage and the linearisation of its depth buffer) for the shapes a
 * descriptor holds, and produces what nbk_frame_cloud_backproject consumes: the same pinhole, the same optical pose, depth along the
 * view axis.  The scene of frame b is the selected robot shapes at row b of q (shape_bits as nbk_cloud_validity_batch) and, with
 * draw_world != 0, the world shapes; q and T have B rows or one row that serves every frame (Bq, Bt).  One kernel, no allocation, no
 * host synchronisation, capturable; q and T are read when the kernel runs.
 *
 * The surface is the set the collision predicates call distance 0: a pixel's ray is sphere-traced on the library's exact shape
 * distance.  The point at depth z on pixel (u, v) is the back-projection's, xc = (((double)u - cx) * z) / fx, ... (depth_scale 1).
 * With L = sqrt(((u - cx) / fx)^2 + ((v - cy) / fy)^2 + 1) and R = (rho + margin) + (1e-6 |rho + margin| + 1e-7) of a shape's
 * bounding ball, the ray's candidates are the shapes (planes apart) for which the span below is not empty; z starts at the smallest
 * z0 and a step takes d, the minimum over the candidates, in the drawn order (selected robot shapes in the descriptor's device
 * order, then world shapes), of the signed distance from the point to the shape.  d < eps: a hit at this z, labelled with the first
 * shape that attains the minimum; otherwise z += d / L.  Past the largest z1, a nearer plane hit or z_far: a miss.  max_steps steps
 * without a decision: unresolved.  A ray that starts inside a shape, or within eps of it, hits at its start (z_near at the least).
 * Planes are intersected in closed form (h = n . (p(z_near) - c): h < eps hits at z_near; else z_near + h / -(n . w) where the ray
 * descends, w the ray per unit depth in the world); a plane hit wins only where it is strictly nearer than the march's.
 *
 * depth (DEVICE) float32 [B][H][W]: the depth of a hit, `miss` otherwise.  label (DEVICE, optional) int32 [B][H][W]: the robot
 * shape in the caller's order, n_rshapes + w for world shape w, -1 for a miss, -2 for an unresolved pixel.  counts (DEVICE, optional)
 * int64 [3], cleared by the call: hit pixels, unresolved pixels, distance evaluations (integer sums: deterministic).  A frame whose q
 * row or pose is not finite, and every frame while the world status of a movable descriptor is set, is unresolved in every pixel.
 * Every pixel's result depends on its own ray alone (u - cx, v - cy, the pose, the scene): not on the image size or its tiles.
 *
 * nbk_render_ray_spans_host (no GPU needed): the span routine on HOST arrays.  For pixel i = v * W + u and ball s (centres [S][3],
 * radii [S]: R as given), in float64, every operation rounded once, in this order:
 *     ax = ((double)u - cx) / fx;  ay = ((double)v - cy) / fy;  A = (ax * ax + ay * ay) + 1
 *     d[e] = c[e] - T[e][3];  xc = (T[0][0] * d[0] + T[1][0] * d[1]) + T[2][0] * d[2];  yc, zc: columns 1 and 2 (as nbk_frame_cloud_carve)
 *     B = (ax * xc + ay * yc) + zc;  C = ((xc * xc + yc * yc) + zc * zc) - R * R;  D = B * B - A * C
 *     hit iff D >= 0 and z0 <= z1 for z0 = max((B - sqrt(D)) / A, z_near), z1 = min((B + sqrt(D)) / A, z_far)
 * hit[i][s] = 1 and span[i][s] = (z0, z1), or 0 and (0, 0).  NBK_ERR_INVALID for H, W or S < 0, focal lengths not positive, a null T,
 * z_near < 0, z_far <= z_near, or a null array that would be read or written.
 *
 * nbk_render_depth_lds_bytes (no GPU needed): the kernel's LDS for a scene of n_shapes selected robot shapes and no world shape
 * (each world shape drawn adds 48 bytes), -1 for n_shapes < 0 or when it does not fit 160 KB: the entry answers NBK_ERR_UNSUPPORTED.
 * NBK_ERR_INVALID -- before any device is looked for -- for a null m, T, depth (or q on a model with joints) with B * H * W > 0,
 * H, W or B < 0, focal lengths or eps not positive (NaN included), z_near < 0, z_far <= z_near, max_steps outside 1..4096, Bq or Bt
 * not in {1, B}, B * H * W >= 2^31.  H * W = 0 or B = 0 does nothing.
 */
int64_t nbk_render_depth_lds_bytes(int32_t n_shapes);                   /* no GPU */
int32_t nbk_render_ray_spans_host(int32_t H, int32_t W, double fx, double fy, double cx, double cy, const double *T,
                                  const double *centres /* [S][3] */, const double *radii /* [S] */, int32_t S, double z_near,
                                  double z_far, double *span /* [H*W][S][2] */, uint8_t *hit /* [H*W][S] */);   /* no GPU */
int32_t nbk_render_depth_batch(const nbk_model *m, const double *q /* DEVICE [Bq][n_q], Bq = B or 1 */, int64_t Bq,
                               const double *T /* DEVICE [Bt][12] optical poses, Bt = B or 1 */, int64_t Bt, int64_t B, int32_t H,
                               int32_t W, double fx, double fy, double cx, double cy, double z_near, double z_far, double eps,
                               int32_t max_steps, const uint64_t *shape_bits /* host, NULL = all */, int32_t draw_world, float miss,
                               float *depth /* DEVICE [B][H][W] */, int32_t *label /* DEVICE [B][H][W] or NULL */,
                               int64_t *counts /* DEVICE [3] or NULL */, void *stream);

/*
 * Proximity records against a cloud: nbk_cloud_clearance_batch's record with WHERE the contact is and WHICH WAY to move -- what
 * nbk_proximity_jacobian_batch / nbk_pair_records_items give for the scene's pairs.  (Named like its siblings over edges and splines,
 * nbk_<what>_cloud_*: the nbk_cloud_* names are the cloud object's own set.)
 *   q (device) [B][n_q]; d_max finite; shape_bits (HOST, optional) as nbk_cloud_clearance_batch.
 *   per_shape == 0, one record per configuration: dist [B], shape [B], point [B], witness [B][9], jrows [B][n_q] (all device);
 *     dist, shape and point are the bits of nbk_cloud_clearance_batch for the same arguments, its tie rule included (smallest shape,
 *     then smallest point index).
 *   per_shape != 0, one record per (configuration, selected shape): [B][n_sel], [B][n_sel][9], [B][n_sel][n_q]; column j is the j-th
 *     selected shape in ascending caller's index, and each entry is what nbk_cloud_clearance_batch reports for that shape selected
 *     alone with the same d_max -- the form a per-link constraint takes.
 *   witness and jrows belong to the winning (shape s, point i): the witness and jrows bits of nbk_proximity_jacobian_batch on a
 *     descriptor that holds point i as a sphere world shape of the cloud's radius (identity rotation), paired with s.  witness =
 *     position on the robot shape, position on the point's sphere, unit normal from target to subject; jrows = n . Jv_subject(position
 *     on subject) -- the cloud is a world target, so there is no target term.
 *   nothing nearer than d_max (an empty cloud and an empty selection included): +inf, -1, -1, witness NaN, jrows all +0.0 -- the
 *     gradient of a hinge cost, so rows can be weighted without a mask.  per_shape with an empty selection writes nothing.
 *   a non-finite configuration or a set cloud status: NaN, -1, -1, NaN, NaN.
 *   shape, point, witness and jrows are each optional.
 * NBK_ERR_INVALID -- before any device is looked for -- for a null m or c, B < 0, a non-finite d_max, or null q / dist with B > 0;
 * B == 0 returns NBK_OK at once.  NBK_ERR_UNSUPPORTED for a selection on a descriptor of more than 256 robot shapes.
 * Asynchronous and capturable: no allocation, no host synchronisation, one kernel on `stream`.  Nothing is parked in LDS beyond the
 * q rows and (with jrows) the joint rows, 8 * 64 * (n_q + 6 n_joints) bytes, so every descriptor is served.
 */
int32_t nbk_records_cloud_batch(const nbk_model *m, const nbk_cloud *c, const double *q, int64_t B, double d_max,
                                const uint64_t *shape_bits /* host, as nbk_cloud_clearance_batch */, int32_t per_shape,
                                double *dist, int32_t *shape, int32_t *point, double *witness /* optional */,
                                double *jrows /* optional */, void *stream);

/*
 * Sampled straight-line edges against a cloud: nbk_edge_validity_batch's edges, nbk_cloud_validity_batch's verdict per sample -- what
 * a planner's connector asks about a scan.  The samples are generated on the device and never written down as q rows.
 *   starts, goals (device) [E][n_q]; dist (device, optional) [E]; the edge rule is nbk_edge_validity_batch's, word for word:
 *   d = dist[e] or the fma-accumulated norm; degenerate when !(d > 2^-23 && d <= DBL_MAX); T_f = max_distance / d when steering
 *   further than max_distance, else 1; step = resolution / d, n = ceil(T_f / step); samples t_i = i * step for i < n and t_n = T_f;
 *   q = (1 - t) * s + t * g in three separately rounded operations per joint.  end (optional) [E][n_q] and n_samples (optional) [E]
 *   get the bits that function writes: NaN / 0 for the degenerate edge, the goal or traj(T_f) and n + 1 otherwise.
 *   valid [E] uint8 = 1 iff the edge is not degenerate and no sample's nbk_cloud_validity_batch verdict (same cloud, threshold and
 *   shape_bits: NULL = every robot shape, a selection needs S <= 256) is 1 -- bit for bit what a descriptor reports through
 *   nbk_edge_validity_batch when it holds the points as sphere world shapes paired with the selected robot shapes.  A non-finite
 *   sample collides; a set cloud status makes every non-degenerate edge invalid; an empty cloud or an empty selection leaves every
 *   non-degenerate edge valid.  (An edge of 2^32 samples or more is reported invalid.)
 *   accumulate != 0: valid is only ever lowered -- an entry that is 0 on entry stays 0 and its samples are not looked at (the fast
 *   path after the scene has rejected the edge), a non-zero entry ends as 1 or 0 by the rule above: nbk_edge_validity_batch followed
 *   by this call on the same `valid` is full edge validity.  accumulate == 0 overwrites.
 *   workspace: caller-owned device memory of at least nbk_edge_cloud_workspace_bytes(E) bytes (no GPU needed; < 0 for E < 0), 64-byte
 *   aligned: the plan, the counts and the offsets, 40 bytes per edge whatever the sample count.  The descriptor's per-stream
 *   scratch is not touched.
 * Asynchronous, no allocation, no host synchronisation, capturable for every descriptor (nothing is parked in LDS beyond the staged
 * q rows): four kernels on `stream` -- plan, scan, the initial valid, then one sample per lane, flat across the edges, over a grid
 * sized from the static bound E * (ceil(max_distance / resolution) + 2); a batch with more samples than that is served completely
 * by the same kernel's stride (the host never learns the count).
 * NBK_ERR_INVALID -- before any device is looked for -- for null m / c, E < 0, null starts / goals / valid / workspace with E > 0,
 * !(resolution > 0), !(max_distance > 0), a mode other than connect / steer, a NaN threshold, a workspace that is too small or
 * misaligned.  E = 0 returns NBK_OK at once.  NBK_ERR_UNSUPPORTED for E > 2^31 - 1 and for a selection with S > 256.  The
 * descriptor's and the cloud's device must be current.
 */
int64_t nbk_edge_cloud_workspace_bytes(int64_t E);
int32_t nbk_edge_cloud_validity_batch(const nbk_model *m, const nbk_cloud *c, const double *starts, const double *goals,
                                      const double *dist /* optional */, int64_t E, double resolution, double max_distance,
                                      int32_t mode, double threshold, const uint64_t *shape_bits /* host, optional */,
                                      int32_t accumulate, uint8_t *valid, double *end /* optional */,
                                      int32_t *n_samples /* optional */, void *workspace, int64_t workspace_bytes, void *stream);

/*
 * Certified continuous edges against a cloud: nbk_edge_continuous_batch's edges (T_f, the degenerate rule, `end`, the keys in
 * t_free while the call runs) and its loop, unchanged, on one (edge e, selected robot shape s) item per lane; the cloud ALONE is
 * looked at.  shape_bits as nbk_cloud_validity_batch (caller's numbering, NULL = every robot shape, a selection needs S <= 256).
 *   mu_s (nbk_edge_shape_motion_bounds_host) bounds how fast any point of shape s moves in the world, which stands still.
 *   The item's distance at t: q(t) = (1 - t) * s + t * g in three roundings per joint; a non-finite q(t) gives NaN (UNDECIDED at t);
 *   else with  D_end = (threshold + slack) + mu_s * (T_f - t),  D_cap = (threshold + slack) + look_ahead,  D = D_end < D_cap ? D_end : D_cap:
 *     some point i has signed distance (shape s, sphere of the cloud's radius at p_i) < D: d = the smallest one (the bits of
 *     nbk_cloud_clearance_batch for shape s alone with d_max = D);  else D == D_end: d = +inf (the item stops FREE at T_f);  else d = D_cap.
 *   Sound: every point of shape s moves at most mu_s |t' - t| and the cloud's points stand still, so no point within D_end at t means
 *   the distance stays above threshold + slack up to T_f; a distance >= D_cap replaced by D_cap is a lower bound, hence conservative.
 *   look_ahead > 0 (+inf allowed) bounds the ball one step searches; it changes how many steps an edge takes, never whether a
 *   reported FREE is free.
 *   Per edge the smallest stop point over the items, COLLISION before UNDECIDED on a tie, as nbk_edge_continuous_batch.
 *   accumulate == 0: an empty cloud (N = 0 on the device) or an empty selection reports every non-degenerate edge FREE at T_f.
 *   accumulate != 0: valid / t_free / status hold on entry what nbk_edge_continuous_batch wrote for the same edges with the same mode,
 *   max_distance and dist; the result is bit for bit that of ONE conservative-advancement call over the scene's pairs and the
 *   cloud's items together (items of an edge the scene stopped at t0 stop once past t0).  A non-degenerate edge that comes in with
 *   a NaN t_free (a movable world whose status is set) keeps 0 / UNDECIDED / NaN.  Degenerate edges are DEGENERATE either way.
 *   While the cloud's status is set every non-degenerate edge is invalid, UNDECIDED, t_free NaN; nothing of the grid is read.  N, the
 *   radius and the status are read from the cloud on the device, in stream order.
 * Asynchronous, no allocation, no host synchronisation, no workspace, capturable for every descriptor (LDS holds the q rows only):
 * three kernels on `stream`, the middle one on a grid of (ceil(E / 64), selected shapes).  NBK_ERR_INVALID -- before any device is
 * looked for -- for null m / c, E < 0, null starts / goals / valid / t_free / status with E > 0, max_iter < 1, slack < 0,
 * !(max_distance > 0), a mode other than connect / steer, a NaN slack / threshold, and look_ahead NaN or <= 0.  E = 0 returns NBK_OK
 * at once.  NBK_ERR_UNSUPPORTED for E > 2^31 - 1, a selection with S > 256, more than 65535 selected shapes.
 */
int32_t nbk_edge_cloud_continuous_batch(const nbk_model *m, const nbk_cloud *c, const double *starts, const double *goals,
                                        const double *dist /* optional */, int64_t E, double max_distance, int32_t mode,
                                        double threshold, int32_t max_iter, double slack, double look_ahead,
                                        const uint64_t *shape_bits /* host, optional */, int32_t accumulate, uint8_t *valid,
                                        double *end /* optional */, double *t_free, int32_t *status, void *stream);
/*
 * The motion bounds mu [E][S] (caller's robot shape order) that nbk_edge_cloud_continuous_batch advances with, on the host by the
 * same routine (no GPU needed): the formula of nbk_edge_motion_bounds_host for a pair of (shape s, a world shape) -- every joint on
 * the shape's path counts.  starts, goals (host) [E][n_q].
 */
int32_t nbk_edge_shape_motion_bounds_host(const nbk_model_desc *desc, const double *starts, const double *goals, int64_t E, double *mu);

/*
 * Sampled B-spline trajectories against a cloud: nbk_spline_validity_batch's trajectories, nbk_cloud_validity_batch's verdict per
 * sample -- re-checking a smoothed plan against the scan it was planned in.  The samples are generated on the device and never
 * written down as q rows.
 *   ctrl (device) [S][n_ctrl][n_q], degree k (1 .. NBK_MAX_SPLINE_DEGREE, k < n_ctrl <= 65536) and the knots tau [n_ctrl + k + 1], a
 *   DEVICE array here (the call reads nothing back).  The trajectory rule is nbk_spline_validity_batch steps 1-4, word for word: V,
 *   the degenerate rule, step, m, t_j, the span rule and de Boor in its operation order.
 *   hit_j = the nbk_cloud_validity_batch verdict of q_j (same cloud, threshold and shape_bits: NULL = every robot shape, a selection
 *   needs at most 256 robot shapes); a non-finite q_j collides.  valid [S] uint8 = no hit_j; t_hit (optional) [S] = t_j of the
 *   SMALLEST colliding j, NaN when valid; n_samples (optional) [S] int32 -- bit for bit what a descriptor reports through
 *   nbk_spline_validity_batch when it holds the points as sphere world shapes paired with the selected robot shapes.  A set cloud
 *   status makes every non-degenerate trajectory invalid with t_hit = 0.0 (its first sample); an empty cloud or an empty selection
 *   leaves every non-degenerate trajectory valid.
 *   Knots that are not finite, nondecreasing and clamped on [0, 1] are found on the device (the rule of
 *   nbk_spline_continuous_batch) and make every trajectory invalid, n_samples 0, t_hit NaN.  A trajectory of more than 2^31 - 1
 *   samples is invalid, t_hit NaN, n_samples -1; none of its samples is looked at.
 *   accumulate != 0: valid, and t_hit when given, hold on entry what nbk_spline_validity_batch wrote for the same arguments.  An
 *   entry that is 0 on entry stays 0; with t_hit given only its samples with t_j < t_hit[s] are looked at and t_hit ends as the
 *   smaller of the two, without t_hit none of its samples is looked at.  The scene's call followed by this one is then, bit for
 *   bit, nbk_spline_validity_batch on the descriptor that holds scene and points together.  accumulate == 0 overwrites.
 *   workspace: caller-owned device memory of at least nbk_spline_cloud_workspace_bytes(S) bytes (no GPU needed; < 0 for S < 0 and for S >= 2^26),
 *   64-byte aligned: the plan, the counts, the offsets and one first-hit word per trajectory, 40 bytes per trajectory whatever the
 *   sample count.  The descriptor's per-stream scratch is not touched.
 * Asynchronous, no allocation, no host synchronisation, capturable for every descriptor (LDS holds the q rows only): five kernels on
 * `stream` -- plan, the starting first-hit words (trajectories without samples to look at, or with too many, leave the flat range), scan, then one sample per lane, flat across the trajectories, on a grid of fixed
 * size (8 workgroups of 64 lanes per compute unit) that strides to the sample total, which the host never learns; a hit lowers its
 * trajectory's first-hit sample index with one 64-bit atomic minimum, and a lane whose index lies above it skips its sample; a last
 * kernel decodes valid / t_hit / n_samples.
 * NBK_ERR_INVALID -- before any device is looked for -- for null m / c, S < 0, null ctrl / knots / valid / workspace with S > 0, a
 * degree outside 1 .. NBK_MAX_SPLINE_DEGREE, n_ctrl <= degree or > 65536, a resolution that is not positive and finite, a NaN
 * threshold, a workspace that is too small or misaligned.  S = 0 returns NBK_OK at once.  NBK_ERR_UNSUPPORTED for S >= 2^26 and for a
 * selection on a descriptor of more than 256 robot shapes.  The descriptor's and the cloud's device must be current.
 */
int64_t nbk_spline_cloud_workspace_bytes(int64_t S);
int32_t nbk_spline_cloud_validity_batch(const nbk_model *m, const nbk_cloud *c, const double *ctrl, int64_t S, int32_t n_ctrl,
                                        int32_t degree, const double *knots /* DEVICE, n_ctrl + degree + 1 */, double resolution,
                                        double threshold, const uint64_t *shape_bits /* host, optional */, int32_t accumulate,
                                        uint8_t *valid, double *t_hit /* optional */, int32_t *n_samples /* optional */,
                                        void *workspace, int64_t workspace_bytes, void *stream);

/*
 * Certified continuous B-spline trajectories against a cloud: nbk_spline_continuous_batch's trajectories (the degenerate rule, the
 * knot check on the device, the keys in t_free while the call runs) and its loop, unchanged, on one (trajectory, selected robot
 * shape s) item per lane; the cloud ALONE is looked at.  shape_bits as nbk_cloud_validity_batch.
 *   Entering span ell gives mu = mu[ell][s] (nbk_spline_shape_motion_bounds_host), which bounds how fast any point of shape s moves
 *   on that span; mu_max[s] is the largest of them over the trajectory's non-empty spans.
 *   The item's distance at t: q(t) by de Boor (nbk_spline_validity_batch step 4); a non-finite q(t) gives NaN (UNDECIDED at t); else
 *   with  D_end = (threshold + slack) + mu_max * (1 - t),  D_cap = (threshold + slack) + look_ahead,  D = D_end < D_cap ? D_end : D_cap:
 *     some point i has signed distance (shape s, sphere of the cloud's radius at p_i) < D: d = the smallest one (the bits of
 *     nbk_cloud_clearance_batch for shape s alone with d_max = D);  else D == D_end: d = +inf (the item stops FREE at 1);  else d = D_cap.
 *   Sound: the loop carries an infinite gap across ALL remaining spans without another evaluation, so +inf may only be reported when
 *   no point can be reached on the whole remainder [t, 1].  Each span's mu bounds the speed of the shape's points on that span, so
 *   mu_max * (1 - t) bounds their travel from t to 1 and no point within D_end at t means the distance stays above threshold + slack
 *   up to 1.  (The current span's mu in D_end would NOT be sound: a later span may be faster.)  A distance >= D_cap replaced by D_cap
 *   is a lower bound, hence conservative, and is spent span by span with each span's own mu.
 *   accumulate == 0: an empty cloud or an empty selection reports every non-degenerate trajectory FREE at 1.
 *   accumulate != 0: valid / t_free / status hold on entry what nbk_spline_continuous_batch wrote for the same trajectories; the
 *   result is bit for bit that of ONE conservative-advancement call over the scene's pairs and the cloud's items together.  A
 *   non-degenerate trajectory that comes in with a NaN t_free keeps 0 / UNDECIDED / NaN.  Degenerate ones are DEGENERATE either way.
 *   While the cloud's status is set every non-degenerate trajectory is invalid, UNDECIDED, t_free NaN.
 * With n_ctrl = 2, k = 1, tau = [0, 0, 1, 1] this is nbk_edge_cloud_continuous_batch in connect mode with dist = NULL, bit for bit.
 * Asynchronous, no allocation, no host synchronisation, no workspace, capturable for every descriptor: three kernels on `stream`,
 * the middle one on a grid of (ceil(S / 64), selected shapes).  NBK_ERR_INVALID -- before any device is looked for -- for null m / c,
 * S < 0, null ctrl / knots / valid / t_free / status with S > 0, a degree outside 1 .. NBK_MAX_SPLINE_DEGREE, n_ctrl <= degree or
 * > 65536, max_iter < 1, slack < 0, a NaN slack / threshold, and look_ahead NaN or <= 0.  S = 0 returns NBK_OK at once.
 * NBK_ERR_UNSUPPORTED for S > 2^31 - 1, a selection on more than 256 robot shapes, more than 65535 selected shapes.
 */
int32_t nbk_spline_cloud_continuous_batch(const nbk_model *m, const nbk_cloud *c, const double *ctrl, int64_t S, int32_t n_ctrl,
                                          int32_t degree, const double *knots /* DEVICE, n_ctrl + degree + 1 */, double threshold,
                                          int32_t max_iter, double slack, double look_ahead,
                                          const uint64_t *shape_bits /* host, optional */, int32_t accumulate, uint8_t *valid,
                                          double *t_free, int32_t *status, void *stream);
/*
 * The motion bounds mu [S][n_ctrl - degree][R] (span ell at index ell - degree, R robot shapes in the caller's order) that
 * nbk_spline_cloud_continuous_batch advances with, on the host by the same routine (no GPU needed): the formula of
 * nbk_spline_motion_bounds_host for a pair of (shape s, a world shape) -- every joint on the shape's path counts.  ctrl, knots (host);
 * the knots must pass the rules of nbk_spline_validity_batch (NBK_ERR_INVALID otherwise).  Entries of empty spans are 0.
 */
int32_t nbk_spline_shape_motion_bounds_host(const nbk_model_desc *desc, const double *ctrl /* host */, int64_t S, int32_t n_ctrl,
                                            int32_t degree, const double *knots /* host */, double *mu /* [S][n_ctrl-degree][R] */);

/*
 * Held objects (additive; the reference fixes a body to a link with World.add_constraint, a Bullet dynamics constraint: here it is a
 * kinematic attachment for collision checks).  A held object is H shapes (1 .. 8; sphere, capsule, box, cylinder, and -- made by
 * nbk_held_create_hulls -- convex hull) riding on one link of the descriptor it was made against.  The world pose of held shape h at configuration q is
 *     F(q) . ((A . G) . L_h)
 * F(q) the moving frame `frame` of the descriptor (-1: the base), A [12] the link's constant pose in that frame, G the grasp (the
 * object's pose in the link frame), L_h = shape_local[h] [12] the shape in the object's frame; all 3x4 row-major.  The two constant
 * products are formed per lane on the device, each entry as xf_mul has it:
 *     R[i][j] = fma(a[i][2], b[2][j], fma(a[i][1], b[1][j], a[i][0] * b[0][j]))
 *     t[i]    = fma(a[i][2], tb[2], fma(a[i][1], tb[1], fma(a[i][0], tb[0], ta[i])))
 * whether G is the stored one or comes with the call.  nbk_held_locals_host (no GPU needed) runs that routine on HOST arrays:
 * out[h] = (A . G) . L[h].  shape_param[h] [4] and shape_type[h] are a robot shape's (nbk_model_desc.rshape_param / rshape_type).
 *
 * The entry points below give the held object's verdict ALONE -- the descriptor's own pairs play no part, and the object's copy among
 * the world shapes, where the caller registered one, is still what nbk_validity_batch sees (the caller parks or unpairs it):
 *   held shape h x world shape w for every w of world_shapes (ascending indices of the descriptor's world shapes);
 *   robot shape s x held shape h for every s of robot_bits (HOST, ceil(S / 64) words in the numbering of nbk_model_create; NULL = none;
 *   a set needs S <= 256);
 * each pair by the predicate of nbk_validity_batch -- bit for bit what a descriptor reports that holds the held shapes as robot
 * shapes S .. S+H-1 of `frame` with local pose out[h] and the pairs (s, S+h) and (S+h, (S+H)+w).
 *
 * nbk_held_create: one allocation and one copy; no later call allocates.  NBK_ERR_INVALID for a null pointer, H < 1, a frame outside
 * -1 .. n_joints-1, a non-finite pose or parameter, an unknown shape type, world indices out of range or not ascending;
 * NBK_ERR_UNSUPPORTED for H > 8, an NBK_HULL shape (nbk_held_create_hulls takes those), or robot_bits on a descriptor of more than
 * 256 robot shapes.  The descriptor must outlive the held object, and must be the `m` of every call with it (NBK_ERR_INVALID
 * otherwise, as for a device that is not current).
 *
 * nbk_held_create_hulls: nbk_held_create with the hull tables of the held object behind its arguments -- n_hulls, hull_vert_begin,
 * hull_verts, hull_face_begin, hull_planes in the layout and with the rules of nbk_model_desc's hull fields (a hull may have no
 * planes).  A shape of type NBK_HULL names its hull in shape_param[h][0] and its margin in shape_param[h][3], as a robot shape does.
 * The tables get the checks nbk_model_create gives a descriptor's (unit normals, planes that bound the vertex set, finite values):
 * NBK_ERR_INVALID, as for a hull index outside 0 .. n_hulls-1, before any device is touched.  Still one allocation and one copy: the
 * hulls travel in the held object's own blob.  Every entry of this section serves such an object, each result bit for bit what the
 * descriptor above reports with the held hulls appended to its hull tables; the held-versus-cloud entries below answer
 * NBK_ERR_UNSUPPORTED for it unless nbk_held_set_cloud_hulls has opted it in.  nbk_edge_held_motion_bounds_hulls_host / nbk_spline_held_motion_bounds_hulls_host are the host twins
 * of the motion bound with the same tables behind the held arguments; the twins without them answer NBK_ERR_UNSUPPORTED for a hull.
 *
 * nbk_held_validity_batch: q (device) [B][n_q].  grasp (device) [grasp_rows][16], each row a 4x4 row-major pose whose first three rows
 * are read when the kernel runs (a replayed graph follows a grasp rewritten in place); grasp_rows = 0 (grasp NULL: the stored G), 1
 * (one grasp for every row) or B (row b's own: screening grasp candidates).  Bit b = 1 iff some pair above is closer than
 * `threshold`, or row b of q or its grasp row is not finite, or the world status of a movable descriptor is set.  mask_bits /
 * mask_bytes as nbk_cloud_validity_batch; accumulate != 0 ORs into them: nbk_validity_batch, then this call on the same mask, is
 * validity with the object in the hand.  One kernel, one row per lane; asynchronous, no allocation, capturable; LDS holds the q rows only.
 *
 * nbk_edge_held_validity_batch: nbk_edge_cloud_validity_batch with the held object's verdict per sample: the same edge rule, end,
 * n_samples, accumulate (valid is only ever lowered; an entry that is 0 costs nothing) and workspace
 * (nbk_edge_held_workspace_bytes(E), 40 bytes per edge, 64-byte aligned).  grasp (device, optional) [16]: ONE grasp for the call,
 * NULL = the stored G; a non-finite grasp or a set world status makes every non-degenerate edge invalid.  Four kernels on `stream`.
 * Argument errors as nbk_edge_cloud_validity_batch.
 *
 * Held ITEMS.  The distance and certified entries work on K items (held shape h, other shape), in the order of that descriptor's pair
 * list: first (s, S+h) for the robot shapes s of robot_bits ascending, then h; then (S+h, world w) for h, then world_shapes ascending.
 * nbk_held_item_count gives K; nbk_held_items writes K x (held shape, kind: 0 robot / 1 world, index: s in the numbering of
 * nbk_model_create, or w) to HOST memory.
 *
 * nbk_held_distances_batch: out_d (device) [B][K], the signed distance of every item at every row -- bit for bit what
 * nbk_pair_distances_batch reports for that pair on that descriptor; NaN where row b of q or its grasp row is not finite, or the
 * world status of a movable descriptor is set.  grasp / grasp_rows as nbk_held_validity_batch.  Planes and hull-shaped WORLD shapes
 * are served.  One kernel, one (row, item) per lane, item-major; asynchronous, no allocation, capturable.
 *
 * nbk_held_records_batch / nbk_held_records_items: the items' records -- the distance with WHERE the contact is and WHICH WAY to
 * move, bit for bit what nbk_proximity_jacobian_batch / nbk_pair_records_items report for that pair on that descriptor.  A robot
 * item is its pair (s, S+h): the subject is the link shape, the target the held shape; a world item is (S+h, w): the subject is the
 * held shape.  witness [9] = point on the subject, point on the target, unit normal from the target to the subject; jrows [n_q] =
 * n . Jv_subject(p_subject) - n . Jv_target(p_target), the gradient of the distance, over the joints of the link shape's path and of
 * the holding frame's (a world target adds nothing).  witness and jrows are optional (NULL).
 *   nbk_held_records_batch: dist [B][K], witness [B][K][9], jrows [B][K][n_q] (all device); dist is nbk_held_distances_batch's.
 *   nbk_held_records_items: items (device) [N][2] int32 = (row of q, item index), as nbk_pair_records_items has them; dist [N],
 *     witness [N][9], jrows [N][n_q].  An entry outside [0, B) x [0, K) reads nothing and gets NaN in every field.  A listed item
 *     takes the grasp row of its own b.
 * grasp / grasp_rows as nbk_held_distances_batch.  Every field of an item is NaN where row b of q or its grasp row is not finite,
 * or the world status of a movable descriptor is set.  NBK_ERR_INVALID for a null m, held, q, items or dist that is needed, B < 0,
 * N < 0, grasp_rows outside {0, 1, B} or a grasp pointer that does not go with it -- answered before any device is touched.  Each is
 * one kernel on `stream`, one item per lane; asynchronous, no allocation, capturable.  LDS: the q rows, and [n_joints][6][64] doubles
 * when jrows is given.
 *
 * nbk_edge_held_continuous_batch / nbk_spline_held_continuous_batch: nbk_edge_continuous_batch / nbk_spline_continuous_batch over
 * the K items instead of the descriptor's pairs: the same conservative advancement, each item's motion bound the one
 * nbk_edge_motion_bounds_host / nbk_spline_motion_bounds_host gives for that pair on that descriptor
 * (nbk_edge_held_motion_bounds_host / nbk_spline_held_motion_bounds_host run the device's routine on the host, no GPU needed:
 * mu [E][K] / [S][n_ctrl-degree][K]; the held arguments are nbk_held_create's, against the descriptor `d`).  valid / end / t_free /
 * status as the scene's entries.  accumulate != 0: valid / t_free / status hold the result of a certified call on the same
 * trajectories (the scene's, or the cloud's after it) and the held object's is folded into it -- the smallest stop point, COLLISION
 * winning a tie; a trajectory that comes in with a NaN t_free stays 0 / NaN / UNDECIDED.  grasp (device, optional) [16]: ONE grasp
 * for the call, read when the kernels run; NULL = the stored G.  A non-finite grasp, or a set world status of a movable descriptor,
 * makes every non-degenerate trajectory 0 / NaN / UNDECIDED.  K = 0 leaves every non-degenerate trajectory FREE at its stop point.
 * No workspace (the keys live in t_free while the call runs), no allocation, capturable.
 *
 * nbk_spline_held_validity_batch: nbk_spline_cloud_validity_batch with the held object's verdict per sample: the same plan, samples,
 * first-hit rule, accumulate (valid / t_hit / n_samples as there) and workspace (nbk_spline_held_workspace_bytes(S), the layout of
 * nbk_spline_cloud_workspace_bytes).  grasp as above; a non-finite grasp or a set world status hits every trajectory that has samples
 * at its first sample.  Argument errors as nbk_spline_cloud_validity_batch.
 */
typedef struct nbk_held nbk_held;
int32_t nbk_held_locals_host(const double *A /* [12] */, const double *G /* [12] */, const double *L /* [H][12] */, int32_t H,
                             double *out /* [H][12] */);   /* no GPU */
int32_t nbk_held_create(const nbk_model *m, int32_t frame, const double *A /* host [12] */, const double *G /* host [12] */, int32_t H,
                        const int32_t *shape_type /* host [H] */, const double *shape_local /* host [H][12] */,
                        const double *shape_param /* host [H][4] */, int32_t n_world, const int32_t *world_shapes /* host */,
                        const uint64_t *robot_bits /* host, optional */, nbk_held **out);
int32_t nbk_held_create_hulls(const nbk_model *m, int32_t frame, const double *A /* host [12] */, const double *G /* host [12] */,
                              int32_t H, const int32_t *shape_type /* host [H] */, const double *shape_local /* host [H][12] */,
                              const double *shape_param /* host [H][4] */, int32_t n_world, const int32_t *world_shapes /* host */,
                              const uint64_t *robot_bits /* host, optional */, int32_t n_hulls,
                              const int32_t *hull_vert_begin /* host [n_hulls+1] */, const double *hull_verts /* host [NV][3] */,
                              const int32_t *hull_face_begin /* host [n_hulls+1] */, const double *hull_planes /* host [NF][4] */,
                              nbk_held **out);
void nbk_held_destroy(nbk_held *h);
int32_t nbk_held_validity_batch(const nbk_model *m, const nbk_held *held, const double *q, int64_t B,
                                const double *grasp /* DEVICE [grasp_rows][16] or NULL */, int64_t grasp_rows, double threshold,
                                int32_t accumulate, uint64_t *mask_bits, uint8_t *mask_bytes, void *stream);
int64_t nbk_edge_held_workspace_bytes(int64_t E);
int32_t nbk_edge_held_validity_batch(const nbk_model *m, const nbk_held *held, const double *starts, const double *goals,
                                     const double *dist /* optional */, int64_t E, double resolution, double max_distance,
                                     int32_t mode, double threshold, const double *grasp /* DEVICE [16] or NULL */,
                                     int32_t accumulate, uint8_t *valid, double *end /* optional */,
                                     int32_t *n_samples /* optional */, void *workspace, int64_t workspace_bytes, void *stream);
int32_t nbk_held_item_count(const nbk_held *held);
int32_t nbk_held_items(const nbk_held *held, int32_t *out /* host [K][3] */);
int32_t nbk_held_distances_batch(const nbk_model *m, const nbk_held *held, const double *q, int64_t B,
                                 const double *grasp /* DEVICE [grasp_rows][16] or NULL */, int64_t grasp_rows,
                                 double *out_d /* [B][K] */, void *stream);
int32_t nbk_held_records_batch(const nbk_model *m, const nbk_held *held, const double *q, int64_t B,
                               const double *grasp /* DEVICE [grasp_rows][16] or NULL */, int64_t grasp_rows,
                               double *dist /* [B][K] */, double *witness /* optional [B][K][9] */,
                               double *jrows /* optional [B][K][n_q] */, void *stream);
int32_t nbk_held_records_items(const nbk_model *m, const nbk_held *held, const double *q, int64_t B,
                               const int32_t *items /* DEVICE [N][2] */, int64_t N,
                               const double *grasp /* DEVICE [grasp_rows][16] or NULL */, int64_t grasp_rows,
                               double *dist /* [N] */, double *witness /* optional [N][9] */, double *jrows /* optional [N][n_q] */,
                               void *stream);
int32_t nbk_edge_held_continuous_batch(const nbk_model *m, const nbk_held *held, const double *starts, const double *goals,
                                       const double *dist /* optional */, int64_t E, double max_distance, int32_t mode,
                                       double threshold, int32_t max_iter, double slack, const double *grasp /* DEVICE [16] or NULL */,
                                       int32_t accumulate, uint8_t *valid, double *end /* optional */, double *t_free, int32_t *status,
                                       void *stream);
int32_t nbk_spline_held_continuous_batch(const nbk_model *m, const nbk_held *held, const double *ctrl, int64_t S, int32_t n_ctrl,
                                         int32_t degree, const double *knots /* DEVICE */, double threshold, int32_t max_iter,
                                         double slack, const double *grasp /* DEVICE [16] or NULL */, int32_t accumulate,
                                         uint8_t *valid, double *t_free, int32_t *status, void *stream);
int64_t nbk_spline_held_workspace_bytes(int64_t S);
int32_t nbk_spline_held_validity_batch(const nbk_model *m, const nbk_held *held, const double *ctrl, int64_t S, int32_t n_ctrl,
                                       int32_t degree, const double *knots /* DEVICE */, double resolution, double threshold,
                                       const double *grasp /* DEVICE [16] or NULL */, int32_t accumulate, uint8_t *valid,
                                       double *t_hit /* optional */, int32_t *n_samples /* optional */, void *workspace,
                                       int64_t workspace_bytes, void *stream);
int32_t nbk_edge_held_motion_bounds_host(const nbk_model_desc *d, int32_t frame, const double *A, const double *G, int32_t H,
                                         const int32_t *shape_type, const double *shape_local, const double *shape_param,
                                         int32_t n_world, const int32_t *world_shapes, const uint64_t *robot_bits /* optional */,
                                         const double *starts, const double *goals, int64_t E, double *mu /* [E][K] */);   /* no GPU */
int32_t nbk_spline_held_motion_bounds_host(const nbk_model_desc *d, int32_t frame, const double *A, const double *G, int32_t H,
                                           const int32_t *shape_type, const double *shape_local, const double *shape_param,
                                           int32_t n_world, const int32_t *world_shapes, const uint64_t *robot_bits /* optional */,
                                           const double *ctrl, int64_t S, int32_t n_ctrl, int32_t degree,
                                           const double *knots /* host */, double *mu /* [S][n_ctrl-degree][K] */);   /* no GPU */
int32_t nbk_edge_held_motion_bounds_hulls_host(const nbk_model_desc *d, int32_t frame, const double *A, const double *G, int32_t H,
                                               const int32_t *shape_type, const double *shape_local, const double *shape_param,
                                               int32_t n_world, const int32_t *world_shapes, const uint64_t *robot_bits /* optional */,
                                               int32_t n_hulls, const int32_t *hull_vert_begin, const double *hull_verts,
                                               const int32_t *hull_face_begin, const double *hull_planes, const double *starts,
                                               const double *goals, int64_t E, double *mu /* [E][K] */);   /* no GPU */
int32_t nbk_spline_held_motion_bounds_hulls_host(const nbk_model_desc *d, int32_t frame, const double *A, const double *G, int32_t H,
                                                 const int32_t *shape_type, const double *shape_local, const double *shape_param,
                                                 int32_t n_world, const int32_t *world_shapes, const uint64_t *robot_bits /* optional */,
                                                 int32_t n_hulls, const int32_t *hull_vert_begin, const double *hull_verts,
                                                 const int32_t *hull_face_begin, const double *hull_planes, const double *ctrl, int64_t S,
                                                 int32_t n_ctrl, int32_t degree, const double *knots /* host */,
                                                 double *mu /* [S][n_ctrl-degree][K] */);   /* no GPU */

/*
 * The held object against a point cloud: the held shapes in the robot shapes' place of the cloud's entries.  The verdict of held
 * shape h (world pose F(q) . ((A . G) . L_h), as above) against a cloud of N points of radius r is the OR over (h, i) of the pair
 * predicate for (robot shape, sphere world shape of radius r at p_i), in the operand order of nbk_cloud_validity_batch:
 *     tc = (threshold + margin_h) + r;  rs = (tc + rho_h) + 0;  free unless rs > 0 and |c_h - p_i|^2 < rs^2;  then the exact test,
 *     the point first
 * -- bit for bit what a descriptor reports that holds the held shapes as robot shapes S+h of `frame`, the N points as sphere world
 * shapes and the pairs (S+h, p_i).  This is the held-versus-cloud term ALONE: full validity is scene | arm-versus-cloud |
 * held-versus-scene | held-versus-cloud, each entry accumulating into the same result.  No world shape and no link takes part: the
 * world status of a movable descriptor is not read, and world_shapes / robot_bits of nbk_held_create play no part.  A row of q or a
 * grasp row that is not finite collides; a cloud whose status is set makes every row collide; an empty cloud is free.
 *
 * nbk_held_cloud_validity_batch: q, grasp / grasp_rows (0, 1 or B), mask_bits / mask_bytes and accumulate as
 * nbk_held_validity_batch.  One kernel, one row per lane, the grid walk of nbk_cloud_validity_batch per held shape.
 *
 * nbk_held_cloud_clearance_batch: nbk_cloud_clearance_batch over the held shapes: min_dist [B] the smallest signed distance below
 * d_max, shape [B] (optional) the HELD shape index h, point [B] (optional) the point's index in the last update; +inf, -1, -1 when
 * nothing is nearer than d_max; NaN, -1, -1 for a non-finite q or grasp row or a set status.  On equal distances the smallest h wins,
 * then the smallest point index.  d_max must be finite.
 *
 * nbk_held_cloud_records_batch: nbk_records_cloud_batch over the held shapes -- that clearance's record with the witness and the
 * gradient row.  per_shape == 0: dist [B], shape [B], point [B], witness [B][9], jrows [B][n_q]; dist, shape and point are
 * nbk_held_cloud_clearance_batch's bits.  per_shape != 0: one record per (row, held shape h), [B][H] ..., each the clearance of
 * shape h alone.  shape, point, witness and jrows are optional.  witness = point on the held shape, point on the cloud point's
 * sphere, unit normal from the point to the shape; jrows = n . Jv_held(point on the shape) over the joints of the holding frame's
 * path.  Nothing nearer than d_max: +inf, -1, -1, a NaN witness and a row of +0.0; a non-finite q or grasp row or a set status: NaN,
 * -1, -1, NaN, NaN.  One kernel; LDS: the q rows, and [n_joints][6][64] doubles when jrows is given.
 *
 * nbk_edge_held_cloud_validity_batch / nbk_spline_held_cloud_validity_batch: nbk_edge_cloud_validity_batch /
 * nbk_spline_cloud_validity_batch with this verdict per sample: the same plan, samples, end / t_hit / n_samples, accumulate and
 * workspace (nbk_edge_held_cloud_workspace_bytes(E) / nbk_spline_held_cloud_workspace_bytes(S): the cloud siblings' layouts, no
 * GPU).  grasp (device, optional) [16]: ONE grasp for the call, NULL = the stored G.  A non-finite grasp or a set cloud status makes
 * every non-degenerate edge invalid, and hits every trajectory that has samples at its first sample.
 *
 * Argument rules are those of the held and cloud siblings, answered before any device is touched: NBK_ERR_INVALID for a null pointer,
 * grasp_rows outside {0, 1, B}, a grasp pointer that does not go with grasp_rows, a NaN threshold, a non-finite d_max, a workspace
 * too small or not 64-byte aligned, and a held object made against another descriptor.  Then the held object, the cloud and the
 * descriptor must be on the current device.  All calls are asynchronous, allocate nothing, and are capturable; LDS holds the q rows only.
 *
 * A held object with an NBK_HULL shape (nbk_held_create_hulls) is served against a cloud only after it has opted in:
 * nbk_held_set_cloud_hulls(held, on) sets (on != 0) or clears a host-side flag on the object -- no device work, no kernel reads it;
 * the creators clear it; NBK_ERR_INVALID for a null held; an object without hulls takes the call and nothing changes for it.  Without
 * the flag the entries of this section and the certified ones below answer NBK_ERR_UNSUPPORTED for such an object once their own
 * argument rules are through, before any device is touched and without writing anything.  With it all seven serve the object, each
 * result bit for bit that of the descriptor above with the held hulls appended to its hull tables: the three verdict entries run a
 * second instance of their kernels (chosen by whether the object holds a hull; the instance of an object without one is unchanged)
 * in which a hull is decided by the cloud's own predicate -- a hull at tc = (threshold + margin_h) + radius <= 0 goes straight to
 * the distance iteration, so the hull-box cull's deviation at tc <= 0 does not apply -- and the four distance entries give a hull the
 * treatment a hull link shape gets.  The two *_held_shape_motion_bounds_host twins take no hull tables and answer
 * NBK_ERR_UNSUPPORTED for a hull shape; nbk_edge_held_shape_motion_bounds_hulls_host / nbk_spline_held_shape_motion_bounds_hulls_host
 * take the tables of nbk_held_create_hulls behind the held arguments (checked by nbk_model_desc's hull rules: NBK_ERR_INVALID) and
 * are otherwise the same routine.
 */
int32_t nbk_held_set_cloud_hulls(nbk_held *held, int32_t on);
int32_t nbk_held_cloud_validity_batch(const nbk_model *m, const nbk_held *held, const nbk_cloud *cloud, const double *q, int64_t B,
                                      const double *grasp /* DEVICE [grasp_rows][16] or NULL */, int64_t grasp_rows, double threshold,
                                      int32_t accumulate, uint64_t *mask_bits, uint8_t *mask_bytes, void *stream);
int32_t nbk_held_cloud_clearance_batch(const nbk_model *m, const nbk_held *held, const nbk_cloud *cloud, const double *q, int64_t B,
                                       const double *grasp /* DEVICE [grasp_rows][16] or NULL */, int64_t grasp_rows, double d_max,
                                       double *min_dist, int32_t *shape /* optional */, int32_t *point /* optional */, void *stream);
int32_t nbk_held_cloud_records_batch(const nbk_model *m, const nbk_held *held, const nbk_cloud *cloud, const double *q, int64_t B,
                                     const double *grasp /* DEVICE [grasp_rows][16] or NULL */, int64_t grasp_rows, double d_max,
                                     int32_t per_shape, double *dist, int32_t *shape /* optional */, int32_t *point /* optional */,
                                     double *witness /* optional */, double *jrows /* optional */, void *stream);
int64_t nbk_edge_held_cloud_workspace_bytes(int64_t E);
int32_t nbk_edge_held_cloud_validity_batch(const nbk_model *m, const nbk_held *held, const nbk_cloud *cloud, const double *starts,
                                           const double *goals, const double *dist /* optional */, int64_t E, double resolution,
                                           double max_distance, int32_t mode, double threshold,
                                           const double *grasp /* DEVICE [16] or NULL */, int32_t accumulate, uint8_t *valid,
                                           double *end /* optional */, int32_t *n_samples /* optional */, void *workspace,
                                           int64_t workspace_bytes, void *stream);
int64_t nbk_spline_held_cloud_workspace_bytes(int64_t S);
int32_t nbk_spline_held_cloud_validity_batch(const nbk_model *m, const nbk_held *held, const nbk_cloud *cloud, const double *ctrl,
                                             int64_t S, int32_t n_ctrl, int32_t degree, const double *knots /* DEVICE */,
                                             double resolution, double threshold, const double *grasp /* DEVICE [16] or NULL */,
                                             int32_t accumulate, uint8_t *valid, double *t_hit /* optional */,
                                             int32_t *n_samples /* optional */, void *workspace, int64_t workspace_bytes, void *stream);

/*
 * Certified continuous checks of the held object against a point cloud: nbk_edge_cloud_continuous_batch /
 * nbk_spline_cloud_continuous_batch with the held shapes in the robot shapes' place.  One (trajectory, held shape h) item per lane,
 * grid (ceil(E / 64), H): a wave holds one held shape.  The item's motion bound is mu_h, the bound of held shape h over EVERY joint
 * of the holding path (the cloud stands still; nbk_edge_held_shape_motion_bounds_host / nbk_spline_held_shape_motion_bounds_host
 * run the device's routine on the host with the stored G, no GPU needed: mu [E][H] / [S][n_ctrl-degree][H], 0 on empty spans; the
 * held arguments are nbk_held_create's without the world list and the robot set).  Its distance at t is the clearance of held shape
 * h alone against the cloud at q(t), cut at  D = min(D_end, D_cap),  D_end = (threshold + slack) + mu_h (T_f - t)  (a spline:
 * mu_max (1 - t), mu_max the largest bound over the trajectory's non-empty spans),  D_cap = (threshold + slack) + look_ahead:  the
 * smallest distance below D where there is one; else +inf when D == D_end -- the item stops FREE at its stop point -- else D_cap, a
 * lower bound the advance may use.  The result is bit for bit that of nbk_edge_cloud_continuous_batch /
 * nbk_spline_cloud_continuous_batch on a descriptor that holds the held shapes as robot shapes S+h of `frame`, selected on exactly
 * those shapes.
 *
 * This is the held-versus-cloud term ALONE, as for the four sampled entries above: no world shape and no link takes part, the world
 * status of a movable descriptor is not read, and world_shapes / robot_bits of nbk_held_create play no part.  valid / end / t_free /
 * status, max_distance / mode / dist, max_iter / slack and look_ahead as nbk_edge_cloud_continuous_batch.  accumulate != 0: valid /
 * t_free / status hold the result of a certified call on the same trajectories (the scene's, the cloud's, the held object's) and
 * this term is folded into it -- the smallest stop point, COLLISION winning a tie; a trajectory that comes in with a NaN t_free
 * stays 0 / NaN / UNDECIDED.  grasp (device, optional) [16]: ONE grasp for the call, read when the kernels run (a captured graph is
 * re-grasped by rewriting it); NULL = the stored G.  An empty cloud leaves every non-degenerate trajectory FREE at its stop point; a
 * set cloud status, or a grasp that is not finite, makes every non-degenerate trajectory 0 / NaN / UNDECIDED.
 *
 * Argument rules, answered before any device is touched: NBK_ERR_INVALID for a null m / held / cloud, E < 0 (S < 0), a null starts /
 * goals / ctrl / knots / valid / t_free / status with trajectories to check, a mode outside {0, 1}, a NaN threshold, max_iter < 1,
 * slack < 0 or NaN, and look_ahead that is not > 0 (NaN included; +inf is served); E == 0 returns NBK_OK; E > 2^31 - 1 is
 * NBK_ERR_UNSUPPORTED.  Then the held object must have been made against `m`, and it, the cloud and the descriptor must be on the
 * current device.  No workspace (the keys live in t_free while the call runs), no allocation, one linear chain of kernels on the
 * caller's stream, capturable; LDS holds the q rows only.
 */
int32_t nbk_edge_held_cloud_continuous_batch(const nbk_model *m, const nbk_held *held, const nbk_cloud *cloud, const double *starts,
                                             const double *goals, const double *dist /* optional */, int64_t E, double max_distance,
                                             int32_t mode, double threshold, int32_t max_iter, double slack, double look_ahead,
                                             const double *grasp /* DEVICE [16] or NULL */, int32_t accumulate, uint8_t *valid,
                                             double *end /* optional */, double *t_free, int32_t *status, void *stream);
int32_t nbk_spline_held_cloud_continuous_batch(const nbk_model *m, const nbk_held *held, const nbk_cloud *cloud, const double *ctrl,
                                               int64_t S, int32_t n_ctrl, int32_t degree, const double *knots /* DEVICE */,
                                               double threshold, int32_t max_iter, double slack, double look_ahead,
                                               const double *grasp /* DEVICE [16] or NULL */, int32_t accumulate, uint8_t *valid,
                                               double *t_free, int32_t *status, void *stream);
int32_t nbk_edge_held_shape_motion_bounds_host(const nbk_model_desc *d, int32_t frame, const double *A, const double *G, int32_t H,
                                               const int32_t *shape_type, const double *shape_local, const double *shape_param,
                                               const double *starts, const double *goals, int64_t E, double *mu /* [E][H] */);   /* no GPU */
int32_t nbk_spline_held_shape_motion_bounds_host(const nbk_model_desc *d, int32_t frame, const double *A, const double *G, int32_t H,
                                                 const int32_t *shape_type, const double *shape_local, const double *shape_param,
                                                 const double *ctrl, int64_t S, int32_t n_ctrl, int32_t degree,
                                                 const double *knots /* host */, double *mu /* [S][n_ctrl-degree][H] */);   /* no GPU */
int32_t nbk_edge_held_shape_motion_bounds_hulls_host(const nbk_model_desc *d, int32_t frame, const double *A, const double *G, int32_t H,
                                                     const int32_t *shape_type, const double *shape_local, const double *shape_param,
                                                     int32_t n_hulls, const int32_t *hull_vert_begin, const double *hull_verts,
                                                     const int32_t *hull_face_begin, const double *hull_planes, const double *starts,
                                                     const double *goals, int64_t E, double *mu /* [E][H] */);   /* no GPU */
int32_t nbk_spline_held_shape_motion_bounds_hulls_host(const nbk_model_desc *d, int32_t frame, const double *A, const double *G, int32_t H,
                                                       const int32_t *shape_type, const double *shape_local, const double *shape_param,
                                                       int32_t n_hulls, const int32_t *hull_vert_begin, const double *hull_verts,
                                                       const int32_t *hull_face_begin, const double *hull_planes, const double *ctrl,
                                                       int64_t S, int32_t n_ctrl, int32_t degree, const double *knots /* host */,
                                                       double *mu /* [S][n_ctrl-degree][H] */);   /* no GPU */

/*
 * Exact k nearest neighbours of every point among the points inserted before it (itself included): the neighbour lists
 * an insert-then-query loop over the reference's flat L2 index yields (numbotics/math/geometry/nearest_neighbors.py:6-85,
 * numbotics/planning/sampling_based/graph.py:165-178; faiss.IndexFlatL2 is a third-party dependency: tie-breaking and
 * its float32 summation order are unpinned).  points (device) [N][dim] float32, k <= 64;
 * out_idx (device) [N][k] int32, ascending by (distance, index), -1 padded for the first rows.
 * distance = sum_c (x_c - y_c)^2 accumulated in dimension order with separate float32 roundings.
 */
int32_t nbk_knn_prefix(const float *points, int32_t n_points, int32_t dim, int32_t k, int32_t *out_idx, void *stream);

/* Arithmetic-contract self test: elementwise sincos(a), sqrt(a), a/b computed by the device routines
 * the kernels use (all arrays device, length n). */
int32_t nbk_selftest_math(const double *a, const double *b, int64_t n, double *sin_out, double *cos_out,
                          double *sqrt_out, double *div_out, void *stream);

/*
 * The reference's scalar contracts from HOST memory, latency-optimised: Arm.in_collision(q) on one configuration
 * (numbotics/robots/arm.py:603-604) and DiscreteConnector.connect / steer on one edge (connectors.py:57-100), as the
 * sequential planners call them (numbotics/planning/sampling_based/planners/prm.py:40, rrt.py:36).  Inputs and results go through pinned,
 * device-mapped memory owned by the descriptor (no staging copies), on a private stream; the call returns when the result
 * is there.  q / start / goal / end: host [n_q].  dist < 0 = Euclidean norm.  Calls on one descriptor serialise.
 */
int32_t nbk_validity_scalar_host(const nbk_model *m, const double *q, double threshold, int32_t *in_collision);
int32_t nbk_edge_validity_scalar_host(const nbk_model *m, const double *start, const double *goal, double dist,
                                      double resolution, double max_distance, int32_t mode, double threshold,
                                      int32_t *valid, double *end, int32_t *n_samples);

/* Host-buffer conveniences for callers without a device allocator (PCIe inclusive; they allocate,
 * copy, run, copy back and synchronise). */
int32_t nbk_fk_batch_host(const nbk_model *m, const double *q, int64_t B, const int32_t *path,
                          int32_t path_len, const double *local, double *T_out);
int32_t nbk_validity_batch_host(const nbk_model *m, const double *q, int64_t B, double threshold,
                                uint8_t *mask_bytes);

#ifdef __cplusplus
}
#endif
#endif
