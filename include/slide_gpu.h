/*
 * slide_gpu.h — C-ABI boundary of the MI355X-native SlideSLAM backend hot path.
 *
 * The reference (lunarlab-gatech/SLIDE_SLAM, backend/sloam) has no plugin / FFI interface for this
 * path: the seam is a set of in-process C++ class methods called from SLOAMNode
 * (backend/sloam/src/core/sloamNode.cpp).  Every entry point below names the reference method it
 * replaces (paths relative to backend/sloam/).  All types are POD, all matrices row-major, poses are
 *     pose7 = tx, ty, tz, qx, qy, qz, qw      (geometry_msgs/Pose order; the trajectory file order
 *                                              of sloamNode.cpp:318-337)
 * and always mean T_world<-sensor ("tf_sensor_to_map", include/factorgraph/graph.h:44).
 * Functions return an int status, never throw across the ABI, and every handle serialises its own
 * calls with an internal mutex (the reference leaves add_* vs solve() unsynchronised).
 *
 * There is NO CPU fallback behind this header: every compute entry point runs hand-written HIP
 * kernels on a gfx950 device and fails with SLIDE_ERR_HIP when none is usable.
 */
#ifndef SLIDE_GPU_H_
#define SLIDE_GPU_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SLIDE_OK 0
#define SLIDE_MISSING 1          /* key absent: getPose() == false semantics (graph.cpp:297-311) */
#define SLIDE_ERR_INVALID (-1)   /* bad argument / robot id outside [0, SLIDE_MAX_ROBOTS) */
#define SLIDE_ERR_NOT_SPD (-2)   /* a landmark block or the reduced pose system is not positive definite */
#define SLIDE_ERR_CAPACITY (-3)  /* a fixed on-chip capacity was exceeded (e.g. K > 16384 neighbours in the K-NN gate; the map itself is unbounded) */
#define SLIDE_ERR_HIP (-4)       /* HIP runtime error or no gfx950 device */
#define SLIDE_ERR_RUNTIME (-5)   /* the reference would throw std::runtime_error here (sloam.cpp:349,355); also: a device-side wait gave up (scheduling stall) */

#define SLIDE_MAX_ROBOTS 13      /* include/factorgraph/graph.h:11 */

#define SLIDE_CHART_CAYLEY 0     /* GTSAM 4.0.3 default Pose3 chart (cubeFactor.h:96-97) */
#define SLIDE_CHART_EXPMAP 1     /* GTSAM_POSE3_EXPMAP builds */

#define SLIDE_CLS_CYLINDER 0
#define SLIDE_CLS_CUBE 1
#define SLIDE_CLS_ELLIPSOID 2    /* ellipsoids become Point3 landmarks in the graph (graphWrapper.cpp:157-202) */

/* Parameter names/defaults mirror the rosparam reads of the reference:
 * graphWrapper.cpp:31-34,55,60,63-64 ; graph.cpp:15-17 ; graph.h:125 ; sloamNode.cpp:151-153 ;
 * {cylinder,cube,ellipsoid}MapManager.cpp K = 50 / 30 / 1000. */
typedef struct slide_params_t {
  int pose_chart;                 /* SLIDE_CHART_* */
  double relinearize_threshold;   /* 0.1 */
  double noise_floor;             /* 0.01 */
  double noise_model_prior_first_pose_vec[6]; /* 1e-6 */
  double noise_model_odom_vec[6];             /* 0.1  */
  double noise_model_cube_vec[9];             /* 0.1  */
  double noise_model_rel_meas_vec[6];         /* 0.1  */
  double cylinder_sigma;          /* 400 */
  double bearing_range_sigma;     /* 1   */
  double numdiff_delta;           /* 1e-6 (cubeFactor.cpp:43,48) */
  double cylinder_match_thresh;   /* 2.0 */
  double cuboid_match_thresh;     /* 2.0 */
  double ellipsoid_match_thresh;  /* 0.75 */
  int knn_cylinder, knn_cube, knn_ellipsoid;  /* 50, 30, 1000 */
  int number_of_robots;           /* <= SLIDE_MAX_ROBOTS */
  int device;                     /* HIP device ordinal, -1 = current */
} slide_params_t;

void slide_default_params(slide_params_t* p);
/* 0 when a gfx950 device is present and usable, SLIDE_ERR_HIP otherwise (message via slide_last_error). */
int slide_device_check(int device);
const char* slide_last_error(void);
const char* slide_version(void);

/* ------------------------------------------------------------------------------------------------
 * S1 — SemanticFactorGraph (include/factorgraph/graph.h:70-121, src/factorgraph/graph.cpp)
 * ---------------------------------------------------------------------------------------------- */
typedef struct slide_graph slide_graph_t;
typedef struct slide_backend slide_backend_t;

slide_graph_t* slide_graph_create(const slide_params_t* p);          /* SemanticFactorGraph() graph.cpp:14-22 */
void slide_graph_destroy(slide_graph_t* g);

int slide_graph_set_prior(slide_graph_t* g, int robot, const double pose7[7]);              /* setPriors graph.cpp:24-42 */
int slide_graph_add_keypose_between(slide_graph_t* g, int robot, uint64_t from_idx, uint64_t to_idx,
                                    const double rel7[7], const double est7[7]);            /* addKeyPoseAndBetween graph.cpp:44-151 */
int slide_graph_add_loop_closure(slide_graph_t* g, const double rel7[7], uint64_t from_idx, int from_robot,
                                 uint64_t to_idx, int to_robot);                            /* addLoopClosureFactor graph.cpp:233-245 */
int slide_graph_add_relative_meas(slide_graph_t* g, const double rel7[7], uint64_t from_idx, int from_robot,
                                  uint64_t to_idx, int to_robot);                           /* addRelativeMeasFactor graph.cpp:247-258 */
int slide_graph_add_point_landmark(slide_graph_t* g, uint64_t lm_idx, const double xyz[3]); /* addPointLandmarkKey graph.cpp:153-156 */
int slide_graph_add_range_bearing(slide_graph_t* g, int robot, uint64_t pose_idx, uint64_t lm_idx,
                                  const double bearing[3], double range);                   /* addRangeBearingFactor graph.cpp:158-180 */
int slide_graph_add_cube(slide_graph_t* g, int robot, uint64_t pose_idx, uint64_t cube_idx, const double pose_world7[7],
                         const double cube_world7[7], const double scale[3], int already_exists); /* addCubeFactor graph.cpp:198-231 */
int slide_graph_add_cylinder(slide_graph_t* g, int robot, uint64_t pose_idx, uint64_t cyl_idx,
                             const double pose_world7[7], const double root[3], const double ray[3], double radius,
                             int already_exists);                                           /* addCylinderFactor graph.cpp:182-196 */
/* One iSAM2-equivalent update: isam->update(fgraph, fvalues); currEstimate = calculateEstimate()  (graph.cpp:260-272). */
int slide_graph_solve(slide_graph_t* g);
/* n batch Gauss-Newton iterations over the whole graph (relinearise every variable each time): the
 * "ms per Gauss-Newton iteration" unit of BASELINE.json.  Equivalent to solve() with threshold 0. */
int slide_graph_gauss_newton(slide_graph_t* g, int iterations);

int slide_graph_get_pose(slide_graph_t* g, int robot, uint64_t idx, double out7[7]);        /* getPose graph.cpp:290-312: SLIDE_MISSING + identity */
int slide_graph_get_pose12(slide_graph_t* g, int robot, uint64_t idx, double out12[12]);    /* same, R row-major (9) + t (3) */
int slide_graph_get_all_poses(slide_graph_t* g, int robot, double* out7N, uint64_t cap, uint64_t* n_out); /* getAllPoses graphWrapper.cpp:313-338 */
/* cls = SLIDE_CLS_*: cylinder -> 7 (root, ray, radius), cube -> 15 (R, t, scale), ellipsoid/point -> 3.
 * getCylinder / getCube / getCentroidLandmark graph.cpp:274-288 (absent key: zeros + SLIDE_MISSING). */
int slide_graph_get_landmark(slide_graph_t* g, int cls, uint64_t idx, double* out);
/* getPoseCovariance graph.cpp:314-323 (isam->marginalCovariance(X(idx))): 6x6 row-major, tangent order [rot, trans], at the
 * linearisation point of the last solve (a forward substitution with six right-hand sides on the resident Cholesky factor).
 * SLIDE_MISSING for an unknown pose, SLIDE_ERR_INVALID before the first solve. */
int slide_graph_get_pose_covariance(slide_graph_t* g, int robot, uint64_t idx, double cov36[36]);
/* Marginals of the dormant active-SLAM API (SemanticFactorGraph::logEntropy / estimateClosureInfoGain, graph.h:106,113; bodies
 * commented out in graph.cpp:421-625), on the single-graph path only: SLIDE_ERR_INVALID in sharded or exact-joint mode (ghost factors,
 * shared-landmark slots, a graph joined to a slide_chol_batch), before the first solve, after slide_graph_chi2, and once a call merged
 * pending factors or variables after the last solve (e.g. slide_graph_get_tile_profile); SLIDE_MISSING for an unknown key.  Every
 * value is taken at the linearisation point of the resident factor, from its selected inverse Sigma = S^-1 on the factor's tile
 * profile (computed once per factorisation).
 * isam->marginalCovariance(X(idx[q])) (graph.cpp:314-323) for n poses: out36n[36 q ..], 6x6 row-major, tangent order [rot, trans]. */
int slide_graph_get_pose_covariances(slide_graph_t* g, int robot, const uint64_t* idx, int n, double* out36n);
/* isam->marginalCovariance(L / C / U(idx[q])) (graph.cpp:444): d x d row-major per landmark, d = 7 / 9 / 3 for cylinder / cube /
 * point (SLIDE_CLS_ELLIPSOID), tangent order of the retraction: cylinder [ray, root, radius], cube pose (6) then scale (3), point xyz. */
int slide_graph_get_landmark_covariances(slide_graph_t* g, int cls, const uint64_t* idx, int n, double* out);
/* logEntropy (graph.cpp:423-466): out4 = {sum of the marginal traces of the robot's poses, sum over the point landmarks (U(i),
 * ellipsoids included), #poses, #landmarks}. */
int slide_graph_marginal_traces(slide_graph_t* g, int robot, double out4[4]);
/* estimateClosureInfoGain (graph.cpp:469-623): the drop of those trace sums when Between factors (traj[i+1], traj[i]), i < n - 1, with
 * noise sigma_per_m * travel[i] and zero residual are added (graph.cpp:503-545); sigma_per_m = NULL: the graph's noise_model_odom_vec
 * (the reference's noise_model_pose_vec_per_m, graph.h:115, is never set).  out3 = {10 pose + landmark, pose, landmark}
 * (graph.cpp:622).  Linear-Gaussian model of the resident factor (a rank-6(n-1) update, nothing is re-factored and the graph is left
 * exactly as it was); unlike iSAM2's update it does not relinearise variables while the fake factors are in.  SLIDE_ERR_INVALID for
 * n < 2, a travel distance or sigma <= 0; SLIDE_ERR_CAPACITY for n - 1 > SLIDE_INFO_GAIN_MAX_STEPS. */
#define SLIDE_INFO_GAIN_MAX_STEPS 64
int slide_graph_closure_info_gain(slide_graph_t* g, int robot, const uint64_t* traj, int n, const double* travel, const double sigma_per_m[6],
                                  double out3[3]);
/* estimateClosureInfoGain (graph.cpp:469-623; the planner's request is srv/EvaluateLoopClosure.srv) for a LIST of candidates, ranked in
 * one call: candidate k is the trajectory traj[off[k] .. off[k+1]), travel runs parallel to traj (entry off[k] + i belongs to step i of
 * candidate k; the last entry of each candidate is not read), sigma_per_m = NULL as above.  out3n[3 k ..] is exactly what
 * slide_graph_closure_info_gain documents for candidate k alone: every candidate is evaluated by itself against the resident factor,
 * candidates do not accumulate, and a candidate's result does not depend on what else is in the list.  The list is cut into sweeps of
 * whole candidates of at most SLIDE_INFO_GAIN_SWEEP_COLS columns (six per step); a sweep is one many-column solve, per-candidate
 * block-diagonal grams and a per-candidate Woodbury step on the device.  Any n_cand >= 1.
 * Whole-call refusals are those of slide_graph_closure_info_gain (nothing is written then); n_cand < 1, off = NULL or a decreasing off:
 * SLIDE_ERR_INVALID.  Otherwise SLIDE_OK, and a candidate's own fault goes to status[k] (status may be NULL) with zeros in its outputs:
 * SLIDE_MISSING for an unknown pose, SLIDE_ERR_INVALID for fewer than two poses or a travel distance <= 0, SLIDE_ERR_CAPACITY for more
 * than SLIDE_INFO_GAIN_MAX_STEPS steps, SLIDE_ERR_NOT_SPD if its I + J Sigma J^T is not positive definite. */
#define SLIDE_INFO_GAIN_SWEEP_COLS 384
int slide_graph_closure_info_gain_batch(slide_graph_t* g, int robot, int n_cand, const int32_t* off, const uint64_t* traj,
                                        const double* travel, const double sigma_per_m[6], double* out3n, int32_t* status);
/* counts: [poses, landmarks, factors, relinearised vars in the last solve, chol dim] */
int slide_graph_stats(slide_graph_t* g, int64_t out5[5]);
/* Sum of squared whitened residuals of every factor at the current estimate (= 2 x gtsam::NonlinearFactorGraph::error of the graph
 * ISAM2 holds): out4 = {total, prior factors, Between factors, landmark factors}.  Commits delta into the linearisation point and
 * relinearises (the estimate itself does not move); pending factors are merged first.  The sum is that of the system as
 * linearised: while a robust loss is set (slide_graph_set_robust_loss, slide_graph_set_observation_loss) that is the reweighted
 * system, a selected factor entering with w(s) s^2. */
int slide_graph_chi2(slide_graph_t* g, double out4[4]);
/* ---- Robust loss on the loop-closure and relative-measurement factors: iteratively reweighted least squares ---------------------
 * No counterpart in the reference, whose closures are plain Between factors with sigmas of noise_model_odom_vec * 0.01
 * (graphWrapper.cpp:55): one false closure that passed the vetting bends the whole trajectory.  GTSAM users know this as
 * noiseModel::Robust::Create(mEstimator::{Huber, Cauchy, GemanMcClure, DCS}::Create(param), base) on exactly these factors.
 * For a selected factor with base sigmas sigma0 (what slide_graph_add_loop_closure / _add_relative_meas chose), e its residual
 * Local(measured, x1^-1 x2) and s = |e / sigma0|_2 at the linearisation point, the factor is linearised with sigma0 / sqrt(w(s))
 * (Robust::WhitenSystem), w = mEstimator::weight:
 *     kind 1 Huber          k   (default 1.345)   1 if s <= k, else k / s
 *     kind 2 Cauchy         k   (default 0.1)     k^2 / (k^2 + s^2)
 *     kind 3 Geman-McClure  c   (default 1.0)     (c^2 / (c^2 + s^2))^2
 *     kind 4 DCS            Phi (default 1.0)     1 if s^2 <= Phi, else (2 Phi / (Phi + s^2))^2
 * with w >= 1e-12.  A factor's weight is taken exactly when the factor is relinearised: an incremental slide_graph_solve that
 * keeps a factor's linearisation keeps its weight.  Odometry factors are never reweighted.
 * kind 0 switches the loss off (the default: launches and results are then what they are without this call); param <= 0 takes the
 * default; class_mask bit 0 selects the loop closures, bit 1 the relative measurements.  The setting covers the factors already
 * added and those added later, in slide_graph_gauss_newton, slide_graph_solve (incremental updates included) and so the streaming
 * back-end (slide_backend_graph).  Every call restores the base sigmas and drops the resident factor, as slide_graph_chi2 does: the
 * next solve relinearises everything.  Marginals, the information gain and the Mahalanobis gate read the resident factor and so
 * describe the reweighted system.
 * SLIDE_ERR_INVALID: kind outside 0 .. 4, a class_mask bit other than 0 and 1, a graph that has joined a batch.  Single-graph path
 * only: while a loss is set, slide_graph_join_chol_batch, slide_graph_dist_phase and slide_graph_dist_pass_local return
 * SLIDE_ERR_INVALID (the un-batched sharded passes do not carry a loss; a batch carries its own: slide_chol_batch_set_robust_loss). */
int slide_graph_set_robust_loss(slide_graph_t* g, int kind, double param, int class_mask);
/* What the graph has come to think of its closures (no counterpart in the reference; in GTSAM: mEstimator::weight of each
 * factor's whitened error): every loop-closure (kind 1) and relative-measurement (kind 2) factor in insertion order, with its keys,
 * the weight w and the squared whitened norm s^2 of its last linearisation.  w = 1 when no loss was set then or the factor's class
 * was not selected.  One read-back.  Any output pointer may be NULL; at most cap entries are written, *n_out is the full count.
 * Factors added after the last solve are not listed yet.  SLIDE_ERR_INVALID before the first solve. */
int slide_graph_get_closure_weights(slide_graph_t* g, int cap, int32_t* from_robot, uint64_t* from_idx, int32_t* to_robot, uint64_t* to_idx,
                                    int32_t* kind, double* weight, double* s2, int* n_out);
/* ---- Robust loss on the landmark observation factors: iteratively reweighted least squares -------------------------------------
 * No counterpart in the reference, which adds every match of the per-frame data association as a plain factor: a false match
 * inside the association's gate pulls its pose and its landmark with the full weight of a true one.  In GTSAM:
 * noiseModel::Robust::Create(mEstimator::...::Create(param), base) on the BearingRange / Cube / Cylinder factors.
 * For a selected factor with whitened residual r at the linearisation point (3 rows under bearing_range_sigma, a cube's 9 under its
 * own sigmas, a cylinder's 7 under cylinder_sigma), s^2 = |r|^2 and w = mEstimator::weight(s) as listed above (same kinds, default
 * parameters and floor w >= 1e-12); the factor enters the step as sqrt(w) [r | J] (Robust::WhitenSystem).  The scaling is fused
 * into the linearisation kernel: no further launch, and w = 1 leaves the factor's linearisation bit for bit.
 * kind 0 switches the loss off (the default: launches and results are then what they are without this call); param <= 0 takes the
 * default; class_mask bit 0 selects the bearing-range factors (point / ellipsoid landmarks), bit 1 the cube, bit 2 the cylinder
 * factors.  Independent of slide_graph_set_robust_loss; both may be set.  A factor's weight is taken exactly when the factor is
 * relinearised: an incremental slide_graph_solve that keeps a factor's linearisation keeps the weight inside it.  Covers the factors
 * already added and those added later, in slide_graph_gauss_newton, slide_graph_solve and so the streaming back-end.  Every call
 * (kind 0 included) drops the resident factor, as slide_graph_chi2 does: the next solve relinearises everything.  slide_graph_chi2,
 * the marginals, the information gain and the Mahalanobis gate describe the reweighted system.
 * A landmark all of whose observations are down-weighted to the floor has an H_ll of order 1e-12: there is no guard of its own for
 * it, the solve reports it as it reports any near-singular landmark block.
 * SLIDE_ERR_INVALID: kind outside 0 .. 4, a class_mask bit other than 0 .. 2, a param that is not a number, a graph that has joined
 * a batch.  Single-graph path only: while a loss is set, slide_graph_join_chol_batch, slide_graph_dist_phase and
 * slide_graph_dist_pass_local return SLIDE_ERR_INVALID (the un-batched sharded passes do not carry an observation loss; a batch carries
 * its own: slide_chol_batch_set_observation_loss). */
int slide_graph_set_observation_loss(slide_graph_t* g, int kind, double param, int class_mask);
/* What the graph has come to think of its observations: every landmark factor in insertion order with its pose (robot, pose_idx),
 * its landmark (cls: SLIDE_CLS_*, lm_idx), the weight w and the squared whitened norm s^2 (taken before the scaling) of its last
 * linearisation.  w = 1 when no loss was set then or the factor's class was not selected; s^2 is reported all the same.  One
 * read-back.  Any output pointer may be NULL; at most cap entries are written, *n_out is the full count.  Factors added after the
 * last solve are not listed yet.  SLIDE_ERR_INVALID before the first solve. */
int slide_graph_get_observation_weights(slide_graph_t* g, int cap, int32_t* robot, uint64_t* pose_idx, int32_t* cls, uint64_t* lm_idx,
                                        double* weight, double* s2, int* n_out);
/* isam->update(fgraph, fvalues) (graph.cpp:262) throws when a factor names a key that is in neither the graph nor fvalues, and when a
 * value is inserted under a key that exists already.  Here such an entry is refused, the rest of the update is merged, and the call
 * that consumed it (solve, gauss_newton, dist_phase 0 / 20, set_shared, set_ghosts, chol_batch_pass) returns SLIDE_ERR_INVALID with the
 * first offending key in slide_last_error().  This returns the number of entries refused since the graph was created (0 in a healthy run). */
int64_t slide_graph_rejected_count(slide_graph_t* g);
/* Per-kernel device timings (HIP events on the launch stream) of the solves since the last reset.
 * names: caller buffer of n_max * 32 chars; ms_total / launches: n_max entries.  Returns #entries. */
int slide_graph_set_profiling(slide_graph_t* g, int on);
int slide_graph_get_profile(slide_graph_t* g, char* names, double* ms_total, int64_t* launches, int n_max);

/* ---- one robot per GPU (the reference instead keeps a full replica of every robot's graph in
 * every sloam_node and gossips packets over ROS topics, databaseManager.cpp:219-279) -------------------------
 * Slots are a global, rank-independent enumeration of the landmarks observed by more than one robot.
 * slide_graph_set_shared: slot i is this rank's landmark (cls[i], idx[i]) or none (cls[i] < 0); owner[i] != 0 on
 * exactly one rank per slot (the rank whose value every replica adopts).
 * slide_graph_dist_phase: one distributed Gauss-Newton pass is
 *     phase 0 ; all-reduce(sum) of d_buf[54 * n_slots] ; phase 1 ; all-reduce(sum) of d_buf[9 * n_slots] ; phase 2
 * and a value broadcast is  phase 10 ; all-reduce(sum) of d_buf[15 * n_slots] ; phase 11.
 * d_buf is a DEVICE buffer owned by the caller (the collective itself — RCCL over xGMI — runs outside this
 * library); each call returns after its kernels have completed. */
int slide_graph_set_shared(slide_graph_t* g, const int32_t* cls, const int64_t* idx, const int32_t* owner, int n_slots);
int slide_graph_dist_phase(slide_graph_t* g, int phase, double* d_buf);

/* Several robot graphs on ONE GPU (the 8 / N-robots-per-GPU layout; no counterpart in the reference, whose replica solves one joint
 * graph): the dense factor + solve of phase 1 of all joined graphs runs as one launch sequence, one launch per block column for
 * all of them.  Every joined graph must then run its passes in lockstep from its own host thread (slide_graph_dist_phase(g, 1, ..)
 * returns when all have arrived; SLIDE_ERR_RUNTIME after 60 s).  slide_graph_join_chol_batch(g, NULL, 0) leaves the batch. */
/* Ownership: a batch does not own its graphs, a graph does not own its batch.  slide_graph_destroy / slide_backend_destroy leave the
 * batch first; slide_chol_batch_destroy sends every joined graph back to its own launches.  Neither may run while a pass of the batch
 * is executing on another thread. */
typedef struct slide_chol_batch slide_chol_batch_t;
slide_chol_batch_t* slide_chol_batch_create(int n_graphs);      /* 1 .. 8 */
void slide_chol_batch_destroy(slide_chol_batch_t* b);
int slide_graph_join_chol_batch(slide_graph_t* g, slide_chol_batch_t* b, int slot);
/* One distributed pass (phases 0, 1, 2 of slide_graph_dist_phase) when the batch holds every robot of the job: the two exchanges are
 * device-side sums between the joined graphs' buffers (d_buf: this graph's exchange buffer, 54 doubles per shared slot), no host
 * synchronisation inside the pass.  Called from every joined graph's thread in lockstep. */
int slide_graph_dist_pass_local(slide_graph_t* g, double* d_buf);
/* The same pass for ALL graphs of the batch from ONE host thread: every robot's phases on its own stream, forked from and joined to
 * the batch's stream around the exchanges and the batched factor + solve, captured once and replayed as one hipGraph per pass.
 * d_bufs[i] = exchange buffer (device) of the graph in slot i. */
int slide_chol_batch_pass(slide_chol_batch_t* b, double* const* d_bufs);
/* Marginal covariances on the JOINT multi-robot graph (exact joint passes, slide_chol_batch_set_exact_joint): what a sloam_node's full
 * replica of the multi-robot graph answers (graph.cpp:325-371), from the factor the last slide_chol_batch_pass left — the selected
 * inverse over its elimination tree (segments, windows, separator leaves and top block, lambda block), computed once per pass and
 * cached.  Shared landmarks and inter-robot factors shrink these, unlike the single-graph getters (which keep refusing on a joined graph).
 * SLIDE_ERR_INVALID (+ slide_last_error) before the first whole exact pass, once any joined graph changed after it (pending or merged
 * factors / variables, a re-join), in PCG or block-Jacobi mode, and on a rank that owns one separator leaf (a job spread over GPUs);
 * SLIDE_MISSING for an unknown index.  The queries run on the batch's stream outside any capture and write nothing a pass reads.
 * getPoseCovariance(idx, robotID) (graph.cpp:314-323) / getCurrPose(.., cov) (graphWrapper.cpp:277-297) for n poses of the robot whose
 * graph is in `slot`, by its pose indices: out36n[36 q ..], 6x6 row-major, tangent order [rot, trans]. */
int slide_chol_batch_get_pose_covariances(slide_chol_batch_t* b, int slot, const uint64_t* idx, int n, double* out36n);
/* isam->marginalCovariance(L / C / U(idx[q])) (graph.cpp:444) on the joint graph for n landmarks of the graph in `slot`, by that graph's
 * landmark ids: d x d row-major each, d = 7 / 9 / 3 for cylinder / cube / point; a shared landmark reads the same numbers from every slot. */
int slide_chol_batch_get_landmark_covariances(slide_chol_batch_t* b, int slot, int cls, const uint64_t* idx, int n, double* out);
/* logEntropy (graph.cpp:423-466) on the joint graph: out4 = {sum of the traces of the pose marginals of the robot in `slot`, sum over the
 * job's point landmarks (every graph's private ones, each shared one once), #poses, #point landmarks}. */
int slide_chol_batch_marginal_traces(slide_chol_batch_t* b, int slot, double out4[4]);
/* estimateClosureInfoGain (graph.cpp:469-623) on the JOINT graph — what a sloam_node's replica of the whole multi-robot graph
 * (graph.cpp:325-371) answers an active-SLAM planner: the drop of logEntropy's trace sums when Between factors (traj[i+1], traj[i]),
 * i < n - 1, with noise sigma_per_m * travel[i] and zero residual are added.  Pose q is pose traj[q] of the robot whose graph is in slot
 * traj_slots[q] (traj_slots = NULL: every pose in `slot`); different slots make an inter-robot candidate (a rendezvous).
 * sigma_per_m = NULL: the noise_model_odom_vec of the graph in `slot`.  out4 = {10 pose + landmark (graph.cpp:622), the pose drop of the
 * robot in `slot`, the drop over the job's point landmarks (as slide_chol_batch_marginal_traces), the pose drop summed over every robot}.
 * Linear-Gaussian model of the factor the last slide_chol_batch_pass left: a rank-6(n-1) Woodbury update with J at the pass's
 * linearisation point, nothing re-factored; unlike iSAM2's update it does not relinearise variables while the candidate factors are in.
 * Refusals as the joint marginals (SLIDE_ERR_INVALID before a whole exact pass, after any graph changed, in PCG / block-Jacobi mode, on
 * a rank owning one separator leaf); SLIDE_MISSING for an unknown pose; SLIDE_ERR_INVALID for n < 2 or a travel / sigma <= 0;
 * SLIDE_ERR_CAPACITY for n - 1 > SLIDE_INFO_GAIN_MAX_STEPS; SLIDE_ERR_NOT_SPD if I + J Sigma J^T is not positive definite.  Runs on
 * the batch's stream outside any capture and writes nothing a pass reads (the cached joint Sigma included). */
int slide_chol_batch_closure_info_gain(slide_chol_batch_t* b, int slot, const int32_t* traj_slots, const uint64_t* traj, int n,
                                       const double* travel, const double sigma_per_m[6], double out4[4]);
/* estimateClosureInfoGain (graph.cpp:469-623; srv/EvaluateLoopClosure.srv) on the JOINT graph for a LIST of candidates: the arguments of
 * slide_graph_closure_info_gain_batch, with traj_slots running parallel to traj (NULL: every pose in `slot`).  out4n[4 k ..] is exactly
 * what slide_chol_batch_closure_info_gain documents for candidate k alone; sweeps, per-candidate status and independence as there.
 * Whole-call refusals are those of slide_chol_batch_closure_info_gain (nothing is written then); a slot of traj_slots outside the batch
 * is that candidate's SLIDE_ERR_INVALID. */
int slide_chol_batch_closure_info_gain_batch(slide_chol_batch_t* b, int slot, int n_cand, const int32_t* off, const int32_t* traj_slots,
                                             const uint64_t* traj, const double* travel, const double sigma_per_m[6], double* out4n,
                                             int32_t* status);
/* slide_graph_get_pose_pair_covariances and slide_graph_closure_mahalanobis on the JOINT graph: the two queries those calls refuse for a
 * graph joined to a batch, with a slot (a graph of the batch; its robot is the graph's own) where they take a robot.  The two poses may
 * belong to different slots: the block between two robots is the one covariance the joint marginals above cannot give, and an
 * inter-robot closure or a rendezvous candidate the one closure the single-graph gate cannot judge.  No counterpart in the reference.
 * The pass leaves K = L D L^T with D = +I except on the lambda block of the inter-robot relative-pose factors (D = -I), so
 * B^T K^-1 B = W^T D W with L W = B: the forward half of the substitution slide_chol_batch_closure_info_gain runs, and a signed gram
 * that counts every coordinate of the joint system once.  Sigma is the inverse of the joint system the pass linearised; r_k and A_k are
 * taken at the graphs' current estimates (slide_graph_get_pose12 after the pass) under the pose_chart of the from pose's graph: the
 * linear-Gaussian model of slide_chol_batch_closure_info_gain.  Sweeps, outputs, C36 / r6 / status (each may be NULL) and a candidate's
 * independence of the rest of the list are the single-graph calls'.
 * Whole-call refusals (nothing written): the argument checks of the single-graph calls, made before the batch or the device is looked
 * at (a slot outside [0, SLIDE_MAX_ROBOTS) among them), then those of slide_chol_batch_get_pose_covariances.  Per candidate, with zeros
 * in its outputs: SLIDE_MISSING for a slot the batch does not have or a pose its graph does not hold, SLIDE_ERR_INVALID when both ends
 * are the same pose of the same slot, SLIDE_ERR_NOT_SPD when I + A Sigma A^T has a pivot that is not positive.  n == 0 / L == 0 on a
 * batch that would be served: SLIDE_OK.  Both run on the batch's stream outside any capture and write nothing a pass reads; the cached
 * joint Sigma is neither used nor touched.
 *
 * Marginals::jointMarginalCovariance on the JOINT graph: block k = [[Saa, Sab], [Sba, Sbb]], row-major 12 x 12, pose a's six
 * coordinates then pose b's, tangent order [rot, trans]. */
int slide_chol_batch_get_pose_pair_covariances(slide_chol_batch_t* b, int n, const int32_t* slot_a, const uint64_t* idx_a, const int32_t* slot_b,
                                               const uint64_t* idx_b, double* out144n, int32_t* status);
/* Closure k is the Between factor with sigmas sigma6_k from pose (from_slot, from_idx) to (to_slot, to_idx);
 * d2_k = r_k^T (I + A_k Sigma A_k^T)^-1 r_k, to be compared with 16.81; no threshold is applied. */
int slide_chol_batch_closure_mahalanobis(slide_chol_batch_t* b, int L, const int32_t* from_slot, const uint64_t* from_idx, const int32_t* to_slot,
                                         const uint64_t* to_idx, const double* rel7, const double* sigma6, double* d2, double* C36 /* may be NULL */,
                                         double* r6 /* may be NULL */, int32_t* status /* may be NULL */);
/* slide_graph_observation_mahalanobis on the JOINT graph: the individual-compatibility gate of candidate landmark observations that
 * call refuses for a graph joined to a batch.  The robots of an exact pass are coupled almost entirely through shared landmarks, so a
 * false match onto one of them lands in the separator and pulls every robot that sees it; and one kind of candidate has no
 * single-graph form at all: robot a's pose against a landmark only robot b has mapped, the would-be new shared landmark.  No
 * counterpart in the reference.
 * Candidate k names a pose (pose_slot[k], pose_idx[k]) and an existing landmark (lm_slot[k], cls[k], lm_idx[k]), lm_idx the
 * landmark's index in the graph of lm_slot; the two slots may differ, and lm_slot == NULL means the pose's slot throughout.  meas17,
 * r, A = [Ap | Al], the outputs and the sweeps are the single-graph call's: the noise the POSE's graph would choose, no robust weight,
 * the device-resident estimates (the pose of its graph, the landmark of its own), the pose retracted under its graph's pose_chart and
 * the landmark under its own graph's.  K = L D L^T is the joint system the last whole exact pass factored, and
 *     C = I + G0 + B^T K^-1 B = I + G0 + W^T D W,   L W = B,   d2[k] = r^T C^-1 r.
 * A private landmark (no shared slot in its graph) is eliminated, as on one graph: G0 = Al H_ll^-1 Al^T and
 * B = P_p^T Ap^T - sum_{f in factors(l)} P_{p_f}^T F_f Al^T in joint rows, the factors' poses being poses of the LANDMARK's graph.  A
 * shared landmark is a separator variable the pass does not eliminate: G0 = 0 and B = P_p^T Ap^T + P_l^T Al^T, P_l selecting the
 * landmark's rows of the separator system (entered once, whichever replica names it, so any robot's replica gives the same bits).  The signed gram counts every
 * coordinate once, the lambda rows of the inter-robot relative-pose factors with D = -I (slide_chol_batch_closure_mahalanobis above).
 * Every sweep walks the whole forward half of the joint substitution; a candidate's bits do not depend on the rest of the list.
 * Whole-call refusals (SLIDE_ERR_INVALID, nothing written): the argument checks of slide_graph_observation_mahalanobis in its own
 * words, made before the batch or the device is looked at (lm_slot, where given, is checked like pose_slot; the batch is NULL), then
 * those of slide_chol_batch_get_pose_covariances (no whole exact pass yet, the graphs changed since, PCG passes).  Per candidate, with
 * zeros in its outputs: SLIDE_MISSING for a slot the batch does not have, a pose or landmark its graph does not hold, or a landmark
 * with neither a factor nor a shared slot; SLIDE_ERR_NOT_SPD when C has a pivot that is not positive.  n == 0 on a batch that would be
 * served: SLIDE_OK.  Runs on the batch's stream outside any capture and writes nothing a pass reads; the cached joint Sigma is neither
 * used nor touched. */
int slide_chol_batch_observation_mahalanobis(slide_chol_batch_t* b, int n, const int32_t* pose_slot, const uint64_t* pose_idx,
                                             const int32_t* lm_slot /* may be NULL */, const int32_t* cls, const uint64_t* lm_idx,
                                             const double* meas17, double* d2, int32_t* dof /* may be NULL */, double* C81 /* may be NULL */,
                                             double* r9 /* may be NULL */, int32_t* status /* may be NULL */);
/* slide_graph_observation_joint_compatibility on the JOINT graph: the joint compatibility of a frame's landmark matches, tested
 * together on the factor of the last whole exact pass.  It mirrors that call — the groups (n_groups, group_ptr), prob (0: evaluate
 * only), the rule, every output and the status words are its own — and names its candidates as
 * slide_chol_batch_observation_mahalanobis names them: pose_slot, pose_idx, lm_slot (NULL: the pose's slot), cls, lm_idx, meas17.  A
 * set of matches from one frame onto shared landmarks, or onto landmarks only another robot has mapped, is the hypothesis that ties
 * two maps together; it comes from one pose, so its candidates are strongly correlated and the individual gate accepts sets that no
 * single pose error explains.  No counterpart in the reference.
 * K = L D L^T is the joint system of the last whole exact pass, D = -I on the lambda block of the inter-robot relative-pose factors.
 * With a group's served candidates stacked in the caller's order,
 *     C = I + A K^-1 A^T,     block (i, j) = [i == j] (I + G0_i) + W_i^T D W_j,     L W = B,
 * B_i and G0_i exactly what the individual joint gate forms for candidate i (a private landmark: G0 = Al H_ll^-1 Al^T and the factor
 * sum over the landmark's own graph's poses; a shared landmark: G0 = 0 and Al^T on its separator coordinates), the cross blocks the
 * off-diagonal part of the signed gram.  A PRIVATE landmark — its identity is (lm_slot, lm_idx) — may not be named twice in a group:
 * H_ll is block diagonal and the cross block would miss Al_i H_ll^-1 Al_j^T; the group gets SLIDE_ERR_INVALID.  A SHARED landmark may
 * be named twice, also by two robots' poses through two different replicas: it is a separator variable the pass does not eliminate,
 * everything about it is in K, and its identity is its separator offset, so two replicas are one landmark and give the same bits.
 * Groups are packed whole, in the caller's order, into sweeps of at most SLIDE_INFO_GAIN_SWEEP_COLS columns; every sweep walks the
 * whole forward half of the joint substitution; a group's bits do not depend on what else is in the call or where it stands.
 * Whole-call refusals (SLIDE_ERR_INVALID, nothing written, the message names chol_batch_observation_joint_compatibility and the
 * reason): the group and probability checks of slide_graph_observation_joint_compatibility and the candidate checks of
 * slide_graph_observation_mahalanobis (lm_slot, where given, checked like pose_slot), made before the batch or the device is looked
 * at, the batch is NULL; then those of slide_chol_batch_get_pose_covariances (no whole exact pass yet, the graphs changed since, PCG
 * passes).  Per candidate, with zeros in its outputs: SLIDE_MISSING as slide_chol_batch_observation_mahalanobis decides it — the
 * candidate is skipped and the rest of its group served as if it were absent; SLIDE_ERR_NOT_SPD when a pivot is not positive.  Per
 * group, with zeros everywhere in the group and its neighbours served: SLIDE_ERR_INVALID (a private landmark twice),
 * SLIDE_ERR_CAPACITY (more than SLIDE_INFO_GAIN_SWEEP_COLS served rows).  Runs on the batch's stream outside any capture and writes
 * nothing a pass reads; the cached joint Sigma is neither used nor touched. */
int slide_chol_batch_observation_joint_compatibility(slide_chol_batch_t* b, int n_groups, const int32_t* group_ptr, const int32_t* pose_slot,
                                                     const uint64_t* pose_idx, const int32_t* lm_slot /* may be NULL */, const int32_t* cls,
                                                     const uint64_t* lm_idx, const double* meas17, double prob, int32_t* accepted,
                                                     double* d2_single, double* d2_joint, int32_t* dof_joint, int32_t* status, double* group_d2,
                                                     int32_t* group_dof, int32_t* group_count, int32_t* group_status);
/* slide_graph_landmark_pair_mahalanobis on the JOINT graph: are two landmarks — of one robot, or of TWO — one object?  Which landmarks
 * two robots share is the separator of the exact joint pass, and a pair this test keeps across robots becomes a shared slot through
 * slide_graph_set_shared / slide_graph_set_separator; the call itself merges nothing.  No counterpart in the reference, which merges
 * the robots' maps on a Euclidean threshold.  A landmark is named as slide_chol_batch_observation_mahalanobis names one:
 * (slot_a[k], cls[k], idx_a[k]) and (slot_b[k], cls[k], idx_b[k]), idx the landmark's index in the graph of its slot; a SHARED
 * landmark may be named through any replica (it is read through its lowest one: either name gives the same bits).  Classes, the
 * hypothesis, sigma_point3 / sigma_cylinder7, r, C, d2 and the outputs' layout are the single-graph call's; cubes are refused on the
 * host as there.  K = L D L^T is the joint system of the last whole exact pass, D = -I on the lambda block, and
 *     C = I + G0 + W^T D W,     L W = B,     d2 = r^T C^-1 r,     r = (est_b - est_a) / sigma.
 * A PRIVATE landmark enters as on one graph, in joint rows: -+F_f[.][j] / sigma_j at its factors' poses in its OWN graph, and
 * H_ll^-1 / (sigma_i sigma_j) into G0.  A SHARED landmark is a separator variable the pass does not eliminate: -+I / sigma on its
 * separator coordinates (entered once, at its rows in the border of the lowest robot that holds it), nothing in G0, no factor sum.
 * Served: private-private in one graph, private-private across graphs, private-shared, shared-shared.  The landmark block between two
 * robots is the one the cached joint Sigma does not hold; every pair, also one of a single robot, takes the forward substitution
 * (there is no direct route off the cached Sigma, and no route output).  SLIDE_INFO_GAIN_SWEEP_COLS / D pairs per sweep (128 points,
 * 54 cylinders), every sweep one walk of the whole forward half; a pair's bits do not depend on the rest of the list.
 * Whole-call refusals (SLIDE_ERR_INVALID, nothing written, the message names chol_batch_landmark_pair_mahalanobis and the reason):
 * those of slide_graph_landmark_pair_mahalanobis, made before the batch or the device is looked at (slot_a and slot_b are needed
 * pointers; the batch is NULL), then those of slide_chol_batch_get_pose_covariances (no whole exact pass yet, a cut or profiled pass
 * since, the graphs changed since, PCG passes, a job spread over processes).  Per pair, into status[k] with zeros in its outputs:
 * SLIDE_MISSING for a slot the batch does not have, a landmark its graph does not hold, or a landmark with neither a factor nor a
 * shared slot; SLIDE_ERR_INVALID for two names of one variable — one private landmark twice, or two replicas of one shared slot
 * (told by their separator offset); SLIDE_ERR_NOT_SPD when a pivot of C is not positive.  n == 0 on a batch that would be served:
 * SLIDE_OK.  Runs on the batch's stream outside any capture and writes nothing a pass reads; the cached joint Sigma is neither used
 * nor touched. */
int slide_chol_batch_landmark_pair_mahalanobis(slide_chol_batch_t* b, int n, const int32_t* cls, const int32_t* slot_a, const uint64_t* idx_a,
                                               const int32_t* slot_b, const uint64_t* idx_b, const double* sigma_point3,
                                               const double* sigma_cylinder7, double* d2, int32_t* dof /* may be NULL */,
                                               double* C81 /* may be NULL */, double* r9 /* may be NULL */, int32_t* status /* may be NULL */);
/* slide_graph_get_landmark_pair_covariances on the JOINT graph, the landmarks named as above: out324n[324 k ..] =
 * [[Saa, Sab], [Sba, Sbb]], 2 D x 2 D (D = 3 / 9 / 7, all three classes) row-major with leading dimension 18, zero padded — Sab between
 * landmarks of two robots included.  2 D unit columns per pair through the same forward half; the signed gram plus H_ll^-1 of each
 * private side completes the block, a shared side adds nothing.  Refusals (the message names chol_batch_get_landmark_pair_covariances;
 * any landmark class, no sigma) and the status words SLIDE_MISSING and SLIDE_ERR_INVALID are those of the test. */
int slide_chol_batch_get_landmark_pair_covariances(slide_chol_batch_t* b, int n, const int32_t* cls, const int32_t* slot_a, const uint64_t* idx_a,
                                                   const int32_t* slot_b, const uint64_t* idx_b, double* out324n,
                                                   int32_t* status /* may be NULL */);
/* slide_graph_landmark_pairs_within over the JOB's landmarks of one class: every member's private landmarks and each shared slot ONCE,
 * through its lowest replica, in (slot, index) order; the anchors (point xyz, cube translation, cylinder root) are gathered from the
 * members' device-resident estimates into one array and searched as slide_pairs_within searches.  cross_only != 0 drops the pairs
 * whose two ends are private landmarks of the same member (a shared slot pairs with anything).  Pairs come back as (slot_a, idx_a,
 * slot_b, idx_b, dist), sorted by their positions in that order; *n_pairs is always the total; above cap SLIDE_ERR_CAPACITY and nothing
 * but n_pairs is written.  Refusals as slide_graph_landmark_pairs_within (the message names chol_batch_landmark_pairs_within; the
 * batch is NULL), then those of slide_chol_batch_get_pose_covariances.  The batch is only read. */
int slide_chol_batch_landmark_pairs_within(slide_chol_batch_t* b, int cls, double radius, int cross_only, int64_t cap, int32_t* slot_a,
                                           uint64_t* idx_a, int32_t* slot_b, uint64_t* idx_b, double* dist, int64_t* n_pairs);
/* ---- Robust loss on the exact joint multi-robot pass ------------------------------------------------------------------------------
 * No counterpart in the reference (its inter-robot factors are plain Between factors, graph.cpp:247-258); GTSAM users know it as
 * noiseModel::Robust on the closures of the joint graph.  slide_graph_set_robust_loss's rule, kinds, defaults and class_mask, as a
 * property of the BATCH, uniform over its member graphs: before every linearisation of slide_chol_batch_pass and of a cut pass
 * (part 0, after the ghosts are adopted) each member's loop-closure and relative-measurement Between factors are reweighted as on one
 * graph, and so is every inter-robot relative-pose factor (slide_graph_add_relative_meas_ghost; class bit 1) at BOTH robots that
 * hold it: both see the same two poses as bits, compute the same w, and the factor's six lambda rows enter the joint system scaled
 * by sqrt(w) as a whole.  The step is the Gauss-Newton step of the reweighted joint graph.  kind 0 clears the loss: the pass then has
 * the launches and gives the bits it gives without this call.  Every call restores the members' base sigmas, drops their resident
 * factors and the batch's cached joint Sigma and captures the passes again; the joint marginals, information gain, gate and
 * pose-pair marginals need a pass after it and then describe the reweighted system.  A graph that joins later takes the loss at the
 * next pass; one that leaves gets its base sigmas back and carries no loss.  The per-graph calls keep refusing (a graph with a loss
 * of its own cannot join; slide_graph_set_robust_loss refuses a member).
 * SLIDE_ERR_INVALID: kind outside 0 .. 4, a class_mask bit other than 0 and 1, a batch with PCG passes (slide_chol_batch_set_pcg > 0;
 * likewise slide_chol_batch_set_pcg > 0 while a loss is set: their step leaves the factors' cross block out). */
int slide_chol_batch_set_robust_loss(slide_chol_batch_t* b, int kind, double param, int class_mask);
/* slide_graph_get_closure_weights for the batch, after a pass (SLIDE_ERR_INVALID "pass first" before one, and after a change of the
 * loss or of a member until the next pass): slot by slot, the member's loop-closure (kind 1) and relative-measurement (kind 2)
 * Between factors in insertion order with ghost_id -1, then its ghost factors (kind 2) with ghost_id = their index in the job's
 * list (slide_graph_set_ghost_ids; -1 if unnamed): the local pose stands in from_* when it is the factor's first key and in to_*
 * otherwise, the other end as robot -1 and idx = its ghost slot.  A factor between two robots is listed once by each; the two rows
 * carry the same w and s2 bit for bit.  w = 1 and s2 = |r|^2 where the last pass's loss did not select the factor.  One gather and
 * one read-back for all members.  Any output pointer may be NULL; at most cap rows are written, *n_out is the full count. */
int slide_chol_batch_get_closure_weights(slide_chol_batch_t* b, int cap, int32_t* slot, int32_t* from_robot, uint64_t* from_idx, int32_t* to_robot,
                                         uint64_t* to_idx, int32_t* kind, int32_t* ghost_id, double* weight, double* s2, int* n_out);
/* Measurement (no counterpart in the reference): the reweighting launch of the batch's loss alone between two events on the batch's
 * stream; *ms: milliseconds.  The weights it writes belong to no pass (it sees the last pass's ghost values beside that pass's
 * results): slide_chol_batch_get_closure_weights is refused until the next pass, which writes them all again.  SLIDE_ERR_INVALID
 * without a loss. */
int slide_chol_batch_profile_robust_reweight(slide_chol_batch_t* b, double* const* d_bufs, double* ms);
/* ---- Observation loss on the exact joint multi-robot pass --------------------------------------------------------------------------
 * No counterpart in the reference; GTSAM users know it as noiseModel::Robust on the BearingRange / Cube / Cylinder factors of the
 * joint graph.  slide_graph_set_observation_loss's rule, kinds, defaults, floor and class_mask as a property of the BATCH, uniform
 * over its member graphs: in every slide_chol_batch_pass and cut pass (part 0) each member's landmark factors are linearised by
 * k_lin_lf_robust_b in k_lin_lf_b's place, a selected factor entering as sqrt(w) [r | J] - also into the shared landmarks' rows of
 * the separator system, so a false match onto a shared landmark is down-weighted for every robot that sees the landmark.  The step
 * is the Gauss-Newton step of the reweighted joint graph.  Same number of launches with and without; kind 0 clears the loss: the
 * pass then has the launches and gives the bits it gives without this call.  Independent of slide_chol_batch_set_robust_loss; both
 * may be set.  Every call (kind 0 included) drops the members' resident factors and the batch's cached joint Sigma and captures the
 * passes again; the joint marginals, information gain, gate and pose-pair marginals need a pass after it and then describe the
 * reweighted system.  A graph that joins later takes the loss at the next pass; nothing of a member is rewritten under the loss, so
 * one that leaves has nothing to restore.  The per-graph calls keep refusing (a graph with an observation loss of its own cannot
 * join; slide_graph_set_observation_loss refuses a member); slide_graph_get_observation_weights on a member reports w = 1 and the
 * s^2 of the SCALED record: use slide_chol_batch_get_observation_weights.
 * SLIDE_ERR_INVALID: kind outside 0 .. 4, a class_mask bit other than 0 .. 2, a param that is not a number, a batch with PCG passes
 * (slide_chol_batch_set_pcg > 0; likewise slide_chol_batch_set_pcg > 0 while a loss is set). */
int slide_chol_batch_set_observation_loss(slide_chol_batch_t* b, int kind, double param, int class_mask);
/* slide_graph_get_observation_weights for the batch, after a pass (SLIDE_ERR_INVALID "pass first" before one, after a change of the
 * observation loss, after a member joined, left or was replaced, and while a member holds another number of landmark factors than
 * the last pass linearised): slot by slot, the member's landmark factors in insertion order with the member's slot, the factor's
 * pose index, its landmark (cls: SLIDE_CLS_*, lm_idx: the member's own index), the weight w and the squared whitened norm s^2 (taken
 * before the scaling) of the last pass.  w = 1 where that pass ran without a loss or its mask left the class out.  One launch and
 * one read-back for all members.  Any output pointer may be NULL; at most cap rows are written, *n_out is the full count. */
int slide_chol_batch_get_observation_weights(slide_chol_batch_t* b, int cap, int32_t* slot, uint64_t* pose_idx, int32_t* cls, uint64_t* lm_idx,
                                             double* weight, double* s2, int* n_out);
/* Measurement (no counterpart in the reference): the linearisation launch of a batched pass alone (k_lin_lf_b, or k_lin_lf_robust_b
 * while an observation loss is set) between two events on the batch's stream; *ms: milliseconds.  It linearises at the point the
 * last pass left; the read-backs and the joint queries are refused until the next pass. */
int slide_chol_batch_profile_linearize(slide_chol_batch_t* b, double* const* d_bufs, double* ms);
/* The same pass for a job that spans GPUs, cut at its two exchanges (8 / N robots on each of N GPUs): every part is a captured
 * hipGraph replayed on the batch's stream.
 *   part 0: phase 0 of every robot + the local sum -> every local buffer holds this GPU's sum of the 54-doubles-per-slot blocks;
 *           the caller all-reduces d_bufs[0][0 .. 54 n_slots) across the ranks ON slide_chol_batch_stream() (RCCL), no host sync;
 *   part 1: d_bufs[0] back to the other local buffers, Schur + batched factor + solve + t_l, local sum of 9 doubles per slot;
 *           the caller all-reduces d_bufs[0][0 .. 9 n_slots);
 *   part 2: d_bufs[0] back to the others, landmark back-substitution, retract; ONE host synchronisation, status decoded.
 * slide_chol_batch_stream: the hipStream_t (as void*) the parts run on. */
int slide_chol_batch_pass_part(slide_chol_batch_t* b, double* const* d_bufs, int part);
void* slide_chol_batch_stream(slide_chol_batch_t* b);
/* Joint Gauss-Newton step over the robots (what the reference's replica computes: solve() on ONE graph holding every robot,
 * graph.cpp:260-272 + sloamNode.cpp:912-1002).  With iterations = 0 a pass solves every robot's own reduced pose system only — block
 * Jacobi over robots, which stops converging once the robots share more than a few landmarks.  With iterations > 0 the pass runs
 * that many preconditioned conjugate-gradient iterations on the GLOBAL reduced system after the factorisations (the robots' factors
 * are the preconditioner; the coupling through the shared landmarks is applied matrix-free), two all-reduces per iteration
 * (9 doubles per shared slot, then 2 scalars).  A cut pass then reads
 *     part 0 | AR 54 n | part 1 | { AR 9 n | part 10 | AR 2 | part 11 (12 on the last iteration) } x iterations | AR 9 n | part 2
 * and the un-batched path (slide_graph_set_pcg on every graph)
 *     phase 0 | AR 54 n | phase 1 | { AR 9 n | phase 31 | AR 2 | phase 32 (33 last) } x iterations | AR 9 n | phase 2
 * with every all-reduce on the first max(1, ..) doubles of the exchange buffer. */
int slide_chol_batch_set_pcg(slide_chol_batch_t* b, int iterations);
int slide_graph_set_pcg(slide_graph_t* g, int iterations);
/* Residual-based end of that iteration: `iterations` stays the upper bound per pass; with tol > 0 the solve counts as converged once
 * gamma = r^T M^-1 r has fallen to tol^2 times its value in the first iteration (never later than at eps^2) — the remaining iterations
 * of the pass are no-ops (alpha = beta = 0), so captured launch sequences keep their shape and every rank takes the same decision from
 * the same all-reduced scalars.  Call before slide_*_set_pcg or repeat that call. */
int slide_chol_batch_set_pcg_tolerance(slide_chol_batch_t* b, double tol);
int slide_graph_set_pcg_tolerance(slide_graph_t* g, double tol);
/* EXACT joint Gauss-Newton step over the robots ("arrow" solve) — what the reference's replica computes with ONE solve() on a graph
 * holding every robot (graph.cpp:260-272 on the replica of sloamNode.cpp:912-1002), without an inner iteration.  The landmarks of the
 * shared slots are not eliminated into the robots' pose systems: they stay as the SEPARATOR of the joint graph.  Every robot eliminates
 * its private landmarks, factors its banded pose system with the separator's coupling rows riding below the band (the step kernels),
 * and forms its Schur complement onto the separator with one FP64-MFMA product; the sum over the robots — ONE all-reduce(sum) of the
 * separator buffer per pass for a job that spans GPUs — is the Schur complement of the JOINT graph onto the shared landmarks; every rank
 * factors it (dense, the same step kernels), substitutes back through its bands and retracts.
 *   slide_graph_set_separator: off[i] = offset of shared slot i's tangent coordinates (cylinder 7, cube 9, point 3) in the separator
 *     system — any non-overlapping layout —, off[n_slots] = its dimension; n = n_slots + 1 entries, identical on every rank; after
 *     slide_graph_set_shared.
 *   slide_chol_batch_set_exact_joint(b, 1, sep_buf, len): passes of the batch take the exact joint step (batched passes only; the PCG
 *     setting is ignored).  sep_buf: the caller's device buffer of slide_chol_batch_sep_buffer_len(m) doubles, m = off[n_slots], in which
 *     part 0 of a cut pass leaves this GPU's partial sum of the separator system (packed: the lower tile columns only) and from which
 *     part 2 takes the all-reduced sum; NULL when the job is this process alone (whole passes only).
 * A cut pass then reads   part 0 | all-reduce(sum) of sep_buf[0 .. len) on slide_chol_batch_stream() | part 2.
 * With inter-robot relative-pose factors (slide_graph_set_ghosts) every pass, cut or whole, PCG or exact, opens with the refresh of the
 * ghost poses; a cut pass reads   part 20 | all-reduce(sum) of d_bufs[0][0 .. 12 n_ghost_slots) | part 0 | ...  (the exchange buffers
 * must hold 12 doubles per ghost slot).  The cross block of such a factor is left out of the step (gradient exact). */
int slide_graph_set_separator(slide_graph_t* g, const int32_t* off, int n);
int slide_chol_batch_set_exact_joint(slide_chol_batch_t* b, int on, double* sep_buf, long long len);
/* Tile-level profile of the separator system (64-coordinate tiles, landmark part): prof[c] = last tile row of tile column c that can be
 * non-zero, monotone, c <= prof[c] < n.  Two shared landmarks couple there only if some robot observes both, so with the slots'
 * coordinates laid out along the robots' adjacency (slide_graph_set_separator takes any layout) the system is block-banded; the caller
 * knows every robot's observer set (the cross-robot association), the batch only its own robots'.  Not set: dense. */
int slide_chol_batch_set_separator_profile(slide_chol_batch_t* b, const int32_t* prof, int n);
/* Nested dissection of the separator system itself.  The robots split into two sets; a shared landmark seen only by robots of one set
 * couples with none seen only by robots of the other, so the layout puts those two "leaf" blocks first (Ta, Tb tile columns; each
 * starts at a tile boundary, used_a / used_b coordinates of it carry slots, the rest of its last tile is padding and gets a unit
 * diagonal) and the landmarks seen from both sets ("top" block) behind them.  The leaves are factored side by side — half the serial
 * chain of block columns, and no arithmetic on the structural zeros between them — with the top block's rows riding as their border
 * (as the lambda rows do), then the top block.  The profile (above) must end each leaf at its own last tile row.  Same step: only the
 * elimination order changes.  (0, 0, 0, 0): not dissected (default).  The reference has no counterpart: its replica solves the joint
 * system inside GTSAM (graph.cpp:260-272), whose elimination order is COLAMD's. */
int slide_chol_batch_set_separator_blocks(slide_chol_batch_t* b, int Ta, int Tb, int used_a, int used_b);
/* A job that spans GPUs whose ranks split in two halves ALONG the dissection (the robots of the first half of the ranks see leaf a and
 * the top block only, those of the second half leaf b and the top block): this rank owns leaf `leaf` (0 / 1; -1: none, the default).  It
 * factors that leaf only, and only the top block of the separator system crosses between the halves.  A cut pass then runs
 *   [20 | AR ghosts |] part 0 | all-reduce of the OWN leaf's segment of sep_buf within the own half (nothing when the half is one rank) |
 *   part 1 | all-reduce of the top segment over all ranks | part 2
 * (slide_chol_batch_sep_segment gives the segments' offsets and lengths in doubles: which = 0 leaf a, 1 leaf b, 2 top block + lambdas).
 * leader: non-zero on ONE rank of each half — the one that adds the leaf's Schur complement to the top block's sum.  C4 on two GPUs:
 * 5 MB cross the link per pass instead of 45. */
int slide_chol_batch_set_separator_owner(slide_chol_batch_t* b, int leaf, int leader);
int slide_chol_batch_sep_segment(int m, int n_relmeas, int Ta, int Tb, int which, long long out2[2]);
/* Nested dissection of every robot's own pose chain inside an exact joint pass: the banded pose system of a robot is a serial chain of
 * block columns (one launch each); cut into n_seg segments at windows of poses as wide as the band is (every coupling across a window
 * passes through it), the segments are factored side by side as systems of their own, and the windows' poses — moved into the border
 * next to the shared landmarks — are eliminated at a second level before the robot's Schur complement joins the separator system.
 * Same step (the elimination order changes, not the system); n_seg = 1 (default) factors every band as one chain; at most 8. */
int slide_chol_batch_set_segments(slide_chol_batch_t* b, int n_seg);
/* The cut of this graph's band: returns the number of segments (1: not cut — the batch does not ask for it, or the chain is too short);
 * out[2 i], out[2 i + 1] = tile columns [t0, t1) of segment i, out[2 n] = number of separator poses (cap >= 2 n + 1 ints). */
int slide_graph_get_segments(slide_graph_t* g, int* out, int cap);
/* Which border tile rows are non-zero in which segment of the cut band, and from which block column on (measurement aid: the flop count
 * of the steps and of the border product follows from it).  Returns the table's length (0: the band is not cut) and fills out[0 .. cap):
 * nseg, the segments' last block columns + 1, then per segment nbr + 1 ints = the first block column of every border tile row and of the
 * right-hand side (1 << 30: the row is all-zero in that segment). */
int slide_graph_get_segment_table(slide_graph_t* g, int* out, int cap);
long long slide_chol_batch_sep_buffer_len(int m, int n_relmeas);
/* Doubles at the head of that buffer a cut pass has to all-reduce: all of it, less the block between the two leaves of a dissected
 * layout (slide_chol_batch_set_separator_blocks: Ta x Tb tiles that are structurally zero and left out of the packed layout). */
long long slide_chol_batch_sep_exchange_len(int m, int n_relmeas, int Ta, int Tb);
/* Inter-robot relative-pose factors in an exact joint pass: the factor between pose a of robot A and pose b of robot B is the rank-6
 * term U U^T, U = [J_a^T; J_b^T], of the joint normal equations; it is carried as six further separator coordinates "lambda" (the
 * factor's linearised residual) of the bordered system [H_rest U; U^T -I] [delta; lambda] = [b; -r]: every robot couples to them through
 * its OWN Jacobian only, and the step is exactly the joint replica's.  ids[i] = index, in the job's list of n_total measurements
 * (identical on every rank), of this graph's i-th ghost factor (slide_graph_add_relative_meas_ghost order); the ghost poses are still
 * refreshed at the start of every pass: they are where the factor is linearised. */
int slide_graph_set_ghost_ids(slide_graph_t* g, const int32_t* ids, int n, int n_total);
/* Scalars of the last joint solve this graph took part in: out8 = {gamma of the last but one iteration, alpha of it, alpha, beta of the
 * last iteration, gamma of the FIRST iteration, gamma of the last; 0, 0} with gamma = r^T M^-1 r (M = the robots' own factors), summed
 * over all robots: gamma_last / gamma_first is the squared reduction of the preconditioned residual. */
int slide_graph_get_pcg_stats(slide_graph_t* g, double out8[8]);
/* Tile-level profile (envelope) of the reduced pose system the solver works in (64 x 64 tiles; the reference's sparse elimination,
 * ISAM2 graph.cpp:260-272, exploits the same structure): returns T, the number of block columns, and writes prof[c] = the last tile row
 * of block column c that can be non-zero in the factor (c <= prof[c] < T, monotone) for c < min(T, cap).  Pending additions are
 * merged first.  slide_graph_set_dense_profile(g, 1) makes the solver ignore the structure (every tile of the lower triangle: the
 * GEMM-shaped extreme, a measurement aid); results are the same either way. */
int slide_graph_get_tile_profile(slide_graph_t* g, int* prof, int cap);
/* Incremental re-factorisation of slide_graph_solve (ISAM2::update re-eliminates only the part of the Bayes tree the new factors and the
 * relinearised variables touch, graph.cpp:260-272; here: the block columns of the banded reduced system from the first dirty one on —
 * the columns before it keep the factor of the last solve, the re-assembled trailing tiles catch up with their panels in one product,
 * the step kernels run on the trailing sub-matrix).  out4 = {updates that re-factored a suffix only, updates that re-factored
 * everything, first re-factored block column of the last update, block columns}.  slide_graph_set_incremental(g, 0) (or
 * SLIDE_NO_INCREMENTAL=1 for the whole process) re-factors everything at every update: the same result up to the summation order of
 * the kept columns' panels. */
int slide_graph_get_incremental_stats(slide_graph_t* g, int64_t out4[4]);
/* iSAM2's bounded back-substitution (ISAM2GaussNewtonParams::wildfireThreshold — 1e-3 in the GTSAM 4.0.3 the reference links, used by
 * every ISAM2::update + calculateEstimate() of SemanticFactorGraph::solve, graph.cpp:15-18, 260-272): on an incremental update a block
 * of the reduced system below the first re-factored block column keeps the last solve's solution when every block it depends on moved
 * by less than `threshold` (infinity norm), and so does everything below it; the chained substitution then ends there.  threshold 0 (the
 * default): off — every update solves its linear system exactly, which is what the parity tests compare.  out2 = {blocks kept over all
 * updates, blocks kept by the last update}. */
int slide_graph_set_wildfire(slide_graph_t* g, double threshold);
int slide_graph_get_wildfire_stats(slide_graph_t* g, int64_t out2[2]);
int slide_graph_set_incremental(slide_graph_t* g, int on);
int slide_graph_set_dense_profile(slide_graph_t* g, int on);
/* Exact joint step: the border of this graph's reduced system — returns the number of border row tiles (64 separator coordinates each;
 * 0 when the graph's batch does not run exact joint passes) and writes first[i] = the first block column of the band in which border
 * tile row i can be non-zero (the border product skips the columns before it) for i < min(n, cap). */
int slide_graph_get_border_profile(slide_graph_t* g, int* first, int cap);
/* Measurement aid: the same pass issued without the graph, HIP events around the batched step kernels; *ms_steps = their device time
 * (launch gaps included), *n_launches = their number. */
int slide_chol_batch_profile(slide_chol_batch_t* b, double* const* d_bufs, double* ms_steps, int* n_launches);
/* The same for an exact joint pass, stage by stage (HIP events on the pass's stream): out6 = ms of {assembly (relinearisation ..
 * borders), the bands' factorisations, the border products (k_border_syrk), the separator gather, the separator's factorisation +
 * solve, the back-substitutions}; *n_sep_steps = block columns of the separator system. */
int slide_chol_batch_profile_exact_joint(slide_chol_batch_t* b, double* const* d_bufs, double out6[6], int* n_sep_steps);
/* Sharded mode, inter-robot relative-pose factors (addRelativeMeasFactor graph.cpp:247-258 between poses of two ranks).
 * Ghost slots enumerate, identically on every rank, the poses such factors touch; slot i is this rank's pose
 * (own_robot[i], own_idx[i]) or belongs to another rank (own_robot[i] < 0).  A factor is added on BOTH ranks, each with its
 * own pose as the variable and the other pose as ghost slot; local_first = 1 when the local pose is the Between's first key.
 * Per pass, before phase 0: dist_phase 20 (pack 12 doubles per slot), all-reduce(sum), dist_phase 21 (adopt). */
int slide_graph_set_ghosts(slide_graph_t* g, const int32_t* own_robot, const int64_t* own_idx, int n_slots);
int slide_graph_add_relative_meas_ghost(slide_graph_t* g, const double rel7[7], uint64_t idx, int robot, int ghost_slot, int local_first);
/* Landmark table of this rank (input of the cross-robot association): for class cls, positions (xyz of the
 * current estimate; cylinders: root) and labels of landmarks [0, n).  Returns n (<= cap). */
int slide_backend_landmark_table(slide_backend_t* b, int cls, double* xyz, int32_t* label, int cap);

/* The dense kernel behind solve(): x = A^-1 b for a symmetric positive definite A (n x n, row- or
 * column-major: only the lower triangle in column-major sense, A[i + j*n] with i >= j, is read) by
 * the blocked FP64-MFMA Cholesky the reduced pose system uses (the reference delegates this to
 * GTSAM's CHOLESKY factorisation, graph.cpp:15).  ms_out (may be NULL): device time of `repeats`
 * factor+solve passes measured with HIP events on the launch stream. */
int slide_dense_spd_solve(const double* A, int n, const double* b, double* x, int repeats, double* ms_out);
/* The same solve by an explicit schedule of the factorisation: method 0 = one step launch per 64-column block (what
 * slide_dense_spd_solve runs), 1 = the left-looking persistent factorisation (ONE launch for all block columns, flags between
 * workgroups instead of kernel boundaries; opt-in for the exact joint passes, SLIDE_CHOL_LL), 2 = TWO block columns per launch
 * (k_chol_pair_batched: every type-A workgroup carries the sub-diagonal tile and the next diagonal block as well, so that the second
 * column's chain starts inside the launch — what the exact joint passes use; ISAM2Params::CHOLESKY of graph.cpp:15 all the same). */
int slide_dense_spd_solve_ex(const double* A, int n, const double* b, double* x, int repeats, double* ms_out, int method);
/* Unit-test hook of the same kernels on a BORDERED system with a profile — one system exactly as an exact joint pass hands it to the
 * factorisation (a robot's band segment with the separator's coupling rows riding below it, a leaf of the separator system: DESIGN.md 3):
 * S_in (ld x T*64 doubles, column-major): the band's lower tiles inside the profile, nbr border row tiles from tile row b0 on (0: right
 * behind the band), the right-hand-side row tile behind them.  prof: T ints (last tile row of every block column inside the profile)
 * or NULL = dense; bfirst: nbr non-decreasing ints = first block column (+ kofs) of the j-th border row in the order `ord` lists them
 * (1 << 30: never), or NULL = every row from column 0; ord: nbr ints (the j-th active row is tile row b0 + ord[j]) or NULL.  The system
 * is factored n_copies (<= 32) times side by side in one launch sequence; S_out / Ld_out (T x 64 x 64) / Winv_out (T x 1024) /
 * status_out (8) receive copy 0, *max_copy_diff the largest difference of any other copy from it.  method 0: one step launch per block
 * column, 2: two block columns per launch.  After the call the band tiles hold L, the border rows W = B L^-T, the RHS row y = L^-1 b. */
int slide_debug_chol_bordered(const double* S_in, int ld, int T, int nbr, const int* prof, const int* bfirst, const int* ord, int b0, int kofs,
                              int n_copies, int method, double* S_out, double* Ld_out, double* Winv_out, int* status_out, double* max_copy_diff);
/* The same hook for a MIXED batch: n (1 .. 32) different systems in ONE launch sequence, each with its own tables, and with the launch
 * shape under the caller's control.  Per system i: ld[i], T[i], nbr[i], b0[i], kofs[i] as above; S_in / S_out hold the systems one after
 * the other (system i: ld[i] * T[i] * 64 doubles), Ld_out / Winv_out likewise (T[i] * 4096 / T[i] * 1024 doubles), status_out 8 ints each.
 * prof / bfirst / ord are concatenated tables; prof_off[i] / bfirst_off[i] / ord_off[i] is where system i's T[i] resp. nbr[i] ints start,
 * or -1 for NULL (dense / every row from column 0 / rows in their own order).  method 0 / 2 as above.  cu_share (0 .. 100): the percentage
 * of the compute units the launch sequence may count on, as the production passes hand it to the launches.  assumed_cus: 0 = plan the
 * launches for the device's own number of compute units, 1 .. that number = plan them as a device with that many would (a smaller count
 * only: the grid never grows beyond what the device itself could be given); for the duration of this call, on this thread only.
 * want_l32 != 0: every system with b0[i] == 0 also gets the packed f32 factor copy the joint solve's preconditioner streams
 * (T (T-1) / 2 * 4096 + 4 floats, prefilled with the bit pattern 0x7fc0dead; tile (j, c), c < j, at 4096 * (c (T-1) - c (c-1) / 2 + j - c - 1),
 * element (row, col) at col * 64 + row); L32_out receives them one after the other in system order (the others take no room).  The pair
 * kernel does not write that copy: method 2 then runs the step kernels.  trace_out (5 ints per row, trace_cap rows; may be NULL): one row
 * {k, a_split, a_joins, type-A workgroups, queue items} per launch actually issued (a_split: 0 for the pair kernel), *n_launches their
 * number, *n_cu_out the number of compute units the plan was made for.  SLIDE_ERR_INVALID (nothing launched) for n outside 1 .. 32,
 * cu_share outside 0 .. 100, assumed_cus above the device's count, an ld[i] below (B0 + nbr + 1) * 64. */
int slide_debug_chol_batch(int n, const double* S_in, const int* ld, const int* T, const int* nbr, const int* prof, const int* prof_off,
                           const int* bfirst, const int* bfirst_off, const int* ord, const int* ord_off, const int* b0, const int* kofs,
                           int method, int cu_share, int assumed_cus, int want_l32, double* S_out, double* Ld_out, double* Winv_out,
                           int* status_out, float* L32_out, int* trace_out, int trace_cap, int* n_launches, int* n_cu_out);
/* Its host-only twin: the launches slide_debug_chol_batch would issue for these systems on a device with assumed_cus (>= 1) compute
 * units, from the same planning code, without touching a device.  Returns the number of launches (<= trace_cap rows written) or
 * SLIDE_ERR_INVALID. */
int slide_debug_chol_plan(int n, const int* T, const int* nbr, const int* prof, const int* prof_off, const int* bfirst, const int* bfirst_off,
                          const int* b0, const int* kofs, int method, int cu_share, int assumed_cus, int* trace_out, int trace_cap);
/* LDS flag waits of the pair kernel (method 2) that gave up since the library was loaded: 0 unless the kernel is broken (its waits are
 * bounded so that every wave reaches the end of its launch); the tests assert 0. */
int slide_debug_pair_timeouts(void);
/* Unit-test hook of the border product (k_border_syrk and its reductions) on caller data: n (1 .. 8) systems AFTER their steps, handed to
 * launch_border_syrk (jobs == NULL: the plain (ib, jb, system) grid) or launch_border_syrk_jobs (a job table of njobs codes
 * system << 20 | ib << 10 | jb, lds_pad bytes of idle LDS per workgroup) exactly as the exact joint passes do.  Per system i: S_in holds
 * ld[i] x T[i]*64 doubles (column-major; W^T in the nbr[i] border row tiles from tile row B0 = b0[i] > 0 ? b0[i] : T[i] on, y^T in row 0 of
 * the tile behind them, whose rows 1 .. 63 the caller keeps zero), bord_in ldb[i] x bord_cols[i] doubles (the border block in its first
 * (nbr + 1) * 64 rows and nbr * 64 columns; what lies beyond must come back as it was), the systems one after the other in both.
 * bfirst / segtab are concatenated tables, bfirst_off[i] / segtab_off[i] where system i's nbr[i] + 1 first columns resp. its
 * segtab_len[i] ints in HostGraph::seg_tab's layout (nseg, the segments' end columns, per segment nbr + 1 first columns with 1 << 30 =
 * inactive, then the masks' head) start, or -1 for none (the offset arrays themselves may be NULL).  has_src[i] != 0: system i reads its
 * tiles from bord_src (laid out like bord_in) and writes bord = bord_src - W W^T.  ks > 1: split K of ONE system over ks chunks of its
 * column blocks; fuse_add != 0: the fused two-system launch (system 0's block += system 1's), ks_sys[2] (or NULL: ks for both) chunks
 * each; jb_end >= 0: the table and the reduction stop short of tile column jb_end.  The partial tiles live in scratch the hook allocates
 * itself at the passes' own size, (nbr + 1) * nbr * (max chunks - 1) tiles per system (two systems' for the fused launch), zeroed — or,
 * with use_prefill != 0, filled with `prefill` (what a reused buffer may hold) — between two guard tiles of a fixed bit pattern:
 * SLIDE_ERR_HIP when a guard was written.  bord_out / S_out (may be NULL) receive every system's block and its S (which must be
 * unchanged).  SLIDE_ERR_INVALID, nothing launched, for what the launchers do not define: ks > 1 or the fused launch together with a
 * segtab; fuse_add with n != 2, unequal nbr, a bfirst, no job table or no system split; ks > 1 with n > 1 and no fuse_add; an odd ld or
 * ldb; ld < (B0 + nbr + 1) * 64; ldb < (nbr + 1) * 64; a job code that names a system >= n or, split, a tile column >= jb_end; jb_end,
 * lds_pad or ks_sys without what they belong to; a table the kernels would read out of bounds. */
int slide_debug_border_product(int n, const double* S_in, const int* ld, const int* T, const int* nbr, const int* b0, const double* bord_in,
                               const int* ldb, const int* bord_cols, const int* bfirst, const int* bfirst_off, const int* segtab,
                               const int* segtab_off, const int* segtab_len, const double* bord_src, const int* has_src, const int* jobs,
                               int njobs, int lds_pad, int ks, const int* ks_sys, int jb_end, int fuse_add, int use_prefill, double prefill,
                               double* bord_out, double* S_out);
/* The same for k_border_apply: yv -= W x_loc over the band's columns of n (1 .. 8) systems in ONE launch (launch_border_apply).  S_in, ld,
 * T, nbr, b0 and the segments' tables as above (a table whose masks' head is > 0 takes the mask walk, any other the full walk); yv_in /
 * yv_out: T[i] * 64 doubles per system, x_loc: nbr[i] * 64, each one system after the other. */
int slide_debug_border_apply(int n, const double* S_in, const int* ld, const int* T, const int* nbr, const int* b0, const double* yv_in,
                             const double* x_loc, const int* segtab, const int* segtab_off, const int* segtab_len, double* yv_out);
/* Unit-test hooks of the kernels that READ the factor (cov_kernels.hip, joint_cov_kernels.hip, k_cov_fwd / k_cov_gram), on a caller-given
 * factor: no factorisation runs inside them.  The factor's layout is the one slide_debug_chol_bordered returns: S_in (ld x T*64 doubles,
 * column-major) with L(i, k) in tile (i, k) for k < i <= prof[k] (prof: T ints or NULL = dense), Ld_in (T x 64 x 64) with the sub-diagonal
 * 16x16 blocks of L_kk, Winv_in (T x 1024) with the inverses of its four diagonal 16x16 blocks ((L_bb^-1)[r][j] at b*256 + j*16 + r).
 * Every hook uploads, synchronises, calls the production launcher on the null stream, synchronises and downloads.  SLIDE_ERR_INVALID,
 * nothing launched, for what the launchers do not define: T < 1, ld < T*64, an odd ld, a prof that decreases or has prof[k] < k or >= T,
 * nrhs < 1, ncol_alloc < nrhs, k0 outside 0 .. T-1 (or != 0 with mode 0), a stage or mode other than 0 / 1, a row0 whose six rows leave
 * the system, a gram row outside 0 .. ldx-1.
 * slide_debug_selected_inverse: Sg and Z (ld * T * 64 doubles each, pre-filled by the caller) through launch_selected_inverse (stage 1,
 * as the marginals call it) or its first launch alone (stage 0: k_sinv_prep); both come back, and S_out / Ld_out / Winv_out (may be
 * NULL) receive the factor as the device holds it afterwards (unchanged). */
int slide_debug_selected_inverse(const double* S_in, int ld, int T, const double* Ld_in, const double* Winv_in, const int* prof, int stage,
                                 double* Sg, double* Z, double* S_out, double* Ld_out, double* Winv_out);
/* B and X: ncol_alloc columns of T*64 rows each, in and out.  mode 0: launch_multi_solve (X = S^-1 B over the first nrhs columns, B
 * overwritten); mode 1: launch_multi_fwd from block column k0 on (W = L^-1 B into X). */
int slide_debug_multi_solve(const double* S_in, int ld, int T, const double* Ld_in, const double* Winv_in, const int* prof, double* B, double* X,
                            int ncol_alloc, int nrhs, int mode, int k0);
/* launch_gram on X (ncol columns, leading dimension ldx) over the rows `rows` (nrows ints, or NULL: 0 .. nrows-1) into M: ncol x ncol
 * doubles plus one guard row of ncol behind them, in and out. */
int slide_debug_gram(const double* X, long long ldx, int ncol, const int* rows, int nrows, double* M);
/* launch_pose_covariance for the pose whose first row is row0, on six unit columns built as HostGraph::pose_covariance builds them; S_in
 * must be zero outside the profile (k_cov_fwd walks the dense column).  cov36: 36 doubles; Y_out (6 x T*64, may be NULL): the walk. */
int slide_debug_pose_covariance(const double* S_in, int ld, int T, const double* Ld_in, const double* Winv_in, int row0, double* cov36, double* Y_out);
/* The joint-tree selected inverse (k_jsinv_prep, k_jsinv_tile) on n (1 .. 9) caller-given systems, one after the other in every buffer.
 * System i: factor columns 0 .. Tb[i]-1 in S_in (ld[i] x Tb[i]*64), Tb[i] .. Tc[i]-1 in B_in (ldb[i] x (Tc[i]-Tb[i])*64, rows and columns
 * counted from Tb[i]), Ld_in / Winv_in for all Tc[i] columns (split at Tb[i] inside the hook), D = -I on the columns >= neg0[i], Sg and Z
 * (lds[i] x Trow[i]*64 doubles each, in and out; Trow[i] >= Tc[i] tile rows; the caller's Sg holds the Sigma of the rows past the columns,
 * k_jsig_gather's part).  rp (nrp ints) / rows (nrows ints): the columns' tile-row lists, system i's column c at rp[col0[i] + c] ..
 * rp[col0[i] + c + 1].  jobs: njobs (system, column) pairs, grouped into nsteps steps by step_off (nsteps + 1 ints).  launch_jsinv_prep
 * over all jobs; with stage 1 then one launch_jsinv_step per step with that step's largest row count (CholBatch's sequence).
 * SLIDE_ERR_INVALID, nothing launched: a row at or beyond Trow[i] or <= its column, a row or a job listed twice, leading dimensions below
 * what the lists reach, offsets that leave their tables. */
int slide_debug_joint_selected_inverse(int n, const double* S_in, const int* ld, const int* Tb, const double* B_in, const int* ldb, const int* Tc,
                                       const double* Ld_in, const double* Winv_in, const int* neg0, const int* col0, const int* lds,
                                       const int* Trow, const int* rp, int nrp, const int* rows, int nrows, const int* jobs, int njobs,
                                       const int* step_off, int nsteps, int stage, double* Sg, double* Z);

/* ------------------------------------------------------------------------------------------------
 * S3 — association (include/core/sloam.h:88-108, src/core/sloam.cpp:73-306; *MapManager::getSubmap)
 * Stand-alone entry points on caller-provided host buffers (copied to HBM, kernels run, results copied back).
 * ---------------------------------------------------------------------------------------------- */
/* *MapManager::getSubmap candidate gate (cubeMapManager.cpp:36-75 etc.): exact float32 K-NN of the
 * first-seen cloud to the query position; out_idx = map indices nearest first, *out_k = min(K, n). */
int slide_submap_knn(const float* cloud_xyz, uint64_t n, const double query_xyz[3], int K, int32_t* out_idx, int* out_k);
/* sloam::matchModels sloam.cpp:73-111 (cylinders; objects in the world frame). out = submap index or -1. */
int slide_assoc_match_cylinders(int n_cur, const double* root, const double* ray, const int32_t* label, int n_map,
                                const double* map_root, const double* map_ray, const int32_t* map_label, double thresh,
                                int32_t* out_idx);
/* sloam::matchCubeModels :113-156 (cls = SLIDE_CLS_CUBE, labels ignored) and
 * sloam::matchEllipsoidModels :158-203 (cls = SLIDE_CLS_ELLIPSOID, label-gated). */
int slide_assoc_match_boxes(int cls, int n_cur, const double* xyz, const int32_t* label, int n_map, const double* map_xyz,
                            const int32_t* map_label, double thresh, int32_t* out_idx);
/* Batched association sweep (roofline leg): n_query independent frames, each n_obs ellipsoid detections
 * (xyz + label) against ONE resident map of n_map landmarks: K-NN gate to each query's robot position
 * (ellipsoidMapManager.cpp:40-80), then label-gated nearest neighbour (sloam.cpp:158-203).  Inputs are DEVICE pointers (already
 * resident in HBM); the first-seen cloud is SoA (x[], y[], z[]: three coalesced float32 streams).  Runs on `stream` (a hipStream_t
 * cast to void*, NULL = default stream).  out_map_idx: n_query * n_obs map indices or -1.  The map may be of any size;
 * SLIDE_ERR_CAPACITY when min(K, n_map) exceeds the on-chip sort buffer (16384). */
int slide_assoc_sweep_batch_device(const float* d_cloud_x, const float* d_cloud_y, const float* d_cloud_z, const double* d_model_xyz,
                                   const int32_t* d_label, int n_map, const double* d_query_pos, const double* d_obs_xyz,
                                   const int32_t* d_obs_label, int n_query, int n_obs, int K, double thresh, int32_t* d_out_map_idx,
                                   void* stream);

/* The same sweep on caller-provided HOST buffers (cloud_xyz: AoS float32 as for slide_submap_knn): inputs are uploaded once, then
 * `repeats` launches run on the resident inputs; *ms_out (may be NULL) = their device time measured with HIP events on the launch
 * stream (uploads and the result copy excluded). */
int slide_assoc_sweep_batch(const float* cloud_xyz, const double* model_xyz, const int32_t* label, int n_map, const double* query_pos,
                            const double* obs_xyz, const int32_t* obs_label, int n_query, int n_obs, int K, double thresh,
                            int32_t* out_map_idx, int repeats, double* ms_out);

/* ------------------------------------------------------------------------------------------------
 * S2 + runSLOAMNode — the per-key-frame update (src/core/sloamNode.cpp:762-1036 without ROS):
 * submap gate -> projectModels -> match -> updateMap -> addSLOAMObservation -> solve ->
 * updateFactorGraphMap -> getCurrPose.
 * ---------------------------------------------------------------------------------------------- */
/* Body-frame detections of one key frame: field order/precision of sloam_msgs/SemanticMeasSyncOdom
 * (ROSCylinder/ROSCube/ROSEllipsoid; float32 fields already widened to double by the caller). */
typedef struct slide_detections_t {
  int n_cyl;
  const double* cyl_root;    /* 3 * n_cyl */
  const double* cyl_ray;     /* 3 * n_cyl */
  const double* cyl_radius;  /* n_cyl */
  const int32_t* cyl_label;
  int n_cube;
  const double* cube_pose7;  /* 7 * n_cube */
  const double* cube_scale;  /* 3 * n_cube */
  const int32_t* cube_label;
  int n_ell;
  const double* ell_pose7;
  const double* ell_scale;
  const int32_t* ell_label;
} slide_detections_t;

typedef struct slide_frame_result_t {
  double out_pose7[7];   /* outPose (sloamNode.cpp:1028) */
  int32_t* cyl_match;    /* caller buffers (may be NULL): submap index or -1, sloam.cpp:224-226 */
  int32_t* cube_match;
  int32_t* ell_match;
  int32_t* cyl_id;       /* global landmark ids used in the graph (L / C / U index) */
  int32_t* cube_id;
  int32_t* ell_id;
  int optimized;         /* addSLOAMObservation's return value */
  double ms_association; /* the two timers the reference keeps (sloamNode.cpp:845-849, 888-897), host wall clock */
  double ms_graph;
} slide_frame_result_t;

#define SLIDE_FRAME_HOST 0           /* host robot's own key frame: pose = prev * rel; add + solve + map refresh */
#define SLIDE_FRAME_HOST_DEFERRED 1  /* same, map refresh deferred to slide_backend_end_frame (foreign packets pending) */
#define SLIDE_FRAME_FOREIGN 2        /* another robot's packet (sloamNode.cpp:938-999): prev7 is the key pose ALREADY in the host frame; no solve */

slide_backend_t* slide_backend_create(const slide_params_t* p);
void slide_backend_destroy(slide_backend_t* b);
int slide_backend_process_frame(slide_backend_t* b, int mode, int robot, const double rel7[7], const double prev7[7],
                                const slide_detections_t* det, slide_frame_result_t* res);
int slide_backend_ingest_solve(slide_backend_t* b);                        /* sloamNode.cpp:1000 */
int slide_backend_end_frame(slide_backend_t* b, int robot, double out7[7]); /* sloamNode.cpp:1010-1014 */
slide_graph_t* slide_backend_graph(slide_backend_t* b);                    /* borrowed; owned by the backend */
/* [cyl_counter_, cube_counter_, point_landmark_counter_, #factors] + pose_counter_robot_ (graphWrapper.h:128-134) */
int slide_backend_counts(slide_backend_t* b, uint64_t out4[4], uint64_t* pose_counters, int n_robots);
/* map model read-back (getRawMap): cylinder -> 7 doubles; cube / ellipsoid -> xyz + scale (6 doubles) */
int slide_backend_map_model(slide_backend_t* b, int cls, int idx, double* out, int* hits, int* label);
/* The association gate of the streaming path: a frame's matches tested at the PREDICTED pose before they are added.  No counterpart in
 * the reference, which accepts a match on its Euclidean threshold alone (sloam.cpp:73-203).  Off by default (prob == 0): a back-end
 * that never calls this, or calls it with 0, launches what it launched and gives the bits it gave.
 * With 0 < prob < 1 the gate runs in slide_backend_process_frame for SLIDE_FRAME_HOST / _HOST_DEFERRED frames of a robot whose
 * pose counter is > 0, after the association kernel's read-back and before the map is updated: every matched detection becomes a
 * candidate of slide_graph_predicted_observation_mahalanobis (from pose = pose counter - 1, rel7 and est7 = prev * rel of the frame,
 * the matched landmark id, the measurement the frame would add), ONE call tests them, and a candidate with status 0 and
 * d2 > slide_chi2_quantile(prob, dof) is rejected: SLIDE_GATE_DROP — no factor, no hit, no map entry, *_id[i] = -1; SLIDE_GATE_NEW —
 * treated as unmatched: a new map entry and a new landmark.  Either way *_match[i] = SLIDE_MATCH_GATED.  A candidate whose status
 * is not 0 keeps its match.  Where the query is refused for the graph's state (frames added since the last solve, for example a
 * foreign packet not yet solved), the frame is associated ungated and counted as skipped; so is the robot's first frame, which has
 * no from pose.  A SLIDE_FRAME_FOREIGN frame is neither tested nor counted.  SLIDE_ERR_INVALID: b NULL, prob outside [0, 1) or not a number, on_reject neither value. */
#define SLIDE_GATE_DROP 0
#define SLIDE_GATE_NEW 1
#define SLIDE_MATCH_GATED (-2)
int slide_backend_set_association_gate(slide_backend_t* b, double prob, int on_reject);
/* {frames gated, frames skipped, candidates tested, candidates rejected} since the back-end was created, counted while the gate is on */
int slide_backend_gate_stats(slide_backend_t* b, int64_t out4[4]);

/* ------------------------------------------------------------------------------------------------
 * S4 — inter-robot map-to-map association
 * ---------------------------------------------------------------------------------------------- */
/* SlideMatch parameters: PlaceRecognition::ParamInit (src/core/place_recognition.cpp:24-78). */
typedef struct slide_place_params_t {
  double dilation_factor;            /* 1.2 */
  double search_xy_step_size;        /* 0.5 */
  double match_yaw_half_range;       /* rad (180 deg) */
  double search_yaw_step_size;       /* rad (2 deg) */
  double match_threshold_position;   /* 0.5 */
  double match_threshold_dimension;  /* 1.0 */
  int disable_yaw_search;
  int ignore_dimension;
  int min_num_inliers;               /* 5 */
  int use_nonlinear_least_squares;   /* use_lsq, true */
  int min_num_map_objects_to_start;  /* 1 */
  int max_rings;                     /* -1 = all; replaces the wall-clock compute_budget_sec */
} slide_place_params_t;
void slide_place_default_params(slide_place_params_t* p);
/* PlaceRecognition::MatchMaps place_recognition.cpp:98-387 on already-centred maps.
 * ref7 / qry7: rows [label, x, y, z, d1, d2, d3].  best_xyyaw: winning (x, y, yaw); pair_*: matched pairs
 * (caller buffers of nq entries).  Returns the best inlier count (>= 0) or a negative SLIDE_ERR_*. */
int slide_match_maps(const double* ref7, int nr, const double* qry7, int nq, const slide_place_params_t* p,
                     double best_xyyaw[3], int32_t* pair_ref_idx, int32_t* pair_qry_idx, int64_t* n_candidates);
/* The same sweep (the same host path and launches as slide_match_maps), read back whole: cand_xyyaw (3 per candidate) and
 * cand_inliers (1 per candidate) in lattice order (ring, x, y, then yaw), best_index = the candidate the device arg-max chose (the first
 * of the maximum; -1 when the lattice is empty).  n_candidates is always filled; SLIDE_ERR_CAPACITY when it exceeds `capacity`
 * (nothing is launched then) or when the maps exceed the kernels' on-chip image.  A test seam: the product calls slide_match_maps. */
int slide_match_maps_sweep(const double* ref7, int nr, const double* qry7, int nq, const slide_place_params_t* p, double* cand_xyyaw,
                           int32_t* cand_inliers, int64_t capacity, int64_t* n_candidates, int64_t* best_index);
/* PlaceRecognition::findInterLoopClosure :498-538 (centring, sweep, inlier gate, Kabsch refinement).
 * Returns 1 found / 0 not found / negative error.  tf16: 4x4 row-major query->reference. */
int slide_find_inter_loop_closure(const double* ref7, int nr, const double* qry7, int nq, const slide_place_params_t* p,
                                  double tf16[16], int* inliers, double xyzyaw[4]);
/* The SlideMatch branch of SLOAMNode::interLoopClosureThread_ (sloamNode.cpp:600-694: one findInterLoopClosure,
 * place_recognition.cpp:498-538, per robot without a loopClosureTf; 28 pairs in a central job over eight robots, 7 with one shared
 * reference map on a host robot) as ONE call.  Map i = rows [map_off[i], map_off[i + 1]) of maps7; pair k = (reference map
 * pairs[2 k], query map pairs[2 k + 1]) — the layout of slide_find_inter_loop_closures_clipper.  Every map is centred once and every
 * distinct reference map bucketed once however many pairs name it; all tables go up in one buffer, k_place_sweep_seg sweeps the
 * lattices of all pairs in one launch (workgroups shared out by candidates x distance tests) keeping only a running best per wave,
 * k_place_best_seg reduces per pair, and ONE read-back fetches the winners: one allocation, one upload, two launches and one blocking
 * read-back per call whatever n_pairs is, and no buffer per candidate.  Pair k is evaluated by itself: found[k], inliers[k],
 * xyzyaw4n + 4 k and tf16n + 16 k are bit for bit what slide_find_inter_loop_closure returns and writes for that pair alone, whatever
 * else is in the list, wherever the pair stands in it and however the workgroups are shared out; a pair that is not found has the
 * identity in its tf16 and zeros in its xyzyaw.  n_candidates[k]: the pair's lattice size; best_index[k]: the winning candidate in
 * lattice order (ring, x, y, then yaw), the first of the maximum, -1 when the pair has no lattice or did not run.  best_index,
 * n_candidates, xyzyaw4n and status may be NULL.  The environment variable SLIDE_PLACE_PLAIN is ignored here: the plain kernel
 * exists for comparison with the single call only.
 * Refused as a whole on the host, before the device is touched and with nothing written (SLIDE_ERR_INVALID): n_pairs < 0, n_maps < 0,
 * a NULL that is needed (pairs, map_off, tf16n, inliers, found; maps7 when a map has rows), a negative or decreasing map_off, a pair
 * naming a map outside [0, n_maps).  n_pairs == 0: SLIDE_OK without a device.  Otherwise SLIDE_OK (SLIDE_ERR_HIP: no usable device)
 * and a pair's own outcome in status[k]: a pair stopped by min_num_map_objects_to_start, by an empty map or by an empty lattice has
 * found[k] = 0 and status 0 (the first two never reach the device; an empty lattice leaves inliers[k] = -10000 as the single call
 * does); a pair whose bucketed LDS image exceeds the single call's 150 KiB rule has SLIDE_ERR_CAPACITY, found[k] = 0 and
 * inliers[k] = 0, and its neighbours are unaffected. */
int slide_find_inter_loop_closures(const double* maps7, const int32_t* map_off, int n_maps, const int32_t* pairs, int n_pairs,
                                   const slide_place_params_t* p, double* tf16n, int32_t* inliers, double* xyzyaw4n, int32_t* found,
                                   int64_t* best_index, int64_t* n_candidates, int32_t* status);

/* PlaceRecognition::findIntraLoopClosure :389-496 (same-robot loop closure: the object detections around the query key pose against
 * the submap around an older candidate key pose).  meas7: detections in the query pose's LOCAL frame, submap7: map objects in the
 * map frame (rows [label, x, y, z, d1, d2, d3]).  The detections go into the map frame with the (drifted) query pose, then
 * findTransformation runs with inter_loop_closure == false (:801-816): no centring, the search window is the three intra half
 * ranges (match_{x,y,yaw}_half_range_intra, defaults 5 m / 5 m / 10 deg :53-63; yaw in radians here).  tf16 (row-major 4x4) =
 * candidate^-1 * query * [Rz(yaw) | (x, y, 0)] = tfFromQuery2Candidate.  Returns 1 found / 0 not found (fewer than 4 detections,
 * an empty input, too few inliers) / negative error. */
int slide_find_intra_loop_closure(const double* meas7, int nm, const double* submap7, int ns, const double query_pose7[7],
                                  const double candidate_pose7[7], const slide_place_params_t* p, double x_half_range_intra,
                                  double y_half_range_intra, double yaw_half_range_intra, double tf16[16], int* inliers,
                                  double xyzyaw[4]);
/* getkeyPoseSubmap of the three map managers (cylinderMapManager.cpp:186-211, cubeMapManager.cpp:77-101,
 * ellipsoidMapManager.cpp:82-107) followed by SLOAMNode::prepareLCInput (sloamNode.cpp:544-576), for n_poses key poses at once, on the
 * device: the submap the intra matcher needs around each candidate key pose.  Map tables: cylinders (root, ray — not normalised —,
 * radius, label), cubes and ellipsoids (centre, scale, label).  pose_xyz3n: 3 doubles per pose.  The rule is the reference's: the pose
 * position goes through pcl's PointT, i.e. float32, p = (float)pose.translation(); a model is kept iff model.distance(p) <=
 * submap_radius (inclusive) and |model_z - pose_z| < max_dz (strict) with the DOUBLE pose z.  distance: |centre - p| for cubes and
 * ellipsoids (cube.cpp:26-29, ellipsoid.cpp:28-31); for cylinders the distance from p to the axis through root along ray, minus radius
 * (cylinder.cpp:226-234), and model_z = root z.  max_dz: the reference hard-codes 1.5 (and says so in a TODO); pass 1.5 for its
 * behaviour.  Rows of pose k: rows7 [sub_off[k], sub_off[k + 1]), kept cylinders in map order, then cubes, then ellipsoids; cylinder
 * rows [label, root, radius, 0, 0], cube / ellipsoid rows [label, centre, scale].  src_idx (may be NULL): the row's index in the
 * concatenated table (cylinders, cubes, ellipsoids).  Capacity protocol of slide_match_maps_sweep: *n_rows and sub_off (n_poses + 1)
 * are always filled; SLIDE_ERR_CAPACITY when *n_rows > capacity, and no row is written then.  k_keypose_submap counts per (pose,
 * 256-object chunk) with a 64-lane ballot per wave, k_seg_scan turns the counts into offsets, the emit pass repeats the test and
 * writes each kept row at its offset plus its rank inside the wave: a stable compaction without atomics.  The tables go up once;
 * three launches and two blocking read-backs (the totals, then the rows) per call whatever n_poses is.  SLIDE_ERR_INVALID: a negative
 * count or capacity, a NULL that is needed. */
int slide_keypose_submaps(const double* cyl_root3, const double* cyl_ray3, const double* cyl_radius, const int32_t* cyl_label, int n_cyl,
                          const double* cube_xyz3, const double* cube_scale3, const int32_t* cube_label, int n_cube,
                          const double* ell_xyz3, const double* ell_scale3, const int32_t* ell_label, int n_ell,
                          const double* pose_xyz3n, int n_poses, double submap_radius, double max_dz,
                          int32_t* sub_off /* n_poses + 1 */, double* rows7, int32_t* src_idx, int64_t capacity, int64_t* n_rows);
/* PlaceRecognition::findIntraLoopClosure place_recognition.cpp:389-496 for a LIST of candidate key poses — the attempt of
 * SLOAMNode::intraLoopClosureThread_ (sloamNode.cpp:355-486) over every candidate instead of the one getLoopCandidateIdx returns — as
 * ONE call.  meas7: one set of detections in the query pose's local frame, moved into the map frame once; candidate k: submap rows
 * [sub_off[k], sub_off[k + 1]) of submaps7 with pose candidate_pose7n + 7 k; all candidates share the one intra lattice.  The host path
 * and the launches are those of slide_find_inter_loop_closures (one allocation, one upload, k_place_sweep_seg + k_place_best_seg, one
 * read-back), each submap bucketed once and the query re-bucketed against each submap's labels.  Candidate k is evaluated by itself:
 * found[k], inliers[k], xyzyaw4n + 4 k and tf16n + 16 k are bit for bit what slide_find_intra_loop_closure returns and writes for that
 * candidate alone, whatever else is in the list and wherever it stands in it; a candidate that is not found has the identity in its
 * tf16 and zeros in its xyzyaw.  best_index / n_candidates as in the inter list; they, xyzyaw4n and status may be NULL.
 * nm == 0 or nm < 4 (:396-405): every candidate found = 0, inliers = 0, status 0, no device touched.  An empty lattice:
 * inliers[k] = -10000 as the single call leaves it.  An empty submap: found = 0, status 0, never reaches the device.  A submap whose
 * bucketed image with these detections exceeds the single call's 150 KiB rule: status[k] = SLIDE_ERR_CAPACITY, found = 0, inliers = 0,
 * neighbours unaffected.  Refused as a whole (SLIDE_ERR_INVALID) before the device is touched and with nothing written: negative
 * counts, a NULL that is needed (sub_off, candidate_pose7n, query_pose7, tf16n, inliers, found; meas7 when nm > 0; submaps7 when a
 * submap has rows), a negative or decreasing sub_off.  n_cand == 0: SLIDE_OK without a device. */
int slide_find_intra_loop_closures(const double* meas7, int nm, const double query_pose7[7], const double* submaps7, const int32_t* sub_off,
                                   int n_cand, const double* candidate_pose7n, const slide_place_params_t* p, double x_half_range_intra,
                                   double y_half_range_intra, double yaw_half_range_intra, double* tf16n, int32_t* inliers,
                                   double* xyzyaw4n, int32_t* found, int64_t* best_index, int64_t* n_candidates, int32_t* status);
/* One attempt of SLOAMNode::intraLoopClosureThread_ (sloamNode.cpp:355-486: getkeyPoseSubmap x 3, prepareLCInput :544-576,
 * findIntraLoopClosure) over n_cand candidate key poses in one call: slide_keypose_submaps around the candidates' positions (the first
 * three entries of each candidate_pose7n row), then slide_find_intra_loop_closures on what it produced.  Every output is bit for bit
 * that of the two calls made one after the other; submap_sizes[k] (n_cand, needed) = the rows of candidate k's submap. */
int slide_intra_loop_closure_attempt(const double* cyl_root3, const double* cyl_ray3, const double* cyl_radius, const int32_t* cyl_label, int n_cyl,
                                     const double* cube_xyz3, const double* cube_scale3, const int32_t* cube_label, int n_cube,
                                     const double* ell_xyz3, const double* ell_scale3, const int32_t* ell_label, int n_ell, const double* meas7,
                                     int nm, const double query_pose7[7], const double* candidate_pose7n, int n_cand, double submap_radius,
                                     double max_dz, const slide_place_params_t* p, double x_half_range_intra, double y_half_range_intra,
                                     double yaw_half_range_intra, double* tf16n, int32_t* inliers, double* xyzyaw4n, int32_t* found,
                                     int64_t* best_index, int64_t* n_candidates, int32_t* status, int32_t* submap_sizes);

/* CLIPPER pairwise-consistency affinity (clipper_semantic_object/src/clipper.cpp:21-65 with the
 * EuclideanDistance invariant src/invariants/euclidean_distance.cpp:13-31).  D1: n1 points of `dim`
 * doubles (point-major), A: m x 2 association list.  M_out: m x m row-major, upper triangle filled. */
int slide_clipper_affinity(const double* D1, int n1, const double* D2, int n2, int dim, const int32_t* A, int m,
                           double sigma, double epsilon, double mindist, double affinityeps, double* M_out);

/* CLIPPER solver parameters: clipper.h:27-60 (solver) and invariants/euclidean_distance.h:24-29 (sigma, epsilon, mindist). */
typedef struct {
  double tol_u, tol_F;       /* 1e-8, 1e-9 */
  int maxiniters, maxoliters; /* 200, 1000 */
  double beta;               /* 0.25 */
  int maxlsiters;            /* 99 */
  double eps;                /* 1e-9 */
  double affinityeps;        /* 1e-4 */
  int rescale_u0;            /* 1 */
  double sigma, epsilon, mindist; /* 0.01, 0.06, 0 */
} slide_clipper_params_t;
void slide_clipper_default_params(slide_clipper_params_t* p);
/* CLIPPER::findDenseClique clipper.cpp:172-323 with DSD_HEU rounding (the only mode sloam uses).  M_upper: n x n row-major,
 * upper triangle filled (slide_clipper_affinity's output).  u0: n start weights; NULL draws them from a fixed-seed
 * generator (the reference uses a std::random_device-seeded mt19937, utils.cpp:22-29, i.e. is not reproducible).
 * nodes_out: caller buffer of n entries (selected associations, largest weight first); u_out (n) / score may be NULL.
 * The whole solve runs on the device: M as CSR (like the reference's sparse M / C, clipper.cpp:55-64), every product, reduction,
 * projection, line-search and stopping decision in one persistent workgroup — no host round trip inside the iteration. */
int slide_clipper_dense_clique(const double* M_upper, int n, const double* u0, const slide_clipper_params_t* p,
                               int32_t* nodes_out, int* n_nodes, double* u_out, double* score);
/* scorePairwiseConsistency clipper.cpp:21-65 ending in M_ = M.sparseView(): the SYMMETRIC matrix without its diagonal as CSR,
 * columns ascending (the matrix the solver multiplies with).  rowptr_out: m + 1 ints.  Two-call protocol: *nnz is always set;
 * cap < *nnz -> SLIDE_ERR_CAPACITY, col_out / val_out untouched (rowptr_out still filled).  Built on the device row by row
 * (k_affinity_csr: count, host prefix sum, emit) without the dense m x m form; the values are those of slide_clipper_affinity bit for
 * bit (one shared scoring function), the same on every run.  More than 2^31 - 1 non-zeros: SLIDE_ERR_CAPACITY; an association outside
 * D1 / D2: SLIDE_ERR_INVALID. */
int slide_clipper_affinity_csr(const double* D1, int n1, const double* D2, int n2, int dim, const int32_t* A, int m,
                               double sigma, double epsilon, double mindist, double affinityeps,
                               int32_t* rowptr_out, int32_t* col_out, double* val_out, long long cap, long long* nnz);
/* findDenseClique clipper.cpp:172-323 from that CSR (rowptr: n + 1 ints, col / val: rowptr[n] entries); otherwise as
 * slide_clipper_dense_clique, and the same bits for the same matrix.  The CSR is checked on the host before the device is touched:
 * rowptr[0] == 0 and non-decreasing, columns inside [0, n), strictly ascending within a row, none on the diagonal, every (i, j, v)
 * with its (j, i, v); a violation is SLIDE_ERR_INVALID with the row in slide_last_error(). */
int slide_clipper_dense_clique_csr(const int32_t* rowptr, const int32_t* col, const double* val, int n, const double* u0,
                                   const slide_clipper_params_t* p, int32_t* nodes_out, int* n_nodes, double* u_out, double* score);
/* scorePairwiseConsistency + solve + getSelectedAssociations (clipper.cpp:21-65, 172-323, 67-85) in one call: nothing of size m^2
 * exists anywhere, on the host or the device.  sigma / epsilon / mindist / affinityeps from p.  nodes_out: m entries. */
int slide_clipper_match(const double* D1, int n1, const double* D2, int n2, int dim, const int32_t* A, int m, const double* u0,
                        const slide_clipper_params_t* p, int32_t* nodes_out, int* n_nodes, double* u_out, double* score);
/* ---- Selecting the mutually consistent subset of a list of loop closures ------------------------------------------------------
 * Pairwise-consistency maximisation (PCM; Mangelson, Dominic, Eustice, Vasudevan, ICRA 2018) on the clique solver above.  It has NO
 * counterpart in the reference: there every closure is accepted on an inlier count alone (place_recognition.cpp:845-856), the first
 * that passes goes straight into the graph (sloamNode.cpp:448-476) with a noise of 0.01 x the odometry sigmas (graphWrapper.cpp:55),
 * and one false closure at that weight bends the whole trajectory.
 * A closure k: from_robot, from_idx, to_robot, to_idx, rel7 (the project's 7-double pose layout: x y z, qx qy qz qw) and sigma6, its
 * own six sigmas.  Its meaning is exactly that of slide_graph_add_loop_closure, a Between factor on (X(from), X(to)): rel measures
 * X_from^-1 X_to.  With the current estimates F_k = X(from_k), T_k = X(to_k), two closures i < j of one ordered robot pair close a
 * cycle whose error is  e_ij = se3_log(z_i T_i^-1 T_j z_j^-1 F_j^-1 F_i)  in the tangent order [rot(3), trans(3)] — the order of
 * sigma6, of odom_sigma6 and of every noise vector of slide_params_t.  Only within-robot relative poses (T_i^-1 T_j, F_j^-1 F_i)
 * appear, so the formula holds when the two robots' world frames are unrelated.  Per component
 * s2[c] = sigma6_i[c]^2 + sigma6_j[c]^2 + (|from_idx_i - from_idx_j| + |to_idx_i - to_idx_j|) odom_sigma6[c]^2 (the odometry legs of
 * the cycle), d = sqrt(sum_c e[c]^2 / s2[c]), and the score is d < gate ? exp(-0.5 d^2 / sigma^2) : 0, kept if > affinityeps.  e_ij
 * is not symmetric in (i, j): every entry is evaluated with the smaller closure index as i, so the matrix is symmetric bit for bit.
 * gate = sqrt(16.81) = 4.1, the 0.99 quantile of chi-square with 6 degrees of freedom; sigma = gate / 2, a convention (the score at the
 * gate is exp(-2)); affinityeps = 1e-4, CLIPPER's default; min_set = 1: a group whose selected set is smaller keeps nothing, and with 1
 * a lone closure is kept, the reference's behaviour.  odom_sigma6: per odometry step; slide_graph_select_closures takes it from the
 * graph's noise_model_odom_vec instead. */
typedef struct {
  double gate;            /* 4.1 */
  double sigma;           /* gate / 2 */
  double affinityeps;     /* 1e-4 */
  double odom_sigma6[6];  /* 0.1 (slide_params_t::noise_model_odom_vec's default) */
  int min_set;            /* 1 */
} slide_closure_params_t;
void slide_closure_default_params(slide_closure_params_t* p);
/* Host bookkeeping, no kernel: closures of different unordered robot pairs are different problems ("groups").  Every closure with
 * from_robot > to_robot is canonicalised by swapping its ends and inverting rel (flipped[k] = 1); same-robot closures are not
 * reordered, either orientation closes a valid cycle.  Groups are numbered by ascending (from_robot, to_robot) and filled stably:
 * group[k], and order[k] = the row of closure k in the list of all groups' closures one group after the other.  Every output but
 * n_groups may be NULL. */
int slide_closure_canonicalize(int L, const int32_t* from_robot, const uint64_t* from_idx, const int32_t* to_robot, const uint64_t* to_idx,
                               const double* rel7, int32_t* from_robot_out, uint64_t* from_idx_out, int32_t* to_robot_out,
                               uint64_t* to_idx_out, double* rel7_out, int32_t* flipped, int32_t* group, int32_t* order, int* n_groups);
/* The consistency matrix of ONE group (the caller's closures as they are, nothing canonicalised), poses given per closure
 * (from_pose7 / to_pose7: L x 7): the symmetric CSR without its diagonal, columns ascending, built on the device (k_closure_prepare,
 * k_closure_csr_seg count, k_seg_scan, emit).  The two-call protocol of slide_clipper_affinity_csr: *nnz is always set, cap < *nnz
 * returns SLIDE_ERR_CAPACITY with col_out / val_out untouched (rowptr_out, L + 1 ints, still filled). */
int slide_closure_consistency_csr(const double* from_pose7, const double* to_pose7, const double* rel7, const double* sigma6,
                                  const uint64_t* from_idx, const uint64_t* to_idx, int L, const slide_closure_params_t* p,
                                  int32_t* rowptr_out, int32_t* col_out, double* val_out, long long cap, long long* nnz);
/* A list of closures over any robot pairs, poses given per closure: canonicalise, group, ONE k_closure_prepare, k_closure_csr_seg
 * count, k_seg_scan, emit, then ONE k_clq_solve_b launch for every group below 1024 closures; larger groups go one after another
 * through the single problem's multi-workgroup route on their slice.  DSD_HEU rounding.  A group of one closure never reaches the
 * device (selected 1, score 1, u 1); the single-group case is this path with one group.  A group's bits do not depend on what else is
 * in the list or where it stands.  Blocking read-backs: 2 per call whatever the number of groups (the groups' non-zero counts; the
 * solves' results in one buffer), + 2 for every group of 1024 or more, + 3 when the CSR is asked for.
 * Per closure: keep[k] (0 / 1), group[k], status[k] (SLIDE_OK; SLIDE_ERR_CAPACITY: its group's matrix exceeds 2^31 - 1 non-zeros, keep
 * 0) — group / status may be NULL.  Per group g (arrays of L entries, may be NULL): n_selected[g], score[g]; *n_groups.
 * cp: the solver's parameters (NULL: slide_clipper_default_params; its sigma / epsilon / mindist / affinityeps are not read).
 * u0 (NULL, or one pointer per closure group in group order, each NULL or that group's start weights in row order): NULL draws the
 * fixed-seed start per group.  u_out (NULL or L): the solved weight of each closure.  csr_*: NULL, or the matrices of all groups one
 * after the other for inspection — rowcnt_out[k] the non-zeros of closure k's row, col / val (columns counted within the group) copied
 * when *csr_nnz <= csr_cap.
 * Whole-call refusals (SLIDE_ERR_INVALID, decided on the host before the device is touched, nothing written): a needed pointer NULL,
 * L < 0, a robot outside [0, SLIDE_MAX_ROBOTS), non-finite input, a zero quaternion, a sigma <= 0, gate / sigma <= 0, affinityeps < 0
 * or non-finite, min_set < 0.  L == 0: SLIDE_OK, *n_groups = 0. */
int slide_select_consistent_closures(int L, const int32_t* from_robot, const uint64_t* from_idx, const int32_t* to_robot,
                                     const uint64_t* to_idx, const double* rel7, const double* sigma6, const double* from_pose7,
                                     const double* to_pose7, const slide_closure_params_t* p, const slide_clipper_params_t* cp,
                                     const double* const* u0, int32_t* keep, int32_t* group, int32_t* status, int32_t* n_selected,
                                     double* score, int* n_groups, double* u_out, int32_t* rowcnt_out, int32_t* col_out, double* val_out,
                                     long long csr_cap, long long* csr_nnz);
/* The same with the endpoints resolved against the graph's current estimate (read from the device-resident estimate by slot, nothing
 * is downloaded) and odom_sigma6 = the graph's noise_model_odom_vec (p's own is not read): call it after a solve and before the
 * closures are added.  A closure naming a pose the graph does not hold (or has not taken in by a solve yet): status[k] =
 * SLIDE_MISSING, keep 0, group -1; the others proceed.  It reads the graph and changes nothing in it. */
int slide_graph_select_closures(slide_graph_t* g, int L, const int32_t* from_robot, const uint64_t* from_idx, const int32_t* to_robot,
                                const uint64_t* to_idx, const double* rel7, const double* sigma6, const slide_closure_params_t* p,
                                const slide_clipper_params_t* cp, int32_t* keep, int32_t* group, int32_t* status, int32_t* n_selected,
                                double* score, int* n_groups);
/* ---- One closure against what the graph already knows: the individual-compatibility gate ----------------------------------------
 * slide_graph_select_closures compares closures with each other; it cannot judge a lone closure, and a group of false closures that
 * agree with each other (perceptual aliasing) forms a clique like a true one.  The complement measures a closure's residual against
 * its own noise plus the joint marginal covariance of its two poses under the graph as it stands.  No counterpart in the reference
 * (GTSAM users know the first query as Marginals::jointMarginalCovariance).
 * Both calls use one identity: with S = L L^T the resident factor of the landmark-eliminated pose system and Sigma = S^-1,
 * B^T Sigma B = W^T W where L W = B — a forward substitution only (T launches per sweep, not the 2 T of a solve) and symmetric
 * positive semi-definite by construction.  Single-graph path only (one graph may hold several robots).  Candidates are cut into
 * sweeps of whole candidates of at most SLIDE_INFO_GAIN_SWEEP_COLS columns of B (32 pairs or 64 closures); a sweep is one
 * many-column forward substitution, the candidates' diagonal gram blocks and one read-back, and a candidate's bits do not depend on
 * what else is in the list or where it stands.
 * Whole-call refusals (SLIDE_ERR_INVALID, nothing written): those of slide_graph_get_pose_covariances (sharded or exact-joint mode,
 * before the first solve, after slide_graph_chi2, once anything was merged after the last solve), and — decided on the host before
 * the device is touched — a needed pointer NULL, n or L < 0, a robot outside [0, SLIDE_MAX_ROBOTS), non-finite input, a zero
 * quaternion, a sigma <= 0.  n == 0 / L == 0 on a graph that would be served: SLIDE_OK.  Per candidate, into status[k] (may be NULL)
 * with zeros in its outputs: SLIDE_MISSING for a pose the graph does not hold, SLIDE_ERR_INVALID when both ends are the same pose,
 * SLIDE_ERR_NOT_SPD when I + A Sigma A^T has a pivot that is not positive.  The calls read the graph and change nothing in it.
 *
 * out144n: per pair the 12 x 12 row-major joint marginal [[Saa, Sab], [Sba, Sbb]]: pose a's six coordinates, then pose b's, tangent
 * order [rot, trans] (B = the unit columns of the two poses' rows). */
int slide_graph_get_pose_pair_covariances(slide_graph_t* g, int n, const int32_t* robot_a, const uint64_t* idx_a, const int32_t* robot_b,
                                          const uint64_t* idx_b, double* out144n, int32_t* status);
/* The endpoint arguments, rel7 and sigma6 mean exactly what they mean to slide_graph_select_closures (the same arrays can go to both
 * calls): closure k is the Between factor slide_graph_add_loop_closure(rel7_k, from, to) would add with the sigmas sigma6_k.  r_k (6)
 * is its whitened residual and A_k (6 x 12) its whitened Jacobian, linearised by the solver's own Between text under the graph's
 * pose_chart at the current estimate of the two poses (what slide_graph_get_pose12 returns).  C_k = I + A_k Sigma A_k^T (B = A_k^T) is
 * the innovation covariance in whitened units and d2[k] = r_k^T C_k^-1 r_k: chi-square with 6 degrees of freedom for a true closure
 * that was not added yet.  Compare it with 16.81 (slide_closure_params_t::gate squared); the call itself applies no threshold.
 * C36 (36 per closure, row-major) and r6 (6 per closure) may be NULL. */
int slide_graph_closure_mahalanobis(slide_graph_t* g, int L, const int32_t* from_robot, const uint64_t* from_idx, const int32_t* to_robot,
                                    const uint64_t* to_idx, const double* rel7, const double* sigma6, double* d2, double* C36 /* may be NULL */,
                                    double* r6 /* may be NULL */, int32_t* status /* may be NULL */);
/* ---- One landmark observation against what the graph already knows: the gate's counterpart for observation factors ----------------
 * Most factors of a graph are landmark observations, and the association that produces them tests a Euclidean distance only (0.75 m
 * for ellipsoids, 2 m for cubes and cylinders: sloam.cpp:73-203), whatever the pose's drift and the landmark's own uncertainty.  This
 * is the individual-compatibility (innovation) gate of a candidate match before it becomes a factor: nearest-neighbour association
 * with a chi-square gate.  No counterpart in the reference; GTSAM users would assemble it from
 * Marginals::jointMarginalCovariance({X(i), L(j)}).
 * Candidate k is the factor slide_graph_add_range_bearing / _add_cube / _add_cylinder would add between pose (robot[k], pose_idx[k])
 * and the EXISTING landmark (cls[k], lm_idx[k]) of dimension D = 3 / 9 / 7; it has m = D rows.  meas17[17 k ..] holds the remaining
 * arguments of the class's add call in its order, zero padded: SLIDE_CLS_ELLIPSOID bearing[3], range; SLIDE_CLS_CUBE pose_world7,
 * cube_world7, scale[3]; SLIDE_CLS_CYLINDER pose_world7, root[3], ray[3], radius.  r (m) is its whitened residual and A = [Ap | Al]
 * (m x 6, m x D) its whitened Jacobian, linearised by the solver's own text for the class (analytic for bearing-range, central
 * differences of numdiff_delta for cubes and cylinders) under the graph's pose_chart, with the noise the add call would choose
 * (bearing_range_sigma; noise_model_cube_vec x max(|loc.t|, 0.1); cylinder_sigma) and NO robust weight, whatever
 * slide_graph_set_observation_loss says.  With H the full system as last linearised (reweighted, if a loss is set) and S = L L^T its
 * landmark-eliminated pose system,
 *     C = I + A H^-1 A^T = I + Al H_ll^-1 Al^T + B^T S^-1 B,    B = P_p^T Ap^T - sum_{f in factors(l)} P_{p_f}^T F_f Al^T,
 *     d2[k] = r^T C^-1 r,
 * P_q selecting pose q's six rows and F_f = E_f H_ll^-1 the factor's resident Schur block: the pose-landmark cross block of the
 * marginal is never formed, and B^T S^-1 B = W^T W with L W = B is the forward substitution of the two calls above.  Sigma belongs to
 * the LAST LINEARISATION POINT (the resident factor), r and A to the CURRENT ESTIMATE (what slide_graph_get_pose12 /
 * slide_graph_get_landmark return).  d2 is chi-square with m degrees of freedom for a true match that was not added yet: compare it
 * with the 0.99 quantile, 11.345 (m = 3), 18.475 (m = 7), 21.666 (m = 9); no threshold is applied by the call.  The graph is only
 * read: nothing in it changes.
 * Outputs: dof[k] = 3 / 9 / 7; C81 (81 per candidate) row-major with leading dimension 9, zero outside the m x m block; r9 (9 per
 * candidate).  dof, C81, r9 and status may be NULL.  Candidates are grouped by class and cut into sweeps of at most
 * SLIDE_INFO_GAIN_SWEEP_COLS columns (128 points, 42 cubes, 54 cylinders); a sweep starts its substitution at the block column of the
 * lowest pose it touches (the candidates' poses and their landmarks' first observers), and a candidate's bits do not depend on what
 * else is in the list or where it stands.
 * Whole-call refusals (SLIDE_ERR_INVALID, nothing written, the message names observation_mahalanobis and the reason): decided on the
 * host before the graph or the device is looked at — the graph is NULL, a needed pointer NULL, n < 0, a robot outside
 * [0, SLIDE_MAX_ROBOTS), a class that is none of the three, non-finite input, a zero quaternion, a zero bearing, a range <= 0, a zero
 * ray; then those of slide_graph_get_pose_covariances.  n == 0 on a graph that would be served: SLIDE_OK.  Per candidate, into
 * status[k] with zeros in its outputs: SLIDE_MISSING for a pose or landmark the graph does not hold, SLIDE_ERR_NOT_SPD when C has a
 * pivot that is not positive. */
int slide_graph_observation_mahalanobis(slide_graph_t* g, int n, const int32_t* robot, const uint64_t* pose_idx, const int32_t* cls,
                                        const uint64_t* lm_idx, const double* meas17, double* d2, int32_t* dof /* may be NULL */,
                                        double* C81 /* may be NULL */, double* r9 /* may be NULL */, int32_t* status /* may be NULL */);
/* slide_graph_observation_mahalanobis at a PREDICTED pose: "is this match compatible, before I add it", as an EKF gates at the
 * predicted state.  No counterpart in the reference, whose association accepts a match at poseEstimate = prev * rel on a Euclidean
 * threshold alone (sloam.cpp:73-203), and none in GTSAM short of adding the pose and its factor and taking
 * Marginals::jointMarginalCovariance on the grown graph.
 * Let pose k = (robot, from_idx) be in the graph with estimate X_k, X_n = est7 the predicted pose and rel7 the odometry step whose
 * Between factor slide_graph_add_keypose_between(g, robot, from_idx, ., rel7, est7) would add, with that call's sigmas
 * s = noise_model_odom_vec x max(|t_rel|, noise_floor).  The solver linearises that factor as H_F = -diag(1 / s) Ad,
 * H_T = diag(1 / s), Ad = Ad(X_n^-1 X_k); the new pose touches nothing else, so the marginal of the augmented graph is
 * Sig(n, .) = Ad Sig(k, .), Sig(n, n) = Ad Sig(k, k) Ad^T + diag(s^2); the Between's residual does not enter.  Candidate i is the
 * observation from X_n of the EXISTING landmark (cls[i], lm_idx[i]) that slide_graph_add_range_bearing / _add_cube / _add_cylinder
 * would add; meas17 as for slide_graph_observation_mahalanobis; r and A = [Ap | Al] its whitened residual and Jacobian at
 * (X_n, the landmark's estimate) by the solver's text for the class, no robust weight.  Then
 *     C  = I + Al H_ll^-1 Al^T + Ap diag(s^2) Ap^T + B^T S^-1 B,   B = P_k^T (Ap Ad)^T - sum_{f in factors(l)} P_{p_f}^T F_f Al^T,
 *     d2 = r^T C^-1 r:
 * exactly what slide_graph_observation_mahalanobis would return on the graph extended by the pose and its Between factor, linearised
 * at those values, chi-square with dof = 3 / 9 / 7 for a true match — with no add, no factorisation and no change to the graph.  No
 * threshold is applied.  Outputs, sweeps (128 / 42 / 54 candidates) and status words are that call's; a sweep's walk starts at the
 * block column of min(pose k, the landmarks' first observers); a candidate's bits do not depend on the rest of the list.
 * Whole-call refusals decided before the graph is looked at (SLIDE_ERR_INVALID, nothing written, the message names
 * predicted_observation_mahalanobis): that call's argument checks, rel7 or est7 NULL or non-finite, a zero quaternion, the graph is
 * NULL.  Then SLIDE_MISSING for a from pose the graph does not hold (nothing written), then the refusals of
 * slide_graph_get_pose_covariances.  Per candidate: SLIDE_MISSING (a landmark the graph does not hold), SLIDE_ERR_NOT_SPD. */
int slide_graph_predicted_observation_mahalanobis(slide_graph_t* g, int robot, uint64_t from_idx, const double rel7[7], const double est7[7], int n,
                                                  const int32_t* cls, const uint64_t* lm_idx, const double* meas17, double* d2,
                                                  int32_t* dof /* may be NULL */, double* C81 /* may be NULL */, double* r9 /* may be NULL */,
                                                  int32_t* status /* may be NULL */);
/* The JOINT compatibility of a key frame's landmark matches: Neira and Tardos' joint compatibility test in its greedy sequential form
 * (the sequential compatibility nearest neighbour), on the single graph.  No counterpart in the reference; GTSAM users would stack the
 * hypothesis' factors and take Marginals::jointMarginalCovariance over all their variables.  A frame proposes its matches at once, all
 * from the newest pose, which carries most of each candidate's innovation covariance: the candidates are strongly correlated, and
 * slide_graph_observation_mahalanobis, which tests each alone, accepts sets that no single pose error explains.
 * The call takes n_groups hypotheses; group g is the candidates group_ptr[g] .. group_ptr[g + 1] - 1 in the caller's order, each
 * described exactly as for slide_graph_observation_mahalanobis (robot, pose_idx, cls, lm_idx, meas17; the add call's base noise, no
 * robust weight; the same state rules).  With a group's served candidates stacked, r = [r_1; ..], A = [A_1; ..],
 *     C = I + A H^-1 A^T,     block (i, j) = [i == j] (I + Al_i H_ll^-1 Al_i^T) + W_i^T W_j,     L W = B,
 * B_i the columns of the individual gate: H_ll is block diagonal and a group may not name a landmark twice.
 * The rule, on the device, in the caller's order.  q(k): the prob quantile of chi-square with k degrees of freedom
 * (slide_chi2_quantile, k = 1 .. SLIDE_INFO_GAIN_SWEEP_COLS).  The accepted set S starts empty; for candidate i of m_i = 3 / 9 / 7 rows
 *     d2_single[i] = r_i^T C_ii^-1 r_i,
 *     d2_joint[i]  = the stacked d2 of S + {i}, dof_joint[i] its dimension, by bordering the Cholesky factor of C_SS:
 *                    X = C_iS L_S^-T,  D = C_ii - X X^T = G G^T,  y_i = G^-1 (r_i - X y_S),  d2_joint = d2_S + y_i^T y_i,
 *     accepted[i]  = d2_single[i] <= q(m_i) and d2_joint[i] <= q(dof_joint[i]); the factor and y grow by the block then and stay as they
 *                    were otherwise.
 * prob == 0: evaluate only — every served candidate is accepted, d2_joint is the prefix sequence of the stacked test and group_d2 the
 * joint compatibility of the whole hypothesis.  Per group: group_d2 / group_dof / group_count, the stacked d2, the rows and the number
 * of the accepted set.  Groups are packed whole, in the caller's order, into sweeps of at most SLIDE_INFO_GAIN_SWEEP_COLS columns; a
 * group's bits do not depend on what else is in the call or where it stands.  The graph is only read.
 * Whole-call refusals (SLIDE_ERR_INVALID, nothing written, the message names observation_joint_compatibility and the reason), decided
 * on the host before the graph or the device is looked at: n_groups < 0, a needed pointer NULL (every output is needed), a group_ptr
 * that does not start at 0 or decreases, prob neither 0 nor inside (0, 1) (not a number among them), the per-candidate checks of
 * slide_graph_observation_mahalanobis, the graph is NULL; then those of slide_graph_get_pose_covariances.  Per candidate, status[i]
 * with zeros in its outputs: SLIDE_MISSING as the individual gate decides it — the candidate is skipped and the rest of its group
 * served as if it were absent; SLIDE_ERR_NOT_SPD when a pivot of D or C_ii is not positive — the candidate is rejected and the chain
 * goes on.  Per group, group_status[g] with zeros everywhere in the group, its neighbours served: SLIDE_ERR_INVALID when two served
 * candidates name one landmark, SLIDE_ERR_CAPACITY when the served rows exceed SLIDE_INFO_GAIN_SWEEP_COLS (128 points). */
int slide_graph_observation_joint_compatibility(slide_graph_t* g, int n_groups, const int32_t* group_ptr, const int32_t* robot,
                                                const uint64_t* pose_idx, const int32_t* cls, const uint64_t* lm_idx, const double* meas17,
                                                double prob, int32_t* accepted, double* d2_single, double* d2_joint, int32_t* dof_joint,
                                                int32_t* status, double* group_d2, int32_t* group_dof, int32_t* group_count,
                                                int32_t* group_status);
/* The prob quantile of chi-square with dof degrees of freedom, q with P(dof / 2, q / 2) = prob: Newton on the regularised incomplete
 * gamma function (its series for x < a + 1, its continued fraction elsewhere).  Host code, no device is needed; no counterpart in the
 * reference (boost::math::quantile(chi_squared(dof), prob) is the usual spelling).  SLIDE_ERR_INVALID for prob outside (0, 1) or not a
 * number, dof < 1, q NULL. */
int slide_chi2_quantile(double prob, int dof, double* q);
/* Duplicate landmarks: the Mahalanobis test of a list of landmark PAIRS against the graph as it stands.  The gates above judge a loop
 * closure, an observation and a frame of observations; none of them judges the commonest association failure, one object mapped
 * twice: an object that lost its match and was initialised again under a new id.  The reference has no answer (its Euclidean
 * nearest-neighbour gate decides once, per frame, and never looks back); EKF-SLAM and GTSAM users write this query by hand from
 * Marginals::jointMarginalCovariance({L(i), L(j)}).  A Euclidean distance cannot decide it: a true duplicate re-sighted after 35 poses
 * of drift sits as far from its twin as a distinct object seen from the same poses.
 * Pair k names two EXISTING landmarks (cls[k], idx_a[k]) and (cls[k], idx_b[k]) of one class: SLIDE_CLS_ELLIPSOID (D = 3) or
 * SLIDE_CLS_CYLINDER (D = 7), which both retract additively, so the difference is exact.  Cubes are refused, on the host: a box pose is
 * ambiguous under its own symmetries and a tangent difference means nothing without handling them.  The hypothesis is "a and b are one
 * object, up to a model noise sigma[D]" (sigma_point3 / sigma_cylinder7, per call and class, every entry > 0; a class no pair names may
 * pass NULL): two fits of one object from different views differ by centimetres.  In the tangent order of
 * slide_graph_get_landmark_covariances (point xyz; cylinder [ray, root, radius]):
 *     d     = est_b - est_a                       at the CURRENT ESTIMATE (what slide_graph_get_landmark returns)
 *     r     = d / sigma
 *     Sig_d = Sig_aa + Sig_bb - Sig_ab - Sig_ba   at the LAST LINEARISATION POINT (the resident factor)
 *     C     = I + diag(1 / sigma) Sig_d diag(1 / sigma)
 *     d2[k] = r^T C^-1 r                          chi-square with D degrees of freedom for one object
 * No threshold is applied by the call: compare d2 with slide_chi2_quantile(0.99, D), 11.345 or 18.475.  The graph is only read.
 * With the landmarks eliminated H_ll is block diagonal; with Al = -I / sigma on a and +I / sigma on b,
 *     C = I + Al_a Hinv_a Al_a^T + Al_b Hinv_b Al_b^T + B^T S^-1 B,
 *     B = - sum_{f in factors(a)} P_{p_f}^T F_f Al_a^T - sum_{f in factors(b)} P_{p_f}^T F_f Al_b^T,
 * and the landmark-landmark cross block is never formed.  The host chooses one of two routes per pair, from the structure alone, so a
 * pair's bits do not depend on the rest of the list; route[k] says which.  Route 0, direct: every pose that observes a or b lies inside
 * one reach of the tile profile (always, on a dense profile), so every Sigma(p_f, p_g) needed is an entry of the selected inverse that
 * slide_graph_get_pose_covariances computes once per factorisation; one wavefront per pair sums the four blocks, scales, factors C and
 * solves — no substitution at all.  This is the common case, a landmark initialised again a few frames after it was lost.  Route 1,
 * substitution: every other pair (a revisit across the profile) goes through the forward substitution of the gates above, B^T S^-1 B =
 * W^T W with L W = B, SLIDE_INFO_GAIN_SWEEP_COLS / D pairs per sweep (128 points, 54 cylinders), the walk starting at the block column
 * of the sweep's lowest observer.  SLIDE_LM_PAIR_SUBSTITUTE=1 in the environment sends every pair down route 1 (a measurement and test
 * aid).
 * Outputs follow slide_graph_observation_mahalanobis: dof[k] = D; C81 row-major with leading dimension 9, zero outside the D x D block,
 * symmetric bit for bit; r9; route[k] 0 or 1.  dof, C81, r9, route and status may be NULL.
 * Whole-call refusals (SLIDE_ERR_INVALID, nothing written, the message names landmark_pair_mahalanobis and the reason), decided on the
 * host before the graph or the device is looked at: n < 0, a needed pointer NULL, a class that is neither of the two, a sigma that is
 * non-finite or <= 0, the graph is NULL; then those of slide_graph_get_pose_covariances.  n == 0 on a graph that would be served:
 * SLIDE_OK.  Per pair, into status[k] with zeros in its outputs: SLIDE_MISSING for a landmark the graph does not hold or one without a
 * factor, SLIDE_ERR_INVALID when a and b are the same landmark, SLIDE_ERR_NOT_SPD when a pivot of C is not positive. */
int slide_graph_landmark_pair_mahalanobis(slide_graph_t* g, int n, const int32_t* cls, const uint64_t* idx_a, const uint64_t* idx_b,
                                          const double* sigma_point3, const double* sigma_cylinder7, double* d2,
                                          int32_t* dof /* may be NULL */, double* C81 /* may be NULL */, double* r9 /* may be NULL */,
                                          int32_t* route /* may be NULL */, int32_t* status /* may be NULL */);
/* Marginals::jointMarginalCovariance({L(a), L(b)}) for n landmark pairs of one class each, the counterpart of
 * slide_graph_get_pose_pair_covariances.  All three classes are served: a covariance at the linearisation point has no symmetry
 * problem.  out324n[324 k ..] = [[Saa, Sab], [Sba, Sbb]], the 2 D x 2 D block (D = 3 / 9 / 7) row-major with leading dimension 18, zero
 * padded, in the tangent order of slide_graph_get_landmark_covariances.  Routes as above: the four blocks off the selected inverse, or
 * 2 D unit columns through the forward substitution.  Route choice, refusals (the message names get_landmark_pair_covariances; any
 * landmark class is accepted and there is no sigma) and the status words SLIDE_MISSING and SLIDE_ERR_INVALID are those of the test;
 * route and status may be NULL.  It lets a caller rebuild Sig_d, or test another hypothesis than the difference. */
int slide_graph_get_landmark_pair_covariances(slide_graph_t* g, int n, const int32_t* cls, const uint64_t* idx_a, const uint64_t* idx_b,
                                              double* out324n, int32_t* route /* may be NULL */, int32_t* status /* may be NULL */);
/* Finding the candidates: a deterministic fixed-radius pair search on the device.  Every i < j of the n points xyz (3 doubles each)
 * with |x_i - x_j| <= radius, the distance in double, and label[i] == label[j] where label is given; sorted by (i, j).  *n_pairs is
 * always the total.  Above cap: SLIDE_ERR_CAPACITY, and nothing but n_pairs is written.  SLIDE_ERR_INVALID (nothing written, the
 * message names pairs_within): n < 0, cap < 0, a needed pointer NULL (the outputs are needed when cap > 0), a radius that is non-finite
 * or <= 0.  Count, scan, emit: ballot compaction orders the output, no atomic does.  No counterpart in the reference. */
int slide_pairs_within(const double* xyz, const int32_t* label /* may be NULL */, int n, double radius, int64_t cap, int32_t* out_i,
                       int32_t* out_j, double* out_dist, int64_t* n_pairs);
/* The same search over the graph's device-resident landmark estimates of one class: the anchor is the point's xyz, the cube's
 * translation or the cylinder's root.  sel_idx: the n_sel landmark keys to search among, or NULL: every landmark of the class, in the
 * graph's order (n_sel is not read then).  sel_label (may be NULL): one label per selected landmark.  Pairs come back as landmark
 * keys idx_a / idx_b with their distance, sorted by their positions in the selection.  A selected key the graph does not hold:
 * SLIDE_MISSING for the call.  Refusals as slide_pairs_within (the message names landmark_pairs_within), and a class that is not a
 * landmark class; then the graph is NULL. */
int slide_graph_landmark_pairs_within(slide_graph_t* g, int cls, double radius, int n_sel, const uint64_t* sel_idx /* may be NULL */,
                                      const int32_t* sel_label /* may be NULL */, int64_t cap, uint64_t* idx_a, uint64_t* idx_b, double* dist,
                                      int64_t* n_pairs);
/* Acting on what the two calls above find: MERGE duplicate landmarks into the graph — one variable, fused estimate.  No counterpart
 * in the reference, whose graph is append-only; GTSAM users remove the dropped landmark's factors (removeFactorIndices) and add them
 * again rekeyed, EKF-SLAM calls it landmark fusion.  Single-graph path only.
 * Pair k says: landmark (cls[k], drop_idx[k]) and landmark (cls[k], keep_idx[k]) are one object; keep the latter.  All three classes.
 * The call judges nothing: slide_graph_landmark_pair_mahalanobis is the caller's evidence, or the caller has its own.  Pairs are
 * applied in list order, and a key dropped by an earlier pair — of this call or an earlier one — stands for its survivor at both
 * ends, so chains and triangles such as (a, b), (a, c), (b, c) are legal.  After the call
 *  - every factor of the dropped landmark is a factor of the survivor; its measurement, sigmas, robust-loss arrays and position in
 *    insertion order are unchanged.  A pose that observed both now holds two factors on one landmark;
 *  - the dropped key is an ALIAS of the survivor: slide_graph_get_landmark returns the survivor's estimate for it, a later
 *    slide_graph_add_range_bearing / _add_cube / _add_cylinder (exists = 1) on it adds to the survivor, slide_graph_add_point_landmark
 *    or exists = 0 on it is refused by the next update as "value inserted twice", and slide_graph_landmark_alias names the survivor.
 *    A SlideBackend's association may thus go on matching the old id (its graph: slide_backend_graph);
 *  - the dropped landmark's slot stays in the arrays as a tombstone without key and factors: slide_graph_stats' n_lm goes down by
 *    one per drop, and slide_graph_marginal_traces, the information gain's landmark drop, slide_graph_landmark_pairs_within
 *    (sel_idx NULL) and slide_graph_get_observation_weights (a moved factor's row names the survivor's own key) skip or resolve it.
 * into[k]: the key pair k's landmarks resolve to when the call returns.  moved[k]: factors re-pointed by pair k; 0, with status
 * SLIDE_OK, when both ends were one landmark already.  status[k]: SLIDE_MISSING when either key is absent (into[k] = 0),
 * SLIDE_ERR_INVALID when keep_idx[k] == drop_idx[k], SLIDE_ERR_NOT_SPD when the fusion of its cluster failed (the structure is merged
 * all the same and the survivor keeps its own estimate); such a pair changes nothing.  into, moved and status may be NULL.
 * fuse = 0: the survivor keeps its estimate.  fuse = 1, for points and cylinders (both retract additively; a cube always keeps the
 * survivor's estimate, a box pose being ambiguous under its symmetries): per survivor that gained members in this call, in the
 * tangent order of slide_graph_get_landmark_covariances,
 *     x = (sum_i H_i)^-1 sum_i H_i est_i,
 * i over {survivor, members} in ascending internal id, H_i the member's own H_ll = sum Jl^T Jl at the LAST LINEARISATION, est_i its
 * CURRENT ESTIMATE: the minimiser of the merged landmark's linearised cost with the poses held (each member's conditional cost is
 * 1/2 (x - est_i)^T H_i (x - est_i), the back-substitution having left est_i at its conditional optimum).  A member without factors
 * contributes nothing.  One wavefront per cluster (k_lm_merge_fuse), one launch per class, one read-back; the bits of x depend on the
 * cluster alone, not on the list's order or on other clusters.
 * A merge that moved something drops the resident factor: the marginal, gate and pair queries refuse until the next update, and that
 * update — slide_graph_solve included — linearises every factor at the current estimate and factors from block column 0, the step
 * slide_graph_gauss_newton(g, 1) takes (counted as a full update by slide_graph_get_incremental_stats).  Later updates are
 * incremental again.
 * Whole-call refusals (SLIDE_ERR_INVALID, nothing changed, the message names merge_landmarks and the reason), decided on the host:
 * n < 0, a needed pointer NULL, a class that is not a landmark class, fuse neither 0 nor 1, the graph is NULL; a graph with shared
 * slots, ghosts, separator offsets or a batch; with fuse = 1 whatever slide_graph_get_pose_covariances refuses (no resident
 * single-graph factorisation, anything pending or merged since the last solve).  fuse = 0 has no such requirement and merges pending
 * entries first, like every other call.  n == 0 on a graph that would be served: SLIDE_OK. */
int slide_graph_merge_landmarks(slide_graph_t* g, int n, const int32_t* cls, const uint64_t* keep_idx, const uint64_t* drop_idx, int fuse,
                                uint64_t* into /* may be NULL */, int32_t* moved /* may be NULL */, int32_t* status /* may be NULL */);
/* The key landmark (cls, idx) resolves to: itself for a landmark never dropped, its survivor's own key after
 * slide_graph_merge_landmarks dropped it.  SLIDE_MISSING (*into = idx) for a key the graph does not know; SLIDE_ERR_INVALID for a NULL
 * pointer or a class that is not a landmark class.  Host only.  No counterpart in the reference. */
int slide_graph_landmark_alias(slide_graph_t* g, int cls, uint64_t idx, uint64_t* into);
/* Measurement aid: what the LAST slide_graph_merge_landmarks call of this graph spent, in ms — out4 = {host restructure, upload of the
 * merged structure (wall, stream synchronised), the fusion with its table upload and read-back (wall), k_lm_merge_fuse's launches alone
 * between two HIP events}; zeros for what did not run. */
int slide_graph_merge_timing(slide_graph_t* g, double out4[4]);
/* One LARGE problem (n >= 1024 associations; SURVEY A15 speaks of m ~ 1e4) runs on several co-resident workgroups — the rows of the
 * sparse product over the waves of up to 128 workgroups (cooperative launch), one grid barrier per gradient evaluation, everything
 * else repeated per workgroup so that the iterates equal the one-workgroup solve's bit for bit.  SLIDE_CLIPPER_WGS=<k> in the
 * environment forces the workgroup count (1 = one workgroup).  slide_clipper_last_solve_info: how the last
 * slide_clipper_dense_clique call of this process ran (workgroups, gradient evaluations); either pointer may be NULL. */
void slide_clipper_last_solve_info(int* n_workgroups, double* grad_evals);
/* Measurement aid of bench.py's SlideMatch / SlideGraph / CLIPPER legs (pair-tests/s of place_recognition.cpp:98-387, triangle
 * pairs/s of semantic_clipper.cpp:49-118, nnz * 12 B per product of clipper.cpp:172-323): what the LAST stand-alone call of this process
 * spent in its kernels — HIP events on the launch stream right around the launches; uploads, host prefix sums and read-backs excluded —
 * and the work those kernels were given. */
enum {
  SLIDE_MS_PLACE_SWEEP = 0,       /* ms: k_place_sweep + k_place_argmax of the last slide_match_maps / loop-closure search (a list: the whole list) */
  SLIDE_MS_TRI_MATCH = 1,         /* ms: k_tri_prepare x 2 + k_tri_match count and emit passes */
  SLIDE_MS_CLQ_CSR = 2,           /* ms: k_clq_csr count + fill (CSR of the affinity matrix from its dense upper triangle) */
  SLIDE_MS_CLQ_SOLVE = 3,         /* ms: the projected-gradient solve (k_clq_solve or k_clq_solve_coop) */
  SLIDE_MS_AFFINITY = 4,          /* ms: k_clipper_affinity */
  SLIDE_MS_CLQ_NNZ = 5,           /* count: non-zeros of the last CSR built or solved (dense, from associations, or the caller's) */
  SLIDE_MS_PLACE_PAIR_TESTS = 6,  /* count: candidates x query objects x reference objects of the last sweep (a first hit ends a query
                                     object's scan early: upper bound of the pair tests executed) */
  SLIDE_MS_TRI_PAIRS = 7,         /* count: model triangles x data triangles of the last triangle match */
  SLIDE_MS_PLACE_DIST_TESTS = 8,  /* count: distance tests the bucketed sweep was given (candidates x sum over the query objects of the
                                     reference objects of their label): what is left of the pair tests once the label test is a table */
  SLIDE_MS_AFFINITY_CSR = 9,      /* ms: k_affinity_csr count + emit (CSR of the affinity matrix straight from the associations) */
  SLIDE_MS_COUNT = 10
};
int slide_last_device_ms(int what, double* out);
/* The same for several independent problems in ONE launch, a persistent workgroup per problem — the robot pairs of a multi-robot job
 * (semantic_clipper.cpp:227-235 once per pair; 28 pairs at eight robots).  Job j: M_upper[j] (n[j] x n[j]), u0[j] or NULL,
 * nodes_out[j] (>= n[j] ints), u_out[j] (n[j] doubles or NULL); n_nodes[j], score[j].  Results equal n_jobs single calls. */
int slide_clipper_dense_clique_batch(int n_jobs, const double* const* M_upper, const int* n, const double* const* u0, const slide_clipper_params_t* p,
                                     int32_t* const* nodes_out, int* n_nodes, double* const* u_out, double* score);
/* semantic_clipper::match_triangles / compute_triangle_diff semantic_clipper.cpp:49-118.  Triangles: 3 x (x, y) doubles each
 * (the Delaunay triangulation, observation.cpp:13-88, is the caller's).  pts_out: per matched pair three rows
 * [model x, model y, data x, data y] in ascending vertex-to-centroid distance; pairs in the reference's loop order
 * (model-major).  n_pairs returns the total; at most cap_pairs are written. */
int slide_match_triangles(const double* tri_model, int ntm, const double* tri_data, int ntd, double threshold,
                          double* pts_out, double* diffs_out, int cap_pairs, int* n_pairs);
/* semantic_clipper::estimate_tf :122-138 (2-D Kabsch a -> b; tf3 row-major 3x3). */
int slide_estimate_tf2d(const double* a_xy, const double* b_xy, int n, double tf3[9]);
/* semantic_clipper::run_semantic_clipper :140-274 from the triangle lists on: triangle matching, identity association
 * list, affinity (as CSR straight from the associations: no m x m matrix, any number of putative associations whose CSR stays below
 * 2^31 non-zeros), dense clique, min_num_pairs gate, estimate_tf, yaw + xy in a 4x4 row-major tf16 (query -> reference;
 * the caller inverts as place_recognition.cpp:621-624 does).  u0: start weights for the 3 * n_pairs putative
 * associations or NULL (fixed-seed generator).  counts: {putative associations, inliers}.  *found = 1 / 0. */
int slide_semantic_clipper(const double* tri_model, int ntm, const double* tri_data, int ntd, const slide_clipper_params_t* p,
                           int min_num_pairs, double matching_threshold, const double* u0, int n_u0, double tf16[16],
                           int counts[2], int32_t* inliers_out, int cap_inliers, int* found);

/* Input::PickNextMeasurementToAdd backend/sloam/src/core/input.cpp:26-108 (chronological measurement picker + key-frame
 * distance gate; pinned by src/test/input_test.cpp).  Queues are flat arrays with the front at index 0; stamps are (sec, nsec).
 * out4 = {meas_to_add (0 none, 1 odometry, 2 observation, 3 relative measurement), entries the reference pops from the front
 * of the odometry / observation / relative-measurement queue}.  Host bookkeeping, no kernel. */
int slide_pick_next_measurement(const int64_t* odom_sec, const int64_t* odom_nsec, const double* odom_pose7, int n_odom,
                                const int64_t* obs_sec, const int64_t* obs_nsec, int n_obs, const int64_t* rel_sec,
                                const int64_t* rel_nsec, int n_rel, int64_t latest_sec, int64_t latest_nsec,
                                const double latest_pose7[7], double current_time, double msg_delay_tolerance,
                                float min_odom_distance, int out4[4]);
/* CylinderMapManager::InLoopClosureRegion cylinderMapManager.cpp:115-160: is any key pose older than
 * at_least_num_of_poses_old within (max_dist_xy, max_dist_z) of the pose?  cloud: float32 xyz of the key poses
 * (robotPoseCloud_).  *inside = 0 / 1.  Host bookkeeping (a few thousand points per call). */
int slide_in_loop_closure_region(const float* cloud_xyz, int n, const double pose_xyz[3], double max_dist_xy, double max_dist_z,
                                 uint64_t at_least_num_of_poses_old, int* inside);

/* CylinderMapManager::getLoopCandidateIdx cylinderMapManager.cpp:160-184: the first key pose, in FLANN's nearest-first order, within
 * max_dist (float32 squared distances, strict '<') of key pose pose_idx that is not pose_idx itself and has
 * pose_idx - idx > at_least_num_of_poses_old in size_t arithmetic (so an index ABOVE pose_idx wraps around and qualifies, as in the
 * reference).  Equidistant neighbours are ordered by index (FLANN leaves that order unspecified).  Fewer than 50 key poses: not found.
 * Host bookkeeping. */
int slide_loop_candidate_idx(const float* cloud_xyz, int n, double max_dist, uint64_t pose_idx, uint64_t at_least_num_of_poses_old,
                             uint64_t* candidate_idx, int* found);
/* The same test (cylinderMapManager.cpp:160-184) for EVERY key pose that passes it, not only the first FLANN returns: cand_idx in
 * slide_loop_candidate_idx's order (float32 squared distance ascending, then index), so entry 0 is exactly that function's result.
 * *n_found is the full count even when it exceeds cap; at most cap entries are written.  Host bookkeeping. */
int slide_loop_candidate_list(const float* cloud_xyz, int n, double max_dist, uint64_t pose_idx, uint64_t at_least_num_of_poses_old,
                              uint64_t* cand_idx, int cap, int* n_found);

/* 2-D Delaunay triangulation (replaces the qhull call of DelaunayTriangulation::Observation, triangulation/observation.cpp:13-88,
 * options "Qt Qbb Qc Qz Q12 d").  Host code (sweep-hull + Lawson flips, long double predicates).  tri_out: vertex-index triples,
 * ascending inside a triangle, triangles in lexicographic order — the same triangle SET as qhull for points in general position;
 * the list order (qhull: facet order) only permutes SlideGraph's putative association list.  At most cap triangles are written. */
int slide_delaunay_2d(const double* xy, int n, int32_t* tri_out, int cap, int* n_tri);
/* semantic_clipper::run_semantic_clipper semantic_clipper.cpp:140-274 from the two object maps on (rows [label, x, y, z, d1, d2,
 * d3]; only x, y are used there): Delaunay of both, then slide_semantic_clipper.  sigma / epsilon: the EuclideanDistance
 * invariant's parameters as passed by the reference's caller. */
int slide_run_semantic_clipper(const double* ref7, int nr, const double* qry7, int nq, double sigma, double epsilon,
                               int min_num_pairs, double matching_threshold, const double* u0, int n_u0, double tf16[16],
                               int counts[2], int* found);

/* The SlideGraph parameters of PlaceRecognition, names and defaults of place_recognition.cpp:65-75 (ns "<prefix>_slidegraph"). */
typedef struct {
  double sigma;                     /* 0.1   sigma                          (:70-71) */
  double epsilon;                   /* 0.1   epsilon                        (:72-73) */
  int num_inliers_threshold;        /* 10    num_inliners_threshold         (:66-67) -> run_semantic_clipper's min_num_pairs */
  double matching_threshold;        /* 0.1   descriptor_matching_threshold  (:68-69) */
  int min_num_map_objects_to_start; /* 20    min_num_map_objects_to_start   (:74-75) */
} slide_slidegraph_params_t;
void slide_slidegraph_default_params(slide_slidegraph_params_t* p);
/* PlaceRecognition::findInterLoopClosureWithClipper place_recognition.cpp:541-629 (seam S4), the method itself, in its order:
 * 1. rows with x == 0.0 && y == 0.0 are dropped from both maps (:584, :601); 2. the matcher runs only when BOTH maps keep at least
 * min_num_map_objects_to_start objects (:618); 3. run_semantic_clipper on the kept rows (:621: Delaunay, triangle matching, CSR
 * affinity, clique, num_inliers_threshold); 4. tf16 is the INVERSE of what run_semantic_clipper estimated (:624), in the closed form of
 * a planar rigid 4x4 (R^T, -R^T t) — the matrix the reference stores as tfFromQueryToRef.  Nothing found (gate, no matched triangle,
 * too few inliers): *found = 0 and tf16 = identity.  Maps: rows [label, x, y, z, d1, d2, d3]; p NULL: the defaults; u0 / n_u0 as
 * slide_run_semantic_clipper.  counts = {kept reference objects, kept query objects, putative associations, inliers}.  A pair
 * stopped by the gate or without triangles never touches the device.  This is the list form below with one pair; the pair's
 * status is the return value. */
int slide_find_inter_loop_closure_clipper(const double* ref7, int nr, const double* qry7, int nq, const slide_slidegraph_params_t* p,
                                          const double* u0, int n_u0, double tf16[16], int counts[4], int* found);
/* The loop of SLOAMNode::interLoopClosureThread_ (sloamNode.cpp:587-694: one findInterLoopClosureWithClipper per robot without a
 * loopClosureTf, 28 pairs in a central job over eight robots) as ONE call.  Map i = rows [map_off[i], map_off[i + 1]) of maps7;
 * pair k = (reference map pairs[2 k], query map pairs[2 k + 1]).  Every map is filtered and triangulated once however many pairs
 * name it; triangle matching (k_tri_match_seg), the CSRs (k_affinity_csr_seg) and the solves (k_clq_solve_b; a pair of 1024
 * associations or more takes the single call's cooperative route on its slice) run for all pairs together, with three blocking
 * read-backs per call (triangle totals, non-zero totals, results) whatever n_pairs is.  Pair k is evaluated by itself: tf16n + 16 k,
 * counts4n + 4 k and found[k] are exactly what slide_find_inter_loop_closure_clipper gives for that pair alone, bit for bit,
 * whatever else is in the list and wherever the pair stands in it.  u0 may be NULL, u0[k] may be NULL (the fixed-seed start).
 * Refused as a whole on the host, before the device is touched and with nothing written (SLIDE_ERR_INVALID): n_pairs < 0, n_maps < 0,
 * a NULL that is needed (pairs, map_off, tf16n, counts4n, found; maps7 when a map has rows; n_u0 when a u0[k] is given), a negative
 * or decreasing map_off, a pair naming a map outside [0, n_maps).  Otherwise SLIDE_OK (SLIDE_ERR_HIP: no usable device), and a
 * pair's own fault goes to status[k] (status may be NULL) with found[k] = 0 and identity in its tf16: SLIDE_ERR_INVALID for a u0[k]
 * whose length is not the pair's number of putative associations, SLIDE_ERR_CAPACITY for a pair whose CSR would pass 2^31 - 1
 * non-zeros or that would take the list's associations past 2^30 in total.  n_pairs == 0: SLIDE_OK without a device. */
int slide_find_inter_loop_closures_clipper(const double* maps7, const int32_t* map_off, int n_maps, const int32_t* pairs, int n_pairs,
                                           const slide_slidegraph_params_t* p, const double* const* u0, const int* n_u0, double* tf16n,
                                           int32_t* counts4n, int32_t* found, int32_t* status);

/* sloam::FindRelativeMeasurementMatch / GetIndexClosestPoseMstPair (src/core/sloam.cpp:321-440).
 * Stamps are (sec, nsec) pairs.  Host-side logic (tiny, sequential): no kernel. */
int slide_closest_stamp(const int64_t* sec, const int64_t* nsec, int n, int64_t qsec, int64_t qnsec, int* idx, double* diff);
/* sloam::FindRelativeMeasurementMatch sloam.cpp:321-412.  Packets of all robots concatenated (pk_sec / pk_nsec) with
 * offsets[n_robots + 1]; pose_counter per robot; pending measurements (stamp, observed robot, onlyUseOdom flag, caller tag) are
 * compacted IN PLACE exactly as feasible_relative_meas_for_factors is (matched and stale ones erased).  match_out: 4 ints per
 * match {tag, position in the pending list at match time, host pose index, other pose index}.  *n_matches >= 0; returns
 * SLIDE_ERR_INVALID where the reference throws std::runtime_error (robotIndex == host, onlyUseOdom measurement). */
int slide_find_relative_meas_match(int n_robots, const int64_t* pk_sec, const int64_t* pk_nsec, const int32_t* offsets,
                                   const uint64_t* pose_counter, int host, int* n_pending_io, int64_t* m_sec, int64_t* m_nsec,
                                   int32_t* m_robot, int32_t* m_only_odom, int32_t* m_tag, int32_t* match_out, int* n_matches);

#ifdef __cplusplus
}
#endif
#endif /* SLIDE_GPU_H_ */
