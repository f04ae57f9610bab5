// extern "C" boundary (include/slide_gpu.h) of the graph, the batch and the backend: thin wrappers that take the handle's lock and
// forward to HostGraph / CholBatch / HostBackend.  Besides them: the stand-alone dense solve and bordered-factorisation hooks,
// stand-alone association, and five small pure-host functions of the reference's bookkeeping.  The matchers live in files of their
// own: host_place.hip (SlideMatch), host_clipper.hip (CLIPPER), host_slidegraph.hip (SlideGraph), host_closure.hip (closure selection).
// Every compute entry point drives HIP kernels; there is no CPU fallback.
#include <unistd.h>
#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <utility>
#include <vector>

#include "capi_handles.hpp"
#include "delaunay.hpp"
#include "host_backend.hpp"
#include "host_clipper.hpp"

using namespace sl;

struct slide_backend {
  HostBackend b;
  slide_graph_t* gview = nullptr;
  explicit slide_backend(const slide_params_t& p) : b(p) {}
};

static thread_local std::string t_err;

// The gate of CylinderMapManager::getLoopCandidateIdx (cylinderMapManager.cpp:160-184), ONE text for the two functions below:
// visit(d2, i) for every key pose i inside the radius that is old enough, in index order; d2 = its float32 squared distance.
template <class Visit>
static void loop_candidates(const float* cloud_xyz, int n, double max_dist, uint64_t pose_idx, uint64_t at_least_num_of_poses_old, Visit visit) {
  const float qx = cloud_xyz[3 * pose_idx], qy = cloud_xyz[3 * pose_idx + 1], qz = cloud_xyz[3 * pose_idx + 2];
  const float r2 = (float)(max_dist * max_dist);                 // pcl radiusSearch hands radius^2 to FLANN as float
  for (int i = 0; i < n; ++i) {
    const float dx = cloud_xyz[3 * i] - qx, dy = cloud_xyz[3 * i + 1] - qy, dz = cloud_xyz[3 * i + 2] - qz;
    float d2 = dx * dx;
    d2 += dy * dy;
    d2 += dz * dz;
    if (!(d2 < r2)) continue;
    // "nnIdx != poseIdx && poseIdx - nnIdx > at_least_num_of_poses_old" with poseIdx a size_t: a LATER pose wraps around and passes
    if ((uint64_t)i == pose_idx || !(pose_idx - (uint64_t)i > at_least_num_of_poses_old)) continue;
    visit(d2, (uint64_t)i);
  }
}

extern "C" {

void slide_default_params(slide_params_t* p) {
  std::memset(p, 0, sizeof(*p));
  p->pose_chart = SLIDE_CHART_CAYLEY;
  p->relinearize_threshold = 0.1;
  p->noise_floor = 0.01;
  for (int i = 0; i < 6; ++i) {
    p->noise_model_prior_first_pose_vec[i] = 1e-6;
    p->noise_model_odom_vec[i] = 0.1;
    p->noise_model_rel_meas_vec[i] = 0.1;
  }
  for (int i = 0; i < 9; ++i) p->noise_model_cube_vec[i] = 0.1;
  p->cylinder_sigma = 400.0;
  p->bearing_range_sigma = 1.0;
  p->numdiff_delta = 1e-6;
  p->cylinder_match_thresh = 2.0;
  p->cuboid_match_thresh = 2.0;
  p->ellipsoid_match_thresh = 0.75;
  p->knn_cylinder = 50;
  p->knn_cube = 30;
  p->knn_ellipsoid = 1000;
  p->number_of_robots = 1;
  p->device = -1;
}

const char* slide_last_error(void) {
  t_err = g_last_error;
  return t_err.c_str();
}
const char* slide_version(void) { return "slide_slam_amd 0.1 (gfx950, HIP)"; }

int slide_device_check(int device) {
  int n = 0;
  if (!hip_ok(hipGetDeviceCount(&n), "hipGetDeviceCount") || n == 0) {
    if (n == 0) g_last_error = "no HIP device visible";
    return SLIDE_ERR_HIP;
  }
  int dev = device;
  if (dev < 0 && !hip_ok(hipGetDevice(&dev), "hipGetDevice")) return SLIDE_ERR_HIP;
  hipDeviceProp_t prop;
  if (!hip_ok(hipGetDeviceProperties(&prop, dev), "hipGetDeviceProperties")) return SLIDE_ERR_HIP;
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
    g_last_error = std::string("device is ") + prop.gcnArchName + ", this library carries gfx950 code objects only";
    return SLIDE_ERR_HIP;
  }
  return SLIDE_OK;
}

// ---- graph --------------------------------------------------------------------------------------------
slide_graph_t* slide_graph_create(const slide_params_t* p) {
  slide_params_t q;
  if (p) q = *p; else slide_default_params(&q);
  if (slide_device_check(q.device) != SLIDE_OK) return nullptr;
  auto* g = new slide_graph(q);
  if (g->g.init() != SLIDE_OK) { delete g; return nullptr; }
  return g;
}
void slide_graph_destroy(slide_graph_t* g) { delete g; }

int slide_graph_set_prior(slide_graph_t* g, int robot, const double pose7[7]) { if (!g) return SLIDE_ERR_INVALID; LOCK(g); return g->g.set_prior(robot, pose7); }
int slide_graph_add_keypose_between(slide_graph_t* g, int robot, uint64_t from_idx, uint64_t to_idx, const double rel7[7],
                                    const double est7[7]) {
  if (!g) return SLIDE_ERR_INVALID;
  LOCK(g);
  return g->g.add_keypose_between(robot, from_idx, to_idx, rel7, est7);
}
int slide_graph_add_loop_closure(slide_graph_t* g, const double rel7[7], uint64_t i1, int r1, uint64_t i2, int r2) {
  if (!g) return SLIDE_ERR_INVALID;
  LOCK(g);
  return g->g.add_loop_closure(rel7, i1, r1, i2, r2);
}
int slide_graph_add_relative_meas(slide_graph_t* g, const double rel7[7], uint64_t i1, int r1, uint64_t i2, int r2) {
  if (!g) return SLIDE_ERR_INVALID;
  LOCK(g);
  return g->g.add_relative_meas(rel7, i1, r1, i2, r2);
}
int slide_graph_add_point_landmark(slide_graph_t* g, uint64_t lm_idx, const double xyz[3]) {
  if (!g) return SLIDE_ERR_INVALID;
  LOCK(g);
  return g->g.add_point_landmark(lm_idx, xyz);
}
int slide_graph_add_range_bearing(slide_graph_t* g, int robot, uint64_t pose_idx, uint64_t lm_idx, const double bearing[3],
                                  double range) {
  if (!g) return SLIDE_ERR_INVALID;
  LOCK(g);
  return g->g.add_range_bearing(robot, pose_idx, lm_idx, bearing, range);
}
int slide_graph_add_cube(slide_graph_t* g, int robot, uint64_t pose_idx, uint64_t cube_idx, const double pose_world7[7],
                         const double cube_world7[7], const double scale[3], int already_exists) {
  if (!g) return SLIDE_ERR_INVALID;
  LOCK(g);
  return g->g.add_cube(robot, pose_idx, cube_idx, from7(pose_world7), from7(cube_world7), scale, already_exists != 0);
}
int slide_graph_add_cylinder(slide_graph_t* g, int robot, uint64_t pose_idx, uint64_t cyl_idx, const double pose_world7[7],
                             const double root[3], const double ray[3], double radius, int already_exists) {
  if (!g) return SLIDE_ERR_INVALID;
  LOCK(g);
  return g->g.add_cylinder(robot, pose_idx, cyl_idx, from7(pose_world7), root, ray, radius, already_exists != 0);
}
int slide_graph_solve(slide_graph_t* g) { if (!g) return SLIDE_ERR_INVALID; LOCK(g); return g->g.solve(); }
int slide_graph_gauss_newton(slide_graph_t* g, int iterations) { if (!g) return SLIDE_ERR_INVALID; LOCK(g); return g->g.gauss_newton(iterations); }

int slide_graph_get_pose12(slide_graph_t* g, int robot, uint64_t idx, double out12[12]) {
  if (!g) return SLIDE_ERR_INVALID;
  LOCK(g);
  return g->g.get_pose12(robot, idx, out12);
}
int slide_graph_get_pose(slide_graph_t* g, int robot, uint64_t idx, double out7[7]) {
  double p12[12];
  const int rc = slide_graph_get_pose12(g, robot, idx, p12);
  to7(from12(p12), out7);
  return rc;
}
int slide_graph_get_all_poses(slide_graph_t* g, int robot, double* out7N, uint64_t cap, uint64_t* n_out) {
  if (!g) return SLIDE_ERR_INVALID;
  uint64_t n = 0;
  for (uint64_t i = 0; i < cap; ++i) {
    double p7[7];
    const int rc = slide_graph_get_pose(g, robot, i, p7);
    if (rc != SLIDE_OK) break;
    std::memcpy(out7N + 7 * n, p7, sizeof(p7));
    ++n;
  }
  *n_out = n;
  return SLIDE_OK;
}
int slide_graph_get_landmark(slide_graph_t* g, int cls, uint64_t idx, double* out) {
  if (!g || cls < 0 || cls > 2) return SLIDE_ERR_INVALID;
  LOCK(g);
  return g->g.get_landmark(cls, idx, out);
}
// landmark fusion (HostGraph::merge_landmarks): the argument checks come before the graph or the device is looked at
int slide_graph_merge_landmarks(slide_graph_t* g, int n, const int32_t* cls, const uint64_t* keep_idx, const uint64_t* drop_idx, int fuse,
                                uint64_t* into, int32_t* moved, int32_t* status) {
  auto bad = [](const char* what) { g_last_error = std::string("merge_landmarks: ") + what; return SLIDE_ERR_INVALID; };
  if (n < 0) return bad("n < 0");
  if (n > 0 && (!cls || !keep_idx || !drop_idx)) return bad("a needed pointer is NULL");
  for (int k = 0; k < n; ++k)
    if (cls[k] != SLIDE_CLS_ELLIPSOID && cls[k] != SLIDE_CLS_CUBE && cls[k] != SLIDE_CLS_CYLINDER) return bad("a class that is not a landmark class");
  if (fuse != 0 && fuse != 1) return bad("fuse is neither 0 nor 1");
  if (!g) return bad("the graph is NULL");
  LOCK(g);
  return g->g.merge_landmarks(n, cls, keep_idx, drop_idx, fuse == 1, into, moved, status);
}
int slide_graph_landmark_alias(slide_graph_t* g, int cls, uint64_t idx, uint64_t* into) {
  if (!g || !into || (cls != SLIDE_CLS_ELLIPSOID && cls != SLIDE_CLS_CUBE && cls != SLIDE_CLS_CYLINDER)) return SLIDE_ERR_INVALID;
  LOCK(g);
  return g->g.landmark_alias(cls, idx, into);
}
int slide_graph_merge_timing(slide_graph_t* g, double out4[4]) { if (!g || !out4) return SLIDE_ERR_INVALID; LOCK(g); g->g.merge_timing(out4); return SLIDE_OK; }
int slide_graph_stats(slide_graph_t* g, int64_t out5[5]) { if (!g) return SLIDE_ERR_INVALID; LOCK(g); g->g.stats(out5); return SLIDE_OK; }
int64_t slide_graph_rejected_count(slide_graph_t* g) { if (!g) return -1; LOCK(g); return g->g.rejected(); }
int slide_graph_set_profiling(slide_graph_t* g, int on) {
  if (!g) return SLIDE_ERR_INVALID;
  LOCK(g);
  g->g.prof.on = on != 0;
  g->g.prof.reset();
  return SLIDE_OK;
}
int slide_graph_get_profile(slide_graph_t* g, char* names, double* ms_total, int64_t* launches, int n_max) {
  if (!g) return SLIDE_ERR_INVALID;
  LOCK(g);
  const Profiler& p = g->g.prof;
  const int n = std::min<int>(n_max, (int)p.names.size());
  for (int i = 0; i < n; ++i) {
    std::strncpy(names + 32 * i, p.names[i].c_str(), 31);
    names[32 * i + 31] = 0;
    ms_total[i] = p.ms[i];
    launches[i] = p.count[i];
  }
  return n;
}

int slide_graph_set_shared(slide_graph_t* g, const int32_t* cls, const int64_t* idx, const int32_t* owner, int n_slots) {
  if (!g || n_slots < 0) return SLIDE_ERR_INVALID;
  LOCK(g);
  return g->g.set_shared(cls, idx, owner, n_slots);
}
int slide_graph_get_pose_covariance(slide_graph_t* g, int robot, uint64_t idx, double cov36[36]) {
  if (!g) return SLIDE_ERR_INVALID;
  LOCK(g);
  return g->g.pose_covariance(robot, idx, cov36);
}
int slide_graph_get_pose_covariances(slide_graph_t* g, int robot, const uint64_t* idx, int n, double* out36n) {
  if (!g) return SLIDE_ERR_INVALID;
  LOCK(g);
  return g->g.pose_covariances(robot, idx, n, out36n);
}
int slide_graph_get_landmark_covariances(slide_graph_t* g, int cls, const uint64_t* idx, int n, double* out) {
  if (!g) return SLIDE_ERR_INVALID;
  LOCK(g);
  return g->g.landmark_covariances(cls, idx, n, out);
}
int slide_graph_marginal_traces(slide_graph_t* g, int robot, double out4[4]) {
  if (!g || !out4) return SLIDE_ERR_INVALID;
  LOCK(g);
  return g->g.marginal_traces(robot, out4);
}
int slide_graph_closure_info_gain(slide_graph_t* g, int robot, const uint64_t* traj, int n, const double* travel, const double sigma_per_m[6],
                                  double out3[3]) {
  if (!g || !out3) return SLIDE_ERR_INVALID;
  LOCK(g);
  return g->g.closure_info_gain(robot, traj, n, travel, sigma_per_m, out3);
}
int slide_graph_closure_info_gain_batch(slide_graph_t* g, int robot, int n_cand, const int32_t* off, const uint64_t* traj,
                                        const double* travel, const double sigma_per_m[6], double* out3n, int32_t* status) {
  if (!g) return SLIDE_ERR_INVALID;
  LOCK(g);
  return g->g.closure_info_gain_batch(robot, n_cand, off, traj, travel, sigma_per_m, out3n, status);
}
int slide_graph_add_relative_meas_ghost(slide_graph_t* g, const double rel7[7], uint64_t idx, int robot, int ghost_slot, int local_first) {
  if (!g) return SLIDE_ERR_INVALID;
  LOCK(g);
  return g->g.add_relative_meas_ghost(rel7, idx, robot, ghost_slot, local_first != 0);
}
int slide_graph_set_ghosts(slide_graph_t* g, const int32_t* own_robot, const int64_t* own_idx, int n_slots) {
  if (!g || n_slots < 0) return SLIDE_ERR_INVALID;
  LOCK(g);
  return g->g.set_ghosts(own_robot, own_idx, n_slots);
}
int slide_graph_dist_phase(slide_graph_t* g, int phase, double* d_buf) {
  if (!g) return SLIDE_ERR_INVALID;
  LOCK(g);
  return g->g.dist_phase(phase, d_buf);
}

slide_chol_batch_t* slide_chol_batch_create(int n_graphs) {
  if (n_graphs < 1 || n_graphs > 8) return nullptr;
  return new slide_chol_batch(n_graphs);
}
void slide_chol_batch_destroy(slide_chol_batch_t* b) { delete b; }
int slide_graph_join_chol_batch(slide_graph_t* g, slide_chol_batch_t* b, int slot) {
  if (!g) return SLIDE_ERR_INVALID;
  if (b && (slot < 0 || slot >= b->b.n_slots())) return SLIDE_ERR_INVALID;
  if (b) {
    LOCK(g);
    if (g->g.robust_on()) {
      g_last_error = "join_chol_batch: a robust loss is set on this graph; the sharded and joint paths do not carry it (slide_graph_set_robust_loss(g, 0, 0, 0) first)";
      return SLIDE_ERR_INVALID;
    }
    if (g->g.observation_loss_on()) {
      g_last_error = "join_chol_batch: an observation loss is set on this graph; the sharded and joint paths do not carry it (slide_graph_set_observation_loss(g, 0, 0, 0) first)";
      return SLIDE_ERR_INVALID;
    }
  }
  g->g.join_batch(b ? &b->b : nullptr, slot);      // (takes the graph's lock itself, and the batch's only after releasing it)
  return SLIDE_OK;
}

int slide_chol_batch_pass(slide_chol_batch_t* b, double* const* d_bufs) {
  if (!b || !d_bufs) return SLIDE_ERR_INVALID;
  return b->b.pass_all(d_bufs);
}
int slide_chol_batch_get_pose_covariances(slide_chol_batch_t* b, int slot, const uint64_t* idx, int n, double* out36n) {
  if (!b) return SLIDE_ERR_INVALID;
  return b->b.joint_pose_covariances(slot, idx, n, out36n);
}
int slide_chol_batch_get_landmark_covariances(slide_chol_batch_t* b, int slot, int cls, const uint64_t* idx, int n, double* out) {
  if (!b) return SLIDE_ERR_INVALID;
  return b->b.joint_landmark_covariances(slot, cls, idx, n, out);
}
int slide_chol_batch_marginal_traces(slide_chol_batch_t* b, int slot, double out4[4]) {
  if (!b || !out4) return SLIDE_ERR_INVALID;
  return b->b.joint_marginal_traces(slot, out4);
}
int slide_chol_batch_closure_info_gain(slide_chol_batch_t* b, int slot, const int32_t* traj_slots, const uint64_t* traj, int n,
                                       const double* travel, const double sigma_per_m[6], double out4[4]) {
  if (!b || !out4) return SLIDE_ERR_INVALID;
  return b->b.joint_closure_info_gain(slot, traj_slots, traj, n, travel, sigma_per_m, out4);
}
int slide_chol_batch_closure_info_gain_batch(slide_chol_batch_t* b, int slot, int n_cand, const int32_t* off, const int32_t* traj_slots,
                                             const uint64_t* traj, const double* travel, const double sigma_per_m[6], double* out4n,
                                             int32_t* status) {
  if (!b) return SLIDE_ERR_INVALID;
  return b->b.joint_closure_info_gain_batch(slot, n_cand, off, traj_slots, traj, travel, sigma_per_m, out4n, status);
}
int slide_chol_batch_set_pcg(slide_chol_batch_t* b, int iterations) {
  if (!b || iterations < 0) return SLIDE_ERR_INVALID;
  if (iterations > 0 && b->b.robust_on()) {
    g_last_error = "chol_batch_set_pcg: a robust loss is set on this batch; the PCG passes do not carry it (slide_chol_batch_set_robust_loss(b, 0, 0, 0) first)";
    return SLIDE_ERR_INVALID;
  }
  if (iterations > 0 && b->b.observation_loss_on()) {
    g_last_error = "chol_batch_set_pcg: an observation loss is set on this batch; the PCG passes do not carry it (slide_chol_batch_set_observation_loss(b, 0, 0, 0) first)";
    return SLIDE_ERR_INVALID;
  }
  b->b.set_pcg(iterations, b->b.pcg_tolerance());
  return SLIDE_OK;
}
int slide_graph_set_pcg(slide_graph_t* g, int iterations) {
  if (!g || iterations < 0) return SLIDE_ERR_INVALID;
  LOCK(g);
  g->g.set_pcg(iterations, g->g.pcg_tolerance());
  return SLIDE_OK;
}
int slide_chol_batch_set_pcg_tolerance(slide_chol_batch_t* b, double tol) {
  if (!b || !(tol >= 0.0)) return SLIDE_ERR_INVALID;
  b->b.set_pcg(b->b.pcg(), tol);
  return SLIDE_OK;
}
int slide_graph_set_pcg_tolerance(slide_graph_t* g, double tol) {
  if (!g || !(tol >= 0.0)) return SLIDE_ERR_INVALID;
  LOCK(g);
  g->g.set_pcg(g->g.pcg(), tol);
  return SLIDE_OK;
}
int slide_graph_set_separator(slide_graph_t* g, const int32_t* off, int n) {
  if (!g) return SLIDE_ERR_INVALID;
  LOCK(g);
  return g->g.set_separator(off, n);
}
int slide_chol_batch_set_exact_joint(slide_chol_batch_t* b, int on, double* sep_buf, long long len) {
  if (!b || len < 0) return SLIDE_ERR_INVALID;
  return b->b.set_arrow(on != 0, sep_buf, len);
}
int slide_chol_batch_set_separator_profile(slide_chol_batch_t* b, const int32_t* prof, int n) {
  if (!b || n < 0 || (n > 0 && !prof)) return SLIDE_ERR_INVALID;
  return b->b.set_separator_profile(prof, n);
}
int slide_chol_batch_set_separator_blocks(slide_chol_batch_t* b, int Ta, int Tb, int used_a, int used_b) {
  if (!b) return SLIDE_ERR_INVALID;
  return b->b.set_separator_blocks(Ta, Tb, used_a, used_b);
}
int slide_chol_batch_set_separator_owner(slide_chol_batch_t* b, int leaf, int leader) {
  if (!b) return SLIDE_ERR_INVALID;
  return b->b.set_separator_owner(leaf, leader != 0);
}
int slide_chol_batch_sep_segment(int m, int n_relmeas, int Ta, int Tb, int which, long long out2[2]) {
  if (m < 0 || n_relmeas < 0 || Ta <= 0 || Tb <= 0 || which < 0 || which > 2 || !out2 || (long long)(Ta + Tb) * 64 >= m) return SLIDE_ERR_INVALID;
  sl::CholBatch::sep_segment(m, 6 * n_relmeas, Ta, Tb, which, &out2[0], &out2[1]);
  return SLIDE_OK;
}
int slide_chol_batch_set_segments(slide_chol_batch_t* b, int n_seg) {
  if (!b || n_seg < 1) return SLIDE_ERR_INVALID;
  b->b.set_segments(n_seg);
  return SLIDE_OK;
}
long long slide_chol_batch_sep_exchange_len(int m, int n_relmeas, int Ta, int Tb) {
  return (m < 0 || n_relmeas < 0 || Ta < 0 || Tb < 0 || (long long)(Ta + Tb) * 64 > m) ? 0 : sl::CholBatch::sep_exchange_len(m, 6 * n_relmeas, Ta, Tb);
}
long long slide_chol_batch_sep_buffer_len(int m, int n_relmeas) { return (m < 0 || n_relmeas < 0) ? 0 : sl::CholBatch::sep_buffer_len(m, 6 * n_relmeas); }
int slide_graph_set_ghost_ids(slide_graph_t* g, const int32_t* ids, int n, int n_total) {
  if (!g) return SLIDE_ERR_INVALID;
  LOCK(g);
  return g->g.set_ghost_ids(ids, n, n_total);
}
int slide_graph_set_robust_loss(slide_graph_t* g, int kind, double param, int class_mask) {
  if (!g) return SLIDE_ERR_INVALID;
  LOCK(g);
  return g->g.set_robust_loss(kind, param, class_mask);
}
int slide_graph_get_closure_weights(slide_graph_t* g, int cap, int32_t* from_robot, uint64_t* from_idx, int32_t* to_robot, uint64_t* to_idx,
                                    int32_t* kind, double* weight, double* s2, int* n_out) {
  if (!g || !n_out || cap < 0) return SLIDE_ERR_INVALID;
  LOCK(g);
  return g->g.get_closure_weights(cap, from_robot, from_idx, to_robot, to_idx, kind, weight, s2, n_out);
}
int slide_chol_batch_set_robust_loss(slide_chol_batch_t* b, int kind, double param, int class_mask) {
  if (!b) return SLIDE_ERR_INVALID;
  return b->b.set_robust_loss(kind, param, class_mask);
}
int slide_chol_batch_get_closure_weights(slide_chol_batch_t* b, int cap, int32_t* slot, int32_t* from_robot, uint64_t* from_idx, int32_t* to_robot,
                                         uint64_t* to_idx, int32_t* kind, int32_t* ghost_id, double* weight, double* s2, int* n_out) {
  if (!b || !n_out || cap < 0) return SLIDE_ERR_INVALID;
  return b->b.get_closure_weights(cap, slot, from_robot, from_idx, to_robot, to_idx, kind, ghost_id, weight, s2, n_out);
}
int slide_chol_batch_profile_robust_reweight(slide_chol_batch_t* b, double* const* d_bufs, double* ms) {
  if (!b || !d_bufs || !ms) return SLIDE_ERR_INVALID;
  return b->b.profile_robust_reweight(d_bufs, ms);
}
int slide_chol_batch_set_observation_loss(slide_chol_batch_t* b, int kind, double param, int class_mask) {
  if (!b) return SLIDE_ERR_INVALID;
  return b->b.set_observation_loss(kind, param, class_mask);
}
int slide_chol_batch_get_observation_weights(slide_chol_batch_t* b, int cap, int32_t* slot, uint64_t* pose_idx, int32_t* cls, uint64_t* lm_idx, double* weight,
                                             double* s2, int* n_out) {
  if (!b || !n_out || cap < 0) return SLIDE_ERR_INVALID;
  return b->b.get_observation_weights(cap, slot, pose_idx, cls, lm_idx, weight, s2, n_out);
}
int slide_chol_batch_profile_linearize(slide_chol_batch_t* b, double* const* d_bufs, double* ms) {
  if (!b || !d_bufs || !ms) return SLIDE_ERR_INVALID;
  return b->b.profile_linearize(d_bufs, ms);
}
int slide_graph_set_observation_loss(slide_graph_t* g, int kind, double param, int class_mask) {
  if (!g) return SLIDE_ERR_INVALID;
  LOCK(g);
  return g->g.set_observation_loss(kind, param, class_mask);
}
int slide_graph_get_observation_weights(slide_graph_t* g, int cap, int32_t* robot, uint64_t* pose_idx, int32_t* cls, uint64_t* lm_idx, double* weight,
                                        double* s2, int* n_out) {
  if (!g || !n_out || cap < 0) return SLIDE_ERR_INVALID;
  LOCK(g);
  return g->g.get_observation_weights(cap, robot, pose_idx, cls, lm_idx, weight, s2, n_out);
}
int slide_graph_chi2(slide_graph_t* g, double out4[4]) { if (!g || !out4) return SLIDE_ERR_INVALID; LOCK(g); return g->g.chi2(out4); }
int slide_graph_get_pcg_stats(slide_graph_t* g, double out8[8]) { if (!g || !out8) return SLIDE_ERR_INVALID; LOCK(g); return g->g.pcg_stats(out8); }
int slide_graph_get_tile_profile(slide_graph_t* g, int* prof, int cap) { if (!g || (cap > 0 && !prof)) return SLIDE_ERR_INVALID; LOCK(g); return g->g.get_tile_profile(prof, cap); }
int slide_graph_get_border_profile(slide_graph_t* g, int* first, int cap) { if (!g || (cap > 0 && !first)) return SLIDE_ERR_INVALID; LOCK(g); return g->g.get_border_profile(first, cap); }
int slide_graph_set_incremental(slide_graph_t* g, int on) { if (!g) return SLIDE_ERR_INVALID; LOCK(g); g->g.set_incremental(on != 0); return SLIDE_OK; }
int slide_graph_set_wildfire(slide_graph_t* g, double threshold) { if (!g) return SLIDE_ERR_INVALID; LOCK(g); g->g.set_wildfire(threshold); return SLIDE_OK; }
int slide_graph_get_wildfire_stats(slide_graph_t* g, int64_t out2[2]) { if (!g || !out2) return SLIDE_ERR_INVALID; LOCK(g); g->g.wildfire_stats(out2); return SLIDE_OK; }
int slide_graph_get_incremental_stats(slide_graph_t* g, int64_t out4[4]) { if (!g || !out4) return SLIDE_ERR_INVALID; LOCK(g); g->g.incremental_stats(out4); return SLIDE_OK; }
int slide_graph_get_segment_table(slide_graph_t* g, int* out, int cap) { if (!g || (cap > 0 && !out)) return SLIDE_ERR_INVALID; LOCK(g); return g->g.get_segment_table(out, cap); }
int slide_graph_get_segments(slide_graph_t* g, int* out, int cap) { if (!g || (cap > 0 && !out)) return SLIDE_ERR_INVALID; LOCK(g); return g->g.get_segments(out, cap); }
int slide_graph_set_dense_profile(slide_graph_t* g, int on) { if (!g) return SLIDE_ERR_INVALID; LOCK(g); g->g.set_dense_profile(on != 0); return SLIDE_OK; }
int slide_chol_batch_pass_part(slide_chol_batch_t* b, double* const* d_bufs, int part) {
  if (!b || !d_bufs) return SLIDE_ERR_INVALID;
  return b->b.pass_part(d_bufs, part);
}
int slide_chol_batch_profile_exact_joint(slide_chol_batch_t* b, double* const* d_bufs, double out6[6], int* n_sep_steps) {
  if (!b || !d_bufs || !out6) return SLIDE_ERR_INVALID;
  return b->b.profile_arrow(d_bufs, out6, n_sep_steps);
}
void* slide_chol_batch_stream(slide_chol_batch_t* b) { return b ? (void*)b->b.pass_stream() : nullptr; }
int slide_chol_batch_profile(slide_chol_batch_t* b, double* const* d_bufs, double* ms_steps, int* n_launches) {
  if (!b || !d_bufs) return SLIDE_ERR_INVALID;
  return b->b.profile_pass(d_bufs, ms_steps, n_launches);
}
int slide_graph_dist_pass_local(slide_graph_t* g, double* d_buf) {
  if (!g) return SLIDE_ERR_INVALID;
  LOCK(g);
  return g->g.dist_pass_local(d_buf);
}

// ---- stand-alone dense SPD solve (the Schur-system kernel on caller buffers) -------------------------
int slide_dense_spd_solve(const double* A, int n, const double* b, double* x, int repeats, double* ms_out) {
  return slide_dense_spd_solve_ex(A, n, b, x, repeats, ms_out, 0);
}
int slide_dense_spd_solve_ex(const double* A, int n, const double* b, double* x, int repeats, double* ms_out, int method) {
  if (slide_device_check(-1) != SLIDE_OK) return SLIDE_ERR_HIP;
  if (n <= 0 || repeats < 1 || method < 0 || method > 2) return SLIDE_ERR_INVALID;
  const int T = (n + NB - 1) / NB;
  const size_t ld = (size_t)(T + 1) * NB, ncol = (size_t)T * NB;
  std::vector<double> S(ld * ncol, 0.0);
  for (int j = 0; j < n; ++j)
    for (int i = j; i < n; ++i) S[(size_t)j * ld + i] = A[(size_t)j * n + i];
  for (size_t i = n; i < ncol; ++i) S[i * ld + i] = 1.0;
  for (int j = 0; j < n; ++j) S[(size_t)j * ld + ncol] = b[j];
  Tmp Tm;
  double* dS0 = Tm.up(S.data(), S.size());
  double* dS = Tm.up<double>(nullptr, S.size());
  double* dW = Tm.up<double>(nullptr, (size_t)T * NB * NB);
  double* dWi = Tm.up<double>(nullptr, (size_t)T * 1024);
  double* dy = Tm.up<double>(nullptr, ncol);
  double* dx = Tm.up<double>(nullptr, ncol);
  int* dst = Tm.up<int>(nullptr, 8);
  int* dctr = Tm.up<int>(nullptr, (size_t)T + 2);
  int* dtick = Tm.up<int>(nullptr, CHOL_STEP_BATCH_MAX);
  if (!dS0 || !dS || !dW || !dWi || !dy || !dx || !dst || !dctr || !dtick) { g_last_error = "hipMalloc/hipMemcpy failed"; return SLIDE_ERR_HIP; }
  SL_HIP(hipMemset(dtick, 0, CHOL_STEP_BATCH_MAX * sizeof(int)));
  SL_HIP(hipMemset(dst, 0, 8 * sizeof(int)));
  SL_HIP(hipMemset(dctr, 0, ((size_t)T + 2) * sizeof(int)));
  hipEvent_t e0, e1;
  SL_HIP(hipEventCreate(&e0));
  SL_HIP(hipEventCreate(&e1));
  float total = 0.f;
  CholSystem cs{};
  cs.S = dS; cs.ld = (int)ld; cs.T = T; cs.Ld = dW; cs.Winv = dWi; cs.yv = dy; cs.dp = dx; cs.status = dst;
  CholLLPlan* plan = method == 1 ? chol_ll_plan_create(&cs, 1) : nullptr;
  if (method == 1 && !plan) { g_last_error = "hipMalloc failed (left-looking plan)"; return SLIDE_ERR_HIP; }
  for (int r = 0; r < repeats; ++r) {
    SL_HIP(hipMemcpyAsync(dS, dS0, S.size() * sizeof(double), hipMemcpyDeviceToDevice, nullptr));
    SL_HIP(hipEventRecord(e0, nullptr));
    if (plan) {
      int* trace = nullptr;
      const int nt = chol_ll_plan_tasks(plan);
      static const bool want_trace = getenv("SLIDE_LL_TRACE") && getenv("SLIDE_LL_TRACE")[0] == '1';
      if (want_trace && hipHostMalloc(reinterpret_cast<void**>(&trace), (size_t)nt * 16 * sizeof(int), hipHostMallocMapped) == hipSuccess)
        memset(trace, 0, (size_t)nt * 16 * sizeof(int));
      launch_chol_ll(plan, &cs, 1, nullptr, trace);
      if (trace) {
        // diagnostic watchdog: the launch must be through within seconds; if not, print where every task stands and leave the process
        hipEvent_t done;
        SL_HIP(hipEventCreate(&done));
        SL_HIP(hipEventRecord(done, nullptr));
        int waited = 0;
        while (hipEventQuery(done) == hipErrorNotReady && waited < 8000) { usleep(1000); ++waited; }
        if (hipEventQuery(done) == hipErrorNotReady) {
          fprintf(stderr, "k_chol_ll still running after %d ms; tasks (ticket: stage kind k row | barrier-1 waves, barrier-2 waves):\n", waited);
          for (int t = 0; t < nt; ++t)
            if (trace[16 * t] != 5) fprintf(stderr, "  %4d: stage %d kind %d k %d row %d | %03x %03x\n", t, trace[16 * t], trace[16 * t + 1], trace[16 * t + 2], trace[16 * t + 3], trace[16 * t + 4], trace[16 * t + 5]);
          fflush(stderr);
          _exit(3);
        }
        (void)hipEventDestroy(done);
        if (const char* path = getenv("SLIDE_LL_TRACE_FILE")) {      // the stage clocks of every task, for tools/ll_trace.py
          if (FILE* f = fopen(path, "wb")) { fwrite(trace, sizeof(int), (size_t)nt * 16, f); fclose(f); }
        }
        (void)hipHostFree(trace);
      }
      launch_chol_bwd_all(dS, (int)ld, T, dW, dWi, dy, dx, dst, nullptr, nullptr);
    } else if (method == 2) {      // two block columns per launch (k_chol_pair_batched), then the usual extraction and backward chain
      launch_chol_batch(&cs, 1, dctr, nullptr, nullptr, false, 100, dtick);
      launch_chol_bwd_all(dS, (int)ld, T, dW, dWi, dy, dx, dst, nullptr, nullptr);
    } else {
      chol_factor_solve(dS, (int)ld, T, dW, dWi, dy, dx, dst, dctr, nullptr);
    }
    SL_HIP(hipEventRecord(e1, nullptr));
    SL_HIP(hipEventSynchronize(e1));
    float ms = 0.f;
    SL_HIP(hipEventElapsedTime(&ms, e0, e1));
    total += ms;
  }
  if (plan) { (void)hipDeviceSynchronize(); chol_ll_plan_destroy(plan); }
  SL_HIP(hipGetLastError());
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  int st[8];
  SL_HIP(hipMemcpy(st, dst, sizeof(st), hipMemcpyDeviceToHost));
  std::vector<double> xs(ncol);
  SL_HIP(hipMemcpy(xs.data(), dx, ncol * sizeof(double), hipMemcpyDeviceToHost));
  for (int i = 0; i < n; ++i) x[i] = xs[i];
  if (ms_out) *ms_out = total;
  if (st[1] & 1) { g_last_error = "matrix not positive definite"; return SLIDE_ERR_NOT_SPD; }
  st[0] = 0;
  return decode_status(st);
}

// ---- the factorisation of a BORDERED system with a profile, on caller data (unit-test hook of the step / pair kernels) ----------------
// One system exactly as the exact joint passes hand it to launch_chol_batch: S (ld x T*NB, column-major: the band's lower tiles inside
// the profile, nbr border row tiles from tile row b0 (0: right behind the band) on, the right-hand-side row tile behind them), the
// host tables of CholSystem (prof: T ints or NULL = dense; bfirst: nbr ints, non-decreasing, first block column (+ kofs) of every
// border row in the order `ord` lists them, or NULL = every row from column 0; ord: nbr ints or NULL).  The system is factored
// n_copies times side by side in ONE launch sequence (separate buffers); S_out / Ld_out / Winv_out receive copy 0, *max_copy_diff
// the largest |difference| of any other copy's S from it (0: the launch treats every system alike).  method 0: one step launch per
// block column, 2: two block columns per launch.
int slide_debug_chol_bordered(const double* S_in, int ld, int T, int nbr, const int* prof, const int* bfirst, const int* ord, int b0, int kofs,
                              int n_copies, int method, double* S_out, double* Ld_out, double* Winv_out, int* status_out, double* max_copy_diff) {
  if (slide_device_check(-1) != SLIDE_OK) return SLIDE_ERR_HIP;
  if (!S_in || T < 1 || nbr < 0 || n_copies < 1 || n_copies > CHOL_STEP_BATCH_MAX || (method != 0 && method != 2)) return SLIDE_ERR_INVALID;
  const int B0 = b0 > 0 ? b0 : T;
  if (ld < (B0 + nbr + 1) * NB) return SLIDE_ERR_INVALID;
  const size_t len = (size_t)ld * T * NB;
  Tmp Tm;
  std::vector<CholSystem> sys(n_copies);
  std::vector<double*> dS(n_copies);
  int* d_ord = ord ? Tm.up(ord, (size_t)nbr) : nullptr;
  int* d_ctr = Tm.up<int>(nullptr, (size_t)T + 3);
  if ((ord && !d_ord) || !d_ctr) { g_last_error = "hipMalloc/hipMemcpy failed"; return SLIDE_ERR_HIP; }
  SL_HIP(hipMemset(d_ctr, 0, ((size_t)T + 3) * sizeof(int)));
  for (int c = 0; c < n_copies; ++c) {
    dS[c] = Tm.up(S_in, len);
    CholSystem cs{};
    cs.S = dS[c]; cs.ld = ld; cs.T = T;
    cs.Ld = Tm.up<double>(nullptr, (size_t)T * NB * NB); cs.Winv = Tm.up<double>(nullptr, (size_t)T * 1024);
    cs.yv = Tm.up<double>(nullptr, (size_t)T * NB); cs.dp = Tm.up<double>(nullptr, (size_t)T * NB);
    cs.status = Tm.up<int>(nullptr, 8);
    if (!cs.S || !cs.Ld || !cs.Winv || !cs.yv || !cs.dp || !cs.status) { g_last_error = "hipMalloc/hipMemcpy failed"; return SLIDE_ERR_HIP; }
    SL_HIP(hipMemset(cs.status, 0, 8 * sizeof(int)));
    SL_HIP(hipMemset(cs.Ld, 0, (size_t)T * NB * NB * sizeof(double)));
    cs.h_prof = prof; cs.nbr = nbr; cs.h_bfirst = bfirst; cs.b0 = b0; cs.kofs = kofs; cs.ord = d_ord;
    sys[c] = cs;
  }
  int* d_tick = Tm.up<int>(nullptr, CHOL_STEP_BATCH_MAX);
  if (!d_tick) { g_last_error = "hipMalloc failed"; return SLIDE_ERR_HIP; }
  SL_HIP(hipMemset(d_tick, 0, CHOL_STEP_BATCH_MAX * sizeof(int)));
  launch_chol_batch(sys.data(), n_copies, d_ctr, nullptr, nullptr, false, 100, method == 2 ? d_tick : nullptr);
  if (method == 2) {      // (the counters are back at zero once the launches are through)
    int tk[CHOL_STEP_BATCH_MAX];
    SL_HIP(hipMemcpy(tk, d_tick, sizeof(tk), hipMemcpyDeviceToHost));
    for (int c = 0; c < CHOL_STEP_BATCH_MAX; ++c)
      if (tk[c] != 0) { g_last_error = "pair kernel: a ticket counter was left at " + std::to_string(tk[c]); return SLIDE_ERR_HIP; }
  }
  SL_HIP(hipDeviceSynchronize());
  SL_HIP(hipGetLastError());
  std::vector<double> ref(len), other;
  SL_HIP(hipMemcpy(ref.data(), dS[0], len * sizeof(double), hipMemcpyDeviceToHost));
  double worst = 0.0;
  for (int c = 1; c < n_copies; ++c) {
    other.resize(len);
    SL_HIP(hipMemcpy(other.data(), dS[c], len * sizeof(double), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < len; ++i) {
      const double d = std::fabs(other[i] - ref[i]);
      if (!(d <= worst)) worst = std::isnan(d) ? (std::isnan(ref[i]) && std::isnan(other[i]) ? worst : INFINITY) : d;
    }
  }
  if (S_out) std::memcpy(S_out, ref.data(), len * sizeof(double));
  if (Ld_out) SL_HIP(hipMemcpy(Ld_out, sys[0].Ld, (size_t)T * NB * NB * sizeof(double), hipMemcpyDeviceToHost));
  if (Winv_out) SL_HIP(hipMemcpy(Winv_out, sys[0].Winv, (size_t)T * 1024 * sizeof(double), hipMemcpyDeviceToHost));
  if (status_out) SL_HIP(hipMemcpy(status_out, sys[0].status, 8 * sizeof(int), hipMemcpyDeviceToHost));
  if (max_copy_diff) *max_copy_diff = worst;
  return SLIDE_OK;
}

// ---- the same on a MIXED batch, every launch shape (slide_gpu.h) -----------------------------------------------------------------------
// What both entries check of the systems' descriptors; fills the host side of the CholSystems (no device pointer).
static bool debug_chol_systems(int n, const int* ld, const int* T, const int* nbr, const int* prof, const int* prof_off, const int* bfirst,
                               const int* bfirst_off, const int* b0, const int* kofs, int method, int cu_share, std::vector<CholSystem>& sys) {
  if (n < 1 || n > CHOL_STEP_BATCH_MAX || !T || !nbr || (method != 0 && method != 2) || cu_share < 0 || cu_share > 100) return false;
  sys.assign(n, CholSystem{});
  for (int i = 0; i < n; ++i) {
    CholSystem& cs = sys[i];
    cs.T = T[i]; cs.nbr = nbr[i]; cs.b0 = b0 ? b0[i] : 0; cs.kofs = kofs ? kofs[i] : 0;
    if (cs.T < 1 || cs.nbr < 0 || cs.b0 < 0 || (cs.b0 > 0 && cs.b0 < cs.T)) return false;
    if (ld) {
      cs.ld = ld[i];
      if (cs.ld < ((cs.b0 > 0 ? cs.b0 : cs.T) + cs.nbr + 1) * NB) return false;
    }
    if (prof_off && prof_off[i] >= 0) {
      if (!prof) return false;
      cs.h_prof = prof + prof_off[i];
      for (int c = 0; c < cs.T; ++c)      // monotone, inside the band: the kernels index S by it
        if (cs.h_prof[c] < c || cs.h_prof[c] >= cs.T || (c > 0 && cs.h_prof[c] < cs.h_prof[c - 1])) return false;
    }
    if (bfirst_off && bfirst_off[i] >= 0) {
      if (!bfirst) return false;
      cs.h_bfirst = bfirst + bfirst_off[i];
    }
  }
  return true;
}
static int copy_trace(const std::vector<int>& trace, int* trace_out, int trace_cap) {
  const int rows = (int)(trace.size() / 5);
  if (trace_out && trace_cap > 0) std::memcpy(trace_out, trace.data(), (size_t)std::min(rows, trace_cap) * 5 * sizeof(int));
  return rows;
}
int slide_debug_chol_plan(int n, const int* T, const int* nbr, const int* prof, const int* prof_off, const int* bfirst, const int* bfirst_off,
                          const int* b0, const int* kofs, int method, int cu_share, int assumed_cus, int* trace_out, int trace_cap) {
  std::vector<CholSystem> sys;
  if (assumed_cus < 1 || !debug_chol_systems(n, nullptr, T, nbr, prof, prof_off, bfirst, bfirst_off, b0, kofs, method, cu_share, sys)) return SLIDE_ERR_INVALID;
  int tick = 0;      // (never dereferenced: a dry run launches nothing)
  CholPlanHook hook(assumed_cus, true);
  launch_chol_batch(sys.data(), n, nullptr, nullptr, nullptr, false, cu_share, method == 2 ? &tick : nullptr);
  return copy_trace(hook.trace, trace_out, trace_cap);
}
int slide_debug_chol_batch(int n, const double* S_in, const int* ld, const int* T, const int* nbr, const int* prof, const int* prof_off,
                           const int* bfirst, const int* bfirst_off, const int* ord, const int* ord_off, const int* b0, const int* kofs,
                           int method, int cu_share, int assumed_cus, int want_l32, double* S_out, double* Ld_out, double* Winv_out,
                           int* status_out, float* L32_out, int* trace_out, int trace_cap, int* n_launches, int* n_cu_out) {
  if (n_launches) *n_launches = 0;
  if (slide_device_check(-1) != SLIDE_OK) return SLIDE_ERR_HIP;
  std::vector<CholSystem> sys;
  if (!S_in || !ld || assumed_cus < 0 || assumed_cus > chol_device_cus() ||
      !debug_chol_systems(n, ld, T, nbr, prof, prof_off, bfirst, bfirst_off, b0, kofs, method, cu_share, sys))
    return SLIDE_ERR_INVALID;
  for (int i = 0; i < n; ++i)
    if (ord_off && ord_off[i] >= 0) {      // (the j-th active border row is tile row B0 + ord[j]: inside the border)
      if (!ord) return SLIDE_ERR_INVALID;
      for (int j = 0; j < sys[i].nbr; ++j)
        if (ord[ord_off[i] + j] < 0 || ord[ord_off[i] + j] >= sys[i].nbr) return SLIDE_ERR_INVALID;
    }
  Tmp Tm;
  int Tmax = 0;
  std::vector<size_t> s_off(n + 1, 0), t_off(n + 1, 0), l_off(n + 1, 0);
  for (int i = 0; i < n; ++i) {
    CholSystem& cs = sys[i];
    const size_t T_ = cs.T, l32 = (want_l32 && cs.b0 == 0) ? T_ * (T_ - 1) / 2 * NB * NB + 4 : 0;
    s_off[i + 1] = s_off[i] + (size_t)cs.ld * T_ * NB; t_off[i + 1] = t_off[i] + T_; l_off[i + 1] = l_off[i] + l32;
    Tmax = std::max(Tmax, cs.T);
    cs.S = Tm.up(S_in + s_off[i], (size_t)cs.ld * T_ * NB);
    cs.Ld = Tm.up<double>(nullptr, T_ * NB * NB); cs.Winv = Tm.up<double>(nullptr, T_ * 1024);
    cs.yv = Tm.up<double>(nullptr, T_ * NB); cs.dp = Tm.up<double>(nullptr, T_ * NB);
    cs.status = Tm.up<int>(nullptr, 8);
    if (ord_off && ord_off[i] >= 0) cs.ord = Tm.up(ord + ord_off[i], (size_t)cs.nbr);
    if (l32) cs.L32 = Tm.up<float>(nullptr, l32);
    if (!cs.S || !cs.Ld || !cs.Winv || !cs.yv || !cs.dp || !cs.status || (ord_off && ord_off[i] >= 0 && !cs.ord) || (l32 && !cs.L32)) {
      g_last_error = "hipMalloc/hipMemcpy failed";
      return SLIDE_ERR_HIP;
    }
    SL_HIP(hipMemset(cs.status, 0, 8 * sizeof(int)));
    SL_HIP(hipMemset(cs.Ld, 0, T_ * NB * NB * sizeof(double)));
    SL_HIP(hipMemset(cs.Winv, 0, T_ * 1024 * sizeof(double)));
    if (l32) SL_HIP(hipMemsetD32(reinterpret_cast<hipDeviceptr_t>(cs.L32), 0x7fc0dead, l32));
  }
  int* d_ctr = Tm.up<int>(nullptr, (size_t)Tmax + 3);
  int* d_tick = Tm.up<int>(nullptr, CHOL_STEP_BATCH_MAX);
  if (!d_ctr || !d_tick) { g_last_error = "hipMalloc failed"; return SLIDE_ERR_HIP; }
  SL_HIP(hipMemset(d_ctr, 0, ((size_t)Tmax + 3) * sizeof(int)));
  SL_HIP(hipMemset(d_tick, 0, CHOL_STEP_BATCH_MAX * sizeof(int)));
  SL_HIP(hipDeviceSynchronize());
  std::vector<int> trace;
  int planned_cus = 0;
  {
    CholPlanHook hook(assumed_cus, false);      // (gone again before anything below can return)
    launch_chol_batch(sys.data(), n, d_ctr, nullptr, nullptr, false, cu_share, method == 2 ? d_tick : nullptr);
    trace.swap(hook.trace);
    planned_cus = assumed_cus > 0 ? assumed_cus : chol_device_cus();
  }
  if (n_launches) *n_launches = copy_trace(trace, trace_out, trace_cap);
  if (n_cu_out) *n_cu_out = planned_cus;
  SL_HIP(hipDeviceSynchronize());
  SL_HIP(hipGetLastError());
  if (method == 2) {      // (the pair kernel's counters are back at zero once its launches are through)
    int tk[CHOL_STEP_BATCH_MAX];
    SL_HIP(hipMemcpy(tk, d_tick, sizeof(tk), hipMemcpyDeviceToHost));
    for (int c = 0; c < CHOL_STEP_BATCH_MAX; ++c)
      if (tk[c] != 0) { g_last_error = "pair kernel: a ticket counter was left at " + std::to_string(tk[c]); return SLIDE_ERR_HIP; }
  }
  for (int i = 0; i < n; ++i) {
    const CholSystem& cs = sys[i];
    const size_t T_ = cs.T;
    if (S_out) SL_HIP(hipMemcpy(S_out + s_off[i], cs.S, (s_off[i + 1] - s_off[i]) * sizeof(double), hipMemcpyDeviceToHost));
    if (Ld_out) SL_HIP(hipMemcpy(Ld_out + t_off[i] * NB * NB, cs.Ld, T_ * NB * NB * sizeof(double), hipMemcpyDeviceToHost));
    if (Winv_out) SL_HIP(hipMemcpy(Winv_out + t_off[i] * 1024, cs.Winv, T_ * 1024 * sizeof(double), hipMemcpyDeviceToHost));
    if (status_out) SL_HIP(hipMemcpy(status_out + 8 * (size_t)i, cs.status, 8 * sizeof(int), hipMemcpyDeviceToHost));
    if (L32_out && cs.L32) SL_HIP(hipMemcpy(L32_out + l_off[i], cs.L32, (l_off[i + 1] - l_off[i]) * sizeof(float), hipMemcpyDeviceToHost));
  }
  return SLIDE_OK;
}

// ---- the border product and its apply on caller data (slide_gpu.h) ---------------------------------------------------------------------
// A segments' table as the kernels index it (HostGraph::seg_tab): nseg, nseg end columns, nseg x (nbr + 1) first columns, then the masks'
// head (0, or Tb >= T and Tb x (low, high) words with no bit at or above nbr).  What the kernels would read out of bounds is refused here.
static bool debug_segtab_ok(const int* st, int len, int T, int nbr) {
  if (!st || len < 2 || st[0] < 1) return false;
  const int nseg = st[0];
  const long long head = 1 + (long long)nseg + (long long)nseg * (nbr + 1);
  if (len < head + 1) return false;
  for (int q = 0; q < nseg; ++q)
    if (st[1 + q] < 0 || st[1 + q] > T) return false;
  for (long long e = 1 + nseg; e < head; ++e)
    if (st[e] < 0) return false;
  const int Tb = st[head];
  if (Tb == 0) return true;
  if (Tb < T || len < head + 1 + 2LL * Tb) return false;
  for (int c = 0; c < Tb; ++c) {
    const unsigned long long m = (unsigned long long)(unsigned)st[head + 1 + 2 * c] | ((unsigned long long)(unsigned)st[head + 2 + 2 * c] << 32);
    if (nbr < 64 && (m >> nbr)) return false;
  }
  return true;
}
// what both entries check of a system's shape (the launchers index S by it)
static bool debug_border_shape_ok(int ld, int T, int nbr, int b0) {
  if (T < 1 || nbr < 1 || nbr > 1023 || b0 < 0 || (b0 > 0 && b0 < T) || (ld & 1)) return false;
  return ld >= ((b0 > 0 ? b0 : T) + nbr + 1) * NB;
}
constexpr unsigned long long BORDER_GUARD = 0x7FF8B0DE5C4A7C11ull;      // a quiet-NaN payload in the tiles around the scratch: no partial product equals it
int slide_debug_border_product(int n, const double* S_in, const int* ld, const int* T, const int* nbr, const int* b0, const double* bord_in,
                               const int* ldb, const int* bord_cols, const int* bfirst, const int* bfirst_off, const int* segtab,
                               const int* segtab_off, const int* segtab_len, const double* bord_src, const int* has_src, const int* jobs,
                               int njobs, int lds_pad, int ks, const int* ks_sys, int jb_end, int fuse_add, int use_prefill, double prefill,
                               double* bord_out, double* S_out) {
  if (slide_device_check(-1) != SLIDE_OK) return SLIDE_ERR_HIP;
  if (n < 1 || n > CHOL_BATCH_HOST_MAX || !S_in || !ld || !T || !nbr || !bord_in || !ldb || !bord_cols || ks < 1 || ks > 64 || lds_pad < 0 || lds_pad > 65536) return SLIDE_ERR_INVALID;
  if ((jobs && njobs < 1) || (!jobs && (fuse_add || jb_end >= 0 || lds_pad > 0)) || (ks_sys && !fuse_add)) return SLIDE_ERR_INVALID;
  bool any_seg = false, any_bfirst = false;
  std::vector<size_t> s_off(n + 1, 0), b_off(n + 1, 0);
  for (int i = 0; i < n; ++i) {
    if (!debug_border_shape_ok(ld[i], T[i], nbr[i], b0 ? b0[i] : 0)) return SLIDE_ERR_INVALID;
    if ((ldb[i] & 1) || ldb[i] < (nbr[i] + 1) * NB || bord_cols[i] < nbr[i] * NB) return SLIDE_ERR_INVALID;
    if (bfirst_off && bfirst_off[i] >= 0) {
      if (!bfirst) return SLIDE_ERR_INVALID;
      for (int j = 0; j <= nbr[i]; ++j)
        if (bfirst[bfirst_off[i] + j] < 0) return SLIDE_ERR_INVALID;
      any_bfirst = true;
    }
    if (segtab_off && segtab_off[i] >= 0) {
      if (!segtab || !segtab_len || !debug_segtab_ok(segtab + segtab_off[i], segtab_len[i], T[i], nbr[i])) return SLIDE_ERR_INVALID;
      any_seg = true;
    }
    if (has_src && has_src[i] && !bord_src) return SLIDE_ERR_INVALID;
    s_off[i + 1] = s_off[i] + (size_t)ld[i] * T[i] * NB;
    b_off[i + 1] = b_off[i] + (size_t)ldb[i] * bord_cols[i];
  }
  int ka = ks, kb = ks;
  if (fuse_add) {      // (launch_border_syrk_jobs: two systems with the same border, each with its own number of chunks)
    if (n != 2 || nbr[0] != nbr[1] || any_bfirst) return SLIDE_ERR_INVALID;
    if (ks_sys) { ka = ks_sys[0]; kb = ks_sys[1]; }
    if (ka < 1 || kb < 1 || ka > 64 || kb > 64) return SLIDE_ERR_INVALID;
  }
  const int km = std::max(ka, kb);
  if (fuse_add && km < 2) return SLIDE_ERR_INVALID;      // (without scratch the launcher would run the plain table launch and add nothing)
  if (km > 1 && (any_seg || (n > 1 && !fuse_add))) return SLIDE_ERR_INVALID;
  if (jobs) {
    if (jb_end == 0 || jb_end > nbr[0]) return SLIDE_ERR_INVALID;
    for (int j = 0; j < njobs; ++j) {
      if (jobs[j] < 0 || (jobs[j] >> 20) >= n) return SLIDE_ERR_INVALID;
      if (jb_end >= 0 && km > 1 && (jobs[j] & 1023) >= jb_end) return SLIDE_ERR_INVALID;      // (a partial the reduction would never add)
    }
  }
  Tmp Tm;
  std::vector<CholSystem> sys(n, CholSystem{});
  for (int i = 0; i < n; ++i) {
    CholSystem& cs = sys[i];
    cs.ld = ld[i]; cs.T = T[i]; cs.nbr = nbr[i]; cs.b0 = b0 ? b0[i] : 0; cs.ldb = ldb[i];
    cs.S = Tm.up(S_in + s_off[i], s_off[i + 1] - s_off[i]);
    cs.bord = Tm.up(bord_in + b_off[i], b_off[i + 1] - b_off[i]);
    bool ok = cs.S && cs.bord;
    if (bfirst_off && bfirst_off[i] >= 0) { cs.bfirst = Tm.up(bfirst + bfirst_off[i], (size_t)nbr[i] + 1); ok = ok && cs.bfirst; }
    if (segtab_off && segtab_off[i] >= 0) { cs.segtab = Tm.up(segtab + segtab_off[i], (size_t)segtab_len[i]); ok = ok && cs.segtab; }
    if (has_src && has_src[i]) { cs.bord_src = Tm.up(bord_src + b_off[i], b_off[i + 1] - b_off[i]); ok = ok && cs.bord_src; }
    if (!ok) { g_last_error = "hipMalloc/hipMemcpy failed"; return SLIDE_ERR_HIP; }
  }
  int* d_jobs = jobs ? Tm.up(jobs, (size_t)njobs) : nullptr;
  if (jobs && !d_jobs) { g_last_error = "hipMalloc/hipMemcpy failed"; return SLIDE_ERR_HIP; }
  // the partial tiles, exactly as many as HostGraph allocates, between two guard tiles
  const size_t tile = (size_t)NB * NB, body = (size_t)(nbr[0] + 1) * nbr[0] * (km - 1) * (fuse_add ? 2 : 1) * tile;
  double* d_scr = nullptr;
  if (km > 1) {
    std::vector<double> h(body + 2 * tile, use_prefill ? prefill : 0.0);
    double guard;
    std::memcpy(&guard, &BORDER_GUARD, sizeof(guard));
    std::fill(h.begin(), h.begin() + tile, guard);
    std::fill(h.end() - tile, h.end(), guard);
    d_scr = Tm.up(h.data(), h.size());
    if (!d_scr) { g_last_error = "hipMalloc/hipMemcpy failed"; return SLIDE_ERR_HIP; }
  }
  SL_HIP(hipDeviceSynchronize());
  double* scratch = d_scr ? d_scr + tile : nullptr;
  if (jobs) launch_border_syrk_jobs(sys.data(), n, d_jobs, njobs, lds_pad, nullptr, scratch, ks, jb_end, fuse_add ? ks_sys : nullptr, fuse_add != 0);
  else launch_border_syrk(sys.data(), n, nullptr, scratch, ks);
  SL_HIP(hipDeviceSynchronize());
  SL_HIP(hipGetLastError());
  if (d_scr) {
    std::vector<unsigned long long> g(2 * tile);
    SL_HIP(hipMemcpy(g.data(), d_scr, tile * sizeof(double), hipMemcpyDeviceToHost));
    SL_HIP(hipMemcpy(g.data() + tile, d_scr + tile + body, tile * sizeof(double), hipMemcpyDeviceToHost));
    for (size_t e = 0; e < 2 * tile; ++e)
      if (g[e] != BORDER_GUARD) {
        g_last_error = std::string("border product: the guard tile ") + (e < tile ? "in front of" : "behind") + " the scratch was written at element " + std::to_string(e % tile);
        return SLIDE_ERR_HIP;
      }
  }
  for (int i = 0; i < n; ++i) {
    if (bord_out) SL_HIP(hipMemcpy(bord_out + b_off[i], sys[i].bord, (b_off[i + 1] - b_off[i]) * sizeof(double), hipMemcpyDeviceToHost));
    if (S_out) SL_HIP(hipMemcpy(S_out + s_off[i], sys[i].S, (s_off[i + 1] - s_off[i]) * sizeof(double), hipMemcpyDeviceToHost));
  }
  return SLIDE_OK;
}
int slide_debug_border_apply(int n, const double* S_in, const int* ld, const int* T, const int* nbr, const int* b0, const double* yv_in,
                             const double* x_loc, const int* segtab, const int* segtab_off, const int* segtab_len, double* yv_out) {
  if (slide_device_check(-1) != SLIDE_OK) return SLIDE_ERR_HIP;
  if (n < 1 || n > CHOL_BATCH_HOST_MAX || !S_in || !ld || !T || !nbr || !yv_in || !x_loc || !yv_out) return SLIDE_ERR_INVALID;
  std::vector<size_t> s_off(n + 1, 0), y_off(n + 1, 0), x_off(n + 1, 0);
  for (int i = 0; i < n; ++i) {
    if (!debug_border_shape_ok(ld[i], T[i], nbr[i], b0 ? b0[i] : 0)) return SLIDE_ERR_INVALID;
    if (segtab_off && segtab_off[i] >= 0 && (!segtab || !segtab_len || !debug_segtab_ok(segtab + segtab_off[i], segtab_len[i], T[i], nbr[i]))) return SLIDE_ERR_INVALID;
    s_off[i + 1] = s_off[i] + (size_t)ld[i] * T[i] * NB;
    y_off[i + 1] = y_off[i] + (size_t)T[i] * NB;
    x_off[i + 1] = x_off[i] + (size_t)nbr[i] * NB;
  }
  Tmp Tm;
  std::vector<CholSystem> sys(n, CholSystem{});
  std::vector<const double*> xl(n);
  for (int i = 0; i < n; ++i) {
    CholSystem& cs = sys[i];
    cs.ld = ld[i]; cs.T = T[i]; cs.nbr = nbr[i]; cs.b0 = b0 ? b0[i] : 0;
    cs.S = Tm.up(S_in + s_off[i], s_off[i + 1] - s_off[i]);
    cs.yv = Tm.up(yv_in + y_off[i], y_off[i + 1] - y_off[i]);
    xl[i] = Tm.up(x_loc + x_off[i], x_off[i + 1] - x_off[i]);
    bool ok = cs.S && cs.yv && xl[i];
    if (segtab_off && segtab_off[i] >= 0) { cs.segtab = Tm.up(segtab + segtab_off[i], (size_t)segtab_len[i]); ok = ok && cs.segtab; }
    if (!ok) { g_last_error = "hipMalloc/hipMemcpy failed"; return SLIDE_ERR_HIP; }
  }
  SL_HIP(hipDeviceSynchronize());
  launch_border_apply(sys.data(), n, xl.data(), nullptr);
  SL_HIP(hipDeviceSynchronize());
  SL_HIP(hipGetLastError());
  for (int i = 0; i < n; ++i) SL_HIP(hipMemcpy(yv_out + y_off[i], sys[i].yv, (y_off[i + 1] - y_off[i]) * sizeof(double), hipMemcpyDeviceToHost));
  return SLIDE_OK;
}

// ---- the readers of the factor on caller data (slide_gpu.h): selected inverse, many-column solves, gram, single-pose walk ---------------
// No factorisation runs here: S / Ld / Winv are the caller's, in the layout of chol_kernels.hip.
// what every entry checks of the factor's shape (the launchers index S, Ld, Winv and the profile by it)
static bool debug_factor_shape_ok(int ld, int T, const int* prof) {
  if (T < 1 || ld < T * NB || (ld & 1)) return false;
  if (prof)
    for (int k = 0; k < T; ++k)
      if (prof[k] < k || prof[k] >= T || (k > 0 && prof[k] < prof[k - 1])) return false;
  return true;
}
struct DebugFactor {
  double *S = nullptr, *Ld = nullptr, *Winv = nullptr;
  int* prof = nullptr;
  bool up(Tmp& Tm, const double* S_in, int ld, int T, const double* Ld_in, const double* Winv_in, const int* prof_in) {
    S = Tm.up(S_in, (size_t)ld * T * NB);
    Ld = Tm.up(Ld_in, (size_t)T * NB * NB);
    Winv = Tm.up(Winv_in, (size_t)T * 1024);
    if (prof_in) prof = Tm.up(prof_in, (size_t)T);
    return S && Ld && Winv && (!prof_in || prof);
  }
};
int slide_debug_selected_inverse(const double* S_in, int ld, int T, const double* Ld_in, const double* Winv_in, const int* prof, int stage,
                                 double* Sg, double* Z, double* S_out, double* Ld_out, double* Winv_out) {
  if (slide_device_check(-1) != SLIDE_OK) return SLIDE_ERR_HIP;
  if (!S_in || !Ld_in || !Winv_in || !Sg || !Z || (stage != 0 && stage != 1) || !debug_factor_shape_ok(ld, T, prof)) return SLIDE_ERR_INVALID;
  const size_t len = (size_t)ld * T * NB;
  Tmp Tm;
  DebugFactor F;
  double* dSg = Tm.up(Sg, len);
  double* dZ = Tm.up(Z, len);
  if (!F.up(Tm, S_in, ld, T, Ld_in, Winv_in, prof) || !dSg || !dZ) { g_last_error = "hipMalloc/hipMemcpy failed"; return SLIDE_ERR_HIP; }
  SL_HIP(hipDeviceSynchronize());
  if (stage == 0) launch_selected_inverse_prep(F.S, ld, T, F.Ld, F.Winv, prof, F.prof, dSg, dZ, nullptr);
  else launch_selected_inverse(F.S, ld, T, F.Ld, F.Winv, prof, F.prof, dSg, dZ, nullptr);
  SL_HIP(hipDeviceSynchronize());
  SL_HIP(hipGetLastError());
  SL_HIP(hipMemcpy(Sg, dSg, len * sizeof(double), hipMemcpyDeviceToHost));
  SL_HIP(hipMemcpy(Z, dZ, len * sizeof(double), hipMemcpyDeviceToHost));
  if (S_out) SL_HIP(hipMemcpy(S_out, F.S, len * sizeof(double), hipMemcpyDeviceToHost));
  if (Ld_out) SL_HIP(hipMemcpy(Ld_out, F.Ld, (size_t)T * NB * NB * sizeof(double), hipMemcpyDeviceToHost));
  if (Winv_out) SL_HIP(hipMemcpy(Winv_out, F.Winv, (size_t)T * 1024 * sizeof(double), hipMemcpyDeviceToHost));
  return SLIDE_OK;
}
int slide_debug_multi_solve(const double* S_in, int ld, int T, const double* Ld_in, const double* Winv_in, const int* prof, double* B, double* X,
                            int ncol_alloc, int nrhs, int mode, int k0) {
  if (slide_device_check(-1) != SLIDE_OK) return SLIDE_ERR_HIP;
  if (!S_in || !Ld_in || !Winv_in || !B || !X || (mode != 0 && mode != 1) || !debug_factor_shape_ok(ld, T, prof)) return SLIDE_ERR_INVALID;
  if (nrhs < 1 || ncol_alloc < nrhs || k0 < 0 || k0 >= T || (mode == 0 && k0 != 0)) return SLIDE_ERR_INVALID;
  const size_t len = (size_t)ncol_alloc * T * NB;
  Tmp Tm;
  DebugFactor F;
  double* dB = Tm.up(B, len);
  double* dX = Tm.up(X, len);
  if (!F.up(Tm, S_in, ld, T, Ld_in, Winv_in, nullptr) || !dB || !dX) { g_last_error = "hipMalloc/hipMemcpy failed"; return SLIDE_ERR_HIP; }
  SL_HIP(hipDeviceSynchronize());
  if (mode == 0) launch_multi_solve(F.S, ld, T, F.Ld, F.Winv, prof, dB, dX, nrhs, nullptr);
  else launch_multi_fwd(F.S, ld, T, F.Ld, F.Winv, prof, dB, dX, nrhs, nullptr, k0);
  SL_HIP(hipDeviceSynchronize());
  SL_HIP(hipGetLastError());
  SL_HIP(hipMemcpy(B, dB, len * sizeof(double), hipMemcpyDeviceToHost));
  SL_HIP(hipMemcpy(X, dX, len * sizeof(double), hipMemcpyDeviceToHost));
  return SLIDE_OK;
}
int slide_debug_gram(const double* X, long long ldx, int ncol, const int* rows, int nrows, double* M) {
  if (slide_device_check(-1) != SLIDE_OK) return SLIDE_ERR_HIP;
  if (!X || !M || ncol < 1 || nrows < 1 || ldx < 1 || (!rows && nrows > ldx)) return SLIDE_ERR_INVALID;
  if (rows)
    for (int q = 0; q < nrows; ++q)
      if (rows[q] < 0 || rows[q] >= ldx) return SLIDE_ERR_INVALID;
  const size_t mlen = (size_t)ncol * ncol + ncol;      // (one guard row behind the block)
  Tmp Tm;
  double* dX = Tm.up(X, (size_t)ldx * ncol);
  double* dM = Tm.up(M, mlen);
  int* d_rows = rows ? Tm.up(rows, (size_t)nrows) : nullptr;
  if (!dX || !dM || (rows && !d_rows)) { g_last_error = "hipMalloc/hipMemcpy failed"; return SLIDE_ERR_HIP; }
  SL_HIP(hipDeviceSynchronize());
  launch_gram(dX, (size_t)ldx, ncol, d_rows, nrows, dM, nullptr);
  SL_HIP(hipDeviceSynchronize());
  SL_HIP(hipGetLastError());
  SL_HIP(hipMemcpy(M, dM, mlen * sizeof(double), hipMemcpyDeviceToHost));
  return SLIDE_OK;
}
int slide_debug_pose_covariance(const double* S_in, int ld, int T, const double* Ld_in, const double* Winv_in, int row0, double* cov36, double* Y_out) {
  if (slide_device_check(-1) != SLIDE_OK) return SLIDE_ERR_HIP;
  if (!S_in || !Ld_in || !Winv_in || !cov36 || !debug_factor_shape_ok(ld, T, nullptr) || row0 < 0 || row0 + 6 > T * NB) return SLIDE_ERR_INVALID;
  const size_t nT = (size_t)T * NB;
  Tmp Tm;
  DebugFactor F;
  double* dY = Tm.up<double>(nullptr, 6 * nT + 36);
  if (!F.up(Tm, S_in, ld, T, Ld_in, Winv_in, nullptr) || !dY) { g_last_error = "hipMalloc/hipMemcpy failed"; return SLIDE_ERR_HIP; }
  SL_HIP(hipMemset(dY, 0, (6 * nT + 36) * sizeof(double)));      // (the six unit columns, as HostGraph::pose_covariance builds them)
  const double one = 1.0;
  for (int c = 0; c < 6; ++c) SL_HIP(hipMemcpy(dY + (size_t)c * nT + row0 + c, &one, sizeof(double), hipMemcpyHostToDevice));
  SL_HIP(hipDeviceSynchronize());
  launch_pose_covariance(F.S, ld, T, F.Ld, F.Winv, dY, row0, dY + 6 * nT, nullptr);
  SL_HIP(hipDeviceSynchronize());
  SL_HIP(hipGetLastError());
  SL_HIP(hipMemcpy(cov36, dY + 6 * nT, 36 * sizeof(double), hipMemcpyDeviceToHost));
  if (Y_out) SL_HIP(hipMemcpy(Y_out, dY, 6 * nT * sizeof(double), hipMemcpyDeviceToHost));
  return SLIDE_OK;
}
int slide_debug_joint_selected_inverse(int n, const double* S_in, const int* ld, const int* Tb, const double* B_in, const int* ldb, const int* Tc,
                                       const double* Ld_in, const double* Winv_in, const int* neg0, const int* col0, const int* lds,
                                       const int* Trow, const int* rp, int nrp, const int* rows, int nrows, const int* jobs, int njobs,
                                       const int* step_off, int nsteps, int stage, double* Sg, double* Z) {
  if (slide_device_check(-1) != SLIDE_OK) return SLIDE_ERR_HIP;
  if (n < 1 || n > 1 + JSIG_ROBOTS_MAX || !S_in || !ld || !Tb || !B_in || !ldb || !Tc || !Ld_in || !Winv_in || !neg0 || !col0 || !lds || !Trow ||
      !rp || nrp < 2 || !rows || nrows < 0 || !jobs || njobs < 1 || !step_off || nsteps < 1 || (stage != 0 && stage != 1) || !Sg || !Z)
    return SLIDE_ERR_INVALID;
  for (int e = 0; e < nrp; ++e)
    if (rp[e] < 0 || rp[e] > nrows || (e > 0 && rp[e] < rp[e - 1])) return SLIDE_ERR_INVALID;
  std::vector<size_t> s_off(n + 1, 0), b_off(n + 1, 0), t_off(n + 1, 0), g_off(n + 1, 0);
  for (int i = 0; i < n; ++i) {
    if (Tc[i] < 1 || Tb[i] < 0 || Tb[i] > Tc[i] || Trow[i] < Tc[i] || lds[i] < Trow[i] * NB || neg0[i] < 0) return SLIDE_ERR_INVALID;
    if (Tb[i] > 0 && ld[i] < Trow[i] * NB) return SLIDE_ERR_INVALID;
    if (Tc[i] > Tb[i] && ldb[i] < (Trow[i] - Tb[i]) * NB) return SLIDE_ERR_INVALID;
    if (col0[i] < 0 || col0[i] + Tc[i] + 1 > nrp) return SLIDE_ERR_INVALID;
    for (int c = 0; c < Tc[i]; ++c)      // a column's rows: below it, inside the system's tile rows, each once
      for (int q = rp[col0[i] + c]; q < rp[col0[i] + c + 1]; ++q) {
        if (rows[q] <= c || rows[q] >= Trow[i]) return SLIDE_ERR_INVALID;
        for (int p = rp[col0[i] + c]; p < q; ++p)
          if (rows[p] == rows[q]) return SLIDE_ERR_INVALID;
      }
    s_off[i + 1] = s_off[i] + (size_t)ld[i] * Tb[i] * NB;
    b_off[i + 1] = b_off[i] + (size_t)ldb[i] * (Tc[i] - Tb[i]) * NB;
    t_off[i + 1] = t_off[i] + (size_t)Tc[i];
    g_off[i + 1] = g_off[i] + (size_t)lds[i] * Trow[i] * NB;
  }
  if (step_off[0] != 0 || step_off[nsteps] != njobs) return SLIDE_ERR_INVALID;
  for (int q = 0; q < nsteps; ++q)
    if (step_off[q + 1] < step_off[q]) return SLIDE_ERR_INVALID;
  for (int j = 0; j < njobs; ++j) {
    const int sy = jobs[2 * j], k = jobs[2 * j + 1];
    if (sy < 0 || sy >= n || k < 0 || k >= Tc[sy]) return SLIDE_ERR_INVALID;
    for (int p = 0; p < j; ++p)
      if (jobs[2 * p] == sy && jobs[2 * p + 1] == k) return SLIDE_ERR_INVALID;
  }
  Tmp Tm;
  std::vector<JSinvSys> Y(n);
  for (int i = 0; i < n; ++i) {
    JSinvSys& y = Y[i];
    const size_t nb = (size_t)Tb[i], nc = (size_t)Tc[i];
    y.S = Tm.up(S_in + s_off[i], s_off[i + 1] - s_off[i]); y.ld = ld[i]; y.Tb = Tb[i];
    y.B = Tm.up(B_in + b_off[i], b_off[i + 1] - b_off[i]); y.ldb = ldb[i];
    y.Ld = Tm.up(Ld_in + t_off[i] * NB * NB, nb * NB * NB); y.Winv = Tm.up(Winv_in + t_off[i] * 1024, nb * 1024);
    y.Ld2 = Tm.up(Ld_in + (t_off[i] + nb) * NB * NB, (nc - nb) * NB * NB); y.Winv2 = Tm.up(Winv_in + (t_off[i] + nb) * 1024, (nc - nb) * 1024);
    y.neg0 = neg0[i]; y.col0 = col0[i]; y.lds = lds[i];
    y.Sg = Tm.up(Sg + g_off[i], g_off[i + 1] - g_off[i]);
    y.Z = Tm.up(Z + g_off[i], g_off[i + 1] - g_off[i]);
    if (!y.S || !y.B || !y.Ld || !y.Winv || !y.Ld2 || !y.Winv2 || !y.Sg || !y.Z) { g_last_error = "hipMalloc/hipMemcpy failed"; return SLIDE_ERR_HIP; }
  }
  std::vector<int2> hj(njobs);
  for (int j = 0; j < njobs; ++j) hj[j] = make_int2(jobs[2 * j], jobs[2 * j + 1]);
  auto nr = [&](int j) { const int b = col0[hj[j].x] + hj[j].y; return rp[b + 1] - rp[b]; };
  int max_rows = 0;
  for (int j = 0; j < njobs; ++j) max_rows = std::max(max_rows, nr(j));
  JSinvSys* d_sys = Tm.up(Y.data(), (size_t)n);
  int2* d_jobs = Tm.up(hj.data(), (size_t)njobs);
  int* d_rp = Tm.up(rp, (size_t)nrp);
  int* d_rows = Tm.up(rows, (size_t)nrows);
  if (!d_sys || !d_jobs || !d_rp || !d_rows) { g_last_error = "hipMalloc/hipMemcpy failed"; return SLIDE_ERR_HIP; }
  SL_HIP(hipDeviceSynchronize());
  launch_jsinv_prep(d_sys, d_jobs, njobs, max_rows, d_rp, d_rows, nullptr);      // (CholBatch::ensure_joint_sigma's sequence)
  if (stage == 1)
    for (int q = 0; q < nsteps; ++q) {
      int mr = 0;
      for (int j = step_off[q]; j < step_off[q + 1]; ++j) mr = std::max(mr, nr(j));
      launch_jsinv_step(d_sys, d_jobs + step_off[q], step_off[q + 1] - step_off[q], mr, d_rp, d_rows, nullptr);
    }
  SL_HIP(hipDeviceSynchronize());
  SL_HIP(hipGetLastError());
  for (int i = 0; i < n; ++i) {
    SL_HIP(hipMemcpy(Sg + g_off[i], Y[i].Sg, (g_off[i + 1] - g_off[i]) * sizeof(double), hipMemcpyDeviceToHost));
    SL_HIP(hipMemcpy(Z + g_off[i], Y[i].Z, (g_off[i + 1] - g_off[i]) * sizeof(double), hipMemcpyDeviceToHost));
  }
  return SLIDE_OK;
}

// ---- stand-alone association ------------------------------------------------------------------------

// One class through the frame kernel on caller buffers.  n_cur == 0: pure K-NN gate at `qpos` (cloud = AoS float xyz, as the caller
// holds it; split into the kernel's three streams here).  n_cur > 0: pure matcher (gate = 0): the submap is the map in the caller's
// order, as sloam::match*Models receive it; the pose is the identity so world-frame detections pass through projectModels unchanged.
static int run_single_class(int cls_kind /*0 cyl,1 cube,2 ell*/, int n_cur, const double* det_world, int det_stride,
                            const int32_t* label, int n_map, const float* cloud, const double* model, const int32_t* mlabel,
                            const double* qpos, int K, double thresh, double best_init, int label_gate, int32_t* out_sub,
                            int32_t* out_submap, int* out_k) {
  if (slide_device_check(-1) != SLIDE_OK) return SLIDE_ERR_HIP;
  const bool gate = cloud != nullptr;          // K-NN gate (slide_submap_knn) vs pure matcher (no cloud)
  if (!gate && n_cur == 0) return SLIDE_OK;
  Tmp T;
  std::vector<double> det((size_t)std::max(n_cur, 0) * (cls_kind == 0 ? 7 : 12), 0.0);
  for (int i = 0; i < n_cur; ++i) {
    if (cls_kind == 0) std::memcpy(&det[7 * (size_t)i], det_world + (size_t)det_stride * i, 7 * sizeof(double));
    else {
      double* o = &det[12 * (size_t)i];
      o[0] = o[4] = o[8] = 1.0;
      o[9] = det_world[(size_t)det_stride * i]; o[10] = det_world[(size_t)det_stride * i + 1]; o[11] = det_world[(size_t)det_stride * i + 2];
    }
  }
  double pose12[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
  if (gate) { pose12[9] = qpos[0]; pose12[10] = qpos[1]; pose12[11] = qpos[2]; }
  AssocFrameDev F[3];
  std::memset(F, 0, sizeof(F));
  AssocFrameDev& C = F[0];
  size_t lds = 0;
  if (!assoc_plan(n_map, K, gate ? 1 : 0, cls_kind == 0 ? 7 : 3, &C.Kp, &C.cached, &C.staged, &lds)) {
    g_last_error = "K-NN gate: K exceeds the on-chip sort buffer (16384 neighbours)";
    return SLIDE_ERR_CAPACITY;
  }
  C.gate = gate ? 1 : 0;
  if (gate) {
    std::vector<float> soa(3 * (size_t)std::max(n_map, 1));
    for (int i = 0; i < n_map; ++i) { soa[i] = cloud[3 * (size_t)i]; soa[(size_t)n_map + i] = cloud[3 * (size_t)i + 1]; soa[2 * (size_t)n_map + i] = cloud[3 * (size_t)i + 2]; }
    const float* d = T.up(soa.data(), soa.size());
    if (!d) { g_last_error = "hipMalloc/hipMemcpy failed"; return SLIDE_ERR_HIP; }
    C.cx = d; C.cy = d + n_map; C.cz = d + 2 * (size_t)n_map;
  }
  C.model = T.up(model, (size_t)(cls_kind == 0 ? 7 : 3) * n_map);
  C.label = T.up(mlabel, n_map);
  C.n = n_map; C.K = K; C.thresh = thresh; C.best_init = best_init; C.label_gate = label_gate; C.is_cyl = cls_kind == 0;
  C.det = T.up(det.data(), det.size());
  C.det_label = T.up(label, n_cur);
  C.n_det = n_cur;
  C.det_world = T.up<double>(nullptr, det.size());
  C.match_sub = T.up<int32_t>(nullptr, n_cur);
  C.match_map = T.up<int32_t>(nullptr, n_cur);
  C.submap = gate ? T.up<int32_t>(nullptr, std::max(std::min(K, n_map), 1)) : nullptr;
  int32_t* nsub = T.up<int32_t>(nullptr, 4);
  C.n_sub = nsub;
  F[1] = C; F[1].n_det = 0; F[1].n = 0; F[1].n_sub = nsub + 1; F[1].submap = nullptr;
  F[2] = C; F[2].n_det = 0; F[2].n = 0; F[2].n_sub = nsub + 2; F[2].submap = nullptr;
  AssocFrameDev* dF = T.up(F, 3);
  double* dpose = T.up(pose12, 12);
  if (!C.model || !C.label || !C.det || !C.det_label || !C.det_world || !C.match_sub || !C.match_map || (gate && !C.submap) ||
      !nsub || !dF || !dpose) {
    g_last_error = "hipMalloc/hipMemcpy failed";
    return SLIDE_ERR_HIP;
  }
  launch_assoc_frame(dF, lds, dpose, nullptr);
  SL_HIP(hipDeviceSynchronize());
  SL_HIP(hipGetLastError());
  int k = 0;
  SL_HIP(hipMemcpy(&k, nsub, sizeof(int), hipMemcpyDeviceToHost));
  if (out_k) *out_k = k;
  if (out_submap && k && gate) SL_HIP(hipMemcpy(out_submap, C.submap, k * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (out_sub && n_cur) SL_HIP(hipMemcpy(out_sub, C.match_sub, n_cur * sizeof(int32_t), hipMemcpyDeviceToHost));
  return SLIDE_OK;
}

int slide_submap_knn(const float* cloud_xyz, uint64_t n, const double query_xyz[3], int K, int32_t* out_idx, int* out_k) {
  if (n > (uint64_t)INT32_MAX || (n > 0 && !cloud_xyz)) return SLIDE_ERR_INVALID;
  if (n == 0) {
    if (slide_device_check(-1) != SLIDE_OK) return SLIDE_ERR_HIP;
    if (out_k) *out_k = 0;
    return SLIDE_OK;
  }
  std::vector<double> model(3 * (size_t)std::max<uint64_t>(n, 1), 0.0);
  std::vector<int32_t> lab(std::max<uint64_t>(n, 1), 0);
  return run_single_class(2, 0, nullptr, 3, nullptr, (int)n, cloud_xyz, model.data(), lab.data(), query_xyz, K, 0.0, 1000.0, 1,
                          nullptr, out_idx, out_k);
}

int slide_assoc_match_cylinders(int n_cur, const double* root, const double* ray, const int32_t* label, int n_map,
                                const double* map_root, const double* map_ray, const int32_t* map_label, double thresh,
                                int32_t* out_idx) {
  std::vector<double> det(7 * (size_t)n_cur), model(7 * (size_t)n_map);
  for (int i = 0; i < n_cur; ++i) { for (int k = 0; k < 3; ++k) { det[7 * i + k] = root[3 * i + k]; det[7 * i + 3 + k] = ray[3 * i + k]; } det[7 * i + 6] = 0; }
  for (int i = 0; i < n_map; ++i) { for (int k = 0; k < 3; ++k) { model[7 * i + k] = map_root[3 * i + k]; model[7 * i + 3 + k] = map_ray[3 * i + k]; } model[7 * i + 6] = 0; }
  const double q[3] = {0, 0, 0};
  return run_single_class(0, n_cur, det.data(), 7, label, n_map, nullptr, model.data(), map_label, q, std::max(n_map, 1), thresh,
                          thresh + 100, 2, out_idx, nullptr, nullptr);
}
int slide_assoc_match_boxes(int cls, int n_cur, const double* xyz, const int32_t* label, int n_map, const double* map_xyz,
                            const int32_t* map_label, double thresh, int32_t* out_idx) {
  if (cls != SLIDE_CLS_CUBE && cls != SLIDE_CLS_ELLIPSOID) return SLIDE_ERR_INVALID;
  const double q[3] = {0, 0, 0};
  const bool cube = cls == SLIDE_CLS_CUBE;
  return run_single_class(cube ? 1 : 2, n_cur, xyz, 3, label, n_map, nullptr, map_xyz, map_label, q, std::max(n_map, 1), thresh,
                          cube ? 30.0 : 1000.0, cube ? 0 : 1, out_idx, nullptr, nullptr);
}

int slide_assoc_sweep_batch_device(const float* d_cloud_x, const float* d_cloud_y, const float* d_cloud_z, const double* d_model_xyz,
                                   const int32_t* d_label, int n_map, const double* d_query_pos, const double* d_obs_xyz,
                                   const int32_t* d_obs_label, int n_query, int n_obs, int K, double thresh, int32_t* d_out_map_idx,
                                   void* stream) {
  if (n_query <= 0) return SLIDE_OK;
  if (n_map < 0 || n_obs < 0 || K <= 0) return SLIDE_ERR_INVALID;
  if (launch_assoc_sweep(d_cloud_x, d_cloud_y, d_cloud_z, d_model_xyz, d_label, n_map, d_query_pos, d_obs_xyz, d_obs_label, n_query,
                         n_obs, K, thresh, d_out_map_idx, (hipStream_t)stream) != 0) {
    g_last_error = "K-NN gate: K exceeds the on-chip sort buffer (16384 neighbours)";
    return SLIDE_ERR_CAPACITY;
  }
  SL_HIP(hipGetLastError());
  return SLIDE_OK;
}

// The same sweep on caller-provided HOST buffers (uploaded once, then `repeats` timed launches on resident inputs, results copied back):
// cloud_xyz is AoS float32 as the callers of slide_submap_knn hold it and is split into the kernel's three streams here.
int slide_assoc_sweep_batch(const float* cloud_xyz, const double* model_xyz, const int32_t* label, int n_map, const double* query_pos,
                            const double* obs_xyz, const int32_t* obs_label, int n_query, int n_obs, int K, double thresh,
                            int32_t* out_map_idx, int repeats, double* ms_out) {
  if (slide_device_check(-1) != SLIDE_OK) return SLIDE_ERR_HIP;
  if (n_map < 0 || n_obs < 0 || n_query < 0 || K <= 0) return SLIDE_ERR_INVALID;
  if (ms_out) *ms_out = 0.0;
  if (n_query == 0) return SLIDE_OK;
  Tmp T;
  std::vector<float> soa(3 * (size_t)std::max(n_map, 1));
  for (int i = 0; i < n_map; ++i) { soa[i] = cloud_xyz[3 * (size_t)i]; soa[(size_t)n_map + i] = cloud_xyz[3 * (size_t)i + 1]; soa[2 * (size_t)n_map + i] = cloud_xyz[3 * (size_t)i + 2]; }
  const float* dc = T.up(soa.data(), soa.size());
  const double* dm = T.up(model_xyz, 3 * (size_t)std::max(n_map, 1));
  const int32_t* dl = T.up(label, (size_t)std::max(n_map, 1));
  const double* dq = T.up(query_pos, 3 * (size_t)n_query);
  const double* dox = T.up(obs_xyz, 3 * (size_t)n_query * std::max(n_obs, 1));
  const int32_t* dol = T.up(obs_label, (size_t)n_query * std::max(n_obs, 1));
  int32_t* dout = T.up<int32_t>(nullptr, (size_t)n_query * std::max(n_obs, 1));
  if (!dc || !dm || !dl || !dq || !dox || !dol || !dout) { g_last_error = "hipMalloc/hipMemcpy failed"; return SLIDE_ERR_HIP; }
  hipEvent_t e0, e1;
  SL_HIP(hipEventCreate(&e0));
  SL_HIP(hipEventCreate(&e1));
  int rc = slide_assoc_sweep_batch_device(dc, dc + n_map, dc + 2 * (size_t)n_map, dm, dl, n_map, dq, dox, dol, n_query, n_obs, K, thresh, dout, nullptr);   // warm-up
  if (rc == SLIDE_OK) {
    SL_HIP(hipEventRecord(e0, nullptr));
    for (int r = 0; r < std::max(repeats, 1) && rc == SLIDE_OK; ++r)
      rc = slide_assoc_sweep_batch_device(dc, dc + n_map, dc + 2 * (size_t)n_map, dm, dl, n_map, dq, dox, dol, n_query, n_obs, K, thresh, dout, nullptr);
    SL_HIP(hipEventRecord(e1, nullptr));
    SL_HIP(hipEventSynchronize(e1));
    float ms = 0.f;
    SL_HIP(hipEventElapsedTime(&ms, e0, e1));
    if (ms_out) *ms_out = ms;
  }
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  if (rc != SLIDE_OK) return rc;
  SL_HIP(hipGetLastError());
  if (n_obs) SL_HIP(hipMemcpy(out_map_idx, dout, (size_t)n_query * n_obs * sizeof(int32_t), hipMemcpyDeviceToHost));
  return SLIDE_OK;
}

// ---- backend ------------------------------------------------------------------------------------------
slide_backend_t* slide_backend_create(const slide_params_t* p) {
  slide_params_t q;
  if (p) q = *p; else slide_default_params(&q);
  if (slide_device_check(q.device) != SLIDE_OK) return nullptr;
  auto* b = new slide_backend(q);
  if (b->b.init() != SLIDE_OK) { delete b; return nullptr; }
  return b;
}
void slide_backend_destroy(slide_backend_t* b) { delete b; }
#define BLOCK(B) std::lock_guard<std::mutex> lk((B)->b.g.mtx)
int slide_backend_process_frame(slide_backend_t* b, int mode, int robot, const double rel7[7], const double prev7[7],
                                const slide_detections_t* det, slide_frame_result_t* res) {
  if (!b || !det) return SLIDE_ERR_INVALID;
  BLOCK(b);
  return b->b.process_frame(mode, robot, rel7, prev7, *det, res);
}
int slide_backend_ingest_solve(slide_backend_t* b) { if (!b) return SLIDE_ERR_INVALID; BLOCK(b); return b->b.ingest_solve(); }
int slide_backend_end_frame(slide_backend_t* b, int robot, double out7[7]) { if (!b) return SLIDE_ERR_INVALID; BLOCK(b); return b->b.end_frame(robot, out7); }
int slide_backend_counts(slide_backend_t* b, uint64_t out4[4], uint64_t* pose_counters, int n_robots) {
  if (!b) return SLIDE_ERR_INVALID;
  BLOCK(b);
  int64_t st[5];
  b->b.g.stats(st);
  out4[0] = b->b.cyl_counter; out4[1] = b->b.cube_counter; out4[2] = b->b.point_counter; out4[3] = (uint64_t)st[2];
  for (int i = 0; i < n_robots && i < SLIDE_MAX_ROBOTS; ++i) pose_counters[i] = b->b.pose_counter[i];
  return SLIDE_OK;
}
int slide_backend_map_model(slide_backend_t* b, int cls, int idx, double* out, int* hits, int* label) {
  if (!b) return SLIDE_ERR_INVALID;
  BLOCK(b);
  return b->b.map_model(cls, idx, out, hits, label);
}
// The association gate of the streaming path (host_backend.hip, gate_frame): prob == 0 turns it off
int slide_backend_set_association_gate(slide_backend_t* b, double prob, int on_reject) {
  if (!b) { g_last_error = "set_association_gate: the back-end is NULL"; return SLIDE_ERR_INVALID; }
  if (!(prob >= 0.0 && prob < 1.0)) { g_last_error = "set_association_gate: prob is neither 0 (off) nor inside (0, 1)"; return SLIDE_ERR_INVALID; }
  if (on_reject != SLIDE_GATE_DROP && on_reject != SLIDE_GATE_NEW) {
    g_last_error = "set_association_gate: on_reject is neither SLIDE_GATE_DROP nor SLIDE_GATE_NEW";
    return SLIDE_ERR_INVALID;
  }
  BLOCK(b);
  return b->b.set_association_gate(prob, on_reject);
}
int slide_backend_gate_stats(slide_backend_t* b, int64_t out4[4]) {
  if (!b || !out4) { g_last_error = "gate_stats: a NULL pointer"; return SLIDE_ERR_INVALID; }
  BLOCK(b);
  for (int i = 0; i < 4; ++i) out4[i] = b->b.gate_stats[i];
  return SLIDE_OK;
}

int slide_backend_landmark_table(slide_backend_t* b, int cls, double* xyz, int32_t* label, int cap) {
  if (!b || cls < 0 || cls > 2) return SLIDE_ERR_INVALID;
  BLOCK(b);
  const uint64_t counters[3] = {b->b.cyl_counter, b->b.cube_counter, b->b.point_counter};
  const int n = (int)std::min<uint64_t>(counters[cls], (uint64_t)cap);
  for (int i = 0; i < n; ++i) {
    double v[15];
    if (b->b.g.get_landmark(cls, (uint64_t)i, v) != SLIDE_OK) return SLIDE_ERR_INVALID;
    const double* pos = cls == SLIDE_CLS_CUBE ? v + 9 : v;
    xyz[3 * i] = pos[0]; xyz[3 * i + 1] = pos[1]; xyz[3 * i + 2] = pos[2];
    label[i] = b->b.maps[cls].h_label[i];
  }
  return n;
}

// graph access of a backend: thin views that forward to the backend's own graph (no second graph object; capi_handles.hpp)
slide_graph_t* slide_backend_graph(slide_backend_t* b) { return b ? reinterpret_cast<slide_graph_t*>(&b->b.g) : nullptr; }

// GetIndexClosestPoseMstPair sloam.cpp:428-440 (strict '<': first index wins ties)
int slide_closest_stamp(const int64_t* sec, const int64_t* nsec, int n, int64_t qsec, int64_t qnsec, int* idx, double* diff) {
  *idx = -1;
  *diff = 1.7976931348623157e308;
  for (int i = 0; i < n; ++i) {
    int64_t s = sec[i] - qsec, ns = nsec[i] - qnsec;
    while (ns < 0) { ns += 1000000000LL; s -= 1; }
    while (ns >= 1000000000LL) { ns -= 1000000000LL; s += 1; }
    const double d = std::fabs((double)s + 1e-9 * (double)ns);
    if (d < *diff) { *idx = i; *diff = d; }
  }
  return SLIDE_OK;
}

// Input::PickNextMeasurementToAdd input.cpp:26-108
int slide_pick_next_measurement(const int64_t* odom_sec, const int64_t* odom_nsec, const double* odom_pose7, int n_odom,
                                const int64_t* obs_sec, const int64_t* obs_nsec, int n_obs, const int64_t* rel_sec,
                                const int64_t* rel_nsec, int n_rel, int64_t latest_sec, int64_t latest_nsec,
                                const double latest_pose7[7], double current_time, double msg_delay_tolerance,
                                float min_odom_distance, int out4[4]) {
  if (!out4 || n_odom < 0 || n_obs < 0 || n_rel < 0) return SLIDE_ERR_INVALID;
  auto before = [](int64_t as, int64_t an, int64_t bs, int64_t bn) { return as < bs || (as == bs && an < bn); };
  auto secs = [](int64_t s, int64_t n) { return (double)s + 1e-9 * (double)n; };
  int po = 0, pb = 0, pr = 0;
  while (po < n_odom && before(odom_sec[po], odom_nsec[po], latest_sec, latest_nsec)) ++po;     // :35-43
  while (pb < n_obs && before(obs_sec[pb], obs_nsec[pb], latest_sec, latest_nsec)) ++pb;
  while (pr < n_rel && before(rel_sec[pr], rel_nsec[pr], latest_sec, latest_nsec)) ++pr;
  const bool vobs = pb < n_obs && (current_time - secs(obs_sec[pb], obs_nsec[pb])) >= msg_delay_tolerance;
  const bool vrel = pr < n_rel && (current_time - secs(rel_sec[pr], rel_nsec[pr])) >= msg_delay_tolerance;
  int pick = 0;
  if (vobs && vrel) pick = before(obs_sec[pb], obs_nsec[pb], rel_sec[pr], rel_nsec[pr]) ? 2 : 3;   // the older one
  else if (vobs) pick = 2;
  else if (vrel) pick = 3;
  else {
    const SE3 L = from7(latest_pose7);
    for (int i = n_odom - 1; i >= po; --i) {                                                        // newest first, :84-104
      if ((current_time - secs(odom_sec[i], odom_nsec[i])) < msg_delay_tolerance) continue;
      const SE3 rel = compose(inverse(L), from7(odom_pose7 + 7 * (size_t)i));
      if (norm(rel.t) > (double)min_odom_distance) { pick = 1; po = i; }
      break;
    }
  }
  out4[0] = pick; out4[1] = po; out4[2] = pb; out4[3] = pr;
  return SLIDE_OK;
}

// CylinderMapManager::InLoopClosureRegion cylinderMapManager.cpp:115-160
int slide_in_loop_closure_region(const float* cloud_xyz, int n, const double pose_xyz[3], double max_dist_xy, double max_dist_z,
                                 uint64_t at_least_num_of_poses_old, int* inside) {
  if (!inside || n < 0) return SLIDE_ERR_INVALID;
  *inside = 0;
  if ((uint64_t)n < at_least_num_of_poses_old) return SLIDE_OK;
  const float qx = (float)pose_xyz[0], qy = (float)pose_xyz[1], qz = (float)pose_xyz[2];
  const double r3 = std::sqrt(max_dist_xy * max_dist_xy + max_dist_z * max_dist_z);
  const float r2 = (float)(r3 * r3);                       // pcl radiusSearch hands radius^2 to FLANN as float
  for (int i = 0; i < n; ++i) {
    const float dx = cloud_xyz[3 * i] - qx, dy = cloud_xyz[3 * i + 1] - qy, dz = cloud_xyz[3 * i + 2] - qz;
    if (!(dx * dx + dy * dy + dz * dz < r2)) continue;
    const double ex = (double)(cloud_xyz[3 * i] - qx), ey = (double)(cloud_xyz[3 * i + 1] - qy);
    if (std::sqrt(ex * ex + ey * ey) > max_dist_xy || std::fabs((double)(cloud_xyz[3 * i + 2] - qz)) > max_dist_z) continue;
    if ((uint64_t)(n - 1) - (uint64_t)i > at_least_num_of_poses_old) { *inside = 1; break; }
  }
  return SLIDE_OK;
}

// CylinderMapManager::getLoopCandidateIdx cylinderMapManager.cpp:160-184
int slide_loop_candidate_idx(const float* cloud_xyz, int n, double max_dist, uint64_t pose_idx, uint64_t at_least_num_of_poses_old,
                             uint64_t* candidate_idx, int* found) {
  if (!found || !candidate_idx || n < 0 || (n > 0 && !cloud_xyz)) return SLIDE_ERR_INVALID;
  *found = 0;
  if (n < 50) return SLIDE_OK;                                   // :163
  if (pose_idx >= (uint64_t)n) return SLIDE_ERR_INVALID;         // (the reference would index out of bounds)
  // FLANN returns the neighbours nearest first; the first one that qualifies wins = the nearest qualifying one
  // (equidistant neighbours: by index, as in the K-NN gate)
  bool have = false;
  float bd = 0.f;
  uint64_t bi = 0;
  loop_candidates(cloud_xyz, n, max_dist, pose_idx, at_least_num_of_poses_old, [&](float d2, uint64_t i) {
    if (!have || d2 < bd) { have = true; bd = d2; bi = i; }
  });
  if (have) { *candidate_idx = bi; *found = 1; }
  return SLIDE_OK;
}

// every key pose that passes getLoopCandidateIdx's test (cylinderMapManager.cpp:160-184), in slide_loop_candidate_idx's order
int slide_loop_candidate_list(const float* cloud_xyz, int n, double max_dist, uint64_t pose_idx, uint64_t at_least_num_of_poses_old,
                              uint64_t* cand_idx, int cap, int* n_found) {
  if (!n_found || n < 0 || cap < 0 || (cap > 0 && !cand_idx) || (n > 0 && !cloud_xyz)) return SLIDE_ERR_INVALID;
  *n_found = 0;
  if (n < 50) return SLIDE_OK;                                   // :163
  if (pose_idx >= (uint64_t)n) return SLIDE_ERR_INVALID;
  std::vector<std::pair<float, uint64_t>> hits;                  // (float32 squared distance, index): the sibling's order is this pair's order
  loop_candidates(cloud_xyz, n, max_dist, pose_idx, at_least_num_of_poses_old, [&](float d2, uint64_t i) { hits.emplace_back(d2, i); });
  std::stable_sort(hits.begin(), hits.end(), [](const std::pair<float, uint64_t>& a, const std::pair<float, uint64_t>& b) { return a.first < b.first; });
  *n_found = (int)hits.size();
  for (size_t i = 0; i < hits.size() && (int)i < cap; ++i) cand_idx[i] = hits[i].second;
  return SLIDE_OK;
}

int slide_delaunay_2d(const double* xy, int n, int32_t* tri_out, int cap, int* n_tri) {
  if (!n_tri || n < 0) return SLIDE_ERR_INVALID;
  const std::vector<std::array<int32_t, 3>> t = delaunay::triangulate(xy, n);
  *n_tri = (int)t.size();
  for (size_t i = 0; i < t.size() && (int)i < cap; ++i)
    for (int k = 0; k < 3; ++k) tri_out[3 * i + k] = t[i][k];
  return SLIDE_OK;
}

}  // extern "C"
