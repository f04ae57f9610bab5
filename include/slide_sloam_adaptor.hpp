// slide_sloam_adaptor.hpp — source-compatible C++ adaptor over the C-ABI of slide_gpu.h (header only, no GTSAM / Sophus / ROS).
//
// The reference calls the hot path through two classes of backend/sloam:
//   S1  SemanticFactorGraph          include/factorgraph/graph.h:70-121        (src/factorgraph/graph.cpp)
//   S2  SemanticFactorGraphWrapper   include/factorgraph/graphWrapper.h:82-134 (src/factorgraph/graphWrapper.cpp)
// The two classes below carry the SAME method names, argument order and return conventions, so that the call sites in
// graphWrapper.cpp / sloamNode.cpp compile against them after a type alias — every pose argument is a template parameter that only
// has to provide what gtsam::Pose3 / Sophus::SE3d provide at those call sites:
//     pose.translation()   -> something indexable [0..2]
//     pose.rotation().toQuaternion() / pose.unit_quaternion()  -> x(), y(), z(), w()
// (slide::Pose7 below is the plain carrier used when neither library is present, e.g. in this repository's compile test).
// Errors: the reference's bool / throw behaviour is kept — getPose() returns false + identity for an absent key (graph.cpp:290-312),
// getCylinder / getCube throw std::out_of_range like gtsam::Values::at (graph.cpp:274-280), getCentroidLandmark returns the zero
// point (graph.cpp:282-288); a device / solver failure throws slide::Error carrying slide_last_error().
#ifndef SLIDE_SLOAM_ADAPTOR_HPP_
#define SLIDE_SLOAM_ADAPTOR_HPP_

#include <algorithm>
#include <array>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "slide_gpu.h"

namespace slide {

struct Error : std::runtime_error {
  int code;
  Error(int c, const char* what) : std::runtime_error(std::string(what) + ": " + slide_last_error()), code(c) {}
  // the whole message (a fault the library reported in a status word, not through slide_last_error)
  Error(int c, const std::string& message) : std::runtime_error(message), code(c) {}
};

// tx ty tz qx qy qz qw — geometry_msgs/Pose order, T_world<-sensor (graph.h:44)
struct Pose7 {
  double v[7] = {0, 0, 0, 0, 0, 0, 1};
  struct Q { double x_, y_, z_, w_; double x() const { return x_; } double y() const { return y_; } double z() const { return z_; } double w() const { return w_; } };
  std::array<double, 3> translation() const { return {v[0], v[1], v[2]}; }
  Q unit_quaternion() const { return {v[3], v[4], v[5], v[6]}; }
};

namespace detail {
template <class T>
auto quat_of(const T& p, int) -> decltype(p.unit_quaternion()) { return p.unit_quaternion(); }                 // Sophus::SE3d, slide::Pose7
template <class T>
auto quat_of(const T& p, long) -> decltype(p.rotation().toQuaternion()) { return p.rotation().toQuaternion(); }  // gtsam::Pose3
template <class T>
void to7(const T& p, double o[7]) {
  const auto t = p.translation();
  const auto q = quat_of(p, 0);
  o[0] = t[0]; o[1] = t[1]; o[2] = t[2];
  o[3] = q.x(); o[4] = q.y(); o[5] = q.z(); o[6] = q.w();
}
template <class V>
void to3(const V& p, double o[3]) { o[0] = p[0]; o[1] = p[1]; o[2] = p[2]; }
// point of the world frame in the frame of pose7 (R^T (p - t)): graphWrapper.cpp:165-173 computes curr_pose^-1 * ellipsoid_world
inline void to_body(const double T[7], const double p[3], double o[3]) {
  const double x = T[3], y = T[4], z = T[5], w = T[6];
  const double R[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                       2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                       2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)};
  const double d[3] = {p[0] - T[0], p[1] - T[1], p[2] - T[2]};
  for (int c = 0; c < 3; ++c) o[c] = R[c] * d[0] + R[3 + c] * d[1] + R[6 + c] * d[2];
}
inline void check(int rc, const char* what) { if (rc < 0) throw Error(rc, what); }
}  // namespace detail

// Customisation point for the read-back methods that hand poses to the CALLER's types (getCurrPose, updateFactorGraphMap, ...):
// slide_assign_pose(dst, pose7) is found by argument-dependent lookup; the overload for slide::Pose7 is below, a maintainer adds
//     inline void slide_assign_pose(Sophus::SE3d& d, const double p[7]) { d = Sophus::SE3d(Eigen::Quaterniond(p[6], p[3], p[4], p[5]), {p[0], p[1], p[2]}); }
// next to the type.
inline void slide_assign_pose(Pose7& dst, const double p[7]) { for (int i = 0; i < 7; ++i) dst.v[i] = p[i]; }

// gtsam_cylinder::CylinderMeasurement / gtsam_cube::CubeMeasurement as the reference's call sites fill them
// (cylinderFactor.h:22-40, cubeFactor.h:25-44): plain aggregates here.
struct CylinderMeasurement { double root[3], ray[3], radius; };
struct CubeMeasurement { Pose7 pose; double scale[3]; };

// ---- S1 ----------------------------------------------------------------------------------------------------------------------
class SemanticFactorGraph {
 public:
  explicit SemanticFactorGraph(const slide_params_t* p = nullptr) : g_(slide_graph_create(p)), own_(true) {
    if (!g_) throw Error(SLIDE_ERR_HIP, "slide_graph_create");
  }
  explicit SemanticFactorGraph(slide_graph_t* borrowed) : g_(borrowed), own_(false) {}
  SemanticFactorGraph(const SemanticFactorGraph&) = delete;             // (the reference copy-assigns the wrapper and shares the raw ISAM2*, sloamNode.cpp:150: not reproduced)
  SemanticFactorGraph& operator=(const SemanticFactorGraph&) = delete;
  ~SemanticFactorGraph() { if (own_ && g_) slide_graph_destroy(g_); }

  template <class Pose>
  void setPriors(const Pose& pose_prior, const int& robotID) {                                          // graph.cpp:24-42
    double p[7]; detail::to7(pose_prior, p);
    detail::check(slide_graph_set_prior(g_, robotID, p), "setPriors");
  }
  template <class Pose>
  void addKeyPoseAndBetween(const size_t fromIdx, const size_t toIdx, const Pose& relativeMotion, const Pose& poseEstimate,
                            const int& robotID) {                                                      // graph.cpp:44-151
    double r[7], e[7]; detail::to7(relativeMotion, r); detail::to7(poseEstimate, e);
    detail::check(slide_graph_add_keypose_between(g_, robotID, fromIdx, toIdx, r, e), "addKeyPoseAndBetween");
  }
  template <class Pose>
  void addCylinderFactor(const size_t poseIdx, const size_t cylIdx, const Pose& pose, const CylinderMeasurement& cylinder,
                         bool alreadyExists, const int& robotID) {                                     // graph.cpp:182-196
    double p[7]; detail::to7(pose, p);
    detail::check(slide_graph_add_cylinder(g_, robotID, poseIdx, cylIdx, p, cylinder.root, cylinder.ray, cylinder.radius, alreadyExists ? 1 : 0),
                  "addCylinderFactor");
  }
  template <class Pose>
  void addCubeFactor(const size_t poseIdx, const size_t cubeIdx, const Pose& pose, const CubeMeasurement& cube_global_meas,
                     bool alreadyExists, const int& robotID) {                                         // graph.cpp:198-231
    double p[7], c[7]; detail::to7(pose, p); detail::to7(cube_global_meas.pose, c);
    detail::check(slide_graph_add_cube(g_, robotID, poseIdx, cubeIdx, p, c, cube_global_meas.scale, alreadyExists ? 1 : 0), "addCubeFactor");
  }
  template <class Point>
  void addPointLandmarkKey(const size_t ugvIdx, const Point& landmark_position) {                       // graph.cpp:153-156
    double x[3]; detail::to3(landmark_position, x);
    detail::check(slide_graph_add_point_landmark(g_, ugvIdx, x), "addPointLandmarkKey");
  }
  template <class Point>
  void addRangeBearingFactor(const size_t poseIdx, const size_t ugvIdx, const Point& bearing_measurement, const double& range_measurement,
                             const int& robotID) {                                                     // graph.cpp:158-180
    double b[3]; detail::to3(bearing_measurement, b);
    detail::check(slide_graph_add_range_bearing(g_, robotID, poseIdx, ugvIdx, b, range_measurement), "addRangeBearingFactor");
  }
  template <class Pose>
  void addLoopClosureFactor(const Pose& poseRelative, const size_t fromIdx, const size_t fromRobot, const size_t toIdx, const size_t toRobot) {
    double r[7]; detail::to7(poseRelative, r);                                                          // graph.cpp:233-245
    detail::check(slide_graph_add_loop_closure(g_, r, fromIdx, (int)fromRobot, toIdx, (int)toRobot), "addLoopClosureFactor");
  }
  template <class Pose>
  void addRelativeMeasFactor(const Pose& poseRelative, const size_t fromIdx, const size_t fromRobot, const size_t toIdx, const size_t toRobot) {
    double r[7]; detail::to7(poseRelative, r);                                                          // graph.cpp:247-258
    detail::check(slide_graph_add_relative_meas(g_, r, fromIdx, (int)fromRobot, toIdx, (int)toRobot), "addRelativeMeasFactor");
  }
  void solve() { detail::check(slide_graph_solve(g_), "solve"); }                                       // graph.cpp:260-272

  // getPose graph.cpp:290-312: false + identity when the key is absent
  bool getPose(const size_t idx, const int& robotID, Pose7& out) const {
    const int rc = slide_graph_get_pose(g_, robotID, idx, out.v);
    detail::check(rc, "getPose");
    return rc == SLIDE_OK;
  }
  CylinderMeasurement getCylinder(const int idx) const {                                                // graph.cpp:274-276 (Values::at throws)
    double o[15];
    const int rc = slide_graph_get_landmark(g_, SLIDE_CLS_CYLINDER, (uint64_t)idx, o);
    detail::check(rc, "getCylinder");
    if (rc == SLIDE_MISSING) throw std::out_of_range("getCylinder: key not in the graph");
    return CylinderMeasurement{{o[0], o[1], o[2]}, {o[3], o[4], o[5]}, o[6]};
  }
  // getCube graph.cpp:278-280: out15 = R row-major (9), t (3), scale (3)
  std::array<double, 15> getCube(const int idx) const {
    std::array<double, 15> o{};
    const int rc = slide_graph_get_landmark(g_, SLIDE_CLS_CUBE, (uint64_t)idx, o.data());
    detail::check(rc, "getCube");
    if (rc == SLIDE_MISSING) throw std::out_of_range("getCube: key not in the graph");
    return o;
  }
  std::array<double, 3> getCentroidLandmark(const int idx) const {                                      // graph.cpp:282-288 (zero point when absent)
    double o[15] = {0};
    detail::check(slide_graph_get_landmark(g_, SLIDE_CLS_ELLIPSOID, (uint64_t)idx, o), "getCentroidLandmark");
    return {o[0], o[1], o[2]};
  }
  std::array<double, 36> getPoseCovariance(const int idx, const int& robotID) const {                   // graph.cpp:314-323, row-major 6x6 [rot, trans]
    std::array<double, 36> c{};
    detail::check(slide_graph_get_pose_covariance(g_, robotID, (uint64_t)idx, c.data()), "getPoseCovariance");
    return c;
  }
  // ---- the dormant active-SLAM API (graph.h:106-115; bodies commented out in graph.cpp:421-625) ----------------------------------
  // logEntropy (graph.cpp:423-466) without its log file: the sums of the marginal-covariance traces of the robot's poses X(i) and of
  // the point landmarks U(i), and how many of each were summed
  struct EntropyTerms { double sum_entropy_pose, sum_entropy_landmark; size_t num_valid_poses, num_valid_landmarks; };
  EntropyTerms logEntropy(const int& robotID = 0) const {
    double o[4];
    detail::check(slide_graph_marginal_traces(g_, robotID, o), "logEntropy");
    return EntropyTerms{o[0], o[1], (size_t)o[2], (size_t)o[3]};
  }
  // estimateClosureInfoGain (graph.cpp:469-623): 10 * info_gain_pose + info_gain_landmark of Between factors along the candidate
  // trajectory (noise noise_model_pose_vec_per_m * travel distance); the graph is left as it was
  double estimateClosureInfoGain(const std::vector<size_t>& candidateTrajPoseIndices, const std::vector<double>& travel_distances,
                                 const int& robotID = 0) const {
    if (candidateTrajPoseIndices.size() != travel_distances.size() + 1)
      throw Error(SLIDE_ERR_INVALID, "estimateClosureInfoGain: one travel distance per step of the trajectory");
    std::vector<uint64_t> traj(candidateTrajPoseIndices.begin(), candidateTrajPoseIndices.end());
    double o[3];
    if (!noise_model_pose_vec_per_m.empty() && noise_model_pose_vec_per_m.size() != 6)
      throw Error(SLIDE_ERR_INVALID, "estimateClosureInfoGain: noise_model_pose_vec_per_m has six entries");
    const int rc = slide_graph_closure_info_gain(g_, robotID, traj.data(), (int)traj.size(), travel_distances.data(),
                                                 noise_model_pose_vec_per_m.empty() ? nullptr : noise_model_pose_vec_per_m.data(), o);
    detail::check(rc, "estimateClosureInfoGain");
    if (rc == SLIDE_MISSING) throw std::out_of_range("estimateClosureInfoGain: trajectory pose not in the graph");
    return o[0];
  }
  // estimateClosureInfoGain for a list of candidates, ranked in one call (slide_graph_closure_info_gain_batch): one value per
  // candidate, 10 * info_gain_pose + info_gain_landmark as above, each candidate evaluated alone; throws as estimateClosureInfoGain
  // does, for the first candidate with a fault
  std::vector<double> estimateClosureInfoGains(const std::vector<std::vector<size_t>>& candidateTrajPoseIndices,
                                               const std::vector<std::vector<double>>& travel_distances, const int& robotID = 0) const {
    if (candidateTrajPoseIndices.size() != travel_distances.size())
      throw Error(SLIDE_ERR_INVALID, "estimateClosureInfoGains: one list of travel distances per candidate");
    if (!noise_model_pose_vec_per_m.empty() && noise_model_pose_vec_per_m.size() != 6)
      throw Error(SLIDE_ERR_INVALID, "estimateClosureInfoGains: noise_model_pose_vec_per_m has six entries");
    const size_t n = candidateTrajPoseIndices.size();
    std::vector<int32_t> off(n + 1, 0), status(n, 0);
    std::vector<uint64_t> traj;
    std::vector<double> travel;
    for (size_t k = 0; k < n; ++k) {
      const std::vector<size_t>& t = candidateTrajPoseIndices[k];
      if (t.size() != travel_distances[k].size() + 1)
        throw Error(SLIDE_ERR_INVALID, "estimateClosureInfoGains: one travel distance per step of the trajectory");
      traj.insert(traj.end(), t.begin(), t.end());
      travel.insert(travel.end(), travel_distances[k].begin(), travel_distances[k].end());
      travel.push_back(0.0);                        // (parallel to traj: a candidate's last entry is not read)
      off[k + 1] = (int32_t)traj.size();
    }
    std::vector<double> o(3 * n, 0.0), gains(n, 0.0);
    detail::check(slide_graph_closure_info_gain_batch(g_, robotID, (int)n, off.data(), traj.data(), travel.data(),
                                                      noise_model_pose_vec_per_m.empty() ? nullptr : noise_model_pose_vec_per_m.data(),
                                                      o.data(), status.data()),
                  "estimateClosureInfoGains");
    for (size_t k = 0; k < n; ++k) {
      if (status[k] == SLIDE_MISSING) throw std::out_of_range("estimateClosureInfoGains: trajectory pose not in the graph");
      if (status[k] != SLIDE_OK)
        throw Error(status[k], "estimateClosureInfoGains: candidate " + std::to_string(k) + ": " +
                                   (status[k] == SLIDE_ERR_CAPACITY  ? "more than SLIDE_INFO_GAIN_MAX_STEPS steps"
                                    : status[k] == SLIDE_ERR_NOT_SPD ? "I + J Sigma J^T is not positive definite"
                                                                     : "fewer than two poses or a travel distance <= 0"));
      gains[k] = o[3 * k];
    }
    return gains;
  }
  // graph.h:115 (never set in the reference): empty = the graph's own noise_model_odom_vec, else six sigmas per metre
  std::vector<double> noise_model_pose_vec_per_m;

  // The mutually consistent subset of a list of loop closures (slide_graph_select_closures; no counterpart in the reference, which
  // adds the first closure that passes straight into the graph, sloamNode.cpp:448-476): what addLoopClosureFactor takes, as vectors,
  // plus each closure's own six sigmas [rot, trans]; keep[k] = closure k belongs to the consistent set of its robot pair.  Call it
  // after solve() and before the closures are added; the graph is only read.  A closure naming a pose the graph does not hold is
  // not kept (status, when given, holds SLIDE_MISSING for it).  params = nullptr: slide_closure_default_params.
  template <class Pose>
  std::vector<bool> selectConsistentClosures(const std::vector<Pose>& posesRelative, const std::vector<size_t>& fromIdx,
                                             const std::vector<size_t>& fromRobot, const std::vector<size_t>& toIdx,
                                             const std::vector<size_t>& toRobot, const std::vector<std::array<double, 6>>& sigmas,
                                             const slide_closure_params_t* params = nullptr, std::vector<int32_t>* status = nullptr) const {
    const size_t n = posesRelative.size();
    if (fromIdx.size() != n || fromRobot.size() != n || toIdx.size() != n || toRobot.size() != n || sigmas.size() != n)
      throw Error(SLIDE_ERR_INVALID, std::string("selectConsistentClosures: one entry per closure in every vector"));
    std::vector<double> rel(7 * n + 1), sg(6 * n + 1);
    std::vector<int32_t> fr(n + 1), tr(n + 1), keep(n + 1, 0), st(n + 1, 0);
    std::vector<uint64_t> fi(n + 1), ti(n + 1);
    for (size_t k = 0; k < n; ++k) {
      detail::to7(posesRelative[k], rel.data() + 7 * k);
      for (int c = 0; c < 6; ++c) sg[6 * k + c] = sigmas[k][c];
      fr[k] = (int32_t)fromRobot[k]; tr[k] = (int32_t)toRobot[k]; fi[k] = fromIdx[k]; ti[k] = toIdx[k];
    }
    int n_groups = 0;
    detail::check(slide_graph_select_closures(g_, (int)n, fr.data(), fi.data(), tr.data(), ti.data(), rel.data(), sg.data(), params, nullptr,
                                              keep.data(), nullptr, st.data(), nullptr, nullptr, &n_groups),
                  "selectConsistentClosures");
    if (status) status->assign(st.begin(), st.begin() + n);
    std::vector<bool> out(n);
    for (size_t k = 0; k < n; ++k) out[k] = keep[k] != 0;
    return out;
  }

  // Marginals::jointMarginalCovariance of two poses (slide_graph_get_pose_pair_covariances): the 12 x 12 block
  // [[Saa, Sab], [Sba, Sbb]], pose a's six coordinates then pose b's, tangent order [rot, trans].  Mat12: anything written through
  // m(r, c) that default-constructs to 12 x 12 (Eigen::Matrix<double, 12, 12>); the plain form returns it row-major.  Throws
  // std::out_of_range for a pose the graph does not hold, Error for one pose named twice.
  std::array<double, 144> jointPoseCovariance(const size_t idxA, const size_t robotA, const size_t idxB, const size_t robotB) const {
    std::array<double, 144> c{};
    const int32_t ra = (int32_t)robotA, rb = (int32_t)robotB;
    const uint64_t ia = idxA, ib = idxB;
    int32_t st = SLIDE_OK;
    detail::check(slide_graph_get_pose_pair_covariances(g_, 1, &ra, &ia, &rb, &ib, c.data(), &st), "jointPoseCovariance");
    if (st == SLIDE_MISSING) throw std::out_of_range("jointPoseCovariance: pose not in the graph");
    if (st != SLIDE_OK) throw Error(st, std::string("jointPoseCovariance: both ends are the same pose"));
    return c;
  }
  template <class Mat12>
  Mat12 jointPoseCovariance(const size_t idxA, const size_t robotA, const size_t idxB, const size_t robotB) const {
    const std::array<double, 144> c = jointPoseCovariance(idxA, robotA, idxB, robotB);
    Mat12 m;
    for (int r = 0; r < 12; ++r)
      for (int q = 0; q < 12; ++q) m(r, q) = c[12 * r + q];
    return m;
  }
  // The individual-compatibility gate of a list of loop closures (slide_graph_closure_mahalanobis), over the vectors
  // selectConsistentClosures takes: d2[k] = r^T (I + A Sigma A^T)^-1 r of closure k against the graph as it stands, chi-square with 6
  // degrees of freedom for a true closure — compare it with 16.81; no threshold is applied here.  Call it after solve() and before the
  // closures are added; the graph is only read.  A closure with a fault of its own (status, when given: SLIDE_MISSING,
  // SLIDE_ERR_INVALID for from == to, SLIDE_ERR_NOT_SPD) has d2 = 0: read the status before the value.
  template <class Pose>
  std::vector<double> closureMahalanobis(const std::vector<Pose>& posesRelative, const std::vector<size_t>& fromIdx,
                                         const std::vector<size_t>& fromRobot, const std::vector<size_t>& toIdx,
                                         const std::vector<size_t>& toRobot, const std::vector<std::array<double, 6>>& sigmas,
                                         std::vector<int32_t>* status = nullptr) const {
    const size_t n = posesRelative.size();
    if (fromIdx.size() != n || fromRobot.size() != n || toIdx.size() != n || toRobot.size() != n || sigmas.size() != n)
      throw Error(SLIDE_ERR_INVALID, std::string("closureMahalanobis: one entry per closure in every vector"));
    std::vector<double> rel(7 * n + 1), sg(6 * n + 1), d2(n + 1, 0.0);
    std::vector<int32_t> fr(n + 1), tr(n + 1), st(n + 1, 0);
    std::vector<uint64_t> fi(n + 1), ti(n + 1);
    for (size_t k = 0; k < n; ++k) {
      detail::to7(posesRelative[k], rel.data() + 7 * k);
      for (int c = 0; c < 6; ++c) sg[6 * k + c] = sigmas[k][c];
      fr[k] = (int32_t)fromRobot[k]; tr[k] = (int32_t)toRobot[k]; fi[k] = fromIdx[k]; ti[k] = toIdx[k];
    }
    detail::check(slide_graph_closure_mahalanobis(g_, (int)n, fr.data(), fi.data(), tr.data(), ti.data(), rel.data(), sg.data(), d2.data(),
                                                  nullptr, nullptr, st.data()),
                  "closureMahalanobis");
    if (status) status->assign(st.begin(), st.begin() + n);
    d2.resize(n);
    return d2;
  }
  // The individual-compatibility gate of candidate landmark observations (slide_graph_observation_mahalanobis; no counterpart in the
  // reference, whose association tests a Euclidean distance only, sloam.cpp:73-203).  A candidate holds what addRangeBearingFactor /
  // addCubeFactor / addCylinderFactor would be given for an EXISTING landmark; build it with the three makers.  d2[k] = r^T C^-1 r of
  // candidate k against the graph as it stands, chi-square with dof[k] = 3 / 9 / 7 degrees of freedom for a true match — compare it
  // with 11.345 / 21.666 / 18.475; no threshold is applied here.  Call it after solve() and before the observations are added; the
  // graph is only read.  A candidate with a fault of its own (status, when given: SLIDE_MISSING, SLIDE_ERR_NOT_SPD) has d2 = 0: read
  // the status before the value.
  struct ObservationCandidate { int cls = SLIDE_CLS_ELLIPSOID; size_t robot = 0, poseIdx = 0, lmIdx = 0; std::array<double, 17> meas{}; };
  template <class Point>
  static ObservationCandidate pointCandidate(const size_t poseIdx, const size_t ugvIdx, const Point& bearing_measurement,
                                             const double& range_measurement, const int& robotID) {
    ObservationCandidate c;
    c.cls = SLIDE_CLS_ELLIPSOID; c.robot = (size_t)robotID; c.poseIdx = poseIdx; c.lmIdx = ugvIdx;
    detail::to3(bearing_measurement, c.meas.data());
    c.meas[3] = range_measurement;
    return c;
  }
  template <class Pose>
  static ObservationCandidate cubeCandidate(const size_t poseIdx, const size_t cubeIdx, const Pose& pose, const CubeMeasurement& cube_global_meas,
                                            const int& robotID) {
    ObservationCandidate c;
    c.cls = SLIDE_CLS_CUBE; c.robot = (size_t)robotID; c.poseIdx = poseIdx; c.lmIdx = cubeIdx;
    detail::to7(pose, c.meas.data());
    detail::to7(cube_global_meas.pose, c.meas.data() + 7);
    for (int i = 0; i < 3; ++i) c.meas[14 + i] = cube_global_meas.scale[i];
    return c;
  }
  template <class Pose>
  static ObservationCandidate cylinderCandidate(const size_t poseIdx, const size_t cylIdx, const Pose& pose, const CylinderMeasurement& cylinder,
                                                const int& robotID) {
    ObservationCandidate c;
    c.cls = SLIDE_CLS_CYLINDER; c.robot = (size_t)robotID; c.poseIdx = poseIdx; c.lmIdx = cylIdx;
    detail::to7(pose, c.meas.data());
    for (int i = 0; i < 3; ++i) { c.meas[7 + i] = cylinder.root[i]; c.meas[10 + i] = cylinder.ray[i]; }
    c.meas[13] = cylinder.radius;
    return c;
  }
  std::vector<double> observationMahalanobis(const std::vector<ObservationCandidate>& candidates, std::vector<int32_t>* dof = nullptr,
                                             std::vector<int32_t>* status = nullptr) const {
    const size_t n = candidates.size();
    std::vector<double> meas(17 * n + 1), d2(n + 1, 0.0);
    std::vector<int32_t> rb(n + 1), cls(n + 1), df(n + 1, 0), st(n + 1, 0);
    std::vector<uint64_t> pi(n + 1), li(n + 1);
    for (size_t k = 0; k < n; ++k) {
      const ObservationCandidate& c = candidates[k];
      rb[k] = (int32_t)c.robot; cls[k] = (int32_t)c.cls; pi[k] = c.poseIdx; li[k] = c.lmIdx;
      for (int i = 0; i < 17; ++i) meas[17 * k + i] = c.meas[i];
    }
    detail::check(slide_graph_observation_mahalanobis(g_, (int)n, rb.data(), pi.data(), cls.data(), li.data(), meas.data(), d2.data(), df.data(),
                                                      nullptr, nullptr, st.data()),
                  "observationMahalanobis");
    if (dof) dof->assign(df.begin(), df.begin() + n);
    if (status) status->assign(st.begin(), st.begin() + n);
    d2.resize(n);
    return d2;
  }
  // The same gate at a PREDICTED pose (slide_graph_predicted_observation_mahalanobis; no counterpart in the reference, which matches
  // at poseEstimate = prevKeyPose * relativeMotion on a Euclidean threshold alone): "is this match compatible, before I add it".
  // predictedPose is the value addKeyPoseAndBetween(fromIdx, fromIdx + 1, relativeMotion, predictedPose, robotID) would give the new
  // pose; neither it nor anything else is added.  The candidates are observationMahalanobis's, their robot and poseIdx fields ignored:
  // every one sits at the predicted pose.  d2[k] is what observationMahalanobis would return on the graph extended by the pose and
  // its Between factor.  Returns false, d2 untouched, when the graph does not hold the from pose (SLIDE_MISSING).
  template <class Pose>
  bool predictedObservationMahalanobis(const size_t fromIdx, const Pose& relativeMotion, const Pose& predictedPose, const int& robotID,
                                       const std::vector<ObservationCandidate>& candidates, std::vector<double>& d2,
                                       std::vector<int32_t>* dof = nullptr, std::vector<int32_t>* status = nullptr) const {
    const size_t n = candidates.size();
    double r[7], p[7]; detail::to7(relativeMotion, r); detail::to7(predictedPose, p);
    std::vector<double> meas(17 * n + 1), out(n + 1, 0.0);
    std::vector<int32_t> cls(n + 1), df(n + 1, 0), st(n + 1, 0);
    std::vector<uint64_t> li(n + 1);
    for (size_t k = 0; k < n; ++k) {
      const ObservationCandidate& c = candidates[k];
      cls[k] = (int32_t)c.cls; li[k] = c.lmIdx;
      for (int i = 0; i < 17; ++i) meas[17 * k + i] = c.meas[i];
    }
    const int rc = slide_graph_predicted_observation_mahalanobis(g_, robotID, fromIdx, r, p, (int)n, cls.data(), li.data(), meas.data(), out.data(),
                                                                 df.data(), nullptr, nullptr, st.data());
    detail::check(rc, "predictedObservationMahalanobis");
    if (rc == SLIDE_MISSING) return false;
    if (dof) dof->assign(df.begin(), df.begin() + n);
    if (status) status->assign(st.begin(), st.begin() + n);
    d2.assign(out.begin(), out.begin() + n);
    return true;
  }
  // Duplicate landmarks: are landmarks a and b of one class the same object mapped twice (slide_graph_landmark_pair_mahalanobis; no
  // counterpart in the reference, whose association never compares two landmarks of the map)?  cls: SLIDE_CLS_ELLIPSOID (sigma: 3
  // entries) or SLIDE_CLS_CYLINDER (7, tangent order [ray, root, radius]); cubes are refused.  d2[k] = r^T C^-1 r of pair k with
  // r = (b - a) / sigma and C = I + diag(1 / sigma) (Saa + Sbb - Sab - Sba) diag(1 / sigma), chi-square with 3 / 7 degrees of freedom
  // for one object — compare it with 11.345 / 18.475; no threshold is applied here.  Call it after solve(); the graph is only read.
  // A pair with a fault of its own (status, when given: SLIDE_MISSING, SLIDE_ERR_INVALID for a == b, SLIDE_ERR_NOT_SPD) has d2 = 0:
  // read the status before the value.  route, when given: 0 read off the selected inverse, 1 forward substitution.
  struct LandmarkPair { size_t a = 0, b = 0; };
  std::vector<double> landmarkPairMahalanobis(const int cls, const std::vector<LandmarkPair>& pairs, const std::vector<double>& sigma,
                                              std::vector<int32_t>* status = nullptr, std::vector<int32_t>* route = nullptr) const {
    const size_t n = pairs.size(), D = cls == SLIDE_CLS_CYLINDER ? 7 : 3;
    if (sigma.size() != D) throw Error(SLIDE_ERR_INVALID, std::string("landmarkPairMahalanobis: sigma takes one entry per tangent coordinate"));
    std::vector<double> d2(n + 1, 0.0);
    std::vector<int32_t> c(n + 1, (int32_t)cls), st(n + 1, 0), rt(n + 1, 0);
    std::vector<uint64_t> ia(n + 1, 0), ib(n + 1, 0);
    for (size_t k = 0; k < n; ++k) { ia[k] = pairs[k].a; ib[k] = pairs[k].b; }
    detail::check(slide_graph_landmark_pair_mahalanobis(g_, (int)n, c.data(), ia.data(), ib.data(), sigma.data(), sigma.data(), d2.data(), nullptr,
                                                        nullptr, nullptr, rt.data(), st.data()),
                  "landmarkPairMahalanobis");
    if (status) status->assign(st.begin(), st.begin() + n);
    if (route) route->assign(rt.begin(), rt.begin() + n);
    d2.resize(n);
    return d2;
  }
  // Marginals::jointMarginalCovariance of two landmarks of one class (slide_graph_get_landmark_pair_covariances): the 2 D x 2 D block
  // [[Saa, Sab], [Sba, Sbb]] row-major, D = 3 / 9 / 7 for ellipsoids / cubes / cylinders, tangent order of the landmark covariances.
  // Throws std::out_of_range for a landmark the graph does not hold, Error for one landmark named twice.
  std::vector<double> jointLandmarkCovariance(const int cls, const size_t idxA, const size_t idxB) const {
    const int D = cls == SLIDE_CLS_CYLINDER ? 7 : cls == SLIDE_CLS_CUBE ? 9 : 3;
    std::array<double, 324> c{};
    const int32_t cl = (int32_t)cls;
    const uint64_t ia = idxA, ib = idxB;
    int32_t st = SLIDE_OK;
    detail::check(slide_graph_get_landmark_pair_covariances(g_, 1, &cl, &ia, &ib, c.data(), nullptr, &st), "jointLandmarkCovariance");
    if (st == SLIDE_MISSING) throw std::out_of_range("jointLandmarkCovariance: landmark not in the graph");
    if (st != SLIDE_OK) throw Error(st, std::string("jointLandmarkCovariance: both ends are the same landmark"));
    std::vector<double> out((size_t)(4 * D * D));
    for (int r = 0; r < 2 * D; ++r)
      for (int q = 0; q < 2 * D; ++q) out[(size_t)(2 * D * r + q)] = c[(size_t)(18 * r + q)];
    return out;
  }
  // The search and the test together: the pairs of landmarks of class cls whose anchors lie within radius
  // (slide_graph_landmark_pairs_within over every landmark of the class) and that pass the test at the prob quantile of chi-square.
  struct DuplicateLandmark { size_t a = 0, b = 0; double d2 = 0.0, dist = 0.0; };
  std::vector<DuplicateLandmark> findDuplicateLandmarks(const int cls, const double radius, const std::vector<double>& sigma,
                                                        const double prob = 0.99) const {
    int64_t total = 0;
    std::vector<uint64_t> ia(1), ib(1);
    std::vector<double> dist(1);
    int rc = slide_graph_landmark_pairs_within(g_, cls, radius, 0, nullptr, nullptr, 0, ia.data(), ib.data(), dist.data(), &total);
    if (rc == SLIDE_ERR_CAPACITY) {      // (the first call counted)
      ia.resize((size_t)total); ib.resize((size_t)total); dist.resize((size_t)total);
      rc = slide_graph_landmark_pairs_within(g_, cls, radius, 0, nullptr, nullptr, total, ia.data(), ib.data(), dist.data(), &total);
    }
    detail::check(rc, "findDuplicateLandmarks");
    std::vector<LandmarkPair> pairs((size_t)total);
    for (size_t k = 0; k < pairs.size(); ++k) { pairs[k].a = (size_t)ia[k]; pairs[k].b = (size_t)ib[k]; }
    std::vector<int32_t> st;
    const std::vector<double> d2 = landmarkPairMahalanobis(cls, pairs, sigma, &st);
    double q = 0.0;
    detail::check(slide_chi2_quantile(prob, cls == SLIDE_CLS_CYLINDER ? 7 : 3, &q), "findDuplicateLandmarks");
    std::vector<DuplicateLandmark> out;
    for (size_t k = 0; k < pairs.size(); ++k)
      if (st[k] == SLIDE_OK && d2[k] <= q) out.push_back(DuplicateLandmark{pairs[k].a, pairs[k].b, d2[k], dist[k]});
    return out;
  }
  // Acting on the duplicates: merge landmark `drop` into landmark `keep` of one class (slide_graph_merge_landmarks; no counterpart in
  // the reference — GTSAM users call removeFactorIndices and add the factors again rekeyed).  Every factor of drop becomes a factor
  // of keep, the dropped key stays an alias of the survivor (getLandmark, later observations), pairs are applied in order and a
  // dropped key stands for its survivor.  fuse (points and cylinders; call it after solve()): the survivor takes the
  // information-weighted mean (sum H_i)^-1 sum H_i est_i of its cluster, else it keeps its estimate.  Per pair: into (the key it
  // resolves to), moved (factors re-pointed), status (SLIDE_MISSING, SLIDE_ERR_INVALID for keep == drop, SLIDE_ERR_NOT_SPD for a
  // failed fusion).  The next solve() is a full update; the marginal queries refuse until it ran.  A node would call it after a
  // solve and before the next frame.
  struct LandmarkMerge { size_t keep = 0, drop = 0; };
  struct MergeResult { std::vector<size_t> into; std::vector<int32_t> moved, status; };
  MergeResult mergeLandmarks(const int cls, const std::vector<LandmarkMerge>& pairs, const bool fuse = true) {
    const size_t n = pairs.size();
    std::vector<int32_t> c(n + 1, (int32_t)cls), mv(n + 1, 0), st(n + 1, 0);
    std::vector<uint64_t> keep(n + 1, 0), drop(n + 1, 0), into(n + 1, 0);
    for (size_t k = 0; k < n; ++k) { keep[k] = pairs[k].keep; drop[k] = pairs[k].drop; }
    detail::check(slide_graph_merge_landmarks(g_, (int)n, c.data(), keep.data(), drop.data(), fuse ? 1 : 0, into.data(), mv.data(), st.data()),
                  "mergeLandmarks");
    MergeResult out;
    out.into.assign(into.begin(), into.begin() + n);
    out.moved.assign(mv.begin(), mv.begin() + n);
    out.status.assign(st.begin(), st.begin() + n);
    return out;
  }
  // The key a landmark resolves to: itself unless mergeLandmarks dropped it, then its survivor's.  Throws std::out_of_range for a
  // landmark the graph does not know.
  size_t landmarkAlias(const int cls, const size_t idx) const {
    uint64_t into = 0;
    const int rc = slide_graph_landmark_alias(g_, cls, idx, &into);
    if (rc == SLIDE_MISSING) throw std::out_of_range("landmarkAlias: landmark not in the graph");
    detail::check(rc, "landmarkAlias");
    return (size_t)into;
  }
  // findDuplicateLandmarks, the clusters of its pairs (union-find; a cluster's smallest key survives), mergeLandmarks.  Returns the
  // (keep, drop) rows it merged, sorted; result (when given): mergeLandmarks' per-row outputs.
  std::vector<LandmarkMerge> mergeDuplicateLandmarks(const int cls, const double radius, const std::vector<double>& sigma, const double prob = 0.99,
                                                     const bool fuse = true, MergeResult* result = nullptr) {
    const std::vector<DuplicateLandmark> dup = findDuplicateLandmarks(cls, radius, sigma, prob);
    std::vector<std::pair<size_t, size_t>> parent;      // (key, parent key), sorted by key
    for (const DuplicateLandmark& d : dup) { parent.emplace_back(d.a, d.a); parent.emplace_back(d.b, d.b); }
    std::sort(parent.begin(), parent.end());
    parent.erase(std::unique(parent.begin(), parent.end()), parent.end());
    auto slot = [&](size_t key) { return (size_t)(std::lower_bound(parent.begin(), parent.end(), std::make_pair(key, (size_t)0)) - parent.begin()); };
    auto find = [&](size_t key) {
      while (parent[slot(key)].second != key) key = parent[slot(key)].second;
      return key;
    };
    for (const DuplicateLandmark& d : dup) {
      const size_t ra = find(d.a), rb = find(d.b);
      if (ra != rb) parent[slot(std::max(ra, rb))].second = std::min(ra, rb);
    }
    std::vector<LandmarkMerge> rows;
    for (const auto& kv : parent)
      if (find(kv.first) != kv.first) rows.push_back(LandmarkMerge{find(kv.first), kv.first});
    std::sort(rows.begin(), rows.end(), [](const LandmarkMerge& x, const LandmarkMerge& y) { return x.keep != y.keep ? x.keep < y.keep : x.drop < y.drop; });
    const MergeResult res = mergeLandmarks(cls, rows, fuse);
    if (result) *result = res;
    return rows;
  }
  // The joint compatibility of a key frame's matches, tested together (slide_graph_observation_joint_compatibility; no counterpart in
  // the reference): groups[g] is one hypothesis, its candidates tried in the given order.  A candidate is accepted iff it passes alone
  // (d2Single against the prob quantile of its own rows) and stacked on those accepted before it (d2Joint against the quantile of
  // dofJoint); prob == 0 evaluates only.  The per-candidate vectors run over the groups' candidates in order (group g starts at
  // groupPtr[g]); groupD2 / groupDof / groupCount describe each group's accepted set.  status: SLIDE_MISSING (skipped),
  // SLIDE_ERR_NOT_SPD (rejected); groupStatus: SLIDE_ERR_INVALID (a landmark named twice), SLIDE_ERR_CAPACITY (more than
  // SLIDE_INFO_GAIN_SWEEP_COLS rows), zeros in the group then.  The graph is only read.
  struct JointCompatibility {
    std::vector<int32_t> groupPtr, accepted, dofJoint, status, groupDof, groupCount, groupStatus;
    std::vector<double> d2Single, d2Joint, groupD2;
  };
  JointCompatibility observationJointCompatibility(const std::vector<std::vector<ObservationCandidate>>& groups, double prob = 0.99) const {
    const size_t ng = groups.size();
    JointCompatibility out;
    out.groupPtr.assign(ng + 1, 0);
    for (size_t g = 0; g < ng; ++g) out.groupPtr[g + 1] = out.groupPtr[g] + (int32_t)groups[g].size();
    const size_t n = (size_t)out.groupPtr[ng];
    std::vector<double> meas(17 * n + 1);
    std::vector<int32_t> rb(n + 1), cls(n + 1);
    std::vector<uint64_t> pi(n + 1), li(n + 1);
    size_t k = 0;
    for (const std::vector<ObservationCandidate>& grp : groups)
      for (const ObservationCandidate& c : grp) {
        rb[k] = (int32_t)c.robot; cls[k] = (int32_t)c.cls; pi[k] = c.poseIdx; li[k] = c.lmIdx;
        for (int i = 0; i < 17; ++i) meas[17 * k + i] = c.meas[i];
        ++k;
      }
    out.accepted.assign(n + 1, 0); out.dofJoint.assign(n + 1, 0); out.status.assign(n + 1, 0);
    out.d2Single.assign(n + 1, 0.0); out.d2Joint.assign(n + 1, 0.0);
    out.groupD2.assign(ng + 1, 0.0); out.groupDof.assign(ng + 1, 0); out.groupCount.assign(ng + 1, 0); out.groupStatus.assign(ng + 1, 0);
    detail::check(slide_graph_observation_joint_compatibility(g_, (int)ng, out.groupPtr.data(), rb.data(), pi.data(), cls.data(), li.data(),
                                                              meas.data(), prob, out.accepted.data(), out.d2Single.data(), out.d2Joint.data(),
                                                              out.dofJoint.data(), out.status.data(), out.groupD2.data(), out.groupDof.data(),
                                                              out.groupCount.data(), out.groupStatus.data()),
                  "observationJointCompatibility");
    out.accepted.resize(n); out.dofJoint.resize(n); out.status.resize(n); out.d2Single.resize(n); out.d2Joint.resize(n);
    out.groupD2.resize(ng); out.groupDof.resize(ng); out.groupCount.resize(ng); out.groupStatus.resize(ng);
    return out;
  }

  // Robust loss on the loop-closure / relative-measurement factors (slide_graph_set_robust_loss; no counterpart in the reference —
  // GTSAM's noiseModel::Robust with mEstimator::Huber / Cauchy / GemanMcClure / DCS): kind 0 none, 1 .. 4 in that order; param <= 0:
  // the loss's default.  Covers the factors already added and those added later.
  void setRobustLoss(int kind, double param = 0.0, bool closures = true, bool relativeMeas = true) {
    detail::check(slide_graph_set_robust_loss(g_, kind, param, (closures ? 1 : 0) | (relativeMeas ? 2 : 0)), "setRobustLoss");
  }
  // slide_graph_get_closure_weights: every loop-closure (kind 1) and relative-measurement (kind 2) factor in insertion order with
  // the weight and squared whitened norm of its last linearisation.  Call it after solve().
  struct ClosureWeight { size_t fromIdx, fromRobot, toIdx, toRobot; int kind; double weight, s2; };
  std::vector<ClosureWeight> closureWeights() const {
    int n = 0;
    detail::check(slide_graph_get_closure_weights(g_, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &n), "closureWeights");
    std::vector<int32_t> fr(n + 1), tr(n + 1), kd(n + 1);
    std::vector<uint64_t> fi(n + 1), ti(n + 1);
    std::vector<double> w(n + 1), s2(n + 1);
    int m = 0;
    detail::check(slide_graph_get_closure_weights(g_, n, fr.data(), fi.data(), tr.data(), ti.data(), kd.data(), w.data(), s2.data(), &m),
                  "closureWeights");
    std::vector<ClosureWeight> out((size_t)(m < n ? m : n));
    for (size_t k = 0; k < out.size(); ++k)
      out[k] = ClosureWeight{(size_t)fi[k], (size_t)fr[k], (size_t)ti[k], (size_t)tr[k], (int)kd[k], w[k], s2[k]};
    return out;
  }

  // Robust loss on the landmark observation factors (slide_graph_set_observation_loss; no counterpart in the reference — GTSAM's
  // noiseModel::Robust on the BearingRange / Cube / Cylinder factors): kinds and defaults as setRobustLoss, independent of it.
  void setObservationLoss(int kind, double param = 0.0, bool points = true, bool cubes = true, bool cylinders = true) {
    detail::check(slide_graph_set_observation_loss(g_, kind, param, (points ? 1 : 0) | (cubes ? 2 : 0) | (cylinders ? 4 : 0)), "setObservationLoss");
  }
  // slide_graph_get_observation_weights: every landmark factor in insertion order with the weight and (unscaled) squared whitened
  // norm of its last linearisation.  cls: SLIDE_CLS_*.  Call it after solve().
  struct ObservationWeight { size_t poseIdx, robot; int cls; size_t lmIdx; double weight, s2; };
  std::vector<ObservationWeight> observationWeights() const {
    int n = 0;
    detail::check(slide_graph_get_observation_weights(g_, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &n), "observationWeights");
    std::vector<int32_t> rb(n + 1), cl(n + 1);
    std::vector<uint64_t> pi(n + 1), li(n + 1);
    std::vector<double> w(n + 1), s2(n + 1);
    int m = 0;
    detail::check(slide_graph_get_observation_weights(g_, n, rb.data(), pi.data(), cl.data(), li.data(), w.data(), s2.data(), &m), "observationWeights");
    std::vector<ObservationWeight> out((size_t)(m < n ? m : n));
    for (size_t k = 0; k < out.size(); ++k) out[k] = ObservationWeight{(size_t)pi[k], (size_t)rb[k], (int)cl[k], (size_t)li[k], w[k], s2[k]};
    return out;
  }

  slide_graph_t* handle() const { return g_; }

 protected:
  slide_graph_t* g_;
  bool own_;
};

// ---- S2 ----------------------------------------------------------------------------------------------------------------------
// addSLOAMObservation (graphWrapper.cpp:99-237) consumes map managers' match tables; on the MI355X the whole per-key-frame body
// (submap gate -> match -> updateMap -> addSLOAMObservation -> solve -> updateFactorGraphMap) is one call, so the wrapper owns a
// slide_backend_t and exposes the S2 read-back methods over it.
class SemanticFactorGraphWrapper : public SemanticFactorGraph {
 public:
  explicit SemanticFactorGraphWrapper(const slide_params_t* p = nullptr) : SemanticFactorGraphWrapper(make(p)) {}
  ~SemanticFactorGraphWrapper() { if (b_) slide_backend_destroy(b_); }

  // runSLOAMNode body for one key frame (sloamNode.cpp:819-1014 incl. addSLOAMObservation :889); returns "optimized"
  template <class Pose>
  bool addSLOAMObservation(const slide_detections_t& detections, const Pose& relativeMotion, const Pose& prevKeyPose, const int& robotID,
                           Pose7* outPose = nullptr, slide_frame_result_t* matches = nullptr, int mode = SLIDE_FRAME_HOST) {
    double r[7], p[7]; detail::to7(relativeMotion, r); detail::to7(prevKeyPose, p);
    slide_frame_result_t local{};
    slide_frame_result_t* res = matches ? matches : &local;
    detail::check(slide_backend_process_frame(b_, mode, robotID, r, p, &detections, res), "addSLOAMObservation");
    if (outPose) for (int i = 0; i < 7; ++i) outPose->v[i] = res->out_pose7[i];
    return res->optimized != 0;
  }
  // getCurrPose graphWrapper.cpp:277-297
  bool getCurrPose(Pose7& curr_pose, const int& robotID) const {
    const size_t n = getPoseCounterById(robotID);
    return n > 0 && getPose(n - 1, robotID, curr_pose);
  }
  // getAllPoses graphWrapper.cpp:313-338
  bool getAllPoses(std::vector<Pose7>& optimized_poses, std::vector<size_t>& pose_inds, const int& robotID) const {
    const size_t n = getPoseCounterById(robotID);
    std::vector<double> flat(7 * (n ? n : 1));
    uint64_t got = 0;
    detail::check(slide_graph_get_all_poses(g_, robotID, flat.data(), n, &got), "getAllPoses");
    optimized_poses.resize(got);
    pose_inds.resize(got);
    for (uint64_t i = 0; i < got; ++i) { for (int k = 0; k < 7; ++k) optimized_poses[i].v[k] = flat[7 * i + k]; pose_inds[i] = i; }
    return got > 0;
  }
  size_t getPoseCounterById(const int& robotID) const {                                                // graphWrapper.h:127
    uint64_t out4[4], pc[SLIDE_MAX_ROBOTS];
    detail::check(slide_backend_counts(b_, out4, pc, SLIDE_MAX_ROBOTS), "getPoseCounterById");
    return robotID >= 0 && robotID < SLIDE_MAX_ROBOTS ? (size_t)pc[robotID] : 0;
  }
  slide_backend_t* backend() const { return b_; }
  // The association gate (slide_backend_set_association_gate; no counterpart in the reference): with 0 < prob < 1 addSLOAMObservation
  // tests every match of a host frame at the predicted pose (predictedObservationMahalanobis) before it is added and rejects those
  // above the prob quantile — onReject SLIDE_GATE_DROP: the detection is left out (its *_match SLIDE_MATCH_GATED, its *_id -1),
  // SLIDE_GATE_NEW: it becomes a new landmark (its *_match SLIDE_MATCH_GATED).  prob 0, the default state: off.
  void setAssociationGate(const double prob, const int onReject = SLIDE_GATE_DROP) {
    detail::check(slide_backend_set_association_gate(b_, prob, onReject), "setAssociationGate");
  }
  // {frames gated, frames skipped, candidates tested, candidates rejected}
  std::array<int64_t, 4> gateStats() const {
    std::array<int64_t, 4> out{};
    detail::check(slide_backend_gate_stats(b_, out.data()), "gateStats");
    return out;
  }

  // ---- the reference's own S2 signatures (graphWrapper.h:82-122) over the S1 entry points --------------------------------------
  // For a caller that keeps the reference's map managers and association (RunSloam, *MapManager::updateMap) on the host and hands
  // the match vectors over, exactly as sloamNode.cpp:889 / :993 do.  The types are template parameters that only have to provide
  // what graphWrapper.cpp:99-237 uses: map.getMatchesMap().at(int) -> int, map.getRawMap()[i].model, cylinder.model.{root, ray,
  // radius}, cube.model.{pose, scale}, ellipsoid.model.{pose, scale, semantic_label}.  These methods keep the reference's counters
  // (graphWrapper.h:128-134) themselves; do not mix them with the whole-frame addSLOAMObservation above on one object.
  std::vector<size_t> pose_counter_robot_ = std::vector<size_t>(SLIDE_MAX_ROBOTS, 0);                    // graphWrapper.h:128 (public there too)

  template <class CylMap, class CubeMap, class EllMap, class Cyl, class Cube, class Ell, class SE3>
  bool addSLOAMObservation(const CylMap& semanticMap, const CubeMap& cubeSemanticMap, const EllMap& ellipsoidSemanticMap,
                           const std::vector<int>& cyl_matches, const std::vector<Cyl>& cylinders, const std::vector<int>& cube_matches,
                           const std::vector<Cube>& cubes, const std::vector<int>& ellipsoid_matches, const std::vector<Ell>& ellipsoids,
                           const SE3& relativeMotion, const SE3& poseEstimate, const int& robotID, bool opt = true) {   // graphWrapper.cpp:99-237
    if (robotID < 0 || robotID >= SLIDE_MAX_ROBOTS) throw Error(SLIDE_ERR_INVALID, "addSLOAMObservation: robotID");
    Pose7 curr; detail::to7(poseEstimate, curr.v);
    const size_t pose_counter = pose_counter_robot_[robotID];
    if (pose_counter == 0) setPriors(poseEstimate, robotID);                                             // :114-119
    else addKeyPoseAndBetween(pose_counter - 1, pose_counter, relativeMotion, poseEstimate, robotID);    // :121
    const auto matchesMap = semanticMap.getMatchesMap();
    const auto cubeMatchesMap = cubeSemanticMap.getMatchesMap();
    for (size_t i = 0; i < cyl_matches.size(); ++i) {                                                    // :127-140
      CylinderMeasurement m;
      detail::to3(cylinders[i].model.root, m.root); detail::to3(cylinders[i].model.ray, m.ray); m.radius = cylinders[i].model.radius;
      if (cyl_matches[i] == -1) { addCylinderFactor(pose_counter, cyl_counter_, curr, m, false, robotID); ++cyl_counter_; }
      else addCylinderFactor(pose_counter, (size_t)matchesMap.at(cyl_matches[i]), curr, m, true, robotID);
    }
    for (size_t i = 0; i < cube_matches.size(); ++i) {                                                   // :143-156
      CubeMeasurement m;
      detail::to7(cubes[i].model.pose, m.pose.v); detail::to3(cubes[i].model.scale, m.scale);
      if (cube_matches[i] == -1) { addCubeFactor(pose_counter, cube_counter_, curr, m, false, robotID); ++cube_counter_; }
      else addCubeFactor(pose_counter, (size_t)cubeMatchesMap.at(cube_matches[i]), curr, m, true, robotID);
    }
    const auto ellipMatchesMap = ellipsoidSemanticMap.getMatchesMap();
    for (size_t i = 0; i < ellipsoid_matches.size(); ++i) {                                              // :159-203: body-frame bearing + range
      double w[3], b[3];
      detail::to3(ellipsoids[i].model.pose.translation(), w);
      detail::to_body(curr.v, w, b);
      const double range = std::sqrt(b[0] * b[0] + b[1] * b[1] + b[2] * b[2]);
      // (an ellipsoid AT the sensor: Eigen's .normalized() of the reference, graphWrapper.cpp:176-184, leaves the zero vector as it is —
      // dividing would hand NaNs to the solve)
      const double inv = range > 0.0 ? 1.0 / range : 0.0;
      const double bearing[3] = {b[0] * inv, b[1] * inv, b[2] * inv};
      if (ellipsoid_matches[i] == -1) {
        addPointLandmarkKey(point_landmark_counter_, w);
        addRangeBearingFactor(pose_counter, point_landmark_counter_, bearing, range, robotID);
        point_landmark_labels_.push_back(ellipsoids[i].model.semantic_label);
        ++point_landmark_counter_;
      } else {
        addRangeBearingFactor(pose_counter, (size_t)ellipMatchesMap.at(ellipsoid_matches[i]), bearing, range, robotID);
      }
    }
    pose_counter_robot_[robotID] = pose_counter + 1;                                                     // :206-207
    if (opt) { solve(); return true; }                                                                   // :212-230
    return false;
  }
  // updateFactorGraphMap graphWrapper.cpp:259-275 (+ updateCylinder / updateCube / updateEllipsoid :239-256): every optimised landmark
  // back into the caller's map models; an ellipsoid's pose becomes identity rotation + the optimised point (:252-255)
  template <class CylMap, class CubeMap, class EllMap>
  void updateFactorGraphMap(CylMap& semanticMap, CubeMap& cubeSemanticMap, EllMap& ellipsoidSemanticMap) {
    auto& map = semanticMap.getRawMap();
    auto& cube_map = cubeSemanticMap.getRawMap();
    auto& ellipsoid_map = ellipsoidSemanticMap.getRawMap();
    for (size_t i = 0; i < cyl_counter_; ++i) {
      const CylinderMeasurement m = getCylinder((int)i);
      for (int k = 0; k < 3; ++k) { map[i].model.root[k] = m.root[k]; map[i].model.ray[k] = m.ray[k]; }
      map[i].model.radius = m.radius;
    }
    for (size_t i = 0; i < cube_counter_; ++i) {
      const std::array<double, 15> c = getCube((int)i);
      double p7[7];
      rt_to7(c.data(), c.data() + 9, p7);
      slide_assign_pose(cube_map[i].model.pose, p7);
      for (int k = 0; k < 3; ++k) cube_map[i].model.scale[k] = c[12 + k];
    }
    for (size_t i = 0; i < point_landmark_counter_; ++i) {
      const std::array<double, 3> x = getCentroidLandmark((int)i);
      const double p7[7] = {x[0], x[1], x[2], 0, 0, 0, 1};
      slide_assign_pose(ellipsoid_map[i].model.pose, p7);
    }
  }
  // getCurrPose graphWrapper.cpp:277-297 with the reference's argument list; cov (optional, boost::optional<MatrixXd&> there) = the
  // 6x6 marginal covariance of that pose, row-major [rot, trans]
  template <class SE3>
  void getCurrPose(SE3& curr_pose, const int& robotID, std::array<double, 36>* cov) {
    const size_t n = robotID >= 0 && robotID < SLIDE_MAX_ROBOTS ? pose_counter_robot_[robotID] : 0;
    Pose7 p;
    if (n > 0) (void)getPose(n - 1, robotID, p);                  // (absent: identity, as the reference after its ROS_ERROR)
    slide_assign_pose(curr_pose, p.v);
    if (cov && n > 0) *cov = getPoseCovariance((int)(n - 1), robotID);
  }
  // getAllCentroidLandmarks / ...AndLabels graphWrapper.cpp:340-400: a landmark whose optimised point is exactly (0, 0, 0) counts as
  // missing (:345-347)
  template <class SE3>
  void getAllCentroidLandmarks(std::vector<SE3>& optimized_landmark_pos, std::vector<size_t>& landmark_inds) {
    for (size_t i = 0; i < point_landmark_counter_; ++i) {
      const std::array<double, 3> x = getCentroidLandmark((int)i);
      if (x[0] == 0.0 && x[1] == 0.0 && x[2] == 0.0) continue;
      const double p7[7] = {x[0], x[1], x[2], 0, 0, 0, 1};
      SE3 pose; slide_assign_pose(pose, p7);
      optimized_landmark_pos.push_back(pose);
      landmark_inds.push_back(i);
    }
  }
  template <class SE3>
  void getAllCentroidLandmarksAndLabels(std::vector<SE3>& optimized_landmark_pos, std::vector<int>& landmark_labels) {
    for (size_t i = 0; i < point_landmark_counter_; ++i) {
      const std::array<double, 3> x = getCentroidLandmark((int)i);
      if (x[0] == 0.0 && x[1] == 0.0 && x[2] == 0.0) continue;
      const double p7[7] = {x[0], x[1], x[2], 0, 0, 0, 1};
      SE3 pose; slide_assign_pose(pose, p7);
      optimized_landmark_pos.push_back(pose);
      landmark_labels.push_back(i < point_landmark_labels_.size() ? point_landmark_labels_[i] : -1);     // (:392-398)
    }
  }

 private:
  size_t cyl_counter_ = 0, cube_counter_ = 0, point_landmark_counter_ = 0;                                // graphWrapper.h:131-133
  std::vector<int> point_landmark_labels_;
  static void rt_to7(const double R[9], const double t[3], double o[7]) {                                  // row-major R -> unit quaternion
    const double tr = R[0] + R[4] + R[8];
    double w, x, y, z;
    if (tr > 0) { const double s = std::sqrt(tr + 1.0) * 2; w = 0.25 * s; x = (R[7] - R[5]) / s; y = (R[2] - R[6]) / s; z = (R[3] - R[1]) / s; }
    else if (R[0] > R[4] && R[0] > R[8]) { const double s = std::sqrt(1.0 + R[0] - R[4] - R[8]) * 2; w = (R[7] - R[5]) / s; x = 0.25 * s; y = (R[1] + R[3]) / s; z = (R[2] + R[6]) / s; }
    else if (R[4] > R[8]) { const double s = std::sqrt(1.0 + R[4] - R[0] - R[8]) * 2; w = (R[2] - R[6]) / s; x = (R[1] + R[3]) / s; y = 0.25 * s; z = (R[5] + R[7]) / s; }
    else { const double s = std::sqrt(1.0 + R[8] - R[0] - R[4]) * 2; w = (R[3] - R[1]) / s; x = (R[2] + R[6]) / s; y = (R[5] + R[7]) / s; z = 0.25 * s; }
    o[0] = t[0]; o[1] = t[1]; o[2] = t[2]; o[3] = x; o[4] = y; o[5] = z; o[6] = w;
  }
  static slide_backend_t* make(const slide_params_t* p) {
    slide_backend_t* b = slide_backend_create(p);
    if (!b) throw Error(SLIDE_ERR_HIP, "slide_backend_create");
    return b;
  }
  explicit SemanticFactorGraphWrapper(slide_backend_t* b) : SemanticFactorGraph(slide_backend_graph(b)), b_(b) {}
  slide_backend_t* b_ = nullptr;
};

// ---- S4 (the SlideGraph side) ----------------------------------------------------------------------------------------------------
// PlaceRecognition::findInterLoopClosureWithClipper include/core/place_recognition.h, src/core/place_recognition.cpp:541-629, with the
// reference's argument order and container shapes: Objects = a container of rows indexable [0..6] ([label, x, y, z, d1, d2, d3];
// std::vector<Eigen::Vector7d> at the call site), Mat4 = a 4x4 written through m(r, c) (Eigen::Matrix4d; slide::Mat4 below when Eigen
// is absent).  The (0, 0) filter, the object-count gate and the inversion of run_semantic_clipper's estimate happen inside the
// library; tfFromQueryToRef is the identity when nothing is found (sloamNode.cpp:618-620 starts from the identity).
struct Mat4 {
  double m[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  double& operator()(int r, int c) { return m[4 * r + c]; }
  double operator()(int r, int c) const { return m[4 * r + c]; }
};
class PlaceRecognition {
 public:
  slide_slidegraph_params_t slidegraph;      // place_recognition.cpp:65-75: sigma, epsilon, num_inliners_threshold, descriptor_matching_threshold, min_num_map_objects_to_start
  slide_place_params_t place;                // place_recognition.cpp:24-78: the SlideMatch parameters (slide_place_default_params)
  explicit PlaceRecognition(const slide_slidegraph_params_t* p = nullptr) {
    if (p) slidegraph = *p; else slide_slidegraph_default_params(&slidegraph);
    slide_place_default_params(&place);
  }

  // PlaceRecognition::findInterLoopClosure place_recognition.cpp:498-538 (SlideMatch, the branch interLoopClosureThread_ takes when
  // use_slidematch_ is set): centring, the lattice sweep, the inlier gate and the refinement happen inside the library;
  // tfFromQueryToRef is the identity when nothing is found.
  template <class Objects, class M4>
  bool findInterLoopClosure(const Objects& reference_objects, const Objects& query_objects, M4& tfFromQueryToRef) const {
    std::vector<double> ref, qry;
    flatten(reference_objects, ref);
    flatten(query_objects, qry);
    double tf[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    int inliers = 0;
    const int rc = slide_find_inter_loop_closure(ref.data(), (int)(ref.size() / 7), qry.data(), (int)(qry.size() / 7), &place, tf, &inliers, nullptr);
    if (rc < 0) detail::check(rc, "findInterLoopClosure");
    assign(tfFromQueryToRef, tf);
    return rc == 1;
  }

  // The SlideMatch loop of SLOAMNode::interLoopClosureThread_ (sloamNode.cpp:600-694) as one call, the reference map as map 0:
  // tfs[k] / found[k] are what findInterLoopClosure(reference_objects, query_maps[k], ...) gives, bit for bit.
  template <class Objects, class M4>
  void findInterLoopClosures(const Objects& reference_objects, const std::vector<Objects>& query_maps, std::vector<M4>& tfs,
                             std::vector<bool>& found) const {
    const int n = (int)query_maps.size();
    std::vector<double> flat;
    std::vector<int32_t> off(1, 0), pairs;
    flatten(reference_objects, flat);
    off.push_back((int32_t)(flat.size() / 7));
    for (int k = 0; k < n; ++k) {
      flatten(query_maps[k], flat);
      off.push_back((int32_t)(flat.size() / 7));
      pairs.push_back(0);
      pairs.push_back(k + 1);
    }
    std::vector<double> tf(16 * (size_t)n + 1);
    std::vector<int32_t> inl(n + 1), f(n + 1), status(n + 1);
    detail::check(slide_find_inter_loop_closures(flat.data(), off.data(), n + 1, pairs.data(), n, &place, tf.data(), inl.data(), nullptr, f.data(),
                                                 nullptr, nullptr, status.data()),
                  "findInterLoopClosures");
    tfs.resize(n);
    found.assign(n, false);
    for (int k = 0; k < n; ++k) {
      if (status[k] < 0) throw Error(status[k], "findInterLoopClosures: query map " + std::to_string(k) + ": the two maps exceed the sweep's on-chip image");
      assign(tfs[k], tf.data() + 16 * (size_t)k);
      found[k] = f[k] != 0;
    }
  }

  // PlaceRecognition::findIntraLoopClosure place_recognition.cpp:389-496 with the reference's argument list (place_recognition.h:88-91;
  // the caller has inter_loop_closure == false): reference_objects = the submap around the candidate key pose (map frame),
  // query_objects = the detections in the query pose's local frame.  The intra window is the three rosparams of :53-63 (yaw in
  // radians here).  tfFromQueryToCandidate is left alone when nothing is found, as in the reference.
  double match_x_half_range_intra = 5.0, match_y_half_range_intra = 5.0, match_yaw_half_range_intra = 10.0 * 3.14159265358979323846 / 180.0;
  template <class Objects, class SE3, class M4>
  bool findIntraLoopClosure(const Objects& reference_objects, const Objects& query_objects, const SE3& query_pose, const SE3& reference_pose,
                            M4& tfFromQueryToCandidate) const {
    std::vector<double> sub, meas;
    flatten(reference_objects, sub);
    flatten(query_objects, meas);
    double q7[7], c7[7], tf[16];
    detail::to7(query_pose, q7);
    detail::to7(reference_pose, c7);
    int inliers = 0;
    const int rc = slide_find_intra_loop_closure(meas.data(), (int)(meas.size() / 7), sub.data(), (int)(sub.size() / 7), q7, c7, &place,
                                                 match_x_half_range_intra, match_y_half_range_intra, match_yaw_half_range_intra, tf, &inliers, nullptr);
    if (rc < 0) detail::check(rc, "findIntraLoopClosure");
    if (rc == 1) assign(tfFromQueryToCandidate, tf);
    return rc == 1;
  }
  // One attempt of SLOAMNode::intraLoopClosureThread_ (sloamNode.cpp:355-486) over a LIST of candidate key poses in one call:
  // tfs[k] / found[k] are what findIntraLoopClosure(submaps[k], query_objects, query_pose, reference_poses[k], ...) gives, bit for
  // bit; tfs[k] is the identity when candidate k is not found.
  template <class Objects, class SE3, class M4>
  void findIntraLoopClosures(const std::vector<Objects>& submaps, const Objects& query_objects, const SE3& query_pose,
                             const std::vector<SE3>& reference_poses, std::vector<M4>& tfs, std::vector<bool>& found) const {
    const int n = (int)submaps.size();
    if (reference_poses.size() != submaps.size()) throw Error(SLIDE_ERR_INVALID, "findIntraLoopClosures: one reference pose per submap");
    std::vector<double> flat, meas, c7(7 * (size_t)n + 1);
    std::vector<int32_t> off(1, 0);
    flatten(query_objects, meas);
    for (int k = 0; k < n; ++k) {
      flatten(submaps[k], flat);
      off.push_back((int32_t)(flat.size() / 7));
      detail::to7(reference_poses[k], c7.data() + 7 * (size_t)k);
    }
    double q7[7];
    detail::to7(query_pose, q7);
    std::vector<double> tf(16 * (size_t)n + 1);
    std::vector<int32_t> inl(n + 1), f(n + 1), status(n + 1);
    detail::check(slide_find_intra_loop_closures(meas.data(), (int)(meas.size() / 7), q7, flat.data(), off.data(), n, c7.data(), &place,
                                                 match_x_half_range_intra, match_y_half_range_intra, match_yaw_half_range_intra, tf.data(),
                                                 inl.data(), nullptr, f.data(), nullptr, nullptr, status.data()),
                  "findIntraLoopClosures");
    tfs.resize(n);
    found.assign(n, false);
    for (int k = 0; k < n; ++k) {
      if (status[k] < 0) throw Error(status[k], "findIntraLoopClosures: candidate " + std::to_string(k) + ": the submap and the detections exceed the sweep's on-chip image");
      assign(tfs[k], tf.data() + 16 * (size_t)k);
      found[k] = f[k] != 0;
    }
  }

  template <class Objects, class M4>
  bool findInterLoopClosureWithClipper(const Objects& reference_objects, const Objects& query_objects, M4& tfFromQueryToRef) const {
    std::vector<double> ref, qry;
    flatten(reference_objects, ref);
    flatten(query_objects, qry);
    double tf[16];
    int counts[4], found = 0;
    detail::check(slide_find_inter_loop_closure_clipper(ref.data(), (int)(ref.size() / 7), qry.data(), (int)(qry.size() / 7), &slidegraph, nullptr, 0,
                                                        tf, counts, &found),
                  "findInterLoopClosureWithClipper");
    assign(tfFromQueryToRef, tf);
    return found != 0;
  }

  // The loop of SLOAMNode::interLoopClosureThread_ (sloamNode.cpp:600-694: the host robot's map against every robot without a
  // loopClosureTf) as one call: tfs[k] / found[k] are what findInterLoopClosureWithClipper(reference_objects, query_maps[k], ...) gives.
  template <class Objects, class M4>
  void findInterLoopClosuresWithClipper(const Objects& reference_objects, const std::vector<Objects>& query_maps, std::vector<M4>& tfs,
                                        std::vector<bool>& found) const {
    const int n = (int)query_maps.size();
    std::vector<double> flat;
    std::vector<int32_t> off(1, 0), pairs;
    flatten(reference_objects, flat);
    off.push_back((int32_t)(flat.size() / 7));
    for (int k = 0; k < n; ++k) {
      flatten(query_maps[k], flat);
      off.push_back((int32_t)(flat.size() / 7));
      pairs.push_back(0);
      pairs.push_back(k + 1);
    }
    std::vector<double> tf(16 * (size_t)n + 1);
    std::vector<int32_t> counts(4 * (size_t)n + 1), f(n + 1), status(n + 1);
    detail::check(slide_find_inter_loop_closures_clipper(flat.data(), off.data(), n + 1, pairs.data(), n, &slidegraph, nullptr, nullptr, tf.data(),
                                                         counts.data(), f.data(), status.data()),
                  "findInterLoopClosuresWithClipper");
    tfs.resize(n);
    found.assign(n, false);
    for (int k = 0; k < n; ++k) {
      if (status[k] < 0) throw Error(status[k], "findInterLoopClosuresWithClipper: query map " + std::to_string(k) + ": more associations or non-zeros than the library holds");
      assign(tfs[k], tf.data() + 16 * (size_t)k);
      found[k] = f[k] != 0;
    }
  }

 private:
  template <class Objects>
  static void flatten(const Objects& objs, std::vector<double>& out) {
    for (const auto& o : objs)
      for (int c = 0; c < 7; ++c) out.push_back(o[c]);
  }
  template <class M4>
  static void assign(M4& dst, const double tf[16]) {
    for (int r = 0; r < 4; ++r)
      for (int c = 0; c < 4; ++c) dst(r, c) = tf[4 * r + c];
  }
};

// getkeyPoseSubmap of the three map managers (cylinderMapManager.cpp:186-211, cubeMapManager.cpp:77-101, ellipsoidMapManager.cpp:82-107)
// followed by SLOAMNode::prepareLCInput (sloamNode.cpp:544-576) around a list of key poses, on the device (slide_keypose_submaps):
// submaps[k] = the Vector7d rows the intra matcher takes for key pose k.  Objects as the reference has them: cylinder.model.{root,
// ray, radius, semantic_label}, cube / ellipsoid .model.{pose, scale, semantic_label}.  max_dz: the reference hard-codes 1.5.
template <class Cylinders, class Cubes, class Ellipsoids, class SE3>
std::vector<std::vector<std::array<double, 7>>> getkeyPoseSubmaps(const Cylinders& cylinders, const Cubes& cubes, const Ellipsoids& ellipsoids,
                                                                  const std::vector<SE3>& poses, double submap_radius, double max_dz = 1.5) {
  std::vector<double> cr, ca, crad, bx, bs, ex, es, px;
  std::vector<int32_t> cl, bl, el;
  for (const auto& c : cylinders) {
    for (int k = 0; k < 3; ++k) { cr.push_back(c.model.root[k]); ca.push_back(c.model.ray[k]); }
    crad.push_back(c.model.radius);
    cl.push_back((int32_t)c.model.semantic_label);
  }
  for (const auto& c : cubes) {
    const auto t = c.model.pose.translation();
    for (int k = 0; k < 3; ++k) { bx.push_back(t[k]); bs.push_back(c.model.scale[k]); }
    bl.push_back((int32_t)c.model.semantic_label);
  }
  for (const auto& c : ellipsoids) {
    const auto t = c.model.pose.translation();
    for (int k = 0; k < 3; ++k) { ex.push_back(t[k]); es.push_back(c.model.scale[k]); }
    el.push_back((int32_t)c.model.semantic_label);
  }
  for (const auto& p : poses) {
    const auto t = p.translation();
    for (int k = 0; k < 3; ++k) px.push_back(t[k]);
  }
  const int n = (int)poses.size();
  std::vector<int32_t> off((size_t)n + 1, 0);
  std::vector<double> rows;
  int64_t n_rows = 0;
  auto call = [&](int64_t cap) {
    return slide_keypose_submaps(cr.data(), ca.data(), crad.data(), cl.data(), (int)cl.size(), bx.data(), bs.data(), bl.data(), (int)bl.size(), ex.data(),
                                 es.data(), el.data(), (int)el.size(), px.data(), n, submap_radius, max_dz, off.data(), rows.data(), nullptr, cap, &n_rows);
  };
  int rc = call(0);                                   // sizes only
  if (rc == SLIDE_ERR_CAPACITY && n_rows > 0) {
    rows.resize(7 * (size_t)n_rows);
    rc = call(n_rows);
  }
  detail::check(rc, "getkeyPoseSubmaps");
  std::vector<std::vector<std::array<double, 7>>> out((size_t)n);
  for (int k = 0; k < n; ++k)
    for (int32_t r = off[k]; r < off[k + 1]; ++r) {
      std::array<double, 7> row;
      for (int c = 0; c < 7; ++c) row[c] = rows[7 * (size_t)r + c];
      out[k].push_back(row);
    }
  return out;
}

}  // namespace slide
#endif  // SLIDE_SLOAM_ADAPTOR_HPP_
