// Compile-and-run check of slide::SemanticFactorGraph::observationJointCompatibility (include/slide_sloam_adaptor.hpp) against
// libslide_gpu.so: tests/test_joint_compat_adaptor.py builds it without a device (no argument: link check only) and runs it on the GPU
// (any argument), where the method must return what the C call returns.  The graph is observation_gate_adaptor_check.cpp's: a 12-pose
// chain along x with a point, a cylinder and a cube landmark seen from its first poses.  Two hypotheses from pose 5: one that agrees
// with the map (point, cylinder, cube: accepted whole) and one whose point measures a place 2 m off and names a landmark the graph
// does not hold beside it (the point rejected alone, the unknown one skipped, the cylinder kept).
#include <array>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "slide_sloam_adaptor.hpp"

using Graph = slide::SemanticFactorGraph;

static slide::Pose7 at(double x, double y = 0.0) {
  slide::Pose7 p;
  p.v[0] = x; p.v[1] = y;
  return p;
}
static Graph::ObservationCandidate point_from(size_t k, size_t lm, double x, double y) {
  const double q[3] = {x - (double)k, y, 0.0}, rho = std::sqrt(q[0] * q[0] + q[1] * q[1]);
  const std::array<double, 3> b = {q[0] / rho, q[1] / rho, 0.0};
  return Graph::pointCandidate(k, lm, b, rho, 0);
}

int main(int argc, char** argv) {
  if (argc < 2) return 0;
  try {
    slide_params_t prm;
    slide_default_params(&prm);
    for (int c = 0; c < 6; ++c) prm.noise_model_odom_vec[c] = c < 3 ? 0.004 : 0.02;
    prm.bearing_range_sigma = 0.05;
    prm.cylinder_sigma = 0.1;
    Graph g(&prm);
    g.setPriors(at(0.0), 0);
    for (size_t k = 1; k < 12; ++k) g.addKeyPoseAndBetween(k - 1, k, at(1.0), at((double)k), 0);
    const std::array<double, 3> pt = {3.0, 2.0, 0.0};
    g.addPointLandmarkKey(0, pt);
    const slide::CylinderMeasurement cyl{{4.0, -2.0, 0.0}, {0.0, 0.0, 1.0}, 0.3};
    slide::CubeMeasurement cube;
    cube.pose = at(5.0, 3.0);
    cube.scale[0] = 1.0; cube.scale[1] = 2.0; cube.scale[2] = 0.5;
    for (size_t k = 0; k < 3; ++k) {
      const Graph::ObservationCandidate c = point_from(k, 0, pt[0], pt[1]);
      const std::array<double, 3> b = {c.meas[0], c.meas[1], c.meas[2]};
      g.addRangeBearingFactor(k, 0, b, c.meas[3], 0);
      g.addCylinderFactor(k, 0, at((double)k), cyl, k > 0, 0);
      g.addCubeFactor(k, 0, at((double)k), cube, k > 0, 0);
    }
    g.solve();
    const std::vector<std::vector<Graph::ObservationCandidate>> groups = {
        {point_from(5, 0, pt[0], pt[1]), Graph::cylinderCandidate(5, 0, at(5.0), cyl, 0), Graph::cubeCandidate(5, 0, at(5.0), cube, 0)},
        {point_from(5, 0, pt[0], pt[1] - 2.0), point_from(5, 40, pt[0], pt[1]), Graph::cylinderCandidate(5, 0, at(5.0), cyl, 0)}};
    const Graph::JointCompatibility r = g.observationJointCompatibility(groups, 0.99);
    bool good = r.accepted.size() == 6 && r.groupD2.size() == 2 && r.groupPtr.size() == 3 && r.groupPtr[1] == 3 && r.groupPtr[2] == 6;
    good = good && r.accepted[0] && r.accepted[1] && r.accepted[2] && !r.accepted[3] && !r.accepted[4] && r.accepted[5];
    good = good && r.dofJoint[0] == 3 && r.dofJoint[1] == 10 && r.dofJoint[2] == 19 && r.dofJoint[3] == 3 && r.dofJoint[5] == 7;
    good = good && r.status[3] == SLIDE_OK && r.status[4] == SLIDE_MISSING && r.d2Single[3] > 11.345 && r.d2Joint[4] == 0.0;
    good = good && r.groupCount[0] == 3 && r.groupDof[0] == 19 && r.groupCount[1] == 1 && r.groupDof[1] == 7 && r.groupStatus[0] == SLIDE_OK;
    good = good && r.groupD2[0] == r.d2Joint[2] && r.groupD2[1] == r.d2Joint[5];
    // the C call on the same groups
    const int32_t ptr[3] = {0, 3, 6};
    int32_t rb[6], cls[6], acc[6], dof[6], st[6], gdof[2], gcnt[2], gst[2];
    uint64_t pi[6], li[6];
    double d1[6], dj[6], gd[2];
    std::vector<double> meas;
    int k = 0;
    for (const auto& grp : groups)
      for (const auto& c : grp) {
        rb[k] = 0; cls[k] = c.cls; pi[k] = c.poseIdx; li[k] = c.lmIdx;
        meas.insert(meas.end(), c.meas.begin(), c.meas.end());
        ++k;
      }
    good = good && slide_graph_observation_joint_compatibility(g.handle(), 2, ptr, rb, pi, cls, li, meas.data(), 0.99, acc, d1, dj, dof, st, gd, gdof,
                                                               gcnt, gst) == SLIDE_OK;
    for (int i = 0; good && i < 6; ++i) good = d1[i] == r.d2Single[i] && dj[i] == r.d2Joint[i] && acc[i] == r.accepted[i] && dof[i] == r.dofJoint[i];
    for (int i = 0; good && i < 2; ++i) good = gd[i] == r.groupD2[i] && gcnt[i] == r.groupCount[i];
    double q = 0.0;
    good = good && slide_chi2_quantile(0.99, 3, &q) == SLIDE_OK && std::fabs(q - 11.345) < 1e-3;
    std::printf("joint compat ok n=%zu accepted=%d%d%d%d%d%d count=%d%d dof=%d%d status4=%d\n", r.accepted.size(), (int)r.accepted[0], (int)r.accepted[1],
                (int)r.accepted[2], (int)r.accepted[3], (int)r.accepted[4], (int)r.accepted[5], (int)r.groupCount[0], (int)r.groupCount[1],
                (int)r.groupDof[0], (int)r.groupDof[1], (int)r.status[4]);
    return good ? 0 : 1;
  } catch (const slide::Error& e) {
    std::printf("slide::Error %d: %s\n", e.code, e.what());
    return 2;
  }
}
