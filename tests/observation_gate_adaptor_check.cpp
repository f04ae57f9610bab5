// Compile-and-run check of slide::SemanticFactorGraph::observationMahalanobis (include/slide_sloam_adaptor.hpp) against
// libslide_gpu.so: tests/test_observation_gate_adaptor.py builds it without a device (no argument: link check only) and runs it on the
// GPU (any argument), where the method must return what the C call returns: a 12-pose chain along x with a point, a cylinder and a cube
// landmark seen from its first poses; a point, a cylinder and a cube candidate from pose 5 that agree with the map, a point candidate
// that measures a place 2 m off, and one naming a landmark the graph does not hold.
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
// the bearing and range of the world point (x, y, 0) from the pose at (k, 0, 0), identity rotation
static Graph::ObservationCandidate point_from(size_t k, size_t lm, double x, double y) {
  const double q[3] = {x - (double)k, y, 0.0}, rho = std::sqrt(q[0] * q[0] + q[1] * q[1]);
  const std::array<double, 3> b = {q[0] / rho, q[1] / rho, 0.0};
  return Graph::pointCandidate(k, lm, b, rho, 0);
}

int main(int argc, char** argv) {
  if (argc < 2) return 0;
  try {
    // sigmas at which a 2 m mistake is far outside the gate: 0.004 rad / 0.02 m of odometry per step, 0.05 on bearing and range, 0.1
    // on the cylinder (under the defaults of 1 and 400 the point and cylinder gates pass almost anything)
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
    const std::vector<Graph::ObservationCandidate> cands = {
        point_from(5, 0, pt[0], pt[1]), point_from(5, 0, pt[0], pt[1] - 2.0), Graph::cylinderCandidate(5, 0, at(5.0), cyl, 0),
        Graph::cubeCandidate(5, 0, at(5.0), cube, 0), point_from(5, 40, pt[0], pt[1])};
    std::vector<int32_t> dof, status;
    const std::vector<double> d2 = g.observationMahalanobis(cands, &dof, &status);
    bool good = d2.size() == 5 && dof.size() == 5 && status.size() == 5;
    good = good && d2[0] < 11.345 && d2[1] > 11.345 && d2[2] < 18.475 && d2[3] < 21.666 && d2[4] == 0.0;
    good = good && dof[0] == 3 && dof[2] == 7 && dof[3] == 9 && status[0] == SLIDE_OK && status[3] == SLIDE_OK && status[4] == SLIDE_MISSING;
    // the C call on the same candidates
    int32_t rb[5], cls[5];
    uint64_t pi[5], li[5];
    std::vector<double> meas;
    for (int k = 0; k < 5; ++k) {
      rb[k] = 0; cls[k] = cands[k].cls; pi[k] = cands[k].poseIdx; li[k] = cands[k].lmIdx;
      meas.insert(meas.end(), cands[k].meas.begin(), cands[k].meas.end());
    }
    double c5[5] = {-1, -1, -1, -1, -1};
    good = good && slide_graph_observation_mahalanobis(g.handle(), 5, rb, pi, cls, li, meas.data(), c5, nullptr, nullptr, nullptr, nullptr) == SLIDE_OK;
    for (int k = 0; good && k < 5; ++k) good = d2[k] == c5[k];
    std::printf("obs gate ok n=%zu verdicts=%d%d%d%d dof=%d%d%d status4=%d\n", d2.size(), (int)(d2[0] < 11.345), (int)(d2[1] < 11.345),
                (int)(d2[2] < 18.475), (int)(d2[3] < 21.666), (int)dof[0], (int)dof[2], (int)dof[3], (int)status[4]);
    return good ? 0 : 1;
  } catch (const slide::Error& e) {
    std::printf("slide::Error %d: %s\n", e.code, e.what());
    return 2;
  }
}
