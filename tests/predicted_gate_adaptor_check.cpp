// Compile-and-run check of slide::SemanticFactorGraph::predictedObservationMahalanobis and
// slide::SemanticFactorGraphWrapper::setAssociationGate / gateStats (include/slide_sloam_adaptor.hpp) against libslide_gpu.so:
// tests/test_predicted_gate_adaptor.py builds it without a device (no argument: link check only) and runs it on the GPU (any
// argument), where the methods must return what the C calls return.  The graph: a 12-pose chain along x, point 0 at (3, 2, 0) seen
// from poses 0 and 1.  The prediction: pose 12 = pose 11 moved 1 m along x, not added.  Candidates against point 0: its own geometry
// seen from the predicted pose (a true match) and the geometry of a point 3 m to the side (a false one).  The wrapper: two frames
// with two ellipsoid detections each under the gate — the first is skipped (no from pose), the second gated, nothing rejected.
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
static void bearing_range(double px, double x, double y, std::array<double, 3>& b, double& rho) {
  const double q[2] = {x - px, y};
  rho = std::sqrt(q[0] * q[0] + q[1] * q[1]);
  b = {q[0] / rho, q[1] / rho, 0.0};
}

int main(int argc, char** argv) {
  if (argc < 2) return 0;
  try {
    slide_params_t prm;
    slide_default_params(&prm);
    for (int c = 0; c < 6; ++c) prm.noise_model_odom_vec[c] = c < 3 ? 0.004 : 0.02;
    prm.bearing_range_sigma = 0.01;
    Graph g(&prm);
    g.setPriors(at(0.0), 0);
    for (size_t k = 1; k < 12; ++k) g.addKeyPoseAndBetween(k - 1, k, at(1.0), at((double)k), 0);
    const std::array<double, 3> p0 = {3.01, 2.0, 0.0};
    g.addPointLandmarkKey(0, p0);
    std::array<double, 3> b;
    double rho;
    for (size_t k = 0; k < 2; ++k) { bearing_range((double)k, 3.0, 2.0, b, rho); g.addRangeBearingFactor(k, 0, b, rho, 0); }
    g.solve();
    std::vector<Graph::ObservationCandidate> cands;
    bearing_range(12.0, 3.0, 2.0, b, rho);
    cands.push_back(Graph::pointCandidate(0, 0, b, rho, 0));       // (the candidate's own pose index is ignored)
    bearing_range(12.0, 3.0, 5.0, b, rho);
    cands.push_back(Graph::pointCandidate(0, 0, b, rho, 0));
    cands.push_back(Graph::pointCandidate(0, 40, b, rho, 0));      // a landmark the graph does not hold
    std::vector<double> d2;
    std::vector<int32_t> dof, status;
    bool good = g.predictedObservationMahalanobis(11, at(1.0), at(12.0), 0, cands, d2, &dof, &status);
    good = good && d2.size() == 3 && dof.size() == 3 && status.size() == 3 && dof[0] == 3;
    good = good && d2[0] < 11.345 && d2[1] > 11.345 && d2[2] == 0.0 && status[0] == SLIDE_OK && status[1] == SLIDE_OK && status[2] == SLIDE_MISSING;
    // the C call on the same candidates
    const double rel7[7] = {1, 0, 0, 0, 0, 0, 1}, est7[7] = {12, 0, 0, 0, 0, 0, 1};
    const int32_t cls[3] = {SLIDE_CLS_ELLIPSOID, SLIDE_CLS_ELLIPSOID, SLIDE_CLS_ELLIPSOID};
    const uint64_t lm[3] = {0, 0, 40};
    double meas[51], c3[3] = {-1, -1, -1};
    for (int k = 0; k < 3; ++k)
      for (int i = 0; i < 17; ++i) meas[17 * k + i] = cands[k].meas[i];
    good = good && slide_graph_predicted_observation_mahalanobis(g.handle(), 0, 11, rel7, est7, 3, cls, lm, meas, c3, nullptr, nullptr, nullptr,
                                                                 nullptr) == SLIDE_OK;
    for (int k = 0; good && k < 3; ++k) good = d2[k] == c3[k];
    // a from pose the graph does not hold: false, d2 untouched
    std::vector<double> keep = {7.0};
    const bool missing = !g.predictedObservationMahalanobis(40, at(1.0), at(41.0), 0, cands, keep);
    good = good && missing && keep.size() == 1 && keep[0] == 7.0;

    // the wrapper's gate
    slide::SemanticFactorGraphWrapper w(&prm);
    w.setAssociationGate(0.99, SLIDE_GATE_DROP);
    bool refused = false;
    try { w.setAssociationGate(1.5); } catch (const slide::Error&) { refused = true; }
    good = good && refused;
    const int32_t labels[2] = {1, 1};
    const double scale[6] = {0.5, 0.5, 0.9, 0.5, 0.5, 0.9};
    int32_t match[2] = {7, 7}, id[2] = {7, 7};
    slide::Pose7 prev = at(0.0);
    for (int k = 0; k < 2; ++k) {
      const double ell[14] = {3.0 - k, 2.0, 0.0, 0, 0, 0, 1, 4.0 - k, -3.0, 0.5, 0, 0, 0, 1};      // two points, seen from (k, 0, 0)
      slide_detections_t det{};
      det.n_ell = 2; det.ell_pose7 = ell; det.ell_scale = scale; det.ell_label = labels;
      slide_frame_result_t res{};
      res.ell_match = match; res.ell_id = id;
      slide::Pose7 out;
      w.addSLOAMObservation(det, k == 0 ? at(0.0) : at(1.0), prev, 0, &out, &res);
      prev = out;
    }
    const std::array<int64_t, 4> st = w.gateStats();
    good = good && st[0] == 1 && st[1] == 1 && st[2] == 2 && st[3] == 0 && match[0] >= 0 && match[1] >= 0 && id[0] == 0 && id[1] == 1;
    std::printf("predicted gate ok verdicts=%d%d missing=%d stats=%lld,%lld,%lld,%lld\n", (int)(d2[0] < 11.345), (int)(d2[1] < 11.345), (int)missing,
                (long long)st[0], (long long)st[1], (long long)st[2], (long long)st[3]);
    return good ? 0 : 1;
  } catch (const slide::Error& e) {
    std::printf("slide::Error %d: %s\n", e.code, e.what());
    return 2;
  }
}
