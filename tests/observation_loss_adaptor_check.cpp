// Compile-and-run check of slide::SemanticFactorGraph::setObservationLoss and ::observationWeights (include/slide_sloam_adaptor.hpp)
// against libslide_gpu.so: tests/test_observation_loss_adaptor.py builds it without a device (no argument: link check only) and runs
// it on the GPU (any argument), where the methods must return what the C calls return: a 4-pose chain along x, two point landmarks
// seen from every pose, one of the observations 10 m off in range (ten default sigmas), under Geman-McClure.
#include <array>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "slide_sloam_adaptor.hpp"

static slide::Pose7 at(double x, double y = 0.0) {
  slide::Pose7 p;
  p.v[0] = x; p.v[1] = y;
  return p;
}

int main(int argc, char** argv) {
  if (argc < 2) return 0;
  try {
    slide::SemanticFactorGraph g;
    g.setPriors(at(0.0), 0);
    for (size_t k = 1; k < 4; ++k) g.addKeyPoseAndBetween(k - 1, k, at(1.0), at((double)k), 0);
    const double lm[2][3] = {{2.0, 3.0, 0.5}, {1.0, -4.0, 1.0}};
    for (size_t l = 0; l < 2; ++l) {
      g.addPointLandmarkKey(l, std::array<double, 3>{lm[l][0], lm[l][1], lm[l][2]});
      for (size_t k = 0; k < 4; ++k) {
        const std::array<double, 3> q{lm[l][0] - (double)k, lm[l][1], lm[l][2]};
        const double rho = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2]);
        g.addRangeBearingFactor(k, l, std::array<double, 3>{q[0] / rho, q[1] / rho, q[2] / rho}, rho + (l == 1 && k == 2 ? 10.0 : 0.0), 0);
      }
    }
    bool threw = false;
    try { g.setObservationLoss(7); } catch (const slide::Error& e) { threw = e.code == SLIDE_ERR_INVALID; }
    g.setObservationLoss(3);          // Geman-McClure, default c, every class
    g.solve();
    const std::vector<slide::SemanticFactorGraph::ObservationWeight> w = g.observationWeights();
    bool good = threw && w.size() == 8;
    int down = 0;
    for (size_t f = 0; good && f < 8; ++f) {
      good = w[f].robot == 0 && w[f].poseIdx == f % 4 && w[f].lmIdx == f / 4 && w[f].cls == SLIDE_CLS_ELLIPSOID;
      if (f == 6) good = good && w[f].weight < 1e-3 && w[f].s2 > 99.0 && w[f].s2 < 101.0;
      else good = good && w[f].weight == 1.0 && w[f].s2 < 1e-20;
      down += w[f].weight < 1.0;
    }
    // the C call
    int32_t cl[8];
    uint64_t li[8];
    double cw[8], cs[8];
    int n = 0;
    good = good && slide_graph_get_observation_weights(g.handle(), 8, nullptr, nullptr, cl, li, cw, cs, &n) == SLIDE_OK && n == 8;
    for (int k = 0; good && k < 8; ++k) good = cw[k] == w[k].weight && cs[k] == w[k].s2 && cl[k] == w[k].cls && li[k] == w[k].lmIdx;
    g.setObservationLoss(3, 0.0, false, true, true);          // the points' class left out
    g.solve();
    const auto off = g.observationWeights();
    good = good && off.size() == 8;
    for (size_t f = 0; good && f < 8; ++f) good = off[f].weight == 1.0;
    std::printf("observation loss ok n=%zu down=%d\n", w.size(), down);
    return good ? 0 : 1;
  } catch (const slide::Error& e) {
    std::printf("slide::Error %d: %s\n", e.code, e.what());
    return 2;
  }
}
