// Compile-and-run check of slide::SemanticFactorGraph::landmarkPairMahalanobis / jointLandmarkCovariance / findDuplicateLandmarks
// (include/slide_sloam_adaptor.hpp) against libslide_gpu.so: tests/test_landmark_pair_adaptor.py builds it without a device (no
// argument: link check only) and runs it on the GPU (any argument), where the methods must return what the C calls return: a 12-pose
// chain along x; point 0 seen from poses 0 and 1, point 1 at the same place seen from poses 2 and 3 (one object mapped twice), point 2
// 0.6 m to the side seen from poses 0, 1 and 2 (another object); a pair naming a landmark the graph does not hold.
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
// the range-bearing factor of the world point (x, y, 0) seen from the pose at (k, 0, 0), identity rotation
static void observe(Graph& g, size_t k, size_t lm, double x, double y) {
  const double q[3] = {x - (double)k, y, 0.0}, rho = std::sqrt(q[0] * q[0] + q[1] * q[1]);
  const std::array<double, 3> b = {q[0] / rho, q[1] / rho, 0.0};
  g.addRangeBearingFactor(k, lm, b, rho, 0);
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
    const std::array<double, 3> p0 = {3.01, 2.0, 0.0}, p1 = {3.0, 2.01, 0.0}, p2 = {3.0, 2.6, 0.01};
    g.addPointLandmarkKey(0, p0);
    g.addPointLandmarkKey(1, p1);
    g.addPointLandmarkKey(2, p2);
    for (size_t k = 0; k < 2; ++k) observe(g, k, 0, 3.0, 2.0);
    for (size_t k = 2; k < 4; ++k) observe(g, k, 1, 3.0, 2.0);
    for (size_t k = 0; k < 3; ++k) observe(g, k, 2, 3.0, 2.6);
    g.solve();
    const std::vector<double> sigma = {0.05, 0.05, 0.05};
    const std::vector<Graph::LandmarkPair> pairs = {{0, 1}, {0, 2}, {1, 2}, {0, 40}, {2, 2}};
    std::vector<int32_t> status, route;
    const std::vector<double> d2 = g.landmarkPairMahalanobis(SLIDE_CLS_ELLIPSOID, pairs, sigma, &status, &route);
    bool good = d2.size() == 5 && status.size() == 5 && route.size() == 5;
    good = good && d2[0] < 11.345 && d2[1] > 11.345 && d2[2] > 11.345 && d2[3] == 0.0 && d2[4] == 0.0;
    good = good && status[0] == SLIDE_OK && status[2] == SLIDE_OK && status[3] == SLIDE_MISSING && status[4] == SLIDE_ERR_INVALID;
    // the C call on the same pairs
    const int32_t cls[5] = {SLIDE_CLS_ELLIPSOID, SLIDE_CLS_ELLIPSOID, SLIDE_CLS_ELLIPSOID, SLIDE_CLS_ELLIPSOID, SLIDE_CLS_ELLIPSOID};
    const uint64_t ia[5] = {0, 0, 1, 0, 2}, ib[5] = {1, 2, 2, 40, 2};
    double c5[5] = {-1, -1, -1, -1, -1};
    good = good && slide_graph_landmark_pair_mahalanobis(g.handle(), 5, cls, ia, ib, sigma.data(), nullptr, c5, nullptr, nullptr, nullptr, nullptr,
                                                         nullptr) == SLIDE_OK;
    for (int k = 0; good && k < 5; ++k) good = d2[k] == c5[k];
    // the joint marginal: 6 x 6, symmetric, positive diagonal
    const std::vector<double> S = g.jointLandmarkCovariance(SLIDE_CLS_ELLIPSOID, 0, 1);
    good = good && S.size() == 36;
    for (int r = 0; good && r < 6; ++r) {
      good = S[7 * r] > 0.0;
      for (int q = 0; good && q < r; ++q) good = std::fabs(S[6 * r + q] - S[6 * q + r]) <= 1e-9 * std::sqrt(S[7 * r] * S[7 * q]);
    }
    // the search and the test together: exactly the planted duplicate
    const std::vector<Graph::DuplicateLandmark> dup = g.findDuplicateLandmarks(SLIDE_CLS_ELLIPSOID, 0.75, sigma);
    good = good && dup.size() == 1 && dup[0].a == 0 && dup[0].b == 1 && dup[0].d2 == d2[0] && dup[0].dist < 0.1;
    std::printf("landmark pairs ok n=%zu verdicts=%d%d%d status=%d,%d duplicates=%zu\n", d2.size(), (int)(d2[0] < 11.345), (int)(d2[1] < 11.345),
                (int)(d2[2] < 11.345), (int)status[3], (int)status[4], dup.size());
    return good ? 0 : 1;
  } catch (const slide::Error& e) {
    std::printf("slide::Error %d: %s\n", e.code, e.what());
    return 2;
  }
}
