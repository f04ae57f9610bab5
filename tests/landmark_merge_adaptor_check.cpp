// Compile-and-run check of slide::SemanticFactorGraph::mergeLandmarks / landmarkAlias / mergeDuplicateLandmarks
// (include/slide_sloam_adaptor.hpp) against libslide_gpu.so: tests/test_landmark_merge_adaptor.py builds it without a device (no
// argument: link check only) and runs it on the GPU (any argument), where the methods must do what the C calls do.  The graph of
// landmark_pair_adaptor_check.cpp: a 12-pose chain along x; point 0 seen from poses 0 and 1, point 1 at the same place seen from poses
// 2 and 3 (one object mapped twice), point 2 0.6 m to the side seen from poses 0, 1 and 2 (another object).
#include <array>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <stdexcept>
#include <vector>

#include "slide_sloam_adaptor.hpp"

using Graph = slide::SemanticFactorGraph;

static slide::Pose7 at(double x, double y = 0.0) {
  slide::Pose7 p;
  p.v[0] = x; p.v[1] = y;
  return p;
}
static void observe(Graph& g, size_t k, size_t lm, double x, double y) {
  const double q[3] = {x - (double)k, y, 0.0}, rho = std::sqrt(q[0] * q[0] + q[1] * q[1]);
  const std::array<double, 3> b = {q[0] / rho, q[1] / rho, 0.0};
  g.addRangeBearingFactor(k, lm, b, rho, 0);
}
static void build(Graph& g) {
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
}

int main(int argc, char** argv) {
  if (argc < 2) return 0;
  try {
    slide_params_t prm;
    slide_default_params(&prm);
    for (int c = 0; c < 6; ++c) prm.noise_model_odom_vec[c] = c < 3 ? 0.004 : 0.02;
    prm.bearing_range_sigma = 0.01;
    const std::vector<double> sigma = {0.05, 0.05, 0.05};
    // the search, the test and the merge together: exactly the planted duplicate, 1 into 0
    Graph g(&prm);
    build(g);
    Graph::MergeResult res;
    const std::vector<Graph::LandmarkMerge> rows = g.mergeDuplicateLandmarks(SLIDE_CLS_ELLIPSOID, 0.75, sigma, 0.99, true, &res);
    bool good = rows.size() == 1 && rows[0].keep == 0 && rows[0].drop == 1;
    good = good && res.into.size() == 1 && res.into[0] == 0 && res.moved[0] == 2 && res.status[0] == SLIDE_OK;
    good = good && g.landmarkAlias(SLIDE_CLS_ELLIPSOID, 1) == 0 && g.landmarkAlias(SLIDE_CLS_ELLIPSOID, 0) == 0 &&
           g.landmarkAlias(SLIDE_CLS_ELLIPSOID, 2) == 2;
    bool threw = false;
    try { (void)g.landmarkAlias(SLIDE_CLS_ELLIPSOID, 40); } catch (const std::out_of_range&) { threw = true; }
    good = good && threw;
    const std::array<double, 3> a0 = g.getCentroidLandmark(0), a1 = g.getCentroidLandmark(1);      // the alias reads the survivor
    good = good && a0[0] == a1[0] && a0[1] == a1[1] && a0[2] == a1[2];
    int64_t st5[5];
    good = good && slide_graph_stats(g.handle(), st5) == SLIDE_OK && st5[1] == 2;
    // the same merge by mergeLandmarks on a twin: the same fused estimate, bit for bit; then the C call's per-pair words
    Graph h(&prm);
    build(h);
    const Graph::MergeResult one = h.mergeLandmarks(SLIDE_CLS_ELLIPSOID, {{0, 1}}, true);
    const std::array<double, 3> b0 = h.getCentroidLandmark(0);
    good = good && one.moved.size() == 1 && one.moved[0] == 2 && b0[0] == a0[0] && b0[1] == a0[1] && b0[2] == a0[2];
    const Graph::MergeResult more = h.mergeLandmarks(SLIDE_CLS_ELLIPSOID, {{0, 1}, {0, 40}, {2, 2}, {2, 1}}, false);
    good = good && more.status[0] == SLIDE_OK && more.moved[0] == 0 && more.status[1] == SLIDE_MISSING && more.status[2] == SLIDE_ERR_INVALID &&
           more.status[3] == SLIDE_OK && more.moved[3] == 4 && more.into[3] == 2 && more.into[0] == 2;
    // an observation on the dropped key lands on the survivor, and the next solve is served
    observe(g, 4, 1, 3.0, 2.0);
    g.solve();
    h.solve();
    std::printf("landmark merge ok rows=%zu moved=%d alias=%zu n_lm=%lld status=%d,%d chain=%d\n", rows.size(), (int)res.moved[0],
                g.landmarkAlias(SLIDE_CLS_ELLIPSOID, 1), (long long)st5[1], (int)more.status[1], (int)more.status[2], (int)more.moved[3]);
    return good ? 0 : 1;
  } catch (const slide::Error& e) {
    std::printf("slide::Error %d: %s\n", e.code, e.what());
    return 2;
  }
}
