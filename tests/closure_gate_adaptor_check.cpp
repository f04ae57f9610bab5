// Compile-and-run check of slide::SemanticFactorGraph::jointPoseCovariance and ::closureMahalanobis
// (include/slide_sloam_adaptor.hpp) against libslide_gpu.so: tests/test_closure_gate_adaptor.py builds it without a device (no
// argument: link check only) and runs it on the GPU (any argument), where the methods must return what the C calls return: a 12-pose
// chain along x, two closures that agree with it, one that is 3 m off, one naming a pose the graph does not hold.
#include <array>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "slide_sloam_adaptor.hpp"

static slide::Pose7 at(double x, double y = 0.0) {
  slide::Pose7 p;
  p.v[0] = x; p.v[1] = y;
  return p;
}
struct Mat12 {
  double a[144];
  double& operator()(int r, int c) { return a[12 * r + c]; }
};

int main(int argc, char** argv) {
  if (argc < 2) return 0;
  try {
    // odometry sigmas of 0.004 rad / 0.02 m per step: nine steps leave the far end about 0.1 m of lateral uncertainty, so a closure
    // 3 m off lies far outside the gate (at the default 0.1 rad per step it would not)
    slide_params_t prm;
    slide_default_params(&prm);
    for (int c = 0; c < 6; ++c) prm.noise_model_odom_vec[c] = c < 3 ? 0.004 : 0.02;
    slide::SemanticFactorGraph g(&prm);
    g.setPriors(at(0.0), 0);
    for (size_t k = 1; k < 12; ++k) g.addKeyPoseAndBetween(k - 1, k, at(1.0), at((double)k), 0);
    g.solve();
    const std::vector<slide::Pose7> rel = {at(-9.0), at(-9.0, 0.01), at(-9.0, 3.0), at(-9.0)};
    const std::vector<size_t> from = {9, 10, 10, 11}, to = {0, 1, 1, 40}, robot(4, 0);
    const std::vector<std::array<double, 6>> sigmas(4, std::array<double, 6>{0.01, 0.01, 0.01, 0.05, 0.05, 0.05});
    std::vector<int32_t> status;
    const std::vector<double> d2 = g.closureMahalanobis(rel, from, robot, to, robot, sigmas, &status);
    bool good = d2.size() == 4 && status.size() == 4 && d2[0] < 16.81 && d2[1] < 16.81 && d2[2] > 16.81 && d2[3] == 0.0;
    good = good && status[0] == SLIDE_OK && status[2] == SLIDE_OK && status[3] == SLIDE_MISSING;
    // the C call on the same closures
    std::vector<double> rel7, sg;
    for (const slide::Pose7& p : rel) rel7.insert(rel7.end(), p.v, p.v + 7);
    for (const auto& s6 : sigmas) sg.insert(sg.end(), s6.begin(), s6.end());
    const int32_t r4[4] = {0, 0, 0, 0};
    const uint64_t f4[4] = {9, 10, 10, 11}, t4[4] = {0, 1, 1, 40};
    double c4[4] = {-1, -1, -1, -1};
    good = good && slide_graph_closure_mahalanobis(g.handle(), 4, r4, f4, r4, t4, rel7.data(), sg.data(), c4, nullptr, nullptr, nullptr) == SLIDE_OK;
    for (int k = 0; good && k < 4; ++k) good = d2[k] == c4[k];
    // the joint marginal: its diagonal blocks are the single-pose getter's, its off-diagonal blocks each other's transposes
    const std::array<double, 144> J = g.jointPoseCovariance(2, 0, 9, 0);
    const Mat12 M = g.jointPoseCovariance<Mat12>(2, 0, 9, 0);
    const std::array<double, 36> c2 = g.getPoseCovariance(2, 0), c9 = g.getPoseCovariance(9, 0);
    for (int r = 0; good && r < 12; ++r)
      for (int c = 0; good && c < 12; ++c) good = M.a[12 * r + c] == J[12 * r + c] && J[12 * r + c] == J[12 * c + r];
    for (int r = 0; good && r < 6; ++r)
      for (int c = 0; good && c < 6; ++c) {
        const double e2 = J[12 * r + c] - c2[6 * r + c], e9 = J[12 * (r + 6) + c + 6] - c9[6 * r + c];
        good = (e2 < 0 ? -e2 : e2) <= 1e-9 * c9[21] && (e9 < 0 ? -e9 : e9) <= 1e-9 * c9[21];
      }
    bool threw = false;
    try { g.jointPoseCovariance(2, 0, 40, 0); } catch (const std::out_of_range&) { threw = true; }
    good = good && threw;
    std::printf("gate ok n=%zu verdicts=%d%d%d status3=%d\n", d2.size(), (int)(d2[0] < 16.81), (int)(d2[1] < 16.81), (int)(d2[2] < 16.81), (int)status[3]);
    return good ? 0 : 1;
  } catch (const slide::Error& e) {
    std::printf("slide::Error %d: %s\n", e.code, e.what());
    return 2;
  }
}
