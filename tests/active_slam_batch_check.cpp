// Compile-and-run check of estimateClosureInfoGains of include/slide_sloam_adaptor.hpp (a list of loop-closure candidates ranked in one
// call) against libslide_gpu.so: tests/test_active_slam_batch_adaptor.py builds it without a device (no argument: link check only)
// and runs it on the GPU (any argument).
#include <cmath>
#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>

#include "slide_sloam_adaptor.hpp"

int main(int argc, char** argv) {
  if (argc < 2) return 0;
  try {
    slide::SemanticFactorGraph g;
    slide::Pose7 a, step;
    step.v[0] = 1.0;
    g.setPriors(a, 0);
    for (size_t k = 1; k < 8; ++k) {
      slide::Pose7 est;
      est.v[0] = (double)k;
      g.addKeyPoseAndBetween(k - 1, k, step, est, 0);
    }
    double xyz[3] = {2.0, 3.0, 0.0};
    g.addPointLandmarkKey(0, xyz);
    for (size_t k = 0; k < 4; ++k) {
      const double dx = 2.0 - (double)k, dy = 3.0, r = std::sqrt(dx * dx + dy * dy);
      const double b[3] = {dx / r, dy / r, 0.0};
      g.addRangeBearingFactor(k, 0, b, r, 0);
    }
    g.solve();
    const std::vector<std::vector<size_t>> trajs = {{7, 0}, {1, 0}, {7, 4, 0}};
    const std::vector<std::vector<double>> travels = {{3.0}, {3.0}, {2.0, 2.5}};
    const std::vector<double> many = g.estimateClosureInfoGains(trajs, travels);
    bool same = many.size() == 3;
    for (size_t k = 0; same && k < 3; ++k) {
      const double one = g.estimateClosureInfoGain(trajs[k], travels[k]);
      same = std::fabs(many[k] - one) <= 1e-9 * std::fabs(one);
    }
    bool threw = false, missing = false;
    try { g.estimateClosureInfoGain({70, 0}, {1.0}); } catch (const std::out_of_range&) {}      // (leaves no text a later message may carry)
    try {
      g.estimateClosureInfoGains({{7, 0}, {3, 0}}, {{3.0}, {0.0}});
    } catch (const slide::Error& e) {      // the candidate's own fault, in words of its own
      threw = e.code == SLIDE_ERR_INVALID && std::string(e.what()) == "estimateClosureInfoGains: candidate 1: fewer than two poses or a travel distance <= 0";
    }
    try { g.estimateClosureInfoGains({{7, 0}, {30, 0}}, {{3.0}, {1.0}}); } catch (const std::out_of_range&) { missing = true; }
    std::printf("batch ok n=%zu far=%.6e near=%.6e two_steps=%.6e\n", many.size(), many[0], many[1], many[2]);
    return same && many[0] > many[1] && many[1] > 0.0 && threw && missing ? 0 : 1;
  } catch (const slide::Error& e) {
    std::printf("slide::Error %d: %s\n", e.code, e.what());
    return 2;
  }
}
