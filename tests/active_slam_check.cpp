// Compile-and-run check of the active-SLAM methods of include/slide_sloam_adaptor.hpp (logEntropy, estimateClosureInfoGain with the
// reference's argument lists, graph.h:106-115) against libslide_gpu.so: tests/test_active_slam_adaptor.py builds it without a device
// (no argument: link check only) and runs it on the GPU (any argument).
#include <cstdio>
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
    const auto e0 = g.logEntropy(0);
    const double far = g.estimateClosureInfoGain({7, 0}, {3.0});
    const double near = g.estimateClosureInfoGain({1, 0}, {3.0});
    const auto e1 = g.logEntropy(0);
    bool threw = false;
    try { g.estimateClosureInfoGain({7, 0}, {0.0}); } catch (const slide::Error&) { threw = true; }
    std::printf("active ok poses=%zu landmarks=%zu pose_trace=%.6e far=%.6e near=%.6e\n", e0.num_valid_poses, e0.num_valid_landmarks,
                e0.sum_entropy_pose, far, near);
    const bool ok = e0.num_valid_poses == 8 && e0.num_valid_landmarks == 1 && e0.sum_entropy_pose > 0.0 && e0.sum_entropy_landmark > 0.0 &&
                    far > near && near > 0.0 && threw && e1.sum_entropy_pose == e0.sum_entropy_pose;
    return ok ? 0 : 1;
  } catch (const slide::Error& e) {
    std::printf("slide::Error %d: %s\n", e.code, e.what());
    return 2;
  }
}
