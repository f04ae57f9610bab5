// Compile-and-run check of slide::SemanticFactorGraph::setRobustLoss and ::closureWeights (include/slide_sloam_adaptor.hpp) against
// libslide_gpu.so: tests/test_robust_adaptor.py builds it without a device (no argument: link check only) and runs it on the GPU (any
// argument), where the methods must return what the C calls return: a 12-pose chain along x, one closure that agrees with it, one that
// is 3 m off, and a relative measurement that agrees, under Geman-McClure.
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
    for (size_t k = 1; k < 12; ++k) g.addKeyPoseAndBetween(k - 1, k, at(1.0), at((double)k), 0);
    g.addLoopClosureFactor(at(-9.0), 9, 0, 0, 0);
    g.addLoopClosureFactor(at(-9.0, 3.0), 10, 0, 1, 0);
    g.addRelativeMeasFactor(at(4.0), 2, 0, 6, 0);
    bool threw = false;
    try { g.setRobustLoss(7); } catch (const slide::Error& e) { threw = e.code == SLIDE_ERR_INVALID; }
    g.setRobustLoss(3, 0.0, true, false);          // Geman-McClure, default c, loop closures only
    g.solve();
    const std::vector<slide::SemanticFactorGraph::ClosureWeight> w = g.closureWeights();
    bool good = threw && w.size() == 3 && w[0].kind == 1 && w[1].kind == 1 && w[2].kind == 2;
    good = good && w[0].fromIdx == 9 && w[0].toIdx == 0 && w[1].fromIdx == 10 && w[1].toIdx == 1 && w[2].fromIdx == 2 && w[2].toIdx == 6;
    good = good && w[0].weight > 0.9 && w[1].weight < 0.1 && w[1].s2 > 1e6 && w[2].weight == 1.0;
    // the C call
    int32_t kd[3];
    double cw[3], cs[3];
    int n = 0;
    good = good && slide_graph_get_closure_weights(g.handle(), 3, nullptr, nullptr, nullptr, nullptr, kd, cw, cs, &n) == SLIDE_OK && n == 3;
    for (int k = 0; good && k < 3; ++k) good = cw[k] == w[k].weight && cs[k] == w[k].s2 && kd[k] == w[k].kind;
    g.setRobustLoss(0);
    g.solve();
    const auto off = g.closureWeights();
    good = good && off.size() == 3 && off[0].weight == 1.0 && off[1].weight == 1.0 && off[2].weight == 1.0;
    std::printf("robust ok n=%zu kept=%d%d rel=%d\n", w.size(), (int)(w[0].weight > 0.9), (int)(w[1].weight > 0.9), (int)(w[2].weight == 1.0));
    return good ? 0 : 1;
  } catch (const slide::Error& e) {
    std::printf("slide::Error %d: %s\n", e.code, e.what());
    return 2;
  }
}
