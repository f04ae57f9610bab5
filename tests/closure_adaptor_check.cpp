// Compile-and-run check of slide::SemanticFactorGraph::selectConsistentClosures (include/slide_sloam_adaptor.hpp) against
// libslide_gpu.so: tests/test_closure_adaptor.py builds it without a device (no argument: link check only) and runs it on the GPU (any
// argument), where the method must return slide_graph_select_closures' keep mask: a 12-pose chain along x, three closures that agree
// with it and one that is 3 m off, and one naming a pose the graph does not hold.
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

int main(int argc, char** argv) {
  if (argc < 2) return 0;
  try {
    slide::SemanticFactorGraph g;
    g.setPriors(at(0.0), 0);
    for (size_t k = 1; k < 12; ++k) g.addKeyPoseAndBetween(k - 1, k, at(1.0), at((double)k), 0);
    g.solve();
    // closures from poses 9, 10, 11 back to poses 0, 1, 2: the true relative pose is 9 m back along x
    const std::vector<slide::Pose7> rel = {at(-9.0), at(-9.0, 0.01), at(-9.0), at(-9.0, 3.0), at(-9.0)};
    const std::vector<size_t> from = {9, 10, 11, 10, 11}, to = {0, 1, 2, 1, 40}, robot(5, 0);
    const std::vector<std::array<double, 6>> sigmas(5, std::array<double, 6>{0.01, 0.01, 0.01, 0.05, 0.05, 0.05});
    std::vector<int32_t> status;
    const std::vector<bool> keep = g.selectConsistentClosures(rel, from, robot, to, robot, sigmas, nullptr, &status);
    bool good = keep.size() == 5 && keep[0] && keep[1] && keep[2] && !keep[3] && !keep[4];
    good = good && status.size() == 5 && status[4] == SLIDE_MISSING && status[0] == SLIDE_OK && status[3] == SLIDE_OK;
    // the C call on the same closures
    std::vector<double> rel7, sg;
    for (const slide::Pose7& p : rel) rel7.insert(rel7.end(), p.v, p.v + 7);
    for (const auto& s6 : sigmas) sg.insert(sg.end(), s6.begin(), s6.end());
    const int32_t r5[5] = {0, 0, 0, 0, 0};
    const uint64_t f5[5] = {9, 10, 11, 10, 11}, t5[5] = {0, 1, 2, 1, 40};
    int32_t k5[5] = {0, 0, 0, 0, 0};
    int ng = 0;
    good = good && slide_graph_select_closures(g.handle(), 5, r5, f5, r5, t5, rel7.data(), sg.data(), nullptr, nullptr, k5, nullptr, nullptr, nullptr,
                                               nullptr, &ng) == SLIDE_OK && ng == 1;
    for (int k = 0; good && k < 5; ++k) good = keep[k] == (k5[k] != 0);
    std::printf("closure ok n=%zu keep=%d%d%d%d%d\n", keep.size(), (int)keep[0], (int)keep[1], (int)keep[2], (int)keep[3], (int)keep[4]);
    return good ? 0 : 1;
  } catch (const slide::Error& e) {
    std::printf("slide::Error %d: %s\n", e.code, e.what());
    return 2;
  }
}
