// Compile-and-run check of slide::PlaceRecognition of include/slide_sloam_adaptor.hpp (findInterLoopClosureWithClipper for one pair of
// maps and findInterLoopClosuresWithClipper for the thread's loop) against libslide_gpu.so: tests/test_slidegraph_adaptor.py builds it
// without a device (no argument: link check only) and runs it on the GPU (any argument).
#include <array>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "slide_sloam_adaptor.hpp"

using Object = std::array<double, 7>;      // Eigen::Vector7d at the reference's call site
using Objects = std::vector<Object>;

static double uniform(uint64_t& x) {       // splitmix64 -> U[0, 1)
  x += 0x9E3779B97F4A7C15ull;
  uint64_t z = x;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  return (double)(z >> 11) * (1.0 / 9007199254740992.0);
}
// the reference map seen from a frame with ref = R(yaw) qry + t, objects in another order, one invalid (0, 0) row in front
static Objects view_of(const Objects& ref, double yaw, double tx, double ty, size_t shift) {
  Objects q;
  q.push_back(Object{1, 0, 0, 2.0, 0.5, 0.5, 0.5});
  const double c = std::cos(yaw), s = std::sin(yaw);
  for (size_t i = 0; i < ref.size(); ++i) {
    const Object& o = ref[(i + shift) % ref.size()];
    const double dx = o[1] - tx, dy = o[2] - ty;
    q.push_back(Object{o[0], c * dx + s * dy, -s * dx + c * dy, o[3], 0, 0, 0});
  }
  return q;
}

int main(int argc, char** argv) {
  if (argc < 2) return 0;
  try {
    uint64_t seed = 12345;
    Objects ref;
    for (int i = 0; i < 40; ++i) ref.push_back(Object{1, 60.0 * uniform(seed) - 30.0, 60.0 * uniform(seed) - 30.0, 0, 0, 0, 0});
    slide_slidegraph_params_t p;
    slide_slidegraph_default_params(&p);
    p.sigma = 0.05; p.epsilon = 0.15; p.num_inliers_threshold = 4;
    const slide::PlaceRecognition pr(&p);
    const double yaw[3] = {0.4, -1.3, 2.2}, tx[3] = {1.5, -3.0, 0.5}, ty[3] = {-2.0, 4.0, 2.5};
    std::vector<Objects> queries;
    for (int k = 0; k < 3; ++k) queries.push_back(view_of(ref, yaw[k], tx[k], ty[k], 7 * (size_t)k + 3));
    slide::Mat4 one;
    const bool found_one = pr.findInterLoopClosureWithClipper(ref, queries[0], one);
    std::vector<slide::Mat4> tfs;
    std::vector<bool> found;
    pr.findInterLoopClosuresWithClipper(ref, queries, tfs, found);
    bool good = found_one && tfs.size() == 3 && found.size() == 3;
    for (int k = 0; good && k < 3; ++k) {
      // tfFromQueryToRef: the query frame's pose in the reference frame (tolerances of tests/test_gpu_place.py's map test)
      good = found[k] && std::fabs(tfs[k](0, 0) - std::cos(yaw[k])) < 0.02 && std::fabs(tfs[k](1, 0) - std::sin(yaw[k])) < 0.02 &&
             std::fabs(tfs[k](0, 3) - tx[k]) < 0.3 && std::fabs(tfs[k](1, 3) - ty[k]) < 0.3 && tfs[k](3, 3) == 1.0;
    }
    for (int i = 0; good && i < 16; ++i) good = one.m[i] == tfs[0].m[i];          // the single call and the list: the same bits
    // a map below the gate: not found, identity
    Objects few(ref.begin(), ref.begin() + 10);
    slide::Mat4 none;
    good = good && !pr.findInterLoopClosureWithClipper(ref, few, none) && none(0, 0) == 1.0 && none(0, 3) == 0.0;
    std::printf("slidegraph ok n=%zu yaw0=%.6f tx0=%.6f ty0=%.6f\n", tfs.size(), tfs.empty() ? 0.0 : std::atan2(tfs[0](1, 0), tfs[0](0, 0)),
                tfs.empty() ? 0.0 : tfs[0](0, 3), tfs.empty() ? 0.0 : tfs[0](1, 3));
    return good ? 0 : 1;
  } catch (const slide::Error& e) {
    std::printf("slide::Error %d: %s\n", e.code, e.what());
    return 2;
  }
}
