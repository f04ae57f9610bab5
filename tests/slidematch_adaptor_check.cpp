// Compile-and-run check of the SlideMatch side of slide::PlaceRecognition of include/slide_sloam_adaptor.hpp (findInterLoopClosure for
// one pair of maps and findInterLoopClosures for the thread's loop) against libslide_gpu.so: tests/test_slidematch_adaptor.py builds
// it without a device (no argument: link check only) and runs it on the GPU (any argument), where both methods must return the C
// calls' values.
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
// the reference map seen from a frame with ref = R(yaw) qry + t, objects in another order
static Objects view_of(const Objects& ref, double yaw, double tx, double ty, size_t shift) {
  Objects q;
  const double c = std::cos(yaw), s = std::sin(yaw);
  for (size_t i = 0; i < ref.size(); ++i) {
    const Object& o = ref[(i + shift) % ref.size()];
    const double dx = o[1] - tx, dy = o[2] - ty;
    q.push_back(Object{o[0], c * dx + s * dy, -s * dx + c * dy, o[3], o[4], o[5], o[6]});
  }
  return q;
}
static void flatten(const Objects& m, std::vector<double>& out) {
  for (const Object& o : m)
    for (int c = 0; c < 7; ++c) out.push_back(o[c]);
}

int main(int argc, char** argv) {
  if (argc < 2) return 0;
  try {
    uint64_t seed = 777;
    Objects ref;
    for (int i = 0; i < 40; ++i)
      ref.push_back(Object{(double)(1 + i % 3), 24.0 * uniform(seed) - 12.0, 24.0 * uniform(seed) - 12.0, 0.4 * uniform(seed), 0.5, 0.5, 0.5});
    slide::PlaceRecognition pr;
    pr.place.search_yaw_step_size = 5.0 * M_PI / 180.0;
    pr.place.ignore_dimension = 1;
    const double yaw[3] = {0.35, -1.2, 2.0}, tx[3] = {2.5, -1.0, 0.5}, ty[3] = {-1.75, 2.0, 1.5};
    std::vector<Objects> queries;
    for (int k = 0; k < 3; ++k) queries.push_back(view_of(ref, yaw[k], tx[k], ty[k], 7 * (size_t)k + 3));
    queries.push_back(Objects());                                  // an empty map: not found, identity
    slide::Mat4 one;
    const bool found_one = pr.findInterLoopClosure(ref, queries[0], one);
    std::vector<slide::Mat4> tfs;
    std::vector<bool> found;
    pr.findInterLoopClosures(ref, queries, tfs, found);
    bool good = found_one && tfs.size() == 4 && found.size() == 4;
    // the C calls on the same rows
    std::vector<double> r7, flat;
    std::vector<int32_t> off(1, 0), pairs;
    flatten(ref, r7);
    flat = r7;
    off.push_back(40);
    for (int k = 0; k < 4; ++k) { flatten(queries[k], flat); off.push_back((int32_t)(flat.size() / 7)); pairs.push_back(0); pairs.push_back(k + 1); }
    double tfn[64];
    int32_t inl[4], f[4], st[4];
    good = good && slide_find_inter_loop_closures(flat.data(), off.data(), 5, pairs.data(), 4, &pr.place, tfn, inl, nullptr, f, nullptr, nullptr, st) == SLIDE_OK;
    for (int k = 0; good && k < 4; ++k) {
      good = st[k] == 0 && found[k] == (f[k] != 0) && found[k] == (k < 3);
      for (int i = 0; good && i < 16; ++i) good = tfs[k].m[i] == tfn[16 * k + i];
      if (k == 3) good = good && tfs[k](0, 0) == 1.0 && tfs[k](0, 3) == 0.0 && tfs[k](1, 0) == 0.0;
      if (good && k < 3)      // tfFromQueryToRef: the query frame's pose in the reference frame (tolerances of tests/test_gpu_place.py)
        good = std::fabs(std::atan2(tfs[k](1, 0), tfs[k](0, 0)) - yaw[k]) < 3.0 * M_PI / 180.0 && std::fabs(tfs[k](0, 3) - tx[k]) < 0.5 &&
               std::fabs(tfs[k](1, 3) - ty[k]) < 0.5;
    }
    std::vector<double> q7;
    flatten(queries[0], q7);
    double tf1[16];
    int inl1 = 0;
    good = good && slide_find_inter_loop_closure(r7.data(), 40, q7.data(), 40, &pr.place, tf1, &inl1, nullptr) == 1 && inl1 == inl[0];
    for (int i = 0; good && i < 16; ++i) good = one.m[i] == tf1[i] && one.m[i] == tfs[0].m[i];      // single, list, C: the same bits
    std::printf("slidematch ok n=%zu inliers0=%d yaw0=%.6f tx0=%.6f ty0=%.6f\n", tfs.size(), (int)inl[0],
                tfs.empty() ? 0.0 : std::atan2(tfs[0](1, 0), tfs[0](0, 0)), tfs.empty() ? 0.0 : tfs[0](0, 3), tfs.empty() ? 0.0 : tfs[0](1, 3));
    return good ? 0 : 1;
  } catch (const slide::Error& e) {
    std::printf("slide::Error %d: %s\n", e.code, e.what());
    return 2;
  }
}
