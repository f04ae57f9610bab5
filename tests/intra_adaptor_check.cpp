// Compile-and-run check of the same-robot side of include/slide_sloam_adaptor.hpp (slide::PlaceRecognition::findIntraLoopClosure with
// the reference's argument list, findIntraLoopClosures over a list of candidates, the free slide::getkeyPoseSubmaps) against
// libslide_gpu.so: tests/test_intra_adaptor.py builds it without a device (no argument: link check only) and runs it on the GPU (any
// argument), where the methods must return the C calls' values.
#include <array>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "slide_sloam_adaptor.hpp"

using Object = std::array<double, 7>;      // Eigen::Vector7d at the reference's call site
using Objects = std::vector<Object>;
namespace ref {                            // the reference's object classes as far as getkeyPoseSubmap and prepareLCInput read them
struct CylModel { double root[3], ray[3], radius; int semantic_label; };
struct BoxModel { slide::Pose7 pose; double scale[3]; int semantic_label; };
struct Cylinder { CylModel model; };
struct Cube { BoxModel model; };
struct Ellipsoid { BoxModel model; };
}  // namespace ref

static double uniform(uint64_t& x) {       // splitmix64 -> U[0, 1)
  x += 0x9E3779B97F4A7C15ull;
  uint64_t z = x;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  return (double)(z >> 11) * (1.0 / 9007199254740992.0);
}
static slide::Pose7 pose_at(double x, double y, double z, double yaw) {
  slide::Pose7 p;
  p.v[0] = x; p.v[1] = y; p.v[2] = z; p.v[5] = std::sin(yaw / 2); p.v[6] = std::cos(yaw / 2);
  return p;
}

int main(int argc, char** argv) {
  if (argc < 2) return 0;
  try {
    uint64_t seed = 4242;
    // a map of 90 cylinders, 60 cubes and 60 ellipsoids within 30 m of the origin, one floor
    std::vector<ref::Cylinder> cyls;
    std::vector<ref::Cube> cubes;
    std::vector<ref::Ellipsoid> ells;
    for (int i = 0; i < 90; ++i)
      cyls.push_back(ref::Cylinder{{{60.0 * uniform(seed) - 30.0, 60.0 * uniform(seed) - 30.0, 0.2 * uniform(seed)}, {0.05, -0.02, 1.0}, 0.2 + 0.2 * uniform(seed), 1}});
    for (int i = 0; i < 120; ++i) {
      ref::BoxModel m{pose_at(60.0 * uniform(seed) - 30.0, 60.0 * uniform(seed) - 30.0, 0.3 * uniform(seed), 0.0), {0.5 + uniform(seed), 0.5 + uniform(seed), 0.5 + uniform(seed)}, 2 + i % 2};
      if (i < 60) cubes.push_back(ref::Cube{m}); else ells.push_back(ref::Ellipsoid{m});
    }
    // candidate key poses: two near the query, one far above the map (an empty submap)
    const std::vector<slide::Pose7> cands = {pose_at(3.1, -2.3, 0.1, -0.2), pose_at(4.7, -1.1, 0.2, 1.1), pose_at(0.1, 0.2, 50.3, 0.0)};
    const std::vector<Objects> submaps = slide::getkeyPoseSubmaps(cyls, cubes, ells, cands, 20.0);
    bool good = submaps.size() == 3 && submaps[0].size() > 20 && submaps[1].size() > 20 && submaps[2].empty();
    // 20 detections: objects of submap 0 seen from the true query pose; the query pose handed over has drifted
    const double yaw = 0.6, tq[3] = {3.6, -1.9, 0.1};
    const slide::Pose7 drifted = pose_at(tq[0] + 0.8, tq[1] - 0.6, tq[2], yaw + 4.0 * M_PI / 180.0);
    Objects meas;
    for (size_t i = 0; good && i < 20; ++i) {
      const Object& o = submaps[0][i * (submaps[0].size() / 20)];
      const double c = std::cos(yaw), s = std::sin(yaw), dx = o[1] - tq[0], dy = o[2] - tq[1];
      meas.push_back(Object{o[0], c * dx + s * dy, -s * dx + c * dy, o[3] - tq[2], o[4], o[5], o[6]});
    }
    slide::PlaceRecognition pr;
    slide::Mat4 one;
    const bool found_one = good && pr.findIntraLoopClosure(submaps[0], meas, drifted, cands[0], one);
    std::vector<slide::Mat4> tfs;
    std::vector<bool> found;
    pr.findIntraLoopClosures(submaps, meas, drifted, cands, tfs, found);
    good = good && found_one && tfs.size() == 3 && found.size() == 3 && found[0] && found[1] && !found[2];
    // the C calls on the same rows
    std::vector<double> flat, m7, c7;
    std::vector<int32_t> off(1, 0);
    for (const Objects& sm : submaps) {
      for (const Object& o : sm) flat.insert(flat.end(), o.begin(), o.end());
      off.push_back((int32_t)(flat.size() / 7));
    }
    for (const Object& o : meas) m7.insert(m7.end(), o.begin(), o.end());
    for (const slide::Pose7& p : cands) c7.insert(c7.end(), p.v, p.v + 7);
    double tfn[48];
    int32_t inl[3] = {0, 0, 0}, f[3], st[3];
    good = good && slide_find_intra_loop_closures(m7.data(), 20, drifted.v, flat.data(), off.data(), 3, c7.data(), &pr.place, 5.0, 5.0, 10.0 * M_PI / 180.0,
                                                  tfn, inl, nullptr, f, nullptr, nullptr, st) == SLIDE_OK;
    for (int k = 0; good && k < 3; ++k) {
      good = st[k] == 0 && found[k] == (f[k] != 0);
      for (int i = 0; good && i < 16; ++i) good = tfs[k].m[i] == tfn[16 * k + i];
      if (k == 2) good = good && tfs[k](0, 0) == 1.0 && tfs[k](0, 3) == 0.0 && tfs[k](1, 0) == 0.0;
    }
    double tf1[16];
    int inl1 = 0;
    good = good && slide_find_intra_loop_closure(m7.data(), 20, flat.data(), off[1], drifted.v, cands[0].v, &pr.place, 5.0, 5.0, 10.0 * M_PI / 180.0, tf1,
                                                 &inl1, nullptr) == 1 && inl1 == inl[0];
    for (int i = 0; good && i < 16; ++i) good = one.m[i] == tf1[i] && one.m[i] == tfs[0].m[i];      // single, list, C: the same bits
    std::printf("intra ok n=%zu sizes=%zu,%zu,%zu inliers0=%d inliers1=%d\n", tfs.size(), submaps.size() > 0 ? submaps[0].size() : 0,
                submaps.size() > 1 ? submaps[1].size() : 0, submaps.size() > 2 ? submaps[2].size() : 0, (int)inl[0], (int)inl[1]);
    return good ? 0 : 1;
  } catch (const slide::Error& e) {
    std::printf("slide::Error %d: %s\n", e.code, e.what());
    return 2;
  }
}
