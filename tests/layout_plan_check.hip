// Stand-alone host program around the layout planner (slide_slam_amd/csrc/host_layout.hpp: the functions HostGraph::upload_new calls)
// — it touches no device.  tests/test_layout_plan_host.py compiles it, feeds it one case and compares every table it writes with the
// restatement in tests/layout_reference.py.  Built with -Xarch_host -fsanitize=address,undefined it is the sanitizer run of that text.
//
// Both files are streams of int64 words.  Input: op, then arrays as (length, words...); a list of lists travels as its CSR pair (ptr,
// val).  Output: the arrays of the result in the order written below, in the same form; a refusal's message as its characters.
#include <hip/hip_runtime.h>      // (graph_dev.hpp's device half wants its keywords; nothing of the runtime is called)

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "host_layout.hpp"

using namespace sl;
typedef std::vector<int64_t> Words;

static Words g_in;
static size_t g_at = 0;
static bool g_bad = false;
static Words next() {
  if (g_at >= g_in.size() || g_in[g_at] < 0 || (size_t)g_in[g_at] > g_in.size() - g_at - 1) { g_bad = true; return {}; }
  const size_t n = (size_t)g_in[g_at];
  Words w(g_in.begin() + g_at + 1, g_in.begin() + g_at + 1 + n);
  g_at += 1 + n;
  return w;
}
static std::vector<int> ints() { const Words w = next(); return std::vector<int>(w.begin(), w.end()); }
static std::vector<std::vector<int>> lists() {
  const std::vector<int> ptr = ints(), val = ints();
  std::vector<std::vector<int>> out;
  for (size_t i = 0; i + 1 < ptr.size(); ++i) {
    if (ptr[i] < 0 || ptr[i + 1] < ptr[i] || (size_t)ptr[i + 1] > val.size()) { g_bad = true; return {}; }
    out.emplace_back(val.begin() + ptr[i], val.begin() + ptr[i + 1]);
  }
  return out;
}

static Words g_out;
template <class V>
static void put(const V& v) {
  g_out.push_back((int64_t)v.size());
  for (const auto& x : v) g_out.push_back((int64_t)x);
}
template <class V>
static void put_lists(const std::vector<V>& vv) {      // the lengths, then the lists end to end
  Words len, flat;
  for (const V& v : vv) { len.push_back((int64_t)v.size()); flat.insert(flat.end(), v.begin(), v.end()); }
  put(len); put(flat);
}

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int64_t buf[256];
  size_t got;
  while ((got = std::fread(buf, sizeof(int64_t), 256, f)) > 0) g_in.insert(g_in.end(), buf, buf + got);
  std::fclose(f);
  if (g_in.empty()) return 2;
  const int op = (int)g_in[0];
  g_at = 1;
  if (op == 0) {                    // [Pn, dense], reach
    const Words sc = next();
    const std::vector<int> reach = ints();
    if (g_bad || sc.size() != 2) return 2;
    const TileProfile tp = plan_tile_profile(reach, (size_t)sc[0], sc[1] != 0);
    put(tp.prof); put(tp.first);
  } else if (op == 1) {             // [Pn, lam_total, want_seg], lf_pose, lf_lm, lm_type, lm_fids, bt_i, bt_j, sh_lid, sep_off, gh_pose, gh_gid
    const Words sc = next();
    const std::vector<int> lf_pose = ints(), lf_lm = ints(), lm_type = ints();
    const std::vector<std::vector<int>> lm_fids = lists();
    const std::vector<int> bt_i = ints(), bt_j = ints(), sh_lid = ints(), sep_off = ints(), gh_pose = ints(), gh_gid = ints();
    if (g_bad || sc.size() != 3) return 2;
    const BorderPlan B = plan_border((size_t)sc[0], lf_pose, lf_lm, lm_type, lm_fids, bt_i, bt_j, sh_lid, sep_off, gh_pose, gh_gid, (int)sc[1], (int)sc[2]);
    const char* msg = B.refused ? B.refused : "";
    put(std::vector<unsigned char>(msg, msg + std::strlen(msg)));
    put(std::vector<int>{B.nbr, B.nsep, B.nsep_dim, B.n_sep_poses, B.seg_tab_head});
    put(B.lm_bord); put(B.sep_map); put(B.gh_bord); put(B.bfirst);
    std::vector<int> segs;
    for (const Seg& sg : B.segs) { segs.push_back(sg.t0); segs.push_back(sg.t1); }
    put(segs); put(B.pose_sep);
    put_lists(B.seg_ord); put_lists(B.seg_sfirst);
    put(B.flat_ord); put(B.seg_tab);
  } else if (op == 2) {             // prof, segs (t0, t1 pairs)
    const std::vector<int> prof = ints(), flat = ints();
    if (g_bad || flat.size() % 2) return 2;
    std::vector<Seg> segs;
    for (size_t i = 0; i < flat.size(); i += 2) segs.push_back(Seg{flat[i], flat[i + 1]});
    const SegmentProfiles sp = plan_segment_profiles(prof, segs);
    put_lists(sp.seg_prof); put(sp.seg_prof_off); put(sp.flat);
  } else if (op == 3) {             // [ebuf_used], pose_fids, lm_fids, prof, lf_pose, lf_lm, lf_eoff, lm_type, lm_bord
    const Words sc = next();
    const std::vector<std::vector<int>> pose_fids = lists(), lm_fids = lists();
    const std::vector<int> prof = ints(), lf_pose = ints(), lf_lm = ints();
    const Words eoff = next();
    const std::vector<int> lm_type = ints(), lm_bord = ints();
    if (g_bad || sc.size() != 1) return 2;
    const SchurPairs sp = plan_schur_pairs(pose_fids, lm_fids, prof, lf_pose, lf_lm, eoff, lm_type, lm_bord, sc[0]);
    put(std::vector<int>{sp.walk ? 1 : 0, sp.W});
    if (sp.walk) { put(std::vector<int>()); put(std::vector<int>()); }      // (whatever a refused plan had listed so far is nobody's business)
    else { put(sp.idx); put(sp.pairs); }
  } else if (op == 4) {             // [Ln], sh_lid
    const Words sc = next();
    const std::vector<int> sh_lid = ints();
    if (g_bad || sc.size() != 1) return 2;
    const LmSlot ls = plan_lm_slot(sh_lid, (size_t)sc[0]);
    put(std::vector<int>{ls.onto ? 1 : 0});
    put(ls.slot);
  } else return 2;
  FILE* o = std::fopen(argv[2], "wb");
  if (!o) return 2;
  std::fwrite(g_out.data(), sizeof(int64_t), g_out.size(), o);
  std::fclose(o);
  std::printf("layout plan ok op=%d words=%zu\n", op, g_out.size());
  return 0;
}
