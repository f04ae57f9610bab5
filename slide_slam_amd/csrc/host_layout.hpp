// Layout planning of the reduced pose system and of the exact joint step's border: pure host index arithmetic over the graph's
// host arrays.  No device call, no allocation on the device, no global state — HostGraph::upload_new (host_graph.hip) calls these between
// its uploads and moves the results into its members; tests/layout_plan_check.hip runs them alone, also under a host sanitizer.
//
//   plan_tile_profile      the tile-level profile of the reduced system (prof, first)
//   plan_border            the cuts of the pose chain (segments, separator poses), the border items and their permutation, the first
//                          block column of every border tile row, the per-segment activity tables — or a refusal
//   plan_segment_profiles  the segments' own profiles
//   plan_schur_pairs       the pair lists of the Schur assembly, or "walk"
//   plan_lm_slot           the landmark -> shared slot table
#pragma once
#include <algorithm>
#include <utility>
#include <vector>

#include "graph_dev.hpp"

namespace sl {

struct Seg { int t0, t1; };                          // tile columns [t0, t1) of a segment

// Profile of the reduced pose system at tile level.  reach(p) = the last pose coupled to pose p (a landmark both observe, a
// relative-pose factor); block column c reaches the tile row of the farthest reach of its poses; the running maximum over c is
// closed under the fill of the factorisation (eliminating column c fills rows <= prof[c] of columns <= prof[c] only).
// first[r]: the first block column whose profile reaches tile row r.  dense: ignore the structure (a measurement aid).
struct TileProfile { std::vector<int> prof, first; };
inline TileProfile plan_tile_profile(const std::vector<int>& reach, size_t Pn, bool dense) {
  const int T = (int)((6 * Pn + NB - 1) / NB);
  TileProfile out;
  std::vector<int>& prof = out.prof;
  std::vector<int>& first = out.first;
  prof.resize(T); first.resize(T);
  for (int c = 0; c < T; ++c) prof[c] = dense ? T - 1 : c;
  for (size_t p = 0; p < Pn && !dense; ++p) {
    const int rt = (6 * reach[p] + 5) / NB;
    const int ta = (int)(6 * p) / NB, tb = (int)(6 * p + 5) / NB;
    prof[ta] = std::max(prof[ta], rt);
    prof[tb] = std::max(prof[tb], rt);
  }
  for (int c = 1; c < T; ++c) prof[c] = std::max(prof[c], prof[c - 1]);
  for (int r = 0, c = 0; r < T; ++r) {
    while (prof[c] < r) ++c;
    first[r] = c;
  }
  return out;
}

// The exact joint step's border of one robot: its shared landmarks and the lambda coordinates of its relative-pose factors, behind the
// poses of the cuts of its own chain.
struct BorderPlan {
  const char* refused = nullptr;                       // non-null: the layout is refused with this message (an invalid argument); nothing else is set
  std::vector<int> lm_bord, sep_map, gh_bord;          // landmark -> border offset; global separator coordinate -> border coordinate; ghost factor -> border offset of its lambda coordinates
  std::vector<int> bfirst;                             // first block column per border tile row (+ one entry)
  int nbr = 0;                                         // border tile rows
  // nested dissection of the own pose chain
  std::vector<Seg> segs;
  std::vector<int> pose_sep;                           // pose -> border offset of a separator pose, or -1
  int nsep = 0, nsep_dim = 0, n_sep_poses = 0;
  // per segment: which border tile rows are non-zero in it and from which block column on (a shared landmark seen only from the first
  // half of the trajectory has no coupling to the second segment's poses; the poses of a cut couple to the few block columns before it and
  // to the segment behind it).  seg_ord[s]: the border tile rows in the order of that first column (the rows still all-zero at a block
  // column are then a suffix again, per segment); seg_sfirst[s]: the first columns in that order; seg_tab: what the border product
  // reads — nseg, the segments' last block columns + 1, then per segment the first column of every tile row + the right-hand side; from
  // seg_tab_head on the per-column activity masks; flat_ord: seg_ord end to end (the device's copy)
  std::vector<std::vector<int>> seg_ord, seg_sfirst;
  std::vector<int> seg_tab, flat_ord;
  int seg_tab_head = 0;
};
// lf_pose / lf_lm: the landmark factors' pose and landmark; lm_type: VT_* per landmark; lm_fids: per landmark its factors; bt_i / bt_j:
// the between factors' poses; sh_lid / sep_off: per shared slot its landmark (or < 0) and the global offset of its coordinates (one more
// entry: their total m); gh_pose / gh_gid: per ghost factor its pose and its index in the job's relative-pose list (lam_total: six lambda coordinates per entry of that list);
// want_seg: the requested segment count.
inline BorderPlan plan_border(size_t Pn, const std::vector<int>& h_lf_pose, const std::vector<int>& h_lf_lm, const std::vector<int>& h_lm_type,
                              const std::vector<std::vector<int>>& lm_fids, const std::vector<int>& h_bt_i, const std::vector<int>& h_bt_j,
                              const std::vector<int>& h_sh_lid, const std::vector<int>& h_sep_off, const std::vector<int>& h_gh_pose,
                              const std::vector<int>& h_gh_gid, int lam_total, int want_seg) {
  BorderPlan B;
  auto refuse = [](const char* msg) { BorderPlan R; R.refused = msg; return R; };
  const size_t Ln = h_lm_type.size(), nlf = h_lf_lm.size(), nbt = h_bt_i.size();
  const int ns = (int)h_sh_lid.size(), m = h_sep_off.back();
  const bool lam_on = lam_total > 0 && h_gh_gid.size() == h_gh_pose.size();
  if (lam_total > 0 && !lam_on) return refuse("exact joint step: slide_graph_set_ghost_ids must name every ghost factor of the graph");
  std::vector<int>&h_lm_bord = B.lm_bord, &h_sep_map = B.sep_map, &h_gh_bord = B.gh_bord, &h_bfirst = B.bfirst, &h_pose_sep = B.pose_sep;
  std::vector<Seg>& segs = B.segs;
  int &nsep = B.nsep, &nsep_dim = B.nsep_dim, &n_sep_poses = B.n_sep_poses;
  h_lm_bord.assign(std::max<size_t>(Ln, 1), -1);
  h_sep_map.assign(std::max(m + lam_total, 1), -1);
  h_gh_bord.assign(std::max<size_t>(h_gh_pose.size(), 1), -1);
  // border items: this robot's shared landmarks and the lambda coordinates of its relative-pose factors, ordered by the first block
  // column of the band in which their coupling row is non-zero (the first observing key frame) — the rows that are still all-zero at a
  // block column are then a SUFFIX of the border, which the steps and the border product skip (the maps below carry the permutation)
  // Nested dissection of the own pose chain (CholBatch::set_segments): cut the chain at n_seg - 1 places; the separator behind a cut at
  // pose q0 is [q0, q1) with q1 = 1 + the furthest pose any pose before q0 couples to (a landmark both observe, a relative-pose factor):
  // nothing couples across it.  Its poses become the FIRST border rows (whole tiles: the second level factors them as a dense system).
  h_pose_sep.assign(std::max<size_t>(Pn, 1), -1);
  std::vector<std::pair<int, int>> seg_cuts;        // the windows [q0, q1) of poses behind the segments (all but the last)
  // (reach: HostGraph keeps a twin of it incrementally, h_reach, the input of plan_tile_profile; this one is computed from the factor
  // lists as they stand and covers no ghost factor — the two are not merged)
  std::vector<int> reach;
  if (want_seg >= 2 && Pn >= 64) {
    std::vector<int> lm_last(Ln, -1);
    reach.assign(Pn, 0);
    for (size_t f = 0; f < nlf; ++f) lm_last[h_lf_lm[f]] = std::max(lm_last[h_lf_lm[f]], h_lf_pose[f]);
    for (size_t p = 0; p < Pn; ++p) reach[p] = (int)p;
    for (size_t f = 0; f < nlf; ++f) reach[h_lf_pose[f]] = std::max(reach[h_lf_pose[f]], lm_last[h_lf_lm[f]]);
    for (size_t b = 0; b < nbt; ++b) {
      const int lo = std::min(h_bt_i[b], h_bt_j[b]), hi = std::max(h_bt_i[b], h_bt_j[b]);
      reach[lo] = std::max(reach[lo], hi);
    }
    std::vector<int> run(Pn);                       // furthest reach of the poses 0 .. p
    for (size_t p = 0; p < Pn; ++p) run[p] = std::max(reach[p], p ? run[p - 1] : 0);
    std::vector<std::pair<int, int>> cuts;
    int seg_start = 0;
    bool ok = true;
    std::vector<Seg> tmp;
    for (int i = 1; i < want_seg && ok; ++i) {
      const int q0 = (int)(Pn * (size_t)i / want_seg);
      if (q0 <= seg_start + 8) continue;
      const int q1 = run[q0 - 1] + 1;
      if (q1 <= q0 || q1 + 8 >= (int)Pn) continue;      // (nothing couples across q0: no separator needed — or no room for a segment behind it)
      const Seg sg{6 * seg_start / NB, (6 * q0 + NB - 1) / NB};
      if (!tmp.empty() && sg.t0 < tmp.back().t1) { ok = false; break; }      // (a separator narrower than a tile: segments would share one)
      tmp.push_back(sg);
      cuts.emplace_back(q0, q1);
      seg_start = q1;
    }
    if (ok && !cuts.empty()) {
      const Seg last{6 * seg_start / NB, (int)((6 * Pn + NB - 1) / NB)};
      if (last.t0 >= tmp.back().t1) {
        tmp.push_back(last);
        segs = tmp;
        seg_cuts = cuts;
        for (const auto& c : cuts)
          for (int q = c.first; q < c.second; ++q) { h_pose_sep[q] = 6 * n_sep_poses; ++n_sep_poses; }
        nsep_dim = 6 * n_sep_poses;
        nsep = (nsep_dim + NB - 1) / NB;
      }
    }
  }
  struct Item { int cb, kind, id, dim, goff; };
  std::vector<Item> items;
  std::vector<char> taken((size_t)std::max(m, 0), 0);      // (a caller's own layout with overlapping slots would add two landmarks into the same separator coordinates)
  for (int i = 0; i < ns; ++i) {
    const int lid = h_sh_lid[i];
    if (lid < 0 || (size_t)lid >= Ln) continue;
    const int dim = lm_dim(h_lm_type[lid]);      // (the slots' coordinates may be laid out in any order: separator_offsets orders them along the robots' adjacency)
    if (h_sep_off[i] + dim > m) return refuse("separator offsets do not match the landmark classes of the shared slots");
    for (int k = 0; k < dim; ++k) {
      if (taken[(size_t)h_sep_off[i] + k]) return refuse("separator offsets: the coordinate ranges of two shared slots overlap");
      taken[(size_t)h_sep_off[i] + k] = 1;
    }
    int fp = 1 << 30;
    for (int f : lm_fids[lid]) fp = std::min(fp, h_lf_pose[f]);
    items.push_back(Item{fp == (1 << 30) ? 0 : 6 * fp / NB, 0, lid, dim, h_sep_off[i]});
  }
  if (lam_on)
    for (size_t q = 0; q < h_gh_pose.size(); ++q) {
      for (int k = 0; k < 6; ++k)
        if (h_sep_map[m + 6 * h_gh_gid[q] + k] == -2) return refuse("exact joint step: two ghost factors of one graph name the same measurement");
      for (int k = 0; k < 6; ++k) h_sep_map[m + 6 * h_gh_gid[q] + k] = -2;
      items.push_back(Item{6 * h_gh_pose[q] / NB, 1, (int)q, 6, m + 6 * h_gh_gid[q]});
    }
  std::stable_sort(items.begin(), items.end(), [](const Item& x, const Item& y) { return x.cb < y.cb; });
  int o = nsep * NB;                                 // (the separator poses' rows come first, in whole tiles)
  for (const Item& it : items) {
    if (it.kind == 0) h_lm_bord[it.id] = o; else h_gh_bord[it.id] = o;
    for (int k = 0; k < it.dim; ++k) h_sep_map[it.goff + k] = o + k;
    o += it.dim;
  }
  const int nbr_new = B.nbr = (o + NB - 1) / NB;
  h_bfirst.assign(nbr_new + 1, 0);
  for (int t = nsep; t < nbr_new; ++t) h_bfirst[t] = 1 << 30;      // (separator-pose rows: always active, 0)
  o = nsep * NB;
  for (const Item& it : items) {
    for (int t = o / NB; t <= (o + it.dim - 1) / NB; ++t) h_bfirst[t] = std::min(h_bfirst[t], it.cb);
    o += it.dim;
  }
  for (int t = 0; t < nbr_new; ++t) if (h_bfirst[t] == (1 << 30)) h_bfirst[t] = 0;
  for (int t = 1; t < nbr_new; ++t) h_bfirst[t] = std::max(h_bfirst[t], h_bfirst[t - 1]);      // (non-decreasing by construction; kept so by force)
  // per-segment activity of the border rows (BorderPlan)
  if (segs.empty()) return B;
  std::vector<std::vector<int>>&seg_ord = B.seg_ord, &seg_sfirst = B.seg_sfirst;
  std::vector<int>&seg_tab = B.seg_tab, &flat_ord = B.flat_ord;
  const int NS = (int)segs.size(), INF = 1 << 30;
  std::vector<std::vector<int>> sf(NS, std::vector<int>(nbr_new + 1, INF));
  auto seg_of = [&](int col) { for (int q = 0; q < NS; ++q) if (col >= segs[q].t0 && col < segs[q].t1) return q; return -1; };
  auto touch = [&](int t_lo, int t_hi, int pose) {
    if (pose < 0 || (size_t)pose >= Pn || h_pose_sep[pose] >= 0) return;      // (a cut's pose: that coupling lives in the border block)
    const int c = 6 * pose / NB, q = seg_of(c);
    if (q < 0) return;
    for (int t = t_lo; t <= t_hi; ++t) sf[q][t] = std::min(sf[q][t], c);
  };
  int o2 = nsep * NB;
  for (const Item& it : items) {
    const int t_lo = o2 / NB, t_hi = (o2 + it.dim - 1) / NB;
    if (it.kind == 0) { for (int f : lm_fids[it.id]) touch(t_lo, t_hi, h_lf_pose[f]); }
    else touch(t_lo, t_hi, h_gh_pose[it.id]);
    o2 += it.dim;
  }
  // the cuts' poses: window w lies between segment w and segment w + 1; before it, the poses whose reach crosses its start couple to
  // it (contiguous up to the cut); behind it, the segment's first block columns do
  int nb4 = 0;
  for (size_t w = 0; w < seg_cuts.size(); ++w) {
    const int q0 = seg_cuts[w].first, q1 = seg_cuts[w].second;
    const int t_lo = 6 * nb4 / NB, t_hi = (6 * (nb4 + q1 - q0) - 1) / NB;
    int pf = q0;
    for (int pz = q0 - 1; pz >= 0 && 6 * pz / NB >= segs[w].t0; --pz) if (reach[pz] >= q0) pf = pz;
    if (pf < q0) for (int t = t_lo; t <= t_hi; ++t) sf[w][t] = std::min(sf[w][t], std::max(6 * pf / NB, segs[w].t0));
    if (w + 1 < segs.size()) for (int t = t_lo; t <= t_hi; ++t) sf[w + 1][t] = std::min(sf[w + 1][t], segs[w + 1].t0);
    nb4 += q1 - q0;
  }
  seg_tab.push_back(NS);
  for (int q = 0; q < NS; ++q) seg_tab.push_back(segs[q].t1);
  for (int q = 0; q < NS; ++q) {
    sf[q][nbr_new] = segs[q].t0;                  // the right-hand-side row rides from the segment's first block column
    std::vector<int> ord(nbr_new);
    for (int t = 0; t < nbr_new; ++t) ord[t] = t;
    std::stable_sort(ord.begin(), ord.end(), [&](int a, int b) { return sf[q][a] < sf[q][b]; });
    std::vector<int> sorted(nbr_new + 1);
    for (int j = 0; j < nbr_new; ++j) sorted[j] = sf[q][ord[j]];
    sorted[nbr_new] = segs[q].t0;
    seg_ord.push_back(ord); seg_sfirst.push_back(sorted);
    flat_ord.insert(flat_ord.end(), ord.begin(), ord.end());
    seg_tab.insert(seg_tab.end(), sf[q].begin(), sf[q].end());
  }
  // and, behind it, per block column of the band the set of border tile rows some segment works on there (k_border_apply reads
  // only those): T, then T x (low, high) words of a 64-bit mask — T = 0: more than 64 border tile rows, no masks
  const int Tb = (int)((6 * Pn + NB - 1) / NB);
  B.seg_tab_head = (int)seg_tab.size();
  if (nbr_new <= 64) {
    seg_tab.push_back(Tb);
    for (int c = 0; c < Tb; ++c) {
      unsigned long long mask = 0;
      for (int q = 0; q < NS; ++q)
        if (c < segs[q].t1)
          for (int t = 0; t < nbr_new; ++t)
            if (sf[q][t] <= c && c >= segs[q].t0) mask |= 1ull << t;
      seg_tab.push_back((int)(unsigned)(mask & 0xffffffffull));
      seg_tab.push_back((int)(unsigned)(mask >> 32));
    }
  } else seg_tab.push_back(0);
  return B;
}

// The segments' own profiles (their rows end where the separator begins: what lay beyond moved into the border): per segment its
// profile in its own numbering, their offsets in `flat`, and the profiles end to end (the device's copy).
struct SegmentProfiles {
  std::vector<std::vector<int>> seg_prof;
  std::vector<size_t> seg_prof_off;
  std::vector<int> flat;
};
inline SegmentProfiles plan_segment_profiles(const std::vector<int>& h_prof, const std::vector<Seg>& segs) {
  SegmentProfiles out;
  for (const Seg& sg : segs) {
    std::vector<int> pv(sg.t1 - sg.t0);
    for (int c = sg.t0; c < sg.t1; ++c) pv[c - sg.t0] = std::min(h_prof[c], sg.t1 - 1) - sg.t0;
    out.seg_prof_off.push_back(out.flat.size());
    out.flat.insert(out.flat.end(), pv.begin(), pv.end());
    out.seg_prof.push_back(pv);
  }
  return out;
}

// Pair lists of the Schur assembly.  k_schur's block (pi, pj) is the sum over the pairs (factor x of pose pi, factor y of pose pj) on one
// landmark of F_x E_y^T; walking pose pi's list and looking every landmark up in pose pj's costs ~20 probes per block for ~2 hits.  Between
// the passes of a batched job the topology does not change, so the hits are listed once, in the order the walk finds them (x ascending
// in pi's list, y ascending in pj's).  Separator landmarks are left out (H_ll^-1 = 0 there: their F is zero).  Only inside a monotone
// profile whose strips are at most 256 poses wide; otherwise (walk) k_schur walks.
// idx[2 (pj W + d)], idx[.. + 1]: first pair and pair count of block (pj + d, pj); pairs: per pair the two E records (offset << 4 | tangent dimension)
struct SchurPairs {
  bool walk = true;
  int W = 1;
  std::vector<int> idx;
  std::vector<long long> pairs;
};
inline SchurPairs plan_schur_pairs(const std::vector<std::vector<int>>& pose_fids, const std::vector<std::vector<int>>& lm_fids,
                                   const std::vector<int>& h_prof, const std::vector<int>& h_lf_pose, const std::vector<int>& h_lf_lm,
                                   const std::vector<int64_t>& h_lf_eoff, const std::vector<int>& h_lm_type, const std::vector<int>& h_lm_bord,
                                   int64_t ebuf_used) {
  SchurPairs out;
  const int Pn = (int)pose_fids.size();
  if (Pn == 0 || h_prof.empty()) return out;
  auto p_end = [&](int pj) { return std::min(Pn, ((h_prof[(6 * pj + 5) / NB] + 1) * NB + 5) / 6); };
  int& W = out.W;
  for (int pj = 0; pj < Pn; ++pj) W = std::max(W, p_end(pj) - pj);
  if (W > 256) return out;
  // k_schur_lb addresses the E / F records by 32-bit byte offsets into ebuf — it truncates a pair entry's record offset to
  // (unsigned)(entry >> 4) and multiplies by eight — so every record has to end below 4 GB = 2^29 doubles; past that the walk runs
  if (ebuf_used >= (1LL << 29)) return out;
  std::vector<int>& idx = out.idx;
  std::vector<long long>& pairs = out.pairs;
  idx.assign((size_t)2 * Pn * W, 0);
  auto ed_of = [&](int f) {
    const int ty = h_lm_type[h_lf_lm[f]];
    return ((long long)h_lf_eoff[f] << 4) | (ty == VT_POINT ? 3 : (ty == VT_CUBE ? 9 : 7));
  };
  const bool have_bord = !h_lm_bord.empty();
  std::vector<std::vector<std::pair<int, int>>> rows(W);      // per d = pi - pj: (x, y) factor ids
  for (int pj = 0; pj < Pn; ++pj) {
    const int pe = p_end(pj);
    for (auto& r : rows) r.clear();
    // every factor y of pose pj: the other factors x of its landmark on poses pi in [pj, pe)
    for (int y : pose_fids[pj]) {
      const int l = h_lf_lm[y];
      if (have_bord && (size_t)l < h_lm_bord.size() && h_lm_bord[l] >= 0) continue;
      for (int x : lm_fids[l]) {
        const int pi = h_lf_pose[x];
        if (pi >= pj && pi < pe) rows[pi - pj].emplace_back(x, y);
      }
    }
    for (int d = 0; d < pe - pj; ++d) {
      auto& r = rows[d];
      if (r.empty()) continue;
      // the walk's order: x in the order of pose pi's list (landmark id, factor id), then y in the order of pose pj's list
      std::sort(r.begin(), r.end(), [&](const std::pair<int, int>& a, const std::pair<int, int>& b) {
        const int la = h_lf_lm[a.first], lb = h_lf_lm[b.first];
        if (la != lb) return la < lb;
        if (a.first != b.first) return a.first < b.first;
        return a.second < b.second;
      });
      idx[2 * ((size_t)pj * W + d)] = (int)(pairs.size() / 2);
      idx[2 * ((size_t)pj * W + d) + 1] = (int)r.size();
      for (const auto& xy : r) { pairs.push_back(ed_of(xy.first)); pairs.push_back(ed_of(xy.second)); }
    }
  }
  if (pairs.size() / 2 > (size_t)0x7fffffff) return out;
  out.walk = false;
  return out;
}

// The landmark -> shared slot table (-1: none).  onto: every slot that names a landmark (sh_lid[i] >= 0) is the slot its landmark's entry
// leads back to — no two slots on one landmark, none out of range; then the exact pass's back-substitution writes those landmarks'
// deltas itself (launch_arrow_finish_batched).
struct LmSlot { std::vector<int> slot; bool onto = true; };
inline LmSlot plan_lm_slot(const std::vector<int>& h_sh_lid, size_t Ln) {
  LmSlot out;
  std::vector<int>& slot = out.slot;
  slot.assign(std::max<size_t>(Ln, 1), -1);
  for (size_t i = 0; i < h_sh_lid.size(); ++i)
    if (h_sh_lid[i] >= 0 && (size_t)h_sh_lid[i] < Ln) slot[h_sh_lid[i]] = (int)i;
  for (size_t i = 0; i < h_sh_lid.size(); ++i)
    if (h_sh_lid[i] >= 0 && ((size_t)h_sh_lid[i] >= Ln || slot[h_sh_lid[i]] != (int)i)) out.onto = false;
  return out;
}

}  // namespace sl
