// Host side of SlideGraph (semantic CLIPPER, semantic_clipper.cpp; findInterLoopClosureWithClipper, place_recognition.cpp:541-629):
// triangle matching and the clique solve for one pair of maps and for a list of pairs, and their extern "C" entry points
// (include/slide_gpu.h).  The solves go through host_clipper.hpp's one path.
#include <cmath>

#include "delaunay.hpp"
#include "host_clipper.hpp"

using namespace sl;

namespace {
// ---- PlaceRecognition::findInterLoopClosureWithClipper place_recognition.cpp:541-629 for a list of map pairs ----------------------------
struct MapView { const double* rows7; int n; };
struct MapTris {                       // one map, filtered (:584, :601) and triangulated ONCE however many pairs name it
  bool filtered = false, triangulated = false;
  std::vector<double> xy;              // the kept rows' (x, y)
  std::vector<double> tri;             // 6 doubles per Delaunay triangle (semantic_clipper.cpp:150-165)
  int kept = 0, ntri = 0, tri0 = -1;   // tri0: first triangle in the prepared arrays of all maps
};

// Outputs are initialised by the caller; every pair is evaluated by itself.  Stages: host filter + gate + Delaunay; ONE k_tri_prepare;
// k_tri_match_seg count, segmented scan, read-back 1 (matched pairs per map pair); k_tri_match_seg emit straight into P1 / P2;
// k_affinity_csr_seg count, segmented scan into per-pair row pointers, read-back 2 (non-zeros per pair); emit; ONE k_clq_solve_b for
// the pairs below the cooperative threshold; read-back 3 (out4, u, P1, P2 of all pairs, one buffer); the pairs at or above the
// threshold one after another through solve_csr_device on their slice; rounding, estimate_tf and the inverse on the host.
int inter_loop_closures_clipper(const std::vector<MapView>& maps, const int32_t* pairs, int n_pairs, const slide_slidegraph_params_t& G,
                                const double* const* u0, const int* n_u0, double* tf16n, int32_t* counts4n, int32_t* found,
                                int32_t* status) {
  std::vector<MapTris> M(maps.size());
  auto filter = [&](int i) {
    MapTris& m = M[i];
    if (m.filtered) return;
    m.filtered = true;
    for (int r = 0; r < maps[i].n; ++r) {
      const double x = maps[i].rows7[7 * (size_t)r + 1], y = maps[i].rows7[7 * (size_t)r + 2];
      if (x == 0.0 && y == 0.0) continue;
      m.xy.push_back(x); m.xy.push_back(y);
    }
    m.kept = (int)(m.xy.size() / 2);
  };
  auto triangulate = [&](int i) {
    MapTris& m = M[i];
    if (m.triangulated) return;
    m.triangulated = true;
    const std::vector<std::array<int32_t, 3>> t = delaunay::triangulate(m.xy.data(), m.kept);
    m.tri.resize(6 * t.size());
    for (size_t k = 0; k < t.size(); ++k)
      for (int v = 0; v < 3; ++v) { m.tri[6 * k + 2 * v] = m.xy[2 * t[k][v]]; m.tri[6 * k + 2 * v + 1] = m.xy[2 * t[k][v] + 1]; }
    m.ntri = (int)t.size();
  };
  auto fail = [&](int k, int rc) { if (status) status[k] = rc; };
  // the segments: pairs that pass the gate (:618) and have triangles on both sides
  std::vector<int> seg_pair;
  std::vector<int> rowoff(1, 0);
  for (int k = 0; k < n_pairs; ++k) {
    const int a = pairs[2 * k], b = pairs[2 * k + 1];
    filter(a); filter(b);
    counts4n[4 * k] = M[a].kept; counts4n[4 * k + 1] = M[b].kept;
    if (M[a].kept < G.min_num_map_objects_to_start || M[b].kept < G.min_num_map_objects_to_start) continue;
    triangulate(a); triangulate(b);
    if (M[a].ntri == 0 || M[b].ntri == 0) continue;
    if ((long long)rowoff.back() + M[a].ntri > INT32_MAX) { fail(k, SLIDE_ERR_CAPACITY); continue; }
    seg_pair.push_back(k);
    rowoff.push_back(rowoff.back() + M[a].ntri);
  }
  const int n_seg = (int)seg_pair.size(), n_rows = rowoff.back();
  if (n_seg == 0) return SLIDE_OK;
  if (slide_device_check(-1) != SLIDE_OK) return SLIDE_ERR_HIP;
  slide_clipper_params_t P = clipper_params_or_default(nullptr);
  P.sigma = G.sigma;
  P.epsilon = G.epsilon;
  // the triangles of every map a segment names, one after the other
  std::vector<double> tri_all;
  std::vector<TriSeg> segs(n_seg);
  for (int s = 0; s < n_seg; ++s) {
    const int k = seg_pair[s];
    for (int side = 0; side < 2; ++side) {
      MapTris& m = M[pairs[2 * k + side]];
      if (m.tri0 >= 0) continue;
      if (tri_all.size() / 6 + (size_t)m.ntri > (size_t)INT32_MAX) { g_last_error = "more than 2^31 triangles in the list's maps"; return SLIDE_ERR_CAPACITY; }
      m.tri0 = (int)(tri_all.size() / 6);
      tri_all.insert(tri_all.end(), m.tri.begin(), m.tri.end());
    }
    segs[s] = TriSeg{M[pairs[2 * k]].tri0, M[pairs[2 * k + 1]].tri0, M[pairs[2 * k + 1]].ntri};
  }
  const int n_tri = (int)(tri_all.size() / 6);
  Tmp T;
  double* d_tri = T.up(tri_all.data(), tri_all.size());
  double* d_sd = T.up<double>(nullptr, 3 * (size_t)n_tri);
  double* d_sx = T.up<double>(nullptr, 6 * (size_t)n_tri);
  int* d_rowoff = T.up(rowoff.data(), rowoff.size());
  TriSeg* d_segs = T.up(segs.data(), segs.size());
  int* d_tcnt = T.up<int>(nullptr, n_rows);
  long long* d_toff = T.up<long long>(nullptr, n_rows);
  long long* d_tot = T.up<long long>(nullptr, n_seg);
  if (!d_tri || !d_sd || !d_sx || !d_rowoff || !d_segs || !d_tcnt || !d_toff || !d_tot) { g_last_error = "hipMalloc/hipMemcpy failed"; return SLIDE_ERR_HIP; }
  launch_tri_prepare(d_tri, n_tri, d_sd, d_sx, nullptr);
  launch_tri_match_seg(false, d_sd, d_sx, d_rowoff, d_segs, n_seg, n_rows, G.matching_threshold, d_tcnt, nullptr, nullptr, nullptr, nullptr, nullptr);
  launch_seg_scan64(d_tcnt, d_rowoff, n_seg, d_toff, d_tot, nullptr);
  SL_HIP(hipGetLastError());
  std::vector<long long> tot(n_seg);
  SL_HIP(hipMemcpy(tot.data(), d_tot, sizeof(long long) * n_seg, hipMemcpyDeviceToHost));                 // read-back 1
  // associations per pair; a pair's own faults drop it here (base < 0: nothing of it is emitted)
  std::vector<long long> base(n_seg, -1);
  std::vector<int> aoff(n_seg + 1, 0);
  for (int s = 0; s < n_seg; ++s) {
    const int k = seg_pair[s];
    aoff[s + 1] = aoff[s];
    if (tot[s] > (1LL << 30) / 3 || (long long)aoff[s] + 3 * tot[s] > (1LL << 30)) { fail(k, SLIDE_ERR_CAPACITY); continue; }
    const int m = (int)(3 * tot[s]);
    counts4n[4 * k + 2] = m;
    if (m == 0) continue;
    if (u0 && u0[k] && n_u0[k] != m) { fail(k, SLIDE_ERR_INVALID); continue; }
    base[s] = aoff[s] / 3;
    aoff[s + 1] = aoff[s] + m;
  }
  const int n_assoc = aoff[n_seg];
  if (n_assoc == 0) return SLIDE_OK;
  // one result buffer for the one read-back at the end: [out4 per segment | u | P1 | P2]
  const size_t res_len = 4 * (size_t)n_seg + 5 * (size_t)n_assoc;
  double* d_res = T.up<double>(nullptr, res_len);
  long long* d_base = T.up(base.data(), base.size());
  int* d_aoff = T.up(aoff.data(), aoff.size());
  int* d_rcnt = T.up<int>(nullptr, n_assoc);
  int* d_rptr = T.up<int>(nullptr, (size_t)n_assoc + n_seg);
  if (!d_res || !d_base || !d_aoff || !d_rcnt || !d_rptr) { g_last_error = "hipMalloc/hipMemcpy failed"; return SLIDE_ERR_HIP; }
  double* d_p1 = d_res + 4 * (size_t)n_seg + n_assoc;
  double* d_p2 = d_p1 + 2 * (size_t)n_assoc;
  SL_HIP(hipMemsetAsync(d_res, 0, (4 * (size_t)n_seg + (size_t)n_assoc) * sizeof(double), nullptr));
  launch_tri_match_seg(true, d_sd, d_sx, d_rowoff, d_segs, n_seg, n_rows, G.matching_threshold, nullptr, d_toff, d_base, d_p1, d_p2, nullptr);
  launch_affinity_csr_seg(false, d_p1, d_p2, d_aoff, n_seg, n_assoc, P.sigma, P.epsilon, P.mindist, P.affinityeps, d_rcnt, nullptr, nullptr, nullptr,
                          nullptr, nullptr);
  launch_seg_scan_rowptr(d_rcnt, d_aoff, n_seg, d_rptr, d_tot, nullptr);
  SL_HIP(hipGetLastError());
  SL_HIP(hipMemcpy(tot.data(), d_tot, sizeof(long long) * n_seg, hipMemcpyDeviceToHost));                 // read-back 2
  std::vector<long long> nnz0(n_seg, -1);
  long long nnz_all = 0;
  for (int s = 0; s < n_seg; ++s) {
    if (aoff[s + 1] == aoff[s]) continue;
    if (tot[s] > INT32_MAX) { fail(seg_pair[s], SLIDE_ERR_CAPACITY); continue; }      // ClqSolve::rowptr is per problem, 32 bits
    nnz0[s] = nnz_all;
    nnz_all += tot[s];
  }
  long long* d_nnz0 = T.up(nnz0.data(), nnz0.size());
  int* d_col = T.up<int>(nullptr, (size_t)std::max<long long>(nnz_all, 1));
  double* d_val = T.up<double>(nullptr, (size_t)std::max<long long>(nnz_all, 1));
  if (!d_nnz0 || !d_col || !d_val) { g_last_error = "hipMalloc/hipMemcpy failed"; return SLIDE_ERR_HIP; }
  launch_affinity_csr_seg(true, d_p1, d_p2, d_aoff, n_seg, n_assoc, P.sigma, P.epsilon, P.mindist, P.affinityeps, nullptr, d_rptr, d_nnz0, d_col, d_val,
                          nullptr);
  // the solves (solve_csr_segments): one launch for every pair below the single call's cooperative threshold
  double* d_work = T.up<double>(nullptr, 6 * (size_t)n_assoc);
  if (!d_work) { g_last_error = "hipMalloc failed"; return SLIDE_ERR_HIP; }
  std::vector<const double*> seg_u0(n_seg, nullptr);
  for (int s = 0; u0 && s < n_seg; ++s) seg_u0[s] = u0[seg_pair[s]];
  const ClqSegments segments{n_seg, aoff.data(), d_aoff, d_rptr, d_col, d_val, nnz0.data(), tot.data(), d_work, d_res, res_len};
  std::vector<double> res;
  return solve_csr_segments(T, segments, seg_u0, P, res, [&](int s, const std::vector<int>& nodes, const std::vector<double>&, double) {      // read-back 3
    const int k = seg_pair[s];
    const double* h_p1 = res.data() + 4 * (size_t)n_seg + n_assoc;
    const double* h_p2 = h_p1 + 2 * (size_t)n_assoc;
    counts4n[4 * k + 3] = (int)nodes.size();
    if ((int)nodes.size() < G.num_inliers_threshold) return;
    std::vector<double> a(2 * nodes.size()), b(2 * nodes.size());
    for (size_t i = 0; i < nodes.size(); ++i) {
      const size_t j = (size_t)aoff[s] + nodes[i];
      a[2 * i] = h_p1[2 * j]; a[2 * i + 1] = h_p1[2 * j + 1]; b[2 * i] = h_p2[2 * j]; b[2 * i + 1] = h_p2[2 * j + 1];
    }
    double tf3[9];
    estimate_tf2d(a.data(), b.data(), (int)nodes.size(), tf3);
    // run_semantic_clipper's 4x4 (yaw + xy, semantic_clipper.cpp:255-268) and its inverse (place_recognition.cpp:624): R^T, -R^T t
    const double yaw = std::atan2(tf3[3], tf3[0]), c = std::cos(yaw), sn = std::sin(yaw), tx = tf3[2], ty = tf3[5];
    double* tf = tf16n + 16 * (size_t)k;
    tf[0] = c; tf[1] = sn; tf[4] = -sn; tf[5] = c;
    tf[3] = -(c * tx + sn * ty); tf[7] = -(-sn * tx + c * ty);
    found[k] = 1;
  });
}
}  // namespace

extern "C" {
int slide_match_triangles(const double* tri_model, int ntm, const double* tri_data, int ntd, double threshold, double* pts_out,
                          double* diffs_out, int cap_pairs, int* n_pairs) {
  if (slide_device_check(-1) != SLIDE_OK) return SLIDE_ERR_HIP;
  if (!n_pairs || ntm < 0 || ntd < 0) return SLIDE_ERR_INVALID;
  Tmp T;
  double *dp = nullptr, *dd = nullptr;
  long long np = 0;
  const int rc = match_triangles_device(T, tri_model, ntm, tri_data, ntd, threshold, &dp, &dd, &np);
  if (rc != SLIDE_OK) return rc;
  if (np > 2147483647LL) { g_last_error = "more than 2^31 matched triangle pairs"; return SLIDE_ERR_CAPACITY; }
  *n_pairs = (int)np;
  const long long w = std::min<long long>(np, cap_pairs);
  if (w > 0 && pts_out) SL_HIP(hipMemcpy(pts_out, dp, sizeof(double) * 12 * (size_t)w, hipMemcpyDeviceToHost));
  if (w > 0 && diffs_out) SL_HIP(hipMemcpy(diffs_out, dd, sizeof(double) * (size_t)w, hipMemcpyDeviceToHost));
  return SLIDE_OK;
}

int slide_semantic_clipper(const double* tri_model, int ntm, const double* tri_data, int ntd, const slide_clipper_params_t* p,
                           int min_num_pairs, double matching_threshold, const double* u0, int n_u0, double tf16[16], int counts[2],
                           int32_t* inliers_out, int cap_inliers, int* found) {
  if (slide_device_check(-1) != SLIDE_OK) return SLIDE_ERR_HIP;
  if (!found || !counts) return SLIDE_ERR_INVALID;
  const slide_clipper_params_t P = clipper_params_or_default(p);
  identity16(tf16);
  *found = 0;
  counts[0] = counts[1] = 0;
  Tmp T;
  double *dp = nullptr, *dd = nullptr;
  long long np = 0;
  int rc = match_triangles_device(T, tri_model, ntm, tri_data, ntd, matching_threshold, &dp, &dd, &np);
  if (rc != SLIDE_OK) return rc;
  const long long m = 3 * np;
  if (m > (1 << 30)) { g_last_error = "more than 2^30 putative associations"; return SLIDE_ERR_CAPACITY; }
  counts[0] = (int)m;
  if (m == 0) return SLIDE_OK;
  if (u0 && n_u0 != (int)m) { g_last_error = "u0 length does not match the number of putative associations"; return SLIDE_ERR_INVALID; }
  // matched points back to the host (inlier gather, estimate_tf), split model / data for the affinity kernel
  std::vector<double> pts(4 * (size_t)m);
  SL_HIP(hipMemcpy(pts.data(), dp, sizeof(double) * 4 * (size_t)m, hipMemcpyDeviceToHost));
  std::vector<double> D1(2 * (size_t)m), D2(2 * (size_t)m);
  std::vector<int32_t> A(2 * (size_t)m);
  for (long long i = 0; i < m; ++i) {
    D1[2 * i] = pts[4 * i]; D1[2 * i + 1] = pts[4 * i + 1]; D2[2 * i] = pts[4 * i + 2]; D2[2 * i + 1] = pts[4 * i + 3];
    A[2 * i] = (int32_t)i; A[2 * i + 1] = (int32_t)i;          // identity association list, semantic_clipper.cpp:207-211
  }
  double* d1 = T.up(D1.data(), D1.size());
  double* d2 = T.up(D2.data(), D2.size());
  int32_t* dA = T.up(A.data(), A.size());
  if (!d1 || !d2 || !dA) { g_last_error = "hipMalloc/hipMemcpy failed"; return SLIDE_ERR_HIP; }
  // the affinity matrix as CSR straight from the associations (M_ = M.sparseView(), clipper.cpp:64): no m x m matrix, so no m is
  // refused for its dense size; the CSR is the one k_clipper_affinity + k_clq_csr gave, bit for bit
  DevCsr S;
  rc = csr_from_assoc_device(T, d1, d2, 2, dA, (int)m, P.sigma, P.epsilon, P.mindist, P.affinityeps, S);
  if (rc != SLIDE_OK) return rc;
  std::vector<int> nodes;
  std::vector<double> u;
  double sc = 0;
  rc = solve_csr_device(T, S, (int)m, u0, P, nodes, u, sc);
  if (rc != SLIDE_OK) return rc;
  counts[1] = (int)nodes.size();
  if (inliers_out) for (size_t i = 0; i < nodes.size() && (int)i < cap_inliers; ++i) inliers_out[i] = nodes[i];
  if ((int)nodes.size() < min_num_pairs) return SLIDE_OK;
  std::vector<double> a(2 * nodes.size()), b(2 * nodes.size());
  for (size_t k = 0; k < nodes.size(); ++k) {
    const int i = nodes[k];
    a[2 * k] = D1[2 * i]; a[2 * k + 1] = D1[2 * i + 1]; b[2 * k] = D2[2 * i]; b[2 * k + 1] = D2[2 * i + 1];
  }
  double tf3[9];
  estimate_tf2d(a.data(), b.data(), (int)nodes.size(), tf3);
  const double yaw = std::atan2(tf3[3], tf3[0]);
  tf16[0] = std::cos(yaw); tf16[1] = -std::sin(yaw); tf16[4] = std::sin(yaw); tf16[5] = std::cos(yaw);
  tf16[3] = tf3[2]; tf16[7] = tf3[5];
  *found = 1;
  return SLIDE_OK;
}

int slide_run_semantic_clipper(const double* ref7, int nr, const double* qry7, int nq, double sigma, double epsilon,
                               int min_num_pairs, double matching_threshold, const double* u0, int n_u0, double tf16[16], int counts[2],
                               int* found) {
  if (nr < 0 || nq < 0) return SLIDE_ERR_INVALID;
  auto tris = [](const double* rows7, int n) {
    std::vector<double> xy(2 * (size_t)std::max(n, 1));
    for (int i = 0; i < n; ++i) { xy[2 * i] = rows7[7 * (size_t)i + 1]; xy[2 * i + 1] = rows7[7 * (size_t)i + 2]; }   // semantic_clipper.cpp:150-165
    const std::vector<std::array<int32_t, 3>> t = delaunay::triangulate(xy.data(), n);
    std::vector<double> out(6 * t.size());
    for (size_t k = 0; k < t.size(); ++k)
      for (int v = 0; v < 3; ++v) { out[6 * k + 2 * v] = xy[2 * t[k][v]]; out[6 * k + 2 * v + 1] = xy[2 * t[k][v] + 1]; }
    return out;
  };
  const std::vector<double> tm = tris(ref7, nr), td = tris(qry7, nq);
  slide_clipper_params_t P = clipper_params_or_default(nullptr);
  P.sigma = sigma;
  P.epsilon = epsilon;
  return slide_semantic_clipper(tm.data(), (int)(tm.size() / 6), td.data(), (int)(td.size() / 6), &P, min_num_pairs, matching_threshold,
                                u0, n_u0, tf16, counts, nullptr, 0, found);
}

void slide_slidegraph_default_params(slide_slidegraph_params_t* p) {      // place_recognition.cpp:65-75
  p->sigma = 0.1; p->epsilon = 0.1; p->num_inliers_threshold = 10; p->matching_threshold = 0.1; p->min_num_map_objects_to_start = 20;
}

int slide_find_inter_loop_closures_clipper(const double* maps7, const int32_t* map_off, int n_maps, const int32_t* pairs, int n_pairs,
                                           const slide_slidegraph_params_t* p, const double* const* u0, const int* n_u0, double* tf16n,
                                           int32_t* counts4n, int32_t* found, int32_t* status) {
  if (n_pairs < 0 || n_maps < 0) return SLIDE_ERR_INVALID;
  if (n_pairs == 0) return SLIDE_OK;
  if (!map_off || !pairs || !tf16n || !counts4n || !found) { g_last_error = "find_inter_loop_closures_clipper: a needed pointer is NULL"; return SLIDE_ERR_INVALID; }
  if (n_maps > 0 && map_off[0] < 0) { g_last_error = "find_inter_loop_closures_clipper: map_off[0] is negative"; return SLIDE_ERR_INVALID; }
  for (int i = 0; i < n_maps; ++i)
    if (map_off[i + 1] < map_off[i]) { g_last_error = "find_inter_loop_closures_clipper: map_off decreases at map " + std::to_string(i); return SLIDE_ERR_INVALID; }
  if (n_maps > 0 && map_off[n_maps] > map_off[0] && !maps7) { g_last_error = "find_inter_loop_closures_clipper: maps7 is NULL"; return SLIDE_ERR_INVALID; }
  for (int k = 0; k < n_pairs; ++k) {
    if (pairs[2 * k] < 0 || pairs[2 * k] >= n_maps || pairs[2 * k + 1] < 0 || pairs[2 * k + 1] >= n_maps) {
      g_last_error = "find_inter_loop_closures_clipper: pair " + std::to_string(k) + " names a map outside [0, n_maps)";
      return SLIDE_ERR_INVALID;
    }
    if (u0 && u0[k] && !n_u0) { g_last_error = "find_inter_loop_closures_clipper: u0 given without n_u0"; return SLIDE_ERR_INVALID; }
  }
  slide_slidegraph_params_t G;
  if (p) G = *p; else slide_slidegraph_default_params(&G);
  std::vector<MapView> maps(n_maps);
  for (int i = 0; i < n_maps; ++i) maps[i] = MapView{maps7 ? maps7 + 7 * (size_t)map_off[i] : nullptr, map_off[i + 1] - map_off[i]};
  for (int k = 0; k < n_pairs; ++k) {
    identity16(tf16n + 16 * (size_t)k);
    for (int c = 0; c < 4; ++c) counts4n[4 * k + c] = 0;
    found[k] = 0;
    if (status) status[k] = SLIDE_OK;
  }
  return inter_loop_closures_clipper(maps, pairs, n_pairs, G, u0, n_u0, tf16n, counts4n, found, status);
}

int slide_find_inter_loop_closure_clipper(const double* ref7, int nr, const double* qry7, int nq, const slide_slidegraph_params_t* p,
                                          const double* u0, int n_u0, double tf16[16], int counts[4], int* found) {
  if (nr < 0 || nq < 0 || !tf16 || !counts || !found || (nr > 0 && !ref7) || (nq > 0 && !qry7)) return SLIDE_ERR_INVALID;
  slide_slidegraph_params_t G;
  if (p) G = *p; else slide_slidegraph_default_params(&G);
  const std::vector<MapView> maps = {MapView{ref7, nr}, MapView{qry7, nq}};
  const int32_t pair[2] = {0, 1};
  identity16(tf16);
  int32_t c4[4] = {0, 0, 0, 0}, f = 0, st = SLIDE_OK;
  const double* const u0s[1] = {u0};
  const int rc = inter_loop_closures_clipper(maps, pair, 1, G, u0s, &n_u0, tf16, c4, &f, &st);
  for (int c = 0; c < 4; ++c) counts[c] = c4[c];
  *found = f;
  if (rc == SLIDE_OK && st == SLIDE_ERR_INVALID) g_last_error = "u0 length does not match the number of putative associations";
  if (rc == SLIDE_OK && st == SLIDE_ERR_CAPACITY) g_last_error = "more than 2^30 putative associations or 2^31 - 1 non-zeros in the affinity matrix";
  return rc != SLIDE_OK ? rc : st;
}

}  // extern "C"
