// Host side of loop-closure selection: the mutually consistent subset of a list of loop closures (PCM on the clique solver through
// host_clipper.hpp's solve_csr_segments; no counterpart in the reference, which adds the first closure that passes straight into the
// graph: sloamNode.cpp:448-476, graphWrapper.cpp:55), and behind it the entry points that share its argument checks (pose-pair
// covariances, the closures' Mahalanobis gate), the observations' Mahalanobis gate with checks of its own in the same style, and
// slide_find_relative_meas_match.
#include <cmath>

#include "capi_handles.hpp"
#include "host_clipper.hpp"

using namespace sl;

namespace {
struct ClosureCanon {
  std::vector<int32_t> fr, tr, flipped, group, order;      // per closure; group / order -1 for a skipped closure
  std::vector<uint64_t> fi, ti;
  std::vector<SE3> z;
  std::vector<int> goff;                                   // rows of group g: goff[g] .. goff[g + 1]
  int n_groups = 0;
};
// from_robot > to_robot: ends swapped, rel inverted.  Groups by ascending (from_robot, to_robot), filled in list order.
void closure_canonicalize(int L, const int32_t* from_robot, const uint64_t* from_idx, const int32_t* to_robot, const uint64_t* to_idx,
                          const double* rel7, const int32_t* skip, ClosureCanon& C) {
  C.fr.assign(from_robot, from_robot + L); C.tr.assign(to_robot, to_robot + L);
  C.fi.assign(from_idx, from_idx + L); C.ti.assign(to_idx, to_idx + L);
  C.flipped.assign(L, 0); C.group.assign(L, -1); C.order.assign(L, -1);
  C.z.resize(L);
  std::vector<int> keys;
  for (int k = 0; k < L; ++k) {
    C.z[k] = from7(rel7 + 7 * (size_t)k);
    if (C.fr[k] > C.tr[k]) {
      std::swap(C.fr[k], C.tr[k]); std::swap(C.fi[k], C.ti[k]);
      C.z[k] = inverse(C.z[k]);
      C.flipped[k] = 1;
    }
    if (!(skip && skip[k])) keys.push_back(C.fr[k] * (SLIDE_MAX_ROBOTS + 1) + C.tr[k]);
  }
  std::sort(keys.begin(), keys.end());
  keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
  C.n_groups = (int)keys.size();
  C.goff.assign(C.n_groups + 1, 0);
  for (int k = 0; k < L; ++k) {
    if (skip && skip[k]) continue;
    C.group[k] = (int)(std::lower_bound(keys.begin(), keys.end(), C.fr[k] * (SLIDE_MAX_ROBOTS + 1) + C.tr[k]) - keys.begin());
    C.goff[C.group[k] + 1] += 1;
  }
  for (int g = 0; g < C.n_groups; ++g) C.goff[g + 1] += C.goff[g];
  std::vector<int> fill(C.goff.begin(), C.goff.end() - 1);
  for (int k = 0; k < L; ++k)
    if (C.group[k] >= 0) C.order[k] = fill[C.group[k]]++;
}
bool closure_finite(const double* v, size_t n) {
  for (size_t i = 0; i < n; ++i)
    if (!std::isfinite(v[i])) return false;
  return true;
}
bool closure_quats_ok(const double* p7, int L) {
  for (int k = 0; k < L; ++k) {
    const double* q = p7 + 7 * (size_t)k + 3;
    if (!(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3] > 0.0)) return false;
  }
  return true;
}
int closure_bad(const char* what) { g_last_error = std::string("closure selection: ") + what; return SLIDE_ERR_INVALID; }
int closure_check_params(const slide_closure_params_t& P, bool odom) {
  if (!(P.gate > 0.0) || !std::isfinite(P.gate) || !(P.sigma > 0.0) || !std::isfinite(P.sigma)) return closure_bad("gate and sigma must be > 0");
  if (!(P.affinityeps >= 0.0) || !std::isfinite(P.affinityeps)) return closure_bad("affinityeps must be >= 0");
  if (P.min_set < 0) return closure_bad("min_set must be >= 0");
  for (int c = 0; odom && c < 6; ++c)
    if (!(P.odom_sigma6[c] > 0.0) || !std::isfinite(P.odom_sigma6[c])) return closure_bad("odom_sigma6 must be > 0");
  return SLIDE_OK;
}
// rel7 / sigma6 (and the poses when given) of L closures: finite, quaternions not zero, sigmas > 0
int closure_check_values(int L, const double* rel7, const double* sigma6, const double* from_pose7, const double* to_pose7) {
  if (!closure_finite(rel7, 7 * (size_t)L) || !closure_quats_ok(rel7, L)) return closure_bad("rel7 holds a non-finite value or a zero quaternion");
  if (!closure_finite(sigma6, 6 * (size_t)L)) return closure_bad("sigma6 holds a non-finite value");
  for (size_t i = 0; i < 6 * (size_t)L; ++i)
    if (!(sigma6[i] > 0.0)) return closure_bad("a sigma <= 0");
  for (const double* p : {from_pose7, to_pose7})
    if (p && (!closure_finite(p, 7 * (size_t)L) || !closure_quats_ok(p, L))) return closure_bad("a pose holds a non-finite value or a zero quaternion");
  return SLIDE_OK;
}
ClosureScore closure_score_params(const slide_closure_params_t& P) {
  ClosureScore S;
  S.gate = P.gate; S.sigma = P.sigma; S.affinityeps = P.affinityeps;
  for (int c = 0; c < 6; ++c) S.odom2[c] = P.odom_sigma6[c] * P.odom_sigma6[c];
  return S;
}

// The device side of one list: its rows (closures of the groups of two or more, group after group) prepared, counted, scanned, emitted.
struct ClosureRows {
  int n_seg = 0, n_rows = 0;
  std::vector<int> goff;                  // n_seg + 1
  std::vector<double> z12, sig2, fpose12, tpose12;
  std::vector<unsigned long long> idx2;
  std::vector<int32_t> fslot, tslot;      // graph form: rows of pose_est
  // device
  int* d_goff = nullptr; int* d_rcnt = nullptr; int* d_rptr = nullptr; long long* d_tot = nullptr; long long* d_nnz0 = nullptr;
  int* d_col = nullptr; double* d_val = nullptr;
  std::vector<long long> tot, nnz0;
  long long nnz_all = 0;
};
// d_pose_est: null = the rows' own pose arrays.  After it: the CSR of every segment on the device (nnz0[s] < 0: more than 2^31 - 1
// non-zeros, dropped).  ONE blocking read-back (the segments' totals).
int closure_build_csr(Tmp& T, ClosureRows& R, const double* d_pose_est, const ClosureScore& S) {
  const int n = R.n_rows;
  double* d_z = T.up(R.z12.data(), R.z12.size());
  double* d_sig2 = T.up(R.sig2.data(), R.sig2.size());
  unsigned long long* d_idx2 = T.up(R.idx2.data(), R.idx2.size());
  double* d_pre = T.up<double>(nullptr, CLOSURE_PRE * (size_t)n);
  R.d_goff = T.up(R.goff.data(), R.goff.size());
  R.d_rcnt = T.up<int>(nullptr, n);
  R.d_rptr = T.up<int>(nullptr, (size_t)n + R.n_seg);
  R.d_tot = T.up<long long>(nullptr, R.n_seg);
  if (!d_z || !d_sig2 || !d_idx2 || !d_pre || !R.d_goff || !R.d_rcnt || !R.d_rptr || !R.d_tot) { g_last_error = "hipMalloc/hipMemcpy failed"; return SLIDE_ERR_HIP; }
  if (d_pose_est) {
    int32_t* d_fs = T.up(R.fslot.data(), R.fslot.size());
    int32_t* d_ts = T.up(R.tslot.data(), R.tslot.size());
    if (!d_fs || !d_ts) { g_last_error = "hipMalloc/hipMemcpy failed"; return SLIDE_ERR_HIP; }
    launch_closure_prepare(d_pose_est, d_pose_est, d_fs, d_ts, d_z, n, d_pre, nullptr);
  } else {
    double* d_f = T.up(R.fpose12.data(), R.fpose12.size());
    double* d_t = T.up(R.tpose12.data(), R.tpose12.size());
    if (!d_f || !d_t) { g_last_error = "hipMalloc/hipMemcpy failed"; return SLIDE_ERR_HIP; }
    launch_closure_prepare(d_f, d_t, nullptr, nullptr, d_z, n, d_pre, nullptr);
  }
  launch_closure_csr_seg(false, d_pre, d_sig2, d_idx2, R.d_goff, R.n_seg, n, S, R.d_rcnt, nullptr, nullptr, nullptr, nullptr, nullptr);
  launch_seg_scan_rowptr(R.d_rcnt, R.d_goff, R.n_seg, R.d_rptr, R.d_tot, nullptr);
  SL_HIP(hipGetLastError());
  R.tot.assign(R.n_seg, 0);
  SL_HIP(hipMemcpy(R.tot.data(), R.d_tot, sizeof(long long) * R.n_seg, hipMemcpyDeviceToHost));           // read-back 1
  R.nnz0.assign(R.n_seg, -1);
  R.nnz_all = 0;
  for (int s = 0; s < R.n_seg; ++s) {
    if (R.tot[s] > INT32_MAX) continue;      // ClqSolve::rowptr is per problem, 32 bits
    R.nnz0[s] = R.nnz_all;
    R.nnz_all += R.tot[s];
  }
  R.d_nnz0 = T.up(R.nnz0.data(), R.nnz0.size());
  R.d_col = T.up<int>(nullptr, (size_t)std::max<long long>(R.nnz_all, 1));
  R.d_val = T.up<double>(nullptr, (size_t)std::max<long long>(R.nnz_all, 1));
  if (!R.d_nnz0 || !R.d_col || !R.d_val) { g_last_error = "hipMalloc/hipMemcpy failed"; return SLIDE_ERR_HIP; }
  launch_closure_csr_seg(true, d_pre, d_sig2, d_idx2, R.d_goff, R.n_seg, n, S, nullptr, R.d_rptr, R.d_nnz0, R.d_col, R.d_val, nullptr);
  SL_HIP(hipGetLastError());
  return SLIDE_OK;
}
void closure_row_values(ClosureRows& R, const SE3& z, const double* sigma6, uint64_t fi, uint64_t ti) {
  double z12[12];
  to12(z, z12);
  R.z12.insert(R.z12.end(), z12, z12 + 12);
  for (int c = 0; c < 6; ++c) R.sig2.push_back(sigma6[c] * sigma6[c]);
  R.idx2.push_back(fi); R.idx2.push_back(ti);
}
void closure_row_pose(std::vector<double>& dst, const double* pose7) {
  double p12[12];
  to12(from7(pose7), p12);
  dst.insert(dst.end(), p12, p12 + 12);
}

struct ClosureOut {
  int32_t* keep; int32_t* group; int32_t* status; int32_t* n_selected; double* score; int* n_groups; double* u_out;
  int32_t* rowcnt_out; int32_t* col_out; double* val_out; long long csr_cap; long long* csr_nnz;
};
// C: the canonical list (status of its skipped closures already written by the caller).  Poses: per closure on the host (input
// order, as given: a flipped closure's ends are swapped here), or the graph's device estimate with per-closure slots.
int select_closures_core(int L, const ClosureCanon& C, const double* sigma6, const double* from_pose7, const double* to_pose7,
                         const double* d_pose_est, const int32_t* fslot, const int32_t* tslot, const slide_closure_params_t& P,
                         const slide_clipper_params_t& CP, const double* const* u0, const ClosureOut& O) {
  const int NG = C.n_groups;
  *O.n_groups = NG;
  if (O.csr_nnz) *O.csr_nnz = 0;
  for (int k = 0; k < L; ++k) {
    O.keep[k] = 0;
    if (O.group) O.group[k] = C.group[k];
    if (O.status && C.group[k] >= 0) O.status[k] = SLIDE_OK;
    if (O.u_out) O.u_out[k] = 0.0;
    if (O.rowcnt_out) O.rowcnt_out[k] = 0;
  }
  for (int g = 0; g < NG; ++g) {
    if (O.n_selected) O.n_selected[g] = 0;
    if (O.score) O.score[g] = 0.0;
  }
  std::vector<int> by_row(C.goff[NG], -1);      // closure of every row
  for (int k = 0; k < L; ++k)
    if (C.order[k] >= 0) by_row[C.order[k]] = k;
  // a lone closure never reaches the device: the clique of a 1 x 1 problem is that closure (u = 1, F = u (M + I) u = 1)
  ClosureRows R;
  std::vector<int> seg_group;
  R.goff.push_back(0);
  for (int g = 0; g < NG; ++g) {
    const int m = C.goff[g + 1] - C.goff[g];
    if (m == 1) {
      const int k = by_row[C.goff[g]];
      if (O.n_selected) O.n_selected[g] = 1;
      if (O.score) O.score[g] = 1.0;
      if (O.u_out) O.u_out[k] = 1.0;
      O.keep[k] = 1 >= P.min_set ? 1 : 0;
      continue;
    }
    seg_group.push_back(g);
    for (int r = C.goff[g]; r < C.goff[g + 1]; ++r) {
      const int k = by_row[r];
      closure_row_values(R, C.z[k], sigma6 + 6 * (size_t)k, C.fi[k], C.ti[k]);
      const bool fl = C.flipped[k] != 0;
      if (d_pose_est) {
        R.fslot.push_back(fl ? tslot[k] : fslot[k]);
        R.tslot.push_back(fl ? fslot[k] : tslot[k]);
      } else {
        closure_row_pose(R.fpose12, (fl ? to_pose7 : from_pose7) + 7 * (size_t)k);
        closure_row_pose(R.tpose12, (fl ? from_pose7 : to_pose7) + 7 * (size_t)k);
      }
    }
    R.goff.push_back(R.goff.back() + m);
  }
  R.n_seg = (int)seg_group.size();
  R.n_rows = R.goff.back();
  if (R.n_seg == 0) return SLIDE_OK;
  if (slide_device_check(-1) != SLIDE_OK) return SLIDE_ERR_HIP;
  Tmp T;
  int rc = closure_build_csr(T, R, d_pose_est, closure_score_params(P));
  if (rc != SLIDE_OK) return rc;
  const int n_seg = R.n_seg, n_rows = R.n_rows;
  const std::vector<int>& goff = R.goff;
  auto row_closure = [&](int s, int i) { return by_row[C.goff[seg_group[s]] + i]; };
  // the solves (solve_csr_segments): one launch for every group below the single problem's multi-workgroup threshold; results
  // [out4 per group | u]
  const size_t res_len = 4 * (size_t)n_seg + (size_t)n_rows;
  double* d_res = T.up<double>(nullptr, res_len);
  double* d_work = T.up<double>(nullptr, 6 * (size_t)n_rows);
  if (!d_res || !d_work) { g_last_error = "hipMalloc failed"; return SLIDE_ERR_HIP; }
  SL_HIP(hipMemsetAsync(d_res, 0, res_len * sizeof(double), nullptr));
  std::vector<const double*> seg_u0(n_seg, nullptr);
  for (int s = 0; s < n_seg; ++s) {
    if (u0) seg_u0[s] = u0[seg_group[s]];
    for (int i = 0; R.nnz0[s] < 0 && O.status && i < goff[s + 1] - goff[s]; ++i) O.status[row_closure(s, i)] = SLIDE_ERR_CAPACITY;
  }
  const ClqSegments segments{n_seg, goff.data(), R.d_goff, R.d_rptr, R.d_col, R.d_val, R.nnz0.data(), R.tot.data(), d_work, d_res, res_len};
  std::vector<double> res;
  rc = solve_csr_segments(T, segments, seg_u0, CP, res, [&](int s, const std::vector<int>& nodes, const std::vector<double>& u, double sc) {      // read-back 2
    const int m = goff[s + 1] - goff[s], g = seg_group[s];
    if (O.n_selected) O.n_selected[g] = (int)nodes.size();
    if (O.score) O.score[g] = sc;
    if (O.u_out) for (int i = 0; i < m; ++i) O.u_out[row_closure(s, i)] = u[i];
    if ((int)nodes.size() >= P.min_set && !nodes.empty())
      for (int i : nodes) O.keep[row_closure(s, i)] = 1;
  });
  if (rc != SLIDE_OK) return rc;
  // the matrices themselves, for inspection (three more blocking copies)
  if (O.csr_nnz) *O.csr_nnz = R.nnz_all;
  if (O.rowcnt_out) {
    std::vector<int> cnt(n_rows);
    SL_HIP(hipMemcpy(cnt.data(), R.d_rcnt, sizeof(int) * n_rows, hipMemcpyDeviceToHost));
    for (int s = 0; s < n_seg; ++s)
      for (int i = 0; i < goff[s + 1] - goff[s]; ++i)
        if (R.nnz0[s] >= 0) O.rowcnt_out[row_closure(s, i)] = cnt[goff[s] + i];
  }
  if (O.col_out && O.val_out && R.nnz_all > 0 && R.nnz_all <= O.csr_cap) {
    SL_HIP(hipMemcpy(O.col_out, R.d_col, sizeof(int32_t) * (size_t)R.nnz_all, hipMemcpyDeviceToHost));
    SL_HIP(hipMemcpy(O.val_out, R.d_val, sizeof(double) * (size_t)R.nnz_all, hipMemcpyDeviceToHost));
  }
  return SLIDE_OK;
}
int closure_check_list(int L, const int32_t* from_robot, const uint64_t* from_idx, const int32_t* to_robot, const uint64_t* to_idx,
                       const double* rel7, const double* sigma6, const void* keep, const void* n_groups) {
  if (L < 0) return closure_bad("L < 0");
  if (!n_groups) return closure_bad("n_groups is NULL");
  if (L > 0 && (!from_robot || !from_idx || !to_robot || !to_idx || !rel7 || !sigma6 || !keep)) return closure_bad("a needed pointer is NULL");
  for (int k = 0; k < L; ++k)
    if (!robot_ok(from_robot[k]) || !robot_ok(to_robot[k])) return closure_bad("a robot outside [0, SLIDE_MAX_ROBOTS)");
  return SLIDE_OK;
}
}  // namespace
extern "C" {

void slide_closure_default_params(slide_closure_params_t* p) {
  p->gate = 4.1;                 // sqrt(16.81): the 0.99 quantile of chi-square with 6 degrees of freedom
  p->sigma = p->gate / 2;        // a convention: the score at the gate is exp(-2)
  p->affinityeps = 1e-4;         // CLIPPER's default
  for (int c = 0; c < 6; ++c) p->odom_sigma6[c] = 0.1;
  p->min_set = 1;
}

int slide_closure_canonicalize(int L, const int32_t* from_robot, const uint64_t* from_idx, const int32_t* to_robot, const uint64_t* to_idx,
                               const double* rel7, int32_t* from_robot_out, uint64_t* from_idx_out, int32_t* to_robot_out,
                               uint64_t* to_idx_out, double* rel7_out, int32_t* flipped, int32_t* group, int32_t* order, int* n_groups) {
  int dummy = 0;
  int rc = closure_check_list(L, from_robot, from_idx, to_robot, to_idx, rel7, rel7, &dummy, n_groups);
  if (rc != SLIDE_OK) return rc;
  if (L > 0 && (!closure_finite(rel7, 7 * (size_t)L) || !closure_quats_ok(rel7, L))) return closure_bad("rel7 holds a non-finite value or a zero quaternion");
  ClosureCanon C;
  closure_canonicalize(L, from_robot, from_idx, to_robot, to_idx, rel7, nullptr, C);
  *n_groups = C.n_groups;
  for (int k = 0; k < L; ++k) {
    if (from_robot_out) from_robot_out[k] = C.fr[k];
    if (from_idx_out) from_idx_out[k] = C.fi[k];
    if (to_robot_out) to_robot_out[k] = C.tr[k];
    if (to_idx_out) to_idx_out[k] = C.ti[k];
    if (rel7_out) {
      if (C.flipped[k]) to7(C.z[k], rel7_out + 7 * (size_t)k);
      else std::memcpy(rel7_out + 7 * (size_t)k, rel7 + 7 * (size_t)k, 7 * sizeof(double));      // untouched closures keep their bits
    }
    if (flipped) flipped[k] = C.flipped[k];
    if (group) group[k] = C.group[k];
    if (order) order[k] = C.order[k];
  }
  return SLIDE_OK;
}

int slide_closure_consistency_csr(const double* from_pose7, const double* to_pose7, const double* rel7, const double* sigma6,
                                  const uint64_t* from_idx, const uint64_t* to_idx, int L, const slide_closure_params_t* p,
                                  int32_t* rowptr_out, int32_t* col_out, double* val_out, long long cap, long long* nnz) {
  if (L < 0) return closure_bad("L < 0");
  if (cap < 0 || !nnz || !rowptr_out) return closure_bad("cap < 0, or nnz / rowptr_out is NULL");
  if (L > 0 && (!from_pose7 || !to_pose7 || !rel7 || !sigma6 || !from_idx || !to_idx)) return closure_bad("a needed pointer is NULL");
  slide_closure_params_t P;
  if (p) P = *p; else slide_closure_default_params(&P);
  int rc = closure_check_params(P, true);
  if (rc == SLIDE_OK && L > 0) rc = closure_check_values(L, rel7, sigma6, from_pose7, to_pose7);
  if (rc != SLIDE_OK) return rc;
  *nnz = 0;
  if (L <= 1) {          // no pair: the empty matrix, no device
    for (int i = 0; i <= L; ++i) rowptr_out[i] = 0;
    return SLIDE_OK;
  }
  if (slide_device_check(-1) != SLIDE_OK) return SLIDE_ERR_HIP;
  ClosureRows R;
  R.n_seg = 1; R.n_rows = L; R.goff = {0, L};
  for (int k = 0; k < L; ++k) {
    closure_row_values(R, from7(rel7 + 7 * (size_t)k), sigma6 + 6 * (size_t)k, from_idx[k], to_idx[k]);
    closure_row_pose(R.fpose12, from_pose7 + 7 * (size_t)k);
    closure_row_pose(R.tpose12, to_pose7 + 7 * (size_t)k);
  }
  Tmp T;
  rc = closure_build_csr(T, R, nullptr, closure_score_params(P));
  if (rc != SLIDE_OK) return rc;
  if (R.nnz0[0] < 0) { g_last_error = "the consistency matrix has more than 2^31 - 1 non-zeros"; return SLIDE_ERR_CAPACITY; }
  *nnz = R.tot[0];
  SL_HIP(hipMemcpy(rowptr_out, R.d_rptr, sizeof(int32_t) * ((size_t)L + 1), hipMemcpyDeviceToHost));
  if (*nnz > cap) { g_last_error = "the CSR has " + std::to_string(*nnz) + " non-zeros, the caller's buffers hold " + std::to_string(cap); return SLIDE_ERR_CAPACITY; }
  if (*nnz > 0) {
    if (!col_out || !val_out) return closure_bad("col_out / val_out is NULL");
    SL_HIP(hipMemcpy(col_out, R.d_col, sizeof(int32_t) * (size_t)*nnz, hipMemcpyDeviceToHost));
    SL_HIP(hipMemcpy(val_out, R.d_val, sizeof(double) * (size_t)*nnz, hipMemcpyDeviceToHost));
  }
  return SLIDE_OK;
}

int slide_select_consistent_closures(int L, const int32_t* from_robot, const uint64_t* from_idx, const int32_t* to_robot,
                                     const uint64_t* to_idx, const double* rel7, const double* sigma6, const double* from_pose7,
                                     const double* to_pose7, const slide_closure_params_t* p, const slide_clipper_params_t* cp,
                                     const double* const* u0, int32_t* keep, int32_t* group, int32_t* status, int32_t* n_selected,
                                     double* score, int* n_groups, double* u_out, int32_t* rowcnt_out, int32_t* col_out, double* val_out,
                                     long long csr_cap, long long* csr_nnz) {
  int rc = closure_check_list(L, from_robot, from_idx, to_robot, to_idx, rel7, sigma6, keep, n_groups);
  if (rc != SLIDE_OK) return rc;
  if (L > 0 && (!from_pose7 || !to_pose7)) return closure_bad("a needed pointer is NULL");
  if (csr_cap < 0) return closure_bad("csr_cap < 0");
  slide_closure_params_t P;
  if (p) P = *p; else slide_closure_default_params(&P);
  rc = closure_check_params(P, true);
  if (rc == SLIDE_OK && L > 0) rc = closure_check_values(L, rel7, sigma6, from_pose7, to_pose7);
  if (rc != SLIDE_OK) return rc;
  const slide_clipper_params_t CP = clipper_params_or_default(cp);
  if (L == 0) { *n_groups = 0; if (csr_nnz) *csr_nnz = 0; return SLIDE_OK; }
  ClosureCanon C;
  closure_canonicalize(L, from_robot, from_idx, to_robot, to_idx, rel7, nullptr, C);
  const ClosureOut O{keep, group, status, n_selected, score, n_groups, u_out, rowcnt_out, col_out, val_out, csr_cap, csr_nnz};
  return select_closures_core(L, C, sigma6, from_pose7, to_pose7, nullptr, nullptr, nullptr, P, CP, u0, O);
}

int slide_graph_select_closures(slide_graph_t* g, int L, const int32_t* from_robot, const uint64_t* from_idx, const int32_t* to_robot,
                                const uint64_t* to_idx, const double* rel7, const double* sigma6, const slide_closure_params_t* p,
                                const slide_clipper_params_t* cp, int32_t* keep, int32_t* group, int32_t* status, int32_t* n_selected,
                                double* score, int* n_groups) {
  if (!g) return closure_bad("the graph is NULL");
  int rc = closure_check_list(L, from_robot, from_idx, to_robot, to_idx, rel7, sigma6, keep, n_groups);
  if (rc != SLIDE_OK) return rc;
  slide_closure_params_t P;
  if (p) P = *p; else slide_closure_default_params(&P);
  rc = closure_check_params(P, false);
  if (rc == SLIDE_OK && L > 0) rc = closure_check_values(L, rel7, sigma6, nullptr, nullptr);
  if (rc != SLIDE_OK) return rc;
  const slide_clipper_params_t CP = clipper_params_or_default(cp);
  if (L == 0) { *n_groups = 0; return SLIDE_OK; }
  LOCK(g);
  for (int c = 0; c < 6; ++c) P.odom_sigma6[c] = g->g.P.noise_model_odom_vec[c];
  rc = closure_check_params(P, true);
  if (rc != SLIDE_OK) return rc;
  std::vector<int32_t> fslot(L), tslot(L), skip(L, 0);
  g->g.pose_slots(from_robot, from_idx, L, fslot.data());
  g->g.pose_slots(to_robot, to_idx, L, tslot.data());
  for (int k = 0; k < L; ++k)
    if (fslot[k] < 0 || tslot[k] < 0) { skip[k] = 1; if (status) status[k] = SLIDE_MISSING; }
  ClosureCanon C;
  closure_canonicalize(L, from_robot, from_idx, to_robot, to_idx, rel7, skip.data(), C);
  SL_HIP(hipStreamSynchronize(g->g.stream));      // the estimate of the last solve is in place; this call only reads it
  const ClosureOut O{keep, group, status, n_selected, score, n_groups, nullptr, nullptr, nullptr, nullptr, 0, nullptr};
  return select_closures_core(L, C, sigma6, nullptr, nullptr, g->g.pose_est_dev(), fslot.data(), tslot.data(), P, CP, nullptr, O);
}

// Marginals::jointMarginalCovariance for a list of pose pairs.  The argument checks come first and need neither graph nor device.
int slide_graph_get_pose_pair_covariances(slide_graph_t* g, int n, const int32_t* robot_a, const uint64_t* idx_a, const int32_t* robot_b,
                                          const uint64_t* idx_b, double* out144n, int32_t* status) {
  if (n < 0) { g_last_error = "get_pose_pair_covariances: n < 0"; return SLIDE_ERR_INVALID; }
  if (n > 0 && (!robot_a || !idx_a || !robot_b || !idx_b || !out144n)) { g_last_error = "get_pose_pair_covariances: a needed pointer is NULL"; return SLIDE_ERR_INVALID; }
  for (int k = 0; k < n; ++k)
    if (!robot_ok(robot_a[k]) || !robot_ok(robot_b[k])) { g_last_error = "get_pose_pair_covariances: a robot outside [0, SLIDE_MAX_ROBOTS)"; return SLIDE_ERR_INVALID; }
  if (!g) { g_last_error = "get_pose_pair_covariances: the graph is NULL"; return SLIDE_ERR_INVALID; }
  LOCK(g);
  return g->g.pose_pair_covariances(n, robot_a, idx_a, robot_b, idx_b, out144n, status);
}

// The individual-compatibility gate of a list of loop closures (the complement of slide_graph_select_closures, same arrays)
int slide_graph_closure_mahalanobis(slide_graph_t* g, int L, const int32_t* from_robot, const uint64_t* from_idx, const int32_t* to_robot,
                                    const uint64_t* to_idx, const double* rel7, const double* sigma6, double* d2, double* C36, double* r6,
                                    int32_t* status) {
  int dummy = 0;
  int rc = closure_check_list(L, from_robot, from_idx, to_robot, to_idx, rel7, sigma6, d2, &dummy);
  if (rc == SLIDE_OK && L > 0) rc = closure_check_values(L, rel7, sigma6, nullptr, nullptr);
  if (rc != SLIDE_OK) { g_last_error = "closure_mahalanobis: " + g_last_error; return rc; }
  if (!g) { g_last_error = "closure_mahalanobis: the graph is NULL"; return SLIDE_ERR_INVALID; }
  LOCK(g);
  return g->g.closure_mahalanobis(L, from_robot, from_idx, to_robot, to_idx, rel7, sigma6, d2, C36, r6, status);
}

// The same two queries on the joint graph of a CholBatch (a slot where the calls above take a robot).  The argument checks are the
// single-graph calls' own and come before the batch or the device is looked at.
int slide_chol_batch_get_pose_pair_covariances(slide_chol_batch_t* b, int n, const int32_t* slot_a, const uint64_t* idx_a, const int32_t* slot_b,
                                               const uint64_t* idx_b, double* out144n, int32_t* status) {
  if (n < 0) { g_last_error = "get_pose_pair_covariances: n < 0"; return SLIDE_ERR_INVALID; }
  if (n > 0 && (!slot_a || !idx_a || !slot_b || !idx_b || !out144n)) { g_last_error = "get_pose_pair_covariances: a needed pointer is NULL"; return SLIDE_ERR_INVALID; }
  for (int k = 0; k < n; ++k)
    if (!robot_ok(slot_a[k]) || !robot_ok(slot_b[k])) { g_last_error = "get_pose_pair_covariances: a slot outside [0, SLIDE_MAX_ROBOTS)"; return SLIDE_ERR_INVALID; }
  if (!b) { g_last_error = "get_pose_pair_covariances: the batch is NULL"; return SLIDE_ERR_INVALID; }
  return b->b.joint_pose_pair_covariances(n, slot_a, idx_a, slot_b, idx_b, out144n, status);
}
int slide_chol_batch_closure_mahalanobis(slide_chol_batch_t* b, int L, const int32_t* from_slot, const uint64_t* from_idx, const int32_t* to_slot,
                                         const uint64_t* to_idx, const double* rel7, const double* sigma6, double* d2, double* C36, double* r6,
                                         int32_t* status) {
  int dummy = 0;
  int rc = closure_check_list(L, from_slot, from_idx, to_slot, to_idx, rel7, sigma6, d2, &dummy);
  if (rc == SLIDE_OK && L > 0) rc = closure_check_values(L, rel7, sigma6, nullptr, nullptr);
  if (rc != SLIDE_OK) { g_last_error = "closure_mahalanobis: " + g_last_error; return rc; }
  if (!b) { g_last_error = "closure_mahalanobis: the batch is NULL"; return SLIDE_ERR_INVALID; }
  return b->b.joint_closure_mahalanobis(L, from_slot, from_idx, to_slot, to_idx, rel7, sigma6, d2, C36, r6, status);
}

// The individual-compatibility gate of a list of candidate landmark observations (the closure gate's counterpart for the factors the
// association produces).  The argument checks come first and need neither graph nor device; nothing is written on a refusal.
static int obs_gate_bad(const char* what, const char* who = "observation_mahalanobis") {
  g_last_error = std::string(who) + ": " + what;
  return SLIDE_ERR_INVALID;
}
// (the list's own checks, shared with the batch's call — robot2, or null, is its second list of slots — and with the joint-compatibility
// call, which names itself in the message)
static int obs_gate_check_list(int n, const int32_t* robot, const int32_t* robot2, const uint64_t* pose_idx, const int32_t* cls, const uint64_t* lm_idx,
                               const double* meas17, const double* d2, const char* who = "observation_mahalanobis") {
  auto bad = [who](const char* what) { return obs_gate_bad(what, who); };
  auto zero3 = [](const double* v) { return !(v[0] * v[0] + v[1] * v[1] + v[2] * v[2] > 0.0); };
  auto zero_quat = [](const double* p7) { return !(p7[3] * p7[3] + p7[4] * p7[4] + p7[5] * p7[5] + p7[6] * p7[6] > 0.0); };
  if (n < 0) return bad("n < 0");
  if (n > 0 && (!robot || !pose_idx || !cls || !lm_idx || !meas17 || !d2)) return bad("a needed pointer is NULL");
  for (int k = 0; k < n; ++k)
    if (!robot_ok(robot[k]) || (robot2 && !robot_ok(robot2[k]))) return bad("a robot outside [0, SLIDE_MAX_ROBOTS)");
  for (int k = 0; k < n; ++k)
    if (cls[k] != SLIDE_CLS_ELLIPSOID && cls[k] != SLIDE_CLS_CUBE && cls[k] != SLIDE_CLS_CYLINDER) return bad("a class that is not a landmark class");
  if (n > 0 && !closure_finite(meas17, 17 * (size_t)n)) return bad("meas17 holds a non-finite value");
  for (int k = 0; k < n; ++k) {
    const double* a = meas17 + 17 * (size_t)k;
    if (cls[k] == SLIDE_CLS_ELLIPSOID) {
      if (zero3(a)) return bad("a zero bearing");
      if (!(a[3] > 0.0)) return bad("a range <= 0");
    } else if (cls[k] == SLIDE_CLS_CUBE) {
      if (zero_quat(a) || zero_quat(a + 7)) return bad("a zero quaternion");
    } else {
      if (zero_quat(a)) return bad("a zero quaternion");
      if (zero3(a + 10)) return bad("a zero ray");
    }
  }
  return SLIDE_OK;
}
int slide_graph_observation_mahalanobis(slide_graph_t* g, int n, const int32_t* robot, const uint64_t* pose_idx, const int32_t* cls,
                                        const uint64_t* lm_idx, const double* meas17, double* d2, int32_t* dof, double* C81, double* r9,
                                        int32_t* status) {
  const int rc = obs_gate_check_list(n, robot, nullptr, pose_idx, cls, lm_idx, meas17, d2);
  if (rc != SLIDE_OK) return rc;
  if (!g) return obs_gate_bad("the graph is NULL");
  LOCK(g);
  return g->g.observation_mahalanobis(n, robot, pose_idx, cls, lm_idx, meas17, d2, dof, C81, r9, status);
}
// The same gate at a predicted pose.  The list's checks are the call above's (every candidate at the one robot), then the step's and
// the prediction's own; all of them before the graph is looked at.
int slide_graph_predicted_observation_mahalanobis(slide_graph_t* g, int robot, uint64_t from_idx, const double rel7[7], const double est7[7], int n,
                                                  const int32_t* cls, const uint64_t* lm_idx, const double* meas17, double* d2, int32_t* dof,
                                                  double* C81, double* r9, int32_t* status) {
  const char* who = "predicted_observation_mahalanobis";
  if (n < 0) return obs_gate_bad("n < 0", who);
  if (!robot_ok(robot)) return obs_gate_bad("a robot outside [0, SLIDE_MAX_ROBOTS)", who);
  if (!rel7 || !est7) return obs_gate_bad("a needed pointer is NULL", who);
  const std::vector<int32_t> robots((size_t)std::max(n, 1), robot);
  const std::vector<uint64_t> poses((size_t)std::max(n, 1), from_idx);
  const int rc = obs_gate_check_list(n, robots.data(), nullptr, poses.data(), cls, lm_idx, meas17, d2, who);
  if (rc != SLIDE_OK) return rc;
  if (!closure_finite(rel7, 7) || !closure_finite(est7, 7)) return obs_gate_bad("rel7 or est7 holds a non-finite value", who);
  for (const double* p7 : {rel7, est7})
    if (!(p7[3] * p7[3] + p7[4] * p7[4] + p7[5] * p7[5] + p7[6] * p7[6] > 0.0)) return obs_gate_bad("a zero quaternion", who);
  if (!g) return obs_gate_bad("the graph is NULL", who);
  LOCK(g);
  return g->g.predicted_observation_mahalanobis(robot, from_idx, rel7, est7, n, cls, lm_idx, meas17, d2, dof, C81, r9, status);
}
// The joint-compatibility test of groups of such candidates (obs_joint_kernels.hip).  The argument checks come first, need neither
// graph nor device and write nothing: the groups' own, the probability, then the candidates' as above.
// (the groups' and the probability's, shared with the batch's call.  group_outs / cand_outs: every per-group / per-candidate output
// is there; *n: the number of candidates the groups hold)
static int joint_compat_check_groups(const char* who, int n_groups, const int32_t* group_ptr, double prob, bool group_outs, bool cand_outs, int* n) {
  if (n_groups < 0) return obs_gate_bad("n_groups < 0", who);
  if (n_groups > 0 && (!group_ptr || !group_outs)) return obs_gate_bad("a needed pointer is NULL", who);
  if (n_groups > 0 && group_ptr[0] != 0) return obs_gate_bad("group_ptr does not start at 0", who);
  for (int i = 0; i < n_groups; ++i)
    if (group_ptr[i + 1] < group_ptr[i]) return obs_gate_bad("group_ptr decreases", who);
  if (!(prob == 0.0 || (prob > 0.0 && prob < 1.0))) return obs_gate_bad("prob is neither 0 (evaluate only) nor inside (0, 1)", who);
  *n = n_groups > 0 ? group_ptr[n_groups] : 0;
  if (*n > 0 && !cand_outs) return obs_gate_bad("a needed pointer is NULL", who);
  return SLIDE_OK;
}
int slide_graph_observation_joint_compatibility(slide_graph_t* g, int n_groups, const int32_t* group_ptr, const int32_t* robot,
                                                const uint64_t* pose_idx, const int32_t* cls, const uint64_t* lm_idx, const double* meas17,
                                                double prob, int32_t* accepted, double* d2_single, double* d2_joint, int32_t* dof_joint,
                                                int32_t* status, double* group_d2, int32_t* group_dof, int32_t* group_count,
                                                int32_t* group_status) {
  const char* who = "observation_joint_compatibility";
  int n = 0;
  int rc = joint_compat_check_groups(who, n_groups, group_ptr, prob, group_d2 && group_dof && group_count && group_status,
                                     accepted && d2_single && d2_joint && dof_joint && status, &n);
  if (rc == SLIDE_OK) rc = obs_gate_check_list(n, robot, nullptr, pose_idx, cls, lm_idx, meas17, d2_joint, who);
  if (rc != SLIDE_OK) return rc;
  if (!g) return obs_gate_bad("the graph is NULL", who);
  LOCK(g);
  return g->g.observation_joint_compatibility(n_groups, group_ptr, robot, pose_idx, cls, lm_idx, meas17, prob, accepted, d2_single, d2_joint,
                                              dof_joint, status, group_d2, group_dof, group_count, group_status);
}
// The `prob` quantile of chi-square with dof degrees of freedom, as the call above builds its table (host code; no device needed).
int slide_chi2_quantile(double prob, int dof, double* q) { return chi2_quantile(prob, dof, q); }
// The same on the joint graph of a CholBatch: slots where the call above takes robots, the landmark's slot of its own (NULL: the
// pose's).  The argument checks are the single-graph call's and come before the batch or the device is looked at.
int slide_chol_batch_observation_mahalanobis(slide_chol_batch_t* b, int n, const int32_t* pose_slot, const uint64_t* pose_idx, const int32_t* lm_slot,
                                             const int32_t* cls, const uint64_t* lm_idx, const double* meas17, double* d2, int32_t* dof, double* C81,
                                             double* r9, int32_t* status) {
  const int rc = obs_gate_check_list(n, pose_slot, lm_slot, pose_idx, cls, lm_idx, meas17, d2);
  if (rc != SLIDE_OK) return rc;
  if (!b) return obs_gate_bad("the batch is NULL");
  return b->b.joint_observation_mahalanobis(n, pose_slot, pose_idx, lm_slot, cls, lm_idx, meas17, d2, dof, C81, r9, status);
}
// The joint-compatibility test on the joint graph of a CholBatch: slide_graph_observation_joint_compatibility's groups, probability and
// outputs, the candidates named as the call above names them.  The argument checks — that call's group and probability checks, then
// the candidates' with lm_slot checked like pose_slot — come before the batch or the device is looked at and write nothing.
int slide_chol_batch_observation_joint_compatibility(slide_chol_batch_t* b, int n_groups, const int32_t* group_ptr, const int32_t* pose_slot,
                                                     const uint64_t* pose_idx, const int32_t* lm_slot, const int32_t* cls, const uint64_t* lm_idx,
                                                     const double* meas17, double prob, int32_t* accepted, double* d2_single, double* d2_joint,
                                                     int32_t* dof_joint, int32_t* status, double* group_d2, int32_t* group_dof,
                                                     int32_t* group_count, int32_t* group_status) {
  const char* who = "chol_batch_observation_joint_compatibility";
  int n = 0;
  int rc = joint_compat_check_groups(who, n_groups, group_ptr, prob, group_d2 && group_dof && group_count && group_status,
                                     accepted && d2_single && d2_joint && dof_joint && status, &n);
  if (rc == SLIDE_OK) rc = obs_gate_check_list(n, pose_slot, lm_slot, pose_idx, cls, lm_idx, meas17, d2_joint, who);
  if (rc != SLIDE_OK) return rc;
  if (!b) return obs_gate_bad("the batch is NULL", who);
  return b->b.joint_observation_joint_compatibility(n_groups, group_ptr, pose_slot, pose_idx, lm_slot, cls, lm_idx, meas17, prob, accepted, d2_single,
                                                    d2_joint, dof_joint, status, group_d2, group_dof, group_count, group_status);
}

// The duplicate-landmark queries: the Mahalanobis test and the joint marginal of landmark pairs, and the fixed-radius search that
// proposes the pairs.  The argument checks come first and need neither graph nor device; nothing is written on a refusal.
static int lm_pair_check_list(const char* who, bool cov, int n, const int32_t* cls, const uint64_t* idx_a, const uint64_t* idx_b, const double* sig3,
                              const double* sig7, const void* out) {
  auto bad = [who](const char* what) { return obs_gate_bad(what, who); };
  if (n < 0) return bad("n < 0");
  if (n > 0 && (!cls || !idx_a || !idx_b || !out)) return bad("a needed pointer is NULL");
  bool any3 = false, any7 = false;
  for (int k = 0; k < n; ++k) {
    if (cls[k] == SLIDE_CLS_ELLIPSOID) any3 = true;
    else if (cls[k] == SLIDE_CLS_CYLINDER) any7 = true;
    else if (cov && cls[k] == SLIDE_CLS_CUBE) continue;
    else return bad(cov ? "a class that is not a landmark class"
                        : "a class that is neither SLIDE_CLS_ELLIPSOID nor SLIDE_CLS_CYLINDER (a cube's tangent difference is ambiguous under its symmetries)");
  }
  if (cov) return SLIDE_OK;
  if ((any3 && !sig3) || (any7 && !sig7)) return bad("a needed pointer is NULL");
  for (int i = 0; any3 && i < 3; ++i)
    if (!std::isfinite(sig3[i]) || !(sig3[i] > 0.0)) return bad("a sigma that is non-finite or <= 0");
  for (int i = 0; any7 && i < 7; ++i)
    if (!std::isfinite(sig7[i]) || !(sig7[i] > 0.0)) return bad("a sigma that is non-finite or <= 0");
  return SLIDE_OK;
}
int slide_graph_landmark_pair_mahalanobis(slide_graph_t* g, int n, const int32_t* cls, const uint64_t* idx_a, const uint64_t* idx_b,
                                          const double* sigma_point3, const double* sigma_cylinder7, double* d2, int32_t* dof, double* C81,
                                          double* r9, int32_t* route, int32_t* status) {
  const char* who = "landmark_pair_mahalanobis";
  const int rc = lm_pair_check_list(who, false, n, cls, idx_a, idx_b, sigma_point3, sigma_cylinder7, d2);
  if (rc != SLIDE_OK) return rc;
  if (!g) return obs_gate_bad("the graph is NULL", who);
  LOCK(g);
  return g->g.landmark_pairs(false, n, cls, idx_a, idx_b, sigma_point3, sigma_cylinder7, d2, dof, C81, r9, nullptr, route, status);
}
int slide_graph_get_landmark_pair_covariances(slide_graph_t* g, int n, const int32_t* cls, const uint64_t* idx_a, const uint64_t* idx_b,
                                              double* out324n, int32_t* route, int32_t* status) {
  const char* who = "get_landmark_pair_covariances";
  const int rc = lm_pair_check_list(who, true, n, cls, idx_a, idx_b, nullptr, nullptr, out324n);
  if (rc != SLIDE_OK) return rc;
  if (!g) return obs_gate_bad("the graph is NULL", who);
  LOCK(g);
  return g->g.landmark_pairs(true, n, cls, idx_a, idx_b, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, out324n, route, status);
}
static int pairs_within_check(const char* who, int n, double radius, int64_t cap, const void* o1, const void* o2, const void* o3, const void* n_pairs) {
  if (n < 0) return obs_gate_bad("n < 0", who);
  if (cap < 0) return obs_gate_bad("cap < 0", who);
  if (!n_pairs || (cap > 0 && (!o1 || !o2 || !o3))) return obs_gate_bad("a needed pointer is NULL", who);
  if (!std::isfinite(radius) || !(radius > 0.0)) return obs_gate_bad("a radius that is non-finite or <= 0", who);
  return SLIDE_OK;
}
int slide_pairs_within(const double* xyz, const int32_t* label, int n, double radius, int64_t cap, int32_t* out_i, int32_t* out_j, double* out_dist,
                       int64_t* n_pairs) {
  const char* who = "pairs_within";
  const int rc = pairs_within_check(who, n, radius, cap, out_i, out_j, out_dist, n_pairs);
  if (rc != SLIDE_OK) return rc;
  if (n > 0 && !xyz) return obs_gate_bad("a needed pointer is NULL", who);
  if ((long long)n > (long long)INT32_MAX - 256) return obs_gate_bad("more than 2^31 - 257 points", who);
  return pairs_within_host(xyz, label, n, radius, cap, out_i, out_j, out_dist, n_pairs);
}
int slide_graph_landmark_pairs_within(slide_graph_t* g, int cls, double radius, int n_sel, const uint64_t* sel_idx, const int32_t* sel_label,
                                      int64_t cap, uint64_t* idx_a, uint64_t* idx_b, double* dist, int64_t* n_pairs) {
  const char* who = "landmark_pairs_within";
  if (cls != SLIDE_CLS_ELLIPSOID && cls != SLIDE_CLS_CUBE && cls != SLIDE_CLS_CYLINDER) return obs_gate_bad("a class that is not a landmark class", who);
  const int rc = pairs_within_check(who, sel_idx ? n_sel : 0, radius, cap, idx_a, idx_b, dist, n_pairs);
  if (rc != SLIDE_OK) return rc;
  if (!g) return obs_gate_bad("the graph is NULL", who);
  LOCK(g);
  return g->g.landmark_pairs_within(cls, radius, n_sel, sel_idx, sel_label, cap, idx_a, idx_b, dist, n_pairs);
}

// The same three on the joint graph of a CholBatch: a landmark is (slot, cls, idx).  The argument checks are the single-graph calls'
// (then the slots' pointers) and come before the batch or the device is looked at; nothing is written on a refusal.
int slide_chol_batch_landmark_pair_mahalanobis(slide_chol_batch_t* b, int n, const int32_t* cls, const int32_t* slot_a, const uint64_t* idx_a,
                                               const int32_t* slot_b, const uint64_t* idx_b, const double* sigma_point3,
                                               const double* sigma_cylinder7, double* d2, int32_t* dof, double* C81, double* r9, int32_t* status) {
  const char* who = "chol_batch_landmark_pair_mahalanobis";
  const int rc = lm_pair_check_list(who, false, n, cls, idx_a, idx_b, sigma_point3, sigma_cylinder7, d2);
  if (rc != SLIDE_OK) return rc;
  if (n > 0 && (!slot_a || !slot_b)) return obs_gate_bad("a needed pointer is NULL", who);
  if (!b) return obs_gate_bad("the batch is NULL", who);
  return b->b.joint_landmark_pairs(false, n, cls, slot_a, idx_a, slot_b, idx_b, sigma_point3, sigma_cylinder7, d2, dof, C81, r9, nullptr, status);
}
int slide_chol_batch_get_landmark_pair_covariances(slide_chol_batch_t* b, int n, const int32_t* cls, const int32_t* slot_a, const uint64_t* idx_a,
                                                   const int32_t* slot_b, const uint64_t* idx_b, double* out324n, int32_t* status) {
  const char* who = "chol_batch_get_landmark_pair_covariances";
  const int rc = lm_pair_check_list(who, true, n, cls, idx_a, idx_b, nullptr, nullptr, out324n);
  if (rc != SLIDE_OK) return rc;
  if (n > 0 && (!slot_a || !slot_b)) return obs_gate_bad("a needed pointer is NULL", who);
  if (!b) return obs_gate_bad("the batch is NULL", who);
  return b->b.joint_landmark_pairs(true, n, cls, slot_a, idx_a, slot_b, idx_b, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, out324n, status);
}
int slide_chol_batch_landmark_pairs_within(slide_chol_batch_t* b, int cls, double radius, int cross_only, int64_t cap, int32_t* slot_a,
                                           uint64_t* idx_a, int32_t* slot_b, uint64_t* idx_b, double* dist, int64_t* n_pairs) {
  const char* who = "chol_batch_landmark_pairs_within";
  if (cls != SLIDE_CLS_ELLIPSOID && cls != SLIDE_CLS_CUBE && cls != SLIDE_CLS_CYLINDER) return obs_gate_bad("a class that is not a landmark class", who);
  const int rc = pairs_within_check(who, 0, radius, cap, idx_a, idx_b, dist, n_pairs);
  if (rc != SLIDE_OK) return rc;
  if (cap > 0 && (!slot_a || !slot_b)) return obs_gate_bad("a needed pointer is NULL", who);
  if (!b) return obs_gate_bad("the batch is NULL", who);
  return b->b.joint_landmark_pairs_within(cls, radius, cross_only != 0, cap, slot_a, idx_a, slot_b, idx_b, dist, n_pairs);
}

// sloam::FindRelativeMeasurementMatch sloam.cpp:321-412 (host-side bookkeeping: a few dozen stamps per call)
int slide_find_relative_meas_match(int n_robots, const int64_t* pk_sec, const int64_t* pk_nsec, const int32_t* offsets,
                                   const uint64_t* pose_counter, int host, int* n_pending_io, int64_t* m_sec, int64_t* m_nsec,
                                   int32_t* m_robot, int32_t* m_only_odom, int32_t* m_tag, int32_t* match_out, int* n_matches) {
  if (!n_pending_io || !n_matches || host < 0 || host >= n_robots) return SLIDE_ERR_INVALID;
  *n_matches = 0;
  int np = *n_pending_io;
  if (np <= 0) return SLIDE_OK;
  const double max_dt = 0.001;                                        // sloam.cpp:324
  auto closest = [&](int robot, int64_t qs, int64_t qn, int& idx, double& diff) {
    slide_closest_stamp(pk_sec + offsets[robot], pk_nsec + offsets[robot], offsets[robot + 1] - offsets[robot], qs, qn, &idx, &diff);
  };
  auto erase = [&](int i) {
    for (int k = i; k + 1 < np; ++k) {
      m_sec[k] = m_sec[k + 1]; m_nsec[k] = m_nsec[k + 1]; m_robot[k] = m_robot[k + 1]; m_only_odom[k] = m_only_odom[k + 1];
      m_tag[k] = m_tag[k + 1];
    }
    --np;
  };
  for (int i = 0; i < np; ++i) {
    const int r = m_robot[i];
    if (r == host || r < 0 || r >= n_robots || m_only_odom[i]) { *n_pending_io = np; return SLIDE_ERR_INVALID; }
    int io, ih;
    double dt;
    closest(r, m_sec[i], m_nsec[i], io, dt);
    if (io == -1 || dt > max_dt || (uint64_t)io >= pose_counter[r]) continue;
    closest(host, m_sec[i], m_nsec[i], ih, dt);
    if (ih == -1 || dt > max_dt || (uint64_t)ih >= pose_counter[host]) continue;
    int32_t* mo = match_out + 4 * (size_t)(*n_matches);
    mo[0] = m_tag[i]; mo[1] = i; mo[2] = ih; mo[3] = io;
    ++*n_matches;
    erase(i);
    --i;
  }
  // prune measurements both robots have already passed (sloam.cpp:388-410)
  auto later = [](int64_t as, int64_t an, int64_t bs, int64_t bn) { return as > bs || (as == bs && an > bn); };
  for (int i = 0; i < np; ++i) {
    const int r = m_robot[i];
    int64_t os = 0, on = 0, hs = 0, hn = 0;
    if (pose_counter[r] > 0) { os = pk_sec[offsets[r] + pose_counter[r] - 1]; on = pk_nsec[offsets[r] + pose_counter[r] - 1]; }
    if (pose_counter[host] > 0) { hs = pk_sec[offsets[host] + pose_counter[host] - 1]; hn = pk_nsec[offsets[host] + pose_counter[host] - 1]; }
    if (later(os, on, m_sec[i], m_nsec[i]) && later(hs, hn, m_sec[i], m_nsec[i])) { erase(i); --i; }
  }
  *n_pending_io = np;
  return SLIDE_OK;
}

}  // extern "C"
