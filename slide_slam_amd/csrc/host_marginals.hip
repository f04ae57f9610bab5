// Marginal covariances and loop-closure information gain, on one graph and on the exact joint multi-robot graph: the host side of
// cov_kernels.hip and joint_cov_kernels.hip (the classes are declared in host_graph.hpp).  The quadratic forms B^T Sigma B and the
// gates built on them: host_gates.hip.
#include "host_sigma.hpp"

#include <cmath>
#include <functional>
#include <map>
#include <unordered_map>

namespace sl {

// block k of the kernels' 81-stride output -> the packed d x d block q of the caller's
static void unpack_block(const std::vector<double>& h, size_t k, int d, double* out, size_t q) {
  for (int e = 0; e < d * d; ++e) out[q * d * d + e] = h[81 * k + e];
}

// ---- marginals and loop-closure information gain (logEntropy / estimateClosureInfoGain, graph.cpp:421-625) -----------------------
// Single-graph path only: a shard's factor (ghost factors, shared-landmark slots) or a factor shared with a CholBatch is not the
// system of this graph alone.
int HostGraph::marginal_state(const char* who) const {
  if (batch || arrow_on() || up_gh > 0 || !h_gslot_pose.empty() || !h_sh_lid.empty()) {
    g_last_error = std::string(who) + ": marginals are served on the single-graph path only (not in sharded or exact-joint mode)";
    return SLIDE_ERR_INVALID;
  }
  if (!factor_valid || G.T == 0) { g_last_error = std::string(who) + ": no factorisation yet (call solve first)"; return SLIDE_ERR_INVALID; }
  // factors or variables merged since the last solve (any call that uploads pending additions) change the system the device buffers
  // describe — and may re-allocate S, Ld and Winv, or grow ld — while the resident factor is still the old one's
  size_t now[8];
  fact_shape_now(now);
  if (fact_gen != S_gen || std::memcmp(now, fact_shape, sizeof(now)) != 0) {
    g_last_error = std::string(who) + ": the graph changed since the last solve (call solve first)";
    return SLIDE_ERR_INVALID;
  }
  return SLIDE_OK;
}
void HostGraph::fact_shape_now(size_t* out) const {
  const size_t v[8] = {(size_t)G.T, (size_t)G.ld, up_P, up_L, up_pr, up_bt, up_lf, up_gh};
  std::memcpy(out, v, sizeof(v));
}
// the selected inverse of the resident factor, computed once per factorisation
// (marginal_state first: the factor is the one of the uploaded system, so G.T / G.ld are its geometry)
int HostGraph::ensure_sigma() {
  if (sig_serial == fact_serial && sig_T == G.T && sig_ld == G.ld) return SLIDE_OK;
  hipStream_t s = stream;
  const size_t n = (size_t)G.ld * G.T * NB;
  sig_serial = ~0ull;
  if (d_sig.cap != n && d_sig.ensure_exact(n, s) != SLIDE_OK) return SLIDE_ERR_HIP;
  DevArr<double> Z;      // Z_I = L_Ik L_kk^-1 of the recursion: only while it runs (freed at the end of this scope, after a sync)
  if (Z.ensure_exact(n, s) != SLIDE_OK) return SLIDE_ERR_HIP;
  const bool dense = h_prof.size() != (size_t)G.T;
  launch_selected_inverse(G.S, G.ld, G.T, G.Ld, G.Winv, dense ? nullptr : h_prof.data(), dense ? nullptr : G.prof, d_sig.d, Z.d, s);
  SL_HIP(hipGetLastError());
  SL_HIP(hipStreamSynchronize(s));
  sig_serial = fact_serial;
  sig_T = G.T;
  sig_ld = G.ld;
  return SLIDE_OK;
}
int HostGraph::pose_id(int robot, uint64_t idx) const {
  auto it = key2pose.find(pose_key(robot, idx));
  return it == key2pose.end() || (size_t)it->second >= up_P ? -1 : it->second;
}
void HostGraph::robot_poses(int robot, std::vector<int>& out) const {
  out.clear();
  const uint64_t tag = pose_key(robot, 0) >> 56;
  for (const auto& kv : key2pose)
    if ((kv.first >> 56) == tag && (size_t)kv.second < up_P) out.push_back(kv.second);
  std::sort(out.begin(), out.end());
}
void HostGraph::point_landmarks(std::vector<int>& out) const {
  out.clear();
  for (size_t l = 0; l < up_L && l < h_lm_type.size(); ++l)
    if (h_lm_type[l] == VT_POINT && !lm_tomb(l)) out.push_back((int)l);      // (a tombstone of merge_landmarks is no landmark)
}
// isam->marginalCovariance(X(idx)) for n poses of one robot: out36n[36 q ..] row-major, tangent order [rot, trans]
int HostGraph::pose_covariances(int robot, const uint64_t* idx, int n, double* out36n) {
  if (!robot_ok(robot) || n < 0 || (n > 0 && (!idx || !out36n))) return SLIDE_ERR_INVALID;
  for (int i = 0; i < 36 * n; ++i) out36n[i] = 0.0;
  int rc = marginal_state("get_pose_covariances");
  if (rc != SLIDE_OK) return rc;
  std::vector<int> ids(n);
  for (int q = 0; q < n; ++q)
    if ((ids[q] = pose_id(robot, idx[q])) < 0) return SLIDE_MISSING;
  if (n == 0) return SLIDE_OK;
  if ((rc = ensure_sigma()) != SLIDE_OK) return rc;
  hipStream_t s = stream;
  if (d_midx.ensure(n, 0, s) != SLIDE_OK || d_mout.ensure(36 * (size_t)n, 0, s) != SLIDE_OK) return SLIDE_ERR_HIP;
  SL_HIP(hipMemcpyAsync(d_midx.d, ids.data(), n * sizeof(int), hipMemcpyHostToDevice, s));
  launch_pose_blocks(d_sig.d, G.ld, d_midx.d, n, d_mout.d, s);
  SL_HIP(hipMemcpyAsync(out36n, d_mout.d, 36 * (size_t)n * sizeof(double), hipMemcpyDeviceToHost, s));
  SL_HIP(hipStreamSynchronize(s));
  SL_HIP(hipGetLastError());
  return SLIDE_OK;
}
// isam->marginalCovariance(L / C / U(idx)) for n landmarks of one class: d x d each (d = 7 / 9 / 3), tangent order of var_retract
int HostGraph::landmark_covariances(int cls, const uint64_t* idx, int n, double* out) {
  const int d = landmark_dim(cls);
  if (!d || n < 0 || (n > 0 && (!idx || !out))) return SLIDE_ERR_INVALID;
  for (int i = 0; i < d * d * n; ++i) out[i] = 0.0;
  int rc = marginal_state("get_landmark_covariances");
  if (rc != SLIDE_OK) return rc;
  std::vector<int> ids(n);
  for (int q = 0; q < n; ++q)
    if ((ids[q] = lm_lid(cls, idx[q])) < 0) return SLIDE_MISSING;
  if (n == 0) return SLIDE_OK;
  if ((rc = ensure_sigma()) != SLIDE_OK) return rc;
  hipStream_t s = stream;
  if (d_midx.ensure(n, 0, s) != SLIDE_OK || d_mout.ensure(81 * (size_t)n, 0, s) != SLIDE_OK) return SLIDE_ERR_HIP;
  SL_HIP(hipMemcpyAsync(d_midx.d, ids.data(), n * sizeof(int), hipMemcpyHostToDevice, s));
  launch_landmark_covariances(G, d_sig.d, G.ld, d_midx.d, n, d_mout.d, s);
  std::vector<double> h(81 * (size_t)n);
  SL_HIP(hipMemcpyAsync(h.data(), d_mout.d, h.size() * sizeof(double), hipMemcpyDeviceToHost, s));
  SL_HIP(hipStreamSynchronize(s));
  SL_HIP(hipGetLastError());
  for (int q = 0; q < n; ++q) unpack_block(h, q, d, out, q);
  return SLIDE_OK;
}
// logEntropy (graph.cpp:423-466): {sum of the robot's pose marginal traces, sum of the point landmarks' traces, #poses, #landmarks}
int HostGraph::marginal_traces(int robot, double* out4) {
  for (int i = 0; i < 4; ++i) out4[i] = 0.0;
  if (!robot_ok(robot)) return SLIDE_ERR_INVALID;
  int rc = marginal_state("marginal_traces");
  if (rc != SLIDE_OK) return rc;
  std::vector<int> poses, lms;
  robot_poses(robot, poses);
  point_landmarks(lms);
  if ((rc = ensure_sigma()) != SLIDE_OK) return rc;
  hipStream_t s = stream;
  const size_t np = poses.size(), nl = lms.size();
  if (d_midx.ensure(np + nl + 1, 0, s) != SLIDE_OK || d_mout.ensure(36 * np + 81 * nl + 1, 0, s) != SLIDE_OK) return SLIDE_ERR_HIP;
  if (np) SL_HIP(hipMemcpyAsync(d_midx.d, poses.data(), np * sizeof(int), hipMemcpyHostToDevice, s));
  if (nl) SL_HIP(hipMemcpyAsync(d_midx.d + np, lms.data(), nl * sizeof(int), hipMemcpyHostToDevice, s));
  launch_pose_blocks(d_sig.d, G.ld, d_midx.d, (int)np, d_mout.d, s);
  launch_landmark_covariances(G, d_sig.d, G.ld, d_midx.d + np, (int)nl, d_mout.d + 36 * np, s);
  std::vector<double> h(36 * np + 81 * nl);
  if (!h.empty()) SL_HIP(hipMemcpyAsync(h.data(), d_mout.d, h.size() * sizeof(double), hipMemcpyDeviceToHost, s));
  SL_HIP(hipStreamSynchronize(s));
  SL_HIP(hipGetLastError());
  for (size_t p = 0; p < np; ++p)
    for (int a = 0; a < 6; ++a) out4[0] += h[36 * p + 7 * a];
  for (size_t l = 0; l < nl; ++l)
    for (int a = 0; a < 3; ++a) out4[1] += h[36 * np + 81 * l + 4 * a];
  out4[2] = (double)np;
  out4[3] = (double)nl;
  return SLIDE_OK;
}
// The Adjoint of T_b^-1 T_a (row-major 12-double poses: R row-major, then t): the whitened Jacobian of a Between factor (a, b) at zero
// residual is -Ad / sigma on a and I / sigma on b (both charts)
static void between_adjoint(const double* Ta, const double* Tb, double Ad[6][6]) {
  double R[9], t[3], dt[3] = {Ta[9] - Tb[9], Ta[10] - Tb[10], Ta[11] - Tb[11]};
  for (int r = 0; r < 3; ++r) {                      // T_b^-1 T_a = (Rb^T Ra, Rb^T (ta - tb))
    for (int c = 0; c < 3; ++c) R[3 * r + c] = Tb[r] * Ta[c] + Tb[3 + r] * Ta[3 + c] + Tb[6 + r] * Ta[6 + c];
    t[r] = Tb[r] * dt[0] + Tb[3 + r] * dt[1] + Tb[6 + r] * dt[2];
  }
  for (int r = 0; r < 6; ++r)                        // [R 0; t^ R  R]
    for (int c = 0; c < 6; ++c) Ad[r][c] = 0.0;
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) {
      Ad[r][c] = R[3 * r + c];
      Ad[3 + r][3 + c] = R[3 * r + c];
    }
  const double tx[9] = {0, -t[2], t[1], t[2], 0, -t[0], -t[1], t[0], 0};
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) Ad[3 + r][c] = tx[3 * r] * R[c] + tx[3 * r + 1] * R[3 + c] + tx[3 * r + 2] * R[6 + c];
}
// The Woodbury step's host part: C (ncol x ncol, row-major, C = I + J U) symmetrised, C^-1 by Cholesky, g[k] = sum_ab (C^-1)_ab M_k,ab
// (M: the nM matrices one after the other)
static int woodbury_drops(std::vector<double>& Cm, int ncol, const double* M, int nM, double* g) {
  // C^-1 by Cholesky (C = I + J Sigma J^T is SPD); the gains are sum_ab (C^-1)_ab M_ab of the symmetrised matrices
  for (int a = 0; a < ncol; ++a)
    for (int b = 0; b < a; ++b) Cm[(size_t)a * ncol + b] = Cm[(size_t)b * ncol + a] = 0.5 * (Cm[(size_t)a * ncol + b] + Cm[(size_t)b * ncol + a]);
  std::vector<double> Lc((size_t)ncol * ncol, 0.0);
  for (int j = 0; j < ncol; ++j) {
    double d = Cm[(size_t)j * ncol + j];
    for (int k = 0; k < j; ++k) d -= Lc[(size_t)j * ncol + k] * Lc[(size_t)j * ncol + k];
    if (!(d > 0.0)) { g_last_error = "closure_info_gain: I + J Sigma J^T is not positive definite"; return SLIDE_ERR_NOT_SPD; }
    const double ljj = std::sqrt(d);
    Lc[(size_t)j * ncol + j] = ljj;
    for (int i = j + 1; i < ncol; ++i) {
      double v = Cm[(size_t)i * ncol + j];
      for (int k = 0; k < j; ++k) v -= Lc[(size_t)i * ncol + k] * Lc[(size_t)j * ncol + k];
      Lc[(size_t)i * ncol + j] = v / ljj;
    }
  }
  // (on the host: O((6m)^3), about 10^8 flops at the cap m = 64 — the largest part of such a query; a device version is a follow-up)
  std::vector<double> LcT((size_t)ncol * ncol), Ci((size_t)ncol * ncol, 0.0), col(ncol);
  for (int i = 0; i < ncol; ++i)
    for (int k = 0; k < ncol; ++k) LcT[(size_t)i * ncol + k] = Lc[(size_t)k * ncol + i];
  for (int j = 0; j < ncol; ++j) {                   // column j of C^-1: L L^T x = e_j (L^-1 e_j is zero above row j)
    for (int i = 0; i < j; ++i) col[i] = 0.0;
    for (int i = j; i < ncol; ++i) {
      double v = i == j ? 1.0 : 0.0;
      for (int k = j; k < i; ++k) v -= Lc[(size_t)i * ncol + k] * col[k];
      col[i] = v / Lc[(size_t)i * ncol + i];
    }
    for (int i = ncol - 1; i >= 0; --i) {
      double v = col[i];
      for (int k = i + 1; k < ncol; ++k) v -= LcT[(size_t)i * ncol + k] * col[k];
      col[i] = v / Lc[(size_t)i * ncol + i];
    }
    for (int i = 0; i < ncol; ++i) Ci[(size_t)i * ncol + j] = col[i];
  }
  for (int k = 0; k < nM; ++k) {
    double gk = 0.0;
    for (size_t e = 0; e < (size_t)ncol * ncol; ++e) gk += Ci[e] * M[(size_t)k * ncol * ncol + e];
    g[k] = gk;
  }
  return SLIDE_OK;
}
// ---- what the information-gain queries on one graph and on the joint graph share -------------------------------------------------
// The fake Between factors of one query.  The caller maps every pose of the trajectory to its first row of U (six consecutive rows) and
// to its linearisation value on the device; gain_jt builds J^T from those; once U = K^-1 J^T is solved and the grams are queued,
// gain_fetch brings what the host needs of them and gain_drops gives the trace drops.
// A batch holds several candidates: candidate k's poses are p0[k] .. p0[k + 1] - 1 of row / val_src and its fake factors own the
// columns col0[k] .. col0[k + 1] - 1 of J^T, so the candidates' column blocks stand side by side and share no column.
struct GainQuery {
  explicit GainQuery(int n) : GainQuery(std::vector<int>{0, n}) {}
  explicit GainQuery(const std::vector<int>& p0)
      : p0(p0), n(p0.back()), m(n - ((int)p0.size() - 1)), ncol(6 * m), row(n), val_src(n) {
    for (size_t k = 0; k < p0.size(); ++k) col0.push_back(6 * (p0[k] - (int)k));
  }
  const std::vector<int> p0;                // first pose of every candidate, then the number of poses
  const int n, m, ncol;                     // poses of the trajectories, fake factors, columns of J^T
  std::vector<int> col0;                    // first column of every candidate, then ncol
  std::vector<int> row;
  std::vector<const double*> val_src;
  std::vector<int> rcv;                     // J^T's entries ordered by (row, column): the pairs ...
  std::vector<double> vv;                   // ... and the values
  int cands() const { return (int)p0.size() - 1; }
};
// what is wrong with one trajectory, or null
static const char* gain_steps_fault(const uint64_t* traj, int n, const double* travel, int* code) {
  const int m = n - 1;
  *code = SLIDE_ERR_INVALID;
  if (m < 1 || !traj || !travel) return "closure_info_gain: the trajectory needs at least two poses";
  if (m > SLIDE_INFO_GAIN_MAX_STEPS) { *code = SLIDE_ERR_CAPACITY; return "closure_info_gain: more than SLIDE_INFO_GAIN_MAX_STEPS steps"; }
  for (int i = 0; i < m; ++i)
    if (!(travel[i] > 0.0) || !std::isfinite(travel[i])) return "closure_info_gain: travel distances must be > 0";
  *code = SLIDE_OK;
  return nullptr;
}
static int gain_check_steps(const uint64_t* traj, int n, const double* travel) {
  int rc;
  if (const char* why = gain_steps_fault(traj, n, travel, &rc)) g_last_error = why;
  return rc;
}
static int gain_check_sigma(const double* sigma6) {
  for (int a = 0; a < 6; ++a)
    if (!(sigma6[a] > 0.0) || !std::isfinite(sigma6[a])) { g_last_error = "closure_info_gain: sigma_per_m must be > 0"; return SLIDE_ERR_INVALID; }
  return SLIDE_OK;
}
// J^T, entry by entry (row of U, column col0[k] + 6 i + a for step i of candidate k); a repeated pose sums its blocks.  val: the
// linearisation values of the poses (12 each), travel: one entry per pose (a candidate's last one is not read)
static void gain_jt(GainQuery& q, const double* val, const double* travel, const double* sigma6) {
  std::map<std::pair<int, int>, double> jt;
  for (int k = 0; k < q.cands(); ++k)
    for (int p = q.p0[k]; p + 1 < q.p0[k + 1]; ++p) {
      const int col = q.col0[k] + 6 * (p - q.p0[k]);
      double Ad[6][6];
      between_adjoint(val + 12 * (size_t)(p + 1), val + 12 * (size_t)p, Ad);      // (c_{i+1}, c_i)
      for (int a = 0; a < 6; ++a) {
        const double w = 1.0 / (sigma6[a] * travel[p]);
        for (int c = 0; c < 6; ++c) jt[{q.row[p + 1] + c, col + a}] += -Ad[a][c] * w;
        jt[{q.row[p] + a, col + a}] += w;
      }
    }
  for (const auto& kv : jt) { q.rcv.push_back(kv.first.first); q.rcv.push_back(kv.first.second); q.vv.push_back(kv.second); }
}
// the same with the values read from the device, pose by pose (val_src)
static int gain_jt(GainQuery& q, const double* travel, const double* sigma6, hipStream_t s) {
  std::vector<double> val(12 * (size_t)q.n);
  for (int k = 0; k < q.n; ++k) SL_HIP(hipMemcpyAsync(val.data() + 12 * k, q.val_src[k], 12 * sizeof(double), hipMemcpyDeviceToHost, s));
  SL_HIP(hipStreamSynchronize(s));
  gain_jt(q, val.data(), travel, sigma6);
  return SLIDE_OK;
}
// Behind the solve and the grams: U (leading dimension ldu) and the nM gram matrices Md on the device, to the host
static int gain_fetch(const GainQuery& q, const double* U, size_t ldu, const double* Md, int nM, hipStream_t s, GainFetched& h) {
  const int ncol = q.ncol;
  h.M.resize((size_t)nM * ncol * ncol);
  h.Urow.resize((size_t)q.n * 6 * ncol);
  SL_HIP(hipMemcpyAsync(h.M.data(), Md, h.M.size() * sizeof(double), hipMemcpyDeviceToHost, s));
  for (int k = 0; k < q.n; ++k)
    SL_HIP(hipMemcpy2DAsync(h.Urow.data() + (size_t)k * 6 * ncol, 6 * sizeof(double), U + q.row[k], ldu * sizeof(double), 6 * sizeof(double), ncol,
                            hipMemcpyDeviceToHost, s));
  SL_HIP(hipStreamSynchronize(s));
  SL_HIP(hipGetLastError());
  return SLIDE_OK;
}
// g[k] = tr(C^-1 M_k), C = I + J U (host only)
static int gain_drops(const GainQuery& q, const GainFetched& h, int nM, double* g) {
  const int ncol = q.ncol;
  const size_t nn = (size_t)ncol * ncol;
  std::unordered_map<int, int> row_of;      // row of U -> 6 (trajectory slot) + coordinate
  for (int k = 0; k < q.n; ++k)
    for (int a = 0; a < 6; ++a) row_of.emplace(q.row[k] + a, 6 * k + a);
  std::vector<double> Cm(nn, 0.0);
  for (int a = 0; a < ncol; ++a) Cm[(size_t)a * ncol + a] = 1.0;
  for (size_t e = 0; e < q.vv.size(); ++e) {          // (J U)[jrow][col] += J[jrow][row] U[row][col]
    const int jrow = q.rcv[2 * e + 1], qa = row_of[q.rcv[2 * e]];
    const double* u = h.Urow.data() + (size_t)(qa / 6) * 6 * ncol + qa % 6;
    for (int c = 0; c < ncol; ++c) Cm[(size_t)jrow * ncol + c] += q.vv[e] * u[6 * (size_t)c];
  }
  return woodbury_drops(Cm, ncol, h.M.data(), nM, g);
}

// ---- many candidates in one call (closure_info_gain_batch on one graph and on the joint graph) -----------------------------------
// The list is cut into sweeps of whole candidates, SLIDE_INFO_GAIN_SWEEP_COLS columns of J^T at the most.  Per sweep: the candidates'
// column blocks of J^T side by side, ONE multi-column solve U = K^-1 J^T, per candidate the diagonal blocks of the grams
// (k_gram_blocks) and the Woodbury step on the device (k_woodbury_blocks).  Of U, C and the grams nothing comes to the host: a sweep
// reads back GAIN_MAX_GRAMS doubles and a flag per candidate.  Every candidate stands alone against the resident factor, and its bits do
// not depend on its neighbours (the substitutions treat each column by itself; the new kernels' orders depend on the candidate alone).
static_assert(GAIN_MAX_STEPS == SLIDE_INFO_GAIN_MAX_STEPS && 6 * GAIN_MAX_STEPS <= SLIDE_INFO_GAIN_SWEEP_COLS, "a sweep holds any one candidate");
// One candidate as its back end checked and located it: st (a fault keeps it out of the sweeps), its poses' first rows in U and their
// linearisation values, its travel distances
struct GainCand { int st = SLIDE_OK; std::vector<int> row; std::vector<double> val; const double* travel = nullptr; };
// What differs between the back ends.  alloc: R and U (ldu rows by the widest sweep's columns) and the back end's own tables, from the
// query's scratch.  A sweep: begin (zero what the solve adds into), J^T scattered into R by the driver, solve (U = K^-1 R), grams (the
// nM row sums, each through `gram`: rows of X, the list or null for 0 .. nrows - 1).
struct GainBackend {
  using Gram = std::function<void(int q, const double* X, size_t ldx, const int* rows, int nrows)>;
  hipStream_t s = nullptr;
  size_t ldu = 0;
  int nM = 0;
  double *R = nullptr, *U = nullptr;
  std::function<int(Scratch& sc, int max_ncol)> alloc;
  std::function<int(int ncol)> begin, solve;
  std::function<void(int ncol, const Gram& gram)> grams;
};
// whole-call faults of a candidate list
static int gain_check_list(int n_cand, const int32_t* off, const uint64_t* traj, const double* travel, const void* out) {
  if (n_cand < 1 || !off || !out) { g_last_error = "closure_info_gain_batch: needs at least one candidate, its offsets and an output"; return SLIDE_ERR_INVALID; }
  for (int k = 0; k < n_cand; ++k)
    if (off[k] < 0 || off[k + 1] < off[k]) { g_last_error = "closure_info_gain_batch: the candidates' offsets must not decrease"; return SLIDE_ERR_INVALID; }
  if (off[n_cand] > off[0] && (!traj || !travel)) { g_last_error = "closure_info_gain_batch: no trajectories"; return SLIDE_ERR_INVALID; }
  return SLIDE_OK;
}
// g: GAIN_MAX_GRAMS doubles per candidate (nM written, zeros for a candidate with a fault); a candidate whose C is not positive definite
// gets SLIDE_ERR_NOT_SPD
static int gain_batch(GainBackend& be, std::vector<GainCand>& cands, const double* sigma6, double* g) {
  hipStream_t s = be.s;
  struct Sweep {
    std::vector<int> ids, p0{0};
    std::vector<GainCandDev> cd;
    std::vector<int4> jobs;
    size_t msz = 0, part = 0, work = 0;
    int ncol = 0;
  };
  std::vector<Sweep> sweeps;
  for (size_t k = 0; k < cands.size(); ++k) {
    for (int q = 0; q < GAIN_MAX_GRAMS; ++q) g[GAIN_MAX_GRAMS * k + q] = 0.0;
    if (cands[k].st != SLIDE_OK) continue;
    const int nk = 6 * ((int)cands[k].row.size() - 1);
    if (sweeps.empty() || sweeps.back().ncol + nk > SLIDE_INFO_GAIN_SWEEP_COLS) sweeps.emplace_back();
    Sweep& w = sweeps.back();
    GainCandDev cd{w.ncol, nk, gain_gram_splits(nk), 0, (long long)w.msz, (long long)w.part, (long long)w.work};
    gram_jobs(w.jobs, (int)w.ids.size(), nk, cd.nsplit);
    w.msz += (size_t)nk * nk;
    w.part += (size_t)nk * nk * cd.nsplit;
    if (nk > GAIN_LDS_DIM) w.work += (size_t)nk * nk;
    w.ncol += nk;
    w.p0.push_back(w.p0.back() + (int)cands[k].row.size());
    w.ids.push_back((int)k);
    w.cd.push_back(cd);
  }
  if (sweeps.empty()) return SLIDE_OK;
  size_t max_nc = 0, max_jobs = 0, max_msz = 0, max_part = 0, max_work = 0;
  int max_ncol = 0;
  for (const Sweep& w : sweeps) {
    max_nc = std::max(max_nc, w.ids.size()); max_jobs = std::max(max_jobs, w.jobs.size()); max_msz = std::max(max_msz, w.msz);
    max_part = std::max(max_part, w.part); max_work = std::max(max_work, w.work); max_ncol = std::max(max_ncol, w.ncol);
  }
  const size_t max_ne = 7 * (size_t)max_ncol;        // (a row of J: six entries on c_{i+1}, one on c_i)
  Scratch sc(s);
  int rc = be.alloc(sc, max_ncol);
  if (rc != SLIDE_OK) return rc;
  int* d_rc = sc.alloc<int>(2 * max_ne);
  int* d_jptr = sc.alloc<int>((size_t)max_ncol + 1);
  int* d_jrow = sc.alloc<int>(max_ne);
  int* d_flag = sc.alloc<int>(max_nc);
  double* d_val = sc.alloc<double>(max_ne);
  double* d_jval = sc.alloc<double>(max_ne);
  double* d_g = sc.alloc<double>(GAIN_MAX_GRAMS * max_nc);
  double* d_M = sc.alloc<double>(be.nM * max_msz);
  double* d_part = sc.alloc<double>(max_part);
  double* d_work = sc.alloc<double>(max_work);
  GainCandDev* d_cd = sc.alloc<GainCandDev>(max_nc);
  int4* d_jobs = sc.alloc<int4>(max_jobs);
  if (!sc.ok()) { g_last_error = "closure_info_gain_batch: out of device memory"; return SLIDE_ERR_HIP; }
  std::vector<double> hg(GAIN_MAX_GRAMS * max_nc);
  std::vector<int> hflag(max_nc);
  for (const Sweep& w : sweeps) {
    const int nc = (int)w.ids.size();
    GainQuery q(w.p0);
    std::vector<double> val(12 * (size_t)q.n), tv(q.n, 0.0);
    for (int k = 0; k < nc; ++k) {
      const GainCand& c = cands[w.ids[k]];
      std::copy(c.row.begin(), c.row.end(), q.row.begin() + w.p0[k]);
      std::copy(c.val.begin(), c.val.end(), val.begin() + 12 * (size_t)w.p0[k]);
      std::copy(c.travel, c.travel + c.row.size() - 1, tv.begin() + w.p0[k]);
    }
    gain_jt(q, val.data(), tv.data(), sigma6);
    // the same entries by column of J^T (a row of J), rows ascending: what the Woodbury step walks
    const int ne = (int)q.vv.size();
    std::vector<int> jptr(q.ncol + 1, 0), jrow(ne);
    std::vector<double> jval(ne);
    for (int e = 0; e < ne; ++e) ++jptr[q.rcv[2 * e + 1] + 1];
    for (int c = 0; c < q.ncol; ++c) jptr[c + 1] += jptr[c];
    std::vector<int> at(jptr.begin(), jptr.end() - 1);
    for (int e = 0; e < ne; ++e) { const int o = at[q.rcv[2 * e + 1]]++; jrow[o] = q.rcv[2 * e]; jval[o] = q.vv[e]; }
    SL_HIP(sc.upload(d_rc, q.rcv));
    SL_HIP(sc.upload(d_val, q.vv));
    SL_HIP(sc.upload(d_jptr, jptr));
    SL_HIP(sc.upload(d_jrow, jrow));
    SL_HIP(sc.upload(d_jval, jval));
    SL_HIP(sc.upload(d_cd, w.cd));
    SL_HIP(sc.upload(d_jobs, w.jobs));
    if ((rc = be.begin(q.ncol)) != SLIDE_OK) return rc;
    launch_scatter(d_rc, d_val, ne, be.R, (int)be.ldu, s);
    if ((rc = be.solve(q.ncol)) != SLIDE_OK) return rc;
    be.grams(q.ncol, [&](int qi, const double* X, size_t ldx, const int* rows, int nrows) {
      launch_gram_blocks(X, ldx, rows, nrows, d_cd, nc, d_jobs, (int)w.jobs.size(), d_part, d_M + qi * w.msz, s);
    });
    if (launch_woodbury_blocks(be.U, be.ldu, d_cd, nc, d_jptr, d_jrow, d_jval, d_M, w.msz, be.nM, d_work, d_g, d_flag, w.work < w.msz, w.work > 0, s)) {
      g_last_error = "closure_info_gain_batch: the device refuses the Woodbury kernel's LDS";
      return SLIDE_ERR_HIP;
    }
    SL_HIP(hipGetLastError());
    SL_HIP(hipMemcpyAsync(hg.data(), d_g, GAIN_MAX_GRAMS * (size_t)nc * sizeof(double), hipMemcpyDeviceToHost, s));
    SL_HIP(hipMemcpyAsync(hflag.data(), d_flag, nc * sizeof(int), hipMemcpyDeviceToHost, s));
    SL_HIP(hipStreamSynchronize(s));
    for (int k = 0; k < nc; ++k) {
      if (hflag[k]) { cands[w.ids[k]].st = SLIDE_ERR_NOT_SPD; continue; }
      for (int qi = 0; qi < be.nM; ++qi) g[GAIN_MAX_GRAMS * (size_t)w.ids[k] + qi] = hg[GAIN_MAX_GRAMS * (size_t)k + qi];
    }
  }
  return SLIDE_OK;
}

// estimateClosureInfoGain (graph.cpp:469-623) in the linear-Gaussian model of the resident factor.  Fake factor i is a Between factor
// (c_{i+1}, c_i) measuring the relative pose of the linearisation values (residual 0), noise sigma_per_m * travel[i]; its whitened
// Jacobian there is  -Ad(T_{c_i}^-1 T_{c_{i+1}}) / sigma  on c_{i+1} and  I / sigma  on c_i (both charts).  With J (6m x n) these rows,
// U = Sigma J^T (substitutions with 6m right-hand sides on the factor), C = I + J U:
//     Sigma - (H + J^T J)^-1 = U C^-1 U^T      (Woodbury)
// so the trace drops are tr(C^-1 sum_p U_p U_p^T) over the robot's poses and tr(C^-1 sum_l V_l V_l^T) over the point landmarks,
// V_l = sum_f U_{p_f} F_f (Sigma_lP = -sum_f F_f^T Sigma(p_f, :)).  total = 10 pose + landmark (graph.cpp:622).  iSAM2's update could
// relinearise variables while the fake factors are in; this linear model does not.  The graph, its factor and Sigma are left untouched.
int HostGraph::closure_info_gain(int robot, const uint64_t* traj, int n, const double* travel, const double* sigma6, double* out3) {
  for (int i = 0; i < 3; ++i) out3[i] = 0.0;
  if (!robot_ok(robot)) return SLIDE_ERR_INVALID;
  int rc = gain_check_steps(traj, n, travel);
  if (rc != SLIDE_OK) return rc;
  if (!sigma6) sigma6 = P.noise_model_odom_vec;      // (noise_model_pose_vec_per_m, graph.h:115, is never set in the reference)
  if ((rc = gain_check_sigma(sigma6)) != SLIDE_OK) return rc;
  if ((rc = marginal_state("closure_info_gain")) != SLIDE_OK) return rc;
  GainQuery q(n);
  for (int k = 0; k < n; ++k) {
    const int id = pose_id(robot, traj[k]);
    if (id < 0) return SLIDE_MISSING;
    q.row[k] = 6 * id;
    q.val_src[k] = G.pose_val + 12 * (size_t)id;
  }
  hipStream_t s = stream;
  const int ncol = q.ncol, T = G.T, nT = T * NB;
  if ((rc = gain_jt(q, travel, sigma6, s)) != SLIDE_OK) return rc;
  const int ne = (int)q.vv.size();
  std::vector<int> poses, lms;
  robot_poses(robot, poses);
  point_landmarks(lms);
  std::vector<int> prow;
  for (int p : poses)
    for (int a = 0; a < 6; ++a) prow.push_back(6 * p + a);
  const size_t nl = lms.size(), ldv = std::max<size_t>(9 * nl, 1);
  if (d_igB.ensure((size_t)ncol * nT, 0, s) != SLIDE_OK || d_igU.ensure((size_t)ncol * nT, 0, s) != SLIDE_OK ||
      d_igV.ensure((size_t)ncol * ldv, 0, s) != SLIDE_OK || d_igM.ensure(2 * (size_t)ncol * ncol, 0, s) != SLIDE_OK ||
      d_igrc.ensure(2 * (size_t)ne + prow.size() + nl + 1, 0, s) != SLIDE_OK || d_igval.ensure(ne, 0, s) != SLIDE_OK)
    return SLIDE_ERR_HIP;
  int* d_rows = d_igrc.d + 2 * ne;
  int* d_lms = d_rows + prow.size();
  SL_HIP(hipMemsetAsync(d_igB.d, 0, (size_t)ncol * nT * sizeof(double), s));
  SL_HIP(hipMemcpyAsync(d_igrc.d, q.rcv.data(), q.rcv.size() * sizeof(int), hipMemcpyHostToDevice, s));
  SL_HIP(hipMemcpyAsync(d_igval.d, q.vv.data(), ne * sizeof(double), hipMemcpyHostToDevice, s));
  if (!prow.empty()) SL_HIP(hipMemcpyAsync(d_rows, prow.data(), prow.size() * sizeof(int), hipMemcpyHostToDevice, s));
  if (nl) SL_HIP(hipMemcpyAsync(d_lms, lms.data(), nl * sizeof(int), hipMemcpyHostToDevice, s));
  launch_scatter(d_igrc.d, d_igval.d, ne, d_igB.d, nT, s);
  const bool dense = h_prof.size() != (size_t)T;
  launch_multi_solve(G.S, G.ld, T, G.Ld, G.Winv, dense ? nullptr : h_prof.data(), d_igB.d, d_igU.d, ncol, s);
  double* Mp = d_igM.d;
  double* Ml = d_igM.d + (size_t)ncol * ncol;
  launch_gram(d_igU.d, nT, ncol, d_rows, (int)prow.size(), Mp, s);
  SL_HIP(hipMemsetAsync(Ml, 0, (size_t)ncol * ncol * sizeof(double), s));
  if (nl) {
    launch_landmark_V(G, d_igU.d, nT, ncol, d_lms, (int)nl, d_igV.d, ldv, s);
    launch_gram(d_igV.d, ldv, ncol, nullptr, (int)(9 * nl), Ml, s);
  }
  double gs[2];
  GainFetched h;
  if ((rc = gain_fetch(q, d_igU.d, nT, d_igM.d, 2, s, h)) != SLIDE_OK || (rc = gain_drops(q, h, 2, gs)) != SLIDE_OK) return rc;
  const double gp = gs[0], gl = gs[1];
  out3[0] = 10.0 * gp + gl;
  out3[1] = gp;
  out3[2] = gl;
  return SLIDE_OK;
}
// The same for a list: candidate k is traj[off[k] .. off[k + 1]) with the travel distances at the same places, out3n[3 k ..] what the
// call above gives for it alone, status[k] its own fault (or null).  Whole-call refusals as above, nothing written then.
int HostGraph::closure_info_gain_batch(int robot, int n_cand, const int32_t* off, const uint64_t* traj, const double* travel,
                                       const double* sigma6, double* out3n, int32_t* status) {
  if (!robot_ok(robot)) return SLIDE_ERR_INVALID;
  int rc = gain_check_list(n_cand, off, traj, travel, out3n);
  if (rc != SLIDE_OK) return rc;
  if (!sigma6) sigma6 = P.noise_model_odom_vec;
  if ((rc = gain_check_sigma(sigma6)) != SLIDE_OK) return rc;
  if ((rc = marginal_state("closure_info_gain")) != SLIDE_OK) return rc;
  hipStream_t s = stream;
  std::vector<double> pv(12 * up_P);                 // every pose's linearisation value, in one copy
  SL_HIP(hipMemcpyAsync(pv.data(), G.pose_val, pv.size() * sizeof(double), hipMemcpyDeviceToHost, s));
  SL_HIP(hipStreamSynchronize(s));
  std::vector<GainCand> cands(n_cand);
  for (int k = 0; k < n_cand; ++k) {
    GainCand& c = cands[k];
    const int nk = off[k + 1] - off[k];
    c.travel = travel + off[k];
    if (gain_steps_fault(traj + off[k], nk, c.travel, &c.st)) continue;
    for (int i = 0; i < nk && c.st == SLIDE_OK; ++i) {
      const int id = pose_id(robot, traj[off[k] + i]);
      if (id < 0) { c.st = SLIDE_MISSING; break; }
      c.row.push_back(6 * id);
      c.val.insert(c.val.end(), pv.begin() + 12 * (size_t)id, pv.begin() + 12 * (size_t)id + 12);
    }
  }
  const int T = G.T, nT = T * NB;
  std::vector<int> poses, lms, prow;
  robot_poses(robot, poses);
  point_landmarks(lms);
  for (int p : poses)
    for (int a = 0; a < 6; ++a) prow.push_back(6 * p + a);
  const size_t nl = lms.size(), ldv = std::max<size_t>(9 * nl, 1);
  const bool dense = h_prof.size() != (size_t)T;
  int *d_rows = nullptr, *d_lms = nullptr;
  double* V = nullptr;
  GainBackend be;
  be.s = s; be.ldu = nT; be.nM = 2;
  be.alloc = [&](Scratch& sc, int max_ncol) -> int {
    be.R = sc.alloc<double>((size_t)max_ncol * nT);
    be.U = sc.alloc<double>((size_t)max_ncol * nT);
    V = sc.alloc<double>((size_t)max_ncol * ldv);
    d_rows = sc.alloc<int>(prow.size() + nl);
    if (!sc.ok()) { g_last_error = "closure_info_gain_batch: out of device memory"; return SLIDE_ERR_HIP; }
    d_lms = d_rows + prow.size();
    SL_HIP(sc.upload(d_rows, prow));
    SL_HIP(sc.upload(d_lms, lms));
    return SLIDE_OK;
  };
  be.begin = [&](int ncol) -> int {
    SL_HIP(hipMemsetAsync(be.R, 0, (size_t)ncol * nT * sizeof(double), s));
    return SLIDE_OK;
  };
  be.solve = [&](int ncol) -> int {
    launch_multi_solve(G.S, G.ld, T, G.Ld, G.Winv, dense ? nullptr : h_prof.data(), be.R, be.U, ncol, s);
    return SLIDE_OK;
  };
  be.grams = [&](int ncol, const GainBackend::Gram& gram) {
    gram(0, be.U, nT, d_rows, (int)prow.size());
    if (nl) launch_landmark_V(G, be.U, nT, ncol, d_lms, (int)nl, V, ldv, s);
    gram(1, V, ldv, nullptr, (int)(9 * nl));
  };
  std::vector<double> g(GAIN_MAX_GRAMS * (size_t)n_cand);
  if ((rc = gain_batch(be, cands, sigma6, g.data())) != SLIDE_OK) return rc;
  for (int k = 0; k < n_cand; ++k) {
    const bool ok = cands[k].st == SLIDE_OK;
    const double gp = ok ? g[GAIN_MAX_GRAMS * (size_t)k] : 0.0, gl = ok ? g[GAIN_MAX_GRAMS * (size_t)k + 1] : 0.0;
    out3n[3 * k] = ok ? 10.0 * gp + gl : 0.0;
    out3n[3 * k + 1] = gp;
    out3n[3 * k + 2] = gl;
    if (status) status[k] = cands[k].st;
  }
  return SLIDE_OK;
}

// ---- marginals on the joint graph: the selected inverse over the exact joint pass's factor (joint_cov_kernels.hip) -------
// What the pass leaves behind and this reads (nothing of it is scratch of the pass): every robot's band factor in S (segments' diagonal
// blocks in Ld / Winv, their border rows W^T below the band), the windows' second-level factor in bord (Ld2 / Winv2), the separator's
// leaves and top block in sepS (sep_Ld / sep_Winv; the top block holds the factor of the per-half sums after the canonical pass), its lambda
// rows below them, and the lambda block's negative factored in lamS (lam_Ld / lam_Winv).  The queries write none of it.
void CholBatch::free_joint_sigma() {
  if (jsig_sep) (void)hipFree(jsig_sep);
  jsig_sep = nullptr;
  for (double* p : jsig_rob) if (p) (void)hipFree(p);
  for (int* p : jsig_prow) if (p) (void)hipFree(p);
  jsig_rob.clear(); jsig_prow.clear(); jsig_lds.clear();
  jsig_serial = 0;
}
int CholBatch::joint_state(const char* who, int slot) {
  const std::string w = std::string(who) + ": ";
  if (slot < 0 || slot >= n) { g_last_error = w + "no such slot"; return SLIDE_ERR_INVALID; }
  if (!arrow || pcg_iters > 0) { g_last_error = w + "the batch does not run exact joint passes (a PCG or block-Jacobi pass leaves no joint factor)"; return SLIDE_ERR_INVALID; }
  if (sep_owner >= 0) { g_last_error = w + "this rank owns one leaf of the separator (a job spread over GPUs): it holds only that leaf's factor"; return SLIDE_ERR_INVALID; }
  if (exact_serial == 0 || (int)exact_shape.size() != n) {
    g_last_error = w + "no whole exact joint pass has run since the batch was configured (call pass_all first)";
    return SLIDE_ERR_INVALID;
  }
  {
    std::lock_guard<std::mutex> lk(mtx);
    if (pass_dirty) { g_last_error = w + "the batch's graphs changed since the last pass"; return SLIDE_ERR_INVALID; }
  }
  for (int i = 0; i < n; ++i) {
    HostGraph* g = graphs[i];
    if (!g) { g_last_error = w + "a slot of the batch is empty"; return SLIDE_ERR_INVALID; }
    std::lock_guard<std::mutex> gl(g->mtx);
    std::vector<size_t> now(10);
    g->fact_shape_now(now.data());
    now[8] = (size_t)g->fact_serial; now[9] = (size_t)g->S_gen;
    if (!g->pend_facs.empty() || !g->pend_vars.empty() || now != exact_shape[i]) {
      g_last_error = w + "the graphs changed since the last exact joint pass (run a pass first)";
      return SLIDE_ERR_INVALID;
    }
  }
  return SLIDE_OK;
}
int CholBatch::joint_robot(int slot) const {
  const HostGraph* g = graphs[slot];
  for (const auto& kv : g->key2pose)
    if (kv.second == 0)
      for (int r = 0; r < SLIDE_MAX_ROBOTS; ++r)
        if ((HostGraph::pose_key(r, 0) >> 56) == (kv.first >> 56)) return r;
  return 0;
}
// The elimination tree of the last exact pass (joint_state first: hG / the graphs' host tables describe the factor the buffers hold).
// Shared by the selected inverse and the many-right-hand-side solve.
void CholBatch::joint_tree(JointTree& t) const {
  const int Ts = sep_Ts, nl = sep_nl, Tsep = Ts + nl;
  t.Ts = Ts; t.Tsep = Tsep;
  t.sTa = sep_leafT[0]; t.sTL = sep_dissected() ? t.sTa + sep_leafT[1] : 0;
  std::vector<JSinvSys>& Y = t.Y;
  std::vector<int>& rp = t.rp;
  std::vector<int>& rows = t.rows;
  auto add_col = [&](const std::vector<int>& r) { rows.insert(rows.end(), r.begin(), r.end()); rp.push_back((int)rows.size()); };
  // system 0: the separator — leaf a, leaf b (no rows of the other leaf), the top block, then the lambda block (D = -I)
  {
    JSinvSys y{};
    y.S = sepS; y.ld = (Ts + nl + 1) * NB; y.Tb = Ts; y.B = lamS; y.ldb = (nl + 1) * NB;
    y.Ld = sep_Ld; y.Winv = sep_Winv; y.Ld2 = lam_Ld; y.Winv2 = lam_Winv; y.neg0 = Ts; y.col0 = 0; y.lds = (long long)Tsep * NB;
    const int sTa = t.sTa, sTL = t.sTL;
    for (int k = 0; k < Tsep; ++k) {
      std::vector<int> r;
      if (k < Ts) {
        int hi = Ts - 1, top0 = Ts;
        if (sep_dissected() && k < sTL) {
          const int b = k >= sTa, t0 = b ? sTa : 0;
          hi = t0 + h_leaf_prof[b][k - t0];
          top0 = sTL;
        } else if (!sep_dissected() && sep_prof_on && (int)h_sep_prof.size() == Ts) hi = h_sep_prof[k];
        for (int i = k + 1; i <= hi; ++i) r.push_back(i);
        for (int i = top0; i < Ts; ++i) r.push_back(i);      // (a leaf's column: the top block's rows, past the leaf)
        for (int i = Ts; i < Tsep; ++i) r.push_back(i);
      } else {
        for (int i = k + 1; i < Tsep; ++i) r.push_back(i);
      }
      add_col(r);
    }
    Y.push_back(y);
  }
  // systems 1 .. n: the robots — band columns of the segments (a segment's profile, its active border rows), then the windows (dense)
  t.steps.assign(n, {}); t.ranges.assign(n, {});
  t.T.assign(n, 0); t.Tc.assign(n, 0); t.Trow.assign(n, 0); t.gn.assign(n, 0); t.map.assign(n, {}); t.prow.assign(n, {});
  for (int i = 0; i < n; ++i) {
    const HostGraph* g = graphs[i];
    const GraphDev& G = hG[i];
    const int T = G.T, nbr = G.nbr, nsep = G.nsep > 0 && !g->segs.empty() ? G.nsep : 0, Tc = T + nsep, Trow = T + nbr;
    JSinvSys y{};
    y.S = G.S; y.ld = G.ld; y.Tb = T; y.B = G.bord; y.ldb = G.ldb; y.Ld = G.Ld; y.Winv = G.Winv; y.Ld2 = g->d_Ld2.d; y.Winv2 = g->d_Winv2.d;
    y.neg0 = 1 << 30; y.col0 = (int)rp.size() - 1; y.lds = (long long)Trow * NB;
    std::vector<std::vector<int>> colrows(Tc);
    std::vector<std::pair<int, int>>& ranges = t.ranges[i];      // the column ranges factored side by side
    if (nsep > 0) {
      const int NS = (int)g->segs.size();
      for (int q = 0; q < NS; ++q) {
        const HostGraph::Seg sg = g->segs[q];
        ranges.emplace_back(sg.t0, sg.t1);
        for (int k = sg.t0; k < sg.t1; ++k) {
          const int hi = std::min(sg.t1 - 1, sg.t0 + g->seg_prof[q][k - sg.t0]);
          for (int r = k + 1; r <= hi; ++r) colrows[k].push_back(r);
          for (int tt = 0; tt < nbr; ++tt) {
            const size_t e = 1 + (size_t)NS + (size_t)q * (nbr + 1) + tt;
            const int sf = e < g->seg_tab.size() ? g->seg_tab[e] : 0;
            if (sf <= k) colrows[k].push_back(T + tt);
          }
        }
      }
      for (int k = T; k < Tc; ++k)
        for (int r = k + 1; r < Trow; ++r) colrows[k].push_back(r);
    } else {
      ranges.emplace_back(0, T);
      const bool dense = g->h_prof.size() != (size_t)T;
      for (int k = 0; k < T; ++k) {
        const int hi = dense ? T - 1 : g->h_prof[k];
        for (int r = k + 1; r <= hi; ++r) colrows[k].push_back(r);
        for (int tt = 0; tt < nbr; ++tt)
          if ((size_t)tt >= g->h_bfirst.size() || g->h_bfirst[tt] <= k) colrows[k].push_back(T + tt);
      }
    }
    for (int k = 0; k < Tc; ++k) add_col(colrows[k]);
    for (int k = Tc - 1; k >= T; --k) t.steps[i].push_back({k});
    for (int st = 0;; ++st) {
      std::vector<int> cs;
      for (const auto& rg : ranges) if (rg.second - 1 - st >= rg.first) cs.push_back(rg.second - 1 - st);
      if (cs.empty()) break;
      t.steps[i].push_back(cs);
    }
    Y.push_back(y);
    // the border map (border coordinate past the windows -> row of the separator's system) and the pose rows
    const int gn = (nbr - nsep) * NB, m = g->h_sep_off.empty() ? 0 : g->h_sep_off.back();
    std::vector<int>& mp = t.map[i];
    mp.assign(std::max(gn, 1), -1);
    for (size_t c = 0; c < g->h_sep_map.size(); ++c) {
      const int o = g->h_sep_map[c] - nsep * NB;
      if (o >= 0 && o < gn) mp[o] = (int)c < m ? (int)c : Ts * NB + ((int)c - m);
    }
    std::vector<int>& prow = t.prow[i];
    prow.assign(std::max<size_t>(G.P, 1), 0);
    for (int p = 0; p < G.P; ++p)
      prow[p] = (size_t)p < g->h_pose_sep.size() && g->h_pose_sep[p] >= 0 ? T * NB + g->h_pose_sep[p] : 6 * p;
    t.T[i] = T; t.Tc[i] = Tc; t.Trow[i] = Trow; t.gn[i] = gn;
  }
}
// The schedule of the many-right-hand-side solve.  Nodes: a robot's band segments (level 0), its windows (1), its rows of separator
// coordinates (2, no columns); the separator's leaves (3), its top block with the lambda block (4; all of it when the separator is not
// dissected)
void CholBatch::JointTree::solve_plan(SolvePlan& P) const {
  const int n = (int)T.size(), NS = 1 + n;
  std::vector<std::vector<int>> node(NS);
  for (int i = 0; i < n; ++i) {
    node[1 + i].assign(Trow[i], 2000);
    for (size_t q = 0; q < ranges[i].size(); ++q)
      for (int k = ranges[i][q].first; k < ranges[i][q].second; ++k) node[1 + i][k] = (int)q;
    for (int k = T[i]; k < Tc[i]; ++k) node[1 + i][k] = 1000;
  }
  node[0].assign(Tsep, 4000);
  for (int k = 0; k < sTL; ++k) node[0][k] = k < sTa ? 3000 : 3001;
  auto level = [](int nd) { return nd < 1000 ? 0 : nd / 1000; };
  auto ncols = [&](int sy) { return sy == 0 ? Tsep : Tc[sy - 1]; };
  // per system and tile: the forward push rows (same node), backward push columns (same node, transposed), forward pull columns
  // (nodes below), backward pull rows (nodes above)
  std::vector<std::vector<std::vector<int>>> fpush(NS), bpush(NS), fpull(NS), bpull(NS);
  for (int sy = 0; sy < NS; ++sy) {
    const int nt = (int)node[sy].size();
    fpush[sy].assign(nt, {}); bpush[sy].assign(nt, {}); fpull[sy].assign(nt, {}); bpull[sy].assign(nt, {});
    for (int c = 0; c < ncols(sy); ++c) {
      const int b = Y[sy].col0 + c;
      for (int q = rp[b]; q < rp[b + 1]; ++q) {
        const int i = rows[q];
        if (node[sy][i] == node[sy][c]) { fpush[sy][c].push_back(i); bpush[sy][i].push_back(c); }
        else { fpull[sy][i].push_back(c); bpull[sy][c].push_back(i); }
      }
    }
  }
  auto add_job = [&](int sy, int k, const std::vector<int>& l) {
    P.jobs.push_back(make_int4(sy, k, (int)P.lst.size(), (int)(P.lst.size() + l.size())));
    P.lst.insert(P.lst.end(), l.begin(), l.end());
    return (int)l.size();
  };
  // a push launch: the columns cols (system, column) side by side
  auto push = [&](const std::vector<std::pair<int, int>>& cols, bool bwd) {
    if (cols.empty()) return;
    SolvePlan::Launch L{0, bwd, (int)P.jobs.size(), 0, 0};
    for (const auto& sc : cols) L.maxl = std::max(L.maxl, add_job(sc.first, sc.second, (bwd ? bpush : fpush)[sc.first][sc.second]));
    L.nj = (int)P.jobs.size() - L.j0;
    P.launches.push_back(L);
  };
  // a pull launch over the tiles of the given level (forward, a tile with nothing to take is left out; backward, every column starts
  // its right-hand side there: R_k = D_k S_k - ..)
  auto pull = [&](int lev, bool bwd) {
    SolvePlan::Launch L{1, bwd, (int)P.jobs.size(), 0, 0};
    for (int sy = 0; sy < NS; ++sy)
      for (int k = 0; k < (int)node[sy].size(); ++k) {
        if (level(node[sy][k]) != lev || (bwd && k >= ncols(sy))) continue;
        const std::vector<int>& l = (bwd ? bpull : fpull)[sy][k];
        if (l.empty() && !bwd) continue;
        add_job(sy, k, l);
      }
    L.nj = (int)P.jobs.size() - L.j0;
    if (L.nj > 0) P.launches.push_back(L);
  };
  auto robot_band_steps = [&](bool bwd) {
    int nst = 0;
    for (int i = 0; i < n; ++i) for (const auto& rg : ranges[i]) nst = std::max(nst, rg.second - rg.first);
    for (int st = 0; st < nst; ++st) {
      std::vector<std::pair<int, int>> cols;
      for (int i = 0; i < n; ++i)
        for (const auto& rg : ranges[i])
          if (st < rg.second - rg.first) cols.emplace_back(1 + i, bwd ? rg.second - 1 - st : rg.first + st);
      push(cols, bwd);
    }
  };
  auto robot_window_steps = [&](bool bwd) {
    int nst = 0;
    for (int i = 0; i < n; ++i) nst = std::max(nst, Tc[i] - T[i]);
    for (int st = 0; st < nst; ++st) {
      std::vector<std::pair<int, int>> cols;
      for (int i = 0; i < n; ++i)
        if (st < Tc[i] - T[i]) cols.emplace_back(1 + i, bwd ? Tc[i] - 1 - st : T[i] + st);
      push(cols, bwd);
    }
  };
  auto leaf_steps = [&](bool bwd) {
    const int na = sTa, nb = sTL > 0 ? sTL - sTa : 0;
    if (sTL == 0) return;
    for (int st = 0; st < std::max(na, nb); ++st) {
      std::vector<std::pair<int, int>> cols;
      if (st < na) cols.emplace_back(0, bwd ? na - 1 - st : st);
      if (st < nb) cols.emplace_back(0, bwd ? sTL - 1 - st : na + st);
      push(cols, bwd);
    }
  };
  auto top_steps = [&](bool bwd) {
    for (int st = 0; st < Tsep - sTL; ++st) push({{0, bwd ? Tsep - 1 - st : sTL + st}}, bwd);
  };
  robot_band_steps(false);
  pull(1, false); robot_window_steps(false);
  pull(2, false);
  P.launches.push_back({2, 0, 0, 0, 0});
  leaf_steps(false);
  pull(4, false); top_steps(false);
  P.n_fwd = (int)P.launches.size();      // (from here on: the backward half)
  pull(4, true); top_steps(true);
  pull(3, true); leaf_steps(true);
  P.launches.push_back({3, 0, 0, 0, 0});
  pull(1, true); robot_window_steps(true);
  pull(0, true); robot_band_steps(true);
  // the separator's rows from the robots' (the inverse of the border maps, robot order)
  std::vector<std::vector<int2>> inv(Tsep * NB);
  for (int i = 0; i < n; ++i) {
    for (int o = 0; o < gn[i]; ++o)
      if (map[i][o] >= 0) inv[map[i][o]].push_back(make_int2(i, Tc[i] * NB + o));
    P.max_gn = std::max(P.max_gn, gn[i]);
  }
  for (const auto& v : inv) { P.sent.insert(P.sent.end(), v.begin(), v.end()); P.sptr.push_back((int)P.sent.size()); }
}
void CholBatch::job_point_landmarks(std::vector<std::vector<int>>& priv, std::vector<int>& shared_off) const {
  priv.assign(n, {});
  shared_off.clear();
  std::vector<char> seen;
  for (int i = 0; i < n; ++i) {
    const HostGraph* g = graphs[i];
    for (size_t l = 0; l < g->up_L && l < g->h_lm_type.size(); ++l)
      if (g->h_lm_type[l] == VT_POINT && !(l < g->h_lm_bord.size() && g->h_lm_bord[l] >= 0)) priv[i].push_back((int)l);
    seen.resize(std::max(seen.size(), g->h_sh_lid.size()), 0);
    for (size_t k = 0; k < g->h_sh_lid.size(); ++k) {
      const int l = g->h_sh_lid[k];
      if (l < 0 || (size_t)l >= g->up_L || g->h_lm_type[l] != VT_POINT || seen[k]) continue;
      seen[k] = 1;
      shared_off.push_back(g->h_sep_off[k]);
    }
  }
}
// Sigma of the separator system and of every robot's band + border, computed once per exact pass (joint_state first: the buffers hold
// that pass's factor and hG / the graphs' host tables describe it)
int CholBatch::ensure_joint_sigma() {
  if (jsig_serial == exact_serial && jsig_sep) return SLIDE_OK;
  free_joint_sigma();
  const int rc = compute_joint_sigma();
  if (rc == SLIDE_OK) jsig_serial = exact_serial;
  else free_joint_sigma();
  return rc;
}
// (the jsig_* buffers are the batch's as soon as they exist; Z, the row lists and the border maps are scratch of this call)
int CholBatch::compute_joint_sigma() {
  hipStream_t s = master;
  JointTree t;
  joint_tree(t);
  const int Tsep = t.Tsep;
  std::vector<JSinvSys>& Y = t.Y;
  const std::vector<int>& rp = t.rp;
  const std::vector<int>& rows = t.rows;
  const std::vector<std::vector<std::vector<int>>>& steps = t.steps;      // per robot: the columns of each backward step
  Scratch sc(s);
  JSigGather gA{};
  int max_gn = 0;
  jsig_rob.assign(n, nullptr); jsig_prow.assign(n, nullptr); jsig_lds.assign(n, 0);
  for (int i = 0; i < n; ++i) {
    JSinvSys& y = Y[1 + i];
    const int Tc = t.Tc[i], gn = t.gn[i];
    // Sigma, Z; the border map and the pose rows
    const size_t nsg = (size_t)y.lds * y.lds, nz = (size_t)y.lds * Tc * NB;
    jsig_rob[i] = sc.keep(sc.alloc<double>(nsg));
    y.Z = sc.alloc<double>(nz);
    int* d_map = sc.alloc<int>(t.map[i].size());
    jsig_prow[i] = sc.keep(sc.alloc<int>(t.prow[i].size()));
    if (!sc.ok()) return SLIDE_ERR_HIP;
    SL_HIP(hipMemsetAsync(jsig_rob[i], 0, nsg * sizeof(double), s));
    y.Sg = jsig_rob[i];
    jsig_lds[i] = y.lds;
    SL_HIP(sc.upload(d_map, t.map[i]));
    SL_HIP(sc.upload(jsig_prow[i], t.prow[i]));
    gA.dst[i] = jsig_rob[i]; gA.map[i] = d_map; gA.lds[i] = y.lds; gA.o0[i] = Tc * NB; gA.n[i] = gn;
    max_gn = std::max(max_gn, gn);
  }
  // the separator's Sigma and Z
  jsig_lds_sep = (long long)Tsep * NB;
  {
    const size_t nsg = (size_t)jsig_lds_sep * jsig_lds_sep, nz = (size_t)jsig_lds_sep * Tsep * NB;
    jsig_sep = sc.keep(sc.alloc<double>(nsg));
    Y[0].Z = sc.alloc<double>(nz);
    if (!sc.ok()) return SLIDE_ERR_HIP;
    SL_HIP(hipMemsetAsync(jsig_sep, 0, nsg * sizeof(double), s));
    Y[0].Sg = jsig_sep;
  }
  gA.src = jsig_sep; gA.lds_src = jsig_lds_sep;
  // the jobs: the separator's columns one step each (last first), then the robots' steps side by side
  std::vector<int2> jobs;
  std::vector<std::pair<int, int>> step_at;          // (first job, jobs) per step
  std::vector<int> step_rows;
  auto nrows = [&](int sy, int k) { const int b = Y[sy].col0 + k; return rp[b + 1] - rp[b]; };
  for (int k = Tsep - 1; k >= 0; --k) {
    step_at.emplace_back((int)jobs.size(), 1);
    step_rows.push_back(nrows(0, k));
    jobs.push_back(make_int2(0, k));
  }
  const int n_sep_steps = (int)step_at.size();
  size_t nst = 0;
  for (int i = 0; i < n; ++i) nst = std::max(nst, steps[i].size());
  for (size_t st = 0; st < nst; ++st) {
    const int j0 = (int)jobs.size();
    int mr = 0;
    for (int i = 0; i < n; ++i)
      if (st < steps[i].size())
        for (int k : steps[i][st]) { jobs.push_back(make_int2(1 + i, k)); mr = std::max(mr, nrows(1 + i, k)); }
    step_at.emplace_back(j0, (int)jobs.size() - j0);
    step_rows.push_back(mr);
  }
  int max_rows = 0;
  for (int r : step_rows) max_rows = std::max(max_rows, r);
  JSinvSys* d_sys = sc.alloc<JSinvSys>(Y.size());
  int2* d_jobs = sc.alloc<int2>(jobs.size());
  int* d_rp = sc.alloc<int>(rp.size());
  int* d_rows = sc.alloc<int>(rows.size());
  if (!sc.ok()) return SLIDE_ERR_HIP;
  SL_HIP(sc.upload(d_sys, Y));
  SL_HIP(sc.upload(d_jobs, jobs));
  SL_HIP(sc.upload(d_rp, rp));
  SL_HIP(sc.upload(d_rows, rows));
  launch_jsinv_prep(d_sys, d_jobs, (int)jobs.size(), max_rows, d_rp, d_rows, s);
  for (int q = 0; q < (int)step_at.size(); ++q) {
    if (q == n_sep_steps) launch_jsig_gather(gA, n, max_gn, s);      // (the robots' rows of separator coordinates, once it is complete)
    launch_jsinv_step(d_sys, d_jobs + step_at[q].first, step_at[q].second, step_rows[q], d_rp, d_rows, s);
  }
  if ((int)step_at.size() == n_sep_steps) launch_jsig_gather(gA, n, max_gn, s);
  const hipError_t e1 = hipGetLastError(), e2 = hipStreamSynchronize(s);
  return hip_ok(e1, "joint selected inverse") && hip_ok(e2, "joint selected inverse") ? SLIDE_OK : SLIDE_ERR_HIP;
}
// isam->marginalCovariance(X(idx)) on the joint graph (graph.cpp:314-323 on a replica): the poses of the robot of `slot`
int CholBatch::joint_pose_covariances(int slot, const uint64_t* idx, int n_q, double* out36n) {
  if (n_q < 0 || (n_q > 0 && (!idx || !out36n))) return SLIDE_ERR_INVALID;
  for (int i = 0; i < 36 * n_q; ++i) out36n[i] = 0.0;
  std::lock_guard<std::mutex> pl(pass_mtx);
  int rc = joint_state("get_pose_covariances", slot);
  if (rc != SLIDE_OK) return rc;
  HostGraph* g = graphs[slot];
  const int robot = joint_robot(slot);
  std::vector<int> ids(n_q);
  for (int q = 0; q < n_q; ++q)
    if ((ids[q] = g->pose_id(robot, idx[q])) < 0) return SLIDE_MISSING;
  if (n_q == 0) return SLIDE_OK;
  if ((rc = ensure_joint_sigma()) != SLIDE_OK) return rc;
  hipStream_t s = master;
  Scratch sc(s);
  int* d_idx = sc.alloc<int>(n_q);
  double* d_out = sc.alloc<double>(36 * (size_t)n_q);
  if (!sc.ok()) return SLIDE_ERR_HIP;
  SL_HIP(sc.upload(d_idx, ids));
  launch_pose_blocks(jsig_rob[slot], (int)jsig_lds[slot], d_idx, n_q, d_out, s, jsig_prow[slot]);
  SL_HIP(hipGetLastError());
  SL_HIP(hipMemcpyAsync(out36n, d_out, 36 * (size_t)n_q * sizeof(double), hipMemcpyDeviceToHost, s));
  SL_HIP(hipStreamSynchronize(s));
  return SLIDE_OK;
}
// isam->marginalCovariance(L / C / U(idx)) on the joint graph: a private landmark through its robot's pose Sigma (k_lm_cov), a shared one
// straight from the separator's Sigma at its slot's coordinates — every replica reads the same numbers
int CholBatch::joint_landmark_covariances(int slot, int cls, const uint64_t* idx, int n_q, double* out) {
  const int d = landmark_dim(cls);
  if (!d || n_q < 0 || (n_q > 0 && (!idx || !out))) return SLIDE_ERR_INVALID;
  for (int i = 0; i < d * d * n_q; ++i) out[i] = 0.0;
  std::lock_guard<std::mutex> pl(pass_mtx);
  int rc = joint_state("get_landmark_covariances", slot);
  if (rc != SLIDE_OK) return rc;
  HostGraph* g = graphs[slot];
  std::vector<int> priv, pq, row0, dims, sq;
  for (int q = 0; q < n_q; ++q) {
    const int l = g->lm_lid(cls, idx[q]);
    if (l < 0) return SLIDE_MISSING;
    int sl = -1;
    if ((size_t)l < g->h_lm_bord.size() && g->h_lm_bord[l] >= 0)
      for (size_t k = 0; k < g->h_sh_lid.size(); ++k) if (g->h_sh_lid[k] == l) { sl = (int)k; break; }
    if (sl >= 0) { row0.push_back(g->h_sep_off[sl]); dims.push_back(d); sq.push_back(q); }
    else { priv.push_back(l); pq.push_back(q); }
  }
  if (n_q == 0) return SLIDE_OK;
  if ((rc = ensure_joint_sigma()) != SLIDE_OK) return rc;
  hipStream_t s = master;
  const size_t np = priv.size(), ns = row0.size();
  Scratch sc(s);
  int* d_i = sc.alloc<int>(np + 2 * ns + 1);
  double* d_out = sc.alloc<double>(81 * (np + ns));
  if (!sc.ok()) return SLIDE_ERR_HIP;
  SL_HIP(sc.upload(d_i, priv));
  SL_HIP(sc.upload(d_i + np, row0));
  SL_HIP(sc.upload(d_i + np + ns, dims));
  launch_landmark_covariances(hG[slot], jsig_rob[slot], (int)jsig_lds[slot], d_i, (int)np, d_out, s, jsig_prow[slot]);
  launch_sym_blocks(jsig_sep, (size_t)jsig_lds_sep, d_i + np, d_i + np + ns, (int)ns, d_out + 81 * np, s);
  std::vector<double> h(81 * (np + ns));
  SL_HIP(hipGetLastError());
  SL_HIP(hipMemcpyAsync(h.data(), d_out, h.size() * sizeof(double), hipMemcpyDeviceToHost, s));
  SL_HIP(hipStreamSynchronize(s));
  for (size_t k = 0; k < np; ++k) unpack_block(h, k, d, out, pq[k]);
  for (size_t k = 0; k < ns; ++k) unpack_block(h, np + k, d, out, sq[k]);
  return SLIDE_OK;
}
// logEntropy (graph.cpp:423-466) on the joint graph: {the traces of the robot's pose marginals, the traces of the job's point landmarks
// (every graph's private ones, each shared slot once), #poses, #point landmarks}
int CholBatch::joint_marginal_traces(int slot, double* out4) {
  for (int i = 0; i < 4; ++i) out4[i] = 0.0;
  std::lock_guard<std::mutex> pl(pass_mtx);
  int rc = joint_state("marginal_traces", slot);
  if (rc != SLIDE_OK) return rc;
  if ((rc = ensure_joint_sigma()) != SLIDE_OK) return rc;
  hipStream_t s = master;
  std::vector<int> poses;
  graphs[slot]->robot_poses(joint_robot(slot), poses);
  std::vector<std::vector<int>> priv;
  std::vector<int> row0;
  job_point_landmarks(priv, row0);
  const std::vector<int> dims(row0.size(), 3);
  size_t nq = poses.size() + row0.size();
  for (int i = 0; i < n; ++i) nq += priv[i].size();
  Scratch sc(s);
  int* d_i = sc.alloc<int>(nq + row0.size() + 1);
  double* d_out = sc.alloc<double>(81 * nq + 1);
  if (!sc.ok()) return SLIDE_ERR_HIP;
  hipError_t e = hipSuccess;
  size_t o = 0;
  auto up = [&](const std::vector<int>& v) { if (e == hipSuccess) e = sc.upload(d_i + o, v); o += v.size(); };
  const size_t o_pose = o; up(poses);
  std::vector<size_t> o_priv(n);
  for (int i = 0; i < n; ++i) { o_priv[i] = o; up(priv[i]); }
  const size_t o_sh = o; up(row0); up(dims);
  SL_HIP(e);
  launch_pose_blocks(jsig_rob[slot], (int)jsig_lds[slot], d_i + o_pose, (int)poses.size(), d_out, s, jsig_prow[slot]);
  for (int i = 0; i < n; ++i)
    launch_landmark_covariances(hG[i], jsig_rob[i], (int)jsig_lds[i], d_i + o_priv[i], (int)priv[i].size(), d_out + 81 * o_priv[i], s, jsig_prow[i]);
  launch_sym_blocks(jsig_sep, (size_t)jsig_lds_sep, d_i + o_sh, d_i + o_sh + row0.size(), (int)row0.size(), d_out + 81 * o_sh, s);
  std::vector<double> h(81 * nq);
  SL_HIP(hipGetLastError());
  if (!h.empty()) SL_HIP(hipMemcpyAsync(h.data(), d_out, h.size() * sizeof(double), hipMemcpyDeviceToHost, s));
  SL_HIP(hipStreamSynchronize(s));
  for (size_t p = 0; p < poses.size(); ++p)      // (pose blocks: 36 per pose, packed from the front of d_out)
    for (int a = 0; a < 6; ++a) out4[0] += h[36 * p + 7 * a];
  for (size_t q = o_priv.empty() ? o_sh : o_priv[0]; q < o_sh + row0.size(); ++q)
    for (int a = 0; a < 3; ++a) out4[1] += h[81 * q + 4 * a];
  out4[2] = (double)poses.size();
  out4[3] = (double)(o_sh + row0.size() - poses.size());
  return SLIDE_OK;
}

// estimateClosureInfoGain (graph.cpp:469-623) on the joint graph (graph.cpp:325-371: every replica holds the whole multi-robot graph),
// in the linear-Gaussian model of the last exact pass's factor K = L D L^T, as the single-graph call: U = K^-1 J^T by substitutions with
// 6m right-hand sides through the pass's elimination tree (joint_cov_kernels.hip's k_jms_*), C = I + J U, the drops tr(C^-1 U_P^T U_P).
// A candidate's endpoints may sit in different robots' graphs (a rendezvous); J is taken at the graphs' pose_val, the pass's
// linearisation point.  Every system's U lives in one buffer (robots first, then the separator; leading dimension N), so the grams run
// over row lists of it.  Nothing the pass reads is written and the cached joint Sigma is left as it was.
int CholBatch::joint_closure_info_gain(int slot, const int32_t* traj_slots, const uint64_t* traj, int n_q, const double* travel,
                                       const double* sigma6, double* out4) {
  for (int i = 0; i < 4; ++i) out4[i] = 0.0;
  int rc = gain_check_steps(traj, n_q, travel);
  if (rc != SLIDE_OK) return rc;
  std::lock_guard<std::mutex> pl(pass_mtx);
  if ((rc = joint_state("closure_info_gain", slot)) != SLIDE_OK) return rc;
  if (!sigma6) sigma6 = graphs[slot]->P.noise_model_odom_vec;
  if ((rc = gain_check_sigma(sigma6)) != SLIDE_OK) return rc;
  std::vector<int> qs(n_q), ids(n_q);
  for (int k = 0; k < n_q; ++k) {
    qs[k] = traj_slots ? traj_slots[k] : slot;
    if (qs[k] < 0 || qs[k] >= n) { g_last_error = "closure_info_gain: no such slot in traj_slots"; return SLIDE_ERR_INVALID; }
    if ((ids[k] = graphs[qs[k]]->pose_id(joint_robot(qs[k]), traj[k])) < 0) return SLIDE_MISSING;
  }
  hipStream_t s = master;
  JointGain jg;
  jg.build(*this, slot);
  const size_t N = jg.N;
  GainQuery q(n_q);
  for (int k = 0; k < n_q; ++k) {
    q.row[k] = jg.prow_of(qs[k], ids[k]);
    q.val_src[k] = hG[qs[k]].pose_val + 12 * (size_t)ids[k];
  }
  if ((rc = gain_jt(q, travel, sigma6, s)) != SLIDE_OK) return rc;
  const int ncol = q.ncol, ne = (int)q.vv.size();
  const size_t nn = (size_t)ncol * ncol;
  Scratch sc(s);
  double* X = sc.alloc<double>(N * ncol);
  double* Rb = sc.alloc<double>(N * ncol);
  double* V = sc.alloc<double>(jg.ldv * ncol);
  double* Md = sc.alloc<double>(4 * nn);
  double* d_val = sc.alloc<double>(ne);
  int* d_rc = nullptr;
  rc = jg.upload(sc, X, Rb, ne, &d_rc);
  if (!sc.ok()) { g_last_error = "closure_info_gain: out of device memory"; return SLIDE_ERR_HIP; }
  if (rc != SLIDE_OK) return rc;
  SL_HIP(hipMemsetAsync(X, 0, N * ncol * sizeof(double), s));
  SL_HIP(hipMemsetAsync(Rb, 0, N * ncol * sizeof(double), s));
  SL_HIP(sc.upload(d_rc, q.rcv));
  SL_HIP(sc.upload(d_val, q.vv));
  // R = J^T, then X = K^-1 R in S
  launch_scatter(d_rc, d_val, ne, Rb, (int)N, s);
  jg.solve(X, Rb, ncol, s);
  // the grams: poses of `slot`, poses of every robot, private point landmarks (through V), shared point landmarks
  launch_gram(X, N, ncol, jg.d_rslot, (int)jg.rows_slot.size(), Md, s);
  launch_gram(X, N, ncol, jg.d_rall, (int)jg.rows_all.size(), Md + nn, s);
  jg.landmark_V(*this, X, ncol, V, s);
  launch_gram(V, jg.ldv, ncol, nullptr, (int)(9 * jg.nl), Md + 2 * nn, s);
  launch_gram(X, N, ncol, jg.d_rsh, (int)jg.rows_sh.size(), Md + 3 * nn, s);
  double gs[4];
  GainFetched& h = ig_host;
  if ((rc = gain_fetch(q, X, N, Md, 4, s, h)) != SLIDE_OK) return rc;
  sc.release();      // (the query's largest buffers: gone before the host's share, the longest part of a query at m = 64)
  if ((rc = gain_drops(q, h, 4, gs)) != SLIDE_OK) return rc;
  out4[1] = gs[0];
  out4[2] = gs[2] + gs[3];
  out4[0] = 10.0 * out4[1] + out4[2];
  out4[3] = gs[1];
  return SLIDE_OK;
}
// The same for a list (the single-graph closure_info_gain_batch's arguments; traj_slots runs parallel to traj): out4n[4 k ..] what the
// call above gives for candidate k alone, status[k] its own fault (or null).  Whole-call refusals as above, nothing written then.
int CholBatch::joint_closure_info_gain_batch(int slot, int n_cand, const int32_t* off, const int32_t* traj_slots, const uint64_t* traj,
                                             const double* travel, const double* sigma6, double* out4n, int32_t* status) {
  int rc = gain_check_list(n_cand, off, traj, travel, out4n);
  if (rc != SLIDE_OK) return rc;
  std::lock_guard<std::mutex> pl(pass_mtx);
  if ((rc = joint_state("closure_info_gain", slot)) != SLIDE_OK) return rc;
  if (!sigma6) sigma6 = graphs[slot]->P.noise_model_odom_vec;
  if ((rc = gain_check_sigma(sigma6)) != SLIDE_OK) return rc;
  hipStream_t s = master;
  JointGain jg;
  jg.build(*this, slot);
  const size_t N = jg.N;
  std::vector<std::vector<double>> pv(n);            // the linearisation values of a graph's poses, in one copy, once a candidate names it
  std::vector<GainCand> cands(n_cand);
  for (int k = 0; k < n_cand; ++k) {
    GainCand& c = cands[k];
    const int nk = off[k + 1] - off[k];
    c.travel = travel + off[k];
    if (gain_steps_fault(traj + off[k], nk, c.travel, &c.st)) continue;
    for (int i = 0; i < nk; ++i) {
      const int sl = traj_slots ? traj_slots[off[k] + i] : slot;
      if (sl < 0 || sl >= n) { c.st = SLIDE_ERR_INVALID; break; }
      const int id = graphs[sl]->pose_id(joint_robot(sl), traj[off[k] + i]);
      if (id < 0) { c.st = SLIDE_MISSING; break; }
      if (pv[sl].empty()) {
        pv[sl].resize(12 * (size_t)hG[sl].P);
        SL_HIP(hipMemcpyAsync(pv[sl].data(), hG[sl].pose_val, pv[sl].size() * sizeof(double), hipMemcpyDeviceToHost, s));
        SL_HIP(hipStreamSynchronize(s));
      }
      c.row.push_back(jg.prow_of(sl, id));
      c.val.insert(c.val.end(), pv[sl].begin() + 12 * (size_t)id, pv[sl].begin() + 12 * (size_t)id + 12);
    }
  }
  double* V = nullptr;
  GainBackend be;
  be.s = s; be.ldu = N; be.nM = 4;
  be.alloc = [&](Scratch& sc, int max_ncol) -> int {
    be.U = sc.alloc<double>(N * max_ncol);
    be.R = sc.alloc<double>(N * max_ncol);
    V = sc.alloc<double>(jg.ldv * max_ncol);
    const int rc_up = jg.upload(sc, be.U, be.R);
    if (!sc.ok()) { g_last_error = "closure_info_gain_batch: out of device memory"; return SLIDE_ERR_HIP; }
    return rc_up;
  };
  be.begin = [&](int ncol) -> int {
    SL_HIP(hipMemsetAsync(be.U, 0, N * ncol * sizeof(double), s));
    SL_HIP(hipMemsetAsync(be.R, 0, N * ncol * sizeof(double), s));
    return SLIDE_OK;
  };
  be.solve = [&](int ncol) -> int { jg.solve(be.U, be.R, ncol, s); return SLIDE_OK; };
  // the grams as the single call's: poses of `slot`, poses of every robot, private point landmarks (through V), shared point landmarks
  be.grams = [&](int ncol, const GainBackend::Gram& gram) {
    gram(0, be.U, N, jg.d_rslot, (int)jg.rows_slot.size());
    gram(1, be.U, N, jg.d_rall, (int)jg.rows_all.size());
    jg.landmark_V(*this, be.U, ncol, V, s);
    gram(2, V, jg.ldv, nullptr, (int)(9 * jg.nl));
    gram(3, be.U, N, jg.d_rsh, (int)jg.rows_sh.size());
  };
  std::vector<double> g(GAIN_MAX_GRAMS * (size_t)n_cand);
  if ((rc = gain_batch(be, cands, sigma6, g.data())) != SLIDE_OK) return rc;
  for (int k = 0; k < n_cand; ++k) {
    const double* gs = g.data() + GAIN_MAX_GRAMS * (size_t)k;
    double* o = out4n + 4 * (size_t)k;
    for (int i = 0; i < 4; ++i) o[i] = 0.0;
    if (cands[k].st == SLIDE_OK) {
      o[1] = gs[0];
      o[2] = gs[2] + gs[3];
      o[0] = 10.0 * o[1] + o[2];
      o[3] = gs[1];
    }
    if (status) status[k] = cands[k].st;
  }
  return SLIDE_OK;
}
}  // namespace sl
