// Marginal covariances and loop-closure information gain, on one graph and on the exact joint multi-robot graph: the host side of
// cov_kernels.hip and joint_cov_kernels.hip (the classes are declared in host_graph.hpp).
#include "host_graph.hpp"

#include <algorithm>
#include <cmath>
#include <functional>
#include <map>
#include <unordered_map>

namespace sl {

// Device scratch of one query.  Every buffer a query allocates for itself comes from here and is freed when the query returns, on
// whatever path, behind the work still queued on its stream.
class Scratch {
 public:
  explicit Scratch(hipStream_t s) : s(s) {}
  Scratch(const Scratch&) = delete;
  Scratch& operator=(const Scratch&) = delete;
  ~Scratch() { release(); }
  void release() {
    if (bufs.empty()) return;
    (void)hipStreamSynchronize(s);
    for (void* p : bufs) (void)hipFree(p);
    bufs.clear();
  }
  // n elements (never null for n = 0); null once an allocation has failed: ask ok() after the last one
  template <class T>
  T* alloc(size_t n) {
    void* p = nullptr;
    if (failed || !hip_ok(hipMalloc(&p, std::max<size_t>(n * sizeof(T), 8)), "hipMalloc (query scratch)")) {
      (void)hipGetLastError();
      failed = true;
      return nullptr;
    }
    bufs.push_back(p);
    return static_cast<T*>(p);
  }
  bool ok() const { return !failed; }
  // a buffer that outlives the query (a cached result): its owner is the caller from here on
  template <class T>
  T* keep(T* p) {
    bufs.erase(std::remove(bufs.begin(), bufs.end(), static_cast<void*>(p)), bufs.end());
    return p;
  }
  // host -> device on the query's stream
  template <class T>
  hipError_t upload(T* dst, const std::vector<T>& v) const {
    return v.empty() ? hipSuccess : hipMemcpyAsync(dst, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, s);
  }

 private:
  hipStream_t s;
  std::vector<void*> bufs;
  bool failed = false;
};

// tangent dimension of a landmark class (its covariance is d x d), 0: no such class
static int landmark_dim(int cls) { return cls == SLIDE_CLS_CYLINDER ? 7 : cls == SLIDE_CLS_CUBE ? 9 : cls == SLIDE_CLS_ELLIPSOID ? 3 : 0; }
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
    const int nt = (nk + 15) / 16;
    for (int ta = 0; ta < nt; ++ta)
      for (int tb = 0; tb < nt; ++tb)
        for (int sp = 0; sp < cd.nsplit; ++sp) w.jobs.push_back(make_int4((int)w.ids.size(), ta, tb, sp));
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

// ---- quadratic forms B^T Sigma B of many candidates: the joint marginal of pose pairs and the closure gate -----------------------------
// With S = L L^T the resident reduced pose system and Sigma = S^-1, B^T Sigma B = W^T W where L W = B: a forward substitution and a
// gram, no backward pass — half the launch chain of launch_multi_solve — and symmetric positive semi-definite by construction.  The
// ncand candidates own nk columns of B each and are cut into sweeps of whole candidates of at most SLIDE_INFO_GAIN_SWEEP_COLS
// columns.  Per sweep: B zeroed, fill() queues the kernel that writes the candidates' columns, ONE launch_multi_fwd, the candidates'
// nk x nk diagonal blocks of W^T W over all rows (k_gram_blocks + k_gram_reduce; nsplit from nk alone), then done() queues what
// follows and reads back (M: nk x nk per candidate of the sweep, on the device).  As in gain_batch, a candidate's bits do not depend
// on what else is in the list or where it stands: the substitution treats every column by itself.  (marginal_state first.)
// One driver serves this and the joint graph of a CholBatch (joint_sigma_forms) through a back end, as gain_batch does.
//
// What differs between one graph and the joint graph of a batch.  alloc: B and W (ld rows by the widest sweep's columns) and the back
// end's own tables, from the query's scratch.  A sweep: B zeroed and filled by the driver, fwd (W = L^-1 B; B may be overwritten), then
// the grams over the row list `rows` (null: 0 .. nrows - 1) and, where the factor has rows with D = -I, over rows_neg, subtracted.
struct FormBackend {
  hipStream_t s = nullptr;
  size_t ld = 0;
  double *B = nullptr, *W = nullptr;
  const int *rows = nullptr, *rows_neg = nullptr;
  int nrows = 0, nrows_neg = 0;
  std::function<int(Scratch& sc, int max_ncol)> alloc;
  std::function<void(int ncol)> fwd;
  // the short walk (single graph, optional): start(k0, nc) = the first block column whose rows of B the sweep's candidates touch; the
  // driver zeroes the rows of W above it and fwd walks from kb on.  The gram keeps its row range and split, so the bits are those of
  // the walk from column 0.
  FormStart start;
  int kb = 0;
};
static int sigma_forms_core(const char* who, FormBackend& be, int ncand, int nk, const FormFill& fill, const FormDone& done) {
  hipStream_t s = be.s;
  const int per = SLIDE_INFO_GAIN_SWEEP_COLS / nk, max_nc = std::min(ncand, per);
  const int nsplit = gain_gram_splits(nk), nt = (nk + 15) / 16, jobs_per = nt * nt * nsplit;
  const size_t nn = (size_t)nk * nk;
  std::vector<GainCandDev> cd(max_nc);
  std::vector<int4> jobs;
  for (int i = 0; i < max_nc; ++i) {
    cd[i] = GainCandDev{nk * i, nk, nsplit, 0, (long long)(nn * i), (long long)(nn * nsplit * i), 0};
    for (int ta = 0; ta < nt; ++ta)
      for (int tb = 0; tb < nt; ++tb)
        for (int sp = 0; sp < nsplit; ++sp) jobs.push_back(make_int4(i, ta, tb, sp));
  }
  Scratch sc(s);
  int rc = be.alloc(sc, max_nc * nk);
  double* d_M = sc.alloc<double>(nn * max_nc);
  double* d_Mneg = sc.alloc<double>(be.nrows_neg > 0 ? nn * max_nc : 0);
  double* d_part = sc.alloc<double>(nn * nsplit * max_nc);
  GainCandDev* d_cd = sc.alloc<GainCandDev>(max_nc);
  int4* d_jobs = sc.alloc<int4>(jobs.size());
  if (!sc.ok()) { g_last_error = std::string(who) + ": out of device memory"; return SLIDE_ERR_HIP; }
  if (rc != SLIDE_OK) return rc;
  SL_HIP(sc.upload(d_cd, cd));
  SL_HIP(sc.upload(d_jobs, jobs));
  for (int k0 = 0; k0 < ncand; k0 += per) {
    const int nc = std::min(per, ncand - k0), ncol = nc * nk;
    SL_HIP(hipMemsetAsync(be.B, 0, (size_t)ncol * be.ld * sizeof(double), s));
    fill(k0, nc, be.B, (int)be.ld);
    be.kb = be.start ? std::max(0, be.start(k0, nc)) : 0;
    if (be.kb > 0) SL_HIP(hipMemset2DAsync(be.W, be.ld * sizeof(double), 0, (size_t)be.kb * NB * sizeof(double), (size_t)ncol, s));
    be.fwd(ncol);
    launch_gram_blocks(be.W, be.ld, be.rows, be.nrows, d_cd, nc, d_jobs, nc * jobs_per, d_part, d_M, s);
    if (be.nrows_neg > 0) {
      launch_gram_blocks(be.W, be.ld, be.rows_neg, be.nrows_neg, d_cd, nc, d_jobs, nc * jobs_per, d_part, d_Mneg, s);
      launch_gram_sub(d_M, d_Mneg, nn * nc, s);
    }
    SL_HIP(hipGetLastError());
    rc = done(k0, nc, d_M);
    if (rc != SLIDE_OK) return rc;
  }
  return SLIDE_OK;
}
// (one graph's back end: B and W of nT rows, the forward half of the resident factor's substitution from block column kb on)
void HostGraph::form_backend(FormBackend& be, const FormStart& start) {
  hipStream_t s = stream;
  const int T = G.T, nT = T * NB;
  const bool dense = h_prof.size() != (size_t)T;
  be.s = s; be.ld = nT; be.nrows = nT;
  be.alloc = [&be, nT](Scratch& sc, int max_ncol) -> int {
    be.B = sc.alloc<double>((size_t)max_ncol * nT);
    be.W = sc.alloc<double>((size_t)max_ncol * nT);
    return SLIDE_OK;
  };
  be.start = start;
  be.fwd = [this, &be, T, dense, s](int ncol) {
    launch_multi_fwd(G.S, G.ld, T, G.Ld, G.Winv, dense ? nullptr : h_prof.data(), be.B, be.W, ncol, s, std::min(be.kb, T - 1));
  };
}
int HostGraph::sigma_forms(const char* who, int ncand, int nk, const FormFill& fill, const FormDone& done, const FormStart& start) {
  FormBackend be;
  form_backend(be, start);
  return sigma_forms_core(who, be, ncand, nk, fill, done);
}
// sigma_forms_core's sibling for GROUPS of unequal width whose whole gram is wanted (the joint-compatibility test): a sweep is a list
// of groups packed by the caller, group g of it one "candidate" of launch_gram_blocks — cd[g] = {first column, columns, splits, .,
// moff, poff, .} — with a job table of its own over (group, tile row >= tile column, split): only the lower 16 x 16 tiles of a
// group's nk x nk gram are formed (k_gram_reduce adds the splits of every entry; the upper tiles' sums are of partials nobody wrote
// and nobody reads).  The split count depends on the group's columns alone, so a group's bits do not depend on its neighbours.  Per
// sweep: B zeroed, fill(si), the walk from start(si, groups) on, the gram's two launches, done(si, the table on the device, M).
// Where the factor has rows with D = -I (the joint graph of a batch with lambda rows) the gram is SIGNED as sigma_forms_core signs it:
// the same job table over rows_neg into Mneg, then k_gram_sub over the sweep's whole M — the never-written upper tiles hold sums of
// partials nobody wrote in M and Mneg alike, and their difference is read by nobody; a variant restricted to the lower tiles would
// save a few kilobytes of traffic in a launch that is bound by its latency.  The subtraction is entry by entry, so a group's bits
// still depend on its own columns and the row lists alone.  A back end without such rows queues exactly the launches above.
struct FormGroups { int ncol = 0; std::vector<GainCandDev> cd; std::vector<int4> jobs; size_t msz = 0, psz = 0; };
using GroupFill = std::function<int(int si, double* B, int ld)>;
using GroupDone = std::function<int(int si, const GainCandDev* d_cd, const double* M)>;
static int sigma_forms_groups_core(const char* who, FormBackend& be, const std::vector<const FormGroups*>& sweeps, const GroupFill& fill,
                                   const GroupDone& done) {
  hipStream_t s = be.s;
  int max_ncol = 0;
  size_t max_m = 0, max_p = 0, max_g = 0, max_j = 0;
  for (const FormGroups* w : sweeps) {
    max_ncol = std::max(max_ncol, w->ncol);
    max_m = std::max(max_m, w->msz); max_p = std::max(max_p, w->psz);
    max_g = std::max(max_g, w->cd.size()); max_j = std::max(max_j, w->jobs.size());
  }
  Scratch sc(s);
  int rc = be.alloc(sc, max_ncol);
  double* d_M = sc.alloc<double>(max_m);
  double* d_Mneg = sc.alloc<double>(be.nrows_neg > 0 ? max_m : 0);
  double* d_part = sc.alloc<double>(max_p);
  GainCandDev* d_cd = sc.alloc<GainCandDev>(max_g);
  int4* d_jobs = sc.alloc<int4>(max_j);
  if (!sc.ok()) { g_last_error = std::string(who) + ": out of device memory"; return SLIDE_ERR_HIP; }
  if (rc != SLIDE_OK) return rc;
  for (int si = 0; si < (int)sweeps.size(); ++si) {
    const FormGroups& w = *sweeps[si];
    const int ng = (int)w.cd.size();
    SL_HIP(sc.upload(d_cd, w.cd));
    SL_HIP(sc.upload(d_jobs, w.jobs));
    SL_HIP(hipMemsetAsync(be.B, 0, (size_t)w.ncol * be.ld * sizeof(double), s));
    if ((rc = fill(si, be.B, (int)be.ld)) != SLIDE_OK) return rc;
    be.kb = be.start ? std::max(0, be.start(si, ng)) : 0;
    if (be.kb > 0) SL_HIP(hipMemset2DAsync(be.W, be.ld * sizeof(double), 0, (size_t)be.kb * NB * sizeof(double), (size_t)w.ncol, s));
    be.fwd(w.ncol);
    launch_gram_blocks(be.W, be.ld, be.rows, be.nrows, d_cd, ng, d_jobs, (int)w.jobs.size(), d_part, d_M, s);
    if (be.nrows_neg > 0) {
      launch_gram_blocks(be.W, be.ld, be.rows_neg, be.nrows_neg, d_cd, ng, d_jobs, (int)w.jobs.size(), d_part, d_Mneg, s);
      launch_gram_sub(d_M, d_Mneg, w.msz, s);
    }
    SL_HIP(hipGetLastError());
    if ((rc = done(si, d_cd, d_M)) != SLIDE_OK) return rc;
  }
  return SLIDE_OK;
}
// Marginals::jointMarginalCovariance of n pose pairs: out144n[144 k ..] the 12 x 12 row-major block [[Saa, Sab], [Sba, Sbb]] of pair k
// (pose a's six coordinates, then b's; tangent order [rot, trans]).  B: the unit columns of the two poses' rows, so W^T W is the block
// itself.  status[k] (or null): SLIDE_MISSING for a pose the graph does not hold, SLIDE_ERR_INVALID when a and b are one pose; zeros
// then.  Whole-call refusals as pose_covariances, nothing written.  The arguments were checked by the caller (capi.hip).
int HostGraph::pose_pair_covariances(int n, const int32_t* robot_a, const uint64_t* idx_a, const int32_t* robot_b, const uint64_t* idx_b,
                                     double* out144n, int32_t* status) {
  int rc = marginal_state("get_pose_pair_covariances");
  if (rc != SLIDE_OK) return rc;
  std::vector<int32_t> as, bs;
  std::vector<int> ids;
  for (int k = 0; k < n; ++k) {
    for (int e = 0; e < 144; ++e) out144n[144 * (size_t)k + e] = 0.0;
    const int a = pose_id(robot_a[k], idx_a[k]), b = pose_id(robot_b[k], idx_b[k]);
    const int st = a < 0 || b < 0 ? SLIDE_MISSING : a == b ? SLIDE_ERR_INVALID : SLIDE_OK;
    if (status) status[k] = st;
    if (st != SLIDE_OK) continue;
    as.push_back(a); bs.push_back(b); ids.push_back(k);
  }
  if (ids.empty()) return SLIDE_OK;
  hipStream_t s = stream;
  Scratch sc(s);
  int32_t* d_as = sc.alloc<int32_t>(as.size());
  int32_t* d_bs = sc.alloc<int32_t>(bs.size());
  if (!sc.ok()) { g_last_error = "get_pose_pair_covariances: out of device memory"; return SLIDE_ERR_HIP; }
  SL_HIP(sc.upload(d_as, as));
  SL_HIP(sc.upload(d_bs, bs));
  std::vector<double> h;
  return sigma_forms(
      "get_pose_pair_covariances", (int)ids.size(), 12,
      [&](int k0, int nc, double* B, int nT) { launch_pair_identity(d_as + k0, d_bs + k0, nc, nullptr, B, nT, s); },
      [&](int k0, int nc, const double* M) -> int {
        h.resize(144 * (size_t)nc);
        SL_HIP(hipMemcpyAsync(h.data(), M, h.size() * sizeof(double), hipMemcpyDeviceToHost, s));
        SL_HIP(hipStreamSynchronize(s));
        for (int i = 0; i < nc; ++i) std::copy(h.begin() + 144 * (size_t)i, h.begin() + 144 * (size_t)(i + 1), out144n + 144 * (size_t)ids[k0 + i]);
        return SLIDE_OK;
      });
}
// The individual-compatibility test of L closures against the resident factor: closure k is the Between factor
// add_loop_closure(rel7_k, from, to) with sigmas sigma6_k would add, r_k / A_k its whitened residual and Jacobian at the current
// estimate of its two poses (k_closure_gate_lin: the solver's own Between text under the graph's chart), C_k = I + A_k Sigma A_k^T the
// innovation covariance in whitened units (B = A_k^T in sigma_forms), d2_k = r_k^T C_k^-1 r_k (k_closure_gate_finish): chi-square
// with 6 degrees of freedom for a true closure not yet added.  No threshold is applied here.  C36 / r6 / status may be null.
// status[k]: SLIDE_MISSING (a pose the graph does not hold), SLIDE_ERR_INVALID (from and to are one pose), SLIDE_ERR_NOT_SPD (C_k);
// zeros in its outputs then.  Per sweep of 64 closures: one linearisation launch, T substitution launches, two gram launches, one
// finish launch, one read-back.  Whole-call refusals as pose_covariances, nothing written.  Arguments checked by the caller.
int HostGraph::closure_mahalanobis(int L, const int32_t* from_robot, const uint64_t* from_idx, const int32_t* to_robot, const uint64_t* to_idx,
                                   const double* rel7, const double* sigma6, double* d2, double* C36, double* r6, int32_t* status) {
  int rc = marginal_state("closure_mahalanobis");
  if (rc != SLIDE_OK) return rc;
  std::vector<int32_t> fs, ts;
  std::vector<double> z, sg;
  std::vector<int> ids;
  for (int k = 0; k < L; ++k) {
    d2[k] = 0.0;
    for (int e = 0; C36 && e < 36; ++e) C36[36 * (size_t)k + e] = 0.0;
    for (int e = 0; r6 && e < 6; ++e) r6[6 * (size_t)k + e] = 0.0;
    const int a = pose_id(from_robot[k], from_idx[k]), b = pose_id(to_robot[k], to_idx[k]);
    const int st = a < 0 || b < 0 ? SLIDE_MISSING : a == b ? SLIDE_ERR_INVALID : SLIDE_OK;
    if (status) status[k] = st;
    if (st != SLIDE_OK) continue;
    double z12[12];
    to12(from7(rel7 + 7 * (size_t)k), z12);
    fs.push_back(a); ts.push_back(b); ids.push_back(k);
    z.insert(z.end(), z12, z12 + 12);
    sg.insert(sg.end(), sigma6 + 6 * (size_t)k, sigma6 + 6 * (size_t)k + 6);
  }
  if (ids.empty()) return SLIDE_OK;
  hipStream_t s = stream;
  const int m = (int)ids.size(), max_nc = std::min(m, SLIDE_INFO_GAIN_SWEEP_COLS / 6);
  Scratch sc(s);
  int32_t* d_fs = sc.alloc<int32_t>(m);
  int32_t* d_ts = sc.alloc<int32_t>(m);
  double* d_z = sc.alloc<double>(12 * (size_t)m);
  double* d_sg = sc.alloc<double>(6 * (size_t)m);
  double* d_r = sc.alloc<double>(6 * (size_t)m);
  double* d_out = sc.alloc<double>(GATE_OUT * (size_t)max_nc);
  int* d_flag = sc.alloc<int>(max_nc);
  if (!sc.ok()) { g_last_error = "closure_mahalanobis: out of device memory"; return SLIDE_ERR_HIP; }
  SL_HIP(sc.upload(d_fs, fs));
  SL_HIP(sc.upload(d_ts, ts));
  SL_HIP(sc.upload(d_z, z));
  SL_HIP(sc.upload(d_sg, sg));
  std::vector<double> h(GATE_OUT * (size_t)max_nc);
  std::vector<int> hflag(max_nc);
  return sigma_forms(
      "closure_mahalanobis", m, 6,
      [&](int k0, int nc, double* B, int nT) {
        launch_closure_gate_lin(d_pose_est.d, d_fs + k0, d_ts + k0, d_z + 12 * (size_t)k0, d_sg + 6 * (size_t)k0, nc, G.chart, nullptr, B, nT,
                                d_r + 6 * (size_t)k0, s);
      },
      [&](int k0, int nc, const double* M) -> int {
        launch_closure_gate_finish(M, d_r + 6 * (size_t)k0, nc, d_out, d_flag, s);
        SL_HIP(hipGetLastError());
        SL_HIP(hipMemcpyAsync(h.data(), d_out, GATE_OUT * (size_t)nc * sizeof(double), hipMemcpyDeviceToHost, s));
        SL_HIP(hipMemcpyAsync(hflag.data(), d_flag, nc * sizeof(int), hipMemcpyDeviceToHost, s));
        SL_HIP(hipStreamSynchronize(s));
        for (int i = 0; i < nc; ++i) {
          const size_t k = (size_t)ids[k0 + i];
          if (hflag[i]) {
            if (status) status[k] = SLIDE_ERR_NOT_SPD;
            continue;
          }
          const double* o = h.data() + GATE_OUT * (size_t)i;
          d2[k] = o[0];
          if (C36) std::copy(o + 1, o + 37, C36 + 36 * k);
          if (r6) std::copy(o + 37, o + 43, r6 + 6 * k);
        }
        return SLIDE_OK;
      });
}
// What the observation gates resolve of a candidate before the device is asked: its pose and landmark ids (SLIDE_MISSING for a pose
// or landmark the graph does not hold, or a landmark without a factor), its class's factor type, and z and the sigmas by the add
// calls' own text (br_meas / cube_meas / cyl_meas; bearing_range_sigma, noise_model_cube_vec x max(|loc.t|, 0.1), cylinder_sigma).
HostGraph::ObsCand HostGraph::obs_candidate(int robot, uint64_t pose_idx, int cls, uint64_t lm_idx, const double* a) const {
  ObsCand c;
  c.type = cls == SLIDE_CLS_ELLIPSOID ? FT_BR : cls == SLIDE_CLS_CUBE ? FT_CUBE : FT_CYL;
  c.p = pose_id(robot, pose_idx);
  c.l = lm_lid(cls, lm_idx);
  c.st = c.p < 0 || c.l < 0 || lm_fids[c.l].empty() ? SLIDE_MISSING : SLIDE_OK;
  if (c.st != SLIDE_OK) return c;
  if (c.type == FT_BR) {
    br_meas(a, a[3], c.z);
    for (int i = 0; i < 3; ++i) c.sg[i] = P.bearing_range_sigma;
  } else if (c.type == FT_CUBE) {
    cube_meas(from7(a), from7(a + 7), a + 14, c.z, c.sg);
  } else {
    cyl_meas(from7(a), a + 7, a + 10, a[13], c.z);
    for (int i = 0; i < 7; ++i) c.sg[i] = P.cylinder_sigma;
  }
  return c;
}
// The block column at which a sweep of n such candidates starts its forward substitution: that of the lowest pose it touches, the
// candidates' poses and their landmarks' first observers.  (SLIDE_OBS_GATE_FULL_WALK=1, a measurement aid: column 0.)
int HostGraph::obs_walk_start(const int32_t* pid, const int32_t* lid, int n) const {
  const char* fw = std::getenv("SLIDE_OBS_GATE_FULL_WALK");
  if (fw && fw[0] == '1') return 0;
  int lo = 1 << 30;
  for (int i = 0; i < n; ++i) lo = std::min(lo, std::min((int)pid[i], h_lm_first[lid[i]]));
  return std::min((6 * lo) / NB, G.T - 1);
}
// The individual-compatibility test of n candidate landmark observations against the resident factor — the closure gate's counterpart
// for the factors that make up most of a graph (obs_gate_kernels.hip has the invariant).  Candidate k is the factor
// add_range_bearing / add_cube / add_cylinder would add between pose (robot, pose_idx) and the EXISTING landmark (cls, lm_idx): z and
// the sigmas by the add calls' own text (br_meas / cube_meas / cyl_meas; bearing_range_sigma, noise_model_cube_vec x max(|loc.t|, 0.1),
// cylinder_sigma), r and A = [Ap | Al] at the current estimate by k_obs_gate_lin, no robust weight.  C = I + Al H_ll^-1 Al^T + W^T W
// with L W = B, d2 = r^T C^-1 r (k_obs_gate_finish): chi-square with dof = 3 / 9 / 7 for a true match not yet added; no threshold is
// applied.  The candidates are grouped by class and run through sigma_forms with nk = 3, 9, 7 (128, 42, 54 candidates per sweep);
// results go back in the caller's order.  A sweep starts its forward substitution at the block column of the lowest pose it touches
// (the candidates' poses and their landmarks' first observers): a frame's detections sit at the newest pose and see recent landmarks.
// Per sweep: one linearise-and-fill launch, T - k0 substitution launches, two gram launches, one finish launch, one read-back.
// status[k]: SLIDE_MISSING (a pose or landmark the graph does not hold), SLIDE_ERR_NOT_SPD (C_k); zeros in its outputs then.
// Whole-call refusals as pose_covariances, nothing written.  Arguments checked by the caller.
int HostGraph::observation_mahalanobis(int n, const int32_t* robot, const uint64_t* pose_idx, const int32_t* cls, const uint64_t* lm_idx,
                                       const double* meas17, double* d2, int32_t* dof, double* C81, double* r9, int32_t* status) {
  int rc = marginal_state("observation_mahalanobis");
  if (rc != SLIDE_OK) return rc;
  struct Group { int type = 0; std::vector<int32_t> pid, lid; std::vector<double> z, sg; std::vector<int> ids; };
  Group groups[3];
  groups[0].type = FT_BR; groups[1].type = FT_CUBE; groups[2].type = FT_CYL;
  for (int k = 0; k < n; ++k) {
    d2[k] = 0.0;
    for (int e = 0; C81 && e < 81; ++e) C81[81 * (size_t)k + e] = 0.0;
    for (int e = 0; r9 && e < 9; ++e) r9[9 * (size_t)k + e] = 0.0;
    if (dof) dof[k] = landmark_dim(cls[k]);
    const ObsCand c = obs_candidate(robot[k], pose_idx[k], cls[k], lm_idx[k], meas17 + 17 * (size_t)k);
    if (status) status[k] = c.st;
    if (c.st != SLIDE_OK) continue;
    Group& g = groups[c.type == FT_BR ? 0 : c.type == FT_CUBE ? 1 : 2];
    g.pid.push_back(c.p); g.lid.push_back(c.l); g.ids.push_back(k);
    g.z.insert(g.z.end(), c.z, c.z + 15);
    g.sg.insert(g.sg.end(), c.sg, c.sg + 9);
  }
  hipStream_t s = stream;
  for (Group& g : groups) {
    if (g.ids.empty()) continue;
    const int m = (int)g.ids.size(), nk = lf_rows(g.type), max_nc = std::min(m, SLIDE_INFO_GAIN_SWEEP_COLS / nk);
    Scratch sc(s);
    int32_t* d_pid = sc.alloc<int32_t>(m);
    int32_t* d_lid = sc.alloc<int32_t>(m);
    double* d_z = sc.alloc<double>(15 * (size_t)m);
    double* d_sg = sc.alloc<double>(9 * (size_t)m);
    double* d_r = sc.alloc<double>(9 * (size_t)max_nc);
    double* d_G0 = sc.alloc<double>(81 * (size_t)max_nc);
    double* d_out = sc.alloc<double>(OBS_GATE_OUT * (size_t)max_nc);
    int* d_flag = sc.alloc<int>(max_nc);
    if (!sc.ok()) { g_last_error = "observation_mahalanobis: out of device memory"; return SLIDE_ERR_HIP; }
    SL_HIP(sc.upload(d_pid, g.pid));
    SL_HIP(sc.upload(d_lid, g.lid));
    SL_HIP(sc.upload(d_z, g.z));
    SL_HIP(sc.upload(d_sg, g.sg));
    std::vector<double> h(OBS_GATE_OUT * (size_t)max_nc);
    std::vector<int> hflag(max_nc);
    rc = sigma_forms(
        "observation_mahalanobis", m, nk,
        [&](int k0, int nc, double* B, int nT) {
          launch_obs_gate_lin(G, g.type, d_pid + k0, d_lid + k0, d_z + 15 * (size_t)k0, d_sg + 9 * (size_t)k0, nc, B, nT, d_r, d_G0, s);
        },
        [&](int k0, int nc, const double* M) -> int {
          launch_obs_gate_finish(nk, M, d_G0, d_r, nc, d_out, d_flag, s);
          SL_HIP(hipGetLastError());
          SL_HIP(hipMemcpyAsync(h.data(), d_out, OBS_GATE_OUT * (size_t)nc * sizeof(double), hipMemcpyDeviceToHost, s));
          SL_HIP(hipMemcpyAsync(hflag.data(), d_flag, nc * sizeof(int), hipMemcpyDeviceToHost, s));
          SL_HIP(hipStreamSynchronize(s));
          for (int i = 0; i < nc; ++i) {
            const size_t k = (size_t)g.ids[k0 + i];
            if (hflag[i]) {
              if (status) status[k] = SLIDE_ERR_NOT_SPD;
              continue;
            }
            const double* o = h.data() + OBS_GATE_OUT * (size_t)i;
            d2[k] = o[0];
            if (C81) std::copy(o + 1, o + 82, C81 + 81 * k);
            if (r9) std::copy(o + 82, o + 91, r9 + 9 * k);
          }
          return SLIDE_OK;
        },
        [&](int k0, int nc) -> int { return obs_walk_start(g.pid.data() + k0, g.lid.data() + k0, nc); });
    if (rc != SLIDE_OK) return rc;
  }
  return SLIDE_OK;
}

// ---- landmark pairs: are two landmarks of one class the same object? ----------------------------------------------------------------
// What the pair queries resolve of a pair before the device is asked: the two landmarks' ids (SLIDE_MISSING for a landmark the graph
// does not hold, or one without a factor; SLIDE_ERR_INVALID when a and b are one landmark), the lowest pose that observes either, and
// the route, from the structure alone.  Route 0 needs every Sigma(p_f, p_g) between the observers of a and b inside the selected
// inverse: with lo / hi the lowest and highest row of those poses, every block column of tile(lo) .. tile(hi) must reach tile(hi)
// (prof[tile(lo)] >= tile(hi) says it all where the profile does not decrease; a dense profile always does).
// SLIDE_LM_PAIR_SUBSTITUTE=1 (a measurement and test aid): route 1 for every pair.
HostGraph::LmPair HostGraph::lm_pair(int cls, uint64_t idx_a, uint64_t idx_b) const {
  LmPair p;
  p.a = lm_lid(cls, idx_a);
  p.b = lm_lid(cls, idx_b);
  if (p.a < 0 || p.b < 0 || lm_fids[p.a].empty() || lm_fids[p.b].empty()) { p.st = SLIDE_MISSING; return p; }
  if (p.a == p.b) { p.st = SLIDE_ERR_INVALID; return p; }
  int lo = 1 << 30, hi = -1;
  for (int l : {p.a, p.b})
    for (int f : lm_fids[l]) { lo = std::min(lo, h_lf_pose[f]); hi = std::max(hi, h_lf_pose[f]); }
  p.lo = lo;
  const char* fs = std::getenv("SLIDE_LM_PAIR_SUBSTITUTE");
  if (fs && fs[0] == '1') { p.route = 1; return p; }
  if (h_prof.size() != (size_t)G.T) return p;
  const int tl = (6 * lo) / NB, th = (6 * hi + 5) / NB;
  for (int t = tl; t <= th && t < G.T; ++t)
    if (h_prof[t] < th) { p.route = 1; break; }
  return p;
}
// The two pair queries (cov_kernels.hip and obs_gate_kernels.hip have the invariants).  Pair k names the EXISTING landmarks
// (cls[k], idx_a[k]) and (cls[k], idx_b[k]).  cov = false, the test: with d = est_b - est_a at the current estimate, r = d / sigma,
// Sig_d = Sig_aa + Sig_bb - Sig_ab - Sig_ba at the last linearisation point, C = I + diag(1 / sigma) Sig_d diag(1 / sigma) and
// d2 = r^T C^-1 r, chi-square with D degrees of freedom when a and b are one object up to the model noise sigma (sig3 for points,
// sig7 for cylinders, tangent order); no threshold is applied.  cov = true: the pair's joint marginal, 2 D x 2 D with leading
// dimension 18.  The pairs are grouped by class and route; results go back in the caller's order, and a pair's bits do not depend on
// what else is in the list: route 0 is one wavefront per pair on the selected inverse (ensure_sigma only if some pair takes it),
// route 1 sigma_forms with nk = D (2 D) columns per pair, the walk starting at the block column of the sweep's lowest observer.
// status[k]: SLIDE_MISSING, SLIDE_ERR_INVALID (a == b), SLIDE_ERR_NOT_SPD (a pivot of C); zeros in its outputs then.  Whole-call
// refusals as pose_covariances, nothing written.  Arguments checked by the caller.
int HostGraph::landmark_pairs(bool cov, int n, const int32_t* cls, const uint64_t* idx_a, const uint64_t* idx_b, const double* sig3,
                              const double* sig7, double* d2, int32_t* dof, double* C81, double* r9, double* out324, int32_t* route,
                              int32_t* status) {
  const char* who = cov ? "get_landmark_pair_covariances" : "landmark_pair_mahalanobis";
  int rc = marginal_state(who);
  if (rc != SLIDE_OK) return rc;
  struct Group { std::vector<int2> pr; std::vector<int> ids, lo; };
  Group groups[3][2];      // [SLIDE_CLS_*][route]
  bool any0 = false;
  for (int k = 0; k < n; ++k) {
    if (cov) {
      for (int e = 0; e < LM_PAIR_COV; ++e) out324[LM_PAIR_COV * (size_t)k + e] = 0.0;
    } else {
      d2[k] = 0.0;
      for (int e = 0; C81 && e < 81; ++e) C81[81 * (size_t)k + e] = 0.0;
      for (int e = 0; r9 && e < 9; ++e) r9[9 * (size_t)k + e] = 0.0;
      if (dof) dof[k] = landmark_dim(cls[k]);
    }
    const LmPair p = lm_pair(cls[k], idx_a[k], idx_b[k]);
    if (status) status[k] = p.st;
    if (route) route[k] = p.st == SLIDE_OK ? p.route : 0;
    if (p.st != SLIDE_OK) continue;
    Group& g = groups[cls[k]][p.route];
    g.pr.push_back(make_int2(p.a, p.b)); g.ids.push_back(k); g.lo.push_back(p.lo);
    any0 = any0 || p.route == 0;
  }
  if (any0 && (rc = ensure_sigma()) != SLIDE_OK) return rc;
  hipStream_t s = stream;
  for (int c = 0; c < 3; ++c)
    for (int rt = 0; rt < 2; ++rt) {
      const Group& g = groups[c][rt];
      if (g.ids.empty()) continue;
      const int m = (int)g.ids.size(), D = landmark_dim(c), nk = cov ? 2 * D : D;
      const int max_nc = rt == 0 ? m : std::min(m, SLIDE_INFO_GAIN_SWEEP_COLS / nk);
      const size_t per_out = cov ? LM_PAIR_COV : OBS_GATE_OUT;
      LmPairSigma sg{};
      for (int i = 0; i < D && !cov; ++i) sg.s[i] = (D == 3 ? sig3 : sig7)[i];
      Scratch sc(s);
      int2* d_pr = sc.alloc<int2>(m);
      double* d_r = sc.alloc<double>(9 * (size_t)max_nc);
      double* d_G0 = sc.alloc<double>(81 * (size_t)max_nc);
      double* d_out = sc.alloc<double>(per_out * (size_t)max_nc);
      int* d_flag = sc.alloc<int>(max_nc);
      if (!sc.ok()) { g_last_error = std::string(who) + ": out of device memory"; return SLIDE_ERR_HIP; }
      SL_HIP(sc.upload(d_pr, g.pr));
      std::vector<double> h(per_out * (size_t)max_nc);
      std::vector<int> hflag(max_nc, 0);
      // the sweep's (route 1) or the group's (route 0) results, pairs k0 .. k0 + nc - 1 of the group, into the caller's arrays
      auto read_back = [&](int k0, int nc) -> int {
        SL_HIP(hipGetLastError());
        SL_HIP(hipMemcpyAsync(h.data(), d_out, per_out * (size_t)nc * sizeof(double), hipMemcpyDeviceToHost, s));
        if (!cov) SL_HIP(hipMemcpyAsync(hflag.data(), d_flag, nc * sizeof(int), hipMemcpyDeviceToHost, s));
        SL_HIP(hipStreamSynchronize(s));
        for (int i = 0; i < nc; ++i) {
          const size_t k = (size_t)g.ids[k0 + i];
          const double* o = h.data() + per_out * (size_t)i;
          if (cov) { std::copy(o, o + LM_PAIR_COV, out324 + LM_PAIR_COV * k); continue; }
          if (hflag[i]) {
            if (status) status[k] = SLIDE_ERR_NOT_SPD;
            continue;
          }
          d2[k] = o[0];
          if (C81) std::copy(o + 1, o + 82, C81 + 81 * k);
          if (r9) std::copy(o + 82, o + 91, r9 + 9 * k);
        }
        return SLIDE_OK;
      };
      if (rt == 0) {
        if (cov) launch_lm_pair_cov(G, d_sig.d, G.ld, d_pr, m, d_out, s);
        else launch_lm_pair_direct(G, d_sig.d, G.ld, D, d_pr, m, sg, d_out, d_flag, s);
        rc = read_back(0, m);
      } else {
        rc = sigma_forms(
            who, m, nk,
            [&](int k0, int nc, double* B, int nT) { launch_lm_pair_fill(G, D, cov, d_pr + k0, sg, nc, B, nT, d_r, d_G0, s); },
            [&](int k0, int nc, const double* M) -> int {
              if (cov) launch_lm_pair_cov_finish(G, D, d_pr + k0, M, nc, d_out, s);
              else launch_obs_gate_finish(nk, M, d_G0, d_r, nc, d_out, d_flag, s);
              return read_back(k0, nc);
            },
            [&](int k0, int nc) -> int {
              const char* fw = std::getenv("SLIDE_OBS_GATE_FULL_WALK");
              if (fw && fw[0] == '1') return 0;
              int lo = 1 << 30;
              for (int i = 0; i < nc; ++i) lo = std::min(lo, g.lo[k0 + i]);
              return std::min((6 * lo) / NB, G.T - 1);
            });
      }
      if (rc != SLIDE_OK) return rc;
    }
  return SLIDE_OK;
}

// ---- the fixed-radius pair search (pairs_kernels.hip) -----------------------------------------------------------------------------
// Point q of n is the three doubles at d_pts + stride * (d_sel ? d_sel[q] : q), all on the device.  Launches: count, k_seg_scan, emit;
// blocking read-backs: the total, then the pairs.  *n_pairs is always the total; above cap SLIDE_ERR_CAPACITY and the vectors stay
// empty.  neq: d_label holds group words and only pairs of DIFFERENT groups are kept (the sibling kernel; the joint graph's cross_only).
static int pairs_within_dev(const char* who, hipStream_t s, const double* d_pts, int stride, const int* d_sel, const int32_t* d_label, int n,
                            double radius, int64_t cap, std::vector<int32_t>& vi, std::vector<int32_t>& vj, std::vector<double>& vd,
                            int64_t* n_pairs, bool neq = false) {
  *n_pairs = 0;
  vi.clear(); vj.clear(); vd.clear();
  if (n < 2) return SLIDE_OK;
  Scratch sc(s);
  int* d_cnt = sc.alloc<int>(n);
  long long* d_off = sc.alloc<long long>(n);
  int* d_seg = sc.alloc<int>(2);
  long long* d_tot = sc.alloc<long long>(1);
  if (!sc.ok()) { g_last_error = std::string(who) + ": out of device memory"; return SLIDE_ERR_HIP; }
  const std::vector<int> seg{0, n};
  SL_HIP(sc.upload(d_seg, seg));
  if (neq) launch_pairs_within_neq(false, d_pts, stride, d_sel, d_label, n, radius, d_cnt, nullptr, nullptr, nullptr, nullptr, s);
  else launch_pairs_within(false, d_pts, stride, d_sel, d_label, n, radius, d_cnt, nullptr, nullptr, nullptr, nullptr, s);
  launch_seg_scan64(d_cnt, d_seg, 1, d_off, d_tot, s);
  long long tot = 0;
  SL_HIP(hipMemcpyAsync(&tot, d_tot, sizeof(tot), hipMemcpyDeviceToHost, s));
  SL_HIP(hipStreamSynchronize(s));
  SL_HIP(hipGetLastError());
  *n_pairs = tot;
  if (tot > cap) { g_last_error = std::string(who) + ": more pairs than cap (n_pairs holds the total)"; return SLIDE_ERR_CAPACITY; }
  if (tot == 0) return SLIDE_OK;
  int32_t* d_i = sc.alloc<int32_t>((size_t)tot);
  int32_t* d_j = sc.alloc<int32_t>((size_t)tot);
  double* d_d = sc.alloc<double>((size_t)tot);
  if (!sc.ok()) { g_last_error = std::string(who) + ": out of device memory"; return SLIDE_ERR_HIP; }
  if (neq) launch_pairs_within_neq(true, d_pts, stride, d_sel, d_label, n, radius, nullptr, d_off, d_i, d_j, d_d, s);
  else launch_pairs_within(true, d_pts, stride, d_sel, d_label, n, radius, nullptr, d_off, d_i, d_j, d_d, s);
  vi.resize((size_t)tot); vj.resize((size_t)tot); vd.resize((size_t)tot);
  SL_HIP(hipMemcpyAsync(vi.data(), d_i, sizeof(int32_t) * (size_t)tot, hipMemcpyDeviceToHost, s));
  SL_HIP(hipMemcpyAsync(vj.data(), d_j, sizeof(int32_t) * (size_t)tot, hipMemcpyDeviceToHost, s));
  SL_HIP(hipMemcpyAsync(vd.data(), d_d, sizeof(double) * (size_t)tot, hipMemcpyDeviceToHost, s));
  SL_HIP(hipStreamSynchronize(s));
  SL_HIP(hipGetLastError());
  return SLIDE_OK;
}
// the search over n host points (xyz: 3 per point; label: one per point, or null); arguments checked by the caller
int pairs_within_host(const double* xyz, const int32_t* label, int n, double radius, int64_t cap, int32_t* out_i, int32_t* out_j, double* out_dist,
                      int64_t* n_pairs) {
  *n_pairs = 0;
  if (n < 2) return SLIDE_OK;
  if (slide_device_check(-1) != SLIDE_OK) return SLIDE_ERR_HIP;
  Scratch sc(nullptr);
  double* d_pts = sc.alloc<double>(3 * (size_t)n);
  int32_t* d_label = label ? sc.alloc<int32_t>(n) : nullptr;
  if (!sc.ok()) { g_last_error = "pairs_within: out of device memory"; return SLIDE_ERR_HIP; }
  SL_HIP(hipMemcpyAsync(d_pts, xyz, sizeof(double) * 3 * (size_t)n, hipMemcpyHostToDevice, nullptr));
  if (label) SL_HIP(hipMemcpyAsync(d_label, label, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, nullptr));
  std::vector<int32_t> vi, vj;
  std::vector<double> vd;
  const int rc = pairs_within_dev("pairs_within", nullptr, d_pts, 3, nullptr, d_label, n, radius, cap, vi, vj, vd, n_pairs);
  if (rc != SLIDE_OK) return rc;
  std::copy(vi.begin(), vi.end(), out_i);
  std::copy(vj.begin(), vj.end(), out_j);
  std::copy(vd.begin(), vd.end(), out_dist);
  return SLIDE_OK;
}
// The same search over the device-resident estimate of the landmarks of one class: the anchor is the point's xyz, the cube's t or the
// cylinder's root (lm_est, 15 doubles per landmark).  The selection: sel_idx (n_sel keys; one the graph does not hold: SLIDE_MISSING
// for the call, nothing written) or, null, every landmark of the class the device holds, in the graph's order (n_sel is not read;
// sel_label then has one entry per such landmark).  Pairs come back as keys, sorted by their positions in the selection.
int HostGraph::landmark_pairs_within(int cls, double radius, int n_sel, const uint64_t* sel_idx, const int32_t* sel_label, int64_t cap,
                                     uint64_t* idx_a, uint64_t* idx_b, double* dist, int64_t* n_pairs) {
  std::vector<int> lids;
  std::vector<uint64_t> keys;
  if (sel_idx) {
    for (int q = 0; q < n_sel; ++q) {
      const int l = lm_lid(cls, sel_idx[q]);
      if (l < 0) { g_last_error = "landmark_pairs_within: a selected landmark is not in the graph"; return SLIDE_MISSING; }
      lids.push_back(l); keys.push_back(sel_idx[q]);
    }
  } else {
    const uint64_t tag = lm_key(cls, 0) >> 56;
    std::vector<std::pair<int, uint64_t>> all;
    for (const auto& kv : key2lm)
      if ((kv.first >> 56) == tag && (size_t)kv.second < up_L && h_lm_key[kv.second] == kv.first)      // (not the aliases merge_landmarks left)
        all.emplace_back(kv.second, kv.first & ((1ull << 56) - 1ull));
    std::sort(all.begin(), all.end());
    for (const auto& e : all) { lids.push_back(e.first); keys.push_back(e.second); }
  }
  *n_pairs = 0;
  const int n = (int)lids.size();
  if (n < 2) return SLIDE_OK;
  hipStream_t s = stream;
  Scratch sc(s);
  int* d_sel = sc.alloc<int>(n);
  int32_t* d_label = sel_label ? sc.alloc<int32_t>(n) : nullptr;
  if (!sc.ok()) { g_last_error = "landmark_pairs_within: out of device memory"; return SLIDE_ERR_HIP; }
  SL_HIP(sc.upload(d_sel, lids));
  if (sel_label) SL_HIP(hipMemcpyAsync(d_label, sel_label, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, s));
  std::vector<int32_t> vi, vj;
  std::vector<double> vd;
  const int rc = pairs_within_dev("landmark_pairs_within", s, d_lm_est.d + (cls == SLIDE_CLS_CUBE ? 9 : 0), 15, d_sel, d_label, n, radius, cap, vi,
                                  vj, vd, n_pairs);
  if (rc != SLIDE_OK) return rc;
  for (size_t k = 0; k < vi.size(); ++k) { idx_a[k] = keys[vi[k]]; idx_b[k] = keys[vj[k]]; dist[k] = vd[k]; }
  return SLIDE_OK;
}

// The regularised incomplete gamma functions P(a, x) (*lower: by its series, x < a + 1) or Q(a, x) (by Lentz's continued fraction),
// whichever converges fast at x, and the density x^(a-1) e^-x / Gamma(a) — the textbook pair.
static double gamma_pq(double a, double x, bool* lower, double* dens) {
  const double lg = std::lgamma(a), front = std::exp(-x + a * std::log(x) - lg);
  *dens = front / x;
  *lower = x < a + 1.0;
  if (*lower) {
    double ap = a, del = 1.0 / a, sum = del;
    for (int n = 0; n < 100000; ++n) {
      ap += 1.0;
      del *= x / ap;
      sum += del;
      if (std::fabs(del) < std::fabs(sum) * 1e-17) break;
    }
    return sum * front;
  }
  const double tiny = 1e-300;
  double b = x + 1.0 - a, c = 1.0 / tiny, d = 1.0 / b, h = d;
  for (int i = 1; i < 100000; ++i) {
    const double an = -i * (i - a);
    b += 2.0;
    d = an * d + b;
    if (std::fabs(d) < tiny) d = tiny;
    c = b + an / c;
    if (std::fabs(c) < tiny) c = tiny;
    d = 1.0 / d;
    const double del = d * c;
    h *= del;
    if (std::fabs(del - 1.0) < 3e-16) break;
  }
  return front * h;
}
// q with P(dof / 2, q / 2) = prob: Newton on x = q / 2 from the mean, kept inside the bracket the signs seen so far give (a step that
// leaves it is replaced by the bracket's middle).  The residual is taken on the side the function was computed on (P - prob below
// the mean's neighbourhood, (1 - prob) - Q above), so the upper tail keeps its digits.
int chi2_quantile(double prob, int dof, double* q) {
  if (!q || !(prob > 0.0) || !(prob < 1.0) || dof < 1) {
    g_last_error = "chi2_quantile: prob outside (0, 1), dof < 1 or a NULL pointer";
    return SLIDE_ERR_INVALID;
  }
  const double a = 0.5 * dof;
  double lo = 0.0, hi = 0.0, x = a;      // (hi == 0: no upper end yet)
  for (int it = 0; it < 200; ++it) {
    bool lower;
    double dens;
    const double v = gamma_pq(a, x, &lower, &dens);
    const double f = lower ? v - prob : (1.0 - prob) - v;      // (P(a, x) - prob either way)
    if (f > 0.0) hi = x; else lo = x;
    double xn = x - f / dens;
    if (!(xn > lo) || (hi > 0.0 && !(xn < hi)) || !std::isfinite(xn)) xn = hi > 0.0 ? 0.5 * (lo + hi) : 2.0 * x;
    const double step = std::fabs(xn - x);
    x = xn;
    if (step <= 1e-15 * x) break;
  }
  *q = 2.0 * x;
  return SLIDE_OK;
}

// ---- what the two joint-compatibility calls share (one graph below, the joint graph of a CholBatch at the end of this file) -----------
// The caller resolves its candidates (JcCand: the class's factor type or -1 for a skipped one, the two ids the sweep's table carries,
// the landmark's identity and whether a group may name it once only, z and the sigmas); JcPlan packs whole groups into sweeps, holds
// the quantile table, the device buffers of the fill and the chain and the read-back's layout, runs the chain and scatters.
struct JcOutputs {
  int32_t* accepted; double *d2_single, *d2_joint; int32_t *dof_joint, *status;
  double* group_d2; int32_t *group_dof, *group_count, *group_status;
};
struct JcCand { int type = -1, p = -1, l = -1; long long ident = 0; bool once = true; const double *z = nullptr, *sg = nullptr; };
struct JcSweep : FormGroups {
  std::vector<int> gid, src;      // the caller's group of each group, the caller's candidate of each entry
  std::vector<int2> gcand;
  std::vector<int4> tab;          // {type (-1: skipped), p, l, first column} per entry: what the fill and the chain read
  std::vector<double> z, sg;
  size_t wsz = 0;
  int lds_rows = 0;
  bool big = false;
};
struct JcPlan {
  std::vector<JcSweep> sweeps;
  std::vector<const FormGroups*> forms;
  std::vector<double> qtab, h;
  size_t max_c = 0, max_g = 0, max_w = 0, o_gd = 0, o_i = 0, n_out = 0;
  int4* d_tab = nullptr;
  int2* d_gcand = nullptr;
  double *d_z = nullptr, *d_sg = nullptr, *d_r = nullptr, *d_G0 = nullptr, *d_q = nullptr, *d_work = nullptr, *d_out = nullptr;
  // q(1 .. JOINT_MAX_ROWS) of the call's probability, built once and kept while the probability stays (zeros: evaluate only)
  int quantiles(double prob) {
    qtab.assign(JOINT_MAX_ROWS, 0.0);
    if (!(prob > 0.0)) return SLIDE_OK;
    static std::mutex q_mtx;
    static double q_prob = 0.0;
    static std::vector<double> q_tab;
    std::lock_guard<std::mutex> lk(q_mtx);
    if (q_prob != prob) {
      q_tab.assign(JOINT_MAX_ROWS, 0.0);
      q_prob = 0.0;
      for (int d = 0; d < JOINT_MAX_ROWS; ++d) {
        const int rc = chi2_quantile(prob, d + 1, &q_tab[d]);
        if (rc != SLIDE_OK) return rc;
      }
      q_prob = prob;
    }
    qtab = q_tab;
    return SLIDE_OK;
  }
  // the sweeps: whole groups in the caller's order; every candidate of a packed group has an entry of the sweep's table.  A group
  // that names a once-only landmark twice (SLIDE_ERR_INVALID) or has more than a sweep's rows (SLIDE_ERR_CAPACITY) is left out.
  void pack(int n_groups, const int32_t* group_ptr, const std::vector<JcCand>& cs, const JcOutputs& o) {
    for (int g = 0; g < n_groups; ++g) {
      o.group_d2[g] = 0.0; o.group_dof[g] = 0; o.group_count[g] = 0; o.group_status[g] = SLIDE_OK;
      int rows = 0;
      bool twice = false;
      std::vector<long long> seen;
      for (int k = group_ptr[g]; k < group_ptr[g + 1]; ++k) {
        if (cs[k].type < 0) continue;
        rows += lf_rows(cs[k].type);
        if (!cs[k].once) continue;
        twice = twice || std::find(seen.begin(), seen.end(), cs[k].ident) != seen.end();
        seen.push_back(cs[k].ident);
      }
      if (twice) { o.group_status[g] = SLIDE_ERR_INVALID; continue; }
      if (rows > SLIDE_INFO_GAIN_SWEEP_COLS) { o.group_status[g] = SLIDE_ERR_CAPACITY; continue; }
      if (rows == 0) continue;
      if (sweeps.empty() || sweeps.back().ncol + rows > SLIDE_INFO_GAIN_SWEEP_COLS) sweeps.emplace_back();
      JcSweep& w = sweeps.back();
      const int gi = (int)w.cd.size(), nsplit = gain_gram_splits(rows), nt = (rows + 15) / 16;
      const size_t nn = (size_t)rows * rows;
      w.cd.push_back(GainCandDev{w.ncol, rows, nsplit, 0, (long long)w.msz, (long long)w.psz, (long long)w.wsz});
      w.gid.push_back(g);
      w.gcand.push_back(make_int2((int)w.tab.size(), group_ptr[g + 1] - group_ptr[g]));
      for (int ta = 0; ta < nt; ++ta)
        for (int tb = 0; tb <= ta; ++tb)
          for (int sp = 0; sp < nsplit; ++sp) w.jobs.push_back(make_int4(gi, ta, tb, sp));
      w.msz += nn;
      w.psz += nn * nsplit;
      if (rows > GAIN_LDS_DIM) { w.wsz += nn; w.big = true; }
      else w.lds_rows = std::max(w.lds_rows, rows);
      for (int k = group_ptr[g]; k < group_ptr[g + 1]; ++k) {
        const JcCand& c = cs[k];
        const bool on = c.type >= 0;
        w.tab.push_back(make_int4(on ? c.type : -1, c.p, c.l, w.ncol));
        w.src.push_back(k);
        w.z.insert(w.z.end(), c.z, c.z + 15);
        w.sg.insert(w.sg.end(), c.sg, c.sg + 9);
        if (on) w.ncol += lf_rows(c.type);
      }
    }
    for (const JcSweep& w : sweeps) {
      max_c = std::max(max_c, w.tab.size()); max_g = std::max(max_g, w.cd.size()); max_w = std::max(max_w, w.wsz);
      forms.push_back(&w);
    }
    // what comes back, in one buffer: {d2_single, d2_joint} per entry, d2 per group, then {accepted, dof_joint, not SPD} per entry and
    // {rows, count} per group as ints
    o_gd = 2 * max_c; o_i = o_gd + max_g;
    n_out = o_i + (3 * max_c + 2 * max_g + 1) / 2;
  }
  // the buffers of the fill and the chain, from the query's scratch (the caller asks sc.ok() after its own allocations)
  void alloc(Scratch& sc) {
    d_tab = sc.alloc<int4>(max_c);
    d_gcand = sc.alloc<int2>(max_g);
    d_z = sc.alloc<double>(15 * max_c);
    d_sg = sc.alloc<double>(9 * max_c);
    d_r = sc.alloc<double>(9 * max_c);
    d_G0 = sc.alloc<double>(81 * max_c);
    d_q = sc.alloc<double>(JOINT_MAX_ROWS);
    d_work = sc.alloc<double>(max_w);
    d_out = sc.alloc<double>(n_out);
    h.resize(n_out);
  }
  int upload(Scratch& sc, int si) {
    const JcSweep& w = sweeps[si];
    SL_HIP(sc.upload(d_tab, w.tab));
    SL_HIP(sc.upload(d_gcand, w.gcand));
    SL_HIP(sc.upload(d_z, w.z));
    SL_HIP(sc.upload(d_sg, w.sg));
    return SLIDE_OK;
  }
  // the chain on the sweep's (signed) gram, one read-back, the scatter into the caller's arrays
  int finish(const char* who, int si, const GainCandDev* d_cd, const double* M, double prob, hipStream_t s, const JcOutputs& o) {
    const JcSweep& w = sweeps[si];
    const int ng = (int)w.cd.size(), nc = (int)w.tab.size();
    int* d_outi = reinterpret_cast<int*>(d_out + o_i);
    if (launch_joint_compat_chain(d_cd, d_gcand, ng, d_tab, M, d_G0, d_r, d_q, prob > 0.0 ? 0 : 1, d_work, w.lds_rows, w.big, d_out, d_outi,
                                  d_out + o_gd, d_outi + 3 * max_c, s)) {
      g_last_error = std::string(who) + ": the device refuses the chain kernel's LDS";
      return SLIDE_ERR_HIP;
    }
    SL_HIP(hipGetLastError());
    SL_HIP(hipMemcpyAsync(h.data(), d_out, n_out * sizeof(double), hipMemcpyDeviceToHost, s));
    SL_HIP(hipStreamSynchronize(s));
    const int* hi = reinterpret_cast<const int*>(h.data() + o_i);
    for (int e = 0; e < nc; ++e) {
      const int k = w.src[e];
      if (w.tab[e].x < 0) continue;
      if (hi[3 * e + 2]) { o.status[k] = SLIDE_ERR_NOT_SPD; continue; }
      o.accepted[k] = hi[3 * e]; o.dof_joint[k] = hi[3 * e + 1];
      o.d2_single[k] = h[2 * e]; o.d2_joint[k] = h[2 * e + 1];
    }
    for (int gi = 0; gi < ng; ++gi) {
      const int g = w.gid[gi];
      o.group_d2[g] = h[o_gd + gi];
      o.group_dof[g] = hi[3 * max_c + 2 * gi];
      o.group_count[g] = hi[3 * max_c + 2 * gi + 1];
    }
    return SLIDE_OK;
  }
};

// The joint-compatibility test of n_groups hypotheses against the resident factor (obs_joint_kernels.hip has the invariant and the
// rule; observation_mahalanobis above tests each candidate alone).  Group g is the candidates group_ptr[g] .. group_ptr[g + 1] - 1 in
// the caller's order, resolved as the individual gate resolves them (obs_candidate); a SLIDE_MISSING candidate is skipped and the rest
// of its group served as if it were absent.  group_status: SLIDE_ERR_INVALID when two served candidates name one landmark (the
// invariant needs distinct landmarks), SLIDE_ERR_CAPACITY when the served rows exceed SLIDE_INFO_GAIN_SWEEP_COLS; zeros everywhere in
// such a group, its neighbours served.  The groups are packed whole, in the caller's order, into sweeps of at most
// SLIDE_INFO_GAIN_SWEEP_COLS columns; a group's columns are contiguous, its candidates in the caller's order, classes mixed.  Per
// sweep: one fill launch (k_obs_joint_lin, a class per wavefront), T - k0 substitution launches (the short walk over all its
// candidates), the gram's two launches over the lower tiles of every group's whole W^T W, the chain (k_joint_compat_chain, one launch
// per kind of group: factored in LDS up to GAIN_LDS_DIM rows, in the work buffer past it), one read-back.  A group's bits do not
// depend on what else is in the call or where it stands.  prob == 0: evaluate only, every served candidate is accepted (its d2_joint
// the prefix sequence of the stacked test).  Whole-call refusals as pose_covariances, nothing written.  Arguments checked by the caller.
int HostGraph::observation_joint_compatibility(int n_groups, const int32_t* group_ptr, const int32_t* robot, const uint64_t* pose_idx,
                                               const int32_t* cls, const uint64_t* lm_idx, const double* meas17, double prob, int32_t* accepted,
                                               double* d2_single, double* d2_joint, int32_t* dof_joint, int32_t* status, double* group_d2,
                                               int32_t* group_dof, int32_t* group_count, int32_t* group_status) {
  static_assert(JOINT_MAX_ROWS == SLIDE_INFO_GAIN_SWEEP_COLS, "a group fills one sweep at the most");
  int rc = marginal_state("observation_joint_compatibility");
  if (rc != SLIDE_OK) return rc;
  const char* who = "observation_joint_compatibility";
  const JcOutputs o{accepted, d2_single, d2_joint, dof_joint, status, group_d2, group_dof, group_count, group_status};
  JcPlan P;
  if ((rc = P.quantiles(prob)) != SLIDE_OK) return rc;
  const int n = n_groups > 0 ? group_ptr[n_groups] : 0;
  std::vector<ObsCand> cs(n);
  std::vector<JcCand> jc(n);
  for (int k = 0; k < n; ++k) {
    cs[k] = obs_candidate(robot[k], pose_idx[k], cls[k], lm_idx[k], meas17 + 17 * (size_t)k);
    accepted[k] = 0; d2_single[k] = 0.0; d2_joint[k] = 0.0; dof_joint[k] = 0;
    status[k] = cs[k].st;
    jc[k] = JcCand{cs[k].st == SLIDE_OK ? cs[k].type : -1, cs[k].p, cs[k].l, cs[k].l, true, cs[k].z, cs[k].sg};
  }
  P.pack(n_groups, group_ptr, jc, o);
  if (P.sweeps.empty()) return SLIDE_OK;
  hipStream_t s = stream;
  Scratch sc(s);
  P.alloc(sc);
  if (!sc.ok()) { g_last_error = std::string(who) + ": out of device memory"; return SLIDE_ERR_HIP; }
  SL_HIP(sc.upload(P.d_q, P.qtab));
  FormBackend be;
  form_backend(be, [&](int si, int) -> int {      // (the walk's start: the served candidates' ids)
    std::vector<int32_t> pid, lid;
    for (const int4& e : P.sweeps[si].tab)
      if (e.x >= 0) { pid.push_back(e.y); lid.push_back(e.z); }
    return obs_walk_start(pid.data(), lid.data(), (int)pid.size());
  });
  return sigma_forms_groups_core(
      who, be, P.forms,
      [&](int si, double* B, int nT) -> int {
        if ((rc = P.upload(sc, si)) != SLIDE_OK) return rc;
        launch_obs_joint_lin(G, P.d_tab, P.d_z, P.d_sg, (int)P.sweeps[si].tab.size(), B, nT, P.d_r, P.d_G0, s);
        return SLIDE_OK;
      },
      [&](int si, const GainCandDev* d_cd, const double* M) -> int { return P.finish(who, si, d_cd, M, prob, s, o); });
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

// What the joint gain queries share: the last exact pass's elimination tree and the schedule of the many-right-hand-side solve over it,
// where every system's rows lie in the buffers X (solutions, U at the end) and Rb (right-hand sides) — the robots first, then the
// separator; leading dimension N — and the grams' row lists: the poses of the robot in `slot`, of every robot, the job's shared point
// landmarks (each slot once); the private point landmarks of every graph (k_lm_V on its robot's rows)
struct CholBatch::JointGain {
  JointTree t;
  JointTree::SolvePlan plan;
  std::vector<size_t> off;
  size_t N = 0, nl = 0, ldv = 1;
  std::vector<int> rows_slot, rows_all, rows_sh, lms, lm0;
  std::vector<int> rows_pos, rows_neg;               // (joint_form_backend: form_rows' two lists)
  std::vector<long long> sep_first;                  // (joint_obs_candidate: per separator row its entry row, built on first use)
  // the device side, from the query's scratch
  JSinvSys* d_sys = nullptr;
  int4* d_jobs = nullptr;
  int2* d_sent = nullptr;
  int *d_lst = nullptr, *d_sptr = nullptr, *d_rslot = nullptr, *d_rall = nullptr, *d_rsh = nullptr, *d_lms = nullptr;
  std::vector<int*> d_prow, d_map;
  int prow_of(int sl, int p) const { return (int)off[1 + sl] + t.prow[sl][p]; }
  void build(const CholBatch& b, int slot) {
    const int n = b.n;
    b.joint_tree(t);
    off.assign(n + 1, 0);
    for (int i = 0; i < n; ++i) { off[1 + i] = N; N += (size_t)t.Trow[i] * NB; }
    off[0] = N; N += (size_t)t.Tsep * NB;
    t.solve_plan(plan);
    lm0.assign(n + 1, 0);
    for (int i = 0; i < n; ++i) {
      std::vector<int> poses;
      b.graphs[i]->robot_poses(b.joint_robot(i), poses);
      for (int p : poses)
        for (int a = 0; a < 6; ++a) {
          rows_all.push_back(prow_of(i, p) + a);
          if (i == slot) rows_slot.push_back(prow_of(i, p) + a);
        }
    }
    std::vector<std::vector<int>> priv;
    std::vector<int> sh_off;
    b.job_point_landmarks(priv, sh_off);
    for (int i = 0; i < n; ++i) { lms.insert(lms.end(), priv[i].begin(), priv[i].end()); lm0[i + 1] = (int)lms.size(); }
    for (int o : sh_off)
      for (int a = 0; a < 3; ++a) rows_sh.push_back((int)off[0] + o + a);
    nl = lms.size();
    ldv = std::max<size_t>(9 * nl, 1);
  }
  // the tables to the device; X and Rb are bound.  ne, d_rc: room for that many (row, column) pairs of J^T behind the lists, d_rc points
  // there (the batch keeps its pairs elsewhere)
  int upload(Scratch& sc, double* X, double* Rb, size_t ne = 0, int** d_rc = nullptr) {
    const int n = (int)t.T.size(), NS = 1 + n;
    d_sys = sc.alloc<JSinvSys>(NS);
    d_jobs = sc.alloc<int4>(plan.jobs.size());
    d_sent = sc.alloc<int2>(plan.sent.size());
    d_lst = sc.alloc<int>(plan.lst.size() + plan.sptr.size() + 2 * ne + rows_slot.size() + rows_all.size() + rows_sh.size() + nl);
    d_prow.assign(n, nullptr); d_map.assign(n, nullptr);
    for (int i = 0; i < n; ++i) {
      d_prow[i] = sc.alloc<int>(t.prow[i].size());
      d_map[i] = sc.alloc<int>(t.map[i].size());
    }
    if (!sc.ok()) return SLIDE_OK;                    // (the caller asks sc.ok() after its own allocations)
    for (int sy = 0; sy < NS; ++sy) { t.Y[sy].Sg = X + off[sy]; t.Y[sy].Z = Rb + off[sy]; t.Y[sy].lds = (long long)N; }
    d_sptr = d_lst + plan.lst.size();
    int* pairs = d_sptr + plan.sptr.size();
    if (d_rc) *d_rc = pairs;
    d_rslot = pairs + 2 * ne;
    d_rall = d_rslot + rows_slot.size();
    d_rsh = d_rall + rows_all.size();
    d_lms = d_rsh + rows_sh.size();
    SL_HIP(sc.upload(d_sys, t.Y));
    SL_HIP(sc.upload(d_jobs, plan.jobs));
    SL_HIP(sc.upload(d_sent, plan.sent));
    SL_HIP(sc.upload(d_lst, plan.lst));
    SL_HIP(sc.upload(d_sptr, plan.sptr));
    SL_HIP(sc.upload(d_rslot, rows_slot));
    SL_HIP(sc.upload(d_rall, rows_all));
    SL_HIP(sc.upload(d_rsh, rows_sh));
    SL_HIP(sc.upload(d_lms, lms));
    for (int i = 0; i < n; ++i) { SL_HIP(sc.upload(d_prow[i], t.prow[i])); SL_HIP(sc.upload(d_map[i], t.map[i])); }
    return SLIDE_OK;
  }
  // X = K^-1 R in S (R = J^T in Rb on entry)
  void solve(double* X, double* Rb, int ncol, hipStream_t s) const { walk(X, Rb, ncol, s, plan.launches.size()); }
  // The forward half alone: W = L^-1 R in the column tiles of X (a robot's rows of separator coordinates are not written: their
  // partial sums went into the separator's R).  B^T K^-1 B = W^T D W.
  void forward(double* X, double* Rb, int ncol, hipStream_t s) const { walk(X, Rb, ncol, s, (size_t)plan.n_fwd); }
  // The rows of the signed gram, every coordinate of the joint system once: each robot's own columns' rows [0, Tc NB) and the
  // separator's landmark rows (D = +I) into pos, the lambda rows (D = -I) into neg
  void form_rows(std::vector<int>& pos, std::vector<int>& neg) const {
    for (size_t i = 0; i < t.T.size(); ++i)
      for (int r = 0; r < t.Tc[i] * NB; ++r) pos.push_back((int)off[1 + i] + r);
    for (int r = 0; r < t.Tsep * NB; ++r) (r < t.Ts * NB ? pos : neg).push_back((int)off[0] + r);
  }
  JointPoseTab* d_tab = nullptr;             // (joint_sigma_forms: what the fill kernels address the poses by)
  void walk(double* X, double* Rb, int ncol, hipStream_t s, size_t n_launch) const {
    const int n = (int)t.T.size();
    JMSum sA{};
    JSigGather gA{};
    for (int i = 0; i < n; ++i) {
      sA.src[i] = Rb + off[1 + i];
      gA.dst[i] = X + off[1 + i]; gA.map[i] = d_map[i]; gA.lds[i] = (long long)N; gA.o0[i] = t.Tc[i] * NB; gA.n[i] = t.gn[i];
    }
    sA.dst = Rb + off[0]; sA.ld = (long long)N;
    gA.src = X + off[0]; gA.lds_src = (long long)N;
    for (size_t q = 0; q < n_launch; ++q) {
      const JointTree::SolvePlan::Launch& L = plan.launches[q];
      if (L.kind == 0) launch_jms_push(d_sys, d_jobs + L.j0, L.nj, L.maxl, d_lst, ncol, L.bwd, s);
      else if (L.kind == 1) launch_jms_pull(d_sys, d_jobs + L.j0, L.nj, d_lst, ncol, L.bwd, s);
      else if (L.kind == 2) launch_jms_sum(sA, d_sptr, d_sent, t.Tsep * NB, ncol, s);
      else launch_jms_gather(gA, n, plan.max_gn, ncol, s);
    }
  }
  // V of every graph's private point landmarks from its robot's rows of X
  void landmark_V(const CholBatch& b, const double* X, int ncol, double* V, hipStream_t s) const {
    for (int i = 0; i < (int)t.T.size(); ++i)
      launch_landmark_V(b.hG[i], X + off[1 + i], (int)N, ncol, d_lms + lm0[i], lm0[i + 1] - lm0[i], V + 9 * (size_t)lm0[i], ldv, s, d_prow[i]);
  }
};

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

// ---- quadratic forms on the joint graph: the joint marginal of pose pairs and the closure gate across robots ---------------------------
// The pass leaves K = L D L^T, D = +I but on the lambda block (factored as its negative: D = -I), so B^T K^-1 B = W^T D W with
// L W = B: the FORWARD half of the many-right-hand-side solve (JointGain::forward — the plan's launches before the backward pull of
// the top block) and a signed gram, every coordinate once (JointGain::form_rows).  The driver, the sweeps and the per-candidate grams
// are sigma_forms' (sigma_forms_core): per sweep one memset of R, one fill launch, one walk of the forward half, the grams (a second
// pair of launches and the subtraction only where the job has lambda rows), what done() queues, one read-back.  A candidate's bits
// depend on its own columns and the row lists alone.  joint_state first, under pass_mtx; nothing the pass reads is written and the
// cached joint Sigma is neither used nor touched.
// (the batch's back end of the quadratic-form drivers, for candidates of equal width and for groups alike: R and W of N rows, the
// joint plan's forward half — it has no short walk, so be.start stays unset — and form_rows' two lists, kept in jg)
void CholBatch::joint_form_backend(FormBackend& be, JointGain& jg) {
  hipStream_t s = master;
  std::vector<int>&pos = jg.rows_pos, &neg = jg.rows_neg;
  pos.clear(); neg.clear();
  jg.form_rows(pos, neg);
  be.s = s; be.ld = jg.N; be.nrows = (int)pos.size(); be.nrows_neg = (int)neg.size();
  be.alloc = [this, &be, &jg, &pos, &neg](Scratch& sc, int max_ncol) -> int {
    be.W = sc.alloc<double>(jg.N * max_ncol);
    be.B = sc.alloc<double>(jg.N * max_ncol);
    int* d_rows = sc.alloc<int>(pos.size() + neg.size());
    jg.d_tab = sc.alloc<JointPoseTab>(1);
    const int rc = jg.upload(sc, be.W, be.B);
    if (!sc.ok() || rc != SLIDE_OK) return rc;       // (the driver asks sc.ok() after its own allocations)
    be.rows = d_rows; be.rows_neg = d_rows + pos.size();
    SL_HIP(sc.upload(d_rows, pos));
    SL_HIP(sc.upload(d_rows + pos.size(), neg));
    std::vector<JointPoseTab> tab(1);
    for (int i = 0; i < n; ++i) {
      tab[0].est[i] = hG[i].pose_est; tab[0].prow[i] = jg.d_prow[i]; tab[0].off[i] = (long long)jg.off[1 + i]; tab[0].chart[i] = hG[i].chart;
    }
    SL_HIP(sc.upload(jg.d_tab, tab));
    return SLIDE_OK;
  };
  be.fwd = [&be, &jg, s](int ncol) { jg.forward(be.W, be.B, ncol, s); };
}
int CholBatch::joint_sigma_forms(const char* who, JointGain& jg, int ncand, int nk, const FormFill& fill, const FormDone& done) {
  FormBackend be;
  joint_form_backend(be, jg);
  return sigma_forms_core(who, be, ncand, nk, fill, done);
}
// One end of a candidate: its pose id in the graph of `slot`, or -1 (a slot the batch does not have, a pose its graph does not hold)
int CholBatch::joint_end(const JointGain& jg, int slot, uint64_t idx) const {
  if (slot < 0 || slot >= n) return -1;
  const int id = graphs[slot]->pose_id(joint_robot(slot), idx);
  return id >= 0 && (size_t)id < jg.t.prow[slot].size() ? id : -1;
}
// Marginals::jointMarginalCovariance on the joint graph: HostGraph::pose_pair_covariances with (slot, pose index) for each end.  A
// block between two robots is the one covariance the cached joint Sigma does not hold.  status[k] (or null): SLIDE_MISSING,
// SLIDE_ERR_INVALID (one pose twice); zeros then.  Whole-call refusals: joint_state's, nothing written.
int CholBatch::joint_pose_pair_covariances(int n_q, const int32_t* slot_a, const uint64_t* idx_a, const int32_t* slot_b, const uint64_t* idx_b,
                                           double* out144n, int32_t* status) {
  std::lock_guard<std::mutex> pl(pass_mtx);
  int rc = joint_state("get_pose_pair_covariances", 0);
  if (rc != SLIDE_OK) return rc;
  JointGain jg;
  jg.build(*this, 0);
  std::vector<int4> ends;
  std::vector<int> ids;
  for (int k = 0; k < n_q; ++k) {
    for (int e = 0; e < 144; ++e) out144n[144 * (size_t)k + e] = 0.0;
    const int a = joint_end(jg, slot_a[k], idx_a[k]), b = joint_end(jg, slot_b[k], idx_b[k]);
    const int st = a < 0 || b < 0 ? SLIDE_MISSING : (slot_a[k] == slot_b[k] && a == b) ? SLIDE_ERR_INVALID : SLIDE_OK;
    if (status) status[k] = st;
    if (st != SLIDE_OK) continue;
    ends.push_back(make_int4(slot_a[k], a, slot_b[k], b)); ids.push_back(k);
  }
  if (ids.empty()) return SLIDE_OK;
  hipStream_t s = master;
  Scratch sc(s);
  int4* d_ends = sc.alloc<int4>(ends.size());
  if (!sc.ok()) { g_last_error = "get_pose_pair_covariances: out of device memory"; return SLIDE_ERR_HIP; }
  SL_HIP(sc.upload(d_ends, ends));
  std::vector<double> h;
  return joint_sigma_forms(
      "get_pose_pair_covariances", jg, (int)ids.size(), 12,
      [&](int k0, int nc, double* B, int ld) { launch_joint_pair_identity(jg.d_tab, d_ends + k0, nc, B, (size_t)ld, s); },
      [&](int k0, int nc, const double* M) -> int {
        h.resize(144 * (size_t)nc);
        SL_HIP(hipMemcpyAsync(h.data(), M, h.size() * sizeof(double), hipMemcpyDeviceToHost, s));
        SL_HIP(hipStreamSynchronize(s));
        for (int i = 0; i < nc; ++i) std::copy(h.begin() + 144 * (size_t)i, h.begin() + 144 * (size_t)(i + 1), out144n + 144 * (size_t)ids[k0 + i]);
        return SLIDE_OK;
      });
}
// HostGraph::closure_mahalanobis on the joint graph: closure k is the Between factor with sigmas sigma6_k from pose (from_slot,
// from_idx) to (to_slot, to_idx); r_k and A_k by the same device text (closure_gate_lin_body) at the two graphs' device-resident
// estimates under the chart of the from pose's graph, Sigma the inverse of the joint system the pass linearised at pose_val — the
// linear-Gaussian model of joint_closure_info_gain.  C_k = I + A_k Sigma A_k^T from the signed gram, d2_k by k_closure_gate_finish.
// status[k] (or null): SLIDE_MISSING, SLIDE_ERR_INVALID (from and to are one pose), SLIDE_ERR_NOT_SPD; zeros then.
int CholBatch::joint_closure_mahalanobis(int L, const int32_t* from_slot, const uint64_t* from_idx, const int32_t* to_slot, const uint64_t* to_idx,
                                         const double* rel7, const double* sigma6, double* d2, double* C36, double* r6, int32_t* status) {
  std::lock_guard<std::mutex> pl(pass_mtx);
  int rc = joint_state("closure_mahalanobis", 0);
  if (rc != SLIDE_OK) return rc;
  JointGain jg;
  jg.build(*this, 0);
  std::vector<int4> ends;
  std::vector<double> z, sg;
  std::vector<int> ids;
  for (int k = 0; k < L; ++k) {
    d2[k] = 0.0;
    for (int e = 0; C36 && e < 36; ++e) C36[36 * (size_t)k + e] = 0.0;
    for (int e = 0; r6 && e < 6; ++e) r6[6 * (size_t)k + e] = 0.0;
    const int a = joint_end(jg, from_slot[k], from_idx[k]), b = joint_end(jg, to_slot[k], to_idx[k]);
    const int st = a < 0 || b < 0 ? SLIDE_MISSING : (from_slot[k] == to_slot[k] && a == b) ? SLIDE_ERR_INVALID : SLIDE_OK;
    if (status) status[k] = st;
    if (st != SLIDE_OK) continue;
    double z12[12];
    to12(from7(rel7 + 7 * (size_t)k), z12);
    ends.push_back(make_int4(from_slot[k], a, to_slot[k], b)); ids.push_back(k);
    z.insert(z.end(), z12, z12 + 12);
    sg.insert(sg.end(), sigma6 + 6 * (size_t)k, sigma6 + 6 * (size_t)k + 6);
  }
  if (ids.empty()) return SLIDE_OK;
  hipStream_t s = master;
  const int m = (int)ids.size(), max_nc = std::min(m, SLIDE_INFO_GAIN_SWEEP_COLS / 6);
  Scratch sc(s);
  int4* d_ends = sc.alloc<int4>(m);
  double* d_z = sc.alloc<double>(12 * (size_t)m);
  double* d_sg = sc.alloc<double>(6 * (size_t)m);
  double* d_r = sc.alloc<double>(6 * (size_t)m);
  double* d_out = sc.alloc<double>(GATE_OUT * (size_t)max_nc);
  int* d_flag = sc.alloc<int>(max_nc);
  if (!sc.ok()) { g_last_error = "closure_mahalanobis: out of device memory"; return SLIDE_ERR_HIP; }
  SL_HIP(sc.upload(d_ends, ends));
  SL_HIP(sc.upload(d_z, z));
  SL_HIP(sc.upload(d_sg, sg));
  std::vector<double> h(GATE_OUT * (size_t)max_nc);
  std::vector<int> hflag(max_nc);
  return joint_sigma_forms(
      "closure_mahalanobis", jg, m, 6,
      [&](int k0, int nc, double* B, int ld) {
        launch_joint_closure_gate_lin(jg.d_tab, d_ends + k0, d_z + 12 * (size_t)k0, d_sg + 6 * (size_t)k0, nc, B, (size_t)ld, d_r + 6 * (size_t)k0, s);
      },
      [&](int k0, int nc, const double* M) -> int {
        launch_closure_gate_finish(M, d_r + 6 * (size_t)k0, nc, d_out, d_flag, s);
        SL_HIP(hipGetLastError());
        SL_HIP(hipMemcpyAsync(h.data(), d_out, GATE_OUT * (size_t)nc * sizeof(double), hipMemcpyDeviceToHost, s));
        SL_HIP(hipMemcpyAsync(hflag.data(), d_flag, nc * sizeof(int), hipMemcpyDeviceToHost, s));
        SL_HIP(hipStreamSynchronize(s));
        for (int i = 0; i < nc; ++i) {
          const size_t k = (size_t)ids[k0 + i];
          if (hflag[i]) {
            if (status) status[k] = SLIDE_ERR_NOT_SPD;
            continue;
          }
          const double* o = h.data() + GATE_OUT * (size_t)i;
          d2[k] = o[0];
          if (C36) std::copy(o + 1, o + 37, C36 + 36 * k);
          if (r6) std::copy(o + 37, o + 43, r6 + 6 * k);
        }
        return SLIDE_OK;
      });
}
// What the two observation queries on the joint graph resolve of a candidate before the device is asked (HostGraph::obs_candidate's
// counterpart): the pose's id in the graph of pose_slot, the landmark's id in the graph of lm_slot, SLIDE_MISSING for a slot the batch
// lacks, a pose or landmark its graph does not hold, or a landmark with neither a factor nor a shared slot; for a SHARED landmark its
// separator offset sep_off and the joint row sep at which Al^T enters the walk; z and the sigmas by the add calls' own text with the
// parameters of the POSE's graph.
// Where a right-hand side on the separator coordinates [so, so + d) enters the walk: the separator's own rows of R are WRITTEN by
// the walk (k_jms_sum: the sum of the robots' rows of separator coordinates), so the entry goes to those rows of the LOWEST robot
// whose border holds them — one place whichever replica names the landmark, and 0 + x = x in the sum.  -1: no robot holds them.
static long long sep_entry_row(const std::vector<long long>& sep_first, int so, int d) {
  if (so < 0 || (size_t)(so + d) >= sep_first.size() || sep_first[so] < 0) return -1;
  for (int c = 1; c < d; ++c)
    if (sep_first[so + c] != sep_first[so] + c) return -1;      // (a landmark's coordinates are one run of its robot's border)
  return sep_first[so];
}
// One landmark of the joint graph as the joint queries name it, (slot, cls, local idx): its id l in the graph of `ls` (-1: a slot the
// batch lacks, a landmark its graph does not hold, or one with neither a factor nor a shared slot) and, for a SHARED landmark, its
// slot sh, its separator offset sep_off and the joint row sep at which a right-hand side on its coordinates enters the walk.
CholBatch::JointLmEnd CholBatch::joint_lm_end(JointGain& jg, int ls, int cls, uint64_t lm_idx) const {
  JointLmEnd e;
  if (ls < 0 || ls >= n) return e;
  const HostGraph* gl = graphs[ls];
  int l = gl->lm_lid(cls, lm_idx);
  if (l >= 0 && (size_t)l >= gl->up_L) l = -1;
  if (l >= 0 && (size_t)l < gl->h_lm_bord.size() && gl->h_lm_bord[l] >= 0) {
    int so = -1;
    for (size_t q = 0; q < gl->h_sh_lid.size(); ++q)
      if (gl->h_sh_lid[q] == l) { so = gl->h_sep_off[q]; e.sh = (int)q; break; }
    if (so >= 0 && jg.sep_first.empty()) {      // per separator row: its joint row in the lowest robot that maps it (-1: none)
      jg.sep_first.assign((size_t)jg.t.Tsep * NB + 1, -1);
      for (int i = n - 1; i >= 0; --i)
        for (int o = 0; o < jg.t.gn[i]; ++o)
          if (jg.t.map[i][o] >= 0) jg.sep_first[jg.t.map[i][o]] = (long long)jg.off[1 + i] + (long long)jg.t.Tc[i] * NB + o;
    }
    e.sep = so >= 0 ? sep_entry_row(jg.sep_first, so, landmark_dim(cls)) : -1;
    e.sep_off = e.sep >= 0 ? so : -1;
    if (e.sep < 0) l = -1;
  }
  if (l >= 0 && e.sep < 0 && gl->lm_fids[l].empty()) l = -1;
  e.l = l;
  return e;
}
CholBatch::JointObsCand CholBatch::joint_obs_candidate(JointGain& jg, int ps, uint64_t pose_idx, int ls, int cls, uint64_t lm_idx,
                                                       const double* a) const {
  JointObsCand c;
  c.type = cls == SLIDE_CLS_ELLIPSOID ? FT_BR : cls == SLIDE_CLS_CUBE ? FT_CUBE : FT_CYL;
  const int p = joint_end(jg, ps, pose_idx);
  const JointLmEnd le = joint_lm_end(jg, ls, cls, lm_idx);
  const int l = le.l;
  c.sep = le.sep;
  c.sep_off = le.sep_off;
  c.st = p < 0 || l < 0 ? SLIDE_MISSING : SLIDE_OK;
  if (c.st != SLIDE_OK) return c;
  c.ends = make_int4(ps, p, ls, l);
  const HostGraph* gp = graphs[ps];
  if (c.type == FT_BR) {
    HostGraph::br_meas(a, a[3], c.z);
    for (int i = 0; i < 3; ++i) c.sg[i] = gp->P.bearing_range_sigma;
  } else if (c.type == FT_CUBE) {
    gp->cube_meas(from7(a), from7(a + 7), a + 14, c.z, c.sg);
  } else {
    HostGraph::cyl_meas(from7(a), a + 7, a + 10, a[13], c.z);
    for (int i = 0; i < 7; ++i) c.sg[i] = gp->P.cylinder_sigma;
  }
  return c;
}
// HostGraph::observation_mahalanobis on the joint graph (obs_gate_kernels.hip has the invariant): candidate k is the factor
// add_range_bearing / add_cube / add_cylinder would add between pose (pose_slot, pose_idx) and the EXISTING landmark (cls, lm_idx) of
// the graph in lm_slot (null: the pose's slot) — the two may differ: robot a's pose against a landmark only robot b has mapped.  z and
// the sigmas by the add calls' own text with the parameters of the POSE's graph, r and A = [Ap | Al] at the two graphs' device-resident
// estimates by k_joint_obs_gate_lin, no robust weight.  A private landmark enters as on one graph, with joint rows and the factors'
// poses taken in the landmark's graph; a shared one is a separator variable the pass does not eliminate: Al^T is a right-hand side
// on its separator coordinates (h_sep_off of its slot, the coordinates JointGain::build lists in rows_sh) and G0 = 0.  The walk forms
// the separator's rows of R as the sum of the robots' rows of separator coordinates, so Al^T is written into those rows of the lowest
// robot that holds the landmark (sep_entry_row): one place whichever replica names it.  C = I + G0 + W^T D W from the signed gram, d2 by
// k_obs_gate_finish on M - Mneg.  Grouped by class, nk = 3 / 9 / 7 (128 / 42 / 54 candidates per sweep); every sweep walks the whole
// forward half of the joint plan (the single graph's short walk from a late block column has no counterpart there).  status[k] (or
// null): SLIDE_MISSING (a slot the batch lacks, a pose or landmark its graph does not hold, a landmark with neither a factor nor a
// shared slot), SLIDE_ERR_NOT_SPD; zeros then.  Whole-call refusals: joint_state's, nothing written.
int CholBatch::joint_observation_mahalanobis(int n_q, const int32_t* pose_slot, const uint64_t* pose_idx, const int32_t* lm_slot, const int32_t* cls,
                                             const uint64_t* lm_idx, const double* meas17, double* d2, int32_t* dof, double* C81, double* r9,
                                             int32_t* status) {
  std::lock_guard<std::mutex> pl(pass_mtx);
  int rc = joint_state("observation_mahalanobis", 0);
  if (rc != SLIDE_OK) return rc;
  JointGain jg;
  jg.build(*this, 0);
  struct Group { int type = 0; std::vector<int4> ends; std::vector<long long> sep; std::vector<double> z, sg; std::vector<int> ids; };
  Group groups[3];
  groups[0].type = FT_BR; groups[1].type = FT_CUBE; groups[2].type = FT_CYL;
  for (int k = 0; k < n_q; ++k) {
    d2[k] = 0.0;
    for (int e = 0; C81 && e < 81; ++e) C81[81 * (size_t)k + e] = 0.0;
    for (int e = 0; r9 && e < 9; ++e) r9[9 * (size_t)k + e] = 0.0;
    if (dof) dof[k] = landmark_dim(cls[k]);
    const JointObsCand c = joint_obs_candidate(jg, pose_slot[k], pose_idx[k], lm_slot ? lm_slot[k] : pose_slot[k], cls[k], lm_idx[k],
                                               meas17 + 17 * (size_t)k);
    if (status) status[k] = c.st;
    if (c.st != SLIDE_OK) continue;
    Group& g = groups[c.type == FT_BR ? 0 : c.type == FT_CUBE ? 1 : 2];
    g.ends.push_back(c.ends); g.sep.push_back(c.sep); g.ids.push_back(k);
    g.z.insert(g.z.end(), c.z, c.z + 15);
    g.sg.insert(g.sg.end(), c.sg, c.sg + 9);
  }
  hipStream_t s = master;
  for (Group& g : groups) {
    if (g.ids.empty()) continue;
    const int m = (int)g.ids.size(), nk = lf_rows(g.type), max_nc = std::min(m, SLIDE_INFO_GAIN_SWEEP_COLS / nk);
    Scratch sc(s);
    int4* d_ends = sc.alloc<int4>(m);
    long long* d_sep = sc.alloc<long long>(m);
    double* d_z = sc.alloc<double>(15 * (size_t)m);
    double* d_sg = sc.alloc<double>(9 * (size_t)m);
    double* d_r = sc.alloc<double>(9 * (size_t)max_nc);
    double* d_G0 = sc.alloc<double>(81 * (size_t)max_nc);
    double* d_out = sc.alloc<double>(OBS_GATE_OUT * (size_t)max_nc);
    int* d_flag = sc.alloc<int>(max_nc);
    if (!sc.ok()) { g_last_error = "observation_mahalanobis: out of device memory"; return SLIDE_ERR_HIP; }
    SL_HIP(sc.upload(d_ends, g.ends));
    SL_HIP(sc.upload(d_sep, g.sep));
    SL_HIP(sc.upload(d_z, g.z));
    SL_HIP(sc.upload(d_sg, g.sg));
    std::vector<double> h(OBS_GATE_OUT * (size_t)max_nc);
    std::vector<int> hflag(max_nc);
    rc = joint_sigma_forms(
        "observation_mahalanobis", jg, m, nk,
        [&](int k0, int nc, double* B, int ld) {
          launch_joint_obs_gate_lin(d_Gs, jg.d_tab, g.type, d_ends + k0, d_sep + k0, d_z + 15 * (size_t)k0, d_sg + 9 * (size_t)k0, nc, B, (size_t)ld,
                                    d_r, d_G0, s);
        },
        [&](int k0, int nc, const double* M) -> int {
          launch_obs_gate_finish(nk, M, d_G0, d_r, nc, d_out, d_flag, s);
          SL_HIP(hipGetLastError());
          SL_HIP(hipMemcpyAsync(h.data(), d_out, OBS_GATE_OUT * (size_t)nc * sizeof(double), hipMemcpyDeviceToHost, s));
          SL_HIP(hipMemcpyAsync(hflag.data(), d_flag, nc * sizeof(int), hipMemcpyDeviceToHost, s));
          SL_HIP(hipStreamSynchronize(s));
          for (int i = 0; i < nc; ++i) {
            const size_t k = (size_t)g.ids[k0 + i];
            if (hflag[i]) {
              if (status) status[k] = SLIDE_ERR_NOT_SPD;
              continue;
            }
            const double* o = h.data() + OBS_GATE_OUT * (size_t)i;
            d2[k] = o[0];
            if (C81) std::copy(o + 1, o + 82, C81 + 81 * k);
            if (r9) std::copy(o + 82, o + 91, r9 + 9 * k);
          }
          return SLIDE_OK;
        });
    if (rc != SLIDE_OK) return rc;
  }
  return SLIDE_OK;
}
// HostGraph::observation_joint_compatibility on the joint graph (obs_joint_kernels.hip has the invariant): the groups, prob, outputs
// and status words are that call's, the candidates are named and resolved as joint_observation_mahalanobis names and resolves them
// (joint_obs_candidate).  With a group's served candidates stacked, block (i, j) of C is [i == j] (I + G0_i) + W_i^T D W_j, L W = B on
// the pass's K = L D L^T: B_i and G0_i exactly what the individual joint gate writes, the cross blocks the off-diagonal part of the
// signed gram over form_rows' two lists.  A PRIVATE landmark — identity (lm_slot, local id) — may not be named twice in a group: H_ll
// is block diagonal and the cross block would miss Al_i H_ll^-1 Al_j^T (group_status SLIDE_ERR_INVALID).  A SHARED landmark —
// identity its separator offset, so two replicas are one landmark — may: it is a separator variable the pass does not eliminate,
// everything about it is in K, and W_i^T D W_j is the whole cross block.  Whole groups are packed into sweeps as on one graph
// (JcPlan); per sweep: one memset of R, one fill launch (k_joint_obs_joint_lin, classes mixed), one walk of the whole forward half of
// the joint plan, the gram's two launches over the lower tiles (a second pair and k_gram_sub only where the job has lambda rows), the
// chain, one read-back.  A group's bits do not depend on what else is in the call or where it stands.  Per candidate: SLIDE_MISSING
// (skipped, the group served without it), SLIDE_ERR_NOT_SPD; per group: SLIDE_ERR_INVALID, SLIDE_ERR_CAPACITY (zeros, the neighbours
// served).  Whole-call refusals: joint_state's, nothing written.  Nothing the pass reads is written; the cached joint Sigma is
// neither used nor touched.  Arguments checked by the caller.
int CholBatch::joint_observation_joint_compatibility(int n_groups, const int32_t* group_ptr, const int32_t* pose_slot, const uint64_t* pose_idx,
                                                     const int32_t* lm_slot, const int32_t* cls, const uint64_t* lm_idx, const double* meas17,
                                                     double prob, int32_t* accepted, double* d2_single, double* d2_joint, int32_t* dof_joint,
                                                     int32_t* status, double* group_d2, int32_t* group_dof, int32_t* group_count,
                                                     int32_t* group_status) {
  const char* who = "chol_batch_observation_joint_compatibility";
  std::lock_guard<std::mutex> pl(pass_mtx);
  int rc = joint_state(who, 0);
  if (rc != SLIDE_OK) return rc;
  JointGain jg;
  jg.build(*this, 0);
  const JcOutputs o{accepted, d2_single, d2_joint, dof_joint, status, group_d2, group_dof, group_count, group_status};
  JcPlan P;
  if ((rc = P.quantiles(prob)) != SLIDE_OK) return rc;
  const int nq = n_groups > 0 ? group_ptr[n_groups] : 0;
  std::vector<JointObsCand> cs(nq);
  std::vector<JcCand> jc(nq);
  for (int k = 0; k < nq; ++k) {
    JointObsCand& c = cs[k];
    c = joint_obs_candidate(jg, pose_slot[k], pose_idx[k], lm_slot ? lm_slot[k] : pose_slot[k], cls[k], lm_idx[k], meas17 + 17 * (size_t)k);
    accepted[k] = 0; d2_single[k] = 0.0; d2_joint[k] = 0.0; dof_joint[k] = 0;
    status[k] = c.st;
    const bool shared = c.sep >= 0;
    jc[k] = JcCand{c.st == SLIDE_OK ? c.type : -1, c.ends.y, c.ends.w, shared ? (long long)c.sep_off : ((long long)c.ends.z << 32) | (unsigned)c.ends.w,
                   !shared, c.z, c.sg};
  }
  P.pack(n_groups, group_ptr, jc, o);
  if (P.sweeps.empty()) return SLIDE_OK;
  hipStream_t s = master;
  Scratch sc(s);
  P.alloc(sc);
  int4* d_ends = sc.alloc<int4>(P.max_c);
  long long* d_sep = sc.alloc<long long>(P.max_c);
  if (!sc.ok()) { g_last_error = std::string(who) + ": out of device memory"; return SLIDE_ERR_HIP; }
  SL_HIP(sc.upload(P.d_q, P.qtab));
  std::vector<int4> ends;
  std::vector<long long> sep;
  FormBackend be;
  joint_form_backend(be, jg);
  return sigma_forms_groups_core(
      who, be, P.forms,
      [&](int si, double* B, int ld) -> int {
        const JcSweep& w = P.sweeps[si];
        ends.clear(); sep.clear();
        for (int k : w.src) { ends.push_back(cs[k].ends); sep.push_back(cs[k].sep); }
        if ((rc = P.upload(sc, si)) != SLIDE_OK) return rc;
        SL_HIP(sc.upload(d_ends, ends));
        SL_HIP(sc.upload(d_sep, sep));
        launch_joint_obs_joint_lin(d_Gs, jg.d_tab, P.d_tab, d_ends, d_sep, P.d_z, P.d_sg, (int)w.tab.size(), B, (size_t)ld, P.d_r, P.d_G0, s);
        return SLIDE_OK;
      },
      [&](int si, const GainCandDev* d_cd, const double* M) -> int { return P.finish(who, si, d_cd, M, prob, s, o); });
}

// ---- landmark pairs on the joint graph: are two landmarks, of one robot or of two, the same object? ------------------------------------
// HostGraph::landmark_pairs on the joint graph (obs_gate_kernels.hip's k_joint_lm_pair_fill has the invariant).  Pair k names the
// EXISTING landmarks (slot_a, cls, idx_a) and (slot_b, cls, idx_b) as the joint observation gate names a landmark; a shared landmark
// may be named through any replica and is read through its lowest one, so its two names give the same bits.  cov = false, the test:
// r = (est_b - est_a) / sigma at the members' device-resident estimates, C = I + G0 + W^T D W with L W = B on the pass's
// K = L D L^T, d2 = r^T C^-1 r by k_obs_gate_finish on the signed gram.  cov = true: 2 D unit columns per pair, whose signed gram
// plus the private sides' H_ll^-1 is [[Saa, Sab], [Sba, Sbb]] — between two robots the one landmark block the cached joint Sigma does
// not hold.  A PRIVATE side enters through its factors' poses in its own graph and its H_ll^-1; a SHARED side is a separator
// variable: -+I / sigma on its separator coordinates at sep_entry_row's row, nothing in G0.  Grouped by class, nk = D (2 D) columns
// per pair, 128 point / 54 cylinder pairs per sweep of the test; per sweep one fill launch, one walk of the whole forward half, the
// gram, the finish, one read-back; a pair's bits do not depend on the list.  status[k] (or null): SLIDE_MISSING (joint_lm_end's),
// SLIDE_ERR_INVALID (two names of one variable: one private landmark twice, or two replicas of one shared slot, told by their
// separator offset), SLIDE_ERR_NOT_SPD; zeros then.  Whole-call refusals: joint_state's, nothing written.  No route off the cached
// joint Sigma for pairs of one robot: every pair takes the substitution.  Nothing the pass reads is written; the cached joint Sigma is
// neither used nor touched.  Arguments checked by the caller.
int CholBatch::joint_landmark_pairs(bool cov, int n_q, const int32_t* cls, const int32_t* slot_a, const uint64_t* idx_a, const int32_t* slot_b,
                                    const uint64_t* idx_b, const double* sig3, const double* sig7, double* d2, int32_t* dof, double* C81,
                                    double* r9, double* out324, int32_t* status) {
  const char* who = cov ? "chol_batch_get_landmark_pair_covariances" : "chol_batch_landmark_pair_mahalanobis";
  std::lock_guard<std::mutex> pl(pass_mtx);
  int rc = joint_state(who, 0);
  if (rc != SLIDE_OK) return rc;
  JointGain jg;
  jg.build(*this, 0);
  struct Group { std::vector<int4> ends; std::vector<long long> sep; std::vector<int> ids; };
  Group groups[3];      // [SLIDE_CLS_*]
  for (int k = 0; k < n_q; ++k) {
    if (cov) {
      for (int e = 0; e < LM_PAIR_COV; ++e) out324[LM_PAIR_COV * (size_t)k + e] = 0.0;
    } else {
      d2[k] = 0.0;
      for (int e = 0; C81 && e < 81; ++e) C81[81 * (size_t)k + e] = 0.0;
      for (int e = 0; r9 && e < 9; ++e) r9[9 * (size_t)k + e] = 0.0;
      if (dof) dof[k] = landmark_dim(cls[k]);
    }
    JointLmEnd ea = joint_lm_end(jg, slot_a[k], cls[k], idx_a[k]), eb = joint_lm_end(jg, slot_b[k], cls[k], idx_b[k]);
    int ga = slot_a[k], gb = slot_b[k];
    int st = ea.l < 0 || eb.l < 0 ? SLIDE_MISSING : SLIDE_OK;
    if (st == SLIDE_OK) {
      const bool sha = ea.sep >= 0, shb = eb.sep >= 0;
      if (sha == shb && (sha ? ea.sep_off == eb.sep_off : (ga == gb && ea.l == eb.l))) st = SLIDE_ERR_INVALID;
    }
    if (status) status[k] = st;
    if (st != SLIDE_OK) continue;
    for (int side = 0; side < 2; ++side) {      // a shared landmark is read through its lowest replica
      JointLmEnd& e = side ? eb : ea;
      if (e.sep < 0) continue;
      for (int i = 0; i < (side ? gb : ga); ++i)
        if ((size_t)e.sh < graphs[i]->h_sh_lid.size() && graphs[i]->h_sh_lid[e.sh] >= 0 && (size_t)graphs[i]->h_sh_lid[e.sh] < graphs[i]->up_L) {
          (side ? gb : ga) = i; e.l = graphs[i]->h_sh_lid[e.sh];
          break;
        }
    }
    Group& g = groups[cls[k]];
    g.ends.push_back(make_int4(ga, ea.l, gb, eb.l)); g.sep.push_back(ea.sep); g.sep.push_back(eb.sep); g.ids.push_back(k);
  }
  hipStream_t s = master;
  for (int c = 0; c < 3; ++c) {
    const Group& g = groups[c];
    if (g.ids.empty()) continue;
    const int m = (int)g.ids.size(), D = landmark_dim(c), nk = cov ? 2 * D : D, max_nc = std::min(m, SLIDE_INFO_GAIN_SWEEP_COLS / nk);
    const size_t per_out = cov ? LM_PAIR_COV : OBS_GATE_OUT;
    LmPairSigma sg{};
    for (int i = 0; i < D && !cov; ++i) sg.s[i] = (D == 3 ? sig3 : sig7)[i];
    Scratch sc(s);
    int4* d_ends = sc.alloc<int4>(m);
    long long* d_sep = sc.alloc<long long>(2 * (size_t)m);
    double* d_r = sc.alloc<double>(9 * (size_t)max_nc);
    double* d_G0 = sc.alloc<double>(81 * (size_t)max_nc);
    double* d_out = sc.alloc<double>(per_out * (size_t)max_nc);
    int* d_flag = sc.alloc<int>(max_nc);
    if (!sc.ok()) { g_last_error = std::string(who) + ": out of device memory"; return SLIDE_ERR_HIP; }
    SL_HIP(sc.upload(d_ends, g.ends));
    SL_HIP(sc.upload(d_sep, g.sep));
    std::vector<double> h(per_out * (size_t)max_nc);
    std::vector<int> hflag(max_nc, 0);
    rc = joint_sigma_forms(
        who, jg, m, nk,
        [&](int k0, int nc, double* B, int ld) {
          launch_joint_lm_pair_fill(d_Gs, jg.d_tab, D, cov, d_ends + k0, d_sep + 2 * (size_t)k0, sg, nc, B, (size_t)ld, d_r, d_G0, s);
        },
        [&](int k0, int nc, const double* M) -> int {
          if (cov) launch_joint_lm_pair_cov_finish(d_Gs, D, d_ends + k0, d_sep + 2 * (size_t)k0, M, nc, d_out, s);
          else launch_obs_gate_finish(nk, M, d_G0, d_r, nc, d_out, d_flag, s);
          SL_HIP(hipGetLastError());
          SL_HIP(hipMemcpyAsync(h.data(), d_out, per_out * (size_t)nc * sizeof(double), hipMemcpyDeviceToHost, s));
          if (!cov) SL_HIP(hipMemcpyAsync(hflag.data(), d_flag, nc * sizeof(int), hipMemcpyDeviceToHost, s));
          SL_HIP(hipStreamSynchronize(s));
          for (int i = 0; i < nc; ++i) {
            const size_t k = (size_t)g.ids[k0 + i];
            const double* o = h.data() + per_out * (size_t)i;
            if (cov) { std::copy(o, o + LM_PAIR_COV, out324 + LM_PAIR_COV * k); continue; }
            if (hflag[i]) {
              if (status) status[k] = SLIDE_ERR_NOT_SPD;
              continue;
            }
            d2[k] = o[0];
            if (C81) std::copy(o + 1, o + 82, C81 + 81 * k);
            if (r9) std::copy(o + 82, o + 91, r9 + 9 * k);
          }
          return SLIDE_OK;
        });
    if (rc != SLIDE_OK) return rc;
  }
  return SLIDE_OK;
}
// HostGraph::landmark_pairs_within over the job's landmarks of one class: every member's private ones and each shared slot ONCE,
// through its lowest replica, in (slot, local index) order.  k_joint_lm_anchor_gather writes their anchors (point xyz, cube t,
// cylinder root of the members' device-resident lm_est) and a group word each — the member's slot for a private landmark, n + the
// shared slot for a shared one — into one contiguous array, on which the count / k_seg_scan / emit sequence runs; cross_only takes
// the group-inequality sibling, which drops the pairs whose two ends are private landmarks of one member (a shared slot's word is
// its own, so it pairs with anything).  Pairs come back as (slot, local index) of either end, sorted by position in that order.
// *n_pairs is always the total; above cap SLIDE_ERR_CAPACITY, nothing else written.  joint_state's refusals first.
int CholBatch::joint_landmark_pairs_within(int cls, double radius, bool cross_only, int64_t cap, int32_t* slot_a, uint64_t* idx_a, int32_t* slot_b,
                                           uint64_t* idx_b, double* dist, int64_t* n_pairs) {
  const char* who = "chol_batch_landmark_pairs_within";
  std::lock_guard<std::mutex> pl(pass_mtx);
  int rc = joint_state(who, 0);
  if (rc != SLIDE_OK) return rc;
  *n_pairs = 0;
  std::vector<int4> ent;      // {member graph, landmark, group word, .}
  std::vector<uint64_t> keys;
  const uint64_t tag = HostGraph::lm_key(cls, 0) >> 56;
  for (int i = 0; i < n; ++i) {
    const HostGraph* g = graphs[i];
    std::vector<std::pair<uint64_t, int>> all;
    for (const auto& kv : g->key2lm)
      if ((kv.first >> 56) == tag && (size_t)kv.second < g->up_L) all.emplace_back(kv.first & ((1ull << 56) - 1ull), kv.second);
    std::sort(all.begin(), all.end());
    for (const auto& e : all) {
      int sh = -1;
      for (size_t q = 0; q < g->h_sh_lid.size() && sh < 0; ++q)
        if (g->h_sh_lid[q] == e.second) sh = (int)q;
      bool lower = false;
      for (int j = 0; j < i && sh >= 0 && !lower; ++j)
        lower = (size_t)sh < graphs[j]->h_sh_lid.size() && graphs[j]->h_sh_lid[sh] >= 0 && (size_t)graphs[j]->h_sh_lid[sh] < graphs[j]->up_L;
      if (lower) continue;
      ent.push_back(make_int4(i, e.second, sh >= 0 ? n + sh : i, 0)); keys.push_back(e.first);
    }
  }
  const int m = (int)ent.size();
  if (m < 2) return SLIDE_OK;
  hipStream_t s = master;
  Scratch sc(s);
  int4* d_ent = sc.alloc<int4>(m);
  double* d_pts = sc.alloc<double>(3 * (size_t)m);
  int32_t* d_group = sc.alloc<int32_t>(m);
  if (!sc.ok()) { g_last_error = std::string(who) + ": out of device memory"; return SLIDE_ERR_HIP; }
  SL_HIP(sc.upload(d_ent, ent));
  launch_joint_lm_anchor_gather(d_Gs, d_ent, cls == SLIDE_CLS_CUBE ? 9 : 0, m, d_pts, d_group, s);
  std::vector<int32_t> vi, vj;
  std::vector<double> vd;
  rc = pairs_within_dev(who, s, d_pts, 3, nullptr, cross_only ? d_group : nullptr, m, radius, cap, vi, vj, vd, n_pairs, cross_only);
  if (rc != SLIDE_OK) return rc;
  for (size_t k = 0; k < vi.size(); ++k) {
    slot_a[k] = ent[vi[k]].x; idx_a[k] = keys[vi[k]];
    slot_b[k] = ent[vj[k]].x; idx_b[k] = keys[vj[k]];
    dist[k] = vd[k];
  }
  return SLIDE_OK;
}
}  // namespace sl
