// Host side of the CLIPPER clique solver: the CSR builders, THE one path to a projected-gradient clique solve (clq_job ->
// solve_csr_device for one problem, solve_csr_segments for a list of them), triangle matching, and the CLIPPER entry points of
// include/slide_gpu.h.  Users of the path: SlideGraph (host_slidegraph.hip) and loop-closure selection (host_closure.hip).
#include <cmath>

#include "host_clipper.hpp"

using namespace sl;

// CLIPPER::findDenseClique (clipper.cpp:172-323, DSD_HEU rounding) runs entirely on the device (clipper_kernels.hip): the host only
// draws the start weights, sizes the CSR (one prefix sum over the row counts) and rounds the result.
namespace sl {
double g_dev_ms[SLIDE_MS_COUNT];

// DSD_HEU rounding (clipper.cpp:302-310 with utils.cpp:33-55): the omega entries of u the reference's bounded min-heap scan keeps —
// an entry replaces the heap's smallest (value, index) pair only when its value is strictly larger — largest pair first.
static std::vector<int> top_entries(const std::vector<double>& x, int k) {
  std::vector<int> heap;                                   // indices, min-heap on (x[i], i)
  if (k < 1) return heap;
  auto greater = [&](int a, int b) { return x[a] > x[b] || (x[a] == x[b] && a > b); };
  for (int i = 0; i < (int)x.size(); ++i) {
    if ((int)heap.size() < k) { heap.push_back(i); std::push_heap(heap.begin(), heap.end(), greater); }
    else if (x[heap.front()] < x[i]) { std::pop_heap(heap.begin(), heap.end(), greater); heap.back() = i; std::push_heap(heap.begin(), heap.end(), greater); }
  }
  std::sort_heap(heap.begin(), heap.end(), greater);      // descending in the heap's order = largest pair first
  return heap;
}
static void default_u0(std::vector<double>& u) {             // fixed-seed splitmix64 -> U[0, 1)
  uint64_t x = 0x9E3779B97F4A7C15ull;
  for (double& v : u) {
    x += 0x9E3779B97F4A7C15ull;
    uint64_t z = x;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    v = (double)(z >> 11) * (1.0 / 9007199254740992.0);
  }
}

// row counts (device) -> row pointers on both sides + col / val allocated; nnz summed in 64 bits
// cap >= 0: more non-zeros than cap end the build with SLIDE_ERR_CAPACITY before col / val exist (h_ptr and nnz are set)
static int csr_scan_alloc(Tmp& T, const int* d_cnt, int n, DevCsr& S, long long cap = -1) {
  std::vector<int> cnt(n);
  S.h_ptr.assign((size_t)n + 1, 0);
  SL_HIP(hipMemcpy(cnt.data(), d_cnt, sizeof(int) * n, hipMemcpyDeviceToHost));
  long long nnz = 0;
  for (int i = 0; i < n; ++i) {
    nnz += cnt[i];
    if (nnz > INT32_MAX) { g_last_error = "affinity matrix has more than 2^31 non-zeros"; return SLIDE_ERR_CAPACITY; }
    S.h_ptr[i + 1] = (int)nnz;
  }
  S.nnz = nnz;
  if (cap >= 0 && nnz > cap) { g_last_error = "the CSR has " + std::to_string(nnz) + " non-zeros, the caller's buffers hold " + std::to_string(cap); return SLIDE_ERR_CAPACITY; }
  S.ptr = T.up(S.h_ptr.data(), (size_t)n + 1);
  S.col = T.up<int>(nullptr, (size_t)std::max<long long>(nnz, 1));
  S.val = T.up<double>(nullptr, (size_t)std::max<long long>(nnz, 1));
  if (!S.ptr || !S.col || !S.val) { g_last_error = "hipMalloc/hipMemcpy failed"; return SLIDE_ERR_HIP; }
  return SLIDE_OK;
}
// dM: device, n x n row-major upper-filled (n > 0)
static int csr_from_dense_device(Tmp& T, const double* dM, int n, DevCsr& S) {
  int* d_cnt = T.up<int>(nullptr, n);
  if (!d_cnt) { g_last_error = "hipMalloc failed"; return SLIDE_ERR_HIP; }
  {
    DevTimer tm(SLIDE_MS_CLQ_CSR);
    launch_clq_csr_count(dM, n, d_cnt, nullptr);
  }
  const int rc = csr_scan_alloc(T, d_cnt, n, S);
  if (rc != SLIDE_OK) return rc;
  {
    DevTimer tm(SLIDE_MS_CLQ_CSR, true);
    launch_clq_csr_fill(dM, n, S.ptr, S.col, S.val, nullptr);
  }
  g_dev_ms[SLIDE_MS_CLQ_NNZ] = (double)S.nnz;
  return SLIDE_OK;
}
// scorePairwiseConsistency clipper.cpp:21-65 ending in M_ = M.sparseView(): k_affinity_csr count, host scan, emit — nothing of size
// m^2.  d1 / d2 / dA: device copies of D1 / D2 / A (m > 0).  The points are gathered per association first (k_affinity_gather: 2 m dim
// doubles); SLIDE_AFFINITY_CSR_GATHER=0 in the environment reads them through A instead (the variant DESIGN.md 7 measures against;
// the same bits).
int csr_from_assoc_device(Tmp& T, const double* d1, const double* d2, int dim, const int32_t* dA, int m, double sigma, double epsilon,
                          double mindist, double affinityeps, DevCsr& S, long long cap) {
  int* d_cnt = T.up<int>(nullptr, m);
  double *p1 = nullptr, *p2 = nullptr;
  const char* e = getenv("SLIDE_AFFINITY_CSR_GATHER");
  if (!(e && e[0] == '0' && e[1] == 0)) {
    p1 = T.up<double>(nullptr, (size_t)m * dim);
    p2 = T.up<double>(nullptr, (size_t)m * dim);
    if (!p1 || !p2) { g_last_error = "hipMalloc failed"; return SLIDE_ERR_HIP; }
  }
  if (!d_cnt) { g_last_error = "hipMalloc failed"; return SLIDE_ERR_HIP; }
  {
    DevTimer tm(SLIDE_MS_AFFINITY_CSR);
    if (p1) launch_affinity_gather(d1, d2, dim, dA, m, p1, p2, nullptr);
    launch_affinity_csr(false, d1, d2, p1, p2, dim, dA, m, sigma, epsilon, mindist, affinityeps, d_cnt, nullptr, nullptr, nullptr, nullptr);
  }
  SL_HIP(hipGetLastError());
  const int rc = csr_scan_alloc(T, d_cnt, m, S, cap);
  if (rc != SLIDE_OK) return rc;
  {
    DevTimer tm(SLIDE_MS_AFFINITY_CSR, true);
    launch_affinity_csr(true, d1, d2, p1, p2, dim, dA, m, sigma, epsilon, mindist, affinityeps, nullptr, S.ptr, S.col, S.val, nullptr);
  }
  SL_HIP(hipGetLastError());
  g_dev_ms[SLIDE_MS_CLQ_NNZ] = (double)S.nnz;
  return SLIDE_OK;
}
// A (m x 2) names points of D1 (n1) and D2 (n2)
static int check_associations(const int32_t* A, int m, int n1, int n2) {
  for (int j = 0; j < m; ++j)
    if (A[2 * (size_t)j] < 0 || A[2 * (size_t)j] >= n1 || A[2 * (size_t)j + 1] < 0 || A[2 * (size_t)j + 1] >= n2) {
      g_last_error = "association " + std::to_string(j) + " names a point outside D1 / D2";
      return SLIDE_ERR_INVALID;
    }
  return SLIDE_OK;
}

// host-side check of a caller's CSR (before anything touches the device): rowptr from 0 and non-decreasing, columns inside [0, n),
// strictly ascending within a row and off the diagonal, every (i, j, v) with its (j, i, v)
static int check_symmetric_csr(const int32_t* rowptr, const int32_t* col, const double* val, int n) {
  auto bad = [](int row, const char* what) { g_last_error = "clipper CSR, row " + std::to_string(row) + ": " + what; return SLIDE_ERR_INVALID; };
  if (rowptr[0] != 0) return bad(0, "rowptr[0] is not 0");
  for (int i = 0; i < n; ++i)
    if (rowptr[i + 1] < rowptr[i]) return bad(i, "rowptr decreases");
  if (rowptr[n] > 0 && (!col || !val)) return bad(0, "col / val missing");
  for (int i = 0; i < n; ++i)
    for (int k = rowptr[i]; k < rowptr[i + 1]; ++k) {
      if (col[k] < 0 || col[k] >= n) return bad(i, "a column outside [0, n)");
      if (col[k] == i) return bad(i, "an entry on the diagonal");
      if (k > rowptr[i] && col[k] <= col[k - 1]) return bad(i, "columns not strictly ascending");
    }
  for (int i = 0; i < n; ++i)
    for (int k = rowptr[i]; k < rowptr[i + 1]; ++k) {
      const int j = col[k];
      const int32_t* lo = col + rowptr[j];
      const int32_t* hi = col + rowptr[j + 1];
      const int32_t* q = std::lower_bound(lo, hi, (int32_t)i);
      if (q == hi || *q != i) return bad(i, "an entry without its transpose");
      if (!(val[q - col] == val[k])) return bad(i, "an entry whose transpose holds another value");
    }
  return SLIDE_OK;
}

// Below this many rows one CU is quicker than a grid barrier per evaluation: a problem at or above it runs on several co-resident
// workgroups (solve_csr_device), one below it in one workgroup, and a list's problems below it share ONE launch (solve_csr_segments).
constexpr int CLQ_COOP_N = 1024;

// THE set-up of a clique job: the problem's CSR, its n rows, work = 6 n doubles [u | unew | g | gnew | Mu | Cu], the start weights and
// out4 on the device.  d_mc4n non-null: the cooperative kernel's layout (u alone in work, Mu / Cu in that buffer of 4 n doubles).
static ClqSolve clq_job(const DevCsr& S, int n, double* d_work, const double* d_u0, double* d_out4, const slide_clipper_params_t& P,
                        double* d_mc4n = nullptr) {
  ClqSolve A{};
  A.rowptr = S.ptr; A.col = S.col; A.val = S.val; A.n = n; A.u0 = d_u0;
  double* w = d_work;
  A.u = w;
  if (d_mc4n) { A.Mu = d_mc4n; A.Cu = d_mc4n + n; }
  else { A.unew = w + n; A.g = w + 2 * (size_t)n; A.gnew = w + 3 * (size_t)n; A.Mu = w + 4 * (size_t)n; A.Cu = w + 5 * (size_t)n; }
  A.tol_u = P.tol_u; A.tol_F = P.tol_F; A.beta = P.beta; A.eps = P.eps;
  A.maxin = P.maxiniters; A.maxol = P.maxoliters; A.maxls = P.maxlsiters; A.rescale = P.rescale_u0;
  A.out = d_out4;
  return A;
}

// findDenseClique on a device CSR (n > 0): the cooperative or the one-workgroup kernel, read-back, DSD_HEU rounding
static int g_clq_last_wgs = 1;          // workgroups the last single-problem solve ran on, and its gradient evaluations
static double g_clq_last_evals = 0.0;
int solve_csr_device(Tmp& T, const DevCsr& S, int n, const double* u0, const slide_clipper_params_t& P, std::vector<int>& nodes,
                     std::vector<double>& u, double& score) {
  nodes.clear();
  u.assign(n, 0.0);
  score = 0.0;
  std::vector<double> start(n);
  if (u0) start.assign(u0, u0 + n); else default_u0(start);
  double* d_u0 = T.up(start.data(), n);
  double* d_work = T.up<double>(nullptr, 6 * (size_t)n);
  double* d_out = T.up<double>(nullptr, 4);
  if (!d_u0 || !d_work || !d_out) { g_last_error = "hipMalloc/hipMemcpy failed"; return SLIDE_ERR_HIP; }
  // one large problem: the product's rows over several workgroups (4 rows per wave and product, at most 128 workgroups).
  // SLIDE_CLIPPER_WGS forces a count (1 = the one-workgroup kernel).
  int n_wg = n >= CLQ_COOP_N ? std::min(128, (n + 63) / 64) : 1;
  if (const char* e = getenv("SLIDE_CLIPPER_WGS")) { const int v = atoi(e); if (v >= 1) n_wg = std::min(v, 256); }
  g_clq_last_wgs = 1;
  bool done = false;
  DevTimer* solve_tm = nullptr;
  if (n_wg > 1) {
    double* d_priv = T.up<double>(nullptr, (size_t)n_wg * 4 * n);
    double* d_mc = T.up<double>(nullptr, 4 * (size_t)n);
    int* d_bar = T.up<int>(nullptr, 2);
    if (!d_priv || !d_mc || !d_bar) { g_last_error = "hipMalloc failed"; return SLIDE_ERR_HIP; }
    const ClqSolve A = clq_job(S, n, d_work, d_u0, d_out, P, d_mc);
    solve_tm = new DevTimer(SLIDE_MS_CLQ_SOLVE);
    done = launch_clq_solve_coop(A, d_priv, d_bar, n_wg, nullptr);
    if (done) g_clq_last_wgs = n_wg;
    else { delete solve_tm; solve_tm = nullptr; }
  }
  if (!done) {
    solve_tm = new DevTimer(SLIDE_MS_CLQ_SOLVE);
    launch_clq_solve(S.ptr, S.col, S.val, n, d_u0, d_work, P.tol_u, P.tol_F, P.beta, P.eps, P.maxiniters, P.maxoliters, P.maxlsiters,
                     P.rescale_u0, d_out, nullptr);
  }
  delete solve_tm;
  double out4[4];
  SL_HIP(hipMemcpy(out4, d_out, sizeof(out4), hipMemcpyDeviceToHost));
  if (out4[2] < 0.0) { g_last_error = "clipper: a grid barrier of the multi-workgroup solve timed out"; return SLIDE_ERR_HIP; }
  g_clq_last_evals = out4[2];
  SL_HIP(hipMemcpy(u.data(), d_work, sizeof(double) * n, hipMemcpyDeviceToHost));
  SL_HIP(hipGetLastError());
  score = out4[0];
  nodes = top_entries(u, (int)std::round(score));
  return SLIDE_OK;
}

// A list of problems (ClqSegments, host_clipper.hpp).  Host start weights of every segment below the threshold, ONE upload, ONE
// launch_clq_solve_batch + launch_clq_pack_u, ONE read-back of d_res; then segment after segment: rounding of what came back, or
// the single problem's route on the segment's slice of the shared buffers.
int solve_csr_segments(Tmp& T, const ClqSegments& G, const std::vector<const double*>& u0, const slide_clipper_params_t& P,
                       std::vector<double>& res, const ClqVisit& visit) {
  const int n_seg = G.n_seg, n_rows = G.off[n_seg];
  double* d_u = G.d_res + 4 * (size_t)n_seg;
  auto rows = [&](int s) { return G.off[s + 1] - G.off[s]; };
  auto batched = [&](int s) { return G.nnz0[s] >= 0 && rows(s) < CLQ_COOP_N; };
  auto slice = [&](int s) {
    DevCsr S;
    S.ptr = G.d_rptr + G.off[s] + s; S.col = G.d_col + G.nnz0[s]; S.val = G.d_val + G.nnz0[s]; S.nnz = G.tot[s];
    return S;
  };
  std::vector<double> start(n_rows, 0.0);
  int n_jobs = 0;
  for (int s = 0; s < n_seg; ++s) {
    if (!batched(s)) continue;
    std::vector<double> d(rows(s));
    if (u0[s]) d.assign(u0[s], u0[s] + rows(s)); else default_u0(d);
    std::copy(d.begin(), d.end(), start.begin() + G.off[s]);
    ++n_jobs;
  }
  if (n_jobs > 0) {
    double* d_start = T.up(start.data(), start.size());
    if (!d_start) { g_last_error = "hipMalloc/hipMemcpy failed"; return SLIDE_ERR_HIP; }
    std::vector<ClqSolve> jobs;
    for (int s = 0; s < n_seg; ++s)
      if (batched(s)) jobs.push_back(clq_job(slice(s), rows(s), G.d_work + 6 * (size_t)G.off[s], d_start + G.off[s], G.d_res + 4 * (size_t)s, P));
    ClqSolve* d_jobs = T.up(jobs.data(), jobs.size());
    if (!d_jobs) { g_last_error = "hipMalloc/hipMemcpy failed"; return SLIDE_ERR_HIP; }
    launch_clq_solve_batch(d_jobs, n_jobs, nullptr);
    launch_clq_pack_u(G.d_work, G.d_off, n_seg, n_rows, d_u, nullptr);
  }
  SL_HIP(hipGetLastError());
  res.assign(G.res_len, 0.0);
  SL_HIP(hipMemcpy(res.data(), G.d_res, sizeof(double) * G.res_len, hipMemcpyDeviceToHost));
  for (int s = 0; s < n_seg; ++s) {
    if (G.nnz0[s] < 0) continue;
    std::vector<int> nodes;
    std::vector<double> u;
    double sc = res[4 * (size_t)s];
    if (batched(s)) {
      u.assign(res.begin() + 4 * (size_t)n_seg + G.off[s], res.begin() + 4 * (size_t)n_seg + G.off[s + 1]);
      nodes = top_entries(u, (int)std::round(sc));
    } else {
      const int rc = solve_csr_device(T, slice(s), rows(s), u0[s], P, nodes, u, sc);
      if (rc != SLIDE_OK) return rc;
    }
    visit(s, nodes, u, sc);
  }
  return SLIDE_OK;
}
// dM: device, n x n row-major upper-filled.  Returns SLIDE_OK and fills nodes / u / score.
static int dense_clique_device(const double* dM, int n, const double* u0, const slide_clipper_params_t& P, std::vector<int>& nodes,
                        std::vector<double>& u, double& score) {
  nodes.clear();
  u.assign(n, 0.0);
  score = 0.0;
  if (n == 0) return SLIDE_OK;
  Tmp T;
  DevCsr S;
  const int rc = csr_from_dense_device(T, dM, n, S);
  if (rc != SLIDE_OK) return rc;
  return solve_csr_device(T, S, n, u0, P, nodes, u, score);
}

// semantic_clipper.cpp:122-138; see the oracle's note on the reflection branch
void estimate_tf2d(const double* a, const double* b, int n, double* tf3) {
  double ca[2] = {0, 0}, cb[2] = {0, 0};
  for (int i = 0; i < n; ++i) { ca[0] += a[2 * i]; ca[1] += a[2 * i + 1]; cb[0] += b[2 * i]; cb[1] += b[2 * i + 1]; }
  for (int k = 0; k < 2; ++k) { ca[k] /= n; cb[k] /= n; }
  double H[4] = {0, 0, 0, 0};
  for (int i = 0; i < n; ++i) {
    const double ax = a[2 * i] - ca[0], ay = a[2 * i + 1] - ca[1], bx = b[2 * i] - cb[0], by = b[2 * i + 1] - cb[1];
    H[0] += ax * bx; H[1] += ax * by; H[2] += ay * bx; H[3] += ay * by;
  }
  // V U^T of H = U S V^T maximises trace(R H) over orthogonal R: a rotation when det H >= 0, else a reflection whose
  // column 1 the reference negates (:130-132) — which yields the rotation by the reflection's own angle.
  const double detH = H[0] * H[3] - H[1] * H[2];
  const double th = detH >= 0.0 ? std::atan2(H[1] - H[2], H[0] + H[3]) : std::atan2(H[1] + H[2], H[0] - H[3]);
  const double c = std::cos(th), s = std::sin(th);
  tf3[0] = c; tf3[1] = -s; tf3[2] = cb[0] - (c * ca[0] - s * ca[1]);
  tf3[3] = s; tf3[4] = c; tf3[5] = cb[1] - (s * ca[0] + c * ca[1]);
  tf3[6] = 0; tf3[7] = 0; tf3[8] = 1;
}

// device-side triangle matching: returns pairs in d_pts (12 doubles per pair) / d_diffs, count in np
int match_triangles_device(Tmp& T, const double* tri_model, int ntm, const double* tri_data, int ntd, double thr, double** d_pts,
                           double** d_diffs, long long* np) {
  *np = 0; *d_pts = nullptr; *d_diffs = nullptr;
  if (ntm <= 0 || ntd <= 0) return SLIDE_OK;
  double* dtm = T.up(tri_model, 6 * (size_t)ntm);
  double* dtd = T.up(tri_data, 6 * (size_t)ntd);
  double* sdm = T.up<double>(nullptr, 3 * (size_t)ntm);
  double* sxm = T.up<double>(nullptr, 6 * (size_t)ntm);
  double* sdd = T.up<double>(nullptr, 3 * (size_t)ntd);
  double* sxd = T.up<double>(nullptr, 6 * (size_t)ntd);
  int* dcnt = T.up<int>(nullptr, ntm);
  long long* doff = T.up<long long>(nullptr, ntm);
  if (!dtm || !dtd || !sdm || !sxm || !sdd || !sxd || !dcnt || !doff) { g_last_error = "hipMalloc/hipMemcpy failed"; return SLIDE_ERR_HIP; }
  {
    DevTimer tm(SLIDE_MS_TRI_MATCH);
    launch_tri_prepare(dtm, ntm, sdm, sxm, nullptr);
    launch_tri_prepare(dtd, ntd, sdd, sxd, nullptr);
    launch_tri_match(false, sdm, sxm, ntm, sdd, sxd, ntd, thr, dcnt, nullptr, nullptr, nullptr, nullptr);
  }
  g_dev_ms[SLIDE_MS_TRI_PAIRS] = (double)ntm * (double)ntd;
  std::vector<int> cnt(ntm);
  SL_HIP(hipMemcpy(cnt.data(), dcnt, sizeof(int) * ntm, hipMemcpyDeviceToHost));
  std::vector<long long> off(ntm);
  long long tot = 0;
  for (int i = 0; i < ntm; ++i) { off[i] = tot; tot += cnt[i]; }
  *np = tot;
  if (tot == 0) return SLIDE_OK;
  SL_HIP(hipMemcpy(doff, off.data(), sizeof(long long) * ntm, hipMemcpyHostToDevice));
  *d_pts = T.up<double>(nullptr, 12 * (size_t)tot);
  *d_diffs = T.up<double>(nullptr, (size_t)tot);
  if (!*d_pts || !*d_diffs) { g_last_error = "hipMalloc failed"; return SLIDE_ERR_HIP; }
  {
    DevTimer tm(SLIDE_MS_TRI_MATCH, true);
    launch_tri_match(true, sdm, sxm, ntm, sdd, sxd, ntd, thr, dcnt, doff, *d_pts, *d_diffs, nullptr);
  }
  SL_HIP(hipGetLastError());
  return SLIDE_OK;
}
}  // namespace sl

static int clique_out(int rc, int n, const std::vector<int>& nodes, const std::vector<double>& u, double sc, int32_t* nodes_out, int* n_nodes,
                      double* u_out, double* score) {
  if (rc != SLIDE_OK) return rc;
  *n_nodes = (int)nodes.size();
  for (size_t i = 0; i < nodes.size(); ++i) nodes_out[i] = nodes[i];
  if (u_out) for (int i = 0; i < n; ++i) u_out[i] = u[i];
  if (score) *score = sc;
  return SLIDE_OK;
}

extern "C" {
int slide_clipper_affinity(const double* D1, int n1, const double* D2, int n2, int dim, const int32_t* A, int m, double sigma,
                           double epsilon, double mindist, double affinityeps, double* M_out) {
  if (slide_device_check(-1) != SLIDE_OK) return SLIDE_ERR_HIP;
  if (m <= 0) return SLIDE_OK;
  Tmp T;
  double* d1 = T.up(D1, (size_t)n1 * dim);
  double* d2 = T.up(D2, (size_t)n2 * dim);
  int32_t* dA = T.up(A, 2 * (size_t)m);
  double* dM = T.up<double>(nullptr, (size_t)m * m);
  if (!d1 || !d2 || !dA || !dM) { g_last_error = "hipMalloc/hipMemcpy failed"; return SLIDE_ERR_HIP; }
  {
    DevTimer tm(SLIDE_MS_AFFINITY);
    launch_clipper_affinity(d1, d2, dim, dA, m, sigma, epsilon, mindist, affinityeps, dM, nullptr);
  }
  SL_HIP(hipMemcpy(M_out, dM, (size_t)m * m * sizeof(double), hipMemcpyDeviceToHost));
  SL_HIP(hipGetLastError());
  return SLIDE_OK;
}

void slide_clipper_default_params(slide_clipper_params_t* p) {
  p->tol_u = 1e-8; p->tol_F = 1e-9; p->maxiniters = 200; p->maxoliters = 1000; p->beta = 0.25; p->maxlsiters = 99;
  p->eps = 1e-9; p->affinityeps = 1e-4; p->rescale_u0 = 1; p->sigma = 0.01; p->epsilon = 0.06; p->mindist = 0.0;
}

int slide_clipper_dense_clique(const double* M_upper, int n, const double* u0, const slide_clipper_params_t* p,
                               int32_t* nodes_out, int* n_nodes, double* u_out, double* score) {
  if (slide_device_check(-1) != SLIDE_OK) return SLIDE_ERR_HIP;
  if (n < 0 || !n_nodes) return SLIDE_ERR_INVALID;
  const slide_clipper_params_t P = clipper_params_or_default(p);
  Tmp T;
  double* dM = T.up(M_upper, (size_t)n * n);
  if (n > 0 && !dM) { g_last_error = "hipMalloc/hipMemcpy failed"; return SLIDE_ERR_HIP; }
  std::vector<int> nodes;
  std::vector<double> u;
  double sc = 0;
  const int rc = dense_clique_device(dM, n, u0, P, nodes, u, sc);
  return clique_out(rc, n, nodes, u, sc, nodes_out, n_nodes, u_out, score);
}

int slide_clipper_affinity_csr(const double* D1, int n1, const double* D2, int n2, int dim, const int32_t* A, int m, double sigma,
                               double epsilon, double mindist, double affinityeps, int32_t* rowptr_out, int32_t* col_out, double* val_out,
                               long long cap, long long* nnz) {
  if (m < 0 || dim < 1 || n1 < 0 || n2 < 0 || cap < 0 || !nnz || !rowptr_out || (m > 0 && (!A || !D1 || !D2))) return SLIDE_ERR_INVALID;
  *nnz = 0;
  if (m > (1 << 30)) { g_last_error = "more than 2^30 associations"; return SLIDE_ERR_CAPACITY; }
  int rc = check_associations(A, m, n1, n2);
  if (rc != SLIDE_OK) return rc;
  if (slide_device_check(-1) != SLIDE_OK) return SLIDE_ERR_HIP;
  rowptr_out[0] = 0;
  if (m == 0) return SLIDE_OK;
  Tmp T;
  double* d1 = T.up(D1, (size_t)n1 * dim);
  double* d2 = T.up(D2, (size_t)n2 * dim);
  int32_t* dA = T.up(A, 2 * (size_t)m);
  if (!d1 || !d2 || !dA) { g_last_error = "hipMalloc/hipMemcpy failed"; return SLIDE_ERR_HIP; }
  DevCsr S;
  rc = csr_from_assoc_device(T, d1, d2, dim, dA, m, sigma, epsilon, mindist, affinityeps, S, cap);
  if (S.nnz >= 0) {          // the scan finished: counts and pointers are valid
    *nnz = S.nnz;
    for (int i = 0; i <= m; ++i) rowptr_out[i] = S.h_ptr[i];
  }
  if (rc != SLIDE_OK) return rc;
  if (S.nnz > 0) {
    if (!col_out || !val_out) return SLIDE_ERR_INVALID;
    SL_HIP(hipMemcpy(col_out, S.col, sizeof(int32_t) * (size_t)S.nnz, hipMemcpyDeviceToHost));
    SL_HIP(hipMemcpy(val_out, S.val, sizeof(double) * (size_t)S.nnz, hipMemcpyDeviceToHost));
  }
  return SLIDE_OK;
}

int slide_clipper_dense_clique_csr(const int32_t* rowptr, const int32_t* col, const double* val, int n, const double* u0,
                                   const slide_clipper_params_t* p, int32_t* nodes_out, int* n_nodes, double* u_out, double* score) {
  if (n < 0 || !n_nodes || !rowptr || (n > 0 && !nodes_out)) return SLIDE_ERR_INVALID;
  int rc = check_symmetric_csr(rowptr, col, val, n);
  if (rc != SLIDE_OK) return rc;
  if (slide_device_check(-1) != SLIDE_OK) return SLIDE_ERR_HIP;
  const slide_clipper_params_t P = clipper_params_or_default(p);
  std::vector<int> nodes;
  std::vector<double> u;
  double sc = 0;
  if (n > 0) {
    Tmp T;
    DevCsr S;
    S.nnz = rowptr[n];
    S.ptr = T.up(rowptr, (size_t)n + 1);
    S.col = T.up(col, (size_t)S.nnz);
    S.val = T.up(val, (size_t)S.nnz);
    if (!S.ptr || !S.col || !S.val) { g_last_error = "hipMalloc/hipMemcpy failed"; return SLIDE_ERR_HIP; }
    g_dev_ms[SLIDE_MS_CLQ_NNZ] = (double)S.nnz;
    rc = solve_csr_device(T, S, n, u0, P, nodes, u, sc);
  }
  return clique_out(rc, n, nodes, u, sc, nodes_out, n_nodes, u_out, score);
}

int slide_clipper_match(const double* D1, int n1, const double* D2, int n2, int dim, const int32_t* A, int m, const double* u0,
                        const slide_clipper_params_t* p, int32_t* nodes_out, int* n_nodes, double* u_out, double* score) {
  if (m < 0 || dim < 1 || n1 < 0 || n2 < 0 || !n_nodes || (m > 0 && (!A || !D1 || !D2 || !nodes_out))) return SLIDE_ERR_INVALID;
  if (m > (1 << 30)) { g_last_error = "more than 2^30 associations"; return SLIDE_ERR_CAPACITY; }
  int rc = check_associations(A, m, n1, n2);
  if (rc != SLIDE_OK) return rc;
  if (slide_device_check(-1) != SLIDE_OK) return SLIDE_ERR_HIP;
  const slide_clipper_params_t P = clipper_params_or_default(p);
  std::vector<int> nodes;
  std::vector<double> u;
  double sc = 0;
  if (m > 0) {
    Tmp T;
    double* d1 = T.up(D1, (size_t)n1 * dim);
    double* d2 = T.up(D2, (size_t)n2 * dim);
    int32_t* dA = T.up(A, 2 * (size_t)m);
    if (!d1 || !d2 || !dA) { g_last_error = "hipMalloc/hipMemcpy failed"; return SLIDE_ERR_HIP; }
    DevCsr S;
    rc = csr_from_assoc_device(T, d1, d2, dim, dA, m, P.sigma, P.epsilon, P.mindist, P.affinityeps, S);
    if (rc == SLIDE_OK) rc = solve_csr_device(T, S, m, u0, P, nodes, u, sc);
  }
  return clique_out(rc, m, nodes, u, sc, nodes_out, n_nodes, u_out, score);
}

int slide_last_device_ms(int what, double* out) {
  if (what < 0 || what >= SLIDE_MS_COUNT || !out) return SLIDE_ERR_INVALID;
  *out = g_dev_ms[what];
  return SLIDE_OK;
}
void slide_clipper_last_solve_info(int* n_workgroups, double* grad_evals) {
  if (n_workgroups) *n_workgroups = g_clq_last_wgs;
  if (grad_evals) *grad_evals = g_clq_last_evals;
}

// Several dense-clique problems at once (the robot pairs of a multi-robot job: 28 at eight robots; semantic_clipper.cpp:227-235
// once per pair): the CSR builds are issued one after the other, the projected-gradient solves run as ONE launch, a persistent
// workgroup per job.  Job j: M_upper[j] (n[j] x n[j], row-major, upper triangle used), u0[j] or NULL (the default start);
// nodes_out[j] (>= n[j] ints), u_out[j] (n[j] doubles, may be NULL), n_nodes[j], score[j].  Results equal n_jobs single calls.
int slide_clipper_dense_clique_batch(int n_jobs, const double* const* M_upper, const int* n, const double* const* u0, const slide_clipper_params_t* p,
                                     int32_t* const* nodes_out, int* n_nodes, double* const* u_out, double* score) {
  if (slide_device_check(-1) != SLIDE_OK) return SLIDE_ERR_HIP;
  if (n_jobs < 0 || (n_jobs > 0 && (!M_upper || !n || !nodes_out || !n_nodes))) return SLIDE_ERR_INVALID;
  const slide_clipper_params_t P = clipper_params_or_default(p);
  Tmp T;
  std::vector<ClqSolve> jobs(n_jobs, ClqSolve{});      // (an empty problem keeps its place in the launch: n = 0)
  std::vector<double*> d_work(n_jobs, nullptr), d_out(n_jobs, nullptr);
  for (int j = 0; j < n_jobs; ++j) {
    const int nj = n[j];
    if (nj < 0) return SLIDE_ERR_INVALID;
    n_nodes[j] = 0;
    if (score) score[j] = 0.0;
    if (nj == 0) continue;
    double* dM = T.up(M_upper[j], (size_t)nj * nj);
    std::vector<double> start(nj);
    if (u0 && u0[j]) start.assign(u0[j], u0[j] + nj); else default_u0(start);
    int* d_cnt = T.up<int>(nullptr, nj);
    double* d_u0 = T.up(start.data(), nj);
    d_work[j] = T.up<double>(nullptr, 6 * (size_t)nj);
    d_out[j] = T.up<double>(nullptr, 4);
    if (!dM || !d_cnt || !d_u0 || !d_work[j] || !d_out[j]) { g_last_error = "hipMalloc/hipMemcpy failed"; return SLIDE_ERR_HIP; }
    // csr_from_dense_device without its timer: this call leaves slide_last_device_ms as it found it
    launch_clq_csr_count(dM, nj, d_cnt, nullptr);
    DevCsr S;
    const int rc = csr_scan_alloc(T, d_cnt, nj, S);
    if (rc != SLIDE_OK) return rc;
    launch_clq_csr_fill(dM, nj, S.ptr, S.col, S.val, nullptr);
    jobs[j] = clq_job(S, nj, d_work[j], d_u0, d_out[j], P);
  }
  if (n_jobs > 0) {
    ClqSolve* d_jobs = T.up(jobs.data(), (size_t)n_jobs);
    if (!d_jobs) { g_last_error = "hipMalloc/hipMemcpy failed"; return SLIDE_ERR_HIP; }
    launch_clq_solve_batch(d_jobs, n_jobs, nullptr);
    SL_HIP(hipDeviceSynchronize());
    SL_HIP(hipGetLastError());
  }
  for (int j = 0; j < n_jobs; ++j) {
    const int nj = n[j];
    if (nj == 0) continue;
    double out4[4];
    std::vector<double> u(nj);
    SL_HIP(hipMemcpy(out4, d_out[j], sizeof(out4), hipMemcpyDeviceToHost));
    SL_HIP(hipMemcpy(u.data(), d_work[j], sizeof(double) * nj, hipMemcpyDeviceToHost));
    clique_out(SLIDE_OK, nj, top_entries(u, (int)std::round(out4[0])), u, out4[0], nodes_out[j], &n_nodes[j], u_out ? u_out[j] : nullptr,
               score ? &score[j] : nullptr);
  }
  return SLIDE_OK;
}

int slide_estimate_tf2d(const double* a_xy, const double* b_xy, int n, double tf3[9]) {
  if (n <= 0) return SLIDE_ERR_INVALID;
  estimate_tf2d(a_xy, b_xy, n, tf3);
  return SLIDE_OK;
}

}  // extern "C"
