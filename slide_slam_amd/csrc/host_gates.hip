// The covariance-weighted queries built on the quadratic forms B^T Sigma B, on one graph and on the exact joint multi-robot graph: the
// joint marginal of pose pairs, the closure and observation gates, joint compatibility, landmark pairs, and the fixed-radius pair
// search that proposes the pairs — the host side of closure_kernels.hip, obs_gate_kernels.hip, obs_joint_kernels.hip and
// pairs_kernels.hip (the classes are declared in host_graph.hpp; the selected inverse and the joint tree: host_marginals.hip).
#include "host_sigma.hpp"

#include <cmath>
#include <functional>

namespace sl {

// ---- where the results of a list of candidates go ---------------------------------------------------------------------------------------
// The caller's arrays of one call and the read-back of a sweep.  What a sweep leaves on the device is one record per candidate: of a
// test {d2, C (D x D, row-major), r (D)} — GATE_OUT with D = 6, OBS_GATE_OUT with D = 9 — and a flag word, set where C is not positive
// definite; of a covariance query the plain block of `rec` doubles, no flag.  The contract of every such call is kept here: a
// candidate that is not served (refused on the host, or flagged) has zeros in its outputs and its status word set; dof is written
// for served and refused candidates alike; C, r, dof and status may be null, and this is the only place that asks.
struct GateSink {
  const char* who;
  double *d2 = nullptr, *C = nullptr, *r = nullptr, *block = nullptr;
  int32_t *dof = nullptr, *status = nullptr;
  size_t D = 0, rec = 0;
  bool flag = false;
  // per group of sweeps, from the query's scratch: the records and flags of a sweep and, for the fills that linearise, the
  // residuals d_r (9 per candidate) and the landmarks' own terms d_G0 (81 per candidate)
  double *d_out = nullptr, *d_r = nullptr, *d_G0 = nullptr;
  int* d_flag = nullptr;
  std::vector<double> h;
  std::vector<int> hflag;
  static GateSink test(const char* who, int D, double* d2, double* C, double* r, int32_t* dof, int32_t* status) {
    GateSink k{who};
    k.d2 = d2; k.C = C; k.r = r; k.dof = dof; k.status = status;
    k.D = D; k.rec = 1 + (size_t)D * D + D; k.flag = true;
    return k;
  }
  static GateSink blocks(const char* who, size_t rec, double* block, int32_t* status) {
    GateSink k{who};
    k.block = block; k.status = status; k.rec = rec;
    return k;
  }
  // candidate k before it is resolved: zeros, its dof, SLIDE_OK
  void clear(size_t k, int dof_k = 0) {
    for (size_t e = 0; block && e < rec; ++e) block[rec * k + e] = 0.0;
    if (d2) d2[k] = 0.0;
    for (size_t e = 0; C && e < D * D; ++e) C[D * D * k + e] = 0.0;
    for (size_t e = 0; r && e < D; ++e) r[D * k + e] = 0.0;
    if (dof) dof[k] = dof_k;
    refuse(k, SLIDE_OK);
  }
  void refuse(size_t k, int st) { if (status) status[k] = st; }
  int alloc(Scratch& sc, int max_nc, bool lin) {
    if (lin) { d_r = sc.alloc<double>(9 * (size_t)max_nc); d_G0 = sc.alloc<double>(81 * (size_t)max_nc); }
    d_out = sc.alloc<double>(rec * (size_t)max_nc);
    if (flag) d_flag = sc.alloc<int>(max_nc);
    if (!sc.ok()) { g_last_error = std::string(who) + ": out of device memory"; return SLIDE_ERR_HIP; }
    return SLIDE_OK;
  }
  // Behind a sweep's last launch: the records of its nc candidates (src; the caller's candidate of record i is ids[i]) and their
  // flags to the host, the sweep's ONE synchronise, and the scatter into the caller's arrays
  int read_back(hipStream_t s, const int* ids, int nc, const double* src) {
    h.resize(rec * (size_t)nc);
    hflag.resize(flag ? nc : 0);
    SL_HIP(hipGetLastError());
    SL_HIP(hipMemcpyAsync(h.data(), src, h.size() * sizeof(double), hipMemcpyDeviceToHost, s));
    if (flag) SL_HIP(hipMemcpyAsync(hflag.data(), d_flag, nc * sizeof(int), hipMemcpyDeviceToHost, s));
    SL_HIP(hipStreamSynchronize(s));
    for (int i = 0; i < nc; ++i) {
      const size_t k = (size_t)ids[i];
      const double* o = h.data() + rec * (size_t)i;
      if (!flag) { std::copy(o, o + rec, block + rec * k); continue; }
      if (hflag[i]) { refuse(k, SLIDE_ERR_NOT_SPD); continue; }
      d2[k] = o[0];
      if (C) std::copy(o + 1, o + 1 + D * D, C + D * D * k);
      if (r) std::copy(o + 1 + D * D, o + rec, r + D * k);
    }
    return SLIDE_OK;
  }
  int read_back(hipStream_t s, const int* ids, int nc) { return read_back(s, ids, nc, d_out); }
};
static_assert(GATE_OUT == 1 + 36 + 6 && OBS_GATE_OUT == 1 + 81 + 9, "a test's record is {d2, C, r}");

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
    gram_jobs(jobs, i, nk, nsplit);
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
  GateSink sink = GateSink::blocks("get_pose_pair_covariances", 144, out144n, status);
  std::vector<int32_t> as, bs;
  std::vector<int> ids;
  for (int k = 0; k < n; ++k) {
    sink.clear(k);
    const int a = pose_id(robot_a[k], idx_a[k]), b = pose_id(robot_b[k], idx_b[k]);
    if (a < 0 || b < 0 || a == b) { sink.refuse(k, a < 0 || b < 0 ? SLIDE_MISSING : SLIDE_ERR_INVALID); continue; }
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
  return sigma_forms(
      sink.who, (int)ids.size(), 12,
      [&](int k0, int nc, double* B, int nT) { launch_pair_identity(d_as + k0, d_bs + k0, nc, nullptr, B, nT, s); },
      [&](int k0, int nc, const double* M) -> int { return sink.read_back(s, ids.data() + k0, nc, M); });
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
  GateSink sink = GateSink::test("closure_mahalanobis", 6, d2, C36, r6, nullptr, status);
  std::vector<int32_t> fs, ts;
  std::vector<double> z, sg;
  std::vector<int> ids;
  for (int k = 0; k < L; ++k) {
    sink.clear(k);
    const int a = pose_id(from_robot[k], from_idx[k]), b = pose_id(to_robot[k], to_idx[k]);
    if (a < 0 || b < 0 || a == b) { sink.refuse(k, a < 0 || b < 0 ? SLIDE_MISSING : SLIDE_ERR_INVALID); continue; }
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
  double* d_r = sc.alloc<double>(6 * (size_t)m);      // (by the closure's place in the list, not in its sweep)
  if ((rc = sink.alloc(sc, max_nc, false)) != SLIDE_OK) return rc;
  SL_HIP(sc.upload(d_fs, fs));
  SL_HIP(sc.upload(d_ts, ts));
  SL_HIP(sc.upload(d_z, z));
  SL_HIP(sc.upload(d_sg, sg));
  return sigma_forms(
      sink.who, m, 6,
      [&](int k0, int nc, double* B, int nT) {
        launch_closure_gate_lin(d_pose_est.d, d_fs + k0, d_ts + k0, d_z + 12 * (size_t)k0, d_sg + 6 * (size_t)k0, nc, G.chart, nullptr, B, nT,
                                d_r + 6 * (size_t)k0, s);
      },
      [&](int k0, int nc, const double* M) -> int {
        launch_closure_gate_finish(M, d_r + 6 * (size_t)k0, nc, sink.d_out, sink.d_flag, s);
        return sink.read_back(s, ids.data() + k0, nc);
      });
}
// The factor type of a landmark class (returned), and z and the sigmas of the observation meas17 describes, by the add calls' own
// text under THIS graph's parameters (br_meas / cube_meas / cyl_meas; bearing_range_sigma, noise_model_cube_vec x max(|loc.t|, 0.1),
// cylinder_sigma) — on the joint graph, the graph of the candidate's pose
int HostGraph::obs_measurement(int cls, const double* a, double* z15, double* sigma9) const {
  if (cls == SLIDE_CLS_ELLIPSOID) {
    br_meas(a, a[3], z15);
    for (int i = 0; i < 3; ++i) sigma9[i] = P.bearing_range_sigma;
    return FT_BR;
  }
  if (cls == SLIDE_CLS_CUBE) {
    cube_meas(from7(a), from7(a + 7), a + 14, z15, sigma9);
    return FT_CUBE;
  }
  cyl_meas(from7(a), a + 7, a + 10, a[13], z15);
  for (int i = 0; i < 7; ++i) sigma9[i] = P.cylinder_sigma;
  return FT_CYL;
}
// What the observation gates resolve of a candidate before the device is asked: its pose and landmark ids (SLIDE_MISSING for a pose
// or landmark the graph does not hold, or a landmark without a factor), its class's factor type, z and the sigmas
HostGraph::ObsCand HostGraph::obs_candidate(int robot, uint64_t pose_idx, int cls, uint64_t lm_idx, const double* a) const {
  ObsCand c;
  c.p = pose_id(robot, pose_idx);
  c.l = lm_lid(cls, lm_idx);
  c.st = c.p < 0 || c.l < 0 || lm_fids[c.l].empty() ? SLIDE_MISSING : SLIDE_OK;
  if (c.st == SLIDE_OK) c.type = obs_measurement(cls, a, c.z, c.sg);
  return c;
}
// The block column at which a sweep starts its forward substitution: that of the lowest pose `lo` its candidates touch.
// (SLIDE_OBS_GATE_FULL_WALK=1, a measurement aid: column 0.)
int HostGraph::walk_start(int lo) const {
  const char* fw = std::getenv("SLIDE_OBS_GATE_FULL_WALK");
  if (fw && fw[0] == '1') return 0;
  return std::min((6 * lo) / NB, G.T - 1);
}
// (of n observation candidates: their poses and their landmarks' first observers)
int HostGraph::obs_walk_start(const int32_t* pid, const int32_t* lid, int n) const {
  int lo = 1 << 30;
  for (int i = 0; i < n; ++i) lo = std::min(lo, std::min((int)pid[i], h_lm_first[lid[i]]));
  return walk_start(lo);
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
  return obs_gate("observation_mahalanobis", nullptr, 0, 0, n, robot, pose_idx, cls, lm_idx, meas17, d2, dof, C81, r9, status);
}
// The same gate at a PREDICTED pose, as an EKF gates at the predicted state (obs_gate_kernels.hip, k_obs_gate_lin_pred, has the
// identity).  The n candidates sit at est7, the value add_keypose_between(robot, from_idx, ., rel7, est7) would give a new pose n; the
// Between factor's sigmas are that call's own, noise_model_odom_vec x max(|t_rel|, noise_floor).  The result is the gate
// observation_mahalanobis would compute on the graph extended by pose n and that factor, linearised at those values: no add, no
// factorisation, the graph untouched.  Candidates resolve as obs_candidate resolves them at pose (robot, from_idx) — the pose whose
// rows of B they enter through — are grouped, swept and finished as above, and a sweep's walk starts at the block column of
// min(from pose, the landmarks' first observers).  A from pose the graph does not hold: SLIDE_MISSING, nothing written; then
// marginal_state's refusals.  Arguments checked by the caller.
int HostGraph::predicted_observation_mahalanobis(int robot, uint64_t from_idx, const double* rel7, const double* est7, int n, const int32_t* cls,
                                                 const uint64_t* lm_idx, const double* meas17, double* d2, int32_t* dof, double* C81, double* r9,
                                                 int32_t* status) {
  const char* who = "predicted_observation_mahalanobis";
  if (pose_id(robot, from_idx) < 0) { g_last_error = std::string(who) + ": the from pose is not in the graph"; return SLIDE_MISSING; }
  PredPoseDev pred{};
  to12(from7(est7), pred.x);
  const double dist = std::max(norm(from7(rel7).t), P.noise_floor);      // (add_keypose_between's own text)
  for (int i = 0; i < 6; ++i) { const double sg = P.noise_model_odom_vec[i] * dist; pred.s2[i] = sg * sg; }
  return obs_gate(who, &pred, robot, from_idx, n, nullptr, nullptr, cls, lm_idx, meas17, d2, dof, C81, r9, status);
}
// (the two gates' one body.  pred == null: candidate k at the graph's pose (robot[k], pose_idx[k]); else every candidate at the
// predicted pose *pred behind the graph's pose (pred_robot, pred_from), whose id this fills into pred->k once the state is checked)
int HostGraph::obs_gate(const char* who, PredPoseDev* pred, int pred_robot, uint64_t pred_from, int n, const int32_t* robot,
                        const uint64_t* pose_idx, const int32_t* cls, const uint64_t* lm_idx, const double* meas17, double* d2, int32_t* dof,
                        double* C81, double* r9, int32_t* status) {
  int rc = marginal_state(who);
  if (rc != SLIDE_OK) return rc;
  if (pred) pred->k = pose_id(pred_robot, pred_from);
  GateSink sink = GateSink::test(who, 9, d2, C81, r9, dof, status);
  struct Group { int type = 0; std::vector<int32_t> pid, lid; std::vector<double> z, sg; std::vector<int> ids; };
  Group groups[3];
  groups[0].type = FT_BR; groups[1].type = FT_CUBE; groups[2].type = FT_CYL;
  for (int k = 0; k < n; ++k) {
    sink.clear(k, landmark_dim(cls[k]));
    const ObsCand c = obs_candidate(pred ? pred_robot : robot[k], pred ? pred_from : pose_idx[k], cls[k], lm_idx[k], meas17 + 17 * (size_t)k);
    if (c.st != SLIDE_OK) { sink.refuse(k, c.st); continue; }
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
    if ((rc = sink.alloc(sc, max_nc, true)) != SLIDE_OK) return rc;
    SL_HIP(sc.upload(d_pid, g.pid));
    SL_HIP(sc.upload(d_lid, g.lid));
    SL_HIP(sc.upload(d_z, g.z));
    SL_HIP(sc.upload(d_sg, g.sg));
    rc = sigma_forms(
        sink.who, m, nk,
        [&](int k0, int nc, double* B, int nT) {
          if (pred) launch_obs_gate_lin_pred(G, g.type, *pred, d_lid + k0, d_z + 15 * (size_t)k0, d_sg + 9 * (size_t)k0, nc, B, nT, sink.d_r, sink.d_G0, s);
          else launch_obs_gate_lin(G, g.type, d_pid + k0, d_lid + k0, d_z + 15 * (size_t)k0, d_sg + 9 * (size_t)k0, nc, B, nT, sink.d_r, sink.d_G0, s);
        },
        [&](int k0, int nc, const double* M) -> int {
          launch_obs_gate_finish(nk, M, sink.d_G0, sink.d_r, nc, sink.d_out, sink.d_flag, s);
          return sink.read_back(s, g.ids.data() + k0, nc);
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
  GateSink sink = cov ? GateSink::blocks(who, LM_PAIR_COV, out324, status) : GateSink::test(who, 9, d2, C81, r9, dof, status);
  struct Group { std::vector<int2> pr; std::vector<int> ids, lo; };
  Group groups[3][2];      // [SLIDE_CLS_*][route]
  bool any0 = false;
  for (int k = 0; k < n; ++k) {
    sink.clear(k, landmark_dim(cls[k]));
    const LmPair p = lm_pair(cls[k], idx_a[k], idx_b[k]);
    if (route) route[k] = p.st == SLIDE_OK ? p.route : 0;
    if (p.st != SLIDE_OK) { sink.refuse(k, p.st); continue; }
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
      LmPairSigma sg{};
      for (int i = 0; i < D && !cov; ++i) sg.s[i] = (D == 3 ? sig3 : sig7)[i];
      Scratch sc(s);
      int2* d_pr = sc.alloc<int2>(m);
      if ((rc = sink.alloc(sc, max_nc, rt == 1)) != SLIDE_OK) return rc;
      SL_HIP(sc.upload(d_pr, g.pr));
      if (rt == 0) {     // (the whole group in one launch, read back as one sweep)
        if (cov) launch_lm_pair_cov(G, d_sig.d, G.ld, d_pr, m, sink.d_out, s);
        else launch_lm_pair_direct(G, d_sig.d, G.ld, D, d_pr, m, sg, sink.d_out, sink.d_flag, s);
        rc = sink.read_back(s, g.ids.data(), m);
      } else {
        rc = sigma_forms(
            who, m, nk,
            [&](int k0, int nc, double* B, int nT) { launch_lm_pair_fill(G, D, cov, d_pr + k0, sg, nc, B, nT, sink.d_r, sink.d_G0, s); },
            [&](int k0, int nc, const double* M) -> int {
              if (cov) launch_lm_pair_cov_finish(G, D, d_pr + k0, M, nc, sink.d_out, s);
              else launch_obs_gate_finish(nk, M, sink.d_G0, sink.d_r, nc, sink.d_out, sink.d_flag, s);
              return sink.read_back(s, g.ids.data() + k0, nc);
            },
            [&](int k0, int nc) -> int { return walk_start(*std::min_element(g.lo.begin() + k0, g.lo.begin() + k0 + nc)); });
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
      const int gi = (int)w.cd.size(), nsplit = gain_gram_splits(rows);
      const size_t nn = (size_t)rows * rows;
      w.cd.push_back(GainCandDev{w.ncol, rows, nsplit, 0, (long long)w.msz, (long long)w.psz, (long long)w.wsz});
      w.gid.push_back(g);
      w.gcand.push_back(make_int2((int)w.tab.size(), group_ptr[g + 1] - group_ptr[g]));
      gram_jobs(w.jobs, gi, rows, nsplit, true);
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
  GateSink sink = GateSink::blocks("get_pose_pair_covariances", 144, out144n, status);
  std::vector<int4> ends;
  std::vector<int> ids;
  for (int k = 0; k < n_q; ++k) {
    sink.clear(k);
    const int a = joint_end(jg, slot_a[k], idx_a[k]), b = joint_end(jg, slot_b[k], idx_b[k]);
    const int st = a < 0 || b < 0 ? SLIDE_MISSING : (slot_a[k] == slot_b[k] && a == b) ? SLIDE_ERR_INVALID : SLIDE_OK;
    if (st != SLIDE_OK) { sink.refuse(k, st); continue; }
    ends.push_back(make_int4(slot_a[k], a, slot_b[k], b)); ids.push_back(k);
  }
  if (ids.empty()) return SLIDE_OK;
  hipStream_t s = master;
  Scratch sc(s);
  int4* d_ends = sc.alloc<int4>(ends.size());
  if (!sc.ok()) { g_last_error = "get_pose_pair_covariances: out of device memory"; return SLIDE_ERR_HIP; }
  SL_HIP(sc.upload(d_ends, ends));
  return joint_sigma_forms(
      sink.who, jg, (int)ids.size(), 12,
      [&](int k0, int nc, double* B, int ld) { launch_joint_pair_identity(jg.d_tab, d_ends + k0, nc, B, (size_t)ld, s); },
      [&](int k0, int nc, const double* M) -> int { return sink.read_back(s, ids.data() + k0, nc, M); });
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
  GateSink sink = GateSink::test("closure_mahalanobis", 6, d2, C36, r6, nullptr, status);
  std::vector<int4> ends;
  std::vector<double> z, sg;
  std::vector<int> ids;
  for (int k = 0; k < L; ++k) {
    sink.clear(k);
    const int a = joint_end(jg, from_slot[k], from_idx[k]), b = joint_end(jg, to_slot[k], to_idx[k]);
    const int st = a < 0 || b < 0 ? SLIDE_MISSING : (from_slot[k] == to_slot[k] && a == b) ? SLIDE_ERR_INVALID : SLIDE_OK;
    if (st != SLIDE_OK) { sink.refuse(k, st); continue; }
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
  double* d_r = sc.alloc<double>(6 * (size_t)m);      // (by the closure's place in the list, as on one graph)
  if ((rc = sink.alloc(sc, max_nc, false)) != SLIDE_OK) return rc;
  SL_HIP(sc.upload(d_ends, ends));
  SL_HIP(sc.upload(d_z, z));
  SL_HIP(sc.upload(d_sg, sg));
  return joint_sigma_forms(
      sink.who, jg, m, 6,
      [&](int k0, int nc, double* B, int ld) {
        launch_joint_closure_gate_lin(jg.d_tab, d_ends + k0, d_z + 12 * (size_t)k0, d_sg + 6 * (size_t)k0, nc, B, (size_t)ld, d_r + 6 * (size_t)k0, s);
      },
      [&](int k0, int nc, const double* M) -> int {
        launch_closure_gate_finish(M, d_r + 6 * (size_t)k0, nc, sink.d_out, sink.d_flag, s);
        return sink.read_back(s, ids.data() + k0, nc);
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
  const int p = joint_end(jg, ps, pose_idx);
  const JointLmEnd le = joint_lm_end(jg, ls, cls, lm_idx);
  const int l = le.l;
  c.sep = le.sep;
  c.sep_off = le.sep_off;
  c.st = p < 0 || l < 0 ? SLIDE_MISSING : SLIDE_OK;
  if (c.st != SLIDE_OK) return c;
  c.ends = make_int4(ps, p, ls, l);
  c.type = graphs[ps]->obs_measurement(cls, a, c.z, c.sg);
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
  GateSink sink = GateSink::test("observation_mahalanobis", 9, d2, C81, r9, dof, status);
  struct Group { int type = 0; std::vector<int4> ends; std::vector<long long> sep; std::vector<double> z, sg; std::vector<int> ids; };
  Group groups[3];
  groups[0].type = FT_BR; groups[1].type = FT_CUBE; groups[2].type = FT_CYL;
  for (int k = 0; k < n_q; ++k) {
    sink.clear(k, landmark_dim(cls[k]));
    const JointObsCand c = joint_obs_candidate(jg, pose_slot[k], pose_idx[k], lm_slot ? lm_slot[k] : pose_slot[k], cls[k], lm_idx[k],
                                               meas17 + 17 * (size_t)k);
    if (c.st != SLIDE_OK) { sink.refuse(k, c.st); continue; }
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
    if ((rc = sink.alloc(sc, max_nc, true)) != SLIDE_OK) return rc;
    SL_HIP(sc.upload(d_ends, g.ends));
    SL_HIP(sc.upload(d_sep, g.sep));
    SL_HIP(sc.upload(d_z, g.z));
    SL_HIP(sc.upload(d_sg, g.sg));
    rc = joint_sigma_forms(
        sink.who, jg, m, nk,
        [&](int k0, int nc, double* B, int ld) {
          launch_joint_obs_gate_lin(d_Gs, jg.d_tab, g.type, d_ends + k0, d_sep + k0, d_z + 15 * (size_t)k0, d_sg + 9 * (size_t)k0, nc, B, (size_t)ld,
                                    sink.d_r, sink.d_G0, s);
        },
        [&](int k0, int nc, const double* M) -> int {
          launch_obs_gate_finish(nk, M, sink.d_G0, sink.d_r, nc, sink.d_out, sink.d_flag, s);
          return sink.read_back(s, g.ids.data() + k0, nc);
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
  GateSink sink = cov ? GateSink::blocks(who, LM_PAIR_COV, out324, status) : GateSink::test(who, 9, d2, C81, r9, dof, status);
  struct Group { std::vector<int4> ends; std::vector<long long> sep; std::vector<int> ids; };
  Group groups[3];      // [SLIDE_CLS_*]
  for (int k = 0; k < n_q; ++k) {
    sink.clear(k, landmark_dim(cls[k]));
    JointLmEnd ea = joint_lm_end(jg, slot_a[k], cls[k], idx_a[k]), eb = joint_lm_end(jg, slot_b[k], cls[k], idx_b[k]);
    int ga = slot_a[k], gb = slot_b[k];
    int st = ea.l < 0 || eb.l < 0 ? SLIDE_MISSING : SLIDE_OK;
    if (st == SLIDE_OK) {
      const bool sha = ea.sep >= 0, shb = eb.sep >= 0;
      if (sha == shb && (sha ? ea.sep_off == eb.sep_off : (ga == gb && ea.l == eb.l))) st = SLIDE_ERR_INVALID;
    }
    if (st != SLIDE_OK) { sink.refuse(k, st); continue; }
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
    LmPairSigma sg{};
    for (int i = 0; i < D && !cov; ++i) sg.s[i] = (D == 3 ? sig3 : sig7)[i];
    Scratch sc(s);
    int4* d_ends = sc.alloc<int4>(m);
    long long* d_sep = sc.alloc<long long>(2 * (size_t)m);
    if ((rc = sink.alloc(sc, max_nc, true)) != SLIDE_OK) return rc;
    SL_HIP(sc.upload(d_ends, g.ends));
    SL_HIP(sc.upload(d_sep, g.sep));
    rc = joint_sigma_forms(
        who, jg, m, nk,
        [&](int k0, int nc, double* B, int ld) {
          launch_joint_lm_pair_fill(d_Gs, jg.d_tab, D, cov, d_ends + k0, d_sep + 2 * (size_t)k0, sg, nc, B, (size_t)ld, sink.d_r, sink.d_G0, s);
        },
        [&](int k0, int nc, const double* M) -> int {
          if (cov) launch_joint_lm_pair_cov_finish(d_Gs, D, d_ends + k0, d_sep + 2 * (size_t)k0, M, nc, sink.d_out, s);
          else launch_obs_gate_finish(nk, M, sink.d_G0, sink.d_r, nc, sink.d_out, sink.d_flag, s);
          return sink.read_back(s, g.ids.data() + k0, nc);
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
