// The two robust losses (iteratively reweighted least squares) on one graph and on a batch: the closure loss on the loop-closure /
// relative-measurement / inter-robot factors (k_robust_reweight) and the observation loss on the landmark factors (k_lin_lf_robust).
// Their setters, the batch's views of its members, the weight read-backs and the two measurement launches: the host side of those
// kernels in solver_kernels.hip (the classes are declared in host_graph.hpp).
#include "host_graph.hpp"

#include <algorithm>

namespace sl {

static const char kClosureMask[] = "bit 0 (loop closures) and bit 1 (relative measurements)";
static const char kObservationMask[] = "bit 0 (bearing-range), bit 1 (cube) and bit 2 (cylinder)";
static const uint64_t kKeyIndex = 0x00ffffffffffffffull;      // a key without its class / robot byte

int parse_loss(const char* who, int kind, double param, int class_mask, int allowed_mask, const char* mask_text, LossSetting* out,
               const char* refusal) {
  auto refuse = [who](const std::string& what) { g_last_error = std::string(who) + ": " + what; return SLIDE_ERR_INVALID; };
  if (kind < 0 || kind > 4) return refuse("kind must be 0 (off), 1 Huber, 2 Cauchy, 3 Geman-McClure or 4 DCS");
  if (class_mask & ~allowed_mask) return refuse(std::string("class_mask has ") + mask_text + " only");
  if (refusal) return refuse(refusal);
  if (!(param == param)) return refuse("param is not a number");
  static const double kDefault[5] = {0.0, 1.345, 0.1, 1.0, 1.0};      // GTSAM's defaults of Huber, Cauchy, GemanMcClure, DCS
  out->kind = kind;
  out->mask = kind ? class_mask : 0;
  out->param = kind ? (param > 0.0 ? param : kDefault[kind]) : 0.0;
  return SLIDE_OK;
}

int key_robot(uint64_t key) {
  for (int r = 0; r < SLIDE_MAX_ROBOTS; ++r)
    if ((HostGraph::pose_key(r, 0) >> 56) == (key >> 56)) return r;
  return -1;
}

// ---- what the four read-backs share ----------------------------------------------------------------------------------------------
// rows a read-back writes: all `total` of them up to the caller's capacity (rows past cap are not written); *n_out: the full count
static int rows_within(long long total, int cap, int* n_out) {
  *n_out = (int)total;
  return (int)std::min<long long>(total, std::max(cap, 0));
}
// their tail: the (weight, s^2) pairs of m rows from the device, behind the launch that wrote them on s
static int fetch_pairs(const double* d_out, int m, hipStream_t s, std::vector<double>& out) {
  out.resize(2 * (size_t)m);
  SL_HIP(hipMemcpyAsync(out.data(), d_out, out.size() * sizeof(double), hipMemcpyDeviceToHost, s));
  SL_HIP(hipStreamSynchronize(s));
  SL_HIP(hipGetLastError());
  return SLIDE_OK;
}
static void put_closure(const ClosureCols& c, size_t k, int slot, int r0, uint64_t i0, int r1, uint64_t i1, int kind, int ghost_id, const double* ws) {
  if (c.slot) c.slot[k] = slot;
  if (c.from_robot) c.from_robot[k] = r0;
  if (c.from_idx) c.from_idx[k] = i0;
  if (c.to_robot) c.to_robot[k] = r1;
  if (c.to_idx) c.to_idx[k] = i1;
  if (c.kind) c.kind[k] = kind;
  if (c.ghost_id) c.ghost_id[k] = ghost_id;
  if (c.weight) c.weight[k] = ws[2 * k];
  if (c.s2) c.s2[k] = ws[2 * k + 1];
}
void HostGraph::closure_row(const ClosureCols& c, size_t k, int slot, const ClosureRec& rec, const double* ws) const {
  put_closure(c, k, slot, key_robot(rec.k0), rec.k0 & kKeyIndex, key_robot(rec.k1), rec.k1 & kKeyIndex, h_bt_kind[rec.bt], -1, ws);
}
// (kind 2; the local pose in from_* when it is the factor's first key, else in to_*; the other end: robot -1, idx = its ghost slot)
void HostGraph::ghost_row(const ClosureCols& c, size_t k, int slot, int gh, const double* ws) const {
  const int rl = key_robot(h_gh_key[gh]), gid = (size_t)gh < h_gh_gid.size() ? h_gh_gid[gh] : -1;
  const uint64_t il = h_gh_key[gh] & kKeyIndex, ig = (uint64_t)h_gh_slot[gh];
  if (h_gh_first[gh] != 0) put_closure(c, k, slot, rl, il, -1, ig, 2, gid, ws);
  else put_closure(c, k, slot, -1, ig, rl, il, 2, gid, ws);
}
void HostGraph::inverse_keys(bool poses, bool lms, std::vector<uint64_t>& pkey, std::vector<uint64_t>& lkey) const {
  if (poses) { pkey.assign(h_pose_val.size() / 12, 0); for (const auto& kv : key2pose) pkey[kv.second] = kv.first; }
  if (lms) lkey = h_lm_key;      // (a landmark's own first key: key2lm also holds the aliases merge_landmarks left)
}
void HostGraph::observation_rows(const ObsCols& c, size_t at, int count, int slot, const double* ws) const {
  std::vector<uint64_t> pkey, lkey;
  inverse_keys((slot < 0 && c.who) || c.pose_idx, c.lm_idx != nullptr, pkey, lkey);
  for (int f = 0; f < count; ++f) {
    const size_t k = at + f;
    if (c.who) c.who[k] = slot < 0 ? key_robot(pkey[h_lf_pose[f]]) : slot;
    if (c.pose_idx) c.pose_idx[k] = pkey[h_lf_pose[f]] & kKeyIndex;
    if (c.cls) c.cls[k] = h_lf_type[f] == FT_CYL ? SLIDE_CLS_CYLINDER : (h_lf_type[f] == FT_CUBE ? SLIDE_CLS_CUBE : SLIDE_CLS_ELLIPSOID);
    if (c.lm_idx) c.lm_idx[k] = lkey[h_lf_lm[f]] & kKeyIndex;
    if (c.weight) c.weight[k] = ws[2 * k];
    if (c.s2) c.s2[k] = ws[2 * k + 1];
  }
}
// Measurement: `launch` alone between two events on s, the stream synchronised behind it.  An event pair around one short launch
// mostly measures the launch.
template <class F>
static int time_on_stream(hipStream_t s, F&& launch, double* ms) {
  hipEvent_t e0 = nullptr, e1 = nullptr;
  SL_HIP(hipEventCreate(&e0));
  SL_HIP(hipEventCreate(&e1));
  (void)hipEventRecord(e0, s);
  launch();
  (void)hipEventRecord(e1, s);
  float t = 0.f;
  const bool ok = hipStreamSynchronize(s) == hipSuccess && hipEventElapsedTime(&t, e0, e1) == hipSuccess;
  *ms = t;
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  return ok ? SLIDE_OK : SLIDE_ERR_HIP;
}

// ---- one graph -----------------------------------------------------------------------------------------------------------------
// After either setter the resident factor, the kept records and the last solution belong to the system as it was weighted: as after
// chi2(), the next solve relinearises and re-factors everything and keeps no block of dp.
int HostGraph::set_robust_loss(int kind, double param, int class_mask) {
  LossSetting v;
  const int rc = parse_loss("set_robust_loss", kind, param, class_mask, 3, kClosureMask, &v,
                            batch ? "the graph has joined a batch; the sharded and joint paths do not carry a robust loss" : nullptr);
  if (rc != SLIDE_OK) return rc;
  RB.kind = v.kind; RB.mask = v.mask; RB.param = v.param;
  if (v.on() && !rb_arrays) { rb_arrays = true; topo_dirty = true; }      // (upload_new creates and fills the robust arrays)
  // every sigma back to its base value; the next solve takes the weights of the new setting everywhere
  if (restore_base_sigmas() != SLIDE_OK) return SLIDE_ERR_HIP;
  drop_factor();
  drop_stream_state();
  if (!v.on()) prof.forget("k_robust_reweight");
  return SLIDE_OK;
}
int HostGraph::set_observation_loss(int kind, double param, int class_mask) {
  LossSetting v;
  const int rc = parse_loss("set_observation_loss", kind, param, class_mask, 7, kObservationMask, &v,
                            batch ? "the graph has joined a batch; a batch carries its own observation loss (slide_chol_batch_set_observation_loss), "
                                    "the un-batched sharded passes carry none" : nullptr);
  if (rc != SLIDE_OK) return rc;
  OB.kind = v.kind; OB.mask = v.mask; OB.param = v.param;
  if (v.on() && !ol_arrays) { ol_arrays = true; topo_dirty = true; }      // (upload_new creates the weight arrays)
  drop_factor();
  drop_stream_state();
  return SLIDE_OK;
}
int HostGraph::restore_base_sigmas() {
  if (up_rb > 0) SL_HIP(hipMemcpyAsync(d_bt_sigma.d, d_bt_sigma0.d, 6 * std::min(up_rb, up_bt) * sizeof(double), hipMemcpyDeviceToDevice, stream));
  if (up_rbg > 0) SL_HIP(hipMemcpyAsync(d_gh_sigma.d, d_gh_sigma0.d, 6 * std::min(up_rbg, up_gh) * sizeof(double), hipMemcpyDeviceToDevice, stream));
  return SLIDE_OK;
}
int HostGraph::get_closure_weights(int cap, int32_t* from_robot, uint64_t* from_idx, int32_t* to_robot, uint64_t* to_idx, int32_t* kind,
                                   double* weight, double* s2, int* n_out) {
  if (!lin_done) { g_last_error = "get_closure_weights: nothing was linearised yet (call solve first)"; return SLIDE_ERR_INVALID; }
  std::vector<int> idx, rec;      // the kernel's factor numbers and their records in h_closures
  for (size_t q = 0; q < h_closures.size(); ++q)
    if ((size_t)h_closures[q].bt < lin_bt) { idx.push_back(h_closures[q].bt); rec.push_back((int)q); }      // (a factor added after the last solve has no linearisation to report)
  const int m = rows_within((long long)idx.size(), cap, n_out);
  if (m == 0) return SLIDE_OK;
  hipStream_t s = stream;
  if (d_rb_idx.ensure(m, 0, s) != SLIDE_OK || d_rb_out.ensure(2 * (size_t)m, 0, s) != SLIDE_OK) return SLIDE_ERR_HIP;
  SL_HIP(hipMemcpyAsync(d_rb_idx.d, idx.data(), m * sizeof(int), hipMemcpyHostToDevice, s));
  RobustDev Rq = RB;
  Rq.kind = lin_rb_kind; Rq.mask = lin_rb_mask;
  launch_closure_weights(G, Rq, d_rb_idx.d, m, d_rb_out.d, s);
  std::vector<double> out;
  const int rc = fetch_pairs(d_rb_out.d, m, s, out);
  if (rc != SLIDE_OK) return rc;
  const ClosureCols c{nullptr, from_robot, from_idx, to_robot, to_idx, kind, nullptr, weight, s2};
  for (int k = 0; k < m; ++k) closure_row(c, k, -1, h_closures[rec[k]], out.data());
  return SLIDE_OK;
}
int HostGraph::get_observation_weights(int cap, int32_t* robot, uint64_t* pose_idx, int32_t* cls, uint64_t* lm_idx, double* weight, double* s2,
                                       int* n_out) {
  if (!lin_done) { g_last_error = "get_observation_weights: nothing was linearised yet (call solve first)"; return SLIDE_ERR_INVALID; }
  const int m = rows_within((long long)std::min(lin_lf, up_lf), cap, n_out);      // (a factor added after the last solve has no linearisation to report)
  if (m == 0) return SLIDE_OK;
  std::vector<double> out;
  if (weight || s2) {
    if (d_ol_out.ensure(2 * (size_t)m, 0, stream) != SLIDE_OK) return SLIDE_ERR_HIP;
    launch_observation_weights(G, OB, lin_ol_kind != 0, m, d_ol_out.d, stream);
    const int rc = fetch_pairs(d_ol_out.d, m, stream, out);
    if (rc != SLIDE_OK) return rc;
  }
  observation_rows(ObsCols{robot, pose_idx, cls, lm_idx, weight, s2}, 0, m, -1, out.data());
  return SLIDE_OK;
}

// ---- a batch ---------------------------------------------------------------------------------------------------------------------
// The settings live here, not in the members: a member's own RobustDev / ObsLossDev carries its arrays under kind 0 (its own solves
// stay unweighted, the per-graph refusals hold), the batch's views add the batch's loss.  Under the closure loss the members' sigmas
// are rewritten (restored when the setting changes, a member leaves or the batch goes); under the observation loss nothing of a
// member is - the weight sits inside the records the next linearisation writes again - so there is nothing to restore.
RobustDev CholBatch::member_view(const HostGraph* g) const {
  RobustDev R = g->RB;
  R.kind = rb.kind; R.mask = rb.mask; R.param = rb.param;
  return R;
}
ObsLossDev CholBatch::member_obs_view(const HostGraph* g) const {
  ObsLossDev O = g->OB;
  O.kind = ol.kind; O.mask = ol.mask; O.param = ol.param;
  return O;
}
int CholBatch::set_loss(bool closures, int kind, double param, int class_mask) {
  const char* who = closures ? "chol_batch_set_robust_loss" : "chol_batch_set_observation_loss";
  LossSetting v;
  int rc = parse_loss(who, kind, param, class_mask, closures ? 3 : 7, closures ? kClosureMask : kObservationMask, &v);
  if (rc != SLIDE_OK) return rc;
  std::lock_guard<std::mutex> pl(pass_mtx);
  if (v.on() && pcg_iters > 0) {
    g_last_error = std::string(who) + ": the batch runs PCG passes (pcg_iters > 0), whose step leaves the inter-robot factors' cross block out; they do not carry " +
                   (closures ? "a robust loss" : "an observation loss");
    return SLIDE_ERR_INVALID;
  }
  std::vector<HostGraph*> gs;
  {
    std::lock_guard<std::mutex> lk(mtx);
    (closures ? rb : ol) = v;
    pass_dirty = true;
    gs.assign(graphs.begin(), graphs.end());
  }
  exact_serial = 0;           // (the joint queries wait for the next pass: the factor and the cached joint Sigma are the old weighting's)
  (closures ? rb_pass_done : ol_pass_done) = false;
  for (HostGraph* g : gs) {      // (the members' weight arrays of the observation loss come with the next pass: begin_pass, upload_new)
    if (!g) continue;
    std::lock_guard<std::mutex> gl(g->mtx);
    if (closures) {
      if (g->restore_base_sigmas() != SLIDE_OK) rc = SLIDE_ERR_HIP;      // every sigma back to its base value: the next pass weights under the new setting
      if (v.on() && !g->rb_arrays) { g->rb_arrays = true; g->topo_dirty = true; }
    }
    g->drop_factor();
    g->drop_stream_state();
  }
  return rc;
}
// the members of a read-back, or the refusal while the device tables are not these graphs' (a member joined, left or was replaced, or
// the batch's configuration changed since the last pass)
int CholBatch::readback_members(const char* who, bool pass_done, size_t n_noted, std::vector<HostGraph*>& gs) {
  if (!pass_done || (int)n_noted != n || !master) { g_last_error = std::string(who) + ": nothing was linearised under the current setting yet (pass first)"; return SLIDE_ERR_INVALID; }
  std::lock_guard<std::mutex> lk(mtx);
  if (pass_dirty) { g_last_error = std::string(who) + ": the batch changed since the last pass (pass first)"; return SLIDE_ERR_INVALID; }
  gs.assign(graphs.begin(), graphs.end());
  for (HostGraph* g : gs)
    if (!g) { g_last_error = std::string(who) + ": a slot of the batch is empty"; return SLIDE_ERR_INVALID; }
  return SLIDE_OK;
}
int CholBatch::get_closure_weights(int cap, int32_t* slot, int32_t* from_robot, uint64_t* from_idx, int32_t* to_robot, uint64_t* to_idx, int32_t* kind,
                                   int32_t* ghost_id, double* weight, double* s2, int* n_out) {
  static const char who[] = "chol_batch_get_closure_weights";
  std::lock_guard<std::mutex> pl(pass_mtx);
  std::vector<HostGraph*> gs;
  int rc = readback_members(who, rb_pass_done, lin_bt.size(), gs);
  if (rc != SLIDE_OK) return rc;
  struct Row { int slot, fac, bt, gh; };      // fac: the kernel's factor number; bt: index in h_closures, or -1; gh: ghost factor, or -1
  std::vector<Row> rows;
  for (int i = 0; i < n; ++i) {
    HostGraph* g = gs[i];
    std::lock_guard<std::mutex> gl(g->mtx);
    if ((size_t)g->G.n_between != lin_bt[i] || (size_t)g->G.n_ghost != lin_gh[i]) { g_last_error = std::string(who) + ": a member changed since the last pass (pass first)"; return SLIDE_ERR_INVALID; }
    for (size_t c = 0; c < g->h_closures.size(); ++c)
      if ((size_t)g->h_closures[c].bt < lin_bt[i]) rows.push_back(Row{i, g->h_closures[c].bt, (int)c, -1});
    for (size_t q = 0; q < lin_gh[i]; ++q) rows.push_back(Row{i, (int)(lin_bt[i] + q), -1, (int)q});
  }
  const int m = rows_within((long long)rows.size(), cap, n_out);
  if (m == 0) return SLIDE_OK;
  if ((size_t)m > rb_ent_cap) {
    if (d_rb_ent) { (void)hipFree(d_rb_ent); d_rb_ent = nullptr; }
    if (d_rb_out) { (void)hipFree(d_rb_out); d_rb_out = nullptr; }
    rb_ent_cap = 0;
    SL_HIP(hipMalloc(reinterpret_cast<void**>(&d_rb_ent), 2 * (size_t)m * sizeof(int)));
    SL_HIP(hipMalloc(reinterpret_cast<void**>(&d_rb_out), 2 * (size_t)m * sizeof(double)));
    rb_ent_cap = (size_t)m;
  }
  std::vector<int> ent(2 * (size_t)m);
  for (int k = 0; k < m; ++k) { ent[2 * (size_t)k] = rows[k].slot; ent[2 * (size_t)k + 1] = rows[k].fac; }
  // the views of the last pass under the loss it ran with (no loss then: every weight 1, s^2 from the residuals)
  std::vector<RobustDev> Rq(n);
  for (int i = 0; i < n; ++i) { Rq[i] = member_view(gs[i]); Rq[i].kind = lin_rb_kind; Rq[i].mask = lin_rb_mask; }
  if (!d_Rs) SL_HIP(hipMalloc(reinterpret_cast<void**>(&d_Rs), CHOL_BATCH_HOST_MAX * sizeof(RobustDev)));
  SL_HIP(hipMemcpyAsync(d_Rs, Rq.data(), n * sizeof(RobustDev), hipMemcpyHostToDevice, master));      // (what the captured pass reads as well: the same bytes while a loss is set)
  SL_HIP(hipMemcpyAsync(d_rb_ent, ent.data(), ent.size() * sizeof(int), hipMemcpyHostToDevice, master));
  launch_closure_weights_batched(d_Gs, d_Rs, d_rb_ent, m, d_rb_out, master);
  std::vector<double> out;
  if ((rc = fetch_pairs(d_rb_out, m, master, out)) != SLIDE_OK) return rc;
  const ClosureCols c{slot, from_robot, from_idx, to_robot, to_idx, kind, ghost_id, weight, s2};
  for (int k = 0; k < m; ++k) {
    const Row& r = rows[k];
    HostGraph* g = gs[r.slot];
    std::lock_guard<std::mutex> gl(g->mtx);
    if (r.bt >= 0) g->closure_row(c, k, r.slot, g->h_closures[r.bt], out.data());
    else g->ghost_row(c, k, r.slot, r.gh, out.data());
  }
  return SLIDE_OK;
}
int CholBatch::get_observation_weights(int cap, int32_t* slot, uint64_t* pose_idx, int32_t* cls, uint64_t* lm_idx, double* weight, double* s2, int* n_out) {
  static const char who[] = "chol_batch_get_observation_weights";
  std::lock_guard<std::mutex> pl(pass_mtx);
  std::vector<HostGraph*> gs;
  int rc = readback_members(who, ol_pass_done, lin_lf.size(), gs);
  if (rc != SLIDE_OK) return rc;
  int off[CHOL_BATCH_HOST_MAX] = {0}, cnt[CHOL_BATCH_HOST_MAX] = {0};
  long long total = 0;
  for (int i = 0; i < n; ++i) {
    HostGraph* g = gs[i];
    std::lock_guard<std::mutex> gl(g->mtx);
    if ((size_t)g->G.n_lf != lin_lf[i] || g->h_lf_type.size() != lin_lf[i] ||
        (lin_ol_kind != 0 && lin_lf[i] > 0 && (!g->OB.lf_w || !g->OB.lf_s2 || g->up_ol < lin_lf[i]))) {
      g_last_error = std::string(who) + ": a member changed since the last pass (pass first)";
      return SLIDE_ERR_INVALID;
    }
    off[i] = (int)total;
    total += (long long)lin_lf[i];
  }
  if (total > 0x7fffffffLL) { g_last_error = std::string(who) + ": too many factors"; return SLIDE_ERR_INVALID; }
  const int m = rows_within(total, cap, n_out);
  if (m == 0) return SLIDE_OK;
  for (int i = 0; i < n; ++i) cnt[i] = std::max(0, std::min((int)lin_lf[i], m - off[i]));      // (rows past cap are not written)
  std::vector<double> out;
  if (weight || s2) {
    if ((size_t)m > ol_out_cap) {
      if (d_ol_out) { (void)hipFree(d_ol_out); d_ol_out = nullptr; }
      ol_out_cap = 0;
      SL_HIP(hipMalloc(reinterpret_cast<void**>(&d_ol_out), 2 * (size_t)m * sizeof(double)));
      ol_out_cap = (size_t)m;
    }
    // d_Gs and d_Os are the last pass's tables: with a loss then, d_Os holds the members' arrays that pass wrote
    launch_observation_weights_batched(d_Gs, d_Os, lin_ol_kind != 0, off, cnt, n, d_ol_out, master);
    if ((rc = fetch_pairs(d_ol_out, m, master, out)) != SLIDE_OK) return rc;
  }
  const ObsCols c{slot, pose_idx, cls, lm_idx, weight, s2};
  for (int i = 0; i < n; ++i) {
    if (cnt[i] == 0) continue;
    std::lock_guard<std::mutex> gl(gs[i]->mtx);
    gs[i]->observation_rows(c, (size_t)off[i], cnt[i], i, out.data());
  }
  return SLIDE_OK;
}
// Measurement: k_robust_reweight_b alone on the pass's stream.  It runs on what the last pass left - the ghost values of that pass's
// start beside the estimates of its end - so the weights it writes belong to no pass: the read-back is refused until the next pass,
// whose own launch writes every weight and sigma again before anything reads them.
int CholBatch::profile_robust_reweight(double* const* d_bufs, double* ms) {
  std::lock_guard<std::mutex> pl(pass_mtx);
  if (!rb.on()) { g_last_error = "profile_robust_reweight: the batch has no robust loss"; return SLIDE_ERR_INVALID; }
  bool same = false;
  int rc = begin_pass(d_bufs, &same);
  if (rc != SLIDE_OK) return rc;
  rc = time_on_stream(master, [&] { launch_robust_reweight_batched(d_Gs, d_Rs, hG.data(), n, master); }, ms);
  rb_pass_done = false;
  return rc;
}
// Measurement: the pass's linearisation launch alone on the pass's stream, under the batch's current loss.  It linearises at the point
// the last pass left, so what it writes belongs to no pass: both read-backs and the joint queries wait for the next pass.  (The
// reweighting above marks the closure read-back alone: the two have always differed in this, and the difference is kept.)
int CholBatch::profile_linearize(double* const* d_bufs, double* ms) {
  std::lock_guard<std::mutex> pl(pass_mtx);
  bool same = false;
  int rc = begin_pass(d_bufs, &same);
  if (rc != SLIDE_OK) return rc;
  rc = time_on_stream(master, [&] { launch_linearize_batched(d_Gs, hG.data(), n, master, ol.on() ? d_Os : nullptr); }, ms);
  exact_serial = 0;
  rb_pass_done = false;
  ol_pass_done = false;
  return rc;
}

}  // namespace sl
