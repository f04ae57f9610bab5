// What the two host files of the covariance queries share and nobody else sees: host_marginals.hip (the selected inverse, the marginals,
// the information-gain queries, the joint tree and its solve) and host_gates.hip (the quadratic forms B^T Sigma B and everything built
// on them).  Included by those two files only.
#pragma once
#include "host_graph.hpp"

#include <algorithm>

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
inline int landmark_dim(int cls) { return cls == SLIDE_CLS_CYLINDER ? 7 : cls == SLIDE_CLS_CUBE ? 9 : cls == SLIDE_CLS_ELLIPSOID ? 3 : 0; }
// The jobs of launch_gram_blocks for candidate i of a sweep, its gram nk x nk in nsplit row splits: one per (16 x 16 tile, split);
// lower: only the tiles on and below the diagonal (a whole gram that is read as symmetric)
inline void gram_jobs(std::vector<int4>& jobs, int i, int nk, int nsplit, bool lower = false) {
  const int nt = (nk + 15) / 16;
  for (int ta = 0; ta < nt; ++ta)
    for (int tb = 0; tb <= (lower ? ta : nt - 1); ++tb)
      for (int sp = 0; sp < nsplit; ++sp) jobs.push_back(make_int4(i, ta, tb, sp));
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

}  // namespace sl
