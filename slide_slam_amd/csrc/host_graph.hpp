// Host side of the device-resident factor graph: the SemanticFactorGraph seam of the reference
// (backend/sloam/include/factorgraph/graph.h:70-121, src/factorgraph/graph.cpp) re-designed for one
// MI355X: factors and variables are appended to SoA arrays in HBM, the host keeps only keys,
// topology (CSR lists) and the pending fgraph / fvalues queues (graph.h:150-151).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/slide_gpu.h"
#include "graph_dev.hpp"
#include "host_layout.hpp"
#include "kernels.hpp"
#include "sl_math.hpp"

namespace sl {

extern thread_local std::string g_last_error;
void thread_capture_mode_local();      // (host_graph.hip) once per host thread: stream-capture mode thread-local
bool hip_ok(hipError_t e, const char* what);
inline bool robot_ok(int r) { return r >= 0 && r < SLIDE_MAX_ROBOTS; }
int decode_status(const int* st8);      // status words of a pass -> SLIDE_OK / SLIDE_ERR_NOT_SPD / SLIDE_ERR_RUNTIME (+ g_last_error)
// A robust loss as its setter normalised it (host_loss.hip): kind 0 = off with mask and param 0, else GTSAM's Huber, Cauchy,
// GemanMcClure or DCS (1 .. 4) on the factor classes of mask with param > 0.  A graph keeps its two in RB / OB, a batch in rb / ol.
struct LossSetting {
  int kind = 0, mask = 0;
  double param = 0.0;
  bool on() const { return kind != 0; }
};
// The one validator of the four setters.  who: the entry point's prefix of every message; mask_text: its sentence about the bits of
// allowed_mask; refusal (null: none): the entry point's own refusal, reported after the kind and mask checks and before the
// not-a-number check.  param <= 0 becomes the loss's default.  SLIDE_ERR_INVALID (+ g_last_error), *out untouched, or SLIDE_OK.
int parse_loss(const char* who, int kind, double param, int class_mask, int allowed_mask, const char* mask_text, LossSetting* out,
               const char* refusal = nullptr);
int key_robot(uint64_t key);            // (host_loss.hip) the robot of a pose key, -1 for any other key
// the output columns of the weight read-backs (null: not asked for); who: the robot on a graph, the slot on a batch
struct ClosureCols { int32_t *slot, *from_robot; uint64_t* from_idx; int32_t* to_robot; uint64_t* to_idx; int32_t *kind, *ghost_id; double *weight, *s2; };
struct ObsCols { int32_t* who; uint64_t* pose_idx; int32_t* cls; uint64_t* lm_idx; double *weight, *s2; };
#define SL_HIP(x)                                     \
  do {                                                \
    if (!::sl::hip_ok((x), #x)) return SLIDE_ERR_HIP; \
  } while (0)

// Host -> device uploads of one graph update, batched: while a batch is open (thread-local), DevArr::upload copies into one
// pinned staging buffer instead of issuing a hipMemcpyAsync per array (~35 small copies per frame otherwise, each a few
// microseconds of host and copy-engine time); flush() sends the buffer with ONE copy and scatters it on the device.
struct UploadBatch {
  struct Seg { unsigned long long dst; unsigned off, bytes; };
  std::vector<Seg> segs;
  unsigned char* h_pin = nullptr; size_t h_cap = 0, used = 0;
  unsigned char* d_stage = nullptr; size_t d_cap = 0;
  hipEvent_t ev = nullptr;
  bool in_flight = false;
  static thread_local UploadBatch* current;
  ~UploadBatch();
  int begin();                                     // waits for the previous flush's copy before the pinned buffer is reused
  int reserve(size_t need);
  int add(void* dst, const void* src, size_t bytes);
  int flush(hipStream_t s);                        // closes the batch
};

// Device -> host results of one step, batched the same way: gathered on the device, ONE copy into pinned memory, then
// handed out to their host destinations.  run() synchronises the stream.
struct DownloadBatch {
  struct Seg { unsigned long long src; unsigned off, bytes; };
  std::vector<Seg> segs;
  std::vector<void*> host_dst;
  unsigned char* h_pin = nullptr; size_t h_cap = 0, used = 0;
  unsigned char* d_stage = nullptr; size_t d_cap = 0;
  ~DownloadBatch();
  void add(void* host, const void* dev, size_t bytes);     // bytes: multiple of 4
  int run(hipStream_t s);
};

// host mirror of a device CSR (HostGraph: landmark -> factors, pose -> factors, pose -> relative-pose factors)
struct CsrMirror {
  std::vector<int> ptr{0}, val;
  int dirty_from = 0;      // lists from this index on changed since the last upload (lists beyond the mirror are new anyway)
  size_t off0 = 0;         // (set by the upload) first value entry it rewrote
  void touch(int i) { if (i < dirty_from) dirty_from = i; }
};
// growable device array; contents below `used` survive a growth
template <class T>
struct DevArr {
  T* d = nullptr;
  size_t cap = 0;
  ~DevArr() { if (d) (void)hipFree(d); }
  int ensure(size_t n, size_t used, hipStream_t s, bool zero_new = false) {
    if (n <= cap) return SLIDE_OK;
    size_t nc = cap ? cap : 1024;
    while (nc < n) nc *= 2;
    T* nd = nullptr;
    SL_HIP(hipMalloc(&nd, nc * sizeof(T)));
    if (zero_new) SL_HIP(hipMemsetAsync(nd, 0, nc * sizeof(T), s));
    if (d && used) SL_HIP(hipMemcpyAsync(nd, d, used * sizeof(T), hipMemcpyDeviceToDevice, s));
    if (d) {
      SL_HIP(hipStreamSynchronize(s));
      SL_HIP(hipFree(d));
    }
    d = nd;
    cap = nc;
    return SLIDE_OK;
  }
  // exactly n elements (the big per-system buffers: the caller's own growth policy, no rounding up on top of it); contents dropped
  int ensure_exact(size_t n, hipStream_t s, bool zero_new = false) {
    if (d) {
      SL_HIP(hipStreamSynchronize(s));
      SL_HIP(hipFree(d));
      d = nullptr;
      cap = 0;
    }
    if (n == 0) return SLIDE_OK;
    SL_HIP(hipMalloc(&d, n * sizeof(T)));
    cap = n;
    if (zero_new) SL_HIP(hipMemsetAsync(d, 0, n * sizeof(T), s));
    return SLIDE_OK;
  }
  int upload(const T* h, size_t off, size_t count, hipStream_t s) {
    if (count == 0) return SLIDE_OK;
    if (UploadBatch::current && sizeof(T) % 4 == 0) return UploadBatch::current->add(d + off, h, count * sizeof(T));
    SL_HIP(hipMemcpyAsync(d + off, h, count * sizeof(T), hipMemcpyHostToDevice, s));
    return SLIDE_OK;
  }
};

struct Profiler {
  bool on = false;
  struct Rec { int id; hipEvent_t a, b; };
  std::vector<Rec> recs;
  std::vector<hipEvent_t> pool;
  std::vector<std::string> names;
  std::vector<double> ms;
  std::vector<int64_t> count;
  int id_of(const char* name);
  void begin(int id, hipStream_t s);
  void end(hipStream_t s);
  void collect();     // after a stream sync
  void reset();
  void forget(const char* name);     // drops a stage from the table (between solves: no record may be pending)
  ~Profiler();
};

struct PendVar {
  uint64_t key;
  int type;
  double val[15];
};
constexpr int PF_GHOST = 100;
struct PendFac {
  int type;          // 0 prior, 1 between, FT_BR, FT_CUBE, FT_CYL, PF_GHOST (ghost between: k1 = slot, z[12] = local-first flag)
  uint64_t k0, k1;
  double z[15];
  double sigma[9];
  int origin;        // between factors: 0 odometry, 1 loop closure, 2 relative measurement (GraphDev::bt_kind)
};

// The dense factor + solve of several graphs that share a GPU as ONE launch sequence (launch_chol_batch): every graph's thread
// arrives with its system assembled on its own stream, the last one enqueues the batched launches on the batch's stream behind
// all of them, and every graph's stream continues behind the batch.  All joined graphs must solve in lockstep (the distributed
// pass does); a rendezvous that is not completed within 60 s returns SLIDE_ERR_RUNTIME.
class HostGraph;
constexpr int CHOL_BATCH_HOST_MAX = 8;      // graphs a batch holds at most
// what an information-gain query reads back: the gram matrices, the rows of U at the trajectory's poses (for C = I + J U)
struct GainFetched { std::vector<double> M, Urow; };
// The callbacks of the quadratic-form queries (sigma_forms on one graph, joint_sigma_forms on a batch): fill queues the kernel that
// writes the columns of candidates k0 .. k0 + nc - 1 into B (ld rows per column, zero before); done gets their grams on the device
using FormFill = std::function<void(int k0, int nc, double* B, int ld)>;
using FormDone = std::function<int(int k0, int nc, const double* M)>;
// (optional, single graph only) the first block column the sweep's forward substitution has to walk: B is zero above row NB * it
using FormStart = std::function<int(int k0, int nc)>;
struct FormBackend;      // (host_gates.hip: what differs between one graph and the joint graph of a batch)
// the `prob` quantile of chi-square with dof degrees of freedom (host code; SLIDE_ERR_INVALID for prob outside (0, 1) or dof < 1)
int chi2_quantile(double prob, int dof, double* q);
class CholBatch {
 public:
  explicit CholBatch(int n);
  ~CholBatch();
  int n_slots() const { return n; }
  int factor_solve(int slot, const GraphDev& G, hipStream_t s);
  int all_reduce(int slot, double* d_buf, int count, hipStream_t s);     // sum over the joined graphs' buffers, stream-ordered
  // Ownership: a batch does not own its graphs and a graph does not own its batch.  ~HostGraph leaves its batch (detach), ~CholBatch
  // sends every joined graph back to its own launches; either invalidates the captured pass.  Lock order: pass_mtx -> graph -> mtx.
  void set_graph(int slot, HostGraph* g);
  void detach(HostGraph* g);
  // One distributed pass of ALL joined graphs from one host thread: the phases of every robot on its own stream, forked from and
  // joined to the batch's stream around the two device-side exchanges and the batched factor + solve, captured once and replayed
  // as ONE hipGraph per pass.  bufs[i]: exchange buffer of the graph in slot i.
  int pass_all(double* const* d_bufs);
  int pass_part(double* const* d_bufs, int part);       // the same pass cut at its exchanges (multi-GPU jobs): parts 0, 1, 2 and, with the joint solve, 10, 11, 12
  // Joint solve: after the factorisations, `iters` PCG iterations on the global reduced system (pcg_kernels.hip); 0 = each robot's own
  // block solve only (block-Jacobi over robots).  Changing it invalidates the captured launch sequences.
  void set_pcg(int iters, double tol = 0.0);
  // Robust loss (iteratively reweighted least squares) on the members' loop-closure / relative-measurement between factors and on
  // the inter-robot relative-pose (ghost) factors, uniform over the batch (HostGraph::set_robust_loss's arguments and defaults):
  // k_robust_reweight_b ahead of the linearisation of every whole or cut pass.  Not with PCG passes (pcg_iters > 0).
  int set_robust_loss(int kind, double param, int class_mask) { return set_loss(true, kind, param, class_mask); }
  bool robust_on() const { return rb.on(); }
  // per member slot: its loop-closure / relative-measurement between factors in insertion order, then its ghost factors (kind 2;
  // the local pose in from_* when it is the factor's first key, else in to_*; the other end: robot -1, idx = its ghost slot;
  // ghost_id: slide_graph_set_ghost_ids' index, -1 for between factors and unnamed ghosts), with w and s^2 of the last pass
  int get_closure_weights(int cap, int32_t* slot, int32_t* from_robot, uint64_t* from_idx, int32_t* to_robot, uint64_t* to_idx, int32_t* kind,
                          int32_t* ghost_id, double* weight, double* s2, int* n_out);
  int profile_robust_reweight(double* const* d_bufs, double* ms);      // k_robust_reweight_b alone between two events (measurement)
  // Robust loss on the members' landmark observation factors, uniform over the batch (HostGraph::set_observation_loss's arguments,
  // defaults and validation): k_lin_lf_robust_b in k_lin_lf_b's place in every whole or cut pass.  Independent of set_robust_loss.
  // Not with PCG passes (pcg_iters > 0).
  int set_observation_loss(int kind, double param, int class_mask) { return set_loss(false, kind, param, class_mask); }
  bool observation_loss_on() const { return ol.on(); }
  // slot by slot the member's landmark factors in insertion order: its slot, the factor's pose index, its landmark (cls: SLIDE_CLS_*,
  // lm_idx: the member's local index), w and the unscaled s^2 of the last pass.  One launch, one read-back.
  int get_observation_weights(int cap, int32_t* slot, uint64_t* pose_idx, int32_t* cls, uint64_t* lm_idx, double* weight, double* s2, int* n_out);
  int profile_linearize(double* const* d_bufs, double* ms);      // the pass's linearisation launch alone between two events (measurement)
  int pcg() const { return pcg_iters; }
  double pcg_tolerance() const { return pcg_tol; }
  // Exact joint step ("arrow"): the shared landmarks stay as the separator of the joint graph (graph_dev.hpp).  sep_buf: the caller's
  // device buffer of sep_buffer_len(m) doubles in which part 0 of a cut pass leaves this GPU's partial sum of the separator system
  // (packed: lower tile columns only) for the cross-GPU all-reduce, and from which part 2 takes the sum; null: no exchange (the job is
  // this process alone).  Changing it invalidates the captured launch sequences.
  int set_arrow(bool on, double* sep_buf, long long sep_len);
  int set_separator_profile(const int32_t* prof, int n);
  int set_separator_blocks(int Ta, int Tb, int used_a, int used_b);      // nested dissection of the separator system: two leaf blocks + top block (zeros: off)
  // A job that spans GPUs, its ranks split in two halves along the dissection: this rank OWNS leaf `leaf` (0 / 1; -1: none, the default) —
  // it factors that leaf only, and of the separator system only the top block crosses between the halves (cut pass: [20] 0 1 2).
  // leader: the one rank of its half that adds the leaf's Schur complement to the top block's sum.
  int set_separator_owner(int leaf, bool leader);
  static void sep_segment(int ms, int lam, int Ta, int Tb, int which, long long* off, long long* len);      // packed buffer: leaf a | leaf b | top block + lambdas
  // Nested dissection of every robot's own pose chain in exact joint passes: `n` segments per robot factored side by side, the windows
  // of poses between them (as wide as the band) eliminated at a second level (graph_dev.hpp pose_sep).  1: off.
  void set_segments(int n_seg);
  int segments() const { return n_seg; }      // tile profile of the separator system's landmark part (n = its tile columns), or none: dense
  bool is_arrow() const { return arrow; }
  // packed exchange layout of the separator system: ms landmark coordinates + lam lambda coordinates (6 per inter-robot relative-pose factor)
  // doubles of it a cut pass exchanges: a dissected layout (Ta, Tb tile columns in its leaves) leaves the zero block between the leaves out
  static long long sep_exchange_len(int ms, int lam, int Ta, int Tb) { return sep_buffer_len(ms, lam) - (long long)NB * NB * Ta * Tb; }
  static long long sep_buffer_len(int ms, int lam = 0) { const long long Tt = (ms + NB - 1) / NB + (lam + NB - 1) / NB; return (long long)NB * NB * Tt * (Tt + 3) / 2; }
  hipStream_t pass_stream();                             // the stream the passes run on (created on first use)
  int profile_pass(double* const* d_bufs, double* ms_steps, int* n_launches);
  int profile_arrow(double* const* d_bufs, double* out6, int* n_sep_steps);
  // (the queries from here on: host_marginals.hip; from the pose pairs on, host_gates.hip)
  // marginal covariances on the JOINT graph, from the factor the last exact joint pass (pass_all) left (joint_cov_kernels.hip): the
  // poses of the graph in `slot` by its pose indices, its landmarks by its landmark ids, logEntropy's trace sums (job-wide landmarks)
  int joint_pose_covariances(int slot, const uint64_t* idx, int n, double* out36n);
  int joint_landmark_covariances(int slot, int cls, const uint64_t* idx, int n, double* out);
  int joint_marginal_traces(int slot, double* out4);
  // estimateClosureInfoGain on the JOINT graph (the same factor): Between factors (traj[q + 1], traj[q]), pose q of the graph in
  // traj_slots[q] (null: all in `slot`); out4 = {10 pose + landmark, the robot of `slot`'s pose drop, the job's point landmarks' drop,
  // every robot's pose drop}
  int joint_closure_info_gain(int slot, const int32_t* traj_slots, const uint64_t* traj, int n, const double* travel, const double* sigma6,
                              double* out4);
  // a list of candidates in sweeps of one many-column solve each: candidate k = traj[off[k] .. off[k + 1]), out4n[4 k ..], status[k]
  int joint_closure_info_gain_batch(int slot, int n_cand, const int32_t* off, const int32_t* traj_slots, const uint64_t* traj,
                                    const double* travel, const double* sigma6, double* out4n, int32_t* status);
  // the joint marginal of pose pairs and the Mahalanobis gate of a list of closures on the JOINT graph (HostGraph::pose_pair_covariances
  // / closure_mahalanobis with a slot where those take a robot; the two ends may sit in different graphs): B^T K^-1 B = W^T D W with
  // L W = B on the factor K = L D L^T of the last exact pass; the arguments are checked by the C ABI before these are called
  int joint_pose_pair_covariances(int n, const int32_t* slot_a, const uint64_t* idx_a, const int32_t* slot_b, const uint64_t* idx_b,
                                  double* out144n, int32_t* status);
  int joint_closure_mahalanobis(int L, const int32_t* from_slot, const uint64_t* from_idx, const int32_t* to_slot, const uint64_t* to_idx,
                                const double* rel7, const double* sigma6, double* d2, double* C36, double* r6, int32_t* status);
  // the Mahalanobis gate of candidate landmark observations on the JOINT graph (HostGraph::observation_mahalanobis with slots; lm_slot
  // null: the landmark is the pose's graph's, else it may be another robot's): a private landmark through its graph's Schur records, a
  // shared one at its separator rows
  int joint_observation_mahalanobis(int n, const int32_t* pose_slot, const uint64_t* pose_idx, const int32_t* lm_slot, const int32_t* cls,
                                    const uint64_t* lm_idx, const double* meas17, double* d2, int32_t* dof, double* C81, double* r9, int32_t* status);
  // the joint-compatibility test of groups of such candidates on the JOINT graph (HostGraph::observation_joint_compatibility with the
  // call above's naming): a private landmark once per group, a shared one as often as the caller likes
  int joint_observation_joint_compatibility(int n_groups, const int32_t* group_ptr, const int32_t* pose_slot, const uint64_t* pose_idx,
                                            const int32_t* lm_slot, const int32_t* cls, const uint64_t* lm_idx, const double* meas17, double prob,
                                            int32_t* accepted, double* d2_single, double* d2_joint, int32_t* dof_joint, int32_t* status,
                                            double* group_d2, int32_t* group_dof, int32_t* group_count, int32_t* group_status);
  // landmark PAIRS on the JOINT graph (HostGraph::landmark_pairs with a landmark named (slot, cls, local idx), a shared one through
  // any replica): the Mahalanobis test of "a and b are one object" (cov = false) or the pair's joint marginal, the landmark block
  // between two robots included (cov = true: out324); every pair takes the forward substitution.  Arguments checked by the C ABI
  int joint_landmark_pairs(bool cov, int n, const int32_t* cls, const int32_t* slot_a, const uint64_t* idx_a, const int32_t* slot_b,
                           const uint64_t* idx_b, const double* sig3, const double* sig7, double* d2, int32_t* dof, double* C81, double* r9,
                           double* out324, int32_t* status);
  // every pair of the job's landmarks of a class (private ones of every member, each shared slot once) whose anchors lie within
  // radius; cross_only: not the pairs of two private landmarks of one member
  int joint_landmark_pairs_within(int cls, double radius, bool cross_only, int64_t cap, int32_t* slot_a, uint64_t* idx_a, int32_t* slot_b,
                                  uint64_t* idx_b, double* dist, int64_t* n_pairs);

 private:
  int n;
  std::mutex mtx;                        // rendezvous state + the graphs[] table
  std::mutex pass_mtx;                   // pass_all / profile_pass (the captured pass and its device tables)
  bool pass_dirty = false;               // graphs[] changed since the pass was captured (under mtx)
  std::condition_variable cv;
  int arrived = 0;
  unsigned long long generation = 0;
  int gen_status = SLIDE_OK;
  std::vector<CholSystem> sys;
  std::vector<double*> bufs;
  std::vector<HostGraph*> graphs;
  hipGraphExec_t pass_exec = nullptr;
  hipGraphExec_t part_exec[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};     // parts 0, 1, 2, 10, 11, 12 (exact joint step: 0 and 2 only), 20 (ghost refresh)
  int enqueue_ghost_refresh(double* const* d_bufs, int part);
  int last_part = -1;                    // the part of a cut pass that ran last (-1: none / a whole pass): pass_part checks the order
  int pcg_iters = 0;
  double pcg_tol = 0.0;
  bool arrow = false;
  int n_seg = 1;
  std::vector<CholSystem> seg_sys, l2_sys;          // the segments of all joined graphs as systems of their own (views); the second-level systems
  std::vector<int> l2_graph;                        // l2_sys[i] belongs to graphs[l2_graph[i]]
  int* d_ctr2 = nullptr;
  int* d_pair_tickets = nullptr;                    // 12 x CHOL_STEP_BATCH_MAX ints (zero between launches): the pair kernel's per-system counters — one block per launch sequence
                                                    // of the segments (8), the second level (8), the leaves (9), the own leaf (10), the top block (11)
  int* pair_tickets(int block) const { return d_pair_tickets ? d_pair_tickets + block * CHOL_STEP_BATCH_MAX : nullptr; }
  // left-looking persistent factorisations (k_chol_ll): one launch per level instead of one per block column — the segments of all
  // joined graphs, the bands' second level, the separator's leaves (both / the own one of a rank that owns a leaf), its top block.
  // SLIDE_CHOL_LL=0: the step kernels, one launch per block column (round 3's path)
  CholLLPlan *ll_seg = nullptr, *ll_l2 = nullptr, *ll_leaves = nullptr, *ll_leaf_own[2] = {nullptr, nullptr}, *ll_top = nullptr;
  std::vector<const int*> seg_hord;                 // host copies of the segments' border-row orders (CholSystem::ord)
  void free_ll_band_plans();
  void free_ll_sep_plans();
  void sep_leaf_systems(CholSystem* lv) const;      // the two leaf blocks of a dissected separator as systems (views of sepS)
  CholSystem sep_top_system() const;                // its top block (the lambdas' rows as border)
  int* d_syrk_jobs = nullptr;                       // border product: (system << 20 | ib << 10 | jb) of every lower tile + right-hand-side row, longest sum first
  int n_syrk_jobs = 0, syrk_jobs_cap = 0, syrk_lds_pad = 0;
  int* d_l2_jobs = nullptr; int n_l2_jobs = 0, l2_jobs_cap = 0;      // the same for the border products of the bands' second level
  // separator system of the exact joint step: m coordinates, Ts tile columns; factored by the un-batched step kernels on the pass's stream
  double* sepS = nullptr; long long sep_len = 0;          // the system in the factorisation's layout (owned)
  double* sep_x = nullptr; long long sep_x_len = 0;       // the caller's exchange buffer (packed layout), or null: no exchange
  int sep_m = 0, sep_Ts = 0;
  double *sep_Ld = nullptr, *sep_Winv = nullptr, *sep_yv = nullptr, *sep_dp = nullptr;
  int *sep_status = nullptr, *sep_ctr = nullptr, *d_sep_off = nullptr;
  int sep_cap = 0;
  std::vector<int> h_sep_prof; int* d_sep_prof = nullptr; bool sep_prof_on = false;
  // nested dissection of the separator system (set_separator_blocks): two leaf blocks of sep_leafT[0], sep_leafT[1] tile columns that no
  // robot couples, factored side by side as views of sepS with the top block's rows (and the lambda rows) as their border, then the top
  // block; sep_used[b]: coordinates of leaf b that carry a slot (the rest of its last tile is padding with a unit diagonal)
  int sep_leafT[2] = {0, 0}, sep_used[2] = {0, 0};
  int sep_owner = -1; bool sep_leader = true;
  std::vector<int> h_leaf_prof[2];                  // the leaves' own profiles (relative to the view)
  int* d_leaf_prof = nullptr;                       // both, one after the other (backward substitutions of the views)
  int* d_sep_tmask = nullptr;                       // per (virtual) tile of the separator: which joined graphs hold coordinates of it (k_sep_gather)
  int* sep_ctr2 = nullptr; int* d_sep_jobs = nullptr; int n_sep_jobs = 0; double* sep_scratch = nullptr; int sep_ks = 1;
  // a WHOLE pass over a dissected separator takes the same arithmetic as two ranks owning a leaf each: per-half partial sums of the top
  // block (sepS's own top block: the first half's, sep_top2 / sep_bord2: the other's), each minus its leaf's Schur complement, added —
  // so that 1, 2, 4 and 8 ranks give the same bits (SURVEY 7 hard part 5).  sep_mask_b: the joined graphs that hold leaf b.
  double *sep_top2 = nullptr, *sep_bord2 = nullptr; int sep_ld2 = 0; unsigned sep_mask_b = 0;
  int* d_lam_jobs2 = nullptr; int n_lam_jobs2 = 0;      // the same for the lambda block
  int* d_sep_jobs2 = nullptr; int n_sep_jobs2 = 0;      // the top block's product over BOTH leaves as two systems of one launch (system << 20 | ib << 10 | jb)
  int* d_sep_jobs4 = nullptr; int n_sep_jobs4 = 0;      // that table and, behind it, the lambda block's as systems 2, 3: both products in one launch (launch_border_syrk_pairs)
  bool sep_dissected() const { return sep_leafT[0] > 0 && sep_leafT[1] > 0; }
  // lambda coordinates of the inter-robot relative-pose factors: border rows of the separator system, their own small system
  int sep_lam = 0, sep_nl = 0, lam_cap = -1;
  double *lam_scratch = nullptr;      // partial products of the separator's own border product (split K)
  double *sep_bord = nullptr, *lamS = nullptr, *lam_Ld = nullptr, *lam_Winv = nullptr, *lam_yv = nullptr, *lam_dp = nullptr;
  int *lam_status = nullptr, *lam_ctr = nullptr;
  SepLayout sep_layout() const {
    SepLayout Y{sepS, sep_bord, sep_x, sep_Ts, sep_nl, sep_m, sep_lam, {0, 0, 0, 0}, 0, 0};
    if (sep_dissected()) {
      Y.gap[0] = sep_used[0]; Y.gap[1] = sep_leafT[0] * NB;
      Y.gap[2] = sep_leafT[0] * NB + sep_used[1]; Y.gap[3] = (sep_leafT[0] + sep_leafT[1]) * NB;
      Y.hTa = sep_leafT[0]; Y.hTL = sep_leafT[0] + sep_leafT[1];
    }
    return Y;
  }
  int prepare_separator();
  int enqueue_arrow(double* const* d_bufs, int part, hipEvent_t e0, hipEvent_t e1);
  hipEvent_t prof_ev[7] = {};       // (profile_arrow: [6] = behind the robots' border product, before the bands' second level)
  void free_separator();
  int enqueue_pcg_head(double* const* d_bufs);                   // r = b, u = M^-1 b, t_l(u) packed + local sum
  int enqueue_pcg_mid(double* const* d_bufs, bool whole);                    // w = S u, partial dots + local sum
  int enqueue_pcg_tail(double* const* d_bufs, bool last, bool whole);        // alpha, beta, updates; then u = M^-1 r, t_l(u) | dp = x
  int save_systems();                                            // S -> S0 before the factorisation (joint solve only)
  std::vector<GraphDev> pass_G;
  std::vector<double*> pass_bufs;
  hipEvent_t ev_fork = nullptr;
  GraphDev* d_Gs = nullptr;              // the joined graphs' device views, for the kernels batched over blockIdx.z
  // robust loss of the batch: the members' RobustDev views beside d_Gs (their arrays, the batch's setting), compared by begin_pass
  // like the GraphDev views; what the last pass linearised under and how many factors of each member it covered (the read-back)
  LossSetting rb;
  int set_loss(bool closures, int kind, double param, int class_mask);      // both setters: rb (closures) or ol
  int readback_members(const char* who, bool pass_done, size_t n_noted, std::vector<HostGraph*>& gs);
  RobustDev* d_Rs = nullptr;
  std::vector<RobustDev> hR, pass_R;
  RobustDev member_view(const HostGraph* g) const;
  bool rb_pass_done = false;
  int lin_rb_kind = 0, lin_rb_mask = 0;
  std::vector<size_t> lin_bt, lin_gh;
  int* d_rb_ent = nullptr; double* d_rb_out = nullptr; size_t rb_ent_cap = 0;
  void note_pass();
  // observation loss of the batch: the members' ObsLossDev views beside d_Gs and d_Rs (their lf_w / lf_s2, the batch's setting; a
  // member's own OB.kind stays 0), compared by begin_pass like the other two; what the last pass linearised under and how many
  // landmark factors of each member it covered (the read-back).  No array of a member is rewritten under the loss, so nothing is
  // restored when a member leaves or the batch goes.
  LossSetting ol;
  ObsLossDev* d_Os = nullptr;
  std::vector<ObsLossDev> hO, pass_O;
  ObsLossDev member_obs_view(const HostGraph* g) const;
  bool ol_pass_done = false;
  int lin_ol_kind = 0;
  std::vector<size_t> lin_lf;
  double* d_ol_out = nullptr; size_t ol_out_cap = 0;
  int capture_pass(double* const* d_bufs, int part, hipGraphExec_t* exec);
  int prepare_pass();
  int prepare_member(HostGraph* g, bool for_pass);      // (the caller holds g->mtx)
  int begin_pass(double* const* d_bufs, bool* same);
  int end_pass();
  int enqueue_pass(double* const* d_bufs, hipEvent_t e0, hipEvent_t e1, int part);
  std::vector<GraphDev> hG;
  int rendezvous(int slot, hipStream_t s, bool reduce, int count);
  std::vector<hipEvent_t> ev_in;
  hipEvent_t ev_out = nullptr;
  hipStream_t master = nullptr;
  hipStream_t aux[8] = {};               // further streams of the grouped factorisation (the groups' launches overlap on the GPU)
  hipEvent_t ev_aux0 = nullptr, ev_aux1[8] = {};
  int* d_ctr = nullptr;
  int last_groups = 1;                   // launch sequences factor_all used last
  int* d_status_all = nullptr;           // the joined graphs' status words, gathered by the last node of a pass
  int ctr_cap = 0;
  int factor_all(hipEvent_t after);      // the batched factor + solve of all joined systems, in one to four overlapping launch sequences
  // joint marginals: exact_serial = the number of the last whole exact pass whose factor the buffers still hold (0: none — no pass yet, or
  // the last pass was cut, profiled or not exact); per graph, what that pass factored (HostGraph::fact_shape_now + fact_serial)
  unsigned long long n_exact = 0, exact_serial = 0, jsig_serial = 0;
  std::vector<std::vector<size_t>> exact_shape;
  double* jsig_sep = nullptr; long long jsig_lds_sep = 0;                // Sigma of the separator system (landmark coordinates, then lambdas)
  std::vector<double*> jsig_rob; std::vector<long long> jsig_lds;       // per graph: Sigma over its band, window and border rows
  std::vector<int*> jsig_prow;                                          // per graph: a pose's first row in its Sigma
  void free_joint_sigma();
  int joint_state(const char* who, int slot);      // SLIDE_ERR_INVALID (+ message) unless the last exact pass's factor is resident
  int ensure_joint_sigma();
  // kept between the joint gain queries (under pass_mtx): freeing these megabytes right after device-to-host copies filled them
  // made glibc trim the heap under the runtime's pinning, 14 - 25 ms per m = 64 query
  GainFetched ig_host;
  int compute_joint_sigma();                       // (ensure_joint_sigma's work; it drops the jsig_* buffers when this fails)
  // the exact joint pass's elimination tree (system 0: the separator, 1 + i: robot i): every system's JSinvSys (Sg, Z left null, lds its
  // rows), the tile rows of every column, and per robot its backward steps, segments, border map and pose rows
  struct JointTree {
    std::vector<JSinvSys> Y;
    std::vector<int> rp{0}, rows;
    std::vector<std::vector<std::vector<int>>> steps;          // per robot: the columns of each step of the backward recursion
    std::vector<std::vector<std::pair<int, int>>> ranges;      // per robot: the band's column ranges factored side by side
    std::vector<int> T, Tc, Trow, gn;                          // per robot: band, factor columns, rows; rows of separator coordinates past Tc NB
    std::vector<std::vector<int>> map, prow;                   // per robot: border coordinate -> separator row (-1: padding); a pose's first row
    int Ts = 0, Tsep = 0, sTa = 0, sTL = 0;                    // separator: landmark tiles, all tiles, end of leaf a, end of leaf b (0: not dissected)
    // K X = R with many right-hand sides through the tree (k_jms_*): the launches in stream order, their jobs (system, tile, [l0, l1)
    // of lst), and the separator's rows as sums of the robots' (the inverse of the border maps, robot order)
    struct SolvePlan {
      struct Launch { int kind, bwd, j0, nj, maxl; };          // kind 0: push, 1: pull, 2: sum, 3: gather
      std::vector<Launch> launches;
      std::vector<int4> jobs;
      std::vector<int> lst, sptr{0};
      std::vector<int2> sent;
      int max_gn = 0;
      int n_fwd = 0;                                           // the launches before the backward half: W = L^-1 R on its own
    };
    void solve_plan(SolvePlan& p) const;
  };
  void joint_tree(JointTree& t) const;
  struct JointGain;                                // what the joint gain queries share: the tree, the solve's schedule, the grams' row lists
  int joint_sigma_forms(const char* who, JointGain& jg, int ncand, int nk, const FormFill& fill, const FormDone& done);
  void joint_form_backend(FormBackend& be, JointGain& jg);      // the batch's back end of the quadratic-form drivers (jg outlives be)
  // what the two observation queries resolve of a candidate on the host: {pose's graph, pose id, landmark's graph, landmark id}, the
  // row at which a shared landmark enters the walk (-1: private) and its separator offset, z and the sigmas
  struct JointObsCand { int st = SLIDE_OK, type = 0, sep_off = -1; int4 ends = {0, 0, 0, 0}; long long sep = -1; double z[15] = {}, sg[9] = {}; };
  JointObsCand joint_obs_candidate(JointGain& jg, int pose_slot, uint64_t pose_idx, int lm_slot, int cls, uint64_t lm_idx, const double* meas17) const;
  // one landmark of the joint graph, named (slot, cls, local idx): its id in that slot's graph (-1: missing) and, for a shared one,
  // its slot, its separator offset and the joint row at which it enters the walk (-1s: private)
  struct JointLmEnd { int l = -1, sh = -1, sep_off = -1; long long sep = -1; };
  JointLmEnd joint_lm_end(JointGain& jg, int slot, int cls, uint64_t lm_idx) const;
  int joint_robot(int slot) const;                 // robot id of the graph's own poses
  int joint_end(const JointGain& jg, int slot, uint64_t idx) const;      // one end of a pair or closure: its pose id in the graph of `slot`, or -1
  // the job's point landmarks: every graph's private ones (landmark ids), and of each shared slot that holds one, once, its offset in
  // the separator system
  void job_point_landmarks(std::vector<std::vector<int>>& priv, std::vector<int>& shared_off) const;
};

class HostGraph {
  friend class CholBatch;
 public:
  explicit HostGraph(const slide_params_t& p);
  ~HostGraph();
  int init();

  // SemanticFactorGraph API (graph.cpp)
  int set_prior(int robot, const double* pose7);
  int add_keypose_between(int robot, uint64_t from, uint64_t to, const double* rel7, const double* est7);
  int add_between_sigma(uint64_t k0, uint64_t k1, const SE3& rel, const double* sigma6, int origin = 0);
  int add_loop_closure(const double* rel7, uint64_t i1, int r1, uint64_t i2, int r2);
  int add_relative_meas(const double* rel7, uint64_t i1, int r1, uint64_t i2, int r2);
  int add_relative_meas_ghost(const double* rel7, uint64_t idx, int robot, int slot, bool local_first);
  int set_ghosts(const int32_t* own_robot, const int64_t* own_idx, int n_slots);
  int pose_covariance(int robot, uint64_t idx, double* cov36);
  // marginals on the selected inverse of the resident factor, loop-closure information gain (host_marginals.hip, cov_kernels.hip;
  // single-graph path only)
  int pose_covariances(int robot, const uint64_t* idx, int n, double* out36n);
  int landmark_covariances(int cls, const uint64_t* idx, int n, double* out);
  int marginal_traces(int robot, double* out4);
  int closure_info_gain(int robot, const uint64_t* traj, int n, const double* travel, const double* sigma6, double* out3);
  int closure_info_gain_batch(int robot, int n_cand, const int32_t* off, const uint64_t* traj, const double* travel, const double* sigma6,
                              double* out3n, int32_t* status);      // candidate k = traj[off[k] .. off[k + 1]): out3n[3 k ..], status[k]
  // the joint marginal of pose pairs and the Mahalanobis gate of a list of loop closures, both as B^T Sigma B = W^T W with L W = B
  // (host_gates.hip sigma_forms, closure_kernels.hip); the arguments are checked by the C ABI before these are called
  int pose_pair_covariances(int n, const int32_t* robot_a, const uint64_t* idx_a, const int32_t* robot_b, const uint64_t* idx_b, double* out144n,
                            int32_t* status);
  int closure_mahalanobis(int L, const int32_t* from_robot, const uint64_t* from_idx, const int32_t* to_robot, const uint64_t* to_idx,
                          const double* rel7, const double* sigma6, double* d2, double* C36, double* r6, int32_t* status);
  // the Mahalanobis gate of a list of candidate landmark observations (obs_gate_kernels.hip has the invariant): candidate k is the
  // factor add_range_bearing / add_cube / add_cylinder would add between pose (robot, pose_idx) and the existing landmark (cls, lm_idx)
  // from meas17[17 k ..], the class's remaining arguments in the add call's order; arguments checked by the C ABI
  int observation_mahalanobis(int n, const int32_t* robot, const uint64_t* pose_idx, const int32_t* cls, const uint64_t* lm_idx,
                              const double* meas17, double* d2, int32_t* dof, double* C81, double* r9, int32_t* status);
  // the same gate at a PREDICTED pose (host_gates.hip has the text): every candidate sits at est7, the value the Between factor
  // add_keypose_between(robot, from_idx, ., rel7, est7) would tie to pose (robot, from_idx); nothing is added.  SLIDE_MISSING for a
  // from pose the graph does not hold (nothing written); arguments checked by the C ABI
  int predicted_observation_mahalanobis(int robot, uint64_t from_idx, const double* rel7, const double* est7, int n, const int32_t* cls,
                                        const uint64_t* lm_idx, const double* meas17, double* d2, int32_t* dof, double* C81, double* r9,
                                        int32_t* status);
  // additions no solve has merged yet (the resident factor, where there is one, does not describe the graph they will give)
  bool has_pending() const { return !pend_vars.empty() || !pend_facs.empty(); }
  // the joint-compatibility test of n_groups hypotheses (obs_joint_kernels.hip has the invariant and the rule): group g is the
  // candidates group_ptr[g] .. group_ptr[g + 1] - 1, each described as observation_mahalanobis's; prob == 0: evaluate only.  Every
  // output is written (per candidate, then per group); arguments checked by the C ABI
  int observation_joint_compatibility(int n_groups, const int32_t* group_ptr, const int32_t* robot, const uint64_t* pose_idx, const int32_t* cls,
                                      const uint64_t* lm_idx, const double* meas17, double prob, int32_t* accepted, double* d2_single,
                                      double* d2_joint, int32_t* dof_joint, int32_t* status, double* group_d2, int32_t* group_dof,
                                      int32_t* group_count, int32_t* group_status);
  // what the two calls above resolve of a candidate on the host (obs_measurement: its class's factor type, z and the sigmas under
  // this graph's parameters), and where a sweep starts its walk (of candidates; with `lo` its lowest pose)
  struct ObsCand { int st = SLIDE_OK, type = 0, p = -1, l = -1; double z[15] = {}, sg[9] = {}; };
  ObsCand obs_candidate(int robot, uint64_t pose_idx, int cls, uint64_t lm_idx, const double* meas17) const;
  int obs_measurement(int cls, const double* meas17, double* z15, double* sigma9) const;
  int obs_walk_start(const int32_t* pid, const int32_t* lid, int n) const;
  int obs_gate(const char* who, PredPoseDev* pred, int pred_robot, uint64_t pred_from, int n, const int32_t* robot, const uint64_t* pose_idx,
               const int32_t* cls, const uint64_t* lm_idx, const double* meas17, double* d2, int32_t* dof, double* C81, double* r9,
               int32_t* status);
  int walk_start(int lo) const;
  // Landmark PAIRS of one class each (host_gates.hip has the text): the Mahalanobis test of "a and b are one object" (cov = false:
  // sig3 / sig7 the model noise of points / cylinders; d2, dof, C81, r9 as the observation gate's) or the pair's joint marginal
  // (cov = true: out324).  route[k]: 0 = read off the selected inverse, 1 = forward substitution; arguments checked by the C ABI
  int landmark_pairs(bool cov, int n, const int32_t* cls, const uint64_t* idx_a, const uint64_t* idx_b, const double* sig3, const double* sig7,
                     double* d2, int32_t* dof, double* C81, double* r9, double* out324, int32_t* route, int32_t* status);
  // what they resolve of a pair on the host: the landmarks' ids, the status word, the lowest observing pose and the route
  struct LmPair { int st = SLIDE_OK, a = -1, b = -1, route = 0, lo = 0; };
  LmPair lm_pair(int cls, uint64_t idx_a, uint64_t idx_b) const;
  // every pair of the selected landmarks of a class whose anchors (point xyz, cube t, cylinder root of the current estimate) lie
  // within radius, as landmark keys in the selection's order; sel_idx null: every landmark of the class in the graph's order
  int landmark_pairs_within(int cls, double radius, int n_sel, const uint64_t* sel_idx, const int32_t* sel_label, int64_t cap, uint64_t* idx_a,
                            uint64_t* idx_b, double* dist, int64_t* n_pairs);
  // what the three add calls store of their arguments (and the gate evaluates): z as br_z / cu_z / cy_z hold it, the cube's sigmas
  static void br_meas(const double* bearing, double range, double* z4);
  void cube_meas(const SE3& pose, const SE3& cube_world, const double* scale, double* z15, double* sigma9) const;
  static void cyl_meas(const SE3& pose, const double* root, const double* ray, double radius, double* z7);
  void join_batch(CholBatch* b, int slot);      // takes the graph's lock itself (never while the batch's is held the other way round)
  int dist_pass_local(double* d_buf);     // one distributed pass when every robot of the job is in this graph's batch (no host syncs inside)
  int add_point_landmark(uint64_t idx, const double* xyz);
  int add_range_bearing(int robot, uint64_t pose_idx, uint64_t lm_idx, const double* bearing, double range);
  int add_cube(int robot, uint64_t pose_idx, uint64_t cube_idx, const SE3& pose, const SE3& cube_world, const double* scale,
               bool exists);
  int add_cylinder(int robot, uint64_t pose_idx, uint64_t cyl_idx, const SE3& pose, const double* root, const double* ray,
                   double radius, bool exists);
  int solve();                       // one iSAM2-equivalent update
  int gauss_newton(int iterations);  // batch GN iterations (threshold 0)
  int get_pose12(int robot, uint64_t idx, double* out12);   // SLIDE_MISSING + identity when absent
  int get_landmark(int cls, uint64_t idx, double* out);
  // slide_graph_select_closures: slot[k] = row of pose (robot[k], idx[k]) in the device-resident estimate, -1 when the graph does
  // not hold it (or has not uploaded it yet); the estimate itself, 12 doubles per row.  Nothing is changed.
  void pose_slots(const int32_t* robot, const uint64_t* idx, int n, int32_t* slot) const {
    for (int k = 0; k < n; ++k) slot[k] = robot_ok(robot[k]) ? pose_id(robot[k], idx[k]) : -1;
  }
  const double* pose_est_dev() const { return d_pose_est.d; }
  int lm_lid(int cls, uint64_t idx) const;                   // -1 when not merged yet
  // Landmark fusion (host_graph.hip has the text): pair k says landmark (cls[k], drop_idx[k]) is the object (cls[k], keep_idx[k]) mapped
  // a second time; its factors become the survivor's, its key an alias, its slot a tombstone.  fuse: the survivors of points and
  // cylinders take the information-weighted mean of their cluster (k_lm_merge_fuse).  Arguments checked by the C ABI
  int merge_landmarks(int n, const int32_t* cls, const uint64_t* keep_idx, const uint64_t* drop_idx, bool fuse, uint64_t* into, int32_t* moved,
                      int32_t* status);
  int landmark_alias(int cls, uint64_t idx, uint64_t* into);      // the key a landmark key resolves to (itself unless it was dropped), or SLIDE_MISSING
  // what the last merge_landmarks call spent (measurement): host restructure, upload, k_lm_merge_fuse with its read-back (wall ms), and
  // the kernel's launches alone between two events
  void merge_timing(double* out4) const { for (int i = 0; i < 4; ++i) out4[i] = merge_ms[i]; }
  // one-robot-per-GPU mode: shared-landmark slots + the three phases of a distributed GN pass
  int set_shared(const int32_t* cls, const int64_t* idx, const int32_t* owner, int n_slots);
  int dist_phase(int phase, double* d_buf);
  int pcg() const { return pcg_iters; }
  double pcg_tolerance() const { return pcg_tol; }
  void set_pcg(int iters, double tol = 0.0);      // un-batched passes: dist_phase 1 prepares the joint solve, 31 / 32 / 33 run it (0 = block solves only)
  // exact joint step (batched passes only): offsets of the shared slots' tangent coordinates in the separator system, n_slots + 1 ints,
  // the same on every rank (slide_graph_set_separator)
  int set_separator(const int32_t* off, int n);
  // exact joint step: ids[i] = index of this graph's i-th ghost factor in the job's list of n_total inter-robot relative-pose
  // measurements: the factor enters through six separator coordinates of its own ("lambda", graph_dev.hpp gh_bord)
  int set_ghost_ids(const int32_t* ids, int n, int n_total);
  void stats(int64_t* out5) const;
  int64_t rejected() const;
  int chi2(double* out4);                 // sum of squared whitened residuals at the current estimate: total, priors, betweens, landmark factors
  // Robust loss on the loop-closure / relative-measurement factors (iteratively reweighted least squares; k_robust_reweight).
  // kind 0: off; param <= 0: the loss's default; mask bit 0: loop closures, bit 1: relative measurements.  Single-graph path only.
  int set_robust_loss(int kind, double param, int class_mask);
  bool robust_on() const { return RB.kind != 0; }
  // weight and squared whitened norm of every loop-closure / relative-measurement factor at its last linearisation, insertion order
  int get_closure_weights(int cap, int32_t* from_robot, uint64_t* from_idx, int32_t* to_robot, uint64_t* to_idx, int32_t* kind, double* weight,
                          double* s2, int* n_out);
  // Robust loss on the landmark observation factors (iteratively reweighted least squares, fused into the linearisation:
  // k_lin_lf_robust).  kind 0: off; param <= 0: the loss's default; mask bit 0: bearing-range, bit 1: cube, bit 2: cylinder factors.
  // Independent of set_robust_loss.  Single-graph path only.
  int set_observation_loss(int kind, double param, int class_mask);
  bool observation_loss_on() const { return OB.kind != 0; }
  // weight and squared whitened norm of every landmark factor at its last linearisation, insertion order
  int get_observation_weights(int cap, int32_t* robot, uint64_t* pose_idx, int32_t* cls, uint64_t* lm_idx, double* weight, double* s2, int* n_out);
  void set_incremental(bool on) { inc_enabled = on; }
  void incremental_stats(int64_t* out4) const { out4[0] = n_inc; out4[1] = n_full; out4[2] = last_cd; out4[3] = G.T; }
  // iSAM2's wildfire threshold on the back-substitution of a streaming update (ISAM2GaussNewtonParams::wildfireThreshold, 1e-3 in the
  // reference's GTSAM 4.0.3 build; graph.cpp:15-18, 260-272).  0 (the default here): every update solves the linear system exactly.
  void set_wildfire(double thr) { wildfire_thr = thr > 0.0 ? thr : 0.0; }
  void wildfire_stats(int64_t* out2) const { out2[0] = n_wf_kept; out2[1] = last_wf_kept; }      // blocks kept: all updates / the last one
  int get_tile_profile(int* out, int cap);
  int get_border_profile(int* out, int cap);
  int get_segments(int* out, int cap);
  int get_segment_table(int* out, int cap);          // number of segments of the band in exact joint passes (1: not cut); out[2 i], out[2 i + 1] = tile range of segment i; out[2 n] = separator poses   // nbr (>= 0) or a negative error; out[i] = first block column of border tile row i, i < min(nbr, cap)     // T (>= 0) or a negative error; out[c] = prof[c] for c < min(T, cap)
  void set_dense_profile(bool on);        // ignore the structure of the reduced system (measurement aid)
  int pcg_stats(double* out8);            // scalars of the last joint solve: gamma_old, alpha_old, alpha, beta, first gamma, last gamma               // entries merge_pending refused since creation

  static uint64_t pose_key(int robot, uint64_t idx);
  static uint64_t lm_key(int cls, uint64_t idx);

  slide_params_t P;
  hipStream_t stream = nullptr;
  hipStream_t stream2 = nullptr;              // trailing updates of the Cholesky look-ahead
  std::vector<hipEvent_t> ev_dp, ev_upd;
  std::mutex mtx;
  Profiler prof;
  GraphDev G{};
  RobustDev RB{};                    // the robust loss's arrays and setting (null / 0 until a loss is set): kind / mask / param are the only store of it
  ObsLossDev OB{};                   // the observation loss's arrays and setting (null / 0 until one is set), likewise

 private:
  int merge_pending();
  int64_t n_rejected = 0;                 // factors / variables refused by merge_pending since creation (slide_graph_stats)
  int upload_new();                       // what merge_pending added goes to the device, in four stages:
  int upload_tails(hipStream_t s);        //   the array tails, the CSR mirrors, the linearisation buffers
  int upload_border(hipStream_t s);       //   the exact joint step's border (plan_border, host_layout.hpp)
  int upload_system(hipStream_t s);       //   S, the factor buffers, the tile profile (plan_tile_profile) and what it clears in S
  int upload_view(hipStream_t s);         //   the GraphDev view, the pose adjacency, the segments' profiles, the pair lists, the slot table
  int layout_current();                   // merge_pending + upload_new for the layout getters: 0 or the negative error
  int run_update(double relin_thr, int iterations);
  int enqueue_iteration(bool lookahead, bool skip_relin = false, int c_d = 0, int wf_cd = -1);      // one GN / iSAM2-equivalent pass on `stream`; c_d > 0: block columns below it keep their factor
  // Incremental re-factorisation (iSAM2's "re-eliminate only the affected top of the tree", graph.cpp:260-272): the lowest pose whose
  // rows of the reduced system the factors merged since the last solve change; the generation of S the resident factor belongs to
  int dirty_min_pose = 1 << 30;
  std::vector<int> h_lm_first;          // per landmark: lowest pose index observing it
  DevArr<int> d_lm_first;
  unsigned long long S_gen = 0, fact_gen = ~0ull;
  int64_t n_inc = 0, n_full = 0, last_cd = 0;
  double wildfire_thr = 0.0;
  DevArr<double> d_dp_prev;            // the last solve's reduced solution (bounded back-substitution: k_chol_extract_y keeps it)
  int wf_T = 0;                        // block columns of it that are valid (0: none — first solve, or the buffers were re-allocated)
  // streaming updates without a read-back in the middle (round 5): the last update predicted which variables THIS one relinearises
  // (k_estimate_predict -> status[5]), its closing read-back brought the status words and the newest pose's estimate in one copy
  unsigned long long lin_gen = 1, lin_solved_gen = 0;      // re-allocations of the linearisation buffers (their contents are dropped) / the value at the last successful solve
  bool pred_valid = false;             // pred_pose / pred_thr describe the delta the device holds right now
  int pred_pose = 1 << 30;             // lowest pose whose blocks the next relinearisation changes (1 << 30: none)
  double pred_thr = -1.0;
  bool status_clean = false;           // the status words are zero (k_final_pack left them so)
  DevArr<double> d_final;              // 16 doubles: k_final_pack's output
  int cache_pose = -1;                 // pose index whose estimate cache_pose12 holds (-1: none)
  double cache_pose12[12];
  int64_t n_pred_used = 0;
  int64_t n_wf_kept = 0, last_wf_kept = 0;
  bool inc_enabled = true;

  std::vector<PendVar> pend_vars;
  std::vector<PendFac> pend_facs;
  std::unordered_map<uint64_t, int> key2pose, key2lm;
  // merge_landmarks: key2lm sends a dropped key to its survivor.  h_lm_key: per landmark its own (first) key, 0 for a tombstone — a slot
  // whose landmark was dropped: no key, no factors; lm_aliases: per survivor the dropped keys that resolve to it
  std::vector<uint64_t> h_lm_key;
  std::unordered_map<int, std::vector<uint64_t>> lm_aliases;
  size_t n_tomb = 0;
  bool lm_tomb(size_t l) const { return l < h_lm_key.size() && h_lm_key[l] == 0; }
  std::vector<int> lf_lm_moved;         // factors below up_lf whose lf_lm row changed since the last upload (upload_new sends exactly those)
  bool relin_all_next = false;          // the next update folds every delta in and linearises everything (run_update)
  DevArr<int> d_merge;                  // k_lm_merge_fuse's cluster lists and status words
  double merge_ms[4] = {0, 0, 0, 0};
  // merged host mirrors (initial values; theta itself lives in HBM)
  std::vector<double> h_pose_val, h_lm_val;
  std::vector<int> h_lm_type;
  std::vector<int> h_pr_pose; std::vector<double> h_pr_z, h_pr_sigma;
  std::vector<int> h_bt_i, h_bt_j; std::vector<double> h_bt_z, h_bt_sigma;
  // robust loss.  The device arrays it needs (bt_sigma0, bt_kind, bt_w, bt_s2) exist from the first time a loss is set on (rb_arrays):
  // a graph that never sets one uploads and launches exactly what it did before.  h_bt_sigma is the mirror of bt_sigma0.
  std::vector<int> h_bt_kind;
  struct ClosureRec { int bt; uint64_t k0, k1; };
  std::vector<ClosureRec> h_closures;          // the between factors with bt_kind != 0, insertion order
  bool rb_arrays = false;
  size_t up_rb = 0;                            // between factors the robust arrays hold
  bool lin_done = false;                       // a linearisation ran; it covered lin_bt between factors under the loss lin_rb_kind / lin_rb_mask
  size_t lin_bt = 0;
  int lin_rb_kind = 0, lin_rb_mask = 0;
  void note_linearisation() { lin_done = true; lin_bt = up_bt; lin_rb_kind = RB.kind; lin_rb_mask = RB.mask; lin_lf = up_lf; lin_ol_kind = OB.kind; }
  // observation loss.  lf_w / lf_s2 exist from the first time a loss is set on (ol_arrays) and grow with the landmark factors.
  bool ol_arrays = false;
  size_t up_ol = 0;                            // landmark factors the arrays hold
  size_t lin_lf = 0;                           // the last linearisation covered lin_lf landmark factors, under the loss lin_ol_kind
  int lin_ol_kind = 0;
  DevArr<double> d_lf_w, d_lf_s2, d_ol_out;
  std::vector<uint64_t> h_gh_key;              // ghost factor -> key of its local pose
  size_t up_rbg = 0;                           // ghost factors the robust arrays hold (a batch's loss covers them)
  DevArr<double> d_gh_sigma0, d_gh_w, d_gh_s2;
  int restore_base_sigmas();                   // bt_sigma / gh_sigma <- sigma0 (a loss was set, cleared or left behind with a batch)
  // the read-backs' rows (host_loss.hip): ids -> keys (the graph keeps the maps the other way round), one closure or ghost factor's
  // row of the closure columns, the first `count` landmark factors' rows of the observation columns from row `at` on; ws: the
  // (weight, s^2) pairs of all rows as the kernel left them
  void inverse_keys(bool poses, bool lms, std::vector<uint64_t>& pkey, std::vector<uint64_t>& lkey) const;
  void closure_row(const ClosureCols& c, size_t k, int slot, const ClosureRec& rec, const double* ws) const;
  void ghost_row(const ClosureCols& c, size_t k, int slot, int gh, const double* ws) const;
  void observation_rows(const ObsCols& c, size_t at, int count, int slot, const double* ws) const;      // slot < 0: who = the pose's robot
  DevArr<double> d_bt_sigma0, d_bt_w, d_bt_s2, d_rb_out;
  DevArr<int> d_bt_kind, d_rb_idx;
  std::vector<int> h_gh_pose, h_gh_slot, h_gh_first; std::vector<double> h_gh_z, h_gh_sigma;   // ghost-between factors
  std::vector<int> h_gslot_pose;
  std::vector<int> h_lf_type, h_lf_pose, h_lf_lm, h_lf_slot;
  std::vector<int> h_lf_nbr;              // ids of the factors that are not bearing-range (GraphDev::lf_nbr)
  std::vector<int64_t> h_lf_joff, h_lf_eoff;
  std::vector<double> h_br_z, h_cu_z, h_cu_sigma, h_cy_z;
  int64_t jbuf_used = 0, ebuf_used = 0;
  std::vector<std::vector<int>> lm_fids, pose_fids, pose_bt;
  // host mirrors of their device CSR forms.  A streaming update touches the lists of the newest pose and of the few landmarks it
  // observes (the youngest ones: landmark ids grow with the first observation), so only the tail from the lowest touched list on is
  // rebuilt and uploaded (round 5: the three full rebuilds + the two per-factor tables were ~0.1 ms of host work and 350 KB of
  // upload per frame at 625 poses, growing with the graph).
  CsrMirror csr_lm, csr_pose, csr_bt;
  double* ei_final_out = nullptr; int ei_final_pose = -1; bool ei_final_done = false;      // run_update -> enqueue_iteration: the closing pack fused into k_estimate_predict
  std::vector<int> hc_pose_lms;           // per entry of the pose CSR: the factor's landmark
  std::vector<long long> hc_pose_ed;      // ... and its E record (offset << 4 | tangent dimension)
  int lm_first_from = 0;                  // h_lm_first changed from this landmark on since the last upload
  std::vector<int> h_lm_last, h_reach;    // per landmark the last observing pose; per pose the last pose it couples to (the profile's input)
  size_t up_P = 0, up_L = 0, up_pr = 0, up_bt = 0, up_lf = 0, up_br = 0, up_cu = 0, up_cy = 0, up_nbr = 0;
  int last_relin = 0;
  bool topo_dirty = true, uploaded_once = false;      // upload_new has work only after merge_pending consumed something

  DevArr<double> d_pose_val, d_pose_delta, d_pose_est, d_lm_val, d_lm_delta, d_lm_est;
  DevArr<int> d_lm_type;
  DevArr<int> d_pr_pose; DevArr<double> d_pr_z, d_pr_sigma, d_pr_r;
  DevArr<int> d_bt_i, d_bt_j; DevArr<double> d_bt_z, d_bt_sigma, d_bt_r, d_bt_J0;
  DevArr<int> d_gh_pose, d_gh_slot, d_gh_first, d_gslot_pose; DevArr<double> d_gh_z, d_gh_sigma, d_gh_r, d_gh_J, d_ghost_val;
  size_t up_gh = 0;
  DevArr<int> d_lf_type, d_lf_pose, d_lf_lm, d_lf_slot, d_lf_nbr;
  DevArr<int64_t> d_lf_joff, d_lf_eoff;
  DevArr<long long> d_pose_ed, d_sp_pairs;
  DevArr<int> d_sp_idx;                   // pair lists of the Schur assembly (GraphDev::sp_idx), rebuilt by upload_view for graphs in an exact joint batch
  int build_schur_pairs(hipStream_t s);   // plan_schur_pairs (host_layout.hpp) and its two uploads
  DevArr<unsigned> d_pose_adj;
  DevArr<double> d_br_z, d_cu_z, d_cu_sigma, d_cy_z, d_jbuf, d_ebuf;
  DevArr<int> d_lm_ptr, d_lm_fids, d_pose_ptr, d_pose_fids, d_pose_lms, d_pose_bt_ptr, d_pose_bt;
  DevArr<double> d_lm_Hinv, d_lm_g, d_pose_H, d_pose_g, d_lm_Hacc, d_lm_t;
  DevArr<int> d_sh_lid, d_sh_owner;
  std::vector<int> h_sh_lid, h_sh_owner;
  DevArr<double> d_S, d_Ld, d_Winv, d_yv, d_dp;
  DevArr<double> d_S0, d_pcg, d_pcg_scal;              // joint solve (pcg_kernels.hip)
  DevArr<int> d_lm_slot;                               // landmark -> shared slot or -1
  int sync_lm_slot();                                  // rebuilds it from h_sh_lid (upload_view, set_shared): plan_lm_slot (host_layout.hpp) and its upload
  bool lm_slot_onto = false;                           // plan_lm_slot's onto: lm_slot[h_sh_lid[i]] == i for every slot i that names a landmark (no two slots on one landmark, none out of range)
  DevArr<int> d_prof, d_first;                         // tile-level profile of the reduced system (plan_tile_profile, host_layout.hpp), host copies h_prof / h_first
  std::vector<int> h_prof, h_first;
  int prof_ver = 0;
  int joint_Tcap = 0;                                   // Tcap the joint-solve buffers (S0, L32, ctab) are allocated for; 0 = not allocated
  bool force_dense = getenv("SLIDE_CHOL_DENSE") && getenv("SLIDE_CHOL_DENSE")[0] == '1';
  DevArr<double> d_ctab;                               // explicit inverses of the diagonal blocks (k_chain_tables)
  DevArr<float> d_L32;                                 // packed f32 copy of the factor: the joint solve's preconditioner streams this
  DevArr<GraphDev> d_Gself;                             // this graph's view on the device, for the kernels that take an array of views
  GraphDev G_self{};
  bool have_self = false;
  int pcg_iters = 0;
  double pcg_tol = 0.0;
  // exact joint step: this robot's border, planned by plan_border (host_layout.hpp: BorderPlan describes every table below) and moved here
  std::vector<int> h_sep_off;                          // global offsets (n_slots + 1) or empty
  std::vector<int> h_lm_bord, h_sep_map, h_bfirst;     // landmark -> border offset; global separator coordinate -> border coordinate; first column block per border tile row
  // nested dissection of the own pose chain (exact joint passes; CholBatch::set_segments)
  using Seg = sl::Seg;                                 // tile columns [t0, t1) of a segment
  std::vector<Seg> segs;
  std::vector<int> h_pose_sep;                         // pose -> border offset of a separator pose, or -1
  std::vector<std::vector<int>> seg_prof;              // per segment: its profile in its own numbering (plan_segment_profiles; read by plan_step)
  DevArr<int> d_pose_sep, d_seg_prof;
  std::vector<size_t> seg_prof_off;
  std::vector<std::vector<int>> seg_ord, seg_sfirst;   // the per-segment activity of the border rows (BorderPlan; read by plan_step)
  std::vector<int> seg_tab;
  int seg_tab_head = 0;                               // ints of seg_tab in front of the per-column activity masks
  DevArr<int> d_seg_ord, d_seg_tab;
  int nsep = 0, nsep_dim = 0, n_sep_poses = 0;
  DevArr<double> d_Ld2, d_Winv2, d_yv2, d_dp2;
  std::vector<int> h_gh_gid, h_gh_bord;                // ghost factor -> index in the job's relative-pose list; -> border offset of its lambda coordinates
  int lam_total = 0;
  DevArr<int> d_lm_bord, d_sep_map, d_bfirst, d_gh_bord;
  DevArr<double> d_bord, d_bord0, d_xloc;
  int nbr = 0, nbr_alloc = -1, arrow_T = -1;
  bool arrow_on() const;                               // the batch runs exact joint passes and this graph has shared slots + separator offsets
  int sync_self();
  DevArr<int> d_cctr;
  DevArr<double> d_covY;
  bool factor_valid = false;            // S / Ld / Winv hold the factor of the system of the last solve
  // What a streaming update leaves for the next one besides the factor: its prediction of the next relinearisation, the zeroed status
  // words and the cached newest pose.  They describe the device as that update left it, so whatever else writes deltas, estimates or
  // status words (a pass of any other kind, chi2, a changed loss or batch) drops all three together.
  void drop_stream_state() { pred_valid = false; status_clean = false; cache_pose = -1; }
  // The resident factor and the solution kept for the bounded back-substitution are of one system: what makes the factor another
  // system's (a changed weighting, batched or sharded passes factoring into the same S) makes dp no previous solution either.
  // Outside a successful run_update the two are cleared together.  (Two sites clear them apart, as they always have: chi2 drops dp
  // where it folds delta in and the factor only once it has succeeded, dist_pass_local drops dp alone.)
  void drop_factor() { factor_valid = false; wf_T = 0; }
  unsigned long long fact_serial = 0;   // +1 whenever a solve leaves a new factorisation
  size_t fact_shape[8] = {};            // what that factorisation was of: T, ld, the uploaded counts (marginal_state compares)
  void fact_shape_now(size_t* out) const;
  unsigned long long sig_serial = ~0ull;     // the factorisation d_sig is the selected inverse of ...
  int sig_T = -1, sig_ld = -1;               // ... and its geometry
  DevArr<double> d_sig;                 // Sigma = S^-1 on the tile profile (S's layout and ld)
  DevArr<double> d_mout, d_igB, d_igU, d_igV, d_igM;
  DevArr<int> d_midx, d_igrc;
  DevArr<double> d_igval;
  int marginal_state(const char* who) const;      // SLIDE_ERR_INVALID (+ message) unless a single-graph factorisation is resident
  int sigma_forms(const char* who, int ncand, int nk, const FormFill& fill, const FormDone& done, const FormStart& start = nullptr);
  void form_backend(FormBackend& be, const FormStart& start);      // this graph's back end of the quadratic-form drivers
  int ensure_sigma();
  int pose_id(int robot, uint64_t idx) const;     // the uploaded pose's index, or -1
  void robot_poses(int robot, std::vector<int>& out) const;
  void point_landmarks(std::vector<int>& out) const;
  DevArr<int> d_status;
  UploadBatch ub;
  CholBatch* batch = nullptr;           // shared factor + solve with the other graphs of this GPU (not owned)
  int batch_slot = 0;
  int factor_and_solve(hipStream_t s);  // the Cholesky part of a pass: own launches, or the batch's
  int Tcap = 0;
  // hipGraph of one pass, captured when the same resident graph is solved repeatedly (kernel arguments are
  // baked in, so any change of counts / pointers / threshold invalidates it)
  hipGraphExec_t gexec = nullptr;
  GraphDev G_cap{};
  GraphDev G_prev{};
  RobustDev RB_cap{}, RB_prev{};      // (the captured pass bakes the robust view in as well)
  ObsLossDev OB_cap{}, OB_prev{};     // (and the observation loss's)
  struct PhaseGraph { hipGraphExec_t exec = nullptr; GraphDev G{}; double* buf = nullptr; };
  PhaseGraph phase_graph[5];             // captured launch sequences of dist_phase 0 / 1 / 2 and of phase 1's halves (3, 4)
  int enqueue_phase(int phase, double* d_buf);
  int launch_phase(int phase, double* d_buf);      // hipGraph replay of enqueue_phase when nothing changed
  bool have_prev = false;
};

// slide_pairs_within (host_gates.hip, pairs_kernels.hip): every pair i < j of n host points within radius, sorted by (i, j);
// arguments checked by the C ABI
int pairs_within_host(const double* xyz, const int32_t* label, int n, double radius, int64_t cap, int32_t* out_i, int32_t* out_j, double* out_dist,
                      int64_t* n_pairs);

}  // namespace sl
