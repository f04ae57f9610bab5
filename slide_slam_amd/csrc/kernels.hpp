// Launch wrappers of the HIP kernels (definitions in *_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <vector>

#include "graph_dev.hpp"
#include "sl_math.hpp"

namespace sl {

// solver_kernels.hip
void init_solver_kernels();   // one-time kernel attributes (call outside stream capture)
void launch_relin(const GraphDev& G, hipStream_t s);
void launch_linearize(const GraphDev& G, const ObsLossDev& O, hipStream_t s);      // O.kind != 0: the landmark factors under the observation loss (same launch count)
void launch_observation_weights(const GraphDev& G, const ObsLossDev& O, bool robust, int n, double* out2n, hipStream_t s);      // (weight, s^2) of landmark factors [0, n)
// the same for the members of a batch in one launch (dO: their ObsLossDev table beside d; off / cnt: host arrays, member i writes its
// factors [0, cnt[i]) behind off[i] rows of out2n)
void launch_observation_weights_batched(const GraphDev* d, const ObsLossDev* dO, bool robust, const int* off, const int* cnt, int n, double* out2n,
                                        hipStream_t s);
void launch_robust_reweight(const GraphDev& G, const RobustDev& R, hipStream_t s);      // ahead of launch_linearize while a robust loss is set (no launch otherwise)
void launch_closure_weights(const GraphDev& G, const RobustDev& R, const int* idx, int n, double* out2n, hipStream_t s);   // (weight, s^2) of the listed between factors
// the batch's robust loss (dR: the members' RobustDev table beside d): k_robust_reweight_b between k_relin_b and the linearisation
// of launch_phase0_batched (its dR argument; null: no launch); (weight, s^2) of the listed (member, factor) pairs, a member's ghost
// factors numbered behind its between factors
void launch_robust_reweight_batched(const GraphDev* d, const RobustDev* dR, const GraphDev* h, int n, hipStream_t s);
void launch_closure_weights_batched(const GraphDev* d, const RobustDev* dR, const int* ent2, int n, double* out2n, hipStream_t s);
void launch_landmark(const GraphDev& G, int mode, hipStream_t s);      // mode: 0 fused, 1 accumulate, 2 finish from sums
void launch_pose(const GraphDev& G, hipStream_t s);
void launch_schur(const GraphDev& G, hipStream_t s);
void launch_backsub(const GraphDev& G, int mode, hipStream_t s);       // mode: 0 fused, 1 t_l only, 2 delta_l from t_l
void launch_shared_pack(const GraphDev& G, int what, double* buf, hipStream_t s);
void launch_shared_unpack(const GraphDev& G, int what, const double* buf, hipStream_t s);
void launch_estimate(const GraphDev& G, hipStream_t s);
void launch_estimate_predict(const GraphDev& G, hipStream_t s, int pose = -1, double* out17 = nullptr);      // out17 (or null): the closing pack of k_final_pack by the last workgroup — 16 doubles + an arrival counter (zero before the launch)
void launch_final_pack(const GraphDev& G, int pose, double* out16, hipStream_t s);      // out16: 8 status ints (then cleared) | pose_est of `pose` (12 doubles)
void launch_chi2(const GraphDev& G, double* out4, hipStream_t s);   // sum of squared whitened residuals at the last linearisation point
void launch_pose_adj(const GraphDev& G, hipStream_t s);        // pose adjacency bitmap of the Schur assembly (topology only)
void launch_scatter(const void* stage, unsigned desc_off, int nseg, hipStream_t s);
void launch_gather(void* stage, unsigned desc_off, int nseg, hipStream_t s);
void launch_gather_args(void* stage, const void* segs, int nseg, hipStream_t s);      // the same, up to 16 descriptors as kernel arguments
void launch_sum_bcast(double* const* bufs, int n, int count, hipStream_t s);   // local all-reduce(sum) of up to 8 buffers
void launch_bcast(double* const* bufs, int n, int count, hipStream_t s);       // bufs[0] -> the others
void launch_phase0_batched(const GraphDev* d, const GraphDev* h, int n, double* const* bufs, hipStream_t s, bool pack = true, const RobustDev* dR = nullptr,
                           const ObsLossDev* dO = nullptr);   // the per-robot phases 0 / 4 / 2 of a batched pass (dO: the batch's observation loss, k_lin_lf_robust_b in k_lin_lf_b's place),
void launch_linearize_batched(const GraphDev* d, const GraphDev* h, int n, hipStream_t s, const ObsLossDev* dO = nullptr);      // phase 0's linearisation launch alone
void launch_phase4_batched(const GraphDev* d, const GraphDev* h, int n, double* const* bufs, hipStream_t s);   // blockIdx.z = robot
void launch_phase2_batched(const GraphDev* d, const GraphDev* h, int n, double* const* bufs, hipStream_t s);
void launch_phase3_batched(const GraphDev* d, const GraphDev* h, int n, double* const* bufs, hipStream_t s);   // blockIdx.z = robot               // local all-reduce(sum) of up to 8 buffers             // device arrays -> one staging buffer (DownloadBatch)   // staged upload -> destinations (UploadBatch)
void launch_ghost_exchange(const GraphDev& G, int what, double* buf, hipStream_t s);   // what: 0 pack owned poses, 1 adopt
void launch_ghost_exchange_batched(const GraphDev* d, int n, int n_gslots, int what, double* const* bufs, hipStream_t s);   // all robots of a batched pass in one launch
// exact joint step ("arrow", graph_dev.hpp): border rows + border block of every robot; the separator system of all shared landmarks
// gathered from the robots' border blocks (maps[i]: m ints, global separator coordinate -> robot i's border coordinate or -1); its
// solution handed back
void launch_border_assemble_batched(const GraphDev* d, const GraphDev* h, int n, hipStream_t s, bool clear = true, bool fills = true);      // the separate launches: what launch_phase3_arrow_batched did not merge
void launch_sep_extract_batched(const GraphDev* d, const GraphDev* h, int n, const int* n_sep_poses, hipStream_t s);      // separator poses out of the band (k_sep_extract_b)
void launch_sep_pose_scatter_batched(const GraphDev* d, const GraphDev* h, int n, double* const* xloc, hipStream_t s);  // their solution into dp
// Separator system: Ts tile columns of landmark coordinates (ms real) in sys (ld = (Ts + nl + 1) * NB: band, nl border row tiles = the
// coupling rows of the lam "lambda" coordinates of the inter-robot relative-pose factors, right-hand-side tile row), the lambda x lambda
// block + its right-hand-side row in bord (ldb = (nl + 1) * NB); packed: the exchange buffer (lower tile columns of the whole)
struct SepLayout { double* sys; double* bord; double* packed; int Ts, nl, ms, lam; int gap[4]; int hTa, hTL; };      // gap: two ranges [lo, hi) of landmark coordinates no slot uses (padding between the blocks of a dissected layout): unit diagonal; hTa, hTL: tile rows [hTa, hTL) of the tile columns < hTa are structurally zero (leaf b's rows under leaf a's columns) and absent from the packed layout
void launch_ghost_refresh_local(const GraphDev* d, int n, int n_gslots, hipStream_t s);      // ghost poses of a whole pass on one GPU: pack + sum + adopt in one launch
void launch_copy_pairs(const double* const* src, double* const* dst, const int* count, int n, hipStream_t s);      // up to 8 small device-to-device copies in one launch
void launch_sep_gather(const GraphDev* h, int n, const int* const* maps, const SepLayout& Y, bool packed, hipStream_t s, const int* tmask = nullptr,
                       int split_col = -1, unsigned mask_b = 0, double* sys2 = nullptr, int ld2 = 0, double* bord2 = nullptr);      // tmask: Ts + nl ints, bit r = robot r holds a coordinate of the (virtual) tile; split_col ..: per-half partial sums of the top block (k_sep_gather)
void launch_sep_top_add(const SepLayout& Y, int c0, const double* sys2, int ld2, const double* bord2, hipStream_t s);      // tile columns >= c0 of the system (and the lambda block) += the other half's partial
void launch_sep_unpack(const SepLayout& Y, hipStream_t s, int c0 = 0, int c1 = -1, bool to_packed = false);      // tile columns [c0, c1) (virtual: lambda tiles behind the landmarks'); to_packed: the reverse copy
void launch_lam_prepare(const double* bord, int nl, int lam, double* out, hipStream_t s);      // M = -(K22 - L21 L21^T), rhs = -(r2 - L21 z1)
// elements (r, c0 + u * cstride), u < N, of that (k_lam_prepare in solver_kernels.hip: N = 1; k_lam_solve1 in chol_kernels.hip): row r
// of the nl tile columns, r = nl * NB the right-hand-side row; the negated entry, unit diagonal on the padding.  The N loads are issued
// together, then the stores.
template <int N>
__device__ __forceinline__ void lam_prepare_elems(const double* __restrict__ bord, int nl, int lam, double* __restrict__ out, int r, int c0, int cstride) {
  const int NT = nl * NB, ld = (nl + 1) * NB;
  if (r > NT) return;
  const bool rhs = r == NT;
  double v[N];
#pragma unroll
  for (int u = 0; u < N; ++u) {
    const int c = c0 + u * cstride;
    const bool live = c < NT && (rhs || r >= c);
    v[u] = (r == c) ? 1.0 : 0.0;
    if (live && c < lam && (rhs || r < lam)) v[u] = -bord[(size_t)c * ld + r];
  }
#pragma unroll
  for (int u = 0; u < N; ++u) {
    const int c = c0 + u * cstride;
    if (c < NT && (rhs || r >= c)) out[(size_t)c * ld + r] = v[u];
  }
}
void launch_sep_xloc(int n, const int* const* maps, int ms, int lam, const double* xs, const double* xl, double* const* xloc, hipStream_t s);
void launch_arrow_finish_batched(const GraphDev* d, const GraphDev* h, int n, const double* xs, const int* sep_off, hipStream_t s, bool slots_onto);      // slots_onto: lm_slot reaches every slot of every graph (HostGraph::lm_slot_onto)
struct AsmMerge { int mask; };                   // SLIDE_ASM_MERGE (default 6) — solver_kernels.hip, launch_phase3_arrow_batched
AsmMerge asm_merge_env();                        // read on every call: the launch sequence of a pass takes them when it is built
void launch_phase3_arrow_batched(const GraphDev* d, const GraphDev* h, int n, hipStream_t s);   // phase 3 without the exchanged sums: the robots' own H_ll

// chol_kernels.hip — blocked right-looking FP64 Cholesky of the (T*NB)^2 lower matrix S (column-major,
// leading dimension ld = (T+1)*NB; the extra row tile carries the right-hand side), tile edge NB = 64.
// ctr: T + 2 ints, zero before the first factorisation (each step clears the next step's work counter itself)
void launch_chol_step(double* S, int ld, int k, int T, double* Ld, double* Winv, int* status, int* ctr, float* L32, const int* h_prof, hipStream_t s, int nbr = 0);   // L32, h_prof: see CholSystem
void launch_chol_extract_y(const double* S, int ld, int T, double* yv, double* dp, int* status, hipStream_t s, int nbr = 0, int b0 = 0, double* prev = nullptr);   // prev: dp's old content is kept there (bounded back-substitution)   // also clears status[4], the ticket counter of launch_chol_bwd_all
// A quiet-NaN payload no solution value can equal bit for bit: the outputs of the chained substitutions are pre-filled with it and the
// workgroups poll the blocks they depend on ("flag in data").
constexpr unsigned long long CHAIN_SENTINEL = 0x7FF8DEADBEEF0BADull;
struct CholSystem { double* S; int ld, T; double* Ld; double* Winv; double* yv; double* dp; int* status;
                    float* L32;      // packed f32 copy of the factor for the joint solve's preconditioner (null: none), see bwd_chain_body
                    const int* h_prof;           // host: profile of the factor, T ints (plan_step in chol_kernels.hip), or null = dense
                    const int* prof; const int* first;      // device: the same and, per block row, the first block column that reaches it
                    double* ctab;                // 4 * T * 4096 doubles: tables of the chained substitutions in a joint-solve pass (k_chain_tables), or null
                    int nbr;                     // border row tiles between the band and the right-hand-side row (exact joint step: the separator's coupling rows), see b_decode
                    double* bord; int ldb;       // border x border block of the system ((nbr + 1) * NB rows, nbr * NB columns, column-major) — k_border_syrk
                    const double* bord_src;      // or null: the block's content BEFORE the product lives there (same layout) and k_border_syrk WRITES bord = bord_src - W W^T (GraphDev::bord0)
                    const int* bfirst;           // device, nbr + 1 ints: first block column of the band in which border tile row i can be non-zero (non-decreasing)
                    const int* h_bfirst;         // host copy (plan_step: the border rows still all-zero at a block column are skipped) or null: every row always
                    int b0;                      // tile row (in the system's own row numbering) at which its border rows start; 0: right behind the band (= T).  A SEGMENT of
                                                 // a robot's band factored as a system of its own (a view: shifted S, profile) has its border further down: b0 = T_robot - first tile
                    int kofs;                    // the view's first block column in the robot's numbering (bfirst is in that numbering)
                    const int* ord;              // device, nbr ints, or null: the j-th ACTIVE border row of this view is tile row b0 + ord[j] (a segment has its own order
                                                 // of first columns: h_bfirst is then that segment's sorted list)
                    const int* segtab; };        // device or null (border product of a segmented band): nseg, the segments' end columns, per segment the first column of
                                                 // every border tile row + the right-hand side (1 << 30: the row is zero in that segment)
constexpr int CHOL_STEP_BATCH_MAX = 32;      // systems per launch of the batched step kernel (the segments of eight robots' bands in one launch sequence)
void launch_chol_batch(const CholSystem* d, int n, int* ctr, hipStream_t s, hipEvent_t after_steps = nullptr, bool solve = true, int cu_share = 100, int* pair_tickets = nullptr);      // pair_tickets (CHOL_STEP_BATCH_MAX ints, zero, used by no other launch sequence at the same time): two block columns per launch (k_chol_pair_batched) when the systems allow it (chol_pair_supported)
// Test hook of launch_chol_batch's launch shapes (slide_debug_chol_batch / slide_debug_chol_plan).  While a CholPlanHook lives, on the
// thread that made it: the launches are planned for n_cu compute units (0: the device's own), every launch issued appends
// {k, a_split, a_joins, type-A workgroups, queue items} to `trace`, and with dry set nothing is launched at all (no device is touched when
// n_cu > 0).  Scoped: the destructor puts back what was there before.  Without one launch_chol_batch tests one thread-local pointer per launch.
struct CholPlanHook {
  int n_cu; bool dry; std::vector<int> trace;
  CholPlanHook(int n_cu_, bool dry_);
  ~CholPlanHook();
  CholPlanHook(const CholPlanHook&) = delete;
  CholPlanHook& operator=(const CholPlanHook&) = delete;
private:
  CholPlanHook* prev;
};
int chol_device_cus();                         // compute units of the current device (what the launches are planned for without a hook)
bool chol_pair_supported(const CholSystem* d, int n);           // up to 8 systems, one launch per block column; solve = false: steps + extraction of y only; cu_share: percent of the CUs this launch sequence may count on (sequences running side by side)
void launch_chol_bwd_batch(const CholSystem* d, int n, hipStream_t s);       // yv -> dp of up to 8 factored systems (chained backward substitution)
// Left-looking persistent factorisation (k_chol_ll): ALL block columns of the n systems in ONE launch, the kernel boundary per block
// column replaced by flags between workgroups that start in ticket order.  The plan (task table, flags, device copies of the systems'
// parameters) depends on the systems' pointers, profiles and border tables: rebuild it when any of them changes.  h_ord[i]: host copy of
// d[i].ord (or null).  launch_chol_ll = the steps of launch_chol_batch(.., solve = false): factorisation + extraction of y.
struct CholLLPlan;
CholLLPlan* chol_ll_plan_create(const CholSystem* d, int n, const int* const* h_ord = nullptr, hipStream_t upload_stream = nullptr);
void chol_ll_plan_destroy(CholLLPlan* p);
int chol_ll_plan_tasks(const CholLLPlan* p);
int chol_ll_plan_columns(const CholLLPlan* p);
void launch_chol_ll(const CholLLPlan* p, const CholSystem* d, int n, hipStream_t s, int* trace = nullptr);      // trace: diagnostic, 16 host-pinned ints per task (ll_mark / ll_time) or null
// Exact joint step (the border of the systems = the separator's coupling rows, W^T after the steps):
void launch_border_syrk(const CholSystem* d, int n, hipStream_t s, double* scratch = nullptr, int ks = 1, bool reduce = true);          // bord(i, j) -= sum_c W^T(i, c) W^T(j, c)^T, i >= j, right-hand-side row included; scratch + ks: split K (one system); reduce = false: the chunks' partials stay in scratch for the caller's own reduction (launch_lam_solve1)
// SLIDE_LAM_FUSE, a bit mask read whenever a pass's launch sequence is built (one process can take both sides): 1 = the lambda block's
// products over the two leaves ride in the launch of the top block's (a canonical whole pass), 2 = a lambda block of one tile is reduced,
// factored and solved by ONE workgroup (k_lam_solve1).  Default 3; 0 = the separate launches.
struct LamFuse { int mask; };
LamFuse lam_fuse_env();
// sep_nl == 1, behind launch_border_syrk(.., scratch, ks, false) over Tsum column blocks: bord += the partials (k_border_syrk_reduce's
// order), S = -bord padded (k_lam_prepare), its factorisation (the k_chol_step of T = 1), yv / dp (k_chol_extract_y), dp = the solution
// (k_chol_bwd_chain) — one launch of one workgroup; scratch null or ks <= 1: the product was not split
void launch_lam_solve1(double* bord, int ks, const double* scratch, int Tsum, int lam, double* S, double* Ld, double* Winv, double* yv, double* dp,
                       int* status, int* ctr, hipStream_t s);
void launch_border_syrk_jobs(const CholSystem* d, int n, const int* jobs, int njobs, int lds_pad, hipStream_t s, double* scratch = nullptr, int ks = 1, int jb_end = -1,
                             const int* ks_sys = nullptr, bool fuse_add = false);      // fuse_add (n = 2, same border): system 0's block += system 1's, each split its own way (ks_sys)      // the same, workgroups in the order of a job table (system << 20 | ib << 10 | jb), lds_pad bytes of idle LDS per workgroup (bounds the residency)
// two fuse_add pairs in ONE product launch and ONE reduction (a canonical whole pass with lambdas): top[0..1] = systems 0, 1 of the job
// table (tile columns jb < jb_end, ks_top chunks each), lam[0..1] = systems 2, 3 (ks_lam[r] chunks), each pair with its own scratch
void launch_border_syrk_pairs(const CholSystem* top, const CholSystem* lam, const int* jobs, int njobs, hipStream_t s, double* scratch_top,
                              int ks_top, int jb_end, double* scratch_lam, const int* ks_lam);
void launch_border_apply(const CholSystem* d, int n, const double* const* xloc, hipStream_t s);   // yv -= W x_loc (x_loc: nbr * NB doubles per system)
// one of the two triangular solves with the finished factors of up to 8 systems on arbitrary vectors (T * NB doubles each): out = L^-1 in
// (fwd) or L^-T in (bwd); the preconditioner of the joint solve (pcg_kernels.hip)
void launch_chain_batch(const CholSystem* d, int n, const double* const* in, double* const* out, bool fwd, bool f32, bool prepared,
                        double* const* next_out, hipStream_t s);   // needs the tables (launch_chain_tables) of this factorisation
void launch_chain_tables(const CholSystem* d, int n, hipStream_t s);
void launch_chol_bwd_all(const double* S, int ld, int T, const double* Ld, const double* Winv, double* yv, double* dp, int* status, const int* prof, hipStream_t s,
                         const double* wf_prev = nullptr, double wf_thr = 0.0, int wf_Tprev = 0, int wf_lim = -1);      // wf_*: iSAM2's wildfire bound (bwd_chain_body): blocks whose inputs changed by < wf_thr keep wf_prev; status[7] / status[3] must be 0
// marginal covariance of the pose whose first tangent row is row0 (Y: 6 * T * NB scratch doubles holding the six unit columns)
void launch_pose_covariance(const double* S, int ld, int T, const double* Ld, const double* Winv, double* Y, int row0, double* cov36,
                            hipStream_t s);
// cov_kernels.hip — selected inverse Sigma = S^-1 on the tile profile (prof: host copy, null = dense; d_prof its device copy) into Sg,
// with Z (S's size) as scratch; marginal blocks out of it; many right-hand sides on the factor; the information-gain products
void launch_selected_inverse(const double* S, int ld, int T, const double* Ld, const double* Winv, const int* prof, const int* d_prof,
                             double* Sg, double* Z, hipStream_t s);
// its first launch alone (k_sinv_prep: Z and the diagonal tiles' L_kk^-T L_kk^-1); launch_selected_inverse starts with this call
void launch_selected_inverse_prep(const double* S, int ld, int T, const double* Ld, const double* Winv, const int* prof, const int* d_prof,
                                  double* Sg, double* Z, hipStream_t s);
void launch_pose_blocks(const double* Sg, int ld, const int* poses, int n, double* out, hipStream_t s, const int* prow = nullptr);     // out: 36 per pose; prow: a pose's first row (null: 6 p)
void launch_landmark_covariances(const GraphDev& G, const double* Sg, int ld, const int* lids, int n, double* out, hipStream_t s,
                                 const int* prow = nullptr);      // out: 81 per landmark (d x d used)
void launch_multi_solve(const double* S, int ld, int T, const double* Ld, const double* Winv, const int* prof, double* B, double* X,
                        int nrhs, hipStream_t s);      // X = S^-1 B (B: nrhs columns of T * NB rows, overwritten)
// the forward half of launch_multi_solve on its own: W = L^-1 B (S = L L^T; B overwritten), so that B^T S^-1 B = W^T W
// (k0: the first block column walked — the caller knows B is zero above row k0 * NB and has zeroed those rows of W)
void launch_multi_fwd(const double* S, int ld, int T, const double* Ld, const double* Winv, const int* prof, double* B, double* W,
                      int nrhs, hipStream_t s, int k0 = 0);
void launch_gram(const double* X, size_t ldx, int ncol, const int* rows, int nrows, double* M, hipStream_t s);
void launch_landmark_V(const GraphDev& G, const double* U, int nT, int ncol, const int* lids, int n, double* V, size_t ldv, hipStream_t s,
                       const int* prow = nullptr);      // prow: a pose's first row in U (null: 6 p)
void launch_scatter(const int* rc, const double* val, int n, double* B, int nT, hipStream_t s);
// Many candidates in one sweep (closure_info_gain_batch): candidate k owns the columns c0 .. c0 + nk - 1 of U.  moff: its nk x nk block
// in each gram; poff: its nsplit partial blocks (nsplit = gain_gram_splits(nk)); woff: its nk x nk slice of the Woodbury work buffer
// (used past GAIN_LDS_DIM columns; smaller candidates are factored in LDS)
constexpr int GAIN_MAX_STEPS = 64, GAIN_MAX_GRAMS = 4, GAIN_LDS_DIM = 96;
struct GainCandDev { int c0, nk, nsplit, pad; long long moff, poff, woff; };
int gain_gram_splits(int nk);
// M_k = sum over the rows (the list, or null: 0 .. nrows - 1) of X_k^T X_k per candidate; jobs {candidate, tile row, tile column, split}
void launch_gram_blocks(const double* X, size_t ldx, const int* rows, int nrows, const GainCandDev* cand, int ncand, const int4* jobs,
                        int njobs, double* part, double* M, hipStream_t s);
// per candidate: C = I + J U (J by columns of J^T: jptr / jrow / jval), its Cholesky factor, gains[GAIN_MAX_GRAMS k + q] = tr(C^-1 M_q)
// (M_q at M + q msz), flag[k] = 1 where C is not positive definite; non-zero: the device refused the kernel's LDS, nothing launched
int launch_woodbury_blocks(const double* U, size_t ldu, const GainCandDev* cand, int ncand, const int* jptr, const int* jrow,
                           const double* jval, const double* M, size_t msz, int nM, double* work, double* gains, int* flag, bool small,
                           bool big, hipStream_t s);
// joint_cov_kernels.hip — the selected inverse over the exact joint pass's elimination tree (CholBatch::ensure_joint_sigma).  One system:
// factor columns [0, Tb) in S (ld; rows past Tb = its stored border rows), [Tb, Tc) in B (ldb, rows and columns counted from Tb); their
// diagonal blocks in Ld / Winv and Ld2 / Winv2; D = -I on the columns >= neg0; Sigma and Z dense lower with leading dimension lds.
// col0: the system's first entry in the row-list offsets rp (rp[col0 + c] .. rp[col0 + c + 1] index the tile rows of column c)
struct JSinvSys { const double* S; int ld, Tb; const double* B; int ldb; const double *Ld, *Winv, *Ld2, *Winv2; int neg0, col0;
                  double* Sg; double* Z; long long lds; };
// per robot r: dst[r] (its Sigma, leading dimension lds[r]) rows / columns o0[r] .. o0[r] + n[r] - 1 <- src through map[r] (-1: zero)
constexpr int JSIG_ROBOTS_MAX = 8;      // (a CholBatch's slots)
struct JSigGather { double* dst[JSIG_ROBOTS_MAX]; const int* map[JSIG_ROBOTS_MAX]; long long lds[JSIG_ROBOTS_MAX]; int o0[JSIG_ROBOTS_MAX], n[JSIG_ROBOTS_MAX];
                    const double* src; long long lds_src; };
void launch_jsinv_prep(const JSinvSys* d_sys, const int2* d_jobs, int njobs, int max_rows, const int* d_rp, const int* d_rows, hipStream_t s);
void launch_jsinv_step(const JSinvSys* d_sys, const int2* d_jobs, int njobs, int max_rows, const int* d_rp, const int* d_rows, hipStream_t s);   // two launches
void launch_jsig_gather(const JSigGather& A, int n_robots, int max_n, hipStream_t s);
void launch_sym_blocks(const double* Sg, size_t ld, const int* row0, const int* dim, int n, double* out, hipStream_t s);      // out: 81 per block (d x d used)
// X = K^-1 B over the same tree (CholBatch::joint_closure_info_gain): every system's right-hand sides R (JSinvSys::Z, B to start with)
// and solutions S (JSinvSys::Sg, X at the end) in column-major buffers with leading dimension lds.  Jobs {system, tile, list begin, list
// end}.  push: one column of each job's node, applied to the list's rows (forward) / columns (backward) of that node; pull: the rows of
// the nodes below (forward) / above (backward) a tile, the backward one with the D step.  sum: separator rows of R from the robots'
// (CSR of (robot, row) per separator row).  gather: the robots' rows of separator coordinates of S from the separator's.
struct JMSum { const double* src[JSIG_ROBOTS_MAX]; double* dst; long long ld; };
void launch_jms_push(const JSinvSys* d_sys, const int4* d_jobs, int njobs, int max_list, const int* d_list, int ncol, bool bwd, hipStream_t s);
void launch_jms_pull(const JSinvSys* d_sys, const int4* d_jobs, int njobs, const int* d_list, int ncol, bool bwd, hipStream_t s);
void launch_jms_sum(const JMSum& A, const int* d_ptr, const int2* d_ent, int nrows, int ncol, hipStream_t s);
void launch_jms_gather(const JSigGather& A, int n_robots, int max_n, int ncol, hipStream_t s);      // dst[r][o0 + a] = src[map[r][a]], every column
// stand-alone dense SPD solve on device buffers (used by the unit tests and the roofline bench leg)
void launch_chol_solve_bwd(const CholSystem& cs, hipStream_t s);   // yv -> dp after launch_chol_extract_y: one-workgroup substitution for narrow profiles, else the chained kernel
int chol_factor_solve(double* S, int ld, int T, double* Ld, double* Winv, double* yv, double* dp, int* status, int* ctr, hipStream_t s);

// pcg_kernels.hip — joint Gauss-Newton step of the robots of a GPU (and, through the caller's exchanges, of the job): PCG on the
// global reduced pose system with the robots' own factors as preconditioner.  d: device array of the n graphs' views, h: host copy.
enum { PCG_VEC_R = 0, PCG_VEC_U = 1, PCG_VEC_W = 2, PCG_VEC_P = 3, PCG_VEC_S = 4, PCG_VEC_X = 5, PCG_VEC_Y = 6, PCG_VEC_COUNT = 7 };
void launch_status_clear(const GraphDev* d, int n, hipStream_t s, int* x0 = nullptr, int* x1 = nullptr);      // x0 / x1: two more 8-word status blocks cleared in the same launch             // status[0..7] = 0 for every graph of the batch
void launch_status_gather(const GraphDev* d, int n, int* out, hipStream_t s, const int* x0 = nullptr, const int* x1 = nullptr);      // x0 / x1: OR-ed into graph 0's flags first  // out[8 i ..] = graph i's status words
void launch_ints_clear(int* p, int n, hipStream_t s);                          // p[0 .. n-1] = 0 (a kernel node: see launch_status_clear)
void launch_status_or(int* dst, const int* src, int n, hipStream_t s);         // dst[i] |= src[i]
void launch_pcg_init(const GraphDev* d, const GraphDev* h, int n, hipStream_t s);
void launch_pcg_tl(const GraphDev* d, const GraphDev* h, int n, double* const* bufs, int vec, hipStream_t s);      // t_l -> bufs[i][9 slot ..], and w = S0 v in the same launch
void launch_pcg_matvec_dots(const GraphDev* d, const GraphDev* h, int n, double* const* bufs, int nsum, hipStream_t s);     // bufs: summed t_l in, (gamma, delta) partials out (w = S0 u ran in launch_pcg_tl)
void launch_pcg_update(const GraphDev* d, const GraphDev* h, int n, double* const* bufs, int nsum, hipStream_t s);          // bufs: summed (gamma, delta) in
void launch_pcg_finish(const GraphDev* d, const GraphDev* h, int n, hipStream_t s);

// assoc_kernels.hip
struct AssocFrameDev {
  // map of one class, resident in HBM
  const float *cx, *cy, *cz; // n each: first-seen float32 positions, SoA (K-NN gate)
  const double* model;       // cyl: 7 n (root ray radius) ; box: 3 n (xyz)
  const int32_t* label;      // n
  int n;
  int K;
  int gate;                  // 1: K-NN gate; 0: the submap is the whole map in the caller's order (stand-alone matchers)
  int Kp, cached, staged;    // LDS plan of the gate (assoc_plan)
  double thresh;
  double best_init;          // sloam.cpp:90 / :128,136 / :176,180
  int label_gate;            // 0 none (cubes), 1 skip unless equal (ellipsoids), 2 distance = 1000 (cylinders)
  int is_cyl;
  // detections of this frame (body frame) and the pose estimate
  const double* det;         // cyl: 7 per (root ray radius) ; box: pose12 (R t) per detection
  const int32_t* det_label;
  int n_det;
  // outputs
  double* det_world;         // same layout as det
  int32_t* match_sub;        // submap index or -1
  int32_t* match_map;        // map index or -1
  int32_t* submap;           // K entries: map indices nearest first (matchesMap_)
  int32_t* n_sub;            // 1
};
// LDS plan of one class for the K-NN gate: sort buffer length Kp (power of two >= min(K, n)), whether the n distance words are cached
// in LDS, dynamic LDS bytes.  false: min(K, n) exceeds ASSOC_MAX_K.  The cloud itself may be of any size.
bool assoc_plan(int n, int K, int gate, int model_stride, int* Kp, int* cached, int* staged, size_t* bytes);
void launch_assoc_frame(const AssocFrameDev* classes3, size_t lds_bytes /* max over the three classes */, const double* pose12, hipStream_t s);
int launch_assoc_sweep(const float* cx, const float* cy, const float* cz, const double* model_xyz, const int32_t* label, int n_map,
                       const double* query_pos, const double* obs_xyz, const int32_t* obs_label, int n_query,
                       int n_obs, int K, double thresh, int32_t* out_map_idx, hipStream_t s);     // -1: K beyond ASSOC_MAX_K
void launch_map_refresh(double* cyl_model, int n_cyl, const int* cyl_lid, double* cube_xyz, int n_cube, const int* cube_lid,
                        double* ell_xyz, int n_ell, const int* ell_lid, const double* lm_est, hipStream_t s);
constexpr int ASSOC_MAX_K = 16384;                 // neighbours kept by the K-NN gate (LDS sort buffer); the cloud is unbounded
constexpr int ASSOC_LDS_BUDGET = 140 * 1024;      // dynamic part; the select keeps another 16 KB of per-wave histograms (static)

// place_kernels.hip
struct PlaceDev {
  const double* ref7; int nr;
  const double* qry7; int nq;
  const double* xs; const double* ys; const double* yaws;   // candidate lattice values
  const int32_t* cell_x; const int32_t* cell_y;             // per cell indices into xs / ys
  long long n_cells; int n_yaw;
  double thr_pos, thr_dim; int ignore_dim;
  int32_t* inliers;                                         // n_cells * n_yaw
  // round 5 (k_place_sweep_b): both maps bucketed by label on the host (stable: the reference's first-hit order inside a label is kept)
  const double* rxy;       // 2 nr: (x, y) of the reference objects, bucket after bucket; null: the plain kernel
  const double* rdim;      // 3 nr: their dimensions (read when !ignore_dim)
  const double* qxy;       // 2 nq: (x, y) of the query objects, ordered by the bucket of their label
  const double* qdim;      // 3 nq
  const int32_t* qrange;   // 2 nq: [lo, hi) = the reference bucket a query object scans (empty when the reference holds no such label)
  double v_crit;           // smallest double whose correctly rounded square root is >= thr_pos: sqrt(v) < thr_pos <=> v < v_crit
};
void launch_place_sweep(const PlaceDev& P, hipStream_t s);
// A list of map pairs in one launch (slide_find_inter_loop_closures): one PlaceDev per live pair (ref7 / qry7 / inliers unused), a
// workgroup table {pair, rank within the pair, workgroups of the pair}, one partial (first index of the best count) per workgroup and
// one winner per pair; wg0[0 .. n_seg]: first workgroup of every pair.  lds_bytes: the largest pair's image (place_lds_bytes).
struct PlaceWg { int pair, rank, n, pad; };
struct PlaceBest { long long idx; int val, pad; };
size_t place_lds_bytes(int nr, int nq, int ignore_dim);
void launch_place_sweep_seg(const PlaceDev* segs, const PlaceWg* wgs, int n_wg, size_t lds_bytes, PlaceBest* part, const int* wg0, int n_seg,
                            PlaceBest* best, hipStream_t s);
// Submaps around a list of key poses (slide_keypose_submaps): the three map tables, the poses (xyz at pose_xyz + pose_stride * k:
// stride 3 for a position list, 7 for a pose list) and the two thresholds.  blockIdx.x = pose * n_chunk + chunk of 256 objects of the
// concatenated table; count pass: cnt per workgroup; emit pass: rows at base[pose] + chunkoff[workgroup] + rank (src_idx may be null).
struct SubmapDev {
  const double* cyl_root; const double* cyl_ray; const double* cyl_radius; const int32_t* cyl_label; int n_cyl;
  const double* cube_xyz; const double* cube_scale; const int32_t* cube_label; int n_cube;
  const double* ell_xyz; const double* ell_scale; const int32_t* ell_label; int n_ell;
  const double* pose_xyz; int pose_stride;
  double radius, max_dz;
};
void launch_keypose_submap(bool emit, const SubmapDev& S, int n_poses, int n_chunk, int* cnt, const long long* chunkoff, const long long* base,
                           double* rows7, int32_t* src_idx, hipStream_t s);
void launch_place_argmax(const int32_t* inliers, long long n, long long* best_idx, int32_t* best_val, hipStream_t s);
void launch_tri_prepare(const double* tri, int n, double* sdist, double* sxy, hipStream_t s);
void launch_tri_match(bool emit, const double* dm, const double* xm, int ntm, const double* dd, const double* xd, int ntd, double thr,
                      int* counts, const long long* offs, double* pts, double* diffs, hipStream_t s);
// A list of map pairs in one launch (slide_find_inter_loop_closures_clipper): the rows of all pairs flattened behind a row-offset
// table off[0 .. n_seg]; the segment of a row is the LAST s with off[s] <= row (empty segments are passed over).  Called with a
// wave-uniform row, so the search is scalar code.
__device__ __forceinline__ int seg_of_row(const int* __restrict__ off, int n_seg, int row) {
  int lo = 0, hi = n_seg;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (off[mid] <= row) lo = mid; else hi = mid;
  }
  return lo;
}
struct TriSeg { int tm0, td0, ntd; };      // a pair's model / data triangles in the prepared arrays of all maps: first model, first data, data count
void launch_tri_match_seg(bool emit, const double* sd, const double* sx, const int* rowoff, const TriSeg* segs, int n_seg, int n_rows, double thr,
                          int* counts, const long long* offs, const long long* base, double* P1, double* P2, hipStream_t s);
// exclusive scans of per-row counts restarting at every segment, totals[s] = the segment's sum (64 bits); the rowptr form writes the
// n + 1 row pointers of segment s at rowptr[segoff[s] + s ...]
void launch_seg_scan64(const int* cnt, const int* segoff, int n_seg, long long* out, long long* totals, hipStream_t s);
void launch_seg_scan_rowptr(const int* cnt, const int* segoff, int n_seg, int* rowptr, long long* totals, hipStream_t s);
// clipper_kernels.hip — CLIPPER dense clique on the device: CSR of the symmetric affinity matrix from its dense upper triangle (count,
// host prefix sum, fill), then the whole projected-gradient solve in one persistent workgroup.  work6n: 6 n doubles (u comes back in the
// first n), out4: {F, d, gradient evaluations, outer iterations}
struct ClqSolve {
  const int* rowptr; const int* col; const double* val; int n;
  const double* u0;               // start weights
  double *u, *unew, *g, *gnew, *Mu, *Cu;      // n each (global; L2-resident)
  double tol_u, tol_F, beta, eps;
  int maxin, maxol, maxls, rescale;
  double* out;                    // [0] F, [1] d, [2] gradient evaluations, [3] outer iterations
};
void launch_clq_solve_batch(const ClqSolve* d_jobs, int n_jobs, hipStream_t s);      // one persistent workgroup per job (grid = n_jobs)
// one large problem on n_wg co-resident workgroups (cooperative launch): A.u (n) receives the result, A.Mu = 4 n doubles with A.Cu = A.Mu + n,
// priv = n_wg x 4 n doubles, bar2 = 2 ints; false when the cooperative launch is refused.  out[2] < 0 afterwards: a grid barrier timed out.
bool launch_clq_solve_coop(const ClqSolve& A, double* priv, int* bar2, int n_wg, hipStream_t s);
void launch_clq_csr_count(const double* Mup, int n, int* rowcnt, hipStream_t s);
void launch_clq_csr_fill(const double* Mup, int n, const int* rowptr, int* col, double* val, hipStream_t s);
void launch_clq_solve(const int* rowptr, const int* col, const double* val, int n, const double* u0, double* work6n, double tol_u, double tol_F,
                      double beta, double eps, int maxin, int maxol, int maxls, int rescale, double* out4, hipStream_t s);
void launch_clipper_affinity(const double* D1, const double* D2, int dim, const int32_t* A, int m, double sigma, double eps,
                             double mindist, double affinityeps, double* M, hipStream_t s);
// The score of one pair of associations (clipper.cpp:30-52 with euclidean_distance.cpp:13-31), THE one text both k_clipper_affinity
// (dense upper triangle, place_kernels.hip) and k_affinity_csr (the sparse rows, clipper_kernels.hip) evaluate, always called with
// the smaller association index as (i): associations (i0, i1) and (j0, j1), their points pi1 / pj1 in the first set and pi2 / pj2 in
// the second.  Both sources are compiled with -ffp-contract=off, so what is left are correctly rounded IEEE operations in one fixed
// order plus the device library's exp: the same bits wherever it is inlined.  DIM > 0: a compile-time dimension (points in registers).
template <int DIM>
__device__ __forceinline__ double clipper_pair_score(int i0, int i1, int j0, int j1, const double* pi1, const double* pj1, const double* pi2,
                                                     const double* pj2, int dim, double sigma, double eps, double mindist, double affinityeps) {
  double out = 0.0;
  if (i0 != j0 && i1 != j1) {
    const int nd = DIM > 0 ? DIM : dim;
    double s1 = 0, s2 = 0;
    for (int k = 0; k < nd; ++k) {
      s1 += (pi1[k] - pj1[k]) * (pi1[k] - pj1[k]);
      s2 += (pi2[k] - pj2[k]) * (pi2[k] - pj2[k]);
    }
    const double l1 = sqrt(s1), l2 = sqrt(s2);
    if (!(mindist > 0 && (l1 < mindist || l2 < mindist))) {
      const double c = fabs(l1 - l2);
      const double scr = (c < eps) ? exp(-0.5 * c * c / (sigma * sigma)) : 0.0;
      if (scr > affinityeps) out = scr;
    }
  }
  return out;
}
// The same matrix as CSR straight from the associations (scorePairwiseConsistency ending in M_ = M.sparseView(), clipper.cpp:21-65):
// the symmetric matrix without its diagonal, columns ascending.  count: rowcnt[i]; emit: col / val at rowptr[i].  P1 / P2 non-null:
// the associations' points gathered beforehand (launch_affinity_gather: P1[j] = D1[A[j,0]], P2[j] = D2[A[j,1]]), read instead of D1 / D2.
void launch_affinity_gather(const double* D1, const double* D2, int dim, const int32_t* A, int m, double* P1, double* P2, hipStream_t s);
void launch_affinity_csr(bool emit, const double* D1, const double* D2, const double* P1, const double* P2, int dim, const int32_t* A, int m,
                         double sigma, double eps, double mindist, double affinityeps, int* rowcnt, const int* rowptr, int* col, double* val,
                         hipStream_t s);
// The CSRs of a LIST of problems in one launch (dim 2, identity association list; clipper_kernels.hip): P1 / P2 the associations' points of
// all pairs, aoff[0 .. n_seg] their association offsets.  count: rowcnt[row]; emit: pair s at nnz0[s] (< 0: skipped) + its own row
// pointers rowptr[aoff[s] + s ...].  Each pair's CSR equals launch_affinity_csr's for that pair alone bit for bit.
void launch_affinity_csr_seg(bool emit, const double* P1, const double* P2, const int* aoff, int n_seg, int n_rows, double sigma, double eps,
                             double mindist, double affinityeps, int* rowcnt, const int* rowptr, const long long* nnz0, int* col, double* val,
                             hipStream_t s);
// U[aoff[s] + i] = work[6 aoff[s] + i]: the solved weights of all pairs side by side
void launch_clq_pack_u(const double* work, const int* aoff, int n_seg, int n_rows, double* U, hipStream_t s);

// closure_kernels.hip — pairwise-consistency maximisation (PCM; Mangelson et al., ICRA 2018) over a list of loop closures: the
// consistency matrix as CSR on the device, solved by the clique kernels above.  No counterpart in the reference, which adds the first
// closure that passes its inlier test straight into the graph (sloamNode.cpp:448-476).
// A closure k measures z_k = X(from_k)^-1 X(to_k) (the meaning of slide_graph_add_loop_closure).  With the current estimates
// F_k = X(from_k), T_k = X(to_k), two closures i < j of one ordered robot pair close the cycle
//     e_ij = se3_log(z_i T_i^-1 T_j z_j^-1 F_j^-1 F_i) = se3_log(U_i G_j^-1 F_i),   U_k = z_k T_k^-1,  G_k = F_k U_k,
// in se3_log's tangent order [rot(3), trans(3)].  Only T_i^-1 T_j and F_j^-1 F_i — poses of ONE robot each — enter, so the two
// robots' world frames need not be related.  k_closure_prepare writes per closure the 36 doubles [U | G^-1 | F] (R row-major, t).
constexpr int CLOSURE_PRE = 36;
struct ClosureScore { double gate, sigma, affinityeps, odom2[6]; };      // odom2: odom_sigma6 squared
// THE one text of the pair score, called with the smaller closure index as (i) — on the device by k_closure_csr_seg and, being plain
// host + device code, by a stand-alone CPU check: pre_i / pre_j the closures' prepared 36 doubles, s2i / s2j their squared sigmas,
// legs = |from_idx_i - from_idx_j| + |to_idx_i - to_idx_j| odometry steps.  Variance per component s2i + s2j + legs odom2;
// d = sqrt(sum e^2 / s2); d < gate ? exp(-0.5 d^2 / sigma^2) : 0, kept above affinityeps.  closure_kernels.hip is compiled with
// -ffp-contract=off: correctly rounded operations in one fixed order plus the math library's acos / sin / tan / sqrt / exp.
__host__ __device__ __forceinline__ double closure_pair_score(const double* __restrict__ pre_i, const double* __restrict__ pre_j, const double* __restrict__ s2i,
                                                              const double* __restrict__ s2j, double legs, const ClosureScore& P) {
  const SE3 E = compose(compose(from12(pre_i), from12(pre_j + 12)), from12(pre_i + 24));
  double e[6];
  se3_log(E, e);
  double q = 0.0;
#pragma unroll
  for (int c = 0; c < 6; ++c) q += e[c] * e[c] / (s2i[c] + s2j[c] + legs * P.odom2[c]);
  const double d = sqrt(q);
  const double scr = d < P.gate ? exp(-0.5 * d * d / (P.sigma * P.sigma)) : 0.0;
  return scr > P.affinityeps ? scr : 0.0;
}
// what rows and columns of the matrix need of one closure, formed once (k_closure_prepare; host + device like the score)
__host__ __device__ __forceinline__ void closure_prepare_one(const SE3& F, const SE3& T, const SE3& z, double* __restrict__ pre) {
  const SE3 U = compose(z, inverse(T));
  to12(U, pre);
  to12(inverse(compose(F, U)), pre + 12);
  to12(F, pre + 24);
}
// one thread per closure (rows of all groups flattened): F / T from the caller's pose12 arrays (fslot == null, row k at 12 k) or from a
// graph's device-resident estimate by slot (pose12 = pose_est, rows fslot[k] / tslot[k]); z12: the measured relative poses
void launch_closure_prepare(const double* fpose12, const double* tpose12, const int32_t* fslot, const int32_t* tslot, const double* z12, int n,
                            double* pre, hipStream_t s);
// The consistency CSRs of a LIST of groups in one launch, as launch_affinity_csr_seg: rows flattened behind goff[0 .. n_seg], the
// columns of a row run over ITS group only.  sig2: 6 per row (squared sigmas), idx2: from_idx, to_idx per row.  count: rowcnt[row];
// emit: group s at nnz0[s] (< 0: skipped) + its own row pointers rowptr[goff[s] + s ...].
void launch_closure_csr_seg(bool emit, const double* pre, const double* sig2, const unsigned long long* idx2, const int* goff, int n_seg,
                            int n_rows, const ClosureScore& P, int* rowcnt, const int* rowptr, const long long* nnz0, int* col, double* val,
                            hipStream_t s);

// The individual-compatibility gate of a list of closures and the joint marginal of pose pairs (closure_kernels.hip has the
// invariant).  Candidate k of a sweep owns the columns 6 k .. 6 k + 5 (gate) or 12 k .. 12 k + 11 (pairs) of B (nT rows, zero before
// the launch); fslot / tslot / aslot / bslot: rows of the device-resident estimate; prow: a pose's first row of the reduced system
// (null: 6 slot); z12: the measured relative poses; r6: the whitened residuals (6 per candidate).
constexpr int GATE_OUT = 43;      // per candidate: d2, C (36, row-major), r (6)
void launch_closure_gate_lin(const double* pose_est, const int32_t* fslot, const int32_t* tslot, const double* z12, const double* sigma6, int n,
                             int chart, const int* prow, double* B, int nT, double* r6, hipStream_t s);
void launch_pair_identity(const int32_t* aslot, const int32_t* bslot, int n, const int* prow, double* B, int nT, hipStream_t s);
// the same fills on the joint graph of a CholBatch: ends[k] = {graph of pose a / from, its pose id, graph of pose b / to, its pose id};
// tab (in device memory): per graph its estimate, its prow map, its system's first row in the one buffer (ld rows per column), its chart
struct JointPoseTab { SL_GPTR(const double) est[JSIG_ROBOTS_MAX]; SL_GPTR(const int) prow[JSIG_ROBOTS_MAX]; long long off[JSIG_ROBOTS_MAX]; int chart[JSIG_ROBOTS_MAX]; };
static_assert(sizeof(JointPoseTab) == (2 * sizeof(void*) + sizeof(long long) + sizeof(int)) * JSIG_ROBOTS_MAX, "host and device passes see the same bytes");
void launch_joint_closure_gate_lin(const JointPoseTab* tab, const int4* ends, const double* z12, const double* sigma6, int n, double* B,
                                   size_t ld, double* r6, hipStream_t s);
void launch_joint_pair_identity(const JointPoseTab* tab, const int4* ends, int n, double* B, size_t ld, hipStream_t s);
void launch_gram_sub(double* M, const double* Mneg, size_t n, hipStream_t s);      // M <- M - Mneg (the lambda rows' gram: D = -I there)
// M: the candidates' 6 x 6 grams W_k^T W_k (36 each); out: GATE_OUT per candidate; flag[k] = 1 where I + M is not positive definite
void launch_closure_gate_finish(const double* M, const double* r6, int n, double* out, int* flag, hipStream_t s);

// The individual-compatibility gate of landmark observations (obs_gate_kernels.hip has the invariant).  One launch serves candidates of
// one class (type: FT_BR / FT_CUBE / FT_CYL, m = lf_rows(type) rows and columns each); candidate k of a sweep owns the columns
// m k .. m k + m - 1 of B (nT rows, zero before the launch).  pid / lid: its pose and landmark ids; z15 / sg9: its measurement as the
// class's z array holds it and its sigmas (15 / 9 per candidate); r9: the whitened residuals; G0: Al H_ll^-1 Al^T (81 per candidate,
// m x m packed).  M: the candidates' m x m grams; out: OBS_GATE_OUT per candidate; flag[k] = 1 where C is not positive definite.
constexpr int OBS_GATE_OUT = 91;      // per candidate: d2, C (81, row-major, leading dimension 9), r (9)
void launch_obs_gate_lin(const GraphDev& G, int type, const int32_t* pid, const int32_t* lid, const double* z15, const double* sg9, int n,
                         double* B, int nT, double* r9, double* G0, hipStream_t s);
// the same gate at a PREDICTED pose: every candidate sits at the pose value x (12 doubles) that a Between factor of sigmas sqrt(s2)
// would tie to the graph's pose k; the candidates name their landmarks only
struct PredPoseDev { double x[12]; double s2[6]; int k; };
void launch_obs_gate_lin_pred(const GraphDev& G, int type, const PredPoseDev& P, const int32_t* lid, const double* z15, const double* sg9, int n,
                              double* B, int nT, double* r9, double* G0, hipStream_t s);
// the same fill on the joint graph of a CholBatch: Gs the members' views (device), tab as the joint closure gate's, ends[k] = {graph of
// the pose, its pose id, graph of the landmark, its landmark id}, sep_row[k] the joint row at which a separator landmark's first
// coordinate enters the walk, or -1 (a private landmark: its factors' poses are rows of the landmark's graph)
void launch_joint_obs_gate_lin(const GraphDev* Gs, const JointPoseTab* tab, int type, const int4* ends, const long long* sep_row, const double* z15,
                               const double* sg9, int n, double* B, size_t ld, double* r9, double* G0, hipStream_t s);
void launch_obs_gate_finish(int m, const double* M, const double* G0, const double* r9, int n, double* out, int* flag, hipStream_t s);

// The Mahalanobis test and the joint marginal of landmark PAIRS of one class (dimension D): pairs[k] = {landmark a, landmark b}, a != b,
// both with factors.  sg: the hypothesis' model noise in the class's tangent order.  Route 0 (cov_kernels.hip) reads the selected
// inverse Sg and is complete in one launch: the host sends it only pairs whose observers all lie inside the tile profile.  Route 1
// (obs_gate_kernels.hip) fills the pair's columns of B for the forward substitution of sigma_forms: nk = D difference columns
// (cov = false; r9 and G0 as launch_obs_gate_lin leaves them, finished by launch_obs_gate_finish) or nk = 2 D unit columns (cov = true;
// finished by launch_lm_pair_cov_finish from the pairs' nk x nk grams M).
constexpr int LM_PAIR_COV = 324;      // per pair: the 2 D x 2 D joint marginal, row-major, leading dimension 18
struct LmPairSigma { double s[9]; };
// where coordinate i of a landmark's tangent sits in its 15 doubles of lm_est: point xyz; cylinder tangent [ray, root, radius] over
// the value [root, ray, radius]
__host__ __device__ __forceinline__ int lm_pair_coord(int D, int i) { return D == 7 ? (i < 3 ? i + 3 : (i < 6 ? i - 3 : 6)) : i; }
void launch_lm_pair_direct(const GraphDev& G, const double* Sg, int ld, int D, const int2* pairs, int n, const LmPairSigma& sg, double* out,
                           int* flag, hipStream_t s);
void launch_lm_pair_cov(const GraphDev& G, const double* Sg, int ld, const int2* pairs, int n, double* out, hipStream_t s);
void launch_lm_pair_fill(const GraphDev& G, int D, bool cov, const int2* pairs, const LmPairSigma& sg, int n, double* B, int nT, double* r9,
                         double* G0, hipStream_t s);
void launch_lm_pair_cov_finish(const GraphDev& G, int D, const int2* pairs, const double* M, int n, double* out, hipStream_t s);
// The same two on the JOINT graph of a CholBatch (obs_gate_kernels.hip): ends[k] = {graph of a, landmark a, graph of b, landmark b},
// sep_row[2 k + side] = -1 for a private side, else the joint row at which that side's SHARED landmark enters the walk; Gs / tab as
// launch_joint_obs_gate_lin takes them, B of ld rows per column.  The finish takes the pairs' SIGNED grams.
void launch_joint_lm_pair_fill(const GraphDev* Gs, const JointPoseTab* tab, int D, bool cov, const int4* ends, const long long* sep_row,
                               const LmPairSigma& sg, int n, double* B, size_t ld, double* r9, double* G0, hipStream_t s);
void launch_joint_lm_pair_cov_finish(const GraphDev* Gs, int D, const int4* ends, const long long* sep_row, const double* M, int n, double* out,
                                     hipStream_t s);
// Landmark fusion (lm_merge_kernels.hip; HostGraph::merge_landmarks): cluster c of n is the landmarks mem[ptr[c]] .. mem[ptr[c + 1] - 1]
// (ascending ids, one class of dimension D = 3 or 7, the survivor surv[c] among them) as the graph's device lists still hold them.
// x = (sum_i H_i)^-1 sum_i H_i est_i with H_i = sum Jl^T Jl over member i's records goes to lm_val and lm_est of the survivor, zero to
// its lm_delta; status[c] = 1 and nothing written when a pivot of the sum is not positive, else 0.
void launch_lm_merge_fuse(const GraphDev& G, int D, const int* ptr, const int* mem, const int* surv, int n, int* status, hipStream_t s);

// Every pair i < j of n points with |x_i - x_j| <= radius (and label[i] == label[j] where labels are given), sorted by (i, j): the
// count / k_seg_scan / emit idiom, one wavefront per row i, ballot compaction.  Point q is the three doubles at
// pts + stride * (sel ? sel[q] : q); label is indexed by q.  count: cnt[i]; emit: row i writes from off[i] on.
void launch_pairs_within(bool emit, const double* pts, int stride, const int* sel, const int32_t* label, int n, double radius, int* cnt,
                         const long long* off, int32_t* out_i, int32_t* out_j, double* out_dist, hipStream_t s);
// Its sibling for the joint graph of a CholBatch: group[q] (never null) is a group word per point and only pairs of DIFFERENT groups
// are kept; the walk, the order and the bits of the distances are the search's above.  launch_joint_lm_anchor_gather writes that
// search's input: ent[q] = {member graph, landmark, group word, .}; the landmark's anchor (the three doubles at coff of its lm_est)
// into pts[3 q ..] and the group word into group[q].
void launch_pairs_within_neq(bool emit, const double* pts, int stride, const int* sel, const int32_t* group, int n, double radius, int* cnt,
                             const long long* off, int32_t* out_i, int32_t* out_j, double* out_dist, hipStream_t s);
void launch_joint_lm_anchor_gather(const GraphDev* Gs, const int4* ent, int coff, int n, double* pts, int32_t* group, hipStream_t s);

// The joint-compatibility test of groups of candidate observations (obs_joint_kernels.hip has the invariant and the rule).  A sweep
// holds whole groups; cand[k] = {type (FT_BR / FT_CUBE / FT_CYL; < 0: a skipped candidate), pose id, landmark id, first column of the
// sweep's B}, in the caller's order, classes mixed; z15 / sg9 / r9 / G0 per entry of that table as above.  The fill is k_obs_gate_lin's
// body, one wavefront per candidate with the candidate's own class and column.
constexpr int JOINT_MAX_ROWS = 384;      // rows of a group at the most (one sweep: SLIDE_INFO_GAIN_SWEEP_COLS)
constexpr int JOINT_TB = 16;             // columns of the factor one step of the chain's triangular solve takes (a shuffle's width)
void launch_obs_joint_lin(const GraphDev& G, const int4* cand, const double* z15, const double* sg9, int n, double* B, int nT, double* r9,
                          double* G0, hipStream_t s);
// the same fill on the joint graph of a CholBatch: cand[k] = {type, ., ., first column} (what the chain reads of it), the pose and the
// landmark named by ends[k] and sep_row[k] as launch_joint_obs_gate_lin names them
void launch_joint_obs_joint_lin(const GraphDev* Gs, const JointPoseTab* tab, const int4* cand, const int4* ends, const long long* sep_row,
                                const double* z15, const double* sg9, int n, double* B, size_t ld, double* r9, double* G0, hipStream_t s);
// grp[g]: the group as one "candidate" of launch_gram_blocks (c0, nk, nsplit, moff, poff; woff its nk x nk slice of `work`, used past
// GAIN_LDS_DIM rows); gcand[g] = {its first entry of cand, their count}; Mg: the groups' grams (lower 16 x 16 tiles valid);
// qtab[d - 1]: the chi-square quantile of d = 1 .. JOINT_MAX_ROWS degrees of freedom.  out_d: {d2_single, d2_joint} and out_i:
// {accepted, dof_joint, 1 where a pivot was not > 0} per entry of cand; gout_d: d2 and gout_i: {rows, count} of each group's accepted
// set.  lds_rows: the rows of the largest group of at most GAIN_LDS_DIM rows (0: none); any_big: a larger group is in the table.
int launch_joint_compat_chain(const GainCandDev* grp, const int2* gcand, int ngroups, const int4* cand, const double* Mg, const double* G0,
                              const double* r9, const double* qtab, int evaluate_only, double* work, int lds_rows, bool any_big, double* out_d,
                              int* out_i, double* gout_d, int* gout_i, hipStream_t s);

}  // namespace sl
