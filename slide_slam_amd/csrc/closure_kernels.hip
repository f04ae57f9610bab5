// Pairwise-consistency maximisation over a list of loop closures (PCM; Mangelson et al., ICRA 2018): the kernels that build the
// consistency matrix as CSR.  No counterpart in the reference: it adds the first closure that passes its inlier test straight into the
// graph (sloamNode.cpp:448-476) with a noise of 0.01 x the odometry sigmas (graphWrapper.cpp:55).  The matrix goes to the clique
// solver of clipper_kernels.hip (k_clq_solve_b: every group of one list in one launch); kernels.hpp has the invariant and THE one
// scoring function (closure_pair_score).
#include <hip/hip_runtime.h>

#include "kernels.hpp"

namespace sl {

// per closure: U = z T^-1, G^-1 = (F U)^-1 and F, what rows and columns of the matrix need of it, formed once
__global__ __launch_bounds__(256) void k_closure_prepare(const double* __restrict__ fpose12, const double* __restrict__ tpose12,
                                                         const int32_t* __restrict__ fslot, const int32_t* __restrict__ tslot,
                                                         const double* __restrict__ z12, int n, double* __restrict__ pre) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= n) return;
  const SE3 F = from12(fpose12 + 12 * (size_t)(fslot ? fslot[k] : k));
  const SE3 T = from12(tpose12 + 12 * (size_t)(tslot ? tslot[k] : k));
  closure_prepare_one(F, T, from12(z12 + 12 * (size_t)k), pre + CLOSURE_PRE * (size_t)k);
}
void launch_closure_prepare(const double* fpose12, const double* tpose12, const int32_t* fslot, const int32_t* tslot, const double* z12, int n,
                            double* pre, hipStream_t s) {
  if (n > 0) hipLaunchKernelGGL(k_closure_prepare, dim3((n + 255) / 256), dim3(256), 0, s, fpose12, tpose12, fslot, tslot, z12, n, pre);
}

// Row `row` of the flattened list = closure i of group s: one wave per row, four rows per workgroup, the lanes over the columns of
// group s only, in chunks of 64 counted from the group's first closure.  Every entry is one closure_pair_score with the SMALLER
// closure index as (i): e_ij is not symmetric in (i, j), so entries (i, j) and (j, i) are made one evaluation of the same operands and
// the matrix is symmetric bit for bit.  Ballot ranks keep the columns ascending; no atomics: the same bits every run, and nothing a
// row reads or writes depends on the other groups of the list.  EMIT = false: rowcnt[row].  EMIT = true: at nnz0[s] + rowptr[goff[s] + s + i]
// (rowptr: k_seg_scan's n + 1 row pointers per group; col / val indexed in 64 bits; nnz0[s] < 0: the group was dropped).
template <bool EMIT>
__global__ __launch_bounds__(256) void k_closure_csr_seg(const double* __restrict__ pre, const double* __restrict__ sig2,
                                                         const unsigned long long* __restrict__ idx2, const int* __restrict__ goff, int n_seg,
                                                         int n_rows, ClosureScore P, int* __restrict__ rowcnt, const int* __restrict__ rowptr,
                                                         const long long* __restrict__ nnz0, int* __restrict__ col, double* __restrict__ val) {
  const int row = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6))), lane = threadIdx.x & 63;
  if (row >= n_rows) return;
  const int s = seg_of_row(goff, n_seg, row);
  const int a0 = goff[s], m = goff[s + 1] - a0, i = row - a0;
  long long base = 0;
  if (EMIT) {
    if (nnz0[s] < 0) return;
    base = nnz0[s] + rowptr[(size_t)row + s];
  }
  int cnt = 0;
  for (int c0 = 0; c0 < m; c0 += 64) {
    const int j = c0 + lane;
    double v = 0.0;
    if (j < m && j != i) {
      const size_t lo = (size_t)a0 + (j > i ? i : j), hi = (size_t)a0 + (j > i ? j : i);      // the smaller index goes first
      const unsigned long long f0 = idx2[2 * lo], f1 = idx2[2 * hi], t0 = idx2[2 * lo + 1], t1 = idx2[2 * hi + 1];
      const double legs = (double)((f0 > f1 ? f0 - f1 : f1 - f0) + (t0 > t1 ? t0 - t1 : t1 - t0));
      v = closure_pair_score(pre + CLOSURE_PRE * lo, pre + CLOSURE_PRE * hi, sig2 + 6 * lo, sig2 + 6 * hi, legs, P);
    }
    const unsigned long long hit = __ballot(v != 0.0);
    if (EMIT && v != 0.0) {
      const long long k = base + __popcll(hit & ((1ull << lane) - 1ull));
      col[k] = j;
      val[k] = v;
    }
    base += __popcll(hit);
    cnt += __popcll(hit);
  }
  if (!EMIT && lane == 0) rowcnt[row] = cnt;
}
void launch_closure_csr_seg(bool emit, const double* pre, const double* sig2, const unsigned long long* idx2, const int* goff, int n_seg,
                            int n_rows, const ClosureScore& P, int* rowcnt, const int* rowptr, const long long* nnz0, int* col, double* val,
                            hipStream_t s) {
  if (n_rows <= 0) return;
  const dim3 grid((n_rows + 3) / 4), block(256);
  if (emit) hipLaunchKernelGGL(k_closure_csr_seg<true>, grid, block, 0, s, pre, sig2, idx2, goff, n_seg, n_rows, P, rowcnt, rowptr, nnz0, col, val);
  else hipLaunchKernelGGL(k_closure_csr_seg<false>, grid, block, 0, s, pre, sig2, idx2, goff, n_seg, n_rows, P, rowcnt, rowptr, nnz0, col, val);
}

// ---- the individual-compatibility gate: one closure against what the graph already knows about its two poses ----------------------
// d2 = r^T (I + A Sigma A^T)^-1 r, r (6) and A = [A_F | A_T] (6 x 12) the whitened residual and Jacobian of the Between factor
// slide_graph_add_loop_closure(rel, from, to) would add, Sigma the inverse of the resident reduced pose system S = L L^T.  With
// L W = A^T (a forward substitution only), A Sigma A^T = W^T W: the candidate's 6 x 6 diagonal block of the gram (k_gram_blocks).
//
// k_closure_gate_lin, one thread per candidate: the two poses from the device-resident estimate by slot, r and A by the text of
// k_lin_pose_factors_body's Between branch (solver_kernels.hip): e = local(z, F^-1 T) in the graph's chart, H_F = -Ad(T^-1 F), H_T = I,
// row a times 1 / sigma[a].  Column c0 + 6 k + a of B (nT rows, zero before the launch) gets row a of A: six entries at the from
// pose's rows, six at the to pose's (prow: a pose's first row, null = 6 slot).  A candidate stores into its own six columns and its own
// six residuals only, so candidates naming the same pose, or the same pair, need no atomics.
// (the body: candidate k's poses xf / xt, measurement z, sigmas sg; col: its first column of B, columns ld apart; rf / rt: the two poses'
// first rows; r: its six residuals.  One text for the single-graph kernel and the joint one below.)
__device__ __forceinline__ void closure_gate_lin_body(const double* __restrict__ xf, const double* __restrict__ xt,
                                                      const double* __restrict__ z, const double* __restrict__ sg, int chart,
                                                      double* __restrict__ col0, size_t ld, size_t rf, size_t rt, double* __restrict__ r) {
  const SE3 X1 = from12(xf);
  const SE3 X2 = from12(xt);
  const SE3 Z = from12(z);
  double e[6];
  local(Z, between(X1, X2), e, chart);
  double Ad[36];
  adjoint(between(X2, X1), Ad);
#pragma unroll
  for (int a = 0; a < 6; ++a) {
    const double w = 1.0 / sg[a];
    r[a] = e[a] * w;
    double* col = col0 + (size_t)a * ld;
#pragma unroll
    for (int c = 0; c < 6; ++c) {
      col[rf + c] = -Ad[6 * a + c] * w;
      col[rt + c] = a == c ? w : 0.0;
    }
  }
}
__global__ __launch_bounds__(64) void k_closure_gate_lin(const double* __restrict__ pose_est, const int32_t* __restrict__ fslot,
                                                         const int32_t* __restrict__ tslot, const double* __restrict__ z12,
                                                         const double* __restrict__ sigma6, int n, int chart, const int* __restrict__ prow,
                                                         double* __restrict__ B, int nT, double* __restrict__ r6) {
  const int k = blockIdx.x * 64 + threadIdx.x;
  if (k >= n) return;
  const size_t rf = prow ? (size_t)prow[fslot[k]] : 6 * (size_t)fslot[k], rt = prow ? (size_t)prow[tslot[k]] : 6 * (size_t)tslot[k];
  closure_gate_lin_body(pose_est + 12 * (size_t)fslot[k], pose_est + 12 * (size_t)tslot[k], z12 + 12 * (size_t)k, sigma6 + 6 * (size_t)k, chart,
                        B + (size_t)(6 * k) * nT, (size_t)nT, rf, rt, r6 + 6 * (size_t)k);
}
void launch_closure_gate_lin(const double* pose_est, const int32_t* fslot, const int32_t* tslot, const double* z12, const double* sigma6, int n,
                             int chart, const int* prow, double* B, int nT, double* r6, hipStream_t s) {
  if (n > 0) hipLaunchKernelGGL(k_closure_gate_lin, dim3((n + 63) / 64), dim3(64), 0, s, pose_est, fslot, tslot, z12, sigma6, n, chart, prow, B, nT, r6);
}
// The pair query's right-hand sides: pair k owns the columns 12 k .. 12 k + 11, the unit vectors of pose a's six rows, then pose b's
// (B zero before the launch; one thread per column, each storing into its own column)
__global__ __launch_bounds__(64) void k_pair_identity(const int32_t* __restrict__ aslot, const int32_t* __restrict__ bslot, int n,
                                                      const int* __restrict__ prow, double* __restrict__ B, int nT) {
  const int e = blockIdx.x * 64 + threadIdx.x;
  if (e >= 12 * n) return;
  const int k = e / 12, j = e - 12 * k;
  const int p = j < 6 ? aslot[k] : bslot[k];
  const size_t row = (prow ? (size_t)prow[p] : 6 * (size_t)p) + (j < 6 ? j : j - 6);
  B[(size_t)e * nT + row] = 1.0;
}
void launch_pair_identity(const int32_t* aslot, const int32_t* bslot, int n, const int* prow, double* B, int nT, hipStream_t s) {
  if (n > 0) hipLaunchKernelGGL(k_pair_identity, dim3((12 * n + 63) / 64), dim3(64), 0, s, aslot, bslot, n, prow, B, nT);
}
// The same two fills on the JOINT graph (CholBatch): the two ends of a candidate live in different graphs.  ends[k] = {graph of the
// first pose, its pose id, graph of the second, its pose id}; tab (device memory): per graph its device-resident estimate, its prow
// map and its system's first row in the one buffer of ld rows per column; the chart is the first pose's graph's.
__global__ __launch_bounds__(64) void k_joint_closure_gate_lin(const JointPoseTab* __restrict__ tab, const int4* __restrict__ ends,
                                                               const double* __restrict__ z12, const double* __restrict__ sigma6, int n,
                                                               double* __restrict__ B, size_t ld, double* __restrict__ r6) {
  const int k = blockIdx.x * 64 + threadIdx.x;
  if (k >= n) return;
  const int4 e = ends[k];
  const size_t rf = (size_t)tab->off[e.x] + tab->prow[e.x][e.y], rt = (size_t)tab->off[e.z] + tab->prow[e.z][e.w];
  closure_gate_lin_body(tab->est[e.x] + 12 * (size_t)e.y, tab->est[e.z] + 12 * (size_t)e.w, z12 + 12 * (size_t)k, sigma6 + 6 * (size_t)k,
                        tab->chart[e.x], B + (size_t)(6 * k) * ld, ld, rf, rt, r6 + 6 * (size_t)k);
}
void launch_joint_closure_gate_lin(const JointPoseTab* tab, const int4* ends, const double* z12, const double* sigma6, int n, double* B,
                                   size_t ld, double* r6, hipStream_t s) {
  if (n > 0) hipLaunchKernelGGL(k_joint_closure_gate_lin, dim3((n + 63) / 64), dim3(64), 0, s, tab, ends, z12, sigma6, n, B, ld, r6);
}
__global__ __launch_bounds__(64) void k_joint_pair_identity(const JointPoseTab* __restrict__ tab, const int4* __restrict__ ends, int n,
                                                            double* __restrict__ B, size_t ld) {
  const int e = blockIdx.x * 64 + threadIdx.x;
  if (e >= 12 * n) return;
  const int k = e / 12, j = e - 12 * k;
  const int4 en = ends[k];
  const int g = j < 6 ? en.x : en.z, p = j < 6 ? en.y : en.w;
  const size_t row = (size_t)tab->off[g] + tab->prow[g][p] + (j < 6 ? j : j - 6);
  B[(size_t)e * ld + row] = 1.0;
}
void launch_joint_pair_identity(const JointPoseTab* tab, const int4* ends, int n, double* B, size_t ld, hipStream_t s) {
  if (n > 0) hipLaunchKernelGGL(k_joint_pair_identity, dim3((12 * n + 63) / 64), dim3(64), 0, s, tab, ends, n, B, ld);
}
// The signed gram of the joint factor K = L D L^T: M <- M - Mneg, M the candidates' grams over the rows with D = +I, Mneg over the
// lambda rows (D = -I).  Entry by entry, so a block that is symmetric bit for bit stays so.
__global__ __launch_bounds__(256) void k_gram_sub(double* __restrict__ M, const double* __restrict__ Mneg, size_t n) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e < n) M[e] = M[e] - Mneg[e];
}
void launch_gram_sub(double* M, const double* Mneg, size_t n, hipStream_t s) {
  if (n > 0) hipLaunchKernelGGL(k_gram_sub, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, M, Mneg, n);
}
// k_closure_gate_finish, one wavefront per candidate (four to a workgroup): C = I + M (M: the candidate's 6 x 6 gram at 36 k),
// symmetrised as the host's woodbury_drops symmetrises; lane 0 factors C = G G^T in registers, solves G y = r and writes
// d2 = y^T y.  A pivot that is not > 0: flag[k] = 1 and zeros.  out: GATE_OUT doubles per candidate, [d2 | C row-major (36) | r (6)].
__global__ __launch_bounds__(256) void k_closure_gate_finish(const double* __restrict__ M, const double* __restrict__ r6, int n,
                                                             double* __restrict__ out, int* __restrict__ flag) {
  __shared__ double Cs[4][36];
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int k = blockIdx.x * 4 + wv;
  if (k < n && lane < 36) {
    const int a = lane / 6, b = lane - 6 * a;
    const double* Mk = M + 36 * (size_t)k;
    const double ab = (a == b ? 1.0 : 0.0) + Mk[6 * a + b], ba = (a == b ? 1.0 : 0.0) + Mk[6 * b + a];
    Cs[wv][lane] = a == b ? ab : (a > b ? 0.5 * (ab + ba) : 0.5 * (ba + ab));
  }
  __syncthreads();
  if (k >= n || lane != 0) return;
  double G[6][6], y[6];
  bool spd = true;
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    double d = Cs[wv][7 * j];
#pragma unroll
    for (int q = 0; q < j; ++q) d -= G[j][q] * G[j][q];
    if (!(d > 0.0)) spd = false;
    const double g = sqrt(spd ? d : 1.0);
    G[j][j] = g;
#pragma unroll
    for (int i = j + 1; i < 6; ++i) {
      double v = Cs[wv][6 * i + j];
#pragma unroll
      for (int q = 0; q < j; ++q) v -= G[i][q] * G[j][q];
      G[i][j] = v / g;
    }
  }
  double d2 = 0.0;
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    double v = r6[6 * (size_t)k + i];
#pragma unroll
    for (int q = 0; q < i; ++q) v -= G[i][q] * y[q];
    y[i] = v / G[i][i];
    d2 += y[i] * y[i];
  }
  double* o = out + GATE_OUT * (size_t)k;
  o[0] = spd ? d2 : 0.0;
#pragma unroll
  for (int e = 0; e < 36; ++e) o[1 + e] = spd ? Cs[wv][e] : 0.0;
#pragma unroll
  for (int e = 0; e < 6; ++e) o[37 + e] = spd ? r6[6 * (size_t)k + e] : 0.0;
  flag[k] = spd ? 0 : 1;
}
void launch_closure_gate_finish(const double* M, const double* r6, int n, double* out, int* flag, hipStream_t s) {
  if (n > 0) hipLaunchKernelGGL(k_closure_gate_finish, dim3((n + 3) / 4), dim3(256), 0, s, M, r6, n, out, flag);
}

}  // namespace sl
