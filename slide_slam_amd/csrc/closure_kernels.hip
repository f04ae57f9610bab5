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

}  // namespace sl
