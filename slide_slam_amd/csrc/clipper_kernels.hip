// CLIPPER dense-clique solver on the device (clipper_semantic_object/src/clipper.cpp:172-323, DSD_HEU rounding :302-310).
//
// The reference keeps the affinity matrix M and the constraint pattern C (= sparsity pattern of M, clipper.cpp:55-64) as Eigen
// sparse matrices and runs projected gradient ascent with backtracking on F(u) = u^T (M + I - d (11^T - C - I)) u; d grows in an
// outer loop until no constraint is active.  Here: M in CSR (built on the device, from the upper-filled dense affinity matrix by
// k_clq_csr or straight from the associations by k_affinity_csr — the same CSR bit for bit), and
// the WHOLE solve — every product, reduction, clamp, normalisation, line-search and stopping decision — in ONE launch with no host
// round trip inside the loop: a persistent workgroup of 1024 threads per problem (k_clq_solve, k_clq_solve_b: the iteration is
// strictly sequential with O(nnz) work per evaluation, and the problems sloam meets — tens to hundreds of associations — leave a
// second CU nothing to do that outweighs a grid barrier), and for ONE LARGE problem (m in the thousands) k_clq_solve_coop:
// the rows of the product over the waves of up to 128 co-resident workgroups, one grid barrier per evaluation, iterates bit-identical
// to the one-workgroup kernel's.  Loops are bounded by maxoliters x maxiniters x maxlsiters.
#include <hip/hip_runtime.h>

#include "kernels.hpp"

namespace sl {

// row i of the symmetric matrix held as its upper triangle, dense row-major: nonzeros counted (rowcnt) or written (col / val) in
// ascending column order; one wave per row, ballot ranks keep the order
template <bool EMIT>
__global__ __launch_bounds__(256) void k_clq_csr(const double* __restrict__ Mup, int n, int* __restrict__ rowcnt, const int* __restrict__ rowptr,
                                                 int* __restrict__ col, double* __restrict__ val) {
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= n) return;
  int base = EMIT ? rowptr[i] : 0;
  for (int j0 = 0; j0 < n; j0 += 64) {
    const int j = j0 + lane;
    double a = 0.0;
    if (j < n && j != i) a = j > i ? Mup[(size_t)i * n + j] : Mup[(size_t)j * n + i];
    const unsigned long long m = __ballot(a != 0.0);
    if (EMIT && a != 0.0) {
      const int k = base + __popcll(m & ((1ull << lane) - 1ull));
      col[k] = j;
      val[k] = a;
    }
    base += __popcll(m);
  }
  if (!EMIT && lane == 0) rowcnt[i] = base;
}

// ---- the affinity matrix as CSR straight from the associations (clipper.cpp:21-65 ending in M_ = M.sparseView()) -------------------
// Row i of the SYMMETRIC matrix without its diagonal, never passing through the dense m x m form: one wave per row, the lanes over
// the columns in chunks of 64, every entry scored by clipper_pair_score (kernels.hpp: the text k_clipper_affinity evaluates) with the
// smaller association index first, so entry (i, j), entry (j, i) and the dense kernel's (min, max) are one evaluation of the same
// operands.  Ballot ranks keep the columns ascending; no atomics: the same bits every run.  Two passes as k_clq_csr: EMIT = false
// counts, EMIT = true writes at rowptr[i].  DIM 2 / 3: the row's two points in registers; DIM 0: any dim, read per pair.
// GATHERED: X1 / X2 are the associations' points (k_affinity_gather), else D1 / D2 indexed through A.
__global__ __launch_bounds__(256) void k_affinity_gather(const double* __restrict__ D1, const double* __restrict__ D2, int dim,
                                                         const int32_t* __restrict__ A, int m, double* __restrict__ P1, double* __restrict__ P2) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (size_t)m * dim) return;
  const size_t j = t / dim;
  const int k = (int)(t - j * dim);
  P1[t] = D1[(size_t)A[2 * j] * dim + k];
  P2[t] = D2[(size_t)A[2 * j + 1] * dim + k];
}
template <bool EMIT, int DIM, bool GATHERED>
__global__ __launch_bounds__(256) void k_affinity_csr(const double* __restrict__ X1, const double* __restrict__ X2, int dim,
                                                      const int32_t* __restrict__ A, int m, double sigma, double eps, double mindist,
                                                      double affinityeps, int* __restrict__ rowcnt, const int* __restrict__ rowptr,
                                                      int* __restrict__ col, double* __restrict__ val) {
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= m) return;
  const int i0 = A[2 * (size_t)i], i1 = A[2 * (size_t)i + 1];
  const double* ri1 = X1 + (size_t)(GATHERED ? i : i0) * dim;
  const double* ri2 = X2 + (size_t)(GATHERED ? i : i1) * dim;
  constexpr int ND = DIM > 0 ? DIM : 1;
  double a1[ND], a2[ND];
  if (DIM > 0) {
#pragma unroll
    for (int k = 0; k < ND; ++k) { a1[k] = ri1[k]; a2[k] = ri2[k]; }
  }
  int base = EMIT ? rowptr[i] : 0;
  for (int c0 = 0; c0 < m; c0 += 64) {
    const int j = c0 + lane;
    double v = 0.0;
    if (j < m && j != i) {
      const int j0 = A[2 * (size_t)j], j1 = A[2 * (size_t)j + 1];
      const double* cj1 = X1 + (size_t)(GATHERED ? j : j0) * dim;
      const double* cj2 = X2 + (size_t)(GATHERED ? j : j1) * dim;
      const bool up = j > i;          // the row is the smaller index
      if (DIM > 0) {
        double lo1[ND], hi1[ND], lo2[ND], hi2[ND];
#pragma unroll
        for (int k = 0; k < ND; ++k) {
          const double b1 = cj1[k], b2 = cj2[k];
          lo1[k] = up ? a1[k] : b1; hi1[k] = up ? b1 : a1[k];
          lo2[k] = up ? a2[k] : b2; hi2[k] = up ? b2 : a2[k];
        }
        v = clipper_pair_score<DIM>(up ? i0 : j0, up ? i1 : j1, up ? j0 : i0, up ? j1 : i1, lo1, hi1, lo2, hi2, dim, sigma, eps, mindist,
                                    affinityeps);
      } else {
        v = clipper_pair_score<0>(up ? i0 : j0, up ? i1 : j1, up ? j0 : i0, up ? j1 : i1, up ? ri1 : cj1, up ? cj1 : ri1, up ? ri2 : cj2,
                                  up ? cj2 : ri2, dim, sigma, eps, mindist, affinityeps);
      }
    }
    const unsigned long long hit = __ballot(v != 0.0);
    if (EMIT && v != 0.0) {
      const int k = base + __popcll(hit & ((1ull << lane) - 1ull));
      col[k] = j;
      val[k] = v;
    }
    base += __popcll(hit);
  }
  if (!EMIT && lane == 0) rowcnt[i] = base;
}
// The same for a LIST of problems in one launch (the robot pairs of sloamNode.cpp:600-694), dim 2, identity association list
// (semantic_clipper.cpp:207-211: association a names point a of both sets): the rows of all pairs flattened behind aoff[0 .. n_seg],
// the columns of a row run over ITS pair only, in chunks of 64 counted from the pair's first association, every entry one
// clipper_pair_score<2> with the smaller association index first — so the CSR of a pair is k_affinity_csr's for that pair alone, bit
// for bit.  EMIT = false: rowcnt[row].  EMIT = true: row i of pair s at nnz0[s] + rowptr[aoff[s] + s + i] (rowptr: the segmented scan,
// n + 1 entries per pair; col / val: the pairs' arrays one after the other, indexed in 64 bits; nnz0[s] < 0: the pair was dropped).
template <bool EMIT>
__global__ __launch_bounds__(256) void k_affinity_csr_seg(const double* __restrict__ P1, const double* __restrict__ P2, const int* __restrict__ aoff,
                                                          int n_seg, int n_rows, double sigma, double eps, double mindist, double affinityeps,
                                                          int* __restrict__ rowcnt, const int* __restrict__ rowptr,
                                                          const long long* __restrict__ nnz0, int* __restrict__ col, double* __restrict__ val) {
  const int row = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6))), lane = threadIdx.x & 63;
  if (row >= n_rows) return;
  const int s = seg_of_row(aoff, n_seg, row);
  const int a0 = aoff[s], m = aoff[s + 1] - a0, i = row - a0;
  const double* X1 = P1 + 2 * (size_t)a0;
  const double* X2 = P2 + 2 * (size_t)a0;
  long long base = 0;
  if (EMIT) {
    if (nnz0[s] < 0) return;
    base = nnz0[s] + rowptr[(size_t)row + s];
  }
  const double a1[2] = {X1[2 * (size_t)i], X1[2 * (size_t)i + 1]}, a2[2] = {X2[2 * (size_t)i], X2[2 * (size_t)i + 1]};
  int cnt = 0;
  for (int c0 = 0; c0 < m; c0 += 64) {
    const int j = c0 + lane;
    double v = 0.0;
    if (j < m && j != i) {
      const bool up = j > i;          // the row is the smaller index
      double lo1[2], hi1[2], lo2[2], hi2[2];
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const double b1 = X1[2 * (size_t)j + k], b2 = X2[2 * (size_t)j + k];
        lo1[k] = up ? a1[k] : b1; hi1[k] = up ? b1 : a1[k];
        lo2[k] = up ? a2[k] : b2; hi2[k] = up ? b2 : a2[k];
      }
      const int lo = up ? i : j, hi = up ? j : i;
      v = clipper_pair_score<2>(lo, lo, hi, hi, lo1, hi1, lo2, hi2, 2, sigma, eps, mindist, affinityeps);
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
void launch_affinity_csr_seg(bool emit, const double* P1, const double* P2, const int* aoff, int n_seg, int n_rows, double sigma, double eps,
                             double mindist, double affinityeps, int* rowcnt, const int* rowptr, const long long* nnz0, int* col, double* val,
                             hipStream_t s) {
  if (n_rows <= 0) return;
  const dim3 grid((n_rows + 3) / 4), block(256);
  if (emit)
    hipLaunchKernelGGL(k_affinity_csr_seg<true>, grid, block, 0, s, P1, P2, aoff, n_seg, n_rows, sigma, eps, mindist, affinityeps, rowcnt, rowptr, nnz0, col, val);
  else
    hipLaunchKernelGGL(k_affinity_csr_seg<false>, grid, block, 0, s, P1, P2, aoff, n_seg, n_rows, sigma, eps, mindist, affinityeps, rowcnt, rowptr, nnz0, col, val);
}
// the solves' results side by side for ONE read-back: u of pair s (the first n of its 6 n work doubles) to U[aoff[s] ...]
__global__ __launch_bounds__(256) void k_clq_pack_u(const double* __restrict__ work, const int* __restrict__ aoff, int n_seg, int n_rows,
                                                    double* __restrict__ U) {
  const int row = blockIdx.x * 256 + threadIdx.x;
  if (row >= n_rows) return;
  const int a0 = aoff[seg_of_row(aoff, n_seg, row)];
  U[row] = work[6 * (size_t)a0 + (size_t)(row - a0)];
}
void launch_clq_pack_u(const double* work, const int* aoff, int n_seg, int n_rows, double* U, hipStream_t s) {
  if (n_rows > 0) hipLaunchKernelGGL(k_clq_pack_u, dim3((n_rows + 255) / 256), dim3(256), 0, s, work, aoff, n_seg, n_rows, U);
}
void launch_affinity_gather(const double* D1, const double* D2, int dim, const int32_t* A, int m, double* P1, double* P2, hipStream_t s) {
  const size_t n = (size_t)m * dim;
  if (n > 0) hipLaunchKernelGGL(k_affinity_gather, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, D1, D2, dim, A, m, P1, P2);
}
namespace {
template <bool EMIT, int DIM>
void affinity_csr_go(const double* D1, const double* D2, const double* P1, const double* P2, int dim, const int32_t* A, int m, double sigma,
                     double eps, double mindist, double affinityeps, int* rowcnt, const int* rowptr, int* col, double* val, hipStream_t s) {
  const dim3 grid((m + 3) / 4), block(256);
  if (P1 && P2)
    hipLaunchKernelGGL((k_affinity_csr<EMIT, DIM, true>), grid, block, 0, s, P1, P2, dim, A, m, sigma, eps, mindist, affinityeps, rowcnt, rowptr, col, val);
  else
    hipLaunchKernelGGL((k_affinity_csr<EMIT, DIM, false>), grid, block, 0, s, D1, D2, dim, A, m, sigma, eps, mindist, affinityeps, rowcnt, rowptr, col, val);
}
template <bool EMIT>
void affinity_csr_dim(const double* D1, const double* D2, const double* P1, const double* P2, int dim, const int32_t* A, int m, double sigma,
                      double eps, double mindist, double affinityeps, int* rowcnt, const int* rowptr, int* col, double* val, hipStream_t s) {
  if (dim == 2) affinity_csr_go<EMIT, 2>(D1, D2, P1, P2, dim, A, m, sigma, eps, mindist, affinityeps, rowcnt, rowptr, col, val, s);
  else if (dim == 3) affinity_csr_go<EMIT, 3>(D1, D2, P1, P2, dim, A, m, sigma, eps, mindist, affinityeps, rowcnt, rowptr, col, val, s);
  else affinity_csr_go<EMIT, 0>(D1, D2, P1, P2, dim, A, m, sigma, eps, mindist, affinityeps, rowcnt, rowptr, col, val, s);
}
}  // namespace
void launch_affinity_csr(bool emit, const double* D1, const double* D2, const double* P1, const double* P2, int dim, const int32_t* A, int m,
                         double sigma, double eps, double mindist, double affinityeps, int* rowcnt, const int* rowptr, int* col, double* val,
                         hipStream_t s) {
  if (m <= 0) return;
  if (emit) affinity_csr_dim<true>(D1, D2, P1, P2, dim, A, m, sigma, eps, mindist, affinityeps, rowcnt, rowptr, col, val, s);
  else affinity_csr_dim<false>(D1, D2, P1, P2, dim, A, m, sigma, eps, mindist, affinityeps, rowcnt, rowptr, col, val, s);
}

__device__ __forceinline__ double clq_block_sum(double x, double* sh) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) x += __shfl_xor(x, m);
  __syncthreads();                      // (sh may still be read from the previous reduction)
  if ((tid & 63) == 0) sh[tid >> 6] = x;
  __syncthreads();
  double s = 0.0;
  for (int w = 0; w < (int)(blockDim.x >> 6); ++w) s += sh[w];      // same order in every thread: identical result everywhere
  return s;
}

// ---- one LARGE problem on several workgroups (COOP) ---------------------------------------------------------------------------------
// The rows of the product are dealt to the waves of ALL workgroups; everything else — the step, the projection, every reduction,
// the line search and the stopping decisions — each workgroup repeats for the whole vector on PRIVATE copies of u / unew / g / gnew,
// with the very code and thread layout of the one-workgroup solve.  So every workgroup holds bit-identical iterates, takes the same
// branches and reaches the same grid barriers, the iterates equal the one-workgroup kernel's bit for bit, and the only data crossing
// workgroups are Mu / Cu: written with agent-scope (write-through) stores, read with agent-scope loads (the per-XCD L2s are not
// coherent: profiles/r04_tile_hop_bench.txt has the protocol measurements), double-buffered by product parity because a fast
// workgroup may start the next product while a slow one still reads this one's result — ONE grid barrier per product.
struct ClqGrid {
  int* bar;       // [0] arrivals (monotonic), [1] abort word
  int n_wg;
  int epoch;      // barriers passed (same in every thread of every workgroup)
  int par;        // parity of the product being computed
};
template <bool COOP> __device__ __forceinline__ double clq_ld(const double* p) {
  if (COOP) return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return *p;
}
// false: another workgroup gave up (or this one waited too long) — every caller returns at once, so the grid drains
__device__ __forceinline__ bool clq_grid_sync(ClqGrid& G) {
  __shared__ int s_ok;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // this wave's Mu / Cu stores have left
  __syncthreads();
  G.epoch += 1;
  if (threadIdx.x == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    __hip_atomic_fetch_add(G.bar, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int target = G.epoch * G.n_wg;
    int good = 1, spins = 0;
    while (__hip_atomic_load(G.bar, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target) {
      if (__hip_atomic_load(G.bar + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0 || ++spins > (1 << 24)) {
        __hip_atomic_store(G.bar + 1, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        good = 0;
        break;
      }
      __builtin_amdgcn_s_sleep(1);
    }
    s_ok = good;
  }
  __syncthreads();
  return s_ok != 0;
}

// Mu = M v, Cu = C v (C = pattern of M): wave per row.  COOP: rows over the waves of the whole grid, results into the buffer of this
// product's parity, then the grid barrier; returns false when the grid is being abandoned.
template <bool COOP>
__device__ __forceinline__ bool clq_prod(const ClqSolve& A, ClqGrid& G, const double* __restrict__ v, double*& Mu, double*& Cu) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nw = blockDim.x >> 6;
  Mu = A.Mu + (COOP ? (size_t)G.par * 2 * A.n : 0);
  Cu = A.Cu + (COOP ? (size_t)G.par * 2 * A.n : 0);
  const int first = COOP ? (int)blockIdx.x * nw + wave : wave, step = COOP ? G.n_wg * nw : nw;
  for (int i = first; i < A.n; i += step) {
    double s1 = 0.0, s2 = 0.0;
    for (int k = A.rowptr[i] + lane; k < A.rowptr[i + 1]; k += 64) {
      const double x = v[A.col[k]];
      s1 += A.val[k] * x;
      s2 += x;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) { s1 += __shfl_xor(s1, m); s2 += __shfl_xor(s2, m); }
    if (lane == 0) {
      if (COOP) {
        __hip_atomic_store(Mu + i, s1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(Cu + i, s2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      } else {
        Mu[i] = s1; Cu[i] = s2;
      }
    }
  }
  if (COOP) {
    G.par ^= 1;
    return clq_grid_sync(G);
  }
  __syncthreads();
  return true;
}
// gradient of F at v for the current d into gout; F = v . gout      (clipper.cpp:224-226, 246-248)
template <bool COOP>
__device__ __forceinline__ bool clq_grad(const ClqSolve& A, ClqGrid& G, const double* __restrict__ v, double d, double* __restrict__ gout, double* sh,
                                         double* F_out) {
  double part = 0.0;
  for (int i = threadIdx.x; i < A.n; i += blockDim.x) part += v[i];
  const double su = clq_block_sum(part, sh);
  double *Mu, *Cu;
  if (!clq_prod<COOP>(A, G, v, Mu, Cu)) return false;
  part = 0.0;
  for (int i = threadIdx.x; i < A.n; i += blockDim.x) {
    const double gi = (1.0 + d) * v[i] - d * su + clq_ld<COOP>(Mu + i) + clq_ld<COOP>(Cu + i) * d;
    gout[i] = gi;
    part += v[i] * gi;
  }
  *F_out = clq_block_sum(part, sh);
  __syncthreads();
  return true;
}
// mean over the active constraints of (Mu + u) / Cbu, Cbu = sum(u) - Cu - u   (clipper.cpp:201-216, 283-295)
template <bool COOP>
__device__ __forceinline__ bool clq_d_terms(const ClqSolve& A, ClqGrid& G, const double* __restrict__ v, bool absval, int* cnt_out, double* sh,
                                            double* mean_out) {
  double part = 0.0;
  for (int i = threadIdx.x; i < A.n; i += blockDim.x) part += v[i];
  const double su = clq_block_sum(part, sh);
  double *Mu, *Cu;
  if (!clq_prod<COOP>(A, G, v, Mu, Cu)) return false;
  double acc = 0.0, cnt = 0.0;
  for (int i = threadIdx.x; i < A.n; i += blockDim.x) {
    const double cbu = su - clq_ld<COOP>(Cu + i) - v[i];
    if (cbu > A.eps && v[i] > A.eps) {
      const double q = (clq_ld<COOP>(Mu + i) + v[i]) / cbu;
      acc += absval ? fabs(q) : q;
      cnt += 1.0;
    }
  }
  const double sa = clq_block_sum(acc, sh);
  const double sc = clq_block_sum(cnt, sh);
  *cnt_out = (int)sc;
  *mean_out = sc > 0.0 ? sa / sc : 0.0;
  return true;
}

// uw: this workgroup's u / unew / g / gnew (4 n doubles; A.u itself for the one-workgroup solve)
template <bool COOP>
__device__ __forceinline__ void clq_solve_body(const ClqSolve& A, ClqGrid& G, double* uw) {
  __shared__ double sh[16];
  const int tid = threadIdx.x, nt = blockDim.x, n = A.n;
  double *u = uw, *unew = uw + n, *g = uw + 2 * (size_t)n, *gnew = uw + 3 * (size_t)n;
  // u <- normalised (M u0 + u0) or u0   (clipper.cpp:186-199)
  if (A.rescale) {
    double *Mu, *Cu;
    if (!clq_prod<COOP>(A, G, A.u0, Mu, Cu)) return;
    for (int i = tid; i < n; i += nt) u[i] = clq_ld<COOP>(Mu + i) + A.u0[i];
  } else {
    for (int i = tid; i < n; i += nt) u[i] = A.u0[i];
  }
  __syncthreads();
  {
    double part = 0.0;
    for (int i = tid; i < n; i += nt) part += u[i] * u[i];
    const double nn = sqrt(clq_block_sum(part, sh));
    for (int i = tid; i < n; i += nt) u[i] /= nn;
    __syncthreads();
  }
  double d = 0.0, F = 0.0, evals = 0.0;
  int cnt = 0, outer = 0;
  {
    double t;
    if (!clq_d_terms<COOP>(A, G, u, false, &cnt, sh, &t)) return;
    if (cnt > 0) d = t;
  }
  for (outer = 0; outer < A.maxol; ++outer) {
    if (!clq_grad<COOP>(A, G, u, d, g, sh, &F)) return;
    evals += 1.0;
    for (int j = 0; j < A.maxin; ++j) {
      double alpha = 1.0, Fnew = 0.0, deltaF = 0.0;
      for (int k = 0; k < A.maxls; ++k) {
        // step, project onto u >= 0, back onto the sphere   (clipper.cpp:236-245)
        double part = 0.0;
        for (int i = tid; i < n; i += nt) {
          const double x = fmax(u[i] + alpha * g[i], 0.0);
          unew[i] = x;
          part += x * x;
        }
        const double nn = sqrt(clq_block_sum(part, sh));
        for (int i = tid; i < n; i += nt) unew[i] /= nn;
        __syncthreads();
        if (!clq_grad<COOP>(A, G, unew, d, gnew, sh, &Fnew)) return;
        evals += 1.0;
        deltaF = Fnew - F;
        if (deltaF < -A.eps) alpha *= A.beta;        // backtracking line search (every thread holds the same numbers)
        else break;
      }
      double part = 0.0;
      for (int i = tid; i < n; i += nt) { const double e = unew[i] - u[i]; part += e * e; }
      const double du = sqrt(clq_block_sum(part, sh));
      F = Fnew;
      double* t = u; u = unew; unew = t;
      t = g; g = gnew; gnew = t;
      __syncthreads();
      if (du < A.tol_u || fabs(deltaF) < A.tol_F) break;
    }
    double deltad;
    if (!clq_d_terms<COOP>(A, G, u, true, &cnt, sh, &deltad)) return;
    if (cnt > 0) d += deltad;
    else break;
  }
  // the iterate ends up in A.u for the caller (COOP: workgroup 0 hands over its copy)
  if (!COOP || blockIdx.x == 0) {
    if (u != A.u) {
      for (int i = tid; i < n; i += nt) A.u[i] = u[i];
    }
    if (tid == 0) { A.out[0] = F; A.out[1] = d; A.out[2] = evals; A.out[3] = (double)outer; }
  }
}

__global__ __launch_bounds__(1024) void k_clq_solve(ClqSolve A) {
  ClqGrid G{nullptr, 1, 0, 0};
  clq_solve_body<false>(A, G, A.u);
}
// several independent problems (the robot pairs of a multi-robot job, SURVEY 8e: 28 at eight robots), one persistent workgroup each
__global__ __launch_bounds__(1024) void k_clq_solve_b(const ClqSolve* __restrict__ jobs) {
  const ClqSolve A = jobs[blockIdx.x];
  ClqGrid G{nullptr, 1, 0, 0};
  if (A.n > 0) clq_solve_body<false>(A, G, A.u);
}
// one large problem on n_wg co-resident workgroups (cooperative launch); priv: n_wg x 4 n doubles, bar: 2 ints, zero at launch;
// A.Mu: 4 n doubles, [parity][Mu | Cu] (A.Cu = A.Mu + n); A.u receives the result
__global__ __launch_bounds__(1024) void k_clq_solve_coop(ClqSolve A, double* priv, int* bar, int n_wg) {
  ClqGrid G{bar, n_wg, 0, 0};
  clq_solve_body<true>(A, G, priv + (size_t)blockIdx.x * 4 * A.n);
  // a workgroup that left through a failed barrier reports it (out[2] < 0: the host turns it into an error)
  if (threadIdx.x == 0 && blockIdx.x == 0 && __hip_atomic_load(bar + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) A.out[2] = -1.0;
}
void launch_clq_solve_batch(const ClqSolve* d_jobs, int n_jobs, hipStream_t s) {
  if (n_jobs > 0) hipLaunchKernelGGL(k_clq_solve_b, dim3(n_jobs), dim3(1024), 0, s, d_jobs);
}
// false: the cooperative launch was refused (the caller falls back to the one-workgroup kernel)
bool launch_clq_solve_coop(const ClqSolve& A, double* priv, int* bar2, int n_wg, hipStream_t s) {
  if (hipMemsetAsync(bar2, 0, 2 * sizeof(int), s) != hipSuccess) return false;
  ClqSolve a = A;
  void* args[] = {&a, &priv, &bar2, &n_wg};
  const hipError_t e = hipLaunchCooperativeKernel((const void*)k_clq_solve_coop, dim3(n_wg), dim3(1024), args, 0, s);
  if (e != hipSuccess) { (void)hipGetLastError(); return false; }
  return true;
}

void launch_clq_csr_count(const double* Mup, int n, int* rowcnt, hipStream_t s) {
  if (n > 0) hipLaunchKernelGGL(k_clq_csr<false>, dim3((n + 3) / 4), dim3(256), 0, s, Mup, n, rowcnt, nullptr, nullptr, nullptr);
}
void launch_clq_csr_fill(const double* Mup, int n, const int* rowptr, int* col, double* val, hipStream_t s) {
  if (n > 0) hipLaunchKernelGGL(k_clq_csr<true>, dim3((n + 3) / 4), dim3(256), 0, s, Mup, n, nullptr, rowptr, col, val);
}
void launch_clq_solve(const int* rowptr, const int* col, const double* val, int n, const double* u0, double* work6n, double tol_u, double tol_F,
                      double beta, double eps, int maxin, int maxol, int maxls, int rescale, double* out4, hipStream_t s) {
  ClqSolve A;
  A.rowptr = rowptr; A.col = col; A.val = val; A.n = n; A.u0 = u0;
  A.u = work6n; A.unew = work6n + n; A.g = work6n + 2 * (size_t)n; A.gnew = work6n + 3 * (size_t)n; A.Mu = work6n + 4 * (size_t)n; A.Cu = work6n + 5 * (size_t)n;
  A.tol_u = tol_u; A.tol_F = tol_F; A.beta = beta; A.eps = eps; A.maxin = maxin; A.maxol = maxol; A.maxls = maxls; A.rescale = rescale;
  A.out = out4;
  hipLaunchKernelGGL(k_clq_solve, dim3(1), dim3(1024), 0, s, A);
}

}  // namespace sl
