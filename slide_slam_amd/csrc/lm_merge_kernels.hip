// Landmark fusion (slide_graph_merge_landmarks with fuse = 1): the estimate the surviving landmark of a merged cluster takes.  No
// counterpart in the reference; EKF-SLAM calls the operation landmark fusion.
//
// With the poses held at their estimate, member i of a cluster contributes the cost 1/2 (x - est_i)^T H_i (x - est_i) to the merged
// landmark: H_i = sum Jl^T Jl over its factors at the last linearisation is its own H_ll, and the back-substitution left est_i at the
// conditional optimum.  Points and cylinders retract additively, so the minimiser of the sum is
//     x = (sum_i H_i)^-1 sum_i H_i est_i
// in the tangent order of slide_graph_get_landmark_covariances (lm_pair_coord).  H_i is re-summed from the factors' records in jbuf
// exactly as k_landmark sums it (lanes own factors, a fixed xor-shuffle tree), not recovered from lm_Hinv: no inverse is inverted
// back, a member without factors adds nothing, and the only solve is the one of the sum.  The kernel runs BEFORE the merged lists are
// uploaded: lm_ptr / lm_fids still describe every member on its own.
//
// One wavefront per cluster, members in ascending id, every lane with the same sums after the tree; everything indexed by unrolled
// loops (registers, no scratch), no LDS, no atomics.  A cluster's x depends on its members alone.
#include <hip/hip_runtime.h>

#include "kernels.hpp"

namespace sl {

template <int D>
__global__ __launch_bounds__(64) void k_lm_merge_fuse(GraphDev G, const int* __restrict__ ptr, const int* __restrict__ mem,
                                                      const int* __restrict__ surv, int n, int* __restrict__ status) {
  constexpr int NH = D * (D + 1) / 2;
  const int c = blockIdx.x, lane = threadIdx.x;
  if (c >= n) return;
  double A[NH], b[D];
#pragma unroll
  for (int i = 0; i < NH; ++i) A[i] = 0.0;
#pragma unroll
  for (int i = 0; i < D; ++i) b[i] = 0.0;
  for (int m = ptr[c]; m < ptr[c + 1]; ++m) {
    const int l = mem[m];
    const int f0 = G.lm_ptr[l], nf = G.lm_ptr[l + 1] - f0;
    if (nf == 0) continue;
    double h[NH];
#pragma unroll
    for (int i = 0; i < NH; ++i) h[i] = 0.0;
    for (int q = lane; q < nf; q += 64) {
      const double* Jl = G.jbuf + G.lf_joff[G.lm_fids[f0 + q]] + D + 6 * D;
#pragma unroll
      for (int k = 0; k < D; ++k) {
        double row[D];
#pragma unroll
        for (int a = 0; a < D; ++a) row[a] = Jl[D * k + a];
#pragma unroll
        for (int a = 0; a < D; ++a)
#pragma unroll
          for (int e = 0; e <= a; ++e) h[a * (a + 1) / 2 + e] += row[a] * row[e];
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
#pragma unroll
      for (int i = 0; i < NH; ++i) h[i] += __shfl_xor(h[i], off);
    double e[D];
#pragma unroll
    for (int i = 0; i < D; ++i) e[i] = G.lm_est[15 * (size_t)l + lm_pair_coord(D, i)];
#pragma unroll
    for (int a = 0; a < D; ++a) {
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < D; ++k) s += h[a >= k ? a * (a + 1) / 2 + k : k * (k + 1) / 2 + a] * e[k];
      b[a] += s;
    }
#pragma unroll
    for (int i = 0; i < NH; ++i) A[i] += h[i];
  }
  // A = C C^T in registers (every lane the same), C y = b, C^T x = y
  double Cm[D][D];
  bool ok = true;
#pragma unroll
  for (int j = 0; j < D; ++j) {
    double s = A[j * (j + 1) / 2 + j];
#pragma unroll
    for (int k = 0; k < j; ++k) s -= Cm[j][k] * Cm[j][k];
    if (!(s > 0.0)) { ok = false; s = 1.0; }
    const double dj = sqrt(s);
    Cm[j][j] = dj;
#pragma unroll
    for (int i = j + 1; i < D; ++i) {
      double t = A[i * (i + 1) / 2 + j];
#pragma unroll
      for (int k = 0; k < j; ++k) t -= Cm[i][k] * Cm[j][k];
      Cm[i][j] = t / dj;
    }
  }
  double x[D];
#pragma unroll
  for (int i = 0; i < D; ++i) {
    double v = b[i];
#pragma unroll
    for (int k = 0; k < i; ++k) v -= Cm[i][k] * x[k];
    x[i] = v / Cm[i][i];
  }
#pragma unroll
  for (int i = D - 1; i >= 0; --i) {
    double v = x[i];
#pragma unroll
    for (int k = i + 1; k < D; ++k) v -= Cm[k][i] * x[k];
    x[i] = v / Cm[i][i];
  }
  if (lane != 0) return;
  status[c] = ok ? 0 : 1;
  if (!ok) return;
  const int sv = surv[c];
#pragma unroll
  for (int i = 0; i < D; ++i) {
    G.lm_val[15 * (size_t)sv + lm_pair_coord(D, i)] = x[i];
    G.lm_est[15 * (size_t)sv + lm_pair_coord(D, i)] = x[i];
    G.lm_delta[9 * (size_t)sv + i] = 0.0;
  }
}

void launch_lm_merge_fuse(const GraphDev& G, int D, const int* ptr, const int* mem, const int* surv, int n, int* status, hipStream_t s) {
  if (n <= 0) return;
  if (D == 3) hipLaunchKernelGGL(k_lm_merge_fuse<3>, dim3(n), dim3(64), 0, s, G, ptr, mem, surv, n, status);
  else hipLaunchKernelGGL(k_lm_merge_fuse<7>, dim3(n), dim3(64), 0, s, G, ptr, mem, surv, n, status);
}

}  // namespace sl
