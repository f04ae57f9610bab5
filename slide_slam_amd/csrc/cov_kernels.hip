// Marginal covariances and loop-closure information gain on the resident Cholesky factor of the reduced pose system
// (the dormant active-SLAM API of the reference: SemanticFactorGraph::logEntropy / estimateClosureInfoGain, graph.h:106,113).
//
// Layout as in chol_kernels.hip: S column-major with leading dimension ld, tile edge NB = 64, the diagonal blocks L_kk as their
// off-diagonal 16x16 sub-blocks in Ld (64x64 column-major per block) plus the inverses of their four 16x16 diagonal sub-blocks in
// Winv (1024 doubles per block, (L_bb^-1)[r][j] at b * 256 + j * 16 + r).  Sigma = S^-1 has S's layout and ld; only tiles inside the
// tile profile are written or read, and the diagonal tiles hold the full symmetric 64x64 block.
//
// Selected inversion (backward over the block columns k, I = k+1 .. prof[k]):
//     Z_I      = L_Ik L_kk^-1                         k_sinv_prep (every k at once)
//     Sigma_Ik = - Sigma_II Z_I                       k_sinv_tile<false>, one workgroup per output tile
//     Sigma_kk = L_kk^-T L_kk^-1 - Sigma_Ik^T Z_I     k_sinv_tile<true>
// Every Sigma(i, j) with i, j in I lies inside the profile (eliminating column k fills exactly that), so the recursion never reads a
// tile outside it.  The products are 64x64 tiles with K = 64 |I| on v_mfma_f64_16x16x4_f64.
// f64 MFMA lane maps (cdna_hip_programming.md §3): A[i = lane&15][k = lane>>4], B[k = lane>>4][j = lane&15],
// D[row = (lane>>4) + 4*reg][col = lane&15].
#include <hip/hip_runtime.h>

#include <algorithm>

#include "graph_dev.hpp"
#include "kernels.hpp"

namespace sl {

namespace {
typedef double v4d __attribute__((ext_vector_type(4)));
__device__ inline v4d mfma_f64(double a, double b, v4d c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }

// Sigma(R, C) of the selected inverse: the lower triangle is stored (and both halves of a diagonal tile)
__device__ __forceinline__ double sig_at(const double* __restrict__ Sg, int ld, int R, int C) {
  return R >= C ? Sg[(size_t)C * ld + R] : Sg[(size_t)R * ld + C];
}

// X[c][r] = (L_kk^-1)[r][c]: block forward substitution on the 64 unit columns, as k_cov_fwd walks the four 16x16 sub-blocks
__device__ void linv_block(double (*X)[NB + 1], const double* __restrict__ Ldk, const double* __restrict__ Wk) {
  const int tid = threadIdx.x;
  for (int e = tid; e < NB * NB; e += 256) X[e >> 6][e & 63] = (e >> 6) == (e & 63) ? 1.0 : 0.0;
  __syncthreads();
  const int c = tid & 63, rq = tid >> 6;        // column c, rows 4 rq .. 4 rq + 3 of a 16-block
#pragma unroll 1
  for (int b = 0; b < 4; ++b) {
    double t[4];
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      double s = 0.0;
#pragma unroll
      for (int j = 0; j < 16; ++j) s += Wk[b * 256 + j * 16 + 4 * rq + rr] * X[c][16 * b + j];
      t[rr] = s;
    }
    __syncthreads();
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) X[c][16 * b + 4 * rq + rr] = t[rr];
    __syncthreads();
    const int nr = 16 * (3 - b);
    for (int e = tid; e < NB * nr; e += 256) {     // rows below block b: y[m] -= sum_n L[m][16 b + n] x[16 b + n]
      const int cc = e / nr, m = 16 * (b + 1) + e % nr;
      double s = 0.0;
#pragma unroll
      for (int n = 0; n < 16; ++n) s += Ldk[(size_t)(16 * b + n) * NB + m] * X[cc][16 * b + n];
      X[cc][m] -= s;
    }
    __syncthreads();
  }
}
}  // namespace

// blockIdx.x = k; blockIdx.y = 0: Sigma_kk <- L_kk^-T L_kk^-1; blockIdx.y = b > 0: Z(k + b, k) = L(k + b, k) L_kk^-1 if inside the profile.
// Every workgroup of column k rebuilds L_kk^-1 in LDS (band + 1 times the work of one): cheap at the chain's band of 2-3 tiles (this
// launch is ~3% of the inversion there); a wide profile would rather build it once per column and read it back.
__global__ __launch_bounds__(256) void k_sinv_prep(const double* __restrict__ S, int ld, int T, const double* __restrict__ Ld,
                                                   const double* __restrict__ Winv, const int* __restrict__ prof, double* __restrict__ Sg,
                                                   double* __restrict__ Z) {
  const int k = blockIdx.x, i = k + (int)blockIdx.y;
  if (i >= T || (prof && i > prof[k])) return;
  __shared__ double X[NB][NB + 1];
  linv_block(X, Ld + (size_t)k * NB * NB, Winv + (size_t)k * 1024);
  const int tid = threadIdx.x;
  if (i == k) {
    for (int e = tid; e < NB * NB; e += 256) {
      const int b = e >> 6, a = e & 63;
      double s = 0.0;
      for (int r = (a > b ? a : b); r < NB; ++r) s += X[a][r] * X[b][r];      // (L^-1 lower triangular)
      Sg[(size_t)(k * NB + b) * ld + (size_t)k * NB + a] = s;
    }
    return;
  }
  const double* L = S + (size_t)(k * NB) * ld + (size_t)i * NB;
  for (int e = tid; e < NB * NB; e += 256) {
    const int c = e >> 6, row = e & 63;
    double s = 0.0;
    for (int q = c; q < NB; ++q) s += L[(size_t)q * ld + row] * X[c][q];
    Z[(size_t)(k * NB + c) * ld + (size_t)i * NB + row] = s;
  }
}

// DIAG = false: blockIdx.x -> tile row i = k + 1 + blockIdx.x, Sigma(i, k) = - sum_{j = k+1 .. i1} Sigma(i, j) Z(j, k).
// DIAG = true (one workgroup): Sigma(k, k) -= sum_{i = k+1 .. i1} Sigma(i, k)^T Z(i, k), then symmetrised.
// Four waves, a 32x32 quadrant each (2 x 2 accumulators); the operand tiles of one K step of 64 are staged in LDS as [k][row / col].
template <bool DIAG>
__global__ __launch_bounds__(256) void k_sinv_tile(double* __restrict__ Sg, const double* __restrict__ Z, int ld, int k, int i1) {
  __shared__ double As[NB][NB + 1];
  __shared__ double Bs[NB][NB + 1];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int lr = lane & 15, lk = lane >> 4, rh = w & 1, ch = w >> 1;
  const int i = DIAG ? k : k + 1 + (int)blockIdx.x;
  v4d acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) acc[a][b] = v4d{0.0, 0.0, 0.0, 0.0};
#pragma unroll 1
  for (int j = k + 1; j <= i1; ++j) {
    if (DIAG) {            // A[r][q] = Sigma(j, k)[q][r]
      const double* src = Sg + (size_t)(k * NB) * ld + (size_t)j * NB;
      for (int e = tid; e < NB * NB; e += 256) { const int r = e >> 6, q = e & 63; As[q][r] = src[(size_t)r * ld + q]; }
    } else if (j <= i) {   // A[r][q] = Sigma(i, j)[r][q]
      const double* src = Sg + (size_t)(j * NB) * ld + (size_t)i * NB;
      for (int e = tid; e < NB * NB; e += 256) { const int q = e >> 6, r = e & 63; As[q][r] = src[(size_t)q * ld + r]; }
    } else {               // A[r][q] = Sigma(j, i)[q][r]
      const double* src = Sg + (size_t)(i * NB) * ld + (size_t)j * NB;
      for (int e = tid; e < NB * NB; e += 256) { const int r = e >> 6, q = e & 63; As[q][r] = src[(size_t)r * ld + q]; }
    }
    {                      // B[q][c] = Z(j, k)[q][c]
      const double* src = Z + (size_t)(k * NB) * ld + (size_t)j * NB;
      for (int e = tid; e < NB * NB; e += 256) { const int c = e >> 6, q = e & 63; Bs[q][c] = src[(size_t)c * ld + q]; }
    }
    __syncthreads();
#pragma unroll 4
    for (int q0 = 0; q0 < NB; q0 += 4) {
      double a[2], b[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        a[t] = As[q0 + lk][32 * rh + 16 * t + lr];
        b[t] = Bs[q0 + lk][32 * ch + 16 * t + lr];
      }
#pragma unroll
      for (int ra = 0; ra < 2; ++ra)
#pragma unroll
        for (int cb = 0; cb < 2; ++cb) acc[ra][cb] = mfma_f64(a[ra], b[cb], acc[ra][cb]);
    }
    __syncthreads();
  }
  if (!DIAG) {
    double* dst = Sg + (size_t)(k * NB) * ld + (size_t)i * NB;
#pragma unroll
    for (int ra = 0; ra < 2; ++ra)
#pragma unroll
      for (int cb = 0; cb < 2; ++cb)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int row = 32 * rh + 16 * ra + lk + 4 * g, col = 32 * ch + 16 * cb + lr;
          dst[(size_t)col * ld + row] = -acc[ra][cb][g];
        }
    return;
  }
  double* dst = Sg + (size_t)(k * NB) * ld + (size_t)k * NB;
#pragma unroll
  for (int ra = 0; ra < 2; ++ra)
#pragma unroll
    for (int cb = 0; cb < 2; ++cb)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int row = 32 * rh + 16 * ra + lk + 4 * g, col = 32 * ch + 16 * cb + lr;
        As[row][col] = dst[(size_t)col * ld + row] - acc[ra][cb][g];
      }
  __syncthreads();
  for (int e = tid; e < NB * NB; e += 256) {
    const int col = e >> 6, row = e & 63;
    dst[(size_t)col * ld + row] = 0.5 * (As[row][col] + As[col][row]);
  }
}

// host: the selected inverse of the factor (prof: host copy of the tile profile, or null: dense; d_prof the device copy or null)
// its first launch alone: Z(i, k) of every tile inside the profile and L_kk^-T L_kk^-1 into the diagonal tiles of Sg
void launch_selected_inverse_prep(const double* S, int ld, int T, const double* Ld, const double* Winv, const int* prof, const int* d_prof,
                                  double* Sg, double* Z, hipStream_t s) {
  if (T <= 0) return;
  int band = 0;
  for (int k = 0; k < T; ++k) band = std::max(band, (prof ? prof[k] : T - 1) - k);
  hipLaunchKernelGGL(k_sinv_prep, dim3(T, band + 1), dim3(256), 0, s, S, ld, T, Ld, Winv, prof ? d_prof : nullptr, Sg, Z);
}
void launch_selected_inverse(const double* S, int ld, int T, const double* Ld, const double* Winv, const int* prof, const int* d_prof,
                             double* Sg, double* Z, hipStream_t s) {
  if (T <= 0) return;
  launch_selected_inverse_prep(S, ld, T, Ld, Winv, prof, d_prof, Sg, Z, s);
  for (int k = T - 1; k >= 0; --k) {
    const int i1 = prof ? prof[k] : T - 1;
    if (i1 <= k) continue;
    hipLaunchKernelGGL((k_sinv_tile<false>), dim3(i1 - k), dim3(256), 0, s, Sg, (const double*)Z, ld, k, i1);
    hipLaunchKernelGGL((k_sinv_tile<true>), dim3(1), dim3(256), 0, s, Sg, (const double*)Z, ld, k, i1);
  }
}

// 6x6 diagonal blocks of the poses rows[p] (pose indices) out of the selected inverse: out[36 p + 6 a + b].  prow: first row of a pose's
// coordinates in Sg (null: 6 p; joint_cov_kernels.hip: a cut's poses live in the border rows)
__global__ void k_pose_blocks(const double* __restrict__ Sg, int ld, const int* __restrict__ poses, int n, double* __restrict__ out,
                              const int* __restrict__ prow) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= 36 * n) return;
  const int p = e / 36, a = (e % 36) / 6, b = e % 6;
  const int r0 = prow ? prow[poses[p]] : 6 * poses[p];
  out[e] = sig_at(Sg, ld, r0 + a, r0 + b);
}
void launch_pose_blocks(const double* Sg, int ld, const int* poses, int n, double* out, hipStream_t s, const int* prow) {
  if (n > 0) hipLaunchKernelGGL(k_pose_blocks, dim3((36 * n + 255) / 256), dim3(256), 0, s, Sg, ld, poses, n, out, prow);
}

// Landmark marginal (Schur identity): Sigma_ll = H_ll^-1 + sum_{f, g in factors(l)} F_f^T Sigma(p_f, p_g) F_g, F = E H_ll^-1 (ebuf).
// One wavefront per landmark lids[q]; out[81 q ..] = the d x d block, row-major.  Per factor f: Q_f = sum_g Sigma(p_f, p_g) F_g
// (6 x d, lane a d + c), then every lane adds its entries of F_f^T Q_f.
__global__ __launch_bounds__(64) void k_lm_cov(GraphDev G, const double* __restrict__ Sg, int ld, const int* __restrict__ lids, int n,
                                               double* __restrict__ out, const int* __restrict__ prow) {
  const int q = blockIdx.x, lane = threadIdx.x;
  if (q >= n) return;
  __shared__ double Qs[54];
  const int l = lids[q];
  const int D = lm_dim(G.lm_type[l]);
  const int f0 = G.lm_ptr[l], nf = G.lm_ptr[l + 1] - f0;
  double acc[2] = {0.0, 0.0};
  const int a = lane / D, c = lane - (lane / D) * D;
  for (int qf = 0; qf < nf; ++qf) {
    const int f = G.lm_fids[f0 + qf];
    const int rf = prow ? prow[G.lf_pose[f]] : 6 * G.lf_pose[f];
    if (lane < 6 * D) {
      double s = 0.0;
      for (int qg = 0; qg < nf; ++qg) {
        const int g = G.lm_fids[f0 + qg];
        const int rg = prow ? prow[G.lf_pose[g]] : 6 * G.lf_pose[g];
        const double* Fg = G.ebuf + G.lf_eoff[g] + 6 * D;
#pragma unroll
        for (int b = 0; b < 6; ++b) s += sig_at(Sg, ld, rf + a, rg + b) * Fg[b * D + c];
      }
      Qs[lane] = s;
    }
    __syncthreads();
    const double* Ff = G.ebuf + G.lf_eoff[f] + 6 * D;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int e = lane + 64 * h;
      if (e < D * D) {
        const int r = e / D, cc = e - r * D;
        double s = 0.0;
#pragma unroll
        for (int aa = 0; aa < 6; ++aa) s += Ff[aa * D + r] * Qs[aa * D + cc];
        acc[h] += s;
      }
    }
    __syncthreads();
  }
  const double* Hi = G.lm_Hinv + 81 * (size_t)l;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int e = lane + 64 * h;
    if (e < D * D) out[81 * (size_t)q + e] = Hi[e] + acc[h];
  }
}
void launch_landmark_covariances(const GraphDev& G, const double* Sg, int ld, const int* lids, int n, double* out, hipStream_t s,
                                 const int* prow) {
  if (n > 0) hipLaunchKernelGGL(k_lm_cov, dim3(n), dim3(64), 0, s, G, Sg, ld, lids, n, out, prow);
}

// ---- landmark pairs on the selected inverse (slide_graph_landmark_pair_mahalanobis / _get_landmark_pair_covariances, route 0) -------
// With the landmarks eliminated H_ll is block diagonal, so the joint marginal of two landmarks a != b of one class (dimension D) is
//     Sig_aa = Hinv_a + X(a, a),   Sig_bb = Hinv_b + X(b, b),   Sig_ab = X(a, b),
//     X(u, v) = sum_{f in factors(u)} sum_{g in factors(v)} F_f^T Sigma(p_f, p_g) F_g,
// F = E H_ll^-1 the factors' Schur records (ebuf) and Sigma the selected inverse: k_lm_cov's sum with the second factor list taken
// from v.  The host sends a pair here only when every Sigma(p_f, p_g) it reads lies inside the tile profile.  One wavefront per pair.
// X(u, v) (D x D, row-major, rows u's coordinates) into Xs; Qs: 54 doubles of LDS.  Every lane of the wavefront calls it.
__device__ __forceinline__ void lm_pair_block(const GraphDev& G, const double* __restrict__ Sg, int ld, int u, int v, int D, double* Qs,
                                              double* Xs) {
  const int lane = threadIdx.x;
  const int fu0 = G.lm_ptr[u], nfu = G.lm_ptr[u + 1] - fu0, fv0 = G.lm_ptr[v], nfv = G.lm_ptr[v + 1] - fv0;
  double acc[2] = {0.0, 0.0};
  const int a = lane / D, c = lane - (lane / D) * D;
  for (int qf = 0; qf < nfu; ++qf) {
    const int f = G.lm_fids[fu0 + qf];
    const int rf = 6 * G.lf_pose[f];
    if (lane < 6 * D) {
      double s = 0.0;
      for (int qg = 0; qg < nfv; ++qg) {
        const int g = G.lm_fids[fv0 + qg];
        const int rg = 6 * G.lf_pose[g];
        const double* Fg = G.ebuf + G.lf_eoff[g] + 6 * D;
#pragma unroll
        for (int b = 0; b < 6; ++b) s += sig_at(Sg, ld, rf + a, rg + b) * Fg[b * D + c];
      }
      Qs[lane] = s;
    }
    __syncthreads();
    const double* Ff = G.ebuf + G.lf_eoff[f] + 6 * D;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int e = lane + 64 * h;
      if (e < D * D) {
        const int r = e / D, cc = e - r * D;
        double s = 0.0;
#pragma unroll
        for (int aa = 0; aa < 6; ++aa) s += Ff[aa * D + r] * Qs[aa * D + cc];
        acc[h] += s;
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int e = lane + 64 * h;
    if (e < D * D) Xs[e] = acc[h];
  }
  __syncthreads();
}
// The pair test: Sig_d = Sig_aa + Sig_bb - Sig_ab - Sig_ab^T, C = I + diag(1 / sigma) Sig_d diag(1 / sigma) from ONE triangle of the
// sum, mirrored, so C is symmetric bit for bit; r = (est_b - est_a) / sigma in the class's tangent order (both classes retract
// additively); then lane 0 factors C = G G^T in registers, solves G y = r and forms d2 = y^T y as k_obs_gate_finish does.  A pivot
// that is not > 0: flag[k] = 1 and zeros.  out: OBS_GATE_OUT doubles per pair, that kernel's layout.
template <int M>
__global__ __launch_bounds__(64) void k_lm_pair_direct(GraphDev G, const double* __restrict__ Sg, int ld, const int2* __restrict__ pairs, int n,
                                                       LmPairSigma sg, double* __restrict__ out, int* __restrict__ flag) {
  __shared__ double Qs[54], Xaa[M * M], Xbb[M * M], Xab[M * M], Cs[M * M], rs[M];
  const int k = blockIdx.x, lane = threadIdx.x;
  if (k >= n) return;
  const int la = pairs[k].x, lb = pairs[k].y;
  lm_pair_block(G, Sg, ld, la, la, M, Qs, Xaa);
  lm_pair_block(G, Sg, ld, lb, lb, M, Qs, Xbb);
  lm_pair_block(G, Sg, ld, la, lb, M, Qs, Xab);
  const double* Ha = G.lm_Hinv + 81 * (size_t)la;
  const double* Hb = G.lm_Hinv + 81 * (size_t)lb;
  if (lane < M * M) {
    const int a = lane / M, b = lane - M * a, hi = a > b ? a : b, lo = a > b ? b : a;
    const double saa = Ha[M * hi + lo] + Xaa[M * hi + lo], sbb = Hb[M * hi + lo] + Xbb[M * hi + lo];
    const double sd = ((saa + sbb) - Xab[M * hi + lo]) - Xab[M * lo + hi];
    Cs[lane] = (a == b ? 1.0 : 0.0) + sd / (sg.s[hi] * sg.s[lo]);
  }
  if (lane < M) {
    const int c = lm_pair_coord(M, lane);
    rs[lane] = (G.lm_est[15 * (size_t)lb + c] - G.lm_est[15 * (size_t)la + c]) / sg.s[lane];
  }
  __syncthreads();
  double d2 = 0.0;
  int bad = 0;
  if (lane == 0) {
    double Gm[M][M], y[M];
    bool spd = true;
#pragma unroll
    for (int j = 0; j < M; ++j) {
      double d = Cs[(M + 1) * j];
#pragma unroll
      for (int q = 0; q < j; ++q) d -= Gm[j][q] * Gm[j][q];
      if (!(d > 0.0)) spd = false;
      const double g = sqrt(spd ? d : 1.0);
      Gm[j][j] = g;
#pragma unroll
      for (int i = j + 1; i < M; ++i) {
        double v = Cs[M * i + j];
#pragma unroll
        for (int q = 0; q < j; ++q) v -= Gm[i][q] * Gm[j][q];
        Gm[i][j] = v / g;
      }
    }
#pragma unroll
    for (int i = 0; i < M; ++i) {
      double v = rs[i];
#pragma unroll
      for (int q = 0; q < i; ++q) v -= Gm[i][q] * y[q];
      y[i] = v / Gm[i][i];
      d2 += y[i] * y[i];
    }
    bad = spd ? 0 : 1;
    flag[k] = bad;
  }
  d2 = __shfl(d2, 0);
  bad = __shfl(bad, 0);
  double* o = out + OBS_GATE_OUT * (size_t)k;
  for (int e = lane; e < OBS_GATE_OUT; e += 64) {
    double v = 0.0;
    if (!bad) {
      if (e == 0) v = d2;
      else if (e < 82) {
        const int a = (e - 1) / 9, b = (e - 1) - 9 * a;
        if (a < M && b < M) v = Cs[M * a + b];
      } else if (e - 82 < M) v = rs[e - 82];
    }
    o[e] = v;
  }
}
void launch_lm_pair_direct(const GraphDev& G, const double* Sg, int ld, int D, const int2* pairs, int n, const LmPairSigma& sg, double* out,
                           int* flag, hipStream_t s) {
  if (n <= 0) return;
  if (D == 3) hipLaunchKernelGGL(k_lm_pair_direct<3>, dim3(n), dim3(64), 0, s, G, Sg, ld, pairs, n, sg, out, flag);
  else hipLaunchKernelGGL(k_lm_pair_direct<7>, dim3(n), dim3(64), 0, s, G, Sg, ld, pairs, n, sg, out, flag);
}
// The joint marginal itself: out[LM_PAIR_COV * k ..] = [[Sig_aa, Sig_ab], [Sig_ab^T, Sig_bb]], 2 D x 2 D row-major with leading
// dimension 18, zero elsewhere.  The diagonal blocks are k_lm_cov's sums in k_lm_cov's order.  Any of the three classes.
__global__ __launch_bounds__(64) void k_lm_pair_cov(GraphDev G, const double* __restrict__ Sg, int ld, const int2* __restrict__ pairs, int n,
                                                    double* __restrict__ out) {
  __shared__ double Qs[54], Xaa[81], Xbb[81], Xab[81];
  const int k = blockIdx.x, lane = threadIdx.x;
  if (k >= n) return;
  const int la = pairs[k].x, lb = pairs[k].y;
  const int D = lm_dim(G.lm_type[la]);
  lm_pair_block(G, Sg, ld, la, la, D, Qs, Xaa);
  lm_pair_block(G, Sg, ld, lb, lb, D, Qs, Xbb);
  lm_pair_block(G, Sg, ld, la, lb, D, Qs, Xab);
  const double* Ha = G.lm_Hinv + 81 * (size_t)la;
  const double* Hb = G.lm_Hinv + 81 * (size_t)lb;
  double* o = out + LM_PAIR_COV * (size_t)k;
  for (int e = lane; e < LM_PAIR_COV; e += 64) {
    const int r = e / 18, c = e - 18 * r;
    double v = 0.0;
    if (r < 2 * D && c < 2 * D) {
      if (r < D && c < D) v = Ha[D * r + c] + Xaa[D * r + c];
      else if (r >= D && c >= D) v = Hb[D * (r - D) + c - D] + Xbb[D * (r - D) + c - D];
      else if (r < D) v = Xab[D * r + c - D];
      else v = Xab[D * c + r - D];
    }
    o[e] = v;
  }
}
void launch_lm_pair_cov(const GraphDev& G, const double* Sg, int ld, const int2* pairs, int n, double* out, hipStream_t s) {
  if (n > 0) hipLaunchKernelGGL(k_lm_pair_cov, dim3(n), dim3(64), 0, s, G, Sg, ld, pairs, n, out);
}

// ---- many right-hand sides: U = S^-1 B (B: nrhs columns of nT = T * NB rows, column-major) --------------------------------------------
// Forward, one launch per block column k: blockIdx.y = chunk of 16 columns; workgroup 0 solves the 64 x 16 block of L_kk and stores
// x_k into X (tile row k), workgroup b > 0 applies tile (k + b, k) to its own rows of Y (in place).  Tile row k of Y is only read in
// this launch, so no workgroup sees another's write.
__global__ __launch_bounds__(256) void k_sub_fwd(const double* __restrict__ S, int ld, int k, const double* __restrict__ Ldk,
                                                 const double* __restrict__ Wk, double* __restrict__ Y, double* __restrict__ X, int nT,
                                                 int nrhs) {
  __shared__ double yk[16][NB];
  __shared__ double xk[16][NB];
  const int tid = threadIdx.x, c0 = 16 * (int)blockIdx.y;
  const int nc = nrhs - c0 < 16 ? nrhs - c0 : 16;
  for (int e = tid; e < 16 * NB; e += 256) {
    const int cc = e / NB, r = e % NB;
    yk[cc][r] = cc < nc ? Y[(size_t)(c0 + cc) * nT + (size_t)k * NB + r] : 0.0;
  }
  __syncthreads();
  const int c = tid >> 4, r = tid & 15;
#pragma unroll 1
  for (int b = 0; b < 4; ++b) {
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < 16; ++j) s += Wk[(size_t)b * 256 + j * 16 + r] * yk[c][16 * b + j];
    xk[c][16 * b + r] = s;
    __syncthreads();
    for (int e = tid; e < 16 * 16 * (3 - b); e += 256) {
      const int cc = e / (16 * (3 - b)), m = 16 * (b + 1) + e % (16 * (3 - b));
      double t = 0.0;
#pragma unroll
      for (int n = 0; n < 16; ++n) t += Ldk[(size_t)(16 * b + n) * NB + m] * xk[cc][16 * b + n];
      yk[cc][m] -= t;
    }
    __syncthreads();
  }
  if (blockIdx.x == 0) {
    for (int e = tid; e < nc * NB; e += 256) X[(size_t)(c0 + e / NB) * nT + (size_t)k * NB + e % NB] = xk[e / NB][e % NB];
    return;
  }
  const int i = k + (int)blockIdx.x;
  const double* tile = S + (size_t)(k * NB) * ld + (size_t)i * NB;
  for (int e = tid; e < nc * NB; e += 256) {
    const int cc = e / NB, row = e % NB;
    double s = 0.0;
#pragma unroll 8
    for (int q = 0; q < NB; ++q) s += tile[(size_t)q * ld + row] * xk[cc][q];
    Y[(size_t)(c0 + cc) * nT + (size_t)i * NB + row] -= s;
  }
}
// Backward, one launch per block column k (from the last): x_k = L_kk^-T (x_k - sum_{i = k+1 .. i1} L_ik^T x_i), in place in X;
// one workgroup per chunk of 16 columns.
__global__ __launch_bounds__(256) void k_sub_bwd(const double* __restrict__ S, int ld, int k, int i1, const double* __restrict__ Ldk,
                                                 const double* __restrict__ Wk, double* __restrict__ X, int nT, int nrhs) {
  __shared__ double Lt[NB][NB + 1];
  __shared__ double xi[16][NB];
  __shared__ double tk[16][NB];
  const int tid = threadIdx.x, c0 = 16 * (int)blockIdx.x;
  const int nc = nrhs - c0 < 16 ? nrhs - c0 : 16;
  for (int e = tid; e < 16 * NB; e += 256) {
    const int cc = e / NB, r = e % NB;
    tk[cc][r] = cc < nc ? X[(size_t)(c0 + cc) * nT + (size_t)k * NB + r] : 0.0;
  }
#pragma unroll 1
  for (int i = k + 1; i <= i1; ++i) {
    const double* tile = S + (size_t)(k * NB) * ld + (size_t)i * NB;
    for (int e = tid; e < NB * NB; e += 256) { const int m = e >> 6, row = e & 63; Lt[m][row] = tile[(size_t)m * ld + row]; }
    for (int e = tid; e < 16 * NB; e += 256) {
      const int cc = e / NB, r = e % NB;
      xi[cc][r] = cc < nc ? X[(size_t)(c0 + cc) * nT + (size_t)i * NB + r] : 0.0;
    }
    __syncthreads();
    for (int e = tid; e < 16 * NB; e += 256) {
      const int cc = e / NB, m = e % NB;
      double s = 0.0;
#pragma unroll 8
      for (int row = 0; row < NB; ++row) s += Lt[m][row] * xi[cc][row];
      tk[cc][m] -= s;
    }
    __syncthreads();
  }
  __syncthreads();
  const int c = tid >> 4, r = tid & 15;
#pragma unroll 1
  for (int b = 3; b >= 0; --b) {
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < 16; ++j) s += Wk[(size_t)b * 256 + r * 16 + j] * tk[c][16 * b + j];      // (L_bb^-1)[j][r]
    __syncthreads();
    tk[c][16 * b + r] = s;
    __syncthreads();
    for (int e = tid; e < 16 * 16 * b; e += 256) {       // rows n of the blocks before b: t[n] -= sum_m L[16 b + m][n] x[16 b + m]
      const int cc = e / (16 * b), n = e % (16 * b);
      double t = 0.0;
#pragma unroll
      for (int m = 0; m < 16; ++m) t += Ldk[(size_t)n * NB + 16 * b + m] * tk[cc][16 * b + m];
      tk[cc][n] -= t;
    }
    __syncthreads();
  }
  for (int e = tid; e < nc * NB; e += 256) X[(size_t)(c0 + e / NB) * nT + (size_t)k * NB + e % NB] = tk[e / NB][e % NB];
}
// B (nrhs columns of T * NB rows) is overwritten; X = S^-1 B
void launch_multi_solve(const double* S, int ld, int T, const double* Ld, const double* Winv, const int* prof, double* B, double* X,
                        int nrhs, hipStream_t s) {
  const int nT = T * NB, nch = (nrhs + 15) / 16;
  if (T <= 0 || nrhs <= 0) return;
  for (int k = 0; k < T; ++k) {
    const int i1 = prof ? prof[k] : T - 1;
    hipLaunchKernelGGL(k_sub_fwd, dim3(i1 - k + 1, nch), dim3(256), 0, s, S, ld, k, Ld + (size_t)k * NB * NB, Winv + (size_t)k * 1024,
                       B, X, nT, nrhs);
  }
  for (int k = T - 1; k >= 0; --k) {
    const int i1 = prof ? prof[k] : T - 1;
    hipLaunchKernelGGL(k_sub_bwd, dim3(nch), dim3(256), 0, s, S, ld, k, i1, Ld + (size_t)k * NB * NB, Winv + (size_t)k * 1024, X, nT, nrhs);
  }
}
// The forward launches alone: W = L^-1 B (B overwritten).  B^T S^-1 B = W^T W needs no backward pass: T launches, not 2 T.
// k0 > 0 (the short walk): B is zero above row k0 * NB, so W is zero there too and the launches of the block columns before k0 would
// subtract zeros from the rows below; the caller has zeroed those rows of W, and the rows from k0 * NB on come out with the bits of
// the walk from column 0 (y - 0 = y).
void launch_multi_fwd(const double* S, int ld, int T, const double* Ld, const double* Winv, const int* prof, double* B, double* W,
                      int nrhs, hipStream_t s, int k0) {
  const int nT = T * NB, nch = (nrhs + 15) / 16;
  if (T <= 0 || nrhs <= 0) return;
  for (int k = k0 < 0 ? 0 : k0; k < T; ++k) {
    const int i1 = prof ? prof[k] : T - 1;
    hipLaunchKernelGGL(k_sub_fwd, dim3(i1 - k + 1, nch), dim3(256), 0, s, S, ld, k, Ld + (size_t)k * NB * NB, Winv + (size_t)k * 1024,
                       B, W, nT, nrhs);
  }
}

// M[a][b] = sum_q X[a ldx + row_q] X[b ldx + row_q] (a, b < ncol), rows = the list or (null) 0 .. nrows-1.  16x16 output tiles.
__global__ __launch_bounds__(256) void k_gram(const double* __restrict__ X, size_t ldx, int ncol, const int* __restrict__ rows, int nrows,
                                              double* __restrict__ M) {
  __shared__ double xa[16][65], xb[16][65];
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const int a0 = 16 * (int)blockIdx.y, b0 = 16 * (int)blockIdx.x;
  double s = 0.0;
  for (int q0 = 0; q0 < nrows; q0 += 64) {
    for (int e = threadIdx.x; e < 16 * 64; e += 256) {
      const int cc = e >> 6, qq = e & 63, q = q0 + qq;
      const int row = q < nrows ? (rows ? rows[q] : q) : -1;
      xa[cc][qq] = (row >= 0 && a0 + cc < ncol) ? X[(size_t)(a0 + cc) * ldx + row] : 0.0;
      xb[cc][qq] = (row >= 0 && b0 + cc < ncol) ? X[(size_t)(b0 + cc) * ldx + row] : 0.0;
    }
    __syncthreads();
#pragma unroll 8
    for (int qq = 0; qq < 64; ++qq) s += xa[ty][qq] * xb[tx][qq];
    __syncthreads();
  }
  if (a0 + ty < ncol && b0 + tx < ncol) M[(size_t)(a0 + ty) * ncol + b0 + tx] = s;
}
void launch_gram(const double* X, size_t ldx, int ncol, const int* rows, int nrows, double* M, hipStream_t s) {
  const int nb = (ncol + 15) / 16;
  if (ncol > 0) hipLaunchKernelGGL(k_gram, dim3(nb, nb), dim3(256), 0, s, X, ldx, ncol, rows, nrows, M);
}

// ---- many candidates side by side (closure_info_gain_batch): candidate k owns the columns c0 .. c0 + nk - 1 of U -------------------------
// Only the nk x nk diagonal blocks of U^T U are formed.  A job is one 16x16 tile of one candidate's block over one split of the row
// list: {candidate, tile row, tile column, split}; split s of a candidate's nsplit covers the rows [s rps, (s + 1) rps), rps the
// rows per split rounded up to 64.  nsplit depends on nk alone and the splits are added in their order by k_gram_reduce, so a block's
// bits depend on its own columns and the row list only — not on what else is in the launch.  No atomics.
__global__ __launch_bounds__(256) void k_gram_blocks(const double* __restrict__ X, size_t ldx, const int* __restrict__ rows, int nrows,
                                                     const GainCandDev* __restrict__ cand, const int4* __restrict__ jobs,
                                                     double* __restrict__ part) {
  __shared__ double xa[16][65], xb[16][65];
  const int4 job = jobs[blockIdx.x];
  const GainCandDev cd = cand[job.x];
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const int la = 16 * job.y, lb = 16 * job.z, nk = cd.nk;
  const int rps = ((nrows + cd.nsplit - 1) / cd.nsplit + 63) & ~63;
  const int q_beg = job.w * rps, q_end = q_beg + rps < nrows ? q_beg + rps : nrows;
  double s = 0.0;
  for (int q0 = q_beg; q0 < q_end; q0 += 64) {
    for (int e = threadIdx.x; e < 16 * 64; e += 256) {
      const int cc = e >> 6, qq = e & 63, q = q0 + qq;
      const int row = q < q_end ? (rows ? rows[q] : q) : -1;
      xa[cc][qq] = (row >= 0 && la + cc < nk) ? X[(size_t)(cd.c0 + la + cc) * ldx + row] : 0.0;
      xb[cc][qq] = (row >= 0 && lb + cc < nk) ? X[(size_t)(cd.c0 + lb + cc) * ldx + row] : 0.0;
    }
    __syncthreads();
#pragma unroll 8
    for (int qq = 0; qq < 64; ++qq) s += xa[ty][qq] * xb[tx][qq];
    __syncthreads();
  }
  if (la + ty < nk && lb + tx < nk) part[cd.poff + (size_t)job.w * nk * nk + (size_t)(la + ty) * nk + lb + tx] = s;
}
// M_k = the sum of candidate k's splits, first to last (blockIdx.x = k)
__global__ __launch_bounds__(256) void k_gram_reduce(const GainCandDev* __restrict__ cand, const double* __restrict__ part,
                                                     double* __restrict__ M) {
  const GainCandDev cd = cand[blockIdx.x];
  const int nn = cd.nk * cd.nk;
  for (int e = threadIdx.x; e < nn; e += 256) {
    double s = 0.0;
    for (int sp = 0; sp < cd.nsplit; ++sp) s += part[cd.poff + (size_t)sp * nn + e];
    M[cd.moff + e] = s;
  }
}
int gain_gram_splits(int nk) {
  const int tiles = ((nk + 15) / 16) * ((nk + 15) / 16);
  return std::max(1, std::min(32, 1024 / tiles));
}
void launch_gram_blocks(const double* X, size_t ldx, const int* rows, int nrows, const GainCandDev* cand, int ncand, const int4* jobs,
                        int njobs, double* part, double* M, hipStream_t s) {
  if (ncand <= 0) return;
  hipLaunchKernelGGL(k_gram_blocks, dim3(njobs), dim3(256), 0, s, X, ldx, rows, nrows, cand, jobs, part);
  hipLaunchKernelGGL(k_gram_reduce, dim3(ncand), dim3(256), 0, s, cand, (const double*)part, M);
}

// The Woodbury step of one candidate per workgroup: C = I + J U from the candidate's rows of J (jptr / jrow / jval: per column of J^T
// the rows of U it touches, ascending) symmetrised as the host's woodbury_drops does, C = L L^T in place (right-looking, lower triangle,
// column-major), L^-1 in place, then g_q = sum_ab (L^-T L^-1)_ab M_q,ab for the nM grams.  C lives in LDS for nk <= GAIN_LDS_DIM
// (SMALL; leading dimension nk | 1) and in the candidate's own slice of `work` otherwise; a launch of either kind leaves the other
// kind's candidates alone.  A pivot that is not > 0: flag[k] = 1 and zeros.  Every loop's order depends on nk alone.
template <bool SMALL>
__global__ __launch_bounds__(256) void k_woodbury_blocks(const double* __restrict__ U, size_t ldu, const GainCandDev* __restrict__ cand,
                                                         const int* __restrict__ jptr, const int* __restrict__ jrow,
                                                         const double* __restrict__ jval, const double* __restrict__ M, size_t msz, int nM,
                                                         double* __restrict__ work, double* __restrict__ gains, int* __restrict__ flag) {
  extern __shared__ double w_lds[];
  __shared__ double dg[6 * GAIN_MAX_STEPS], red[GAIN_MAX_GRAMS][256];
  const GainCandDev cd = cand[blockIdx.x];
  const int n = cd.nk, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  if ((n <= GAIN_LDS_DIM) != SMALL) return;
  double* A = SMALL ? w_lds : work + cd.woff;
  const int lda = SMALL ? (n | 1) : n;
  for (int e = tid; e < n * n; e += 256) {           // C[jr][c] at A[c lda + jr]
    const int c = e / n, jr = e - c * n;
    double v = jr == c ? 1.0 : 0.0;
    const double* u = U + (size_t)(cd.c0 + c) * ldu;
    for (int t = jptr[cd.c0 + jr]; t < jptr[cd.c0 + jr + 1]; ++t) v += jval[t] * u[jrow[t]];
    A[(size_t)c * lda + jr] = v;
  }
  __syncthreads();
  for (int e = tid; e < n * n; e += 256) {
    const int c = e / n, r = e - c * n;
    if (r > c) A[(size_t)c * lda + r] = A[(size_t)r * lda + c] = 0.5 * (A[(size_t)c * lda + r] + A[(size_t)r * lda + c]);
  }
  __syncthreads();
  bool spd = true;
#pragma unroll 1
  for (int j = 0; j < n; ++j) {                      // (the diagonal of L in dg, A's own diagonal is left alone)
    const double d = A[(size_t)j * lda + j];
    if (!(d > 0.0)) { spd = false; break; }          // (every thread reads the same d)
    const double ljj = sqrt(d);
    double* Aj = A + (size_t)j * lda;
    for (int i = j + 1 + tid; i < n; i += 256) Aj[i] /= ljj;
    if (tid == 0) dg[j] = ljj;
    __syncthreads();
    for (int c = j + 1 + wv; c < n; c += 4) {
      const double lcj = Aj[c];
      double* Ac = A + (size_t)c * lda;
      for (int i = c + lane; i < n; i += 64) Ac[i] -= Aj[i] * lcj;
    }
    __syncthreads();
  }
  if (!spd) {
    if (tid < nM) gains[(size_t)blockIdx.x * GAIN_MAX_GRAMS + tid] = 0.0;
    if (tid == 0) flag[blockIdx.x] = 1;
    return;
  }
  // L^-1 in place, last column first: column j below the diagonal = -(L^-1)[j+1.., j+1..] L[j+1.., j] / L[j][j]; dg <- 1 / dg
#pragma unroll 1
  for (int j = n - 1; j >= 0; --j) {
    const double ij = 1.0 / dg[j];
    const double* Aj = A + (size_t)j * lda;
    double v[2] = {0.0, 0.0};
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int i = j + 1 + tid + 256 * h;
      if (i < n) {
        double t = 0.0;
        for (int k = j + 1; k < i; ++k) t += A[(size_t)k * lda + i] * Aj[k];
        v[h] = t + dg[i] * Aj[i];
      }
    }
    __syncthreads();
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int i = j + 1 + tid + 256 * h;
      if (i < n) A[(size_t)j * lda + i] = -v[h] * ij;
    }
    if (tid == 0) dg[j] = ij;
    __syncthreads();
  }
  // (C^-1)_ab = sum_{k >= a} (L^-1)_ka (L^-1)_kb for a >= b; the grams are taken as M_ab + M_ba off the diagonal
  double acc[GAIN_MAX_GRAMS];
#pragma unroll
  for (int q = 0; q < GAIN_MAX_GRAMS; ++q) acc[q] = 0.0;
  for (int e = tid; e < n * n; e += 256) {
    const int a = e / n, b = e - a * n;
    if (b > a) continue;
    const double *Aa = A + (size_t)a * lda, *Ab = A + (size_t)b * lda;
    double ci = a == b ? dg[a] * dg[a] : dg[a] * Ab[a];
    for (int k = a + 1; k < n; ++k) ci += Aa[k] * Ab[k];
#pragma unroll
    for (int q = 0; q < GAIN_MAX_GRAMS; ++q)
      if (q < nM) {
        const double* Mq = M + q * msz + cd.moff;
        acc[q] += ci * (a == b ? Mq[(size_t)a * n + a] : Mq[(size_t)a * n + b] + Mq[(size_t)b * n + a]);
      }
  }
#pragma unroll
  for (int q = 0; q < GAIN_MAX_GRAMS; ++q) red[q][tid] = acc[q];
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if (tid < st)
#pragma unroll
      for (int q = 0; q < GAIN_MAX_GRAMS; ++q) red[q][tid] += red[q][tid + st];
    __syncthreads();
  }
  if (tid < nM) gains[(size_t)blockIdx.x * GAIN_MAX_GRAMS + tid] = red[tid][0];
  if (tid == 0) flag[blockIdx.x] = 0;
}
// gains: GAIN_MAX_GRAMS per candidate (nM used); flag: 0, or 1 where C was not positive definite; small / big: a candidate of that
// kind is in the table.  Returns non-zero when the device refuses the LDS the small kind needs (nothing launched then)
int launch_woodbury_blocks(const double* U, size_t ldu, const GainCandDev* cand, int ncand, const int* jptr, const int* jrow,
                           const double* jval, const double* M, size_t msz, int nM, double* work, double* gains, int* flag, bool small,
                           bool big, hipStream_t s) {
  constexpr size_t lds = (size_t)GAIN_LDS_DIM * (GAIN_LDS_DIM | 1) * sizeof(double);      // (72.75 KiB: past the 64 KiB a launch gets unasked)
  if (ncand <= 0) return 0;
  if (small) {
    // (asked for on every call: the attribute belongs to the current device, and a refusal must not surface as a launch error)
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(k_woodbury_blocks<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
      (void)hipGetLastError();
      return -1;
    }
    hipLaunchKernelGGL((k_woodbury_blocks<true>), dim3(ncand), dim3(256), lds, s, U, ldu, cand, jptr, jrow, jval, M, msz, nM, work, gains, flag);
  }
  if (big) hipLaunchKernelGGL((k_woodbury_blocks<false>), dim3(ncand), dim3(256), 0, s, U, ldu, cand, jptr, jrow, jval, M, msz, nM, work, gains, flag);
  return 0;
}

// V_l = sum_{f in factors(l)} U_{p_f} F_f for the landmarks lids[q]: V[a ldv + 9 q + c] (6m x d, c < 9, zero for c >= d).
// U: ncol columns of nT rows; prow: a pose's first row in U (null: 6 p; a joint system's window poses sit in its border rows).
// One workgroup per landmark, threads over the columns a.
__global__ __launch_bounds__(256) void k_lm_V(GraphDev G, const double* __restrict__ U, int nT, int ncol, const int* __restrict__ lids,
                                              int n, double* __restrict__ V, size_t ldv, const int* __restrict__ prow) {
  const int q = blockIdx.x;
  if (q >= n) return;
  const int l = lids[q];
  const int D = lm_dim(G.lm_type[l]);
  const int f0 = G.lm_ptr[l], f1 = G.lm_ptr[l + 1];
  for (int a = threadIdx.x; a < ncol; a += 256) {
    double v[9];
#pragma unroll
    for (int c = 0; c < 9; ++c) v[c] = 0.0;
    for (int qf = f0; qf < f1; ++qf) {
      const int f = G.lm_fids[qf];
      const double* u = U + (size_t)a * nT + (prow ? (size_t)prow[G.lf_pose[f]] : 6 * (size_t)G.lf_pose[f]);
      const double* F = G.ebuf + G.lf_eoff[f] + 6 * D;
#pragma unroll
      for (int b = 0; b < 6; ++b) {
        const double ub = u[b];
#pragma unroll
        for (int c = 0; c < 9; ++c)
          if (c < D) v[c] += ub * F[b * D + c];
      }
    }
#pragma unroll
    for (int c = 0; c < 9; ++c) V[(size_t)a * ldv + 9 * (size_t)q + c] = v[c];
  }
}
void launch_landmark_V(const GraphDev& G, const double* U, int nT, int ncol, const int* lids, int n, double* V, size_t ldv, hipStream_t s,
                       const int* prow) {
  if (n > 0) hipLaunchKernelGGL(k_lm_V, dim3(n), dim3(256), 0, s, G, U, nT, ncol, lids, n, V, ldv, prow);
}

// scatter (row, col, value) entries into a column-major matrix of nT rows (the whitened Jacobian rows of the candidate closure)
__global__ void k_jt_scatter(const int* __restrict__ rc, const double* __restrict__ val, int n, double* __restrict__ B, int nT) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e < n) B[(size_t)rc[2 * e + 1] * nT + rc[2 * e]] = val[e];
}
void launch_scatter(const int* rc, const double* val, int n, double* B, int nT, hipStream_t s) {
  if (n > 0) hipLaunchKernelGGL(k_jt_scatter, dim3((n + 255) / 256), dim3(256), 0, s, rc, val, n, B, nT);
}

}  // namespace sl
