// The joint-compatibility test of a key frame's landmark matches (slide_graph_observation_joint_compatibility): the candidates of a
// group are judged TOGETHER, as Neira and Tardos' joint compatibility test does, in its greedy sequential form.  No counterpart in
// the reference, whose association accepts each match on a Euclidean threshold alone (sloam.cpp:73-203).
//
// A group's served candidates are the factors obs_gate_kernels.hip describes (m_i = 3 / 9 / 7 rows each), stacked in the caller's
// order: r = [r_1; ..], A = [A_1; ..], n = sum m_i rows.  With S = L L^T the landmark-eliminated pose system and L W = B the forward
// substitution of the sweep (B_i the columns the fill writes for candidate i, exactly those of the individual gate),
//     C = I + A H^-1 A^T,     block (i, j) = [i == j] (I + Al_i H_ll^-1 Al_i^T) + W_i^T W_j,
// because H_ll is block diagonal and a group names no landmark twice: the landmark-landmark part of H^-1 between two different
// landmarks is F_i^T S^-1 F_j alone, which the columns of B carry already.  So C is the group's whole gram W^T W (cov_kernels.hip's
// k_gram_blocks over the lower 16 x 16 tiles) plus I + G0_i on the diagonal blocks.
//
//
// On the JOINT graph of a CholBatch (slide_chol_batch_observation_joint_compatibility) K = L D L^T is the joint system of the last whole
// exact pass, D = -I on the lambda block of the inter-robot relative-pose factors, and with the same stacking
//     C = I + A K^-1 A^T,     block (i, j) = [i == j] (I + G0_i) + W_i^T D W_j,     L W = B,
// B_i and G0_i exactly what k_joint_obs_gate_lin writes for candidate i (obs_gate_kernels.hip; k_joint_obs_joint_lin is that fill with a
// class and a column per wavefront).  Private landmark: G0 = Al H_ll^-1 Al^T, the factor sum over the landmark's own graph's poses in
// joint rows.  Shared landmark: G0 = 0, Al^T on its separator coordinates through the lowest robot's rows.  The cross blocks are the
// off-diagonal part of the SIGNED gram M - Mneg over JointGain::form_rows' two lists (host_sigma.hpp).  A private landmark may not
// be named twice in a group — identity (landmark's slot, local id): H_ll is block diagonal and the cross block would miss
// Al_i H_ll^-1 Al_j^T.  A shared landmark may — identity its separator offset, two replicas being one landmark: it is a separator
// variable the pass does not eliminate, everything about it is in K, and W_i^T D W_j is the whole cross block.  The chain below runs on
// the signed gram as it is: it reads ([a == b] + G0[hi][lo]) + M[hi][lo] below the diagonal only, so C stays symmetric bit for bit.
//
// The rule (k_joint_compat_chain, one workgroup per group, the candidates in the caller's order): S the accepted set, L_S L_S^T = C_SS
// and y_S = L_S^-1 r_S kept as they grow, d2_S = y_S^T y_S.  For candidate i
//     d2_single = r_i^T C_ii^-1 r_i,
//     X = C_iS L_S^-T,   D = C_ii - X X^T = G G^T,   y_i = G^-1 (r_i - X y_S),   d2_joint = d2_S + y_i^T y_i,   dof_joint = |S| + m_i,
// accepted iff d2_single <= q(m_i) and d2_joint <= q(dof_joint), q the chi-square quantiles of the call's probability (evaluate only:
// always); on acceptance [X | G] become the factor's next rows and y_i the next entries of y.  A pivot of D or C_ii that is not > 0:
// the candidate is rejected with SLIDE_ERR_NOT_SPD and zeros, the chain goes on.
#include <hip/hip_runtime.h>

#include "kernels.hpp"

namespace sl {

// C = G G^T of an M x M block (row-major, lower triangle read), G y = rhs, d2 = y^T y, in one thread's registers as k_obs_gate_finish
// does.  Gout (row-major M x M, lower triangle written) and yout may be null.  False when a pivot is not > 0.
template <int M>
__device__ __forceinline__ bool jc_factor(const double* Cm, const double* rhs, double* Gout, double* yout, double& d2) {
  double Gm[M][M], y[M];
  bool spd = true;
#pragma unroll
  for (int j = 0; j < M; ++j) {
    double d = Cm[(M + 1) * j];
#pragma unroll
    for (int q = 0; q < j; ++q) d -= Gm[j][q] * Gm[j][q];
    if (!(d > 0.0)) spd = false;
    const double g = sqrt(spd ? d : 1.0);
    Gm[j][j] = g;
#pragma unroll
    for (int i = j + 1; i < M; ++i) {
      double v = Cm[M * i + j];
#pragma unroll
      for (int q = 0; q < j; ++q) v -= Gm[i][q] * Gm[j][q];
      Gm[i][j] = v / g;
    }
  }
  d2 = 0.0;
#pragma unroll
  for (int i = 0; i < M; ++i) {
    double v = rhs[i];
#pragma unroll
    for (int q = 0; q < i; ++q) v -= Gm[i][q] * y[q];
    y[i] = v / Gm[i][i];
    d2 += y[i] * y[i];
  }
  if (Gout) {
#pragma unroll
    for (int i = 0; i < M; ++i)
#pragma unroll
      for (int j = 0; j <= i; ++j) Gout[M * i + j] = Gm[i][j];
  }
  if (yout) {
#pragma unroll
    for (int i = 0; i < M; ++i) yout[i] = y[i];
  }
  return spd;
}

// what the workgroup keeps in LDS beside the factor
struct JcShared {
  double Xs[9][JOINT_MAX_ROWS + 1];      // the new block's rows against the accepted columns: C_iS, then X
  double ys[JOINT_MAX_ROWS];             // y_S
  double Cii[81], Dm[81], Gs[81];        // C_ii, D (C_ii before the dots are taken off), G
  double ri[9], rj[9], ynew[9];          // r_i, r_i - X y_S, y_i
  double d2[2];                          // d2_single, y_i^T y_i
  int spd[2];
  int fcol[JOINT_MAX_ROWS];              // factor row -> row of the group's C
};

// One step of the chain: candidate k (of the sweep's table) with M rows at the group's rows o .. o + M - 1; s rows accepted so far in
// the factor Lf (row-major, leading dimension lda).  On acceptance s, d2S and count move on.
template <int M>
__device__ __forceinline__ void jc_step(JcShared& sh, double* Lf, int lda, const double* __restrict__ Mg, int n, int o, size_t k,
                                        const double* __restrict__ G0, const double* __restrict__ r9, const double* __restrict__ qtab,
                                        int evaluate_only, int& s, double& d2S, int& count, double* __restrict__ out_d,
                                        int* __restrict__ out_i) {
  const int tid = threadIdx.x;
  // C_iS (the gram's rows of the candidate at the accepted columns: below the diagonal, so in the lower tiles) and C_ii, each sum
  // read from the one place (hi, lo) that holds it
  for (int e = tid; e < M * s; e += 256) {
    const int a = e / s, t = e - a * s;
    sh.Xs[a][t] = Mg[(size_t)(o + a) * n + sh.fcol[t]];
  }
  if (tid < M * M) {
    const int a = tid / M, b = tid - M * a, hi = a > b ? a : b, lo = a > b ? b : a;
    const double v = ((a == b ? 1.0 : 0.0) + G0[81 * k + M * hi + lo]) + Mg[(size_t)(o + hi) * n + o + lo];
    sh.Cii[tid] = v;
    sh.Dm[tid] = v;
  }
  if (tid < M) sh.ri[tid] = r9[9 * k + tid];
  __syncthreads();
  // X L_S^T = C_iS, JOINT_TB columns at a time.  The block's triangle: 16 lanes per row of X, lane j holding column t0 + j of the
  // row and row t0 + j of the triangle in registers; step t divides lane t's entry by the pivot and hands it round (a shuffle inside
  // the 16 lanes), the lanes to its right take their part off — the sums in the columns' order.  Then every column to the right of
  // the block takes the block's part off, the workgroup over rows x columns (a full block: only the last one can be short).
  const int pa = tid >> 4, pj = tid & 15;
#pragma unroll 1
  for (int t0 = 0; t0 < s; t0 += JOINT_TB) {
    const int w = s - t0 < JOINT_TB ? s - t0 : JOINT_TB;
    if (pa < M) {
      const bool on = pj < w;
      const double* Lr = Lf + (size_t)(t0 + (on ? pj : 0)) * lda + t0;
      double Lrow[JOINT_TB];
#pragma unroll
      for (int q = 0; q < JOINT_TB; ++q) Lrow[q] = (on && q < pj) ? Lr[q] : 0.0;
      const double dg = on ? Lr[pj] : 1.0;
      double x = on ? sh.Xs[pa][t0 + pj] : 0.0;
#pragma unroll
      for (int t = 0; t < JOINT_TB; ++t) {
        if (pj == t) x = x / dg;
        const double xt = __shfl(x, t, JOINT_TB);
        if (pj > t) x -= Lrow[t] * xt;
      }
      if (on) sh.Xs[pa][t0 + pj] = x;
    }
    __syncthreads();
    const int rem = s - t0 - w;
    for (int e = tid; e < M * rem; e += 256) {
      const int uu = e / M, a = e - M * uu, u = t0 + JOINT_TB + uu;
      const double* Lu = Lf + (size_t)u * lda + t0;
      double v = sh.Xs[a][u];
#pragma unroll
      for (int q = 0; q < JOINT_TB; ++q) v -= sh.Xs[a][t0 + q] * Lu[q];
      sh.Xs[a][u] = v;
    }
    __syncthreads();
  }
  // D = C_ii - X X^T (the lower triangle: all the factorisation reads) and r_i - X y_S, one thread per entry, the sums in the columns' order
  if (tid < M * (M + 1) / 2) {
    int a = 0;
    while ((a + 1) * (a + 2) / 2 <= tid) ++a;
    const int b = tid - a * (a + 1) / 2;      // (a >= b)
    double dot = 0.0;
#pragma unroll 8
    for (int t = 0; t < s; ++t) dot += sh.Xs[a][t] * sh.Xs[b][t];
    sh.Dm[M * a + b] = sh.Dm[M * a + b] - dot;
  } else if (tid >= 64 && tid < 64 + M) {
    const int a = tid - 64;
    double dot = 0.0;
#pragma unroll 8
    for (int t = 0; t < s; ++t) dot += sh.Xs[a][t] * sh.ys[t];
    sh.rj[a] = sh.ri[a] - dot;
  }
  __syncthreads();
  // the two M x M factorisations, each in one thread's registers, on two wavefronts
  if (tid == 0) {
    double d2 = 0.0;
    sh.spd[1] = jc_factor<M>(sh.Dm, sh.rj, sh.Gs, sh.ynew, d2) ? 1 : 0;
    sh.d2[1] = d2;
  } else if (tid == 64) {
    double d2 = 0.0;
    sh.spd[0] = jc_factor<M>(sh.Cii, sh.ri, nullptr, nullptr, d2) ? 1 : 0;
    sh.d2[0] = d2;
  }
  __syncthreads();
  const bool spd = sh.spd[0] && sh.spd[1];
  const double d2s = sh.d2[0], d2j = d2S + sh.d2[1];
  const int dof = s + M;
  const bool acc = spd && (evaluate_only || (d2s <= qtab[M - 1] && d2j <= qtab[dof - 1]));
  if (tid == 0) {
    out_d[2 * k] = spd ? d2s : 0.0;
    out_d[2 * k + 1] = spd ? d2j : 0.0;
    out_i[3 * k] = acc ? 1 : 0;
    out_i[3 * k + 1] = spd ? dof : 0;
    out_i[3 * k + 2] = spd ? 0 : 1;
  }
  if (acc) {
    for (int e = tid; e < M * s; e += 256) {
      const int a = e / s, t = e - a * s;
      Lf[(size_t)(s + a) * lda + t] = sh.Xs[a][t];
    }
    if (tid < M * M) {
      const int a = tid / M, b = tid - M * a;
      if (b <= a) Lf[(size_t)(s + a) * lda + s + b] = sh.Gs[tid];
    }
    if (tid < M) {
      sh.ys[s + tid] = sh.ynew[tid];
      sh.fcol[s + tid] = o + tid;
    }
    s += M;
    d2S = d2j;
    ++count;
  }
  __syncthreads();
}

// k_joint_compat_chain, one workgroup per group.  grp[g]: the group's first column c0 of the sweep, its rows nk, its gram at Mg + moff
// (nk x nk row-major, the lower 16 x 16 tiles valid), its slice of the work buffer at woff; gcand[g] = {first candidate, count} in the
// sweep's table cand[k] = {type (FT_BR / FT_CUBE / FT_CYL; < 0: skipped), pose id, landmark id, first column in the sweep}; G0 / r9:
// what the fill stored per candidate (81 / 9).  qtab[d - 1]: the quantile of d degrees of freedom, d = 1 .. JOINT_MAX_ROWS.  The factor
// lives in LDS (SMALL: nk <= GAIN_LDS_DIM, leading dimension nk | 1) or in the group's slice of `work`; a launch of either kind
// leaves the other kind's groups alone (k_woodbury_blocks' pattern).  Every loop's order depends on the group's own sizes alone.
// Per candidate out_d = {d2_single, d2_joint}, out_i = {accepted, dof_joint, 1 where a pivot was not > 0} (zeros for a skipped one);
// per group gout_d = d2 of the accepted set, gout_i = {its rows, its count}.
template <bool SMALL>
__global__ __launch_bounds__(256) void k_joint_compat_chain(const GainCandDev* __restrict__ grp, const int2* __restrict__ gcand,
                                                            const int4* __restrict__ cand, const double* __restrict__ Mg,
                                                            const double* __restrict__ G0, const double* __restrict__ r9,
                                                            const double* __restrict__ qtab, int evaluate_only, double* work,
                                                            double* __restrict__ out_d, int* __restrict__ out_i,
                                                            double* __restrict__ gout_d, int* __restrict__ gout_i) {
  extern __shared__ double jc_lds[];
  __shared__ JcShared sh;
  const GainCandDev cd = grp[blockIdx.x];
  const int n = cd.nk;
  if ((n <= GAIN_LDS_DIM) != SMALL) return;
  double* Lf = SMALL ? jc_lds : work + cd.woff;
  const int lda = SMALL ? (n | 1) : n;
  const int2 gc = gcand[blockIdx.x];
  const double* Mgrp = Mg + cd.moff;
  int s = 0, count = 0;
  double d2S = 0.0;
#pragma unroll 1
  for (int i = 0; i < gc.y; ++i) {
    const size_t k = (size_t)gc.x + i;
    const int4 c = cand[k];
    const int o = c.w - cd.c0;
    if (c.x == FT_BR) jc_step<3>(sh, Lf, lda, Mgrp, n, o, k, G0, r9, qtab, evaluate_only, s, d2S, count, out_d, out_i);
    else if (c.x == FT_CUBE) jc_step<9>(sh, Lf, lda, Mgrp, n, o, k, G0, r9, qtab, evaluate_only, s, d2S, count, out_d, out_i);
    else if (c.x == FT_CYL) jc_step<7>(sh, Lf, lda, Mgrp, n, o, k, G0, r9, qtab, evaluate_only, s, d2S, count, out_d, out_i);
    else if (threadIdx.x == 0) {
      out_d[2 * k] = 0.0; out_d[2 * k + 1] = 0.0;
      out_i[3 * k] = 0; out_i[3 * k + 1] = 0; out_i[3 * k + 2] = 0;
    }
  }
  if (threadIdx.x == 0) {
    gout_d[blockIdx.x] = d2S;
    gout_i[2 * blockIdx.x] = s;
    gout_i[2 * blockIdx.x + 1] = count;
  }
}
// lds_rows: the rows of the largest group that is factored in LDS (0: none), any_big: a group past GAIN_LDS_DIM rows is in the table.
// Returns non-zero when the device refuses the LDS the small kind needs (nothing launched then).
int launch_joint_compat_chain(const GainCandDev* grp, const int2* gcand, int ngroups, const int4* cand, const double* Mg, const double* G0,
                              const double* r9, const double* qtab, int evaluate_only, double* work, int lds_rows, bool any_big, double* out_d,
                              int* out_i, double* gout_d, int* gout_i, hipStream_t s) {
  if (ngroups <= 0) return 0;
  if (lds_rows > 0) {
    const size_t lds = (size_t)lds_rows * (lds_rows | 1) * sizeof(double);
    // (asked for on every call, as launch_woodbury_blocks does: the attribute belongs to the current device)
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(k_joint_compat_chain<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)((size_t)GAIN_LDS_DIM * (GAIN_LDS_DIM | 1) * sizeof(double))) != hipSuccess) {
      (void)hipGetLastError();
      return -1;
    }
    hipLaunchKernelGGL((k_joint_compat_chain<true>), dim3(ngroups), dim3(256), lds, s, grp, gcand, cand, Mg, G0, r9, qtab, evaluate_only, work,
                       out_d, out_i, gout_d, gout_i);
  }
  if (any_big)
    hipLaunchKernelGGL((k_joint_compat_chain<false>), dim3(ngroups), dim3(256), 0, s, grp, gcand, cand, Mg, G0, r9, qtab, evaluate_only, work,
                       out_d, out_i, gout_d, gout_i);
  return 0;
}

}  // namespace sl
