// The individual-compatibility gate of landmark observations: one candidate observation against what the graph already knows about its
// pose AND its landmark (slide_graph_observation_mahalanobis).  No counterpart in the reference, whose association accepts a match on
// a Euclidean threshold alone (sloam.cpp:73-203); GTSAM users would assemble it from Marginals::jointMarginalCovariance({X(i), L(j)}).
//
// A candidate is the factor slide_graph_add_range_bearing / _add_cube / _add_cylinder would add between pose p and the EXISTING landmark
// l of dimension D (3 / 9 / 7); it has m = D rows.  r (m) and A = [Ap | Al] (m x 6, m x D) are its whitened residual and Jacobian at
// the current estimate (pose_est, lm_est), no robust weight applied.  With H the full system as last linearised and S = L L^T its
// landmark-eliminated pose system,
//     C  = I + A H^-1 A^T = I + Al H_ll^-1 Al^T + B^T S^-1 B,      B = P_p^T Ap^T - sum_{f in factors(l)} P_{p_f}^T F_f Al^T,
//     d2 = r^T C^-1 r,
// F_f = E_f H_ll^-1 the 6 x D block of the factor's Schur record (ebuf + lf_eoff[f] + 6 D, as k_lm_cov and k_lm_V read it) and
// H_ll^-1 the landmark's block of lm_Hinv: the pose-landmark cross block of the marginal is never formed.  B^T S^-1 B = W^T W with
// L W = B is the forward substitution and gram of sigma_forms (host_gates.hip); candidate k of a sweep owns the columns
// m k .. m k + m - 1 of B.
//
// On the JOINT graph of a CholBatch (slide_chol_batch_observation_mahalanobis) K = L D L^T is the exact joint pass's system and
//     C = I + G0 + W^T D W,   L W = B,
// for a PRIVATE landmark with G0 = Al H_ll^-1 Al^T and the B above in joint rows, the factors' poses being poses of the landmark's
// graph (which need not be the candidate pose's); for a SHARED landmark — a separator variable the pass does not eliminate: its
// H_ll^-1 and F are zero — with G0 = 0, no factor sum and Al^T as a right-hand side on the landmark's separator coordinates.  The
// signed gram (D = -I on the lambda rows) is the joint closure gate's (closure_kernels.hip, host_gates.hip's joint_sigma_forms).
#include <hip/hip_runtime.h>

#include "kernels.hpp"

namespace sl {

// (the error functions of the cube and cylinder factors, restated from solver_kernels.hip: cubeFactor.cpp:35, cylinderFactor.cpp:35)
__device__ __forceinline__ void og_cube_err(const SE3& X, const SE3& C, const double* cs, const double* z, double* e) {
  const SE3 M = from12(z);
  const SE3 err = compose(inverse(C), compose(X, M));
  se3_log(err, e);
  e[6] = z[12] - cs[0]; e[7] = z[13] - cs[1]; e[8] = z[14] - cs[2];
}
__device__ __forceinline__ void og_cyl_err(const SE3& X, const double* q, const double* z, double* e) {
  const V3 root = transform_from(X, V3{z[0], z[1], z[2]});
  const V3 ray = mul(X.R, V3{z[3], z[4], z[5]});
  e[0] = q[3] - ray.x; e[1] = q[4] - ray.y; e[2] = q[5] - ray.z;
  e[3] = q[0] - root.x; e[4] = q[1] - root.y; e[5] = q[2] - root.z;
  e[6] = z[6] - q[6];
}

// The linearise-and-fill body of one candidate, one wavefront, shared by k_obs_gate_lin (one graph) and k_joint_obs_gate_lin (the joint
// graph of a CholBatch), as closure_gate_lin_body serves both closure gate kernels.  `type` (FT_BR / FT_CUBE / FT_CYL) is the launch's:
// the host groups candidates by class.  Gp: the graph of the candidate's pose p (its pose_est, numdiff_delta and chart); Gl: the graph
// of its landmark l (its lm_est, chart, Schur records and lm_Hinv) — one and the same on one graph.  z: the measurement as br_z / cu_z /
// cy_z hold it (4 / 15 / 7 used of 15); sg: the sigmas (m used of 9).  The three branches restate k_lin_lf_body's (solver_kernels.hip) at
// pose_est / lm_est: analytic for bearing-range (lane 0), central differences through the variables' own retract for cubes and cylinders
// (lane = 2 column + sign within 32 lanes, lanes 30 / 31 the unperturbed error; the upper 32 lanes repeat the lower ones and store
// nothing).  The record [r | Ap | Al] is staged in LDS (rec, 144 doubles) in jbuf's layout.  colB: the candidate's first column of B
// (ld rows per column).  Rows: row_p the first row of the candidate's pose; pose q of the LANDMARK's graph starts at
// off_l + (prow_l ? prow_l[q] : 6 q); sep_row < 0: a private landmark, else the first row of a separator landmark's coordinates.
// Private: lane 6 j + a owns the entries (row a of a pose, column j) of B for every pose: Ap[j][a] at the candidate's pose, minus
// sum_c F_f[a][c] Al[j][c] at the pose of every factor f of the landmark, in the order of lm_fids — the same lane reads and writes the
// same entry every time, so a pose met twice (the candidate's own pose observing l, a pose holding two factors on l) is an ordered
// read-modify-write, and no atomics are needed; G0 = Al H_ll^-1 Al^T, one triangle computed and mirrored.  Separator landmark (an
// exact pass leaves its H_ll^-1 and F zero: it is not eliminated): Al^T goes to its own rows, no factor sum, G0 = 0.  B is zero before
// the launch and the candidates own disjoint columns.  Stored for the finish: r (r9k, 9) and G0 (G0k, 81, m x m packed).
//
// obs_gate_lin_rec is the linearisation alone — the record [r | Ap | Al] of the candidate at the pose value X (retracted under chart_p,
// differences of step dl) and lm_est[l], staged in rec behind a barrier — so that the gate of a PREDICTED pose (k_obs_gate_lin_pred
// below), whose X is no row of pose_est, linearises by the same text.
__device__ __forceinline__ void obs_gate_lin_rec(const SE3& X, int chart_p, double dl, const GraphDev& Gl, int type, int l,
                                                 const double* __restrict__ z, const double* __restrict__ sg, double* __restrict__ rec) {
  const int lane = threadIdx.x;
  const int m = lf_rows(type);
  const double* lv = Gl.lm_est + 15 * (size_t)l;
  double* Jp = rec + m;
  double* Jl = rec + 7 * m;
  const int j = lane & 31, col = j >> 1;
  const bool st = lane < 32;
  const double fac = 1.0 / (2.0 * dl);
  const double d = (j & 1) ? -dl : dl;
  if (type == FT_BR) {
    const double w = 1.0 / sg[0];
    const V3 q = transform_to(X, V3{lv[0], lv[1], lv[2]});
    const double rho = norm(q);
    const V3 b = (1.0 / rho) * q;
    double e2[2];
    sphere_local(V3{z[0], z[1], z[2]}, b, e2);
    V3 b1, b2;
    sphere_basis(b, b1, b2);
    double Dm[9];
    const double bb[3] = {b.x, b.y, b.z}, c1[3] = {b1.x, b1.y, b1.z}, c2[3] = {b2.x, b2.y, b2.z};
#pragma unroll
    for (int jj = 0; jj < 3; ++jj) {
      double s1 = 0, s2 = 0;
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const double dn = ((i == jj ? 1.0 : 0.0) - bb[i] * bb[jj]) / rho;
        s1 += c1[i] * dn; s2 += c2[i] * dn;
      }
      Dm[jj] = s1; Dm[3 + jj] = s2; Dm[6 + jj] = bb[jj];
    }
    const M3 Q = hat(q);
    if (lane == 0) {
      rec[0] = e2[0] * w; rec[1] = e2[1] * w; rec[2] = (rho - z[3]) * w;
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int jj = 0; jj < 3; ++jj) {
          double s = 0, u = 0;
#pragma unroll
          for (int kk = 0; kk < 3; ++kk) { s += Dm[3 * r + kk] * Q.a[3 * kk + jj]; u += Dm[3 * r + kk] * X.R.a[3 * jj + kk]; }
          Jp[6 * r + jj] = s * w;
          Jp[6 * r + 3 + jj] = -Dm[3 * r + jj] * w;
          Jl[3 * r + jj] = u * w;
        }
    }
  } else if (type == FT_CUBE) {
    const SE3 C = from12(lv);
    double dX[6], dC[6], cs[3];
#pragma unroll
    for (int kk = 0; kk < 6; ++kk) { dX[kk] = (col == kk) ? d : 0.0; dC[kk] = (col == 6 + kk) ? d : 0.0; }
#pragma unroll
    for (int kk = 0; kk < 3; ++kk) cs[kk] = lv[12 + kk] + ((col == 12 + kk) ? d : 0.0);
    double e[9];
    og_cube_err(retract(X, dX, chart_p), retract(C, dC, Gl.chart), cs, z, e);
#pragma unroll
    for (int i = 0; i < 9; ++i) {
      const double hx = __shfl(e[i], 30, 32), eo = __shfl_xor(e[i], 1, 32), w = 1.0 / sg[i];
      if (st && j == 30) rec[i] = hx * w;
      if (st && (j & 1) == 0 && col < 15) {
        const double v = ((e[i] - hx) - (eo - hx)) * fac * w;
        if (col < 6) Jp[6 * i + col] = v;
        else Jl[9 * i + col - 6] = v;
      }
    }
  } else {
    const int jl = col - 6;
    const int vi = jl < 0 ? -1 : (jl < 3 ? jl + 3 : (jl < 6 ? jl - 3 : (jl == 6 ? 6 : -1)));      // tangent [ray, root, radius] onto [root, ray, radius]
    double dX[6], q[7];
#pragma unroll
    for (int kk = 0; kk < 6; ++kk) dX[kk] = (col == kk) ? d : 0.0;
#pragma unroll
    for (int kk = 0; kk < 7; ++kk) q[kk] = lv[kk] + ((vi == kk) ? d : 0.0);
    double e[7];
    og_cyl_err(retract(X, dX, chart_p), q, z, e);
#pragma unroll
    for (int i = 0; i < 7; ++i) {
      const double hx = __shfl(e[i], 30, 32), eo = __shfl_xor(e[i], 1, 32), w = 1.0 / sg[i];
      if (st && j == 30) rec[i] = hx * w;
      if (st && (j & 1) == 0 && col < 13) {
        const double v = ((e[i] - hx) - (eo - hx)) * fac * w;
        if (col < 6) Jp[6 * i + col] = v;
        else Jl[7 * i + jl] = v;
      }
    }
  }
  __syncthreads();
}
__device__ __forceinline__ void obs_gate_lin_body(const GraphDev& Gp, const GraphDev& Gl, int type, int p, int l, const double* __restrict__ z,
                                                  const double* __restrict__ sg, double* __restrict__ rec, double* __restrict__ colB,
                                                  size_t ld, size_t row_p, size_t off_l, const int* __restrict__ prow_l, long long sep_row,
                                                  double* __restrict__ r9k, double* __restrict__ G0k) {
  const int lane = threadIdx.x;
  const int m = lf_rows(type), D = m;
  const double* Jp = rec + m;
  const double* Jl = rec + 7 * m;
  obs_gate_lin_rec(from12(Gp.pose_est + 12 * (size_t)p), Gp.chart, Gp.numdiff_delta, Gl, type, l, z, sg, rec);
  if (sep_row >= 0) {
    if (lane < 6 * m) {
      const int jc = lane / 6, a = lane - 6 * jc;
      colB[(size_t)jc * ld + row_p + a] = Jp[6 * jc + a];
    }
    for (int e = lane; e < m * D; e += 64) {
      const int jc = e / D, c = e - D * jc;
      colB[(size_t)jc * ld + (size_t)sep_row + c] = Jl[jc * D + c];
    }
    for (int e = lane; e < m * m; e += 64) G0k[e] = 0.0;
  } else {
    const int f0 = Gl.lm_ptr[l], f1 = Gl.lm_ptr[l + 1];
    if (lane < 6 * m) {
      const int jc = lane / 6, a = lane - 6 * jc;
      double* cB = colB + (size_t)jc * ld;
      cB[row_p + a] = Jp[6 * jc + a];
      for (int qf = f0; qf < f1; ++qf) {
        const int f = Gl.lm_fids[qf];
        const double* F = Gl.ebuf + Gl.lf_eoff[f] + 6 * D + a * D;
        double s = 0.0;
        for (int c = 0; c < D; ++c) s += F[c] * Jl[jc * D + c];
        const int q = Gl.lf_pose[f];
        double* at = cB + off_l + (prow_l ? (size_t)prow_l[q] : 6 * (size_t)q) + a;
        *at = *at - s;
      }
    }
    if (lane < m * (m + 1) / 2) {
      int i = 0;
      while ((i + 1) * (i + 2) / 2 <= lane) ++i;
      const int jc = lane - i * (i + 1) / 2;      // (i >= jc)
      const double* Hi = Gl.lm_Hinv + 81 * (size_t)l;
      double s = 0.0;
      for (int c = 0; c < D; ++c) {
        double t = 0.0;
        for (int dd = 0; dd < D; ++dd) t += Hi[c * D + dd] * Jl[jc * D + dd];
        s += Jl[i * D + c] * t;
      }
      G0k[m * i + jc] = s;
      G0k[m * jc + i] = s;
    }
  }
  if (lane < m) r9k[lane] = rec[lane];
}
// k_obs_gate_lin, one wavefront per candidate of one graph.  pid / lid: the candidate's pose and landmark ids; z15 / sg9: 15 / 9 per
// candidate; candidate k owns the columns m k .. m k + m - 1 of B (nT rows); a pose's rows are 6 p .. 6 p + 5.
__global__ __launch_bounds__(64) void k_obs_gate_lin(GraphDev G, int type, const int32_t* __restrict__ pid, const int32_t* __restrict__ lid,
                                                     const double* __restrict__ z15, const double* __restrict__ sg9, int n,
                                                     double* __restrict__ B, int nT, double* __restrict__ r9, double* __restrict__ G0) {
  __shared__ double rec[144];
  const int k = blockIdx.x;
  if (k >= n) return;
  const int p = pid[k], m = lf_rows(type);
  obs_gate_lin_body(G, G, type, p, lid[k], z15 + 15 * (size_t)k, sg9 + 9 * (size_t)k, rec, B + (size_t)(m * k) * nT, (size_t)nT, 6 * (size_t)p, 0,
                    nullptr, -1, r9 + 9 * (size_t)k, G0 + 81 * (size_t)k);
}
void launch_obs_gate_lin(const GraphDev& G, int type, const int32_t* pid, const int32_t* lid, const double* z15, const double* sg9, int n,
                         double* B, int nT, double* r9, double* G0, hipStream_t s) {
  if (n > 0) hipLaunchKernelGGL(k_obs_gate_lin, dim3(n), dim3(64), 0, s, G, type, pid, lid, z15, sg9, n, B, nT, r9, G0);
}

// The gate at a PREDICTED pose (slide_graph_predicted_observation_mahalanobis), one wavefront per candidate of one graph.  The pose X_n
// of the candidates is not in the graph: it is the value add_keypose_between(., k, ., rel, X_n) would give a new pose n, tied to the
// graph's pose k by a Between factor of sigmas sg (P.s2 = sg^2).  That factor linearises to H_F = -diag(1 / sg) Ad, H_T = diag(1 / sg)
// with Ad = Ad(X_n^-1 X_k) (closure_gate_lin_body), n touches nothing else, so eliminating n from the augmented system leaves H as it
// is and the augmented marginal is Sig(n, .) = Ad Sig(k, .), Sig(n, n) = Ad Sig(k, k) Ad^T + diag(sg^2): the Between's residual does
// not enter.  The gate of the augmented graph is therefore the gate above with
//     B  = P_k^T (Ap Ad)^T - sum_{f in factors(l)} P_{p_f}^T F_f Al^T,     G0 = Al H_ll^-1 Al^T + Ap diag(sg^2) Ap^T,
// r and A = [Ap | Al] taken at (X_n, lm_est[l]) by obs_gate_lin_rec: no add, no factorisation, the graph untouched.  Ad is staged in
// LDS beside the record (lane 0, before the record's own barrier); lane 6 j + a owns entry (row a, column j) of B at every pose as in the body
// above — (Ap Ad)[j][a] at pose k first, then the factor sum in the order of lm_fids, pose k among them when it observes l — and G0 is
// one triangle computed and mirrored.  The landmark is private (one graph).
__global__ __launch_bounds__(64) void k_obs_gate_lin_pred(GraphDev G, int type, PredPoseDev P, const int32_t* __restrict__ lid,
                                                          const double* __restrict__ z15, const double* __restrict__ sg9, int n,
                                                          double* __restrict__ B, int nT, double* __restrict__ r9, double* __restrict__ G0) {
  __shared__ double rec[144];
  __shared__ double Ads[36];
  const int kc = blockIdx.x, lane = threadIdx.x;
  if (kc >= n) return;
  const int m = lf_rows(type), D = m, l = lid[kc];
  const double* Jp = rec + m;
  const double* Jl = rec + 7 * m;
  const SE3 Xn = from12(P.x);
  if (lane == 0) {
    double Ad[36];
    adjoint(between(Xn, from12(G.pose_est + 12 * (size_t)P.k)), Ad);
#pragma unroll
    for (int i = 0; i < 36; ++i) Ads[i] = Ad[i];
  }
  obs_gate_lin_rec(Xn, G.chart, G.numdiff_delta, G, type, l, z15 + 15 * (size_t)kc, sg9 + 9 * (size_t)kc, rec);
  double* colB = B + (size_t)(m * kc) * nT;
  const int f0 = G.lm_ptr[l], f1 = G.lm_ptr[l + 1];
  if (lane < 6 * m) {
    const int jc = lane / 6, a = lane - 6 * jc;
    double* cB = colB + (size_t)jc * nT;
    double s = 0.0;
    for (int c = 0; c < 6; ++c) s += Jp[6 * jc + c] * Ads[6 * c + a];
    cB[6 * (size_t)P.k + a] = s;
    for (int qf = f0; qf < f1; ++qf) {
      const int f = G.lm_fids[qf];
      const double* F = G.ebuf + G.lf_eoff[f] + 6 * D + a * D;
      double t = 0.0;
      for (int c = 0; c < D; ++c) t += F[c] * Jl[jc * D + c];
      double* at = cB + 6 * (size_t)G.lf_pose[f] + a;
      *at = *at - t;
    }
  }
  if (lane < m * (m + 1) / 2) {
    int i = 0;
    while ((i + 1) * (i + 2) / 2 <= lane) ++i;
    const int jc = lane - i * (i + 1) / 2;      // (i >= jc)
    const double* Hi = G.lm_Hinv + 81 * (size_t)l;
    double s = 0.0;
    for (int c = 0; c < D; ++c) {
      double t = 0.0;
      for (int dd = 0; dd < D; ++dd) t += Hi[c * D + dd] * Jl[jc * D + dd];
      s += Jl[i * D + c] * t;
    }
    double u = 0.0;
    for (int c = 0; c < 6; ++c) u += Jp[6 * i + c] * (P.s2[c] * Jp[6 * jc + c]);
    s += u;
    G0[81 * (size_t)kc + m * i + jc] = s;
    G0[81 * (size_t)kc + m * jc + i] = s;
  }
  if (lane < m) r9[9 * (size_t)kc + lane] = rec[lane];
}
void launch_obs_gate_lin_pred(const GraphDev& G, int type, const PredPoseDev& P, const int32_t* lid, const double* z15, const double* sg9, int n,
                              double* B, int nT, double* r9, double* G0, hipStream_t s) {
  if (n > 0) hipLaunchKernelGGL(k_obs_gate_lin_pred, dim3(n), dim3(64), 0, s, G, type, P, lid, z15, sg9, n, B, nT, r9, G0);
}

// The same fill for the joint-compatibility test (obs_joint_kernels.hip), one wavefront per candidate of one graph: the classes are
// mixed and a candidate's columns start where its group's layout puts them.  cand[k] = {type, pose id, landmark id, first column of
// B}; type < 0: a candidate the group skips, nothing written.  It sits here because it shares the body above.
__global__ __launch_bounds__(64) void k_obs_joint_lin(GraphDev G, const int4* __restrict__ cand, const double* __restrict__ z15,
                                                      const double* __restrict__ sg9, int n, double* __restrict__ B, int nT,
                                                      double* __restrict__ r9, double* __restrict__ G0) {
  __shared__ double rec[144];
  const int k = blockIdx.x;
  if (k >= n) return;
  const int4 c = cand[k];
  if (c.x < 0) return;
  obs_gate_lin_body(G, G, c.x, c.y, c.z, z15 + 15 * (size_t)k, sg9 + 9 * (size_t)k, rec, B + (size_t)c.w * nT, (size_t)nT, 6 * (size_t)c.y, 0,
                    nullptr, -1, r9 + 9 * (size_t)k, G0 + 81 * (size_t)k);
}
void launch_obs_joint_lin(const GraphDev& G, const int4* cand, const double* z15, const double* sg9, int n, double* B, int nT, double* r9,
                          double* G0, hipStream_t s) {
  if (n > 0) hipLaunchKernelGGL(k_obs_joint_lin, dim3(n), dim3(64), 0, s, G, cand, z15, sg9, n, B, nT, r9, G0);
}

// The same fill on the JOINT graph of a CholBatch (slide_chol_batch_observation_mahalanobis), one wavefront per candidate.  ends[k] =
// {graph of the pose, its pose id, graph of the landmark, its landmark id}: the two graphs may differ (robot a's pose against a landmark
// only robot b has mapped).  Gs: the batch's table of its members' views; tab: per graph its prow map and its system's first row in
// the one buffer of ld rows per column (JointPoseTab); sep_row[k]: -1 for a private landmark, else the joint row at which a separator
// landmark's first coordinate enters the walk (its rows in the border of the lowest robot that holds it: the substitution sums the
// robots' rows of separator coordinates into the separator's own).  The factors of a private landmark sit at poses of the LANDMARK's graph; a window pose has its rows in
// its robot's border, which prow already says.
__global__ __launch_bounds__(64) void k_joint_obs_gate_lin(const GraphDev* __restrict__ Gs, const JointPoseTab* __restrict__ tab, int type,
                                                           const int4* __restrict__ ends, const long long* __restrict__ sep_row,
                                                           const double* __restrict__ z15, const double* __restrict__ sg9, int n,
                                                           double* __restrict__ B, size_t ld, double* __restrict__ r9, double* __restrict__ G0) {
  __shared__ double rec[144];
  const int k = blockIdx.x;
  if (k >= n) return;
  const int4 e = ends[k];
  const int m = lf_rows(type);
  obs_gate_lin_body(Gs[e.x], Gs[e.z], type, e.y, e.w, z15 + 15 * (size_t)k, sg9 + 9 * (size_t)k, rec, B + (size_t)(m * k) * ld, ld,
                    (size_t)tab->off[e.x] + tab->prow[e.x][e.y], (size_t)tab->off[e.z], tab->prow[e.z], sep_row[k], r9 + 9 * (size_t)k,
                    G0 + 81 * (size_t)k);
}
void launch_joint_obs_gate_lin(const GraphDev* Gs, const JointPoseTab* tab, int type, const int4* ends, const long long* sep_row, const double* z15,
                               const double* sg9, int n, double* B, size_t ld, double* r9, double* G0, hipStream_t s) {
  if (n > 0) hipLaunchKernelGGL(k_joint_obs_gate_lin, dim3(n), dim3(64), 0, s, Gs, tab, type, ends, sep_row, z15, sg9, n, B, ld, r9, G0);
}

// The joint graph's fill for the joint-compatibility test (slide_chol_batch_observation_joint_compatibility; obs_joint_kernels.hip has
// the invariant): k_joint_obs_gate_lin with a class, a first column and a separator row per wavefront, as k_obs_joint_lin is to
// k_obs_gate_lin.  cand[k] = {type, ., ., first column of B} (the table k_joint_compat_chain reads; type < 0: a candidate the group
// skips, nothing written), ends[k] and sep_row[k] as above.
__global__ __launch_bounds__(64) void k_joint_obs_joint_lin(const GraphDev* __restrict__ Gs, const JointPoseTab* __restrict__ tab,
                                                            const int4* __restrict__ cand, const int4* __restrict__ ends,
                                                            const long long* __restrict__ sep_row, const double* __restrict__ z15,
                                                            const double* __restrict__ sg9, int n, double* __restrict__ B, size_t ld,
                                                            double* __restrict__ r9, double* __restrict__ G0) {
  __shared__ double rec[144];
  const int k = blockIdx.x;
  if (k >= n) return;
  const int4 c = cand[k];
  if (c.x < 0) return;
  const int4 e = ends[k];
  obs_gate_lin_body(Gs[e.x], Gs[e.z], c.x, e.y, e.w, z15 + 15 * (size_t)k, sg9 + 9 * (size_t)k, rec, B + (size_t)c.w * ld, ld,
                    (size_t)tab->off[e.x] + tab->prow[e.x][e.y], (size_t)tab->off[e.z], tab->prow[e.z], sep_row[k], r9 + 9 * (size_t)k,
                    G0 + 81 * (size_t)k);
}
void launch_joint_obs_joint_lin(const GraphDev* Gs, const JointPoseTab* tab, const int4* cand, const int4* ends, const long long* sep_row,
                                const double* z15, const double* sg9, int n, double* B, size_t ld, double* r9, double* G0, hipStream_t s) {
  if (n > 0) hipLaunchKernelGGL(k_joint_obs_joint_lin, dim3(n), dim3(64), 0, s, Gs, tab, cand, ends, sep_row, z15, sg9, n, B, ld, r9, G0);
}

// The fill of a landmark PAIR (slide_graph_landmark_pair_mahalanobis / _get_landmark_pair_covariances, route 1), one wavefront per pair
// of landmarks a != b of one class (dimension D), both private and eliminated.  The hypothesis "a and b are one object up to the noise
// sigma" is the factor with Al = -I / sigma on a and +I / sigma on b and no pose block, so in the private-landmark branch's terms
//     B  = - sum_{f in factors(a)} P_{p_f}^T F_f Al_a^T - sum_{f in factors(b)} P_{p_f}^T F_f Al_b^T
//        = + F_f[.][j] / sigma_j at a's factors' poses, - F_f[.][j] / sigma_j at b's, in column j,
//     G0 = (H_ll,a^-1 + H_ll,b^-1)[i][j] / (sigma_i sigma_j), one triangle computed and mirrored,
//     r  = (est_b - est_a) / sigma in the class's tangent order,
// and k_obs_gate_finish<D> forms C = I + G0 + W^T W and d2 as for an observation: the landmark-landmark cross block is never formed.
// COV: 2 D unit columns instead — column j < D is coordinate j of a (- F_f[.][j] at a's factors' poses), column D + j coordinate j of
// b — whose gram plus the two H_ll^-1 blocks is the pair's joint marginal (k_lm_pair_cov_finish); r9 and G0 are not touched.
// Entry e = 6 j + a of the pair's columns (row a of a pose, column j) belongs to lane e mod 64 in every pass over the factors, a's in
// the order of lm_fids and then b's: a pose met twice is an ordered read-modify-write, no atomics.  B is zero before the launch.
template <bool COV>
__global__ __launch_bounds__(64) void k_lm_pair_fill(GraphDev G, int D, const int2* __restrict__ pairs, LmPairSigma sg, int n,
                                                     double* __restrict__ B, int nT, double* __restrict__ r9, double* __restrict__ G0) {
  const int k = blockIdx.x, lane = threadIdx.x;
  if (k >= n) return;
  const int la = pairs[k].x, lb = pairs[k].y;
  const int nk = COV ? 2 * D : D;
  double* colB = B + (size_t)(nk * k) * nT;
  for (int e = lane; e < 6 * nk; e += 64) {
    const int jc = e / 6, a = e - 6 * jc;
    double* cB = colB + (size_t)jc * nT;
    for (int side = 0; side < 2; ++side) {
      if (COV && side != (jc >= D ? 1 : 0)) continue;
      const int l = side ? lb : la, c = COV && jc >= D ? jc - D : jc;
      const double w = COV ? -1.0 : (side ? -1.0 : 1.0) / sg.s[c];
      for (int qf = G.lm_ptr[l]; qf < G.lm_ptr[l + 1]; ++qf) {
        const int f = G.lm_fids[qf];
        const double* F = G.ebuf + G.lf_eoff[f] + 6 * D + a * D;
        double* at = cB + 6 * (size_t)G.lf_pose[f] + a;
        *at = *at + F[c] * w;
      }
    }
  }
  if (COV) return;
  const double* Ha = G.lm_Hinv + 81 * (size_t)la;
  const double* Hb = G.lm_Hinv + 81 * (size_t)lb;
  if (lane < D * (D + 1) / 2) {
    int i = 0;
    while ((i + 1) * (i + 2) / 2 <= lane) ++i;
    const int jc = lane - i * (i + 1) / 2;      // (i >= jc)
    const double s = (Ha[D * i + jc] + Hb[D * i + jc]) / (sg.s[i] * sg.s[jc]);
    G0[81 * (size_t)k + D * i + jc] = s;
    G0[81 * (size_t)k + D * jc + i] = s;
  }
  if (lane < D) {
    const int c = lm_pair_coord(D, lane);
    r9[9 * (size_t)k + lane] = (G.lm_est[15 * (size_t)lb + c] - G.lm_est[15 * (size_t)la + c]) / sg.s[lane];
  }
}
void launch_lm_pair_fill(const GraphDev& G, int D, bool cov, const int2* pairs, const LmPairSigma& sg, int n, double* B, int nT, double* r9,
                         double* G0, hipStream_t s) {
  if (n <= 0) return;
  if (cov) hipLaunchKernelGGL(k_lm_pair_fill<true>, dim3(n), dim3(64), 0, s, G, D, pairs, sg, n, B, nT, r9, G0);
  else hipLaunchKernelGGL(k_lm_pair_fill<false>, dim3(n), dim3(64), 0, s, G, D, pairs, sg, n, B, nT, r9, G0);
}
// out[LM_PAIR_COV k ..] = the pair's 2 D x 2 D gram (one triangle, mirrored) plus H_ll,a^-1 and H_ll,b^-1 on the diagonal blocks,
// row-major with leading dimension 18, zero elsewhere.  One wavefront per pair.
__global__ __launch_bounds__(64) void k_lm_pair_cov_finish(GraphDev G, int D, const int2* __restrict__ pairs, const double* __restrict__ Mg,
                                                           int n, double* __restrict__ out) {
  const int k = blockIdx.x, lane = threadIdx.x;
  if (k >= n) return;
  const int nk = 2 * D;
  const double* M = Mg + (size_t)(nk * nk) * k;
  for (int e = lane; e < LM_PAIR_COV; e += 64) {
    const int r = e / 18, c = e - 18 * r;
    double v = 0.0;
    if (r < nk && c < nk) {
      const int hi = r > c ? r : c, lo = r > c ? c : r;
      v = M[nk * hi + lo];
      if (hi < D) v += G.lm_Hinv[81 * (size_t)pairs[k].x + D * hi + lo];
      else if (lo >= D) v += G.lm_Hinv[81 * (size_t)pairs[k].y + D * (hi - D) + lo - D];
    }
    out[LM_PAIR_COV * (size_t)k + e] = v;
  }
}
void launch_lm_pair_cov_finish(const GraphDev& G, int D, const int2* pairs, const double* M, int n, double* out, hipStream_t s) {
  if (n > 0) hipLaunchKernelGGL(k_lm_pair_cov_finish, dim3(n), dim3(64), 0, s, G, D, pairs, M, n, out);
}

// The pair's fill on the JOINT graph of a CholBatch (slide_chol_batch_landmark_pair_mahalanobis / _get_landmark_pair_covariances), one
// wavefront per pair.  Gs and tab as k_joint_obs_gate_lin takes them; ends[k] = {graph of a, landmark a, graph of b, landmark b};
// sep_row[2 k], sep_row[2 k + 1]: per side -1 for a private landmark, else the joint row at which a SHARED landmark's first coordinate
// enters the walk (sep_entry_row: its rows in the border of the lowest robot that holds it).  A private side enters as in
// k_lm_pair_fill, its factors' poses being poses of ITS graph g at the joint rows tab->off[g] + tab->prow[g][lf_pose[f]]; a shared
// side is a separator variable the pass does not eliminate: Al^T itself (-I / sigma for a, +I / sigma for b; COV: the unit column)
// goes onto its separator coordinates, it has no factor sum and adds nothing to G0.  The host sends two different variables, so a
// shared side's rows are met by no other write of the pair.  The ownership rule is k_lm_pair_fill's: entry 6 j + a of the pair's
// columns belongs to one lane in every pass over the factors, a's in the order of lm_fids and then b's, so a pose met twice (both
// landmarks private in one graph) is an ordered read-modify-write; no atomics.  B is zero before the launch.  r reads each side's
// estimate in the graph that names it.
template <bool COV>
__global__ __launch_bounds__(64) void k_joint_lm_pair_fill(const GraphDev* __restrict__ Gs, const JointPoseTab* __restrict__ tab, int D,
                                                           const int4* __restrict__ ends, const long long* __restrict__ sep_row, LmPairSigma sg,
                                                           int n, double* __restrict__ B, size_t ld, double* __restrict__ r9,
                                                           double* __restrict__ G0) {
  const int k = blockIdx.x, lane = threadIdx.x;
  if (k >= n) return;
  const int4 e4 = ends[k];
  const long long sa = sep_row[2 * (size_t)k], sb = sep_row[2 * (size_t)k + 1];
  const int nk = COV ? 2 * D : D;
  double* colB = B + (size_t)(nk * k) * ld;
  for (int e = lane; e < 6 * nk; e += 64) {
    const int jc = e / 6, a = e - 6 * jc;
    double* cB = colB + (size_t)jc * ld;
    for (int side = 0; side < 2; ++side) {
      if (COV && side != (jc >= D ? 1 : 0)) continue;
      if ((side ? sb : sa) >= 0) continue;
      const int gi = side ? e4.z : e4.x, l = side ? e4.w : e4.y, c = COV && jc >= D ? jc - D : jc;
      const GraphDev& G = Gs[gi];
      const int* prow = tab->prow[gi];
      const size_t off = (size_t)tab->off[gi];
      const double w = COV ? -1.0 : (side ? -1.0 : 1.0) / sg.s[c];
      for (int qf = G.lm_ptr[l]; qf < G.lm_ptr[l + 1]; ++qf) {
        const int f = G.lm_fids[qf];
        const double* F = G.ebuf + G.lf_eoff[f] + 6 * D + a * D;
        double* at = cB + off + (size_t)prow[G.lf_pose[f]] + a;
        *at = *at + F[c] * w;
      }
    }
  }
  if (lane < D) {
    for (int side = 0; side < 2; ++side) {
      const long long sr = side ? sb : sa;
      if (sr < 0) continue;
      double* at = colB + (size_t)(COV && side ? D + lane : lane) * ld + (size_t)sr + lane;
      *at = *at + (COV ? 1.0 : (side ? 1.0 : -1.0) / sg.s[lane]);
    }
  }
  if (COV) return;
  const GraphDev& Ga = Gs[e4.x];
  const GraphDev& Gb = Gs[e4.z];
  if (lane < D * (D + 1) / 2) {
    int i = 0;
    while ((i + 1) * (i + 2) / 2 <= lane) ++i;
    const int jc = lane - i * (i + 1) / 2;      // (i >= jc)
    const double ha = sa < 0 ? Ga.lm_Hinv[81 * (size_t)e4.y + D * i + jc] : 0.0;
    const double hb = sb < 0 ? Gb.lm_Hinv[81 * (size_t)e4.w + D * i + jc] : 0.0;
    const double s = (ha + hb) / (sg.s[i] * sg.s[jc]);
    G0[81 * (size_t)k + D * i + jc] = s;
    G0[81 * (size_t)k + D * jc + i] = s;
  }
  if (lane < D) {
    const int c = lm_pair_coord(D, lane);
    r9[9 * (size_t)k + lane] = (Gb.lm_est[15 * (size_t)e4.w + c] - Ga.lm_est[15 * (size_t)e4.y + c]) / sg.s[lane];
  }
}
void launch_joint_lm_pair_fill(const GraphDev* Gs, const JointPoseTab* tab, int D, bool cov, const int4* ends, const long long* sep_row,
                               const LmPairSigma& sg, int n, double* B, size_t ld, double* r9, double* G0, hipStream_t s) {
  if (n <= 0) return;
  if (cov) hipLaunchKernelGGL(k_joint_lm_pair_fill<true>, dim3(n), dim3(64), 0, s, Gs, tab, D, ends, sep_row, sg, n, B, ld, r9, G0);
  else hipLaunchKernelGGL(k_joint_lm_pair_fill<false>, dim3(n), dim3(64), 0, s, Gs, tab, D, ends, sep_row, sg, n, B, ld, r9, G0);
}
// k_lm_pair_cov_finish on the joint graph: the pair's 2 D x 2 D SIGNED gram (one triangle, mirrored) plus H_ll^-1 of each PRIVATE side
// on its diagonal block, read in that side's graph; a shared side's block is the gram's alone.  One wavefront per pair.
__global__ __launch_bounds__(64) void k_joint_lm_pair_cov_finish(const GraphDev* __restrict__ Gs, int D, const int4* __restrict__ ends,
                                                                 const long long* __restrict__ sep_row, const double* __restrict__ Mg, int n,
                                                                 double* __restrict__ out) {
  const int k = blockIdx.x, lane = threadIdx.x;
  if (k >= n) return;
  const int nk = 2 * D;
  const int4 e4 = ends[k];
  const bool pa = sep_row[2 * (size_t)k] < 0, pb = sep_row[2 * (size_t)k + 1] < 0;
  const double* M = Mg + (size_t)(nk * nk) * k;
  for (int e = lane; e < LM_PAIR_COV; e += 64) {
    const int r = e / 18, c = e - 18 * r;
    double v = 0.0;
    if (r < nk && c < nk) {
      const int hi = r > c ? r : c, lo = r > c ? c : r;
      v = M[nk * hi + lo];
      if (hi < D) { if (pa) v += Gs[e4.x].lm_Hinv[81 * (size_t)e4.y + D * hi + lo]; }
      else if (lo >= D) { if (pb) v += Gs[e4.z].lm_Hinv[81 * (size_t)e4.w + D * (hi - D) + lo - D]; }
    }
    out[LM_PAIR_COV * (size_t)k + e] = v;
  }
}
void launch_joint_lm_pair_cov_finish(const GraphDev* Gs, int D, const int4* ends, const long long* sep_row, const double* M, int n, double* out,
                                     hipStream_t s) {
  if (n > 0) hipLaunchKernelGGL(k_joint_lm_pair_cov_finish, dim3(n), dim3(64), 0, s, Gs, D, ends, sep_row, M, n, out);
}

// k_obs_gate_finish, one wavefront per candidate (four to a workgroup): C = (I + G0) + M, M the candidate's m x m gram W_k^T W_k at
// m m k; entries (a, b) and (b, a) are one sum of the same operands, so C is symmetric bit for bit.  Lane 0 factors C = G G^T in
// registers, solves G y = r and forms d2 = y^T y.  A pivot that is not > 0: flag[k] = 1 and zeros.  out: OBS_GATE_OUT doubles per
// candidate, [d2 | C row-major, leading dimension 9, zero outside the m x m block (81) | r (9)].
template <int M>
__global__ __launch_bounds__(256) void k_obs_gate_finish(const double* __restrict__ Mg, const double* __restrict__ G0,
                                                         const double* __restrict__ r9, int n, double* __restrict__ out,
                                                         int* __restrict__ flag) {
  __shared__ double Cs[4][M * M];
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int k = blockIdx.x * 4 + wv;
  if (k < n)
    for (int e = lane; e < M * M; e += 64) {
      const int a = e / M, b = e - M * a, hi = a > b ? a : b, lo = a > b ? b : a;
      Cs[wv][e] = ((a == b ? 1.0 : 0.0) + G0[81 * (size_t)k + M * hi + lo]) + Mg[(size_t)(M * M) * k + M * hi + lo];
    }
  __syncthreads();
  if (k >= n) return;
  double d2 = 0.0;
  int bad = 0;
  if (lane == 0) {
    double Gm[M][M], y[M];
    bool spd = true;
#pragma unroll
    for (int j = 0; j < M; ++j) {
      double d = Cs[wv][(M + 1) * j];
#pragma unroll
      for (int q = 0; q < j; ++q) d -= Gm[j][q] * Gm[j][q];
      if (!(d > 0.0)) spd = false;
      const double g = sqrt(spd ? d : 1.0);
      Gm[j][j] = g;
#pragma unroll
      for (int i = j + 1; i < M; ++i) {
        double v = Cs[wv][M * i + j];
#pragma unroll
        for (int q = 0; q < j; ++q) v -= Gm[i][q] * Gm[j][q];
        Gm[i][j] = v / g;
      }
    }
#pragma unroll
    for (int i = 0; i < M; ++i) {
      double v = r9[9 * (size_t)k + i];
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
        if (a < M && b < M) v = Cs[wv][M * a + b];
      } else if (e - 82 < M) v = r9[9 * (size_t)k + e - 82];
    }
    o[e] = v;
  }
}
void launch_obs_gate_finish(int m, const double* Mg, const double* G0, const double* r9, int n, double* out, int* flag, hipStream_t s) {
  if (n <= 0) return;
  const dim3 grid((n + 3) / 4), block(256);
  if (m == 3) hipLaunchKernelGGL(k_obs_gate_finish<3>, grid, block, 0, s, Mg, G0, r9, n, out, flag);
  else if (m == 7) hipLaunchKernelGGL(k_obs_gate_finish<7>, grid, block, 0, s, Mg, G0, r9, n, out, flag);
  else hipLaunchKernelGGL(k_obs_gate_finish<9>, grid, block, 0, s, Mg, G0, r9, n, out, flag);
}

}  // namespace sl
