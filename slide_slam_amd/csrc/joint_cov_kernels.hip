// Marginal covariances on the factor of the exact joint pass (CholBatch, arrow mode): the selected inverse over the pass's elimination
// tree — the robots' band segments, the bands' second level (the windows of poses between the segments), the separator's leaves and top
// block, then the lambda block of the inter-robot relative-pose factors.
//
// Every node of that tree is a block column c of ONE of nine "systems": the separator (landmark columns in sepS, lambda columns in lamS)
// and every robot (band columns in its S, window columns in its border block bord).  A system's factor columns live in two stores:
//     tile (R, C), C <  Tb:  S + C NB ld  + R NB                (rows R >= Tb: the stored border rows, W^T)
//     tile (R, C), C >= Tb:  B + (C - Tb) NB ldb + (R - Tb) NB
// and its Sigma (and the scratch Z) is one dense lower matrix of Trow NB rows: tile (R, C) at Sg + C NB lds + R NB, both halves of a
// diagonal tile.  Rows of a robot past its factor columns are separator coordinates: k_jsig_gather copies their Sigma from the separator's
// through the robot's border map before the robot's own columns run.
//
// Takahashi's recursion, backward over the columns c of a system, I = the tile rows of column c (host row lists: a profile in the band,
// the border rows active in the segment, the top block + lambda rows of a leaf — never the other leaf):
//     Z_I      = L_Ic L_cc^-1                               k_jsinv_prep (every column of every system at once)
//     Sigma_Ic = - Sigma_II Z_I                             k_jsinv_tile<false>
//     Sigma_cc = L_cc^-T D_c L_cc^-1 - Sigma_Ic^T Z_I       k_jsinv_tile<true>;  D_c = -I on the lambda block (factored as its negative)
// cov_kernels.hip's k_sinv_prep / k_sinv_tile are the one-store, contiguous-row special case of these.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "graph_dev.hpp"
#include "kernels.hpp"

namespace sl {

namespace {
typedef double v4d __attribute__((ext_vector_type(4)));
__device__ inline v4d mfma_f64(double a, double b, v4d c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }

__device__ __forceinline__ const double* jl_tile(const JSinvSys& Y, int R, int C) {
  return C < Y.Tb ? Y.S + (size_t)C * NB * Y.ld + (size_t)R * NB : Y.B + (size_t)(C - Y.Tb) * NB * Y.ldb + (size_t)(R - Y.Tb) * NB;
}
__device__ __forceinline__ int jl_ld(const JSinvSys& Y, int C) { return C < Y.Tb ? Y.ld : Y.ldb; }

// X[c][r] = (L_kk^-1)[r][c] (as cov_kernels.hip's linv_block)
__device__ void jlinv_block(double (*X)[NB + 1], const double* __restrict__ Ldk, const double* __restrict__ Wk) {
  const int tid = threadIdx.x;
  for (int e = tid; e < NB * NB; e += 256) X[e >> 6][e & 63] = (e >> 6) == (e & 63) ? 1.0 : 0.0;
  __syncthreads();
  const int c = tid & 63, rq = tid >> 6;
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
    for (int e = tid; e < NB * nr; e += 256) {
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

// blockIdx.x = job (system, column) of the whole table; blockIdx.y = 0: Sigma_cc <- L_cc^-T D_c L_cc^-1; y = b > 0: Z(rows[b - 1], c).
__global__ __launch_bounds__(256) void k_jsinv_prep(const JSinvSys* __restrict__ sys, const int2* __restrict__ jobs, const int* __restrict__ rp,
                                                    const int* __restrict__ rows) {
  const int2 jb = jobs[blockIdx.x];
  const JSinvSys Y = sys[jb.x];
  const int k = jb.y, base = Y.col0 + k;
  const int r0 = rp[base], nr = rp[base + 1] - r0;
  const int b = blockIdx.y;
  if (b > nr) return;
  __shared__ double X[NB][NB + 1];
  const bool hi = k >= Y.Tb;
  jlinv_block(X, (hi ? Y.Ld2 + (size_t)(k - Y.Tb) * NB * NB : Y.Ld + (size_t)k * NB * NB),
              (hi ? Y.Winv2 + (size_t)(k - Y.Tb) * 1024 : Y.Winv + (size_t)k * 1024));
  const int tid = threadIdx.x;
  if (b == 0) {
    const double sg = k >= Y.neg0 ? -1.0 : 1.0;
    double* dst = Y.Sg + (size_t)k * NB * Y.lds + (size_t)k * NB;
    for (int e = tid; e < NB * NB; e += 256) {
      const int bb = e >> 6, a = e & 63;
      double s = 0.0;
      for (int r = (a > bb ? a : bb); r < NB; ++r) s += X[a][r] * X[bb][r];
      dst[(size_t)bb * Y.lds + a] = sg * s;
    }
    return;
  }
  const int i = rows[r0 + b - 1];
  const double* L = jl_tile(Y, i, k);
  const int ldl = jl_ld(Y, k);
  double* Zt = Y.Z + (size_t)k * NB * Y.lds + (size_t)i * NB;
  for (int e = tid; e < NB * NB; e += 256) {
    const int c = e >> 6, row = e & 63;
    double s = 0.0;
    for (int q = c; q < NB; ++q) s += L[(size_t)q * ldl + row] * X[c][q];
    Zt[(size_t)c * Y.lds + row] = s;
  }
}

// One step of the backward recursion: blockIdx.y = job of this step (system, column k), blockIdx.x = index of the output row.
// DIAG = false: Sigma(i, k) = - sum_{j in I} Sigma(i, j) Z(j, k) for i = I[blockIdx.x].  DIAG = true: Sigma(k, k) -= sum_{j in I}
// Sigma(j, k)^T Z(j, k), then symmetrised.  Four waves, a 32x32 quadrant each; the operand tiles of one K step in LDS as [k][row / col].
template <bool DIAG>
__global__ __launch_bounds__(256) void k_jsinv_tile(const JSinvSys* __restrict__ sys, const int2* __restrict__ jobs, const int* __restrict__ rp,
                                                    const int* __restrict__ rows) {
  __shared__ double As[NB][NB + 1];
  __shared__ double Bs[NB][NB + 1];
  const int2 jb = jobs[blockIdx.y];
  const JSinvSys Y = sys[jb.x];
  const int k = jb.y, base = Y.col0 + k;
  const int r0 = rp[base], nr = rp[base + 1] - r0;
  if (nr == 0 || (!DIAG && (int)blockIdx.x >= nr)) return;
  const size_t lds = Y.lds;
  double* __restrict__ Sg = Y.Sg;
  const double* __restrict__ Z = Y.Z;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int lr = lane & 15, lk = lane >> 4, rh = w & 1, ch = w >> 1;
  const int i = DIAG ? k : rows[r0 + blockIdx.x];
  v4d acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) acc[a][b] = v4d{0.0, 0.0, 0.0, 0.0};
#pragma unroll 1
  for (int q = 0; q < nr; ++q) {
    const int j = rows[r0 + q];
    if (DIAG) {            // A[r][q] = Sigma(j, k)[q][r]
      const double* src = Sg + (size_t)(k * NB) * lds + (size_t)j * NB;
      for (int e = tid; e < NB * NB; e += 256) { const int r = e >> 6, qq = e & 63; As[qq][r] = src[(size_t)r * lds + qq]; }
    } else if (j <= i) {   // A[r][q] = Sigma(i, j)[r][q]
      const double* src = Sg + (size_t)(j * NB) * lds + (size_t)i * NB;
      for (int e = tid; e < NB * NB; e += 256) { const int qq = e >> 6, r = e & 63; As[qq][r] = src[(size_t)qq * lds + r]; }
    } else {               // A[r][q] = Sigma(j, i)[q][r]
      const double* src = Sg + (size_t)(i * NB) * lds + (size_t)j * NB;
      for (int e = tid; e < NB * NB; e += 256) { const int r = e >> 6, qq = e & 63; As[qq][r] = src[(size_t)r * lds + qq]; }
    }
    {                      // B[q][c] = Z(j, k)[q][c]
      const double* src = Z + (size_t)(k * NB) * lds + (size_t)j * NB;
      for (int e = tid; e < NB * NB; e += 256) { const int c = e >> 6, qq = e & 63; Bs[qq][c] = src[(size_t)c * lds + qq]; }
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
    double* dst = Sg + (size_t)(k * NB) * lds + (size_t)i * NB;
#pragma unroll
    for (int ra = 0; ra < 2; ++ra)
#pragma unroll
      for (int cb = 0; cb < 2; ++cb)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int row = 32 * rh + 16 * ra + lk + 4 * g, col = 32 * ch + 16 * cb + lr;
          dst[(size_t)col * lds + row] = -acc[ra][cb][g];
        }
    return;
  }
  double* dst = Sg + (size_t)(k * NB) * lds + (size_t)k * NB;
#pragma unroll
  for (int ra = 0; ra < 2; ++ra)
#pragma unroll
    for (int cb = 0; cb < 2; ++cb)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int row = 32 * rh + 16 * ra + lk + 4 * g, col = 32 * ch + 16 * cb + lr;
        As[row][col] = dst[(size_t)col * lds + row] - acc[ra][cb][g];
      }
  __syncthreads();
  for (int e = tid; e < NB * NB; e += 256) {
    const int col = e >> 6, row = e & 63;
    dst[(size_t)col * lds + row] = 0.5 * (As[row][col] + As[col][row]);
  }
}

void launch_jsinv_prep(const JSinvSys* d_sys, const int2* d_jobs, int njobs, int max_rows, const int* d_rp, const int* d_rows, hipStream_t s) {
  if (njobs > 0) hipLaunchKernelGGL(k_jsinv_prep, dim3(njobs, max_rows + 1), dim3(256), 0, s, d_sys, d_jobs, d_rp, d_rows);
}
void launch_jsinv_step(const JSinvSys* d_sys, const int2* d_jobs, int njobs, int max_rows, const int* d_rp, const int* d_rows, hipStream_t s) {
  if (njobs <= 0 || max_rows <= 0) return;
  hipLaunchKernelGGL((k_jsinv_tile<false>), dim3(max_rows, njobs), dim3(256), 0, s, d_sys, d_jobs, d_rp, d_rows);
  hipLaunchKernelGGL((k_jsinv_tile<true>), dim3(1, njobs), dim3(256), 0, s, d_sys, d_jobs, d_rp, d_rows);
}

// Sigma of a robot's rows past its factor columns (its shared landmarks' and lambda coordinates) from the separator's Sigma:
// dst(o0 + a, o0 + b) = Sigma_sep(map[a], map[b]), a, b < n (both halves); map[a] < 0 (padding of the last border tile): 0.
// blockIdx.z = robot, blockIdx.y = column b.
__global__ __launch_bounds__(256) void k_jsig_gather(JSigGather A) {
  const int r = blockIdx.z, b = blockIdx.y;
  const int n = A.n[r];
  if (b >= n) return;
  const int* map = A.map[r];
  const int mb = map[b];
  const double* src = A.src;
  double* dst = A.dst[r] + (size_t)(A.o0[r] + b) * A.lds[r] + A.o0[r];
  for (int a = blockIdx.x * 256 + threadIdx.x; a < n; a += 256 * gridDim.x) {
    const int ma = map[a];
    double v = 0.0;
    if (ma >= 0 && mb >= 0) v = ma >= mb ? src[(size_t)mb * A.lds_src + ma] : src[(size_t)ma * A.lds_src + mb];
    dst[a] = v;
  }
}
void launch_jsig_gather(const JSigGather& A, int n_robots, int max_n, hipStream_t s) {
  if (n_robots > 0 && max_n > 0) hipLaunchKernelGGL(k_jsig_gather, dim3((max_n + 255) / 256, max_n, n_robots), dim3(256), 0, s, A);
}

// d x d diagonal blocks of a Sigma (dense lower, leading dimension ld) at the rows row0[q]: out[81 q + d a + b]
__global__ void k_sym_blocks(const double* __restrict__ Sg, size_t ld, const int* __restrict__ row0, const int* __restrict__ dim, int n,
                             double* __restrict__ out) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= 81 * n) return;
  const int q = e / 81, ab = e % 81, d = dim[q];
  const int a = ab / d, b = ab % d;
  if (a >= d) return;
  const int R = row0[q] + a, C = row0[q] + b;
  out[81 * (size_t)q + ab] = R >= C ? Sg[(size_t)C * ld + R] : Sg[(size_t)R * ld + C];
}
void launch_sym_blocks(const double* Sg, size_t ld, const int* row0, const int* dim, int n, double* out, hipStream_t s) {
  if (n > 0) hipLaunchKernelGGL(k_sym_blocks, dim3((81 * n + 255) / 256), dim3(256), 0, s, Sg, ld, row0, dim, n, out);
}

// ---- many right-hand sides over the same elimination tree: X = K^-1 B, K = L D L^T the joint factor (CholBatch::joint_closure_info_gain)
// Two buffers per system, both with the rows of its Sigma (column c, row r at c * lds + r): the working right-hand sides R (JSinvSys::Z;
// B to start with) and the solutions S (JSinvSys::Sg: L^-1 B after the forward sweep, X after the backward one).  A column's solve reads
// R and writes S, so no workgroup of a launch overwrites what another one of the same job still reads.  The nodes of the tree are the band
// segments, the windows, the robots' rows of separator coordinates (no columns), the separator's leaves, then its top block with the
// lambda block.  Inside a node the columns run one per launch ("push": the workgroups of a job each redo the 64 x 16 triangular solve of
// the column and one of them stores it, the others apply it to one row of the node each), so no row is written by two workgroups of a
// launch; a node's rows from the nodes below it are summed once before its columns start ("pull", forward) and a node's columns take
// the finished rows above it once before they start (backward) — the two leaves, every segment and every robot side by side.  No
// floating-point atomics: every sum runs in one workgroup in a fixed order.  blockIdx.y = chunk of 16 right-hand sides.
namespace {
// the diagonal block of column k: L_kk (ld NB) and its four 16 x 16 diagonal inverses
__device__ __forceinline__ const double* jm_ld(const JSinvSys& Y, int k) {
  return k < Y.Tb ? Y.Ld + (size_t)k * NB * NB : Y.Ld2 + (size_t)(k - Y.Tb) * NB * NB;
}
__device__ __forceinline__ const double* jm_winv(const JSinvSys& Y, int k) {
  return k < Y.Tb ? Y.Winv + (size_t)k * 1024 : Y.Winv2 + (size_t)(k - Y.Tb) * 1024;
}
// x[c] <- L_kk^-1 t[c], t consumed (16 columns in LDS; cov_kernels.hip's k_sub_fwd)
__device__ void jm_lsolve(double (*t)[NB], double (*x)[NB], const double* __restrict__ Ldk, const double* __restrict__ Wk) {
  const int tid = threadIdx.x, c = tid >> 4, r = tid & 15;
#pragma unroll 1
  for (int b = 0; b < 4; ++b) {
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < 16; ++j) s += Wk[(size_t)b * 256 + j * 16 + r] * t[c][16 * b + j];
    x[c][16 * b + r] = s;
    __syncthreads();
    for (int e = tid; e < 16 * 16 * (3 - b); e += 256) {
      const int cc = e / (16 * (3 - b)), m = 16 * (b + 1) + e % (16 * (3 - b));
      double u = 0.0;
#pragma unroll
      for (int n = 0; n < 16; ++n) u += Ldk[(size_t)(16 * b + n) * NB + m] * x[cc][16 * b + n];
      t[cc][m] -= u;
    }
    __syncthreads();
  }
}
// t[c] <- L_kk^-T t[c] in place (cov_kernels.hip's k_sub_bwd)
__device__ void jm_ltsolve(double (*t)[NB], const double* __restrict__ Ldk, const double* __restrict__ Wk) {
  const int tid = threadIdx.x, c = tid >> 4, r = tid & 15;
#pragma unroll 1
  for (int b = 3; b >= 0; --b) {
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < 16; ++j) s += Wk[(size_t)b * 256 + r * 16 + j] * t[c][16 * b + j];
    __syncthreads();
    t[c][16 * b + r] = s;
    __syncthreads();
    for (int e = tid; e < 16 * 16 * b; e += 256) {
      const int cc = e / (16 * b), n = e % (16 * b);
      double u = 0.0;
#pragma unroll
      for (int m = 0; m < 16; ++m) u += Ldk[(size_t)n * NB + 16 * b + m] * t[cc][16 * b + m];
      t[cc][n] -= u;
    }
    __syncthreads();
  }
}
__device__ __forceinline__ void jm_load(double (*t)[NB], const double* X, long long ld, int tile, int c0, int nc) {
  for (int e = threadIdx.x; e < 16 * NB; e += 256) {
    const int cc = e / NB, r = e % NB;
    t[cc][r] = cc < nc ? X[(size_t)(c0 + cc) * ld + (size_t)tile * NB + r] : 0.0;
  }
}
__device__ __forceinline__ void jm_store(double (*t)[NB], double* X, long long ld, int tile, int c0, int nc) {
  for (int e = threadIdx.x; e < nc * NB; e += 256) X[(size_t)(c0 + e / NB) * ld + (size_t)tile * NB + e % NB] = t[e / NB][e % NB];
}
// acc[cc][row] -= sum_q A[row][q] x[cc][q] for the tile A = L (TR = false: rows i, column k; A[row][q] = L[q ld + row]) or L^T
// (TR = true: A[m][row] = L[m ld + row], staged through LDS so that the global reads stay coalesced)
template <bool TR>
__device__ void jm_tile_sub(double (*acc)[NB], const double* __restrict__ L, int ldl, double (*x)[NB], double (*Lt)[NB + 1], int nc) {
  const int tid = threadIdx.x;
  if (TR) {
    for (int e = tid; e < NB * NB; e += 256) { const int m = e >> 6, row = e & 63; Lt[m][row] = L[(size_t)m * ldl + row]; }
    __syncthreads();
    for (int e = tid; e < nc * NB; e += 256) {
      const int cc = e / NB, m = e % NB;
      double s = 0.0;
#pragma unroll 8
      for (int row = 0; row < NB; ++row) s += Lt[m][row] * x[cc][row];
      acc[cc][m] -= s;
    }
  } else {
    for (int e = tid; e < nc * NB; e += 256) {
      const int cc = e / NB, row = e % NB;
      double s = 0.0;
#pragma unroll 8
      for (int q = 0; q < NB; ++q) s += L[(size_t)q * ldl + row] * x[cc][q];
      acc[cc][row] -= s;
    }
  }
  __syncthreads();
}
}  // namespace

// Push: job = {system, column k, list begin, list end}; blockIdx.x = 0 stores x_k into S, blockIdx.x = b > 0 updates the b-th entry of
// the list in R.  Forward (BWD = false): x_k = L_kk^-1 R_k, then R_i -= L_ik x_k for the rows i of k's node.  Backward:
// x_k = L_kk^-T R_k, then R_j -= L_kj^T x_k for the columns j of k's node whose rows hold k.
template <bool BWD>
__global__ __launch_bounds__(256) void k_jms_push(const JSinvSys* __restrict__ sys, const int4* __restrict__ jobs, const int* __restrict__ list,
                                                  int ncol) {
  __shared__ double t[16][NB];
  __shared__ double x[16][NB];
  __shared__ double Lt[BWD ? NB : 1][NB + 1];
  const int4 jb = jobs[blockIdx.z];
  const int b = blockIdx.x;
  if (b > jb.w - jb.z) return;
  const JSinvSys Y = sys[jb.x];
  const int k = jb.y, c0 = 16 * (int)blockIdx.y;
  const int nc = ncol - c0 < 16 ? ncol - c0 : 16;
  jm_load(t, Y.Z, Y.lds, k, c0, nc);
  __syncthreads();
  if (BWD) jm_ltsolve(t, jm_ld(Y, k), jm_winv(Y, k));
  else jm_lsolve(t, x, jm_ld(Y, k), jm_winv(Y, k));
  double (*xk)[NB] = BWD ? t : x;
  if (b == 0) { jm_store(xk, Y.Sg, Y.lds, k, c0, nc); return; }
  const int j = list[jb.z + b - 1];
  double (*acc)[NB] = BWD ? x : t;      // (the target's rows, in the buffer the solve no longer needs)
  jm_load(acc, Y.Z, Y.lds, j, c0, nc);
  __syncthreads();
  if (BWD) jm_tile_sub<true>(acc, jl_tile(Y, k, j), jl_ld(Y, j), xk, Lt, nc);
  else jm_tile_sub<false>(acc, jl_tile(Y, j, k), jl_ld(Y, k), xk, Lt, nc);
  jm_store(acc, Y.Z, Y.lds, j, c0, nc);
}

// Pull: job = {system, tile k, list begin, list end}.  Forward: R_k -= sum_j L_kj S_j over the columns j of the nodes below k's.
// Backward: R_k = D_k S_k - sum_i L_ik^T S_i over the rows i of the nodes above k's (D_k = -I on the lambda block: the D step).
template <bool BWD>
__global__ __launch_bounds__(256) void k_jms_pull(const JSinvSys* __restrict__ sys, const int4* __restrict__ jobs, const int* __restrict__ list,
                                                  int ncol) {
  __shared__ double t[16][NB];
  __shared__ double x[16][NB];
  __shared__ double Lt[BWD ? NB : 1][NB + 1];
  const int4 jb = jobs[blockIdx.z];
  const JSinvSys Y = sys[jb.x];
  const int k = jb.y, c0 = 16 * (int)blockIdx.y;
  const int nc = ncol - c0 < 16 ? ncol - c0 : 16;
  jm_load(t, BWD ? Y.Sg : Y.Z, Y.lds, k, c0, nc);
  if (BWD && k >= Y.neg0)
    for (int e = threadIdx.x; e < 16 * NB; e += 256) t[e / NB][e % NB] = -t[e / NB][e % NB];
  __syncthreads();
#pragma unroll 1
  for (int q = jb.z; q < jb.w; ++q) {
    const int j = list[q];
    jm_load(x, Y.Sg, Y.lds, j, c0, nc);
    __syncthreads();
    if (BWD) jm_tile_sub<true>(t, jl_tile(Y, j, k), jl_ld(Y, k), x, Lt, nc);
    else jm_tile_sub<false>(t, jl_tile(Y, k, j), jl_ld(Y, j), x, Lt, nc);
  }
  jm_store(t, Y.Z, Y.lds, k, c0, nc);
}

void launch_jms_push(const JSinvSys* d_sys, const int4* d_jobs, int njobs, int max_list, const int* d_list, int ncol, bool bwd, hipStream_t s) {
  if (njobs <= 0 || ncol <= 0) return;
  const dim3 g(max_list + 1, (ncol + 15) / 16, njobs);
  if (bwd) hipLaunchKernelGGL((k_jms_push<true>), g, dim3(256), 0, s, d_sys, d_jobs, d_list, ncol);
  else hipLaunchKernelGGL((k_jms_push<false>), g, dim3(256), 0, s, d_sys, d_jobs, d_list, ncol);
}
void launch_jms_pull(const JSinvSys* d_sys, const int4* d_jobs, int njobs, const int* d_list, int ncol, bool bwd, hipStream_t s) {
  if (njobs <= 0 || ncol <= 0) return;
  const dim3 g(1, (ncol + 15) / 16, njobs);
  if (bwd) hipLaunchKernelGGL((k_jms_pull<true>), g, dim3(256), 0, s, d_sys, d_jobs, d_list, ncol);
  else hipLaunchKernelGGL((k_jms_pull<false>), g, dim3(256), 0, s, d_sys, d_jobs, d_list, ncol);
}

// The separator's right-hand side (R) from the robots' rows of separator coordinates (R): dst[row] = sum over ent[ptr[row] .. ptr[row + 1])
// = (robot, its row), in robot order (the inverse of the border maps; rows nobody maps get 0).  blockIdx.y = right-hand side.
__global__ __launch_bounds__(256) void k_jms_sum(JMSum A, const int* __restrict__ ptr, const int2* __restrict__ ent, int nrows) {
  const int row = blockIdx.x * 256 + threadIdx.x, c = blockIdx.y;
  if (row >= nrows) return;
  double s = 0.0;
  for (int q = ptr[row]; q < ptr[row + 1]; ++q) {
    const int2 e = ent[q];
    s += A.src[e.x][(size_t)c * A.ld + e.y];
  }
  A.dst[(size_t)c * A.ld + row] = s;
}
void launch_jms_sum(const JMSum& A, const int* d_ptr, const int2* d_ent, int nrows, int ncol, hipStream_t s) {
  if (nrows > 0 && ncol > 0) hipLaunchKernelGGL(k_jms_sum, dim3((nrows + 255) / 256, ncol), dim3(256), 0, s, A, d_ptr, d_ent, nrows);
}

// The separator's solution (S) back into every robot's rows of separator coordinates (S; the vector form of k_jsig_gather):
// dst[r][o0 + a] = src[map[r][a]] (0 for padding), a < n[r]; blockIdx.y = right-hand side, blockIdx.z = robot.
__global__ __launch_bounds__(256) void k_jms_gather(JSigGather A) {
  const int r = blockIdx.z, c = blockIdx.y, a = blockIdx.x * 256 + threadIdx.x;
  if (a >= A.n[r]) return;
  const int ma = A.map[r][a];
  A.dst[r][(size_t)c * A.lds[r] + A.o0[r] + a] = ma >= 0 ? A.src[(size_t)c * A.lds_src + ma] : 0.0;
}
void launch_jms_gather(const JSigGather& A, int n_robots, int max_n, int ncol, hipStream_t s) {
  if (n_robots > 0 && max_n > 0 && ncol > 0) hipLaunchKernelGGL(k_jms_gather, dim3((max_n + 255) / 256, ncol, n_robots), dim3(256), 0, s, A);
}

}  // namespace sl
