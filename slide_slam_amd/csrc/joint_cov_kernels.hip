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

}  // namespace sl
