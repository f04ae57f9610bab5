// Inter-robot map-to-map association kernels.
//   SlideMatch sweep: PlaceRecognition::MatchMaps (backend/sloam/src/core/place_recognition.cpp:98-387) —
//   the exhaustive (x, y, yaw) lattice of label-gated inlier counting.  One wavefront per candidate
//   transform; lanes own query objects and scan the reference map (staged in LDS, every lane reads the
//   same entry -> LDS broadcast) in order with the reference's first-hit break; the lattice is
//   produced on the host by the reference's own repeated-addition loops so every candidate value is
//   bit-identical.  FP64 vector ALU / LDS bound: the maps are a few KB, HBM traffic is negligible.
//   CLIPPER affinity: CLIPPER::scorePairwiseConsistency (clipper_semantic_object/src/clipper.cpp:21-65).
// Compiled with -ffp-contract=off (threshold comparisons must round like the reference's x86-64 build).
#include <hip/hip_runtime.h>

#include "kernels.hpp"

namespace sl {

// LDS image: ref objects as 6 doubles [label, x, y, d1, d2, d3]
__global__ __launch_bounds__(256) void k_place_sweep(PlaceDev P, const double* __restrict__ cosv, const double* __restrict__ sinv) {
  extern __shared__ double ref[];
  for (int e = threadIdx.x; e < P.nr * 6; e += blockDim.x) {
    const int k = e / 6, f = e % 6;
    const int src = f == 0 ? 0 : (f <= 2 ? f : f + 1);   // label, x, y, (skip z), d1, d2, d3
    ref[e] = P.ref7[7 * (size_t)k + src];
  }
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const long long wave = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const long long nwaves = ((long long)gridDim.x * blockDim.x) >> 6;
  const long long ncand = P.n_cells * P.n_yaw;
  for (long long cand = wave; cand < ncand; cand += nwaves) {
    const long long cell = cand / P.n_yaw;
    const int iy = (int)(cand % P.n_yaw);
    const double x = P.xs[P.cell_x[cell]], y = P.ys[P.cell_y[cell]];
    const double c = cosv[iy], s = sinv[iy];
    int inl = 0;
    for (int j = lane; j < P.nq; j += 64) {
      const double* q = P.qry7 + 7 * (size_t)j;
      const double ql = q[0];
      double tx = c * q[1] + (-s) * q[2] + x * 1.0;
      double ty = s * q[1] + c * q[2] + y * 1.0;
      const double tw = 0.0 * q[1] + 0.0 * q[2] + 1.0 * 1.0;
      tx = tx / tw; ty = ty / tw;
      for (int k = 0; k < P.nr; ++k) {
        const double* m = ref + 6 * k;
        if (m[0] != ql) continue;
        const double xd = m[1] - tx, yd = m[2] - ty;
        double avg = 0;
        if (m[4] == 0 && m[5] == 0) {
          avg = fabs(m[3] - q[4]);
        } else {
          avg += fabs(m[3] - q[4]);
          avg += fabs(m[4] - q[5]);
          avg += fabs(m[5] - q[6]);
          avg /= 3;
        }
        const bool dist_ok = sqrt(xd * xd + yd * yd) < P.thr_pos;
        const bool dim_ok = P.ignore_dim ? true : (avg < P.thr_dim);
        if (dist_ok && dim_ok) { ++inl; break; }
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) inl += __shfl_xor(inl, off);
    if (lane == 0) P.inliers[cand] = inl;
  }
}

// Round 5: the same count with both maps BUCKETED BY LABEL.  The reference scans, for every query object, the reference objects in
// order, skips those of another label and stops at the first hit (place_recognition.cpp:281-357): a stable bucketing keeps "the first
// hit among the objects of my label" what it was, and the inlier COUNT does not depend on the order of the query objects — so the host
// sorts both maps by label (stably), and a wavefront scans, per chunk of 64 query objects, only the bucket(s) its lanes ask for: no label
// test, a third of the pairs at three labels, LDS broadcast reads ((x, y) as one 16-byte entry), and the distance test
// sqrt(dx^2 + dy^2) < t as dx^2 + dy^2 < v_crit with v_crit = the smallest double whose correctly rounded root is >= t (the same
// decision bit for bit: sqrt is monotone and correctly rounded on both sides) — the f64 square root was most of a pair test's cost.
// Query objects live in LDS too (lane-contiguous), every candidate re-uses them.
// The bucketed LDS image of one pair of maps and the count of ONE candidate on it: THE one text k_place_sweep_b and k_place_sweep_seg
// evaluate (this source is compiled with -ffp-contract=off, and the count is an integer: the same value in both).
struct PlaceLds { const double* rxy; const double* rdim; const double* qxy; const double* qdim; const int* qrange; };
__device__ __forceinline__ PlaceLds place_stage_b(const PlaceDev& P, double* lds) {
  double* rxy = lds;                                   // 2 nr
  double* rdim = rxy + 2 * (size_t)P.nr;               // 3 nr (only when !ignore_dim)
  double* qxy = rdim + (P.ignore_dim ? 0 : 3 * (size_t)P.nr);      // 2 nq
  double* qdim = qxy + 2 * (size_t)P.nq;               // 3 nq (only when !ignore_dim)
  int* qrange = reinterpret_cast<int*>(qdim + (P.ignore_dim ? 0 : 3 * (size_t)P.nq));   // 2 nq
  for (int e = threadIdx.x; e < 2 * P.nr; e += blockDim.x) rxy[e] = P.rxy[e];
  for (int e = threadIdx.x; e < 2 * P.nq; e += blockDim.x) { qxy[e] = P.qxy[e]; qrange[e] = P.qrange[e]; }
  if (!P.ignore_dim) {
    for (int e = threadIdx.x; e < 3 * P.nr; e += blockDim.x) rdim[e] = P.rdim[e];
    for (int e = threadIdx.x; e < 3 * P.nq; e += blockDim.x) qdim[e] = P.qdim[e];
  }
  __syncthreads();
  return PlaceLds{rxy, rdim, qxy, qdim, qrange};
}
// inliers of the candidate (x, y, c = cos yaw, s = sin yaw), summed over the wavefront: every lane returns the count
__device__ __forceinline__ int place_count_b(const PlaceLds& L, int nq, double x, double y, double c, double s, double v_crit, double thr_dim,
                                             bool use_dim, int lane) {
  const double* rxy = L.rxy; const double* rdim = L.rdim; const double* qxy = L.qxy; const double* qdim = L.qdim; const int* qrange = L.qrange;
  int inl = 0;
  for (int j0 = 0; j0 < nq; j0 += 64) {
    const int j = j0 + lane;
    const bool active = j < nq;
    double tx = 0.0, ty = 0.0, q4 = 0.0, q5 = 0.0, q6 = 0.0;
    int lo = 0, hi = 0;
    if (active) {
      const double q1 = qxy[2 * j], q2 = qxy[2 * j + 1];
      tx = c * q1 + (-s) * q2 + x * 1.0;
      ty = s * q1 + c * q2 + y * 1.0;
      const double tw = 0.0 * q1 + 0.0 * q2 + 1.0 * 1.0;
      tx = tx / tw; ty = ty / tw;
      lo = qrange[2 * j]; hi = qrange[2 * j + 1];
      if (use_dim) { q4 = qdim[3 * j]; q5 = qdim[3 * j + 1]; q6 = qdim[3 * j + 2]; }
    }
    bool hit = false;
    unsigned long long todo = __ballot(active && hi > lo);
    while (todo) {      // one bucket per chunk (the query objects are sorted by label), two or three where labels meet
      const int first = __ffsll((long long)todo) - 1;
      const int blo = __shfl(lo, first), bhi = __shfl(hi, first);
      const bool mine = active && lo == blo && hi == bhi;
      bool open_ = mine;                                  // still looking for its first hit
      int k = blo;
      if (!use_dim) {
        // four reference objects per round: whether a query object has A hit does not depend on the order inside the bucket, and
        // four independent distance tests hide each other's latencies (one test is a chain of five dependent f64 operations
        // behind an LDS read: 128 cycles per object and wavefront when taken one by one)
        for (; k + 4 <= bhi; k += 4) {
          if (((k - blo) & 15) == 0 && __ballot(open_) == 0) { k = bhi; break; }
          const double x0 = rxy[2 * k] - tx, y0 = rxy[2 * k + 1] - ty, x1 = rxy[2 * k + 2] - tx, y1 = rxy[2 * k + 3] - ty;
          const double x2 = rxy[2 * k + 4] - tx, y2 = rxy[2 * k + 5] - ty, x3 = rxy[2 * k + 6] - tx, y3 = rxy[2 * k + 7] - ty;
          const bool ok = (x0 * x0 + y0 * y0 < v_crit) | (x1 * x1 + y1 * y1 < v_crit) | (x2 * x2 + y2 * y2 < v_crit) | (x3 * x3 + y3 * y3 < v_crit);
          if (open_ && ok) { hit = true; open_ = false; }
        }
      }
      for (; k < bhi; ++k) {
        if (((k - blo) & 15) == 0 && __ballot(open_) == 0) break;
        const double xd = rxy[2 * k] - tx, yd = rxy[2 * k + 1] - ty;
        bool ok = xd * xd + yd * yd < v_crit;
        if (use_dim) {
          const double m3 = rdim[3 * k], m4 = rdim[3 * k + 1], m5 = rdim[3 * k + 2];
          double avg = 0;
          if (m4 == 0 && m5 == 0) {
            avg = fabs(m3 - q4);
          } else {
            avg += fabs(m3 - q4);
            avg += fabs(m4 - q5);
            avg += fabs(m5 - q6);
            avg /= 3;
          }
          ok = ok && (avg < thr_dim);
        }
        if (open_ && ok) { hit = true; open_ = false; }
      }
      todo &= ~__ballot(mine);
    }
    inl += hit ? 1 : 0;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) inl += __shfl_xor(inl, off);
  return inl;
}
__global__ __launch_bounds__(256) void k_place_sweep_b(PlaceDev P, const double* __restrict__ cosv, const double* __restrict__ sinv) {
  extern __shared__ __align__(16) double lds[];
  const PlaceLds L = place_stage_b(P, lds);
  const int lane = threadIdx.x & 63;
  const long long wave = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const long long nwaves = ((long long)gridDim.x * blockDim.x) >> 6;
  const long long ncand = P.n_cells * P.n_yaw;
  const double v_crit = P.v_crit, thr_dim = P.thr_dim;
  const bool use_dim = !P.ignore_dim;
  for (long long cand = wave; cand < ncand; cand += nwaves) {
    const long long cell = cand / P.n_yaw;
    const int iy = (int)(cand % P.n_yaw);
    const double x = P.xs[P.cell_x[cell]], y = P.ys[P.cell_y[cell]];
    const double c = cosv[iy], s = sinv[iy];
    const int inl = place_count_b(L, P.nq, x, y, c, s, v_crit, thr_dim, use_dim, lane);
    if (lane == 0) P.inliers[cand] = inl;
  }
}

// The sweep of a LIST of map pairs in one launch (slide_find_inter_loop_closures: the robot pairs of sloamNode.cpp:600-694).  segs: one
// PlaceDev per live pair (bucketed tables and lattice in one arena); wgs: per workgroup {pair, rank within the pair, workgroups of the
// pair}, built on the host with shares in proportion to candidates x distance tests.  A workgroup stages ITS pair's image and its four
// waves stride that pair's candidates in ascending order, so a candidate's count is k_place_sweep_b's for that pair alone.  No count is
// stored per candidate: a wave keeps (best count, first index) with strict `>`, the workgroup reduces its four waves (the smaller index
// wins on equal counts) and writes one partial.  The same FP64 VALU / LDS bound as k_place_sweep_b; the dynamic LDS is the largest live
// pair's image, so an image above 80 KiB leaves one workgroup per CU.
__global__ __launch_bounds__(256) void k_place_sweep_seg(const PlaceDev* __restrict__ segs, const PlaceWg* __restrict__ wgs,
                                                         PlaceBest* __restrict__ part) {
  extern __shared__ __align__(16) double lds[];
  __shared__ long long widx[4];
  __shared__ int wval[4];
  const PlaceWg W = wgs[blockIdx.x];
  const PlaceDev P = segs[W.pair];
  const PlaceLds L = place_stage_b(P, lds);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const long long ncand = P.n_cells * P.n_yaw, nwaves = 4LL * W.n;
  const double* cosv = P.yaws + P.n_yaw;
  const double* sinv = P.yaws + 2 * (size_t)P.n_yaw;
  const double v_crit = P.v_crit, thr_dim = P.thr_dim;
  const bool use_dim = !P.ignore_dim;
  int bv = INT32_MIN;
  long long bi = -1;
  for (long long cand = 4LL * W.rank + wv; cand < ncand; cand += nwaves) {
    const long long cell = cand / P.n_yaw;
    const int iy = (int)(cand % P.n_yaw);
    const double x = P.xs[P.cell_x[cell]], y = P.ys[P.cell_y[cell]];
    const double c = cosv[iy], s = sinv[iy];
    const int inl = place_count_b(L, P.nq, x, y, c, s, v_crit, thr_dim, use_dim, lane);
    if (inl > bv) { bv = inl; bi = cand; }
  }
  if (lane == 0) { wval[wv] = bv; widx[wv] = bi; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; ++w)
      if (widx[w] >= 0 && (wval[w] > bv || (wval[w] == bv && (bi < 0 || widx[w] < bi)))) { bv = wval[w]; bi = widx[w]; }
    part[blockIdx.x] = PlaceBest{bi, bv, 0};
  }
}
// per pair: its workgroups' partials [wg0[s], wg0[s + 1]) reduced by the same rule (larger count, then smaller index)
__global__ __launch_bounds__(256) void k_place_best_seg(const PlaceBest* __restrict__ part, const int* __restrict__ wg0, PlaceBest* __restrict__ best) {
  __shared__ long long sidx[256];
  __shared__ int sval[256];
  const int s = blockIdx.x;
  int bv = INT32_MIN;
  long long bi = -1;
  for (int i = wg0[s] + (int)threadIdx.x; i < wg0[s + 1]; i += 256) {
    const PlaceBest b = part[i];
    if (b.idx >= 0 && (b.val > bv || (b.val == bv && (bi < 0 || b.idx < bi)))) { bv = b.val; bi = b.idx; }
  }
  sval[threadIdx.x] = bv;
  sidx[threadIdx.x] = bi;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if (threadIdx.x < st) {
      const int ov = sval[threadIdx.x + st];
      const long long oi = sidx[threadIdx.x + st];
      if (oi >= 0 && (ov > sval[threadIdx.x] || (ov == sval[threadIdx.x] && (sidx[threadIdx.x] < 0 || oi < sidx[threadIdx.x])))) {
        sval[threadIdx.x] = ov;
        sidx[threadIdx.x] = oi;
      }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) best[s] = PlaceBest{sidx[0], sval[0], 0};
}

// first index of the maximum (the reference keeps a candidate only when it has STRICTLY more inliers)
__global__ __launch_bounds__(256) void k_place_argmax(const int32_t* __restrict__ v, long long n, long long* best_idx,
                                                      int32_t* best_val) {
  __shared__ long long sidx[256];
  __shared__ int sval[256];
  int bv = INT32_MIN;
  long long bi = -1;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const int x = v[i];
    if (x > bv) { bv = x; bi = i; }
  }
  sval[threadIdx.x] = bv;
  sidx[threadIdx.x] = bi;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if (threadIdx.x < st) {
      const int ov = sval[threadIdx.x + st];
      const long long oi = sidx[threadIdx.x + st];
      if (oi >= 0 && (ov > sval[threadIdx.x] || (ov == sval[threadIdx.x] && (sidx[threadIdx.x] < 0 || oi < sidx[threadIdx.x])))) {
        sval[threadIdx.x] = ov;
        sidx[threadIdx.x] = oi;
      }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) { best_idx[blockIdx.x] = sidx[0]; best_val[blockIdx.x] = sval[0]; }
}

__global__ void k_clipper_affinity(const double* __restrict__ D1, const double* __restrict__ D2, int dim, const int32_t* __restrict__ A,
                                   int m, double sigma, double eps, double mindist, double affinityeps, double* __restrict__ M) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  const int i = blockIdx.y;
  if (j >= m || i >= m) return;
  double out = 0.0;
  if (j > i) {      // (i < j: the smaller index first, as k_affinity_csr calls it for both (i, j) and (j, i))
    const int i0 = A[2 * i], i1 = A[2 * i + 1], j0 = A[2 * j], j1 = A[2 * j + 1];
    out = clipper_pair_score<0>(i0, i1, j0, j1, D1 + (size_t)i0 * dim, D1 + (size_t)j0 * dim, D2 + (size_t)i1 * dim, D2 + (size_t)j1 * dim, dim,
                                sigma, eps, mindist, affinityeps);
  }
  M[(size_t)i * m + j] = out;
}

// ---- SlideGraph triangle matching (semantic_clipper.cpp:49-118) ------------------------------------------------------
// Per triangle: centroid, the three vertex-centroid distances, stable ascending argsort (the reference's std::sort on
// three indices is an insertion sort), vertices re-ordered accordingly.
__global__ void k_tri_prepare(const double* __restrict__ tri, int n, double* __restrict__ sdist, double* __restrict__ sxy) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const double* v = tri + 6 * (size_t)t;
  const double x0 = v[0], y0 = v[1], x1 = v[2], y1 = v[3], x2 = v[4], y2 = v[5];
  const double cx = (x0 + x1 + x2) / 3.0, cy = (y0 + y1 + y2) / 3.0;
  double d0 = sqrt((x0 - cx) * (x0 - cx) + (y0 - cy) * (y0 - cy));
  double d1 = sqrt((x1 - cx) * (x1 - cx) + (y1 - cy) * (y1 - cy));
  double d2 = sqrt((x2 - cx) * (x2 - cx) + (y2 - cy) * (y2 - cy));
  double ax = x0, ay = y0, bx = x1, by = y1, gx = x2, gy = y2;
  // insertion sort of (d0, d1, d2) with "<" (stable)
  if (d1 < d0) { double t0 = d0; d0 = d1; d1 = t0; t0 = ax; ax = bx; bx = t0; t0 = ay; ay = by; by = t0; }
  if (d2 < d1) {
    double t0 = d1; d1 = d2; d2 = t0; t0 = bx; bx = gx; gx = t0; t0 = by; by = gy; gy = t0;
    if (d1 < d0) { t0 = d0; d0 = d1; d1 = t0; t0 = ax; ax = bx; bx = t0; t0 = ay; ay = by; by = t0; }
  }
  sdist[3 * (size_t)t] = d0; sdist[3 * (size_t)t + 1] = d1; sdist[3 * (size_t)t + 2] = d2;
  double* o = sxy + 6 * (size_t)t;
  o[0] = ax; o[1] = ay; o[2] = bx; o[3] = by; o[4] = gx; o[5] = gy;
}
// compute_triangle_diff (semantic_clipper.cpp:49-66) of one (model, data) triangle pair from their sorted vertex-centroid distances:
// THE one text k_tri_match and k_tri_match_seg evaluate (this source is compiled with -ffp-contract=off: the same bits in both).
__device__ __forceinline__ double tri_pair_diff(double m0, double m1, double m2, const double* __restrict__ d3) {
  const double e0 = m0 - d3[0], e1 = m1 - d3[1], e2 = m2 - d3[2];
  double sacc = 0.0;
  sacc += e0 * e0; sacc += e1 * e1; sacc += e2 * e2;
  return sqrt(sacc);
}
// One wave per model triangle, lanes over the data triangles.  EMIT = false: counts[i] = matches of row i.
// EMIT = true: rows are written at offs[i] in data order (ballot ranks keep the reference's loop order).
template <bool EMIT>
__global__ __launch_bounds__(256) void k_tri_match(const double* __restrict__ dm, const double* __restrict__ xm, int ntm,
                                                   const double* __restrict__ dd, const double* __restrict__ xd, int ntd, double thr,
                                                   int* __restrict__ counts, const long long* __restrict__ offs,
                                                   double* __restrict__ pts, double* __restrict__ diffs) {
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= ntm) return;
  const double m0 = dm[3 * (size_t)i], m1 = dm[3 * (size_t)i + 1], m2 = dm[3 * (size_t)i + 2];
  long long base = EMIT ? offs[i] : 0;
  int cnt = 0;
  for (int j0 = 0; j0 < ntd; j0 += 64) {
    const int j = j0 + lane;
    bool hit = false;
    double diff = 0.0;
    if (j < ntd) {
      diff = tri_pair_diff(m0, m1, m2, dd + 3 * (size_t)j);
      hit = diff < thr;
    }
    const unsigned long long mask = __ballot(hit);
    if (EMIT && hit) {
      const long long row = base + __popcll(mask & ((1ull << lane) - 1ull));
      diffs[row] = diff;
      double* o = pts + 12 * row;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        o[4 * k] = xm[6 * (size_t)i + 2 * k]; o[4 * k + 1] = xm[6 * (size_t)i + 2 * k + 1];
        o[4 * k + 2] = xd[6 * (size_t)j + 2 * k]; o[4 * k + 3] = xd[6 * (size_t)j + 2 * k + 1];
      }
    }
    base += __popcll(mask);
    cnt += __popcll(mask);
  }
  if (!EMIT && lane == 0) counts[i] = cnt;
}
// The same for a LIST of map pairs in one launch (the robot pairs of sloamNode.cpp:600-694): the rows of all pairs flattened, row =
// one model triangle of one pair, one wave per row, four rows per workgroup.  The wave finds its pair in the row-offset table
// (uniform per wave: scalar code) and scans the data triangles of ITS pair only, in chunks of 64 counted from the pair's first data
// triangle — so the test, the ballot ranks and hence the order within a row are k_tri_match's for that pair alone.  sd / sx: the
// prepared triangles of all maps, one after the other (one k_tri_prepare launch).  EMIT = false: counts[row].  EMIT = true: the
// matched pair number base[s] + offs[row] + rank (offs: the segmented scan of counts, restarting at every pair; base[s] < 0: the
// pair was dropped) writes its three associations' points straight into the layout k_affinity_csr_seg reads — P1[a] = model vertex,
// P2[a] = data vertex, a = 3 * pair number + vertex, the identity association list of semantic_clipper.cpp:207-211.
template <bool EMIT>
__global__ __launch_bounds__(256) void k_tri_match_seg(const double* __restrict__ sd, const double* __restrict__ sx,
                                                       const int* __restrict__ rowoff, const TriSeg* __restrict__ segs, int n_seg, int n_rows,
                                                       double thr, int* __restrict__ counts, const long long* __restrict__ offs,
                                                       const long long* __restrict__ base, double* __restrict__ P1, double* __restrict__ P2) {
  const int row = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6))), lane = threadIdx.x & 63;
  if (row >= n_rows) return;
  const int s = seg_of_row(rowoff, n_seg, row);
  const TriSeg S = segs[s];
  const size_t i = (size_t)S.tm0 + (size_t)(row - rowoff[s]);
  const double* dd = sd + 3 * (size_t)S.td0;
  const double* xd = sx + 6 * (size_t)S.td0;
  const double m0 = sd[3 * i], m1 = sd[3 * i + 1], m2 = sd[3 * i + 2];
  long long at = 0;
  if (EMIT) {
    if (base[s] < 0) return;
    at = base[s] + offs[row];
  }
  int cnt = 0;
  for (int j0 = 0; j0 < S.ntd; j0 += 64) {
    const int j = j0 + lane;
    bool hit = false;
    if (j < S.ntd) hit = tri_pair_diff(m0, m1, m2, dd + 3 * (size_t)j) < thr;
    const unsigned long long mask = __ballot(hit);
    if (EMIT && hit) {
      const long long a = 3 * (at + __popcll(mask & ((1ull << lane) - 1ull)));
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        P1[2 * (a + k)] = sx[6 * i + 2 * k]; P1[2 * (a + k) + 1] = sx[6 * i + 2 * k + 1];
        P2[2 * (a + k)] = xd[6 * (size_t)j + 2 * k]; P2[2 * (a + k) + 1] = xd[6 * (size_t)j + 2 * k + 1];
      }
    }
    at += __popcll(mask);
    cnt += __popcll(mask);
  }
  if (!EMIT && lane == 0) counts[row] = cnt;
}

// Exclusive scan of per-row counts that restarts at every segment (pair), on the device: one workgroup per segment walks its rows
// [segoff[s], segoff[s + 1]) in chunks of 256 (wave scans by shuffle, the four wave sums through LDS, a running carry), sums in 64
// bits.  out[row + pad * s]; pad = 1 leaves room for the closing entry of every segment, which is written too: the n + 1 row
// pointers of a CSR per segment (OUT = int: a segment whose total passes 2^31 - 1 shows in totals[s], its entries are not used).
// totals[s]: the segment's sum — all the host reads back.
template <class OUT>
__global__ __launch_bounds__(256) void k_seg_scan(const int* __restrict__ cnt, const int* __restrict__ segoff, OUT* __restrict__ out, int pad,
                                                  long long* __restrict__ totals) {
  __shared__ long long wsum[4];
  const int s = blockIdx.x, r0 = segoff[s], r1 = segoff[s + 1];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  long long carry = 0;
  for (int c0 = r0; c0 < r1; c0 += 256) {
    const int r = c0 + (int)threadIdx.x;
    const long long v = r < r1 ? (long long)cnt[r] : 0;
    long long x = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const long long y = __shfl_up(x, d);
      if (lane >= d) x += y;
    }
    __syncthreads();                      // (wsum may still be read from the previous chunk)
    if (lane == 63) wsum[wave] = x;
    __syncthreads();
    long long before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) { if (w < wave) before += wsum[w]; all += wsum[w]; }
    if (r < r1) out[(size_t)r + (size_t)pad * s] = (OUT)(carry + before + x - v);
    carry += all;
  }
  if (threadIdx.x == 0) {
    totals[s] = carry;
    if (pad) out[(size_t)r1 + (size_t)pad * s] = (OUT)carry;
  }
}

// ---- Submaps around a list of key poses (getkeyPoseSubmap of the three map managers, then prepareLCInput) --------------------------
// cylinderMapManager.cpp:186-211, cubeMapManager.cpp:77-101, ellipsoidMapManager.cpp:82-107, sloamNode.cpp:544-576.  THE one test the
// count and the emit pass evaluate for object i of the concatenated table (cylinders, cubes, ellipsoids) and one key pose: the pose
// goes through pcl's PointT, i.e. float32 (px, py, pz), the height test uses the double pose z; kept iff distance(p) <= radius
// (inclusive) and |model z - pose z| < max_dz (strict).  Cubes and ellipsoids: |centre - p| (cube.cpp:26-29, ellipsoid.cpp:28-31);
// cylinders: the distance from p to the axis through root along the un-normalised ray, minus the radius (cylinder.cpp:226-234), model
// z = root z.  A NaN anywhere fails a comparison: dropped, as in the reference.
__device__ __forceinline__ bool submap_keeps(const SubmapDev& S, int i, double px, double py, double pz, double pose_z) {
  double d, mz;
  if (i < S.n_cyl) {
    const double* r = S.cyl_root + 3 * (size_t)i;
    const double* a = S.cyl_ray + 3 * (size_t)i;
    const double ex = px - r[0], ey = py - r[1], ez = pz - r[2];
    const double t = (ex * a[0] + ey * a[1] + ez * a[2]) / (a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
    const double qx = r[0] + t * a[0], qy = r[1] + t * a[1], qz = r[2] + t * a[2];
    const double dx = px - qx, dy = py - qy, dz = pz - qz;
    d = sqrt(dx * dx + dy * dy + dz * dz) - S.cyl_radius[i];
    mz = r[2];
  } else {
    const double* c = i < S.n_cyl + S.n_cube ? S.cube_xyz + 3 * (size_t)(i - S.n_cyl) : S.ell_xyz + 3 * (size_t)(i - S.n_cyl - S.n_cube);
    const double dx = c[0] - px, dy = c[1] - py, dz = c[2] - pz;
    d = sqrt(dx * dx + dy * dy + dz * dz);
    mz = c[2];
  }
  return d <= S.radius && fabs(mz - pose_z) < S.max_dz;
}
// One workgroup per (pose, chunk of 256 objects): blockIdx.x = pose * n_chunk + chunk.  EMIT = false: cnt[blockIdx.x] = kept objects
// of the chunk (a 64-lane ballot per wave, the four wave counts through LDS).  EMIT = true: the test again, and every kept object
// writes its row at base[pose] + chunkoff[blockIdx.x] (k_seg_scan of cnt, restarting at every pose) + the counts of the waves before
// its own + its rank inside the wave (the popcount of the lanes below it): a stable compaction, no atomic decides the order.
// Rows (prepareLCInput): cylinder [label, root, radius, 0, 0]; cube / ellipsoid [label, centre, scale].  Launch-latency bound at the
// sizes of a key-pose list: a 10 000-object map is 0.5 MB, read once per pose out of L2.
template <bool EMIT>
__global__ __launch_bounds__(256) void k_keypose_submap(SubmapDev S, int n_chunk, int* __restrict__ cnt, const long long* __restrict__ chunkoff,
                                                        const long long* __restrict__ base, double* __restrict__ rows7,
                                                        int32_t* __restrict__ src_idx) {
  __shared__ int wcnt[4];
  const int pose = (int)(blockIdx.x / (unsigned)n_chunk), chunk = (int)(blockIdx.x % (unsigned)n_chunk);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n_all = S.n_cyl + S.n_cube + S.n_ell;
  const int i = chunk * 256 + (int)threadIdx.x;
  const double* pp = S.pose_xyz + (size_t)S.pose_stride * pose;
  const double px = (double)(float)pp[0], py = (double)(float)pp[1], pz = (double)(float)pp[2];
  const bool keep = i < n_all && submap_keeps(S, i, px, py, pz, pp[2]);
  const unsigned long long mask = __ballot(keep);
  if (lane == 0) wcnt[wave] = __popcll(mask);
  __syncthreads();
  if (!EMIT) {
    if (threadIdx.x == 0) cnt[blockIdx.x] = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
    return;
  }
  if (!keep) return;
  long long row = base[pose] + chunkoff[blockIdx.x] + __popcll(mask & ((1ull << lane) - 1ull));
  for (int w = 0; w < wave; ++w) row += wcnt[w];
  double* o = rows7 + 7 * (size_t)row;
  if (i < S.n_cyl) {
    o[0] = (double)S.cyl_label[i];
    o[1] = S.cyl_root[3 * (size_t)i]; o[2] = S.cyl_root[3 * (size_t)i + 1]; o[3] = S.cyl_root[3 * (size_t)i + 2];
    o[4] = S.cyl_radius[i]; o[5] = 0.0; o[6] = 0.0;
  } else {
    const bool cube = i < S.n_cyl + S.n_cube;
    const int j = cube ? i - S.n_cyl : i - S.n_cyl - S.n_cube;
    const double* c = (cube ? S.cube_xyz : S.ell_xyz) + 3 * (size_t)j;
    const double* sc = (cube ? S.cube_scale : S.ell_scale) + 3 * (size_t)j;
    o[0] = (double)(cube ? S.cube_label : S.ell_label)[j];
    o[1] = c[0]; o[2] = c[1]; o[3] = c[2];
    o[4] = sc[0]; o[5] = sc[1]; o[6] = sc[2];
  }
  if (src_idx) src_idx[row] = i;
}
void launch_keypose_submap(bool emit, const SubmapDev& S, int n_poses, int n_chunk, int* cnt, const long long* chunkoff, const long long* base,
                           double* rows7, int32_t* src_idx, hipStream_t s) {
  if (n_poses <= 0 || n_chunk <= 0) return;
  const dim3 grid((unsigned)n_poses * (unsigned)n_chunk), block(256);
  if (emit) hipLaunchKernelGGL(k_keypose_submap<true>, grid, block, 0, s, S, n_chunk, cnt, chunkoff, base, rows7, src_idx);
  else hipLaunchKernelGGL(k_keypose_submap<false>, grid, block, 0, s, S, n_chunk, cnt, chunkoff, base, rows7, src_idx);
}

void launch_tri_match_seg(bool emit, const double* sd, const double* sx, const int* rowoff, const TriSeg* segs, int n_seg, int n_rows, double thr,
                          int* counts, const long long* offs, const long long* base, double* P1, double* P2, hipStream_t s) {
  if (n_rows <= 0) return;
  const dim3 grid((n_rows + 3) / 4), block(256);
  if (emit) hipLaunchKernelGGL(k_tri_match_seg<true>, grid, block, 0, s, sd, sx, rowoff, segs, n_seg, n_rows, thr, counts, offs, base, P1, P2);
  else hipLaunchKernelGGL(k_tri_match_seg<false>, grid, block, 0, s, sd, sx, rowoff, segs, n_seg, n_rows, thr, counts, offs, base, P1, P2);
}
void launch_seg_scan64(const int* cnt, const int* segoff, int n_seg, long long* out, long long* totals, hipStream_t s) {
  if (n_seg > 0) hipLaunchKernelGGL(k_seg_scan<long long>, dim3(n_seg), dim3(256), 0, s, cnt, segoff, out, 0, totals);
}
void launch_seg_scan_rowptr(const int* cnt, const int* segoff, int n_seg, int* rowptr, long long* totals, hipStream_t s) {
  if (n_seg > 0) hipLaunchKernelGGL(k_seg_scan<int>, dim3(n_seg), dim3(256), 0, s, cnt, segoff, rowptr, 1, totals);
}

void launch_tri_prepare(const double* tri, int n, double* sdist, double* sxy, hipStream_t s) {
  if (n > 0) hipLaunchKernelGGL(k_tri_prepare, dim3((n + 255) / 256), dim3(256), 0, s, tri, n, sdist, sxy);
}
void launch_tri_match(bool emit, const double* dm, const double* xm, int ntm, const double* dd, const double* xd, int ntd, double thr,
                      int* counts, const long long* offs, double* pts, double* diffs, hipStream_t s) {
  if (ntm <= 0) return;
  if (emit) hipLaunchKernelGGL(k_tri_match<true>, dim3((ntm + 3) / 4), dim3(256), 0, s, dm, xm, ntm, dd, xd, ntd, thr, counts, offs, pts, diffs);
  else hipLaunchKernelGGL(k_tri_match<false>, dim3((ntm + 3) / 4), dim3(256), 0, s, dm, xm, ntm, dd, xd, ntd, thr, counts, offs, pts, diffs);
}

void launch_place_sweep(const PlaceDev& P, hipStream_t s) {
  // cos/sin tables ride behind the yaw table: yaws[n_yaw .. 3 n_yaw)
  const double* cosv = P.yaws + P.n_yaw;
  const double* sinv = P.yaws + 2 * (size_t)P.n_yaw;
  const long long ncand = P.n_cells * P.n_yaw;
  long long blocks = (ncand + 3) / 4;
  if (blocks > 256 * 8) blocks = 256 * 8;
  if (blocks < 1) blocks = 1;
  if (P.rxy) {
    static const bool attr = (hipFuncSetAttribute(reinterpret_cast<const void*>(k_place_sweep_b), hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024), true);
    (void)attr;
    const size_t lds = place_lds_bytes(P.nr, P.nq, P.ignore_dim);
    hipLaunchKernelGGL(k_place_sweep_b, dim3((unsigned)blocks), dim3(256), lds, s, P, cosv, sinv);
    return;
  }
  // (the same opt-in as above: a reference map of more than 1365 objects takes more than the 64 KiB a launch gets without it)
  static const bool attr_plain = (hipFuncSetAttribute(reinterpret_cast<const void*>(k_place_sweep), hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024), true);
  (void)attr_plain;
  hipLaunchKernelGGL(k_place_sweep, dim3((unsigned)blocks), dim3(256), (size_t)P.nr * 6 * sizeof(double), s, P, cosv, sinv);
}
size_t place_lds_bytes(int nr, int nq, int ignore_dim) {
  return ((size_t)(ignore_dim ? 2 : 5) * ((size_t)nr + (size_t)nq)) * sizeof(double) + 2 * (size_t)nq * sizeof(int) + 16;
}
void launch_place_sweep_seg(const PlaceDev* segs, const PlaceWg* wgs, int n_wg, size_t lds_bytes, PlaceBest* part, const int* wg0, int n_seg,
                            PlaceBest* best, hipStream_t s) {
  if (n_wg <= 0 || n_seg <= 0) return;
  static const bool attr = (hipFuncSetAttribute(reinterpret_cast<const void*>(k_place_sweep_seg), hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024), true);
  (void)attr;
  hipLaunchKernelGGL(k_place_sweep_seg, dim3((unsigned)n_wg), dim3(256), lds_bytes, s, segs, wgs, part);
  hipLaunchKernelGGL(k_place_best_seg, dim3((unsigned)n_seg), dim3(256), 0, s, part, wg0, best);
}
void launch_place_argmax(const int32_t* inliers, long long n, long long* best_idx, int32_t* best_val, hipStream_t s) {
  hipLaunchKernelGGL(k_place_argmax, dim3(256), dim3(256), 0, s, inliers, n, best_idx, best_val);
}
void launch_clipper_affinity(const double* D1, const double* D2, int dim, const int32_t* A, int m, double sigma, double eps,
                             double mindist, double affinityeps, double* M, hipStream_t s) {
  hipLaunchKernelGGL(k_clipper_affinity, dim3((m + 127) / 128, m), dim3(128), 0, s, D1, D2, dim, A, m, sigma, eps, mindist,
                     affinityeps, M);
}

}  // namespace sl
