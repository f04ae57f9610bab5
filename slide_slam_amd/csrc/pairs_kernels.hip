// The fixed-radius pair search (slide_pairs_within / slide_graph_landmark_pairs_within): every pair i < j of n points at most `radius`
// apart, and of one label where labels are given — the candidates of the duplicate-landmark test.  No counterpart in the reference,
// whose association never compares two landmarks of the map with each other.
//
// The count / k_seg_scan / emit idiom of k_tri_match_seg and k_keypose_submap (place_kernels.hip): the count pass leaves the number of
// partners j > i of every row i, k_seg_scan turns the counts into the rows' offsets, the emit pass evaluates the same test again and
// writes.  One wavefront per row i walks j = i + 1 .. n - 1 in chunks of 64; a kept j lands at the row's offset + the kept ones of
// the chunks before + the popcount of the ballot's lanes below it: the output is sorted by (i, j) and no atomic decides an order.
// The distance is sqrt((dx dx + dy dy) + dz dz) in double, products not contracted (this file is built with -ffp-contract=off), so
// a host restatement decides every pair the same way; a NaN fails the comparison and is dropped.
// Launch-latency bound at map sizes: 5000 points are 12.5 M tests on 120 KB that stay in L2.
#include <hip/hip_runtime.h>

#include "kernels.hpp"

namespace sl {

// (the rows' walk, shared by the two kernels below.  NEQ = false: only EQUAL labels pair, where labels are given; NEQ = true: `label` is a
// group word per point and only DIFFERENT groups pair)
template <bool EMIT, bool NEQ>
__device__ __forceinline__ void pairs_within_body(const double* __restrict__ pts, int stride, const int* __restrict__ sel,
                                                  const int32_t* __restrict__ label, int n, double radius, int* __restrict__ cnt,
                                                  const long long* __restrict__ off, int32_t* __restrict__ out_i,
                                                  int32_t* __restrict__ out_j, double* __restrict__ out_dist) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long row = (long long)blockIdx.x * 4 + wave;
  if (row >= n) return;                      // (no barrier below: a wavefront may leave alone)
  const int i = (int)row;
  const double* pi = pts + (size_t)stride * (sel ? sel[i] : i);
  const double xi = pi[0], yi = pi[1], zi = pi[2];
  const int32_t li = label ? label[i] : 0;
  const long long base = EMIT ? off[i] : 0;
  long long c = 0;
  for (int j0 = i + 1; j0 < n; j0 += 64) {
    const int j = j0 + lane;
    bool keep = false;
    double d = 0.0;
    if (j < n) {
      const double* pj = pts + (size_t)stride * (sel ? sel[j] : j);
      const double dx = xi - pj[0], dy = yi - pj[1], dz = zi - pj[2];
      d = sqrt((dx * dx + dy * dy) + dz * dz);
      keep = d <= radius && (NEQ ? label[j] != li : (!label || label[j] == li));
    }
    const unsigned long long mask = __ballot(keep);
    if (EMIT && keep) {
      const long long at = base + c + __popcll(mask & ((1ull << lane) - 1ull));
      out_i[at] = i;
      out_j[at] = j;
      out_dist[at] = d;
    }
    c += __popcll(mask);
  }
  if (!EMIT && lane == 0) cnt[i] = (int)c;
}
template <bool EMIT>
__global__ __launch_bounds__(256) void k_pairs_within(const double* __restrict__ pts, int stride, const int* __restrict__ sel,
                                                      const int32_t* __restrict__ label, int n, double radius, int* __restrict__ cnt,
                                                      const long long* __restrict__ off, int32_t* __restrict__ out_i,
                                                      int32_t* __restrict__ out_j, double* __restrict__ out_dist) {
  pairs_within_body<EMIT, false>(pts, stride, sel, label, n, radius, cnt, off, out_i, out_j, out_dist);
}
// The sibling with the group-INEQUALITY filter (slide_chol_batch_landmark_pairs_within with cross_only): group[q] is one word per point,
// never null, and a pair is kept only where its two groups differ.  Everything else — the walk, the distance, the compaction and with
// them the order of the output — is the kernel's above.
template <bool EMIT>
__global__ __launch_bounds__(256) void k_pairs_within_neq(const double* __restrict__ pts, int stride, const int* __restrict__ sel,
                                                          const int32_t* __restrict__ group, int n, double radius, int* __restrict__ cnt,
                                                          const long long* __restrict__ off, int32_t* __restrict__ out_i,
                                                          int32_t* __restrict__ out_j, double* __restrict__ out_dist) {
  pairs_within_body<EMIT, true>(pts, stride, sel, group, n, radius, cnt, off, out_i, out_j, out_dist);
}
void launch_pairs_within(bool emit, const double* pts, int stride, const int* sel, const int32_t* label, int n, double radius, int* cnt,
                         const long long* off, int32_t* out_i, int32_t* out_j, double* out_dist, hipStream_t s) {
  if (n <= 0) return;
  const dim3 grid((n + 3) / 4), block(256);
  if (emit) hipLaunchKernelGGL(k_pairs_within<true>, grid, block, 0, s, pts, stride, sel, label, n, radius, cnt, off, out_i, out_j, out_dist);
  else hipLaunchKernelGGL(k_pairs_within<false>, grid, block, 0, s, pts, stride, sel, label, n, radius, cnt, off, out_i, out_j, out_dist);
}
void launch_pairs_within_neq(bool emit, const double* pts, int stride, const int* sel, const int32_t* group, int n, double radius, int* cnt,
                             const long long* off, int32_t* out_i, int32_t* out_j, double* out_dist, hipStream_t s) {
  if (n <= 0) return;
  const dim3 grid((n + 3) / 4), block(256);
  if (emit) hipLaunchKernelGGL(k_pairs_within_neq<true>, grid, block, 0, s, pts, stride, sel, group, n, radius, cnt, off, out_i, out_j, out_dist);
  else hipLaunchKernelGGL(k_pairs_within_neq<false>, grid, block, 0, s, pts, stride, sel, group, n, radius, cnt, off, out_i, out_j, out_dist);
}

// The search's input on the joint graph of a CholBatch: entry q of the job's list, ent[q] = {member graph, landmark, group word, .}
// (Gs: the batch's table of its members' views).  The landmark's anchor — the three doubles at `coff` of its 15 of lm_est: 0 for a
// point's xyz and a cylinder's root, 9 for a cube's t — goes to pts[3 q ..] and its group word to group[q], so that the walk above
// runs on one contiguous array whichever graphs hold the landmarks.  The host bounds every ent[q] by what the member's device view
// holds.
__global__ __launch_bounds__(256) void k_joint_lm_anchor_gather(const GraphDev* __restrict__ Gs, const int4* __restrict__ ent, int coff, int n,
                                                                double* __restrict__ pts, int32_t* __restrict__ group) {
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q >= n) return;
  const int4 e = ent[q];
  const double* v = Gs[e.x].lm_est + 15 * (size_t)e.y + coff;
  pts[3 * (size_t)q] = v[0]; pts[3 * (size_t)q + 1] = v[1]; pts[3 * (size_t)q + 2] = v[2];
  group[q] = e.z;
}
void launch_joint_lm_anchor_gather(const GraphDev* Gs, const int4* ent, int coff, int n, double* pts, int32_t* group, hipStream_t s) {
  if (n > 0) hipLaunchKernelGGL(k_joint_lm_anchor_gather, dim3((n + 255) / 256), dim3(256), 0, s, Gs, ent, coff, n, pts, group);
}

}  // namespace sl
