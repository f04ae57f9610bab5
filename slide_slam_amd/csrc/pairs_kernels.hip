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

template <bool EMIT>
__global__ __launch_bounds__(256) void k_pairs_within(const double* __restrict__ pts, int stride, const int* __restrict__ sel,
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
      keep = d <= radius && (!label || label[j] == li);
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
void launch_pairs_within(bool emit, const double* pts, int stride, const int* sel, const int32_t* label, int n, double radius, int* cnt,
                         const long long* off, int32_t* out_i, int32_t* out_j, double* out_dist, hipStream_t s) {
  if (n <= 0) return;
  const dim3 grid((n + 3) / 4), block(256);
  if (emit) hipLaunchKernelGGL(k_pairs_within<true>, grid, block, 0, s, pts, stride, sel, label, n, radius, cnt, off, out_i, out_j, out_dist);
  else hipLaunchKernelGGL(k_pairs_within<false>, grid, block, 0, s, pts, stride, sel, label, n, radius, cnt, off, out_i, out_j, out_dist);
}

}  // namespace sl
