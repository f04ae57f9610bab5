// Stand-alone host program around THE scoring text of the loop-closure consistency matrix (closure_prepare_one and
// closure_pair_score, slide_slam_amd/csrc/kernels.hpp: host + device functions, the ones k_closure_prepare and k_closure_csr_seg call)
// — it touches no device.  tests/test_closure_score_host.py compiles it, feeds it a case (binary doubles: L, then per closure
// from_pose7, to_pose7, rel7, sigma6, from_idx, to_idx; then gate, sigma, affinityeps, odom_sigma6) and compares the L x L matrix it
// writes with the numpy restatement.  Built with -Xarch_host -fsanitize=address,undefined it is the sanitizer run of that text.
#include <cstdio>
#include <vector>

#include "kernels.hpp"

using namespace sl;

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<double> in;
  double buf[256];
  size_t got;
  while ((got = std::fread(buf, sizeof(double), 256, f)) > 0) in.insert(in.end(), buf, buf + got);
  std::fclose(f);
  if (in.empty()) return 2;
  const int L = (int)in[0];
  if (L < 0 || in.size() != 1 + 29 * (size_t)L + 9) return 2;
  const double* row = in.data() + 1;
  const double* tail = row + 29 * (size_t)L;
  ClosureScore P;
  P.gate = tail[0]; P.sigma = tail[1]; P.affinityeps = tail[2];
  for (int c = 0; c < 6; ++c) P.odom2[c] = tail[3 + c] * tail[3 + c];
  std::vector<double> pre(CLOSURE_PRE * (size_t)L + 1), sig2(6 * (size_t)L + 1), M((size_t)L * L + 1, 0.0);
  for (int k = 0; k < L; ++k) {
    const double* r = row + 29 * (size_t)k;
    closure_prepare_one(from7(r), from7(r + 7), from7(r + 14), pre.data() + CLOSURE_PRE * (size_t)k);
    for (int c = 0; c < 6; ++c) sig2[6 * (size_t)k + c] = r[21 + c] * r[21 + c];
  }
  for (int a = 0; a < L; ++a)
    for (int b = 0; b < L; ++b) {
      if (a == b) continue;
      const int i = a < b ? a : b, j = a < b ? b : a;      // the smaller index goes first
      const double* ri = row + 29 * (size_t)i;
      const double* rj = row + 29 * (size_t)j;
      const double df = ri[27] > rj[27] ? ri[27] - rj[27] : rj[27] - ri[27], dt = ri[28] > rj[28] ? ri[28] - rj[28] : rj[28] - ri[28];
      M[(size_t)a * L + b] = closure_pair_score(pre.data() + CLOSURE_PRE * (size_t)i, pre.data() + CLOSURE_PRE * (size_t)j, sig2.data() + 6 * (size_t)i,
                                                sig2.data() + 6 * (size_t)j, df + dt, P);
    }
  FILE* o = std::fopen(argv[2], "wb");
  if (!o) return 2;
  std::fwrite(M.data(), sizeof(double), (size_t)L * L, o);
  std::fclose(o);
  std::printf("closure score ok L=%d\n", L);
  return 0;
}
