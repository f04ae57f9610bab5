// Host side of the CLIPPER clique solver (host_clipper.hip) and the small pieces every stand-alone matcher entry point shares:
// call-scoped device memory, the device-time table behind slide_last_device_ms, the CSR builders and THE one path to a clique solve.
#pragma once
#include <algorithm>
#include <functional>
#include <vector>

#include "host_graph.hpp"

namespace sl {

// device memory of one call: freed when the call returns
struct Tmp {
  std::vector<void*> ptrs;
  ~Tmp() { for (void* p : ptrs) (void)hipFree(p); }
  template <class T>
  T* up(const T* h, size_t n) {
    T* d = nullptr;
    if (hipMalloc(&d, std::max<size_t>(n, 1) * sizeof(T)) != hipSuccess) return nullptr;
    ptrs.push_back(d);
    if (n && h && hipMemcpy(d, h, n * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) return nullptr;
    return d;
  }
};

// Measurement aid (slide_last_device_ms): device time of the kernels of the LAST stand-alone SlideMatch / SlideGraph / CLIPPER call of
// this process, HIP events on the stream those entry points launch on (the legacy stream) right around the launches — uploads, host
// prefix sums and read-backs excluded.  Slots: include/slide_gpu.h.
extern double g_dev_ms[SLIDE_MS_COUNT];
struct DevTimer {
  hipEvent_t a = nullptr, b = nullptr;
  int slot;
  bool add;
  explicit DevTimer(int slot_, bool add_ = false) : slot(slot_), add(add_) {
    if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) { a = b = nullptr; return; }
    (void)hipEventRecord(a, nullptr);
  }
  ~DevTimer() {
    if (!a || !b) return;
    float ms = 0.f;
    if (hipEventRecord(b, nullptr) == hipSuccess && hipEventSynchronize(b) == hipSuccess && hipEventElapsedTime(&ms, a, b) == hipSuccess)
      g_dev_ms[slot] = (add ? g_dev_ms[slot] : 0.0) + (double)ms;
    (void)hipEventDestroy(a);
    (void)hipEventDestroy(b);
  }
};

inline void identity16(double* tf) { for (int i = 0; i < 16; ++i) tf[i] = (i % 5 == 0) ? 1.0 : 0.0; }
inline slide_clipper_params_t clipper_params_or_default(const slide_clipper_params_t* p) {
  slide_clipper_params_t P;
  if (p) P = *p; else slide_clipper_default_params(&P);
  return P;
}

// A CSR of the symmetric affinity matrix on the device (in the caller's Tmp), its row pointers on the host as well.  Three builders
// feed the one solve below: from a dense upper triangle, from the associations, from the caller's own arrays.
struct DevCsr {
  int* ptr = nullptr;
  int* col = nullptr;
  double* val = nullptr;
  long long nnz = -1;          // set once the scan of the row counts has finished
  std::vector<int> h_ptr;
};
int csr_from_assoc_device(Tmp& T, const double* d1, const double* d2, int dim, const int32_t* dA, int m, double sigma, double epsilon,
                          double mindist, double affinityeps, DevCsr& S, long long cap = -1);
int solve_csr_device(Tmp& T, const DevCsr& S, int n, const double* u0, const slide_clipper_params_t& P, std::vector<int>& nodes,
                     std::vector<double>& u, double& score);

// The CSRs of n_seg problems in shared device buffers, as launch_seg_scan_rowptr and the *_csr_seg kernels leave them: segment s owns
// rows off[s] .. off[s + 1], its row pointers stand at d_rptr + off[s] + s, its col / val at nnz0[s] (tot[s] of them; nnz0[s] < 0: the
// segment is skipped).  d_work: 6 doubles per row.  d_res (res_len doubles, the caller's, cleared): [out4 per segment | u of every
// row | whatever else the caller wants in the same read-back].
struct ClqSegments {
  int n_seg;
  const int* off;                // host, n_seg + 1
  const int* d_off;              // the same on the device
  int* d_rptr; int* d_col; double* d_val;
  const long long* nnz0; const long long* tot;      // host, n_seg each
  double* d_work;
  double* d_res; size_t res_len;
};
// Solves every segment that is not skipped and hands each to visit(s, nodes, u, score) in segment order.  u0[s]: the caller's start
// weights of segment s or null (default_u0).  res receives d_res before the first visit.  Segments below the cooperative threshold run
// in ONE launch_clq_solve_batch; a segment at or above it goes through solve_csr_device on its slice when its turn comes.
using ClqVisit = std::function<void(int s, const std::vector<int>& nodes, const std::vector<double>& u, double score)>;
int solve_csr_segments(Tmp& T, const ClqSegments& G, const std::vector<const double*>& u0, const slide_clipper_params_t& P,
                       std::vector<double>& res, const ClqVisit& visit);

void estimate_tf2d(const double* a, const double* b, int n, double* tf3);
int match_triangles_device(Tmp& T, const double* tri_model, int ntm, const double* tri_data, int ntd, double thr, double** d_pts,
                           double** d_diffs, long long* np);

}  // namespace sl
