// The opaque handles of include/slide_gpu.h, for the translation units whose entry points take one (capi.hip, host_closure.hip).
#pragma once
#include <cstddef>
#include <mutex>

#include "host_graph.hpp"

struct slide_graph {
  sl::HostGraph g;
  explicit slide_graph(const slide_params_t& p) : g(p) {}
};
// The backend owns its HostGraph by value; the C-ABI graph functions take slide_graph*, whose only member is
// a HostGraph at offset 0, so a pointer to the backend's graph is a valid slide_graph*.
static_assert(offsetof(slide_graph, g) == 0, "slide_graph must start with its HostGraph");
struct slide_chol_batch { sl::CholBatch b; explicit slide_chol_batch(int n) : b(n) {} };

#define LOCK(G) std::lock_guard<std::mutex> lk((G)->g.mtx)
