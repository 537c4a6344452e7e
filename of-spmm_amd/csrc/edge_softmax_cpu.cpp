// edge_softmax_cpu.cpp — the DeviceType::kCPU kernels of ops "edge_softmax_csr" and
// "edge_softmax_csr_heads" and of their gradients (contract in include/ofx_spmm.h, shared helpers
// in edge_softmax.h).  Row-parallel over OpenMP like spmm_extremum_cpu.cpp; the same bits as the
// HIP kernels (edge_softmax.hip, edge_softmax_heads.hip).  The multi-head entries run the
// single-head code on every column of e[nnz, heads] (element stride `heads`; 1 is the single-head
// op), so a head has the single-head bits by construction: the four entries are one body.
#pragma clang fp contract(off)

#include <omp.h>

#include <type_traits>
#include <vector>

#include "edge_softmax.h"
#include "ofx_internal.h"
#include "spmm_common.h"
#include "spmm_extremum.h"

namespace ofx {
namespace {

using namespace esm;

// The sum's order (tree_sum) and one head's rows (softmax_row, softmax_grad_row) are
// edge_softmax.h's, shared with gat_softmax_cpu.cpp.

template <typename T, typename I>
void cpu_forward(int nthreads, const I* rp, const T* e, T* y, int64_t heads, int64_t row_begin,
                 int64_t row_end) {
#pragma clang fp contract(off)
  using A = typename Num<T>::acc;
#pragma omp parallel num_threads(nthreads)
  {
    std::vector<A> x, leaf;
#pragma omp for schedule(dynamic, 64)
    for (int64_t r = row_begin; r < row_end; ++r) {
      const int64_t j0 = (int64_t)rp[r], len = (int64_t)rp[r + 1] - j0;
      if (len <= 0) continue;
      x.resize((size_t)len);
      for (int64_t h = 0; h < heads; ++h) {
        const T* eh = e + j0 * heads + h;
        for (int64_t p = 0; p < len; ++p) x[(size_t)p] = Num<T>::load(eh[p * heads]);
        softmax_row<T>(x.data(), len, leaf, y + j0 * heads + h, heads);
      }
    }
  }
}

template <typename T, typename I>
void cpu_backward(int nthreads, const I* rp, const T* y, const T* g, T* de, int64_t heads,
                  int64_t row_begin, int64_t row_end) {
  using A = typename Num<T>::acc;
#pragma omp parallel num_threads(nthreads)
  {
    std::vector<A> q, leaf;
#pragma omp for schedule(dynamic, 64)
    for (int64_t r = row_begin; r < row_end; ++r) {
      const int64_t j0 = (int64_t)rp[r], len = (int64_t)rp[r + 1] - j0;
      if (len <= 0) continue;
      q.resize((size_t)len);
      for (int64_t h = 0; h < heads; ++h) {
        T* dh = de + j0 * heads + h;
        softmax_grad_row<T>(y + j0 * heads + h, g + j0 * heads + h, heads, len, q.data(), leaf,
                            [&](int64_t p, T v) { dh[p * heads] = v; });
      }
    }
  }
}

// The four entries: a = e (forward) or y (the gradient, with g); heads = 1 is the single-head op,
// which no heads check can refuse and no heads == 0 can empty.
template <bool BWD>
int cpu_entry(const char* fn, int num_threads, int idx_dtype, int val_dtype, int64_t m,
              int64_t heads, int64_t nnz, const void* row_ptr, const void* a, const void* g,
              void* out, int64_t row_begin, int64_t row_end, const ofx_spmm_options* opts) {
  OFX_READ_OPTIONS(opts, fn);  // validated; no option has an effect
  if (const int rc = check_edge_softmax_heads_args(fn, idx_dtype, val_dtype, m, heads, nnz,
                                                   row_begin, row_end))
    return rc;
  if (row_end == row_begin || nnz == 0 || heads == 0) return OFX_OK;
  OFX_REQUIRE(row_ptr && a && out && (!BWD || g), OFX_EINVAL, "%s: NULL pointer", fn);
  return by_types(idx_dtype, val_dtype, [&](auto* tp, auto* ip) -> int {
    using T = std::remove_pointer_t<decltype(tp)>;
    using I = std::remove_pointer_t<decltype(ip)>;
    if constexpr (BWD)
      cpu_backward<T, I>(threads_of(num_threads), (const I*)row_ptr, (const T*)a, (const T*)g,
                         (T*)out, heads, row_begin, row_end);
    else
      cpu_forward<T, I>(threads_of(num_threads), (const I*)row_ptr, (const T*)a, (T*)out, heads,
                        row_begin, row_end);
    return OFX_OK;
  });
}

}  // namespace
}  // namespace ofx

using namespace ofx;

extern "C" int ofx_edge_softmax_csr_cpu(int num_threads, int idx_dtype, int val_dtype, int64_t m,
                                        int64_t nnz, const void* row_ptr, const void* e, void* y,
                                        int64_t row_begin, int64_t row_end,
                                        const ofx_spmm_options* opts) {
  return ::ofx::guarded(__func__, [&]() -> int {
    return cpu_entry<false>("edge_softmax_csr_cpu", num_threads, idx_dtype, val_dtype, m, 1, nnz,
                            row_ptr, e, nullptr, y, row_begin, row_end, opts);
  });
}

extern "C" int ofx_edge_softmax_csr_grad_cpu(int num_threads, int idx_dtype, int val_dtype,
                                             int64_t m, int64_t nnz, const void* row_ptr,
                                             const void* y, const void* g, void* de,
                                             int64_t row_begin, int64_t row_end,
                                             const ofx_spmm_options* opts) {
  return ::ofx::guarded(__func__, [&]() -> int {
    return cpu_entry<true>("edge_softmax_csr_grad_cpu", num_threads, idx_dtype, val_dtype, m, 1,
                           nnz, row_ptr, y, g, de, row_begin, row_end, opts);
  });
}

extern "C" int ofx_edge_softmax_csr_heads_cpu(int num_threads, int idx_dtype, int val_dtype,
                                              int64_t m, int64_t heads, int64_t nnz,
                                              const void* row_ptr, const void* e, void* y,
                                              int64_t row_begin, int64_t row_end,
                                              const ofx_spmm_options* opts) {
  return ::ofx::guarded(__func__, [&]() -> int {
    return cpu_entry<false>("edge_softmax_csr_heads_cpu", num_threads, idx_dtype, val_dtype, m,
                            heads, nnz, row_ptr, e, nullptr, y, row_begin, row_end, opts);
  });
}

extern "C" int ofx_edge_softmax_csr_heads_grad_cpu(int num_threads, int idx_dtype, int val_dtype,
                                                   int64_t m, int64_t heads, int64_t nnz,
                                                   const void* row_ptr, const void* y,
                                                   const void* g, void* de, int64_t row_begin,
                                                   int64_t row_end, const ofx_spmm_options* opts) {
  return ::ofx::guarded(__func__, [&]() -> int {
    return cpu_entry<true>("edge_softmax_csr_heads_grad_cpu", num_threads, idx_dtype, val_dtype,
                           m, heads, nnz, row_ptr, y, g, de, row_begin, row_end, opts);
  });
}
