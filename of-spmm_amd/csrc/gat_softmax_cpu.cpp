// gat_softmax_cpu.cpp — the DeviceType::kCPU kernels of ops "gat_softmax_csr_heads" and
// "gat_softmax_csr_heads_grad" (contract in include/ofx_spmm.h; shared helpers in
// gat_softmax.h and edge_softmax.h).  Row-parallel over OpenMP like edge_softmax_cpu.cpp; the same
// bits as the HIP kernels (gat_softmax_heads.hip).  A head's scores are formed, rounded to T and
// handed to the edge softmax's own row step (esm::softmax_row), so attn has the bits of
// ofx_edge_softmax_csr_heads on those scores by construction; the gradient takes de from the edge
// softmax's gradient row (esm::softmax_grad_row) in the same way.
#pragma clang fp contract(off)

#include <omp.h>

#include <type_traits>
#include <vector>

#include "edge_softmax.h"
#include "gat_softmax.h"
#include "ofx_internal.h"
#include "spmm_common.h"
#include "spmm_extremum.h"

namespace ofx {
namespace {

using namespace esm;
using namespace gsm;

// z = load(s_row[r, h]) + load(s_col[c, h]); a column outside [0, k) reads +0.
template <typename T, typename I>
typename Num<T>::acc score_sum(typename Num<T>::acc sr, const T* s_col, const I* ci, int64_t j,
                               int64_t heads, int64_t k) {
#pragma clang fp contract(off)
  using A = typename Num<T>::acc;
  const int64_t c = (int64_t)ci[j];
  const A sc = (uint64_t)c < (uint64_t)k ? Num<T>::load(s_col[c * heads]) : A(0);
  return sr + sc;
}

template <typename T, typename I>
void cpu_forward(int nthreads, const I* rp, const I* ci, const T* s_row, const T* s_col,
                 double negative_slope, T* attn, int64_t heads, int64_t k, int64_t row_begin,
                 int64_t row_end) {
#pragma clang fp contract(off)
  using A = typename Num<T>::acc;
  const A slope = (A)negative_slope;
#pragma omp parallel num_threads(nthreads)
  {
    std::vector<A> x, leaf;
#pragma omp for schedule(dynamic, 64)
    for (int64_t r = row_begin; r < row_end; ++r) {
      const int64_t j0 = (int64_t)rp[r], len = (int64_t)rp[r + 1] - j0;
      if (len <= 0) continue;
      x.resize((size_t)len);
      for (int64_t h = 0; h < heads; ++h) {
        const A sr = Num<T>::load(s_row[(r - row_begin) * heads + h]);
        for (int64_t p = 0; p < len; ++p) {
          const A z = score_sum<T, I>(sr, s_col + h, ci, j0 + p, heads, k);
          const T e = Num<T>::store(canonical_nan(leaky<A>(z, slope)));
          x[(size_t)p] = Num<T>::load(e);
        }
        softmax_row<T>(x.data(), len, leaf, attn + j0 * heads + h, heads);
      }
    }
  }
}

template <typename T, typename I>
void cpu_backward(int nthreads, const I* rp, const I* ci, const T* s_row, const T* s_col,
                  double negative_slope, const T* y, const T* g, T* ds, T* d_row, int64_t heads,
                  int64_t k, int64_t row_begin, int64_t row_end) {
#pragma clang fp contract(off)
  using A = typename Num<T>::acc;
  const A slope = (A)negative_slope;
#pragma omp parallel num_threads(nthreads)
  {
    std::vector<A> q, leaf;
#pragma omp for schedule(dynamic, 64)
    for (int64_t r = row_begin; r < row_end; ++r) {
      const int64_t j0 = (int64_t)rp[r], len = (int64_t)rp[r + 1] - j0;
      T* dr = d_row + (r - row_begin) * heads;
      if (len <= 0) {
        for (int64_t h = 0; h < heads; ++h) dr[h] = Num<T>::store(A(0));
        continue;
      }
      q.resize((size_t)len);
      for (int64_t h = 0; h < heads; ++h) {
        T* dh = ds + j0 * heads + h;
        const A sr = Num<T>::load(s_row[(r - row_begin) * heads + h]);
        // the edge softmax's de, scaled by the activation's factor; q collects the second sum
        softmax_grad_row<T>(y + j0 * heads + h, g + j0 * heads + h, heads, len, q.data(), leaf,
                            [&](int64_t p, T de) {
                              const A z = score_sum<T, I>(sr, s_col + h, ci, j0 + p, heads, k);
                              const A scaled = Num<T>::load(de) * leaky_factor<A>(z, slope);
                              dh[p * heads] = Num<T>::store(canonical_nan(scaled));
                              q[(size_t)p] = Num<T>::load(dh[p * heads]);
                            });
        dr[h] = Num<T>::store(canonical_nan(tree_sum(q.data(), len, leaf)));
      }
    }
  }
}

}  // namespace
}  // namespace ofx

using namespace ofx;

extern "C" int ofx_gat_softmax_csr_heads_cpu(int num_threads, int idx_dtype, int val_dtype,
                                             int64_t m, int64_t k, int64_t heads, int64_t nnz,
                                             const void* row_ptr, const void* col_idx,
                                             const void* s_row, const void* s_col,
                                             double negative_slope, void* attn, int64_t row_begin,
                                             int64_t row_end, const ofx_spmm_options* opts) {
  return ::ofx::guarded(__func__, [&]() -> int {
    OFX_READ_OPTIONS(opts, "gat_softmax_csr_heads_cpu");  // validated; no option has an effect
    bool nothing = false;
    if (const int rc = gsm::check_gat_softmax_args(
            "gat_softmax_csr_heads_cpu", false, idx_dtype, val_dtype, m, k, heads, nnz, row_ptr,
            col_idx, s_row, s_col, negative_slope, nullptr, nullptr, attn, nullptr, row_begin,
            row_end, &nothing))
      return rc;
    if (nothing) return OFX_OK;
    return by_types(idx_dtype, val_dtype, [&](auto* tp, auto* ip) -> int {
      using T = std::remove_pointer_t<decltype(tp)>;
      using I = std::remove_pointer_t<decltype(ip)>;
      cpu_forward<T, I>(threads_of(num_threads), (const I*)row_ptr, (const I*)col_idx,
                        (const T*)s_row, (const T*)s_col, negative_slope, (T*)attn, heads, k,
                        row_begin, row_end);
      return OFX_OK;
    });
  });
}

extern "C" int ofx_gat_softmax_csr_heads_grad_cpu(int num_threads, int idx_dtype, int val_dtype,
                                                  int64_t m, int64_t k, int64_t heads, int64_t nnz,
                                                  const void* row_ptr, const void* col_idx,
                                                  const void* s_row, const void* s_col,
                                                  double negative_slope, const void* attn,
                                                  const void* g, void* ds, void* d_row,
                                                  int64_t row_begin, int64_t row_end,
                                                  const ofx_spmm_options* opts) {
  return ::ofx::guarded(__func__, [&]() -> int {
    OFX_READ_OPTIONS(opts, "gat_softmax_csr_heads_grad_cpu");
    bool nothing = false;
    if (const int rc = gsm::check_gat_softmax_args(
            "gat_softmax_csr_heads_grad_cpu", true, idx_dtype, val_dtype, m, k, heads, nnz,
            row_ptr, col_idx, s_row, s_col, negative_slope, attn, g, ds, d_row, row_begin, row_end,
            &nothing))
      return rc;
    if (nothing) return OFX_OK;
    return by_types(idx_dtype, val_dtype, [&](auto* tp, auto* ip) -> int {
      using T = std::remove_pointer_t<decltype(tp)>;
      using I = std::remove_pointer_t<decltype(ip)>;
      cpu_backward<T, I>(threads_of(num_threads), (const I*)row_ptr, (const I*)col_idx,
                         (const T*)s_row, (const T*)s_col, negative_slope, (const T*)attn,
                         (const T*)g, (T*)ds, (T*)d_row, heads, k, row_begin, row_end);
      return OFX_OK;
    });
  });
}
