// gatv2_scores_cpu.cpp — the DeviceType::kCPU kernels of ops "gatv2_scores_csr_heads" and
// "gatv2_scores_csr_heads_grad" (contract in include/ofx_spmm.h; shared helpers in
// gatv2_scores.h).  Row-parallel over OpenMP, every row computed by one thread in a fixed order,
// so the bits do not depend on num_threads; the same bits as the HIP kernels
// (gatv2_scores_heads.hip, gatv2_scores_grad.hip).  The forward is the SDDMM's row loop of
// spmm_rows_cpu.h with the activated, rounded sum in the right factor's place; the gradient is the
// sum's row loop with the per-nonzero terms T1 / T2 in the product's place.
#pragma clang fp contract(off)

#include <omp.h>

#include <type_traits>
#include <vector>

#include "gatv2_scores.h"
#include "ofx_internal.h"
#include "spmm_common.h"

namespace ofx {
namespace {

using namespace gv2;

template <typename T, typename I>
void cpu_forward(int nthreads, const I* rp, const I* col, const T* x_row, int64_t ldr,
                 const T* x_col, int64_t ldc, const T* att, double negative_slope, T* out,
                 int64_t heads, int64_t d, int64_t k, int64_t row_begin, int64_t row_end) {
#pragma clang fp contract(off)
  using A = typename Num<T>::acc;
  const A slope = (A)negative_slope;
  const int64_t leaves = (d + 7) / 8;
  int64_t padded = 1;
  while (padded < leaves) padded *= 2;
#pragma omp parallel num_threads(nthreads)
  {
    std::vector<A> leaf(padded);
#pragma omp for schedule(dynamic, 64)
    for (int64_t r = row_begin; r < row_end; ++r) {
      for (int64_t j = (int64_t)rp[r]; j < (int64_t)rp[r + 1]; ++j) {
        const int64_t cj = (int64_t)col[j];
        for (int64_t h = 0; h < heads; ++h) {
          const T* xr = x_row + (r - row_begin) * ldr + h * d;
          const T* xc = (uint64_t)cj < (uint64_t)k ? x_col + cj * ldc + h * d : nullptr;
          const T* w = att + h * d;
          for (int64_t l = 0; l < padded; ++l) {
            A s = A(0);
            for (int64_t e = 8 * l; e < 8 * l + 8 && e < d; ++e) {
              const A z = Num<T>::load(xr[e]) + (xc ? Num<T>::load(xc[e]) : A(0));
              s = s + Num<T>::load(w[e]) * activated<T>(z, slope);
            }
            leaf[l] = s;
          }
          for (int64_t wd = 1; wd < padded; wd *= 2)
            for (int64_t l = 0; l < padded; l += 2 * wd) leaf[l] = leaf[l] + leaf[l + wd];
          out[j * heads + h] = Num<T>::store(leaf[0]);
        }
      }
    }
  }
}

// Nonzeros [j0, j1) of one head: a1[c] = the sum of T1[j, c] and, with a2, a2[c] = the sum of
// T2[j, c], from +0, ascending.
template <typename T, typename I>
void grad_row_sum(const I* col, const T* de, int64_t heads, const typename Num<T>::acc* xr,
                  const T* x_col, int64_t ldc, int64_t k, const typename Num<T>::acc* wpos,
                  const typename Num<T>::acc* wneg, typename Num<T>::acc slope, int64_t d,
                  int64_t j0, int64_t j1, typename Num<T>::acc* a1, typename Num<T>::acc* a2) {
#pragma clang fp contract(off)
  using A = typename Num<T>::acc;
  for (int64_t c = 0; c < d; ++c) a1[c] = A(0);
  if (a2)
    for (int64_t c = 0; c < d; ++c) a2[c] = A(0);
  for (int64_t j = j0; j < j1; ++j) {
    const A g = Num<T>::load(de[j * heads]);
    const int64_t cj = (int64_t)col[j];
    const T* xc = (uint64_t)cj < (uint64_t)k ? x_col + cj * ldc : nullptr;
    for (int64_t c = 0; c < d; ++c) {
      const A z = xr[c] + (xc ? Num<T>::load(xc[c]) : A(0));
      a1[c] = a1[c] + rounded<T>(g * (z > A(0) ? wpos[c] : wneg[c]));
      if (a2) a2[c] = a2[c] + Num<T>::mul(g, activated<T>(z, slope));
    }
  }
}

template <typename T, typename I>
void cpu_backward(int nthreads, const I* rp, const I* col, const T* x_row, int64_t ldr,
                  const T* x_col, int64_t ldc, const T* att, double negative_slope, const T* de,
                  T* d_x, int64_t ldd, T* p, int64_t ldp, int64_t heads, int64_t d, int64_t k,
                  int64_t row_begin, int64_t row_end, const Schedule& s) {
#pragma clang fp contract(off)
  using A = typename Num<T>::acc;
  const A slope = (A)negative_slope;
  const int64_t rows = row_end - row_begin;
#pragma omp parallel num_threads(nthreads)
  {
    std::vector<A> xr(d), wpos(d), wneg(d), acc1(d), acc2(d), part1(d), part2(d);
#pragma omp for schedule(dynamic, 64)
    for (int64_t g = 0; g < rows; ++g) {
      const int64_t r = row_begin + g;
      const int64_t j0 = (int64_t)rp[r], j1 = (int64_t)rp[r + 1];
      const int64_t len = j1 - j0;
      for (int64_t h = 0; h < heads; ++h) {
        for (int64_t c = 0; c < d; ++c) {
          xr[c] = Num<T>::load(x_row[g * ldr + h * d + c]);
          wpos[c] = Num<T>::load(att[h * d + c]);
          wneg[c] = wpos[c] * slope;
        }
        const T* xc = x_col ? x_col + h * d : nullptr;
        const T* dh = de ? de + h : nullptr;  // NULL with nnz == 0: no row has a nonzero
        if (len <= s.split) {
          grad_row_sum<T, I>(col, dh, heads, xr.data(), xc, ldc, xc ? k : 0, wpos.data(),
                             wneg.data(), slope, d, j0, j1, acc1.data(), p ? acc2.data() : nullptr);
        } else {
          const int64_t nc = num_chunks(len, s.chunk);
          for (int64_t c = 0; c < d; ++c) acc1[c] = acc2[c] = A(0);
          for (int64_t q = 0; q < nc; ++q) {
            const int64_t a = j0 + q * s.chunk;
            const int64_t e = (q == nc - 1) ? j1 : a + s.chunk;
            grad_row_sum<T, I>(col, dh, heads, xr.data(), xc, ldc, xc ? k : 0, wpos.data(),
                               wneg.data(), slope, d, a, e, part1.data(),
                               p ? part2.data() : nullptr);
            for (int64_t c = 0; c < d; ++c) acc1[c] = acc1[c] + part1[c];
            if (p)
              for (int64_t c = 0; c < d; ++c) acc2[c] = acc2[c] + part2[c];
          }
        }
        for (int64_t c = 0; c < d; ++c) d_x[g * ldd + h * d + c] = Num<T>::store(acc1[c]);
        if (p)
          for (int64_t c = 0; c < d; ++c) p[g * ldp + h * d + c] = Num<T>::store(acc2[c]);
      }
    }
  }
}

}  // namespace
}  // namespace ofx

using namespace ofx;

extern "C" int ofx_gatv2_scores_csr_heads_cpu(int num_threads, int idx_dtype, int val_dtype,
                                              int64_t m, int64_t k, int64_t heads, int64_t d,
                                              int64_t nnz, const void* row_ptr, const void* col_idx,
                                              const void* x_row, int64_t ldr, const void* x_col,
                                              int64_t ldc, const void* att, double negative_slope,
                                              void* e, int64_t row_begin, int64_t row_end) {
  return ::ofx::guarded(__func__, [&]() -> int {
    bool nothing = false;
    if (const int rc = gv2::check_gatv2_args(
            "gatv2_scores_csr_heads_cpu", false, idx_dtype, val_dtype, m, k, heads, d, nnz, row_ptr,
            col_idx, x_row, ldr, x_col, ldc, att, negative_slope, nullptr, e, 0, nullptr, 0,
            row_begin, row_end, nullptr, &nothing))
      return rc;
    if (nothing) return OFX_OK;
    return by_types(idx_dtype, val_dtype, [&](auto* tp, auto* ip) -> int {
      using T = std::remove_pointer_t<decltype(tp)>;
      using I = std::remove_pointer_t<decltype(ip)>;
      cpu_forward<T, I>(threads_of(num_threads), (const I*)row_ptr, (const I*)col_idx,
                        (const T*)x_row, ldr, (const T*)x_col, ldc, (const T*)att, negative_slope,
                        (T*)e, heads, d, x_col ? k : 0, row_begin, row_end);
      return OFX_OK;
    });
  });
}

extern "C" int ofx_gatv2_scores_csr_heads_grad_cpu(
    int num_threads, int idx_dtype, int val_dtype, int64_t m, int64_t k, int64_t heads, int64_t d,
    int64_t nnz, const void* row_ptr, const void* col_idx, const void* x_row, int64_t ldr,
    const void* x_col, int64_t ldc, const void* att, double negative_slope, const void* de,
    void* d_x, int64_t ldd, void* p, int64_t ldp, int64_t row_begin, int64_t row_end,
    const ofx_spmm_options* opts) {
  return ::ofx::guarded(__func__, [&]() -> int {
    OFX_READ_OPTIONS(opts, "gatv2_scores_csr_heads_grad_cpu");
    bool nothing = false;
    if (const int rc = gv2::check_gatv2_args(
            "gatv2_scores_csr_heads_grad_cpu", true, idx_dtype, val_dtype, m, k, heads, d, nnz,
            row_ptr, col_idx, x_row, ldr, x_col, ldc, att, negative_slope, de, d_x, ldd, p, ldp,
            row_begin, row_end, opts, &nothing))
      return rc;
    if (nothing) return OFX_OK;
    const Schedule s = resolve_schedule(d, opts);  // of ONE head's width: the numeric contract
    return by_types(idx_dtype, val_dtype, [&](auto* tp, auto* ip) -> int {
      using T = std::remove_pointer_t<decltype(tp)>;
      using I = std::remove_pointer_t<decltype(ip)>;
      cpu_backward<T, I>(threads_of(num_threads), (const I*)row_ptr, (const I*)col_idx,
                         (const T*)x_row, ldr, (const T*)x_col, ldc, (const T*)att, negative_slope,
                         (const T*)de, (T*)d_x, ldd, (T*)p, ldp, heads, d, k, row_begin, row_end,
                         s);
      return OFX_OK;
    });
  });
}
