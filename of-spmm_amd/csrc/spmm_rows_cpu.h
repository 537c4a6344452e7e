// spmm_rows_cpu.h — the row templates of the kCPU SpMM and SDDMM kernels: one for the sum (ops
// "spmm_csr", "fused_spmm_csr", "spmm_csr_heads") and one for the SDDMM ("sddmm_csr", its masked
// form, "sddmm_csr_heads"), each over `heads` heads of width d.  The single-head ops are the
// one-head case (heads = 1, d = n: the value stride is 1 and the column base 0), so every entry
// adds and rounds in the same order, the contract's (spmm_common.h; DESIGN.md §3f for the heads).
// Host code of the *_cpu.cpp units, which are built with -fopenmp.
#ifndef OFX_SPMM_ROWS_CPU_H_
#define OFX_SPMM_ROWS_CPU_H_

#include <omp.h>

#include <vector>

#include "ofx_internal.h"
#include "spmm_common.h"

namespace ofx {

// Nonzeros [j0, j1) of one head: acc[c] = sum of mul(val[j*vs], B[col[j], c]) from +0, ascending.
// A column outside [0, k): the reference CPU gather zero-fills the gathered row of an index >= the
// table size (oneflow/user/kernels/gather_kernel_util.cpp:84-89), so the nonzero adds val * 0; a
// negative index fails its CHECK_GE (:80), reported by the entries as OFX_EINVAL (`neg`).
template <typename T, typename I>
void row_sum(const I* col, const T* val, int64_t vs, const T* B, int64_t ldb, int64_t k, int64_t d,
             int64_t j0, int64_t j1, typename Num<T>::acc* acc, bool* neg) {
#pragma clang fp contract(off)
  using A = typename Num<T>::acc;
  for (int64_t c = 0; c < d; ++c) acc[c] = A(0);
  for (int64_t j = j0; j < j1; ++j) {
    const A v = Num<T>::load(val[j * vs]);
    const int64_t cj = (int64_t)col[j];
    if (cj >= 0 && cj < k) {
      const T* brow = B + cj * ldb;
      for (int64_t c = 0; c < d; ++c) acc[c] = acc[c] + Num<T>::mul(v, Num<T>::load(brow[c]));
    } else {  // the zero-filled gathered row
      if (cj < 0) *neg = true;
      for (int64_t c = 0; c < d; ++c) acc[c] = acc[c] + Num<T>::mul(v, A(0));
    }
  }
}

// C[g, h*d + c] for rows [row_begin, row_end) and every head: a row of at most s.split nonzeros is
// one in-order sum; a longer one is the in-order sum of its chunks' sums (num_chunks), then the
// fused epilogue (none: one rounding to T).  val is [nnz, heads], B and C are [., heads * d], the
// schedule that of ONE head's width.  OFX_EINVAL in `fn`'s name after a negative column.
template <typename T, typename I>
int cpu_spmm_rows(const char* fn, int nthreads, int64_t k, int64_t heads, int64_t d, const I* rp,
                  const I* col, const T* val, const T* B, int64_t ldb, T* C, int64_t ldc,
                  int64_t row_begin, int64_t row_end, const Schedule& s, const T* bias, int act) {
#pragma clang fp contract(off)
  using A = typename Num<T>::acc;
  const int64_t rows = row_end - row_begin;
  bool any_neg = false;
#pragma omp parallel num_threads(nthreads) reduction(|| : any_neg)
  {
    std::vector<A> acc(d), part(d);
    bool neg = false;
#pragma omp for schedule(dynamic, 64)
    for (int64_t g = 0; g < rows; ++g) {
      const int64_t r = row_begin + g;
      const int64_t j0 = (int64_t)rp[r], j1 = (int64_t)rp[r + 1];
      const int64_t len = j1 - j0;
      for (int64_t h = 0; h < heads; ++h) {
        const T* vh = val + h;
        const T* bh = B + h * d;
        if (len <= s.split) {
          row_sum<T, I>(col, vh, heads, bh, ldb, k, d, j0, j1, acc.data(), &neg);
        } else {
          const int64_t nc = num_chunks(len, s.chunk);
          for (int64_t c = 0; c < d; ++c) acc[c] = A(0);
          for (int64_t q = 0; q < nc; ++q) {
            const int64_t a = j0 + q * s.chunk;
            const int64_t e = (q == nc - 1) ? j1 : a + s.chunk;
            row_sum<T, I>(col, vh, heads, bh, ldb, k, d, a, e, part.data(), &neg);
            for (int64_t c = 0; c < d; ++c) acc[c] = acc[c] + part[c];
          }
        }
        T* out = C + g * ldc + h * d;
        for (int64_t c = 0; c < d; ++c) out[c] = epilogue<T>(acc[c], bias, h * d + c, act);
      }
    }
    any_neg = any_neg || neg;
  }
  OFX_REQUIRE(!any_neg, OFX_EINVAL,
              "%s: negative column index (gather_kernel_util.cpp:80 CHECK_GE(idx, 0))", fn);
  return OFX_OK;
}

// The SDDMM in its order contract (csrc/spmm_backward.hip): out[j*heads + h] = the dot of
// a[r, h*d ..] and b[col[j], h*d ..] as 8-wide in-order leaves reduced by a pairwise tree.
// MASKED: d(values) of max / min, the terms of the columns nonzero j did not win
// (arg[r, c] != j) replaced by +0.  A column outside [0, k) reads the gathered zero row as the
// factor A(0).  Returns whether a column was negative (the heads entry reports it; the single-head
// entries refuse it in a pass of their own before anything is written: negative_column).
template <typename T, typename I, bool MASKED>
bool cpu_sddmm_rows(int nthreads, int64_t k, int64_t heads, int64_t d, const I* rp, const I* col,
                    const I* arg, int64_t ldarg, const T* a, int64_t lda, const T* b, int64_t ldb,
                    T* out, int64_t row_begin, int64_t row_end) {
#pragma clang fp contract(off)
  using A = typename Num<T>::acc;
  const int64_t leaves = (d + 7) / 8;
  int64_t padded = 1;
  while (padded < leaves) padded *= 2;
  bool any_neg = false;
#pragma omp parallel num_threads(nthreads) reduction(|| : any_neg)
  {
    std::vector<A> leaf(padded);
    bool neg = false;
#pragma omp for schedule(dynamic, 64)
    for (int64_t r = row_begin; r < row_end; ++r) {
      for (int64_t j = (int64_t)rp[r]; j < (int64_t)rp[r + 1]; ++j) {
        const int64_t cj = (int64_t)col[j];
        if (cj < 0) neg = true;
        for (int64_t h = 0; h < heads; ++h) {
          const T* arow = a + (r - row_begin) * lda + h * d;
          const T* brow = (uint64_t)cj < (uint64_t)k ? b + cj * ldb + h * d : nullptr;
          const I* grow = MASKED ? arg + (r - row_begin) * ldarg + h * d : nullptr;
          for (int64_t l = 0; l < padded; ++l) {
            A s = A(0);
            for (int64_t e = 8 * l; e < 8 * l + 8 && e < d; ++e) {
              A term = Num<T>::load(arow[e]) * (brow ? Num<T>::load(brow[e]) : A(0));
              if constexpr (MASKED) term = (int64_t)grow[e] == j ? term : A(0);
              s = s + term;
            }
            leaf[l] = s;
          }
          for (int64_t w = 1; w < padded; w *= 2)
            for (int64_t l = 0; l < padded; l += 2 * w) leaf[l] = leaf[l] + leaf[l + w];
          out[j * heads + h] = Num<T>::store(leaf[0]);
        }
      }
    }
    any_neg = any_neg || neg;
  }
  return any_neg;
}

// A negative column among nonzeros [j0, j1): the CPU gather's CHECK_GE(idx, 0)
// (gather_kernel_util.cpp:80), which the kCPU forward reports as OFX_EINVAL; the gradient ops
// of the same CPU operator report it the same way.
template <typename I>
bool negative_column(const I* col, int64_t j0, int64_t j1) {
  bool neg = false;
#pragma omp parallel for reduction(|| : neg) schedule(static)
  for (int64_t j = j0; j < j1; ++j) neg = neg || col[j] < 0;
  return neg;
}

}  // namespace ofx

#endif  // OFX_SPMM_ROWS_CPU_H_
