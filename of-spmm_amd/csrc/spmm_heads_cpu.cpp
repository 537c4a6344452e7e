// spmm_heads_cpu.cpp — the DeviceType::kCPU kernels of ops "spmm_csr_heads" and
// "sddmm_csr_heads" (multi-head SpMM / SDDMM over a CSR; contract in include/ofx_spmm.h,
// DESIGN.md §3f).  Each head's slice is computed exactly as spmm_cpu.cpp computes the single-head
// ops on it (the same loops, with the value read at stride H and the columns at base h*D), so the
// bits are those of the per-head composition and of the HIP kernels (spmm_heads.hip,
// sddmm_heads.hip).
#pragma clang fp contract(off)

#include <omp.h>

#include <climits>
#include <vector>

#include "ofx_internal.h"
#include "spmm_common.h"
#include "spmm_extremum.h"

namespace ofx {
namespace {

// Nonzeros [j0, j1) of one head: acc[c] = sum of mul(val[j*vs], B[col[j], c]) from +0, ascending.
// A column outside [0, k) adds val * 0 (the zero-filled gathered row); a negative one is reported.
template <typename T, typename I>
void head_row_sum(const I* col, const T* val, int64_t vs, const T* B, int64_t ldb, int64_t k,
                  int64_t d, int64_t j0, int64_t j1, typename Num<T>::acc* acc, bool* neg) {
#pragma clang fp contract(off)
  using A = typename Num<T>::acc;
  for (int64_t c = 0; c < d; ++c) acc[c] = A(0);
  for (int64_t j = j0; j < j1; ++j) {
    const A v = Num<T>::load(val[j * vs]);
    const int64_t cj = (int64_t)col[j];
    if (cj >= 0 && cj < k) {
      const T* brow = B + cj * ldb;
      for (int64_t c = 0; c < d; ++c) acc[c] = acc[c] + Num<T>::mul(v, Num<T>::load(brow[c]));
    } else {
      if (cj < 0) *neg = true;
      for (int64_t c = 0; c < d; ++c) acc[c] = acc[c] + Num<T>::mul(v, A(0));
    }
  }
}

template <typename T, typename I>
int cpu_spmm_heads(int nthreads, int64_t k, int64_t heads, int64_t d, const I* rp, const I* col,
                   const T* val, const T* B, int64_t ldb, T* C, int64_t ldc, int64_t row_begin,
                   int64_t row_end, const Schedule& s) {
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
          head_row_sum<T, I>(col, vh, heads, bh, ldb, k, d, j0, j1, acc.data(), &neg);
        } else {
          const int64_t nc = num_chunks(len, s.chunk);
          for (int64_t c = 0; c < d; ++c) acc[c] = A(0);
          for (int64_t q = 0; q < nc; ++q) {
            const int64_t a = j0 + q * s.chunk;
            const int64_t e = (q == nc - 1) ? j1 : a + s.chunk;
            head_row_sum<T, I>(col, vh, heads, bh, ldb, k, d, a, e, part.data(), &neg);
            for (int64_t c = 0; c < d; ++c) acc[c] = acc[c] + part[c];
          }
        }
        T* out = C + g * ldc + h * d;
        for (int64_t c = 0; c < d; ++c) out[c] = Num<T>::store(acc[c]);
      }
    }
    any_neg = any_neg || neg;
  }
  OFX_REQUIRE(!any_neg, OFX_EINVAL,
              "spmm_csr_heads_cpu: negative column index (gather_kernel_util.cpp:80 "
              "CHECK_GE(idx, 0))");
  return OFX_OK;
}

// out[j*H + h] in ofx_sddmm_csr's order within the head.
template <typename T, typename I>
int cpu_sddmm_heads(int nthreads, int64_t k, int64_t heads, int64_t d, const I* rp, const I* col,
                    const T* a, int64_t lda, const T* b, int64_t ldb, T* out, int64_t row_begin,
                    int64_t row_end) {
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
          for (int64_t l = 0; l < padded; ++l) {
            A s = A(0);
            for (int64_t e = 8 * l; e < 8 * l + 8 && e < d; ++e)
              s = s + Num<T>::load(arow[e]) * (brow ? Num<T>::load(brow[e]) : A(0));
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
  OFX_REQUIRE(!any_neg, OFX_EINVAL,
              "sddmm_csr_heads_cpu: negative column index (gather_kernel_util.cpp:80 "
              "CHECK_GE(idx, 0))");
  return OFX_OK;
}

int check_heads_sizes(const char* fn, int idx_dtype, int val_dtype, int64_t m, int64_t k,
                      int64_t heads, int64_t d, int64_t nnz, int64_t row_begin, int64_t row_end) {
  OFX_REQUIRE(heads >= 0 && d >= 0 && (d == 0 || heads <= INT64_MAX / d), OFX_EINVAL,
              "%s: bad heads=%lld / d=%lld", fn, (long long)heads, (long long)d);
  if (const int rc = check_types_sizes(fn, idx_dtype, val_dtype, m, k, heads * d, nnz)) return rc;
  return check_row_range(fn, row_begin, row_end, m);
}

}  // namespace
}  // namespace ofx

using namespace ofx;

extern "C" int ofx_spmm_csr_heads_cpu(int num_threads, int idx_dtype, int val_dtype, int64_t m,
                                      int64_t k, int64_t heads, int64_t d, int64_t nnz,
                                      const void* row_ptr, const void* col_idx, const void* values,
                                      const void* b, int64_t ldb, void* c, int64_t ldc,
                                      int64_t row_begin, int64_t row_end,
                                      const ofx_spmm_options* opts) {
  return ::ofx::guarded(__func__, [&]() -> int {
    OFX_READ_OPTIONS(opts, "spmm_csr_heads_cpu");
    int rc = check_heads_sizes("spmm_csr_heads_cpu", idx_dtype, val_dtype, m, k, heads, d, nnz,
                               row_begin, row_end);
    if (rc) return rc;
    OFX_REQUIRE(opts->planned == 0 && opts->variant == 0, OFX_EINVAL,
                "spmm_csr_heads_cpu: options planned=%d / variant=%d are not supported (plan-once "
                "and the tuning variants belong to spmm_csr)", (int)opts->planned,
                (int)opts->variant);
    const int64_t n = heads * d;
    OFX_REQUIRE(ldb >= n && ldc >= n, OFX_EINVAL, "spmm_csr_heads_cpu: ldb=%lld / ldc=%lld < n=%lld",
                (long long)ldb, (long long)ldc, (long long)n);
    if (row_end == row_begin || n == 0) return OFX_OK;
    OFX_REQUIRE(row_ptr && c && (nnz == 0 || (col_idx && values && b)), OFX_EINVAL,
                "spmm_csr_heads_cpu: NULL pointer");
    const int nt = num_threads > 0 ? num_threads : omp_get_max_threads();
    const Schedule s = resolve_schedule(d, opts);  // of ONE head's width: the numeric contract
    return by_types(idx_dtype, val_dtype, [&](auto* tp, auto* ip) -> int {
      using T = std::remove_pointer_t<decltype(tp)>;
      using I = std::remove_pointer_t<decltype(ip)>;
      return cpu_spmm_heads<T, I>(nt, k, heads, d, (const I*)row_ptr, (const I*)col_idx,
                                  (const T*)values, (const T*)b, ldb, (T*)c, ldc, row_begin,
                                  row_end, s);
    });
  });
}

extern "C" int ofx_sddmm_csr_heads_cpu(int num_threads, int idx_dtype, int val_dtype, int64_t m,
                                       int64_t k, int64_t heads, int64_t d, int64_t nnz,
                                       const void* row_ptr, const void* col_idx, const void* a,
                                       int64_t lda, const void* b, int64_t ldb, void* out,
                                       int64_t row_begin, int64_t row_end) {
  return ::ofx::guarded(__func__, [&]() -> int {
    int rc = check_heads_sizes("sddmm_csr_heads_cpu", idx_dtype, val_dtype, m, k, heads, d, nnz,
                               row_begin, row_end);
    if (rc) return rc;
    const int64_t n = heads * d;
    OFX_REQUIRE(lda >= n && ldb >= n, OFX_EINVAL,
                "sddmm_csr_heads_cpu: lda=%lld / ldb=%lld < n=%lld", (long long)lda,
                (long long)ldb, (long long)n);
    if (row_end == row_begin || nnz == 0 || heads == 0) return OFX_OK;
    OFX_REQUIRE(d > 0, OFX_EINVAL, "sddmm_csr_heads_cpu: d == 0 (use a zero fill)");
    OFX_REQUIRE(d <= 2048, OFX_EUNSUPPORTED, "sddmm_csr_heads_cpu: d=%lld > 2048 is not supported",
                (long long)d);
    OFX_REQUIRE(row_ptr && col_idx && out && a && b, OFX_EINVAL, "sddmm_csr_heads_cpu: NULL pointer");
    const int nt = num_threads > 0 ? num_threads : omp_get_max_threads();
    return by_types(idx_dtype, val_dtype, [&](auto* tp, auto* ip) -> int {
      using T = std::remove_pointer_t<decltype(tp)>;
      using I = std::remove_pointer_t<decltype(ip)>;
      return cpu_sddmm_heads<T, I>(nt, k, heads, d, (const I*)row_ptr, (const I*)col_idx,
                                   (const T*)a, lda, (const T*)b, ldb, (T*)out, row_begin, row_end);
    });
  });
}
