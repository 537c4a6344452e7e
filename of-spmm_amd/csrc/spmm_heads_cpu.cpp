// spmm_heads_cpu.cpp — the DeviceType::kCPU kernels of ops "spmm_csr_heads" and
// "sddmm_csr_heads" (multi-head SpMM / SDDMM over a CSR; contract in include/ofx_spmm.h,
// DESIGN.md §3f).  Each head's slice is computed by the row templates spmm_cpu.cpp runs with one
// head (spmm_rows_cpu.h: the same loops, with the value read at stride H and the columns at base
// h*D), so the bits are those of the per-head composition and of the HIP kernels (spmm_heads.hip,
// sddmm_heads.hip).
#pragma clang fp contract(off)

#include <omp.h>

#include <climits>
#include <vector>

#include "ofx_internal.h"
#include "spmm_common.h"
#include "spmm_rows_cpu.h"

namespace ofx {
namespace {

int check_heads_sizes(const char* fn, int idx_dtype, int val_dtype, int64_t m, int64_t k,
                      int64_t heads, int64_t d, int64_t nnz, int64_t row_begin, int64_t row_end) {
  if (const int rc = check_heads_shape(fn, heads, d)) return rc;
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
    if ((rc = check_no_plan_options("spmm_csr_heads_cpu", opts))) return rc;
    const int64_t n = heads * d;
    OFX_REQUIRE(ldb >= n && ldc >= n, OFX_EINVAL, "spmm_csr_heads_cpu: ldb=%lld / ldc=%lld < n=%lld",
                (long long)ldb, (long long)ldc, (long long)n);
    if (row_end == row_begin || n == 0) return OFX_OK;
    OFX_REQUIRE(row_ptr && c && (nnz == 0 || (col_idx && values && b)), OFX_EINVAL,
                "spmm_csr_heads_cpu: NULL pointer");
    const Schedule s = resolve_schedule(d, opts);  // of ONE head's width: the numeric contract
    return by_types(idx_dtype, val_dtype, [&](auto* tp, auto* ip) -> int {
      using T = std::remove_pointer_t<decltype(tp)>;
      using I = std::remove_pointer_t<decltype(ip)>;
      return cpu_spmm_rows<T, I>("spmm_csr_heads_cpu", threads_of(num_threads), k, heads, d,
                                 (const I*)row_ptr, (const I*)col_idx, (const T*)values,
                                 (const T*)b, ldb, (T*)c, ldc, row_begin, row_end, s, nullptr,
                                 OFX_ACT_NONE);
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
    return by_types(idx_dtype, val_dtype, [&](auto* tp, auto* ip) -> int {
      using T = std::remove_pointer_t<decltype(tp)>;
      using I = std::remove_pointer_t<decltype(ip)>;
      const bool neg = cpu_sddmm_rows<T, I, false>(
          threads_of(num_threads), k, heads, d, (const I*)row_ptr, (const I*)col_idx, nullptr, 0,
          (const T*)a, lda, (const T*)b, ldb, (T*)out, row_begin, row_end);
      OFX_REQUIRE(!neg, OFX_EINVAL,
                  "sddmm_csr_heads_cpu: negative column index (gather_kernel_util.cpp:80 "
                  "CHECK_GE(idx, 0))");
      return OFX_OK;
    });
  });
}
