// spmm_extremum.h — what the kCPU kernels (spmm_extremum_cpu.cpp) and the HIP kernels
// (spmm_extremum*.hip) of the max / min / mean reductions share: the comparison rule, the
// degree division and the argument checks of their C-ABI entries (include/ofx_spmm.h).
#ifndef OFX_SPMM_EXTREMUM_H_
#define OFX_SPMM_EXTREMUM_H_

#include <climits>

#include "ofx_internal.h"
#include "spmm_common.h"

namespace ofx {

// Whether candidate p replaces the running best b (both in the accumulation type): strictly
// greater (max) or smaller (min), or NaN where the best is not.  Walking j upwards, the lowest j
// wins ties, +0 and -0 tie, and the first NaN wins and stays.
// Written without short-circuit operators, and used as a select by the kernels (best = take ? p :
// best): one compare chain per element, no branch per candidate.
template <typename A>
OFX_HD bool better(A p, A b, bool is_max) {
  const int cmp = is_max ? int(p > b) : int(p < b);
  const int first_nan = int(p != p) & int(b == b);
  return (cmp | first_nan) != 0;
}

// The contract's product p = Num<T>::mul(v, b) as the extremum kernels need it: with the sign of a
// zero product intact (the winner's own bits are stored, and -0 can win).  On the device the f16
// multiply and its rounding would otherwise be fused into one v_fma_mixlo_f16 with a +0 addend,
// which turns a -0 product into +0; the sum kernels never see the difference (they add the
// product to an accumulator that is never -0), so Num<f16>::mul stays as it is.
template <typename T>
OFX_HD typename Num<T>::acc signed_product(typename Num<T>::acc v, typename Num<T>::acc b) {
#if defined(__HIP_DEVICE_COMPILE__)
  if constexpr (sizeof(T) == 2 && !__is_same(T, bf16)) {
    float p = v * b;
    asm volatile("" : "+v"(p));  // keeps the multiply and the conversion two instructions
    return float(_Float16(p));
  }
#endif
  return Num<T>::mul(v, b);
}

// A NaN winner is stored as the canonical quiet NaN of its type (poison_value's bits): which NaN
// a multiply returns differs between the host's and the device's arithmetic, and the contract
// promises the same bits on both.  Every other winner keeps its own bits.
template <typename A>
OFX_HD A canonical_nan(A x) {
  return x != x ? A(__builtin_nan("")) : x;
}

// dst = store(load(src) / acc(deg)); deg == 0 gives +0 (the mean of an empty row).
template <typename T>
OFX_HD T scale_by_degree(T x, int64_t deg) {
  using A = typename Num<T>::acc;
  if (deg == 0) return Num<T>::store(A(0));
  return Num<T>::store(Num<T>::load(x) / A(deg));
}

// ---- argument checks shared by the device and host entries (on spmm_common.h's generic ones) --
static inline int check_reduce_code(int reduce, const char* fn) {
  OFX_REQUIRE(reduce == OFX_REDUCE_SUM || reduce == OFX_REDUCE_MEAN || reduce == OFX_REDUCE_MAX ||
                  reduce == OFX_REDUCE_MIN,
              OFX_EINVAL, "%s: unknown reduce code %d (OFX_REDUCE_SUM/MEAN/MAX/MIN)", fn, reduce);
  return OFX_OK;
}

static inline int check_reduce_args(const char* fn, int idx_dtype, int val_dtype, int64_t m,
                                    int64_t k, int64_t n, int64_t nnz, int64_t ldb, int64_t ldc,
                                    bool has_arg, int64_t ldarg, int64_t row_begin,
                                    int64_t row_end) {
  if (const int rc = check_types_sizes(fn, idx_dtype, val_dtype, m, k, n, nnz)) return rc;
  if (const int rc = check_row_range(fn, row_begin, row_end, m)) return rc;
  OFX_REQUIRE(ldb >= n && ldc >= n, OFX_EINVAL, "%s: ldb=%lld / ldc=%lld < n=%lld", fn,
              (long long)ldb, (long long)ldc, (long long)n);
  OFX_REQUIRE(!has_arg || ldarg >= n, OFX_EINVAL, "%s: ldarg=%lld < n=%lld", fn, (long long)ldarg,
              (long long)n);
  return OFX_OK;
}

// d(b): A is m x k, so A^T has k rows; rows [row_begin, row_end) of A^T are computed.
static inline int check_select_args(const char* fn, int idx_dtype, int val_dtype, int64_t m,
                                    int64_t k, int64_t n, int64_t nnz, int64_t ldarg, int64_t ldg,
                                    int64_t lddb, int64_t row_begin, int64_t row_end) {
  if (const int rc = check_types_sizes(fn, idx_dtype, val_dtype, m, k, n, nnz)) return rc;
  if (const int rc = check_row_range(fn, row_begin, row_end, k)) return rc;
  OFX_REQUIRE(ldarg >= n, OFX_EINVAL, "%s: ldarg=%lld < n=%lld", fn, (long long)ldarg,
              (long long)n);
  OFX_REQUIRE(ldg >= n && lddb >= n, OFX_EINVAL, "%s: ldg=%lld / lddb=%lld < n=%lld", fn,
              (long long)ldg, (long long)lddb, (long long)n);
  return OFX_OK;
}

static inline int check_sddmm_select_args(const char* fn, int idx_dtype, int val_dtype, int64_t m,
                                          int64_t k, int64_t n, int64_t nnz, int64_t ldarg,
                                          int64_t lda, int64_t ldb, int64_t row_begin,
                                          int64_t row_end) {
  if (const int rc = check_types_sizes(fn, idx_dtype, val_dtype, m, k, n, nnz)) return rc;
  if (const int rc = check_row_range(fn, row_begin, row_end, m)) return rc;
  OFX_REQUIRE(n > 0, OFX_EINVAL, "%s: n == 0 (use a zero fill)", fn);
  OFX_REQUIRE(ldarg >= n, OFX_EINVAL, "%s: ldarg=%lld < n=%lld", fn, (long long)ldarg,
              (long long)n);
  OFX_REQUIRE(lda >= n && ldb >= n, OFX_EINVAL, "%s: lda=%lld / ldb=%lld < n=%lld", fn,
              (long long)lda, (long long)ldb, (long long)n);
  return OFX_OK;
}

static inline int check_row_scale_args(const char* fn, int idx_dtype, int val_dtype, int64_t m,
                                       int64_t n, int64_t ldsrc, int64_t lddst, int64_t row_begin,
                                       int64_t row_end) {
  if (const int rc = check_types_sizes(fn, idx_dtype, val_dtype, m, 0, n, 0)) return rc;
  if (const int rc = check_row_range(fn, row_begin, row_end, m)) return rc;
  OFX_REQUIRE(ldsrc >= n && lddst >= n, OFX_EINVAL, "%s: ldsrc=%lld / lddst=%lld < n=%lld", fn,
              (long long)ldsrc, (long long)lddst, (long long)n);
  return OFX_OK;
}

}  // namespace ofx

#endif  // OFX_SPMM_EXTREMUM_H_
