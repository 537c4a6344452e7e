// spmm_multi.h — what the HIP kernels (spmm_multi.hip) and the kCPU kernel (spmm_multi_cpu.cpp) of
// op "spmm_csr_multi" share: the aggregator mask and its slices, the statistics one gathered
// product feeds, the one finishing step from the moments to sum / mean / var / std, and the
// argument checks of the C-ABI entries (contract in include/ofx_spmm.h).
#ifndef OFX_SPMM_MULTI_H_
#define OFX_SPMM_MULTI_H_

#include <climits>
#include <cstdint>

#include "ofx_internal.h"
#include "spmm_common.h"
#include "spmm_extremum.h"

namespace ofx {
namespace multi {

constexpr int kAllAggrs = OFX_AGGR_SUM | OFX_AGGR_MEAN | OFX_AGGR_MAX | OFX_AGGR_MIN |
                          OFX_AGGR_VAR | OFX_AGGR_STD;

// What a launch tracks, the two compile-time choices of the kernels: the moments (0: none, 1: s1,
// 2: s1 and s2) and the extrema (none or both: a request for max alone tracks both, stores one).
OFX_HD int moments_of(int mask) {
  if (mask & (OFX_AGGR_VAR | OFX_AGGR_STD)) return 2;
  return (mask & (OFX_AGGR_SUM | OFX_AGGR_MEAN)) ? 1 : 0;
}
OFX_HD bool extrema_of(int mask) { return (mask & (OFX_AGGR_MAX | OFX_AGGR_MIN)) != 0; }

// The output slice of aggregator `bit`: the requested aggregators in ascending bit order.
OFX_HD int slice_of(int mask, int bit) { return __builtin_popcount(mask & (bit - 1)); }
OFX_HD int num_slices(int mask) { return __builtin_popcount(mask & kAllAggrs); }

// The outputs of a launch: the slice of each requested aggregator (rows of ldc elements; NULL: not
// requested), the optional args (rows of ldarg) and eps in the accumulation type.
template <typename T, typename I>
struct Outputs {
  T *sum, *mean, *mx, *mn, *var, *sd;
  int64_t ldc;
  I *arg_max, *arg_min;
  int64_t ldarg;
  typename Num<T>::acc eps;
  int mask;
};

template <typename T, typename I>
OFX_HD Outputs<T, I> outputs_of(int mask, void* c, int64_t ldc, int64_t slice_stride, void* arg_max,
                         void* arg_min, int64_t ldarg, double eps) {
  const auto at = [&](int bit) -> T* {
    return (mask & bit) ? static_cast<T*>(c) + slice_of(mask, bit) * slice_stride : nullptr;
  };
  return {at(OFX_AGGR_SUM), at(OFX_AGGR_MEAN), at(OFX_AGGR_MAX), at(OFX_AGGR_MIN),
          at(OFX_AGGR_VAR), at(OFX_AGGR_STD), ldc, static_cast<I*>(arg_max),
          static_cast<I*>(arg_min), ldarg, (typename Num<T>::acc)eps, mask};
}

// The statistics of one (row or chunk, column): the moments from +0, the running extrema with the
// global j of each (-1: none yet).
template <typename A, typename J>
struct Stats {
  A s1, s2, mx, mn;
  J amax, amin;
};

template <typename A, typename J>
OFX_HD Stats<A, J> empty_stats() {
  return {A(0), A(0), A(0), A(0), J(-1), J(-1)};
}

// One product p (rounded to T, in the accumulation type) of nonzero j: added to s1, its square
// (formed in the accumulation type, not rounded to T) to s2, and offered to both extrema by the
// strict rule of spmm_extremum.h.  MOM / EXT: what the caller tracks; the rest is left alone.
template <int MOM, bool EXT, typename A, typename J>
OFX_HD void feed(Stats<A, J>& s, A p, J j) {
#pragma clang fp contract(off)
  if constexpr (MOM >= 1) s.s1 = s.s1 + p;
  if constexpr (MOM >= 2) s.s2 = s.s2 + p * p;
  if constexpr (EXT) {
    const bool tmax = (int(s.amax < 0) | int(better(p, s.mx, true))) != 0;
    const bool tmin = (int(s.amin < 0) | int(better(p, s.mn, false))) != 0;
    s.mx = tmax ? p : s.mx;
    s.amax = tmax ? j : s.amax;
    s.mn = tmin ? p : s.mn;
    s.amin = tmin ? j : s.amin;
  }
}

// A later chunk's statistics q merged into s, in chunk order: the partial moments added, the
// extrema merged by the same strict rule (every chunk holds at least one nonzero).
template <typename A, typename J>
OFX_HD void merge(Stats<A, J>& s, const Stats<A, J>& q) {
#pragma clang fp contract(off)
  s.s1 = s.s1 + q.s1;
  s.s2 = s.s2 + q.s2;
  const bool tmax = better(q.mx, s.mx, true), tmin = better(q.mn, s.mn, false);
  s.mx = tmax ? q.mx : s.mx;
  s.amax = tmax ? q.amax : s.amax;
  s.mn = tmin ? q.mn : s.mn;
  s.amin = tmin ? q.amin : s.amin;
}

// The finishing step, the one definition the main kernel (ordinary rows), the hub combine and the
// kCPU kernel call: the elements of the slices in `mask` from the statistics of one (row, column)
// and the row's degree; the others are left unset.
//   sum  = store(s1)                    mean = scale_by_degree(store(s1), deg)
//   var  = store(max(s2 / deg - (s1 / deg)^2, +0)), +0 for deg = 0; a NaN propagates (canonical)
//   std  = store(sqrt(var + eps)) from the unrounded var
//   max / min: the winner's own bits, a NaN canonical; +0 for an empty row
// The division and the square root are IEEE's correctly rounded ones on host and device.
template <typename T>
struct Finished {
  T sum, mean, mx, mn, var, sd;
};

template <typename T, typename J>
OFX_HD Finished<T> finish(const Stats<typename Num<T>::acc, J>& s, int64_t deg,
                          typename Num<T>::acc eps, int mask) {
#pragma clang fp contract(off)
  using A = typename Num<T>::acc;
  Finished<T> f{};
  if (mask & (OFX_AGGR_SUM | OFX_AGGR_MEAN)) {
    f.sum = Num<T>::store(s.s1);
    if (mask & OFX_AGGR_MEAN) f.mean = scale_by_degree<T>(f.sum, deg);
  }
  if (mask & OFX_AGGR_MAX) f.mx = Num<T>::store(canonical_nan(s.mx));
  if (mask & OFX_AGGR_MIN) f.mn = Num<T>::store(canonical_nan(s.mn));
  if (mask & (OFX_AGGR_VAR | OFX_AGGR_STD)) {
    A var = A(0);
    if (deg > 0) {
      const A mu = s.s1 / A(deg);
      const A v = s.s2 / A(deg) - mu * mu;
      var = canonical_nan(v < A(0) ? A(0) : v);
    }
    f.var = Num<T>::store(var);
    if (mask & OFX_AGGR_STD) {
      A sd;
      if constexpr (sizeof(A) == 8)
        sd = __builtin_sqrt(var + eps);
      else
        sd = __builtin_sqrtf(var + eps);
      f.sd = Num<T>::store(canonical_nan(sd));
    }
  }
  return f;
}

// ---- argument checks shared by the device and host entries ---------------------------------------
static inline int check_multi_sizes(const char* fn, int idx_dtype, int val_dtype, int64_t m,
                                    int64_t k, int64_t n, int64_t nnz, int aggr_mask) {
  if (const int rc = check_types_sizes(fn, idx_dtype, val_dtype, m, k, n, nnz)) return rc;
  OFX_REQUIRE(aggr_mask != 0 && (aggr_mask & ~kAllAggrs) == 0, OFX_EINVAL,
              "%s: aggr_mask=%d is empty or has unknown bits (OFX_AGGR_*)", fn, aggr_mask);
  return OFX_OK;
}

// *nothing: no element to write.
static inline int check_multi_args(const char* fn, int idx_dtype, int val_dtype, int64_t m,
                                   int64_t k, int64_t n, int64_t nnz, const void* row_ptr,
                                   const void* col_idx, const void* values, const void* b,
                                   int64_t ldb, int aggr_mask, double eps, const void* c,
                                   int64_t ldc, int64_t slice_stride, const void* arg_max,
                                   const void* arg_min, int64_t ldarg, int64_t row_begin,
                                   int64_t row_end, bool* nothing) {
  if (const int rc = check_multi_sizes(fn, idx_dtype, val_dtype, m, k, n, nnz, aggr_mask))
    return rc;
  OFX_REQUIRE((arg_max == nullptr || (aggr_mask & OFX_AGGR_MAX)) &&
                  (arg_min == nullptr || (aggr_mask & OFX_AGGR_MIN)),
              OFX_EINVAL, "%s: arg_max / arg_min without max / min in aggr_mask=%d", fn, aggr_mask);
  const bool has_arg = arg_max != nullptr || arg_min != nullptr;
  if (const int rc = check_row_range(fn, row_begin, row_end, m)) return rc;
  OFX_REQUIRE(eps >= 0.0 && eps <= 1.79769313486231570e308, OFX_EINVAL,
              "%s: eps=%g should be finite and >= 0", fn, eps);
  OFX_REQUIRE(ldb >= n && ldc >= n && (!has_arg || ldarg >= n), OFX_EINVAL,
              "%s: a leading dimension is smaller than n=%lld", fn, (long long)n);
  OFX_REQUIRE(num_slices(aggr_mask) == 1 || slice_stride >= n || slice_stride <= -n, OFX_EINVAL,
              "%s: slice_stride=%lld is smaller than n=%lld", fn, (long long)slice_stride,
              (long long)n);
  *nothing = row_end == row_begin || n == 0;
  if (*nothing) return OFX_OK;
  OFX_REQUIRE(row_ptr && c, OFX_EINVAL, "%s: NULL row_ptr or output", fn);
  OFX_REQUIRE(nnz == 0 || (col_idx && values && (b || k == 0)), OFX_EINVAL,
              "%s: NULL col_idx / values / b with nnz=%lld", fn, (long long)nnz);
  return OFX_OK;
}

}  // namespace multi
}  // namespace ofx

#endif  // OFX_SPMM_MULTI_H_
