// gatv2_scores.h — what the HIP kernels (gatv2_scores_heads.hip, gatv2_scores_grad.hip) and the
// kCPU kernels (gatv2_scores_cpu.cpp) of ops "gatv2_scores_csr_heads" / "_grad" share: the
// activated, rounded element of the score and the argument checks of their C-ABI entries (contract
// in include/ofx_spmm.h).  The activation and the slope's check are the GAT
// softmax's (gat_softmax.h).
#ifndef OFX_GATV2_SCORES_H_
#define OFX_GATV2_SCORES_H_

#include <climits>
#include <cstdint>
#include <type_traits>

#include "gat_softmax.h"
#include "graph_attention.h"
#include "ofx_internal.h"
#include "spmm_common.h"

namespace ofx {
namespace gv2 {

constexpr int64_t kMaxD = gat::kMaxD;  // the SDDMM's widest head

// x rounded to T as a step of its own, back in the accumulation type.  For f16 the value is made
// opaque to the device compiler first: left to itself it folds the multiply that produced x into
// the conversion (v_fma_mixlo_f16: the exact product rounded once to f16), where the contract
// rounds the product to f32 and then to f16 as the host does.
template <typename T>
OFX_HD typename Num<T>::acc rounded(typename Num<T>::acc x) {
#if defined(__HIP_DEVICE_COMPILE__)
  if constexpr (std::is_same<T, f16>::value) asm("" : "+v"(x));
#endif
  return Num<T>::load(Num<T>::store(x));
}

// U[j, n] as the dot product and T2 read it: LeakyReLU(z) rounded to T.
template <typename T>
OFX_HD typename Num<T>::acc activated(typename Num<T>::acc z, typename Num<T>::acc slope) {
#pragma clang fp contract(off)
  return rounded<T>(gsm::leaky(z, slope));
}

// A strided [rows, n] tensor's extent in bytes.
static inline uint64_t extent(int64_t rows, int64_t ld, int64_t n, uint64_t es) {
  return rows <= 0 || n <= 0 ? 0 : ((uint64_t)(rows - 1) * (uint64_t)ld + (uint64_t)n) * es;
}

// Everything the forward (grad == false: `de` unused, out = e [nnz, heads], p NULL) and the
// gradient entries (out = d_x [nrows, n] with ldo, p NULL-able with ldp) refuse; *nothing says
// that there is nothing to write.
static inline int check_gatv2_args(const char* fn, bool grad, int idx_dtype, int val_dtype,
                                   int64_t m, int64_t k, int64_t heads, int64_t d, int64_t nnz,
                                   const void* row_ptr, const void* col_idx, const void* x_row,
                                   int64_t ldr, const void* x_col, int64_t ldc, const void* att,
                                   double negative_slope, const void* de, const void* out,
                                   int64_t ldo, const void* p, int64_t ldp, int64_t row_begin,
                                   int64_t row_end, const ofx_spmm_options* opts, bool* nothing) {
  if (const int rc = check_heads_shape(fn, heads, d)) return rc;
  if (const int rc = check_types_sizes(fn, idx_dtype, val_dtype, m, k, heads * d, nnz)) return rc;
  OFX_REQUIRE(heads == 0 || nnz <= INT64_MAX / heads, OFX_EINVAL, "%s: bad heads=%lld for nnz=%lld",
              fn, (long long)heads, (long long)nnz);
  if (const int rc = grad ? check_no_plan_options(fn, opts) : OFX_OK) return rc;
  if (const int rc = check_row_range(fn, row_begin, row_end, m)) return rc;
  if (const int rc = gsm::check_slope(fn, val_dtype, negative_slope)) return rc;
  const int64_t n = heads * d, nrows = row_end - row_begin;
  OFX_REQUIRE(ldr >= n && ldc >= n && (!grad || (ldo >= n && (p == nullptr || ldp >= n))),
              OFX_EINVAL, "%s: a leading dimension is smaller than n=%lld", fn, (long long)n);
  *nothing = grad ? (nrows == 0 || n == 0) : (nrows == 0 || nnz == 0 || heads == 0);
  if (*nothing) return OFX_OK;
  OFX_REQUIRE(d > 0, OFX_EINVAL, "%s: d == 0 (use a zero fill)", fn);
  OFX_REQUIRE(d <= kMaxD, OFX_EUNSUPPORTED, "%s: d=%lld > %lld is not supported", fn, (long long)d,
              (long long)kMaxD);
  OFX_REQUIRE(row_ptr && out && x_row && att, OFX_EINVAL, "%s: NULL pointer", fn);
  OFX_REQUIRE(nnz == 0 || (col_idx && (x_col || k == 0) && (!grad || de)), OFX_EINVAL,
              "%s: NULL pointer with nnz=%lld", fn, (long long)nnz);
  const uint64_t es = (uint64_t)dtype_size(val_dtype), is = (uint64_t)dtype_size(idx_dtype);
  const struct {
    const void* ptr;
    uint64_t bytes;
  } in[] = {{row_ptr, (uint64_t)(m + 1) * is},
            {col_idx, (uint64_t)nnz * is},
            {x_row, extent(nrows, ldr, n, es)},
            {x_col, extent(k, ldc, n, es)},
            {att, (uint64_t)n * es},
            {grad ? de : nullptr, (uint64_t)nnz * (uint64_t)heads * es}};
  const uint64_t ob = grad ? extent(nrows, ldo, n, es) : (uint64_t)nnz * (uint64_t)heads * es;
  const uint64_t pb = extent(nrows, ldp, n, es);
  bool alias = gat::ranges_overlap(out, ob, p, pb);
  for (const auto& x : in)
    alias = alias || gat::ranges_overlap(out, ob, x.ptr, x.bytes) ||
            gat::ranges_overlap(p, pb, x.ptr, x.bytes);
  OFX_REQUIRE(!alias, OFX_EINVAL, "%s: an output overlaps an input or the other output", fn);
  return OFX_OK;
}

}  // namespace gv2
}  // namespace ofx

#endif  // OFX_GATV2_SCORES_H_
