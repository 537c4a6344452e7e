// gat_softmax.h — what the HIP kernels (gat_softmax_heads.hip) and the kCPU kernels
// (gat_softmax_cpu.cpp) of ops "gat_softmax_csr_heads" / "_grad" share: the activation of a score
// and the argument checks of their C-ABI entries (contract in include/ofx_spmm.h).
// Everything after the score is the multi-head edge softmax's (edge_softmax.h).
#ifndef OFX_GAT_SOFTMAX_H_
#define OFX_GAT_SOFTMAX_H_

#include <cfloat>
#include <climits>
#include <cstdint>

#include "edge_softmax.h"
#include "graph_attention.h"
#include "ofx_internal.h"
#include "spmm_common.h"

namespace ofx {
namespace gsm {

// LeakyReLU of z = s_row + s_col: one multiply in the accumulation type on the branch that z = +-0
// and NaN take as well.
template <typename A>
OFX_HD A leaky(A z, A slope) {
#pragma clang fp contract(off)
  return z > A(0) ? z : z * slope;
}

// Its derivative, the factor of the gradient.
template <typename A>
OFX_HD A leaky_factor(A z, A slope) {
  return z > A(0) ? A(1) : slope;
}

// negative_slope as the kernels use it: converted once to the accumulation type of val_dtype
// (f64 for f64, else f32).  It must come out finite and > 0: a slope of 0 would turn the -inf of a
// masked score into NaN (-inf * 0).
static inline int check_slope(const char* fn, int val_dtype, double negative_slope) {
  const bool finite = negative_slope == negative_slope && negative_slope <= DBL_MAX;
  const bool fits = val_dtype == OFX_DT_DOUBLE ||
                    (negative_slope <= (double)FLT_MAX && (float)negative_slope > 0.0f);
  OFX_REQUIRE(finite && negative_slope > 0.0 && fits, OFX_EINVAL,
              "%s: negative_slope=%g must be finite and > 0 in the accumulation type", fn,
              negative_slope);
  return OFX_OK;
}

// Everything the forward (y, g, d_row NULL-able: grad == false) and the gradient entries refuse;
// *nothing says that there is nothing to write.  out is attn (forward) or ds (gradient).
static inline int check_gat_softmax_args(const char* fn, bool grad, int idx_dtype, int val_dtype,
                                         int64_t m, int64_t k, int64_t heads, int64_t nnz,
                                         const void* row_ptr, const void* col_idx,
                                         const void* s_row, const void* s_col,
                                         double negative_slope, const void* y, const void* g,
                                         const void* out, const void* d_row, int64_t row_begin,
                                         int64_t row_end, bool* nothing) {
  OFX_REQUIRE(heads >= 0 && (heads == 0 || nnz <= INT64_MAX / heads), OFX_EINVAL,
              "%s: bad heads=%lld for nnz=%lld", fn, (long long)heads, (long long)nnz);
  if (const int rc = check_types_sizes(fn, idx_dtype, val_dtype, m, k, 0, nnz)) return rc;
  if (const int rc = check_row_range(fn, row_begin, row_end, m)) return rc;
  if (const int rc = check_slope(fn, val_dtype, negative_slope)) return rc;
  const int64_t nrows = row_end - row_begin;
  *nothing = nrows == 0 || nnz == 0 || heads == 0;
  if (*nothing) return OFX_OK;
  OFX_REQUIRE(row_ptr && col_idx && s_row && (s_col || k == 0) && out, OFX_EINVAL,
              "%s: NULL pointer", fn);
  OFX_REQUIRE(!grad || (y && g && d_row), OFX_EINVAL, "%s: NULL pointer", fn);
  OFX_REQUIRE(nrows <= INT64_MAX / heads && k <= INT64_MAX / heads, OFX_EINVAL,
              "%s: bad heads=%lld", fn, (long long)heads);
  const uint64_t es = (uint64_t)dtype_size(val_dtype), is = (uint64_t)dtype_size(idx_dtype);
  const uint64_t h = (uint64_t)heads;
  const struct {
    const void* p;
    uint64_t bytes;
  } in[] = {{row_ptr, (uint64_t)(m + 1) * is}, {col_idx, (uint64_t)nnz * is},
            {s_row, (uint64_t)nrows * h * es},  {s_col, (uint64_t)k * h * es},
            {y, (uint64_t)nnz * h * es},        {g, (uint64_t)nnz * h * es}};
  const uint64_t ob = (uint64_t)nnz * h * es, rb = (uint64_t)nrows * h * es;
  bool alias = gat::ranges_overlap(out, ob, d_row, rb);
  for (const auto& x : in)
    alias = alias || gat::ranges_overlap(out, ob, x.p, x.bytes) ||
            gat::ranges_overlap(d_row, rb, x.p, x.bytes);
  OFX_REQUIRE(!alias, OFX_EINVAL, "%s: an output overlaps an input or the other output", fn);
  return OFX_OK;
}

}  // namespace gsm
}  // namespace ofx

#endif  // OFX_GAT_SOFTMAX_H_
