// spgemm.h — what the kCPU kernel (spgemm_cpu.cpp) and the HIP kernels (spgemm.hip) of the
// CSR x CSR product share: the row classes of the device path, the bits of the bad flag and the
// argument checks of the C-ABI entries (contract in include/ofx_spmm.h).
//
// C = A * B with A [m, k] and B [k, n], both CSR.  Row i of C holds, strictly ascending, the
// distinct columns c that some entry p of A's row i reaches through B's row col_a[p]; its value is
// the chain ((+0 + t_1) + t_2) + ... over ascending p, then ascending q, of t = a_p * b_q rounded to
// the value type, summed in Num<T>::acc and rounded once.  A column of A at or above k selects a
// zero row; B's rows are strictly ascending in [0, n), so one B row never names a column twice.
#ifndef OFX_SPGEMM_H_
#define OFX_SPGEMM_H_

#include <climits>

#include "node_subgraph.h"  // nsg::row_ok: the same rule for a row's entry range
#include "ofx_internal.h"
#include "spmm_common.h"

namespace ofx {
namespace spg {

// The row classes of the device path, by ub_i = the sum of B's row lengths over A's row i (an
// upper bound of the row's distinct columns): a group of 8 lanes, a wave, a block, and the block
// sweeping column ranges for the rows above.  A class's hash table holds twice its bound.  No
// output bit depends on these numbers.
constexpr int kNarrowMax = 32;
constexpr int kWaveMax = 512;
constexpr int kBlockMax = 2048;
constexpr int kClasses = 4;  // narrow, wave, block, hub

OFX_HD int class_of(int64_t ub) {
  return ub <= kNarrowMax ? 0 : ub <= kWaveMax ? 1 : ub <= kBlockMax ? 2 : 3;
}

// The bits of the device bad flag.
constexpr unsigned kBadOutside = 1u;    // a row's entry range, a negative column of A, a column of
                                        // B outside [0, n)
constexpr unsigned kBadAscending = 2u;  // a row of B that is not strictly ascending

// The checks every entry shares (host): the sizes.
static inline int check_spgemm_sizes(const char* fn, int idx_dtype, int64_t m, int64_t k, int64_t n,
                                     int64_t nnz_a, int64_t nnz_b) {
  OFX_REQUIRE(is_index_dtype(idx_dtype), OFX_EUNSUPPORTED, "%s: index dtype %d is not int32/int64",
              fn, idx_dtype);
  const int64_t top = (int64_t)INT32_MAX;
  OFX_REQUIRE(m >= 0 && m <= top && k >= 0 && k <= top && n >= 0 && n <= top, OFX_EINVAL,
              "%s: m %lld, k %lld, n %lld: a size is not in [0, 2^31)", fn, (long long)m,
              (long long)k, (long long)n);
  OFX_REQUIRE(nnz_a >= 0 && nnz_a <= top && nnz_b >= 0 && nnz_b <= top, OFX_EINVAL,
              "%s: nnz_a %lld, nnz_b %lld: a count is not in [0, 2^31)", fn, (long long)nnz_a,
              (long long)nnz_b);
  return OFX_OK;
}

// The sizes, then the pointers of a counting entry.
static inline int check_count_args(const char* fn, int idx_dtype, int64_t m, int64_t k, int64_t n,
                                   int64_t nnz_a, int64_t nnz_b, const void* rp_a, const void* ci_a,
                                   const void* rp_b, const void* ci_b, const void* out_row_ptr,
                                   const void* out_nnz) {
  const int rc = check_spgemm_sizes(fn, idx_dtype, m, k, n, nnz_a, nnz_b);
  if (rc) return rc;
  OFX_REQUIRE(rp_a && rp_b && out_row_ptr && out_nnz, OFX_EINVAL, "%s: NULL pointer", fn);
  OFX_REQUIRE((nnz_a == 0 || ci_a) && (nnz_b == 0 || ci_b), OFX_EINVAL, "%s: NULL pointer", fn);
  return OFX_OK;
}

// The sizes, then the value dtype, nnz_c and the pointers of a filling entry.  The three value
// pointers are all given or all NULL (pattern only).
static inline int check_fill_args(const char* fn, int idx_dtype, int val_dtype, int64_t m, int64_t k,
                                  int64_t n, int64_t nnz_a, int64_t nnz_b, int64_t nnz_c,
                                  const void* rp_a, const void* ci_a, const void* va,
                                  const void* rp_b, const void* ci_b, const void* vb,
                                  const void* rp_c, const void* out_col, const void* out_values) {
  const int rc = check_spgemm_sizes(fn, idx_dtype, m, k, n, nnz_a, nnz_b);
  if (rc) return rc;
  OFX_REQUIRE(is_value_dtype(val_dtype), OFX_EUNSUPPORTED,
              "%s: value dtype %d is not float/double/float16/bfloat16", fn, val_dtype);
  OFX_REQUIRE(nnz_c >= 0 && nnz_c <= (int64_t)INT32_MAX, OFX_EINVAL,
              "%s: nnz_c %lld is not in [0, 2^31)", fn, (long long)nnz_c);
  OFX_REQUIRE(rp_a && rp_b && rp_c, OFX_EINVAL, "%s: NULL pointer", fn);
  OFX_REQUIRE((nnz_a == 0 || ci_a) && (nnz_b == 0 || ci_b) && (nnz_c == 0 || out_col), OFX_EINVAL,
              "%s: NULL pointer", fn);
  const bool pattern = va == nullptr && vb == nullptr && out_values == nullptr;
  OFX_REQUIRE(pattern || ((nnz_a == 0 || va) && (nnz_b == 0 || vb) && (nnz_c == 0 || out_values)),
              OFX_EINVAL, "%s: values_a, values_b and out_values are all given or all NULL", fn);
  return OFX_OK;
}

}  // namespace spg
}  // namespace ofx

#endif  // OFX_SPGEMM_H_
