// row_topk.h — what the kCPU kernel (row_topk_cpu.cpp) and the HIP kernels (row_topk.hip) of the
// per-row top-k selection share: the key of a value, the row classes, the check of a row and the
// argument checks of the C-ABI entries (contract in include/ofx_spmm.h).
//
// A value is compared through its bit pattern alone: the key flips every bit of a negative value
// and the sign bit of any other one, so that keys compared as unsigned integers order
//   -NaN < -inf < ... < -0 < +0 < ... < +inf < +NaN
// and `largest = false` complements the key.  A row keeps its min(deg, k) largest keys, equal keys
// by ascending position, and reports the kept positions in ascending order.  Integers only.
#ifndef OFX_ROW_TOPK_H_
#define OFX_ROW_TOPK_H_

#include <climits>

#include "node_subgraph.h"  // nsg::row_ok: the same rule for a row's entry range
#include "ofx_internal.h"
#include "spmm_common.h"

namespace ofx {
namespace rtk {

// The row classes of the device path, by degree: a group of kNarrowGroup lanes with up to kSlots
// keys per lane, a whole wave with up to kSlots keys per lane, a block per row above that (the hub
// split of the SpMM).
constexpr int kSlots = 8;
constexpr int kNarrowGroup = 8;
constexpr int kNarrowMax = kNarrowGroup * kSlots;  // 64
constexpr int kWaveMax = 64 * kSlots;              // 512

// The key of the value whose bits are `bits` (U: uint16_t, uint32_t or uint64_t); flip is 0 for
// the largest keys and ~0 for the smallest.
template <typename U>
OFX_HD U key_of(U bits, U flip) {
  constexpr U kSign = (U)((U)1 << (8 * sizeof(U) - 1));
  return (U)(bits ^ ((bits & kSign) != 0 ? (U)~(U)0 : kSign) ^ flip);
}

// The unsigned integer of a value dtype's width, as a null pointer: f((uint32_t*)nullptr) ...
template <typename F>
int by_key(int val_dtype, F&& f) {
  switch (val_dtype) {
    case OFX_DT_FLOAT: return f((uint32_t*)nullptr);
    case OFX_DT_DOUBLE: return f((uint64_t*)nullptr);
    default: return f((uint16_t*)nullptr);
  }
}

// k as the kernels use it: no row holds 2^31 entries.
static inline int clamp_k(int64_t k) { return k > (int64_t)INT32_MAX ? INT32_MAX : (int)k; }

// The checks every entry shares (host): the sizes.
static inline int check_topk_sizes(const char* fn, int idx_dtype, int64_t m, int64_t nnz) {
  OFX_REQUIRE(is_index_dtype(idx_dtype), OFX_EUNSUPPORTED, "%s: index dtype %d is not int32/int64",
              fn, idx_dtype);
  OFX_REQUIRE(m >= 0 && m <= (int64_t)INT32_MAX, OFX_EINVAL, "%s: m %lld is not in [0, 2^31)", fn,
              (long long)m);
  OFX_REQUIRE(nnz >= 0 && nnz <= (int64_t)INT32_MAX, OFX_EINVAL, "%s: nnz %lld is not in [0, 2^31)",
              fn, (long long)nnz);
  return OFX_OK;
}

// The sizes, then k, the value dtype and the pointers.
static inline int check_topk_args(const char* fn, int idx_dtype, int val_dtype, int64_t m,
                                  int64_t nnz, const void* row_ptr, const void* col_idx,
                                  const void* values, int64_t k, const void* out_row_ptr,
                                  const void* out_col_idx, const void* out_nnz) {
  const int rc = check_topk_sizes(fn, idx_dtype, m, nnz);
  if (rc) return rc;
  OFX_REQUIRE(is_value_dtype(val_dtype), OFX_EUNSUPPORTED,
              "%s: value dtype %d is not float/double/float16/bfloat16", fn, val_dtype);
  OFX_REQUIRE(k >= 1, OFX_EINVAL, "%s: k %lld is not >= 1", fn, (long long)k);
  OFX_REQUIRE(row_ptr && out_row_ptr && out_nnz, OFX_EINVAL, "%s: NULL pointer", fn);
  OFX_REQUIRE(nnz == 0 || m == 0 || (col_idx && values && out_col_idx), OFX_EINVAL,
              "%s: NULL pointer", fn);
  return OFX_OK;
}

}  // namespace rtk
}  // namespace ofx

#endif  // OFX_ROW_TOPK_H_
