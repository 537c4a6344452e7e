// spmm_edge.h — what the HIP kernels (spmm_edge.hip, spmm_edge_grad.hip) and the kCPU kernels
// (spmm_edge_cpu.cpp) of ops "spmm_csr_edge" / "_grad_e" / "_grad_b" share: the message of one
// nonzero and feature, its gradient terms, the (op, act) dispatch and the argument checks of their
// C-ABI entries (contract in include/ofx_spmm.h).
#ifndef OFX_SPMM_EDGE_H_
#define OFX_SPMM_EDGE_H_

#include <climits>
#include <cstdint>
#include <initializer_list>
#include <type_traits>

#include "gatv2_scores.h"     // rounded, extent
#include "graph_attention.h"  // ranges_overlap
#include "ofx_internal.h"
#include "spmm_common.h"

namespace ofx {
namespace edge {

// t: b op e in the accumulation type (one operation, no FMA), rounded to T as a step of its own
// (for mul: the rounding ofx_spmm_csr gives its product), back in the accumulation type.
template <typename T, int OP>
OFX_HD typename Num<T>::acc combined(typename Num<T>::acc b, typename Num<T>::acc e) {
#pragma clang fp contract(off)
  if constexpr (OP == OFX_EDGE_MUL) return Num<T>::mul(b, e);
  return gv2::rounded<T>(b + e);
}

// The forward's summand: t, or relu(t) (t <= 0 becomes +0, -0 included; NaN stays NaN).
template <typename T, int OP, bool RELU>
OFX_HD typename Num<T>::acc message(typename Num<T>::acc b, typename Num<T>::acc e) {
  using A = typename Num<T>::acc;
  const A t = combined<T, OP>(b, e);
  if constexpr (RELU) return t <= A(0) ? A(0) : t;
  return t;
}

// One element of a gradient: the upstream dy passed on (add) or multiplied by the other factor
// (mul: b for de, e for G) and rounded to T; +0 where the relu's mask (t > 0, t formed again; a NaN
// masks) is off.
template <typename T, int OP, bool RELU>
OFX_HD T grad_term(T dy, typename Num<T>::acc other, typename Num<T>::acc b,
                   typename Num<T>::acc e) {
#pragma clang fp contract(off)
  using A = typename Num<T>::acc;
  if constexpr (RELU) {
    if (!(combined<T, OP>(b, e) > A(0))) return Num<T>::store(A(0));
  }
  if constexpr (OP == OFX_EDGE_MUL) return Num<T>::store(Num<T>::load(dy) * other);
  return dy;
}

// Which operands a gradient kernel reads: e for the mask or as mul's factor in G; b for the mask or
// as mul's factor in de.
constexpr bool grad_e_needs_b(int op, bool relu) { return relu || op == OFX_EDGE_MUL; }
constexpr bool grad_e_needs_e(int, bool relu) { return relu; }
constexpr bool grad_b_needs_e(int op, bool relu) { return relu || op == OFX_EDGE_MUL; }

// f(std::integral_constant<int, OP>, std::bool_constant<RELU>) for checked codes.
template <typename F>
int by_op_act(int op, int act, F&& f) {
  using Mul = std::integral_constant<int, OFX_EDGE_MUL>;
  using Add = std::integral_constant<int, OFX_EDGE_ADD>;
  if (op == OFX_EDGE_MUL)
    return act == OFX_ACT_RELU ? f(Mul{}, std::true_type{}) : f(Mul{}, std::false_type{});
  return act == OFX_ACT_RELU ? f(Add{}, std::true_type{}) : f(Add{}, std::false_type{});
}

// The size part of every entry's checks (all a workspace query checks); `rows`: the rows of the
// CSR the entry walks (m, or k for d(b)'s transposed one).
static inline int check_edge_sizes(const char* fn, int idx_dtype, int val_dtype, int64_t m,
                                   int64_t k, int64_t n, int64_t nnz,
                                   const ofx_spmm_options* opts) {
  if (const int rc = check_types_sizes(fn, idx_dtype, val_dtype, m, k, n, nnz)) return rc;
  OFX_REQUIRE(n == 0 || nnz <= INT64_MAX / n / 8, OFX_EINVAL, "%s: nnz=%lld * n=%lld overflows",
              fn, (long long)nnz, (long long)n);
  return opts != nullptr ? check_no_plan_options(fn, opts) : OFX_OK;
}

static inline int check_op_act(const char* fn, int op, int act) {
  OFX_REQUIRE(op == OFX_EDGE_MUL || op == OFX_EDGE_ADD, OFX_EINVAL,
              "%s: unknown op code %d (OFX_EDGE_MUL / OFX_EDGE_ADD)", fn, op);
  OFX_REQUIRE(act == OFX_ACT_NONE || act == OFX_ACT_RELU, OFX_EINVAL,
              "%s: unknown activation code %d (OFX_ACT_NONE / OFX_ACT_RELU)", fn, act);
  return OFX_OK;
}

struct Operand {
  const void* ptr;
  uint64_t bytes;
};

// No output may overlap an input.
static inline int check_no_alias(const char* fn, const void* out, uint64_t out_bytes,
                                 std::initializer_list<Operand> inputs) {
  bool alias = false;
  for (const Operand& x : inputs) alias = alias || gat::ranges_overlap(out, out_bytes, x.ptr, x.bytes);
  OFX_REQUIRE(!alias, OFX_EINVAL, "%s: the output overlaps an input", fn);
  return OFX_OK;
}

// The forward (dy == NULL-able: unused) and d(e) (grad_e: out = de [nnz, n], dy [nrows, n] with
// lddy): rows [row_begin, row_end) of the m-row CSR, b [k, n] with ldb.  *nothing: no element to
// write.
static inline int check_edge_args(const char* fn, bool grad_e, int idx_dtype, int val_dtype,
                                  int64_t m, int64_t k, int64_t n, int64_t nnz,
                                  const void* row_ptr, const void* col_idx, const void* e,
                                  const void* b, int64_t ldb, int op, int act, const void* dy,
                                  int64_t lddy, const void* out, int64_t ldo, int64_t row_begin,
                                  int64_t row_end, const ofx_spmm_options* opts, bool* nothing) {
  if (const int rc = check_edge_sizes(fn, idx_dtype, val_dtype, m, k, n, nnz, opts)) return rc;
  if (const int rc = check_op_act(fn, op, act)) return rc;
  if (const int rc = check_row_range(fn, row_begin, row_end, m)) return rc;
  OFX_REQUIRE(ldb >= n && (grad_e ? lddy >= n : ldo >= n), OFX_EINVAL,
              "%s: a leading dimension is smaller than n=%lld", fn, (long long)n);
  const int64_t nrows = row_end - row_begin;
  *nothing = nrows == 0 || n == 0 || (grad_e && nnz == 0);
  if (*nothing) return OFX_OK;
  OFX_REQUIRE(row_ptr && out && (!grad_e || dy), OFX_EINVAL, "%s: NULL pointer", fn);
  OFX_REQUIRE(nnz == 0 || (col_idx && e && (b || k == 0)), OFX_EINVAL,
              "%s: NULL col_idx / e / b with nnz=%lld", fn, (long long)nnz);
  const uint64_t es = (uint64_t)dtype_size(val_dtype), is = (uint64_t)dtype_size(idx_dtype);
  const uint64_t eb = (uint64_t)nnz * (uint64_t)n * es;
  return check_no_alias(fn, out, grad_e ? eb : gv2::extent(nrows, ldo, n, es),
                        {{row_ptr, (uint64_t)(m + 1) * is},
                         {col_idx, (uint64_t)nnz * is},
                         {e, eb},
                         {b, gv2::extent(k, ldb, n, es)},
                         {grad_e ? dy : nullptr, gv2::extent(nrows, lddy, n, es)}});
}

// d(b): rows [row_begin, row_end) of the k-row transposed CSR (row_ptr_t, col_idx_t = rows of A,
// perm); b and db hold the rows from row_begin on, dy is the whole [m, n].
static inline int check_edge_grad_b_args(const char* fn, int idx_dtype, int val_dtype, int64_t m,
                                         int64_t k, int64_t n, int64_t nnz, const void* row_ptr_t,
                                         const void* col_idx_t, const void* perm, const void* e,
                                         const void* b, int64_t ldb, int op, int act,
                                         const void* dy, int64_t lddy, const void* db,
                                         int64_t lddb, int64_t row_begin, int64_t row_end,
                                         const ofx_spmm_options* opts, bool* nothing) {
  if (const int rc = check_edge_sizes(fn, idx_dtype, val_dtype, m, k, n, nnz, opts)) return rc;
  if (const int rc = check_op_act(fn, op, act)) return rc;
  if (const int rc = check_row_range(fn, row_begin, row_end, k)) return rc;
  OFX_REQUIRE(ldb >= n && lddy >= n && lddb >= n, OFX_EINVAL,
              "%s: a leading dimension is smaller than n=%lld", fn, (long long)n);
  const int64_t nrows = row_end - row_begin;
  *nothing = nrows == 0 || n == 0;
  if (*nothing) return OFX_OK;
  OFX_REQUIRE(row_ptr_t && db && b, OFX_EINVAL, "%s: NULL pointer", fn);
  OFX_REQUIRE(nnz == 0 || (col_idx_t && perm && e && (dy || m == 0)), OFX_EINVAL,
              "%s: NULL col_idx_t / perm / e / dy with nnz=%lld", fn, (long long)nnz);
  const uint64_t es = (uint64_t)dtype_size(val_dtype), is = (uint64_t)dtype_size(idx_dtype);
  return check_no_alias(fn, db, gv2::extent(nrows, lddb, n, es),
                        {{row_ptr_t, (uint64_t)(k + 1) * is},
                         {col_idx_t, (uint64_t)nnz * is},
                         {perm, (uint64_t)nnz * is},
                         {e, (uint64_t)nnz * (uint64_t)n * es},
                         {b, gv2::extent(nrows, ldb, n, es)},
                         {dy, gv2::extent(m, lddy, n, es)}});
}

}  // namespace edge
}  // namespace ofx

#endif  // OFX_SPMM_EDGE_H_
