// graph_attention.h — the argument checks that the HIP and the kCPU entries of op
// "graph_attention_csr_heads" share (contract in include/ofx_spmm.h).
#ifndef OFX_GRAPH_ATTENTION_H_
#define OFX_GRAPH_ATTENTION_H_

#include <climits>
#include <cstdint>

#include "ofx_internal.h"
#include "spmm_common.h"
#include "spmm_extremum.h"

namespace ofx {
namespace gat {

constexpr int64_t kMaxD = 2048;  // the SDDMM's widest head

static inline bool ranges_overlap(const void* p, uint64_t pbytes, const void* q, uint64_t qbytes) {
  if (p == nullptr || q == nullptr || pbytes == 0 || qbytes == 0) return false;
  const uint64_t a = (uint64_t)(uintptr_t)p, b = (uint64_t)(uintptr_t)q;
  return a < b + qbytes && b < a + pbytes;
}

struct Shape {
  int64_t n, nrows;
  bool nothing;  // nothing to write: return OFX_OK
};

// Everything both entries refuse, in the composition's order; *sh says what is left to do.
static inline int check_graph_attention_args(const char* fn, int idx_dtype, int val_dtype,
                                             int64_t m, int64_t k, int64_t heads, int64_t d,
                                             int64_t nnz, const void* row_ptr, const void* col_idx,
                                             const void* q, int64_t ldq, const void* kk,
                                             int64_t ldk, const void* v, int64_t ldv,
                                             const void* out, int64_t ldo, const void* attn,
                                             int64_t row_begin, int64_t row_end,
                                             const ofx_spmm_options* opts, Shape* sh) {
  if (const int rc = check_heads_shape(fn, heads, d)) return rc;
  if (const int rc = check_types_sizes(fn, idx_dtype, val_dtype, m, k, heads * d, nnz)) return rc;
  OFX_REQUIRE(heads == 0 || nnz <= INT64_MAX / heads, OFX_EINVAL, "%s: bad heads=%lld for nnz=%lld",
              fn, (long long)heads, (long long)nnz);
  if (const int rc = check_no_plan_options(fn, opts)) return rc;
  if (const int rc = check_row_range(fn, row_begin, row_end, m)) return rc;
  const int64_t n = heads * d;
  OFX_REQUIRE(ldq >= n && ldk >= n && ldv >= n && ldo >= n, OFX_EINVAL,
              "%s: ldq=%lld / ldk=%lld / ldv=%lld / ldo=%lld < n=%lld", fn, (long long)ldq,
              (long long)ldk, (long long)ldv, (long long)ldo, (long long)n);
  sh->n = n;
  sh->nrows = row_end - row_begin;
  sh->nothing = sh->nrows == 0 || n == 0;
  if (sh->nothing) return OFX_OK;
  OFX_REQUIRE(d <= kMaxD, OFX_EUNSUPPORTED, "%s: d=%lld > %lld is not supported", fn, (long long)d,
              (long long)kMaxD);
  OFX_REQUIRE(row_ptr && out, OFX_EINVAL, "%s: NULL row_ptr or output", fn);
  OFX_REQUIRE(nnz == 0 || (col_idx && q && kk && v), OFX_EINVAL,
              "%s: NULL col_idx/q/k/v with nnz=%lld", fn, (long long)nnz);
  OFX_REQUIRE(nnz == 0 || attn != nullptr, OFX_EINVAL,
              "%s: attn is NULL (it is the kernel's hand-off buffer and a result)", fn);
  const uint64_t es = val_dtype == OFX_DT_DOUBLE ? 8 : (val_dtype == OFX_DT_FLOAT ? 4 : 2);
  const uint64_t is = idx_dtype == OFX_DT_INT32 ? 4 : 8;
  const uint64_t ab = (uint64_t)nnz * (uint64_t)heads * es;
  const bool alias = ranges_overlap(attn, ab, q, (uint64_t)sh->nrows * (uint64_t)ldq * es) ||
                     ranges_overlap(attn, ab, kk, (uint64_t)k * (uint64_t)ldk * es) ||
                     ranges_overlap(attn, ab, v, (uint64_t)k * (uint64_t)ldv * es) ||
                     ranges_overlap(attn, ab, out, (uint64_t)sh->nrows * (uint64_t)ldo * es) ||
                     ranges_overlap(attn, ab, col_idx, (uint64_t)nnz * is) ||
                     ranges_overlap(attn, ab, row_ptr, (uint64_t)(m + 1) * is);
  OFX_REQUIRE(!alias, OFX_EINVAL, "%s: attn overlaps an input or out", fn);
  return OFX_OK;
}

}  // namespace gat
}  // namespace ofx

#endif  // OFX_GRAPH_ATTENTION_H_
