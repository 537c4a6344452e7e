// node_subgraph.h — what the kCPU kernel (node_subgraph_cpu.cpp) and the HIP kernels
// (node_subgraph.hip) of the induced-subgraph extraction share: the check of a selected row, the
// size of the edge bitmap and the argument checks of the C-ABI entries (contract in
// include/ofx_spmm.h).  Both bitmaps, the one over the nodes and the one over the
// entries, follow the layout and the rank rules of compact_ids.h.  Integers only.
#ifndef OFX_NODE_SUBGRAPH_H_
#define OFX_NODE_SUBGRAPH_H_

#include <climits>

#include "compact_ids.h"
#include "ofx_internal.h"
#include "spmm_common.h"

namespace ofx {
namespace nsg {

// The entry range [lo, hi) of a selected row is used only after this: a degree in [0, 2^31) and a
// range inside [0, nnz).
OFX_HD bool row_ok(int64_t lo, int64_t hi, int64_t nnz) { return lo >= 0 && hi >= lo && hi <= nnz; }

// The edge bitmap covers the positions [0, nnz]: position nnz is never set, but the rank in front
// of it is the end of the last row, so its granule exists.
OFX_HD int64_t edge_tiles_of(int64_t nnz) { return cid::tiles_of(nnz + 1); }

// The set bits in front of position `pos`, from the bitmap's words and the ranks of its granules.
OFX_HD int rank_of(const uint32_t* bitmap, const int32_t* rank, int64_t pos) {
  const int64_t g = pos >> 7;
  const uint32_t* w = bitmap + 4 * g;
  return rank[g] + cid::granule_below(w[0], w[1], w[2], w[3], (int)(pos & 127));
}

// The checks every entry shares (host): the sizes.
static inline int check_subgraph_sizes(const char* fn, int idx_dtype, int64_t m, int64_t nnz,
                                       int64_t n_nodes) {
  OFX_REQUIRE(is_index_dtype(idx_dtype), OFX_EUNSUPPORTED, "%s: index dtype %d is not int32/int64",
              fn, idx_dtype);
  OFX_REQUIRE(m >= 0 && m <= (int64_t)INT32_MAX, OFX_EINVAL, "%s: m %lld is not in [0, 2^31)", fn,
              (long long)m);
  OFX_REQUIRE(nnz >= 0 && nnz <= (int64_t)INT32_MAX, OFX_EINVAL, "%s: nnz %lld is not in [0, 2^31)",
              fn, (long long)nnz);
  OFX_REQUIRE(n_nodes >= 0 && n_nodes <= (int64_t)INT32_MAX, OFX_EINVAL,
              "%s: %lld nodes: the count is not in [0, 2^31)", fn, (long long)n_nodes);
  return OFX_OK;
}

// The sizes, then the pointers of a counting entry.
static inline int check_count_args(const char* fn, int idx_dtype, int64_t m, int64_t nnz,
                                   int64_t n_nodes, const void* row_ptr, const void* col_idx,
                                   const void* nodes, const void* out_src, const void* out_node_pos,
                                   const void* out_counts) {
  const int rc = check_subgraph_sizes(fn, idx_dtype, m, nnz, n_nodes);
  if (rc) return rc;
  OFX_REQUIRE(row_ptr && out_counts, OFX_EINVAL, "%s: NULL pointer", fn);
  OFX_REQUIRE(nnz == 0 || col_idx, OFX_EINVAL, "%s: NULL pointer", fn);
  OFX_REQUIRE(n_nodes == 0 || (nodes && out_node_pos), OFX_EINVAL, "%s: NULL pointer", fn);
  OFX_REQUIRE(n_nodes == 0 || m == 0 || out_src, OFX_EINVAL, "%s: NULL pointer", fn);
  return OFX_OK;
}

// The sizes, then the counts and the pointers of a filling entry.
static inline int check_fill_args(const char* fn, int idx_dtype, int64_t m, int64_t nnz,
                                  int64_t n_nodes, int64_t count, int64_t nnz_s, const void* row_ptr,
                                  const void* col_idx, const void* src, const void* out_row_ptr,
                                  const void* out_col_local) {
  const int rc = check_subgraph_sizes(fn, idx_dtype, m, nnz, n_nodes);
  if (rc) return rc;
  OFX_REQUIRE(count >= 0 && count <= m && count <= n_nodes && nnz_s >= 0 && nnz_s <= nnz, OFX_EINVAL,
              "%s: %lld rows and %lld entries are not what a count over %lld nodes of %lld rows and "
              "%lld entries gives",
              fn, (long long)count, (long long)nnz_s, (long long)n_nodes, (long long)m,
              (long long)nnz);
  OFX_REQUIRE(row_ptr && out_row_ptr, OFX_EINVAL, "%s: NULL pointer", fn);
  OFX_REQUIRE(count == 0 || src, OFX_EINVAL, "%s: NULL pointer", fn);
  OFX_REQUIRE(nnz_s == 0 || (col_idx && out_col_local), OFX_EINVAL, "%s: NULL pointer", fn);
  return OFX_OK;
}

}  // namespace nsg
}  // namespace ofx

#endif  // OFX_NODE_SUBGRAPH_H_
