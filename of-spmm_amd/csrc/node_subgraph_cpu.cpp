// node_subgraph_cpu.cpp — the kCPU kernel of the induced-subgraph extraction: the same arrays as
// node_subgraph.hip (rules in node_subgraph.h and compact_ids.h, contract in include/ofx_spmm.h,
// DESIGN.md §3m).  A count entry and a fill entry, as on the device.  The count entry runs the
// block compaction's kCPU kernel over the nodes (src, node_pos), then checks the rows of src and
// counts what each keeps; the fill entry writes the kept entries of each row from its place in
// row_ptr_s on.  Membership and positions come from the node bitmap and its granule ranks, built
// from src by both.  The rows run under OpenMP, handed out in small dynamic chunks (a hub row is
// one row of a chunk); what each writes is fixed by its row alone, so the output does not depend on
// num_threads.
#include <omp.h>

#include <vector>

#include "compact_ids.h"
#include "node_subgraph.h"
#include "ofx_internal.h"
#include "spmm_common.h"

using namespace ofx;

namespace {

// The node bitmap and the set bits in front of each granule, from the ascending distinct src.
struct NodeSet {
  std::vector<uint32_t> bitmap;
  std::vector<int32_t> rank;
  int64_t m;

  template <typename I>
  NodeSet(int nthreads, int64_t m_, const I* src, int64_t count) : m(m_) {
    const int64_t granules = cid::tiles_of(m) * cid::kTileGranules;
    bitmap.assign((size_t)granules * cid::kGranuleWords, 0u);
    rank.assign((size_t)granules, 0);
#pragma omp parallel for num_threads(nthreads) schedule(static)
    for (int64_t r = 0; r < count; ++r) {
      const int64_t v = (int64_t)src[r];
      __atomic_fetch_or(&bitmap[(size_t)(v >> 5)], 1u << (unsigned)(v & 31), __ATOMIC_RELAXED);
    }
    int32_t before = 0;
    for (int64_t g = 0; g < granules; ++g) {
      rank[(size_t)g] = before;
      const uint32_t* w = bitmap.data() + 4 * g;
      before += cid::granule_count(w[0], w[1], w[2], w[3]);
    }
  }

  bool has(int64_t col) const {
    return cid::id_ok(col, m) && ((bitmap[(size_t)(col >> 5)] >> (unsigned)(col & 31)) & 1u) != 0u;
  }
  int position(int64_t col) const { return nsg::rank_of(bitmap.data(), rank.data(), col); }
};

}  // namespace

extern "C" int ofx_node_subgraph_count_cpu(int num_threads, int idx_dtype, int64_t m, int64_t nnz,
                                           int64_t n_nodes, const void* row_ptr,
                                           const void* col_idx, const void* nodes, void* out_src,
                                           void* out_node_pos, void* out_row_ptr,
                                           int64_t* out_counts) {
  return ::ofx::guarded(__func__, [&]() -> int {
    const int rc = nsg::check_count_args("node_subgraph_count_cpu", idx_dtype, m, nnz, n_nodes,
                                         row_ptr, col_idx, nodes, out_src, out_node_pos, out_counts);
    if (rc) return rc;
    OFX_REQUIRE(out_row_ptr, OFX_EINVAL, "node_subgraph_count_cpu: NULL pointer");
    const int nt = threads_of(num_threads);
    out_counts[0] = out_counts[1] = 0;
    // src and node_pos; an id outside [0, m) is refused here ("outside")
    const int rn = ofx_compact_ids_cpu(num_threads, idx_dtype, m, n_nodes, nodes, 0, nullptr, out_src,
                                       out_node_pos, nullptr, out_counts);
    if (rn) return rn;
    return by_index(idx_dtype, [&](auto* ip) -> int {
      using I = std::remove_pointer_t<decltype(ip)>;
      const I* rp = (const I*)row_ptr;
      const I* ci = (const I*)col_idx;
      const I* src = (const I*)out_src;
      I* rps = (I*)out_row_ptr;
      const int64_t count = out_counts[0];
      const NodeSet set(nt, m, src, count);
      std::vector<int32_t> kept((size_t)count);
      int64_t first_bad = INT64_MAX;
#pragma omp parallel for num_threads(nt) schedule(dynamic, 16) reduction(min : first_bad)
      for (int64_t r = 0; r < count; ++r) {
        const int64_t v = (int64_t)src[r];
        const int64_t lo = (int64_t)rp[v], hi = (int64_t)rp[v + 1];
        int32_t k = 0;
        if (!nsg::row_ok(lo, hi, nnz)) {
          if (r < first_bad) first_bad = r;
        } else {
          for (int64_t j = lo; j < hi; ++j) k += set.has((int64_t)ci[j]) ? 1 : 0;
        }
        kept[(size_t)r] = k;
      }
      if (first_bad != INT64_MAX) {
        const int64_t v = (int64_t)src[first_bad];
        return fail(OFX_EINVAL,
                    "node_subgraph_count_cpu: row %lld has the entry range [%lld, %lld): its degree "
                    "is outside [0, 2^31) or its entries are outside [0, %lld)",
                    (long long)v, (long long)rp[v], (long long)rp[v + 1], (long long)nnz);
      }
      int64_t total = 0;
      for (int64_t r = 0; r < count; ++r) {
        rps[r] = (I)total;
        total += kept[(size_t)r];
      }
      OFX_REQUIRE(total <= nnz, OFX_EINVAL,
                  "node_subgraph_count_cpu: the selected rows overlap: row_ptr is outside a CSR's");
      rps[count] = (I)total;
      out_counts[1] = total;
      return OFX_OK;
    });
  });
}

extern "C" int ofx_node_subgraph_fill_cpu(int num_threads, int idx_dtype, int64_t m, int64_t nnz,
                                          int64_t n_nodes, int64_t count, int64_t nnz_s,
                                          const void* row_ptr, const void* col_idx, const void* src,
                                          const void* row_ptr_s, void* out_col_local,
                                          void* out_edge_ids) {
  return ::ofx::guarded(__func__, [&]() -> int {
    const int rc = nsg::check_fill_args("node_subgraph_fill_cpu", idx_dtype, m, nnz, n_nodes, count,
                                        nnz_s, row_ptr, col_idx, src, row_ptr_s, out_col_local);
    if (rc) return rc;
    const int nt = threads_of(num_threads);
    return by_index(idx_dtype, [&](auto* ip) -> int {
      using I = std::remove_pointer_t<decltype(ip)>;
      const I* rp = (const I*)row_ptr;
      const I* ci = (const I*)col_idx;
      const I* nodes = (const I*)src;
      const I* rps = (const I*)row_ptr_s;
      I* col_local = (I*)out_col_local;
      I* edge_ids = (I*)out_edge_ids;
      for (int64_t r = 0; r < count; ++r)
        OFX_REQUIRE(cid::id_ok((int64_t)nodes[r], m) && (r == 0 || nodes[r - 1] < nodes[r]),
                    OFX_EINVAL, "node_subgraph_fill_cpu: src is outside what the count entry gives");
      const NodeSet set(nt, m, nodes, count);
      int bad = 0;
#pragma omp parallel for num_threads(nt) schedule(dynamic, 16) reduction(| : bad)
      for (int64_t r = 0; r < count; ++r) {
        const int64_t v = (int64_t)nodes[r];
        const int64_t lo = (int64_t)rp[v], hi = (int64_t)rp[v + 1];
        int64_t p = (int64_t)rps[r];
        const int64_t end = (int64_t)rps[r + 1];
        if (!nsg::row_ok(lo, hi, nnz) || p < 0 || end < p || end > nnz_s) {
          bad = 1;
          continue;
        }
        for (int64_t j = lo; j < hi && p < end; ++j) {
          const int64_t col = (int64_t)ci[j];
          if (!set.has(col)) continue;
          if (edge_ids) edge_ids[p] = (I)j;
          col_local[p++] = (I)set.position(col);
        }
      }
      OFX_REQUIRE(!bad, OFX_EINVAL,
                  "node_subgraph_fill_cpu: row_ptr_s is outside what the count entry gives");
      return OFX_OK;
    });
  });
}
