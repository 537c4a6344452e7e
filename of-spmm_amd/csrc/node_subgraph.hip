// node_subgraph.hip — the subgraph induced by a node set on the device, gfx950: the rows of the
// chosen nodes restricted to the chosen columns, both relabelled to positions in the ascending list
// of distinct nodes (contract in include/ofx_spmm.h, rules in node_subgraph.h and compact_ids.h,
// DESIGN.md §3m).  Two bitmaps with rank and select: one over the nodes (the block compaction's,
// run by compact_ids.hip as it is) and one over the entries of the CSR.  The work is split by
// entries, never by rows: no wave walks a hub row on its own, there is no planner and no block
// waits on another.
//
// count entry:
//   node set       : ofx_compact_ids over `nodes` with no columns: src, node_pos, the count C, and
//                    the node bitmap and its granule ranks left in the workspace.
//   degree kernel  : deg of the C rows of src behind dp[0] = 0 (a bad row: flag, degree 0), and the
//                    clear of the edge bitmap, in one launch.
//   hipcub scan    : dp in place (int64: a corrupt row_ptr cannot wrap it), D = dp[C] stays on the
//                    device.
//   mark kernel    : fixed grid; a wave takes 64 gathered positions t in [0, D) at a time.  One
//                    wave-uniform binary search in dp finds the row of the chunk's first position
//                    (empty rows are skipped by it); the 64 next row ends, one per lane, relative to
//                    the chunk, are searched by every lane with six cross-lane reads (again when
//                    the chunk spans more than 64 rows).  Each lane forms j, loads col_idx[j], checks
//                    its range and tests one word of the node bitmap.  The keep bits are combined by
//                    ballot: the first lane of every run of consecutive j inside one 32-bit word
//                    issues one atomic OR (plain C++ vector atomic) into the edge bitmap.
//   tile counts    : compact_ids.hip's count kernel over the edge bitmap, hipcub scan in place.
//   rank kernel    : per tile the exclusive scan of its 256 granule counts plus the tile's base;
//                    its first thread stores nnz_s.
// fill entry (after the one read-back of C, nnz_s and the flag), one launch:
//   blocks over the edge tiles: a thread walks the set bits of its granule from its rank on:
//     edge_ids[p] = j, col_local[p] = node rank of col_idx[j]; ascending, nothing atomic;
//   blocks over the rows: row_ptr_s[r] = edge rank of row_ptr[src[r]], row_ptr_s[C] = nnz_s.
// LDS: 16 bytes in the rank kernel, none elsewhere.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include "compact_ids.h"
#include "node_subgraph.h"
#include "ofx_internal.h"
#include "spmm_common.h"
#include "spmm_plan.h"

namespace ofx {
namespace {

constexpr int kBlock = cid::kTileGranules;  // 256
constexpr int kWaves = kBlock / 64;
constexpr int64_t kMaxGrid = 65536;
constexpr int64_t kMarkGrid = 2048;  // 8 waves on every SIMD of 256 compute units

template <typename I>
__global__ void __launch_bounds__(kBlock)
    subgraph_degree_kernel(const I* __restrict__ row_ptr, const I* __restrict__ src,
                           const int64_t* __restrict__ count, int64_t max_count, int64_t nnz,
                           int64_t* __restrict__ dp, uint4* __restrict__ edge_bitmap,
                           int64_t edge_granules, unsigned int* __restrict__ bad,
                           int64_t* __restrict__ out_nnz_s) {
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  const int64_t first = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (first == 0) {
    dp[0] = 0;
    *out_nnz_s = 0;
  }
  const int64_t c = *count;
  for (int64_t r = first; r < max_count; r += stride) {
    int64_t deg = 0;
    if (r < c) {
      const int64_t v = (int64_t)src[r];  // a present node: inside [0, m)
      const int64_t lo = (int64_t)row_ptr[v], hi = (int64_t)row_ptr[v + 1];
      if (nsg::row_ok(lo, hi, nnz))
        deg = hi - lo;
      else
        *bad = 1u;  // every writer stores the same word; the row counts as empty
    }
    dp[r + 1] = deg;
  }
  for (int64_t g = first; g < edge_granules; g += stride) edge_bitmap[g] = make_uint4(0u, 0u, 0u, 0u);
}

template <typename I>
__global__ void __launch_bounds__(kBlock)
    subgraph_mark_kernel(const I* __restrict__ row_ptr, const I* __restrict__ col_idx,
                         const I* __restrict__ src, const int64_t* __restrict__ count,
                         const int64_t* __restrict__ dp, int64_t m, int64_t nnz,
                         const unsigned int* __restrict__ node_bitmap, unsigned int* edge_bitmap,
                         unsigned int* __restrict__ bad) {
  const int lane = threadIdx.x & 63;
  const int64_t c = *count;
  const int64_t total = dp[c];
  if (total > nnz) {  // rows that overlap: a row_ptr that is no CSR's
    if (blockIdx.x == 0 && threadIdx.x == 0) *bad = 1u;
    return;
  }
  const int64_t waves = (int64_t)gridDim.x * kWaves;
  for (int64_t chunk = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6); chunk * 64 < total;
       chunk += waves) {
    const int64_t t0 = chunk * 64, t = t0 + lane;
    const bool valid = t < total;
    // the row of t0: the last r with dp[r] <= t0 (dp[0] = 0 <= t0 < dp[c]); the same in every lane
    int64_t lo = 0, hi = c;
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (dp[mid] <= t0)
        lo = mid + 1;
      else
        hi = mid;
    }
    int64_t base = lo - 1, row = 0;
    bool done = !valid;
    for (;;) {
      // lane k holds the end of row base + k relative to the chunk, capped at 64; non-decreasing
      const int64_t idx = base + 1 + lane;
      const int64_t end = idx <= c ? dp[idx] - t0 : 64;
      const int end_rel = (int)(end < 64 ? end : 64);
      int ends = 0;  // the row ends at or below this lane's position
      for (int step = 32; step > 0; step >>= 1) {
        const int probe = __shfl(end_rel, ends + step - 1);
        if (probe <= lane) ends += step;
      }
      if (__shfl(end_rel, ends) <= lane) ends += 1;  // ends <= 63 before this: all 64 of them
      if (!done && ends < 64) {
        row = base + ends;
        done = true;
      }
      if (__all(done)) break;
      base += 64;
    }
    int j = -1;
    bool keep = false;
    if (valid) {
      const int64_t v = (int64_t)src[row];
      j = (int)((int64_t)row_ptr[v] + (t - dp[row]));  // inside the row's checked range
      const int64_t col = (int64_t)col_idx[j];
      if (cid::id_ok(col, m)) keep = ((node_bitmap[col >> 5] >> (unsigned)(col & 31)) & 1u) != 0u;
    }
    const unsigned long long kept = __ballot(keep);
    const int before = __shfl_up(j, 1);
    const bool leader = lane == 0 || !valid || j != before + 1 || (j & 31) == 0;
    const unsigned long long leaders = __ballot(leader);
    if (leader && valid) {
      const unsigned long long after = lane == 63 ? 0ull : leaders >> (lane + 1);
      int len = after != 0ull ? __ffsll((unsigned long long)after) : 64 - lane;
      len = len < 32 ? len : 32;  // a run ends at its word's last bit
      const uint32_t bits = (uint32_t)((kept >> lane) & ((1ull << len) - 1ull));
      if (bits != 0u) atomicOr(edge_bitmap + (j >> 5), bits << (unsigned)(j & 31));
    }
  }
}

__global__ void __launch_bounds__(kBlock)
    subgraph_rank_kernel(const uint4* __restrict__ edge_bitmap, const int* __restrict__ tile_incl,
                         int64_t tiles, int* __restrict__ rank, int64_t* __restrict__ out_nnz_s) {
  __shared__ int wave_total[kWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t g = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (g == 0) *out_nnz_s = (int64_t)tile_incl[tiles - 1];
  const uint4 w = edge_bitmap[g];
  const int c = cid::granule_count(w.x, w.y, w.z, w.w);
  int incl = c;
  for (int off = 1; off < 64; off <<= 1) {
    const int up = __shfl_up(incl, off);
    if (lane >= off) incl += up;
  }
  if (lane == 63) wave_total[wave] = incl;
  __syncthreads();
  int r = blockIdx.x == 0 ? 0 : tile_incl[blockIdx.x - 1];
  for (int k = 0; k < kWaves - 1; ++k) r += k < wave ? wave_total[k] : 0;
  rank[g] = r + incl - c;
}

template <typename I>
__global__ void __launch_bounds__(kBlock)
    subgraph_fill_kernel(const I* __restrict__ row_ptr, const I* __restrict__ col_idx,
                         const I* __restrict__ src, int64_t count, int64_t nnz, int64_t nnz_s,
                         int64_t m, const uint4* __restrict__ node_bitmap,
                         const int* __restrict__ node_rank, const uint4* __restrict__ edge_bitmap,
                         const int* __restrict__ edge_rank, int64_t edge_tiles,
                         I* __restrict__ out_row_ptr, I* __restrict__ out_col_local,
                         I* __restrict__ out_edge_ids) {
  if ((int64_t)blockIdx.x >= edge_tiles) {  // the rows
    const int64_t r = ((int64_t)blockIdx.x - edge_tiles) * kBlock + threadIdx.x;
    if (r == count) out_row_ptr[r] = (I)nnz_s;
    if (r >= count) return;
    const int64_t lo = (int64_t)row_ptr[(int64_t)src[r]];
    if (lo < 0 || lo > nnz) return;  // the count entry has raised the flag for this row
    const int64_t g = lo >> 7;
    const uint4 w = edge_bitmap[g];
    out_row_ptr[r] = (I)(edge_rank[g] + cid::granule_below(w.x, w.y, w.z, w.w, (int)(lo & 127)));
    return;
  }
  const int64_t g = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const uint4 w = edge_bitmap[g];
  if ((w.x | w.y | w.z | w.w) == 0u) return;
  int64_t p = (int64_t)edge_rank[g];
  const uint32_t words[cid::kGranuleWords] = {w.x, w.y, w.z, w.w};
#pragma unroll
  for (int k = 0; k < cid::kGranuleWords; ++k) {
    const int64_t base = g * cid::kGranuleBits + k * cid::kWordBits;
    for (uint32_t rest = words[k]; rest != 0u; rest &= rest - 1u, ++p) {
      const int64_t j = base + (__ffs((int)rest) - 1);
      if (p >= nnz_s || j >= nnz) return;  // not this workspace's counts
      if (out_edge_ids) out_edge_ids[p] = (I)j;
      const int64_t col = (int64_t)col_idx[j];
      if (!cid::id_ok(col, m)) continue;  // a kept entry's column is a member
      const int64_t gn = col >> 7;
      const uint4 wn = node_bitmap[gn];
      out_col_local[p] =
          (I)(node_rank[gn] + cid::granule_below(wn.x, wn.y, wn.z, wn.w, (int)(col & 127)));
    }
  }
}

// The workspace: a function of (m, nnz, n_nodes) alone.  Every part is aligned to 256 bytes.
struct SubgraphWs {
  size_t bad, compact, compact_bytes, node_bitmap, node_rank, dp, cub_dp, cub_dp_bytes, edge_bitmap,
      edge_rank, edge_tile, cub_tile, cub_tile_bytes, total;
  int64_t max_count, edge_tiles;
};

int subgraph_ws(int64_t m, int64_t nnz, int64_t n_nodes, SubgraphWs* w) {
  *w = SubgraphWs{};
  w->max_count = n_nodes < m ? n_nodes : m;
  w->edge_tiles = nsg::edge_tiles_of(nnz);
  size_t bitmap = 0, rank = 0;
  const int rc = cid::compact_ws_layout(m, &bitmap, &rank, &w->compact_bytes);
  if (rc) return rc;
  if (w->max_count != 0)
    OFX_HIP_CHECK(hipcub::DeviceScan::InclusiveSum(nullptr, w->cub_dp_bytes, (int64_t*)nullptr,
                                                   (int64_t*)nullptr, (int)w->max_count));
  OFX_HIP_CHECK(hipcub::DeviceScan::InclusiveSum(nullptr, w->cub_tile_bytes, (int*)nullptr,
                                                 (int*)nullptr, (int)w->edge_tiles));
  const size_t tiles = (size_t)w->edge_tiles;
  size_t off = 256;  // the flag
  w->compact = off;
  w->node_bitmap = off + bitmap;
  w->node_rank = off + rank;
  off = plan::align_up(off + w->compact_bytes, 256);
  w->dp = off;
  off = plan::align_up(off + ((size_t)w->max_count + 1) * sizeof(int64_t), 256);
  w->cub_dp = off;
  off = plan::align_up(off + w->cub_dp_bytes, 256);
  w->edge_bitmap = off;
  off = plan::align_up(off + tiles * cid::kTileBytes, 256);
  w->edge_rank = off;
  off = plan::align_up(off + tiles * cid::kTileGranules * sizeof(int), 256);
  w->edge_tile = off;
  off = plan::align_up(off + tiles * sizeof(int), 256);
  w->cub_tile = off;
  w->total = plan::align_up(off + w->cub_tile_bytes, 256);
  return OFX_OK;
}

int check_ws(const char* fn, const SubgraphWs& w, const void* ws, size_t ws_bytes) {
  OFX_REQUIRE(ws && ws_bytes >= w.total, OFX_EWORKSPACE, "%s: workspace of %zu bytes < %zu required",
              fn, ws_bytes, w.total);
  OFX_REQUIRE(((uintptr_t)ws & 15u) == 0, OFX_EWORKSPACE,
              "%s: the workspace must be 16-byte aligned (the bitmaps are read in 16-byte granules)",
              fn);
  return OFX_OK;
}

unsigned grid_of(int64_t items, int64_t cap) {
  const int64_t g = (items + kBlock - 1) / kBlock;
  return (unsigned)(g < 1 ? 1 : g > cap ? cap : g);
}

template <typename I>
int count_phase(hipStream_t s, int idx_dtype, int64_t m, int64_t nnz, int64_t n_nodes,
                const I* row_ptr, const I* col_idx, const I* nodes, I* out_src,
                int64_t* out_node_pos, int64_t* out_counts, unsigned int* bad_out, char* ws,
                const SubgraphWs& w) {
  auto* bad = bad_out ? bad_out : reinterpret_cast<unsigned int*>(ws + w.bad);
  auto* dp = reinterpret_cast<int64_t*>(ws + w.dp);
  auto* edge_bitmap = reinterpret_cast<unsigned int*>(ws + w.edge_bitmap);
  auto* edge_bitmap4 = reinterpret_cast<uint4*>(ws + w.edge_bitmap);
  auto* edge_tile = reinterpret_cast<int*>(ws + w.edge_tile);
  // clears the flag and the count, then src, node_pos, the node bitmap and its ranks
  const int rc = ofx_compact_ids(s, idx_dtype, m, n_nodes, nodes, 0, nullptr, out_src, out_node_pos,
                                 nullptr, out_counts, bad, ws + w.compact, w.compact_bytes);
  if (rc) return rc;
  // Without nodes or without rows nothing is selected: dp = {0}, the edge bitmap stays clear.
  const int64_t granules = w.edge_tiles * cid::kTileGranules;
  const int64_t items = w.max_count > granules ? w.max_count : granules;
  hipLaunchKernelGGL((subgraph_degree_kernel<I>), dim3(grid_of(items, kMaxGrid)), dim3(kBlock), 0,
                     s, row_ptr, out_src, out_counts, w.max_count, nnz, dp, edge_bitmap4, granules,
                     bad, out_counts + 1);
  OFX_HIP_CHECK(hipGetLastError());
  if (w.max_count != 0) {
    size_t cb = w.cub_dp_bytes;
    OFX_HIP_CHECK(hipcub::DeviceScan::InclusiveSum(ws + w.cub_dp, cb, dp + 1, dp + 1,
                                                   (int)w.max_count, s));
    hipLaunchKernelGGL((subgraph_mark_kernel<I>), dim3(grid_of(nnz, kMarkGrid)),  // a wave per 64 entries
                       dim3(kBlock), 0, s, row_ptr, col_idx, out_src, out_counts, dp, m, nnz,
                       reinterpret_cast<const unsigned int*>(ws + w.node_bitmap), edge_bitmap, bad);
    OFX_HIP_CHECK(hipGetLastError());
  }
  const int rt = cid::launch_tile_counts(s, edge_bitmap4, w.edge_tiles, edge_tile);
  if (rt) return rt;
  size_t cb = w.cub_tile_bytes;
  OFX_HIP_CHECK(hipcub::DeviceScan::InclusiveSum(ws + w.cub_tile, cb, edge_tile, edge_tile,
                                                 (int)w.edge_tiles, s));
  hipLaunchKernelGGL(subgraph_rank_kernel, dim3((unsigned)w.edge_tiles), dim3(kBlock), 0, s,
                     edge_bitmap4, edge_tile, w.edge_tiles, reinterpret_cast<int*>(ws + w.edge_rank),
                     out_counts + 1);
  OFX_HIP_CHECK(hipGetLastError());
  return OFX_OK;
}

template <typename I>
int fill_phase(hipStream_t s, int64_t m, int64_t nnz, int64_t count, int64_t nnz_s,
               const I* row_ptr, const I* col_idx, const I* src, I* out_row_ptr, I* out_col_local,
               I* out_edge_ids, char* ws, const SubgraphWs& w) {
  const int64_t row_blocks = count / kBlock + 1;  // rows 0..count: the last one holds nnz_s
  hipLaunchKernelGGL((subgraph_fill_kernel<I>), dim3((unsigned)(w.edge_tiles + row_blocks)),
                     dim3(kBlock), 0, s, row_ptr, col_idx, src, count, nnz, nnz_s, m,
                     reinterpret_cast<const uint4*>(ws + w.node_bitmap),
                     reinterpret_cast<const int*>(ws + w.node_rank),
                     reinterpret_cast<const uint4*>(ws + w.edge_bitmap),
                     reinterpret_cast<const int*>(ws + w.edge_rank), w.edge_tiles, out_row_ptr,
                     out_col_local, out_edge_ids);
  OFX_HIP_CHECK(hipGetLastError());
  return OFX_OK;
}

}  // namespace
}  // namespace ofx

using namespace ofx;

extern "C" int ofx_node_subgraph_workspace_size(int idx_dtype, int64_t m, int64_t nnz,
                                                int64_t n_nodes, size_t* bytes) {
  return ::ofx::guarded(__func__, [&]() -> int {
    OFX_REQUIRE(bytes, OFX_EINVAL, "node_subgraph: NULL pointer");
    const int rc = nsg::check_subgraph_sizes("node_subgraph", idx_dtype, m, nnz, n_nodes);
    if (rc) return rc;
    SubgraphWs w;
    const int rw = subgraph_ws(m, nnz, n_nodes, &w);
    *bytes = w.total;
    return rw;
  });
}

extern "C" int ofx_node_subgraph_count(void* stream, int idx_dtype, int64_t m, int64_t nnz,
                                       int64_t n_nodes, const void* row_ptr, const void* col_idx,
                                       const void* nodes, void* out_src, void* out_node_pos,
                                       void* out_counts, void* bad_flag, void* workspace,
                                       size_t workspace_bytes) {
  return ::ofx::guarded(__func__, [&]() -> int {
    const int rc = nsg::check_count_args("node_subgraph_count", idx_dtype, m, nnz, n_nodes, row_ptr,
                                         col_idx, nodes, out_src, out_node_pos, out_counts);
    if (rc) return rc;
    SubgraphWs w;
    const int rw = subgraph_ws(m, nnz, n_nodes, &w);
    if (rw) return rw;
    const int rs = check_ws("node_subgraph_count", w, workspace, workspace_bytes);
    if (rs) return rs;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return by_index(idx_dtype, [&](auto* ip) -> int {
      using I = std::remove_pointer_t<decltype(ip)>;
      return count_phase<I>(s, idx_dtype, m, nnz, n_nodes, (const I*)row_ptr, (const I*)col_idx,
                            (const I*)nodes, (I*)out_src, (int64_t*)out_node_pos,
                            (int64_t*)out_counts, (unsigned int*)bad_flag, (char*)workspace, w);
    });
  });
}

extern "C" int ofx_node_subgraph_fill(void* stream, int idx_dtype, int64_t m, int64_t nnz,
                                      int64_t n_nodes, int64_t count, int64_t nnz_s,
                                      const void* row_ptr, const void* col_idx, const void* src,
                                      void* out_row_ptr, void* out_col_local, void* out_edge_ids,
                                      void* workspace, size_t workspace_bytes) {
  return ::ofx::guarded(__func__, [&]() -> int {
    const int rc = nsg::check_fill_args("node_subgraph_fill", idx_dtype, m, nnz, n_nodes, count,
                                        nnz_s, row_ptr, col_idx, src, out_row_ptr, out_col_local);
    if (rc) return rc;
    SubgraphWs w;
    const int rw = subgraph_ws(m, nnz, n_nodes, &w);
    if (rw) return rw;
    const int rs = check_ws("node_subgraph_fill", w, workspace, workspace_bytes);
    if (rs) return rs;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return by_index(idx_dtype, [&](auto* ip) -> int {
      using I = std::remove_pointer_t<decltype(ip)>;
      return fill_phase<I>(s, m, nnz, count, nnz_s, (const I*)row_ptr, (const I*)col_idx,
                           (const I*)src, (I*)out_row_ptr, (I*)out_col_local, (I*)out_edge_ids,
                           (char*)workspace, w);
    });
  });
}
