// compact_ids.h — what the kCPU kernel (compact_ids_cpu.cpp) and the HIP kernels (compact_ids.hip)
// of the block compaction share: the layout of the bitmap, the range check, the rank of an id
// inside its granule and the argument checks of the C-ABI entries (contract in
// include/ofx_spmm.h).
//
// The ids live in [0, num_nodes).  One bit per node says "present"; the bits are kept in 32-bit
// words (the width of the cheapest vector atomic, and of the population count instruction), four
// words make a granule of 128 bits (one 16-byte load) and 256 granules make a tile of 32,768 bits
// (one block of 256 threads, one granule per thread).  rank[g] is the number of set bits in front
// of granule g, so the position of a present id in the ascending list of present ids is
//   rank[id / 128] + (set bits of its granule below bit id % 128)
// and that list itself is what a walk over the set bits writes.  Integers only.
#ifndef OFX_COMPACT_IDS_H_
#define OFX_COMPACT_IDS_H_

#include <climits>

#include "ofx_internal.h"
#include "spmm_common.h"

namespace ofx {
namespace cid {

constexpr int kWordBits = 32;
constexpr int kGranuleWords = 4;
constexpr int kGranuleBits = kWordBits * kGranuleWords;  // 128: one 16-byte load
constexpr int kTileGranules = 256;                       // one granule per thread of a block
constexpr int kTileBits = kGranuleBits * kTileGranules;  // 32768
constexpr int kTileBytes = kTileBits / 8;                // 4096

// Whole tiles: every granule a block reads exists, and the bits past num_nodes stay clear.
OFX_HD int64_t tiles_of(int64_t num_nodes) { return (num_nodes + kTileBits - 1) / kTileBits; }

// An id is used as an address only after this.
OFX_HD bool id_ok(int64_t v, int64_t num_nodes) { return v >= 0 && v < num_nodes; }

OFX_HD int popcount32(uint32_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __popc(x);
#else
  return __builtin_popcount(x);
#endif
}

OFX_HD int granule_count(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3) {
  return popcount32(w0) + popcount32(w1) + popcount32(w2) + popcount32(w3);
}

// The set bits of the granule (w0..w3, lowest word first) below bit `bit` (0..127).  Selects, no
// indexing: the four words stay in registers.
OFX_HD int granule_below(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, int bit) {
  const int k = bit >> 5;
  const uint32_t word = k == 0 ? w0 : k == 1 ? w1 : k == 2 ? w2 : w3;
  const int full = (k > 0 ? popcount32(w0) : 0) + (k > 1 ? popcount32(w1) : 0) +
                   (k > 2 ? popcount32(w2) : 0);
  return full + popcount32(word & ((1u << (bit & 31)) - 1u));
}

// The checks every entry shares (host): the sizes, then the pointers.
static inline int check_compact_sizes(const char* fn, int idx_dtype, int64_t num_nodes,
                                      int64_t n_seeds, int64_t n_cols) {
  OFX_REQUIRE(is_index_dtype(idx_dtype), OFX_EUNSUPPORTED, "%s: index dtype %d is not int32/int64",
              fn, idx_dtype);
  OFX_REQUIRE(num_nodes >= 0 && num_nodes <= (int64_t)INT32_MAX, OFX_EINVAL,
              "%s: num_nodes %lld is not in [0, 2^31)", fn, (long long)num_nodes);
  OFX_REQUIRE(n_seeds >= 0 && n_cols >= 0 && n_seeds <= (int64_t)INT32_MAX &&
                  n_cols <= (int64_t)INT32_MAX && n_seeds + n_cols <= (int64_t)INT32_MAX,
              OFX_EINVAL, "%s: %lld seeds and %lld columns: each count is >= 0, their sum < 2^31",
              fn, (long long)n_seeds, (long long)n_cols);
  return OFX_OK;
}

static inline int check_compact_args(const char* fn, int idx_dtype, int64_t num_nodes,
                                     int64_t n_seeds, const void* seeds, int64_t n_cols,
                                     const void* cols, const void* out_src,
                                     const void* out_seed_pos, const void* out_col_local,
                                     const void* out_count) {
  const int rc = check_compact_sizes(fn, idx_dtype, num_nodes, n_seeds, n_cols);
  if (rc) return rc;
  OFX_REQUIRE(out_count, OFX_EINVAL, "%s: NULL pointer", fn);
  OFX_REQUIRE(n_seeds == 0 || (seeds && out_seed_pos), OFX_EINVAL, "%s: NULL pointer", fn);
  OFX_REQUIRE(n_cols == 0 || (cols && out_col_local), OFX_EINVAL, "%s: NULL pointer", fn);
  OFX_REQUIRE(n_seeds + n_cols == 0 || num_nodes == 0 || out_src, OFX_EINVAL, "%s: NULL pointer",
              fn);
  return OFX_OK;
}

#if defined(__HIPCC__) || defined(__HIP__)
// What compact_ids.hip gives another device unit that stands on its bitmap (node_subgraph.hip):
// where a compaction over num_nodes leaves the bitmap and the granule ranks in its workspace, and
// the tile-count launch over any bitmap of this layout.  Host functions: the kernels stay where
// they are.
int compact_ws_layout(int64_t num_nodes, size_t* bitmap_off, size_t* rank_off, size_t* total);
int launch_tile_counts(hipStream_t s, const uint4* bitmap, int64_t tiles, int* tile_count);
#endif

}  // namespace cid
}  // namespace ofx

#endif  // OFX_COMPACT_IDS_H_
