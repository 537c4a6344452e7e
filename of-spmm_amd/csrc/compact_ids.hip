// compact_ids.hip — block compaction on the device, gfx950: the distinct ids of seeds ∪ cols in
// ascending order and the position of every seed and column in that list (contract in
// include/ofx_spmm.h, layout rules in compact_ids.h).  A bitmap over the node ids
// with rank and select: no sort, no hash table, no second path, and no block waits on another.
//
//   clear kernel   : the bitmap (16-byte stores), the bad flag and the count.  A kernel, not
//                    hipMemsetAsync: one launch for all three.
//   mark kernel    : grid-stride over the S + E ids, both arrays in one launch.  A bad id stores 1
//                    to the flag and is never used as an address.  A good id loads its bitmap word
//                    and issues the atomic OR only while its bit is clear: the thousands of
//                    repeats of a hub's id stay off the atomic unit.
//   count kernel   : one block of 256 threads per tile of 32,768 bits, one 128-bit granule per
//                    thread (one 16-byte load), population count, reduce across the lanes of each
//                    wave by cross-lane moves, across the four waves through LDS: one count per tile.
//   hipcub scan    : the tile counts in place (inclusive), as csr_build.hip and the sampler scan;
//                    65,536 tiles at most.  Its last entry is the count.
//   emit kernel    : the same tile shape; an in-block exclusive scan of the 256 granule counts
//                    (wave scan by cross-lane moves, wave totals through LDS) plus the tile's base
//                    gives each granule's rank, stored for the relabel; each thread then writes the
//                    ids of its set bits at its rank, lowest bit first: src comes out ascending.
//   relabel kernel : grid-stride over the ids: one 16-byte load of the id's granule, one rank
//                    load, the population count of the bits below it.
// LDS: four words per block in the count and emit kernels, none elsewhere.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include "compact_ids.h"
#include "ofx_internal.h"
#include "spmm_common.h"
#include "spmm_plan.h"

namespace ofx {
namespace {

constexpr int kBlock = cid::kTileGranules;  // 256
constexpr int kWaves = kBlock / 64;
constexpr int64_t kMaxGrid = 65536;

__global__ void __launch_bounds__(kBlock)
    compact_clear_kernel(uint4* __restrict__ bitmap, int64_t granules, unsigned int* __restrict__ bad,
                         int64_t* __restrict__ out_count) {
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  const int64_t first = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (first == 0) {
    *bad = 0u;
    *out_count = 0;
  }
  for (int64_t g = first; g < granules; g += stride) bitmap[g] = make_uint4(0u, 0u, 0u, 0u);
}

// Id i of the S + E ids: the seeds first, then the columns.
template <typename I>
__device__ __forceinline__ int64_t id_at(const I* __restrict__ seeds, int64_t n_seeds,
                                         const I* __restrict__ cols, int64_t i) {
  return i < n_seeds ? (int64_t)seeds[i] : (int64_t)cols[i - n_seeds];
}

template <typename I>
__global__ void __launch_bounds__(kBlock)
    compact_mark_kernel(const I* __restrict__ seeds, int64_t n_seeds, const I* __restrict__ cols,
                        int64_t n, int64_t num_nodes, unsigned int* bitmap,
                        unsigned int* __restrict__ bad) {
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
    const int64_t v = id_at(seeds, n_seeds, cols, i);
    if (!cid::id_ok(v, num_nodes)) {
      *bad = 1u;  // every writer stores the same word
      continue;
    }
    unsigned int* word = bitmap + (v >> 5);
    const unsigned int bit = 1u << (unsigned)(v & 31);
    // A stale read can only miss a bit another lane has just set: the OR is then issued once more.
    if ((*word & bit) == 0u) atomicOr(word, bit);
  }
}

__global__ void __launch_bounds__(kBlock)
    compact_count_kernel(const uint4* __restrict__ bitmap, int* __restrict__ tile_count) {
  __shared__ int wave_total[kWaves];
  const uint4 w = bitmap[(int64_t)blockIdx.x * kBlock + threadIdx.x];
  int c = cid::granule_count(w.x, w.y, w.z, w.w);
  for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off);
  if ((threadIdx.x & 63) == 0) wave_total[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0)
    tile_count[blockIdx.x] = wave_total[0] + wave_total[1] + wave_total[2] + wave_total[3];
}

template <typename I>
__global__ void __launch_bounds__(kBlock)
    compact_emit_kernel(const uint4* __restrict__ bitmap, const int* __restrict__ tile_incl,
                        int64_t tiles, int* __restrict__ rank, I* __restrict__ src,
                        int64_t* __restrict__ out_count) {
  __shared__ int wave_total[kWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t g = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (g == 0) *out_count = (int64_t)tile_incl[tiles - 1];
  const uint4 w = bitmap[g];
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
  r += incl - c;
  rank[g] = r;
  const uint32_t words[cid::kGranuleWords] = {w.x, w.y, w.z, w.w};
#pragma unroll
  for (int k = 0; k < cid::kGranuleWords; ++k) {
    const int64_t base = g * cid::kGranuleBits + k * cid::kWordBits;
    for (uint32_t rest = words[k]; rest != 0u; rest &= rest - 1u)
      src[r++] = (I)(base + (__ffs((int)rest) - 1));
  }
}

template <typename I>
__global__ void __launch_bounds__(kBlock)
    compact_relabel_kernel(const I* __restrict__ seeds, int64_t n_seeds, const I* __restrict__ cols,
                           int64_t n, int64_t num_nodes, const uint4* __restrict__ bitmap,
                           const int* __restrict__ rank, int64_t* __restrict__ seed_pos,
                           I* __restrict__ col_local) {
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
    const int64_t v = id_at(seeds, n_seeds, cols, i);
    if (!cid::id_ok(v, num_nodes)) continue;  // the flag is up: the outputs are unspecified
    const int64_t g = v >> 7;
    const uint4 w = bitmap[g];
    const int pos = rank[g] + cid::granule_below(w.x, w.y, w.z, w.w, (int)(v & 127));
    if (i < n_seeds)
      seed_pos[i] = (int64_t)pos;
    else
      col_local[i - n_seeds] = (I)pos;
  }
}

struct CompactWs {
  size_t bad, bitmap, rank, tile, cub, cub_bytes, total;
};

int compact_ws(int64_t num_nodes, CompactWs* w) {
  *w = CompactWs{};
  const size_t tiles = (size_t)cid::tiles_of(num_nodes);
  size_t scan = 0;
  if (tiles != 0)
    OFX_HIP_CHECK(hipcub::DeviceScan::InclusiveSum(nullptr, scan, (int*)nullptr, (int*)nullptr,
                                                   (int)tiles));
  size_t off = 256;  // the flag
  w->bitmap = off;
  off = plan::align_up(off + tiles * cid::kTileBytes, 256);
  w->rank = off;
  off = plan::align_up(off + tiles * cid::kTileGranules * sizeof(int), 256);
  w->tile = off;
  off = plan::align_up(off + tiles * sizeof(int), 256);
  w->cub = off;
  w->cub_bytes = scan;
  w->total = plan::align_up(off + scan, 256);
  return OFX_OK;
}

unsigned grid_of(int64_t items) {
  const int64_t g = (items + kBlock - 1) / kBlock;
  return (unsigned)(g < 1 ? 1 : g > kMaxGrid ? kMaxGrid : g);
}

template <typename I>
int compact(hipStream_t s, int64_t num_nodes, int64_t n_seeds, const I* seeds, int64_t n_cols,
            const I* cols, I* out_src, int64_t* out_seed_pos, I* out_col_local, int64_t* out_count,
            unsigned int* bad_out, char* ws, size_t ws_bytes) {
  CompactWs w;
  const int rc = compact_ws(num_nodes, &w);
  if (rc) return rc;
  OFX_REQUIRE(ws && ws_bytes >= w.total, OFX_EWORKSPACE,
              "compact_ids: workspace of %zu bytes < %zu required", ws_bytes, w.total);
  const int64_t n = n_seeds + n_cols;
  const int64_t tiles = cid::tiles_of(num_nodes);
  // Without ids there is nothing to mark, and without nodes every id is bad: the count stays 0.
  const int64_t granules = n == 0 ? 0 : tiles * cid::kTileGranules;
  auto* bad = bad_out ? bad_out : reinterpret_cast<unsigned int*>(ws + w.bad);
  auto* bitmap = reinterpret_cast<unsigned int*>(ws + w.bitmap);
  auto* bitmap4 = reinterpret_cast<uint4*>(ws + w.bitmap);
  auto* rank = reinterpret_cast<int*>(ws + w.rank);
  auto* tile = reinterpret_cast<int*>(ws + w.tile);
  hipLaunchKernelGGL(compact_clear_kernel, dim3(grid_of(granules)), dim3(kBlock), 0, s, bitmap4,
                     granules, bad, out_count);
  OFX_HIP_CHECK(hipGetLastError());
  if (n == 0) return OFX_OK;
  hipLaunchKernelGGL((compact_mark_kernel<I>), dim3(grid_of(n)), dim3(kBlock), 0, s, seeds, n_seeds,
                     cols, n, num_nodes, bitmap, bad);
  OFX_HIP_CHECK(hipGetLastError());
  if (tiles == 0) return OFX_OK;
  hipLaunchKernelGGL(compact_count_kernel, dim3((unsigned)tiles), dim3(kBlock), 0, s, bitmap4, tile);
  OFX_HIP_CHECK(hipGetLastError());
  size_t cb = w.cub_bytes;
  OFX_HIP_CHECK(hipcub::DeviceScan::InclusiveSum(ws + w.cub, cb, tile, tile, (int)tiles, s));
  hipLaunchKernelGGL((compact_emit_kernel<I>), dim3((unsigned)tiles), dim3(kBlock), 0, s, bitmap4,
                     tile, tiles, rank, out_src, out_count);
  OFX_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL((compact_relabel_kernel<I>), dim3(grid_of(n)), dim3(kBlock), 0, s, seeds,
                     n_seeds, cols, n, num_nodes, bitmap4, rank, out_seed_pos, out_col_local);
  OFX_HIP_CHECK(hipGetLastError());
  return OFX_OK;
}

}  // namespace

int cid::compact_ws_layout(int64_t num_nodes, size_t* bitmap_off, size_t* rank_off, size_t* total) {
  CompactWs w;
  const int rc = compact_ws(num_nodes, &w);
  *bitmap_off = w.bitmap;
  *rank_off = w.rank;
  *total = w.total;
  return rc;
}

int cid::launch_tile_counts(hipStream_t s, const uint4* bitmap, int64_t tiles, int* tile_count) {
  hipLaunchKernelGGL(compact_count_kernel, dim3((unsigned)tiles), dim3(kBlock), 0, s, bitmap,
                     tile_count);
  OFX_HIP_CHECK(hipGetLastError());
  return OFX_OK;
}

}  // namespace ofx

using namespace ofx;

extern "C" int ofx_compact_ids_workspace_size(int idx_dtype, int64_t num_nodes, int64_t n_seeds,
                                              int64_t n_cols, size_t* bytes) {
  return ::ofx::guarded(__func__, [&]() -> int {
    OFX_REQUIRE(bytes, OFX_EINVAL, "compact_ids: NULL pointer");
    const int rc = cid::check_compact_sizes("compact_ids", idx_dtype, num_nodes, n_seeds, n_cols);
    if (rc) return rc;
    CompactWs w;
    const int rw = compact_ws(num_nodes, &w);
    *bytes = w.total;
    return rw;
  });
}

extern "C" int ofx_compact_ids(void* stream, int idx_dtype, int64_t num_nodes, int64_t n_seeds,
                               const void* seeds, int64_t n_cols, const void* cols, void* out_src,
                               void* out_seed_pos, void* out_col_local, void* out_count,
                               void* bad_flag, void* workspace, size_t workspace_bytes) {
  return ::ofx::guarded(__func__, [&]() -> int {
    const int rc = cid::check_compact_args("compact_ids", idx_dtype, num_nodes, n_seeds, seeds,
                                           n_cols, cols, out_src, out_seed_pos, out_col_local,
                                           out_count);
    if (rc) return rc;
    OFX_REQUIRE(((uintptr_t)workspace & 15u) == 0, OFX_EWORKSPACE,
                "compact_ids: the workspace must be 16-byte aligned (the bitmap is read in 16-byte "
                "granules)");
    hipStream_t s = static_cast<hipStream_t>(stream);
    return by_index(idx_dtype, [&](auto* ip) -> int {
      using I = std::remove_pointer_t<decltype(ip)>;
      return compact<I>(s, num_nodes, n_seeds, (const I*)seeds, n_cols, (const I*)cols, (I*)out_src,
                        (int64_t*)out_seed_pos, (I*)out_col_local, (int64_t*)out_count,
                        (unsigned int*)bad_flag, (char*)workspace, workspace_bytes);
    });
  });
}
