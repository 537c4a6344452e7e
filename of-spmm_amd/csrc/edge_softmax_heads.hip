// edge_softmax_heads.hip — ops "edge_softmax_csr_heads" and its gradient on gfx950: the scores
// e T[nnz, H] of a CSR's nonzeros normalised over each row, every head on its own, in one launch
// (contract in include/ofx_spmm.h, DESIGN.md §3f "Edge softmax with heads").  Every arithmetic
// step is edge_softmax.hip's (the leaf steps, butterflies and tile stack of edge_softmax.h), so a
// head's column has the single-head op's bits by construction.
//
// A work item is a (row, head group of V heads); item index = row * G + head group, G = H / V, so
// the head groups of one row sit in adjacent lane groups of a wave and one load instruction covers
// whole position records of H elements.  Lane t of the LG-lane group holds leaf t, positions
// [8t, 8t + 8) of the row, for its V heads: 8 loads of V elements at stride H.  A position past the
// row's end is clamped to the row's last one and its value replaced, so the 8 loads of a round are
// unconditional.  Leaf maxima and sums run in the lane per head; the xor butterflies run on the V
// values.  Stores are V elements wide and plain: a lane's 8 stores are 16-byte (8-byte) pieces of 8
// different records, which L2 merges into lines; as non-temporal stores they cost the f32 H = 4
// launch 8.59 ms instead of 6.89 ms forward and 5.87 instead of 3.61 ms backward.
//   packed path:  H % V == 0 and every base aligned to the vector; V = 4 for f32 (16 bytes), 2 for
//     f64 (16 bytes), 4 for f16 / bf16 (8 bytes: 8 heads a lane would double the registers)
//   general path: any other H or base; V = 1, a work item is a (row, head), scalar loads and stores
// LG is picked from the mean degree as the single-head op does.  A row longer than 8 LG is taken
// over by the whole wave, one (row, head group) after another: up to kTile = 512 positions in
// registers, beyond that in tiles of 64 leaves through a binary-counter stack of V values per
// level.  One tile is in flight on the packed path (its 8 V accumulators per operand are a group
// row's) and two on the general path: with the single-head kernel's four, whose 32 loads each
// carry a 64-bit strided address, the general kernels needed 256 VGPRs and AGPR copies (one wave
// per SIMD); with two on the packed path the f32 kernels take 233-256 VGPRs and measured slower
// (DESIGN.md §3f).
//
// No atomics, no workspace, no allocation, no host synchronisation, no LDS, no scratch.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include "edge_softmax.h"
#include "spmm_items_dev.h"

namespace ofx {
namespace {

using namespace item;
using namespace esm;
using namespace esmh;

// The head vectors, the item's split, the leaf loads and stores at stride H and the rows in
// registers / in tiles / by the wave are edge_softmax.h's: graph_attention_heads.hip runs the same
// steps in place.

template <typename T, typename I, int V, int LG, bool BWD>
__global__ void __launch_bounds__(kBlock)
    edge_softmax_heads_kernel(const I* __restrict__ rp, const T* __restrict__ a,
                              const T* __restrict__ g, T* __restrict__ out, int64_t row_begin,
                              int64_t H, int64_t G, int64_t items, int64_t block_base) {
#pragma clang fp contract(off)
  constexpr int GPW = 64 / LG;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t gi = ((block_base + (int64_t)blockIdx.x) * (kBlock / 64) + wave) * GPW + lane / LG;
  int64_t off = 0, len = 0;
  if (gi < items) {
    int64_t row, hg;
    split_item(gi, G, &row, &hg);
    const int64_t j0 = (int64_t)rp[row_begin + row];
    len = (int64_t)rp[row_begin + row + 1] - j0;
    off = j0 * H + hg * V;
  }
  if constexpr (LG == 64) {
    row_by_wave<T, V, BWD>(a, g, out, H, off, len, lane);  // uniform over the wave
  } else {
    const bool fits = len <= (int64_t)LG * kLeaf;
    row_in_registers<T, V, LG, BWD>(a, g, out, H, off, fits ? len : 0, lane & (LG - 1));
    // the items whose row does not fit their group: the whole wave, one after another
    unsigned long long todo = __ballot(!fits && (lane & (LG - 1)) == 0);
    while (todo != 0) {
      const int src = __ffsll((long long)todo) - 1;
      todo &= todo - 1;
      const int64_t woff = __shfl(off, src, 64), wlen = __shfl(len, src, 64);
      row_by_wave<T, V, BWD>(a, g, out, H, woff, wlen, lane);
    }
  }
}

struct EsmHeadsArgs {
  hipStream_t s;
  const void *rp, *a, *g;
  void* out;
  int64_t m, heads, nnz, row_begin, nrows;
  const ofx_spmm_options* opts;
};

template <typename T, typename I, int V, int LG, bool BWD>
int esmh_cfg(const EsmHeadsArgs& x) {
  const int64_t G = x.heads / V;
  const int64_t items = x.nrows * G;
  return launch_cut_grid(items, (kBlock / 64) * (64 / LG), [&](dim3 grid, int64_t b0) {
    hipLaunchKernelGGL((edge_softmax_heads_kernel<T, I, V, LG, BWD>), grid, dim3(kBlock), 0, x.s,
                       static_cast<const I*>(x.rp), static_cast<const T*>(x.a),
                       static_cast<const T*>(x.g), static_cast<T*>(x.out), x.row_begin, x.heads, G,
                       items, b0);
  });
}

// The path and the lane group by the family's rules (edge_softmax.h heads_packed,
// launch_group_lanes); the forward has no g.
template <typename T, typename I, bool BWD>
int esmh_typed(const EsmHeadsArgs& x) {
  constexpr int V = packed_heads<T>();
  const bool packed = heads_packed<T, V>(x.heads, {x.a, x.g, x.out});
  return with_group_lanes(launch_group_lanes(x.m, x.nrows, x.nnz, x.opts), [&](auto lanes) {
    constexpr int LG = decltype(lanes)::value;
    return packed ? esmh_cfg<T, I, V, LG, BWD>(x) : esmh_cfg<T, I, 1, LG, BWD>(x);
  });
}

template <bool BWD>
int esmh_entry(const char* fn, void* stream, int idx_dtype, int val_dtype, int64_t m,
               int64_t heads, int64_t nnz, const void* row_ptr, const void* a, const void* g,
               void* out, int64_t row_begin, int64_t row_end, const ofx_spmm_options* opts) {
  int rc =
      check_edge_softmax_heads_args(fn, idx_dtype, val_dtype, m, heads, nnz, row_begin, row_end);
  if (rc) return rc;
  if (row_end == row_begin || nnz == 0 || heads == 0) return OFX_OK;
  OFX_REQUIRE(row_ptr && a && out && (!BWD || g), OFX_EINVAL, "%s: NULL pointer", fn);
  OFX_REQUIRE(row_end - row_begin <= INT64_MAX / heads, OFX_EINVAL, "%s: bad heads=%lld", fn,
              (long long)heads);
  if (heads == 1) {  // the single-head kernels: the same bits by the contract, contiguous leaves
    return BWD ? ofx_edge_softmax_csr_grad(stream, idx_dtype, val_dtype, m, nnz, row_ptr, a, g,
                                           out, row_begin, row_end, nullptr, 0, opts)
               : ofx_edge_softmax_csr(stream, idx_dtype, val_dtype, m, nnz, row_ptr, a, out,
                                      row_begin, row_end, nullptr, 0, opts);
  }
  const EsmHeadsArgs x{static_cast<hipStream_t>(stream), row_ptr, a, g, out, m, heads, nnz,
                       row_begin, row_end - row_begin, opts};
  return by_types(idx_dtype, val_dtype, [&](auto* tp, auto* ip) -> int {
    return esmh_typed<std::remove_pointer_t<decltype(tp)>, std::remove_pointer_t<decltype(ip)>,
                      BWD>(x);
  });
}

}  // namespace
}  // namespace ofx

using namespace ofx;

extern "C" int ofx_edge_softmax_csr_heads_workspace_size(int idx_dtype, int val_dtype, int64_t m,
                                                         int64_t heads, int64_t nnz,
                                                         const ofx_spmm_options* opts,
                                                         size_t* bytes) {
  return ::ofx::guarded(__func__, [&]() -> int {
    return softmax_workspace_size("edge_softmax_csr_heads_workspace_size", idx_dtype, val_dtype, m,
                                  0, heads, nnz, opts, bytes);
  });
}

extern "C" int ofx_edge_softmax_csr_heads(void* stream, int idx_dtype, int val_dtype, int64_t m,
                                          int64_t heads, int64_t nnz, const void* row_ptr,
                                          const void* e, void* y, int64_t row_begin,
                                          int64_t row_end, void* workspace, size_t workspace_bytes,
                                          const ofx_spmm_options* opts) {
  return ::ofx::guarded(__func__, [&]() -> int {
    OFX_DEVICE_ENTRY("edge_softmax_csr_heads", opts, workspace, workspace_bytes);
    return esmh_entry<false>("edge_softmax_csr_heads", stream, idx_dtype, val_dtype, m, heads, nnz,
                             row_ptr, e, nullptr, y, row_begin, row_end, opts);
  });
}

extern "C" int ofx_edge_softmax_csr_heads_grad(void* stream, int idx_dtype, int val_dtype,
                                               int64_t m, int64_t heads, int64_t nnz,
                                               const void* row_ptr, const void* y, const void* g,
                                               void* de, int64_t row_begin, int64_t row_end,
                                               void* workspace, size_t workspace_bytes,
                                               const ofx_spmm_options* opts) {
  return ::ofx::guarded(__func__, [&]() -> int {
    OFX_DEVICE_ENTRY("edge_softmax_csr_heads_grad", opts, workspace, workspace_bytes);
    return esmh_entry<true>("edge_softmax_csr_heads_grad", stream, idx_dtype, val_dtype, m, heads,
                            nnz, row_ptr, y, g, de, row_begin, row_end, opts);
  });
}
