// edge_softmax.hip — op "edge_softmax_csr" and its gradient on gfx950: the scores of a CSR's
// nonzeros normalised over each row (contract in include/ofx_spmm.h; the
// exponential and the constants of the sum's order in edge_softmax.h).
//
// One lane group of LG lanes per row of the identity work list (work_item with skip_empty; no
// plan is read, so no plan can be invalid).  LG is picked per launch from the mean degree by the
// family's rule (edge_softmax.h launch_group_lanes).  Lane t of a group holds the row's leaf t (8
// consecutive positions) in registers, loaded and stored 16 bytes at a time at whatever alignment
// the row starts (exact on gfx950, probes/unaligned_probe.hip; a vector is taken only where it
// lies wholly inside the row, so nothing outside the launch's nonzeros is read or written).  The
// maximum and the tree sum both go through the SDDMM's xor butterfly.  A row that fits its group
// (at most 8 LG elements) is read once and written once.
//
// Longer rows are taken over by the whole wave, one after another: up to kTile = 512 elements the
// wave is the lane group (still read once); beyond, the row is swept in tiles of 64 leaves, whose
// values (each the butterfly's 64-leaf tree) are added pairwise in tile order through a
// binary-counter stack, as the wide SDDMM does (spmm_backward.hip).  The stack's level l lives in
// lane l, so it costs one register whatever the row's length.  The forward sweeps e three times
// (max, sum, normalise), the backward y and g twice.  Zero-padding the leaves to a larger power of
// two cannot change a bit: a leaf sum starts from +0 and is never -0 (spmm_backward.hip, the
// masked SDDMM's note).
//
// No atomics, no workspace, no allocation, no host synchronisation; y / de leave through
// non-temporal stores.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include "edge_softmax.h"
#include "spmm_items_dev.h"

namespace ofx {
namespace {

using namespace item;
using namespace esm;

constexpr int kSweepTiles = 4;  // tiles of a long row in flight per wave

// 16 bytes (8 for a 4-element f16 / bf16 vector never occur: a 16-bit leaf is one vector) at the
// alignment of their element type.
typedef unsigned u32x4_a2 __attribute__((ext_vector_type(4), aligned(2)));
typedef unsigned u32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));
typedef unsigned u32x4_a8 __attribute__((ext_vector_type(4), aligned(8)));
template <int ALIGN>
struct Vec16;
template <>
struct Vec16<2> {
  using type = u32x4_a2;
};
template <>
struct Vec16<4> {
  using type = u32x4_a4;
};
template <>
struct Vec16<8> {
  using type = u32x4_a8;
};

template <typename T>
struct LeafVec {
  static constexpr int per = 16 / sizeof(T) < kLeaf ? 16 / sizeof(T) : kLeaf;
  using V = typename Vec16<sizeof(T)>::type;
  struct Elems {
    T v[per];
  };
  static_assert(sizeof(Elems) == 16, "a vector of a leaf is 16 bytes");
};

// x[i] = load(p[pos + i]) for the leaf's positions inside [0, len), `fill` for the others.
template <typename T>
__device__ __forceinline__ void load_leaf(const T* __restrict__ p, int64_t pos, int64_t len,
                                          typename Num<T>::acc fill,
                                          typename Num<T>::acc (&x)[kLeaf]) {
  using L = LeafVec<T>;
#pragma unroll
  for (int q = 0; q < kLeaf / L::per; ++q) {
    const int64_t b = pos + q * L::per;
    if (b + L::per <= len) {
      const typename L::V raw = *reinterpret_cast<const typename L::V*>(p + b);
      const typename L::Elems el = __builtin_bit_cast(typename L::Elems, raw);
#pragma unroll
      for (int i = 0; i < L::per; ++i) x[q * L::per + i] = Num<T>::load(el.v[i]);
    } else {
#pragma unroll
      for (int i = 0; i < L::per; ++i)
        x[q * L::per + i] = b + i < len ? Num<T>::load(p[b + i]) : fill;
    }
  }
}

template <typename T>
__device__ __forceinline__ void store_leaf(T* __restrict__ p, int64_t pos, int64_t len,
                                           const T (&y)[kLeaf]) {
  using L = LeafVec<T>;
#pragma unroll
  for (int q = 0; q < kLeaf / L::per; ++q) {
    const int64_t b = pos + q * L::per;
    if (b + L::per <= len) {
      typename L::Elems el;
#pragma unroll
      for (int i = 0; i < L::per; ++i) el.v[i] = y[q * L::per + i];
      __builtin_nontemporal_store(__builtin_bit_cast(typename L::V, el),
                                  reinterpret_cast<typename L::V*>(p + b));
    } else {
#pragma unroll
      for (int i = 0; i < L::per; ++i)
        if (b + i < len) nt_store_one(p + b + i, y[q * L::per + i]);
    }
  }
}

// The leaf steps, the butterflies and the tile stack are in edge_softmax.h (shared with
// edge_softmax_heads.hip).

// A row of at most 8 LG elements over a group of LG lanes, lane gl holding leaf gl.  len == 0:
// nothing is loaded or stored (a group with no row, or whose row the wave takes over).
// Forward: a = e, out = y.  Backward: a = y, g = the upstream gradient, out = de.
template <typename T, int LG, bool BWD>
__device__ __forceinline__ void row_in_registers(const T* __restrict__ a, const T* __restrict__ g,
                                                 T* __restrict__ out, int64_t j0, int64_t len,
                                                 int gl) {
  using A = typename Num<T>::acc;
  const int64_t pos = (int64_t)gl * kLeaf;
  A x[kLeaf];
  T res[kLeaf];
  if constexpr (!BWD) {
    load_leaf<T>(a + j0, pos, len, -__builtin_huge_val(), x);
    const A m = group_max<A, LG>(leaf_max<A>(x, x[0]));
    const A s = group_sum<A, LG>(leaf_exp_sum<A>(x, m, pos, len));
    leaf_divide<T>(x, s, res);
  } else {
    A gg[kLeaf];
    load_leaf<T>(a + j0, pos, len, A(0), x);
    load_leaf<T>(g + j0, pos, len, A(0), gg);
    const A d = group_sum<A, LG>(leaf_dot<A>(x, gg));
    leaf_grad<T>(x, gg, d, res);
  }
  store_leaf<T>(out + j0, pos, len, res);
}

// A row of more than kTile elements, by the whole wave.
template <typename T, bool BWD>
__device__ __forceinline__ void row_in_tiles(const T* __restrict__ a, const T* __restrict__ g,
                                             T* __restrict__ out, int64_t j0, int64_t len,
                                             int lane) {
  using A = typename Num<T>::acc;
  const T* pa = a + j0;
  const T* pg = BWD ? g + j0 : nullptr;
  T* po = out + j0;
  const int64_t tiles = (len + kTile - 1) / kTile;
  const int64_t lpos = (int64_t)lane * kLeaf;
  A m = A(0);
  if constexpr (!BWD) {
    A best = -__builtin_huge_val();
    for (int64_t t0 = 0; t0 < tiles; t0 += kSweepTiles) {
      A x[kSweepTiles][kLeaf];
#pragma unroll
      for (int u = 0; u < kSweepTiles; ++u)
        load_leaf<T>(pa, (t0 + u) * kTile + lpos, len, -__builtin_huge_val(), x[u]);
#pragma unroll
      for (int u = 0; u < kSweepTiles; ++u) best = leaf_max<A>(x[u], best);
    }
    m = group_max<A, 64>(best);
  }
  A stk = A(0);
  for (int64_t t0 = 0; t0 < tiles; t0 += kSweepTiles) {
    A x[kSweepTiles][kLeaf], v[kSweepTiles];
    if constexpr (!BWD) {
#pragma unroll
      for (int u = 0; u < kSweepTiles; ++u)
        load_leaf<T>(pa, (t0 + u) * kTile + lpos, len, -__builtin_huge_val(), x[u]);
#pragma unroll
      for (int u = 0; u < kSweepTiles; ++u)
        v[u] = leaf_exp_sum<A>(x[u], m, (t0 + u) * kTile + lpos, len);
    } else {
      A gg[kSweepTiles][kLeaf];
#pragma unroll
      for (int u = 0; u < kSweepTiles; ++u) {
        load_leaf<T>(pa, (t0 + u) * kTile + lpos, len, A(0), x[u]);
        load_leaf<T>(pg, (t0 + u) * kTile + lpos, len, A(0), gg[u]);
      }
#pragma unroll
      for (int u = 0; u < kSweepTiles; ++u) v[u] = leaf_dot<A>(x[u], gg[u]);
    }
#pragma unroll
    for (int u = 0; u < kSweepTiles; ++u) v[u] = group_sum<A, 64>(v[u]);
#pragma unroll
    for (int u = 0; u < kSweepTiles; ++u)
      if (t0 + u < tiles) stack_push<A>(stk, t0 + u, v[u], lane);
  }
  const A s = stack_fold<A>(stk, tiles);
  for (int64_t t0 = 0; t0 < tiles; t0 += kSweepTiles) {
    A x[kSweepTiles][kLeaf];
    T res[kSweepTiles][kLeaf];
    if constexpr (!BWD) {
#pragma unroll
      for (int u = 0; u < kSweepTiles; ++u)
        load_leaf<T>(pa, (t0 + u) * kTile + lpos, len, -__builtin_huge_val(), x[u]);
#pragma unroll
      for (int u = 0; u < kSweepTiles; ++u) {
        (void)leaf_exp_sum<A>(x[u], m, (t0 + u) * kTile + lpos, len);
        leaf_divide<T>(x[u], s, res[u]);
      }
    } else {
      A gg[kSweepTiles][kLeaf];
#pragma unroll
      for (int u = 0; u < kSweepTiles; ++u) {
        load_leaf<T>(pa, (t0 + u) * kTile + lpos, len, A(0), x[u]);
        load_leaf<T>(pg, (t0 + u) * kTile + lpos, len, A(0), gg[u]);
      }
#pragma unroll
      for (int u = 0; u < kSweepTiles; ++u) leaf_grad<T>(x[u], gg[u], s, res[u]);
    }
#pragma unroll
    for (int u = 0; u < kSweepTiles; ++u)
      store_leaf<T>(po, (t0 + u) * kTile + lpos, len, res[u]);
  }
}

template <typename T, bool BWD>
__device__ __forceinline__ void row_by_wave(const T* __restrict__ a, const T* __restrict__ g,
                                            T* __restrict__ out, int64_t j0, int64_t len,
                                            int lane) {
  if (len <= kTile)
    row_in_registers<T, 64, BWD>(a, g, out, j0, len, lane);
  else
    row_in_tiles<T, BWD>(a, g, out, j0, len, lane);
}

template <typename T, typename I, int LG, bool BWD>
__global__ void __launch_bounds__(kBlock)
    edge_softmax_kernel(const I* __restrict__ rp, const T* __restrict__ a, const T* __restrict__ g,
                        T* __restrict__ out, int64_t row_begin, int64_t nrows,
                        int64_t block_base) {
#pragma clang fp contract(off)
  constexpr int GPW = 64 / LG;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t gi = ((block_base + (int64_t)blockIdx.x) * (kBlock / 64) + wave) * GPW + lane / LG;
  Item it;
  const bool has = work_item<I>(rp, gi, row_begin, nrows, INT64_MAX, nullptr, nullptr, nullptr,
                                &it, true);
  const int64_t j0 = has ? it.j0 : 0;
  const int64_t len = has ? it.j1 - it.j0 : 0;
  if constexpr (LG == 64) {
    row_by_wave<T, BWD>(a, g, out, j0, len, lane);  // uniform over the wave
  } else {
    const bool fits = len <= (int64_t)LG * kLeaf;
    row_in_registers<T, LG, BWD>(a, g, out, j0, fits ? len : 0, lane & (LG - 1));
    // the rows that do not fit their group: the whole wave, one row after another
    unsigned long long todo = __ballot(!fits && (lane & (LG - 1)) == 0);
    while (todo != 0) {
      const int src = __ffsll((long long)todo) - 1;
      todo &= todo - 1;
      const int64_t wj0 = __shfl(j0, src, 64), wlen = __shfl(len, src, 64);
      row_by_wave<T, BWD>(a, g, out, wj0, wlen, lane);
    }
  }
}

struct EsmArgs {
  const char* fn;
  hipStream_t s;
  const void *rp, *a, *g;
  void* out;
  int64_t m, nnz, row_begin, nrows;
  const ofx_spmm_options* opts;
};

template <typename T, typename I, int LG, bool BWD>
int esm_cfg(const EsmArgs& x) {
  return launch_cut_grid(x.nrows, (kBlock / 64) * (64 / LG), [&](dim3 grid, int64_t b0) {
    hipLaunchKernelGGL((edge_softmax_kernel<T, I, LG, BWD>), grid, dim3(kBlock), 0, x.s,
                       static_cast<const I*>(x.rp), static_cast<const T*>(x.a),
                       static_cast<const T*>(x.g), static_cast<T*>(x.out), x.row_begin, x.nrows,
                       b0);
  });
}

// The lane group by the family's rule (edge_softmax.h launch_group_lanes).
template <bool BWD>
int esm_launch(int idx_dtype, int val_dtype, const EsmArgs& x) {
  return by_types(idx_dtype, val_dtype, [&](auto* tp, auto* ip) -> int {
    using T = std::remove_pointer_t<decltype(tp)>;
    using I = std::remove_pointer_t<decltype(ip)>;
    return with_group_lanes(launch_group_lanes(x.m, x.nrows, x.nnz, x.opts), [&](auto lanes) {
      return esm_cfg<T, I, decltype(lanes)::value, BWD>(x);
    });
  });
}

template <bool BWD>
int esm_entry(const char* fn, void* stream, int idx_dtype, int val_dtype, int64_t m, int64_t nnz,
              const void* row_ptr, const void* a, const void* g, void* out, int64_t row_begin,
              int64_t row_end, const ofx_spmm_options* opts) {
  int rc = check_edge_softmax_args(fn, idx_dtype, val_dtype, m, nnz, row_begin, row_end);
  if (rc) return rc;
  if (row_end == row_begin || nnz == 0) return OFX_OK;
  OFX_REQUIRE(row_ptr && a && out && (!BWD || g), OFX_EINVAL, "%s: NULL pointer", fn);
  const EsmArgs args{fn, static_cast<hipStream_t>(stream), row_ptr, a, g, out, m, nnz, row_begin,
                     row_end - row_begin, opts};
  return esm_launch<BWD>(idx_dtype, val_dtype, args);
}

}  // namespace
}  // namespace ofx

using namespace ofx;

extern "C" int ofx_edge_softmax_csr_workspace_size(int idx_dtype, int val_dtype, int64_t m,
                                                   int64_t nnz, const ofx_spmm_options* opts,
                                                   size_t* bytes) {
  return ::ofx::guarded(__func__, [&]() -> int {
    return softmax_workspace_size("edge_softmax_csr_workspace_size", idx_dtype, val_dtype, m, 0, 1,
                                  nnz, opts, bytes);
  });
}

extern "C" int ofx_edge_softmax_csr(void* stream, int idx_dtype, int val_dtype, int64_t m,
                                    int64_t nnz, const void* row_ptr, const void* e, void* y,
                                    int64_t row_begin, int64_t row_end, void* workspace,
                                    size_t workspace_bytes, const ofx_spmm_options* opts) {
  return ::ofx::guarded(__func__, [&]() -> int {
    OFX_DEVICE_ENTRY("edge_softmax_csr", opts, workspace, workspace_bytes);
    return esm_entry<false>("edge_softmax_csr", stream, idx_dtype, val_dtype, m, nnz, row_ptr, e,
                            nullptr, y, row_begin, row_end, opts);
  });
}

extern "C" int ofx_edge_softmax_csr_grad(void* stream, int idx_dtype, int val_dtype, int64_t m,
                                         int64_t nnz, const void* row_ptr, const void* y,
                                         const void* g, void* de, int64_t row_begin,
                                         int64_t row_end, void* workspace, size_t workspace_bytes,
                                         const ofx_spmm_options* opts) {
  return ::ofx::guarded(__func__, [&]() -> int {
    OFX_DEVICE_ENTRY("edge_softmax_csr_grad", opts, workspace, workspace_bytes);
    return esm_entry<true>("edge_softmax_csr_grad", stream, idx_dtype, val_dtype, m, nnz, row_ptr,
                           y, g, de, row_begin, row_end, opts);
  });
}
