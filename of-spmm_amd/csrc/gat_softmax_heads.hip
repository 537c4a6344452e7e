// gat_softmax_heads.hip — ops "gat_softmax_csr_heads" and its gradient on gfx950: the attention
// weights of a GAT layer over a CSR, attn[j, h] = softmax over j's row of
// LeakyReLU(s_row[row(j), h] + s_col[col[j], h]), every head on its own, in one launch (contract in
// include/ofx_spmm.h, DESIGN.md §3h "GAT attention weights").
//
// The layout is edge_softmax_heads.hip's: a work item is a (row, head group of V heads), LG lanes
// per item picked from the mean degree, lane t holding leaf t (positions [8t, 8t + 8) of the row)
// for its V heads, rows longer than 8 LG taken over by the whole wave, beyond kTile = 512 positions
// in tiles through the binary-counter stack.  The rows themselves are edge_softmax.h's
// (esmh::row_in_registers_of / row_by_wave_of); the only new step is where a leaf's 8 values come
// from (GatLeaves): the leaf's 8 column indices, 8 gathered s_col vectors of V heads, the item's
// s_row vector (loaded once), one add, the activation and the rounding to T.  No score is ever
// written: in the wave and tile forms every pass forms its scores again from the gather, so attn is
// only written (it keeps __restrict__) and no fence is needed.
//   packed path:  H % V == 0 and s_row, s_col, attn (backward: g, ds, d_row too) aligned to the
//     vector; V = 4 for f32, f16, bf16 and 2 for f64
//   general path: any other H or base; V = 1
// Backward, in the same launch: de (the edge softmax's gradient, rounded to T), ds = de times the
// activation's derivative at the recomputed z, and d_row = the sum of ds along the row in the
// softmax's leaf / tree order.  The tile form folds the stack of the first sum (y g), clears it and
// pushes the second (ds) through it.  d_col is not computed here: it is the multi-head SpMM on the
// transpose (autograd.py), whose order is fixed by that op.
//
// No atomics, no workspace, no allocation, no host synchronisation, no LDS, no scratch.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include "edge_softmax.h"
#include "gat_softmax.h"
#include "spmm_items_dev.h"

namespace ofx {
namespace {

using namespace item;
using namespace esm;
using namespace esmh;
using namespace gsm;

// The leaf source of one (row, head group): scores from the gather instead of from memory.
template <typename T, typename I, int V>
struct GatLeaves {
  using A = typename Num<T>::acc;
  using HV = HeadVec<T, V>;
  const I* ci;     // the row's first nonzero
  const T* s_col;  // the lane's first head of column 0
  int64_t H, K;
  A s_row[V];
  A slope;

  // z[v][i] = s_row[v] + load(s_col[col[pos + i], v]); a position past the row's end is clamped to
  // the row's last one (len > 0), a column outside [0, K) reads +0.  The 8 loads are unconditional.
  __device__ __forceinline__ void sums(int64_t pos, int64_t len, A (&z)[V][kLeaf]) const {
#pragma clang fp contract(off)
#pragma unroll
    for (int i = 0; i < kLeaf; ++i) {
      const int64_t q = pos + i < len ? pos + i : len - 1;
      const int64_t c = (int64_t)ci[q];
      const bool ok = (uint64_t)c < (uint64_t)K;
      typename HV::Raw raw = typename HV::Raw(0);
      if (K > 0) raw = *reinterpret_cast<const typename HV::Raw*>(s_col + (ok ? c : 0) * H);
      const typename HV::Elems el = __builtin_bit_cast(typename HV::Elems, raw);
#pragma unroll
      for (int v = 0; v < V; ++v) {
        const A sc = ok ? Num<T>::load(el.v[v]) : A(0);
        z[v][i] = s_row[v] + sc;
      }
    }
  }

  // The leaf as the softmax reads it: load(e), e = the activation of z rounded to T; `fill` at the
  // positions outside [0, len).
  __device__ __forceinline__ void load(int64_t pos, int64_t len, A fill,
                                       A (&x)[V][kLeaf]) const {
    sums(pos, len, x);
#pragma unroll
    for (int v = 0; v < V; ++v)
#pragma unroll
      for (int i = 0; i < kLeaf; ++i) {
        const T e = store_rounded<T>(leaky<A>(x[v][i], slope));
        x[v][i] = pos + i < len ? Num<T>::load(e) : fill;
      }
  }

  // The activation's derivative at the leaf's positions.
  __device__ __forceinline__ void factors(int64_t pos, int64_t len, A (&f)[V][kLeaf]) const {
    sums(pos, len, f);
#pragma unroll
    for (int v = 0; v < V; ++v)
#pragma unroll
      for (int i = 0; i < kLeaf; ++i) f[v][i] = leaky_factor<A>(f[v][i], slope);
  }
};

// The source of item (row, head group hg) whose row starts at nonzero j0; len == 0: no s_row load.
template <typename T, typename I, int V>
__device__ __forceinline__ GatLeaves<T, I, V> gat_leaves(const I* ci, const T* s_row,
                                                         const T* s_col, int64_t H, int64_t K,
                                                         typename Num<T>::acc slope, int64_t row,
                                                         int64_t hg, int64_t j0, int64_t len) {
  using HV = HeadVec<T, V>;
  GatLeaves<T, I, V> s;
  s.ci = ci + j0;
  s.s_col = s_col + hg * V;
  s.H = H;
  s.K = K;
  s.slope = slope;
  typename HV::Raw raw = typename HV::Raw(0);
  if (len > 0) raw = *reinterpret_cast<const typename HV::Raw*>(s_row + row * H + hg * V);
  const typename HV::Elems el = __builtin_bit_cast(typename HV::Elems, raw);
#pragma unroll
  for (int v = 0; v < V; ++v) s.s_row[v] = Num<T>::load(el.v[v]);
  return s;
}

// ---- the backward's rows ---------------------------------------------------------------------------
// ds = store(load(de) * f) at the leaf's positions; the leaf's sum of load(ds) from +0 (the positions
// outside the row add +0).
template <typename T>
__device__ __forceinline__ typename Num<T>::acc leaf_scale_sum(
    const T (&de)[kLeaf], const typename Num<T>::acc (&f)[kLeaf], int64_t pos, int64_t len,
    T (&ds)[kLeaf]) {
#pragma clang fp contract(off)
  using A = typename Num<T>::acc;
  A s = A(0);
#pragma unroll
  for (int i = 0; i < kLeaf; ++i) {
    const A p = Num<T>::load(de[i]) * f[i];
    ds[i] = store_rounded<T>(p);
    const A t = pos + i < len ? Num<T>::load(ds[i]) : A(0);
    s = s + t;
  }
  return s;
}

// One leaf of V heads: y, g from memory, the factors from the gather; de with the row's d, ds
// stored; val[v] = the leaf's sum of ds.
template <typename T, typename I, int V>
__device__ __forceinline__ void grad_leaf(const GatLeaves<T, I, V>& src,
                                          const typename Num<T>::acc (&x)[V][kLeaf],
                                          const typename Num<T>::acc (&gg)[V][kLeaf],
                                          const typename Num<T>::acc (&d)[V], T* ds, int64_t H,
                                          int64_t pos, int64_t len,
                                          typename Num<T>::acc (&val)[V]) {
  using A = typename Num<T>::acc;
  A f[V][kLeaf];
  T res[V][kLeaf];
  if (len > 0) {
    src.factors(pos, len, f);
  } else {
#pragma unroll
    for (int v = 0; v < V; ++v)
#pragma unroll
      for (int i = 0; i < kLeaf; ++i) f[v][i] = A(1);
  }
#pragma unroll
  for (int v = 0; v < V; ++v) {
    T de[kLeaf];
    leaf_grad<T>(x[v], gg[v], d[v], de);
    val[v] = leaf_scale_sum<T>(de, f[v], pos, len, res[v]);
  }
  store_leaf_heads<T, V>(ds, H, pos, len, res);
}

// A row of at most 8 LG positions over LG lanes.  y, g, ds point at the row's first position and
// the lane's first head; len == 0 loads and stores nothing and gives dr = +0.
template <typename T, typename I, int V, int LG>
__device__ __forceinline__ void grad_row_in_registers(const GatLeaves<T, I, V>& src, const T* y,
                                                      const T* g, T* ds, int64_t H, int64_t len,
                                                      int gl, typename Num<T>::acc (&dr)[V]) {
  using A = typename Num<T>::acc;
  const int64_t pos = (int64_t)gl * kLeaf;
  A x[V][kLeaf], gg[V][kLeaf], d[V];
  load_leaf_or_fill<T, V>(MemoryLeaves<T, V>{y, H}, pos, len, A(0), x);
  load_leaf_or_fill<T, V>(MemoryLeaves<T, V>{g, H}, pos, len, A(0), gg);
#pragma unroll
  for (int v = 0; v < V; ++v) d[v] = group_sum<A, LG>(leaf_dot<A>(x[v], gg[v]));
  grad_leaf<T, I, V>(src, x, gg, d, ds, H, pos, len, dr);
#pragma unroll
  for (int v = 0; v < V; ++v) dr[v] = group_sum<A, LG>(dr[v]);
}

// A row of more than kTile positions, by the whole wave, one tile in flight.
template <typename T, typename I, int V>
__device__ __forceinline__ void grad_row_in_tiles(const GatLeaves<T, I, V>& src, const T* y,
                                                  const T* g, T* ds, int64_t H, int64_t len,
                                                  int lane, typename Num<T>::acc (&dr)[V]) {
  using A = typename Num<T>::acc;
  const int64_t tiles = (len + kTile - 1) / kTile;
  const int64_t lpos = (int64_t)lane * kLeaf;
  A stk[V], d[V];
#pragma unroll
  for (int v = 0; v < V; ++v) stk[v] = A(0);
  for (int64_t t = 0; t < tiles; ++t) {
    A x[V][kLeaf], gg[V][kLeaf];
    load_leaf_heads<T, V>(y, H, t * kTile + lpos, len, A(0), x);
    load_leaf_heads<T, V>(g, H, t * kTile + lpos, len, A(0), gg);
#pragma unroll
    for (int v = 0; v < V; ++v)
      stack_push<A>(stk[v], t, group_sum<A, 64>(leaf_dot<A>(x[v], gg[v])), lane);
  }
#pragma unroll
  for (int v = 0; v < V; ++v) {
    d[v] = stack_fold<A>(stk[v], tiles);
    stk[v] = A(0);  // the second sum goes through the same stack
  }
  for (int64_t t = 0; t < tiles; ++t) {
    A x[V][kLeaf], gg[V][kLeaf], val[V];
    load_leaf_heads<T, V>(y, H, t * kTile + lpos, len, A(0), x);
    load_leaf_heads<T, V>(g, H, t * kTile + lpos, len, A(0), gg);
    grad_leaf<T, I, V>(src, x, gg, d, ds, H, t * kTile + lpos, len, val);
#pragma unroll
    for (int v = 0; v < V; ++v) stack_push<A>(stk[v], t, group_sum<A, 64>(val[v]), lane);
  }
#pragma unroll
  for (int v = 0; v < V; ++v) dr[v] = stack_fold<A>(stk[v], tiles);
}

template <typename T, int V>
__device__ __forceinline__ void store_row_sum(T* p, const typename Num<T>::acc (&dr)[V]) {
  using HV = HeadVec<T, V>;
  typename HV::Elems el;
#pragma unroll
  for (int v = 0; v < V; ++v) el.v[v] = store_rounded<T>(dr[v]);
  *reinterpret_cast<typename HV::Raw*>(p) = __builtin_bit_cast(typename HV::Raw, el);
}

struct Geometry {
  int64_t row_begin, H, G, K, items, block_base;
};

// One (row, head group) by the whole wave (uniform arguments).
template <typename T, typename I, int V, bool BWD>
__device__ __forceinline__ void item_by_wave(const I* ci, const T* s_row, const T* s_col,
                                             const T* y, const T* g, T* out, T* d_row,
                                             const Geometry& q, typename Num<T>::acc slope,
                                             int64_t row, int64_t hg, int64_t j0, int64_t len,
                                             int lane) {
  using A = typename Num<T>::acc;
  const GatLeaves<T, I, V> src = gat_leaves<T, I, V>(ci, s_row, s_col, q.H, q.K, slope, row, hg,
                                                     j0, len);
  const int64_t off = j0 * q.H + hg * V;
  if constexpr (!BWD) {
    row_by_wave_of<T, V, false>(src, nullptr, out, q.H, off, len, lane);
  } else {
    A dr[V];
    if (len <= kTile)
      grad_row_in_registers<T, I, V, 64>(src, y + off, g + off, out + off, q.H, len, lane, dr);
    else
      grad_row_in_tiles<T, I, V>(src, y + off, g + off, out + off, q.H, len, lane, dr);
    if (lane == 0) store_row_sum<T, V>(d_row + row * q.H + hg * V, dr);
  }
}

// Forward: out = attn.  Backward: y = attn, g = the upstream gradient, out = ds, d_row.
template <typename T, typename I, int V, int LG, bool BWD>
__global__ void __launch_bounds__(kBlock)
    gat_softmax_heads_kernel(const I* __restrict__ rp, const I* __restrict__ ci,
                             const T* __restrict__ s_row, const T* __restrict__ s_col,
                             const T* __restrict__ y, const T* __restrict__ g,
                             T* __restrict__ out, T* __restrict__ d_row,
                             typename Num<T>::acc slope, Geometry q) {
#pragma clang fp contract(off)
  using A = typename Num<T>::acc;
  constexpr int GPW = 64 / LG;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t gi =
      ((q.block_base + (int64_t)blockIdx.x) * (kBlock / 64) + wave) * GPW + lane / LG;
  const bool has = gi < q.items;
  int64_t row = 0, hg = 0, j0 = 0, len = 0;
  if (has) {
    split_item(gi, q.G, &row, &hg);
    j0 = (int64_t)rp[q.row_begin + row];
    len = (int64_t)rp[q.row_begin + row + 1] - j0;
  }
  if constexpr (LG == 64) {
    if (has)  // uniform over the wave
      item_by_wave<T, I, V, BWD>(ci, s_row, s_col, y, g, out, d_row, q, slope, row, hg, j0, len,
                                 lane);
  } else {
    const int gl = lane & (LG - 1);
    const bool fits = len <= (int64_t)LG * kLeaf;
    const int64_t glen = fits ? len : 0;
    const GatLeaves<T, I, V> src = gat_leaves<T, I, V>(ci, s_row, s_col, q.H, q.K, slope, row,
                                                       hg, j0, glen);
    const int64_t off = j0 * q.H + hg * V;
    if constexpr (!BWD) {
      row_in_registers_of<T, V, LG, false>(src, nullptr, out, q.H, off, glen, gl);
    } else {
      A dr[V];
      grad_row_in_registers<T, I, V, LG>(src, y + off, g + off, out + off, q.H, glen, gl, dr);
      if (has && fits && gl == 0) store_row_sum<T, V>(d_row + row * q.H + hg * V, dr);
    }
    // the items whose row does not fit their group: the whole wave, one after another
    unsigned long long todo = __ballot(!fits && gl == 0);
    while (todo != 0) {
      const int from = __ffsll((long long)todo) - 1;
      todo &= todo - 1;
      item_by_wave<T, I, V, BWD>(ci, s_row, s_col, y, g, out, d_row, q, slope,
                                 __shfl(row, from, 64), __shfl(hg, from, 64),
                                 __shfl(j0, from, 64), __shfl(len, from, 64), lane);
    }
  }
}

struct GatArgs {
  hipStream_t s;
  const void *rp, *ci, *s_row, *s_col, *y, *g;
  void *out, *d_row;
  double negative_slope;
  int64_t m, k, heads, nnz, row_begin, nrows;
  const ofx_spmm_options* opts;
};

template <typename T, typename I, int V, int LG, bool BWD>
int gat_cfg(const GatArgs& x) {
  using A = typename Num<T>::acc;
  const int64_t G = x.heads / V;
  const int64_t items = x.nrows * G;
  return launch_cut_grid(items, (kBlock / 64) * (64 / LG), [&](dim3 grid, int64_t b0) {
    hipLaunchKernelGGL((gat_softmax_heads_kernel<T, I, V, LG, BWD>), grid, dim3(kBlock), 0, x.s,
                       static_cast<const I*>(x.rp), static_cast<const I*>(x.ci),
                       static_cast<const T*>(x.s_row), static_cast<const T*>(x.s_col),
                       static_cast<const T*>(x.y), static_cast<const T*>(x.g),
                       static_cast<T*>(x.out), static_cast<T*>(x.d_row), (A)x.negative_slope,
                       Geometry{x.row_begin, x.heads, G, x.k, items, b0});
  });
}

// The path and the lane group by the edge softmax's rules (edge_softmax.h heads_packed,
// launch_group_lanes); the forward has no y, g and d_row.
template <typename T, typename I, bool BWD>
int gat_typed(const GatArgs& x) {
  constexpr int V = packed_heads<T>();
  const bool packed =
      heads_packed<T, V>(x.heads, {x.s_row, x.s_col, x.out, x.y, x.g, x.d_row});
  return with_group_lanes(launch_group_lanes(x.m, x.nrows, x.nnz, x.opts), [&](auto lanes) {
    constexpr int LG = decltype(lanes)::value;
    return packed ? gat_cfg<T, I, V, LG, BWD>(x) : gat_cfg<T, I, 1, LG, BWD>(x);
  });
}

template <bool BWD>
int gat_entry(const char* fn, void* stream, int idx_dtype, int val_dtype, int64_t m, int64_t k,
              int64_t heads, int64_t nnz, const void* row_ptr, const void* col_idx,
              const void* s_row, const void* s_col, double negative_slope, const void* y,
              const void* g, void* out, void* d_row, int64_t row_begin, int64_t row_end,
              const ofx_spmm_options* opts) {
  bool nothing = false;
  if (const int rc = check_gat_softmax_args(fn, BWD, idx_dtype, val_dtype, m, k, heads, nnz,
                                            row_ptr, col_idx, s_row, s_col, negative_slope, y, g,
                                            out, d_row, row_begin, row_end, &nothing))
    return rc;
  if (nothing) return OFX_OK;
  const GatArgs x{static_cast<hipStream_t>(stream), row_ptr, col_idx, s_row, s_col, y, g, out,
                  d_row, negative_slope, m, k, heads, nnz, row_begin, row_end - row_begin, opts};
  return by_types(idx_dtype, val_dtype, [&](auto* tp, auto* ip) -> int {
    return gat_typed<std::remove_pointer_t<decltype(tp)>, std::remove_pointer_t<decltype(ip)>,
                     BWD>(x);
  });
}

}  // namespace
}  // namespace ofx

using namespace ofx;

extern "C" int ofx_gat_softmax_csr_heads_workspace_size(int idx_dtype, int val_dtype, int64_t m,
                                                        int64_t k, int64_t heads, int64_t nnz,
                                                        const ofx_spmm_options* opts,
                                                        size_t* bytes) {
  return ::ofx::guarded(__func__, [&]() -> int {
    return softmax_workspace_size("gat_softmax_csr_heads_workspace_size", idx_dtype, val_dtype, m,
                                  k, heads, nnz, opts, bytes);
  });
}

extern "C" int ofx_gat_softmax_csr_heads(void* stream, int idx_dtype, int val_dtype, int64_t m,
                                         int64_t k, int64_t heads, int64_t nnz,
                                         const void* row_ptr, const void* col_idx,
                                         const void* s_row, const void* s_col,
                                         double negative_slope, void* attn, int64_t row_begin,
                                         int64_t row_end, void* workspace, size_t workspace_bytes,
                                         const ofx_spmm_options* opts) {
  return ::ofx::guarded(__func__, [&]() -> int {
    OFX_DEVICE_ENTRY("gat_softmax_csr_heads", opts, workspace, workspace_bytes);
    return gat_entry<false>("gat_softmax_csr_heads", stream, idx_dtype, val_dtype, m, k, heads,
                            nnz, row_ptr, col_idx, s_row, s_col, negative_slope, nullptr, nullptr,
                            attn, nullptr, row_begin, row_end, opts);
  });
}

extern "C" int ofx_gat_softmax_csr_heads_grad(void* stream, int idx_dtype, int val_dtype,
                                              int64_t m, int64_t k, int64_t heads, int64_t nnz,
                                              const void* row_ptr, const void* col_idx,
                                              const void* s_row, const void* s_col,
                                              double negative_slope, const void* attn,
                                              const void* g, void* ds, void* d_row,
                                              int64_t row_begin, int64_t row_end, void* workspace,
                                              size_t workspace_bytes,
                                              const ofx_spmm_options* opts) {
  return ::ofx::guarded(__func__, [&]() -> int {
    OFX_DEVICE_ENTRY("gat_softmax_csr_heads_grad", opts, workspace, workspace_bytes);
    return gat_entry<true>("gat_softmax_csr_heads_grad", stream, idx_dtype, val_dtype, m, k, heads,
                           nnz, row_ptr, col_idx, s_row, s_col, negative_slope, attn, g, ds, d_row,
                           row_begin, row_end, opts);
  });
}
