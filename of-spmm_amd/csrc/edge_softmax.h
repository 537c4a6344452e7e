// edge_softmax.h — what the kCPU kernels (edge_softmax_cpu.cpp) and the HIP kernels
// (edge_softmax.hip, edge_softmax_heads.hip) of ops "edge_softmax_csr", "edge_softmax_csr_heads"
// and of their gradients share: the exponential, the constants of the sum's order, the host's row
// steps, the argument checks and the workspace query of their C-ABI entries and, for the HIP units,
// the host side of a launch (the lane-group rule, the packed-path predicate), the device steps of a
// leaf, the lane-group butterflies and the tile stack (contract in include/ofx_spmm.h, DESIGN.md
// §3e and §3f).  The multi-head rows take a leaf source, so that gat_softmax_heads.hip (DESIGN.md
// §3h) runs the same rows on scores it forms from a gather; gat_softmax_cpu.cpp shares the host's
// row steps.
#ifndef OFX_EDGE_SOFTMAX_H_
#define OFX_EDGE_SOFTMAX_H_

#include <initializer_list>
#include <type_traits>
#include <vector>

#include "ofx_internal.h"
#include "spmm_common.h"
#include "spmm_extremum.h"

namespace ofx {
namespace esm {

// The sum's order (the SDDMM's, along the row): leaves of kLeaf consecutive positions, summed
// sequentially from +0; the leaves, zero-padded to a power of two, added pairwise level by level.
constexpr int kLeaf = 8;
// The HIP kernels cut a row longer than kTile into tiles of kTileLeaves leaves (one leaf per lane
// of a wave) and add the tile values pairwise in tile order: the same tree.  Rows of at most
// kTile elements are held in registers (the widest lane group is the wave).
constexpr int kTileLeaves = 64;
constexpr int kTile = kTileLeaves * kLeaf;

// exp(t) for t <= 0 in the accumulation type, from IEEE-exact steps only (multiply, add,
// subtract, divide in f64, rint to nearest even, a power of two assembled from exponent bits),
// each rounded separately, so that the host and the device return the same bits.  No library or
// hardware transcendental.
//   t below the cut-off (f32 -87, f64 -708), -inf included: +0; no result is subnormal
//   t == +-0: exactly 1;  NaN: the canonical quiet NaN
// A positive t is never passed (t = e - max(e)).  exp_acc<A> is the entry; exp_acc_of are its two
// forms.
// f32: Cody-Waite reduction t = k ln2 + r with ln2 = C1 + C2 (k C1 is exact), the Cephes expf
// degree-5 polynomial, p = (poly(r) * (r * r) + r) + 1, times 2^k.  -87 <= t gives k >= -126 and
// a result above 1.6e-38, the smallest normal being 1.18e-38.
OFX_HD float exp_acc_of(float t) {
#pragma clang fp contract(off)
  if (t != t) return __builtin_nanf("");
  if (t < -87.0f) return 0.0f;
  const float k = __builtin_rintf(t * 1.44269504088896341f);
  float r = t - k * 0.693359375f;
  r = r - k * -2.12194440e-4f;
  float p = 1.9875691500e-4f;
  p = p * r + 1.3981999507e-3f;
  p = p * r + 8.3334519073e-3f;
  p = p * r + 4.1665795894e-2f;
  p = p * r + 1.6666665459e-1f;
  p = p * r + 5.0000001201e-1f;
  const float z = r * r;
  p = p * z;
  p = p + r;
  p = p + 1.0f;
  const float scale = bits_to_f32((uint32_t)((int)k + 127) << 23);
  return p * scale;
}

// f64: the Cephes exp rational form, e^r = 1 + 2 r P(r^2) / (Q(r^2) - r P(r^2)), with the same
// reduction (C1 = 0.693145751953125).  -708 <= t gives k >= -1021 and a result above 3.3e-308,
// the smallest normal being 2.2e-308.
OFX_HD double exp_acc_of(double t) {
#pragma clang fp contract(off)
  if (t != t) return __builtin_nan("");
  if (t < -708.0) return 0.0;
  const double k = __builtin_rint(t * 1.4426950408889634073599);
  double r = t - k * 6.93145751953125e-1;
  r = r - k * 1.42860682030941723212e-6;
  const double z = r * r;
  double pp = 1.26177193074810590878e-4;
  pp = pp * z + 3.02994407707441961300e-2;
  pp = pp * z + 9.99999999999999999910e-1;
  pp = pp * r;
  double qq = 3.00198505138664455042e-6;
  qq = qq * z + 2.52448340349684104192e-3;
  qq = qq * z + 2.27265548208155028766e-1;
  qq = qq * z + 2.00000000000000000009e0;
  double p = pp / (qq - pp);
  p = p * 2.0;
  p = p + 1.0;
  const double scale =
      __builtin_bit_cast(double, (uint64_t)((int64_t)k + 1023) << 52);
  return p * scale;
}

template <typename A>
OFX_HD A exp_acc(A t) {
  return exp_acc_of(t);
}

// ---- the row on the host (the kCPU kernels: edge_softmax_cpu.cpp, gat_softmax_cpu.cpp) -------------
// The contract's sum of x[0 .. len): leaves of kLeaf positions from +0, zero-padded to a power of
// two, pairwise level by level.  `leaf` is scratch.
template <typename A>
A tree_sum(const A* x, int64_t len, std::vector<A>& leaf) {
#pragma clang fp contract(off)
  const int64_t leaves = (len + kLeaf - 1) / kLeaf;
  int64_t padded = 1;
  while (padded < leaves) padded *= 2;
  leaf.assign((size_t)padded, A(0));
  for (int64_t i = 0; i < leaves; ++i) {
    A s = A(0);
    const int64_t end = (i + 1) * kLeaf < len ? (i + 1) * kLeaf : len;
    for (int64_t p = i * kLeaf; p < end; ++p) s = s + x[p];
    leaf[(size_t)i] = s;
  }
  for (int64_t w = 1; w < padded; w *= 2)
    for (int64_t i = 0; i < padded; i += 2 * w) leaf[(size_t)i] = leaf[(size_t)i] + leaf[(size_t)(i + w)];
  return leaf[0];
}

// One head's row: x[0 .. len) holds the loaded scores and is overwritten with their exponentials;
// y[p * stride] = the softmax rounded to T.  len > 0.
template <typename T>
void softmax_row(typename Num<T>::acc* x, int64_t len, std::vector<typename Num<T>::acc>& leaf,
                 T* y, int64_t stride) {
#pragma clang fp contract(off)
  using A = typename Num<T>::acc;
  A best = x[0];
  for (int64_t p = 1; p < len; ++p) best = better(x[p], best, true) ? x[p] : best;
  for (int64_t p = 0; p < len; ++p) {
    const A t = x[p] - best;
    x[p] = exp_acc<A>(t);
  }
  const A s = tree_sum(x, len, leaf);
  for (int64_t p = 0; p < len; ++p) {
    const A q = x[p] / s;
    y[p * stride] = Num<T>::store(canonical_nan(q));
  }
}

// One head's row of the gradient: y and g at element stride `stride`; sink(p, de) takes
// de = y[p] * (g[p] - sum(y * g)) rounded to T, position by position.  q: scratch of len values,
// not read once the sum is formed, so a sink may reuse it.  len > 0.
template <typename T, typename Sink>
void softmax_grad_row(const T* y, const T* g, int64_t stride, int64_t len,
                      typename Num<T>::acc* q, std::vector<typename Num<T>::acc>& leaf,
                      Sink&& sink) {
#pragma clang fp contract(off)
  using A = typename Num<T>::acc;
  for (int64_t p = 0; p < len; ++p) {
    const A prod = Num<T>::load(y[p * stride]) * Num<T>::load(g[p * stride]);
    q[p] = prod;
  }
  const A d = tree_sum(q, len, leaf);
  for (int64_t p = 0; p < len; ++p) {
    const A diff = Num<T>::load(g[p * stride]) - d;
    const A prod = Num<T>::load(y[p * stride]) * diff;
    sink(p, Num<T>::store(canonical_nan(prod)));
  }
}

// ---- argument checks shared by the device and host entries ----------------------------------
static inline int check_edge_softmax_args(const char* fn, int idx_dtype, int val_dtype, int64_t m,
                                          int64_t nnz, int64_t row_begin, int64_t row_end) {
  if (const int rc = check_types_sizes(fn, idx_dtype, val_dtype, m, 0, 0, nnz)) return rc;
  return check_row_range(fn, row_begin, row_end, m);
}

// The multi-head entries (ops "edge_softmax_csr_heads" / "_grad"): e, y, g, de are T[nnz, heads].
// int32 indices need only address the CSR itself; offsets into e are formed in 64 bits.
static inline int check_edge_softmax_heads_args(const char* fn, int idx_dtype, int val_dtype,
                                                int64_t m, int64_t heads, int64_t nnz,
                                                int64_t row_begin, int64_t row_end) {
  OFX_REQUIRE(heads >= 0 && (heads == 0 || nnz <= INT64_MAX / heads), OFX_EINVAL,
              "%s: bad heads=%lld for nnz=%lld", fn, (long long)heads, (long long)nnz);
  return check_edge_softmax_args(fn, idx_dtype, val_dtype, m, nnz, row_begin, row_end);
}

// The body of the family's *_workspace_size entries (the edge softmax: heads = 1 and k = 0 for the
// single-head op; the GAT weights of gat_softmax_heads.hip, whose columns number k): no op of the
// family plans or keeps partials, so a valid shape needs 0 bytes.
static inline int softmax_workspace_size(const char* fn, int idx_dtype, int val_dtype, int64_t m,
                                         int64_t k, int64_t heads, int64_t nnz,
                                         const ofx_spmm_options* opts, size_t* bytes) {
  OFX_READ_OPTIONS(opts, fn);
  OFX_REQUIRE(bytes != nullptr, OFX_EINVAL, "%s: NULL bytes", fn);
  OFX_REQUIRE(k >= 0, OFX_EINVAL, "%s: negative k=%lld", fn, (long long)k);
  if (const int rc = check_edge_softmax_heads_args(fn, idx_dtype, val_dtype, m, heads, nnz, 0, m))
    return rc;
  *bytes = 0;
  return OFX_OK;
}

}  // namespace esm
}  // namespace ofx

#if defined(__HIP__)
#include <hip/hip_runtime.h>

#include "spmm_items_dev.h"

namespace ofx {
namespace esm {

// ---- the host side of a launch, shared by the HIP units of the family ---------------------------
// The lane group of a launch: the narrowest of 1, 4, 16, 64 lanes whose capacity (kLeaf positions
// per lane) is at least `want`.  Speed only: the bits do not depend on it, so no test can see it
// move; its boundaries are pinned here.
constexpr int group_lanes(int64_t want) {
  int lg = 1;
  while (lg < 64 && (int64_t)lg * kLeaf < want) lg *= 4;
  return lg;
}
static_assert(group_lanes(0) == 1 && group_lanes(8) == 1 && group_lanes(9) == 4 &&
                  group_lanes(32) == 4 && group_lanes(33) == 16 && group_lanes(128) == 16 &&
                  group_lanes(129) == 64,
              "the lane-group rule's boundaries");

// `want` of a launch over nrows > 0 of the matrix's m rows: twice the mean degree of its rows, so
// that most rows fit their group and few wait for the wave.
inline int launch_group_lanes(int64_t m, int64_t nrows, int64_t nnz, const ofx_spmm_options* opts) {
  return group_lanes(2 * (launch_nnz(m, nrows, nnz, opts) / nrows));
}

// f(std::integral_constant<int, LG>) for a run-time lane group: a kernel's instantiation per
// width (spmm_forward_rules.h with_lanes).
template <typename F>
int with_group_lanes(int lg, F&& f) {
  switch (lg) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 4: return f(std::integral_constant<int, 4>{});
    case 16: return f(std::integral_constant<int, 16>{});
    default: return f(std::integral_constant<int, 64>{});
  }
}

// ---- what the HIP units share on the device -----------------------------------------------------
// The steps of one row's leaf (kLeaf positions in a lane's registers), the lane-group butterflies
// and the binary-counter stack of a long row's tiles.  The units take every arithmetic step from
// here, so a head's column has the single-head op's bits by construction.
// These kernels' code generation moves with the inlining structure: passing g + off instead of
// g, off, or building a leaf source at the call site instead of inside a wrapper, changes the
// registers and instruction counts of every kernel that goes through it.  A change here is checked
// by per-kernel assembly comparison (`make asm`, scripts/kernel_asm_diff.py); DESIGN.md §3h has
// the record of what was tried.

// The rounding to T of a quotient or product, as a step of its own: the value passes through a
// register between the arithmetic and the conversion, so no mixed-precision multiply-convert
// (spmm_extremum.h signed_product) can fuse the two roundings.  NaN: the canonical quiet NaN.
template <typename T>
__device__ __forceinline__ T store_rounded(typename Num<T>::acc v) {
  v = canonical_nan(v);
  if constexpr (sizeof(T) == 2) asm volatile("" : "+v"(v));
  return Num<T>::store(v);
}

template <typename A, int LG>
__device__ __forceinline__ A group_max(A best) {
#pragma unroll
  for (int x = 1; x < LG; x <<= 1) {
    const A o = __shfl_xor(best, x, 64);
    best = better(o, best, true) ? o : best;
  }
  return best;
}

template <typename A, int LG>
__device__ __forceinline__ A group_sum(A t) {
#pragma clang fp contract(off)
#pragma unroll
  for (int x = 1; x < LG; x <<= 1) t = t + __shfl_xor(t, x, 64);
  return t;
}

template <typename A>
__device__ __forceinline__ A leaf_max(const A (&x)[kLeaf], A best) {
#pragma unroll
  for (int i = 0; i < kLeaf; ++i) best = better(x[i], best, true) ? x[i] : best;
  return best;
}

// x <- exp_acc(x - m) at the leaf's positions inside the row, +0 at the others; the leaf's sum.
template <typename A>
__device__ __forceinline__ A leaf_exp_sum(A (&x)[kLeaf], A m, int64_t pos, int64_t len) {
#pragma clang fp contract(off)
  A s = A(0);
#pragma unroll
  for (int i = 0; i < kLeaf; ++i) {
    const A t = x[i] - m;
    const A v = exp_acc<A>(t);
    x[i] = pos + i < len ? v : A(0);
    s = s + x[i];
  }
  return s;
}

// The backward's leaf sum of q = y * g (absent positions hold +0 in both).
template <typename A>
__device__ __forceinline__ A leaf_dot(const A (&y)[kLeaf], const A (&g)[kLeaf]) {
#pragma clang fp contract(off)
  A s = A(0);
#pragma unroll
  for (int i = 0; i < kLeaf; ++i) {
    const A q = y[i] * g[i];
    s = s + q;
  }
  return s;
}

template <typename T>
__device__ __forceinline__ void leaf_divide(const typename Num<T>::acc (&x)[kLeaf],
                                            typename Num<T>::acc s, T (&y)[kLeaf]) {
#pragma unroll
  for (int i = 0; i < kLeaf; ++i) y[i] = store_rounded<T>(x[i] / s);
}

template <typename T>
__device__ __forceinline__ void leaf_grad(const typename Num<T>::acc (&y)[kLeaf],
                                          const typename Num<T>::acc (&g)[kLeaf],
                                          typename Num<T>::acc d, T (&de)[kLeaf]) {
#pragma clang fp contract(off)
  using A = typename Num<T>::acc;
#pragma unroll
  for (int i = 0; i < kLeaf; ++i) {
    const A diff = g[i] - d;
    de[i] = store_rounded<T>(y[i] * diff);
  }
}

// The binary-counter stack of tile values, level l in lane l.  Tile t (value v, the same in every
// lane) merges with the levels of t's trailing one bits, earlier subtrees on the left.
template <typename A>
__device__ __forceinline__ void stack_push(A& stk, int64_t t, A v, int lane) {
#pragma clang fp contract(off)
  int l = 0;
  for (; (t >> l) & 1; ++l) v = __shfl(stk, l, 64) + v;
  if (lane == l) stk = v;
}

// The tree's root after `tiles` pushes: the occupied levels, low to high, the higher (earlier)
// subtree on the left; the zero tiles that pad to a power of two add nothing.
template <typename A>
__device__ __forceinline__ A stack_fold(A stk, int64_t tiles) {
#pragma clang fp contract(off)
  A s = A(0);
  bool have = false;
  for (int l = 0; (tiles >> l) != 0; ++l) {
    if ((tiles >> l) & 1) {
      const A v = __shfl(stk, l, 64);
      s = have ? v + s : v;
      have = true;
    }
  }
  return s;
}

// ---- the multi-head rows (edge_softmax_heads.hip, gat_softmax_heads.hip, phase 2 of
// graph_attention_heads.hip) ----------------------------------------------------------------------
// Pointers are not restrict-qualified: the fused attention kernel normalises its scores in place
// (a == out; every position is read and written by the same lane, reads first).
}  // namespace esm

namespace esmh {  // a namespace of its own: edge_softmax.hip has single-head steps of the same names

using namespace esm;
using item::u32x2;
using item::u32x4;

// V consecutive heads of one position as one load or store.
template <int BYTES>
struct RawOf;
template <>
struct RawOf<2> {
  using type = uint16_t;
};
template <>
struct RawOf<4> {
  using type = uint32_t;
};
template <>
struct RawOf<8> {
  using type = u32x2;
};
template <>
struct RawOf<16> {
  using type = u32x4;
};

template <typename T, int V>
struct HeadVec {
  using Raw = typename RawOf<V * sizeof(T)>::type;
  struct Elems {
    T v[V];
  };
  static_assert(sizeof(Elems) == sizeof(Raw), "a head vector is one load");
};

// Heads a lane holds on the packed path.
template <typename T>
constexpr int packed_heads() {
  return sizeof(T) == 8 ? 2 : 4;
}

// Whether a launch takes the packed path (host): whole vectors of V heads, and every base that is
// loaded or stored as one aligned to V * sizeof(T).  A NULL base (an operand the direction does
// not have) counts as aligned.
template <typename T, int V>
bool heads_packed(int64_t heads, std::initializer_list<const void*> bases) {
  bool ok = heads % V == 0;
  for (const void* p : bases) ok = ok && (uintptr_t)p % (V * sizeof(T)) == 0;
  return ok;
}

// Item gi = row * G + head group, in 32 bits where both fit.
__device__ __forceinline__ void split_item(int64_t gi, int64_t G, int64_t* row, int64_t* hg) {
  if ((((uint64_t)gi | (uint64_t)G) >> 32) == 0) {
    const uint32_t r = (uint32_t)gi / (uint32_t)G;
    *row = r;
    *hg = (uint32_t)gi - r * (uint32_t)G;
  } else {
    *row = gi / G;
    *hg = gi - *row * G;
  }
}

// x[v][i] = load(p[(pos + i) * H + v]) for the leaf's positions inside [0, len), `fill` for the
// others; p points at the row's first position and the lane's first head.  len > 0.
template <typename T, int V>
__device__ __forceinline__ void load_leaf_heads(const T* p, int64_t H, int64_t pos,
                                                int64_t len, typename Num<T>::acc fill,
                                                typename Num<T>::acc (&x)[V][kLeaf]) {
  using HV = HeadVec<T, V>;
#pragma unroll
  for (int i = 0; i < kLeaf; ++i) {
    const bool in = pos + i < len;
    const int64_t q = in ? pos + i : len - 1;
    const typename HV::Raw raw = *reinterpret_cast<const typename HV::Raw*>(p + q * H);
    const typename HV::Elems el = __builtin_bit_cast(typename HV::Elems, raw);
#pragma unroll
    for (int v = 0; v < V; ++v) x[v][i] = in ? Num<T>::load(el.v[v]) : fill;
  }
}

template <typename T, int V>
__device__ __forceinline__ void store_leaf_heads(T* p, int64_t H, int64_t pos,
                                                 int64_t len, const T (&y)[V][kLeaf]) {
  using HV = HeadVec<T, V>;
#pragma unroll
  for (int i = 0; i < kLeaf; ++i) {
    if (pos + i < len) {
      typename HV::Elems el;
#pragma unroll
      for (int v = 0; v < V; ++v) el.v[v] = y[v][i];
      *reinterpret_cast<typename HV::Raw*>(p + (pos + i) * H) =
          __builtin_bit_cast(typename HV::Raw, el);
    }
  }
}

// Where a row's leaves come from.  A leaf source has load(pos, len, fill, x): x[v][i] = the value
// of position pos + i and head v for the positions inside [0, len), `fill` for the others (len > 0).
// The memory source reads a T[., H] array: p points at the row's first position and the lane's
// first head.  gat_softmax_heads.hip has one that forms its scores from a gather instead.
template <typename T, int V>
struct MemoryLeaves {
  const T* p;
  int64_t H;
  __device__ __forceinline__ void load(int64_t pos, int64_t len, typename Num<T>::acc fill,
                                       typename Num<T>::acc (&x)[V][kLeaf]) const {
    load_leaf_heads<T, V>(p, H, pos, len, fill, x);
  }
};

// The same for a group that may have no row (len == 0: nothing is loaded).
template <typename T, int V, typename Src>
__device__ __forceinline__ void load_leaf_or_fill(const Src& src, int64_t pos, int64_t len,
                                                  typename Num<T>::acc fill,
                                                  typename Num<T>::acc (&x)[V][kLeaf]) {
  if (len > 0) {
    src.load(pos, len, fill, x);
  } else {
#pragma unroll
    for (int v = 0; v < V; ++v)
#pragma unroll
      for (int i = 0; i < kLeaf; ++i) x[v][i] = fill;
  }
}

// A row of at most 8 LG positions over a group of LG lanes, lane gl holding leaf gl of V heads.
// off: the element offset in g and out of the row's first position and the lane's first head.
// len == 0: nothing is loaded or stored (a group with no item, or whose row the wave takes over).
// Forward: src = e, out = y.  Backward: src = y, g = the upstream gradient, out = de.
template <typename T, int V, int LG, bool BWD, typename Src>
__device__ __forceinline__ void row_in_registers_of(const Src& src, const T* g, T* out, int64_t H,
                                                    int64_t off, int64_t len, int gl) {
  using A = typename Num<T>::acc;
  const int64_t pos = (int64_t)gl * kLeaf;
  A x[V][kLeaf];
  T res[V][kLeaf];
  if constexpr (!BWD) {
    load_leaf_or_fill<T, V>(src, pos, len, -__builtin_huge_val(), x);
#pragma unroll
    for (int v = 0; v < V; ++v) {
      const A m = group_max<A, LG>(leaf_max<A>(x[v], x[v][0]));
      const A s = group_sum<A, LG>(leaf_exp_sum<A>(x[v], m, pos, len));
      leaf_divide<T>(x[v], s, res[v]);
    }
  } else {
    A gg[V][kLeaf];
    load_leaf_or_fill<T, V>(src, pos, len, A(0), x);
    load_leaf_or_fill<T, V>(MemoryLeaves<T, V>{g + off, H}, pos, len, A(0), gg);
#pragma unroll
    for (int v = 0; v < V; ++v) {
      const A d = group_sum<A, LG>(leaf_dot<A>(x[v], gg[v]));
      leaf_grad<T>(x[v], gg[v], d, res[v]);
    }
  }
  store_leaf_heads<T, V>(out + off, H, pos, len, res);
}

// The row from memory: off is the offset in a as well.
template <typename T, int V, int LG, bool BWD>
__device__ __forceinline__ void row_in_registers(const T* a, const T* g,
                                                 T* out, int64_t H, int64_t off,
                                                 int64_t len, int gl) {
  row_in_registers_of<T, V, LG, BWD>(MemoryLeaves<T, V>{a + off, H}, g, out, H, off, len, gl);
}

// A row of more than kTile positions, by the whole wave, for V heads; SW tiles in flight (the
// number has no numeric effect: tiles are pushed in tile order).  Every pass loads its leaves from
// the source again.
template <typename T, int V, bool BWD, typename Src>
__device__ __forceinline__ void row_in_tiles_of(const Src& pa, const T* g, T* out, int64_t H,
                                                int64_t off, int64_t len, int lane) {
  using A = typename Num<T>::acc;
  constexpr int SW = V == 1 ? 2 : 1;
  const T* pg = BWD ? g + off : nullptr;
  T* po = out + off;
  const int64_t tiles = (len + kTile - 1) / kTile;
  const int64_t lpos = (int64_t)lane * kLeaf;
  A m[V];
  if constexpr (!BWD) {
    A best[V];
#pragma unroll
    for (int v = 0; v < V; ++v) best[v] = -__builtin_huge_val();
    for (int64_t t0 = 0; t0 < tiles; t0 += SW) {
      A x[SW][V][kLeaf];
#pragma unroll
      for (int u = 0; u < SW; ++u)
        pa.load((t0 + u) * kTile + lpos, len, -__builtin_huge_val(), x[u]);
#pragma unroll
      for (int u = 0; u < SW; ++u)
#pragma unroll
        for (int v = 0; v < V; ++v) best[v] = leaf_max<A>(x[u][v], best[v]);
    }
#pragma unroll
    for (int v = 0; v < V; ++v) m[v] = group_max<A, 64>(best[v]);
  }
  A stk[V];
#pragma unroll
  for (int v = 0; v < V; ++v) stk[v] = A(0);
  for (int64_t t0 = 0; t0 < tiles; t0 += SW) {
    A x[SW][V][kLeaf], val[SW][V];
    if constexpr (!BWD) {
#pragma unroll
      for (int u = 0; u < SW; ++u)
        pa.load((t0 + u) * kTile + lpos, len, -__builtin_huge_val(), x[u]);
#pragma unroll
      for (int u = 0; u < SW; ++u)
#pragma unroll
        for (int v = 0; v < V; ++v)
          val[u][v] = leaf_exp_sum<A>(x[u][v], m[v], (t0 + u) * kTile + lpos, len);
    } else {
      A gg[SW][V][kLeaf];
#pragma unroll
      for (int u = 0; u < SW; ++u) {
        pa.load((t0 + u) * kTile + lpos, len, A(0), x[u]);
        load_leaf_heads<T, V>(pg, H, (t0 + u) * kTile + lpos, len, A(0), gg[u]);
      }
#pragma unroll
      for (int u = 0; u < SW; ++u)
#pragma unroll
        for (int v = 0; v < V; ++v) val[u][v] = leaf_dot<A>(x[u][v], gg[u][v]);
    }
#pragma unroll
    for (int u = 0; u < SW; ++u)
#pragma unroll
      for (int v = 0; v < V; ++v) val[u][v] = group_sum<A, 64>(val[u][v]);
#pragma unroll
    for (int u = 0; u < SW; ++u)
      if (t0 + u < tiles) {
#pragma unroll
        for (int v = 0; v < V; ++v) stack_push<A>(stk[v], t0 + u, val[u][v], lane);
      }
  }
  A s[V];
#pragma unroll
  for (int v = 0; v < V; ++v) s[v] = stack_fold<A>(stk[v], tiles);
  for (int64_t t0 = 0; t0 < tiles; t0 += SW) {
    A x[SW][V][kLeaf];
    T res[SW][V][kLeaf];
    if constexpr (!BWD) {
#pragma unroll
      for (int u = 0; u < SW; ++u)
        pa.load((t0 + u) * kTile + lpos, len, -__builtin_huge_val(), x[u]);
#pragma unroll
      for (int u = 0; u < SW; ++u)
#pragma unroll
        for (int v = 0; v < V; ++v) {
          (void)leaf_exp_sum<A>(x[u][v], m[v], (t0 + u) * kTile + lpos, len);
          leaf_divide<T>(x[u][v], s[v], res[u][v]);
        }
    } else {
      A gg[SW][V][kLeaf];
#pragma unroll
      for (int u = 0; u < SW; ++u) {
        pa.load((t0 + u) * kTile + lpos, len, A(0), x[u]);
        load_leaf_heads<T, V>(pg, H, (t0 + u) * kTile + lpos, len, A(0), gg[u]);
      }
#pragma unroll
      for (int u = 0; u < SW; ++u)
#pragma unroll
        for (int v = 0; v < V; ++v) leaf_grad<T>(x[u][v], gg[u][v], s[v], res[u][v]);
    }
#pragma unroll
    for (int u = 0; u < SW; ++u)
      store_leaf_heads<T, V>(po, H, (t0 + u) * kTile + lpos, len, res[u]);
  }
}

template <typename T, int V, bool BWD>
__device__ __forceinline__ void row_in_tiles(const T* a, const T* g,
                                             T* out, int64_t H, int64_t off,
                                             int64_t len, int lane) {
  row_in_tiles_of<T, V, BWD>(MemoryLeaves<T, V>{a + off, H}, g, out, H, off, len, lane);
}

template <typename T, int V, bool BWD, typename Src>
__device__ __forceinline__ void row_by_wave_of(const Src& src, const T* g, T* out, int64_t H,
                                               int64_t off, int64_t len, int lane) {
  if (len <= kTile)
    row_in_registers_of<T, V, 64, BWD>(src, g, out, H, off, len, lane);
  else
    row_in_tiles_of<T, V, BWD>(src, g, out, H, off, len, lane);
}

template <typename T, int V, bool BWD>
__device__ __forceinline__ void row_by_wave(const T* a, const T* g,
                                            T* out, int64_t H, int64_t off,
                                            int64_t len, int lane) {
  if (len <= kTile)
    row_in_registers<T, V, 64, BWD>(a, g, out, H, off, len, lane);
  else
    row_in_tiles<T, V, BWD>(a, g, out, H, off, len, lane);
}

}  // namespace esmh
}  // namespace ofx
#endif  // __HIP__

#endif  // OFX_EDGE_SOFTMAX_H_
