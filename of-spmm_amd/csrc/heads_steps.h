// heads_steps.h — the device steps that the multi-head HIP units share: the scores of one work
// item (sddmm_heads.hip and phase 1 of graph_attention_heads.hip) and the in-order accumulation of
// a run of nonzeros into a lane's columns (spmm_heads.hip and phase 3 of
// graph_attention_heads.hip).  Every unit takes these arithmetic steps from here, so the fused
// kernel has the bits of the three ops' composition by construction (contract in
// include/ofx_spmm.h).  Below them, the host side those units and the GATv2
// units share: the layout ladders, the fast path's shape test and the per-nonzero ops' schedule.
// Included by HIP translation units only.
#ifndef OFX_HEADS_STEPS_H_
#define OFX_HEADS_STEPS_H_

#include <hip/hip_runtime.h>

#include "spmm_extremum.h"
#include "spmm_items_dev.h"

namespace ofx {
namespace hsteps {
namespace {  // internal linkage, as spmm_items_dev.h

using namespace item;

constexpr int kLeaf = 8;                      // the SDDMM's leaf: 8 consecutive columns of a head
constexpr int64_t kMaxHeadsN = 256 * kLeaf;   // 64 lanes x 4 leaves

// A lane's leaf in the accumulation type; columns >= n read as +0.
template <typename T, bool ALIGNED>
__device__ __forceinline__ void load_leaf(const T* __restrict__ row, int64_t cb, int64_t n,
                                          typename Num<T>::acc (&x)[kLeaf]) {
  using A = typename Num<T>::acc;
  T raw[kLeaf];
  load_cols<T, kLeaf, ALIGNED>(row, cb, n, Num<T>::store(A(0)), raw);
#pragma unroll
  for (int e = 0; e < kLeaf; ++e) x[e] = Num<T>::load(raw[e]);
}

// The scores of nonzeros [j0, j1) against the row `arow` by a group of LG lanes (gl: the lane in
// the group, gbase: the group's first lane), out[j * heads + h] rounded to T.
// FAST: the group covers the n = H*D columns, a head is `lh` = D/8 leaves (a power of two); the
// rows are 16-byte aligned and kb > 0.  !FAST: the group covers the D columns of `head`.
template <typename T, typename I, int LG, int L, int U, bool FAST>
__device__ __forceinline__ void sddmm_heads_item(const I* __restrict__ col,
                                                 const T* __restrict__ arow,
                                                 const T* __restrict__ B, int64_t ldb, int64_t kb,
                                                 T* out, int64_t heads, int64_t d, int lh,
                                                 int64_t head, int64_t j0, int64_t j1, int gl,
                                                 int gbase) {
#pragma clang fp contract(off)
  using A = typename Num<T>::acc;
  // the columns the group covers: [col0, col0 + w)
  const int64_t col0 = FAST ? 0 : head * d;
  const int64_t w = FAST ? heads * d : d;
  // the tree: `lin` leaves of a head inside a lane, then `seg` lanes of a head
  const int lin = FAST ? (lh < L ? lh : L) : L;
  const int seg = FAST ? (lh / lin) : LG;
  A av[L][kLeaf];
  int hsel[L];  // FAST: the head whose result this lane's leaf l holds after the tree, or -1
#pragma unroll
  for (int l = 0; l < L; ++l) {
    load_leaf<T, FAST>(arow + col0, (int64_t)(gl * L + l) * kLeaf, w, av[l]);
    hsel[l] = -1;
    if constexpr (FAST) {
      const int gleaf = gl * L + l;
      const int h = gleaf / lh;
      if ((l & (lin - 1)) == 0 && gleaf - h * lh == 0 && h < heads) hsel[l] = h;
    }
  }
  for (int64_t jb = j0; jb < j1; jb += LG) {
    const int cnt = (int)((j1 - jb) < LG ? (j1 - jb) : LG);
    const I myc = gl < cnt ? col[jb + gl] : I(0);
    for (int k = 0; k < cnt; k += U) {
      A bv[U][L][kLeaf];
      if constexpr (FAST) {
        // Every load of the round is unconditional and stays a 16-byte word until all are issued
        // (kb > 0 here; as the accumulation below): a slot past the batch's end repeats the
        // batch's last nonzero, a column outside [0, k) reads row 0, a leaf past the row's
        // width reads leaf 0; the last two are then replaced by zeros.
        constexpr int Q = kLeaf * (int)sizeof(T) / 16, PER = 16 / (int)sizeof(T);
        struct Words {
          T v[PER];
        };
        static_assert(sizeof(Words) == sizeof(u32x4), "a 16-byte piece of a leaf");
        u32x4 raw[U][L][Q];
        unsigned inmask = 0;
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int ku = k + u < cnt ? k + u : cnt - 1;
          const int64_t cu = (int64_t)__shfl((int64_t)myc, gbase + (ku & (LG - 1)), 64);
          const bool in = (uint64_t)cu < (uint64_t)kb;
          inmask |= (in ? 1u : 0u) << u;
          const T* brow = B + (in ? cu : 0) * ldb;
#pragma unroll
          for (int l = 0; l < L; ++l) {
            const int64_t cb = (int64_t)(gl * L + l) * kLeaf;
            const u32x4* src = reinterpret_cast<const u32x4*>(brow + (cb < w ? cb : 0));
#pragma unroll
            for (int q = 0; q < Q; ++q) raw[u][l][q] = src[q];
          }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
#pragma unroll
          for (int l = 0; l < L; ++l) {
            const bool keep = ((inmask >> u) & 1u) != 0 && (int64_t)(gl * L + l) * kLeaf < w;
#pragma unroll
            for (int q = 0; q < Q; ++q) {
              const u32x4 r = keep ? raw[u][l][q] : u32x4{0u, 0u, 0u, 0u};
              const Words wd = __builtin_bit_cast(Words, r);
#pragma unroll
              for (int e = 0; e < PER; ++e) bv[u][l][q * PER + e] = Num<T>::load(wd.v[e]);
            }
          }
        }
      } else {
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int64_t cu = (int64_t)__shfl((int64_t)myc, gbase + ((k + u) & (LG - 1)), 64);
          if (k + u < cnt) {
            // a column outside [0, k): the forward gathered a zero row; every leaf reads as out
            // of range and the row's address is never used
            const bool in = (uint64_t)cu < (uint64_t)kb;
#pragma unroll
            for (int l = 0; l < L; ++l)
              load_leaf<T, false>(B + (in ? cu : 0) * ldb + col0,
                                  in ? (int64_t)(gl * L + l) * kLeaf : w, w, bv[u][l]);
          }
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (k + u < cnt) {
          const int64_t j = jb + k + u;
          A leaf[L];
#pragma unroll
          for (int l = 0; l < L; ++l) {
            A s = A(0);
#pragma unroll
            for (int e = 0; e < kLeaf; ++e) s = s + av[l][e] * bv[u][l][e];
            leaf[l] = s;
          }
          // pairwise over the head's leaves in this lane (x < lin: pairs never cross a head)
#pragma unroll
          for (int x = 1; x < L; x <<= 1) {
            if (x < lin) {
#pragma unroll
              for (int l = 0; l < L; l += 2 * x) leaf[l] = leaf[l] + leaf[l + x];
            }
          }
          // the butterfly over the head's lanes (seg > 1 only when the lane holds one head)
          A t = leaf[0];
#pragma unroll
          for (int x = 1; x < LG; x <<= 1)
            if (x < seg) t = t + __shfl_xor(t, x, 64);
          leaf[0] = t;
          if constexpr (FAST) {
#pragma unroll
            for (int l = 0; l < L; ++l)
              // a plain store: the H results of a nonzero are a 16-32 byte piece of a line, and
              // the pieces of consecutive nonzeros merge in L2 (non-temporal, the pieces went out
              // one by one: 11-12.7 ms for f32 N = 128 on the products graph)
              if (hsel[l] >= 0) out[j * heads + hsel[l]] = Num<T>::store(leaf[l]);
          } else {
            if (gl == 0) out[j * heads + head] = Num<T>::store(t);
          }
        }
      }
    }
  }
}

// acc[e] += mul(val[j, head of column cb + e], B[col[j], cb + e]) over nonzeros [j0, j1),
// ascending, for the lane's VEC columns [cb, cb + VEC) of the n = H*D wide row; hd[e]: the head of
// column cb + e (HEADVEC: one head per lane, hd[0]).  Multiply rounded to T, then add in the
// accumulation type.  HEADVEC: 16-byte-aligned rows, D % VEC == 0 and kb > 0.
template <typename T, typename I, int VEC, int LPR, int U, bool HEADVEC>
__device__ __forceinline__ void spmm_heads_accumulate(
    const I* __restrict__ col, const T* val, const T* __restrict__ B, int64_t ldb, int64_t kb,
    int64_t n, int64_t heads, int64_t cb, const int64_t (&hd)[HEADVEC ? 1 : VEC], int64_t j0,
    int64_t j1, int gl, int gbase, typename Num<T>::acc (&acc)[VEC]) {
#pragma clang fp contract(off)
  using A = typename Num<T>::acc;
  constexpr int NV = HEADVEC ? 1 : VEC;  // value loads per lane and nonzero
  const T zero = Num<T>::store(A(0));
  for (int64_t jb = j0; jb < j1; jb += LPR) {
    const int cnt = (int)((j1 - jb) < LPR ? (j1 - jb) : LPR);
    const I myc = gl < cnt ? col[jb + gl] : I(0);
    for (int k = 0; k < cnt; k += U) {
      T vv[U][NV];
      if constexpr (HEADVEC) {
        // Every load of the round is unconditional (kb > 0 here): a slot past the
        // batch's end repeats the batch's last nonzero, a column outside [0, k) reads row 0 and
        // is replaced by zeros, a lane past the row's width reads column 0.  Loads behind
        // per-slot branches were issued one at a time (each followed by a full wait): the bf16
        // H=8 D=32 launch on the products graph took 33.5 ms.  The row piece stays one 16-byte
        // word until it is used (a per-element copy or select is narrowed into misaligned
        // pieces for 16-bit types).
        static_assert(sizeof(Pack<T, VEC>) == sizeof(u32x4), "a lane's columns are 16 bytes");
        u32x4 raw[U];
        unsigned inmask = 0;
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int ku = k + u < cnt ? k + u : cnt - 1;
          const int64_t cu = (int64_t)__shfl((int64_t)myc, gbase + (ku & (LPR - 1)), 64);
          const bool in = (uint64_t)cu < (uint64_t)kb;
          inmask |= (in ? 1u : 0u) << u;
          raw[u] = *reinterpret_cast<const u32x4*>(B + (in ? cu : 0) * ldb + (cb < n ? cb : 0));
          vv[u][0] = val[(jb + ku) * heads + hd[0]];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          // a column outside [0, k): the zero-filled gathered row of the sum op (+0 is all-zero
          // bits in every value type)
          const u32x4 r = ((inmask >> u) & 1u) ? raw[u] : u32x4{0u, 0u, 0u, 0u};
          const Pack<T, VEC> p = __builtin_bit_cast(Pack<T, VEC>, r);
          if (k + u < cnt) {
            const A v = Num<T>::load(vv[u][0]);
#pragma unroll
            for (int e = 0; e < VEC; ++e)
              acc[e] = acc[e] + Num<T>::mul(v, Num<T>::load(p.v[e]));
          }
        }
      } else {
        T bv[U][VEC];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int64_t cu = (int64_t)__shfl((int64_t)myc, gbase + ((k + u) & (LPR - 1)), 64);
          if (k + u < cnt) {
            // a column outside [0, k): the zero-filled gathered row of the sum op
            const bool in = (uint64_t)cu < (uint64_t)kb;
            load_cols<T, VEC, false>(B + (in ? cu : 0) * ldb, in ? cb : n, n, zero, bv[u]);
            const T* vrow = val + (jb + k + u) * heads;
#pragma unroll
            for (int e = 0; e < NV; ++e) vv[u][e] = vrow[hd[e]];
          }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          if (k + u < cnt) {
#pragma unroll
            for (int e = 0; e < VEC; ++e)
              acc[e] = acc[e] + Num<T>::mul(Num<T>::load(vv[u][e]), Num<T>::load(bv[u][e]));
          }
        }
      }
    }
  }
}

// ---- host side: what the units' launch paths share (none of it reaches a kernel) --

constexpr int64_t kHeadsChunk = 256;  // items of at most this many nonzeros (work only)

// The schedule of the ops with one output per (nonzero, head): work layout only (every output is
// its own dot product), the narrow SDDMM's items.
inline Schedule scores_schedule() {
  Schedule s = resolve_schedule(1, nullptr);
  s.split = s.chunk = kHeadsChunk;
  return s;
}

// The shape a score kernel's fast path needs (each user adds rows_aligned of its own operands).
// k == 0 (every column out of range) takes the general path: the fast one needs a row 0.
inline bool fast_score_shape(int64_t heads, int64_t d, int64_t k) {
  const int64_t lh = d / kLeaf;
  return d % kLeaf == 0 && (lh & (lh - 1)) == 0 && heads * d <= kMaxHeadsN && k > 0;
}

template <int V>
using Int = std::integral_constant<int, V>;

// The LG x L table of the score kernels (sddmm_heads_item and its like): f(LG, L, FAST) as
// integral constants, in the style of by_types.  Fast: the group covers the H*D / 8 leaves of the
// row.  General: the ceil(D / 8) leaves of one head.
template <typename F>
int by_score_layout(bool fast, int64_t heads, int64_t d, F&& f) {
  if (fast) {
    const int64_t leaves = heads * d / kLeaf;
    if (leaves <= 1) return f(Int<1>{}, Int<1>{}, std::true_type{});
    if (leaves <= 2) return f(Int<2>{}, Int<1>{}, std::true_type{});
    if (leaves <= 4) return f(Int<4>{}, Int<1>{}, std::true_type{});
    if (leaves <= 8) return f(Int<8>{}, Int<1>{}, std::true_type{});
    if (leaves <= 16) return f(Int<16>{}, Int<1>{}, std::true_type{});
    if (leaves <= 32) return f(Int<32>{}, Int<1>{}, std::true_type{});
    if (leaves <= 64) return f(Int<64>{}, Int<1>{}, std::true_type{});
    if (leaves <= 128) return f(Int<64>{}, Int<2>{}, std::true_type{});
    return f(Int<64>{}, Int<4>{}, std::true_type{});
  }
  const int64_t leaves = (d + kLeaf - 1) / kLeaf;
  if (leaves <= 1) return f(Int<1>{}, Int<1>{}, std::false_type{});
  if (leaves <= 4) return f(Int<4>{}, Int<1>{}, std::false_type{});
  if (leaves <= 16) return f(Int<16>{}, Int<1>{}, std::false_type{});
  if (leaves <= 64) return f(Int<64>{}, Int<1>{}, std::false_type{});
  return f(Int<64>{}, Int<4>{}, std::false_type{});
}

// The lane group of the row-output kernels (spmm_heads_accumulate and its like): f(LPR) for
// `lanes` lanes of 16 bytes; a wider row loops over tiles of 64 lanes.
template <typename F>
int by_lane_group(int64_t lanes, F&& f) {
  if (lanes <= 1) return f(Int<1>{});
  if (lanes <= 4) return f(Int<4>{});
  if (lanes <= 16) return f(Int<16>{});
  if (lanes <= 32) return f(Int<32>{});
  return f(Int<64>{});
}

}  // namespace
}  // namespace hsteps
}  // namespace ofx

#endif  // OFX_HEADS_STEPS_H_
