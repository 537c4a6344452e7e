// gatv2_scores_heads.hip — the attention scores of a GATv2 layer over a CSR pattern (op
// "gatv2_scores_csr_heads"), gfx950:
//   e[j, h] = sum over c of att[h*D + c] * LeakyReLU(x_row[row(j), h*D + c] + x_col[col[j], h*D + c])
// for H heads of width D (e is [nnz, H] row-major).  Contract (include/ofx_spmm.h):
// the activated sum is rounded to T as a step of its own (U, never written), and e has the bits of
// ofx_sddmm_csr_heads for the left row att and the right row U[j, :].
//
// The layout is the multi-head SDDMM's (sddmm_heads.hip, heads_steps.h sddmm_heads_item): a lane
// group per row or 256-nonzero piece of the shared planner's work list (skip_empty), the LG x L
// table, a fast path (D % 8 == 0, D / 8 a power of two, H*D <= 2048, 16-byte-aligned rows: the
// group covers all H*D columns with 16-byte loads, every load of a round unconditional, a column
// outside [0, k) clamped to row 0 and then replaced by zeros, a segmented butterfly per head, the
// first lane of a head storing) and a general path (a lane group per (item, head), scalar loads).
// What differs: the item keeps TWO leaves per lane in registers for its whole life, x_row's and
// att's, and the per-element step is add, select-multiply, round to T, multiply by att.
// No atomics, no LDS, no allocation, no host synchronisation.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include "gatv2_scores.h"
#include "heads_steps.h"
#include "spmm_extremum.h"
#include "spmm_items_dev.h"

namespace ofx {
namespace {

using namespace item;
using namespace hsteps;  // load_leaf, the layout ladder and the schedule (heads_steps.h)

// The scores of nonzeros [j0, j1) of the row `xrow` by a group of LG lanes (gl: the lane in the
// group, gbase: the group's first lane), out[j * heads + h] rounded to T.  FAST / !FAST as
// sddmm_heads_item: the group covers the n = H*D columns (a head is `lh` leaves), or the D columns
// of `head`.
template <typename T, typename I, int LG, int L, int U, bool FAST>
__device__ __forceinline__ void gatv2_scores_item(const I* __restrict__ col,
                                                  const T* __restrict__ xrow,
                                                  const T* __restrict__ att,
                                                  const T* __restrict__ B, int64_t ldb, int64_t kb,
                                                  typename Num<T>::acc slope, T* out,
                                                  int64_t heads, int64_t d, int lh, int64_t head,
                                                  int64_t j0, int64_t j1, int gl, int gbase) {
#pragma clang fp contract(off)
  using A = typename Num<T>::acc;
  const int64_t col0 = FAST ? 0 : head * d;
  const int64_t w = FAST ? heads * d : d;
  // the tree: `lin` leaves of a head inside a lane, then `seg` lanes of a head
  const int lin = FAST ? (lh < L ? lh : L) : L;
  const int seg = FAST ? (lh / lin) : LG;
  A xv[L][kLeaf], wv[L][kLeaf];
  int hsel[L];  // FAST: the head whose result this lane's leaf l holds after the tree, or -1
#pragma unroll
  for (int l = 0; l < L; ++l) {
    load_leaf<T, FAST>(xrow + col0, (int64_t)(gl * L + l) * kLeaf, w, xv[l]);
    load_leaf<T, FAST>(att + col0, (int64_t)(gl * L + l) * kLeaf, w, wv[l]);
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
        // every load of the round is unconditional and stays a 16-byte word until all are issued
        // (kb > 0 here): a slot past the batch's end repeats the batch's last nonzero, a column
        // outside [0, k) reads row 0, a leaf past the row's width reads leaf 0; the last two are
        // then replaced by zeros
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
            // a column outside [0, k): every leaf reads as out of range (+0) and the row's address
            // is never used
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
            for (int e = 0; e < kLeaf; ++e) {
              // a padded column: z = +0, U = +0 * slope = +0, att = +0: the SDDMM's zero product
              const A z = xv[l][e] + bv[u][l][e];
              s = s + wv[l][e] * gv2::activated<T>(z, slope);
            }
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
              if (hsel[l] >= 0) out[j * heads + hsel[l]] = Num<T>::store(leaf[l]);
          } else {
            if (gl == 0) out[j * heads + head] = Num<T>::store(t);
          }
        }
      }
    }
  }
}

// FAST: the group covers the n = H*D columns of an item, a head is `lh` = D/8 leaves (a power of
// two).  !FAST: group index = item * H + head; the group covers the head's D columns.
template <typename T, typename I, int LG, int L, int U, bool FAST>
__global__ void __launch_bounds__(kBlock)
    gatv2_scores_kernel(const I* __restrict__ rp, const I* __restrict__ col,
                        const T* __restrict__ xr, int64_t ldr, const T* __restrict__ att,
                        const T* __restrict__ B, int64_t ldb, int64_t kb,
                        typename Num<T>::acc slope, T* __restrict__ out, int64_t row_begin,
                        int64_t nrows, int64_t heads, int64_t d, int lh, int64_t chunk,
                        const unsigned long long* __restrict__ counters,
                        const int64_t* __restrict__ items, const int64_t* __restrict__ order,
                        int64_t block_base, unsigned* err) {
#pragma clang fp contract(off)
  constexpr int GPW = 64 / LG;
  if (poison_head_nonzeros(counters, block_base, err, rp, row_begin, nrows, heads, out)) return;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int gl = lane & (LG - 1);
  const int gbase = lane & ~(LG - 1);
  const int64_t g = ((block_base + (int64_t)blockIdx.x) * (kBlock / 64) + wave) * GPW + lane / LG;
  const int64_t gi = FAST ? g : g / heads;
  const int64_t head = FAST ? 0 : g - gi * heads;
  Item it;
  if (!work_item<I>(rp, gi, row_begin, nrows, chunk, counters, items, order, &it, true)) return;
  gatv2_scores_item<T, I, LG, L, U, FAST>(col, xr + it.lr * ldr, att, B, ldb, kb, slope, out, heads,
                                          d, lh, head, it.j0, it.j1, gl, gbase);
}

struct Gv2Args {
  hipStream_t s;
  const void *rp, *col, *xr, *xc, *att;
  void* out;
  int64_t ldr, ldc, row_begin, nrows, heads, d, nnz, k;
  double slope;
  void* ws;
  size_t ws_bytes;
};

template <typename T, typename I, int LG, int L, bool FAST>
int gv2_cfg(const Gv2Args& x) {
  using A = typename Num<T>::acc;
  const int lh = FAST ? (int)(x.d / kLeaf) : 0;
  // loads in flight per lane: four leaves' worth; an f64 lane of four leaves holds x_row's and
  // att's 64 registers each, so it streams one nonzero at a time
  constexpr int U = L >= 4 ? (sizeof(T) == 8 ? 1 : 2) : (L == 2 && sizeof(T) == 8 ? 2 : 4);
  Planned p;
  if (const int rc = prepare_plan<I>("gatv2_scores_csr_heads", x.s, static_cast<const I*>(x.rp),
                                     x.row_begin, x.nrows, x.nnz, x.nnz, 0, 0, scores_schedule(),
                                     false, x.ws, x.ws_bytes, &p))
    return rc;
  const int64_t groups = FAST ? p.work : p.work * x.heads;
  return launch_cut_grid(groups, (kBlock / 64) * (64 / LG), [&](dim3 grid, int64_t b0) {
    hipLaunchKernelGGL((gatv2_scores_kernel<T, I, LG, L, U, FAST>), grid, dim3(kBlock), 0, x.s,
                       static_cast<const I*>(x.rp), static_cast<const I*>(x.col),
                       static_cast<const T*>(x.xr), x.ldr, static_cast<const T*>(x.att),
                       static_cast<const T*>(x.xc), x.ldc, x.k, (A)x.slope,
                       static_cast<T*>(x.out), x.row_begin, x.nrows, x.heads, x.d, lh, p.chunk,
                       p.wl.counters, p.wl.items, p.wl.order, b0, p.err);
  });
}

template <typename T, typename I>
int gv2_typed(const Gv2Args& x) {
  const bool fast = fast_score_shape(x.heads, x.d, x.k) &&
                    rows_aligned(x.xr, x.ldr, sizeof(T), kLeaf) &&
                    rows_aligned(x.xc, x.ldc, sizeof(T), kLeaf) &&
                    rows_aligned(x.att, x.heads * x.d, sizeof(T), kLeaf);
  return by_score_layout(fast, x.heads, x.d, [&](auto lg, auto l, auto f) -> int {
    return gv2_cfg<T, I, decltype(lg)::value, decltype(l)::value, decltype(f)::value>(x);
  });
}

}  // namespace
}  // namespace ofx

using namespace ofx;

extern "C" int ofx_gatv2_scores_csr_heads_workspace_size(int idx_dtype, int val_dtype, int64_t m,
                                                         int64_t heads, int64_t d, int64_t nnz,
                                                         size_t* bytes) {
  return ::ofx::guarded(__func__, [&]() -> int {
    OFX_REQUIRE(bytes != nullptr, OFX_EINVAL, "gatv2_scores_csr_heads_workspace_size: bytes is NULL");
    if (const int rc = check_heads_shape("gatv2_scores_csr_heads_workspace_size", heads, d))
      return rc;
    if (const int rc = check_types_sizes("gatv2_scores_csr_heads_workspace_size", idx_dtype,
                                         val_dtype, m, 0, heads * d, nnz))
      return rc;
    *bytes = plan::ws_layout(m, nnz, 0, 0, scores_schedule()).total;
    return OFX_OK;
  });
}

extern "C" int ofx_gatv2_scores_csr_heads(void* stream, int idx_dtype, int val_dtype, int64_t m,
                                          int64_t k, int64_t heads, int64_t d, int64_t nnz,
                                          const void* row_ptr, const void* col_idx,
                                          const void* x_row, int64_t ldr, const void* x_col,
                                          int64_t ldc, const void* att, double negative_slope,
                                          void* e, int64_t row_begin, int64_t row_end,
                                          void* workspace, size_t workspace_bytes) {
  return ::ofx::guarded(__func__, [&]() -> int {
    OFX_TAKE_DEVICE_ERROR("gatv2_scores_csr_heads");  // an earlier launch's loud failure
    bool nothing = false;
    if (const int rc = gv2::check_gatv2_args(
            "gatv2_scores_csr_heads", false, idx_dtype, val_dtype, m, k, heads, d, nnz, row_ptr,
            col_idx, x_row, ldr, x_col, ldc, att, negative_slope, nullptr, e, 0, nullptr, 0,
            row_begin, row_end, nullptr, &nothing))
      return rc;
    if (nothing) return OFX_OK;
    const size_t need = plan::ws_layout(row_end - row_begin, nnz, 0, 0, scores_schedule()).total;
    if (const int rc = check_workspace("gatv2_scores_csr_heads", workspace, workspace_bytes, need))
      return rc;
    const Gv2Args x{static_cast<hipStream_t>(stream), row_ptr, col_idx, x_row, x_col, att, e, ldr,
                    ldc, row_begin, row_end - row_begin, heads, d, nnz, x_col ? k : 0,
                    negative_slope, workspace, workspace_bytes};
    return by_types(idx_dtype, val_dtype, [&](auto* tp, auto* ip) -> int {
      return gv2_typed<std::remove_pointer_t<decltype(tp)>,
                       std::remove_pointer_t<decltype(ip)>>(x);
    });
  });
}
