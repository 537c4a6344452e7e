// spmm_edge_dev.h — the device loop the three kernels of the edge-feature SpMM share (spmm_edge.hip
// the forward, spmm_edge_grad.hip d(e) and d(b)): the walk of a lane over a run of nonzeros with
// its VEC columns of two rows per nonzero, a gathered one (X[col[j], :]: b in the forward and
// d(e), dy in d(b)) and the nonzero's own e row (e[j, :], or e[perm[j], :] in d(b)).  What is done
// with the pair is the caller's functor.  Included by HIP translation units only.
#ifndef OFX_SPMM_EDGE_DEV_H_
#define OFX_SPMM_EDGE_DEV_H_

#include <hip/hip_runtime.h>

#include "spmm_edge.h"
#include "spmm_items_dev.h"

namespace ofx {
namespace edge {
namespace {  // internal linkage, as spmm_items_dev.h

using namespace item;

// The e row of a nonzero is read exactly once by the whole launch and is as many bytes as the
// gathered row: loaded non-temporally it does not push the gathered rows out of L2
// (OFX_EDGE_PLAIN_E_LOADS: the A/B build with plain loads).
__device__ __forceinline__ u32x4 stream_load(const u32x4* p) {
#ifdef OFX_EDGE_PLAIN_E_LOADS
  return *p;
#else
  return __builtin_nontemporal_load(p);
#endif
}

// f(j, x, ev) for the nonzeros jt of [j0, j1), ascending: j = PERM ? perm[jt] : jt is the e row,
// x[VEC] the lane's columns [cb, cb + VEC) of X[col[jt], :] (zeros for a column outside [0, kx)
// and for columns >= n; unspecified without NEED_X) and ev[VEC] those of e[j, :] (unspecified
// without NEED_E).  A group of LPR lanes (gl: the lane in it, gbase: its first lane) loads col and
// perm LPR at a time and broadcasts them; U = min(UMAX, LPR) nonzeros' loads are in flight before
// the first f.
// FAST: n % VEC == 0, X's rows and e 16-byte aligned, kx > 0 (PERM: nnz > 0, which j0 < j1 means).
// There every load is unconditional and stays one 16-byte word until it is used: a slot past the
// batch's end repeats the batch's last nonzero, a column outside [0, kx) reads row 0 and is
// replaced by zeros, a lane past the row's width reads column 0 (loads behind per-slot branches
// are issued one at a time).  A perm entry outside [0, nnz) (never from
// ofx_csr_transpose) reads e row 0.
// A batch holds at most LPR nonzeros, so min(UMAX, LPR) slots are issued: more would repeat the
// batch's last nonzero's loads (at LPR = 1 eight identical pairs per nonzero).
template <typename T, typename I, int VEC, int LPR, int UMAX, bool FAST, bool PERM, bool NEED_X,
          bool NEED_E, typename F>
__device__ __forceinline__ void for_each_nonzero(const I* __restrict__ col,
                                                 const I* __restrict__ perm,
                                                 const T* __restrict__ X, int64_t ldx, int64_t kx,
                                                 const T* __restrict__ E, int64_t n, int64_t nnz,
                                                 int64_t cb, int64_t j0, int64_t j1, int gl,
                                                 int gbase, F&& f) {
  using A = typename Num<T>::acc;
  constexpr int U = UMAX < LPR ? UMAX : LPR;
  const T zero = Num<T>::store(A(0));
  const int64_t cbs = cb < n ? cb : 0;
  for (int64_t jb = j0; jb < j1; jb += LPR) {
    const int cnt = (int)((j1 - jb) < LPR ? (j1 - jb) : LPR);
    I myc = I(0), myp = I(0);
    if constexpr (NEED_X) myc = gl < cnt ? col[jb + gl] : I(0);
    if constexpr (PERM && NEED_E) myp = gl < cnt ? perm[jb + gl] : I(0);
    for (int k = 0; k < cnt; k += U) {
      int64_t je[U];
      Pack<T, VEC> xv[U], ev[U];
      if constexpr (FAST) {
        static_assert(sizeof(Pack<T, VEC>) == sizeof(u32x4), "a lane's columns are 16 bytes");
        u32x4 rx[U], re[U];
        unsigned inmask = 0;
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int ku = k + u < cnt ? k + u : cnt - 1;
          je[u] = jb + ku;
          if constexpr (NEED_X) {
            const int64_t cu = (int64_t)__shfl((int64_t)myc, gbase + (ku & (LPR - 1)), 64);
            const bool in = (uint64_t)cu < (uint64_t)kx;
            inmask |= (in ? 1u : 0u) << u;
            rx[u] = *reinterpret_cast<const u32x4*>(X + (in ? cu : 0) * ldx + cbs);
          }
          if constexpr (PERM && NEED_E) {
            const int64_t pu = (int64_t)__shfl((int64_t)myp, gbase + (ku & (LPR - 1)), 64);
            je[u] = (uint64_t)pu < (uint64_t)nnz ? pu : 0;
          }
          if constexpr (NEED_E) {
            const u32x4* src = reinterpret_cast<const u32x4*>(E + je[u] * n + cbs);
            re[u] = PERM ? *src : stream_load(src);
          }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          if constexpr (NEED_X) {
            const u32x4 r = ((inmask >> u) & 1u) ? rx[u] : u32x4{0u, 0u, 0u, 0u};
            xv[u] = __builtin_bit_cast(Pack<T, VEC>, r);
          }
          if constexpr (NEED_E) ev[u] = __builtin_bit_cast(Pack<T, VEC>, re[u]);
        }
      } else {
#pragma unroll
        for (int u = 0; u < U; ++u) {
          int64_t cu = 0, pu = 0;
          if constexpr (NEED_X) cu = (int64_t)__shfl((int64_t)myc, gbase + ((k + u) & (LPR - 1)), 64);
          if constexpr (PERM && NEED_E)
            pu = (int64_t)__shfl((int64_t)myp, gbase + ((k + u) & (LPR - 1)), 64);
          if (k + u < cnt) {
            je[u] = jb + k + u;
            if constexpr (PERM && NEED_E) je[u] = (uint64_t)pu < (uint64_t)nnz ? pu : 0;
            if constexpr (NEED_X) {
              // a column outside [0, kx): every column reads as out of range and the row's
              // address is never used
              const bool in = (uint64_t)cu < (uint64_t)kx;
              load_cols<T, VEC, false>(X + (in ? cu : 0) * ldx, in ? cb : n, n, zero, xv[u].v);
            }
            if constexpr (NEED_E) load_cols<T, VEC, false>(E + je[u] * n, cb, n, zero, ev[u].v);
          }
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (k + u < cnt) f(je[u], xv[u].v, ev[u].v);
    }
  }
}

// The FAST shape of a launch: whole 16-byte lanes in every row it touches (each user passes its
// operands) and a row 0 to read.
template <typename T>
inline bool fast_shape(int64_t n, int64_t kx) {
  constexpr int VEC = 16 / sizeof(T);
  return n % VEC == 0 && kx > 0;
}

// The lane group of the general path (scalar loads; the correctness path of widths and bases no
// benchmark configuration takes: two layouts, not the fast path's five).
template <typename F>
int by_general_group(int64_t lanes, F&& f) {
  if (lanes <= 4) return f(std::integral_constant<int, 4>{});
  return f(std::integral_constant<int, 64>{});
}

}  // namespace
}  // namespace edge
}  // namespace ofx

#endif  // OFX_SPMM_EDGE_DEV_H_
