// gatv2_scores_grad.hip — the gradient of the GATv2 attention scores over a CSR (op
// "gatv2_scores_csr_heads_grad"), gfx950: from the upstream de [nnz, H],
//   d_x[r, n] = sum over the row's nonzeros j of T1[j, n],  T1 = de[j, h] * (z > 0 ? att[n] : att[n] * slope)
//   p[r, n]   = sum over the row's nonzeros j of T2[j, n],  T2 = de[j, h] * U[j, n]      (on request)
// with z = x_row[r, n] + x_col[col[j], n] formed again and U the forward's activated, rounded sum.
// Contract (include/ofx_spmm.h): T1 and T2 are rounded to T, and d_x / p have the
// bits of ofx_spmm_csr_heads on (row_ptr, arange(nnz)) with values of ones and b = T1 / T2 --
// nonzeros ascending, a hub row (more than `split` nonzeros, the schedule resolved from D) summed
// per chunk from +0 and the partials added in chunk order, one rounding to T.  The gradient in
// x_col is this entry on the transposed CSR with x_row and x_col exchanged; d(att) is the column
// sum of p.
//
// Lane layout as the multi-head SpMM's (spmm_heads.hip): a group of LPR lanes per work item (a row
// or a hub chunk from the shared planner), each lane owning VEC consecutive columns of the whole
// H*D row and holding its x_row, w_pos and w_neg columns and one or two accumulators; col loaded
// LPR at a time and broadcast; per nonzero one 16-byte x_col gather and one de[j*H + h] load, U
// gathers in flight; widths beyond LPR * VEC loop over column tiles.  HEADVEC (D % VEC == 0,
// aligned rows): one head per lane; otherwise every element carries its own head index and the
// loads are scalar.  Hub chunks write accumulation-type partials (two planes when p is
// requested), hub_sum_kernel adds them.  WITH_P is a template flag, not a branch in the loop.
// No atomics, no LDS, no allocation, no host synchronisation.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include "gatv2_scores.h"
#include "heads_steps.h"  // the lane ladder
#include "spmm_extremum.h"
#include "spmm_items_dev.h"

namespace ofx {
namespace {

using namespace item;

// acc1[e] += T1[j, cb + e] and (WITH_P) acc2[e] += T2[j, cb + e] over nonzeros [j0, j1), ascending,
// for the lane's VEC columns [cb, cb + VEC) of the n = H*D wide row; hd[e]: the head of column
// cb + e (HEADVEC: one head per lane, hd[0]).  HEADVEC: 16-byte-aligned rows, D % VEC == 0, kb > 0.
template <typename T, typename I, int VEC, int LPR, int U, bool HEADVEC, bool WITH_P>
__device__ __forceinline__ void gatv2_grad_accumulate(
    const I* __restrict__ col, const T* __restrict__ de, const T* __restrict__ B, int64_t ldb,
    int64_t kb, int64_t n, int64_t heads, int64_t cb, const int64_t (&hd)[HEADVEC ? 1 : VEC],
    const typename Num<T>::acc (&xr)[VEC], const typename Num<T>::acc (&wpos)[VEC],
    const typename Num<T>::acc (&wneg)[VEC], typename Num<T>::acc slope, int64_t j0, int64_t j1,
    int gl, int gbase, typename Num<T>::acc (&acc1)[VEC], typename Num<T>::acc (&acc2)[VEC]) {
#pragma clang fp contract(off)
  using A = typename Num<T>::acc;
  constexpr int NV = HEADVEC ? 1 : VEC;  // de loads per lane and nonzero
  const T zero = Num<T>::store(A(0));
  for (int64_t jb = j0; jb < j1; jb += LPR) {
    const int cnt = (int)((j1 - jb) < LPR ? (j1 - jb) : LPR);
    const I myc = gl < cnt ? col[jb + gl] : I(0);
    for (int k = 0; k < cnt; k += U) {
      T vv[U][NV];
      T bv[U][VEC];
      if constexpr (HEADVEC) {
        // every load of the round is unconditional (kb > 0 here): a slot past the batch's end
        // repeats the batch's last nonzero, a column outside [0, k) reads row 0 and is replaced
        // by zeros, a lane past the row's width reads column 0; the row piece stays one 16-byte
        // word until it is used
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
          vv[u][0] = de[(jb + ku) * heads + hd[0]];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const u32x4 r = ((inmask >> u) & 1u) ? raw[u] : u32x4{0u, 0u, 0u, 0u};
          const Pack<T, VEC> p = __builtin_bit_cast(Pack<T, VEC>, r);
#pragma unroll
          for (int e = 0; e < VEC; ++e) bv[u][e] = p.v[e];
        }
      } else {
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int64_t cu = (int64_t)__shfl((int64_t)myc, gbase + ((k + u) & (LPR - 1)), 64);
          if (k + u < cnt) {
            // a column outside [0, k): x_col reads +0 and the row's address is never used
            const bool in = (uint64_t)cu < (uint64_t)kb;
            load_cols<T, VEC, false>(B + (in ? cu : 0) * ldb, in ? cb : n, n, zero, bv[u]);
            const T* grow = de + (jb + k + u) * heads;
#pragma unroll
            for (int e = 0; e < NV; ++e) vv[u][e] = grow[hd[e]];
          }
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (k + u < cnt) {
#pragma unroll
          for (int e = 0; e < VEC; ++e) {
            const A g = Num<T>::load(vv[u][HEADVEC ? 0 : e]);
            const A z = xr[e] + Num<T>::load(bv[u][e]);
            acc1[e] = acc1[e] + gv2::rounded<T>(g * (z > A(0) ? wpos[e] : wneg[e]));
            if constexpr (WITH_P) acc2[e] = acc2[e] + Num<T>::mul(g, gv2::activated<T>(z, slope));
          }
        }
      }
    }
  }
}

// HEADVEC: ALIGNED rows and D % VEC == 0 (one head per lane).
template <typename T, typename I, int VEC, int LPR, int U, bool HEADVEC, bool WITH_P>
__global__ void __launch_bounds__(kBlock)
    gatv2_scores_grad_kernel(const I* __restrict__ rp, const I* __restrict__ col,
                             const T* __restrict__ xrow, int64_t ldr, const T* __restrict__ att,
                             const T* __restrict__ B, int64_t ldb, int64_t kb,
                             typename Num<T>::acc slope, const T* __restrict__ de,
                             T* __restrict__ dx, int64_t ldd, T* __restrict__ pout, int64_t ldp,
                             int64_t row_begin, int64_t nrows, int64_t n, int64_t heads, int64_t d,
                             int64_t chunk, const unsigned long long* __restrict__ counters,
                             const int64_t* __restrict__ items, const int64_t* __restrict__ order,
                             typename Num<T>::acc* __restrict__ part1,
                             typename Num<T>::acc* __restrict__ part2, int64_t block_base,
                             unsigned* err) {
#pragma clang fp contract(off)
  using A = typename Num<T>::acc;
  constexpr int GPW = 64 / LPR;
  constexpr int NV = HEADVEC ? 1 : VEC;
  if (plan_failed(counters, block_base, err)) {  // a loud NaN fill of both outputs
    const T bad = poison_value<T>();
    const int64_t total = nrows * n;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
      const int64_t r = i / n, c = i - r * n;
      dx[r * ldd + c] = bad;
      if constexpr (WITH_P) pout[r * ldp + c] = bad;
    }
    return;
  }
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int gl = lane & (LPR - 1);
  const int gbase = lane & ~(LPR - 1);
  const int64_t g = ((block_base + (int64_t)blockIdx.x) * (kBlock / 64) + wave) * GPW + lane / LPR;
  Item it;
  if (!work_item<I>(rp, g, row_begin, nrows, chunk, counters, items, order, &it)) return;
  const T zero = Num<T>::store(A(0));
  for (int64_t c0 = 0; c0 < n; c0 += (int64_t)LPR * VEC) {
    const int64_t cb = c0 + (int64_t)gl * VEC;
    // the head of each of the lane's columns (a column >= n: head 0, its sum is never stored)
    int64_t hd[NV];
#pragma unroll
    for (int e = 0; e < NV; ++e) hd[e] = cb + e < n ? (cb + e) / d : 0;
    T rx[VEC], rw[VEC];
    load_cols<T, VEC, HEADVEC>(xrow + it.lr * ldr, cb, n, zero, rx);
    load_cols<T, VEC, HEADVEC>(att, cb, n, zero, rw);
    A xr[VEC], wpos[VEC], wneg[VEC], acc1[VEC], acc2[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      xr[e] = Num<T>::load(rx[e]);
      wpos[e] = Num<T>::load(rw[e]);
      wneg[e] = wpos[e] * slope;
      acc1[e] = A(0);
      acc2[e] = A(0);
    }
    gatv2_grad_accumulate<T, I, VEC, LPR, U, HEADVEC, WITH_P>(col, de, B, ldb, kb, n, heads, cb, hd,
                                                              xr, wpos, wneg, slope, it.j0, it.j1,
                                                              gl, gbase, acc1, acc2);
    if (it.slot >= 0) {  // a hub chunk's partials: added in chunk order by hub_sum_kernel
#pragma unroll
      for (int e = 0; e < VEC; ++e)
        if (cb + e < n) {
          part1[it.slot * n + cb + e] = acc1[e];
          if constexpr (WITH_P) part2[it.slot * n + cb + e] = acc2[e];
        }
    } else {
      T o[VEC];
#pragma unroll
      for (int e = 0; e < VEC; ++e) o[e] = Num<T>::store(acc1[e]);
      store_cols<T, VEC, HEADVEC>(dx + it.lr * ldd, cb, n, o);
      if constexpr (WITH_P) {
#pragma unroll
        for (int e = 0; e < VEC; ++e) o[e] = Num<T>::store(acc2[e]);
        store_cols<T, VEC, HEADVEC>(pout + it.lr * ldp, cb, n, o);
      }
    }
  }
}

struct GradArgs {
  hipStream_t s;
  const void *rp, *col, *xr, *xc, *att, *de;
  void *dx, *p;
  int64_t ldr, ldc, ldd, ldp, m, row_begin, nrows, heads, d, nnz, k;
  double slope;
  void* ws;
  size_t ws_bytes;
  const ofx_spmm_options* opts;
};

template <typename T, typename I, int VEC, int LPR, bool HEADVEC, bool WITH_P>
int grad_cfg(const GradArgs& a) {
  using A = typename Num<T>::acc;
  constexpr int U = 8;
  constexpr int64_t GPB = (kBlock / 64) * (64 / LPR);
  const int64_t n = a.heads * a.d;
  Planned p;
  // the schedule: the sum op's, resolved from the width of ONE head (the numeric contract); the
  // partials are one plane of n columns per output
  int rc = prepare_plan<I>("gatv2_scores_csr_heads_grad", a.s, static_cast<const I*>(a.rp),
                           a.row_begin, a.nrows, a.nnz, launch_nnz(a.m, a.nrows, a.nnz, a.opts),
                           WITH_P ? 2 * n : n, sizeof(A), resolve_schedule(a.d, a.opts), false,
                           a.ws, a.ws_bytes, &p);
  if (rc) return rc;
  A* part1 = static_cast<A*>(p.wl.part);
  A* part2 = (WITH_P && part1 != nullptr) ? part1 + p.w.max_chunks * n : nullptr;
  rc = launch_cut_grid(p.work, GPB, [&](dim3 grid, int64_t b0) {
    hipLaunchKernelGGL((gatv2_scores_grad_kernel<T, I, VEC, LPR, U, HEADVEC, WITH_P>), grid,
                       dim3(kBlock), 0, a.s, static_cast<const I*>(a.rp),
                       static_cast<const I*>(a.col), static_cast<const T*>(a.xr), a.ldr,
                       static_cast<const T*>(a.att), static_cast<const T*>(a.xc), a.ldc, a.k,
                       (A)a.slope, static_cast<const T*>(a.de), static_cast<T*>(a.dx), a.ldd,
                       static_cast<T*>(a.p), a.ldp, a.row_begin, a.nrows, n, a.heads, a.d, p.chunk,
                       p.wl.counters, p.wl.items, p.wl.order, part1, part2, b0, p.err);
  });
  if (rc) return rc;
  rc = launch_hub_sum<T>(a.s, p, part1, static_cast<T*>(a.dx), a.ldd, a.nrows, n);
  if (rc || !WITH_P) return rc;
  return launch_hub_sum<T>(a.s, p, part2, static_cast<T*>(a.p), a.ldp, a.nrows, n);
}

// One layout per width class: the lanes of a group cover the H*D columns in one tile up to
// 64 * VEC of them; wider rows loop over tiles.
template <typename T, typename I, bool HEADVEC, bool WITH_P>
int grad_width(const GradArgs& a) {
  constexpr int VEC = 16 / sizeof(T);
  return hsteps::by_lane_group((a.heads * a.d + VEC - 1) / VEC, [&](auto lpr) -> int {
    return grad_cfg<T, I, VEC, decltype(lpr)::value, HEADVEC, WITH_P>(a);
  });
}

template <typename T, typename I>
int grad_typed(const GradArgs& a) {
  constexpr int VEC = 16 / sizeof(T);
  // k == 0 (every column out of range, x_col may be empty) takes the general path: the fast one
  // loads unconditionally and needs a row 0 to read
  const bool headvec = a.d % VEC == 0 && a.k > 0 && rows_aligned(a.xc, a.ldc, sizeof(T), VEC) &&
                       rows_aligned(a.xr, a.ldr, sizeof(T), VEC) &&
                       rows_aligned(a.att, a.heads * a.d, sizeof(T), VEC) &&
                       rows_aligned(a.dx, a.ldd, sizeof(T), VEC) &&
                       rows_aligned(a.p, a.ldp, sizeof(T), VEC);
  if (a.p != nullptr)
    return headvec ? grad_width<T, I, true, true>(a) : grad_width<T, I, false, true>(a);
  return headvec ? grad_width<T, I, true, false>(a) : grad_width<T, I, false, false>(a);
}

size_t grad_ws_bytes(int64_t nrows, int64_t nnz, int64_t n, int64_t d, bool with_p, int val_dtype,
                     const ofx_spmm_options* opts) {
  return plan::ws_layout(nrows, nnz, with_p ? 2 * n : n, val_dtype == OFX_DT_DOUBLE ? 8 : 4,
                         resolve_schedule(d, opts)).total;
}

}  // namespace
}  // namespace ofx

using namespace ofx;

extern "C" int ofx_gatv2_scores_csr_heads_grad_workspace_size(int idx_dtype, int val_dtype,
                                                              int64_t m, int64_t k, int64_t heads,
                                                              int64_t d, int64_t nnz, int with_p,
                                                              const ofx_spmm_options* opts,
                                                              size_t* bytes) {
  return ::ofx::guarded(__func__, [&]() -> int {
    const char* fn = "gatv2_scores_csr_heads_grad_workspace_size";
    OFX_REQUIRE(bytes != nullptr, OFX_EINVAL, "%s: bytes is NULL", fn);
    OFX_READ_OPTIONS(opts, "gatv2_scores_csr_heads_grad_workspace_size");
    // two planes of partials: 2 * heads * d is representable too
    OFX_REQUIRE(heads >= 0 && d >= 0 && (d == 0 || heads <= INT64_MAX / d / 2), OFX_EINVAL,
                "%s: bad heads=%lld / d=%lld", fn, (long long)heads, (long long)d);
    if (const int rc = check_types_sizes(fn, idx_dtype, val_dtype, m, k, heads * d, nnz)) return rc;
    if (const int rc = check_no_plan_options(fn, opts)) return rc;
    *bytes = grad_ws_bytes(m, nnz, heads * d, d, with_p != 0, val_dtype, opts);
    return OFX_OK;
  });
}

extern "C" int ofx_gatv2_scores_csr_heads_grad(
    void* stream, int idx_dtype, int val_dtype, int64_t m, int64_t k, int64_t heads, int64_t d,
    int64_t nnz, const void* row_ptr, const void* col_idx, const void* x_row, int64_t ldr,
    const void* x_col, int64_t ldc, const void* att, double negative_slope, const void* de,
    void* d_x, int64_t ldd, void* p, int64_t ldp, int64_t row_begin, int64_t row_end,
    void* workspace, size_t workspace_bytes, const ofx_spmm_options* opts) {
  return ::ofx::guarded(__func__, [&]() -> int {
    OFX_TAKE_DEVICE_ERROR("gatv2_scores_csr_heads_grad");  // an earlier launch's loud failure
    OFX_READ_OPTIONS(opts, "gatv2_scores_csr_heads_grad");
    bool nothing = false;
    if (const int rc = gv2::check_gatv2_args(
            "gatv2_scores_csr_heads_grad", true, idx_dtype, val_dtype, m, k, heads, d, nnz, row_ptr,
            col_idx, x_row, ldr, x_col, ldc, att, negative_slope, de, d_x, ldd, p, ldp, row_begin,
            row_end, opts, &nothing))
      return rc;
    if (nothing) return OFX_OK;
    const int64_t nrows = row_end - row_begin;
    const size_t need = grad_ws_bytes(nrows, nnz, heads * d, d, p != nullptr, val_dtype, opts);
    if (const int rc =
            check_workspace("gatv2_scores_csr_heads_grad", workspace, workspace_bytes, need))
      return rc;
    const GradArgs a{static_cast<hipStream_t>(stream), row_ptr, col_idx, x_row, x_col, att, de,
                     d_x, p, ldr, ldc, ldd, ldp, m, row_begin, nrows, heads, d, nnz,
                     x_col ? k : 0, negative_slope, workspace, workspace_bytes, opts};
    return by_types(idx_dtype, val_dtype, [&](auto* tp, auto* ip) -> int {
      return grad_typed<std::remove_pointer_t<decltype(tp)>,
                        std::remove_pointer_t<decltype(ip)>>(a);
    });
  });
}
