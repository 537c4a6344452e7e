// spmm_extremum_grad.hip — d(b) of the max / min reductions of op "spmm_csr_reduce", gfx950:
// the masked SpMM on A^T.
//
// For out = max_j / min_j (val[j] * b[col[j], :]) with arg the winning j and g = d(out):
//   d(b)[k, c] = sum over the entries t of row k of A^T (ofx_csr_transpose: ascending A-row
//                order), j = perm[t], r = col_idx_T[t], of mul(val[j], g[r, c]) if arg[r, c] == j;
//                an entry that did not win the column is skipped (nothing is added).
// The order is numeric here, so the walk is the sum op's on A^T at width n: rows longer than the
// schedule's split are cut into its chunks by the shared planner, each chunk summed from +0 and
// the chunk partials added in chunk order into +0 (include/ofx_spmm.h, "SpMM schedule options").
// Every output element is written by exactly one lane in that fixed order; there are no atomics
// on values, so the gradient is deterministic.  With at most one nonzero per row of A every entry
// wins, and the result is the sum op's grad_b bit for bit.
//
// Lane layout of the forward: LPR lanes per work item, VEC columns per lane, (row, j, value)
// loaded LPR at a time and broadcast, U (g, arg) row pairs in flight before the select-and-add.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include "spmm_extremum.h"
#include "spmm_items_dev.h"

namespace ofx {
namespace {

using namespace item;

template <typename T, typename I, int VEC, int LPR, int U, bool ALIGNED>
__global__ void __launch_bounds__(kBlock)
    select_kernel(const I* __restrict__ rp_t, const I* __restrict__ col_t,
                  const I* __restrict__ perm, const T* __restrict__ val,
                  const I* __restrict__ arg, int64_t ldarg, const T* __restrict__ g, int64_t ldg,
                  int64_t m, int64_t nnz, T* __restrict__ db, int64_t lddb, int64_t row_begin,
                  int64_t nrows, int64_t n, int64_t chunk,
                  const unsigned long long* __restrict__ counters,
                  const int64_t* __restrict__ items, const int64_t* __restrict__ order,
                  typename Num<T>::acc* __restrict__ part, int64_t block_base, unsigned* err) {
#pragma clang fp contract(off)
  using A = typename Num<T>::acc;
  constexpr int GPW = 64 / LPR;
  if (poison_rows(counters, block_base, err, db, lddb, (I*)nullptr, 0, nrows, n)) return;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int gl = lane & (LPR - 1);
  const int gbase = lane & ~(LPR - 1);
  const int64_t gi = ((block_base + (int64_t)blockIdx.x) * (kBlock / 64) + wave) * GPW + lane / LPR;
  Item it;
  if (!work_item<I>(rp_t, gi, row_begin, nrows, chunk, counters, items, order, &it)) return;
  const T zero = Num<T>::store(A(0));
  for (int64_t c0 = 0; c0 < n; c0 += (int64_t)LPR * VEC) {
    const int64_t cb = c0 + (int64_t)gl * VEC;
    A acc[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc[e] = A(0);
    for (int64_t tb = it.j0; tb < it.j1; tb += LPR) {
      const int cnt = (int)((it.j1 - tb) < LPR ? (it.j1 - tb) : LPR);
      // entry t of A^T: the A row it came from and its nonzero index in A; an entry whose row or
      // index lies outside the matrix is skipped (never from ofx_csr_transpose)
      int64_t myr = -1, myj = -1;
      A myv = A(0);
      if (gl < cnt) {
        myr = (int64_t)col_t[tb + gl];
        myj = (int64_t)perm[tb + gl];
        if ((uint64_t)myr >= (uint64_t)m || (uint64_t)myj >= (uint64_t)nnz) myr = myj = -1;
        if (myj >= 0) myv = Num<T>::load(val[myj]);
      }
      for (int k = 0; k < cnt; k += U) {
        T gv[U][VEC];
        I av[U][VEC];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int64_t r = (int64_t)__shfl(myr, gbase + ((k + u) & (LPR - 1)), 64);
          if (k + u < cnt) {
            const bool in = r >= 0;
            load_cols<T, VEC, ALIGNED>(g + (in ? r : 0) * ldg, in ? cb : n, n, zero, gv[u]);
            load_cols<I, VEC, ALIGNED>(arg + (in ? r : 0) * ldarg, in ? cb : n, n, I(-1), av[u]);
          }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const A v = __shfl(myv, gbase + ((k + u) & (LPR - 1)), 64);
          const int64_t j = (int64_t)__shfl(myj, gbase + ((k + u) & (LPR - 1)), 64);
          if (k + u < cnt && j >= 0) {
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
              // a select, not a branch: the sum of a skipped entry is computed and dropped
              const A sum = acc[e] + Num<T>::mul(v, Num<T>::load(gv[u][e]));
              acc[e] = (int64_t)av[u][e] == j ? sum : acc[e];
            }
          }
        }
      }
    }
    if (it.slot >= 0) {  // a hub chunk's partial: added in chunk order by hub_sum_kernel
#pragma unroll
      for (int e = 0; e < VEC; ++e)
        if (cb + e < n) part[it.slot * n + cb + e] = acc[e];
    } else {
      T o[VEC];
#pragma unroll
      for (int e = 0; e < VEC; ++e) o[e] = Num<T>::store(acc[e]);
      store_cols<T, VEC, ALIGNED>(db + it.lr * lddb, cb, n, o);
    }
  }
}

struct SelArgs {
  hipStream_t s;
  const void *rp_t, *col_t, *perm, *val, *arg, *g;
  void* db;
  int64_t ldarg, ldg, lddb, m, k, row_begin, nrows, n, nnz;
  void* ws;
  size_t ws_bytes;
  const ofx_spmm_options* opts;
};

template <typename T, typename I, int VEC, int LPR, bool ALIGNED>
int select_cfg(const SelArgs& a) {
  using A = typename Num<T>::acc;
  constexpr int U = 4;
  constexpr int64_t GPB = (kBlock / 64) * (64 / LPR);
  Planned p;
  // the plan of A^T's k rows at width n: the sum op's schedule on A^T
  int rc = prepare_plan<I>("spmm_csr_select", a.s, static_cast<const I*>(a.rp_t), a.k, a.row_begin,
                           a.nrows, a.nnz, a.n, sizeof(A), a.opts, a.ws, a.ws_bytes, &p);
  if (rc) return rc;
  A* part = static_cast<A*>(p.wl.part);
  rc = launch_cut_grid(p.work, GPB, [&](dim3 grid, int64_t b0) {
    hipLaunchKernelGGL((select_kernel<T, I, VEC, LPR, U, ALIGNED>), grid, dim3(kBlock), 0, a.s,
                       static_cast<const I*>(a.rp_t), static_cast<const I*>(a.col_t),
                       static_cast<const I*>(a.perm), static_cast<const T*>(a.val),
                       static_cast<const I*>(a.arg), a.ldarg, static_cast<const T*>(a.g), a.ldg,
                       a.m, a.nnz, static_cast<T*>(a.db), a.lddb, a.row_begin, a.nrows, a.n,
                       p.chunk, p.wl.counters, p.wl.items, p.wl.order, part, b0, p.err);
  });
  if (rc) return rc;
  // hub rows of A^T
  return launch_hub_sum(a.s, p, static_cast<T*>(a.db), a.lddb, a.nrows, a.n);
}

template <typename T, typename I, bool ALIGNED>
int select_width(const SelArgs& a) {
  constexpr int VEC = 16 / sizeof(T);
  const int64_t lanes = (a.n + VEC - 1) / VEC;
  if (lanes <= 1) return select_cfg<T, I, VEC, 1, ALIGNED>(a);
  if (lanes <= 4) return select_cfg<T, I, VEC, 4, ALIGNED>(a);
  if (lanes <= 16) return select_cfg<T, I, VEC, 16, ALIGNED>(a);
  return select_cfg<T, I, VEC, 64, ALIGNED>(a);
}

template <typename T, typename I>
int select_typed(const SelArgs& a) {
  constexpr int VEC = 16 / sizeof(T);
  const bool aligned = a.n % VEC == 0 && rows_aligned(a.g, a.ldg, sizeof(T), VEC) &&
                       rows_aligned(a.db, a.lddb, sizeof(T), VEC) &&
                       rows_aligned(a.arg, a.ldarg, sizeof(I), VEC);
  return aligned ? select_width<T, I, true>(a) : select_width<T, I, false>(a);
}

}  // namespace
}  // namespace ofx

using namespace ofx;

extern "C" int ofx_spmm_csr_select_workspace_size(int idx_dtype, int val_dtype, int64_t m,
                                                  int64_t k, int64_t n, int64_t nnz,
                                                  const ofx_spmm_options* opts, size_t* bytes) {
  return ::ofx::guarded(__func__, [&]() -> int {
    OFX_REQUIRE(bytes != nullptr, OFX_EINVAL, "spmm_csr_select_workspace_size: bytes is NULL");
    OFX_READ_OPTIONS(opts, "spmm_csr_select_workspace_size");
    int rc = check_types_sizes("spmm_csr_select_workspace_size", idx_dtype, val_dtype, m, k, n, nnz);
    if (rc) return rc;
    *bytes = item::workspace_bytes(k, nnz, n, val_dtype == OFX_DT_DOUBLE ? 8 : 4, opts);
    return OFX_OK;
  });
}

extern "C" int ofx_spmm_csr_select(void* stream, int idx_dtype, int val_dtype, int64_t m, int64_t k,
                                   int64_t n, int64_t nnz, const void* row_ptr_t,
                                   const void* col_idx_t, const void* perm, const void* values,
                                   const void* arg, int64_t ldarg, const void* g, int64_t ldg,
                                   void* db, int64_t lddb, int64_t row_begin, int64_t row_end,
                                   void* workspace, size_t workspace_bytes,
                                   const ofx_spmm_options* opts) {
  return ::ofx::guarded(__func__, [&]() -> int {
    OFX_TAKE_DEVICE_ERROR("spmm_csr_select");  // an earlier launch's loud failure (spmm_plan.h)
    OFX_READ_OPTIONS(opts, "spmm_csr_select");
    int rc = check_select_args("spmm_csr_select", idx_dtype, val_dtype, m, k, n, nnz, ldarg, ldg,
                               lddb, row_begin, row_end);
    if (rc) return rc;
    const int64_t nrows = row_end - row_begin;
    if (nrows == 0 || n == 0) return OFX_OK;  // nothing to write
    OFX_REQUIRE(row_ptr_t && db, OFX_EINVAL, "spmm_csr_select: NULL row_ptr or output");
    OFX_REQUIRE(nnz == 0 || m == 0 || arg != nullptr, OFX_EINVAL,
                "spmm_csr_select: arg is NULL (the gradient of max / min needs it)");
    OFX_REQUIRE(nnz == 0 || (col_idx_t && perm && values && g), OFX_EINVAL,
                "spmm_csr_select: NULL pointer with nnz=%lld", (long long)nnz);
    const SelArgs a{static_cast<hipStream_t>(stream), row_ptr_t, col_idx_t, perm, values, arg, g,
                    db, ldarg, ldg, lddb, m, k, row_begin, nrows, n, nnz, workspace,
                    workspace_bytes, opts};
    return by_types(idx_dtype, val_dtype, [&](auto* tp, auto* ip) -> int {
      return select_typed<std::remove_pointer_t<decltype(tp)>,
                          std::remove_pointer_t<decltype(ip)>>(a);
    });
  });
}
