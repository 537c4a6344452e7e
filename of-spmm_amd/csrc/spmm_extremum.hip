// spmm_extremum.hip — max / min / mean aggregation of the CSR x dense SpMM (op
// "spmm_csr_reduce"), gfx950: the forward extremum kernel with its arg output, the combine of hub
// chunks, and the row scale by 1 / degree that turns the sum into the mean.
//
// Contract (include/ofx_spmm.h): out[r, c] = the extremum over the row's nonzeros j
// (ascending) of p_j[c] = Num<T>::mul(val[j], B[col[j], c]), a candidate replacing the running
// best only if strictly better, or NaN where the best is not (spmm_extremum.h `better`);
// arg[r, c] = the winning global j; an empty row gives +0 and -1.  The result is a pure function
// of the row, so cutting a hub row into chunks and combining the chunk winners in chunk order
// with the same rule changes nothing: the schedule options have no numeric effect here.
//
// Lane layout as the sum kernel's: a group of LPR lanes per work item (a row or a hub chunk from
// the shared planner), each lane owning VEC consecutive columns (16-byte B-row loads); (col, val)
// loaded LPR at a time by the group and broadcast with cross-lane moves; U B-row loads in flight
// before the compare chain; the running (best, arg) pair in registers; non-temporal stores for
// out and arg.  Widths beyond LPR * VEC loop over column tiles.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include "spmm_extremum.h"
#include "spmm_items_dev.h"

namespace ofx {
namespace {

using namespace item;

template <typename T, typename I, int VEC, int LPR, int U, bool ALIGNED>
__global__ void __launch_bounds__(kBlock)
    extremum_kernel(const I* __restrict__ rp, const I* __restrict__ col, const T* __restrict__ val,
                    const T* __restrict__ B, int64_t ldb, int64_t kb, T* __restrict__ out,
                    int64_t ldc, I* __restrict__ arg, int64_t ldarg, int64_t row_begin,
                    int64_t nrows, int64_t n, int64_t chunk, int is_max,
                    const unsigned long long* __restrict__ counters,
                    const int64_t* __restrict__ items, const int64_t* __restrict__ order,
                    typename Num<T>::acc* __restrict__ part_best, int64_t* __restrict__ part_arg,
                    int64_t block_base, unsigned* err) {
#pragma clang fp contract(off)
  using A = typename Num<T>::acc;
  constexpr int GPW = 64 / LPR;
  if (poison_rows(counters, block_base, err, out, ldc, arg, ldarg, nrows, n)) return;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int gl = lane & (LPR - 1);
  const int gbase = lane & ~(LPR - 1);
  const int64_t g = ((block_base + (int64_t)blockIdx.x) * (kBlock / 64) + wave) * GPW + lane / LPR;
  Item it;
  if (!work_item<I>(rp, g, row_begin, nrows, chunk, counters, items, order, &it)) return;
  const bool mx = is_max != 0;
  const T zero = Num<T>::store(A(0));
  for (int64_t c0 = 0; c0 < n; c0 += (int64_t)LPR * VEC) {
    const int64_t cb = c0 + (int64_t)gl * VEC;
    A best[VEC];
    I barg[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      best[e] = A(0);
      barg[e] = I(-1);
    }
    for (int64_t jb = it.j0; jb < it.j1; jb += LPR) {
      const int cnt = (int)((it.j1 - jb) < LPR ? (it.j1 - jb) : LPR);
      const I myc = gl < cnt ? col[jb + gl] : I(0);
      const A myv = gl < cnt ? Num<T>::load(val[jb + gl]) : A(0);
      for (int k = 0; k < cnt; k += U) {
        T bv[U][VEC];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int64_t cu = (int64_t)__shfl((int64_t)myc, gbase + ((k + u) & (LPR - 1)), 64);
          if (k + u < cnt) {
            // a column outside [0, k): the zero-filled gathered row of the sum op
            const bool in = (uint64_t)cu < (uint64_t)kb;
            load_cols<T, VEC, ALIGNED>(B + (in ? cu : 0) * ldb, in ? cb : n, n, zero, bv[u]);
          }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const A v = __shfl(myv, gbase + ((k + u) & (LPR - 1)), 64);
          if (k + u < cnt) {
            const I j = (I)(jb + k + u);
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
              const A p = signed_product<T>(v, Num<T>::load(bv[u][e]));
              const bool take = (int(barg[e] < 0) | int(better(p, best[e], mx))) != 0;
              best[e] = take ? p : best[e];
              barg[e] = take ? j : barg[e];
            }
          }
        }
      }
    }
    if (it.slot >= 0) {  // a hub chunk's winners: combined in chunk order by extremum_hub_kernel
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        if (cb + e < n) {
          part_best[it.slot * n + cb + e] = best[e];
          part_arg[it.slot * n + cb + e] = (int64_t)barg[e];
        }
      }
    } else {
      T o[VEC];
#pragma unroll
      for (int e = 0; e < VEC; ++e) o[e] = Num<T>::store(canonical_nan(best[e]));
      store_cols<T, VEC, ALIGNED>(out + it.lr * ldc, cb, n, o);
      if (arg != nullptr) store_cols<I, VEC, ALIGNED>(arg + it.lr * ldarg, cb, n, barg);
    }
  }
}

// The hub rows: chunk winners combined in chunk order with the same rule (every chunk holds at
// least one nonzero).  One block per hub, grid-strided; threads over the columns.
template <typename T, typename I>
__global__ void __launch_bounds__(kBlock)
    extremum_hub_kernel(const unsigned long long* __restrict__ counters,
                        const int64_t* __restrict__ hubs,
                        const typename Num<T>::acc* __restrict__ part_best,
                        const int64_t* __restrict__ part_arg, T* __restrict__ out, int64_t ldc,
                        I* __restrict__ arg, int64_t ldarg, int64_t nrows, int64_t n, int is_max) {
  using A = typename Num<T>::acc;
  if (!plan::plan_valid(counters)) return;  // the main kernel has poisoned the output
  const bool mx = is_max != 0;
  const int64_t nhubs = (int64_t)counters[1];
  for (int64_t h = blockIdx.x; h < nhubs; h += gridDim.x) {
    const int64_t lr = hubs[3 * h], s0 = hubs[3 * h + 1], nc = hubs[3 * h + 2];
    if ((uint64_t)lr >= (uint64_t)nrows) continue;  // never from a valid plan
    for (int64_t c = threadIdx.x; c < n; c += kBlock) {
      A best = part_best[s0 * n + c];
      int64_t ba = part_arg[s0 * n + c];
      for (int64_t q = 1; q < nc; ++q) {
        const A p = part_best[(s0 + q) * n + c];
        const int64_t pa = part_arg[(s0 + q) * n + c];
        const bool take = better(p, best, mx);
        best = take ? p : best;
        ba = take ? pa : ba;
      }
      nt_store_one(out + lr * ldc + c, Num<T>::store(canonical_nan(best)));
      if (arg != nullptr) nt_store_one(arg + lr * ldarg + c, (I)ba);
    }
  }
}

template <typename T, typename I>
__global__ void __launch_bounds__(kBlock)
    row_scale_kernel(const I* __restrict__ rp, const T* src, int64_t ldsrc, T* dst, int64_t lddst,
                     int64_t row_begin, int64_t nrows, int64_t n) {
#pragma clang fp contract(off)
  const int64_t total = nrows * n;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const int64_t r = i / n, c = i - r * n;
    const int64_t deg = (int64_t)rp[row_begin + r + 1] - (int64_t)rp[row_begin + r];
    dst[r * lddst + c] = scale_by_degree<T>(src[r * ldsrc + c], deg);
  }
}

struct ExtArgs {
  hipStream_t s;
  const void *rp, *col, *val, *b;
  void *c, *arg;
  int64_t ldb, ldc, ldarg, m, row_begin, nrows, n, nnz, k;
  bool is_max;
  void* ws;
  size_t ws_bytes;
  const ofx_spmm_options* opts;
};

// Bytes of a hub chunk's partial per column: the winner in the accumulation type and its int64 j.
template <typename T>
constexpr size_t part_bytes() {
  return sizeof(typename Num<T>::acc) + sizeof(int64_t);
}

template <typename T, typename I, int VEC, int LPR, bool ALIGNED>
int extremum_cfg(const ExtArgs& a) {
  using A = typename Num<T>::acc;
  constexpr int U = 8;
  constexpr int64_t GPB = (kBlock / 64) * (64 / LPR);
  Planned p;
  int rc = prepare_plan<I>("spmm_csr_reduce", a.s, static_cast<const I*>(a.rp), a.m, a.row_begin,
                           a.nrows, a.nnz, a.n, part_bytes<T>(), a.opts, a.ws, a.ws_bytes, &p);
  if (rc) return rc;
  // partials: the int64 args first (8-byte aligned at the region's start), then the winners
  int64_t* part_arg = static_cast<int64_t*>(p.wl.part);
  A* part_best = p.has_plan ? reinterpret_cast<A*>(part_arg + p.w.max_chunks * a.n) : nullptr;
  rc = launch_cut_grid(p.work, GPB, [&](dim3 grid, int64_t b0) {
    hipLaunchKernelGGL((extremum_kernel<T, I, VEC, LPR, U, ALIGNED>), grid, dim3(kBlock), 0, a.s,
                       static_cast<const I*>(a.rp), static_cast<const I*>(a.col),
                       static_cast<const T*>(a.val), static_cast<const T*>(a.b), a.ldb, a.k,
                       static_cast<T*>(a.c), a.ldc, static_cast<I*>(a.arg), a.ldarg, a.row_begin,
                       a.nrows, a.n, p.chunk, a.is_max ? 1 : 0, p.wl.counters, p.wl.items,
                       p.wl.order, part_best, part_arg, b0, p.err);
  });
  if (rc) return rc;
  if (p.has_plan && p.w.max_hubs > 0) {
    const unsigned hgrid = (unsigned)std::min<int64_t>(p.w.max_hubs, 8192);
    hipLaunchKernelGGL((extremum_hub_kernel<T, I>), dim3(hgrid), dim3(kBlock), 0, a.s,
                       p.wl.counters, p.wl.hubs, part_best, part_arg, static_cast<T*>(a.c), a.ldc,
                       static_cast<I*>(a.arg), a.ldarg, a.nrows, a.n, a.is_max ? 1 : 0);
    OFX_HIP_CHECK(hipGetLastError());
  }
  return OFX_OK;
}

// One layout per width class: the lanes of a group cover the width in one column tile up to
// 64 * VEC columns (256 for f32, 512 for 16-bit types, 128 for f64); wider loops over tiles.
template <typename T, typename I, bool ALIGNED>
int extremum_width(const ExtArgs& a) {
  constexpr int VEC = 16 / sizeof(T);
  const int64_t lanes = (a.n + VEC - 1) / VEC;
  if (lanes <= 1) return extremum_cfg<T, I, VEC, 1, ALIGNED>(a);
  if (lanes <= 4) return extremum_cfg<T, I, VEC, 4, ALIGNED>(a);
  if (lanes <= 16) return extremum_cfg<T, I, VEC, 16, ALIGNED>(a);
  return extremum_cfg<T, I, VEC, 64, ALIGNED>(a);
}

template <typename T, typename I>
int extremum_typed(const ExtArgs& a) {
  constexpr int VEC = 16 / sizeof(T);
  const bool aligned = a.n % VEC == 0 && rows_aligned(a.b, a.ldb, sizeof(T), VEC) &&
                       rows_aligned(a.c, a.ldc, sizeof(T), VEC) &&
                       rows_aligned(a.arg, a.ldarg, sizeof(I), VEC);
  return aligned ? extremum_width<T, I, true>(a) : extremum_width<T, I, false>(a);
}

}  // namespace
}  // namespace ofx

using namespace ofx;

extern "C" int ofx_spmm_csr_reduce_workspace_size(int idx_dtype, int val_dtype, int64_t m,
                                                  int64_t k, int64_t n, int64_t nnz, int reduce,
                                                  const ofx_spmm_options* opts, size_t* bytes) {
  return ::ofx::guarded(__func__, [&]() -> int {
    OFX_REQUIRE(bytes != nullptr, OFX_EINVAL, "spmm_csr_reduce_workspace_size: bytes is NULL");
    int rc = check_reduce_code(reduce, "spmm_csr_reduce_workspace_size");
    if (rc) return rc;
    if (reduce == OFX_REDUCE_SUM || reduce == OFX_REDUCE_MEAN)
      return ofx_spmm_csr_workspace_size(idx_dtype, val_dtype, m, k, n, nnz, opts, bytes);
    OFX_READ_OPTIONS(opts, "spmm_csr_reduce_workspace_size");
    rc = check_types_sizes("spmm_csr_reduce_workspace_size", idx_dtype, val_dtype, m, k, n, nnz);
    if (rc) return rc;
    *bytes = item::workspace_bytes(m, nnz, n,
                                   (val_dtype == OFX_DT_DOUBLE ? 8 : 4) + sizeof(int64_t), opts);
    return OFX_OK;
  });
}

extern "C" int ofx_spmm_csr_reduce(void* stream, int idx_dtype, int val_dtype, int64_t m, int64_t k,
                                   int64_t n, int64_t nnz, const void* row_ptr,
                                   const void* col_idx, const void* values, const void* b,
                                   int64_t ldb, void* c, int64_t ldc, void* arg, int64_t ldarg,
                                   int64_t row_begin, int64_t row_end, int reduce, void* workspace,
                                   size_t workspace_bytes, const ofx_spmm_options* opts) {
  return ::ofx::guarded(__func__, [&]() -> int {
    int rc = check_reduce_code(reduce, "spmm_csr_reduce");
    if (rc) return rc;
    if (reduce == OFX_REDUCE_SUM || reduce == OFX_REDUCE_MEAN) {
      rc = ofx_spmm_csr(stream, idx_dtype, val_dtype, m, k, n, nnz, row_ptr, col_idx, values, b,
                        ldb, c, ldc, row_begin, row_end, workspace, workspace_bytes, opts);
      if (rc || reduce == OFX_REDUCE_SUM) return rc;
      // the mean: the sum op's result, then each row divided by its degree in place
      return ofx_row_scale_by_degree(stream, idx_dtype, val_dtype, m, n, row_ptr, c, ldc, c, ldc,
                                     row_begin, row_end);
    }
    OFX_TAKE_DEVICE_ERROR("spmm_csr_reduce");  // an earlier launch's loud failure (spmm_plan.h)
    OFX_READ_OPTIONS(opts, "spmm_csr_reduce");
    rc = check_reduce_args("spmm_csr_reduce", idx_dtype, val_dtype, m, k, n, nnz, ldb, ldc,
                           arg != nullptr, ldarg, row_begin, row_end);
    if (rc) return rc;
    const int64_t nrows = row_end - row_begin;
    if (nrows == 0 || n == 0) return OFX_OK;  // nothing to write
    OFX_REQUIRE(row_ptr && c, OFX_EINVAL, "spmm_csr_reduce: NULL row_ptr or output");
    OFX_REQUIRE(nnz == 0 || (col_idx && values && b), OFX_EINVAL,
                "spmm_csr_reduce: NULL col_idx/values/b with nnz=%lld", (long long)nnz);
    const ExtArgs a{static_cast<hipStream_t>(stream), row_ptr, col_idx, values, b, c, arg, ldb,
                    ldc, ldarg, m, row_begin, nrows, n, nnz, k, reduce == OFX_REDUCE_MAX,
                    workspace, workspace_bytes, opts};
    return by_types(idx_dtype, val_dtype, [&](auto* tp, auto* ip) -> int {
      return extremum_typed<std::remove_pointer_t<decltype(tp)>,
                            std::remove_pointer_t<decltype(ip)>>(a);
    });
  });
}

extern "C" int ofx_row_scale_by_degree(void* stream, int idx_dtype, int val_dtype, int64_t m,
                                       int64_t n, const void* row_ptr, const void* src,
                                       int64_t ldsrc, void* dst, int64_t lddst, int64_t row_begin,
                                       int64_t row_end) {
  return ::ofx::guarded(__func__, [&]() -> int {
    int rc = check_row_scale_args("row_scale_by_degree", idx_dtype, val_dtype, m, n, ldsrc, lddst,
                                  row_begin, row_end);
    if (rc) return rc;
    const int64_t nrows = row_end - row_begin;
    if (nrows == 0 || n == 0) return OFX_OK;
    OFX_REQUIRE(row_ptr && src && dst, OFX_EINVAL, "row_scale_by_degree: NULL pointer");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t total = nrows * n;
    const unsigned grid = (unsigned)std::min<int64_t>((total + kBlock - 1) / kBlock, 1 << 20);
    return by_types(idx_dtype, val_dtype, [&](auto* tp, auto* ip) -> int {
      using T = std::remove_pointer_t<decltype(tp)>;
      using I = std::remove_pointer_t<decltype(ip)>;
      hipLaunchKernelGGL((row_scale_kernel<T, I>), dim3(grid), dim3(kBlock), 0, s,
                         static_cast<const I*>(row_ptr), static_cast<const T*>(src), ldsrc,
                         static_cast<T*>(dst), lddst, row_begin, nrows, n);
      OFX_HIP_CHECK(hipGetLastError());
      return OFX_OK;
    });
  });
}
