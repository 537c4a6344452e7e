// spmm_heads.hip — the multi-head CSR x dense SpMM (op "spmm_csr_heads"), gfx950:
//   out[r, h*D + c] = sum over the row's nonzeros j of values[j, h] * B[col[j], h*D + c]
// for H heads of width D (N = H*D; values is [nnz, H] row-major), the aggregation of multi-head
// graph attention.  Contract (include/ofx_spmm.h): every head's D columns carry the
// bits of ofx_spmm_csr on (values[:, h], B[:, h*D:(h+1)*D]) under the same options -- multiply
// (rounded to T), then add in the accumulation type, nonzeros ascending; a hub row (more than
// `split` nonzeros, the schedule resolved from D, not from N) summed per chunk from +0 and the
// chunk partials added in chunk order into +0; one rounding to T.
//
// Lane layout as the extremum kernel's (spmm_extremum.hip): a group of LPR lanes per work item (a
// row or a hub chunk from the shared planner), each lane owning VEC consecutive columns of the
// whole H*D row (16-byte B-row loads: the row is gathered once, not once per head), col loaded
// LPR at a time and broadcast, U B-row loads in flight before the multiply-add chain, non-temporal
// stores; widths beyond LPR * VEC loop over column tiles.  What is new is the value: with
// D % VEC == 0 a lane's columns lie in one head h and it loads values[j*H + h] itself (the lanes
// of a head read one address: one L1 / L2 hit per nonzero and head, the line fetched once);
// otherwise (D < VEC, odd D, unaligned rows) every element carries its own head index and the
// loads are scalar.  Hub chunks write accumulation-type partials, hub_sum_kernel adds them.
// No atomics, no allocation, no host synchronisation.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include "heads_steps.h"
#include "spmm_extremum.h"
#include "spmm_items_dev.h"

namespace ofx {
namespace {

using namespace item;
using namespace hsteps;  // the accumulation of a run of nonzeros, the lane ladder (heads_steps.h)

// HEADVEC: ALIGNED rows and D % VEC == 0 (one head per lane).
template <typename T, typename I, int VEC, int LPR, int U, bool HEADVEC>
__global__ void __launch_bounds__(kBlock)
    spmm_heads_kernel(const I* __restrict__ rp, const I* __restrict__ col,
                      const T* __restrict__ val, const T* __restrict__ B, int64_t ldb, int64_t kb,
                      T* __restrict__ out, int64_t ldc, int64_t row_begin, int64_t nrows,
                      int64_t n, int64_t heads, int64_t d, int64_t chunk,
                      const unsigned long long* __restrict__ counters,
                      const int64_t* __restrict__ items, const int64_t* __restrict__ order,
                      typename Num<T>::acc* __restrict__ part, int64_t block_base, unsigned* err) {
#pragma clang fp contract(off)
  using A = typename Num<T>::acc;
  constexpr int GPW = 64 / LPR;
  constexpr int NV = HEADVEC ? 1 : VEC;  // value loads per lane and nonzero
  if (poison_rows(counters, block_base, err, out, ldc, (I*)nullptr, (int64_t)0, nrows, n)) return;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int gl = lane & (LPR - 1);
  const int gbase = lane & ~(LPR - 1);
  const int64_t g = ((block_base + (int64_t)blockIdx.x) * (kBlock / 64) + wave) * GPW + lane / LPR;
  Item it;
  if (!work_item<I>(rp, g, row_begin, nrows, chunk, counters, items, order, &it)) return;
  for (int64_t c0 = 0; c0 < n; c0 += (int64_t)LPR * VEC) {
    const int64_t cb = c0 + (int64_t)gl * VEC;
    // the head of each of the lane's columns (a column >= n: head 0, its product is never stored)
    int64_t hd[NV];
#pragma unroll
    for (int e = 0; e < NV; ++e) hd[e] = cb + e < n ? (cb + e) / d : 0;
    A acc[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc[e] = A(0);
    spmm_heads_accumulate<T, I, VEC, LPR, U, HEADVEC>(col, val, B, ldb, kb, n, heads, cb, hd, it.j0,
                                                      it.j1, gl, gbase, acc);
    if (it.slot >= 0) {  // a hub chunk's partial: added in chunk order by hub_sum_kernel
#pragma unroll
      for (int e = 0; e < VEC; ++e)
        if (cb + e < n) part[it.slot * n + cb + e] = acc[e];
    } else {
      T o[VEC];
#pragma unroll
      for (int e = 0; e < VEC; ++e) o[e] = Num<T>::store(acc[e]);
      store_cols<T, VEC, HEADVEC>(out + it.lr * ldc, cb, n, o);
    }
  }
}

struct HeadsArgs {
  hipStream_t s;
  const void *rp, *col, *val, *b;
  void* c;
  int64_t ldb, ldc, m, row_begin, nrows, heads, d, nnz, k;
  void* ws;
  size_t ws_bytes;
  const ofx_spmm_options* opts;
};

template <typename T, typename I, int VEC, int LPR, bool HEADVEC>
int heads_cfg(const HeadsArgs& a) {
  using A = typename Num<T>::acc;
  constexpr int U = 8;
  constexpr int64_t GPB = (kBlock / 64) * (64 / LPR);
  const int64_t n = a.heads * a.d;
  Planned p;
  // the schedule: the sum op's, resolved from the width of ONE head (the numeric contract), with
  // this launch's share of the nonzeros for the automatic heavy threshold
  int rc = prepare_plan<I>("spmm_csr_heads", a.s, static_cast<const I*>(a.rp), a.row_begin,
                           a.nrows, a.nnz, launch_nnz(a.m, a.nrows, a.nnz, a.opts), n, sizeof(A),
                           resolve_schedule(a.d, a.opts), false, a.ws, a.ws_bytes, &p);
  if (rc) return rc;
  A* part = static_cast<A*>(p.wl.part);
  rc = launch_cut_grid(p.work, GPB, [&](dim3 grid, int64_t b0) {
    hipLaunchKernelGGL((spmm_heads_kernel<T, I, VEC, LPR, U, HEADVEC>), grid, dim3(kBlock), 0, a.s,
                       static_cast<const I*>(a.rp), static_cast<const I*>(a.col),
                       static_cast<const T*>(a.val), static_cast<const T*>(a.b), a.ldb, a.k,
                       static_cast<T*>(a.c), a.ldc, a.row_begin, a.nrows, n, a.heads, a.d, p.chunk,
                       p.wl.counters, p.wl.items, p.wl.order, part, b0, p.err);
  });
  if (rc) return rc;
  return launch_hub_sum(a.s, p, static_cast<T*>(a.c), a.ldc, a.nrows, n);
}

// One layout per width class: the lanes of a group cover the H*D columns in one tile up to
// 64 * VEC of them; wider rows loop over tiles.
template <typename T, typename I, bool HEADVEC>
int heads_width(const HeadsArgs& a) {
  constexpr int VEC = 16 / sizeof(T);
  return by_lane_group((a.heads * a.d + VEC - 1) / VEC, [&](auto lpr) -> int {
    return heads_cfg<T, I, VEC, decltype(lpr)::value, HEADVEC>(a);
  });
}

template <typename T, typename I>
int heads_typed(const HeadsArgs& a) {
  constexpr int VEC = 16 / sizeof(T);
  // k == 0 (every column out of range, B may be empty) takes the general path: the fast one
  // loads unconditionally and needs a row 0 to read
  const bool headvec = a.d % VEC == 0 && a.k > 0 && rows_aligned(a.b, a.ldb, sizeof(T), VEC) &&
                       rows_aligned(a.c, a.ldc, sizeof(T), VEC);
  return headvec ? heads_width<T, I, true>(a) : heads_width<T, I, false>(a);
}

int check_heads_args(const char* fn, int idx_dtype, int val_dtype, int64_t m, int64_t k,
                     int64_t heads, int64_t d, int64_t nnz, const ofx_spmm_options* opts) {
  if (const int rc = check_heads_shape(fn, heads, d)) return rc;
  if (const int rc = check_types_sizes(fn, idx_dtype, val_dtype, m, k, heads * d, nnz)) return rc;
  return check_no_plan_options(fn, opts);
}

}  // namespace
}  // namespace ofx

using namespace ofx;

extern "C" int ofx_spmm_csr_heads_workspace_size(int idx_dtype, int val_dtype, int64_t m, int64_t k,
                                                 int64_t heads, int64_t d, int64_t nnz,
                                                 const ofx_spmm_options* opts, size_t* bytes) {
  return ::ofx::guarded(__func__, [&]() -> int {
    OFX_REQUIRE(bytes != nullptr, OFX_EINVAL, "spmm_csr_heads_workspace_size: bytes is NULL");
    OFX_READ_OPTIONS(opts, "spmm_csr_heads_workspace_size");
    if (const int rc = check_heads_args("spmm_csr_heads_workspace_size", idx_dtype, val_dtype, m,
                                        k, heads, d, nnz, opts))
      return rc;
    *bytes = plan::ws_layout(m, nnz, heads * d, val_dtype == OFX_DT_DOUBLE ? 8 : 4,
                             resolve_schedule(d, opts)).total;
    return OFX_OK;
  });
}

extern "C" int ofx_spmm_csr_heads(void* stream, int idx_dtype, int val_dtype, int64_t m, int64_t k,
                                  int64_t heads, int64_t d, int64_t nnz, const void* row_ptr,
                                  const void* col_idx, const void* values, const void* b,
                                  int64_t ldb, void* c, int64_t ldc, int64_t row_begin,
                                  int64_t row_end, void* workspace, size_t workspace_bytes,
                                  const ofx_spmm_options* opts) {
  return ::ofx::guarded(__func__, [&]() -> int {
    OFX_TAKE_DEVICE_ERROR("spmm_csr_heads");  // an earlier launch's loud failure (spmm_plan.h)
    OFX_READ_OPTIONS(opts, "spmm_csr_heads");
    int rc = check_heads_args("spmm_csr_heads", idx_dtype, val_dtype, m, k, heads, d, nnz, opts);
    if (rc) return rc;
    const int64_t n = heads * d;
    rc = check_reduce_args("spmm_csr_heads", idx_dtype, val_dtype, m, k, n, nnz, ldb, ldc, false,
                           0, row_begin, row_end);
    if (rc) return rc;
    const int64_t nrows = row_end - row_begin;
    if (nrows == 0 || n == 0) return OFX_OK;  // nothing to write
    OFX_REQUIRE(row_ptr && c, OFX_EINVAL, "spmm_csr_heads: NULL row_ptr or output");
    OFX_REQUIRE(nnz == 0 || (col_idx && values && b), OFX_EINVAL,
                "spmm_csr_heads: NULL col_idx/values/b with nnz=%lld", (long long)nnz);
    // these entries' wording of the size error, ahead of the shared check
    const size_t need = plan::ws_layout(nrows, nnz, n, val_dtype == OFX_DT_DOUBLE ? 8 : 4,
                                        resolve_schedule(d, opts)).total;
    if ((rc = check_workspace("spmm_csr_heads", workspace, workspace_bytes, need))) return rc;
    const HeadsArgs a{static_cast<hipStream_t>(stream), row_ptr, col_idx, values, b, c, ldb, ldc,
                      m, row_begin, nrows, heads, d, nnz, k, workspace, workspace_bytes, opts};
    return by_types(idx_dtype, val_dtype, [&](auto* tp, auto* ip) -> int {
      return heads_typed<std::remove_pointer_t<decltype(tp)>,
                         std::remove_pointer_t<decltype(ip)>>(a);
    });
  });
}
