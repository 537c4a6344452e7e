// spmm_edge.hip — the SpMM over per-edge feature vectors (op "spmm_csr_edge"), gfx950:
//   out[r, c] = sum over the row's nonzeros j of act(B[col[j], c] op e[j, c])
// for op in {mul, add} and act in {none, relu}: the message sums of GINE (add + relu), CFConv,
// MPNN and CGConv-style layers (mul), DGL's u_add_e / u_mul_e + sum.  Contract (include/ofx_spmm.h,
// DESIGN.md §3q): the operation in the accumulation type, rounded to T as a step of its own, the
// relu, then the add in the accumulation type, nonzeros ascending; a hub row (more than `split`
// nonzeros, the schedule resolved from N as ofx_spmm_csr resolves it) summed per chunk from +0 and
// the chunk partials added in chunk order into +0; one rounding to T.  With mul, no activation and
// e[j, :] = values[j] these are ofx_spmm_csr's bits.
//
// Half of the traffic is a random row gather (B[col]) and half a sequential stream (a row's edge
// block is one contiguous deg * N span read exactly once).  Lane layout as the multi-head SpMM's
// (spmm_heads.hip): a group of LPR lanes per work item (a row or a hub chunk from the shared
// planner), each lane owning VEC consecutive columns, col loaded LPR at a time and broadcast; per
// nonzero and lane two 16-byte loads, the gathered B row through the cache and the e row
// non-temporally, min(8, LPR) nonzeros' loads in flight before the chain of adds; non-temporal stores;
// widths beyond LPR * VEC loop over column tiles (each tile walks the row's nonzeros again: the
// e row's 16-byte pieces of one tile are read once either way).  op and act are template
// parameters.  The general path (scalar loads) covers N % VEC != 0, unaligned bases or leading
// dimensions and K = 0.  Hub chunks write accumulation-type partials, hub_sum_kernel adds them.
// No atomics, no LDS, no allocation, no host synchronisation.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include "heads_steps.h"  // the lane ladder, the launch of a sum over rows
#include "spmm_edge.h"
#include "spmm_edge_dev.h"
#include "spmm_items_dev.h"

namespace ofx {
namespace {

using namespace item;
using namespace hsteps;

template <typename T, typename I, int VEC, int LPR, int U, bool FAST, int OP, bool RELU>
__global__ void __launch_bounds__(kBlock)
    spmm_edge_kernel(const I* __restrict__ rp, const I* __restrict__ col,
                     const T* __restrict__ E, const T* __restrict__ B, int64_t ldb, int64_t kb,
                     T* __restrict__ out, int64_t ldc, int64_t row_begin, int64_t nrows, int64_t n,
                     int64_t nnz, int64_t chunk, const unsigned long long* __restrict__ counters,
                     const int64_t* __restrict__ items, const int64_t* __restrict__ order,
                     typename Num<T>::acc* __restrict__ part, int64_t block_base, unsigned* err) {
#pragma clang fp contract(off)
  using A = typename Num<T>::acc;
  constexpr int GPW = 64 / LPR;
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
    A acc[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc[e] = A(0);
    edge::for_each_nonzero<T, I, VEC, LPR, U, FAST, false, true, true>(
        col, (const I*)nullptr, B, ldb, kb, E, n, nnz, cb, it.j0, it.j1, gl, gbase,
        [&](int64_t, const T(&bv)[VEC], const T(&ev)[VEC]) {
#pragma unroll
          for (int e = 0; e < VEC; ++e)
            acc[e] = acc[e] + edge::message<T, OP, RELU>(Num<T>::load(bv[e]), Num<T>::load(ev[e]));
        });
    if (it.slot >= 0) {  // a hub chunk's partial: added in chunk order by hub_sum_kernel
#pragma unroll
      for (int e = 0; e < VEC; ++e)
        if (cb + e < n) part[it.slot * n + cb + e] = acc[e];
    } else {
      T o[VEC];
#pragma unroll
      for (int e = 0; e < VEC; ++e) o[e] = Num<T>::store(acc[e]);
      store_cols<T, VEC, FAST>(out + it.lr * ldc, cb, n, o);
    }
  }
}

struct EdgeArgs {
  RowSumArgs r;  // val: e [nnz, n]; heads = 1, d = n
  int op, act;
};

// The kernel of one layout, issued by the shared launch (heads_steps.h).
template <typename T, typename I, int LPR, bool FAST>
int edge_cfg(const EdgeArgs& x) {
  constexpr int VEC = 16 / sizeof(T), U = 8;
  const RowSumArgs& a = x.r;
  return edge::by_op_act(x.op, x.act, [&](auto op, auto relu) -> int {
    return launch_row_sum<T, I>("spmm_csr_edge", a, LPR, [&](dim3 grid, int64_t b0, const Planned& p) {
      hipLaunchKernelGGL(
          (spmm_edge_kernel<T, I, VEC, LPR, U, FAST, decltype(op)::value, decltype(relu)::value>),
          grid, dim3(kBlock), 0, a.s, static_cast<const I*>(a.rp), static_cast<const I*>(a.col),
          static_cast<const T*>(a.val), static_cast<const T*>(a.b), a.ldb, a.k,
          static_cast<T*>(a.c), a.ldc, a.row_begin, a.nrows, a.d, a.nnz, p.chunk, p.wl.counters,
          p.wl.items, p.wl.order, static_cast<typename Num<T>::acc*>(p.wl.part), b0, p.err);
    });
  });
}

template <typename T, typename I>
int edge_typed(const EdgeArgs& x) {
  constexpr int VEC = 16 / sizeof(T);
  const RowSumArgs& a = x.r;
  const int64_t lanes = (a.d + VEC - 1) / VEC;
  const bool fast = edge::fast_shape<T>(a.d, a.k) && rows_aligned(a.b, a.ldb, sizeof(T), VEC) &&
                    rows_aligned(a.val, a.d, sizeof(T), VEC) &&
                    rows_aligned(a.c, a.ldc, sizeof(T), VEC);
  if (fast)
    return by_lane_group(lanes, [&](auto lpr) -> int {
      return edge_cfg<T, I, decltype(lpr)::value, true>(x);
    });
  return edge::by_general_group(lanes, [&](auto lpr) -> int {
    return edge_cfg<T, I, decltype(lpr)::value, false>(x);
  });
}

}  // namespace
}  // namespace ofx

using namespace ofx;

extern "C" int ofx_spmm_csr_edge_workspace_size(int idx_dtype, int val_dtype, int64_t m, int64_t k,
                                                int64_t n, int64_t nnz,
                                                const ofx_spmm_options* opts, size_t* bytes) {
  return ::ofx::guarded(__func__, [&]() -> int {
    OFX_REQUIRE(bytes != nullptr, OFX_EINVAL, "spmm_csr_edge_workspace_size: bytes is NULL");
    OFX_READ_OPTIONS(opts, "spmm_csr_edge_workspace_size");
    if (const int rc = edge::check_edge_sizes("spmm_csr_edge_workspace_size", idx_dtype, val_dtype,
                                              m, k, n, nnz, opts))
      return rc;
    *bytes = row_sum_ws_bytes(m, nnz, 1, n, val_dtype, opts);
    return OFX_OK;
  });
}

extern "C" int ofx_spmm_csr_edge(void* stream, int idx_dtype, int val_dtype, int64_t m, int64_t k,
                                 int64_t n, int64_t nnz, const void* row_ptr, const void* col_idx,
                                 const void* e, const void* b, int64_t ldb, int op, int act,
                                 void* c, int64_t ldc, int64_t row_begin, int64_t row_end,
                                 void* workspace, size_t workspace_bytes,
                                 const ofx_spmm_options* opts) {
  return ::ofx::guarded(__func__, [&]() -> int {
    OFX_TAKE_DEVICE_ERROR("spmm_csr_edge");  // an earlier launch's loud failure (spmm_plan.h)
    OFX_READ_OPTIONS(opts, "spmm_csr_edge");
    bool nothing = false;
    int rc = edge::check_edge_args("spmm_csr_edge", false, idx_dtype, val_dtype, m, k, n, nnz,
                                   row_ptr, col_idx, e, b, ldb, op, act, nullptr, 0, c, ldc,
                                   row_begin, row_end, opts, &nothing);
    if (rc || nothing) return rc;
    const int64_t nrows = row_end - row_begin;
    const size_t need = row_sum_ws_bytes(nrows, nnz, 1, n, val_dtype, opts);
    if ((rc = check_workspace("spmm_csr_edge", workspace, workspace_bytes, need))) return rc;
    const EdgeArgs x{{static_cast<hipStream_t>(stream), row_ptr, col_idx, e, b, nullptr, c, ldb,
                      ldc, m, row_begin, nrows, 1, n, nnz, b ? k : 0, workspace, workspace_bytes,
                      opts},
                     op, act};
    return by_types(idx_dtype, val_dtype, [&](auto* tp, auto* ip) -> int {
      return edge_typed<std::remove_pointer_t<decltype(tp)>,
                        std::remove_pointer_t<decltype(ip)>>(x);
    });
  });
}
