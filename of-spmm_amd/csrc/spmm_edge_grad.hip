// spmm_edge_grad.hip — the gradients of the SpMM over per-edge feature vectors (ops
// "spmm_csr_edge_grad_e" and "spmm_csr_edge_grad_b"), gfx950.  With t = B[col[j], c] op e[j, c]
// rounded to T formed again and the relu's mask (t > 0):
//   de[j, c] = dy[r, c] * B[col[j], c] (mul) or dy[r, c] (add), +0 where masked
//   db[k, c] = sum over the nonzeros j of column k, in the transposed CSR's entry order, of
//              G[j, c] = dy[r, c] * e[j, c] (mul) or dy[r, c] (add), +0 where masked
// Contract (include/ofx_spmm.h): every product rounded to T; db has the bits of
// ofx_spmm_csr on the transposed CSR with unit values over G[perm], hub rule of
// resolve_schedule(N, opts).  G is never written.
//
// d(e) is edge-parallel over the narrow SDDMM's items (empty rows skipped, at most 256 nonzeros to
// an item: the cut has no numeric effect, every output is its own element): a group of LPR lanes
// keeps its VEC columns of the item's dy row in registers and per nonzero gathers B[col] through
// the cache, streams e[j] non-temporally (needed for the mask alone: never without an activation)
// and stores de[j, :] non-temporally.  add without activation is a pure row broadcast: neither B
// nor e is loaded.
// d(b) is the forward's row template on the transposed CSR: the item holds its own B[k, :] columns
// in registers (for the mask), dy[row] is gathered through col_idx_t and e[perm[j]] through perm
// (not for add without activation); hub chunks and the partial sum as in the forward.
// Loop and loads: spmm_edge_dev.h.  No atomics, no LDS, no allocation, no host synchronisation.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include "heads_steps.h"  // the lane ladder, the score ops' items, the launch of a sum over rows
#include "spmm_edge.h"
#include "spmm_edge_dev.h"
#include "spmm_items_dev.h"

namespace ofx {
namespace {

using namespace item;
using namespace hsteps;

// ---- d(e) ----------------------------------------------------------------------------------------
template <typename T, typename I, int VEC, int LPR, int U, bool FAST, int OP, bool RELU>
__global__ void __launch_bounds__(kBlock)
    spmm_edge_grad_e_kernel(const I* __restrict__ rp, const I* __restrict__ col,
                            const T* __restrict__ E, const T* __restrict__ B, int64_t ldb,
                            int64_t kb, const T* __restrict__ dy, int64_t lddy,
                            T* __restrict__ de, int64_t row_begin, int64_t nrows, int64_t n,
                            int64_t nnz, int64_t chunk,
                            const unsigned long long* __restrict__ counters,
                            const int64_t* __restrict__ items, const int64_t* __restrict__ order,
                            int64_t block_base, unsigned* err) {
#pragma clang fp contract(off)
  using A = typename Num<T>::acc;
  constexpr int GPW = 64 / LPR;
  constexpr bool NEED_B = edge::grad_e_needs_b(OP, RELU), NEED_E = edge::grad_e_needs_e(OP, RELU);
  if (poison_head_nonzeros(counters, block_base, err, rp, row_begin, nrows, n, de)) return;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int gl = lane & (LPR - 1);
  const int gbase = lane & ~(LPR - 1);
  const int64_t g = ((block_base + (int64_t)blockIdx.x) * (kBlock / 64) + wave) * GPW + lane / LPR;
  Item it;
  if (!work_item<I>(rp, g, row_begin, nrows, chunk, counters, items, order, &it, true)) return;
  const T zero = Num<T>::store(A(0));
  for (int64_t c0 = 0; c0 < n; c0 += (int64_t)LPR * VEC) {
    const int64_t cb = c0 + (int64_t)gl * VEC;
    T g_row[VEC];
    load_cols<T, VEC, FAST>(dy + it.lr * lddy, cb, n, zero, g_row);
    edge::for_each_nonzero<T, I, VEC, LPR, U, FAST, false, NEED_B, NEED_E>(
        col, (const I*)nullptr, B, ldb, kb, E, n, nnz, cb, it.j0, it.j1, gl, gbase,
        [&](int64_t j, const T(&bv)[VEC], const T(&ev)[VEC]) {
          T o[VEC];
#pragma unroll
          for (int e = 0; e < VEC; ++e) {
            const A b = NEED_B ? Num<T>::load(bv[e]) : A(0);
            o[e] = edge::grad_term<T, OP, RELU>(g_row[e], b, b,
                                                NEED_E ? Num<T>::load(ev[e]) : A(0));
          }
          store_cols<T, VEC, FAST>(de + j * n, cb, n, o);
        });
  }
}

struct GradEArgs {
  hipStream_t s;
  const void *rp, *col, *e, *b, *dy;
  void* de;
  int64_t ldb, lddy, row_begin, nrows, n, nnz, k;
  int op, act;
  void* ws;
  size_t ws_bytes;
};

template <typename T, typename I, int LPR, bool FAST>
int grad_e_cfg(const GradEArgs& x) {
  constexpr int VEC = 16 / sizeof(T), U = 8;
  Planned p;
  if (const int rc = prepare_plan<I>("spmm_csr_edge_grad_e", x.s, static_cast<const I*>(x.rp),
                                     x.row_begin, x.nrows, x.nnz, x.nnz, 0, 0, scores_schedule(),
                                     false, x.ws, x.ws_bytes, &p))
    return rc;
  return edge::by_op_act(x.op, x.act, [&](auto op, auto relu) -> int {
    return launch_cut_grid(p.work, (kBlock / 64) * (64 / LPR), [&](dim3 grid, int64_t b0) {
      hipLaunchKernelGGL((spmm_edge_grad_e_kernel<T, I, VEC, LPR, U, FAST, decltype(op)::value,
                                                  decltype(relu)::value>),
                         grid, dim3(kBlock), 0, x.s, static_cast<const I*>(x.rp),
                         static_cast<const I*>(x.col), static_cast<const T*>(x.e),
                         static_cast<const T*>(x.b), x.ldb, x.k, static_cast<const T*>(x.dy),
                         x.lddy, static_cast<T*>(x.de), x.row_begin, x.nrows, x.n, x.nnz, p.chunk,
                         p.wl.counters, p.wl.items, p.wl.order, b0, p.err);
    });
  });
}

template <typename T, typename I>
int grad_e_typed(const GradEArgs& x) {
  constexpr int VEC = 16 / sizeof(T);
  const int64_t lanes = (x.n + VEC - 1) / VEC;
  const bool fast = edge::fast_shape<T>(x.n, x.k) && rows_aligned(x.b, x.ldb, sizeof(T), VEC) &&
                    rows_aligned(x.e, x.n, sizeof(T), VEC) &&
                    rows_aligned(x.de, x.n, sizeof(T), VEC) &&
                    rows_aligned(x.dy, x.lddy, sizeof(T), VEC);
  if (fast)
    return by_lane_group(lanes, [&](auto lpr) -> int {
      return grad_e_cfg<T, I, decltype(lpr)::value, true>(x);
    });
  return edge::by_general_group(lanes, [&](auto lpr) -> int {
    return grad_e_cfg<T, I, decltype(lpr)::value, false>(x);
  });
}

// ---- d(b) ----------------------------------------------------------------------------------------
// rp / col / perm: the transposed CSR; own: this launch's rows of B (for the mask), X = dy [m, n].
template <typename T, typename I, int VEC, int LPR, int U, bool FAST, int OP, bool RELU>
__global__ void __launch_bounds__(kBlock)
    spmm_edge_grad_b_kernel(const I* __restrict__ rp, const I* __restrict__ col,
                            const I* __restrict__ perm, const T* __restrict__ E,
                            const T* __restrict__ own, int64_t ldb, const T* __restrict__ dy,
                            int64_t lddy, int64_t m, T* __restrict__ out, int64_t ldc,
                            int64_t row_begin, int64_t nrows, int64_t n, int64_t nnz,
                            int64_t chunk, const unsigned long long* __restrict__ counters,
                            const int64_t* __restrict__ items, const int64_t* __restrict__ order,
                            typename Num<T>::acc* __restrict__ part, int64_t block_base,
                            unsigned* err) {
#pragma clang fp contract(off)
  using A = typename Num<T>::acc;
  constexpr int GPW = 64 / LPR;
  constexpr bool NEED_E = edge::grad_b_needs_e(OP, RELU);
  if (poison_rows(counters, block_base, err, out, ldc, (I*)nullptr, (int64_t)0, nrows, n)) return;
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
    T b_row[VEC];
    if constexpr (RELU) load_cols<T, VEC, FAST>(own + it.lr * ldb, cb, n, zero, b_row);
    A acc[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc[e] = A(0);
    edge::for_each_nonzero<T, I, VEC, LPR, U, FAST, true, true, NEED_E>(
        col, perm, dy, lddy, m, E, n, nnz, cb, it.j0, it.j1, gl, gbase,
        [&](int64_t, const T(&gv)[VEC], const T(&ev)[VEC]) {
#pragma unroll
          for (int e = 0; e < VEC; ++e) {
            const A ee = NEED_E ? Num<T>::load(ev[e]) : A(0);
            const A b = RELU ? Num<T>::load(b_row[e]) : A(0);
            acc[e] = acc[e] + Num<T>::load(edge::grad_term<T, OP, RELU>(gv[e], ee, b, ee));
          }
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

struct GradBArgs {
  RowSumArgs r;  // the transposed CSR; val: e, b: this launch's rows of B, c: db; m: k, k: m
  const void *perm, *dy;
  int64_t lddy;
  int op, act;
};

template <typename T, typename I, int LPR, bool FAST>
int grad_b_cfg(const GradBArgs& x) {
  constexpr int VEC = 16 / sizeof(T), U = 8;
  const RowSumArgs& a = x.r;
  return edge::by_op_act(x.op, x.act, [&](auto op, auto relu) -> int {
    return launch_row_sum<T, I>(
        "spmm_csr_edge_grad_b", a, LPR, [&](dim3 grid, int64_t b0, const Planned& p) {
          hipLaunchKernelGGL((spmm_edge_grad_b_kernel<T, I, VEC, LPR, U, FAST, decltype(op)::value,
                                                      decltype(relu)::value>),
                             grid, dim3(kBlock), 0, a.s, static_cast<const I*>(a.rp),
                             static_cast<const I*>(a.col), static_cast<const I*>(x.perm),
                             static_cast<const T*>(a.val), static_cast<const T*>(a.b), a.ldb,
                             static_cast<const T*>(x.dy), x.lddy, a.k, static_cast<T*>(a.c), a.ldc,
                             a.row_begin, a.nrows, a.d, a.nnz, p.chunk, p.wl.counters, p.wl.items,
                             p.wl.order, static_cast<typename Num<T>::acc*>(p.wl.part), b0, p.err);
        });
  });
}

template <typename T, typename I>
int grad_b_typed(const GradBArgs& x) {
  constexpr int VEC = 16 / sizeof(T);
  const RowSumArgs& a = x.r;
  const int64_t lanes = (a.d + VEC - 1) / VEC;
  const bool fast = edge::fast_shape<T>(a.d, a.k) && rows_aligned(a.b, a.ldb, sizeof(T), VEC) &&
                    rows_aligned(a.val, a.d, sizeof(T), VEC) &&
                    rows_aligned(a.c, a.ldc, sizeof(T), VEC) &&
                    rows_aligned(x.dy, x.lddy, sizeof(T), VEC);
  if (fast)
    return by_lane_group(lanes, [&](auto lpr) -> int {
      return grad_b_cfg<T, I, decltype(lpr)::value, true>(x);
    });
  return edge::by_general_group(lanes, [&](auto lpr) -> int {
    return grad_b_cfg<T, I, decltype(lpr)::value, false>(x);
  });
}

}  // namespace
}  // namespace ofx

using namespace ofx;

extern "C" int ofx_spmm_csr_edge_grad_e(void* stream, int idx_dtype, int val_dtype, int64_t m,
                                        int64_t k, int64_t n, int64_t nnz, const void* row_ptr,
                                        const void* col_idx, const void* e, const void* b,
                                        int64_t ldb, int op, int act, const void* dy, int64_t lddy,
                                        void* de, int64_t row_begin, int64_t row_end,
                                        void* workspace, size_t workspace_bytes) {
  return ::ofx::guarded(__func__, [&]() -> int {
    OFX_TAKE_DEVICE_ERROR("spmm_csr_edge_grad_e");  // an earlier launch's loud failure
    bool nothing = false;
    int rc = edge::check_edge_args("spmm_csr_edge_grad_e", true, idx_dtype, val_dtype, m, k, n,
                                   nnz, row_ptr, col_idx, e, b, ldb, op, act, dy, lddy, de, 0,
                                   row_begin, row_end, nullptr, &nothing);
    if (rc || nothing) return rc;
    const int64_t nrows = row_end - row_begin;
    const size_t need = plan::ws_layout(nrows, nnz, 0, 0, scores_schedule()).total;
    if ((rc = check_workspace("spmm_csr_edge_grad_e", workspace, workspace_bytes, need))) return rc;
    const GradEArgs x{static_cast<hipStream_t>(stream), row_ptr, col_idx, e, b, dy, de, ldb, lddy,
                      row_begin, nrows, n, nnz, b ? k : 0, op, act, workspace, workspace_bytes};
    return by_types(idx_dtype, val_dtype, [&](auto* tp, auto* ip) -> int {
      return grad_e_typed<std::remove_pointer_t<decltype(tp)>,
                          std::remove_pointer_t<decltype(ip)>>(x);
    });
  });
}

extern "C" int ofx_spmm_csr_edge_grad_b_workspace_size(int idx_dtype, int val_dtype, int64_t m,
                                                       int64_t k, int64_t n, int64_t nnz,
                                                       const ofx_spmm_options* opts,
                                                       size_t* bytes) {
  return ::ofx::guarded(__func__, [&]() -> int {
    OFX_REQUIRE(bytes != nullptr, OFX_EINVAL, "spmm_csr_edge_grad_b_workspace_size: bytes is NULL");
    OFX_READ_OPTIONS(opts, "spmm_csr_edge_grad_b_workspace_size");
    if (const int rc = edge::check_edge_sizes("spmm_csr_edge_grad_b_workspace_size", idx_dtype,
                                              val_dtype, m, k, n, nnz, opts))
      return rc;
    *bytes = row_sum_ws_bytes(k, nnz, 1, n, val_dtype, opts);
    return OFX_OK;
  });
}

extern "C" int ofx_spmm_csr_edge_grad_b(void* stream, int idx_dtype, int val_dtype, int64_t m,
                                        int64_t k, int64_t n, int64_t nnz, const void* row_ptr_t,
                                        const void* col_idx_t, const void* perm, const void* e,
                                        const void* b, int64_t ldb, int op, int act,
                                        const void* dy, int64_t lddy, void* db, int64_t lddb,
                                        int64_t row_begin, int64_t row_end, void* workspace,
                                        size_t workspace_bytes, const ofx_spmm_options* opts) {
  return ::ofx::guarded(__func__, [&]() -> int {
    OFX_TAKE_DEVICE_ERROR("spmm_csr_edge_grad_b");  // an earlier launch's loud failure
    OFX_READ_OPTIONS(opts, "spmm_csr_edge_grad_b");
    bool nothing = false;
    int rc = edge::check_edge_grad_b_args("spmm_csr_edge_grad_b", idx_dtype, val_dtype, m, k, n,
                                          nnz, row_ptr_t, col_idx_t, perm, e, b, ldb, op, act, dy,
                                          lddy, db, lddb, row_begin, row_end, opts, &nothing);
    if (rc || nothing) return rc;
    const int64_t nrows = row_end - row_begin;
    const size_t need = row_sum_ws_bytes(nrows, nnz, 1, n, val_dtype, opts);
    if ((rc = check_workspace("spmm_csr_edge_grad_b", workspace, workspace_bytes, need))) return rc;
    // the gathered operand is dy: its m rows bound the gather (m == 0: the general path)
    const GradBArgs x{{static_cast<hipStream_t>(stream), row_ptr_t, col_idx_t, e, b, nullptr, db,
                       ldb, lddb, k, row_begin, nrows, 1, n, nnz, dy ? m : 0, workspace,
                       workspace_bytes, opts},
                      perm, dy, lddy, op, act};
    return by_types(idx_dtype, val_dtype, [&](auto* tp, auto* ip) -> int {
      return grad_b_typed<std::remove_pointer_t<decltype(tp)>,
                          std::remove_pointer_t<decltype(ip)>>(x);
    });
  });
}
