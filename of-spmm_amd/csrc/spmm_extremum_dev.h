// spmm_extremum_dev.h — device-side pieces the HIP units of the max / min reductions share
// (spmm_extremum.hip, spmm_extremum_grad.hip, spmm_extremum_sddmm.hip): the work item of a
// lane-group (a row or a hub chunk from the shared planner, spmm_plan.h), vector loads of a lane's
// columns, non-temporal stores, and the host side that lays out and plans the workspace.
// Included by HIP translation units only.
#ifndef OFX_SPMM_EXTREMUM_DEV_H_
#define OFX_SPMM_EXTREMUM_DEV_H_

#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

#include "ofx_internal.h"
#include "spmm_common.h"
#include "spmm_extremum.h"
#include "spmm_launch.h"
#include "spmm_plan.h"

namespace ofx {
namespace xt {
namespace {  // internal linkage: every HIP translation unit gets its own copy

constexpr int kBlock = 256;
// Grid pieces: a launch holds fewer than 2^32 threads.
constexpr int64_t kLaunchBlocks = ((int64_t)1 << 31) / kBlock;

// Work item of lane-group g, as the SDDMM reads the work list (spmm_backward.hip sddmm_item): the
// hub chunks first (item index = chunk slot), then the heavy rows, then the light rows.  An empty
// row is an item too (it still writes its output).  slot < 0: a whole row.
struct Item {
  int64_t lr, j0, j1, slot;
};

template <typename I>
__device__ __forceinline__ bool work_item(const I* __restrict__ rp, int64_t g, int64_t row_begin,
                                          int64_t nrows, int64_t chunk,
                                          const unsigned long long* __restrict__ counters,
                                          const int64_t* __restrict__ items,
                                          const int64_t* __restrict__ order, Item* it) {
  int64_t lr, c = -1;
  it->slot = -1;
  if (order == nullptr) {  // identity work list: no plan
    if (g >= nrows) return false;
    lr = g;
  } else {
    const int64_t nchunks = (int64_t)counters[0];
    if (g < nchunks) {
      lr = items[2 * g];
      c = items[2 * g + 1];
      it->slot = g;
    } else {
      const int64_t q = g - nchunks;
      if (q >= nrows - (int64_t)counters[1]) return false;
      lr = plan::order_row(order, nrows, (int64_t)counters[3] - (int64_t)counters[2], q);
    }
  }
  if ((uint64_t)lr >= (uint64_t)nrows) return false;  // never from a valid plan
  const int64_t r = row_begin + lr;
  const int64_t rs = (int64_t)rp[r], re = (int64_t)rp[r + 1];
  it->lr = lr;
  it->j0 = rs;
  it->j1 = re;
  if (c >= 0) {  // chunk c of len / chunk; the last takes the remainder
    it->j0 = rs + c * chunk;
    it->j1 = (re - it->j0 - chunk < chunk) ? re : it->j0 + chunk;
  }
  return true;
}

// VEC consecutive elements of one row as one load of up to 16 bytes.
template <typename E, int VEC>
struct alignas(VEC * sizeof(E) >= 16 ? 16 : VEC * sizeof(E)) Pack {
  E v[VEC];
};

// x[e] = row[cb + e] for the lane's VEC columns [cb, cb + VEC); columns >= n read as `fill`.
// ALIGNED: n % VEC == 0 and the row is 16-byte aligned, so the lane's columns are all in or out.
template <typename E, int VEC, bool ALIGNED>
__device__ __forceinline__ void load_cols(const E* __restrict__ row, int64_t cb, int64_t n,
                                          E fill, E (&x)[VEC]) {
  if constexpr (ALIGNED) {
    if (cb < n) {
      constexpr int per = (VEC * sizeof(E) >= 16 ? 16 : VEC * sizeof(E)) / sizeof(E);
#pragma unroll
      for (int q = 0; q < VEC / per; ++q) {
        const Pack<E, per> p = *reinterpret_cast<const Pack<E, per>*>(row + cb + q * per);
#pragma unroll
        for (int e = 0; e < per; ++e) x[q * per + e] = p.v[e];
      }
      return;
    }
#pragma unroll
    for (int e = 0; e < VEC; ++e) x[e] = fill;
  } else {
#pragma unroll
    for (int e = 0; e < VEC; ++e) x[e] = cb + e < n ? row[cb + e] : fill;
  }
}

// Non-temporal stores of the lane's VEC columns: the outputs are written once and not read by
// this launch, so they should not evict the B rows the gather reuses.
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

template <typename E>
__device__ __forceinline__ void nt_store_one(E* p, E v) {
  using U = std::conditional_t<sizeof(E) == 2, uint16_t,
                               std::conditional_t<sizeof(E) == 4, uint32_t, uint64_t>>;
  __builtin_nontemporal_store(__builtin_bit_cast(U, v), reinterpret_cast<U*>(p));
}

template <typename E, int VEC, bool ALIGNED>
__device__ __forceinline__ void store_cols(E* __restrict__ row, int64_t cb, int64_t n,
                                           const E (&x)[VEC]) {
  if constexpr (ALIGNED) {
    if (cb >= n) return;
    constexpr int bytes = VEC * sizeof(E);
    if constexpr (bytes % 16 == 0) {
      Pack<E, VEC> p;
#pragma unroll
      for (int e = 0; e < VEC; ++e) p.v[e] = x[e];
      struct Raw {
        u32x4 q[bytes / 16];
      };
      const Raw raw = __builtin_bit_cast(Raw, p);
#pragma unroll
      for (int q = 0; q < bytes / 16; ++q)
        __builtin_nontemporal_store(raw.q[q], reinterpret_cast<u32x4*>(row + cb) + q);
    } else {
      static_assert(bytes == 8, "a lane's columns are 8 bytes or a multiple of 16");
      Pack<E, VEC> p;
#pragma unroll
      for (int e = 0; e < VEC; ++e) p.v[e] = x[e];
      __builtin_nontemporal_store(__builtin_bit_cast(u32x2, p), reinterpret_cast<u32x2*>(row + cb));
    }
  } else {
#pragma unroll
    for (int e = 0; e < VEC; ++e)
      if (cb + e < n) nt_store_one(row + cb + e, x[e]);
  }
}

// Whether rows of `ld` elements of `esize` bytes starting at p can be read / written as whole
// lanes of VEC elements.
inline bool rows_aligned(const void* p, int64_t ld, size_t esize, int vec) {
  const size_t bytes = std::min<size_t>(16, (size_t)vec * esize);
  return p == nullptr || (((uintptr_t)p % bytes) == 0 && ((size_t)ld * esize) % bytes == 0);
}

// The work list of a launch over rows [row_begin, row_begin + nrows): laid out in `ws` exactly as
// ofx_spmm_csr lays out its own (launch_schedule, ws_layout; only the partials' size differs), so
// a plan ofx_spmm_csr_plan built there is reused when opts->planned is set.  The small form of the
// sum op plans nothing, so such a launch plans here whatever `planned` says.
struct Planned {
  plan::WsLayout w;
  plan::WorkList wl;
  Schedule sched;
  bool has_plan;
};

template <typename I>
int prepare_plan(const char* fn, hipStream_t stream, const I* rp, int64_t m, int64_t row_begin,
                 int64_t nrows, int64_t nnz, int64_t n, size_t part_bytes_per_elem,
                 const ofx_spmm_options* opts, void* ws, size_t ws_bytes, Planned* out) {
  const int64_t nnz_est = launch_nnz(m, nrows, nnz, opts);
  out->sched = launch_schedule(nrows, nnz_est, n, resolve_schedule(n, opts));
  out->w = plan::ws_layout(nrows, nnz, n, part_bytes_per_elem, out->sched);
  out->wl = plan::WorkList{};
  out->has_plan = out->w.total > 0;
  if (!out->has_plan) return OFX_OK;
  OFX_REQUIRE(ws != nullptr && ws_bytes >= out->w.total, OFX_EWORKSPACE,
              "%s: workspace of %zu bytes is smaller than the %zu bytes required", fn, ws_bytes,
              out->w.total);
  if (opts != nullptr && opts->planned != 0 && !use_small_form(nrows, nnz_est, n, out->sched)) {
    plan::worklist_of(out->w, static_cast<char*>(ws), &out->wl);
    return OFX_OK;
  }
  return plan::launch_plan<I>(stream, rp, row_begin, nrows, nnz_est, out->sched, out->w,
                              static_cast<char*>(ws), &out->wl);
}

inline size_t workspace_bytes(int64_t m, int64_t nnz, int64_t n, size_t part_bytes_per_elem,
                              const ofx_spmm_options* opts) {
  const Schedule s = launch_schedule(m, nnz, n, resolve_schedule(n, opts));
  return plan::ws_layout(m, nnz, n, part_bytes_per_elem, s).total;
}

// Calls f(T*, I*) with null pointers of the value / index types the dtype codes name.
template <typename F>
int by_types(int idx_dtype, int val_dtype, F&& f) {
  auto with_i = [&](auto* ip) -> int {
    switch (val_dtype) {
      case OFX_DT_FLOAT: return f((float*)nullptr, ip);
      case OFX_DT_DOUBLE: return f((double*)nullptr, ip);
      case OFX_DT_BFLOAT16: return f((bf16*)nullptr, ip);
      default: return f((f16*)nullptr, ip);
    }
  };
  if (idx_dtype == OFX_DT_INT32) return with_i((int32_t*)nullptr);
  return with_i((int64_t*)nullptr);
}

}  // namespace
}  // namespace xt
}  // namespace ofx

#endif  // OFX_SPMM_EXTREMUM_DEV_H_
