// spmm_items_dev.h — what the planned-item kernels share (the SDDMMs of spmm_backward.hip, the
// max / min forward of spmm_extremum.hip and its d(b) of spmm_extremum_grad.hip, the multi-head
// SpMM of spmm_heads.hip and the attention of graph_attention_heads.hip): one lane-group
// per work item (a row or a hub chunk from the shared planner, spmm_plan.h), a grid cut into
// launches of fewer than 2^31 threads, a loud NaN fill when the plan is not valid.  Here are the
// work item's decode, the poison fills, vector loads of a lane's columns, non-temporal stores,
// the host side that lays out and plans the workspace and runs the cut grid, and hub_sum_kernel
// with its launch: the one kernel that adds a summing op's hub-chunk partials.
// Included by HIP translation units only.
#ifndef OFX_SPMM_ITEMS_DEV_H_
#define OFX_SPMM_ITEMS_DEV_H_

#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <type_traits>

#include "ofx_internal.h"
#include "spmm_common.h"
#include "spmm_launch.h"
#include "spmm_plan.h"

namespace ofx {
namespace item {
namespace {  // internal linkage: every HIP translation unit gets its own copy

constexpr int kBlock = 256;
// Grid pieces: a launch holds fewer than 2^32 threads (papers-scale row counts would not).
constexpr int64_t kLaunchBlocks = ((int64_t)1 << 31) / kBlock;

// Work item of lane-group g: the hub chunks first (item index = chunk slot), then the heavy rows,
// then the light rows.  An empty row is an item too: a kernel with a per-row output still writes
// it.  One with per-nonzero outputs passes skip_empty and gets false for it (tested here, not
// after the call: as a second test in the narrow SDDMM it cost four instantiations two VGPRs and
// a wave of occupancy).  slot < 0: a whole row.
struct Item {
  int64_t lr, j0, j1, slot;
};

template <typename I>
__device__ __forceinline__ bool work_item(const I* __restrict__ rp, int64_t g, int64_t row_begin,
                                          int64_t nrows, int64_t chunk,
                                          const unsigned long long* __restrict__ counters,
                                          const int64_t* __restrict__ items,
                                          const int64_t* __restrict__ order, Item* it,
                                          bool skip_empty = false) {
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
  return !skip_empty || it->j0 < it->j1;
}

// A work list from a failed, superseded or never-built plan (spmm_plan.h plan_valid): the launch
// reports it (the host's next entry returns OFX_EPLAN) and fills its whole output with the
// canonical quiet NaN, so that nothing stale can be read as a result.  Every launch of a cut grid
// fills the whole output (idempotent).
__device__ __forceinline__ bool plan_failed(const unsigned long long* __restrict__ counters,
                                            int64_t block_base, unsigned* err) {
  if (counters == nullptr || plan::plan_valid(counters)) return false;
  if (block_base + blockIdx.x == 0 && threadIdx.x == 0)
    plan::raise_device_error(err, plan::kErrPlanInvalid);
  return true;
}

// Outputs of nrows x n (padding left alone); arg, where there is one, becomes -1.
template <typename T, typename I>
__device__ __forceinline__ bool poison_rows(const unsigned long long* __restrict__ counters,
                                            int64_t block_base, unsigned* err,
                                            T* __restrict__ out, int64_t ldc, I* __restrict__ arg,
                                            int64_t ldarg, int64_t nrows, int64_t n) {
  if (!plan_failed(counters, block_base, err)) return false;
  const T p = poison_value<T>();
  const int64_t total = nrows * n;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const int64_t r = i / n, c = i - r * n;
    out[r * ldc + c] = p;
    if (arg != nullptr) arg[r * ldarg + c] = I(-1);
  }
  return true;
}

// Per-nonzero outputs: the nonzeros of the launch's rows,
// out[rp[row_begin] .. rp[row_begin + nrows]).
template <typename T, typename I>
__device__ __forceinline__ bool poison_nonzeros(const unsigned long long* __restrict__ counters,
                                                int64_t block_base, unsigned* err,
                                                const I* __restrict__ rp, int64_t row_begin,
                                                int64_t nrows, T* __restrict__ out) {
  if (!plan_failed(counters, block_base, err)) return false;
  const int64_t j0 = (int64_t)rp[row_begin], j1 = (int64_t)rp[row_begin + nrows];
  const T p = poison_value<T>();
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t j = j0 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < j1; j += stride)
    out[j] = p;
  return true;
}

// The same for `heads` outputs per nonzero (out is [nnz, heads] row-major).  A function of its
// own: the narrow SDDMM's kernels keep the one above as it is.
template <typename T, typename I>
__device__ __forceinline__ bool poison_head_nonzeros(const unsigned long long* __restrict__ counters,
                                                     int64_t block_base, unsigned* err,
                                                     const I* __restrict__ rp, int64_t row_begin,
                                                     int64_t nrows, int64_t heads,
                                                     T* __restrict__ out) {
  if (!plan_failed(counters, block_base, err)) return false;
  const int64_t e0 = (int64_t)rp[row_begin] * heads, e1 = (int64_t)rp[row_begin + nrows] * heads;
  const T p = poison_value<T>();
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t e = e0 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < e1; e += stride)
    out[e] = p;
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

// The work list of a launch over rows [row_begin, row_begin + nrows), laid out in `ws` for `sched`
// (partials of part_bytes_per_elem * n bytes per chunk): adopted when `planned` says the workspace
// already holds it (the plan entries lay it out the same way), planned here otherwise.  A launch
// without a plan (no row can be cut) reads the identity work list.
struct Planned {
  plan::WsLayout w;
  plan::WorkList wl;
  Schedule sched;
  bool has_plan;
  int64_t work;   // items of the launch: the rows and, with a plan, the hub chunks' slots
  int64_t chunk;  // work_item's chunk length
  unsigned* err;  // where the kernel reports a plan that is not valid
};

template <typename I>
int prepare_plan(const char* fn, hipStream_t stream, const I* rp, int64_t row_begin, int64_t nrows,
                 int64_t nnz, int64_t nnz_est, int64_t n, size_t part_bytes_per_elem,
                 const Schedule& sched, bool planned, void* ws, size_t ws_bytes, Planned* out) {
  out->sched = sched;
  out->w = plan::ws_layout(nrows, nnz, n, part_bytes_per_elem, sched);
  out->wl = plan::WorkList{};
  out->has_plan = out->w.total > 0;
  out->work = nrows + (out->has_plan ? out->w.max_chunks : 0);
  out->chunk = out->has_plan ? sched.chunk : INT64_MAX;
  out->err = out->has_plan ? device_error_words() : nullptr;
  if (!out->has_plan) return OFX_OK;
  OFX_REQUIRE(ws != nullptr && ws_bytes >= out->w.total, OFX_EWORKSPACE,
              "%s: workspace of %zu bytes < %zu required", fn, ws_bytes, out->w.total);
  if (planned) {
    plan::worklist_of(out->w, static_cast<char*>(ws), &out->wl);
    return OFX_OK;
  }
  return plan::launch_plan<I>(stream, rp, row_begin, nrows, nnz_est, sched, out->w,
                              static_cast<char*>(ws), &out->wl);
}

// The same with the sum op's schedule options, laid out exactly as ofx_spmm_csr lays out its own
// (launch_schedule, ws_layout; only the partials' size differs), so a plan ofx_spmm_csr_plan built
// there is reused when opts->planned is set.  The small form of the sum op plans nothing, so such
// a launch plans here whatever `planned` says.
template <typename I>
int prepare_plan(const char* fn, hipStream_t stream, const I* rp, int64_t m, int64_t row_begin,
                 int64_t nrows, int64_t nnz, int64_t n, size_t part_bytes_per_elem,
                 const ofx_spmm_options* opts, void* ws, size_t ws_bytes, Planned* out) {
  const int64_t nnz_est = launch_nnz(m, nrows, nnz, opts);
  const Schedule sched = launch_schedule(nrows, nnz_est, n, resolve_schedule(n, opts));
  const bool planned = opts != nullptr && opts->planned != 0 &&
                       launch_form(nrows, nnz_est, n, sched) != Form::Small;
  // these entries' wording of the size error, ahead of the shared check
  const size_t need = plan::ws_layout(nrows, nnz, n, part_bytes_per_elem, sched).total;
  if (const int rc = check_workspace(fn, ws, ws_bytes, need)) return rc;
  return prepare_plan<I>(fn, stream, rp, row_begin, nrows, nnz, nnz_est, n, part_bytes_per_elem,
                         sched, planned, ws, ws_bytes, out);
}

inline size_t workspace_bytes(int64_t m, int64_t nnz, int64_t n, size_t part_bytes_per_elem,
                              const ofx_spmm_options* opts) {
  const Schedule s = launch_schedule(m, nnz, n, resolve_schedule(n, opts));
  return plan::ws_layout(m, nnz, n, part_bytes_per_elem, s).total;
}

// Runs launch(grid, block_base) over `work` items, groups_per_block to a block, in pieces of at
// most kLaunchBlocks blocks (fewer than 2^31 threads per launch).
template <typename F>
int launch_cut_grid(int64_t work, int64_t groups_per_block, F&& launch) {
  const int64_t grid = (work + groups_per_block - 1) / groups_per_block;
  for (int64_t b0 = 0; b0 < grid; b0 += kLaunchBlocks) {
    launch(dim3((unsigned)std::min(kLaunchBlocks, grid - b0)), b0);
    OFX_HIP_CHECK(hipGetLastError());
  }
  return OFX_OK;
}

// The hub rows of a sum: the chunk partials added in chunk order into +0, rounded once.  One block
// per hub, grid-strided; threads over the columns.
template <typename T>
__global__ void __launch_bounds__(kBlock)
    hub_sum_kernel(const unsigned long long* __restrict__ counters,
                   const int64_t* __restrict__ hubs,
                   const typename Num<T>::acc* __restrict__ part, T* __restrict__ out,
                   int64_t ldc, int64_t nrows, int64_t n) {
#pragma clang fp contract(off)
  using A = typename Num<T>::acc;
  if (!plan::plan_valid(counters)) return;  // the main kernel has poisoned the output
  const int64_t nhubs = (int64_t)counters[1];
  for (int64_t h = blockIdx.x; h < nhubs; h += gridDim.x) {
    const int64_t lr = hubs[3 * h], s0 = hubs[3 * h + 1], nc = hubs[3 * h + 2];
    if ((uint64_t)lr >= (uint64_t)nrows) continue;  // never from a valid plan
    for (int64_t c = threadIdx.x; c < n; c += kBlock) {
      A acc = A(0);
      for (int64_t q = 0; q < nc; ++q) acc = acc + part[(s0 + q) * n + c];
      nt_store_one(out + lr * ldc + c, Num<T>::store(acc));
    }
  }
}

// Launches it over the hubs of plan `p` (nothing without a plan or without room for a hub), for
// the plane of partials `part`: the workspace's own, or one of several an op laid out there.
template <typename T>
int launch_hub_sum(hipStream_t stream, const Planned& p, const typename Num<T>::acc* part, T* out,
                   int64_t ldc, int64_t nrows, int64_t n) {
  if (!p.has_plan || p.w.max_hubs == 0) return OFX_OK;
  const unsigned hgrid = (unsigned)std::min<int64_t>(p.w.max_hubs, 8192);
  hipLaunchKernelGGL((hub_sum_kernel<T>), dim3(hgrid), dim3(kBlock), 0, stream, p.wl.counters,
                     p.wl.hubs, part, out, ldc, nrows, n);
  OFX_HIP_CHECK(hipGetLastError());
  return OFX_OK;
}
template <typename T>
int launch_hub_sum(hipStream_t stream, const Planned& p, T* out, int64_t ldc, int64_t nrows,
                   int64_t n) {
  return launch_hub_sum<T>(stream, p, static_cast<const typename Num<T>::acc*>(p.wl.part), out, ldc,
                           nrows, n);
}

}  // namespace
}  // namespace item
}  // namespace ofx

#endif  // OFX_SPMM_ITEMS_DEV_H_
