// spmm_multi.hip — the multi-aggregator SpMM (op "spmm_csr_multi"), gfx950: sum, mean, max, min,
// var and std of the messages p_j[c] = mul(val[j], B[col[j], c]) of every row from ONE walk of the
// CSR and one gather of B (Principal Neighbourhood Aggregation, PyG's MultiAggregation).  Contract
// (include/ofx_spmm.h): the sum and mean slices have ofx_spmm_csr's and the mean
// reduction's bits, the max / min slices and their args ofx_spmm_csr_reduce's; var and std come
// from s1 = sum p and s2 = sum p * p in the accumulation type, summed in ofx_spmm_csr's order under
// its hub rule, through the one finishing step of spmm_multi.h.
//
// The gather is the cost (DESIGN.md §3 Roofline), so every gathered element feeds all the running
// statistics while it is in a register: per lane and column s1, s2, the best max and min and their
// two nonzero indices.  Lane layout as the extremum kernel's: a group of LPR lanes per work item (a
// row or a hub chunk from the shared planner), each lane VEC = 16 / sizeof(T) columns; (col, val)
// loaded LPR at a time and broadcast by cross-lane moves; min(U, LPR) unconditional 16-byte B-row
// loads in flight before the chain of updates (a slot past the batch's end repeats its last
// nonzero, a column outside [0, k) reads row 0 and becomes zeros); non-temporal stores; widths
// beyond LPR * VEC loop over column tiles.  What is tracked is two template parameters (the moments
// 0 / 1 / 2, the extrema none / both): five kernels per layout.  The general path (scalar loads:
// N % VEC != 0, unaligned bases or strides, K = 0) tracks everything.  A hub chunk writes one
// record per column (s1, s2, both winners, both indices) and multi_hub_kernel combines a hub's
// records in chunk order.  No atomics, no LDS, no allocation, no host synchronisation.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include "heads_steps.h"  // the lane ladder
#include "spmm_edge_dev.h"  // the general path's lane groups
#include "spmm_items_dev.h"
#include "spmm_multi.h"

namespace ofx {
namespace {

using namespace item;
using multi::Outputs;
using multi::Stats;

// The planes of the hub chunks' records, [max_chunks, n] each: the int64 indices first (the
// region starts 8-byte aligned), then the four statistics in the accumulation type.
template <typename A>
struct Parts {
  int64_t *amax, *amin;
  A *s1, *s2, *mx, *mn;
};

template <typename A>
constexpr size_t record_bytes() {
  return 2 * sizeof(int64_t) + 4 * sizeof(A);
}

template <typename A>
__host__ __device__ __forceinline__ Parts<A> parts_of(void* region, int64_t max_chunks, int64_t n) {
  const int64_t plane = max_chunks * n;
  int64_t* ix = static_cast<int64_t*>(region);
  A* st = reinterpret_cast<A*>(ix + 2 * plane);
  return {ix, ix + plane, st, st + plane, st + 2 * plane, st + 3 * plane};
}

// What a kernel is handed of the outputs and of the hub records.  The slice pointers (Outputs) and
// the record planes are formed where they are used, after the walk: as kernel arguments they were
// 36 scalar registers live across it, and the widest kernels spilled scalars.
struct Dest {
  void *c, *arg_max, *arg_min;
  int64_t ldc, slice_stride, ldarg;
  double eps;
  int mask;
};
struct Records {
  void* region;
  int64_t max_chunks;
};

template <typename T, typename I>
__device__ __forceinline__ Outputs<T, I> outputs_of(const Dest& d) {
  return multi::outputs_of<T, I>(d.mask, d.c, d.ldc, d.slice_stride, d.arg_max, d.arg_min, d.ldarg,
                                 d.eps);
}

// The aggregators a (MOM, EXT) kernel can finish: what it does not track is folded away.
template <int MOM, bool EXT>
constexpr int tracked_mask() {
  return (MOM >= 1 ? OFX_AGGR_SUM | OFX_AGGR_MEAN : 0) | (MOM >= 2 ? OFX_AGGR_VAR | OFX_AGGR_STD : 0) |
         (EXT ? OFX_AGGR_MAX | OFX_AGGR_MIN : 0);
}

// No valid plan: every requested slice becomes the canonical NaN, the args -1, and the device
// error word is raised (poison_rows of the reduce op, over all the outputs).
template <typename T, typename I>
__device__ __forceinline__ bool poison_outputs(const unsigned long long* __restrict__ counters,
                                               int64_t block_base, unsigned* err,
                                               const Dest& dest, int64_t nrows, int64_t n) {
  if (!plan_failed(counters, block_base, err)) return false;
  const Outputs<T, I> o = outputs_of<T, I>(dest);
  const T p = poison_value<T>();
  const int64_t total = nrows * n;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const int64_t r = i / n, c = i - r * n;
    const int64_t at = r * o.ldc + c;
    if (o.sum != nullptr) o.sum[at] = p;
    if (o.mean != nullptr) o.mean[at] = p;
    if (o.mx != nullptr) o.mx[at] = p;
    if (o.mn != nullptr) o.mn[at] = p;
    if (o.var != nullptr) o.var[at] = p;
    if (o.sd != nullptr) o.sd[at] = p;
    if (o.arg_max != nullptr) o.arg_max[r * o.ldarg + c] = I(-1);
    if (o.arg_min != nullptr) o.arg_min[r * o.ldarg + c] = I(-1);
  }
  return true;
}

template <typename T, typename I, int VEC, int LPR, int UMAX, bool FAST, int MOM, bool EXT>
__global__ void __launch_bounds__(kBlock)
    multi_kernel(const I* __restrict__ rp, const I* __restrict__ col, const T* __restrict__ val,
                 const T* __restrict__ B, int64_t ldb, int64_t kb, const Dest dest,
                 int64_t row_begin, int64_t nrows, int64_t n, int64_t chunk,
                 const unsigned long long* __restrict__ counters,
                 const int64_t* __restrict__ items, const int64_t* __restrict__ order,
                 const Records rec, int64_t block_base, unsigned* err) {
#pragma clang fp contract(off)
  using A = typename Num<T>::acc;
  constexpr int GPW = 64 / LPR;
  // a batch holds at most LPR nonzeros: more slots would repeat its last nonzero's load
  constexpr int U = UMAX < LPR ? UMAX : LPR;
  if (poison_outputs<T, I>(counters, block_base, err, dest, nrows, n)) return;
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
    const int64_t cbs = cb < n ? cb : 0;  // a lane past the row's width reads column 0
    Stats<A, I> st[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) st[e] = multi::empty_stats<A, I>();
    for (int64_t jb = it.j0; jb < it.j1; jb += LPR) {
      const int cnt = (int)((it.j1 - jb) < LPR ? (it.j1 - jb) : LPR);
      const I myc = gl < cnt ? col[jb + gl] : I(0);
      const A myv = gl < cnt ? Num<T>::load(val[jb + gl]) : A(0);
      for (int k = 0; k < cnt; k += U) {
        Pack<T, VEC> xv[U];
        if constexpr (FAST) {
          // every load of the round is unconditional and stays one 16-byte word until it is used
          // (loads behind per-slot branches are issued one at a time)
          static_assert(sizeof(Pack<T, VEC>) == sizeof(u32x4), "a lane's columns are 16 bytes");
          u32x4 raw[U];
          unsigned inmask = 0;
#pragma unroll
          for (int u = 0; u < U; ++u) {
            const int ku = k + u < cnt ? k + u : cnt - 1;
            const int64_t cu = (int64_t)__shfl((int64_t)myc, gbase + (ku & (LPR - 1)), 64);
            const bool in = (uint64_t)cu < (uint64_t)kb;
            inmask |= (in ? 1u : 0u) << u;
            raw[u] = *reinterpret_cast<const u32x4*>(B + (in ? cu : 0) * ldb + cbs);
          }
#pragma unroll
          for (int u = 0; u < U; ++u) {
            // a column outside [0, k): the zero-filled gathered row of the sum op
            const u32x4 r = ((inmask >> u) & 1u) ? raw[u] : u32x4{0u, 0u, 0u, 0u};
            xv[u] = __builtin_bit_cast(Pack<T, VEC>, r);
          }
        } else {
#pragma unroll
          for (int u = 0; u < U; ++u) {
            const int64_t cu = (int64_t)__shfl((int64_t)myc, gbase + ((k + u) & (LPR - 1)), 64);
            if (k + u < cnt) {
              // every column reads as out of range and the row's address is never used
              const bool in = (uint64_t)cu < (uint64_t)kb;
              load_cols<T, VEC, false>(B + (in ? cu : 0) * ldb, in ? cb : n, n, zero, xv[u].v);
            }
          }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const A v = __shfl(myv, gbase + ((k + u) & (LPR - 1)), 64);
          if (k + u < cnt) {
            const I j = (I)(jb + k + u);
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
              const A b = Num<T>::load(xv[u].v[e]);
              // the extrema store the winner's own bits: the sign of a zero product is kept
              const A p = EXT ? signed_product<T>(v, b) : Num<T>::mul(v, b);
              multi::feed<MOM, EXT>(st[e], p, j);
            }
          }
        }
      }
    }
    if (it.slot >= 0) {  // a hub chunk's record: combined in chunk order by multi_hub_kernel
      const Parts<A> part = parts_of<A>(rec.region, rec.max_chunks, n);
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        if (cb + e < n) {
          const int64_t at = it.slot * n + cb + e;
          part.s1[at] = st[e].s1;
          part.s2[at] = st[e].s2;
          part.mx[at] = st[e].mx;
          part.mn[at] = st[e].mn;
          part.amax[at] = (int64_t)st[e].amax;
          part.amin[at] = (int64_t)st[e].amin;
        }
      }
    } else {
      const Outputs<T, I> o = outputs_of<T, I>(dest);
      const int64_t deg = it.j1 - it.j0;
      multi::Finished<T> f[VEC];
#pragma unroll
      for (int e = 0; e < VEC; ++e)
        f[e] = multi::finish<T>(st[e], deg, o.eps, o.mask & tracked_mask<MOM, EXT>());
      using F = multi::Finished<T>;
      const auto emit = [&](T* slice, auto get) {
        if (slice == nullptr) return;
        T x[VEC];
#pragma unroll
        for (int e = 0; e < VEC; ++e) x[e] = get(f[e]);
        store_cols<T, VEC, FAST>(slice + it.lr * o.ldc, cb, n, x);
      };
      if constexpr (MOM >= 1) {
        emit(o.sum, [](const F& x) { return x.sum; });
        emit(o.mean, [](const F& x) { return x.mean; });
      }
      if constexpr (MOM >= 2) {
        emit(o.var, [](const F& x) { return x.var; });
        emit(o.sd, [](const F& x) { return x.sd; });
      }
      if constexpr (EXT) {
        emit(o.mx, [](const F& x) { return x.mx; });
        emit(o.mn, [](const F& x) { return x.mn; });
        I a[VEC];
        if (o.arg_max != nullptr) {
#pragma unroll
          for (int e = 0; e < VEC; ++e) a[e] = st[e].amax;
          store_cols<I, VEC, FAST>(o.arg_max + it.lr * o.ldarg, cb, n, a);
        }
        if (o.arg_min != nullptr) {
#pragma unroll
          for (int e = 0; e < VEC; ++e) a[e] = st[e].amin;
          store_cols<I, VEC, FAST>(o.arg_min + it.lr * o.ldarg, cb, n, a);
        }
      }
    }
  }
}

// The hub rows: the records of a hub's chunks merged in chunk order (the moments into +0, the
// extrema by the strict rule), then the finishing step with the whole row's degree.  One block per
// hub, grid-strided; threads over the columns.
template <typename T, typename I>
__global__ void __launch_bounds__(kBlock)
    multi_hub_kernel(const unsigned long long* __restrict__ counters,
                     const int64_t* __restrict__ hubs, const Records rec,
                     const I* __restrict__ rp, int64_t row_begin, const Dest dest, int64_t nrows,
                     int64_t n) {
#pragma clang fp contract(off)
  using A = typename Num<T>::acc;
  if (!plan::plan_valid(counters)) return;  // the main kernel has poisoned the outputs
  const Parts<A> part = parts_of<A>(rec.region, rec.max_chunks, n);
  const Outputs<T, I> o = outputs_of<T, I>(dest);
  const int64_t nhubs = (int64_t)counters[1];
  for (int64_t h = blockIdx.x; h < nhubs; h += gridDim.x) {
    const int64_t lr = hubs[3 * h], s0 = hubs[3 * h + 1], nc = hubs[3 * h + 2];
    if ((uint64_t)lr >= (uint64_t)nrows) continue;  // never from a valid plan
    const int64_t deg = (int64_t)rp[row_begin + lr + 1] - (int64_t)rp[row_begin + lr];
    for (int64_t c = threadIdx.x; c < n; c += kBlock) {
      const auto record = [&](int64_t q) -> Stats<A, int64_t> {
        const int64_t at = (s0 + q) * n + c;
        return {part.s1[at], part.s2[at], part.mx[at], part.mn[at], part.amax[at], part.amin[at]};
      };
      Stats<A, int64_t> s = record(0);
      s.s1 = A(0) + s.s1;
      s.s2 = A(0) + s.s2;
      for (int64_t q = 1; q < nc; ++q) multi::merge(s, record(q));
      const multi::Finished<T> f = multi::finish<T>(s, deg, o.eps, o.mask);
      const int64_t at = lr * o.ldc + c;
      if (o.sum != nullptr) nt_store_one(o.sum + at, f.sum);
      if (o.mean != nullptr) nt_store_one(o.mean + at, f.mean);
      if (o.mx != nullptr) nt_store_one(o.mx + at, f.mx);
      if (o.mn != nullptr) nt_store_one(o.mn + at, f.mn);
      if (o.var != nullptr) nt_store_one(o.var + at, f.var);
      if (o.sd != nullptr) nt_store_one(o.sd + at, f.sd);
      if (o.arg_max != nullptr) nt_store_one(o.arg_max + lr * o.ldarg + c, (I)s.amax);
      if (o.arg_min != nullptr) nt_store_one(o.arg_min + lr * o.ldarg + c, (I)s.amin);
    }
  }
}

struct MultiArgs {
  hipStream_t s;
  const void *rp, *col, *val, *b;
  void *c, *arg_max, *arg_min;
  int64_t ldb, ldc, slice_stride, ldarg, m, row_begin, nrows, n, nnz, k;
  int mask;
  double eps;
  void* ws;
  size_t ws_bytes;
  const ofx_spmm_options* opts;
};

// Loads in flight per lane: 8 for the four-byte and eight-byte types, 4 for the 16-bit ones, whose
// 48 statistic registers sit next to them (the register table).
template <typename T>
constexpr int loads_in_flight() {
  return sizeof(T) == 2 ? 4 : 8;
}

template <typename T, typename I, int LPR, bool FAST, int MOM, bool EXT>
int multi_cfg(const MultiArgs& a) {
  using A = typename Num<T>::acc;
  constexpr int VEC = 16 / sizeof(T), U = loads_in_flight<T>();
  constexpr int64_t GPB = (kBlock / 64) * (64 / LPR);
  Planned p;
  int rc = prepare_plan<I>("spmm_csr_multi", a.s, static_cast<const I*>(a.rp), a.m, a.row_begin,
                           a.nrows, a.nnz, a.n, record_bytes<A>(), a.opts, a.ws, a.ws_bytes, &p);
  if (rc) return rc;
  const Records rec{p.has_plan ? p.wl.part : nullptr, p.has_plan ? p.w.max_chunks : 0};
  const Dest dest{a.c, a.arg_max, a.arg_min, a.ldc, a.slice_stride, a.ldarg, a.eps, a.mask};
  rc = launch_cut_grid(p.work, GPB, [&](dim3 grid, int64_t b0) {
    hipLaunchKernelGGL((multi_kernel<T, I, VEC, LPR, U, FAST, MOM, EXT>), grid, dim3(kBlock), 0,
                       a.s, static_cast<const I*>(a.rp), static_cast<const I*>(a.col),
                       static_cast<const T*>(a.val), static_cast<const T*>(a.b), a.ldb, a.k, dest,
                       a.row_begin, a.nrows, a.n, p.chunk, p.wl.counters, p.wl.items, p.wl.order,
                       rec, b0, p.err);
  });
  if (rc) return rc;
  if (p.has_plan && p.w.max_hubs > 0) {
    const unsigned hgrid = (unsigned)std::min<int64_t>(p.w.max_hubs, 8192);
    hipLaunchKernelGGL((multi_hub_kernel<T, I>), dim3(hgrid), dim3(kBlock), 0, a.s, p.wl.counters,
                       p.wl.hubs, rec, static_cast<const I*>(a.rp), a.row_begin, dest, a.nrows, a.n);
    OFX_HIP_CHECK(hipGetLastError());
  }
  return OFX_OK;
}

// f(moments, extrema) as integral constants for what the mask asks to track.
template <typename F>
int by_tracking(int mask, F&& f) {
  using hsteps::Int;
  const int mom = multi::moments_of(mask);
  if (!multi::extrema_of(mask))
    return mom == 2 ? f(Int<2>{}, std::false_type{}) : f(Int<1>{}, std::false_type{});
  if (mom == 0) return f(Int<0>{}, std::true_type{});
  return mom == 2 ? f(Int<2>{}, std::true_type{}) : f(Int<1>{}, std::true_type{});
}

template <typename T, typename I>
int multi_typed(const MultiArgs& a) {
  constexpr int VEC = 16 / sizeof(T);
  const int64_t lanes = (a.n + VEC - 1) / VEC;
  const bool one = multi::num_slices(a.mask) == 1;
  const bool fast = edge::fast_shape<T>(a.n, a.k) && rows_aligned(a.b, a.ldb, sizeof(T), VEC) &&
                    rows_aligned(a.c, a.ldc, sizeof(T), VEC) &&
                    (one || a.slice_stride * (int64_t)sizeof(T) % 16 == 0) &&
                    rows_aligned(a.arg_max, a.ldarg, sizeof(I), VEC) &&
                    rows_aligned(a.arg_min, a.ldarg, sizeof(I), VEC);
  if (fast)
    return hsteps::by_lane_group(lanes, [&](auto lpr) -> int {
      return by_tracking(a.mask, [&](auto mom, auto ext) -> int {
        return multi_cfg<T, I, decltype(lpr)::value, true, decltype(mom)::value,
                         decltype(ext)::value>(a);
      });
    });
  // the correctness path of widths and bases no benchmark configuration takes: everything tracked
  return edge::by_general_group(lanes, [&](auto lpr) -> int {
    return multi_cfg<T, I, decltype(lpr)::value, false, 2, true>(a);
  });
}

}  // namespace
}  // namespace ofx

using namespace ofx;

extern "C" int ofx_spmm_csr_multi_workspace_size(int idx_dtype, int val_dtype, int64_t m,
                                                 int64_t k, int64_t n, int64_t nnz, int aggr_mask,
                                                 const ofx_spmm_options* opts, size_t* bytes) {
  return ::ofx::guarded(__func__, [&]() -> int {
    OFX_REQUIRE(bytes != nullptr, OFX_EINVAL, "spmm_csr_multi_workspace_size: bytes is NULL");
    OFX_READ_OPTIONS(opts, "spmm_csr_multi_workspace_size");
    if (const int rc = multi::check_multi_sizes("spmm_csr_multi_workspace_size", idx_dtype,
                                                val_dtype, m, k, n, nnz, aggr_mask))
      return rc;
    *bytes = item::workspace_bytes(
        m, nnz, n, 2 * sizeof(int64_t) + 4 * (val_dtype == OFX_DT_DOUBLE ? 8 : 4), opts);
    return OFX_OK;
  });
}

extern "C" int ofx_spmm_csr_multi(void* stream, int idx_dtype, int val_dtype, int64_t m, int64_t k,
                                  int64_t n, int64_t nnz, const void* row_ptr, const void* col_idx,
                                  const void* values, const void* b, int64_t ldb, int aggr_mask,
                                  double eps, void* c, int64_t ldc, int64_t slice_stride,
                                  void* arg_max, void* arg_min, int64_t ldarg, int64_t row_begin,
                                  int64_t row_end, void* workspace, size_t workspace_bytes,
                                  const ofx_spmm_options* opts) {
  return ::ofx::guarded(__func__, [&]() -> int {
    OFX_TAKE_DEVICE_ERROR("spmm_csr_multi");  // an earlier launch's loud failure (spmm_plan.h)
    OFX_READ_OPTIONS(opts, "spmm_csr_multi");
    bool nothing = false;
    const int rc = multi::check_multi_args("spmm_csr_multi", idx_dtype, val_dtype, m, k, n, nnz,
                                           row_ptr, col_idx, values, b, ldb, aggr_mask, eps, c, ldc,
                                           slice_stride, arg_max, arg_min, ldarg, row_begin,
                                           row_end, &nothing);
    if (rc || nothing) return rc;
    const MultiArgs a{static_cast<hipStream_t>(stream), row_ptr, col_idx, values, b, c, arg_max,
                      arg_min, ldb, ldc, slice_stride, ldarg, m, row_begin, row_end - row_begin, n,
                      nnz, b ? k : 0, aggr_mask, eps, workspace, workspace_bytes, opts};
    return by_types(idx_dtype, val_dtype, [&](auto* tp, auto* ip) -> int {
      return multi_typed<std::remove_pointer_t<decltype(tp)>,
                         std::remove_pointer_t<decltype(ip)>>(a);
    });
  });
}
