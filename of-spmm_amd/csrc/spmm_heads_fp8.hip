// spmm_heads_fp8.hip — the multi-head CSR x dense SpMM over an FP8 feature table (op
// "spmm_csr_heads_fp8"), gfx950:
//   out[r, h*D + c] = sum over the row's nonzeros j of V'[j, h] * dequant(b_q[col[j], h*D + c])
// with V'[j, h] = values[j, h] * b_scale[col[j]] rounded to T (b_scale absent: V' = values), b_q
// one byte per element in OCP e4m3fn or e5m2.  Contract (include/ofx_spmm.h): the
// bits of ofx_spmm_csr_heads in type T on (row_ptr, col_idx, V', Bd), Bd the exact dequantisation
// of b_q in T -- multiply rounded to T, add in f32, nonzeros ascending, the hub rule of
// resolve_schedule(D, opts), one rounding to T.
//
// Layout of spmm_heads_kernel (spmm_heads.hip): a group of LPR lanes per work item (a row or a hub
// chunk from the shared planner), col loaded LPR at a time and broadcast, U B-row loads in flight
// before the multiply-add chain, non-temporal stores, wider rows loop over column tiles.  What is
// new is the row: a lane owns CPL = 16 consecutive columns, one 16-byte piece of the FP8 row (an
// N = 128 row is 8 lanes and one 128-byte line), converted four bytes at a time by the packed
// FP8 -> f32 instructions.  The scale is loaded beside the col batch, one per nonzero, and
// broadcast with it; the next batch's col and scale are fetched while this one is accumulated.
// The general path (odd D, D % 16 != 0, unaligned rows, k == 0) owns 4 columns per lane, every
// element with its own head index and byte loads.  Hub chunks write f32 partials, hub_sum_kernel
// adds them.  No atomics, no LDS, no allocation, no host synchronisation.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include "heads_steps.h"  // Int<>
#include "spmm_heads_fp8.h"
#include "spmm_items_dev.h"

namespace ofx {
namespace {

using namespace item;

constexpr int kFastCols = 16;  // columns per lane of the fast path: one 16-byte load
constexpr int kSlowCols = 4;   // of the general path

// Bytes 2*hi and 2*hi + 1 of `word` as f32 (v_cvt_pk_f32_fp8 / _bf8 with the word select).
template <int FMT, bool HI>
__device__ __forceinline__ void cvt_pair(unsigned word, float& x, float& y) {
  if constexpr (FMT == OFX_FP8_E4M3) {
    const auto p = __builtin_amdgcn_cvt_pk_f32_fp8((int)word, HI);
    x = p[0];
    y = p[1];
  } else {
    const auto p = __builtin_amdgcn_cvt_pk_f32_bf8((int)word, HI);
    x = p[0];
    y = p[1];
  }
}

template <int FMT>
__device__ __forceinline__ float cvt_one(uint8_t code) {
  float x, y;
  cvt_pair<FMT, false>((unsigned)code, x, y);
  return x;
}

// The scale of column c: +0 outside [0, kb), without a read.
__device__ __forceinline__ float scale_of(const float* __restrict__ scale, int64_t c, int64_t kb) {
  const bool in = (uint64_t)c < (uint64_t)kb;
  const float s = scale[in ? c : 0];
  return in ? s : 0.0f;
}

// acc[e] += mul(V'[j, head of column cb + e], Bd[col[j], cb + e]) over nonzeros [j0, j1),
// ascending, for the lane's 16 columns [cb, cb + 16) of the n = H*D wide row, all of head `hd`.
// Multiply rounded to T, add in f32.  16-byte-aligned rows, D % 16 == 0 and kb > 0.
template <typename T, typename I, int FMT, int LPR, int U, bool SCALED>
__device__ __forceinline__ void fp8_accumulate_fast(
    const I* __restrict__ col, const T* val, const uint8_t* __restrict__ B, int64_t ldb,
    const float* __restrict__ scale, int64_t kb, int64_t n, int64_t heads, int64_t cb, int64_t hd,
    int64_t j0, int64_t j1, int gl, int gbase, float (&acc)[kFastCols]) {
#pragma clang fp contract(off)
  // the first batch's columns and scales; each later batch's are fetched a batch ahead
  I myc = j0 + gl < j1 ? col[j0 + gl] : I(0);
  float mys = 0.0f;
  if constexpr (SCALED) mys = scale_of(scale, (int64_t)myc, kb);
  for (int64_t jb = j0; jb < j1; jb += LPR) {
    const int cnt = (int)((j1 - jb) < LPR ? (j1 - jb) : LPR);
    const I nextc = jb + LPR + gl < j1 ? col[jb + LPR + gl] : I(0);
    for (int k = 0; k < cnt; k += U) {
      // Every load of the round is unconditional (kb > 0 here): a slot past the batch's end
      // repeats the batch's last nonzero, a column outside [0, k) reads row 0 and is replaced by
      // zeros (code 0 is +0 in both formats), a lane past the row's width reads column 0.
      u32x4 raw[U];
      T vv[U];
      float ss[U];
      unsigned inmask = 0;
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int ku = k + u < cnt ? k + u : cnt - 1;
        const int src = gbase + (ku & (LPR - 1));
        const int64_t cu = (int64_t)__shfl((int64_t)myc, src, 64);
        const bool in = (uint64_t)cu < (uint64_t)kb;
        inmask |= (in ? 1u : 0u) << u;
        raw[u] = *reinterpret_cast<const u32x4*>(B + (in ? cu : 0) * ldb + (cb < n ? cb : 0));
        vv[u] = val[(jb + ku) * heads + hd];
        if constexpr (SCALED) ss[u] = __shfl(mys, src, 64);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const u32x4 r = ((inmask >> u) & 1u) ? raw[u] : u32x4{0u, 0u, 0u, 0u};
        if (k + u < cnt) {
          float v = Num<T>::load(vv[u]);
          if constexpr (SCALED) v = fp8::scaled_value<T>(v, ss[u]);
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            float b[4];
            cvt_pair<FMT, false>(r[q], b[0], b[1]);
            cvt_pair<FMT, true>(r[q], b[2], b[3]);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[4 * q + e] = acc[4 * q + e] + Num<T>::mul(v, b[e]);
          }
        }
      }
    }
    myc = nextc;
    if constexpr (SCALED) mys = scale_of(scale, (int64_t)myc, kb);
  }
}

// The same for the lane's 4 columns [cb, cb + 4), each with its own head hd[e]; byte loads, any
// alignment, any D, kb == 0 included; scale == NULL: V' = values.
template <typename T, typename I, int FMT, int LPR, int U>
__device__ __forceinline__ void fp8_accumulate_general(
    const I* __restrict__ col, const T* val, const uint8_t* __restrict__ B, int64_t ldb,
    const float* __restrict__ scale, int64_t kb, int64_t n, int64_t heads, int64_t cb,
    const int64_t (&hd)[kSlowCols], int64_t j0, int64_t j1, int gl, int gbase,
    float (&acc)[kSlowCols]) {
#pragma clang fp contract(off)
  for (int64_t jb = j0; jb < j1; jb += LPR) {
    const int cnt = (int)((j1 - jb) < LPR ? (j1 - jb) : LPR);
    const I myc = gl < cnt ? col[jb + gl] : I(0);
    float mys = 0.0f;
    if (scale != nullptr && (uint64_t)(int64_t)myc < (uint64_t)kb) mys = scale[(int64_t)myc];
    for (int k = 0; k < cnt; k += U) {
      uint8_t bv[U][kSlowCols];
      T vv[U][kSlowCols];
      float ss[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int src = gbase + ((k + u) & (LPR - 1));
        const int64_t cu = (int64_t)__shfl((int64_t)myc, src, 64);
        ss[u] = __shfl(mys, src, 64);
        if (k + u < cnt) {
          // a column outside [0, k): the zero-filled gathered row; its address is never used
          const bool in = (uint64_t)cu < (uint64_t)kb;
          const uint8_t* brow = B + (in ? cu : 0) * ldb;
          const T* vrow = val + (jb + k + u) * heads;
#pragma unroll
          for (int e = 0; e < kSlowCols; ++e) {
            bv[u][e] = (in && cb + e < n) ? brow[cb + e] : (uint8_t)0;
            vv[u][e] = vrow[hd[e]];
          }
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (k + u < cnt) {
#pragma unroll
          for (int e = 0; e < kSlowCols; ++e) {
            float v = Num<T>::load(vv[u][e]);
            if (scale != nullptr) v = fp8::scaled_value<T>(v, ss[u]);
            acc[e] = acc[e] + Num<T>::mul(v, cvt_one<FMT>(bv[u][e]));
          }
        }
      }
    }
  }
}

// FAST: aligned rows, D % 16 == 0 and kb > 0 (one head per lane); SCALED is read by it alone.
template <typename T, typename I, int FMT, int LPR, int U, bool FAST, bool SCALED>
__global__ void __launch_bounds__(kBlock)
    spmm_heads_fp8_kernel(const I* __restrict__ rp, const I* __restrict__ col,
                          const T* __restrict__ val, const uint8_t* __restrict__ B, int64_t ldb,
                          const float* __restrict__ scale, int64_t kb, T* __restrict__ out,
                          int64_t ldc, int64_t row_begin, int64_t nrows, int64_t n, int64_t heads,
                          int64_t d, int64_t chunk,
                          const unsigned long long* __restrict__ counters,
                          const int64_t* __restrict__ items, const int64_t* __restrict__ order,
                          float* __restrict__ part, int64_t block_base, unsigned* err) {
#pragma clang fp contract(off)
  constexpr int CPL = FAST ? kFastCols : kSlowCols;
  constexpr int GPW = 64 / LPR;
  if (poison_rows(counters, block_base, err, out, ldc, (I*)nullptr, (int64_t)0, nrows, n)) return;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int gl = lane & (LPR - 1);
  const int gbase = lane & ~(LPR - 1);
  const int64_t g = ((block_base + (int64_t)blockIdx.x) * (kBlock / 64) + wave) * GPW + lane / LPR;
  Item it;
  if (!work_item<I>(rp, g, row_begin, nrows, chunk, counters, items, order, &it)) return;
  for (int64_t c0 = 0; c0 < n; c0 += (int64_t)LPR * CPL) {
    const int64_t cb = c0 + (int64_t)gl * CPL;
    float acc[CPL];
#pragma unroll
    for (int e = 0; e < CPL; ++e) acc[e] = 0.0f;
    if constexpr (FAST) {
      // a lane past the row's width: head 0, its products are never stored
      fp8_accumulate_fast<T, I, FMT, LPR, U, SCALED>(col, val, B, ldb, scale, kb, n, heads, cb,
                                                     cb < n ? cb / d : 0, it.j0, it.j1, gl, gbase,
                                                     acc);
    } else {
      int64_t hd[CPL];
#pragma unroll
      for (int e = 0; e < CPL; ++e) hd[e] = cb + e < n ? (cb + e) / d : 0;
      fp8_accumulate_general<T, I, FMT, LPR, U>(col, val, B, ldb, scale, kb, n, heads, cb, hd,
                                                it.j0, it.j1, gl, gbase, acc);
    }
    if (it.slot >= 0) {  // a hub chunk's partial: added in chunk order by hub_sum_kernel
#pragma unroll
      for (int e = 0; e < CPL; ++e)
        if (cb + e < n) part[it.slot * n + cb + e] = acc[e];
    } else {
      T o[CPL];
#pragma unroll
      for (int e = 0; e < CPL; ++e) o[e] = Num<T>::store(acc[e]);
      store_cols<T, CPL, FAST>(out + it.lr * ldc, cb, n, o);
    }
  }
}

struct Fp8Args {
  hipStream_t s;
  const void *rp, *col, *val, *b, *scale;
  void* c;
  int64_t ldb, ldc, m, row_begin, nrows, heads, d, nnz, k;
  void* ws;
  size_t ws_bytes;
  const ofx_spmm_options* opts;
};

template <typename T, typename I, int FMT, int LPR, bool FAST, bool SCALED>
int fp8_cfg(const Fp8Args& a) {
  constexpr int U = 8;
  constexpr int64_t GPB = (kBlock / 64) * (64 / LPR);
  const int64_t n = a.heads * a.d;
  Planned p;
  // the schedule: the sum op's, resolved from the width of ONE head (the numeric contract)
  int rc = prepare_plan<I>("spmm_csr_heads_fp8", a.s, static_cast<const I*>(a.rp), a.row_begin,
                           a.nrows, a.nnz, launch_nnz(a.m, a.nrows, a.nnz, a.opts), n,
                           sizeof(float), resolve_schedule(a.d, a.opts), false, a.ws, a.ws_bytes,
                           &p);
  if (rc) return rc;
  float* part = static_cast<float*>(p.wl.part);
  rc = launch_cut_grid(p.work, GPB, [&](dim3 grid, int64_t b0) {
    hipLaunchKernelGGL((spmm_heads_fp8_kernel<T, I, FMT, LPR, U, FAST, SCALED>), grid,
                       dim3(kBlock), 0, a.s, static_cast<const I*>(a.rp),
                       static_cast<const I*>(a.col), static_cast<const T*>(a.val),
                       static_cast<const uint8_t*>(a.b), a.ldb,
                       static_cast<const float*>(a.scale), a.k, static_cast<T*>(a.c), a.ldc,
                       a.row_begin, a.nrows, n, a.heads, a.d, p.chunk, p.wl.counters, p.wl.items,
                       p.wl.order, part, b0, p.err);
  });
  if (rc) return rc;
  return launch_hub_sum(a.s, p, static_cast<T*>(a.c), a.ldc, a.nrows, n);
}

// The fast path's lane ladder: by_lane_group's steps and one of 8 lanes (N = 128 at 16 columns
// per lane); a wider row loops over tiles of 64 lanes.
template <typename F>
int by_fast_lanes(int64_t lanes, F&& f) {
  using hsteps::Int;
  if (lanes <= 1) return f(Int<1>{});
  if (lanes <= 4) return f(Int<4>{});
  if (lanes <= 8) return f(Int<8>{});
  if (lanes <= 16) return f(Int<16>{});
  if (lanes <= 32) return f(Int<32>{});
  return f(Int<64>{});
}

template <typename F>
int by_general_lanes(int64_t lanes, F&& f) {
  using hsteps::Int;
  if (lanes <= 1) return f(Int<1>{});
  if (lanes <= 4) return f(Int<4>{});
  if (lanes <= 16) return f(Int<16>{});
  return f(Int<64>{});
}

template <typename T, typename I, int FMT>
int fp8_typed(const Fp8Args& a) {
  const int64_t n = a.heads * a.d;
  // k == 0 (every column out of range, b_q may be empty) takes the general path: the fast one
  // loads unconditionally and needs a row 0 to read
  const bool fast = a.d % kFastCols == 0 && a.k > 0 && rows_aligned(a.b, a.ldb, 1, kFastCols) &&
                    rows_aligned(a.c, a.ldc, sizeof(T), kFastCols);
  if (!fast)
    return by_general_lanes((n + kSlowCols - 1) / kSlowCols, [&](auto lpr) -> int {
      return fp8_cfg<T, I, FMT, decltype(lpr)::value, false, false>(a);
    });
  return by_fast_lanes(n / kFastCols, [&](auto lpr) -> int {
    constexpr int LPR = decltype(lpr)::value;
    return a.scale != nullptr ? fp8_cfg<T, I, FMT, LPR, true, true>(a)
                              : fp8_cfg<T, I, FMT, LPR, true, false>(a);
  });
}

size_t fp8_ws_bytes(int64_t nrows, int64_t nnz, int64_t n, int64_t d,
                    const ofx_spmm_options* opts) {
  return plan::ws_layout(nrows, nnz, n, 4, resolve_schedule(d, opts)).total;
}

}  // namespace
}  // namespace ofx

using namespace ofx;

extern "C" int ofx_spmm_csr_heads_fp8_workspace_size(int idx_dtype, int val_dtype, int b_format,
                                                     int64_t m, int64_t k, int64_t heads,
                                                     int64_t d, int64_t nnz,
                                                     const ofx_spmm_options* opts,
                                                     size_t* bytes) {
  return ::ofx::guarded(__func__, [&]() -> int {
    OFX_REQUIRE(bytes != nullptr, OFX_EINVAL, "spmm_csr_heads_fp8_workspace_size: bytes is NULL");
    OFX_READ_OPTIONS(opts, "spmm_csr_heads_fp8_workspace_size");
    if (const int rc = fp8::check_fp8_args("spmm_csr_heads_fp8_workspace_size", idx_dtype,
                                           val_dtype, b_format, m, k, heads, d, nnz, opts))
      return rc;
    *bytes = fp8_ws_bytes(m, nnz, heads * d, d, opts);
    return OFX_OK;
  });
}

extern "C" int ofx_spmm_csr_heads_fp8(void* stream, int idx_dtype, int val_dtype, int b_format,
                                      int64_t m, int64_t k, int64_t heads, int64_t d, int64_t nnz,
                                      const void* row_ptr, const void* col_idx, const void* values,
                                      const void* b_q, int64_t ldb, const void* b_scale, void* c,
                                      int64_t ldc, int64_t row_begin, int64_t row_end,
                                      void* workspace, size_t workspace_bytes,
                                      const ofx_spmm_options* opts) {
  return ::ofx::guarded(__func__, [&]() -> int {
    OFX_TAKE_DEVICE_ERROR("spmm_csr_heads_fp8");  // an earlier launch's loud failure
    OFX_READ_OPTIONS(opts, "spmm_csr_heads_fp8");
    int rc = fp8::check_fp8_args("spmm_csr_heads_fp8", idx_dtype, val_dtype, b_format, m, k, heads,
                                 d, nnz, opts);
    if (rc) return rc;
    if ((rc = check_row_range("spmm_csr_heads_fp8", row_begin, row_end, m))) return rc;
    const int64_t n = heads * d;
    OFX_REQUIRE(ldb >= n && ldc >= n, OFX_EINVAL, "spmm_csr_heads_fp8: ldb=%lld / ldc=%lld < n=%lld",
                (long long)ldb, (long long)ldc, (long long)n);
    const int64_t nrows = row_end - row_begin;
    if (nrows == 0 || n == 0) return OFX_OK;  // nothing to write
    OFX_REQUIRE(row_ptr && c, OFX_EINVAL, "spmm_csr_heads_fp8: NULL row_ptr or output");
    OFX_REQUIRE(nnz == 0 || (col_idx && values && (b_q || k == 0)), OFX_EINVAL,
                "spmm_csr_heads_fp8: NULL col_idx/values/b_q with nnz=%lld", (long long)nnz);
    const size_t need = fp8_ws_bytes(nrows, nnz, n, d, opts);
    if ((rc = check_workspace("spmm_csr_heads_fp8", workspace, workspace_bytes, need))) return rc;
    const Fp8Args a{static_cast<hipStream_t>(stream), row_ptr, col_idx, values, b_q, b_scale, c,
                    ldb, ldc, m, row_begin, nrows, heads, d, nnz, b_q ? k : 0, workspace,
                    workspace_bytes, opts};
    return fp8::by_types(idx_dtype, val_dtype, [&](auto* tp, auto* ip) -> int {
      using T = std::remove_pointer_t<decltype(tp)>;
      using I = std::remove_pointer_t<decltype(ip)>;
      return b_format == OFX_FP8_E4M3 ? fp8_typed<T, I, OFX_FP8_E4M3>(a)
                                      : fp8_typed<T, I, OFX_FP8_E5M2>(a);
    });
  });
}
