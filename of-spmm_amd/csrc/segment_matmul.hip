// segment_matmul.hip — the segment matmul (op "segment_matmul"), gfx950, on matrix instructions:
//   out[i, :] = x[row(i), :] @ W[t]   for seg_ptr[t] <= i < seg_ptr[t+1],  row(i) = idx ? idx[i] : i
// the typed linear transform of RGCN / HGT / HeteroLinear layers (PyG's segment_matmul, DGL's
// segment_mm and, with idx, gather_mm over sorted types).  Contract (include/ofx_spmm.h, DESIGN.md
// §3s): f32 products and f32 sums in the hardware's order, one rounding to T.
//
// A block owns kBM = 128 consecutive output rows and kBN = 128 output columns and walks the
// segments that meet its rows (usually one; over the grid at most ceil(S / kBM) + T passes), so the
// grid is ceil(S / kBM) x ceil(F_out / kBN) whatever seg_ptr holds and nothing is read back.  Per
// segment it walks F_in in slabs of BK (64 of bf16 / f16, 32 of f32): the W[t] slab (BK x kBN) is
// staged in LDS in the operand layout of segment_matmul_dev.h (transposed on the way in; with
// trans_w the stored rows already run along k and are copied), while each lane loads the 64 bytes
// of its gathered x row that it feeds the MFMAs with straight from global memory (four 16-byte
// loads, issued before the staging so that they fly under it; scalar loads on an unaligned row or
// a tail).  Rows of another segment and rows whose idx is outside [0, R) are zero rows and load
// nothing.  W is the MFMA's first operand and x the second: a lane then holds four consecutive
// columns of its own output row per register group, stored as one 8- or 16-byte store.
// No atomics, no workspace, no host synchronisation: capturable in a graph.
#include <hip/hip_runtime.h>

#include "segment_matmul.h"
#include "segment_matmul_dev.h"

namespace ofx {
namespace {

using namespace segmm;

template <typename T, typename I, bool TRANS>
__global__ void __launch_bounds__(kThreads)
    segment_matmul_kernel(const T* __restrict__ x, int64_t ldx, int64_t r, const T* __restrict__ w,
                          const I* __restrict__ seg_ptr, const I* __restrict__ idx,
                          T* __restrict__ out, int64_t ldo, int64_t s, int64_t t_count,
                          int64_t f_in, int64_t f_out, bool xvec, bool wvec, bool ovec) {
  constexpr int VEC = 16 / sizeof(T), BK = kSlabBytes / sizeof(T);
  __shared__ __attribute__((aligned(16))) char lds[kBN * kRowStride];
  const int lane = threadIdx.x & 63, l32 = lane & 31, h = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t tile0 = (int64_t)blockIdx.x * kBM;
  const int64_t tile_end = tile0 + kBM < s ? tile0 + kBM : s;
  const int64_t j0 = (int64_t)blockIdx.y * kBN;
  const int ncols = f_out - j0 < kBN ? (int)(f_out - j0) : kBN;
  const int64_t wave0 = tile0 + wave * 32;
  const int64_t my = wave0 + l32;  // this lane's output row
  const T* xrow = nullptr;
  if (my < tile_end) {
    const int64_t src = idx != nullptr ? (int64_t)idx[my] : my;
    if ((uint64_t)src < (uint64_t)r) xrow = x + src * ldx;
  }
  for (int64_t t = first_segment_after(seg_ptr, t_count, s, tile0); t < t_count; ++t) {
    const int64_t sb = bound(seg_ptr, t, s), se = bound(seg_ptr, t + 1, s);
    if (sb >= tile_end) break;
    const int64_t a = sb > tile0 ? sb : tile0, e = se < tile_end ? se : tile_end;
    if (a >= e) continue;
    const bool mine = my >= a && my < e;
    const bool wave_on = wave0 < e && wave0 + 32 > a;  // wave-uniform
    const T* wt = w + t * f_in * f_out;
    f32x16 acc[4];
#pragma unroll
    for (int ct = 0; ct < 4; ++ct)
#pragma unroll
      for (int v = 0; v < 16; ++v) acc[ct][v] = 0.f;
    for (int64_t k0 = 0; k0 < f_in; k0 += BK) {
      uint4 xf[4];
      const T* xp = mine && xrow != nullptr ? xrow + k0 : nullptr;
#pragma unroll
      for (int c = 0; c < 4; ++c) xf[c] = load_chunk<T>(xp, (h * 4 + c) * VEC, f_in - k0, xvec);
      __syncthreads();  // the previous slab has been read
      if constexpr (TRANS) {
        stage_rows<T, kBN>(
            lds, [&](int j) { return j < ncols ? wt + (j0 + j) * f_in + k0 : nullptr; },
            f_in - k0, wvec);
      } else {
        stage_transposed<T, kBN>(
            lds, [&](int k) { return k0 + k < f_in ? wt + (k0 + k) * f_out + j0 : nullptr; },
            ncols, wvec);
      }
      __syncthreads();
      if (wave_on) {
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) {
          if (ct * 32 >= ncols) break;
#pragma unroll
          for (int c = 0; c < 4; ++c)
            mma_chunk<T>(acc[ct], read_fragment(lds, ct * 32 + l32, h, c), xf[c]);
        }
      }
    }
    if (!mine) continue;
    T* orow = out + my * ldo;
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int64_t col = j0 + ct * 32 + g * 8 + h * 4;
        if (col >= f_out) continue;
        T o[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) o[u] = Num<T>::store(acc[ct][g * 4 + u]);
        if (ovec && col + 4 <= f_out) {
          if constexpr (sizeof(T) == 2)
            *reinterpret_cast<uint2*>(orow + col) = __builtin_bit_cast(uint2, o);
          else
            *reinterpret_cast<uint4*>(orow + col) = __builtin_bit_cast(uint4, o);
        } else {
#pragma unroll
          for (int u = 0; u < 4; ++u)
            if (col + u < f_out) orow[col + u] = o[u];
        }
      }
    }
  }
}

template <typename T, typename I>
int launch_forward(hipStream_t stream, const Args& a, const void* w, int trans_w, void* out,
                   int64_t ldo) {
  const int64_t es = (int64_t)sizeof(T);
  const dim3 grid((unsigned)ceil_div(a.s, kBM), (unsigned)ceil_div(a.f_out, kBN));
  const bool xvec = aligned16(a.x, a.ldx * es), ovec = aligned16(out, ldo * es);
  const bool wvec = aligned16(w, (trans_w ? a.f_in : a.f_out) * es);
  const auto go = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, grid, dim3(kThreads), 0, stream, static_cast<const T*>(a.x), a.ldx,
                       a.r, static_cast<const T*>(w), static_cast<const I*>(a.seg_ptr),
                       static_cast<const I*>(a.idx), static_cast<T*>(out), ldo, a.s, a.t, a.f_in,
                       a.f_out, xvec, wvec, ovec);
  };
  if (trans_w)
    go(segment_matmul_kernel<T, I, true>);
  else
    go(segment_matmul_kernel<T, I, false>);
  OFX_HIP_CHECK(hipGetLastError());
  return OFX_OK;
}

}  // namespace
}  // namespace ofx

using namespace ofx;

extern "C" int ofx_segment_matmul_tiles(int val_dtype, int64_t* bm, int64_t* bn, int64_t* bk) {
  return ::ofx::guarded(__func__, [&]() -> int {
    OFX_REQUIRE(bm != nullptr && bn != nullptr && bk != nullptr, OFX_EINVAL,
                "segment_matmul_tiles: NULL output");
    OFX_REQUIRE(val_dtype == OFX_DT_FLOAT || val_dtype == OFX_DT_FLOAT16 ||
                    val_dtype == OFX_DT_BFLOAT16,
                OFX_EUNSUPPORTED, "segment_matmul_tiles: value dtype %d is not "
                "float/float16/bfloat16", val_dtype);
    *bm = segmm::kBM;
    *bn = segmm::kBN;
    *bk = segmm::slab_elems(dtype_size(val_dtype));
    return OFX_OK;
  });
}

extern "C" int ofx_segment_matmul_workspace_size(int idx_dtype, int val_dtype, int64_t r, int64_t s,
                                                 int64_t t, int64_t f_in, int64_t f_out,
                                                 size_t* bytes) {
  return ::ofx::guarded(__func__, [&]() -> int {
    OFX_REQUIRE(bytes != nullptr, OFX_EINVAL, "segment_matmul_workspace_size: bytes is NULL");
    if (const int rc = segmm::check_sizes("segment_matmul_workspace_size", idx_dtype, val_dtype, r,
                                          s, t, f_in, f_out))
      return rc;
    *bytes = 0;
    return OFX_OK;
  });
}

extern "C" int ofx_segment_matmul(void* stream, int idx_dtype, int val_dtype, int64_t r, int64_t s,
                                  int64_t t, int64_t f_in, int64_t f_out, const void* x,
                                  int64_t ldx, const void* w, int trans_w, const void* seg_ptr,
                                  const void* idx, void* out, int64_t ldo, void* workspace,
                                  size_t workspace_bytes) {
  return ::ofx::guarded(__func__, [&]() -> int {
    OFX_TAKE_DEVICE_ERROR("segment_matmul");
    (void)workspace, (void)workspace_bytes;
    const segmm::Args a{idx_dtype, val_dtype, r, s, t, f_in, f_out, x, ldx, seg_ptr, idx};
    if (const int rc = segmm::check_forward("segment_matmul", a, w, out, ldo)) return rc;
    OFX_REQUIRE(segmm::ceil_div(f_out, segmm::kBN) <= 65535, OFX_EINVAL,
                "segment_matmul: f_out=%lld is beyond the launch grid", (long long)f_out);
    if (s == 0) return OFX_OK;
    return by_types(idx_dtype, val_dtype, [&](auto* tp, auto* ip) -> int {
      using T = std::remove_pointer_t<decltype(tp)>;
      using I = std::remove_pointer_t<decltype(ip)>;
      if constexpr (std::is_same<T, double>::value)
        return OFX_EUNSUPPORTED;  // refused by check_sizes
      else
        return launch_forward<T, I>(static_cast<hipStream_t>(stream), a, w, trans_w, out, ldo);
    });
  });
}
