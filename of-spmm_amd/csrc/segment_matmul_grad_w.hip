// segment_matmul_grad_w.hip — the w-gradient of the segment matmul (op "segment_matmul_grad_w"),
// gfx950, on matrix instructions:
//   dw[t] = sum over seg_ptr[t] <= i < seg_ptr[t+1] of x[row(i), :]^T dy[i, :]     [F_in, F_out]
// Contract (include/ofx_spmm.h): f32 products and sums, the partial sums of a
// segment added in a fixed order, one rounding to T; no atomics, the same bits on every call.
//
// The rows [0, S) are cut into P contiguous parts (a function of the shapes, or the caller's), and
// a block owns one part and one kBN x kBN tile of dw.  It walks the segments its part meets; for
// each it walks the rows in slabs of BK (64 of bf16 / f16, 32 of f32): the x rows (gathered through
// idx) and the dy rows of the slab are staged in LDS transposed, both in the operand layout of
// segment_matmul_dev.h, and each of the four waves multiplies a 64 x 64 quarter of the tile
// (2 x 2 MFMA tiles) out of LDS.  The f32 tile of (part p, segment t) goes to workspace slot
// p + t: parts and segments are both ascending runs of rows, so the pairs that meet form a
// staircase and the slot is unique; there are at most P + T - 1 of them.  The combine kernel adds
// a segment's tiles in ascending p from +0 and rounds; a segment no part meets (an empty one) gets
// +0.  Nothing is read back: grid and workspace depend on the shapes alone.
#include <hip/hip_runtime.h>

#include "segment_matmul.h"
#include "segment_matmul_dev.h"

namespace ofx {
namespace {

using namespace segmm;

template <typename T, typename I>
__global__ void __launch_bounds__(kThreads)
    segment_matmul_grad_w_kernel(const T* __restrict__ x, int64_t ldx, int64_t r,
                                 const T* __restrict__ dy, int64_t lddy,
                                 const I* __restrict__ seg_ptr, const I* __restrict__ idx,
                                 float* __restrict__ part, int64_t s, int64_t t_count, int64_t f_in,
                                 int64_t f_out, int64_t parts, bool xvec, bool yvec) {
  constexpr int BK = kSlabBytes / sizeof(T);
  __shared__ __attribute__((aligned(16))) char lds[2 * kBN * kRowStride];
  char* xs = lds;
  char* ys = lds + kBN * kRowStride;
  const int lane = threadIdx.x & 63, l32 = lane & 31, h = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int64_t tiles_n = ceil_div(f_out, kBN);
  const int64_t a0 = ((int64_t)blockIdx.x / tiles_n) * kBN, b0 = ((int64_t)blockIdx.x % tiles_n) * kBN;
  const int na = f_in - a0 < kBN ? (int)(f_in - a0) : kBN;
  const int nb = f_out - b0 < kBN ? (int)(f_out - b0) : kBN;
  const int64_t p = blockIdx.y;
  const int64_t rb = part_begin(p, parts, s), re = part_begin(p + 1, parts, s);
  if (rb >= re) return;
  const bool wave_on = wm * 64 < na && wn * 64 < nb;
  for (int64_t t = first_segment_after(seg_ptr, t_count, s, rb); t < t_count; ++t) {
    const int64_t sb = bound(seg_ptr, t, s), se = bound(seg_ptr, t + 1, s);
    if (sb >= re) break;
    const int64_t a = sb > rb ? sb : rb, e = se < re ? se : re;
    if (a >= e) continue;
    f32x16 acc[2][2];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int v = 0; v < 16; ++v) acc[q >> 1][q & 1][v] = 0.f;
    for (int64_t i0 = a; i0 < e; i0 += BK) {
      __syncthreads();  // the previous slab has been read
      stage_transposed<T, kBN>(
          xs,
          [&](int k) -> const T* {
            const int64_t i = i0 + k;
            if (i >= e) return nullptr;
            const int64_t src = idx != nullptr ? (int64_t)idx[i] : i;
            return (uint64_t)src < (uint64_t)r ? x + src * ldx + a0 : nullptr;
          },
          na, xvec);
      stage_transposed<T, kBN>(
          ys, [&](int k) -> const T* { return i0 + k < e ? dy + (i0 + k) * lddy + b0 : nullptr; },
          nb, yvec);
      __syncthreads();
      if (wave_on) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          uint4 xa[2], yb[2];
#pragma unroll
          for (int u = 0; u < 2; ++u) {
            xa[u] = read_fragment(xs, wm * 64 + u * 32 + l32, h, c);
            yb[u] = read_fragment(ys, wn * 64 + u * 32 + l32, h, c);
          }
#pragma unroll
          for (int q = 0; q < 4; ++q) mma_chunk<T>(acc[q >> 1][q & 1], xa[q >> 1], yb[q & 1]);
        }
      }
    }
    // the tile of (p, t): rows a0 + ... of F_in from the register index, column from the lane
    float* tile = part + (p + t) * f_in * f_out;
    const int64_t colq = b0 + wn * 64 + l32;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int64_t col = colq + (q & 1) * 32;
      if (col >= f_out) continue;
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const int64_t row = a0 + wm * 64 + (q >> 1) * 32 + (v >> 2) * 8 + h * 4 + (v & 3);
        if (row < f_in) tile[row * f_out + col] = acc[q >> 1][q & 1][v];
      }
    }
  }
}

// dw[t][e] = the sum over the parts that meet segment t, ascending, of their tiles' element e.
template <typename T, typename I>
__global__ void __launch_bounds__(kThreads)
    segment_matmul_grad_w_combine(const float* __restrict__ part, const I* __restrict__ seg_ptr,
                                  T* __restrict__ dw, int64_t s, int64_t t_count, int64_t ne,
                                  int64_t parts) {
  const int64_t el = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (el >= ne) return;
  for (int64_t t = blockIdx.y; t < t_count; t += gridDim.y) {
    const int64_t sb = bound(seg_ptr, t, s), se = bound(seg_ptr, t + 1, s);
    float sum = 0.f;
    if (sb < se) {
      // the first part that ends after sb; parts follow until one begins at or after se
      int64_t lo = 0, hi = parts;
      while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (part_begin(mid + 1, parts, s) > sb)
          hi = mid;
        else
          lo = mid + 1;
      }
      for (int64_t p = lo; p < parts; ++p) {
        const int64_t rb = part_begin(p, parts, s), re = part_begin(p + 1, parts, s);
        if (rb >= se) break;
        if ((sb > rb ? sb : rb) < (se < re ? se : re)) sum = sum + part[(p + t) * ne + el];
      }
    }
    dw[t * ne + el] = Num<T>::store(sum);
  }
}

template <typename T, typename I>
int launch_grad_w(hipStream_t stream, const Args& a, const void* dy, int64_t lddy, void* dw,
                  int64_t parts, void* workspace) {
  const int64_t es = (int64_t)sizeof(T), ne = a.f_in * a.f_out;
  float* part = static_cast<float*>(workspace);
  if (a.s > 0) {
    const dim3 grid((unsigned)(ceil_div(a.f_in, kBN) * ceil_div(a.f_out, kBN)), (unsigned)parts);
    hipLaunchKernelGGL((segment_matmul_grad_w_kernel<T, I>), grid, dim3(kThreads), 0, stream,
                       static_cast<const T*>(a.x), a.ldx, a.r, static_cast<const T*>(dy), lddy,
                       static_cast<const I*>(a.seg_ptr), static_cast<const I*>(a.idx), part, a.s,
                       a.t, a.f_in, a.f_out, parts, aligned16(a.x, a.ldx * es),
                       aligned16(dy, lddy * es));
    OFX_HIP_CHECK(hipGetLastError());
  }
  const dim3 cgrid((unsigned)ceil_div(ne, kThreads), (unsigned)(a.t < 65535 ? a.t : 65535));
  hipLaunchKernelGGL((segment_matmul_grad_w_combine<T, I>), cgrid, dim3(kThreads), 0, stream, part,
                     static_cast<const I*>(a.seg_ptr), static_cast<T*>(dw), a.s, a.t, ne, parts);
  OFX_HIP_CHECK(hipGetLastError());
  return OFX_OK;
}

size_t grad_w_ws_bytes(int64_t s, int64_t t, int64_t f_in, int64_t f_out, int64_t parts) {
  return (size_t)(grad_w_parts(s, f_in, f_out, parts) + t) * (size_t)f_in * (size_t)f_out *
         sizeof(float);
}

}  // namespace
}  // namespace ofx

using namespace ofx;

extern "C" int ofx_segment_matmul_grad_w_workspace_size(int idx_dtype, int val_dtype, int64_t r,
                                                        int64_t s, int64_t t, int64_t f_in,
                                                        int64_t f_out, int64_t parts,
                                                        size_t* bytes) {
  return ::ofx::guarded(__func__, [&]() -> int {
    const char* fn = "segment_matmul_grad_w_workspace_size";
    OFX_REQUIRE(bytes != nullptr, OFX_EINVAL, "%s: bytes is NULL", fn);
    if (const int rc = segmm::check_sizes(fn, idx_dtype, val_dtype, r, s, t, f_in, f_out)) return rc;
    OFX_REQUIRE(parts >= 0, OFX_EINVAL, "%s: parts=%lld is negative", fn, (long long)parts);
    *bytes = grad_w_ws_bytes(s, t, f_in, f_out, parts);
    return OFX_OK;
  });
}

extern "C" int ofx_segment_matmul_grad_w(void* stream, int idx_dtype, int val_dtype, int64_t r,
                                         int64_t s, int64_t t, int64_t f_in, int64_t f_out,
                                         const void* x, int64_t ldx, const void* dy, int64_t lddy,
                                         const void* seg_ptr, const void* idx, void* dw,
                                         int64_t parts, void* workspace, size_t workspace_bytes) {
  return ::ofx::guarded(__func__, [&]() -> int {
    OFX_TAKE_DEVICE_ERROR("segment_matmul_grad_w");
    const segmm::Args a{idx_dtype, val_dtype, r, s, t, f_in, f_out, x, ldx, seg_ptr, idx};
    if (const int rc = segmm::check_grad_w("segment_matmul_grad_w", a, dy, lddy, dw, parts))
      return rc;
    if (const int rc = check_workspace("segment_matmul_grad_w", workspace, workspace_bytes,
                                       grad_w_ws_bytes(s, t, f_in, f_out, parts)))
      return rc;
    const int64_t p = segmm::grad_w_parts(s, f_in, f_out, parts);
    return by_types(idx_dtype, val_dtype, [&](auto* tp, auto* ip) -> int {
      using T = std::remove_pointer_t<decltype(tp)>;
      using I = std::remove_pointer_t<decltype(ip)>;
      if constexpr (std::is_same<T, double>::value)
        return OFX_EUNSUPPORTED;  // refused by check_sizes
      else
        return launch_grad_w<T, I>(static_cast<hipStream_t>(stream), a, dy, lddy, dw, p,
                                   workspace);
    });
  });
}
