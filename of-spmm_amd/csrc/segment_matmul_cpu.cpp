// segment_matmul_cpu.cpp — the DeviceType::kCPU kernels of ops "segment_matmul" and
// "segment_matmul_grad_w" (contract in include/ofx_spmm.h): plain loops, every
// product formed in f32 (no FMA) and added in f32 in ascending k (forward) or ascending row i
// (w-gradient), one rounding to T.  The forward runs in OpenMP over the output rows, the
// w-gradient over (segment, row of dw[t]); a sum is one thread's, so the bits do not depend on the
// thread count.  Beyond the device entries' checks, seg_ptr is checked here: it starts at 0, does
// not decrease and ends at S.
#pragma clang fp contract(off)

#include <omp.h>

#include <vector>

#include "ofx_internal.h"
#include "segment_matmul.h"
#include "spmm_common.h"

using namespace ofx;

namespace {

template <typename I>
int check_seg_ptr(const char* fn, const I* seg_ptr, int64_t t, int64_t s) {
  OFX_REQUIRE((int64_t)seg_ptr[0] == 0, OFX_EINVAL, "%s: seg_ptr[0] = %lld, not 0", fn,
              (long long)seg_ptr[0]);
  for (int64_t i = 0; i < t; ++i)
    OFX_REQUIRE(seg_ptr[i] <= seg_ptr[i + 1], OFX_EINVAL,
                "%s: seg_ptr is decreasing at segment %lld (%lld > %lld)", fn, (long long)i,
                (long long)seg_ptr[i], (long long)seg_ptr[i + 1]);
  OFX_REQUIRE((int64_t)seg_ptr[t] == s, OFX_EINVAL,
              "%s: seg_ptr[T] = %lld does not equal the %lld output rows", fn,
              (long long)seg_ptr[t], (long long)s);
  return OFX_OK;
}

// The source row of output row i, or NULL (idx[i] outside [0, r): a zero row).
template <typename T, typename I>
const T* source_row(const T* x, int64_t ldx, int64_t r, const I* idx, int64_t i) {
  const int64_t src = idx != nullptr ? (int64_t)idx[i] : i;
  return (uint64_t)src < (uint64_t)r ? x + src * ldx : nullptr;
}

template <typename T, typename I>
void forward_rows(int nthreads, const segmm::Args& a, const T* w, bool trans_w, T* out,
                  int64_t ldo) {
#pragma clang fp contract(off)
  const T* x = static_cast<const T*>(a.x);
  const I *seg_ptr = static_cast<const I*>(a.seg_ptr), *idx = static_cast<const I*>(a.idx);
  const int64_t f_in = a.f_in, f_out = a.f_out;
#pragma omp parallel num_threads(nthreads)
  {
    std::vector<float> acc(f_out);
#pragma omp for schedule(static)
    for (int64_t i = 0; i < a.s; ++i) {
      const int64_t t = segmm::first_segment_after(seg_ptr, a.t, a.s, i);
      const T* wt = w + t * f_in * f_out;
      const T* xr = source_row(x, a.ldx, a.r, idx, i);
      for (int64_t j = 0; j < f_out; ++j) acc[j] = 0.f;
      if (trans_w) {
        for (int64_t j = 0; j < f_out; ++j)
          for (int64_t k = 0; k < f_in; ++k)
            acc[j] = acc[j] + (xr ? Num<T>::load(xr[k]) : 0.f) * Num<T>::load(wt[j * f_in + k]);
      } else {
        for (int64_t k = 0; k < f_in; ++k) {
          const float xk = xr ? Num<T>::load(xr[k]) : 0.f;
          for (int64_t j = 0; j < f_out; ++j) acc[j] = acc[j] + xk * Num<T>::load(wt[k * f_out + j]);
        }
      }
      for (int64_t j = 0; j < f_out; ++j) out[i * ldo + j] = Num<T>::store(acc[j]);
    }
  }
}

template <typename T, typename I>
void grad_w_rows(int nthreads, const segmm::Args& a, const T* dy, int64_t lddy, T* dw) {
#pragma clang fp contract(off)
  const T* x = static_cast<const T*>(a.x);
  const I *seg_ptr = static_cast<const I*>(a.seg_ptr), *idx = static_cast<const I*>(a.idx);
  const int64_t f_in = a.f_in, f_out = a.f_out;
#pragma omp parallel num_threads(nthreads)
  {
    std::vector<float> acc(f_out);
#pragma omp for schedule(dynamic, 4)
    for (int64_t ta = 0; ta < a.t * f_in; ++ta) {
      const int64_t t = ta / f_in, ka = ta % f_in;
      for (int64_t j = 0; j < f_out; ++j) acc[j] = 0.f;
      for (int64_t i = (int64_t)seg_ptr[t]; i < (int64_t)seg_ptr[t + 1]; ++i) {
        const T* xr = source_row(x, a.ldx, a.r, idx, i);
        const float xa = xr ? Num<T>::load(xr[ka]) : 0.f;
        for (int64_t j = 0; j < f_out; ++j) acc[j] = acc[j] + xa * Num<T>::load(dy[i * lddy + j]);
      }
      for (int64_t j = 0; j < f_out; ++j) dw[ta * f_out + j] = Num<T>::store(acc[j]);
    }
  }
}

}  // namespace

extern "C" int ofx_segment_matmul_cpu(int num_threads, int idx_dtype, int val_dtype, int64_t r,
                                      int64_t s, int64_t t, int64_t f_in, int64_t f_out,
                                      const void* x, int64_t ldx, const void* w, int trans_w,
                                      const void* seg_ptr, const void* idx, void* out,
                                      int64_t ldo) {
  return ::ofx::guarded(__func__, [&]() -> int {
    const segmm::Args a{idx_dtype, val_dtype, r, s, t, f_in, f_out, x, ldx, seg_ptr, idx};
    if (const int rc = segmm::check_forward("segment_matmul_cpu", a, w, out, ldo)) return rc;
    return by_types(idx_dtype, val_dtype, [&](auto* tp, auto* ip) -> int {
      using T = std::remove_pointer_t<decltype(tp)>;
      using I = std::remove_pointer_t<decltype(ip)>;
      if constexpr (std::is_same<T, double>::value) {
        return OFX_EUNSUPPORTED;  // refused by check_sizes
      } else {
        if (const int rc = check_seg_ptr("segment_matmul_cpu", (const I*)seg_ptr, t, s)) return rc;
        forward_rows<T, I>(threads_of(num_threads), a, (const T*)w, trans_w != 0, (T*)out, ldo);
        return OFX_OK;
      }
    });
  });
}

extern "C" int ofx_segment_matmul_grad_w_cpu(int num_threads, int idx_dtype, int val_dtype,
                                             int64_t r, int64_t s, int64_t t, int64_t f_in,
                                             int64_t f_out, const void* x, int64_t ldx,
                                             const void* dy, int64_t lddy, const void* seg_ptr,
                                             const void* idx, void* dw) {
  return ::ofx::guarded(__func__, [&]() -> int {
    const segmm::Args a{idx_dtype, val_dtype, r, s, t, f_in, f_out, x, ldx, seg_ptr, idx};
    if (const int rc = segmm::check_grad_w("segment_matmul_grad_w_cpu", a, dy, lddy, dw, 0))
      return rc;
    return by_types(idx_dtype, val_dtype, [&](auto* tp, auto* ip) -> int {
      using T = std::remove_pointer_t<decltype(tp)>;
      using I = std::remove_pointer_t<decltype(ip)>;
      if constexpr (std::is_same<T, double>::value) {
        return OFX_EUNSUPPORTED;  // refused by check_sizes
      } else {
        if (const int rc = check_seg_ptr("segment_matmul_grad_w_cpu", (const I*)seg_ptr, t, s))
          return rc;
        grad_w_rows<T, I>(threads_of(num_threads), a, (const T*)dy, lddy, (T*)dw);
        return OFX_OK;
      }
    });
  });
}
