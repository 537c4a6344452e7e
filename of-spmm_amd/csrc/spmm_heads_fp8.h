// spmm_heads_fp8.h — what the HIP kernel (spmm_heads_fp8.hip) and the kCPU kernel
// (spmm_heads_fp8_cpu.cpp) of op "spmm_csr_heads_fp8" share: the decoding of the two OCP FP8
// formats in plain C++, the scaled value V' and the argument checks of the C-ABI entries
// (contract in include/ofx_spmm.h).
#ifndef OFX_SPMM_HEADS_FP8_H_
#define OFX_SPMM_HEADS_FP8_H_

#include <climits>
#include <cstdint>

#include "gatv2_scores.h"  // gv2::rounded: a rounding to T the device compiler cannot fold
#include "ofx_internal.h"
#include "spmm_common.h"

namespace ofx {
namespace fp8 {

// The value of code `c` of format `fmt` (OFX_FP8_E4M3: 1-4-3, bias 7, no infinity, S.1111.111 is
// NaN; OFX_FP8_E5M2: 1-5-2, bias 15, IEEE infinities and NaNs).  Every finite value is exact in
// f32, f16 and bf16.
OFX_HD float decode(int fmt, uint32_t c) {
  const int mbits = fmt == OFX_FP8_E4M3 ? 3 : 2;
  const int bias = fmt == OFX_FP8_E4M3 ? 7 : 15;
  const uint32_t sign = (c >> 7) & 1u;
  const uint32_t e = (c & 0x7fu) >> mbits;
  const uint32_t m = c & ((1u << mbits) - 1u);
  const uint32_t emax = fmt == OFX_FP8_E4M3 ? 15u : 31u;
  uint32_t bits;
  if (fmt == OFX_FP8_E4M3 ? (e == emax && m == 7u) : (e == emax && m != 0u)) {
    bits = 0x7fc00000u;
  } else if (fmt == OFX_FP8_E5M2 && e == emax) {
    bits = 0x7f800000u;
  } else if (e == 0) {
    // subnormal: m * 2^(1 - bias - mbits), an exact f32 product (m < 8 times a power of two)
    const float v = float(m) * bits_to_f32(uint32_t(127 + 1 - bias - mbits) << 23);
    bits = f32_to_bits(v);
  } else {
    bits = ((e + 127u - (uint32_t)bias) << 23) | (m << (23 - mbits));
  }
  return bits_to_f32(bits | (sign << 31));
}

// V'[j, h]: the value times the scale of its column, one product in the accumulation type and one
// rounding to T as a step of its own.
template <typename T>
OFX_HD typename Num<T>::acc scaled_value(typename Num<T>::acc v, float s) {
#pragma clang fp contract(off)
  return gv2::rounded<T>(v * s);
}

static inline int check_format(const char* fn, int b_format) {
  OFX_REQUIRE(b_format == OFX_FP8_E4M3 || b_format == OFX_FP8_E5M2, OFX_EINVAL,
              "%s: unknown FP8 format code %d (OFX_FP8_E4M3 / OFX_FP8_E5M2)", fn, b_format);
  return OFX_OK;
}

// What the three entries refuse ahead of their own pointer and workspace checks.
static inline int check_fp8_args(const char* fn, int idx_dtype, int val_dtype, int b_format,
                                 int64_t m, int64_t k, int64_t heads, int64_t d, int64_t nnz,
                                 const ofx_spmm_options* opts) {
  if (const int rc = check_heads_shape(fn, heads, d)) return rc;
  if (const int rc = check_types_sizes(fn, idx_dtype, val_dtype, m, k, heads * d, nnz)) return rc;
  OFX_REQUIRE(val_dtype != OFX_DT_DOUBLE, OFX_EUNSUPPORTED,
              "%s: value dtype double is not supported (float, float16, bfloat16)", fn);
  if (const int rc = check_format(fn, b_format)) return rc;
  return check_no_plan_options(fn, opts);
}

// Dispatch over the three value types of the op (f64 is refused before it).
template <typename F>
int by_types(int idx_dtype, int val_dtype, F&& f) {
  return by_index(idx_dtype, [&](auto* ip) -> int {
    if (val_dtype == OFX_DT_FLOAT) return f((float*)nullptr, ip);
    if (val_dtype == OFX_DT_BFLOAT16) return f((bf16*)nullptr, ip);
    return f((f16*)nullptr, ip);
  });
}

}  // namespace fp8
}  // namespace ofx

#endif  // OFX_SPMM_HEADS_FP8_H_
