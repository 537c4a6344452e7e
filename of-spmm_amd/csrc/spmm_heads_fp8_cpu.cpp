// spmm_heads_fp8_cpu.cpp — the DeviceType::kCPU kernel of op "spmm_csr_heads_fp8" (multi-head
// SpMM over a CSR with an FP8 feature table and an optional f32 scale per row of it; contract in
// include/ofx_spmm.h).  The sum's row template (spmm_rows_cpu.h) with another
// source of B: the value scaled and rounded to T first (V') and the B element read through a
// 256-entry table of the format's values in T.  The loops are the template's, so the bits are those
// of ofx_spmm_csr_heads_cpu on (V', Bd) by construction, and of the HIP kernel
// (spmm_heads_fp8.hip).
#pragma clang fp contract(off)

#include "ofx_internal.h"
#include "spmm_common.h"
#include "spmm_heads_fp8.h"
#include "spmm_rows_cpu.h"

namespace ofx {
namespace {

// The FP8 source of B (DenseRows of spmm_rows_cpu.h): a column outside [0, k) has scale +0, and
// without a scale there is no multiply.
template <typename T>
struct Fp8Rows {
  using elem = uint8_t;
  const float* scale;
  float lut[256];  // Bd's values: the code's value stored in T (exact) and loaded again
  Fp8Rows(int fmt, const float* scale_) : scale(scale_) {
    for (int c = 0; c < 256; ++c)
      lut[c] = Num<T>::load(Num<T>::store(fp8::decode(fmt, (uint32_t)c)));
  }
  float value(float v, int64_t cj, bool in) const {
    return scale != nullptr ? fp8::scaled_value<T>(v, in ? scale[cj] : 0.0f) : v;
  }
  float at(const uint8_t* brow, int64_t c) const { return lut[brow[c]]; }
};

}  // namespace
}  // namespace ofx

using namespace ofx;

extern "C" int ofx_spmm_csr_heads_fp8_cpu(int num_threads, int idx_dtype, int val_dtype,
                                          int b_format, int64_t m, int64_t k, int64_t heads,
                                          int64_t d, int64_t nnz, const void* row_ptr,
                                          const void* col_idx, const void* values, const void* b_q,
                                          int64_t ldb, const void* b_scale, void* c, int64_t ldc,
                                          int64_t row_begin, int64_t row_end,
                                          const ofx_spmm_options* opts) {
  return ::ofx::guarded(__func__, [&]() -> int {
    OFX_READ_OPTIONS(opts, "spmm_csr_heads_fp8_cpu");
    bool nothing = false;
    if (const int rc = check_heads_spmm("spmm_csr_heads_fp8_cpu", false, &b_format, idx_dtype,
                                        val_dtype, m, k, heads, d, nnz, row_ptr, col_idx, values,
                                        b_q, ldb, c, ldc, row_begin, row_end, opts, &nothing))
      return rc;
    if (nothing) return OFX_OK;
    const Schedule s = resolve_schedule(d, opts);  // of ONE head's width: the numeric contract
    return fp8::by_types(idx_dtype, val_dtype, [&](auto* tp, auto* ip) -> int {
      using T = std::remove_pointer_t<decltype(tp)>;
      using I = std::remove_pointer_t<decltype(ip)>;
      return cpu_spmm_rows<T, I, Fp8Rows<T>>(
          "spmm_csr_heads_fp8_cpu", threads_of(num_threads), b_q ? k : 0, heads, d,
          (const I*)row_ptr, (const I*)col_idx, (const T*)values, (const uint8_t*)b_q, ldb, (T*)c,
          ldc, row_begin, row_end, s, nullptr, OFX_ACT_NONE,
          Fp8Rows<T>(b_format, (const float*)b_scale));
    });
  });
}
