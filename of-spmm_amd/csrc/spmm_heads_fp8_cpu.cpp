// spmm_heads_fp8_cpu.cpp — the DeviceType::kCPU kernel of op "spmm_csr_heads_fp8" (multi-head
// SpMM over a CSR with an FP8 feature table and an optional f32 scale per row of it; contract in
// include/ofx_spmm.h).  A sibling of the sum's row template (spmm_rows_cpu.h, left
// as it is): the same loops per head, with the value scaled and rounded to T first (V') and the
// B element read through a 256-entry table of the format's values in T, so the bits are those of
// ofx_spmm_csr_heads_cpu on (V', Bd) and of the HIP kernel (spmm_heads_fp8.hip).
#pragma clang fp contract(off)

#include <omp.h>

#include <climits>
#include <vector>

#include "ofx_internal.h"
#include "spmm_common.h"
#include "spmm_heads_fp8.h"

namespace ofx {
namespace {

// Nonzeros [j0, j1) of one head: acc[c] = sum of mul(V'[j], lut[B[col[j], c]]) from +0, ascending
// (row_sum of spmm_rows_cpu.h).  A column outside [0, k) reads scale +0 and the zero-filled row;
// a negative one is reported through `neg`.
template <typename T, typename I>
void row_sum_fp8(const I* col, const T* val, int64_t vs, const float* scale, const uint8_t* B,
                 int64_t ldb, int64_t k, int64_t d, int64_t j0, int64_t j1, const float* lut,
                 float* acc, bool* neg) {
#pragma clang fp contract(off)
  for (int64_t c = 0; c < d; ++c) acc[c] = 0.0f;
  for (int64_t j = j0; j < j1; ++j) {
    const int64_t cj = (int64_t)col[j];
    const bool in = cj >= 0 && cj < k;
    float v = Num<T>::load(val[j * vs]);
    if (scale != nullptr) v = fp8::scaled_value<T>(v, in ? scale[cj] : 0.0f);
    if (in) {
      const uint8_t* brow = B + cj * ldb;
      for (int64_t c = 0; c < d; ++c) acc[c] = acc[c] + Num<T>::mul(v, lut[brow[c]]);
    } else {
      if (cj < 0) *neg = true;
      for (int64_t c = 0; c < d; ++c) acc[c] = acc[c] + Num<T>::mul(v, 0.0f);
    }
  }
}

// C[g, h*d + c] for rows [row_begin, row_end) and every head, in cpu_spmm_rows's order: a row of
// at most s.split nonzeros is one in-order sum, a longer one the in-order sum of its chunks' sums.
template <typename T, typename I>
int cpu_spmm_rows_fp8(int nthreads, int fmt, int64_t k, int64_t heads, int64_t d, const I* rp,
                      const I* col, const T* val, const float* scale, const uint8_t* B,
                      int64_t ldb, T* C, int64_t ldc, int64_t row_begin, int64_t row_end,
                      const Schedule& s) {
#pragma clang fp contract(off)
  float lut[256];  // Bd's values: the code's value stored in T (exact) and loaded again
  for (int c = 0; c < 256; ++c) lut[c] = Num<T>::load(Num<T>::store(fp8::decode(fmt, (uint32_t)c)));
  const int64_t rows = row_end - row_begin;
  bool any_neg = false;
#pragma omp parallel num_threads(nthreads) reduction(|| : any_neg)
  {
    std::vector<float> acc(d), part(d);
    bool neg = false;
#pragma omp for schedule(dynamic, 64)
    for (int64_t g = 0; g < rows; ++g) {
      const int64_t r = row_begin + g;
      const int64_t j0 = (int64_t)rp[r], j1 = (int64_t)rp[r + 1];
      const int64_t len = j1 - j0;
      for (int64_t h = 0; h < heads; ++h) {
        const T* vh = val != nullptr ? val + h : nullptr;  // NULL with nnz == 0: never read
        const uint8_t* bh = B != nullptr ? B + h * d : nullptr;
        if (len <= s.split) {
          row_sum_fp8<T, I>(col, vh, heads, scale, bh, ldb, k, d, j0, j1, lut, acc.data(), &neg);
        } else {
          const int64_t nc = num_chunks(len, s.chunk);
          for (int64_t c = 0; c < d; ++c) acc[c] = 0.0f;
          for (int64_t q = 0; q < nc; ++q) {
            const int64_t a = j0 + q * s.chunk;
            const int64_t e = (q == nc - 1) ? j1 : a + s.chunk;
            row_sum_fp8<T, I>(col, vh, heads, scale, bh, ldb, k, d, a, e, lut, part.data(), &neg);
            for (int64_t c = 0; c < d; ++c) acc[c] = acc[c] + part[c];
          }
        }
        T* out = C + g * ldc + h * d;
        for (int64_t c = 0; c < d; ++c) out[c] = Num<T>::store(acc[c]);
      }
    }
    any_neg = any_neg || neg;
  }
  OFX_REQUIRE(!any_neg, OFX_EINVAL,
              "spmm_csr_heads_fp8_cpu: negative column index (gather_kernel_util.cpp:80 "
              "CHECK_GE(idx, 0))");
  return OFX_OK;
}

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
    int rc = fp8::check_fp8_args("spmm_csr_heads_fp8_cpu", idx_dtype, val_dtype, b_format, m, k,
                                 heads, d, nnz, opts);
    if (rc) return rc;
    if ((rc = check_row_range("spmm_csr_heads_fp8_cpu", row_begin, row_end, m))) return rc;
    const int64_t n = heads * d;
    OFX_REQUIRE(ldb >= n && ldc >= n, OFX_EINVAL,
                "spmm_csr_heads_fp8_cpu: ldb=%lld / ldc=%lld < n=%lld", (long long)ldb,
                (long long)ldc, (long long)n);
    if (row_end == row_begin || n == 0) return OFX_OK;
    OFX_REQUIRE(row_ptr && c && (nnz == 0 || (col_idx && values && (b_q || k == 0))), OFX_EINVAL,
                "spmm_csr_heads_fp8_cpu: NULL pointer");
    const Schedule s = resolve_schedule(d, opts);  // of ONE head's width: the numeric contract
    return fp8::by_types(idx_dtype, val_dtype, [&](auto* tp, auto* ip) -> int {
      using T = std::remove_pointer_t<decltype(tp)>;
      using I = std::remove_pointer_t<decltype(ip)>;
      return cpu_spmm_rows_fp8<T, I>(threads_of(num_threads), b_format, b_q ? k : 0, heads, d,
                                     (const I*)row_ptr, (const I*)col_idx, (const T*)values,
                                     (const float*)b_scale, (const uint8_t*)b_q, ldb, (T*)c, ldc,
                                     row_begin, row_end, s);
    });
  });
}
