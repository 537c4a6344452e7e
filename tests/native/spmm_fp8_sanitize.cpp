// spmm_fp8_sanitize.cpp — the kCPU kernel of the multi-head SpMM over an FP8 feature table
// (csrc/spmm_heads_fp8_cpu.cpp with csrc/errors.cpp) compiled from source with
// -fsanitize=address,undefined and driven over the boundary row lengths of the HIP kernel, (H, D)
// of both of its paths, a hub schedule, row ranges, both formats, every value type and both index
// types, with and without the scale, columns at and beyond K, and exactly sized buffers (a read
// past b_q's, b_scale's or values' last element or a write past out's is a heap overflow here).
// The results are also checked against a naive double-precision loop over a table decoded here
// from the formats' definitions, so a sanitizer-clean run is a correctness run.
// Built and run by tests/test_spmm_fp8_cpu.py::test_cpu_kernel_under_sanitizers.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "sanitize_common.h"

namespace {

// The value of a finite code, from the format's definition (ldexp, not the kernel's bit assembly).
double decode(int fmt, unsigned c) {
  const int mbits = fmt == OFX_FP8_E4M3 ? 3 : 2, bias = fmt == OFX_FP8_E4M3 ? 7 : 15;
  const int e = (int)((c & 0x7f) >> mbits), m = (int)(c & ((1u << mbits) - 1));
  const double mag = e == 0 ? std::ldexp((double)m, 1 - bias - mbits)
                            : std::ldexp(1.0 + (double)m / (1 << mbits), e - bias);
  return (c & 0x80) ? -mag : mag;
}

bool finite_code(int fmt, unsigned c) {
  return fmt == OFX_FP8_E4M3 ? (c & 0x7f) != 0x7f : (c & 0x7f) < 0x7c;
}

template <typename T, typename I>
void run_case(int fmt, const std::vector<int64_t>& lens, int64_t heads, int64_t d, int64_t k,
              int64_t row_begin, int64_t row_end, bool scaled, int64_t pad,
              const ofx_spmm_options* opts) {
  using N = ofx::Num<T>;
  const int64_t m = (int64_t)lens.size(), nrows = row_end - row_begin, n = heads * d;
  const int64_t ldb = n + pad, ldc = n + pad;
  std::vector<I> rp(m + 1, 0);
  for (int64_t r = 0; r < m; ++r) rp[r + 1] = (I)(rp[r] + lens[r]);
  const int64_t nnz = (int64_t)rp[m];
  // exactly sized heap buffers (the last row of b_q and out without its padding): ASan flags the
  // first byte outside.  One column in eight lies in [k, k + 3).
  std::vector<I> ci(nnz);
  for (int64_t j = 0; j < nnz; ++j) {
    const int64_t c = (int64_t)(uniform() * (double)k);
    ci[j] = (I)(j % 8 == 5 ? k + (c % 3) : (c >= k ? k - 1 : c));
  }
  std::vector<uint8_t> bq(k > 0 ? (k - 1) * ldb + n : 0);
  for (auto& x : bq) {
    unsigned c = (unsigned)(next() >> 56);
    x = (uint8_t)(finite_code(fmt, c) ? c : 0x80);
  }
  std::vector<float> scale(scaled ? k : 0);
  for (auto& x : scale) x = (float)std::exp2(-8.0 + 4.0 * uniform());
  std::vector<T> vals(nnz * heads), out(nrows > 0 ? (nrows - 1) * ldc + n : 0);
  // small unscaled values: an f16 sum over e5m2's largest codes stays finite
  for (auto& x : vals) x = N::store((float)((2.0 * uniform() - 1.0) * (scaled ? 1.0 : 1.0 / 64)));
  for (auto& x : out) x = N::store(-5.0f);
  const int rc = ofx_spmm_csr_heads_fp8_cpu(
      3, idx_code<I>(), Code<T>::dt, fmt, m, k, heads, d, nnz, rp.data(), ci.data(), vals.data(),
      bq.data(), ldb, scaled ? scale.data() : nullptr, out.data(), ldc, row_begin, row_end, opts);
  EXPECT(rc == OFX_OK, "rc=%d: %s", rc, ofx_last_error());
  for (int64_t g = 0; g < nrows; ++g) {
    const int64_t r = row_begin + g, j0 = (int64_t)rp[r], j1 = (int64_t)rp[r + 1];
    for (int64_t c = 0; c < n; ++c) {
      double want = 0, mag = 0;
      for (int64_t j = j0; j < j1; ++j) {
        const int64_t cj = (int64_t)ci[j];
        if (cj >= k) continue;
        const double v = (double)N::load(vals[j * heads + c / d]) * (scaled ? scale[cj] : 1.0);
        const double b = decode(fmt, bq[cj * ldb + c]);
        want += v * b;
        mag += std::fabs(v * b);
      }
      const double got = (double)N::load(out[g * ldc + c]);
      // V', each product and the result are rounded to T; the sum is f32
      const double bound = (3 * Code<T>::tol + (double)(j1 - j0) * 1e-6) * (1 + mag);
      EXPECT(std::fabs(got - want) <= bound, "fmt %d row %lld col %lld = %g, want %g", fmt,
             (long long)r, (long long)c, got, want);
      EXPECT(j1 > j0 || (got == 0 && !std::signbit(got)), "an empty row's sum is %g", got);
    }
    for (int64_t c = n; c < ldc && g + 1 < nrows; ++c)
      EXPECT((double)N::load(out[g * ldc + c]) == -5, "row %lld: wrote into the padding",
             (long long)r);
  }
}

template <typename T, typename I>
void run_type() {
  const std::vector<int64_t> lens = {0, 1, 2, 7, 8, 9, 63, 64, 65, 130, 513, 1030, 3, 0};
  const int64_t m = (int64_t)lens.size();
  ofx_spmm_options split8 = OFX_SPMM_OPTIONS_INIT;
  split8.split_threshold = 8;
  split8.chunk = 4;
  ofx_spmm_options ordered = OFX_SPMM_OPTIONS_INIT;
  ordered.ordered = 1;
  const int64_t hd[][2] = {{1, 16}, {4, 16}, {3, 5}, {5, 1}, {1, 24}};
  for (int fmt : {OFX_FP8_E4M3, OFX_FP8_E5M2})
    for (const auto& s : hd)
      for (bool scaled : {true, false}) {
        run_case<T, I>(fmt, lens, s[0], s[1], 37, 0, m, scaled, 0, nullptr);
        run_case<T, I>(fmt, lens, s[0], s[1], 37, 0, m, scaled, 5, &split8);
        run_case<T, I>(fmt, lens, s[0], s[1], 37, 3, 12, scaled, 3, &ordered);
        run_case<T, I>(fmt, lens, s[0], s[1], 37, 5, 5, scaled, 0, nullptr);
      }
  run_case<T, I>(OFX_FP8_E4M3, {}, 2, 16, 37, 0, 0, true, 0, nullptr);
  run_case<T, I>(OFX_FP8_E4M3, {0, 0, 0}, 2, 16, 37, 0, 3, true, 0, nullptr);
  run_case<T, I>(OFX_FP8_E5M2, lens, 0, 0, 37, 0, m, false, 0, nullptr);
}

void argument_checks() {
  int32_t rp[3] = {0, 1, 2}, ci[2] = {0, -1};
  float vals[2] = {1, 1}, out[4] = {0, 0, 0, 0}, scale[2] = {1, 1};
  uint8_t bq[4] = {0x38, 0x38, 0x38, 0x38};
  auto call = [&](int vt, int fmt, const void* b, const ofx_spmm_options* o) {
    return ofx_spmm_csr_heads_fp8_cpu(1, OFX_DT_INT32, vt, fmt, 2, 2, 1, 2, 2, rp, ci, vals, b, 2,
                                      scale, out, 2, 0, 2, o);
  };
  EXPECT(call(OFX_DT_FLOAT, OFX_FP8_E4M3, bq, nullptr) == OFX_EINVAL, "a negative column");
  ci[1] = 1;
  EXPECT(call(OFX_DT_FLOAT, OFX_FP8_E4M3, bq, nullptr) == OFX_OK, "%s", ofx_last_error());
  EXPECT(out[0] == 1 && out[3] == 1, "1 * 1 * 1.0");
  EXPECT(call(OFX_DT_DOUBLE, OFX_FP8_E4M3, bq, nullptr) == OFX_EUNSUPPORTED, "f64");
  EXPECT(call(OFX_DT_FLOAT, 0, bq, nullptr) == OFX_EINVAL, "format 0");
  EXPECT(call(OFX_DT_FLOAT, OFX_FP8_E5M2, nullptr, nullptr) == OFX_EINVAL, "NULL b_q");
  ofx_spmm_options planned = OFX_SPMM_OPTIONS_INIT;
  planned.planned = 1;
  EXPECT(call(OFX_DT_FLOAT, OFX_FP8_E4M3, bq, &planned) == OFX_EINVAL, "planned");
}

}  // namespace

int main() {
  g_rng = 20260521;
  run_type<float, int32_t>();
  run_type<ofx::bf16, int64_t>();
  run_type<ofx::f16, int32_t>();
  argument_checks();
  if (g_failures) {
    fprintf(stderr, "%d failures\n", g_failures);
    return 1;
  }
  printf("spmm_fp8_sanitize OK\n");
  return 0;
}
