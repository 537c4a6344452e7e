// gat_softmax_sanitize.cpp — the kCPU kernels of the GAT attention weights
// (csrc/gat_softmax_cpu.cpp with csrc/errors.cpp) compiled from source with
// -fsanitize=address,undefined and driven over the boundary row lengths of the HIP kernel, head
// counts of both of its paths, row ranges, every value type and both index types, columns outside
// [0, K), and exactly sized buffers (a read or write past s_row's, s_col's or a row's last record
// is a heap overflow here).  The results are also checked against a naive double-precision loop
// (scores, LeakyReLU, softmax, its gradient, the mask multiply and the row sum), so a
// sanitizer-clean run is a correctness run.
// Built and run by tests/test_gat_softmax_cpu.py::test_cpu_kernels_under_sanitizers.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sanitize_common.h"

namespace {

constexpr double kSlope = 0.2;

template <typename T, typename I>
void run_case(const std::vector<int64_t>& lens, int64_t heads, int64_t k, int64_t row_begin,
              int64_t row_end) {
  using N = ofx::Num<T>;
  using A = typename N::acc;
  const int64_t m = (int64_t)lens.size(), nrows = row_end - row_begin;
  std::vector<I> rp(m + 1, 0);
  for (int64_t r = 0; r < m; ++r) rp[r + 1] = (I)(rp[r] + lens[r]);
  const int64_t nnz = (int64_t)rp[m], n = nnz * heads;
  // exactly sized heap buffers: ASan flags the first byte outside.  s_row and d_row hold the rows
  // from row_begin on; one column in eight lies outside [0, k).
  std::vector<I> ci(nnz);
  for (int64_t j = 0; j < nnz; ++j) {
    const int64_t c = (int64_t)(uniform() * (double)(k + 2)) - 1;
    ci[j] = (I)(j % 8 == 5 ? (c < 0 ? -1 : k + c) : (c < 0 ? 0 : (c >= k ? k - 1 : c)));
  }
  std::vector<T> s_row(nrows * heads), s_col(k * heads), g(n), attn(n), ds(n), d_row(nrows * heads);
  for (auto& x : s_row) x = N::store((A)(4.0 * uniform() - 2.0));
  for (auto& x : s_col) x = N::store((A)(4.0 * uniform() - 2.0));
  for (int64_t j = 0; j < n; ++j) {
    g[j] = N::store((A)(2.0 * uniform() - 1.0));
    attn[j] = N::store((A)(-5));
    ds[j] = N::store((A)(-5));
  }
  for (auto& x : d_row) x = N::store((A)(-5));
  int rc = ofx_gat_softmax_csr_heads_cpu(3, idx_code<I>(), Code<T>::dt, m, k, heads, nnz, rp.data(),
                                         ci.data(), s_row.data(), s_col.data(), kSlope, attn.data(),
                                         row_begin, row_end, nullptr);
  EXPECT(rc == OFX_OK, "forward rc=%d: %s", rc, ofx_last_error());
  rc = ofx_gat_softmax_csr_heads_grad_cpu(3, idx_code<I>(), Code<T>::dt, m, k, heads, nnz,
                                          rp.data(), ci.data(), s_row.data(), s_col.data(), kSlope,
                                          attn.data(), g.data(), ds.data(), d_row.data(), row_begin,
                                          row_end, nullptr);
  EXPECT(rc == OFX_OK, "backward rc=%d: %s", rc, ofx_last_error());
  const bool nothing = nrows == 0 || nnz == 0 || heads == 0;
  for (int64_t r = 0; r < m; ++r) {
    const bool in = r >= row_begin && r < row_end && !nothing;
    const int64_t j0 = (int64_t)rp[r], j1 = (int64_t)rp[r + 1];
    for (int64_t h = 0; h < heads; ++h) {
      auto at = [&](const std::vector<T>& v, int64_t j) { return (double)N::load(v[j * heads + h]); };
      if (!in) {
        for (int64_t j = j0; j < j1; ++j)
          EXPECT(at(attn, j) == -5 && at(ds, j) == -5,
                 "row %lld head %lld outside the range was written", (long long)r, (long long)h);
        continue;
      }
      const double sr = (double)N::load(s_row[(r - row_begin) * heads + h]);
      std::vector<double> z(j1 - j0), e(j1 - j0);
      double mx = -INFINITY, s = 0, d = 0, sum = 0;
      for (int64_t j = j0; j < j1; ++j) {
        const int64_t c = (int64_t)ci[j];
        z[j - j0] = sr + (c >= 0 && c < k ? (double)N::load(s_col[c * heads + h]) : 0.0);
        // the kernel rounds the score to T before the softmax
        e[j - j0] = (double)N::load(N::store((A)(z[j - j0] > 0 ? z[j - j0] : z[j - j0] * kSlope)));
        mx = std::fmax(mx, e[j - j0]);
      }
      for (int64_t j = j0; j < j1; ++j) s += std::exp(e[j - j0] - mx);
      for (int64_t j = j0; j < j1; ++j) {
        const double want = std::exp(e[j - j0] - mx) / s;
        EXPECT(std::fabs(at(attn, j) - want) <= 4 * Code<T>::tol,
               "row %lld head %lld attn[%lld] = %g, want %g", (long long)r, (long long)h,
               (long long)j, at(attn, j), want);
        d += at(attn, j) * at(g, j);
      }
      for (int64_t j = j0; j < j1; ++j) {
        // |z| below the rounding of the add may fall on either side of the kink: skip those
        const double want = at(attn, j) * (at(g, j) - d) * (z[j - j0] > 0 ? 1.0 : kSlope);
        if (std::fabs(z[j - j0]) > 8 * Code<T>::tol)
          EXPECT(std::fabs(at(ds, j) - want) <= 4 * Code<T>::tol,
                 "row %lld head %lld ds[%lld] = %g, want %g", (long long)r, (long long)h,
                 (long long)j, at(ds, j), want);
        sum += at(ds, j);
      }
      const double got = (double)N::load(d_row[(r - row_begin) * heads + h]);
      EXPECT(std::fabs(got - sum) <= (double)(8 + (j1 - j0)) * Code<T>::tol,
             "row %lld head %lld d_row = %g, want %g", (long long)r, (long long)h, got, sum);
      EXPECT(j1 > j0 || (got == 0 && !std::signbit(got)), "an empty row's d_row is %g", got);
    }
  }
  if (nothing)
    for (auto& x : d_row) EXPECT((double)N::load(x) == -5, "d_row was written with nothing to do");
}

template <typename T, typename I>
void run_type() {
  const std::vector<int64_t> lens = {0,   1,   7,   8,   9,    31,   32,  33, 127,
                                     128, 129, 511, 512, 513,  2048, 2049, 2563, 0};
  const int64_t m = (int64_t)lens.size();
  for (int64_t heads : {1, 3, 4, 8}) {
    run_case<T, I>(lens, heads, 37, 0, m);
    run_case<T, I>(lens, heads, 37, 0, 0);
    run_case<T, I>(lens, heads, 37, 3, 15);
    run_case<T, I>(lens, heads, 1, m - 2, m);
  }
  run_case<T, I>(lens, 0, 37, 0, m);  // no heads: nothing is read or written
  run_case<T, I>({}, 4, 37, 0, 0);
  run_case<T, I>({0, 0, 0}, 4, 37, 0, 3);
}

void error_paths() {
  const int32_t rp[] = {0, 1}, ci[] = {0};
  float s_row[2] = {0, 1}, s_col[2] = {1, -1}, attn[2] = {-5, -5}, ds[2], d_row[2];
  auto fwd = [&](int vdt, int64_t heads, const void* sc, double slope, void* out, int64_t re) {
    return ofx_gat_softmax_csr_heads_cpu(1, OFX_DT_INT32, vdt, 1, 1, heads, 1, rp, ci, s_row, sc,
                                         slope, out, 0, re, nullptr);
  };
  EXPECT(fwd(OFX_DT_FLOAT, -1, s_col, 0.2, attn, 1) == OFX_EINVAL, "negative heads");
  EXPECT(fwd(OFX_DT_FLOAT, 2, s_col, 0.2, attn, 2) == OFX_EINVAL, "row range past m");
  EXPECT(fwd(OFX_DT_INT32, 2, s_col, 0.2, attn, 1) == OFX_EUNSUPPORTED, "value dtype");
  EXPECT(fwd(OFX_DT_FLOAT, 2, nullptr, 0.2, attn, 1) == OFX_EINVAL, "NULL s_col");
  EXPECT(fwd(OFX_DT_FLOAT, 2, s_col, 0.0, attn, 1) == OFX_EINVAL, "slope 0");
  EXPECT(fwd(OFX_DT_FLOAT, 2, s_col, -1.0, attn, 1) == OFX_EINVAL, "negative slope");
  EXPECT(fwd(OFX_DT_FLOAT, 2, s_col, NAN, attn, 1) == OFX_EINVAL, "NaN slope");
  EXPECT(fwd(OFX_DT_FLOAT, 2, s_col, INFINITY, attn, 1) == OFX_EINVAL, "infinite slope");
  EXPECT(fwd(OFX_DT_FLOAT, 2, s_col, 0.2, s_col, 1) == OFX_EINVAL, "attn on s_col");
  EXPECT(attn[0] == -5 && attn[1] == -5, "an error wrote attn");
  ofx_spmm_options o = OFX_SPMM_OPTIONS_INIT;
  o.ordered = 1;
  o.planned = 1;
  EXPECT(ofx_gat_softmax_csr_heads_cpu(1, OFX_DT_INT32, OFX_DT_FLOAT, 1, 1, 2, 1, rp, ci, s_row,
                                       s_col, 0.2, attn, 0, 1, &o) == OFX_OK &&
             attn[0] == 1.0f && attn[1] == 1.0f,
         "options are accepted");
  EXPECT(ofx_gat_softmax_csr_heads_grad_cpu(1, OFX_DT_INT32, OFX_DT_FLOAT, 1, 1, 2, 1, rp, ci,
                                            s_row, s_col, 0.2, attn, nullptr, ds, d_row, 0, 1,
                                            nullptr) == OFX_EINVAL, "NULL g");
  EXPECT(ofx_gat_softmax_csr_heads_grad_cpu(1, OFX_DT_INT32, OFX_DT_FLOAT, 1, 1, 2, 1, rp, ci,
                                            s_row, s_col, 0.2, attn, s_row, ds, ds, 0, 1,
                                            nullptr) == OFX_EINVAL, "d_row on ds");
}

}  // namespace

int main() {
  g_rng = 4242;
  run_type<float, int32_t>();
  run_type<float, int64_t>();
  run_type<double, int32_t>();
  run_type<double, int64_t>();
  run_type<ofx::bf16, int32_t>();
  run_type<ofx::bf16, int64_t>();
  run_type<ofx::f16, int32_t>();
  run_type<ofx::f16, int64_t>();
  error_paths();
  if (g_failures) {
    printf("%d failures\n", g_failures);
    return 1;
  }
  printf("OK\n");
  return 0;
}
