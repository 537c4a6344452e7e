// gatv2_sanitize.cpp — the kCPU kernels of the GATv2 attention scores
// (csrc/gatv2_scores_cpu.cpp with csrc/errors.cpp) compiled from source with
// -fsanitize=address,undefined and driven over the boundary row lengths of the HIP kernels, (H, D)
// of both of their paths, a hub schedule, row ranges, every value type and both index types,
// columns outside [0, K), and exactly sized buffers (a read or write past x_row's, x_col's, att's
// or a row's last record is a heap overflow here).  The results are also checked against a naive
// double-precision loop (the add, LeakyReLU, the rounding to T, the dot product and the two row
// sums of the gradient), so a sanitizer-clean run is a correctness run.
// Built and run by tests/test_gatv2_cpu.py::test_cpu_kernels_under_sanitizers.
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
void run_case(const std::vector<int64_t>& lens, int64_t heads, int64_t d, int64_t k,
              int64_t row_begin, int64_t row_end, bool with_p, const ofx_spmm_options* opts) {
  using N = ofx::Num<T>;
  using A = typename N::acc;
  const int64_t m = (int64_t)lens.size(), nrows = row_end - row_begin, n = heads * d;
  std::vector<I> rp(m + 1, 0);
  for (int64_t r = 0; r < m; ++r) rp[r + 1] = (I)(rp[r] + lens[r]);
  const int64_t nnz = (int64_t)rp[m];
  // exactly sized heap buffers: ASan flags the first byte outside.  x_row, d_x and p hold the rows
  // from row_begin on; one column in eight lies outside [0, k).
  std::vector<I> ci(nnz);
  for (int64_t j = 0; j < nnz; ++j) {
    const int64_t c = (int64_t)(uniform() * (double)(k + 2)) - 1;
    ci[j] = (I)(j % 8 == 5 ? (c < 0 ? -1 : k + c) : (c < 0 ? 0 : (c >= k ? k - 1 : c)));
  }
  std::vector<T> x_row(nrows * n), x_col(k * n), att(n), de(nnz * heads), e(nnz * heads),
      d_x(nrows * n), p(with_p ? nrows * n : 0);
  for (auto& x : x_row) x = N::store((A)(4.0 * uniform() - 2.0));
  for (auto& x : x_col) x = N::store((A)(4.0 * uniform() - 2.0));
  for (auto& x : att) x = N::store((A)(2.0 * uniform() - 1.0));
  for (auto& x : de) x = N::store((A)(2.0 * uniform() - 1.0));
  for (auto& x : e) x = N::store((A)(-5));
  for (auto& x : d_x) x = N::store((A)(-5));
  for (auto& x : p) x = N::store((A)(-5));
  int rc = ofx_gatv2_scores_csr_heads_cpu(3, idx_code<I>(), Code<T>::dt, m, k, heads, d, nnz,
                                          rp.data(), ci.data(), x_row.data(), n, x_col.data(), n,
                                          att.data(), kSlope, e.data(), row_begin, row_end);
  EXPECT(rc == OFX_OK, "forward rc=%d: %s", rc, ofx_last_error());
  rc = ofx_gatv2_scores_csr_heads_grad_cpu(3, idx_code<I>(), Code<T>::dt, m, k, heads, d, nnz,
                                           rp.data(), ci.data(), x_row.data(), n, x_col.data(), n,
                                           att.data(), kSlope, de.data(), d_x.data(), n,
                                           with_p ? p.data() : nullptr, n, row_begin, row_end, opts);
  EXPECT(rc == OFX_OK, "backward rc=%d: %s", rc, ofx_last_error());
  const bool no_scores = nrows == 0 || nnz == 0 || heads == 0;
  const bool no_grad = nrows == 0 || n == 0;
  for (int64_t r = 0; r < m; ++r) {
    const bool in = r >= row_begin && r < row_end;
    const int64_t j0 = (int64_t)rp[r], j1 = (int64_t)rp[r + 1];
    if (!in || no_scores) {
      for (int64_t j = j0 * heads; j < j1 * heads; ++j)
        EXPECT((double)N::load(e[j]) == -5, "row %lld outside the range was written", (long long)r);
    }
    if (!in) continue;
    for (int64_t c = 0; c < n; ++c) {
      const int64_t h = c / d;
      const double xr = (double)N::load(x_row[(r - row_begin) * n + c]);
      const double w = (double)N::load(att[c]);
      double s1 = 0, s2 = 0, mag = 0;
      bool near_kink = false;
      for (int64_t j = j0; j < j1; ++j) {
        const int64_t cj = (int64_t)ci[j];
        const double z = xr + (cj >= 0 && cj < k ? (double)N::load(x_col[cj * n + c]) : 0.0);
        // |z| below the rounding of the add may fall on either side of the kink
        near_kink = near_kink || std::fabs(z) <= 8 * Code<T>::tol;
        const double u = (double)N::load(N::store((A)(z > 0 ? z : z * kSlope)));
        const double g = (double)N::load(de[j * heads + h]);
        s1 += g * (z > 0 ? w : w * kSlope);
        s2 += g * u;
        mag += std::fabs(g) * (std::fabs(w) + std::fabs(u));
      }
      const double bound = (4 + (double)(j1 - j0)) * Code<T>::tol * (1 + mag);
      const double got1 = (double)N::load(d_x[(r - row_begin) * n + c]);
      if (!near_kink)
        EXPECT(std::fabs(got1 - s1) <= bound, "row %lld col %lld d_x = %g, want %g", (long long)r,
               (long long)c, got1, s1);
      EXPECT(j1 > j0 || (got1 == 0 && !std::signbit(got1)), "an empty row's d_x is %g", got1);
      if (with_p) {
        const double got2 = (double)N::load(p[(r - row_begin) * n + c]);
        EXPECT(std::fabs(got2 - s2) <= bound, "row %lld col %lld p = %g, want %g", (long long)r,
               (long long)c, got2, s2);
      }
    }
    if (no_scores) continue;
    for (int64_t j = j0; j < j1; ++j) {
      const int64_t cj = (int64_t)ci[j];
      for (int64_t h = 0; h < heads; ++h) {
        double want = 0, mag = 0;
        for (int64_t c = h * d; c < (h + 1) * d; ++c) {
          const double z = (double)N::load(x_row[(r - row_begin) * n + c]) +
                           (cj >= 0 && cj < k ? (double)N::load(x_col[cj * n + c]) : 0.0);
          const double u = (double)N::load(N::store((A)(z > 0 ? z : z * kSlope)));
          want += (double)N::load(att[c]) * u;
          mag += std::fabs((double)N::load(att[c]) * u);
        }
        const double got = (double)N::load(e[j * heads + h]);
        EXPECT(std::fabs(got - want) <= (4 + (double)d) * Code<T>::tol * (1 + mag),
               "row %lld head %lld e[%lld] = %g, want %g", (long long)r, (long long)h, (long long)j,
               got, want);
      }
    }
  }
  if (no_grad)
    for (auto& x : d_x) EXPECT((double)N::load(x) == -5, "d_x was written with nothing to do");
}

template <typename T, typename I>
void run_type() {
  const std::vector<int64_t> lens = {0, 1, 2, 7, 8, 9, 63, 64, 65, 130, 255, 256, 257, 513, 1030, 0};
  const int64_t m = (int64_t)lens.size();
  ofx_spmm_options split = OFX_SPMM_OPTIONS_INIT;
  split.split_threshold = 8;
  split.chunk = 4;
  const int64_t hd[][2] = {{1, 8}, {3, 5}, {5, 1}, {4, 16}, {2, 24}};
  for (const auto& x : hd) {
    run_case<T, I>(lens, x[0], x[1], 37, 0, m, true, nullptr);
    run_case<T, I>(lens, x[0], x[1], 37, 0, m, false, &split);
    run_case<T, I>(lens, x[0], x[1], 37, 0, 0, true, nullptr);
    run_case<T, I>(lens, x[0], x[1], 37, 3, 15, true, &split);
    run_case<T, I>(lens, x[0], x[1], 1, m - 2, m, false, nullptr);
  }
  run_case<T, I>(lens, 0, 0, 37, 0, m, true, nullptr);  // no heads: nothing is read or written
  run_case<T, I>({}, 4, 8, 37, 0, 0, true, nullptr);
  run_case<T, I>({0, 0, 0}, 4, 8, 37, 0, 3, true, nullptr);
}

void error_paths() {
  const int32_t rp[] = {0, 1}, ci[] = {0};
  float x_row[2] = {0, 1}, x_col[2] = {1, -1}, att[2] = {1, 1}, e[1] = {-5}, de[1] = {1}, d_x[2], p[2];
  auto fwd = [&](int vdt, int64_t heads, int64_t d, const void* xc, double slope, void* out,
                 int64_t re) {
    return ofx_gatv2_scores_csr_heads_cpu(1, OFX_DT_INT32, vdt, 1, 1, heads, d, 1, rp, ci, x_row, 2,
                                          xc, 2, att, slope, out, 0, re);
  };
  EXPECT(fwd(OFX_DT_FLOAT, -1, 2, x_col, 0.2, e, 1) == OFX_EINVAL, "negative heads");
  EXPECT(fwd(OFX_DT_FLOAT, 1, 2, x_col, 0.2, e, 2) == OFX_EINVAL, "row range past m");
  EXPECT(fwd(OFX_DT_INT32, 1, 2, x_col, 0.2, e, 1) == OFX_EUNSUPPORTED, "value dtype");
  EXPECT(fwd(OFX_DT_FLOAT, 1, 2, nullptr, 0.2, e, 1) == OFX_EINVAL, "NULL x_col");
  EXPECT(fwd(OFX_DT_FLOAT, 1, 2, x_col, 0.0, e, 1) == OFX_EINVAL, "slope 0");
  EXPECT(fwd(OFX_DT_FLOAT, 1, 2, x_col, -1.0, e, 1) == OFX_EINVAL, "negative slope");
  EXPECT(fwd(OFX_DT_FLOAT, 1, 2, x_col, NAN, e, 1) == OFX_EINVAL, "NaN slope");
  EXPECT(fwd(OFX_DT_FLOAT, 1, 2, x_col, INFINITY, e, 1) == OFX_EINVAL, "infinite slope");
  EXPECT(fwd(OFX_DT_FLOAT, 1, 2, x_col, 0.2, x_col, 1) == OFX_EINVAL, "e on x_col");
  EXPECT(fwd(OFX_DT_FLOAT, 1, 3, x_col, 0.2, e, 1) == OFX_EINVAL, "ld < n");
  EXPECT(e[0] == -5, "an error wrote e");
  EXPECT(fwd(OFX_DT_FLOAT, 1, 2, x_col, 0.5, e, 1) == OFX_OK && e[0] == 1.0f, "e = 1 + 0, got %g",
         (double)e[0]);
  auto bwd = [&](const void* g, void* dx, void* pp, const ofx_spmm_options* o) {
    return ofx_gatv2_scores_csr_heads_grad_cpu(1, OFX_DT_INT32, OFX_DT_FLOAT, 1, 1, 1, 2, 1, rp, ci,
                                               x_row, 2, x_col, 2, att, 0.5, g, dx, 2, pp, 2, 0, 1, o);
  };
  ofx_spmm_options o = OFX_SPMM_OPTIONS_INIT;
  o.planned = 1;
  EXPECT(bwd(nullptr, d_x, p, nullptr) == OFX_EINVAL, "NULL de");
  EXPECT(bwd(de, d_x, d_x, nullptr) == OFX_EINVAL, "p on d_x");
  EXPECT(bwd(de, x_row, p, nullptr) == OFX_EINVAL, "d_x on x_row");
  EXPECT(bwd(de, d_x, p, &o) == OFX_EINVAL, "planned");
  // z = (1, 0): d_x = (att_0, att_1 * slope), p = (U_0, U_1) = (1, 0)
  EXPECT(bwd(de, d_x, p, nullptr) == OFX_OK && d_x[0] == 1.0f && d_x[1] == 0.5f && p[0] == 1.0f &&
             p[1] == 0.0f, "d_x = (%g, %g), p = (%g, %g)", (double)d_x[0], (double)d_x[1],
         (double)p[0], (double)p[1]);
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
