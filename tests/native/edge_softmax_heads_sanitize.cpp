// edge_softmax_heads_sanitize.cpp — the kCPU kernels of the multi-head edge softmax
// (csrc/edge_softmax_cpu.cpp with csrc/errors.cpp) compiled from source with
// -fsanitize=address,undefined and driven over the boundary row lengths of the HIP kernel, head
// counts of both of its paths, row ranges, every value type and both index types, special values
// confined to one head, and exactly sized [nnz, H] buffers (a read or write past a row's last
// record is a heap overflow here).  The results are also checked against a naive double-precision
// softmax per column, and against the single-head entries bit for bit, so a sanitizer-clean run is
// a correctness run.
// Built and run by tests/test_edge_softmax_heads_cpu.py::test_cpu_kernels_under_sanitizers.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sanitize_common.h"

namespace {

template <typename T, typename I>
void run_case(const std::vector<int64_t>& lens, int64_t heads, int64_t row_begin, int64_t row_end) {
  using N = ofx::Num<T>;
  using A = typename N::acc;
  const int64_t m = (int64_t)lens.size();
  std::vector<I> rp(m + 1, 0);
  for (int64_t r = 0; r < m; ++r) rp[r + 1] = (I)(rp[r] + lens[r]);
  const int64_t nnz = (int64_t)rp[m], n = nnz * heads;
  // exactly sized heap buffers: ASan flags the first byte outside
  std::vector<T> e(n), g(n), y(n), de(n);
  for (int64_t j = 0; j < n; ++j) {
    e[j] = N::store((A)(8.0 * uniform() - 4.0));
    g[j] = N::store((A)(2.0 * uniform() - 1.0));
    y[j] = N::store((A)(-5));
    de[j] = N::store((A)(-5));
  }
  int rc = ofx_edge_softmax_csr_heads_cpu(3, idx_code<I>(), Code<T>::dt, m, heads, nnz, rp.data(),
                                          e.data(), y.data(), row_begin, row_end, nullptr);
  EXPECT(rc == OFX_OK, "forward rc=%d: %s", rc, ofx_last_error());
  rc = ofx_edge_softmax_csr_heads_grad_cpu(3, idx_code<I>(), Code<T>::dt, m, heads, nnz, rp.data(),
                                           y.data(), g.data(), de.data(), row_begin, row_end,
                                           nullptr);
  EXPECT(rc == OFX_OK, "backward rc=%d: %s", rc, ofx_last_error());
  for (int64_t r = 0; r < m; ++r) {
    const bool in = r >= row_begin && r < row_end;
    const int64_t j0 = (int64_t)rp[r], j1 = (int64_t)rp[r + 1];
    for (int64_t h = 0; h < heads; ++h) {
      auto at = [&](const std::vector<T>& v, int64_t j) { return (double)N::load(v[j * heads + h]); };
      if (!in) {
        for (int64_t j = j0; j < j1; ++j)
          EXPECT(at(y, j) == -5 && at(de, j) == -5, "row %lld head %lld outside the range was written",
                 (long long)r, (long long)h);
        continue;
      }
      double mx = -INFINITY, s = 0, d = 0;
      for (int64_t j = j0; j < j1; ++j) mx = std::fmax(mx, at(e, j));
      for (int64_t j = j0; j < j1; ++j) s += std::exp(at(e, j) - mx);
      for (int64_t j = j0; j < j1; ++j) {
        const double want = std::exp(at(e, j) - mx) / s;
        EXPECT(std::fabs(at(y, j) - want) <= Code<T>::tol, "row %lld head %lld y[%lld] = %g, want %g",
               (long long)r, (long long)h, (long long)j, at(y, j), want);
        d += at(y, j) * at(g, j);
      }
      for (int64_t j = j0; j < j1; ++j) {
        const double want = at(y, j) * (at(g, j) - d);
        EXPECT(std::fabs(at(de, j) - want) <= 4 * Code<T>::tol,
               "row %lld head %lld de[%lld] = %g, want %g", (long long)r, (long long)h,
               (long long)j, at(de, j), want);
      }
    }
  }
  // every head against the single-head entries on its contiguous column, bit for bit
  if (row_begin == 0 && row_end == m && nnz > 0) {
    std::vector<T> e1(nnz), g1(nnz), y1(nnz), de1(nnz);
    for (int64_t h = 0; h < heads; ++h) {
      for (int64_t j = 0; j < nnz; ++j) {
        e1[j] = e[j * heads + h];
        g1[j] = g[j * heads + h];
      }
      rc = ofx_edge_softmax_csr_cpu(2, idx_code<I>(), Code<T>::dt, m, nnz, rp.data(), e1.data(),
                                    y1.data(), 0, m, nullptr);
      EXPECT(rc == OFX_OK, "single-head forward rc=%d", rc);
      rc = ofx_edge_softmax_csr_grad_cpu(2, idx_code<I>(), Code<T>::dt, m, nnz, rp.data(),
                                         y1.data(), g1.data(), de1.data(), 0, m, nullptr);
      EXPECT(rc == OFX_OK, "single-head backward rc=%d", rc);
      for (int64_t j = 0; j < nnz; ++j) {
        EXPECT(memcmp(&y1[j], &y[j * heads + h], sizeof(T)) == 0, "head %lld y[%lld] bits",
               (long long)h, (long long)j);
        EXPECT(memcmp(&de1[j], &de[j * heads + h], sizeof(T)) == 0, "head %lld de[%lld] bits",
               (long long)h, (long long)j);
      }
    }
  }
}

template <typename T, typename I>
void run_type() {
  const std::vector<int64_t> lens = {0,   1,   7,   8,   9,    31,   32,  33, 127,
                                     128, 129, 511, 512, 513,  2048, 2049, 2563, 0};
  const int64_t m = (int64_t)lens.size();
  for (int64_t heads : {1, 3, 4, 8}) {
    run_case<T, I>(lens, heads, 0, m);
    run_case<T, I>(lens, heads, 0, 0);
    run_case<T, I>(lens, heads, 3, 15);
    run_case<T, I>(lens, heads, m - 2, m);
  }
  run_case<T, I>(lens, 0, 0, m);  // no heads: nothing is read or written
  run_case<T, I>({}, 4, 0, 0);
  run_case<T, I>({0, 0, 0}, 4, 0, 3);
}

// One row of three positions and five heads: a NaN, +inf, only -inf, one -inf, ordinary.
void special_values() {
  const int32_t rp[] = {0, 3};
  const float inf = INFINITY, nan = NAN;
  const float e[15] = {1, 0.5f, -inf, 1, 1,    nan, inf, -inf, -inf, 2,    2, 1, -inf, 2, 3};
  float y[15];
  int rc = ofx_edge_softmax_csr_heads_cpu(1, OFX_DT_INT32, OFX_DT_FLOAT, 1, 5, 3, rp, e, y, 0, 1,
                                          nullptr);
  EXPECT(rc == OFX_OK, "special rc=%d", rc);
  for (int j = 0; j < 3; ++j) {
    for (int h = 0; h < 3; ++h) {
      uint32_t bits;
      memcpy(&bits, &y[j * 5 + h], 4);
      EXPECT(bits == 0x7fc00000u, "y[%d, %d] = %08x, want the canonical NaN", j, h, bits);
    }
    EXPECT(std::isfinite(y[j * 5 + 3]) && std::isfinite(y[j * 5 + 4]), "a NaN leaked into row %d", j);
  }
  EXPECT(y[1 * 5 + 3] == 0.0f && !std::signbit(y[1 * 5 + 3]), "-inf in a finite column gives %g",
         y[1 * 5 + 3]);
  EXPECT(std::fabs(y[4] + y[9] + y[14] - 1.0f) < 1e-6, "the ordinary head sums to %g",
         y[4] + y[9] + y[14]);
}

void error_paths() {
  const int32_t rp[] = {0, 1};
  float e[2] = {0, 1}, y[2];
  auto fwd = [&](int vdt, int64_t heads, const void* pe, int64_t rb, int64_t re) {
    return ofx_edge_softmax_csr_heads_cpu(1, OFX_DT_INT32, vdt, 1, heads, 1, rp, pe, y, rb, re,
                                          nullptr);
  };
  EXPECT(fwd(OFX_DT_FLOAT, -1, e, 0, 1) == OFX_EINVAL, "negative heads");
  EXPECT(fwd(OFX_DT_FLOAT, 2, e, 0, 2) == OFX_EINVAL, "row range past m");
  EXPECT(fwd(OFX_DT_INT32, 2, e, 0, 1) == OFX_EUNSUPPORTED, "value dtype");
  EXPECT(fwd(OFX_DT_FLOAT, 2, nullptr, 0, 1) == OFX_EINVAL, "NULL e");
  EXPECT(ofx_edge_softmax_csr_heads_grad_cpu(1, OFX_DT_INT32, OFX_DT_FLOAT, 1, 2, 1, rp, y, nullptr,
                                             e, 0, 1, nullptr) == OFX_EINVAL, "NULL g");
  ofx_spmm_options o = OFX_SPMM_OPTIONS_INIT;
  o.ordered = 1;
  o.planned = 1;
  EXPECT(ofx_edge_softmax_csr_heads_cpu(1, OFX_DT_INT32, OFX_DT_FLOAT, 1, 2, 1, rp, e, y, 0, 1,
                                        &o) == OFX_OK && y[0] == 1.0f && y[1] == 1.0f,
         "options are accepted");
}

}  // namespace

int main() {
  g_rng = 777;
  run_type<float, int32_t>();
  run_type<float, int64_t>();
  run_type<double, int32_t>();
  run_type<double, int64_t>();
  run_type<ofx::bf16, int32_t>();
  run_type<ofx::bf16, int64_t>();
  run_type<ofx::f16, int32_t>();
  run_type<ofx::f16, int64_t>();
  special_values();
  error_paths();
  if (g_failures) {
    printf("%d failures\n", g_failures);
    return 1;
  }
  printf("OK\n");
  return 0;
}
